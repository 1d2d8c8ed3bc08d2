"""What the scaling-count tests share - TEST INFRASTRUCTURE (test_scaler_counts_host.py on the CPU,
test_gpu_scaler_counts.py on the device).

Every log-likelihood of the library is log(sum) + count * log(2^-256), and the count comes from a scale buffer: per site,
per site and rate (PLL_ATTRIB_RATE_SCALERS) or per repeat class (PLL_ATTRIB_SITE_REPEATS). A tree only ever produces counts
that grow smoothly towards the root and are nearly equal across the rate categories of a site, and needs hundreds of taxa
to produce any. Here the counts are WRITTEN by the caller instead: partition->scale_buffer[i] is public, the reference
reads it as it stands, and libpll_amd.so is told with pll_gpu_invalidate(PLL_GPU_DIRTY_SCALER, i) that the host copy is the
newer one (driver.Session.write_scaler). The CLVs stay as the traversal computed them; the expected values come from the
reference running live on the same arrays, so an 8-taxon tree exercises every index computation on a scale buffer.

Count tables (deterministic, no tolerance anywhere). Per-site counts cycle through PER_SITE. Per-rate rows cycle, for four
rate categories, through the twelve rows of ROWS4, which together hold: all counts equal (zero and non-zero), the minimum at
every position, a tie for the minimum, one surviving category at each k (every other one at the cap or beyond: the last
four rows), an excess over the minimum of 1, 2, 3, exactly 4 (the cap, PLL_SCALE_RATE_MAXDIFF) and above 4. For another
number of categories entry n carries ROWS4[(i + k) % 12][k % 4] at rate k plus the per-site cycle's value as a base, i the
entry's place in the cycle.
The second end of an edge starts three places further on, so that taking one end's vector for the other's is visible.
The cycle runs separately over each group of entries a case names (invariant and variable sites, the ascertainment
entries), so every pattern occurs in every group large enough; `assert_covered` recomputes that from the written array.

Shapes: the smallest that still reach each kernel family (all balanced trees of W.make_case, 8 taxa; 16 under site
repeats). Which kernels a shape reaches follows from derive_geometry / launch_edge / the partials dispatcher of
csrc/hip/pllgpu.hip:

    id      states x rates  sites  edge log-likelihood                       partials
    dna     4 x 4           130    k_edge_dna (tail / chain / tree forms     k_partials_dna* (fused groups and chains; with
                                   when the traversal directly precedes)     PLL_AMD_NO_FUSE=1 one launch per level)
    dna-r8  4 x 8           70     k_edge_tiled<4> (dna_fast wants R == 4)   k_partials_tiled<4>; more rates than waves
    s5-r3   5 x 3           65     k_edge_tiled<8>                           k_partials_tiled<8>; R no power of two
    aa      20 x 4          65     k_edge_tiled<20>                          k_partials_mfma_cc groups over the tips and
                                                                             k_partials_lean above (matrix pipe), the
                                                                             scalers by k_mfma_scale_epilogue
    codon   61 x 4          33     k_edge_mfma (root: k_edge_tiled<32>)      k_partials_mfma / k_partials_mfma_wide +
                                                                             k_mfma_scale_epilogue; one 32-site item + 1

130 sites are two 64-site tiles and a ragged one, 65 and 33 one tile (item) and one site."""
import numpy as np

from pllamd import api, workload as W

PER_SITE = (0, 1, 3, 4, 5, 9)
ROWS4 = ((0, 0, 0, 0), (2, 2, 2, 2), (0, 1, 2, 3), (3, 2, 1, 0), (0, 4, 0, 4), (5, 0, 0, 9), (7, 7, 7, 8), (6, 2, 6, 6),
         (0, 4, 5, 9), (4, 0, 9, 5), (9, 5, 0, 4), (5, 9, 4, 0))
SECOND_END_SHIFT = 3
ASC_EXTRA = (0, 2, 5, 1)  # the counts of the four ascertainment entries behind the sites of a DNA partition

SHAPES = {"dna": (4, 4, 130), "dna-r8": (4, 8, 70), "s5-r3": (5, 3, 65), "aa": (20, 4, 65), "codon": (61, 4, 33)}
ATTRS = {"plain": 0, "tip": api.PATTERN_TIP, "rs": api.RATE_SCALERS, "rs-tip": api.RATE_SCALERS | api.PATTERN_TIP}
REPEATS = {"rep": api.SITE_REPEATS, "rep-rs": api.SITE_REPEATS | api.RATE_SCALERS}
REPEAT_SHAPES = ("dna", "aa")
REPEAT_SEEDS = {"dna": 900, "aa": 922}  # alignments whose two top nodes stay class-compressed (asserted where they are used)
PINV_SHAPES = ("dna", "dna-r8", "aa")
BRLENS = (0.002, 0.07, 0.4, 1.3)
LOG_THRESHOLD = -256.0 * np.log(2.0)  # log(PLL_SCALE_THRESHOLD)
RATE_MAXDIFF = 4  # PLL_SCALE_RATE_MAXDIFF


def make(shape, attrs, pinv=0.0, asc_type=None):
    """the Case of one shape x attribute word (+ invariant sites, + an ascertainment-bias type)"""
    states, rates, sites = SHAPES[shape]
    seed = 900 + 7 * list(SHAPES).index(shape)
    kw = dict(rate_cats=rates, attributes=attrs, seed=seed)
    if attrs & api.SITE_REPEATS:
        kw.update(seed=REPEAT_SEEDS[shape])
        return W.make_case(shape, states, 16, sites, mutate_pct=5, **kw)
    if pinv:
        kw.update(pinv=pinv, mutate_pct=4)
    if asc_type is not None:
        kw.update(asc_type=asc_type, asc_weights=[3, 1, 4, 1] if asc_type == 3 else None)
    return W.make_case(shape, states, 8, sites, **kw)


def per_rate(case):
    return bool(case.attributes & api.RATE_SCALERS)


def flip(edge):
    return (edge[2], edge[3], edge[0], edge[1], edge[4])


def root_edge(case):
    """the inner-inner edge the balanced traversal ends in"""
    return tuple(case.edges[0])


def tip_edge(case):
    """an inner node and one of its tip children (the tip carries no scaler), across the tip's matrix"""
    parent, pscaler, child, matrix = case.op_batches[0][0][:4]
    assert child < case.tips <= parent
    return (parent, pscaler, child, api.SCALE_BUFFER_NONE, matrix)


def top_ops(case):
    """(ops below the last two, the last two): the two ops whose parents are the ends of root_edge"""
    ops = case.op_batches[0]
    assert {ops[-2][0], ops[-1][0]} == {case.edges[0][0], case.edges[0][2]}
    return ops[:-2], ops[-2:]


def cherry_parents(case):
    """(clv, scaler) of every op over two tips"""
    return [(op[0], op[1]) for op in case.op_batches[0] if op[2] < case.tips and op[5] < case.tips]


# ---- the tables ----------------------------------------------------------------------------------------------------
def pattern(i, rates):
    """the per-rate row at place i of the cycle, without its base"""
    if rates == 4:
        return np.array(ROWS4[i % len(ROWS4)], dtype=np.int64)
    return np.array([ROWS4[(i + k) % len(ROWS4)][k % 4] for k in range(rates)], dtype=np.int64)


def n_classes(rates):
    return len(PER_SITE) if rates is None else len(ROWS4)


def table(entries, rates=None, shift=0, groups=None):
    """counts [entries] (rates None: per-site scalers) or [entries][rates]; groups: index arrays that partition (part of)
    the entries, the cycle starts anew - at place `shift` - in each; entries in no group carry zero"""
    if groups is None:
        groups = [np.arange(entries)]
    out = np.zeros((entries,) if rates is None else (entries, rates), dtype=np.uint32)
    for g in groups:
        for j, n in enumerate(np.asarray(g, dtype=np.int64)):
            i = j + shift
            if rates is None:
                out[n] = PER_SITE[i % len(PER_SITE)]
            else:
                base = 0 if rates == 4 else PER_SITE[(i // len(ROWS4)) % len(PER_SITE)]
                out[n] = pattern(i, rates) + base
    return out


def classes(counts):
    """the place in the cycle (0 .. n_classes - 1) every written entry stands for, recomputed from the array alone"""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim == 1:
        assert np.isin(counts, PER_SITE).all()
        return np.array([PER_SITE.index(int(v)) for v in counts])
    rates = counts.shape[1]
    rows = [pattern(i, rates) for i in range(len(ROWS4))]
    out = np.full(len(counts), -1)
    for n, row in enumerate(counts):
        for i, pat in enumerate(rows):
            base = int(row[0]) - int(pat[0])
            if (base == 0 if rates == 4 else base in PER_SITE) and np.array_equal(row, pat + base):
                out[n] = i
                break
    assert (out >= 0).all(), "a written row is none of the cycle's"
    return out


def assert_covered(counts, among=None, what=""):
    """every pattern class occurs at least once among the entries `among` (default: all) - a condition on the INPUTS"""
    cls = classes(counts)
    rates = None if np.ndim(counts) == 1 else np.shape(counts)[1]
    # rows of the cycle that coincide for this number of rates count as one class
    want = set(classes(table(n_classes(rates), rates)).tolist())
    have = set(cls[among].tolist() if among is not None else cls.tolist())
    assert want <= have, (what, "pattern classes missing", sorted(want - have))


def assert_rows4_properties():
    """what the module docstring says ROWS4 holds, recomputed"""
    rows = np.array(ROWS4)
    ex = rows - rows.min(1, keepdims=True)
    assert any((r == 0).all() for r in rows) and any((r == r[0]).all() and r[0] > 0 for r in rows)
    assert {int(r.argmin()) for r in rows if (r == r.min()).sum() == 1} == {0, 1, 2, 3}, "a unique minimum at every position"
    assert any((r == r.min()).sum() == 2 for r in rows), "a tie for the minimum"
    assert {1, 2, 3, RATE_MAXDIFF} <= set(ex.ravel().tolist()) and (ex > RATE_MAXDIFF).any()
    alone = {int(e.argmin()) for e in ex if (np.sort(e)[1:] >= RATE_MAXDIFF).all()}
    assert alone == {0, 1, 2, 3}, "one surviving category at each k"
    assert len(set(ROWS4)) == len(ROWS4)


def groups_of(session, case, clv_index):
    """the entry groups of a node's scale buffer: invariant and variable sites where the case has invariant sites (read
    from the partition the session drives), the ascertainment entries behind the sites, else all entries as one"""
    entries = session.entries(clv_index)
    real = entries - (case.states if case.asc_alloc else 0)
    groups = [np.arange(real)]
    if case.prop_invar.max() > 0:
        inv = invariant_sites(session)
        groups = [np.flatnonzero(inv), np.flatnonzero(~inv)]
    return entries, real, groups


def invariant_sites(session):
    """bool[sites]: partition->invariant[n] != -1"""
    return api.as_np(session.part.invariant, session.case.sites, np.int32) != -1


def counts_for(session, case, clv_index, second=False, shift=None):
    """the table of one end: [entries] or [entries][rates]; the cycle starts at place `shift` (default: 0, or
    SECOND_END_SHIFT for the second end of an edge)"""
    entries, real, groups = groups_of(session, case, clv_index)
    rates = case.rate_cats if per_rate(case) else None
    out = table(entries, rates, (SECOND_END_SHIFT if second else 0) if shift is None else shift, groups)
    if case.asc_alloc:
        extra = np.array(ASC_EXTRA[:case.states], dtype=np.uint32)
        out[real:] = extra if rates is None else extra[:, None]
    return out


def write_scaler(session, scaler_index, clv_index, counts):
    """see driver.Session.write_scaler: identical for both libraries but for the invalidate"""
    session.write_scaler(scaler_index, clv_index, counts)


# ---- the root log-likelihood restated --------------------------------------------------------------------------------
def root_restated(session, clv_index, counts, per_rate_counts):
    """pll_compute_root_loglikelihood from the partition's host arrays (the REFERENCE's) and the counts given:

        lnl[n] = w_n (log(sum_k r_k (t_k[n] 2^(-256 min(c_k[n] - m[n], 4)) (1 - pinv) + pinv pi[inv[n]])) + m[n] log(2^-256))

    t_k[n] = sum_j pi_j clv[n][k][j], m[n] = min_k c_k[n]; with per-site counts c_k = c. The invariant part stands inside
    the logarithm as in the reference's root formula (src/core_likelihood.c:176-198). The reference itself reads a
    per-rate vector as if it were per site there (:197), which is why its per-rate value is not the expected one.
    -> (total, per site)"""
    part, case = session.part, session.case
    s, sp, r, n = part.states, part.states_padded, part.rate_cats, part.sites
    entries = session.entries(clv_index) - (s if case.asc_alloc else 0)
    sid = session.lib.pll_get_site_id(session.p, clv_index)  # site -> entry under site repeats
    sid = api.as_np(sid, n, np.uint32) if sid else np.arange(n)
    clv = api.as_np(part.clv[clv_index], entries * r * sp, np.float64).reshape(entries, r, sp)[sid, :, :s]
    fi = np.asarray(case.freqs_indices)
    pi = np.stack([api.as_np(part.frequencies[int(f)], sp, np.float64)[:s] for f in fi])  # [rates][states]
    w = api.as_np(part.rate_weights, r, np.float64)
    term = np.einsum("nkj,kj->nk", clv, pi)
    c = np.asarray(counts, dtype=np.int64)[:entries][sid]
    if per_rate_counts:
        m = c.min(1)
        term = term * np.ldexp(1.0, (-256 * np.minimum(c - m[:, None], RATE_MAXDIFF)).astype(np.int64))
    else:
        m = c.reshape(n)
    pinv = np.array([api.as_np(part.prop_invar, part.rate_matrices, np.float64)[int(f)] for f in fi])
    if pinv.max() > 0:
        inv = api.as_np(part.invariant, n, np.int32)
        inv_lk = np.where(inv[:, None] >= 0, pi.T[np.maximum(inv, 0)], 0.0)  # [sites][rates]
        term = term * (1.0 - pinv)[None, :] + inv_lk * pinv[None, :]
    site = np.log(term @ w) + m * LOG_THRESHOLD
    site = site * api.as_np(part.pattern_weights, n, np.uint32)
    return float(site.sum()), site
