"""GPU: pll_gpu_branch_derivatives against the reference, live.

d_f[i], dd_f[i] are the reference's own: pll_update_sumtable into a caller-owned table, then
pll_compute_likelihood_derivatives at the row's length (gradient_cases.per_edge, either library). Tolerance: the project's
deriv_common.close - |d| <= DTOL |exp| + 4e-15 sites, DTOL = 1e-10, sites = the sum of the pattern weights - for EVERY d_f
and EVERY dd_f; the same values through this library's own per-edge path meet the same bound (bit-identity with that path
is not asked for).

Every edge of UTree(taxa, PCG64(7)) over W.random_states(taxa + 2, sites, states, seed 8, mutate 15 %) and
W.gamma_rates_mean(0.7, R) - the insertion tests' inputs - at the tree's own lengths (0.02 .. 0.40) and at four times them.
Much shorter lengths are not used: at a hundredth of the tree's lengths the reference's AVX2 and plain-C builds, two
summation orders of the same arithmetic, already differ by more than the bound on dd_f (conditioning, not an error); at the
lengths used here they agree within 0.13 of it.

The trees are large enough that the ends carry scaling counts - otherwise the excess factors of PLL_ATTRIB_RATE_SCALERS
would never differ from 1. Conditions on the inputs, recomputed from the reference in the test: under rate_scalers at least
half of the edges have a site whose per-rate counts (parent + child) differ between rates (the reference gives every edge
of every shape but 590 of 597 at 4 x 2); otherwise at least half of the edges have an end with a nonzero count. 61 x 4 with
pattern_tip is left out of the large matrix (the reference needs 17 s for it); test_ends_of_every_kind covers that
combination on a small tree.

Observed on an MI355X, every edge of every shape: the batched call's worst deviation is 0.06 - 0.17 of the bound at 4 and 5
states and at 20 x 4, 0.49 of it at 61 x 4; this library's per-edge path gives the same figures."""
import functools

import numpy as np
import pytest

import gradient_cases as GC
import insertion_cases as IC
from pllamd import api, driver, workload as W

pytestmark = pytest.mark.gpu

SHAPES = {"4x4": (4, 4, 300, 200), "4x2": (4, 2, 300, 65), "5x3": (5, 3, 300, 33), "20x4": (20, 4, 200, 33), "61x4": (61, 4, 160, 17)}
ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP, "rate_scalers": api.RATE_SCALERS}
EVERY_EDGE = [(s, a) for s in SHAPES for a in ATTRS if not (s == "61x4" and a == "pattern_tip")]
SMALL = {"4x4": (4, 4, 20, 130), "20x4": (20, 4, 20, 130), "61x4": (61, 4, 20, 17)}
FACTORS = (1.0, 4.0)
_REF = None  # the reference library of the session (functools.cache keys must be hashable)


@functools.lru_cache(maxsize=None)
def _case(states, rate_cats, taxa, sites):
    return IC.make(states, taxa, sites, rate_cats)


def _bed(lib, dims, attrs, **kw):
    states, rate_cats, taxa, sites = dims
    lay, seqs, cmap, exch, freqs = _case(*dims)
    return IC.Bed(lib, lay, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, **kw)


def _weight_sum(dims, kw):
    w = dict(kw).get("pattern_weights")
    return int(np.sum(w)) if w is not None else dims[3]


def _counts(bed, clv, scaler):
    """[sites, R or 1] scaling counts of an end; a tip, or an end without a scaler, counts 0"""
    per = bed.rate_cats if (bed.attrs & api.RATE_SCALERS) else 1
    if clv < bed.lay.tips or scaler < 0:
        return np.zeros((bed.sites, per), dtype=np.int64)
    return bed.scaler(scaler).astype(np.int64).reshape(bed.sites, per)


@functools.lru_cache(maxsize=None)
def _reference(dims, attrs, kw=()):
    """expected [2 E, 2] of every edge at both length factors, per edge (rates differ at some site, some end has a count),
    pll_count_invariant_sites: computed once per case and shared"""
    with _bed(_REF, dims, attrs, **dict(kw)) as b:
        rows = GC.prepare(b, FACTORS)
        exp = GC.per_edge(b, rows)
        differ, nonzero = [], []
        for p, ps, c, cs, _ in rows[:len(rows) // len(FACTORS)]:
            pc, cc = _counts(b, p, ps), _counts(b, c, cs)
            s = pc + cc
            differ.append(bool((s.max(axis=1) != s.min(axis=1)).any()))
            nonzero.append(bool(pc.any() or cc.any()))
        invariant = int(_REF.pll_count_invariant_sites(b.p, None)) if dict(kw).get("prop_invar") else 0
    exp.setflags(write=False)
    return exp, tuple(differ), tuple(nonzero), invariant


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    global _REF
    _REF = ref_lib


def _check(got, exp, sites, what):
    assert np.isfinite(got).all(), what
    assert GC.close(got, exp, sites), (what, GC.worst(got, exp, sites))


@pytest.mark.parametrize("shape,attrs", EVERY_EDGE)
def test_every_edge(amd_lib, shape, attrs):
    dims = SHAPES[shape]
    exp, differ, nonzero, _ = _reference(dims, ATTRS[attrs])
    edges = 2 * dims[2] - 3
    assert exp.shape == (2 * edges, 2) and len(differ) == edges
    print(f"{shape} {attrs}: of {edges} edges {sum(differ)} have a site whose per-rate counts differ, {sum(nonzero)} an end with a count")
    if attrs == "rate_scalers":
        assert sum(differ) >= 0.5 * edges, "the inputs do not exercise the excess factors"
    else:
        assert sum(nonzero) >= 0.5 * edges, "the inputs carry no scaling counts"
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = GC.prepare(b, FACTORS)
        got = GC.batched(b, rows)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        seq = GC.per_edge(b, rows)
    print(f"{shape} {attrs}: batched worst {GC.worst(got, exp, dims[3]):.3f} of the bound, per-edge worst {GC.worst(seq, exp, dims[3]):.3f}, "
          f"{launches} launch(es)")
    _check(got, exp, dims[3], "batched call against the reference")
    _check(seq, exp, dims[3], "per-edge path against the reference")
    assert launches == GC.launches_by_rule(dims[0], dims[1], dims[3], len(rows)) == 1


def _dense_tip(sites, states):
    """non-indicator rows: every state possible, with different weights"""
    rng = np.random.Generator(np.random.PCG64(11))
    return np.ascontiguousarray(rng.uniform(0.05, 1.0, size=(sites, states)))


def _kinds_rows(bed, dense):
    """every edge both ways round, and with dense: the dense spare tip against the other spare tip (codes), both ways round,
    and against an inner end"""
    rows = GC.prepare(bed)
    rows = rows + GC.flipped(rows)
    if dense:
        lay = bed.lay
        assert bed.lib.pll_set_tip_clv(bed.p, lay.T, api.dptr(_dense_tip(bed.sites, bed.states)), 0), (bed.lib.errno(), bed.lib.errmsg())
        inner = next(r for r in rows if r[0] >= lay.tips and r[1] >= 0)
        extra = [(lay.T, IC.NONE, lay.T + 1, IC.NONE, 0.1), (inner[0], inner[1], lay.T, IC.NONE, 0.2)]
        rows = rows + extra + GC.flipped(extra)
    return rows


@functools.lru_cache(maxsize=None)
def _reference_kinds(dims, attrs, dense):
    with _bed(_REF, dims, attrs) as b:
        exp = GC.per_edge(b, _kinds_rows(b, dense))
    exp.setflags(write=False)
    return exp


KINDS = [(s, a) for s in SMALL for a in ("plain", "pattern_tip")]


@pytest.mark.parametrize("shape,attrs", KINDS, ids=[f"{s}-{'compact_tips' if a == 'plain' else a}" for s, a in KINDS])
def test_ends_of_every_kind(amd_lib, shape, attrs):
    """tip as child, tip as parent, inner-inner in both orders; compact tips (plain) and pattern tips; without
    PLL_ATTRIB_PATTERN_TIP also a dense tip (pll_set_tip_clv, non-indicator rows) against a code tip and against an inner
    end, both ways round (the reference refuses two tips under PLL_ATTRIB_PATTERN_TIP). dd_f = NULL: the same d_f bits"""
    dims = SMALL[shape]
    dense = attrs == "plain"
    exp = _reference_kinds(dims, ATTRS[attrs], dense)
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = _kinds_rows(b, dense)
        tips = b.lay.tips
        kinds = {(r[0] < tips, r[2] < tips) for r in rows}
        assert kinds == ({(False, False), (True, False), (False, True), (True, True)} if dense else {(False, False), (True, False), (False, True)})
        got = GC.batched(b, rows)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 1
        _check(got, exp, dims[3], "mixed kinds")
        only_d = GC.batched(b, rows, want_dd=False)
        assert only_d[:, 0].tobytes() == got[:, 0].tobytes() and np.isnan(only_d[:, 1]).all()


PATTERN = (0, 1, 3, 4, 5, 1000, 7, 2)


def _written(sites, rate_cats):
    """counts[site][k] = PATTERN[(site + k) % 8], the first quarter of the sites all 2; and the same reversed in site order
    with the same quarter"""
    a = np.array([[PATTERN[(n + k) % 8] for k in range(rate_cats)] for n in range(sites)], dtype=np.uint32)
    b = a[::-1].copy()
    a[:sites // 4] = 2
    b[:sites // 4] = 2
    return a, b


def _inner_inner(bed, rows):
    lay = bed.lay
    return next(i for i, r in enumerate(rows) if r[0] >= lay.tips and r[2] >= lay.tips and r[1] >= 0 and r[3] >= 0 and r[1] != r[3])


@functools.lru_cache(maxsize=None)
def _reference_written(dims, attrs, one_none):
    with _bed(_REF, dims, attrs) as b:
        rows = GC.prepare(b)
        i = _inner_inner(b, rows)
        p, ps, c, cs, t = rows[i]
        per = dims[1] if attrs & api.RATE_SCALERS else 1
        a, rev = _written(dims[3], per)
        b.write_scaler(ps, a)
        b.write_scaler(cs, rev)
        row = (p, ps, c, IC.NONE if one_none else cs, t)
        exp = GC.per_edge(b, [row, (row[0], row[1], row[2], row[3], 4.0 * t)])
    exp.setflags(write=False)
    return exp


@pytest.mark.parametrize("one_none", [False, True], ids=["both_scalers", "one_scaler_none"])
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_written_scaling_counts(amd_lib, shape, one_none):
    """per-rate counts written by the caller on both ends of an inner-inner edge: sites with no excess, with an excess of
    1..3, of exactly 4 and beyond 4 (capped) all occur"""
    dims = SMALL[shape]
    a, rev = _written(dims[3], dims[1])
    s = a.astype(np.int64) + (0 if one_none else rev.astype(np.int64))
    excess = s - s.min(axis=1, keepdims=True)
    assert (excess.max(axis=1) == 0).any() and ((excess >= 1) & (excess <= 3)).any() and (excess == 4).any() and (excess > 4).any()
    exp = _reference_written(dims, api.RATE_SCALERS, one_none)
    assert np.isfinite(exp).all()
    with _bed(amd_lib, dims, api.RATE_SCALERS) as b:
        rows = GC.prepare(b)
        p, ps, c, cs, t = rows[_inner_inner(b, rows)]
        b.write_scaler(ps, a)
        b.write_scaler(cs, rev)
        row = (p, ps, c, IC.NONE if one_none else cs, t)
        pair = [row, (row[0], row[1], row[2], row[3], 4.0 * t)]
        got = GC.batched(b, pair)
        seq = GC.per_edge(b, pair)
    print(f"{shape} written counts: batched worst {GC.worst(got, exp, dims[3]):.3f} of the bound, per-edge {GC.worst(seq, exp, dims[3]):.3f}")
    _check(got, exp, dims[3], "written per-rate counts")
    _check(seq, exp, dims[3], "written per-rate counts, per-edge path")


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_written_counts_per_site_mode_change_no_bit(amd_lib, shape):
    """per-site scaling cancels in L'/L: the scalers are not read"""
    dims = SMALL[shape]
    a, rev = _written(dims[3], 1)
    with _bed(amd_lib, dims, 0) as b:
        rows = GC.prepare(b)
        before = GC.batched(b, rows)
        p, ps, c, cs, t = rows[_inner_inner(b, rows)]
        b.write_scaler(ps, a)
        b.write_scaler(cs, rev)
        after = GC.batched(b, rows)
    assert np.isfinite(before).all() and after.tobytes() == before.tobytes()


MODEL = {
    "invariant_sites": lambda sites: dict(prop_invar=0.3),
    "pattern_weights": lambda sites: dict(pattern_weights=tuple(int(n % 4) for n in range(sites))),
    "two_rate_matrices": lambda sites: dict(rate_matrices=2, freqs_indices=(0, 1, 0, 1)),
}
MODEL_CASES = [(s, n) for s in ("4x4", "20x4") for n in (1, 64, 65, 130)] + [("61x4", 17)]


@pytest.mark.parametrize("what", list(MODEL))
@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape,sites", MODEL_CASES)
def test_model_features(amd_lib, shape, sites, attrs, what):
    """prop_invar 0.3 after pll_update_invariant_sites, pattern weights site % 4 (zeros included), two rate matrices with
    params_indices (0, 1, 0, 1) - at one site, one tile, a tile and one, three tiles. Invariant sites exist wherever the
    alignment has a tile or more (10 and 6 of 130 sites at 4 x 4 and 20 x 4, 1 of 17 at 61 x 4)"""
    dims = SMALL[shape][:3] + (sites,)
    kw = tuple(sorted(MODEL[what](sites).items()))
    exp, _, _, invariant = _reference(dims, ATTRS[attrs], kw=kw)
    if what == "invariant_sites":
        print(f"{shape} {sites} sites: {invariant} invariant")
        if sites >= 64 or shape == "61x4":
            assert invariant > 0, "no invariant site: the invariant term is not exercised"
    if sites > 1:
        plain, _, _, _ = _reference(dims, ATTRS[attrs])
        assert not GC.close(plain, exp, dims[3]), "the feature does not change the values: nothing is tested"
    with _bed(amd_lib, dims, ATTRS[attrs], **dict(kw)) as b:
        if what == "invariant_sites" and invariant:
            assert amd_lib.pll_count_invariant_sites(b.p, None) == invariant
        _check(GC.batched(b, GC.prepare(b, FACTORS)), exp, _weight_sum(dims, kw), what)


@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_bits_do_not_depend_on_company(amd_lib, shape, attrs):
    """each value alone, in the full list, in the reversed list, with a duplicate row and in a second run: identical bits"""
    dims = SHAPES[shape][:2] + (20,) + SHAPES[shape][3:]
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = GC.prepare(b, FACTORS)
        full = GC.batched(b, rows)
        assert np.isfinite(full).all()
        assert GC.batched(b, rows).tobytes() == full.tobytes()
        assert GC.batched(b, rows[::-1]).tobytes() == full[::-1].tobytes()
        for i in range(len(rows)):
            assert GC.batched(b, [rows[i]]).tobytes() == full[i:i + 1].tobytes(), i
        for i in (0, len(rows) // 2, len(rows) - 1):
            assert GC.batched(b, [rows[i], rows[0], rows[i]]).tobytes() == full[[i, 0, i]].tobytes(), i


@pytest.mark.parametrize("shape,sites", [("4x4", 65), ("20x4", 33)])
def test_long_list_is_cut(amd_lib, shape, sites):
    """more rows than one launch carries descriptors for (8192; include/pll_amd_device.h states the cutting rule): the 37
    edges of the 20-taxon tree repeated cyclically to 8193 rows"""
    dims = SMALL[shape][:3] + (sites,)
    exp, _, _, _ = _reference(dims, 0)
    with _bed(amd_lib, dims, 0) as b:
        rows = GC.prepare(b)
        assert len(rows) == 37
        short = GC.batched(b, rows)
        _check(short, exp[:37], sites, "the unique rows")
        long_rows = [rows[i % 37] for i in range(8193)]
        got = GC.batched(b, long_rows)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        assert launches >= 2 and launches == GC.launches_by_rule(dims[0], dims[1], sites, 8193)
        assert got.tobytes() == short[np.arange(8193) % 37].tobytes()


def test_nothing_is_written(amd_lib):
    """CLVs and scalers of every node, the matrix mirrors, a resident sumtable made with other params_indices, the cached
    launch plan: all as before the call"""
    dims = SMALL["4x4"]
    kw = dict(rate_matrices=2, freqs_indices=(0, 1, 0, 1))
    other = np.ascontiguousarray((1, 0, 1, 0), dtype=np.uint32)
    with _bed(amd_lib, dims, 0, **kw) as b:
        lay, lib = b.lay, amd_lib
        b.query_cherry(lay.T, lay.T + 1)  # a spare slot the list does not name (and the two spare tips' codes go up)
        rows = GC.prepare(b, FACTORS)
        up_ops, _ = lay.upward()  # (the list GC.prepare ran last)

        def again():
            """the unchanged list once more: (went straight to the launches, what it adds to pll_gpu_plan_replays)"""
            r = lib.pll_gpu_plan_replays(b.p)
            b.update(up_ops)
            return lib.pll_gpu_last_update_replayed(b.p), lib.pll_gpu_plan_replays(b.p) - r

        nodes = [(lay.inner0 + i, i) for i in range((lay.T - 2) + (2 * lay.T - 4))] + [lay.cherry]  # inner nodes, upward slots, the spare
        def state():
            assert lib.pll_gpu_sync_pmatrix(b.p, -1)
            n = b.rate_cats * b.states * b.part.states_padded
            return ([(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in nodes],
                    [api.as_np(b.part.pmatrix[m], n, np.float64).tobytes() for m in range(lay.prob_matrices)])

        # a table of this library's per-edge path, made with OTHER params_indices, and its derivatives
        p, ps, c, cs, t = next(r for r in rows if r[0] >= lay.tips and r[2] >= lay.tips)
        n = b.sites * b.rate_cats * b.part.states_padded
        raw = np.zeros(n + 8)
        table = raw[(-raw.ctypes.data // 8) % 8:][:n]
        assert lib.pll_update_sumtable(b.p, p, c, ps, cs, api.uptr(other), api.dptr(table))

        def derivatives():
            import ctypes as C
            d1, d2 = C.c_double(0), C.c_double(0)
            assert lib.pll_compute_likelihood_derivatives(b.p, ps, cs, t, api.uptr(other), api.dptr(table), C.byref(d1), C.byref(d2))
            return d1.value, d2.value

        d_before = derivatives()
        before = state()
        # (the per-edge path's table and the downloads allocate device memory of their own: the plan is kept from here on)
        b.update(up_ops)
        replayed, counted = again()  # (the control: what an unchanged list does when nothing happens in between)
        print(f"an unchanged operation list adds {counted} to pll_gpu_plan_replays")
        assert replayed == 1
        got = GC.batched(b, rows)  # the partition's first batched call: its scratch is allocated here
        assert np.isfinite(got).all()
        assert again() == (1, counted)  # no kept plan was dropped
        assert lib.pll_gpu_pending_clvs(b.p) == 0
        assert derivatives() == d_before  # the resident table
        assert state() == before
        # ... and a later pll_update_sumtable sees the contraction matrices it expects
        assert lib.pll_update_sumtable(b.p, p, c, ps, cs, api.uptr(other), api.dptr(table))
        assert derivatives() == d_before
        assert GC.batched(b, rows).tobytes() == got.tobytes()
        lib.pll_gpu_release_sumtable(b.p, api.dptr(table))


def test_after_the_tree_launch(amd_lib, monkeypatch):
    """the balanced 64-taxon DNA case of tests/test_gpu_dna_lazy_cherries.py: traversal, root-edge log-likelihood, then
    DIRECTLY the call over edges that name cherry parents, which the tree launch left unstored. Bit for bit the values of the
    same sequence through the ordinary route"""
    case = W.make_case("lazy", 4, 64, 65, seed=5)
    ops = case.op_batches[0]
    cherries = [op for op in ops if op[2] < 64 and op[5] < 64]
    assert len(cherries) == 32
    parents = {op[0]: op[1] for op in cherries}
    rows = [(op[0], op[1], op[2], IC.NONE, 0.11) for op in cherries[:5]]              # cherry parent - its own tip
    rows += [(op[0], op[1], op[5], parents[op[5]], 0.23) for op in ops if op[5] in parents][:5]  # its parent - the cherry parent
    rows += [(op[2], parents[op[2]], op[0], op[1], 0.07) for op in ops if op[2] in parents][:5]  # ... the other way round
    assert len(rows) == 15
    out = {}
    for tree in ("1", "0"):
        monkeypatch.setenv("PLL_AMD_FUSE_TREE", tree)
        monkeypatch.delenv("PLL_AMD_LAZY_CHERRIES", raising=False)
        with driver.Session(amd_lib, case, api.ARCH_AVX2) as s:
            # (the case brings transition matrices only: the derivatives need the rate model they could have come from)
            s.set_model(W.GTR_DNA["exch"], case.freqs, W.gamma_rates_mean(0.7, 4))
            s.update_partials()
            lnl = s.edge_lnl(case.edges[0], persite=False)[0]
            pending = s.pending_clvs()
            got = driver.branch_derivatives(amd_lib, s.p, rows, case.freqs_indices)
            assert s.pending_clvs() == 0
            out[tree] = (lnl, got, pending)
    print(f"pending after the tree launch: {out['1'][2]}, through the ordinary route: {out['0'][2]}")
    assert np.isfinite(out["1"][1]).all()
    assert out["1"][0] == out["0"][0]
    assert out["1"][1].tobytes() == out["0"][1].tobytes()
