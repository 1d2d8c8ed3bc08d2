"""GPU: pll_gpu_qmatrix_gradient and pll_gpu_subst_gradient against the definitions restated in numpy on the REFERENCE's
CLVs (qmatrix_gradient_cases), against pll_gpu_rate_gradient through Euler's identity, and, end to end, against central
differences of the reference's log-likelihood.

Inputs: every edge of UTree(taxa, PCG64(7)) over the insertion tests' alignments and W.gamma_rates_mean(0.7, R), at the
tree's own lengths (gradient_cases.prepare: the parent is the root-side end). The criterion for d_q and d_root is
|got - exp| <= DTOL * abs + 4e-15 * sites elementwise, abs the same sum with every term's absolute value.

Observed on an MI355X: see the docstrings of test_parity_with_the_restatement, test_variants,
test_variants_at_the_long_walk and test_gradient_against_the_reference_lnl."""
import functools

import numpy as np
import pytest

import category_common as CC
import gradient_cases as GC
import insertion_cases as IC
import long_walk_cases as LW
import qmatrix_gradient_cases as QC
from deriv_common import DTOL
from pllamd import api, driver

pytestmark = pytest.mark.gpu

TAXA = 7
SHAPES = {"4x4": (4, 4), "4x1": (4, 1), "4x3": (4, 3), "5x4": (5, 4), "20x4": (20, 4), "61x2": (61, 2)}
PARITY = [(s, n) for s in ("4x4", "20x4") for n in (1, 63, 64, 65, 300)] + [(s, 65) for s in ("4x1", "4x3", "5x4", "61x2")]
# shapes beside SHAPES (which other tests run whole): more than four rate categories - a wave of the generic kernel takes two
# (4 x 8, two accumulator blocks per wave) - 5 x 7, the shape the kernel's static_assert names, state counts at a multiple of
# 16 (no padding rows; 64 x 2 fills the largest legal LDS, 140 288 bytes, with eight accumulator blocks per wave) and one
# above it (17: 15 padding rows, two 16-row blocks)
MORE_SHAPES = {"4x8": (4, 8), "5x7": (5, 7), "16x4": (16, 4), "64x2": (64, 2), "17x2": (17, 2)}
PARITY += [(s, 65) for s in MORE_SHAPES]
# the smallest site counts at which a wave (4 x 4) or a workgroup walks a second tile (long_walk_cases.qg_walk restates the
# rule: T tiles, w per walk, B workgroups per branch) - 4x4 16 385: 257, 2, 33; 20x4 1 025: 17, 2, 9; 20x4 3 137: 50, 4, 13;
# 5x4 4 097: 65, 2, 33; 61x2 257: 5, 2, 3 (eight accumulator blocks per wave); 4x8 4 097: 65, 2, 33. The last workgroup holds
# fewer tiles than the others, the last tile one site
LONG_WALK = [("4x4", 16385), ("20x4", 1025), ("20x4", 3137), ("5x4", 4097), ("61x2", 257), ("4x8", 4097)]
PARITY += LONG_WALK
_REF = None  # the reference library of the session (functools.cache keys must be hashable)


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    global _REF
    _REF = ref_lib


def _dims(shape, sites, taxa=TAXA):
    return (SHAPES.get(shape) or MORE_SHAPES[shape]) + (taxa, sites)


@functools.lru_cache(maxsize=None)
def _case(states, rate_cats, taxa, sites):
    return IC.make(states, taxa, sites, rate_cats)


def _bed(lib, dims, attrs, jc=False, exch=None, freqs=None, **kw):
    states, rate_cats, taxa, sites = dims
    lay, seqs, cmap, ex, fr = _case(*dims)
    if jc:
        ex, fr = np.ones(len(ex)), np.full(states, 1.0 / states)
    ex = ex if exch is None else exch
    fr = fr if freqs is None else freqs
    return IC.Bed(lib, lay, states, sites, rate_cats, attrs, seqs, cmap, ex, fr, **kw)


def _dense_tip(sites, states):
    """non-indicator rows, [sites][states]"""
    return np.ascontiguousarray(np.random.Generator(np.random.PCG64(21)).uniform(0.05, 1.0, (sites, states)))


PATTERN = (0, 1, 3, 4, 5, 1000, 7, 2)


def _written(sites, per):
    """counts[site][k] = PATTERN[(site + k) % 8], the first quarter of the sites all 2; and the same reversed in site order:
    sites with no excess, an excess of 1..3, of exactly 4 and beyond 4 (capped) all occur"""
    a = np.array([[PATTERN[(n + k) % 8] for k in range(per)] for n in range(sites)], dtype=np.uint32)
    b = a[::-1].copy()
    a[:sites // 4] = 2
    b[:sites // 4] = 2
    return a, b


def _rows(bed, variant):
    """the rows of a variant, after whatever it writes into the partition (either library)"""
    lay = bed.lay
    rows = GC.prepare(bed)
    if variant == "tip_parent":
        rows = GC.flipped(rows)
    if variant == "dense":
        assert bed.lib.pll_set_tip_clv(bed.p, lay.T, api.dptr(_dense_tip(bed.sites, bed.states)), 0), (bed.lib.errno(), bed.lib.errmsg())
        inner = next(r for r in rows if r[0] >= lay.tips and r[1] >= 0)
        extra = [(lay.T, IC.NONE, lay.T + 1, IC.NONE, 0.1), (inner[0], inner[1], lay.T, IC.NONE, 0.2)]
        rows = extra + GC.flipped(extra) + rows
    if variant in ("site_counts", "rate_counts"):
        per = bed.rate_cats if bed.attrs & api.RATE_SCALERS else 1
        a, rev = _written(bed.sites, per)
        i = next(i for i, r in enumerate(rows) if r[0] >= lay.tips and r[2] >= lay.tips and r[1] >= 0 and r[3] >= 0 and r[1] != r[3])
        bed.write_scaler(rows[i][1], a)
        bed.write_scaler(rows[i][3], rev)
        rows = [rows[i]] + rows[:i] + rows[i + 1:]  # the written edge first: d_root sees it as well
    return rows


def _root_first(bed, rows):
    """the rows with the traversal's root edge first: every other row points away from it (its parent is the root-side end),
    so the root sum - the explicit dependence on pi that d_root is - stands at that edge"""
    lay = bed.lay
    ends = {lay.end(lay.root)[0], lay.end(lay.root.back)[0]}
    i = next(i for i, r in enumerate(rows) if {r[0], r[2]} == ends)
    return [rows[i]] + rows[:i] + rows[i + 1:]


VARIANTS = {  # name: (device attributes, Bed keywords, d_root asked)
    "pattern_weights": (0, lambda sites: dict(pattern_weights=tuple(int(x) for x in CC.pattern_weights_for(sites))), True),
    "pinv": (0, lambda sites: dict(prop_invar=0.2), False),
    "site_counts": (0, lambda sites: {}, True),
    "rate_counts": (api.RATE_SCALERS, lambda sites: {}, True),
    "pattern_tip": (api.PATTERN_TIP, lambda sites: {}, True),
    "dense": (0, lambda sites: {}, True),
    "tip_parent": (api.PATTERN_TIP, lambda sites: {}, True),
    "two_matrices": (0, lambda sites: dict(rate_matrices=3, freqs_indices=(0, 2, 0, 2)), True),
    "jc69": (0, lambda sites: dict(jc=True), True),
}


@functools.lru_cache(maxsize=None)
def _restated(dims, variant):
    """the definitions on the reference's CLVs, once per case and shared"""
    attrs, kw, _ = VARIANTS[variant] if variant else (0, lambda sites: {}, True)
    with _bed(_REF, dims, attrs & api.RATE_SCALERS, **kw(dims[3])) as b:
        rows = _rows(b, variant)
        r = QC.restate(QC.Model.from_bed(b, b.fi), QC.read_ends(b, rows), rows)
    for a in r.values():
        a.setflags(write=False)
    return r


def _fraction(got, exp, scale, sites):
    assert got.shape == exp.shape and np.isfinite(got).all(), got
    return float(np.max(np.abs(got - exp) / (DTOL * scale + 4e-15 * sites)))


def _assert_parity(dims, variant, amd_lib, root=True):
    exp = _restated(dims, variant)
    attrs, kw, _ = VARIANTS[variant] if variant else (0, lambda sites: {}, True)
    with _bed(amd_lib, dims, attrs, **kw(dims[3])) as b:
        rows = _rows(b, variant)
        d_q, d_root = driver.qmatrix_gradient(amd_lib, b.p, rows, b.fi, want_root=root)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        used = len(set(int(x) for x in b.fi))
    fq = _fraction(d_q, exp["d_q"], exp["abs_q"], dims[3])
    fr = _fraction(d_root, exp["d_root"], exp["abs_root"], dims[3]) if root else float("nan")
    print(f"{dims} {variant or 'plain'}: d_q worst {fq:.3f} of the bound, d_root {fr:.3f}; largest |d_q| {np.abs(exp['d_q']).max():.3g}")
    assert np.abs(exp["d_q"]).max() > 1e-3 and (not root or np.abs(exp["d_root"]).max() > 1e-3), "the inputs give no gradient"
    assert fq <= 1.0 and (not root or fr <= 1.0)
    if not root:
        assert np.isnan(d_root).all()
    assert launches == QC.launches_by_rule(dims[0], dims[1], dims[3], len(rows), used, root) == 4
    return d_q, d_root


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,sites", PARITY)
def test_parity_with_the_restatement(amd_lib, shape, sites):
    """d_q and d_root of every edge's list against the restatement. Observed on an MI355X, worst fraction of the bound:
    d_q below 0.0005 at 4 states (every site count, 4 x 1, 4 x 3) and at 5 x 4; 20 x 4 0.000 / 0.006 / 0.002 / 0.002 / 0.002
    at 1 / 63 / 64 / 65 / 300 sites; 61 x 2 0.024; d_root below 0.0005 everywhere (the device differs from the restatement
    by rounding, 1e-13 to 1e-12 of the absolute-value sum, and DTOL is 1e-10 of it).
    MORE_SHAPES at 65 sites: d_q below 0.0005 at 4 x 8 and 5 x 7, 0.001 at 16 x 4, 0.004 at 17 x 2, 0.047 at 64 x 2. LONG_WALK:
    d_q below 0.0005 at 4 x 4 x 16 385, 20 x 4 x 1 025, 5 x 4 x 4 097 and 4 x 8 x 4 097, 0.001 at 20 x 4 x 3 137, 0.024 at
    61 x 2 x 257; d_root below 0.0005 everywhere."""
    if (shape, sites) in LONG_WALK:
        assert LW.qg_walk(*_dims(shape, sites)[:2], sites)[1] >= 2, "the walk is one tile long: nothing new is tested"
    _assert_parity(_dims(shape, sites), None, amd_lib)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_variants(amd_lib, shape, variant):
    """pattern weights; pinv 0.2 (d_q only); caller-written per-site counts (they cancel) and per-rate counts (excess 0, 1..3,
    4 and beyond); tips as codes, with PLL_ATTRIB_PATTERN_TIP, dense (pll_set_tip_clv) against a code tip and an inner end
    both ways round; every tip as the parent; two rate matrices (0, 2, 0, 2) of three - the unused one gets zeros; JC69, whose
    three equal eigenvalues take the degenerate Phi. Observed on an MI355X, worst fraction of the bound (d_q; d_root below
    0.0005 everywhere): 4 x 4 below 0.0005 in every variant; 20 x 4 0.002 pattern weights, 0.001 pinv, 0.002 / 0.001 written
    per-site / per-rate counts, 0.002 pattern tips, 0.001 dense, 0.001 tip as parent, 0.001 two matrices, 0.011 JC69."""
    dims = _dims(shape, 65)
    d_q, d_root = _assert_parity(dims, variant, amd_lib, root=VARIANTS[variant][2])
    if variant == "two_matrices":
        assert (d_q[1] == 0.0).all() and (d_root[1] == 0.0).all() and np.abs(d_q[0]).max() > 0 and np.abs(d_q[2]).max() > 0
        assert not np.allclose(d_q[0], d_q[2], rtol=1e-3)
    if variant == "rate_counts":
        plain = _restated(dims, None)["d_q"]
        assert not np.allclose(plain, _restated(dims, variant)["d_q"], rtol=1e-6), "the written counts change nothing"


@pytest.mark.parametrize("variant", ["pattern_tip", "rate_counts", "two_matrices"])
@pytest.mark.parametrize("shape,sites", [("20x4", 1025), ("4x4", 16385)])
def test_variants_at_the_long_walk(amd_lib, shape, sites, variant):
    """the tip decode, the per-rate excess factor and the second rate matrix inside the second pass of the tile walk.
    Observed on an MI355X, worst fraction of the bound: d_q 0.001 with two matrices at 20 x 4 x 1 025, below 0.0005 in the
    other five cases; d_root below 0.0005 everywhere."""
    dims = _dims(shape, sites)
    d_q, d_root = _assert_parity(dims, variant, amd_lib, root=VARIANTS[variant][2])
    if variant == "two_matrices":
        assert (d_q[1] == 0.0).all() and (d_root[1] == 0.0).all() and np.abs(d_q[0]).max() > 0 and np.abs(d_q[2]).max() > 0
        assert not np.allclose(d_q[0], d_q[2], rtol=1e-3)
    if variant == "rate_counts":
        plain = _restated(dims, None)["d_q"]
        assert not np.allclose(plain, _restated(dims, variant)["d_q"], rtol=1e-6), "the written counts change nothing"


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_euler_identity_with_the_rate_gradient(amd_lib, shape):
    """Q enters the likelihood through Q tau alone: sum_xy d_q[x][y] Q[x][y] is d_scale of pll_gpu_rate_gradient on the same
    list, within gradient_cases.close with d_scale as the expected value"""
    dims = _dims(shape, 65)
    with _bed(amd_lib, dims, 0) as b:
        rows = GC.prepare(b)
        d_q, _ = driver.qmatrix_gradient(amd_lib, b.p, rows, b.fi, want_root=False)
        d_scale = driver.rate_gradient(amd_lib, b.p, rows, b.fi, want_rates=False, want_cat=False, want_d=False)["d_scale"]
        q = QC.Model.from_bed(b, b.fi).q[0]
    euler = float(np.sum(d_q[0] * q))
    print(f"{shape}: sum d_q Q = {euler:.12g}, d_scale = {d_scale:.12g}, {GC.worst([euler], [d_scale], dims[3]):.3f} of the bound")
    assert abs(d_scale) > 1e-3 and GC.close([euler], [d_scale], dims[3])


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs", [0, api.PATTERN_TIP], ids=["plain", "pattern_tip"])
@pytest.mark.parametrize("shape", ["4x4", "5x4", "20x4"])
def test_flipped_rows(amd_lib, shape, attrs):
    """every row the other way round: P_b is used transposed, d_q may differ, the gradient of a reversible model's parameters
    does not"""
    dims = _dims(shape, 65)
    with _bed(amd_lib, dims, attrs) as b:
        rows = GC.prepare(b)
        d_subst, _ = driver.subst_gradient(amd_lib, b.p, rows, b.fi, want_freqs=False)
        flipped, _ = driver.subst_gradient(amd_lib, b.p, GC.flipped(rows), b.fi, want_freqs=False)
    print(f"{shape}: flipped rows, d_subst worst {GC.worst(flipped, d_subst, dims[3]):.3f} of the bound")
    assert np.abs(d_subst).max() > 1e-3 and GC.close(flipped, d_subst, dims[3])


# ---- 4 ---------------------------------------------------------------------------------------------------------------
STEP = 2.0 ** -12
END_TO_END = {"4x4": ((4, 4, 12, 130), 0.0, tuple(range(6)), tuple(range(4))), "4x4_pinv": ((4, 4, 12, 130), 0.2, tuple(range(6)), ()),
              "20x4": ((20, 4, 12, 33), 0.0, (0, 17, 60, 123, 188), (0, 7, 19))}


def _ref_lnl(b, subst, freqs):
    """set params + frequencies + (the eigensystem with) every branch's P matrix + full traversal + edge log-likelihood"""
    b.lib.pll_set_subst_params(b.p, 0, api.dptr(np.ascontiguousarray(subst, dtype=np.float64)))
    b.lib.pll_set_frequencies(b.p, 0, api.dptr(np.ascontiguousarray(freqs, dtype=np.float64)))
    b.matrices(list(b.lay.tree.branches()))
    b.update(b.lay.full_ops())
    r = b.lay.root
    return b.lnl(b.lay.end(r) + b.lay.end(r.back) + (r.pm,))


def _richardson(f, h, lnl):
    """(X, bound) of the derivative of f at 0 from central differences at h and h / 2: X = (4 D_{h/2} - D_h) / 3 within
    2 |D_h - D_{h/2}| + 8 eps |lnL| / (h / 2) + DTOL |X| (test_gpu_rate_gradient.py, section 8)"""
    d1 = (f(h) - f(-h)) / (2.0 * h)
    d2 = (f(h / 2) - f(-h / 2)) / h
    x = (4.0 * d2 - d1) / 3.0
    return x, 2.0 * abs(d1 - d2) + 8.0 * np.finfo(float).eps * abs(lnl) / (h / 2.0) + DTOL * abs(x)


@functools.lru_cache(maxsize=None)
def _end_to_end_reference(dims, pinv, params, states):
    with _bed(_REF, dims, 0, prop_invar=pinv) as b:
        m = QC.Model.from_bed(b, b.fi)
        subst, freqs = m.subst[0].copy(), m.freqs[0].copy()
        lnl = _ref_lnl(b, subst, freqs)
        assert np.isfinite(lnl)
        per_param, per_state = [], []
        for p in params:
            e = np.zeros(len(subst))
            e[p] = 1.0
            per_param.append(_richardson(lambda s: _ref_lnl(b, subst + s * e, freqs), STEP * subst[p], lnl))
        for x in states:  # normalised frequencies: pi(s) = (pi + s e_x) / (1 + s), d pi / ds = e_x - pi
            e = np.zeros(len(freqs))
            e[x] = 1.0
            per_state.append(_richardson(lambda s: _ref_lnl(b, subst, (freqs + s * e) / (1.0 + s)), STEP * freqs[x], lnl))
    return tuple(per_param), tuple(per_state)


@pytest.mark.parametrize("case", list(END_TO_END))
def test_gradient_against_the_reference_lnl(amd_lib, case):
    """The chain rule, the orientation of the ends, Phi and 1 / (1 - pinv), end to end: -d_subst[p] against the reference's
    log-likelihood as a function of subst_params[p] alone, and -(g_x - sum_y pi_y g_y), g = d_freqs, against it along
    pi(s) = (pi + s e_x) / (1 + s). The rows of gradient_cases.prepare point away from the traversal's root edge, so that edge
    is named first: d_root is taken at branches[0] (with a tip edge first the frequency part is off by several per cent,
    on the device and in the restatement alike; d_subst does not care). Observed on an MI355X: the reference's bounds are
    9e-9 to 7e-7 |X|, and the device is within 0.038 of the bound on every component at 4 x 4, 0.021 at 4 x 4 with pinv 0.2,
    0.077 at 20 x 4 (frequencies: at most 0.004). Conditions on the inputs, from the reference alone: every bound below 1e-5 |X|, every |X|
    above 1e-3."""
    dims, pinv, params, states = END_TO_END[case]
    per_param, per_state = _end_to_end_reference(dims, pinv, params, states)
    named = [(f"subst[{p}]", v) for p, v in zip(params, per_param)] + [(f"freq[{x}]", v) for x, v in zip(states, per_state)]
    for name, (x, bound) in named:
        print(f"{case} {name}: X {x:.9g}, bound {bound:.3g} = {bound / abs(x):.2e} |X|")
        assert bound < 1e-5 * abs(x), (name, "the bound could hide a wrong factor")
        assert abs(x) > 1e-3, (name, "a gradient component near zero")
    with _bed(amd_lib, dims, 0, prop_invar=pinv) as b:
        rows = _root_first(b, GC.prepare(b))
        assert len(rows) == 2 * dims[2] - 3
        d_subst, d_freqs = driver.subst_gradient(amd_lib, b.p, rows, b.fi, want_freqs=bool(states))
        pi = QC.Model.from_bed(b, b.fi).freqs[0]
    got = [-d_subst[0][p] for p in params]
    if states:
        g = d_freqs[0]
        got += [-(g[x] - float(np.dot(pi, g))) for x in states]
    for value, (name, (x, bound)) in zip(got, named):
        print(f"{case} {name}: device {value:.12g}, reference {x:.12g}, {abs(value - x) / bound:.3f} of the bound")
    for value, (name, (x, bound)) in zip(got, named):
        assert abs(value - x) <= bound, (name, value, x, bound)


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def test_long_list_is_cut_and_bits_repeat(amd_lib):
    """61 x 2 at 65 sites with d_root: two workgroups per branch leave 2 x 3721 values each, so a launch takes
    floor(4 Mi / (7442 x 2)) = 281 rows; 282 rows are two cuts = 7 launches. The sums over the sites do not depend on the
    cut (d_root: same bits as in the short list); the whole against the restatement; a second call repeats every bit, and
    rows appended after the last leave d_root as it was."""
    dims = _dims("61x2", 65, taxa=6)
    per_launch = QC.per_launch_by_rule(61, 2, 65, 1 << 30)
    assert per_launch == 281
    with _bed(_REF, dims, 0) as b:
        rows = GC.prepare(b)
        n = len(rows)
        long_rows = [rows[i % n] for i in range(per_launch + 1)]
        exp = QC.restate(QC.Model.from_bed(b, b.fi), QC.read_ends(b, rows), long_rows)
    with _bed(amd_lib, dims, 0) as b:
        rows = GC.prepare(b)
        short_q, short_root = driver.qmatrix_gradient(amd_lib, b.p, rows, b.fi)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 4
        d_q, d_root = driver.qmatrix_gradient(amd_lib, b.p, long_rows, b.fi)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        again_q, again_root = driver.qmatrix_gradient(amd_lib, b.p, long_rows, b.fi)
        more_q, more_root = driver.qmatrix_gradient(amd_lib, b.p, rows + rows[::-1], b.fi)
    assert launches == QC.launches_by_rule(61, 2, 65, len(long_rows)) == 7
    assert _fraction(d_q, exp["d_q"], exp["abs_q"], 65) <= 1.0 and _fraction(d_root, exp["d_root"], exp["abs_root"], 65) <= 1.0
    assert d_root.tobytes() == short_root.tobytes() == more_root.tobytes()
    assert again_q.tobytes() == d_q.tobytes() and again_root.tobytes() == d_root.tobytes()
    assert more_q.tobytes() != short_q.tobytes()


# ---- 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_nothing_is_written(amd_lib, shape):
    """CLVs and scalers of every node, the matrix mirrors and the pending CLVs: all as before the call"""
    dims = _dims(shape, 65)
    with _bed(amd_lib, dims, api.RATE_SCALERS) as b:
        lay = b.lay
        rows = GC.prepare(b)
        nodes = [(lay.inner0 + i, i) for i in range((lay.T - 2) + (2 * lay.T - 4))]

        def state():
            assert amd_lib.pll_gpu_sync_pmatrix(b.p, -1)
            n = b.rate_cats * b.states * b.part.states_padded
            return ([(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in nodes],
                    [api.as_np(b.part.pmatrix[m], n, np.float64).tobytes() for m in range(lay.prob_matrices)])

        before = state()
        pending = amd_lib.pll_gpu_pending_clvs(b.p)
        d_q, d_root = driver.qmatrix_gradient(amd_lib, b.p, rows, b.fi)
        d_subst, d_freqs = driver.subst_gradient(amd_lib, b.p, rows, b.fi)
        assert np.isfinite(d_q).all() and np.isfinite(d_subst).all() and np.isfinite(d_freqs).all()
        assert amd_lib.pll_gpu_pending_clvs(b.p) == pending == 0
        assert state() == before
        # pll_gpu_subst_gradient is the device call followed by the host routine
        s, f = np.zeros_like(d_subst[0]), np.zeros_like(d_freqs[0])
        assert amd_lib.pll_gpu_subst_gradient_from_dq(b.p, 0, api.dptr(d_q[0]), api.dptr(d_root[0]), api.dptr(s), api.dptr(f)) == 1
        assert s.tobytes() == d_subst[0].tobytes() and f.tobytes() == d_freqs[0].tobytes()


# ---- 7 ---------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.5


def test_refusals_with_a_device(amd_lib):
    """what is decided with a device context behind the partition: the frequency part with prop_invar > 0 (before any
    launch), a shape whose parked vectors exceed the LDS of a workgroup (61 x 4), class-compressed CLVs aside; outputs stay
    untouched; count == 0 gives zeros without a launch"""
    unsup = api.ERROR_GPU_UNSUPPORTED
    with _bed(amd_lib, _dims("4x4", 65), 0, prop_invar=0.2) as b:
        rows = GC.prepare(b)
        br, n = api.make_branches(rows), len(rows)
        d_q, d_root, d_subst, d_freqs = np.full((1, 4, 4), SENTINEL), np.full((1, 4), SENTINEL), np.full((1, 6), SENTINEL), np.full((1, 4), SENTINEL)
        assert amd_lib.pll_gpu_qmatrix_gradient(b.p, br, n, api.uptr(b.fi), api.dptr(d_q), api.dptr(d_root)) == 0
        assert amd_lib.errno() == unsup and "prop_invar" in amd_lib.errmsg()
        assert amd_lib.pll_gpu_subst_gradient(b.p, br, n, api.uptr(b.fi), api.dptr(d_subst), api.dptr(d_freqs)) == 0
        assert amd_lib.errno() == unsup and "prop_invar" in amd_lib.errmsg()
        assert all((v == SENTINEL).all() for v in (d_q, d_root, d_subst, d_freqs))
        assert amd_lib.pll_gpu_subst_gradient(b.p, br, n, api.uptr(b.fi), api.dptr(d_subst), None) == 1, amd_lib.errmsg()
        assert np.isfinite(d_subst).all() and (d_freqs == SENTINEL).all()
        assert amd_lib.pll_gpu_qmatrix_gradient(b.p, None, 0, None, api.dptr(d_q), api.dptr(d_root)) == 1
        assert (d_q == 0.0).all() and (d_root == 0.0).all()
    SHAPES["61x4"] = (61, 4)
    try:
        with _bed(amd_lib, _dims("61x4", 17), 0) as b:
            rows = GC.prepare(b)
            d_q = np.full((1, 61, 61), SENTINEL)
            assert amd_lib.pll_gpu_qmatrix_gradient(b.p, api.make_branches(rows), len(rows), api.uptr(b.fi), api.dptr(d_q), None) == 0
            assert amd_lib.errno() == unsup and "LDS" in amd_lib.errmsg()
            assert (d_q == SENTINEL).all()
    finally:
        del SHAPES["61x4"]
    # the two boundaries beside it: 20 x 5 needs 174 208 bytes of LDS, more than 160 KB; 61 x 3 more than eight accumulator
    # blocks per wave (and 209 120 bytes)
    for states, rate_cats in ((20, 5), (61, 3)):
        with _bed(amd_lib, (states, rate_cats, TAXA, 17), 0) as b:
            rows = GC.prepare(b)
            d_q, d_root = np.full((1, states, states), SENTINEL), np.full((1, states), SENTINEL)
            assert amd_lib.pll_gpu_qmatrix_gradient(b.p, api.make_branches(rows), len(rows), api.uptr(b.fi), api.dptr(d_q), api.dptr(d_root)) == 0
            assert amd_lib.errno() == unsup and "LDS" in amd_lib.errmsg(), (states, rate_cats, amd_lib.errno(), amd_lib.errmsg())
            assert (d_q == SENTINEL).all() and (d_root == SENTINEL).all()
