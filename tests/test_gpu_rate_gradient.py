"""GPU: pll_gpu_branch_category_derivatives and pll_gpu_rate_gradient against the reference, live.

d_cat[i][k] against the per-category oracle of rate_gradient_cases (the reference's posteriors under one-hot category weights
times the reference's own d_f under one-hot category and pattern weights), within DTOL A[i][k] + 4e-15 sum(pw); sum_k d_cat
against the reference's d_f; d_f / dd_f bit for bit pll_gpu_branch_derivatives'; d_rates / d_scale bit for bit the list-order
sums restated in numpy; and, end to end, -d_rates, -d_scale and the alpha recipe of INTEGRATION.md against Richardson-
extrapolated central differences of the reference's log-likelihood.

Inputs: every edge of UTree(taxa, PCG64(7)) over the insertion tests' alignments and W.gamma_rates_mean(0.7, R), at the
tree's own lengths. The oracle needs prop_invar = 0 where ends carry scaling counts and no counts where prop_invar > 0
(rate_gradient_cases asserts the latter from the reference's scale buffers).

Observed on an MI355X: see the docstrings of test_every_category_of_every_edge, test_scaled_ends and
test_gradient_against_the_reference_lnl."""
import functools

import numpy as np
import pytest

import category_common as CC
import gradient_cases as GC
import insertion_cases as IC
import rate_gradient_cases as RG
from deriv_common import DTOL
from pllamd import api, workload as W

pytestmark = pytest.mark.gpu

SHAPES = {"4x4": (4, 4, 20, 330), "4x2": (4, 2, 20, 65), "5x3": (5, 3, 20, 33), "4x8": (4, 8, 12, 70), "4x33": (4, 33, 8, 65),
          "20x4": (20, 4, 20, 130), "61x4": (61, 4, 20, 17)}
ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP, "rate_scalers": api.RATE_SCALERS}
EVERY_EDGE = [(s, a) for s in SHAPES for a in ATTRS if not (s == "61x4" and a == "pattern_tip")]
SCALED = {"4x4": (4, 4, 300, 65), "4x2": (4, 2, 300, 65), "20x4": (20, 4, 200, 33)}
SMALL = {"4x4": (4, 4, 20, 130), "20x4": (20, 4, 20, 130), "61x4": (61, 4, 20, 17)}
_REF = None  # the reference library of the session (functools.cache keys must be hashable)


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    global _REF
    _REF = ref_lib


@functools.lru_cache(maxsize=None)
def _case(states, rate_cats, taxa, sites):
    return IC.make(states, taxa, sites, rate_cats)


def _bed(lib, dims, attrs, weights=None, rates=None, **kw):
    states, rate_cats, taxa, sites = dims
    lay, seqs, cmap, exch, freqs = _case(*dims)
    b = IC.Bed(lib, lay, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, **kw)
    if weights is not None:
        lib.pll_set_category_weights(b.p, api.dptr(np.ascontiguousarray(weights, dtype=np.float64)))
    if rates is not None:
        _set_rates(b, rates)
    return b


def _set_rates(b, rates):
    """the rates, and every matrix of the layout formed with them"""
    b.lib.pll_set_category_rates(b.p, api.dptr(np.ascontiguousarray(rates, dtype=np.float64)))
    b.matrices(b.lay.branches())


def _weight_sum(dims, kw):
    w = dict(kw).get("pattern_weights")
    return int(np.sum(w)) if w is not None else dims[3]


@functools.lru_cache(maxsize=None)
def _oracle(dims, attrs, kw=(), weighted=False, limit=None):
    """(exp, A, d_f) of every edge (or of the edges `limit` names), once per case and shared"""
    weights = CC.weights_for(dims[1]) if weighted else None
    with _bed(_REF, dims, attrs, weights=weights, **dict(kw)) as b:
        rows, mats = RG.edge_rows(b)
        pick = range(len(rows)) if limit is None else limit
        out = RG.oracle(_REF, b, [rows[i] for i in pick], [mats[i] for i in pick], weights=weights)
    for a in out:
        a.setflags(write=False)
    return out


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,attrs", EVERY_EDGE)
def test_every_category_of_every_edge(amd_lib, shape, attrs):
    """Observed on an MI355X, worst fraction of the bound (d_cat / sum_k d_cat against the reference's d_f), the same under
    every attribute to the last digit shown: 4x4 0.011 / 0.003, 4x2 0.002 / 0.001, 5x3 0.002 / 0.002, 4x8 0.024 / 0.003,
    4x33 0.097 (0.114 with pattern tips) / 0.001, 20x4 0.016 / 0.004, 61x4 0.066 / 0.034."""
    dims = SHAPES[shape]
    exp, scale, d_f = _oracle(dims, ATTRS[attrs])
    assert exp.shape == (2 * dims[2] - 3, dims[1])
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows, _ = RG.edge_rows(b)
        cat, _, _ = RG.category_derivatives(b, rows)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
    RG.assert_categories(cat, exp, scale, d_f, dims[3], f"{shape} {attrs}")
    assert launches == RG.launches_by_rule(dims[0], dims[1], dims[3], len(rows)) == 1


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def _counts(bed, clv, scaler):
    per = bed.rate_cats
    if clv < bed.lay.tips or scaler < 0:
        return np.zeros((bed.sites, per), dtype=np.int64)
    return bed.scaler(scaler).astype(np.int64).reshape(bed.sites, per)


@functools.lru_cache(maxsize=None)
def _scaled_reference(dims):
    """the reference's d_f of every edge, and the edges with a site whose per-rate counts (parent + child) differ between rates"""
    with _bed(_REF, dims, api.RATE_SCALERS) as b:
        rows = GC.prepare(b)
        d_f = GC.per_edge(b, rows)[:, 0].copy()
        differ = []
        for i, (p, ps, c, cs, _) in enumerate(rows):
            s = _counts(b, p, ps) + _counts(b, c, cs)
            if (s.max(axis=1) != s.min(axis=1)).any():
                differ.append(i)
    d_f.setflags(write=False)
    return d_f, tuple(differ)


@pytest.mark.parametrize("shape", list(SCALED))
def test_scaled_ends(amd_lib, shape):
    """trees large enough that the ends carry per-rate scaling counts (prop_invar = 0): the excess factors differ from 1.
    Observed on an MI355X: 597 / 590 / 397 edges have a site whose counts differ between rates; d_cat on the first 40 within
    0.005 / 0.002 / 0.009 of the bound; the sum over the categories against the reference's d_f on every edge within 0.224 /
    0.064 / 0.049 of DTOL |d_f| + 4e-15 sites (4x4 / 4x2 / 20x4)."""
    dims = SCALED[shape]
    ref_d_f, differ = _scaled_reference(dims)
    print(f"{shape}: {len(differ)} of {len(ref_d_f)} edges have a site whose per-rate counts differ")
    assert len(differ) >= 40, "the inputs do not exercise the excess factors"
    first = tuple(differ[:40])
    exp, scale, d_f = _oracle(dims, api.RATE_SCALERS, limit=first)
    with _bed(amd_lib, dims, api.RATE_SCALERS) as b:
        rows, _ = RG.edge_rows(b)
        cat, _, _ = RG.category_derivatives(b, rows)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 1
    assert np.isfinite(cat).all()
    RG.assert_categories(cat[list(first)], exp, scale, d_f, dims[3], f"{shape} scaled, 40 edges")
    every = RG.sum_identity(cat, ref_d_f, dims[3])
    print(f"{shape}: sum_k d_cat against the reference's d_f on every edge: worst {every:.3f} of the bound")
    assert every <= 1.0


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_d_f_bits(amd_lib, shape, attrs):
    dims = SHAPES[shape]
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = GC.prepare(b)
        old = GC.batched(b, rows)
        _, d, dd = RG.category_derivatives(b, rows)
        g = RG.rate_gradient(b, rows)
    assert np.isfinite(old).all()
    assert (d.view(np.uint64) == old[:, 0].copy().view(np.uint64)).all()
    assert (dd.view(np.uint64) == old[:, 1].copy().view(np.uint64)).all()
    assert (g["d_f"].view(np.uint64) == d.view(np.uint64)).all()


# ---- 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_bits_do_not_depend_on_company(amd_lib, shape):
    dims = SHAPES[shape]
    with _bed(amd_lib, dims, 0) as b:
        rows = GC.prepare(b)
        full, _, _ = RG.category_derivatives(b, rows)
        assert np.isfinite(full).all()
        again, _, _ = RG.category_derivatives(b, rows)
        assert again.tobytes() == full.tobytes()
        order = np.random.Generator(np.random.PCG64(3)).permutation(len(rows))
        shuffled, _, _ = RG.category_derivatives(b, [rows[i] for i in order])
        assert shuffled.tobytes() == full[order].tobytes()
        for i in range(len(rows)):
            alone, _, _ = RG.category_derivatives(b, [rows[i]], want_d=False, want_dd=False)
            assert alone.tobytes() == full[i:i + 1].tobytes(), i
        for i in (0, len(rows) // 2, len(rows) - 1):
            twice, _, _ = RG.category_derivatives(b, [rows[i], rows[0], rows[i]])
            assert twice.tobytes() == full[[i, 0, i]].tobytes(), i


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def _rates(dims):
    return np.ascontiguousarray(W.gamma_rates_mean(0.7, dims[1]), dtype=np.float64)


def _assert_contraction(g, rows, rates):
    exp_rates, exp_scale = RG.restated(g["d_cat"], g["d_f"], [r[4] for r in rows], rates)
    assert np.isfinite(g["d_rates"]).all() and np.isfinite(g["d_scale"])
    assert (g["d_rates"].view(np.uint64) == exp_rates.view(np.uint64)).all(), (g["d_rates"], exp_rates)
    assert np.float64(g["d_scale"]).tobytes() == np.float64(exp_scale).tobytes(), (g["d_scale"], exp_scale)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rate_gradient_is_the_contraction(amd_lib, shape):
    dims = SHAPES[shape]
    with _bed(amd_lib, dims, 0) as b:
        rows = GC.prepare(b)
        g = RG.rate_gradient(b, rows)
        with_sums = amd_lib.pll_gpu_last_launch_count(b.p)
        cat, d, _ = RG.category_derivatives(b, rows)
        without = amd_lib.pll_gpu_last_launch_count(b.p)
        only_scale = RG.rate_gradient(b, rows, want_rates=False, want_cat=False, want_d=False)
        only_rates = RG.rate_gradient(b, rows, want_scale=False, want_cat=False, want_d=False)
    assert with_sums == without + 1 == RG.launches_by_rule(dims[0], dims[1], dims[3], len(rows), contraction=True)
    assert g["d_cat"].tobytes() == cat.tobytes() and g["d_f"].tobytes() == d.tobytes()
    _assert_contraction(g, rows, _rates(dims))
    assert only_scale["d_scale"] == g["d_scale"] and np.isnan(only_scale["d_rates"]).all()
    assert only_rates["d_rates"].tobytes() == g["d_rates"].tobytes() and np.isnan(only_rates["d_scale"])


# ---- 6 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sites", [33, 961], ids=["one_workgroup", "sixteen_workgroups"])
def test_long_list_is_cut(amd_lib, sites):
    """4 x 33: R + 2 = 35 values per workgroup. One workgroup per branch: the descriptor limit cuts (8192 rows a launch).
    Sixteen workgroups per branch: floor(4 Mi / (35 x 16)) = 7489 rows a launch, where two values per workgroup would still
    have fitted 8192 - the R + 2 rule itself cuts. Row counts from the rule include/pll_amd_device.h states."""
    dims = SHAPES["4x33"][:3] + (sites,)
    per_launch = RG.per_launch_by_rule(dims[0], dims[1], sites, 1 << 30)
    assert per_launch == (8192 if sites == 33 else 7489)
    count = per_launch + 1
    with _bed(amd_lib, dims, 0) as b:
        rows = GC.prepare(b)
        n = len(rows)
        short, short_d, short_dd = RG.category_derivatives(b, rows)
        assert np.isfinite(short).all() and amd_lib.pll_gpu_last_launch_count(b.p) == 1
        long_rows = [rows[i % n] for i in range(count)]
        got, d, dd = RG.category_derivatives(b, long_rows)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        g = RG.rate_gradient(b, long_rows)
        launches_sums = amd_lib.pll_gpu_last_launch_count(b.p)
    assert launches == RG.launches_by_rule(dims[0], dims[1], sites, count) == 2
    assert launches_sums == 3
    pick = np.arange(count) % n
    assert got.tobytes() == short[pick].tobytes() and d.tobytes() == short_d[pick].tobytes() and dd.tobytes() == short_dd[pick].tobytes()
    assert g["d_cat"].tobytes() == got.tobytes()
    _assert_contraction(g, long_rows, _rates(dims))


# ---- 7 ---------------------------------------------------------------------------------------------------------------
MODEL = {
    "prop_invar": lambda dims: (dict(prop_invar=0.2), False),
    "category_weights": lambda dims: (dict(), True),
    "pattern_weights": lambda dims: (dict(pattern_weights=tuple(int(x) for x in CC.pattern_weights_for(dims[3]))), False),
    "two_rate_matrices": lambda dims: (dict(rate_matrices=2, freqs_indices=(0, 1, 0, 1)), False),
}


@pytest.mark.parametrize("what", list(MODEL))
@pytest.mark.parametrize("shape", list(SMALL))
def test_prop_invar_weights_mixture(amd_lib, shape, what):
    dims = SMALL[shape]
    kw, weighted = MODEL[what](dims)
    key = tuple(sorted(kw.items()))
    exp, scale, d_f = _oracle(dims, 0, kw=key, weighted=weighted)
    plain, _, _ = _oracle(dims, 0)
    assert not (np.abs(plain - exp) <= RG.bound(scale, _weight_sum(dims, key))).all(), "the feature does not change the values"
    weights = CC.weights_for(dims[1]) if weighted else None
    with _bed(amd_lib, dims, 0, weights=weights, **kw) as b:
        rows, _ = RG.edge_rows(b)
        cat, _, _ = RG.category_derivatives(b, rows)
    RG.assert_categories(cat, exp, scale, d_f, _weight_sum(dims, key), f"{shape} {what}")


# ---- 8 ---------------------------------------------------------------------------------------------------------------
ALPHA = 0.7
GAMMA_RATES_MEAN = 0  # PLL_GAMMA_RATES_MEAN
STEP = 2.0 ** -12
END_TO_END = {"4x4": ((4, 4, 12, 130), 0.0), "4x4_pinv": ((4, 4, 12, 130), 0.2), "20x4": ((20, 4, 12, 33), 0.0)}


def _gamma(alpha, cats):
    r = np.zeros(cats)
    assert _REF.pll_compute_gamma_cats(float(alpha), cats, api.dptr(r), GAMMA_RATES_MEAN)
    return r


def _ref_lnl(b, rates, factor=1.0):
    """set rates + every branch's P matrix + full traversal + edge log-likelihood, on the reference"""
    b.lib.pll_set_category_rates(b.p, api.dptr(np.ascontiguousarray(rates, dtype=np.float64)))
    b.matrices([(m, x * factor) for m, x in b.lay.tree.branches()])
    b.update(b.lay.full_ops())
    r = b.lay.root
    return b.lnl(b.lay.end(r) + b.lay.end(r.back) + (r.pm,))


def _richardson(f, h, lnl):
    """(X, bound) of the derivative of f at 0 from central differences at h and h / 2: X = (4 D_{h/2} - D_h) / 3 within
    2 |D_h - D_{h/2}| + 8 eps |lnL| / (h / 2) + DTOL |X|"""
    d1 = (f(h) - f(-h)) / (2.0 * h)
    d2 = (f(h / 2) - f(-h / 2)) / h
    x = (4.0 * d2 - d1) / 3.0
    return x, 2.0 * abs(d1 - d2) + 8.0 * np.finfo(float).eps * abs(lnl) / (h / 2.0) + DTOL * abs(x)


@functools.lru_cache(maxsize=None)
def _end_to_end_reference(dims, pinv):
    """per rate k, for the length multiplier and for alpha: (X, bound) from the reference's log-likelihood alone"""
    rates = _gamma(ALPHA, dims[1])
    with _bed(_REF, dims, 0, weights=CC.weights_for(dims[1]), prop_invar=pinv) as b:
        lnl = _ref_lnl(b, rates)
        assert np.isfinite(lnl)
        per_rate = []
        for k in range(dims[1]):
            e_k = np.zeros(dims[1])
            e_k[k] = 1.0
            per_rate.append(_richardson(lambda s: _ref_lnl(b, rates + s * e_k), STEP * rates[k], lnl))
        scale = _richardson(lambda s: _ref_lnl(b, rates, 1.0 + s), STEP, lnl)
        alpha = _richardson(lambda s: _ref_lnl(b, _gamma(ALPHA + s, dims[1])), STEP * ALPHA, lnl)
    return tuple(per_rate), scale, alpha


@pytest.mark.parametrize("case", list(END_TO_END))
def test_gradient_against_the_reference_lnl(amd_lib, case):
    """The chain rule, the orientation of the ends and 1 / (1 - pinv), end to end: -d_rates[k], -d_scale and the alpha recipe
    (sum_k d_rates[k] dr_k/dalpha, dr_k/dalpha a central difference of pll_compute_gamma_cats at 2^-16 alpha) against the
    reference's log-likelihood as a function of r_k alone (no renormalisation), of a multiplier of all lengths, and of alpha.
    Conditions on the inputs, from the reference alone: every bound below 1e-5 |X|, every |X| above 1e-3. The step is
    h = 2^-12 r_k (2^-12 for the multiplier, 2^-12 alpha): at 2^-10 the truncation term of r_0 at 20 x 4, whose |X| = 0.093 lies
    beside a sign change, makes the bound 3.1e-5 |X|; at 2^-12 every bound is below 2.7e-6 |X|.
    Observed fractions of the bound on an MI355X (r_0 .. r_3, multiplier, alpha): 4x4 0.017 0.001 0.009 0.002 0.000 0.032;
    4x4 with pinv 0.2 0.002 0.000 0.008 0.003 0.002 0.193; 20x4 0.052 0.000 0.001 0.000 0.001 0.013."""
    dims, pinv = END_TO_END[case]
    per_rate, scale, alpha = _end_to_end_reference(dims, pinv)
    for name, (x, bound) in [(f"r_{k}", v) for k, v in enumerate(per_rate)] + [("scale", scale), ("alpha", alpha)]:
        print(f"{case} {name}: X {x:.9g}, bound {bound:.3g} = {bound / abs(x):.2e} |X|")
        assert bound < 1e-5 * abs(x), (name, "the bound could hide a wrong factor")
        assert abs(x) > 1e-3, (name, "a gradient component near zero")
    rates = _gamma(ALPHA, dims[1])
    with _bed(amd_lib, dims, 0, weights=CC.weights_for(dims[1]), rates=rates, prop_invar=pinv) as b:
        rows = GC.prepare(b)
        assert len(rows) == 2 * dims[2] - 3
        g = RG.rate_gradient(b, rows)
    got = [(-g["d_rates"][k], per_rate[k], f"r_{k}") for k in range(dims[1])] + [(-g["d_scale"], scale, "scale")]
    da = 2.0 ** -16 * ALPHA
    dr = (_gamma(ALPHA + da, dims[1]) - _gamma(ALPHA - da, dims[1])) / (2.0 * da)
    got.append((-float(np.dot(g["d_rates"], dr)), alpha, "alpha"))
    for value, (x, bound), name in got:
        print(f"{case} {name}: device {value:.12g}, reference {x:.12g}, {abs(value - x) / bound:.3f} of the bound")
    for value, (x, bound), name in got:
        assert abs(value - x) <= bound, (name, value, x, bound)


# ---- 9 ---------------------------------------------------------------------------------------------------------------
SENTINEL = -12345.5
TIPS, INNER, SITES, MATRICES = 7, 6, 20, 9
SEQ = b"ACGTACGTACGTACGTACGT"
GOOD = [(TIPS, 0, TIPS + 1, 1, 0.1), (TIPS + 2, 2, 0, -1, 0.25), (3, 4, TIPS + 5, -1, 0.0), (TIPS + 4, -1, TIPS + 3, 5, 1.5)]


def _partition(lib, attrs=0):
    p = lib.pll_partition_create(TIPS, INNER, 4, SITES, 1, MATRICES, 4, INNER, attrs | api.ARCH_AVX2)
    assert p, (lib.errno(), lib.errmsg())
    nt = lib.state_map("pll_map_nt")
    for t in range(TIPS):
        assert lib.pll_set_tip_states(p, t, nt, SEQ), (lib.errno(), lib.errmsg())
    return p


def _outputs():
    return {"d_cat": np.full((4, 4), SENTINEL), "d_f": np.full(4, SENTINEL), "dd_f": np.full(4, SENTINEL), "d_rates": np.full(4, SENTINEL),
            "d_scale": np.full(1, SENTINEL)}


def _both(lib, p, rows, pi, out, null_list=False, count=None):
    """the status of both calls on the same input"""
    br = None if null_list else api.make_branches(rows)
    n = len(rows) if count is None else count
    a = lib.pll_gpu_branch_category_derivatives(p, br, n, api.uptr(pi), api.dptr(out["d_cat"]), api.dptr(out["d_f"]), api.dptr(out["dd_f"]))
    ea = lib.errno()
    b = lib.pll_gpu_rate_gradient(p, br, n, api.uptr(pi), api.dptr(out["d_rates"]), api.dptr(out["d_scale"]), api.dptr(out["d_cat"]),
                                  api.dptr(out["d_f"]))
    return (a, ea), (b, lib.errno())


def _with(row, field, value, rows=GOOD):
    rows = [list(r) for r in rows]
    rows[row][field] = value
    return rows


def test_checks_and_refusals(amd_lib):
    """in order of precedence: all outputs NULL; NULL list; index out of range; negative length; two code-tip ends; site
    repeats; an ascertainment-bias attribute; a zero rate with d_rates asked. Each case also carries every fault that comes
    later in the order where one input can: the earlier one is reported. Outputs stay untouched on failure."""
    lib = amd_lib
    pi = np.zeros(4, dtype=np.uint32)
    zero_rate = np.array([0.0, 0.5, 1.0, 2.5])
    inv, unsup = api.ERROR_PARAM_INVALID, api.ERROR_GPU_UNSUPPORTED
    bad_index, bad_length, two_tips = _with(1, 0, TIPS + INNER), _with(0, 4, -1.0), _with(2, 2, 5)
    # an index and a length wrong in one row (the list is checked row by row, the index first) and two code tips in another
    later = _with(1, 4, -1.0, _with(2, 2, 5, bad_index))

    def expect(attrs, rows, code, null_list=False, rates=None, contains=None):
        p = _partition(lib, attrs)
        try:
            if rates is not None:
                lib.pll_set_category_rates(p, api.dptr(rates))
            out = _outputs()
            for status, errno in _both(lib, p, rows, pi, out, null_list=null_list):
                assert status == 0 and errno == code, (status, errno, lib.errmsg())
            if contains:
                assert contains in lib.errmsg(), lib.errmsg()
            assert all((v == SENTINEL).all() for v in out.values())
        finally:
            lib.pll_partition_destroy(p)

    worst_attrs = api.SITE_REPEATS  # (no partition has site repeats and an ascertainment-bias correction at once)
    # all outputs NULL, everything else wrong as well
    p = _partition(lib, worst_attrs)
    try:
        lib.pll_set_category_rates(p, api.dptr(zero_rate))
        assert lib.pll_gpu_branch_category_derivatives(p, None, 4, api.uptr(pi), None, None, None) == 0
        assert lib.errno() == inv and "output" in lib.errmsg()
        assert lib.pll_gpu_rate_gradient(p, None, 4, api.uptr(pi), None, None, None, None) == 0
        assert lib.errno() == inv and "output" in lib.errmsg()
    finally:
        lib.pll_partition_destroy(p)
    expect(worst_attrs, later, inv, null_list=True, rates=zero_rate, contains="NULL")
    expect(worst_attrs, later, inv, rates=zero_rate, contains="index out of range")
    expect(worst_attrs, _with(0, 4, -1.0, two_tips), inv, rates=zero_rate, contains="length")
    expect(worst_attrs, two_tips, inv, rates=zero_rate, contains="tips given by codes")
    for rows in (bad_index, bad_length, two_tips):
        expect(0, rows, inv)
    expect(worst_attrs, GOOD, unsup, rates=zero_rate, contains="SITE_REPEATS")
    expect(api.AB_FLAG | api.AB_LEWIS, later, inv, rates=zero_rate, contains="index out of range")
    expect(api.AB_FLAG | api.AB_LEWIS, GOOD, unsup, rates=zero_rate, contains="ascertainment")
    expect(api.AB_FLAG | api.AB_STAMATAKIS, GOOD, unsup)

    # a zero rate: refused where d_rates is asked for, served where it is not; count == 0
    dims = SMALL["4x4"]
    with _bed(lib, dims, 0) as b:
        _set_rates(b, zero_rate)
        rows = GC.prepare(b)
        n = len(rows)
        br = api.make_branches(rows)
        d_rates, d_scale, d_cat, d_f = np.full(4, SENTINEL), np.full(1, SENTINEL), np.full((n, 4), SENTINEL), np.full(n, SENTINEL)
        assert lib.pll_gpu_rate_gradient(b.p, br, n, api.uptr(b.fi), api.dptr(d_rates), api.dptr(d_scale), api.dptr(d_cat), api.dptr(d_f)) == 0
        assert lib.errno() == inv and "rate" in lib.errmsg()
        assert (d_rates == SENTINEL).all() and (d_scale == SENTINEL).all() and (d_cat == SENTINEL).all() and (d_f == SENTINEL).all()
        assert lib.pll_gpu_rate_gradient(b.p, br, n, api.uptr(b.fi), None, api.dptr(d_scale), api.dptr(d_cat), api.dptr(d_f)) == 1, lib.errmsg()
        assert np.isfinite(d_cat).all() and np.isfinite(d_f).all() and np.isfinite(d_scale).all() and (d_rates == SENTINEL).all()
        assert (d_cat[:, 0] == 0.0).all()  # a category of rate zero does not see the branch lengths
        cat, d, dd = RG.category_derivatives(b, rows)
        assert cat.tobytes() == d_cat.tobytes() and d.tobytes() == d_f.tobytes()

        # count == 0: no launch, nothing read; d_rates and d_scale are sums over no branch
        out = _outputs()
        assert lib.pll_gpu_rate_gradient(b.p, None, 0, None, api.dptr(out["d_rates"]), api.dptr(out["d_scale"]), api.dptr(out["d_cat"]),
                                         api.dptr(out["d_f"])) == 1
        assert (out["d_rates"] == 0.0).all() and (out["d_scale"] == 0.0).all()
        assert (out["d_cat"] == SENTINEL).all() and (out["d_f"] == SENTINEL).all()
        assert lib.pll_gpu_branch_category_derivatives(b.p, None, 0, None, None, None, None) == 1
        assert lib.pll_gpu_branch_category_derivatives(b.p, None, 0, None, api.dptr(out["d_cat"]), api.dptr(out["d_f"]), api.dptr(out["dd_f"])) == 1
        assert (out["d_cat"] == SENTINEL).all() and (out["d_f"] == SENTINEL).all() and (out["dd_f"] == SENTINEL).all()
