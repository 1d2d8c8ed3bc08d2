"""The batched calls where a wave (4 x 4) or a workgroup (every other shape) walks a SECOND 64-site tile, against the
reference, live: insertion, placement, quartets, resampled quartets, branch derivatives, per-category derivatives and the
rate gradient at the smallest site counts that reach tiles_per = 2 (long_walk_cases.SIZES):

    shape   sites     T      w   B     last workgroup
    4 x 4   262 145   4 097  2   513   wave 0: one tile holding 1 site, then it leaves; waves 1-3 leave at once
    20 x 4  65 537    1 025  2   513   one tile holding 1 site, then the whole workgroup leaves in front of the barrier
    5 x 3   65 537    1 025  2   513   as above, fewer rate categories than waves

B = 513 partial sums per candidate are more than the 256 threads that add them, and the ticket counts 513 workgroups.
Trees: UTree(5, PCG64(7)) - 7 candidates / branches, 2 inner edges, 2 extra tips. Expected values are the reference's own
through the existing test beds (insertion_cases.Bed.per_edge, placement_cases.reference, quartet_cases.per_edge,
resample_cases.persite_per_edge, gradient_cases.per_edge), each call under its existing tolerance.

Every call also repeats its bytes in a second call (the tickets are back at zero) and returns, for the first candidate
alone and for the first two, the bytes they have in the full list.

Sensitivity, a condition on the inputs from the reference alone (test_a_lost_tile_would_show, no GPU): the last site - the
only site of the last tile, the one the short last workgroup holds - has pattern weight 50 in both libraries, every other
site 1, and the reference's values with that weight at 0 differ from those at 50 by at least ten times the tolerance of
the comparison for every candidate, branch and category. The per-site rows of the resampling call show a misplaced tile
directly.

The per-category oracle of rate_gradient_cases forms one reference call per site and category, each over every site:
quadratic in the site count and out of reach here. In its place d_cat is held to (a) sum_k d_cat against the
reference's d_f (rate_gradient_cases.sum_identity, which asks no less than the oracle's bound on the sum), (b) per
category, under the one-hot category weights e_k set in both libraries, d_cat[:, k] against the reference's d_f within
gradient_cases.close - with weights e_k the posterior of category k is 1, so the two are the same sum, and A[k] >= |d_f|
makes this bound no wider than rate_gradient_cases.bound - and the other categories exactly 0, (c) d_f / dd_f bit for bit
pll_gpu_branch_derivatives', d_rates / d_scale bit for bit rate_gradient_cases.restated.

Observed on an MI355X: see the docstring of each test. A library whose 4 x 4 walk and whose k_quartet_tiled walk ignore the
tile number t (the first tile taken twice) fails every 4 x 4 case and every quartet case here by 5e-4 to 4e-3 of |lnL| -
finite, plausible, wrong - and the derivatives by eleven orders of magnitude of their bound."""
import functools
import time

import numpy as np
import pytest

import gradient_cases as GC
import insertion_cases as IC
import long_walk_cases as LW
import placement_cases as PC
import qmatrix_gradient_cases as QG
import quartet_cases as QC
import rate_gradient_cases as RG
import resample_cases as RC
from compare import RTOL
from deriv_common import DTOL
from pllamd import api, workload as W

gpu = pytest.mark.gpu

SIZES, BOTH = LW.SIZES, LW.BOTH
ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP, "rate_scalers": api.RATE_SCALERS}
# the insertion call: a query tip at every size; a cherry, pattern tips and per-rate scalers at 4 x 4 and 20 x 4
INSERTION = [(s, "plain", "tip") for s in SIZES] + [(s, a, e) for s in BOTH for a, e in (("plain", "cherry"), ("pattern_tip", "tip"), ("rate_scalers", "tip"))]
FACTOR = 10.0  # a lost tile moves every value by at least this many tolerances
_REF = None  # the reference library of the session (functools.cache keys must be hashable)


@pytest.fixture
def ref(ref_lib):
    """the tests that take it read the reference library as _REF (the rule test needs none)"""
    global _REF
    _REF = ref_lib


# ---- the rule --------------------------------------------------------------------------------------------------------
def test_the_sizes_reach_a_second_tile():
    """T, w and B of every size from the rule include/pll_amd_device.h states: every walk is at least two tiles long, the
    batched sizes leave more partial sums than a workgroup has threads, and the last workgroup is short - one tile of one
    site at the batched sizes. A change of max_blocks fails here instead of quietly testing the short walk again."""
    assert {k: LW.walk(*v[:2], v[3]) for k, v in SIZES.items()} == {"4x4": (4097, 2, 513), "20x4": (1025, 2, 513), "5x3": (1025, 2, 513)}
    for states, rate_cats, _, sites in SIZES.values():
        tiles, w, blocks = LW.walk(states, rate_cats, sites)
        assert w >= 2 and blocks > 256
        assert LW.walk(states, rate_cats, sites - 1)[1] == w - 1, "not the smallest size of this walk length"
        assert LW.last_workgroup(states, rate_cats, sites) == (1, 4 * w if states == 4 else w, 1)
    expected = {(4, 4, 16385): (257, 2, 33), (20, 4, 1025): (17, 2, 9), (20, 4, 3137): (50, 4, 13), (5, 4, 4097): (65, 2, 33),
                (61, 2, 257): (5, 2, 3), (4, 8, 4097): (65, 2, 33)}
    assert set(expected) == set(LW.QG_SIZES)
    for dims in LW.QG_SIZES:
        tiles, w, blocks = LW.qg_walk(*dims)
        assert (tiles, w, blocks) == expected[dims]
        assert w >= 2
        held, full, sites_last = LW.last_workgroup(*dims, rule=LW.qg_walk)
        assert held < full and sites_last == 1, dims
    # the restatements the other modules carry agree
    for states, rate_cats, _, sites in SIZES.values():
        assert RG.blocks_by_rule(states, rate_cats, sites) == LW.walk(states, rate_cats, sites)[2]
    for dims in LW.QG_SIZES:
        assert QG.blocks_by_rule(*dims) == LW.qg_walk(*dims)[2]
    # the slot budget, not the descriptor limit, cuts a long list at B = 513
    assert PC.MAX_SLOTS // 513 == 8176 < PC.MAX_CANDS and PC.launches(4, 4, 262145, 1, 8177) == 2


# ---- the reference side, once per case and shared -----------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _subtree(b, end):
    return b.query_cherry(b.lay.T, b.lay.T + 1) if end == "cherry" else (b.lay.T, IC.NONE, b.lay.pm_pendant)


@functools.lru_cache(maxsize=None)
def _ref_insertion(shape, attrs, end):
    """(expected, the same with the last site's weight at 0)"""
    with LW.bed(_REF, SIZES[shape], ATTRS[attrs]) as b:
        sub = _subtree(b, end)
        rows = b.prepare()
        exp = b.per_edge(sub, rows)
        LW.drop_last_site(b)
        lost = b.per_edge(sub, rows)
    return _frozen(exp, lost)


def _placement_kw(sites, last):
    return (("pattern_weights", tuple(int(x) for x in LW.pattern_weights(sites, last))),)


@functools.lru_cache(maxsize=None)
def _ref_placement(shape):
    dims = SIZES[shape]
    exp, _ = PC.reference(_REF, dims, 0, 2, (0, 1), kw=_placement_kw(dims[3], LW.LAST_WEIGHT))
    lost, _ = PC.reference(_REF, dims, 0, 2, (0, 1), kw=_placement_kw(dims[3], 0))
    return exp, lost


@functools.lru_cache(maxsize=None)
def _ref_quartets(shape):
    with LW.bed(_REF, SIZES[shape]) as b:
        rows = QC.prepare(b)
        exp = QC.per_edge(b, rows)
        LW.drop_last_site(b)
        lost = QC.per_edge(b, rows)
    return _frozen(exp, lost)


@functools.lru_cache(maxsize=None)
def _ref_persite(shape):
    """(lnl [2, 3], u [2, 3, sites]) on pattern weights 1"""
    with LW.bed(_REF, SIZES[shape], last=None) as b:
        lnl, u = RC.persite_per_edge(b, QC.prepare(b))
    return _frozen(lnl, u)


def _branch_rows(b, shape):
    rows = GC.prepare(b)
    return rows + GC.flipped(rows) if shape in BOTH else rows


def _one_hot(b, k):
    e = np.zeros(b.rate_cats)
    e[k] = 1.0
    b.lib.pll_set_category_weights(b.p, api.dptr(e))


@functools.lru_cache(maxsize=None)
def _ref_gradient(shape):
    """(expected [rows, 2], the same without the last site, per category k the expected [rows, 2] under the category
    weights e_k, the same without the last site)"""
    with LW.bed(_REF, SIZES[shape]) as b:
        rows = _branch_rows(b, shape)
        exp = GC.per_edge(b, rows)
        per_cat = []
        for k in range(b.rate_cats):
            _one_hot(b, k)
            per_cat.append(GC.per_edge(b, rows))
        LW.drop_last_site(b)
        lost_cat = []
        for k in range(b.rate_cats):
            _one_hot(b, k)
            lost_cat.append(GC.per_edge(b, rows))
        b.lib.pll_set_category_weights(b.p, api.dptr(np.full(b.rate_cats, 1.0 / b.rate_cats)))
        lost = GC.per_edge(b, rows)
    return _frozen(exp, lost, np.stack(per_cat), np.stack(lost_cat))


def _replicates(sites):
    """2 rows of resample_cases.weights with the last site's count raised to 50: the site a lost tile would drop counts"""
    w = RC.weights(sites, 2).copy()
    w[:, -1] = LW.LAST_WEIGHT
    return w


# ---- the condition on the inputs (no GPU) -----------------------------------------------------------------------------
def _lnl_margin(exp, lost):
    return float(np.min(np.abs(exp - lost) / (RTOL * np.maximum(np.abs(exp), 1.0))))


def _deriv_margin(exp, lost, weight_sum):
    return float(np.min(np.abs(exp - lost) / (DTOL * np.abs(exp) + 4e-15 * weight_sum)))


def _margins(shape, call):
    sites = SIZES[shape][3]
    wsum = LW.weight_sum(sites)
    if call == "insertion":
        return {f"insertion {a} {e}": _lnl_margin(*_ref_insertion(s, a, e)) for s, a, e in INSERTION if s == shape}
    if call == "placement":
        return {"placement": _lnl_margin(*_ref_placement(shape))}
    if call == "quartets":
        return {"quartets": _lnl_margin(*_ref_quartets(shape))}
    if call == "derivatives":
        exp, lost, cat, lost_cat = _ref_gradient(shape)
        return {"d_f, dd_f": _deriv_margin(exp, lost, wsum), "d_f under e_k": _deriv_margin(cat[:, :, 0], lost_cat[:, :, 0], wsum)}
    # the resampled sums: the last site's term against the comparison's tolerance and against the contraction's bound
    lnl, u = _ref_persite(shape)
    w = _replicates(sites)
    assert u.shape == (2, 3, sites) and np.isfinite(u).all()
    term = w[:, -1].astype(np.float64)[None, :, None] * np.abs(u[:, None, :, -1])
    res = RC.resampled_from(u, w)
    return {"resampled": float(np.min(term / (RTOL * np.maximum(np.abs(res), 1.0)))), "resampled, stage 2": float(np.min(term / RC.stage2_bound(u, w)))}


LOST = [(s, c) for s in SIZES for c in ("insertion", "placement", "quartets", "derivatives")] + [(s, "resampled") for s in BOTH]


@pytest.mark.parametrize("shape,call", LOST)
def test_a_lost_tile_would_show(ref, shape, call):
    """from the reference alone: with the last site's weight at 0 instead of 50 every expected value moves by at least ten
    times its tolerance. Smallest margins, in tolerances, 4 x 4 / 20 x 4 / 5 x 3: insertion 9.3e5 (cherry) / 3.3e6 (cherry) /
    3.6e6, placement 1.0e6 / 3.6e6 / 3.6e6, quartets 1.2e6 / 4.1e6 / 4.1e6, d_f and dd_f 2.7e4 / 8.6e3 / 6.6e4, d_f under the
    category weights e_k 4.3e4 / 1.0e5 / 2.3e5, resampled sums 1.2e6 / 4.1e6 (4.0e6 / 5.6e7 of the contraction's own bound)."""
    margins = _margins(shape, call)
    for what, m in margins.items():
        print(f"{shape} {what}: a lost last tile moves every value by at least {m:.3g} tolerances")
    assert margins and all(m >= FACTOR for m in margins.values()), margins


# ---- what every call is asked ----------------------------------------------------------------------------------------------
def _same(x, y):
    xs, ys = (x, y) if isinstance(x, tuple) else ((x,), (y,))
    return all(np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes() for a, b in zip(xs, ys))


def _repeat_and_prefix(call, rows, full, what):
    """a second identical call returns the same bytes; the first candidate alone, and the first two, the bytes they have
    in the full list"""
    assert _same(call(rows), full), (what, "a second call")
    for count in (1, 2):
        part = call(rows[:count])
        head = tuple(a[:count] for a in full) if isinstance(full, tuple) else full[:count]
        assert _same(part, head), (what, "the first", count)


def _check_lnl(got, exp, what):
    assert got.shape == exp.shape and np.isfinite(got).all(), what
    print(f"{what}: worst {IC.worst(got, exp) / RTOL:.4f} of the bound")
    assert IC.close(got, exp, RTOL), (what, IC.worst(got, exp))


@gpu
@pytest.mark.parametrize("shape,attrs,end", INSERTION)
def test_insertion(amd_lib, ref, shape, attrs, end):
    """every edge; a cherry of the two extra tips (an inner CLV with a scaler) as the subtree end, tip codes in the walk
    (PLL_ATTRIB_PATTERN_TIP) and per-rate scalers at 4 x 4 and 20 x 4. Observed on an MI355X, worst fraction of the bound:
    4 x 4 0.010 (cherry 0.022), 20 x 4 0.001, 5 x 3 0.003, the same under every attribute to the digits shown."""
    dims = SIZES[shape]
    exp, _ = _ref_insertion(shape, attrs, end)
    with LW.bed(amd_lib, dims, ATTRS[attrs]) as b:
        sub = _subtree(b, end)
        rows = b.prepare()
        assert len(rows) == 7
        got = b.batched(sub, rows)
        assert 1 <= amd_lib.pll_gpu_last_launch_count(b.p) <= 3  # (with what the upward operations held back)
        _check_lnl(got, exp, f"insertion {shape} {attrs} {end}")
        assert _same(b.batched(sub, rows), got)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == PC.launches(dims[0], dims[1], dims[3], 1, len(rows)) == 1
        _repeat_and_prefix(lambda r: b.batched(sub, r), rows, got, "insertion")


@gpu
@pytest.mark.parametrize("shape", list(SIZES))
def test_placement(amd_lib, ref, shape):
    """2 queries x every edge against placement_cases.reference; each row is the insertion call's, byte for byte. Observed on
    an MI355X, worst fraction of the bound: 4 x 4 0.011, 20 x 4 0.001, 5 x 3 0.003."""
    dims = SIZES[shape]
    exp, _ = _ref_placement(shape)
    with PC.bed(amd_lib, dims, 0, 2, **dict(_placement_kw(dims[3], LW.LAST_WEIGHT))) as b:
        rows = b.prepare()
        tips = [b.lay.T, b.lay.T + 1]
        got = PC.placement(b, tips, rows)
        assert 1 <= amd_lib.pll_gpu_last_launch_count(b.p) <= 3  # (with what the upward operations held back)
        _check_lnl(got, exp, f"placement {shape}")
        assert _same(PC.placement(b, tips, rows), got), "a second call"
        assert amd_lib.pll_gpu_last_launch_count(b.p) == PC.launches(dims[0], dims[1], dims[3], 2, len(rows)) == 1
        assert (got[0] != got[1]).all(), "two queries give the same value somewhere: the query axis is not tested"
        assert _same(PC.placement(b, tips, rows), got), "a second call"
        for count in (1, 2):
            assert _same(PC.placement(b, tips, rows[:count]), got[:, :count]), count
        for r, t in enumerate(tips):
            assert _same(b.batched(PC.query(b.lay, t), rows), got[r]), ("row of query tip", t)


@gpu
@pytest.mark.parametrize("shape", list(SIZES))
def test_quartets(amd_lib, ref, shape):
    """all three arrangements of both inner edges against quartet_cases.per_edge. Observed on an MI355X, worst fraction of
    the bound: 4 x 4 0.016, 20 x 4 0.001, 5 x 3 0.002."""
    exp, _ = _ref_quartets(shape)
    with LW.bed(amd_lib, SIZES[shape]) as b:
        rows = QC.prepare(b)
        assert len(rows) == 2
        got = QC.batched(b, rows)
        assert 1 <= amd_lib.pll_gpu_last_launch_count(b.p) <= 3  # (with what the upward operations held back)
        _check_lnl(got, exp, f"quartets {shape}")
        assert _same(QC.batched(b, rows), got)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 1
        _repeat_and_prefix(lambda r: QC.batched(b, r), rows, got, "quartets")


@gpu
@pytest.mark.parametrize("shape", BOTH)
def test_resampled_quartets(amd_lib, ref, shape):
    """want_persite with 2 replicate rows on pattern weights 1: the per-site rows - the one output that shows which site a
    tile of the walk went to - against resample_cases.persite_per_edge entry by entry, their length, no NaN; the resampled
    sums against fsum over the reference's rows and, against the device's own rows, within resample_cases.stage2_bound.
    Observed on an MI355X, worst fraction of the bound, 4 x 4 / 20 x 4: lnl 0.016 / 0.001, per-site entries below 0.0001 /
    0.0002, resampled sums 0.0001 / below 0.0001, the contraction 0.0003 / 0.0005 of its own bound."""
    dims = SIZES[shape]
    sites = dims[3]
    lnl_exp, u_exp = _ref_persite(shape)
    w = _replicates(sites)
    with LW.bed(amd_lib, dims, last=None) as b:
        rows = QC.prepare(b)
        got = RC.call(b, rows, w)
        lnl, res, per = got
        assert per.shape == (2, 3, sites) and res.shape == (2, 2, 3)
        assert not np.isnan(per).any() and not np.isnan(res).any()
        _check_lnl(lnl, lnl_exp, f"resampled quartets {shape}: lnl")
        _check_lnl(per, u_exp, f"resampled quartets {shape}: persite")
        _check_lnl(res, RC.resampled_from(u_exp, w), f"resampled quartets {shape}: resampled")
        bound = RC.stage2_bound(per, w)
        stage2 = np.abs(res - RC.resampled_from(per, w)) / bound
        print(f"resampled quartets {shape}: stage 2 worst {stage2.max():.4f} of its bound")
        assert (bound > 0).all() and (stage2 <= 1.0).all()
        assert _same(lnl, QC.batched(b, rows)), "lnl is not what pll_gpu_quartet_loglikelihoods returns"
        _repeat_and_prefix(lambda r: RC.call(b, r, w), rows, got, "resampled quartets")


@gpu
@pytest.mark.parametrize("shape", list(SIZES))
def test_branch_and_category_derivatives(amd_lib, ref, shape):
    """d_f and dd_f of every branch (both ways round at 4 x 4 and 20 x 4: a tip by codes is parent and child in the walk)
    against gradient_cases.per_edge within gradient_cases.close; d_cat, d_rates and d_scale as the module docstring says.
    Observed on an MI355X, worst fraction of the bound, 4 x 4 / 20 x 4 / 5 x 3: d_f and dd_f 0.031 / 0.006 / 0.009, sum_k d_cat
    against the reference's d_f 0.010 / 0.006 / 0.001, d_cat[:, k] under the weights e_k 0.009 / 0.097 / 0.001."""
    dims = SIZES[shape]
    states, rate_cats, _, sites = dims
    wsum = LW.weight_sum(sites)
    exp, _, exp_cat, _ = _ref_gradient(shape)
    with LW.bed(amd_lib, dims) as b:
        rows = _branch_rows(b, shape)
        assert len(rows) == (14 if shape in BOTH else 7)
        got = GC.batched(b, rows)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == GC.launches_by_rule(states, rate_cats, sites, len(rows)) == 1
        assert np.isfinite(got).all()
        print(f"derivatives {shape}: d_f, dd_f worst {GC.worst(got, exp, wsum):.4f} of the bound")
        assert GC.close(got, exp, wsum), GC.worst(got, exp, wsum)
        _repeat_and_prefix(lambda r: GC.batched(b, r), rows, got, "branch derivatives")

        cat, d, dd = RG.category_derivatives(b, rows)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == RG.launches_by_rule(states, rate_cats, sites, len(rows)) == 1
        assert np.isfinite(cat).all() and cat.shape == (len(rows), rate_cats)
        assert _same(d, got[:, 0]) and _same(dd, got[:, 1])
        every = RG.sum_identity(cat, exp[:, 0], wsum)
        print(f"derivatives {shape}: sum_k d_cat against the reference's d_f worst {every:.4f} of the bound")
        assert every <= 1.0
        _repeat_and_prefix(lambda r: RG.category_derivatives(b, r), rows, (cat, d, dd), "category derivatives")

        g = RG.rate_gradient(b, rows)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == RG.launches_by_rule(states, rate_cats, sites, len(rows), contraction=True) == 2
        assert _same(g["d_cat"], cat) and _same(g["d_f"], d)
        rates = np.ascontiguousarray(W.gamma_rates_mean(0.7, rate_cats), dtype=np.float64)
        exp_rates, exp_scale = RG.restated(cat, d, [r[4] for r in rows], rates)
        assert np.isfinite(g["d_rates"]).all() and np.isfinite(g["d_scale"])
        assert _same(g["d_rates"], exp_rates) and np.float64(g["d_scale"]).tobytes() == np.float64(exp_scale).tobytes()
        again = RG.rate_gradient(b, rows)
        assert _same(again["d_rates"], g["d_rates"]) and again["d_scale"] == g["d_scale"]

        worst = 0.0
        for k in range(rate_cats):
            _one_hot(b, k)
            one, _, _ = RG.category_derivatives(b, rows, want_d=False, want_dd=False)
            assert np.isfinite(one).all()
            assert (np.delete(one, k, axis=1) == 0.0).all(), (k, "a category of weight 0 contributes")
            assert RG.worst(one[:, k], exp_cat[k][:, 0], np.abs(exp_cat[k][:, 0]), wsum) <= 1.0, k
            worst = max(worst, RG.worst(one[:, k], exp_cat[k][:, 0], np.abs(exp_cat[k][:, 0]), wsum))
        print(f"derivatives {shape}: d_cat[:, k] under the weights e_k worst {worst:.4f} of the bound")


@gpu
def test_the_slot_budget_cuts_a_long_list(amd_lib, ref):
    """4 x 4 x 262 145, the 7 rows repeated to 8 177 candidates: with B = 513 a launch has partial slots for
    floor(4 Mi / 513) = 8 176, fewer than the 16 384 descriptors, so the slot budget cuts: two launches, and every value
    has the bytes it has in the short list. Observed on an MI355X: 0.07 s for the long call."""
    dims = SIZES["4x4"]
    exp, _ = _ref_insertion("4x4", "plain", "tip")
    with LW.bed(amd_lib, dims) as b:
        sub = _subtree(b, "tip")
        rows = b.prepare()
        short = b.batched(sub, rows)
        _check_lnl(short, exp, "the short list")
        long_rows = [rows[i % 7] for i in range(8177)]
        t0 = time.perf_counter()
        got = b.batched(sub, long_rows)
        print(f"8177 candidates x 262145 sites: {time.perf_counter() - t0:.2f} s")
        assert amd_lib.pll_gpu_last_launch_count(b.p) == PC.launches(4, 4, dims[3], 1, 8177) == 2
        assert got.tobytes() == short[np.arange(8177) % 7].tobytes()
