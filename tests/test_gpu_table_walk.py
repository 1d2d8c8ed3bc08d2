"""The two calls that leave a table per site - pll_compute_node_ancestral and pll_gpu_edge_category_posteriors /
pll_gpu_category_weights_em - where a wave (4 x 4) or a workgroup (every other shape) of stage A walks a SECOND 64-site tile,
against the reference, live. Both cut with tile_walk(c, kTableBlocks = 4096), so the sizes are four times those of
test_gpu_long_walk.py (long_walk_cases.TABLE_SIZES; the rule restated in long_walk_cases.table_walk / mix_walk /
reduce_rounds and held to these figures by test_the_table_sizes_reach_a_second_tile):

    size   sites      stage A: T, w, B                                      stage B (k_category_mix)        stage C
    4x4    1 048 577  16385, 2, 2049  last workgroup: wave 0, 1 tile of 1   4097 tiles over 1024 workgroups  1 round
    20x4   262 145    4097, 2, 2049   last workgroup: 1 tile of 1 site      1025 tiles: workgroup 0 walks    1 round
                                                                            twice, its second tile 1 site
    4x8    262 145    4097, 2, 2049   the tiled form, 8 categories over 4   as 20x4                          2 rounds
                                      waves                                                                  (7 + 2 values)
    5x3    524 353    8194, 3, 2732   last workgroup: 1 of 3 tiles; 3 waves 2049 tiles                       1 round

The partition is long_walk_cases.TableBed: 4 tips, 2 inner CLVs, the inner edge (4, 0, 5, 1, 4) and the tip edge
(4, 0, 0, NONE, 0), category rates gamma_rates_mean(0.7, R), category weights category_common.weights_for(R) normalised,
pattern weights 1 but 50 at the last site - the only site of the last tile, the one the short last workgroup holds.

Every expectation is the reference's through the existing helpers under the existing tolerances (compare.RTOL,
ancestral_common.SUMTOL / assert_table, category_common.expected / assert_outputs); with per-rate counts that differ between
the categories of a site the ancestral expectation is ancestral_common.restated on the reference's host arrays, as everywhere
(kernels_ancestral.h). Every output buffer is prefilled with -7 and carries 64 guard entries behind it that must stay -7.

pll_compute_node_ancestral adds its one launch to pll_gpu_last_launch_count without setting it back (test_gpu_ancestral.py
reads it the same way): "one launch" is asserted as the count's growth over the call.

Written counts (both libraries, Bed.write_scaler): at sites 0, 63, 64 (the first site of a walker's second tile), the last
site of workgroup 0's walk and the last site; per-rate rows whose excess over the site's smallest summed count is 0..3 -
below the cap of 4, whose subnormal special case test_gpu_categories.py owns - and per-site counts 0..3.

Sensitivity, from the reference alone (test_a_lost_table_tile_would_show, no GPU): see its docstring.

Observed on an MI355X: see the docstring of each test."""
import functools

import numpy as np
import pytest

import category_common as CC
import insertion_cases as IC
import long_walk_cases as LW
from ancestral_common import SUMTOL, assert_table, restated
from compare import RTOL
from pllamd import api
from test_gpu_categories import WANT_SETS

gpu = pytest.mark.gpu

SIZES = LW.TABLE_SIZES
ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP, "rate_scalers": api.RATE_SCALERS}
INNER, TIP = LW.TableLayout.INNER, LW.TableLayout.TIP
ANCESTRAL_EDGES = {"inner": INNER, "inner, the other way round": (INNER[2], INNER[3], INNER[0], INNER[1], INNER[4]), "tip": TIP}
CATEGORY_EDGES = {"inner": INNER, "tip": TIP}
EVERY = [(s, a) for s in SIZES for a in ("plain", "pattern_tip")]
ANCESTRAL_WRITTEN = ("4x4", "20x4")
CATEGORY_WRITTEN = [(s, a) for s in ("4x4", "4x8") for a in ("plain", "rate_scalers")]
EM_SIZES = ("4x8", "4x4")
EM_STEPS = 2
FACTOR = 10.0  # a lost tile moves every sum by at least this many tolerances
GUARD, SENTINEL = 64, -7.0
_REF = None  # the reference library of the session (functools.cache keys must be hashable)


@pytest.fixture
def ref(ref_lib):
    """the tests that take it read the reference library as _REF (the rule test needs none)"""
    global _REF
    _REF = ref_lib


def _weights(rate_cats):
    w = CC.weights_for(rate_cats)
    return w / w.sum()


def _bed(lib, size, attrs):
    dims = SIZES[size]
    return LW.TableBed(lib, dims, ATTRS[attrs], _weights(dims[1]))


# ---- the rule --------------------------------------------------------------------------------------------------------
def test_the_table_sizes_reach_a_second_tile():
    """T, w and B of stage A, the tiles and workgroups of stage B and the rounds of stage C at every size, from the rule
    include/pll_amd_device.h states: every stage A walk is at least two tiles long, three sizes are the smallest of their
    walk length, the last workgroup is short and the last tile holds one site; stage B's stride runs a second time and
    stage C makes a second round at 4 x 8 alone. A change of kTableBlocks or kCategoryReduceDoubles fails here instead of
    quietly testing the short walk again."""
    assert SIZES == {"4x4": (4, 4, 1048577), "20x4": (20, 4, 262145), "4x8": (4, 8, 262145), "5x3": (5, 3, 524353)}
    assert {k: LW.table_walk(*v) for k, v in SIZES.items()} == {"4x4": (16385, 2, 2049), "20x4": (4097, 2, 2049), "4x8": (4097, 2, 2049),
                                                                "5x3": (8194, 3, 2732)}
    assert {k: LW.mix_walk(v[2]) for k, v in SIZES.items()} == {"4x4": (4097, 1024), "20x4": (1025, 1024), "4x8": (1025, 1024), "5x3": (2049, 1024)}
    assert {k: LW.reduce_rounds(v[1], LW.mix_walk(v[2])[1]) for k, v in SIZES.items()} == {"4x4": 1, "20x4": 1, "4x8": 2, "5x3": 1}
    for key, (states, rate_cats, sites) in SIZES.items():
        tiles, w, blocks = LW.table_walk(states, rate_cats, sites)
        assert w >= 2
        if key in LW.TABLE_SMALLEST:
            assert LW.table_walk(states, rate_cats, sites - 1)[1] == w - 1, "not the smallest size of this walk length"
        held, full, sites_last = LW.last_workgroup(states, rate_cats, sites, rule=LW.table_walk)
        assert held == 1 and held < full and sites_last == 1, key
        mix_tiles, mix_blocks = LW.mix_walk(sites)
        assert mix_tiles > mix_blocks == 1024, key
        if sites == 262145:  # workgroup 0 alone walks twice, its second tile holds 1 site
            assert mix_tiles == mix_blocks + 1 and sites - 256 * (mix_tiles - 1) == 1, key
        where = LW.written_sites(states, rate_cats, sites)
        assert where == [0, 63, 64, 64 * full - 1, sites - 1] and len(set(where)) == 5
    assert set(LW.TABLE_SMALLEST) == {"4x4", "20x4", "4x8"}


# ---- written counts ----------------------------------------------------------------------------------------------------
def _counts(dims, attrs, scaler):
    """the counts of scaler 0 or 1: zero but at long_walk_cases.written_sites. Per rate: (i + k) % 3 + i % 2 for scaler 0,
    ((i + k) // 2) % 2 for scaler 1 at the i-th written site, category k - the two added spread by at most 3; per site:
    1 + i % 3 and i % 2"""
    states, rate_cats, sites = dims
    per = rate_cats if attrs & api.RATE_SCALERS else 1
    out = np.zeros((sites, per), dtype=np.uint32)
    k = np.arange(per)
    for i, n in enumerate(LW.written_sites(*dims)):
        if per == 1:
            out[n, 0] = 1 + i % 3 if scaler == 0 else i % 2
        else:
            out[n] = (i + k) % 3 + i % 2 if scaler == 0 else ((i + k) // 2) % 2
    return out


def _write(b, size, attrs):
    for scaler in (0, 1):
        b.write_scaler(scaler, _counts(SIZES[size], ATTRS[attrs], scaler))


def test_the_written_counts_are_uneven_below_the_cap():
    """a condition on the inputs: at the written sites the per-rate counts of both ends added exceed the site's smallest by
    0, 1, 2 and 3 and by no more, those of the node's end alone (the tip edge) by 0, 1 and 2; the per-site counts are 1..3
    and 0..1"""
    for size in ("4x4", "20x4", "4x8"):
        dims = SIZES[size]
        where = LW.written_sites(*dims)
        c0, c1 = (_counts(dims, api.RATE_SCALERS, s).astype(np.int64) for s in (0, 1))
        assert not np.delete(c0, where, axis=0).any() and not np.delete(c1, where, axis=0).any()
        both = (c0 + c1)[where]
        assert set((both - both.min(1, keepdims=True)).ravel().tolist()) == {0, 1, 2, 3}, size
        assert set((c0[where] - c0[where].min(1, keepdims=True)).ravel().tolist()) == {0, 1, 2}, size
        assert ((both.max(1) - both.min(1)) > 0).all(), "a written site with even counts"
        p0, p1 = (_counts(dims, 0, s)[where, 0].tolist() for s in (0, 1))
        assert set(p0) == {1, 2, 3} and set(p1) == {0, 1}


# ---- the reference side, once per (size, attributes) and shared ---------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


def _ref_call_ancestral(b, edge):
    out = np.full((b.sites, b.states), SENTINEL)
    assert b.lib.pll_compute_node_ancestral(b.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(b.fi), api.dptr(out)), (b.lib.errno(), b.lib.errmsg())
    return out


@functools.lru_cache(maxsize=None)
def _ref_ancestral(size, attrs):
    """{edge: the expected table}: the reference's own call; under rate_scalers - with the written counts - the restatement
    on the reference's host arrays"""
    with _bed(_REF, size, attrs) as b:
        if attrs == "rate_scalers":
            _write(b, size, attrs)
            return {name: _frozen(restated(_REF, b.p, edge, b.fi)) for name, edge in ANCESTRAL_EDGES.items()}
        return {name: _frozen(_ref_call_ancestral(b, edge)) for name, edge in ANCESTRAL_EDGES.items()}


KEPT = ("cat_lnl", "posterior", "site_rates", "site_rates_scale", "weight_sums", "lnl")


@functools.lru_cache(maxsize=None)
def _ref_categories(size, attrs, written=False):
    """{edge: category_common.expected (what assert_outputs reads of it) + "lost": (weight_sums, lnl) with the last site's
    pattern weight at 0}"""
    dims = SIZES[size]
    out = {}
    with _bed(_REF, size, attrs) as b:
        if written:
            _write(b, size, attrs)
        rates = api.as_np(b.part.rates, dims[1], np.float64).copy()
        for name, edge in CATEGORY_EDGES.items():
            exp = CC.expected(_REF, b.p, edge, b.fi, None, rates)
            assert not exp["at_cap"].any(), "a written count at the cap: test_gpu_categories.py owns that case"
            out[name] = {k: _frozen(exp[k]) if isinstance(exp[k], np.ndarray) else exp[k] for k in KEPT}
        LW.drop_last_site(b)
        pw = LW.pattern_weights(dims[2], 0).astype(np.float64)
        for name, edge in CATEGORY_EDGES.items():
            out[name]["lost"] = ((pw[:, None] * out[name]["posterior"]).sum(0), float(b.lnl(edge)))
    return out


# ---- the condition on the inputs (no GPU) -----------------------------------------------------------------------------
def _same_rows(table, n, log_values):
    """how many of the rows 0..63 the comparison could not tell from row n: every entry within its tolerance"""
    head, row = table[:64], table[n][None, :]
    scale = np.maximum(1.0, np.abs(head)) if log_values else np.abs(head)
    return int((np.abs(head - row) <= RTOL * scale).all(1).sum())


def _differs(table, n, m, log_values):
    scale = np.maximum(1.0, np.abs(table[m])) if log_values else np.abs(table[m])
    return bool((np.abs(table[n] - table[m]) > RTOL * scale).any())


@pytest.mark.parametrize("size", list(SIZES))
def test_a_lost_table_tile_would_show(ref, size):
    """from the reference alone. The sums: with the last site's pattern weight at 0 instead of 50 (pll_set_pattern_weights)
    weight_sums[k] for every k and lnl move by at least ten tolerances on both edges. The per-site tables (ancestral states
    of the three edges, posterior, cat_lnl): a walk that took the first tile twice would store the row of site l at site
    64 + l. The expected row of site 64 differs from that of site 0 by more than the comparison's tolerance in at least one
    entry in every table, and so do the rows of most other lanes (printed: 44 to 64 of the 64), so such a walk cannot pass by
    coincidence; the last site's ancestral rows differ from site 0's as well.
    What the inputs do NOT give: a row unlike EVERY row of the sites 0..63. Four tips leave few distinct site patterns, so
    the row of site 64 is also the row of 2 (20 x 4) to 23 (4 x 8, tip edge) of the first 64 sites, at other lanes; and at
    4 x 8 the last site's posterior and cat_lnl rows are those of site 0 - there its weight of 50 in the sums holds it."""
    dims = SIZES[size]
    last = dims[2] - 1
    cat = _ref_categories(size, "plain")
    for name, exp in cat.items():
        ws, lnl = exp["lost"]
        m_ws = float(np.min(np.abs(exp["weight_sums"] - ws) / (RTOL * np.abs(exp["weight_sums"]))))
        m_lnl = abs(exp["lnl"] - lnl) / (RTOL * max(1.0, abs(exp["lnl"])))
        print(f"{size} {name}: a lost last tile moves weight_sums by at least {m_ws:.3g} tolerances ({m_ws * RTOL:.2e} relative), lnl by {m_lnl:.3g} ({m_lnl * RTOL:.2e})")
        assert m_ws >= FACTOR and m_lnl >= FACTOR, (size, name, m_ws, m_lnl)
    tables = [(f"ancestral {name}", t, False) for name, t in _ref_ancestral(size, "plain").items()]
    tables += [(f"posterior {name}", exp["posterior"], False) for name, exp in cat.items()]
    tables += [(f"cat_lnl {name}", exp["cat_lnl"], True) for name, exp in cat.items()]
    for what, table, log_values in tables:
        lanes = sum(_differs(table, 64 + lane, lane, log_values) for lane in range(64))
        print(f"{size} {what}: {lanes} of the 64 rows of the second tile differ from the first tile's; the row of site 64 is the row of "
              f"{_same_rows(table, 64, log_values)} of the sites 0..63, the last site's of {_same_rows(table, last, log_values)}")
        assert _differs(table, 64, 0, log_values), (size, what, "site 64 has the row of site 0")
        if what.startswith("ancestral"):
            assert _differs(table, last, 0, log_values), (size, what, "the last site has the row of site 0")


# ---- what every call is asked ----------------------------------------------------------------------------------------------
def _guarded(shape):
    """a buffer of `shape` prefilled with the sentinel, GUARD entries behind it -> (the whole, the view of the output)"""
    n = int(np.prod(shape))
    whole = np.full(n + GUARD, SENTINEL)
    return whole, whole[:n].reshape(shape)


def _untouched(whole, what):
    assert (whole[-GUARD:] == SENTINEL).all(), (what, "written past the output")


def _ancestral(b, edge, what):
    whole, table = _guarded((b.sites, b.states))
    assert b.lib.pll_compute_node_ancestral(b.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(b.fi), api.dptr(whole)), (what, b.lib.errno(), b.lib.errmsg())
    _untouched(whole, what)
    return table


def _categories(b, edge, what, want=CC.OUTPUTS):
    """category_common.call with a guard region behind every output"""
    n, r = b.sites, b.rate_cats
    shapes = {"cat_lnl": (n, r), "posterior": (n, r), "site_rates": (n,), "weight_sums": (r,), "lnl": (1,)}
    bufs = {k: _guarded(shapes[k]) for k in CC.OUTPUTS if k in want}
    ok = b.lib.pll_gpu_edge_category_posteriors(b.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(b.fi),
                                                *[api.dptr(bufs[k][0]) if k in bufs else None for k in CC.OUTPUTS])
    assert ok, (what, want, b.lib.errno(), b.lib.errmsg())
    out = {}
    for k, (whole, view) in bufs.items():
        _untouched(whole, (what, k))
        out[k] = view
    if "lnl" in out:
        out["lnl"] = float(out["lnl"][0])
    return out


def _same(x, y):
    return all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x) and set(x) == set(y)


def _check_ancestral(b, exp, what):
    worst = 0.0
    for name, edge in ANCESTRAL_EDGES.items():
        got = _ancestral(b, edge, (what, name))
        worst = max(worst, assert_table(got, exp[name], (what, name)))
        assert np.abs(got.sum(1) - 1.0).max() <= SUMTOL
        before = b.lib.pll_gpu_last_launch_count(b.p)
        again = _ancestral(b, edge, (what, name, "a second call"))
        assert b.lib.pll_gpu_last_launch_count(b.p) - before == 1, (what, name)
        assert again.tobytes() == got.tobytes(), (what, name, "a second call")
    print(f"ancestral {what}: worst {worst / RTOL:.4f} of the bound")


def _check_categories(b, exp, what, launches=True):
    worst = {}
    for name, edge in CATEGORY_EDGES.items():
        own = b.lnl(edge)  # (whatever the traversal held back is out after this)
        got = _categories(b, edge, (what, name))
        fig = CC.assert_outputs(got, exp[name], (what, name))
        assert IC.close(got["lnl"], own, RTOL), (what, name, "lnl against pll_compute_edge_loglikelihood", got["lnl"], own)
        for k, v in fig.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert _same(_categories(b, edge, (what, name)), got), (what, name, "a second call")
        alone = _categories(b, edge, (what, name), ("weight_sums",))
        assert alone["weight_sums"].tobytes() == got["weight_sums"].tobytes(), (what, name, "weight_sums alone")
        if launches:
            for want, count in WANT_SETS:
                part = _categories(b, edge, (what, name), want)
                assert b.lib.pll_gpu_last_launch_count(b.p) == count, (what, name, want)
                assert _same(part, {k: got[k] for k in part}), (what, name, want, "not the bytes of the full call")
    print(f"categories {what}: worst of the bound " + " ".join(f"{k} {v / (SUMTOL if k == 'row_sum' else RTOL):.4f}" for k, v in worst.items()))


CHERRY_SITES = 2304 * 32 + 1


@gpu
@pytest.mark.parametrize("attrs", ["plain", "pattern_tip"])
def test_tip_cherries_past_two_items_per_workgroup(amd_lib, ref, attrs):
    """what the 20 x 4 size found. Two tip x tip operations that form no group go to k_partials_lean as a level launch
    (launch_lean), whose workgroups take ipb = max(2, min(floor(items * ops / 1536), 32)) items of 32 sites each; a plain
    launch never advanced the entries behind a tip child's codes past the workgroup's second item, so with ipb >= 3 - two
    cherries from 2304 items, 73 697 sites, on - every later item was computed from the second item's codes. Here: 2305
    items, ipb = 3, the last item one site; both CLVs against the reference's, entry by entry within RTOL. Observed on an
    MI355X: 0.003 of the bound; before the fix 204 000 of the 262 145 rows of either CLV at 20 x 4 were another site's."""
    dims = (20, 4, CHERRY_SITES)
    items = -(-CHERRY_SITES // 32)
    assert max(2, min(items * 2 // 1536, 32)) == 3 and max(2, min((items - 2) * 2 // 1536, 32)) == 2
    w = _weights(4)
    with LW.TableBed(amd_lib, dims, ATTRS[attrs], w) as b, LW.TableBed(_REF, dims, ATTRS[attrs], w) as r:
        n = CHERRY_SITES * 4 * b.part.states_padded
        for clv in (4, 5):
            assert amd_lib.pll_gpu_sync_clv(b.p, clv)
            got, exp = api.as_np(b.part.clv[clv], n, np.float64), api.as_np(r.part.clv[clv], n, np.float64)
            assert np.isfinite(got).all() and (got[exp == 0] == 0).all(), clv
            worst = float(np.max(np.abs(got - exp)[exp != 0] / exp[exp != 0]))
            print(f"tip cherries {attrs} clv {clv}: worst {worst / RTOL:.4f} of the bound")
            assert worst <= RTOL, (attrs, clv, worst)


@gpu
@pytest.mark.parametrize("size,attrs", EVERY)
def test_ancestral_states(amd_lib, ref, size, attrs):
    """the inner edge both ways round and the tip edge (tip codes under pattern_tip: the CTIP kernels), the whole
    [sites][states] table against the reference's pll_compute_node_ancestral, rows summing to 1, nothing behind the table
    written, a second call the same bytes in one launch. Observed on an MI355X, worst fraction of the bound: 20 x 4 0.0034,
    every other size 0.0001, the same under both attributes; 0.2 to 1.0 s a case with the reference side."""
    exp = _ref_ancestral(size, attrs)
    with _bed(amd_lib, size, attrs) as b:
        _check_ancestral(b, exp, f"{size} {attrs}")


@gpu
@pytest.mark.parametrize("size", ANCESTRAL_WRITTEN)
def test_ancestral_states_written_counts(amd_lib, ref, size):
    """per-rate counts written by the caller at long_walk_cases.written_sites, in both libraries; expected:
    ancestral_common.restated on the reference's host arrays. Observed on an MI355X, worst fraction of the bound: 4 x 4
    0.0001, 20 x 4 0.0034; 1.8 and 1.6 s."""
    exp = _ref_ancestral(size, "rate_scalers")
    with _bed(amd_lib, size, "rate_scalers") as b:
        _write(b, size, "rate_scalers")
        _check_ancestral(b, exp, f"{size} rate_scalers, written counts")


@gpu
@pytest.mark.parametrize("size,attrs", EVERY)
def test_category_posteriors(amd_lib, ref, size, attrs):
    """the inner edge and the tip edge: all five outputs against category_common.expected, lnl also against the library's own
    pll_compute_edge_loglikelihood, the launch counts of every set of outputs, a second call the same bytes, weight_sums
    asked alone the bytes it has with everything. Observed on an MI355X, worst fraction of the bound, 4 x 4 / 20 x 4 / 4 x 8 /
    5 x 3, the same under both attributes: weight_sums 0.095 / 0.007 / 0.032 / 0.034, lnl 0.053 / 0.003 / 0.019 / 0.049,
    posterior 0.001 at 20 x 4 and below 0.0001 elsewhere, cat_lnl and site_rates 0.0002 and below, row sums 0.0002 of SUMTOL;
    0.4 to 1.4 s a case."""
    exp = _ref_categories(size, attrs)
    with _bed(amd_lib, size, attrs) as b:
        _check_categories(b, exp, f"{size} {attrs}")


@gpu
@pytest.mark.parametrize("size,attrs", CATEGORY_WRITTEN)
def test_category_posteriors_written_counts(amd_lib, ref, size, attrs):
    """per-site counts (plain) and per-rate counts (rate_scalers) written at long_walk_cases.written_sites in both
    libraries: a.count[nn], the rate_scaled table entries and cat_lnl's s * PLLGPU_LOG_THRESHOLD at the second tile. Observed
    on an MI355X, worst fraction of the bound, 4 x 4 / 4 x 8 under either kind of count: weight_sums 0.095 / 0.032, lnl 0.053 /
    0.019, posterior 0.0009, site_rates 0.0007 and below, cat_lnl below 0.0001; 1.2 and 0.6 s a case."""
    exp = _ref_categories(size, attrs, True)
    with _bed(amd_lib, size, attrs) as b:
        _write(b, size, attrs)
        _check_categories(b, exp, f"{size} {attrs}, written counts", launches=False)


@gpu
@pytest.mark.parametrize("size", EM_SIZES)
def test_em(amd_lib, ref, size):
    """pll_gpu_category_weights_em, 2 steps from the partition's non-uniform weights on the inner edge: every weight row and
    every lnl against category_common.expected re-evaluated under that row (test_gpu_categories.test_em's oracle), row 0's
    lnl the posteriors call's bit for bit. At 4 x 8 stage C's second round writes weight_sums[7] and lnl, and both rounds feed
    the next row. Observed on an MI355X, worst fraction of the bound, 4 x 8 / 4 x 4: weight rows 0.030 / 0.108, lnl 0.030 /
    0.105; 0.5 and 1.0 s."""
    rate_cats, sites = SIZES[size][1:]
    with _bed(amd_lib, size, "plain") as b, _bed(_REF, size, "plain") as r:
        start = b.weights.copy()
        assert len(set(start.tolist())) > 1
        b.lnl(INNER)  # (whatever the traversal held back is out after this: the call's own launches are counted below)
        rows, lnl = CC.em(amd_lib, b.p, INNER, b.fi, start, EM_STEPS)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 1 + 2 * (EM_STEPS + 1)
        assert np.array_equal(rows[0], start)
        rates = api.as_np(r.part.rates, rate_cats, np.float64).copy()
        worst_row = worst_lnl = 0.0
        for i in range(EM_STEPS + 1):
            exp = CC.expected(_REF, r.p, INNER, r.fi, rows[i], rates)
            worst_lnl = max(worst_lnl, IC.worst(lnl[i], exp["lnl"]))
            assert IC.close(lnl[i], exp["lnl"], RTOL), (size, i, lnl[i], exp["lnl"])
            if i < EM_STEPS:
                nxt = exp["weight_sums"] / exp["weight_sums"].sum()
                worst_row = max(worst_row, CC.worst_rel(rows[i + 1], nxt))
                assert CC.worst_rel(rows[i + 1], nxt) <= RTOL, (size, i, CC.worst_rel(rows[i + 1], nxt))
            assert abs(rows[i].sum() - 1.0) <= SUMTOL, (size, i, rows[i].sum())
        print(f"EM {size}: worst of the bound rows {worst_row / RTOL:.4f} lnl {worst_lnl / RTOL:.4f}")
        assert (np.diff(lnl) >= -RTOL * np.abs(lnl[:-1])).all(), (size, "the log-likelihood fell", lnl)
        assert lnl[0] == _categories(b, INNER, (size, "lnl"), ("lnl",))["lnl"]
        again = CC.em(amd_lib, b.p, INNER, b.fi, start, EM_STEPS)
        assert again[0].tobytes() == rows.tobytes() and again[1].tobytes() == lnl.tobytes(), (size, "a second call")
