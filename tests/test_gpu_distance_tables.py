"""GPU: pll_gpu_pairwise_distances at the edges of its count tables, of the site loop, of the 32-bit counts and of the iteration.

The expectation is the reference's per-pair path (distance_cases.Tips: pll_update_sumtable on the two tips, then
pll_compute_likelihood_derivatives), as in test_gpu_distances.py, with that file's bounds: every d_f and dd_f within
gradient_cases.close, |d| <= 1e-10 |exp| + 4e-15 W; p_distance exact; the iteration (t_start 0.1, bounds [1e-6, 100], tolerance
1e-8 W, at most 32 evaluations) by status, trace length, slope and gap. One input cannot go through the reference: it indexes
its character map with a signed char, so the 128-code case, which uses byte 128, is compared with pllamd/distances.py
(distance_cases.Restated) under the same bounds; the 127-code case, against the reference, anchors it
(tests/test_distances_host.py holds the restatement against the reference on these inputs).

The tables (distance_cases.TABLE_CASES; copies_by_rule restates how many a workgroup keeps): 5 x 3 with 5 and 8 codes - 256
tables, one per thread, and 128; 20 x 4 with 68, 96, 127 and 128 codes - one table for all 256 threads, the first table above
the 36 KB budget, the first launch above 64 KB of dynamic LDS (67 076 B) and PLLGPU_DISTANCE_MAX_CODES itself; 61 x 49 with
127 codes - 160 164 of the 161 792 B a launch may ask for. 61 x 50 and 129 codes are refused. The inputs come from
distance_cases.generated: exactly C codes, every tip running through all of them, the corner cells of the table counted.

The site loop: 1029 sites are 257 quads (one thread takes a second step; a tail of 1), 2051 sites two full steps and a tail
of 3. The counts: weights that add up to 2^32 - 1 with one cell above 2^31, met from two private tables.

How a run ends: max_iters 1, 2, 3 against newton.Bracket replayed on the device's own derivatives (the point of evaluation k
is exact) and against the reference-driven recipe (NEWTON_MAXITER where it says so); t_start outside the bounds;
t_min == t_max; a tip of nothing but '-'.

Observed on an MI355X (every case prints its figure): the worst deviation of an evaluation is 0.10 of the bound, 4 x 4 with
t_start clamped to t_min = 0.01 (0.08 at t_max = 100, 0.10 against the tip of gaps, where the expectation itself is rounding
noise of 2e-14); at most 0.004 in the table, site-loop and weight cases (61 x 49 at t = 0.05), 0.001 and less elsewhere."""
import functools

import numpy as np
import pytest

import distance_cases as DC
import gradient_cases as GC
from pllamd import api, driver, newton

pytestmark = pytest.mark.gpu

ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP}
OPT = (0.1, 1e-6, 100.0)
_REF = None


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    global _REF
    _REF = ref_lib


def _one_evaluation(b, exp, p_exp, tips, what):
    """test_gpu_distances.test_one_evaluation_of_every_pair on an open Tips: exp [pairs, T_POINTS, 2], p_exp {pair: p}"""
    W, pairs = b.weight_sum, DC.pairs(tips)
    for ti, t in enumerate(DC.T_POINTS):
        out = b.distances(range(tips), driver.newton_options(t, 1e-6, 100.0, 1e-8 * W, 1))
        assert b.launches() == DC.launches_by_rule(tips) == 2
        got = np.array([[out["d_f"][x, y], out["dd_f"][x, y]] for x, y in pairs])
        print(f"{what} t {t}: worst {GC.worst(got, exp[:, ti], W):.3f} of the bound")
        assert GC.close(got, exp[:, ti], W), GC.worst(got, exp[:, ti], W)
        for x, y in pairs:
            assert out["distance"][x, y] == t and out["iterations"][x, y] == 1
            assert out["p_distance"][x, y] == p_exp[x, y]
        for a in out.values():
            assert (a == a.T).all() and (np.diag(a) == 0).all()


def _iteration(b, r, tips, opt):
    """test_gpu_distances.test_the_iteration's assertions on every pair of the list `tips`: b the library under test, r the
    expectation (a Tips of the reference, or a Restated); the statuses seen"""
    t_start, t_min, t_max, tol, cap = opt
    out = b.distances(tips, driver.newton_options(*opt))
    seen = set()
    for i, j in DC.pairs(len(tips)):
        x, y = tips[i], tips[j]
        t_ref, status_ref, trace = r.pair_newton(x, y, *opt)
        t, status, its = out["distance"][i, j], out["status"][i, j], out["iterations"][i, j]
        seen.add(int(status))
        assert status == status_ref, (i, j, status, status_ref, t, t_ref)
        assert abs(int(its) - len(trace)) <= 1, (i, j, its, len(trace))
        d_at, dd_at = r.derivatives(None, r.sumtable, t)  # (the table of pair_newton's pair)
        if status == api.NEWTON_CONVERGED:
            assert abs(d_at) <= 2 * tol, (i, j, d_at, tol)
            assert abs(t - t_ref) <= 6 * tol / trace[-1][2], (i, j, t, t_ref, trace[-1][2])
        elif status == api.NEWTON_AT_MIN:
            assert t == t_min and d_at > 0
        elif status == api.NEWTON_AT_MAX:
            assert t == t_max and d_at < 0
        # the returned derivatives are those of one evaluation at the returned distance: bit for bit
        one = b.distances([x, y], driver.newton_options(t, t_min, t_max, tol, 1))
        assert one["distance"][0, 1] == t
        assert one["d_f"][0, 1] == out["d_f"][i, j] and one["dd_f"][0, 1] == out["dd_f"][i, j]
    return seen


# ---- the count tables ---------------------------------------------------------------------------------------------------
TABLE_RUNS = [(s, c, n, "plain") for s, c, n in DC.TABLE_CASES] + [("20x4", c, 300, "pattern_tip") for c in (127, 128)]


@functools.lru_cache(maxsize=None)
def _table_reference(shape, ncodes, sites):
    """[pairs, 3, 2] through the reference's per-pair path (computed once, shared); None for an input it cannot take"""
    if ncodes > 127:
        return None
    states, rate_cats = DC.TABLE_SHAPES[shape]
    with DC.Tips(_REF, states, rate_cats, *DC.table_case(shape, ncodes, sites)) as b:
        exp = np.array([b.pair_derivatives(x, y) for x, y in DC.pairs(b.tips)])
    exp.setflags(write=False)
    return exp


@pytest.mark.parametrize("shape,ncodes,sites,attrs", TABLE_RUNS)
def test_every_pair_at_the_edges_of_the_count_table(amd_lib, shape, ncodes, sites, attrs):
    states, rate_cats = DC.TABLE_SHAPES[shape]
    seqs, cmap, exch, freqs = DC.table_case(shape, ncodes, sites)
    tips = len(seqs)
    assert DC.copies_by_rule(states, rate_cats, ncodes) == {5: 256, 8: 128}.get(ncodes, 1)
    opt = OPT + (1e-8 * sites, 32)
    with DC.Tips(amd_lib, states, rate_cats, seqs, cmap, exch, freqs, attrs=ATTRS[attrs]) as b:
        restated = DC.Restated(b, seqs, cmap)
        exp = _table_reference(shape, ncodes, sites)
        if exp is None:
            exp = np.array([restated.pair_derivatives(x, y) for x, y in DC.pairs(tips)])
        p_exp = {(x, y): restated.p_distance(x, y) for x, y in DC.pairs(tips)}
        _one_evaluation(b, exp, p_exp, tips, f"{shape} {ncodes} codes {attrs}")
        if ncodes > 127:
            _iteration(b, restated, list(range(tips)), opt)
        else:
            with DC.Tips(_REF, states, rate_cats, seqs, cmap, exch, freqs) as r:
                _iteration(b, r, list(range(tips)), opt)


@pytest.mark.parametrize("shape,ncodes,sites", DC.TABLE_REFUSED)
def test_a_table_beyond_the_limit_is_refused_with_a_device(amd_lib, shape, ncodes, sites):
    """ERROR_GPU_UNSUPPORTED, the outputs untouched, nothing launched"""
    states, rate_cats = DC.TABLE_SHAPES[shape]
    sentinel = 12345.5
    for attrs in ATTRS.values():
        with DC.Tips(amd_lib, states, rate_cats, *DC.table_case(shape, ncodes, sites), attrs=attrs) as b:
            with pytest.raises(RuntimeError) as err:
                b.distances(range(b.tips), driver.newton_options(*OPT, 1e-6, 32), fill=sentinel)
            assert amd_lib.errno() == api.ERROR_GPU_UNSUPPORTED, (amd_lib.errno(), amd_lib.errmsg())
            assert all((a == np.array(sentinel).astype(a.dtype)).all() for a in err.value.outputs.values())
            assert b.launches() == 0


# ---- the four-sites-per-thread loop and the 32-bit counts ------------------------------------------------------------------
SHAPES = {"4x4": (4, 4), "20x4": (20, 4)}


@pytest.mark.parametrize("sites", [1029, 2051])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_thread_takes_a_second_step_of_the_site_loop(amd_lib, shape, sites):
    """1029 sites: 257 quads and a tail of 1; 2051 sites: 512 quads and a tail of 3"""
    states, rate_cats = SHAPES[shape]
    seqs, cmap, exch, freqs = DC.sequences(states, 4, sites)
    with DC.Tips(_REF, states, rate_cats, seqs, cmap, exch, freqs) as r:
        exp = np.array([r.pair_derivatives(x, y) for x, y in DC.pairs(4)])
    with DC.Tips(amd_lib, states, rate_cats, seqs, cmap, exch, freqs) as b:
        restated = DC.Restated(b, seqs, cmap)
        p_exp = {(x, y): restated.p_distance(x, y) for x, y in DC.pairs(4)}
        for (x, y), p in p_exp.items():
            differ, compared = DC.p_distance_by_sites(seqs[x], seqs[y], cmap, states, b.weights)
            assert p == differ / compared
        _one_evaluation(b, exp, p_exp, 4, f"{shape} {sites} sites")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_count_above_two_to_the_31(amd_lib, shape):
    """weights adding up to 2^32 - 1, one cell of the pair (0, 1) above 2^31 and met from two private tables
    (test_distances_host.py holds the conditions): d_f and dd_f with W = 2^32 - 1, p_distance exactly the per-site loop's"""
    states, rate_cats = SHAPES[shape]
    seqs, cmap, exch, freqs, weights = DC.weights_case(states)
    with DC.Tips(_REF, states, rate_cats, seqs, cmap, exch, freqs, pattern_weights=weights) as r:
        exp = np.array([r.pair_derivatives(x, y) for x, y in DC.pairs(4)])
    with DC.Tips(amd_lib, states, rate_cats, seqs, cmap, exch, freqs, pattern_weights=weights) as b:
        assert b.weight_sum == (1 << 32) - 1
        p_exp = {}
        for x, y in DC.pairs(4):
            differ, compared = DC.p_distance_by_sites(seqs[x], seqs[y], cmap, states, weights)
            p_exp[x, y] = differ / compared
        _one_evaluation(b, exp, p_exp, 4, f"{shape} weights up to 2^31")


# ---- how a run ends ----------------------------------------------------------------------------------------------------
END_SITES = 130


@functools.lru_cache(maxsize=None)
def _end_sequences(shape):
    """five related tips, tip 5 = tip 0 again, tip 6 = independent random states, tip 7 = nothing but '-'"""
    states = SHAPES[shape][0]
    seqs, cmap, exch, freqs = DC.sequences(states, 5, END_SITES)
    assert int(cmap[ord("-")]) == (1 << states) - 1
    return tuple(seqs) + (seqs[0], DC.unrelated(states, END_SITES, 99), b"-" * END_SITES), cmap, exch, freqs


def _end_beds(lib, shape):
    seqs, cmap, exch, freqs = _end_sequences(shape)
    return DC.Tips(lib, *SHAPES[shape], list(seqs), cmap, exch, freqs)


GAPS = 7


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_capped_run_ends_at_the_last_point_it_evaluated(amd_lib, shape):
    tol = 1e-8 * END_SITES
    with _end_beds(amd_lib, shape) as b, _end_beds(_REF, shape) as r:
        tips = list(range(b.tips))
        outs = {k: b.distances(tips, driver.newton_options(*OPT, tol, k)) for k in (1, 2, 3)}
        capped = 0
        for x, y in DC.pairs(len(tips)):
            br, t, ended = newton.Bracket(OPT[1], OPT[2]), OPT[0], None
            for k in (1, 2, 3):
                got = {name: outs[k][name][x, y] for name in driver.DISTANCE_OUTPUTS}
                if ended is not None:  # the run was over before the cap: the same answer under every larger cap
                    assert got == ended, (x, y, k)
                    continue
                # evaluation k is where the recipe, replayed on the device's own derivatives, puts it - exactly
                assert got["distance"] == t and got["iterations"] == k, (x, y, k, got, t)
                status, nxt = br.step(t, got["d_f"], got["dd_f"], tol)
                if status is None:
                    assert got["status"] == api.NEWTON_MAXITER, (x, y, k, got)
                    t = nxt
                else:
                    assert got["status"] == status, (x, y, k, got, status)
                    ended = got
                _, status_ref, trace = r.pair_newton(x, y, *OPT, tol, k)
                if status_ref == api.NEWTON_MAXITER:
                    capped += 1
                    assert got["status"] == api.NEWTON_MAXITER and got["iterations"] == k == len(trace), (x, y, k, got)
                    one = b.distances([x, y], driver.newton_options(got["distance"], OPT[1], OPT[2], tol, 1))
                    assert one["distance"][0, 1] == got["distance"]
                    assert one["d_f"][0, 1] == got["d_f"] and one["dd_f"][0, 1] == got["dd_f"]
        assert capped >= 3 * 10  # (the ten pairs of the five related tips need more than three evaluations)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_start_outside_the_bounds_and_bounds_that_meet(amd_lib, shape):
    tol = 1e-8 * END_SITES
    with _end_beds(amd_lib, shape) as b, _end_beds(_REF, shape) as r:
        tips = list(range(b.tips))
        pairs = DC.pairs(len(tips))
        # t_start beyond a bound, one evaluation: the bound is where it is made
        for t_start, t_min, t_max, bound in ((200.0, 1e-6, 100.0, 100.0), (0.0, 0.01, 100.0, 0.01), (1e-9, 0.01, 100.0, 0.01)):
            out = b.distances(tips, driver.newton_options(t_start, t_min, t_max, tol, 1))
            at = b.distances(tips, driver.newton_options(bound, t_min, t_max, tol, 1))
            assert all(out["distance"][p] == bound and out["iterations"][p] == 1 for p in pairs)
            for name in driver.DISTANCE_OUTPUTS:
                assert out[name].tobytes() == at[name].tobytes(), name
            exp = np.array([r.pair_derivatives(x, y, (bound,))[0] for x, y in pairs])
            got = np.array([[out["d_f"][p], out["dd_f"][p]] for p in pairs])
            print(f"{shape} start {t_start} in [{t_min}, {t_max}]: worst {GC.worst(got, exp, END_SITES):.3f} of the bound")
            assert GC.close(got, exp, END_SITES), GC.worst(got, exp, END_SITES)
        # t_min == t_max: that point, and what the recipe says of it
        seen = set()
        for point in (0.3, 1e-6):
            opt = (0.1, point, point, tol, 32)
            out = b.distances(tips, driver.newton_options(*opt))
            for x, y in pairs:
                t_ref, status_ref, trace = r.pair_newton(x, y, *opt)
                assert t_ref == point and len(trace) == 1
                assert out["distance"][x, y] == point and out["iterations"][x, y] == 1
                assert out["status"][x, y] == status_ref, (x, y, point, out["status"][x, y], status_ref, out["d_f"][x, y], trace)
                seen.add(int(status_ref))
        assert seen == {api.NEWTON_AT_MIN, api.NEWTON_AT_MAX, api.NEWTON_CONVERGED}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_tip_of_nothing_but_gaps(amd_lib, shape):
    """nothing comparable: p_distance 0.0; the function is flat, so d_f and dd_f are 0 within the bound and the run is
    CONVERGED after the one evaluation at t_start"""
    tol = 1e-8 * END_SITES
    with _end_beds(amd_lib, shape) as b, _end_beds(_REF, shape) as r:
        tips = list(range(b.tips))
        out = b.distances(tips, driver.newton_options(*OPT, tol, 32))
        with_gaps = [(x, GAPS) for x in range(GAPS)]
        exp = np.array([r.pair_derivatives(x, y, (OPT[0],))[0] for x, y in with_gaps])
        got = np.array([[out["d_f"][p], out["dd_f"][p]] for p in with_gaps])
        print(f"{shape} against a tip of gaps: worst {GC.worst(got, exp, END_SITES):.3f} of the bound")
        assert GC.close(got, exp, END_SITES), GC.worst(got, exp, END_SITES)
        for p in with_gaps:
            assert out["p_distance"][p] == 0.0 and out["status"][p] == api.NEWTON_CONVERGED
            assert out["iterations"][p] == 1 and out["distance"][p] == OPT[0]
            assert r.pair_newton(*p, *OPT, tol, 32)[1] == api.NEWTON_CONVERGED
        # and the other pairs are not disturbed by it: a list without the tip gives their bits
        rest = b.distances(tips[:GAPS], driver.newton_options(*OPT, tol, 32))
        for name in driver.DISTANCE_OUTPUTS:
            assert out[name][:GAPS, :GAPS].tobytes() == rest[name].tobytes(), name
