"""GPU: pll_gpu_pairwise_distances against the reference, live.

The expectation of a pair (x, y), x earlier in the list, is the reference's own per-pair path on a plain partition of the same
data: pll_update_sumtable(x, y) on the two tips, then pll_compute_likelihood_derivatives (distance_cases.Tips). PATTERN_TIP is
exercised on this library only - the reference refuses tip-tip under it - against that same expectation; RATE_SCALERS gives
the plain bits (tips carry no scaler). Inputs: insertion_cases.alignment at 15 % mutation with 10 % '-' and 10 % partial
ambiguity characters.

Tolerance of every d_f and dd_f: gradient_cases.close, |d| <= 1e-10 |exp| + 4e-15 W, W = the sum of the pattern weights.
p_distance is compared with pllamd/distances.py exactly. The iteration (t_start 0.1, bounds [1e-6, 100], tolerance 1e-8 W, at
most 32 evaluations) is compared with newton.host_newton driven by the reference's derivatives: the same status, a trace
length within 1, and for a CONVERGED pair the reference's own |d_f| at the returned distance <= 2 tolerance and
|t - t_ref| <= 6 tolerance / dd_f_ref(t_ref) (both points have a slope of at most 2 tolerance; by the mean-value theorem the gap
is the slope difference over the curvature, and the factor lets the curvature halve in between).

One workgroup serves one pair, so the "pair block" of the launch is one pair: tip counts 2 and 3 are one more than it in
each direction; 9 tips are 36 workgroups. Site counts 1, 63, 64, 65, 130 and 1000: below, at and above a wave's stride, a
tail that is no multiple of the four sites a thread reads at once, and 250 quads of four sites: almost every one of the 256
threads takes one step of the site loop, none a second (tests/test_gpu_distance_tables.py runs 1029 and 2051 sites, where
threads take a second step, and the table sizes these cases leave out).

Observed on an MI355X: the worst deviation of one evaluation is 0.05 of the bound (61 x 4 at t = 1.2), below 0.04 elsewhere."""
import functools

import numpy as np
import pytest

import distance_cases as DC
import gradient_cases as GC
from pllamd import api, distances, driver

pytestmark = pytest.mark.gpu

SHAPES = {"4x4": (4, 4), "4x2": (4, 2), "5x3": (5, 3), "20x4": (20, 4), "61x4": (61, 4)}
ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP, "rate_scalers": api.RATE_SCALERS}
_REF = None


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    global _REF
    _REF = ref_lib


def _weights(sites):
    w = np.arange(sites, dtype=np.uint32) % 4
    w[min(5, sites - 1)] = 100000
    return w


def _features(rate_cats, sites):
    return {
        "none": {},
        "weights": dict(pattern_weights=tuple(int(v) for v in _weights(sites))),
        "two_matrices": dict(rate_matrices=2, params_indices=tuple([0, 1, 0, 1][:rate_cats])),
        "rate_weights": dict(rate_weights=tuple(np.arange(1, rate_cats + 1) / np.arange(1, rate_cats + 1).sum())),
    }


# (shape, attrs, tips, sites, feature)
CASES = [(s, a, 9, 130, "none") for s in SHAPES for a in ATTRS]
CASES += [(s, "plain", n, 130, "none") for s in ("4x4", "20x4") for n in (2, 3)]
CASES += [(s, "plain", 4, n, "none") for s in ("4x4", "20x4") for n in (1, 63, 64, 65, 1000)]
CASES += [(s, "plain", 5, 130, f) for s in ("4x4", "20x4") for f in ("weights", "two_matrices", "rate_weights")]


@functools.lru_cache(maxsize=None)
def _data(shape, tips, sites):
    return DC.sequences(SHAPES[shape][0], tips, sites)


def _bed(lib, shape, attrs, tips, sites, feature, seqs=None):
    states, rate_cats = SHAPES[shape]
    data_seqs, cmap, exch, freqs = _data(shape, tips, sites)
    return DC.Tips(lib, states, rate_cats, seqs or data_seqs, cmap, exch, freqs, attrs=ATTRS[attrs], **_features(rate_cats, sites)[feature])


@functools.lru_cache(maxsize=None)
def _reference(shape, tips, sites, feature):
    """[pairs, 3, 2]: (d_f, dd_f) of every pair at T_POINTS through the reference's per-pair path; computed once, shared"""
    with _bed(_REF, shape, "plain", tips, sites, feature) as b:
        exp = np.array([b.pair_derivatives(x, y) for x, y in DC.pairs(tips)])
    exp.setflags(write=False)
    return exp


def _restated_p(shape, tips, sites, weights):
    states = SHAPES[shape][0]
    seqs, cmap, _, _ = _data(shape, tips, sites)
    codes, masks, w = DC.restated(seqs, cmap, states, weights)
    return {(x, y): distances.p_distance(distances.code_pair_counts(codes[x], codes[y], w, len(masks)), masks, states) for x, y in DC.pairs(tips)}


@pytest.mark.parametrize("shape,attrs,tips,sites,feature", CASES)
def test_one_evaluation_of_every_pair(amd_lib, shape, attrs, tips, sites, feature):
    exp = _reference(shape, tips, sites, feature)
    pairs = DC.pairs(tips)
    with _bed(amd_lib, shape, attrs, tips, sites, feature) as b:
        W = b.weight_sum
        p_exp = _restated_p(shape, tips, sites, b.weights)
        for ti, t in enumerate(DC.T_POINTS):
            out = b.distances(range(tips), driver.newton_options(t, 1e-6, 100.0, 1e-8 * W, 1))
            assert b.launches() == DC.launches_by_rule(tips) == 2
            got = np.array([[out["d_f"][x, y], out["dd_f"][x, y]] for x, y in pairs])
            print(f"{shape} {attrs} {tips} tips {sites} sites {feature} t {t}: worst {GC.worst(got, exp[:, ti], W):.3f} of the bound")
            assert GC.close(got, exp[:, ti], W), GC.worst(got, exp[:, ti], W)
            for x, y in pairs:
                assert out["distance"][x, y] == t and out["iterations"][x, y] == 1
                assert out["p_distance"][x, y] == p_exp[x, y]
            for a in out.values():
                assert (a == a.T).all() and (np.diag(a) == 0).all()


def test_the_inputs_exercise_the_counts():
    """conditions on the inputs of test_one_evaluation_of_every_pair, from the data: a pair with an all-states code on one side
    only, a pair with two disjoint partial-ambiguity sets, a weight of 0 - and the restated p-distance is the per-site loop's"""
    for shape in ("4x4", "20x4", "61x4"):
        states = SHAPES[shape][0]
        seqs, cmap, _, _ = _data(shape, 9, 130)
        full = (1 << states) - 1
        one_sided = disjoint_partials = False
        for x, y in DC.pairs(9):
            for ca, cb in zip(seqs[x], seqs[y]):
                ma, mb = int(cmap[ca]), int(cmap[cb])
                one_sided |= (ma == full) != (mb == full)
                disjoint_partials |= bin(ma).count("1") > 1 and bin(mb).count("1") > 1 and full not in (ma, mb) and ma & mb == 0
        assert one_sided and disjoint_partials, shape
    w = _weights(130)
    assert (w == 0).any() and (w == 100000).sum() == 1
    seqs, cmap, _, _ = _data("4x4", 5, 130)
    p = _restated_p("4x4", 5, 130, w)
    for x, y in DC.pairs(5):
        differ, compared = DC.p_distance_by_sites(seqs[x], seqs[y], cmap, 4, w)
        assert p[x, y] == differ / compared


ITERATED = {"4x4": 130, "20x4": 65, "61x4": 65}


def _iteration_sequences(shape):
    """six related tips, tip 6 = tip 0 again (identical sequences), tip 7 = independent random states"""
    states, sites = SHAPES[shape][0], ITERATED[shape]
    seqs = list(_data(shape, 6, sites)[0])
    return seqs + [seqs[0], DC.unrelated(states, sites, 99)]


@pytest.mark.parametrize("shape", list(ITERATED))
def test_the_iteration(amd_lib, shape):
    sites = ITERATED[shape]
    seqs = _iteration_sequences(shape)
    tips = list(range(len(seqs))) + [2]  # (tip 2 twice: a tip against itself)
    tol = 1e-8 * sites
    opt = (0.1, 1e-6, 100.0, tol, 32)
    with _bed(amd_lib, shape, "plain", 6, sites, "none", seqs=seqs) as b, _bed(_REF, shape, "plain", 6, sites, "none", seqs=seqs) as r:
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
                assert t == 1e-6 and d_at > 0
            elif status == api.NEWTON_AT_MAX:
                assert t == 100.0 and d_at < 0
            # the returned derivatives are those of one evaluation at the returned distance: bit for bit
            one = b.distances([x, y], driver.newton_options(t, 1e-6, 100.0, tol, 1))
            assert one["distance"][0, 1] == t
            assert one["d_f"][0, 1] == out["d_f"][i, j] and one["dd_f"][0, 1] == out["dd_f"][i, j]
        assert out["status"][0, 6] == out["status"][2, 8] == api.NEWTON_AT_MIN  # identical sequences, a tip against itself
        assert out["status"][0, 7] in (api.NEWTON_CONVERGED, api.NEWTON_AT_MAX)  # the unrelated pair
        assert api.NEWTON_CONVERGED in seen


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_a_pair_depends_on_nothing_but_itself(amd_lib, shape, monkeypatch):
    """the full list, a sub-list, a permuted list, a second call and a list cut into several launches give the same bits for
    the same ordered pair; the launch count is the cutting rule's"""
    tips, sites = 9, 130
    opt = driver.newton_options(0.1, 1e-6, 100.0, 1e-8 * sites, 32)

    def run(b, order):
        out = b.distances(order, opt)
        for a in out.values():
            assert (a == a.T).all() and (np.diag(a) == 0).all()
        return {(order[i], order[j]): tuple(out[name][i, j] for name in driver.DISTANCE_OUTPUTS) for i, j in DC.pairs(len(order))}

    with _bed(amd_lib, shape, "plain", tips, sites, "none") as b:
        full = run(b, list(range(tips)))
        assert b.launches() == DC.launches_by_rule(tips) == 2
        assert run(b, list(range(tips))) == full
        sub = run(b, [1, 4, 6, 7])
        assert all(full[k] == v for k, v in sub.items())
        perm = run(b, [3, 8, 0, 5, 1])
        assert {k for k in perm if k[0] < k[1]} and all(full[k] == v for k, v in perm.items() if k[0] < k[1])
    monkeypatch.setenv("PLL_AMD_DISTANCE_PAIRS", str(2 * tips))  # two rows of the pair matrix per launch
    with _bed(amd_lib, shape, "plain", tips, sites, "none") as b:
        assert run(b, list(range(tips))) == full
        assert b.launches() == DC.launches_by_rule(tips, 2 * tips) == 5


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_rate_scalers_give_the_plain_bits(amd_lib, shape):
    """tips carry no scaler: a PLL_ATTRIB_RATE_SCALERS partition returns what the plain one returns, bit for bit"""
    opt = driver.newton_options(0.1, 1e-6, 100.0, 1e-8 * 130, 32)
    with _bed(amd_lib, shape, "plain", 9, 130, "none") as b, _bed(amd_lib, shape, "rate_scalers", 9, 130, "none") as s:
        plain, scaled = b.distances(range(9), opt), s.distances(range(9), opt)
    for name in driver.DISTANCE_OUTPUTS:
        assert plain[name].tobytes() == scaled[name].tobytes(), name


def test_refusals_and_shortcuts_with_a_device(amd_lib):
    """a dense tip, invariant sites and an over-long code table are refused with the outputs untouched; 0 and 1 tips succeed
    without a launch"""
    sentinel = 12345.5
    opt = driver.newton_options(0.1, 1e-6, 100.0, 1e-6, 32)

    def refused(b, code, tips=(0, 1, 2)):
        with pytest.raises(RuntimeError) as err:
            b.distances(tips, opt, fill=sentinel)
        assert amd_lib.errno() == code, (amd_lib.errno(), amd_lib.errmsg())
        assert all((a == np.array(sentinel).astype(a.dtype)).all() for a in err.value.outputs.values())

    states, rate_cats = SHAPES["20x4"]
    seqs, cmap, exch, freqs = _data("20x4", 4, 65)
    with DC.Tips(amd_lib, states, rate_cats, seqs, cmap, exch, freqs, dense=(1,)) as b:
        refused(b, api.ERROR_PARAM_INVALID)
        b.distances((0, 2, 3), opt)  # the others are served
    with DC.Tips(amd_lib, states, rate_cats, seqs, cmap, exch, freqs, prop_invar=0.2) as b:
        refused(b, api.ERROR_GPU_UNSUPPORTED)
    wide = np.zeros(256, dtype=np.uint64)
    wide[1:201] = np.arange(1, 201, dtype=np.uint64)
    seq = bytes(range(1, 201))
    for attrs in (0, api.PATTERN_TIP):
        with DC.Tips(amd_lib, states, rate_cats, [seq, seq[::-1], seq], wide, exch, freqs, attrs=attrs) as b:
            refused(b, api.ERROR_GPU_UNSUPPORTED)
    with DC.Tips(amd_lib, states, rate_cats, seqs, cmap, exch, freqs) as b:
        b.distances((0, 1), opt)
        assert b.launches() == 2
        assert b.distances((), opt)["distance"].shape == (0, 0)
        one = b.distances((3,), opt, fill=sentinel)
        assert b.launches() == 0 and all(a.shape == (1, 1) and a[0, 0] == 0 for a in one.values())
