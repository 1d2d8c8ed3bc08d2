"""GPU: pll_gpu_edge_category_posteriors and pll_gpu_category_weights_em against the reference build.

The expected values come from the reference alone (category_common.py): its per-site log-likelihoods under the unit
weight rows e_k and under the real weights, both with pattern weights 1, give posterior, cat_lnl, weight_sums and site
rates; its edge log-likelihood gives lnl. Tolerances are the project's: RTOL (1e-10) on log values with max(1, |v|), RTOL
relative on probabilities and sums, exact zeros, rows of posterior summing to 1 within SUMTOL (1e-12).

Written counts at the cap and above. Where the count of a (site, category) exceeds the site's smallest by 4 or more, the
reference mixes l 2^-1024, a SUBNORMAL number for every l < 4: its logarithm carries as few bits as l 2^-1024 has left
(17 to 40 here), not 53 - it is off by up to 3.5e-5 of its value (printed below). For those pairs - and only those -
cat_lnl is checked against the reference's value of the same edge with both scale buffers written as zeros, plus
-256 ln2 s from the integers written: the same quantity at full precision, nothing weaker; for every other pair the two
expectations are asserted to agree. The posterior of such a pair is about 2^-1024 and is compared as it stands."""
import numpy as np
import pytest

import category_common as CC
import insertion_cases as IC
import scaler_cases as SC
from ancestral_common import SUMTOL
from compare import RTOL
from pllamd import api, driver, workload as W
from test_gpu_ancestral import _deep_records, _tree_pair

pytestmark = pytest.mark.gpu

WANT_SETS = ((("cat_lnl",), 1), (("posterior",), 2), (("site_rates",), 2), (("posterior", "site_rates", "cat_lnl"), 2),
             (("weight_sums",), 3), (("lnl",), 3), (CC.OUTPUTS, 3))


def _prepare(case):
    """the tests' weights into the case: non-uniform category weights, pattern weights that are not all 1"""
    case.rate_weights = CC.weights_for(case.rate_cats)
    case.pattern_weights = CC.pattern_weights_for(case.sites)
    return case


class Pair:
    """one session per library over a case, the traversal done, the category rates set"""

    def __init__(self, amd_lib, ref_lib, case):
        self.case, self.amd_lib, self.ref_lib = case, amd_lib, ref_lib
        self.a, self.r = driver.Session(amd_lib, case), driver.Session(ref_lib, case)
        self.both = (self.a, self.r)
        self.fi = np.ascontiguousarray(case.freqs_indices, dtype=np.uint32)
        self.rates = np.ascontiguousarray(case.model["rates"], dtype=np.float64)
        for s in self.both:
            s.lib.pll_set_category_rates(s.p, api.dptr(self.rates))
            s.update_partials()

    def close(self):
        self.a.close()
        self.r.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def expected(self, edge, weights=None):
        return CC.expected(self.ref_lib, self.r.p, edge, self.fi, weights, self.rates)

    def got(self, edge, want=CC.OUTPUTS):
        return CC.call(self.amd_lib, self.a.p, edge, self.fi, want)

    def check(self, edge, what, want=CC.OUTPUTS):
        """all outputs against the reference, lnl also against the library's own evaluation"""
        own = self.a.edge_lnl(edge, persite=False)[0]  # (whatever the traversal held back is out after this)
        exp = self.expected(edge)
        got = self.got(edge, want)
        fig = CC.assert_outputs(got, exp, what)
        if "lnl" in got:
            assert IC.close(got["lnl"], own, RTOL), (what, "lnl against pll_compute_edge_loglikelihood", got["lnl"], own)
        return got, exp, fig


def _edges(case):
    """the inner-inner root edge and a tip edge, each in both orientations"""
    return [SC.root_edge(case), SC.flip(SC.root_edge(case)), SC.tip_edge(case), SC.flip(SC.tip_edge(case))]


def _launches(pair, edge):
    for want, count in WANT_SETS:
        pair.got(edge, want)
        assert pair.amd_lib.pll_gpu_last_launch_count(pair.a.p) == count, (want, pair.amd_lib.pll_gpu_last_launch_count(pair.a.p))


# ---- 1. shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs", list(SC.ATTRS))
@pytest.mark.parametrize("shape", list(SC.SHAPES))
def test_shapes(amd_lib, ref_lib, shape, attrs):
    case = _prepare(SC.make(shape, SC.ATTRS[attrs]))
    assert len(set(case.pattern_weights.tolist())) > 1 and len(set(case.rate_weights.tolist())) > 1
    with Pair(amd_lib, ref_lib, case) as pair:
        for edge in _edges(case):
            pair.check(edge, (shape, attrs, edge))
        _launches(pair, SC.root_edge(case))
        _launches(pair, SC.tip_edge(case))


# ---- 2. more than one workgroup in every stage ---------------------------------------------------------------------------
def _large(which, attrs=0):
    states, sites = {"dna": (4, 1000), "aa": (20, 300)}[which]
    return _prepare(W.make_case(which, states, 8, sites, attributes=attrs, seed=77 + states))


@pytest.mark.parametrize("which", ["dna", "aa"])
def test_several_workgroups(amd_lib, ref_lib, which):
    case = _large(which)
    with Pair(amd_lib, ref_lib, case) as pair:
        for edge in _edges(case):
            got, _, _ = pair.check(edge, (which, edge))
            again = pair.got(edge)
            for k in CC.OUTPUTS:
                assert np.array_equal(got[k], again[k]), (which, edge, k, "two calls differ")
            via = pair.a.edge_categories(edge)
            assert all(np.array_equal(got[k], via[k]) for k in CC.OUTPUTS), (which, edge, "Session.edge_categories")
            alone = pair.got(edge, ("weight_sums",))
            assert np.array_equal(alone["weight_sums"], got["weight_sums"]), (which, edge, "weight_sums alone")
            sums = pair.got(edge, ("weight_sums", "lnl"))
            assert np.array_equal(sums["weight_sums"], got["weight_sums"]) and sums["lnl"] == got["lnl"], (which, edge)
        _launches(pair, SC.root_edge(case))


# ---- 3. written counts ---------------------------------------------------------------------------------------------------
def _write(pair, edge, on=True):
    """the count tables of scaler_cases into the scalers of both ends, in both libraries -> the arrays written"""
    out = []
    for second, (clv, scaler) in enumerate(((edge[0], edge[1]), (edge[2], edge[3]))):
        if scaler < 0:
            out.append(None)
            continue
        counts = SC.counts_for(pair.r, pair.case, clv, second=bool(second))
        SC.assert_covered(counts, what=(clv, second))
        if not on:
            counts = np.zeros_like(counts)
        for s in pair.both:
            SC.write_scaler(s, scaler, clv, counts)
        out.append(counts)
    return out


def _cat_lnl_over_cap(pair, edge, exp, what):
    """module docstring: the pairs above the cap, from the reference's zero-count evaluation and the integers written"""
    s = CC.summed_counts(pair.r.p, edge)
    _write(pair, edge, on=False)
    plain = pair.expected(edge)
    _write(pair, edge)
    assert np.array_equal(CC.summed_counts(pair.r.p, edge), s)
    full = plain["cat_lnl"] + s * CC.LOG_THRESHOLD
    over = exp["at_cap"]
    below = ~over & np.isfinite(exp["cat_lnl"])
    # where the reference's own value is good, the two expectations agree: the replacement changes nothing else
    assert CC.worst_log(full[below], exp["cat_lnl"][below]) <= RTOL, (what, "the two expectations disagree below the cap")
    print("categories", what, "cat_lnl at the cap and above:", int(over.sum()), "pairs; the reference's subnormal values deviate by",
          f"{CC.worst_log(exp['cat_lnl'][over], full[over]):.2e}" if over.any() else "-")
    exp["cat_lnl"] = np.where(over, full, exp["cat_lnl"])


@pytest.mark.parametrize("attrs", ["rs", "plain"])
@pytest.mark.parametrize("shape", ["dna", "dna-r8", "aa"])
def test_written_counts(amd_lib, ref_lib, shape, attrs):
    case = _prepare(SC.make(shape, SC.ATTRS[attrs]))
    with Pair(amd_lib, ref_lib, case) as pair:
        seen_over = False
        for edge in _edges(case):
            what = (shape, attrs, edge)
            _write(pair, edge)
            exp = pair.expected(edge)
            if attrs == "rs":
                ex = CC.summed_counts(pair.r.p, edge)
                ex = ex - ex.min(1, keepdims=True)
                if edge[1] >= 0 and edge[3] >= 0:
                    assert {1, 2, 3, 4} <= set(ex.ravel().tolist()) and (ex > CC.CAP).any(), (what, "the written tables hold no such excess")
                seen_over = seen_over or bool(exp["over_cap"].any())
                _cat_lnl_over_cap(pair, edge, exp, what)
            else:
                assert not exp["over_cap"].any()
            own = pair.a.edge_lnl(edge, persite=False)[0]
            got = pair.got(edge)
            CC.assert_outputs(got, exp, what)
            assert IC.close(got["lnl"], own, RTOL), (what, got["lnl"], own)
        assert seen_over == (attrs == "rs")


# ---- 4. invariant sites --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs", ["plain", "rs"])
@pytest.mark.parametrize("shape", list(SC.PINV_SHAPES))
def test_invariant_sites(amd_lib, ref_lib, shape, attrs):
    case = _prepare(SC.make(shape, SC.ATTRS[attrs], pinv=0.3))
    with Pair(amd_lib, ref_lib, case) as pair:
        for edge in _edges(case):
            _, exp, _ = pair.check(edge, (shape, attrs, "pinv", "tree counts", edge))
            assert exp["invariant"].any() and not exp["invariant"].all(), "the case has no invariant site, or nothing else"
        scaled_invariant = 0
        for edge in _edges(case):
            what = (shape, attrs, "pinv", "written counts", edge)
            _write(pair, edge)
            exp = pair.expected(edge)
            scaled_invariant += int((exp["invariant"] & exp["scaled"]).sum())
            if attrs == "rs":
                _cat_lnl_over_cap(pair, edge, exp, what)
            own = pair.a.edge_lnl(edge, persite=False)[0]
            got = pair.got(edge)
            CC.assert_outputs(got, exp, what)
            assert IC.close(got["lnl"], own, RTOL), (what, got["lnl"], own)
        assert scaled_invariant, "no invariant site with a scaling count: the written leg shows nothing"


# ---- 5. trees that rescale -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs", [0, api.RATE_SCALERS], ids=["per-site", "per-rate"])
@pytest.mark.parametrize("states,tips,sites,least", [(4, 600, 700, 250), (20, 200, 300, 90)], ids=["dna600", "aa200"])
def test_trees_that_rescale(amd_lib, ref_lib, states, tips, sites, least, attrs):
    rng, tree, (a, r) = _tree_pair(amd_lib, ref_lib, states, tips, sites, attrs, (8300 if attrs else 8100) + states)
    w, pw = CC.weights_for(4), CC.pattern_weights_for(sites)
    rates = W.gamma_rates_mean(0.7, 4)
    uneven = 0
    try:
        for d in (a, r):
            d.lib.pll_set_category_weights(d.p, api.dptr(w))
            d.lib.pll_set_pattern_weights(d.p, api.uptr(pw))
        for rec in _deep_records(tree, rng, 3, least):
            ops = tree.ops_for(rec)
            a.update(ops)
            r.update(ops)
            edge = tree.edge_args(rec)
            s = CC.summed_counts(r.p, edge)
            assert s.any(), ("the reference did not rescale at the evaluated edge", edge)
            uneven += int((s.max(1) != s.min(1)).sum())
            own = amd_lib.pll_compute_edge_loglikelihood(a.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(a.fi), None)
            exp = CC.expected(ref_lib, r.p, edge, r.fi, None, rates)
            assert not exp["over_cap"].any()
            got = CC.call(amd_lib, a.p, edge, a.fi)
            CC.assert_outputs(got, exp, (states, attrs, edge))
            assert IC.close(got["lnl"], own, RTOL), (edge, got["lnl"], own)
        if attrs:
            assert uneven, "no site whose categories carry different counts: the case shows nothing"
    finally:
        a.close()
        r.close()


# ---- 6. a mixture --------------------------------------------------------------------------------------------------------
def test_mixture_of_frequency_sets(amd_lib, ref_lib):
    case = _prepare(W.make_case("mixture", 20, 8, 65, seed=611))
    rng = np.random.Generator(np.random.PCG64(612))
    sets = rng.uniform(0.2, 1.8, size=(4, 20))
    case.freqs = np.ascontiguousarray(sets / sets.sum(1, keepdims=True))
    case.freqs_indices = np.arange(4, dtype=np.uint32)
    case.prop_invar = np.zeros(4)
    with Pair(amd_lib, ref_lib, case) as pair:
        assert pair.a.part.rate_matrices == 4
        for edge in _edges(case):
            pair.check(edge, ("mixture", edge))


# ---- 7. EM ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["dna", "aa"])
def test_em(amd_lib, ref_lib, which):
    case = _large(which)
    steps = 5
    with Pair(amd_lib, ref_lib, case) as pair:
        edge = SC.root_edge(case)
        before = pair.a.edge_lnl(edge, persite=False)[0]
        start = CC.weights_for(4)
        rows, lnl = CC.em(amd_lib, pair.a.p, edge, pair.fi, start, steps)
        assert amd_lib.pll_gpu_last_launch_count(pair.a.p) == 1 + 2 * (steps + 1)
        assert np.array_equal(rows[0], start)
        pw = case.pattern_weights.astype(np.float64)
        for i in range(steps + 1):
            exp = pair.expected(edge, rows[i])
            assert IC.close(lnl[i], exp["lnl"], RTOL), (which, i, lnl[i], exp["lnl"])
            if i < steps:
                s = (pw[:, None] * exp["posterior"]).sum(0)
                nxt = s / s.sum()
                worst = CC.worst_rel(rows[i + 1], nxt)
                print("categories EM", which, "row", i + 1, f"{worst:.2e}", "lnl", lnl[i])
                assert worst <= RTOL, (which, i, worst)
            assert abs(rows[i].sum() - 1.0) <= SUMTOL, (which, i, rows[i].sum())
        assert (np.diff(lnl) >= -RTOL * np.abs(lnl[:-1])).all(), (which, "the log-likelihood fell", lnl)
        # steps == 0 is one evaluation: the posteriors call's lnl, bit for bit; NULL start = the partition's weights
        r0, l0 = CC.em(amd_lib, pair.a.p, edge, pair.fi, None, 0)
        assert amd_lib.pll_gpu_last_launch_count(pair.a.p) == 3
        assert np.array_equal(r0[0], case.rate_weights)
        assert l0[0] == pair.got(edge, ("lnl",))["lnl"] and l0[0] == lnl[0]
        r1, l1 = CC.em(amd_lib, pair.a.p, edge, pair.fi, None, steps)
        assert np.array_equal(r1, rows) and np.array_equal(l1, lnl)
        r2, l2 = pair.a.category_weights_em(edge, start, steps)
        assert np.array_equal(r2, rows) and np.array_equal(l2, lnl), "Session.category_weights_em"
        # the partition's own weights are neither written nor forgotten
        assert np.array_equal(api.as_np(pair.a.part.rate_weights, 4, np.float64), case.rate_weights)
        assert pair.a.edge_lnl(edge, persite=False)[0] == before


# ---- 8. nothing is written -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs", ["plain", "rs-tip"])
def test_nothing_is_written(amd_lib, ref_lib, attrs):
    case = _prepare(SC.make("dna", SC.ATTRS[attrs]))
    with Pair(amd_lib, ref_lib, case) as pair:
        a = pair.a
        for edge in (SC.root_edge(case), SC.tip_edge(case)):
            def state():
                ends = [(clv, sc) for clv, sc in ((edge[0], edge[1]), (edge[2], edge[3])) if not (clv < case.tips and attrs == "rs-tip")]
                return ([a.read_clv(clv) for clv, _ in ends], [a.read_scaler(sc, clv) for clv, sc in ends if sc >= 0], a.edge_lnl(edge)[1])

            clvs, scalers, persite = state()
            pair.got(edge)
            CC.em(amd_lib, a.p, edge, pair.fi, None, 2)
            clvs2, scalers2, persite2 = state()
            assert all(np.array_equal(x, y) for x, y in zip(clvs, clvs2))
            assert all(np.array_equal(x, y) for x, y in zip(scalers, scalers2))
            assert np.array_equal(persite, persite2)
