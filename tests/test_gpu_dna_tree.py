"""A balanced 64-taxon DNA traversal and the evaluation of its root edge as ONE launch (kernels_dna.h: k_edge_dna_tree;
chosen by size, PLL_AMD_FUSE_TREE=1 / 0 forces it on / off). pll_update_partials holds the whole plan, the edge
evaluation takes it; whatever else the caller does next sends it out as the ordinary launches. Every CLV, scaler and
log-likelihood must equal the ordinary route's bit for bit, and the oracle's within RTOL."""
import functools
import os

import numpy as np
import pytest

from compare import RTOL, assert_results_match, scalers_equal
from oracle import oracle as O
from pllamd import api, driver, workload as W

pytestmark = pytest.mark.gpu

SWITCH = "PLL_AMD_FUSE_TREE"


def _counts_apply():
    """eager mirroring reads every CLV back right after the traversal and dense tips have no seven-op groups: nothing is held"""
    return all(os.environ.get(v, "0") in ("", "0") for v in ("PLL_AMD_EAGER_MIRROR", "PLL_AMD_NO_TIP_CODES", "PLL_AMD_NO_TAIL_FUSION",
                                                              "PLL_AMD_NO_FUSE", "PLL_AMD_NO_FUSE_CC", "PLL_AMD_NO_CHAINS"))


@functools.lru_cache(maxsize=None)
def _case_and_oracle(sites, seed=5, **kw):
    case = W.make_case("tree", 4, 64, sites, seed=seed, **kw)
    return case, O.run_case(case)


def _step(lib, case, persite=True):
    """traversal, then DIRECTLY the edge evaluation (nothing in between that would send the held plan out), then every
    CLV and scaler: the shape of driver.run_case's result, + the launch counts after the two calls"""
    out = {"clv": {}, "scaler": {}, "lnl": [], "persite": [], "root_lnl": [], "root_persite": []}
    with driver.Session(lib, case, api.ARCH_AVX2) as s:
        s.update_partials()
        held = lib.pll_gpu_last_launch_count(s.p)
        v, ps = s.edge_lnl(case.edges[0], persite=persite)
        out["launches"] = (held, lib.pll_gpu_last_launch_count(s.p))
        out["lnl"].append(v)
        if persite:
            out["persite"].append(ps)
        for op in case.op_batches[0]:
            out["clv"][op[0]] = s.read_clv(op[0])
            if op[1] >= 0:
                out["scaler"][op[0]] = s.read_scaler(op[1], op[0])
    return out


def _both(lib, case, monkeypatch, persite=True):
    monkeypatch.setenv(SWITCH, "1")
    tree = _step(lib, case, persite)
    monkeypatch.setenv(SWITCH, "0")
    plain = _step(lib, case, persite)
    if _counts_apply():
        assert tree["launches"] == (0, 1), tree["launches"]   # the whole step is the evaluation's launch
        assert plain["launches"] == (1, 2), plain["launches"]
    return tree, plain


def _assert_same_bits(tree, plain):
    assert tree["lnl"] == plain["lnl"]
    for a, b in zip(tree["persite"], plain["persite"]):
        assert (a == b).all()
    assert len(plain["clv"]) == 62
    for k, v in plain["clv"].items():
        assert (tree["clv"][k] == v).all(), k
    assert set(tree["scaler"]) == set(plain["scaler"])
    for k, v in plain["scaler"].items():
        assert (tree["scaler"][k] == v).all(), k


@pytest.mark.parametrize("sites", [1, 63, 64, 65, 130, 1000])
def test_bits_at_tile_edges(amd_lib, monkeypatch, sites):
    """one lane, a tile less one, a whole tile, a tile and one, three tiles (the last ragged), sixteen"""
    case, exp = _case_and_oracle(sites, ambiguity_pct=3, partial_pct=2)
    tree, plain = _both(amd_lib, case, monkeypatch)
    _assert_same_bits(tree, plain)
    assert_results_match(tree, exp, what="tree-%d" % sites)


@pytest.mark.parametrize("kw", [dict(brlen_scale=1e-4, mutate_pct=60),                                # level 5 only, and only some sites: a mixed decision
                                dict(brlen_scale=1e-7, mutate_pct=60),                                # levels 4 and 5
                                dict(brlen_scale=1e-6, mutate_pct=90, attributes=api.RATE_SCALERS)],  # per rate
                         ids=["level5-mixed", "levels4-5", "rate-scalers"])
def test_scaling_decisions_inside_the_launch(amd_lib, monkeypatch, kw):
    """a 64-taxon tree does not scale with ordinary branch lengths; with (nearly) identical sequences on very short
    branches the products of the upper levels fall below 2^-256: the decisions are taken by the waves that form levels
    4 and 5 from the LDS exchange"""
    case, exp = _case_and_oracle(130, **kw)
    assert sum(int(v.sum()) for v in exp["scaler"].values()) > 0  # the input does scale
    tree, plain = _both(amd_lib, case, monkeypatch)
    _assert_same_bits(tree, plain)
    assert_results_match(tree, exp, what="tree-scaling")
    assert scalers_equal(tree, exp)


@pytest.mark.parametrize("kw,persite", [(dict(pattern_weights=np.arange(130, dtype=np.uint32) % 5 + 1), False),
                                        (dict(pinv=0.3, mutate_pct=4), False),
                                        (dict(), True),
                                        (dict(scalers=False), False)],
                         ids=["pattern-weights", "invariant-sites", "per-site-output", "no-scalers"])
def test_edge_options(amd_lib, monkeypatch, kw, persite):
    case = W.make_case("tree-opt", 4, 64, 130, seed=7, ambiguity_pct=3, **kw)
    exp = O.run_case(case)
    tree, plain = _both(amd_lib, case, monkeypatch, persite=persite)
    _assert_same_bits(tree, plain)
    assert abs(tree["lnl"][0] - exp["lnl"][0]) <= RTOL * abs(exp["lnl"][0])
    if persite:
        assert np.all(np.abs(tree["persite"][0] - exp["persite"][0]) <= RTOL * np.maximum(np.abs(exp["persite"][0]), 1.0))


@pytest.mark.parametrize("sites", [128, 130], ids=["extra-entries-in-their-own-tile", "extra-entries-behind-the-sites"])
@pytest.mark.parametrize("kw", [dict(asc_type=1), dict(asc_type=3, asc_weights=[5, 4, 6, 2])], ids=["lewis", "stamatakis"])
def test_ascertainment_bias_entries_ride_along(amd_lib, monkeypatch, kw, sites):
    """every CLV of an ascertainment-bias partition has one entry per state behind its sites: the launch computes and stores
    them like sites (the correction reads them from the two ends right after the evaluation), no site likelihood sees them"""
    case, exp = _case_and_oracle(sites, seed=9, ambiguity_pct=3, asc_type=kw["asc_type"], asc_weights=tuple(kw.get("asc_weights", ())) or None)
    tree, plain = _both(amd_lib, case, monkeypatch)
    _assert_same_bits(tree, plain)
    for a in tree["clv"].values():
        assert a.shape[0] == sites + 4
    assert_results_match(tree, exp, what="tree-asc")
    assert scalers_equal(tree, exp)


def test_the_hold_is_invisible(amd_lib, monkeypatch):
    """whatever follows the traversal instead of the matching evaluation sees the state the ordinary launches leave"""
    case, exp = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    ops = case.op_batches[0]
    e = case.edges[0]
    other = (ops[-3][0], ops[-3][1], ops[-4][0], ops[-4][1], e[4])
    bottom = ops[0]
    inner = api.make_ops([op for op in ops if op[2] >= 64 and op[5] >= 64])

    def observe():
        out = {}
        with driver.Session(amd_lib, case, api.ARCH_AVX2) as s:
            s.update_partials()
            out["held"] = amd_lib.pll_gpu_last_launch_count(s.p)
            out["edge"] = s.edge_lnl(e, persite=False)[0]
            out["taken"] = amd_lib.pll_gpu_last_launch_count(s.p)
            s.update_partials()
            out["bottom_clv"] = s.read_clv(bottom[0])
            s.update_partials()
            out["bottom_scaler"] = s.read_scaler(bottom[1], bottom[0])
            s.update_partials()
            out["end_clv"] = s.read_clv(e[0])
            s.update_partials()
            out["end_scaler"] = s.read_scaler(e[3], e[2])
            s.update_partials()
            out["root"] = s.root_lnl((e[0], e[1]), persite=False)[0]
            s.update_partials()
            out["other_edge"] = s.edge_lnl(other, persite=False)[0]
            out["edge_after"] = s.edge_lnl(e, persite=False)[0]
            s.update_partials()
            s.update_partials()                                     # the first call's plan goes out before the second is held
            out["edge_twice"] = s.edge_lnl(e, persite=False)[0]
            s.update_partials()
            amd_lib.pll_update_partials(s.p, inner, 30)             # the 30 inner x inner ops: another list
            out["edge_partial"] = s.edge_lnl(e, persite=False)[0]
            out["top_clv"] = s.read_clv(e[2])
            # a matrix that the held groups read goes up between the two calls: the plan is sent out first, with the matrix it was
            # planned with (the caller wrote the host copy after the traversal)
            s.update_partials()
            m, sp = bottom[3], s.sp
            host = api.as_np(s.part.pmatrix[m], case.rate_cats * 4 * sp, np.float64)
            host[:] = api.as_np(s.part.pmatrix[e[4]], case.rate_cats * 4 * sp, np.float64)
            amd_lib.pll_gpu_invalidate(s.p, api.DIRTY_PMATRIX, m)
            out["edge_bottom_matrix"] = s.edge_lnl((e[0], e[1], e[2], e[3], m), persite=False)[0]
            out["bottom_clv_after_upload"] = s.read_clv(bottom[0])
            s.update_partials()                                     # closed with the plan still held
        return out

    monkeypatch.setenv(SWITCH, "1")
    tree = observe()
    monkeypatch.setenv(SWITCH, "0")
    plain = observe()
    if _counts_apply():
        assert (tree["held"], tree["taken"]) == (0, 1)
        assert (plain["held"], plain["taken"]) == (1, 2)
    for k in plain:
        if k in ("held", "taken"):
            continue
        assert np.array_equal(tree[k], plain[k]), k
    assert abs(tree["edge"] - exp["lnl"][0]) <= RTOL * abs(exp["lnl"][0])
    assert tree["edge"] == tree["edge_after"] == tree["edge_twice"] == tree["edge_partial"]
    assert (tree["bottom_clv_after_upload"] == tree["bottom_clv"]).all()  # the traversal did not see the new matrix


def test_replay_and_a_new_branch_length(amd_lib, monkeypatch):
    """the kept plan is launched again as it is; a matrix rewritten on the device is what the next step reads"""
    case, _ = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    e = case.edges[0]
    nmat = case.prob_matrices
    brlen = np.ascontiguousarray(W.branch_lengths(nmat))
    pi = np.zeros(case.rate_cats, dtype=np.uint32)
    changed = 5  # the matrix of a branch in the bottom groups

    def session(s, lengths):
        s.set_model(case.model["exch"], case.freqs, case.model["rates"])
        mi = np.arange(nmat, dtype=np.uint32)
        assert amd_lib.pll_update_prob_matrices(s.p, api.uptr(pi), api.uptr(mi), api.dptr(np.ascontiguousarray(lengths)), nmat)

    def step(s):
        s.update_partials()
        return s.edge_lnl(e)

    def run():
        longer = brlen.copy()
        longer[changed] *= 3.0
        with driver.Session(amd_lib, case, api.ARCH_AVX2) as s:
            session(s, brlen)
            steps = [step(s) for _ in range(3)]
            one = np.array([changed], dtype=np.uint32)
            assert amd_lib.pll_update_prob_matrices(s.p, api.uptr(pi), api.uptr(one), api.dptr(longer[changed:changed + 1].copy()), 1)
            moved = step(s)
        with driver.Session(amd_lib, case, api.ARCH_AVX2) as s:
            session(s, longer)
            fresh = step(s)
        return steps, moved, fresh

    monkeypatch.setenv(SWITCH, "1")
    steps, moved, fresh = run()
    for v, ps in steps[1:]:
        assert v == steps[0][0] and (ps == steps[0][1]).all()
    assert moved[0] != steps[0][0]
    assert moved[0] == fresh[0] and (moved[1] == fresh[1]).all()
    monkeypatch.setenv(SWITCH, "0")
    psteps, pmoved, _ = run()
    assert psteps[0][0] == steps[0][0] and (psteps[0][1] == steps[0][1]).all()
    assert pmoved[0] == moved[0] and (pmoved[1] == moved[1]).all()


def test_small_lists_keep_their_plan(amd_lib, monkeypatch):
    """by size: 640 sites are far below the threshold - one launch for the groups, the chain tail inside the evaluation"""
    monkeypatch.delenv(SWITCH, raising=False)
    case = W.make_case("tree-small", 4, 64, 640, seed=97)
    launches = _step(amd_lib, case, persite=False)["launches"]
    if _counts_apply():
        assert launches == (1, 2)
