"""Lazy subtrees: inside a loop that reads no CLV between its steps, the whole-traversal launch of a balanced 64-taxon DNA
tree (kernels_dna.h: k_edge_dna_tree) stores NOTHING of its eight complete 8-tip subtrees - the 56 ops of levels 1 to 3 -
and only the six CLVs of levels 4 and 5 (TreeStores::TopsOnly). The first launch of a plan leaves the 32 tip x tip parents
unstored as before (tests/test_gpu_dna_lazy_cherries.py); from the second step on, as long as each step finds the previous
one's CLVs still pending, 56 are. One seven-op group launch stores them before anything reads them, overwrites them or
changes their codes; a change of a matrix they read makes them keep the 112 matrices of the step aside.
PLL_AMD_LAZY_SUBTREES=0/1 switches the deep form; unset it follows the tree launch's own size rule (20 000 entries).

The yardstick is that file's: the SAME call sequence through the ordinary route (PLL_AMD_FUSE_TREE=0), bit for bit, on
all 62 CLVs, all scalers, lnL and per-site lnL, plus the oracle within RTOL. The tree launch is forced (PLL_AMD_FUSE_TREE=1)
and the deep form allowed (PLL_AMD_LAZY_SUBTREES=1) at 1, 65 and 130 sites unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_dna_lazy_cherries as LC
from compare import RTOL, assert_results_match, scalers_equal
from pllamd import api, driver, workload as W

pytestmark = pytest.mark.gpu

TREE, LAZY, DEEP = "PLL_AMD_FUSE_TREE", "PLL_AMD_LAZY_CHERRIES", "PLL_AMD_LAZY_SUBTREES"
CHERRIES, GROUP_OPS = 32, 56
SIZES = LC.SIZES


def _levels(case):
    """parent CLV -> level of its op, tip x tip = 1"""
    level = {}
    for op in case.op_batches[0]:
        level[op[0]] = 1 + max(level.get(op[2], 0), level.get(op[5], 0))
    return level


def _ops_at(case, lv):
    level = _levels(case)
    ops = [op for op in case.op_batches[0] if level[op[0]] == lv]
    assert len(ops) == 64 >> lv
    return ops


def _run(lib, case, monkeypatch, seq, tree, lazy=None, deep="1"):
    for name, value in ((TREE, tree), (LAZY, lazy), (DEEP, deep)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    out = {"persite": [], "root_lnl": [], "root_persite": []}
    with driver.Session(lib, case, api.ARCH_AVX2) as s:
        seq(s, out)
    return out


def _both(lib, case, monkeypatch, seq, **kw):
    """the same call sequence through the tree launch and through the ordinary route"""
    return _run(lib, case, monkeypatch, seq, "1", **kw), _run(lib, case, monkeypatch, seq, "0", **kw)


def _policy(steps):
    """what is pending after each step of an undisturbed loop: the first launch of a plan is the lean form"""
    return [CHERRIES] + [GROUP_OPS] * (steps - 1)


def _assert_step_counts(tree, plain, pending):
    if not LC._counts_apply():
        return
    assert tree["n_launches"] == [(0, 1)] * len(pending), tree["n_launches"]  # the whole step is the evaluation's launch
    assert tree["n_pending"] == pending, tree["n_pending"]
    assert plain["n_pending"] == [0] * len(pending), plain["n_pending"]


def _first_result(out, exp):
    """the steps repeat one computation: the oracle's single evaluation against the first of them"""
    return dict(out, lnl=out["lnl"][:len(exp["lnl"])], persite=out["persite"][:len(exp["persite"])])


def _three_steps_and_read_all(case):
    def seq(s, out):
        for _ in range(3):
            LC._step(s, case, out)
        out["one_level_2"] = s.read_clv(_ops_at(case, 2)[0][0])
        out["n_after_read"] = s.pending_clvs()  # the first read of an unstored CLV stores all of them
        LC._read_all(s, case, out)
    return seq


# ---- bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sites", SIZES)
def test_three_steps_then_read_everything(amd_lib, monkeypatch, sites):
    case, exp = LC._case_and_oracle(sites, ambiguity_pct=3, partial_pct=2)
    tree, plain = _both(amd_lib, case, monkeypatch, _three_steps_and_read_all(case))
    _assert_step_counts(tree, plain, _policy(3))
    assert tree["n_after_read"] == 0
    LC._assert_same_bits(tree, plain)
    assert tree["lnl"][0] == tree["lnl"][1] == tree["lnl"][2]
    assert all(np.array_equal(tree["persite"][0], ps) for ps in tree["persite"][1:])
    assert_results_match(_first_result(tree, exp), exp, what="subtrees-%d" % sites)
    if LC._counts_apply():
        # what the deep launch moves: 6 CLVs + scalers out, 64 code bytes in, per entry
        assert tree["n_bytes"] == sites * (6 * 132 + 64), tree["n_bytes"]


def test_one_step_then_read_never_enters_the_deep_form(amd_lib, monkeypatch):
    case, exp = LC._case_and_oracle(130, ambiguity_pct=3, partial_pct=2)

    def seq(s, out):
        for _ in range(3):  # a caller who reads after every step
            LC._step(s, case, out)
            out.setdefault("level_2", []).append(s.read_clv(_ops_at(case, 2)[0][0]))
            out.setdefault("n_after_read", []).append(s.pending_clvs())
        LC._read_all(s, case, out)

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, [CHERRIES] * 3)
    assert tree["n_after_read"] == [0] * 3
    LC._assert_same_bits(tree, plain)
    assert_results_match(_first_result(tree, exp), exp, what="subtrees-read-each-step")
    if LC._counts_apply():
        assert tree["n_bytes"] == 130 * (30 * 132 + 64), tree["n_bytes"]


@pytest.mark.parametrize("kw,levels", [(dict(brlen_scale=1e-12, mutate_pct=90), (3,)),
                                       (dict(brlen_scale=1e-14, mutate_pct=90, attributes=api.RATE_SCALERS), (1, 2, 3, 4, 5))],
                         ids=["per-site-scalers", "rate-scalers"])
def test_scaling_below_level_4(amd_lib, monkeypatch, kw, levels):
    """the scaler words of the unstored levels come out with their CLVs, and the tops are scaled on top of them"""
    case, exp = LC._case_and_oracle(130, ambiguity_pct=3, partial_pct=2, **kw)
    for lv in levels:  # the input does scale there
        assert sum(int(np.count_nonzero(exp["scaler"][op[0]])) for op in _ops_at(case, lv)) > 0, lv
    tree, plain = _both(amd_lib, case, monkeypatch, _three_steps_and_read_all(case))
    _assert_step_counts(tree, plain, _policy(3))
    LC._assert_same_bits(tree, plain)
    for lv in (1, 2, 3):
        for op in _ops_at(case, lv):
            assert op[0] in tree["scaler"]
    assert_results_match(_first_result(tree, exp), exp, what="subtrees-scaling")
    assert scalers_equal(tree, exp)


def test_ascertainment_bias_entries_of_the_unstored_clvs(amd_lib, monkeypatch):
    """130 sites + 4 per-state entries behind them: stored on demand like the sites"""
    case, exp = LC._case_and_oracle(130, seed=9, ambiguity_pct=3, asc_type=1)
    tree, plain = _both(amd_lib, case, monkeypatch, _three_steps_and_read_all(case))
    _assert_step_counts(tree, plain, _policy(3))
    LC._assert_same_bits(tree, plain)
    for a in tree["clv"].values():
        assert a.shape[0] == 134
    assert_results_match(_first_result(tree, exp), exp, what="subtrees-asc")
    assert scalers_equal(tree, exp)


# ---- the loop the deep form is for ----------------------------------------------------------------------------------------
def test_a_model_parameter_loop_stores_nothing(amd_lib, monkeypatch):
    """new category rates, every matrix formed again, full traversal, root-edge evaluation - four times: whatever the last
    step left unstored stays so, with the 64 or 112 matrices of that step kept aside; then every matrix once more, and
    everything read afterwards is the last step's, from the matrices of that step"""
    case, _ = LC._case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    nmat = case.prob_matrices
    brlen = W.branch_lengths(nmat)
    rates = np.asarray(case.model["rates"], dtype=np.float64)

    def seq(s, out):
        pend = []
        for k in range(4):
            s.set_model(case.model["exch"], case.freqs, rates * (1.0 + 0.25 * k))
            pend.append(s.pending_clvs())
            LC._form_matrices(s, case, np.arange(nmat), brlen)
            pend.append(s.pending_clvs())
            LC._step(s, case, out, persite=False)
        LC._form_matrices(s, case, np.arange(nmat), brlen * 1.5)
        pend.append(s.pending_clvs())
        out["n_pend"] = pend
        LC._read_all(s, case, out)
        out["n_end"] = s.pending_clvs()
        LC._step(s, case, out, persite=False)  # ... and the next step reads the new matrices

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, _policy(4) + [CHERRIES])
    if LC._counts_apply():
        assert tree["n_pend"] == [0, 0] + [CHERRIES] * 2 + [GROUP_OPS] * 5, tree["n_pend"]
    assert tree["n_end"] == 0
    LC._assert_same_bits(tree, plain)
    assert len(set(tree["lnl"])) == 5


def test_calls_that_keep_all_56_pending(amd_lib, monkeypatch):
    """a wait for the stream, a second (per-site) evaluation of the root edge, a new matrix on the root edge, sumtable,
    derivatives and the Newton call at the root edge: the two ends of the root edge are stored, nothing else is read"""
    case, exp = LC._case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    e = case.edges[0]
    edge = (e[0], e[1], e[2], e[3])
    nmat = case.prob_matrices

    def seq(s, out):
        lib = s.lib
        s.set_model(case.model["exch"], case.freqs, case.model["rates"])
        LC._form_matrices(s, case, np.arange(nmat), W.branch_lengths(nmat))
        for _ in range(2):
            LC._step(s, case, out, persite=False)
        pend = []
        assert lib.pll_gpu_synchronize(s.p)
        pend.append(s.pending_clvs())
        out["again"], out["again_persite"] = s.edge_lnl(e, persite=True)
        pend.append(s.pending_clvs())
        n = case.rate_cats * 4 * s.sp  # the edge's own matrix rewritten on the host: goes up with the next evaluation
        api.as_np(s.part.pmatrix[e[4]], n, np.float64)[:] = api.as_np(s.part.pmatrix[3], n, np.float64)
        lib.pll_gpu_invalidate(s.p, api.DIRTY_PMATRIX, e[4])
        out["moved"] = s.edge_lnl(e, persite=False)[0]
        pend.append(s.pending_clvs())
        st = s.new_sumtable()
        s.update_sumtable(edge, st)
        out["derivatives"] = s.derivatives(edge, st, 0.13)
        pend.append(s.pending_clvs())
        res, trace = s.optimize_branch(edge, st, 0.1, t_min=1e-6, t_max=100.0, tolerance=1e-9, matrix_index=e[4])
        out["newton"] = (res.t, trace)
        pend.append(s.pending_clvs())
        out["after_newton"] = s.edge_lnl(e, persite=False)[0]
        pend.append(s.pending_clvs())
        out["n_pend"] = pend
        LC._read_all(s, case, out)
        out["n_end"] = s.pending_clvs()

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, _policy(2))
    if LC._counts_apply():
        assert tree["n_pend"] == [GROUP_OPS] * 6, tree["n_pend"]
    assert tree["n_end"] == 0
    LC._assert_same_bits(tree, plain)
    assert tree["again"] == tree["lnl"][1] and tree["moved"] != tree["lnl"][1] and tree["after_newton"] != tree["moved"]


# ---- what stores them first -----------------------------------------------------------------------------------------------
def _read_a_level_2_clv(s, case, out):
    out["value"] = s.read_clv(_ops_at(case, 2)[3][0])


def _read_a_level_3_clv(s, case, out):
    out["value"] = s.read_clv(_ops_at(case, 3)[5][0])


def _read_a_scaler(s, case, out):
    op = _ops_at(case, 2)[7]
    out["value"] = s.read_scaler(op[1], op[0]).astype(np.float64)


def _sumtable_at_a_level_3_edge(s, case, out):
    a, b = _ops_at(case, 3)[0], _ops_at(case, 3)[1]
    edge = (a[0], a[1], b[0], b[1])
    st = s.new_sumtable()
    s.update_sumtable(edge, st)
    out["value"] = s.derivatives(edge, st, 0.13)
    out["sumtable"] = s.read_sumtable(st)


def _new_tip_codes(s, case, out):
    """the host keeps new codes until a device call wants that tip: the evaluation of an edge from a stored end of the root
    edge to the tip sends them up, and the upload stores what was formed from the old ones first"""
    LC._new_tip_codes(s, case, out)
    e, tip = case.edges[0], LC._cherry_ops(case)[0][2]
    out["value"] = s.edge_lnl((e[0], e[1], tip, -1, 5), persite=False)[0]


@pytest.mark.parametrize("action", [_read_a_level_2_clv, _read_a_level_3_clv, _read_a_scaler, _sumtable_at_a_level_3_edge,
                                    _new_tip_codes, LC._inner_ops_as_another_list],
                         ids=["level-2-read", "level-3-read", "scaler-read", "sumtable-at-level-3", "tip-codes", "another-list"])
def test_calls_that_store_them_first(amd_lib, monkeypatch, action):
    """two steps (56 unstored), the action, then reads at every unstored level: what the ordinary route holds under the same
    sequence - the values of the step, formed from the matrices and codes of the step"""
    case, _ = LC._case_and_oracle(130, ambiguity_pct=3, partial_pct=2)

    def seq(s, out):
        s.set_model(case.model["exch"], case.freqs, case.model["rates"])  # (the derivatives want an eigensystem)
        for _ in range(2):
            LC._step(s, case, out, persite=False)
        action(s, case, out)
        out["n_after"] = s.pending_clvs()
        for lv in (1, 2, 3):
            for name, op in (("first", _ops_at(case, lv)[0]), ("last", _ops_at(case, lv)[-1])):
                out["%s_%d" % (name, lv)] = s.read_clv(op[0])
                out["%s_%d_scaler" % (name, lv)] = s.read_scaler(op[1], op[0])
        out["n_end"] = s.pending_clvs()
        # ... and the tree goes on from there: a new loop starts with the lean form
        for _ in range(2):
            LC._step(s, case, out, persite=False)

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, _policy(2) + _policy(2))
    assert tree["n_after"] == 0 and tree["n_end"] == 0
    LC._assert_same_bits(tree, plain)
    assert np.all(np.isfinite(np.asarray(tree["value"])))


def test_a_wait_between_the_traversal_and_the_evaluation_inside_a_loop(amd_lib, monkeypatch):
    """pll_gpu_synchronize sends the held traversal out as the ordinary two launches, which cannot leave the group parents
    unstored (the chains read them from memory): 32 pending, launches and bytes as without the deep form"""
    case, exp = LC._case_and_oracle(130, ambiguity_pct=3, partial_pct=2)

    def seq(s, out):
        for _ in range(2):
            LC._step(s, case, out, persite=False)
        s.update_partials()
        out["n_held"] = (s.lib.pll_gpu_last_launch_count(s.p), s.pending_clvs(), s.lib.pll_gpu_last_algorithmic_bytes(s.p))
        assert s.lib.pll_gpu_synchronize(s.p)
        out["n_sync"] = (s.lib.pll_gpu_last_launch_count(s.p), s.pending_clvs(), s.lib.pll_gpu_last_algorithmic_bytes(s.p))
        v, ps = s.edge_lnl(case.edges[0], persite=True)
        out["lnl"].append(v)
        out["persite"] = [ps]
        out["n_eval"] = s.pending_clvs()
        LC._read_all(s, case, out)
        out["n_end"] = s.pending_clvs()

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, _policy(2))
    if LC._counts_apply():
        assert tree["n_held"] == (0, 0, 130 * (6 * 132 + 64)), tree["n_held"]  # held for the deep launch: what that would move
        # the seven-op groups and the two chains: 30 CLVs + scalers out, 64 code bytes in, the 8 group parents read back
        assert tree["n_sync"] == (2, CHERRIES, 130 * (30 * 132 + 64 + 8 * 132)), tree["n_sync"]
        assert plain["n_sync"][:2] == (2, 0) and plain["n_sync"][2] == tree["n_sync"][2] + 130 * CHERRIES * 132
        assert tree["n_eval"] == CHERRIES
    assert tree["n_end"] == 0
    LC._assert_same_bits(tree, plain)
    assert tree["lnl"][0] == tree["lnl"][1] == tree["lnl"][2]
    assert_results_match(dict(tree, lnl=tree["lnl"][:1]), exp, what="subtrees-wait")


# ---- the switches, the default and the end --------------------------------------------------------------------------------
@pytest.mark.parametrize("lazy,deep,pending", [(None, "0", [CHERRIES] * 3), ("0", "1", [0] * 3), (None, None, [CHERRIES] * 3)],
                         ids=["subtrees-off", "cherries-off", "default-below-the-size-rule"])
def test_switches(amd_lib, monkeypatch, lazy, deep, pending):
    """PLL_AMD_LAZY_SUBTREES=0: the lean form throughout; PLL_AMD_LAZY_CHERRIES=0: everything is stored; both unset at 130
    sites with the tree launch forced: the deep form follows the tree launch's size rule and stays off"""
    case, exp = LC._case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    seq = _three_steps_and_read_all(case)
    tree = _run(amd_lib, case, monkeypatch, seq, "1", lazy=lazy, deep=deep)
    plain = _run(amd_lib, case, monkeypatch, seq, "0", lazy=lazy, deep=deep)
    _assert_step_counts(tree, plain, pending)
    assert tree["n_after_read"] == 0
    LC._assert_same_bits(tree, plain)
    if LC._counts_apply():
        assert tree["n_bytes"] == 130 * ((62 if lazy == "0" else 30) * 132 + 64), tree["n_bytes"]
    assert_results_match(_first_result(tree, exp), exp, what="subtrees-switch")


def test_default_at_the_threshold(amd_lib, monkeypatch):
    """20 000 sites, no switch set: the tree launch is used by size and so is its deep form"""
    sites = 20000
    case = W.make_case("lazy-threshold", 4, LC.TIPS, sites, seed=5, ambiguity_pct=3, partial_pct=2)

    def seq(s, out):
        for _ in range(3):
            LC._step(s, case, out)
        op = _ops_at(case, 2)[0]
        out["one_level_2"], out["one_level_2_scaler"] = s.read_clv(op[0]), s.read_scaler(op[1], op[0])
        out["n_after_read"] = s.pending_clvs()

    tree = _run(amd_lib, case, monkeypatch, seq, None, deep=None)
    plain = _run(amd_lib, case, monkeypatch, seq, "0", deep=None)
    _assert_step_counts(tree, plain, _policy(3))
    assert tree["n_after_read"] == 0
    LC._assert_same_bits(tree, plain)
    assert tree["lnl"][0] == tree["lnl"][1] == tree["lnl"][2]
    if LC._counts_apply():
        assert tree["n_bytes"] == sites * (6 * 132 + 64), tree["n_bytes"]


def test_closing_with_56_pending(amd_lib, monkeypatch):
    case, exp = LC._case_and_oracle(65, ambiguity_pct=3, partial_pct=2)
    monkeypatch.setenv(TREE, "1")
    monkeypatch.setenv(DEEP, "1")
    monkeypatch.delenv(LAZY, raising=False)
    for _ in range(2):  # ... and the next session starts clean
        s = driver.Session(amd_lib, case, api.ARCH_AVX2)
        try:
            assert s.pending_clvs() == 0
            for _ in range(2):
                s.update_partials()
                v = s.edge_lnl(case.edges[0], persite=False)[0]
            if LC._counts_apply():
                assert s.pending_clvs() == GROUP_OPS
                assert s.lib.pll_gpu_last_launch_count(s.p) == 1  # nothing was stored on the way
        finally:
            s.close()
        assert abs(v - exp["lnl"][0]) <= RTOL * abs(exp["lnl"][0])
