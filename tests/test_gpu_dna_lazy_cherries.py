"""Lazy cherries: the whole-traversal launch of a balanced 64-taxon DNA tree (kernels_dna.h: k_edge_dna_tree, forced here
with PLL_AMD_FUSE_TREE=1) leaves the 32 tip x tip parents UNSTORED (PLL_AMD_LAZY_CHERRIES, default on); the device layer
keeps them as pending and stores them in one launch before anything reads them, overwrites them or changes their codes
(pllgpu.hip: materialise_pending); a change of a matrix they read only makes them keep the old one aside
(keep_pending_matrices). pll_gpu_pending_clvs says how many are unstored.

The yardstick everywhere is the ordinary route (PLL_AMD_FUSE_TREE=0) driven through the SAME call sequence, bit for bit,
plus the oracle within RTOL as tests/test_gpu_dna_tree.py has it."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from compare import RTOL, assert_results_match, scalers_equal
from oracle import oracle as O
from pllamd import api, driver, workload as W

pytestmark = pytest.mark.gpu

TREE, LAZY = "PLL_AMD_FUSE_TREE", "PLL_AMD_LAZY_CHERRIES"
TIPS = 64
CHERRIES = 32
SIZES = [1, 65, 130]  # one lane; a tile and one; three tiles, the last ragged


def _counts_apply():
    """eager mirroring reads every CLV back right after the traversal and dense tips have no seven-op groups: nothing is
    held, nothing is left pending"""
    return all(os.environ.get(v, "0") in ("", "0") for v in ("PLL_AMD_EAGER_MIRROR", "PLL_AMD_NO_TIP_CODES", "PLL_AMD_NO_TAIL_FUSION",
                                                              "PLL_AMD_NO_FUSE", "PLL_AMD_NO_FUSE_CC", "PLL_AMD_NO_CHAINS"))


@functools.lru_cache(maxsize=None)
def _case_and_oracle(sites, seed=5, **kw):
    case = W.make_case("lazy", 4, TIPS, sites, seed=seed, **kw)
    return case, O.run_case(case)


def _cherry_ops(case):
    ops = [op for op in case.op_batches[0] if op[2] < TIPS and op[5] < TIPS]
    assert len(ops) == CHERRIES
    return ops


def _read_all(s, case, out):
    out["clv"], out["scaler"] = {}, {}
    for op in case.op_batches[0]:
        out["clv"][op[0]] = s.read_clv(op[0])
        if op[1] >= 0:
            out["scaler"][op[0]] = s.read_scaler(op[1], op[0])


def _step(s, case, out, persite=True):
    """traversal, then DIRECTLY the evaluation of the root edge; the launch counts after the two calls and what is pending"""
    lib = s.lib
    s.update_partials()
    held = lib.pll_gpu_last_launch_count(s.p)
    out["n_bytes"] = lib.pll_gpu_last_algorithmic_bytes(s.p)
    v, ps = s.edge_lnl(case.edges[0], persite=persite)
    out.setdefault("n_launches", []).append((held, lib.pll_gpu_last_launch_count(s.p)))
    out.setdefault("n_pending", []).append(s.pending_clvs())
    out.setdefault("lnl", []).append(v)
    if persite:
        out.setdefault("persite", []).append(ps)


def _run(lib, case, monkeypatch, seq, tree, lazy=None):
    monkeypatch.setenv(TREE, tree)
    if lazy is None:
        monkeypatch.delenv(LAZY, raising=False)  # the default: on wherever the tree launch is used
    else:
        monkeypatch.setenv(LAZY, lazy)
    out = {"persite": [], "root_lnl": [], "root_persite": []}
    with driver.Session(lib, case, api.ARCH_AVX2) as s:
        seq(s, out)
    return out


def _both(lib, case, monkeypatch, seq):
    """the same call sequence through the lean tree launch and through the ordinary route"""
    return _run(lib, case, monkeypatch, seq, "1"), _run(lib, case, monkeypatch, seq, "0")


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b))


def _assert_same_bits(tree, plain):
    """everything observed but the counts (keys n_*)"""
    assert set(tree) == set(plain)
    for k in plain:
        if not k.startswith("n_"):
            assert _same(tree[k], plain[k]), k
    if "clv" in plain:
        assert len(plain["clv"]) == 62


def _assert_step_counts(tree, plain, steps=1, pending=CHERRIES):
    if not _counts_apply():
        return
    assert tree["n_launches"] == [(0, 1)] * steps, tree["n_launches"]  # the whole step is the evaluation's launch
    assert tree["n_pending"] == [pending] * steps, tree["n_pending"]
    assert plain["n_pending"] == [0] * steps, plain["n_pending"]


def _step_and_read_all(case, persite=True):
    def seq(s, out):
        _step(s, case, out, persite)
        first = _cherry_ops(case)[0]
        out["first_cherry"] = s.read_clv(first[0])
        out["n_after_read"] = s.pending_clvs()  # the first read of a cherry stores all of them
        _read_all(s, case, out)
    return seq


# ---- bits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sites", SIZES)
def test_every_clv_and_scaler_after_a_step(amd_lib, monkeypatch, sites):
    case, exp = _case_and_oracle(sites, ambiguity_pct=3, partial_pct=2)
    tree, plain = _both(amd_lib, case, monkeypatch, _step_and_read_all(case))
    _assert_step_counts(tree, plain)
    assert tree["n_after_read"] == 0
    _assert_same_bits(tree, plain)
    assert_results_match(tree, exp, what="lazy-%d" % sites)


@pytest.mark.parametrize("kw", [dict(brlen_scale=1e-7, mutate_pct=60),                                # levels 4 and 5 rescale
                                dict(brlen_scale=1e-6, mutate_pct=90, attributes=api.RATE_SCALERS)],  # per rate
                         ids=["short-branches", "rate-scalers"])
def test_scalers_of_the_cherries_are_stored_too(amd_lib, monkeypatch, kw):
    case, exp = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2, **kw)
    assert sum(int(v.sum()) for v in exp["scaler"].values()) > 0  # the input does scale
    tree, plain = _both(amd_lib, case, monkeypatch, _step_and_read_all(case))
    _assert_step_counts(tree, plain)
    _assert_same_bits(tree, plain)
    for op in _cherry_ops(case):
        assert op[0] in tree["scaler"]
    assert_results_match(tree, exp, what="lazy-scaling")
    assert scalers_equal(tree, exp)


def test_ascertainment_bias_entries_of_the_cherries(amd_lib, monkeypatch):
    """130 sites + 4 per-state entries behind them: stored on demand like the sites"""
    case, exp = _case_and_oracle(130, seed=9, ambiguity_pct=3, asc_type=1)
    tree, plain = _both(amd_lib, case, monkeypatch, _step_and_read_all(case))
    _assert_step_counts(tree, plain)
    _assert_same_bits(tree, plain)
    for a in tree["clv"].values():
        assert a.shape[0] == 134
    assert_results_match(tree, exp, what="lazy-asc")
    assert scalers_equal(tree, exp)


# ---- steady state -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sites", SIZES)
def test_three_steps_in_a_row(amd_lib, monkeypatch, sites):
    """the kept plan's own list again recomputes all 32: nothing is stored between the steps"""
    case, exp = _case_and_oracle(sites, ambiguity_pct=3, partial_pct=2)

    def seq(s, out):
        for _ in range(3):
            _step(s, case, out)
        out["first_cherry"] = s.read_clv(_cherry_ops(case)[0][0])
        out["n_after_read"] = s.pending_clvs()
        _read_all(s, case, out)

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, steps=3)
    assert tree["n_after_read"] == 0
    _assert_same_bits(tree, plain)
    assert tree["lnl"][0] == tree["lnl"][1] == tree["lnl"][2]
    assert abs(tree["lnl"][2] - exp["lnl"][0]) <= RTOL * abs(exp["lnl"][0])
    if _counts_apply():
        # what the launch really stores: 30 CLVs + scalers out, 64 code bytes in, per entry; the ordinary route's figure
        # for the same list is larger (every CLV out, the group parents read back)
        assert tree["n_bytes"] == sites * (30 * 132 + 64), tree["n_bytes"]
        assert plain["n_bytes"] > sites * (62 * 132 + 64)


# ---- what keeps the cherries pending --------------------------------------------------------------------------------------
def test_calls_that_keep_them_pending(amd_lib, monkeypatch):
    """a wait for the stream, an upload of the evaluated edge's own matrix, a second (per-site) evaluation of the root edge:
    none reads a cherry or changes what it is a function of"""
    case, exp = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    e = case.edges[0]

    def seq(s, out):
        lib = s.lib
        _step(s, case, out, persite=False)
        pend = []
        assert lib.pll_gpu_synchronize(s.p)
        pend.append(s.pending_clvs())
        v, ps = s.edge_lnl(e, persite=True)                       # the second evaluation, per site
        out["again"], out["again_persite"] = v, ps
        pend.append(s.pending_clvs())
        # the edge's own matrix is rewritten on the host and goes up with the next evaluation
        n = case.rate_cats * 4 * s.sp
        api.as_np(s.part.pmatrix[e[4]], n, np.float64)[:] = api.as_np(s.part.pmatrix[3], n, np.float64)
        lib.pll_gpu_invalidate(s.p, api.DIRTY_PMATRIX, e[4])
        out["moved"] = s.edge_lnl(e, persite=False)[0]
        pend.append(s.pending_clvs())
        out["n_pend"] = pend
        _read_all(s, case, out)
        out["n_end"] = s.pending_clvs()

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain)
    if _counts_apply():
        assert tree["n_pend"] == [CHERRIES] * 3, tree["n_pend"]
    assert tree["n_end"] == 0
    _assert_same_bits(tree, plain)
    assert tree["again"] == tree["lnl"][0] and tree["moved"] != tree["lnl"][0]
    assert_results_match(dict(tree, lnl=tree["lnl"][:1], persite=[tree["again_persite"]]), exp, what="lazy-kept")


def _form_matrices(s, case, indices, lengths):
    pi = np.zeros(case.rate_cats, dtype=np.uint32)
    mi = np.ascontiguousarray(indices, dtype=np.uint32)
    bl = np.ascontiguousarray(lengths, dtype=np.float64)
    assert s.lib.pll_update_prob_matrices(s.p, api.uptr(pi), api.uptr(mi), api.dptr(bl), len(mi))


def test_matrices_formed_on_the_device_keep_them_pending(amd_lib, monkeypatch):
    """pll_update_prob_matrices after a step - of the evaluated edge's own matrix (a branch-length pass: new matrix, sumtable,
    derivatives, evaluation), then of EVERY matrix (what a model-parameter loop does before its next traversal) - stores
    nothing: the cherries keep the matrices of the step aside, and a read afterwards still gives the values of the step"""
    case, _ = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    e = case.edges[0]
    nmat = case.prob_matrices
    brlen = W.branch_lengths(nmat)

    def seq(s, out):
        s.set_model(case.model["exch"], case.freqs, case.model["rates"])
        _form_matrices(s, case, np.arange(nmat), brlen)
        _step(s, case, out, persite=False)
        pend = []
        _form_matrices(s, case, [e[4]], [brlen[e[4]] * 2.0])          # the edge's own matrix
        pend.append(s.pending_clvs())
        edge = (e[0], e[1], e[2], e[3])
        st = s.new_sumtable()
        s.update_sumtable(edge, st)                                    # neither end of the root edge is a cherry
        out["derivatives"] = s.derivatives(edge, st, 0.13)
        pend.append(s.pending_clvs())
        out["moved"] = s.edge_lnl(e, persite=False)[0]
        pend.append(s.pending_clvs())
        _form_matrices(s, case, np.arange(nmat), brlen * 1.5)          # every matrix, those of the cherries among them
        pend.append(s.pending_clvs())
        out["n_pend"] = pend
        _read_all(s, case, out)                                        # ... the CLVs of the step, from the matrices of the step
        out["n_end"] = s.pending_clvs()
        _step(s, case, out, persite=False)                             # ... and the next step reads the new ones

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, steps=2)
    if _counts_apply():
        assert tree["n_pend"] == [CHERRIES] * 4, tree["n_pend"]
    assert tree["n_end"] == 0
    _assert_same_bits(tree, plain)
    assert tree["moved"] != tree["lnl"][0] and tree["lnl"][1] != tree["lnl"][0]


def test_newton_that_writes_a_matrix_a_cherry_reads(amd_lib, monkeypatch):
    """a sumtable at a cherry edge, a step, then pll_gpu_optimize_branch_length with matrix_index = a matrix a cherry reads:
    the call forms that matrix anew on the device and stores nothing - the cherries read afterwards are those of the step,
    from the old matrix, and the next step reads the new one"""
    case, _ = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    nmat = case.prob_matrices
    cherries = _cherry_ops(case)
    a, b = cherries[0], cherries[1]
    edge, m = (a[0], a[1], b[0], b[1]), a[3]

    def seq(s, out):
        s.set_model(case.model["exch"], case.freqs, case.model["rates"])
        _form_matrices(s, case, np.arange(nmat), W.branch_lengths(nmat))
        _step(s, case, out, persite=False)
        st = s.new_sumtable()
        s.update_sumtable(edge, st)                                    # (stores the cherries: both ends are cherry parents)
        out["n_table"] = s.pending_clvs()
        _step(s, case, out, persite=False)                             # pending again
        res, trace = s.optimize_branch(edge, st, 0.1, t_min=1e-6, t_max=100.0, tolerance=1e-9, matrix_index=m)
        out["newton"] = (res.t, trace)
        out["n_newton"] = s.pending_clvs()
        for name, op in (("first", a), ("last", cherries[-1])):
            out[name] = s.read_clv(op[0])
            out[name + "_scaler"] = s.read_scaler(op[1], op[0])
        out["n_end"] = s.pending_clvs()
        _step(s, case, out, persite=False)
        # ... and the same write while a traversal is still held: it goes out without the cherry stores, then the matrix moves
        s.update_partials()
        res, trace = s.optimize_branch(edge, st, 0.3, t_min=1e-6, t_max=100.0, tolerance=1e-9, max_iters=1, matrix_index=m)
        out["newton_held"] = (res.t, trace)
        out["n_held"] = s.pending_clvs()
        out["held_first"] = s.read_clv(a[0])
        out["held_edge"] = s.edge_lnl(case.edges[0], persite=False)[0]

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, steps=3)
    if _counts_apply():
        assert (tree["n_table"], tree["n_newton"], tree["n_held"]) == (0, CHERRIES, CHERRIES)
    assert tree["newton_held"][0] != tree["newton"][0]
    assert tree["n_end"] == 0
    _assert_same_bits(tree, plain)
    assert tree["lnl"][0] == tree["lnl"][1] != tree["lnl"][2]          # the matrix did move


def test_a_model_parameter_loop_stores_nothing(amd_lib, monkeypatch):
    """new category rates, every matrix formed again, full traversal, root-edge evaluation - three times: the cherries are
    pending all the way through and never stored; each step equals the ordinary route's, and so does everything read at
    the end"""
    case, _ = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    nmat = case.prob_matrices
    brlen = W.branch_lengths(nmat)
    rates = np.asarray(case.model["rates"], dtype=np.float64)

    def seq(s, out):
        pend = []
        for k in range(3):
            s.set_model(case.model["exch"], case.freqs, rates * (1.0 + 0.25 * k))
            pend.append(s.pending_clvs())
            _form_matrices(s, case, np.arange(nmat), brlen)
            pend.append(s.pending_clvs())
            _step(s, case, out, persite=False)
        out["n_pend"] = pend
        _read_all(s, case, out)
        out["n_end"] = s.pending_clvs()

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain, steps=3)
    if _counts_apply():
        assert tree["n_pend"] == [0, 0] + [CHERRIES] * 4, tree["n_pend"]
    assert tree["n_end"] == 0
    _assert_same_bits(tree, plain)
    assert len(set(tree["lnl"])) == 3


def test_a_wait_between_the_traversal_and_the_evaluation(amd_lib, monkeypatch):
    """pll_gpu_synchronize sends the held traversal out as the ordinary launches; it reads no CLV, so the tip x tip parents stay
    unstored there too, and the evaluation that follows finds its two ends in memory"""
    case, exp = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)

    def seq(s, out):
        s.update_partials()
        assert s.lib.pll_gpu_synchronize(s.p)
        out["n_sync"] = (s.lib.pll_gpu_last_launch_count(s.p), s.pending_clvs(), s.lib.pll_gpu_last_algorithmic_bytes(s.p))
        v, ps = s.edge_lnl(case.edges[0], persite=True)
        out["lnl"], out["persite"] = [v], [ps]
        out["n_eval"] = s.pending_clvs()
        _read_all(s, case, out)
        out["n_end"] = s.pending_clvs()

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    if _counts_apply():
        # the seven-op groups and the two chains: 30 CLVs + scalers out, 64 code bytes in, the 8 group parents read back
        assert tree["n_sync"] == (2, CHERRIES, 130 * (30 * 132 + 64 + 8 * 132)), tree["n_sync"]
        assert plain["n_sync"][:2] == (2, 0) and plain["n_sync"][2] == tree["n_sync"][2] + 130 * CHERRIES * 132
        assert tree["n_eval"] == CHERRIES
    assert tree["n_end"] == 0
    _assert_same_bits(tree, plain)
    assert_results_match(tree, exp, what="lazy-wait")


# ---- what stores them, with the inputs of the step (a new matrix: at the read that follows it) ------------------------------
def _dirty_cherry_matrix(s, case, out):
    """a matrix a cherry reads is rewritten on the host and goes up with an evaluation that uses it"""
    e, m = case.edges[0], _cherry_ops(case)[0][3]
    n = case.rate_cats * 4 * s.sp
    api.as_np(s.part.pmatrix[m], n, np.float64)[:] = api.as_np(s.part.pmatrix[e[4]], n, np.float64)
    s.lib.pll_gpu_invalidate(s.p, api.DIRTY_PMATRIX, m)
    out["value"] = s.edge_lnl((e[0], e[1], e[2], e[3], m), persite=False)[0]


def _new_tip_codes(s, case, out):
    tip = _cherry_ops(case)[0][2]
    cmap = (C.c_ulonglong * 256)(*[int(x) for x in case.charmap])
    assert s.lib.pll_set_tip_states(s.p, tip, cmap, bytes(reversed(case.sequences[tip])))
    out["value"] = 0.0


def _inner_ops_as_another_list(s, case, out):
    inner = [op for op in case.op_batches[0] if op[2] >= TIPS and op[5] >= TIPS]
    assert len(inner) == 30
    s.lib.pll_update_partials(s.p, api.make_ops(inner), 30)
    out["value"] = s.edge_lnl(case.edges[0], persite=False)[0]


def _derivatives_at_a_cherry_edge(s, case, out):
    a, b = _cherry_ops(case)[0], _cherry_ops(case)[1]
    edge = (a[0], a[1], b[0], b[1])
    st = s.new_sumtable()
    s.update_sumtable(edge, st)
    out["value"] = s.derivatives(edge, st, 0.13)
    out["sumtable"] = s.read_sumtable(st)


def _edge_from_a_cherry_parent_to_a_tip(s, case, out):
    a = _cherry_ops(case)[0]
    out["value"], out["value_persite"] = s.edge_lnl((a[0], a[1], 5, -1, 5), persite=True)


def _root_at_a_cherry_parent(s, case, out):
    a = _cherry_ops(case)[0]
    out["value"], out["value_persite"] = s.root_lnl((a[0], a[1]), persite=True)


@pytest.mark.parametrize("action", [_dirty_cherry_matrix, _new_tip_codes, _inner_ops_as_another_list, _derivatives_at_a_cherry_edge,
                                    _edge_from_a_cherry_parent_to_a_tip, _root_at_a_cherry_parent],
                         ids=["cherry-matrix-upload", "tip-codes", "another-list", "derivatives", "edge-at-a-cherry", "root-at-a-cherry"])
def test_calls_that_store_them_first(amd_lib, monkeypatch, action):
    """after a step, the action, then reads of cherry parents: what the ordinary route holds under the same sequence - the
    values of the step, formed from the matrices and codes of the step"""
    case, _ = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    cherries = _cherry_ops(case)

    def seq(s, out):
        s.set_model(case.model["exch"], case.freqs, case.model["rates"])  # (the derivatives want an eigensystem)
        _step(s, case, out, persite=False)
        action(s, case, out)
        for name, op in (("first", cherries[0]), ("last", cherries[-1])):
            out[name] = s.read_clv(op[0])
            out[name + "_scaler"] = s.read_scaler(op[1], op[0])
        out["n_end"] = s.pending_clvs()
        # ... and the tree goes on from there
        s.update_partials()
        out["next"] = s.edge_lnl(case.edges[0], persite=False)[0]

    tree, plain = _both(amd_lib, case, monkeypatch, seq)
    _assert_step_counts(tree, plain)
    assert tree["n_end"] == 0
    _assert_same_bits(tree, plain)
    assert np.all(np.isfinite(np.asarray(tree["value"])))


# ---- the switch, and the end ----------------------------------------------------------------------------------------------
def test_switched_off_everything_is_stored(amd_lib, monkeypatch):
    case, exp = _case_and_oracle(130, ambiguity_pct=3, partial_pct=2)
    seq = _step_and_read_all(case)
    off = _run(amd_lib, case, monkeypatch, seq, "1", lazy="0")
    plain = _run(amd_lib, case, monkeypatch, seq, "0", lazy="0")
    _assert_step_counts(off, plain, pending=0)
    assert off["n_after_read"] == 0
    _assert_same_bits(off, plain)
    if _counts_apply():
        assert off["n_bytes"] == 130 * (62 * 132 + 64)
    assert_results_match(off, exp, what="lazy-off")


def test_closing_with_cherries_pending(amd_lib, monkeypatch):
    case, exp = _case_and_oracle(65, ambiguity_pct=3, partial_pct=2)
    monkeypatch.setenv(TREE, "1")
    monkeypatch.delenv(LAZY, raising=False)
    for _ in range(2):  # ... and the next session starts clean
        s = driver.Session(amd_lib, case, api.ARCH_AVX2)
        try:
            assert s.pending_clvs() == 0
            s.update_partials()
            v = s.edge_lnl(case.edges[0], persite=False)[0]
            if _counts_apply():
                assert s.pending_clvs() == CHERRIES
        finally:
            s.close()
        assert abs(v - exp["lnl"][0]) <= RTOL * abs(exp["lnl"][0])
