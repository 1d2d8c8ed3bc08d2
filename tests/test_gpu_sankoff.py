"""GPU: weighted (Sankoff) parsimony on the device against the reference's recorded results (tests/golden/sankoff.json),
the NumPy restatement pllamd.sankoff_cases.Model (pinned to the same file by tests/test_sankoff_host.py) and, where it is
built, the live reference.

Tolerances. Score buffers: none - add and min do not depend on the order of evaluation. Scores under `unit` / `tv`: none
- every term is an integer below 2^53. Scores under `real`: |got - ref| <= sites * 2^-52 * ref - both sides add the
same `sites` non-negative terms in different orders, each order's rounding error is at most (sites - 1) * 2^-53 of the
sum."""
import functools
import os

import numpy as np
import pytest

from pllamd import api, sankoff_cases as SC
import sankoff_common as K

pytestmark = pytest.mark.gpu

GOLDEN = K.golden()
# (8,0,1) | (9,8,2) | (8,8,3) | (10,9,8) | (9,4,5) | (11,9,10) | (11,11,6) | (12,11,8) | (8,12,8): parents that are their
# own children, buffers rewritten after they were read, a parent written twice - every entry depends on the one before
HAZARD_LIST = [(8, 0, 1), (9, 8, 2), (8, 8, 3), (10, 9, 8), (9, 4, 5), (11, 9, 10), (11, 11, 6), (12, 11, 8), (8, 12, 8)]
LIST_CASES = [("dna_8x65", "real"), ("aa_33x130", "real"), ("s64_8x65", "unit"), ("s5_12x130", "real")]
RECONSTRUCT_STATS_CASES = [("dna_16x300_balanced", "unit"), ("dna_16x300_balanced", "tv"), ("dna_16x300_balanced", "real"),
                           ("aa_33x130", "real")]


@pytest.fixture(scope="module")
def ref_or_none():
    p = os.path.join(K.ROOT, "oracle", "_ref", "libpll_ref.so")
    return api.PllLib(p) if os.path.exists(p) else None


@functools.lru_cache(maxsize=None)
def _built_model(case_name, mname):
    """the Model after set tips + build + reconstruct + the insertion tree's vectors; computed once, never modified"""
    lib = api.PllLib()
    case = SC.BY_NAME[case_name]
    model, cmap = K.model(lib, case, mname)
    ops, root = SC.tree_ops(case)
    score = model.build(ops)
    stats = [0, 0]
    model.reconstruct(cmap, SC.reconstruct_ops(ops, root, case.tips), stats)
    dops, edges = K.insertion_tree(case)
    model.build(dops)
    ins = [model.insertion_score(case.tips - 1, a, b) for a, b in edges]
    return model, score, stats, ins


def _close(got, ref, case, mname):
    """the bound of the module docstring; the figures go to the log first"""
    bound = 0.0 if mname in ("unit", "tv") else case.sites * 2.0 ** -52 * abs(ref)
    print(f"{case.name}-{mname}: got {got!r} ref {ref!r} |diff| {abs(got - ref):.3e} bound {bound:.3e}")
    return abs(got - ref) <= bound


def _hazard_list(case):
    """HAZARD_LIST (written for 8 tips) with its inner indices moved behind the case's tips"""
    return [tuple(i if i < 8 else i - 8 + case.tips for i in op) for op in HAZARD_LIST]


def _crcs(s, indices):
    return [SC.crc(s.buffer(i), "<f8") for i in indices]


# ---- 1. golden sweep, 2. the score ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mname", SC.CASE_MATRICES, ids=SC.CASE_MATRIX_IDS)
def test_buffers_and_score_equal_the_reference(amd_lib, case, mname):
    exp = GOLDEN[case.name][mname]
    ops, root = SC.tree_ops(case)
    with K.session(amd_lib, case, mname) as s:
        K.set_tips(s, amd_lib, case)
        score = s.build(ops)
        assert s.launches() == SC.levels(ops) + 1  # one launch per level and the score
        assert s.score(root) == score and s.launches() == 1  # same bits from run to run
        # the host mirror is lazy: parents are still zero there
        assert not s.buffer(root).any()
        s.sync(-1)
        assert {str(p): SC.crc(s.buffer(p), "<f8") for p, _, _ in ops} == exp["buffer_crc"]
        assert _crcs(s, range(case.tips)) == exp["tip_crc"]  # tips come back as they went up
        assert not s.buffer(case.spare[0]).any()
        assert _close(score, float.fromhex(exp["score"]), case, mname)


# ---- 3. list semantics -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mname", LIST_CASES)
def test_list_equals_in_order_execution(amd_lib, name, mname):
    case = SC.BY_NAME[name]
    ops = _hazard_list(case)
    written = sorted({p for p, _, _ in ops})
    model, _ = K.model(amd_lib, case, mname)
    ref_score = model.build(ops)
    with K.session(amd_lib, case, mname) as s, K.session(amd_lib, case, mname) as t:
        K.set_tips(s, amd_lib, case)
        K.set_tips(t, amd_lib, case)
        score = s.build(ops)
        assert s.launches() == len(ops) + 1  # every entry waits for the one before
        s.sync(-1)
        for n in written:
            assert (s.buffer(n) == model.sb[n]).all(), n
        assert _close(score, ref_score, case, mname)
        # one call equals one call per operation, bit for bit
        assert t.build(ops, per_op=True) == score
        t.sync(-1)
        for n in written:
            assert (t.buffer(n) == s.buffer(n)).all(), n
        # two independent cherries and a self-referencing entry that waits for neither: two levels
        top = case.tips
        assert s.build([(top, 0, 1), (top + 1, 2, 3), (top + 2, top + 2, 4), (top + 3, top, top + 1)]) > 0 and s.launches() == 3


# ---- 4. reconstruct --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mname", SC.CASE_MATRICES, ids=SC.CASE_MATRIX_IDS)
def test_reconstruct_equals_the_reference(amd_lib, case, mname):
    exp = GOLDEN[case.name][mname]
    ops, root = SC.tree_ops(case)
    rows = SC.reconstruct_ops(ops, root, case.tips)
    with K.session(amd_lib, case, mname) as s:
        cmap = K.set_tips(s, amd_lib, case)
        s.build(ops)
        s.reconstruct(cmap, rows)
        assert s.launches() == SC.levels(ops)  # the tree's depth: a node waits for its parent alone
        # anc_states is the call's result: no sync
        got = {p: s.ancestral(p) for p, _, _ in ops}
        assert {str(p): SC.crc(a, "<u4") for p, a in got.items()} == exp["anc_crc"]
    # split over two calls: the second reads what the first assigned
    with K.session(amd_lib, case, mname) as s:
        cmap = K.set_tips(s, amd_lib, case)
        s.build(ops)
        half = max(1, len(rows) // 2)
        s.reconstruct(cmap, rows[:half])
        if rows[half:]:
            # the second call's first row reads no parent in the reference: lead with the root's row again
            s.reconstruct(cmap, rows[:1] + rows[half:])
        assert all((s.ancestral(p) == got[p]).all() for p in got)


@pytest.mark.parametrize("name,mname", RECONSTRUCT_STATS_CASES)
def test_reconstruct_inputs_take_both_branches(amd_lib, name, mname):
    """a condition on the INPUTS, from the Model: the parent's character is kept, and the node's own first minimum
    taken, in at least a tenth of the (node, site) pairs each"""
    case = SC.BY_NAME[name]
    _, _, (kept, own), _ = _built_model(name, mname)
    print(f"{name}-{mname}: kept {kept} own {own}")
    assert kept + own == (case.tips - 2) * case.sites
    assert kept >= (kept + own) / 10 and own >= (kept + own) / 10
    # and the device takes them the way the Model does
    ops, root = SC.tree_ops(case)
    model = _built_model(name, mname)[0]
    with K.session(amd_lib, case, mname) as s:
        cmap = K.set_tips(s, amd_lib, case)
        s.build(ops)
        s.reconstruct(cmap, SC.reconstruct_ops(ops, root, case.tips))
        assert all((s.ancestral(p) == model.anc[p]).all() for p, _, _ in ops)


# ---- 5. insertion scores -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mname", SC.CASE_MATRICES, ids=SC.CASE_MATRIX_IDS)
def test_insertion_scores(amd_lib, ref_or_none, case, mname):
    exp = [float.fromhex(x) for x in GOLDEN[case.name][mname]["insertion_scores"]]
    _, _, _, ins = _built_model(case.name, mname)
    dops, edges = K.insertion_tree(case)
    node = case.tips - 1
    assert len(edges) == 2 * (case.tips - 1) - 3
    with K.session(amd_lib, case, mname) as s:
        K.set_tips(s, amd_lib, case)
        s.build(dops)
        s.sync(-1)
        before = _crcs(s, range(case.buffers))
        got = s.insertion_scores(node, edges)
        assert s.launches() == 1
        for g, m, e in zip(got, ins, exp):
            assert _close(float(g), m, case, mname) and _close(float(g), e, case, mname)
        # the same bits alone, among others and in reversed order
        assert (s.insertion_scores(node, edges[::-1])[::-1] == got).all()
        for i in (0, len(edges) // 2, len(edges) - 1):
            assert s.insertion_scores(node, [edges[i]])[0] == got[i]
        # equal to the two-operation build it is defined by, which needs the two spare buffers
        two = s.insertion_scores_per_edge(node, edges[:3], case.spare)
        assert all(_close(float(g), float(t), case, mname) for g, t in zip(got, two))
        out = np.full(1, 7.5)
        assert amd_lib.pll_gpu_parsimony_insertion_scores(s.pars, node, None, 0, api.dptr(out)) == 1 and s.launches() == 0 and out[0] == 7.5
        s.sync(-1)
        after = _crcs(s, range(case.buffers))
        assert after[:case.spare[0]] == before[:case.spare[0]]  # (the spares were written by the builds just above)
    if ref_or_none is not None:
        with K.session(ref_or_none, case, mname) as r:
            K.set_tips(r, ref_or_none, case)
            r.build(dops)
            live = r.insertion_scores_per_edge(node, edges, case.spare)
        assert all(_close(float(g), float(x), case, mname) for g, x in zip(got, live))


def test_insertion_scores_leave_every_buffer_alone(amd_lib):
    case = SC.BY_NAME["aa_33x130"]
    dops, edges = K.insertion_tree(case)
    with K.session(amd_lib, case, "real") as s:
        K.set_tips(s, amd_lib, case)
        s.build(dops)
        s.sync(-1)
        before = _crcs(s, range(case.buffers))
        s.insertion_scores(case.tips - 1, edges)
        s.sync(-1)
        assert _crcs(s, range(case.buffers)) == before


# ---- 6. tip replacement ------------------------------------------------------------------------------------------------
def test_a_tip_set_again_is_uploaded(amd_lib):
    case = SC.BY_NAME["dna_9x257_caterpillar"]
    ops, root = SC.tree_ops(case)
    model, cmap = K.model(amd_lib, case, "tv")
    with K.session(amd_lib, case, "tv") as s:
        K.set_tips(s, amd_lib, case)
        first = s.build(ops)
        assert first == model.build(ops)
        seq = SC.alignment(case)[3][::-1]
        assert s.set_sequence(3, cmap, seq) == 1
        model.set_sequence(3, cmap, seq)
        second = s.build(ops)
        assert second == model.build(ops) and second != first
        s.sync(-1)
        assert all((s.buffer(p) == model.sb[p]).all() for p, _, _ in ops)
        # a buffer the caller wrote directly goes up once it says so
        host = api.as_np(s.s.sbuffer[5], case.sites * 4, np.float64)
        host[:] = model.sb[4].ravel()
        model.sb[5] = model.sb[4]
        assert s.build(ops) == second  # not announced: the device still holds the old tip
        assert amd_lib.pll_gpu_parsimony_invalidate(s.pars, 5) == 1
        assert s.build(ops) == model.build(ops)


def test_eager_mirror_downloads_the_parents(amd_lib, monkeypatch):
    monkeypatch.setenv("PLL_AMD_EAGER_MIRROR", "1")
    case = SC.BY_NAME["dna_8x65"]
    ops, _ = SC.tree_ops(case)
    with K.session(amd_lib, case, "real") as s:
        K.set_tips(s, amd_lib, case)
        s.build(ops)
        assert {str(p): SC.crc(s.buffer(p), "<f8") for p, _, _ in ops} == GOLDEN[case.name]["real"]["buffer_crc"]


# ---- 7. failures -------------------------------------------------------------------------------------------------------
def test_failed_calls_launch_nothing_and_write_nothing(amd_lib):
    case = SC.BY_NAME["dna_8x65"]
    ops, root = SC.tree_ops(case)
    nbuf, hi = case.buffers, case.tips + case.ancestral_buffers
    with K.session(amd_lib, case, "unit") as s:
        cmap = K.set_tips(s, amd_lib, case)
        s.build(ops)
        s.reconstruct(cmap, SC.reconstruct_ops(ops, root, case.tips))
        s.sync(-1)
        before = _crcs(s, range(nbuf))
        anc = [s.ancestral(i) for i in range(case.tips, hi)]
        out = np.full(2, 7.5)
        e = np.array([0, 1, 2, nbuf], dtype=np.uint32)
        calls = [
            (lambda: s.build(ops + [(nbuf, 0, 1)]), -np.inf),
            (lambda: s.score(nbuf), -np.inf),
            (lambda: s.reconstruct(cmap, [(root, root, root, root), (8, hi, root, root)]), None),
            (lambda: amd_lib.pll_gpu_parsimony_insertion_scores(s.pars, 0, api.uptr(e), 2, api.dptr(out)), 0),
        ]
        for call, expect in calls:
            assert s.score(root) > 0 and s.launches() == 1
            api.C.c_int.in_dll(amd_lib.dll, "pll_errno").value = 0
            assert call() == expect
            assert amd_lib.errno() == api.ERROR_PARAM_INVALID and s.launches() == 0
        s.sync(-1)
        assert _crcs(s, range(nbuf)) == before and (out == 7.5).all()
        assert all((s.ancestral(case.tips + i) == a).all() for i, a in enumerate(anc))
