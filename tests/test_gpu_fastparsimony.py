"""GPU: bit-parallel Fitch parsimony (pll_fastparsimony_*, pll_gpu_fastparsimony_*) against the reference.

Every comparison is exact integer equality; there is no tolerance anywhere. Expected values come from
tests/golden/fastparsimony.json (written by the reference build, tools/gen_fastparsimony_golden.py) and, for operation
lists the file does not hold, from pllamd.parsimony_cases.Model - a NumPy restatement of the reference's loops that
tests/test_fastparsimony_host.py pins to the same file - and from the reference library itself wherever it has been
built (oracle/_ref/libpll_ref.so)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from pllamd import api, driver, parsimony_cases as PC
from utree import Rec, UTree, link

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fastparsimony.json")))
CASE_SETS = [(c, label, attrs) for c in PC.CASES for label, attrs in PC.attribute_sets(c)]
CASE_SET_IDS = [f"{c.name}-{label}" for c, label, _ in CASE_SETS]


@pytest.fixture(scope="module")
def ref_or_none():
    """the reference library where it has been built, else None: the golden file and the model always apply"""
    p = os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so")
    return api.PllLib(p) if os.path.exists(p) else None


def _session(lib, case, attrs=api.PATTERN_TIP):
    seqs, weights = PC.alignment(case)
    return driver.ParsimonySession(lib, case.states, seqs, PC.charmap(lib, case), weights, attrs)


def _model(session, case):
    """the NumPy restatement, started from the session's (reference-checked) tip vectors"""
    return PC.Model([session.vector(t) for t in range(case.tips)], case.nodes, session.s.const_cost)


def _insertion_tree(case):
    return UTree(case.tips - 1, np.random.default_rng(case.seed + 1000))


# ---- 1. golden sweep ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,label,attrs", CASE_SETS, ids=CASE_SET_IDS)
def test_golden_sweep(amd_lib, ref_or_none, case, label, attrs):
    exp = GOLDEN[case.name][label]
    ops, edge = PC.traversal(case)
    with _session(amd_lib, case, attrs) as s:
        st = s.s
        assert (st.packedvector_count, st.const_cost, st.informative_count) == (exp["packedvector_count"], exp["const_cost"], exp["informative_count"])
        assert PC.informative_string(s.informative()) == exp["informative"]
        assert [PC.crc(s.vector(t)) for t in range(case.tips)] == exp["tip_crc"]
        s.update(ops)
        assert s.edge_score(*edge) == exp["edge_score"]
        assert s.root_score(edge[0]) == exp["root_score"]
        s.sync(-1)
        assert [int(x) for x in s.costs()[:case.tips + len(ops)]] == exp["node_cost"]
        assert {str(p): PC.crc(s.vector(p)) for p, _, _ in ops} == exp["vector_crc"]
        assert [PC.crc(s.vector(t)) for t in range(case.tips)] == exp["tip_crc"]  # tips come back as they went up
        if ref_or_none is not None:
            with _session(ref_or_none, case, attrs) as r:
                r.update(ops)
                for p, _, _ in ops:
                    assert (s.vector(p) == r.vector(p)).all(), p
                assert (s.costs()[:case.tips + len(ops)] == r.costs()[:case.tips + len(ops)]).all()


# ---- 2. list semantics -------------------------------------------------------------------------------------------------
# parents that are their own children, vectors rewritten after an earlier entry read them, a parent written twice
HAZARD_LIST = [(8, 0, 1), (9, 8, 2), (8, 8, 3), (10, 9, 8), (9, 4, 5), (11, 9, 10), (11, 11, 6), (12, 11, 8), (8, 12, 8)]


def _hazard_list(case):
    """HAZARD_LIST (written for 8 tips) with its inner indices moved behind the case's tips"""
    return [tuple(i if i < 8 else i - 8 + case.tips for i in op) for op in HAZARD_LIST]


@pytest.mark.parametrize("name", ["dna_8x300_tail", "aa_8x64", "dna_16x3000_weights"])
def test_list_equals_in_order_execution(amd_lib, ref_or_none, name):
    case = PC.BY_NAME[name]
    ops = _hazard_list(case)
    top = case.tips
    with _session(amd_lib, case) as s:
        model = _model(s, case)
        model.update(ops)
        s.update(ops)  # (how many launches it takes: test_hazard_list_levels)
        s.sync(-1)
        written = sorted({p for p, _, _ in ops})
        for n in written:
            assert (s.vector(n) == model.vec[n]).all(), n
            assert int(s.costs()[n]) == int(model.cost[n]), n
        assert s.edge_score(top, 7) == model.edge_score(top, 7)
        if ref_or_none is not None:
            with _session(ref_or_none, case) as r:
                r.update(ops)
                for n in written:
                    assert (s.vector(n) == r.vector(n)).all(), n
                    assert int(s.costs()[n]) == int(r.costs()[n]), n
                assert s.edge_score(top, 7) == r.edge_score(top, 7)


@pytest.mark.parametrize("name", ["dna_9x40_weights_caterpillar", "aa_33x700_weights"])
def test_one_call_equals_one_call_per_operation(amd_lib, name):
    case = PC.BY_NAME[name]
    exp = GOLDEN[case.name]["tip"]
    ops, edge = PC.traversal(case)
    got = []
    for per_op in (False, True):
        with _session(amd_lib, case) as s:
            s.update(ops, per_op=per_op)
            s.sync(-1)
            got.append(([int(x) for x in s.costs()], [PC.crc(s.vector(n)) for n in range(s.nodes)], s.edge_score(*edge)))
    assert got[0] == got[1]
    assert got[0][0][:case.tips + len(ops)] == exp["node_cost"] and got[0][2] == exp["edge_score"]


# ---- 3. batched calls --------------------------------------------------------------------------------------------------
def test_batched_edge_scores_equal_per_call_scores(amd_lib):
    case = PC.BY_NAME["dna_8x300_tail"]
    ops, _ = PC.traversal(case)
    with _session(amd_lib, case) as s:
        s.update(ops)
        used = case.tips + len(ops)
        pairs = [(a, b) for a in range(used) for b in range(used)]
        batched = s.edge_scores(pairs)
        assert amd_lib.pll_gpu_fastparsimony_last_launch_count(s.pars) == 1
        model = _model(s, case)
        model.update(ops)
        assert [int(x) for x in batched] == [model.edge_score(a, b) for a, b in pairs]
        for i in range(0, len(pairs), 7):  # and the synchronous call, on a sample of them
            assert s.edge_score(*pairs[i]) == int(batched[i]), pairs[i]


@pytest.mark.parametrize("name", ["dna_9x40_weights_caterpillar", "aa_33x700_weights", "s61_12x200", "dna_16x3000_weights"])
def test_insertion_scores_equal_update_plus_edge_score(amd_lib, ref_or_none, name):
    case = PC.BY_NAME[name]
    exp = GOLDEN[case.name]["tip"]["insertion_scores"]
    node, spare = case.tips - 1, case.nodes - 1
    dops, edges = PC.directional_ops(_insertion_tree(case), case.tips)
    assert len(edges) == 2 * (case.tips - 1) - 3 and len(dops) == 3 * (case.tips - 3)
    with _session(amd_lib, case) as s:
        s.update(dops)
        batched = s.insertion_scores(node, edges)
        assert amd_lib.pll_gpu_fastparsimony_last_launch_count(s.pars) == 1
        assert [int(x) for x in batched] == exp
        # nothing was written but the scores: the per-edge pattern through a spare index gives the same numbers afterwards
        assert [int(x) for x in s.insertion_scores_per_edge(node, edges, spare)] == exp
        if ref_or_none is not None:
            with _session(ref_or_none, case) as r:
                r.update(dops)
                assert [int(x) for x in r.insertion_scores_per_edge(node, edges, spare)] == [int(x) for x in batched]


# ---- 4. stepwise addition ----------------------------------------------------------------------------------------------
class StepTree:
    """the tree of a stepwise addition: starts as tips 0, 1, 2 around one inner node; insert() hangs the next tip into an
    edge. Records as in utree.py; ring j keeps the score indices tips + 3 j .. + 2 (pllamd.parsimony_cases.record_index)."""

    def __init__(self, tips):
        self.tips, self._uid = tips, 0
        self.tip_recs = {}
        self.rings = []
        ring = self._ring()
        for k, r in enumerate(ring):
            link(r, self._tip(k), 0.0, 0)

    def _rec(self, clv):
        self._uid += 1
        return Rec(clv, -1, self._uid)

    def _tip(self, t):
        self.tip_recs[t] = self._rec(t)
        return self.tip_recs[t]

    def _ring(self):
        a, b, c = (self._rec(self.tips + len(self.rings)) for _ in range(3))
        a.next, b.next, c.next = b, c, a
        self.rings.append(a)
        return a, b, c

    def records(self):
        yield from self.tip_recs.values()
        for n in self.rings:
            yield from (n, n.next, n.next.next)

    def edges(self):
        return [r for r in self.records() if r.uid < r.back.uid]

    def insert(self, tip, r):
        rb = r.back
        ring = self._ring()
        link(ring[0], self._tip(tip), 0.0, 0)
        link(ring[1], r, 0.0, 0)
        link(ring[2], rb, 0.0, 0)


def _stepwise(case, update, insertion_scores, edge_score):
    """taxa in index order, every step: all directional vectors, the scores of all edges, the first minimum"""
    tree, chosen = StepTree(case.tips), []
    for tip in range(3, case.tips):
        dops, edges = PC.directional_ops(tree, case.tips)
        update(dops)
        scores = [int(x) for x in insertion_scores(tip, edges)]
        best = scores.index(min(scores))
        chosen.append((best, scores[best]))
        tree.insert(tip, tree.edges()[best])
    dops, edges = PC.directional_ops(tree, case.tips)
    update(dops)
    return chosen, edge_score(*edges[0])


def test_stepwise_addition(amd_lib, ref_or_none):
    case = PC.BY_NAME["dna_16x3000_weights"]
    spare = case.nodes - 1
    with _session(amd_lib, case) as s:
        got = _stepwise(case, s.update, s.insertion_scores, s.edge_score)
        model = _model(s, case)
    exp = _stepwise(case, model.update, lambda node, edges: [model.insertion_score(node, a, b) for a, b in edges], model.edge_score)
    assert got == exp
    assert got[1] == got[0][-1][1]  # the tree's score is the score the last insertion promised
    if ref_or_none is not None:
        with _session(ref_or_none, case) as r:
            assert got == _stepwise(case, r.update, lambda node, edges: r.insertion_scores_per_edge(node, edges, spare), r.edge_score)


# ---- 5. launch accounting ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dna_9x40_weights_caterpillar", "aa_33x700_weights", "dna_16x3000_weights", "s61_12x200"])
def test_one_launch_per_dependency_level(amd_lib, name):
    case = PC.BY_NAME[name]
    ops, edge = PC.traversal(case)
    with _session(amd_lib, case) as s:
        assert s.update(ops) == PC.chain_depth(ops)
        assert s.update(ops, per_op=True) == len(ops)
        s.edge_score(*edge)
        assert amd_lib.pll_gpu_fastparsimony_last_launch_count(s.pars) == 1
        s.root_score(edge[0])
        assert amd_lib.pll_gpu_fastparsimony_last_launch_count(s.pars) == 0
        dops, edges = PC.directional_ops(_insertion_tree(case), case.tips)
        # three orientations per inner node: the deepest chain of the tree, still one launch per level
        assert s.update(dops) == PC.chain_depth(dops)
        s.edge_scores(edges)
        assert amd_lib.pll_gpu_fastparsimony_last_launch_count(s.pars) == 1
        s.insertion_scores(case.tips - 1, edges)
        assert amd_lib.pll_gpu_fastparsimony_last_launch_count(s.pars) == 1


def test_hazard_list_levels(amd_lib):
    """HAZARD_LIST in order: (8,0,1) | (9,8,2) | (8,8,3) | (10,9,8) | (9,4,5) | (11,9,10) | (11,11,6) | (12,11,8) | (8,12,8):
    every entry depends on the one before through a read-after-write, a write-after-read or a write-after-write"""
    case = PC.BY_NAME["dna_8x300_tail"]
    with _session(amd_lib, case) as s:
        assert s.update(HAZARD_LIST) == len(HAZARD_LIST)
        # two independent cherries and a self-referencing entry that waits for neither: two levels
        assert s.update([(8, 0, 1), (9, 2, 3), (10, 10, 4), (11, 8, 9)]) == 2


# ---- 6. independence from the partition ----------------------------------------------------------------------------------
def test_structure_outlives_its_partition(amd_lib):
    case = PC.BY_NAME["dna_8x300_tail"]
    exp = GOLDEN[case.name]["tip"]
    ops, edge = PC.traversal(case)
    with _session(amd_lib, case) as s:
        s.drop_partition()
        s.update(ops)
        assert s.edge_score(*edge) == exp["edge_score"] and s.root_score(edge[0]) == exp["root_score"]
        s.sync(-1)
        assert [int(x) for x in s.costs()[:case.tips + len(ops)]] == exp["node_cost"]


# ---- 7. error paths ----------------------------------------------------------------------------------------------------
def test_error_paths(amd_lib):
    case = PC.BY_NAME["s61_12x200"]
    seqs, _ = PC.alignment(case)
    with pytest.raises(RuntimeError, match=r"\[129\] Use PLL_ATTRIB_PATTERN_TIP for more than 20 states\."):
        driver.ParsimonySession(amd_lib, case.states, seqs, PC.charmap(amd_lib, case), None, 0)
    case = PC.BY_NAME["dna_8x300_tail"]
    seqs, _ = PC.alignment(case)
    with pytest.raises(RuntimeError, match=r"\[902\]"):
        driver.ParsimonySession(amd_lib, case.states, seqs, PC.charmap(amd_lib, case), None, api.SITE_REPEATS)
    ops, edge = PC.traversal(case)
    with _session(amd_lib, case) as s:
        s.update(ops)
        good = s.edge_score(*edge)
        assert s.edge_score(s.nodes, 0) == api.UINT_MAX and amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert s.edge_score(0, s.nodes) == api.UINT_MAX and amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert s.root_score(s.nodes) == api.UINT_MAX and amd_lib.errno() == api.ERROR_PARAM_INVALID
        pairs = np.array([[0, 1], [s.nodes, 1]], dtype=np.uint32)
        out = np.full(2, 0xDEADBEEF, dtype=np.uint32)
        assert amd_lib.pll_gpu_fastparsimony_edge_scores(s.pars, api.uptr(pairs), 2, api.uptr(out)) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and (out == 0xDEADBEEF).all()
        assert amd_lib.pll_gpu_fastparsimony_insertion_scores(s.pars, s.nodes, api.uptr(pairs), 1, api.uptr(out)) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and (out == 0xDEADBEEF).all()
        assert amd_lib.pll_gpu_sync_parsimony(s.pars, s.nodes) == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID
        # an update with an index out of range does nothing at all
        s.update([(8, 0, 1), (s.nodes, 2, 3)])
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert s.edge_score(*edge) == good
        # a structure this library did not create
        foreign = api.Parsimony()
        assert amd_lib.pll_fastparsimony_edge_score(C.byref(foreign), 0, 1) == api.UINT_MAX
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID
    amd_lib.pll_parsimony_destroy(None)
