"""Seeded fast-parsimony cases shared by tools/gen_fastparsimony_golden.py, the tests and
tools/fastparsimony_timing.py - plumbing, like the rest of this package; the product is the C/HIP library.

A case is an alignment (one ancestral state per site, each tip copies it unless a uniform draw falls below the
mutation rate; DNA cases carry one all-N column), optional pattern weights, and a tree given as the list of
(parent, child1, child2) score indices that pll_fastparsimony_update_vectors takes. The module also carries a NumPy
restatement of the Fitch step (`Model`), checked against the golden file by the CPU tests, which the GPU tests use
where no reference library is at hand.
"""
import zlib
from dataclasses import dataclass

import numpy as np

from . import api

NT, AA, BIN = b"ACGT", b"ARNDCQEGHILKMFPSTWYV", b"01"
# symbols of the custom maps (5 and 61 states): printable, one state each
CUSTOM = bytes(range(48, 48 + 61))


@dataclass(frozen=True)
class ParsCase:
    name: str
    tips: int
    sites: int
    states: int
    mutation: float
    seed: int
    max_weight: int = 0        # 0: no pattern weights; otherwise weights cycle 1..max_weight
    tree: str = "balanced"     # or "caterpillar"
    pattern_tip_only: bool = False  # more than 20 states: the reference refuses anything else

    @property
    def nodes(self):
        return self.tips + 3 * (self.tips - 1)


CASES = [
    ParsCase("dna_3x5_none_informative", 3, 5, 4, 0.5, 101),
    ParsCase("dna_8x40_constant", 8, 40, 4, 0.0, 102),
    ParsCase("dna_8x31_one_word", 8, 31, 4, 0.6, 103),
    ParsCase("dna_8x300_tail", 8, 300, 4, 0.5, 104),
    ParsCase("dna_9x40_weights_caterpillar", 9, 40, 4, 0.6, 105, max_weight=39, tree="caterpillar"),
    ParsCase("aa_8x64", 8, 64, 20, 0.6, 106),
    ParsCase("s61_12x200", 12, 200, 61, 0.6, 107, pattern_tip_only=True),
    ParsCase("s61_12x200_weights_caterpillar", 12, 200, 61, 0.6, 108, max_weight=8, tree="caterpillar", pattern_tip_only=True),
    ParsCase("aa_33x700_weights", 33, 700, 20, 0.5, 109, max_weight=39),
    ParsCase("dna_16x3000_weights", 16, 3000, 4, 0.6, 110, max_weight=63),
    ParsCase("s5_8x40", 8, 40, 5, 0.6, 111),
    ParsCase("bin_8x40", 8, 40, 2, 0.6, 112),
]
BY_NAME = {c.name: c for c in CASES}


def symbols(case):
    return {4: NT, 20: AA, 2: BIN}.get(case.states, CUSTOM[:case.states])


def charmap(lib, case):
    """uint64[256] character -> state mask: the library's own map where it has one, otherwise one bit per symbol"""
    name = {4: "pll_map_nt", 20: "pll_map_aa", 2: "pll_map_bin"}.get(case.states)
    if name:
        return np.array(lib.state_map(name), dtype=np.uint64)
    m = np.zeros(256, dtype=np.uint64)
    for i, ch in enumerate(symbols(case)):
        m[ch] = np.uint64(1) << np.uint64(i)
    return m


def alignment(case):
    """(sequences: list of bytes, weights: uint32[sites] or None)"""
    rng = np.random.default_rng(case.seed)
    sym = np.frombuffer(symbols(case), dtype=np.uint8)
    ancestral = rng.integers(0, case.states, size=case.sites)
    mutate = rng.random((case.tips, case.sites)) < case.mutation
    drawn = rng.integers(0, case.states, size=(case.tips, case.sites))
    idx = np.where(mutate, drawn, ancestral[None, :])
    chars = sym[idx]
    if case.states == 4:
        chars[:, case.sites // 2] = ord("N")
    weights = None
    if case.max_weight:
        weights = (np.arange(case.sites, dtype=np.uint32) % case.max_weight) + 1
    return [bytes(row) for row in chars], weights


def attribute_sets(case):
    """(label, attribute word) the golden file and the tests cover for a case"""
    sets = [("tip", api.PATTERN_TIP), ("tip_avx2", api.PATTERN_TIP | api.ARCH_AVX2)]
    if not case.pattern_tip_only and case.states <= 20:
        sets.append(("clv", 0))
    return sets


def traversal(case):
    """ops that combine tips 0 .. tips-2 into one vector, and the edge (that vector, the last tip) to score at.
    Parents take the score indices tips, tips+1, ..."""
    leaves = list(range(case.tips - 1))
    nxt = case.tips
    ops = []
    if case.tree == "caterpillar":
        top = leaves[0]
        for leaf in leaves[1:]:
            ops.append((nxt, top, leaf))
            top, nxt = nxt, nxt + 1
    else:
        level = leaves
        while len(level) > 1:
            up = []
            for i in range(0, len(level) - 1, 2):
                ops.append((nxt, level[i], level[i + 1]))
                up.append(nxt)
                nxt += 1
            if len(level) % 2:
                up.append(level[-1])
            level = up
        top = level[0]
    return ops, (top, case.tips - 1)


def chain_depth(ops):
    """number of dependency levels of a list in which every entry only reads what earlier entries wrote"""
    depth = {}
    for p, a, b in ops:
        depth[p] = max(depth.get(a, 0), depth.get(b, 0)) + 1
    return max(depth.values()) if depth else 0


# ---- directional vectors of an unrooted tree (tests/utree.py's UTree, or anything with its records) ------------------

def record_index(rec, tree_tips, total_tips):
    """score index of the vector at a record, oriented towards rec.back: a tip's own index; the three records of the
    inner node with clv c share the block total_tips + 3 (c - tree_tips) .. + 2"""
    if not rec.inner:
        return rec.clv
    # position in the ring, counted from the ring's record with the smallest uid
    q, k = min((rec, rec.next, rec.next.next), key=lambda x: x.uid), 0
    while q is not rec:
        q, k = q.next, k + 1
    return total_tips + 3 * (rec.clv - tree_tips) + k


def postorder_ops(tree, rec, total_tips):
    """ops of one full traversal towards the edge at `rec`: the vectors of rec and rec.back, children before parents"""
    ops = []
    for top in (rec, rec.back):
        stack = [(top, False)]
        while stack:
            q, ready = stack.pop()
            if not q.inner:
                continue
            c1, c2 = q.next.back, q.next.next.back
            if ready:
                ops.append(tuple(record_index(x, tree.tips, total_tips) for x in (q, c1, c2)))
            else:
                stack += [(q, True), (c2, False), (c1, False)]
    return ops, (record_index(rec, tree.tips, total_tips), record_index(rec.back, tree.tips, total_tips))


def directional_ops(tree, total_tips):
    """ops (children before parents) that compute the vector of EVERY inner record of `tree`, and the list of
    (a, b) facing vectors of every edge"""
    ops, done = [], set()

    def visit(r):
        if not r.inner or r.uid in done:
            return
        stack = [(r, False)]
        while stack:
            q, ready = stack.pop()
            if not q.inner or q.uid in done:
                continue
            c1, c2 = q.next.back, q.next.next.back
            if ready:
                done.add(q.uid)
                ops.append((record_index(q, tree.tips, total_tips), record_index(c1, tree.tips, total_tips),
                            record_index(c2, tree.tips, total_tips)))
            else:
                stack.append((q, True))
                stack.append((c2, False))
                stack.append((c1, False))

    for r in tree.records():
        visit(r)
    edges = [(record_index(r, tree.tips, total_tips), record_index(r.back, tree.tips, total_tips)) for r in tree.edges()]
    return ops, edges


# ---- NumPy restatement of the Fitch step ------------------------------------------------------------------------------

class Model:
    """Executes operation lists in order on copies of the tip vectors: vec[node] is uint32[states][words]."""

    def __init__(self, tip_vectors, nodes, const_cost):
        states, words = tip_vectors[0].shape
        self.vec = np.zeros((nodes, states, words), dtype=np.uint32)
        self.vec[:len(tip_vectors)] = np.stack(tip_vectors) if words else 0
        self.cost = np.zeros(nodes, dtype=np.uint64)
        self.const_cost = int(const_cost)

    @staticmethod
    def _miss(a, b):
        return ~np.bitwise_or.reduce(a & b, axis=0)

    @staticmethod
    def _popcount(words):
        return int(np.unpackbits(np.ascontiguousarray(words).view(np.uint8)).sum())

    def parent(self, a, b):
        miss = self._miss(a, b)
        return (a & b) | (miss[None, :] & (a | b)), self._popcount(miss)

    def update(self, ops):
        for p, c1, c2 in ops:
            vec, mism = self.parent(self.vec[c1], self.vec[c2])
            cost = mism + int(self.cost[c1]) + int(self.cost[c2])
            self.vec[p], self.cost[p] = vec, cost

    def edge_score(self, a, b):
        return self._popcount(self._miss(self.vec[a], self.vec[b])) + int(self.cost[a]) + int(self.cost[b]) + self.const_cost

    def root_score(self, n):
        return int(self.cost[n]) + self.const_cost

    def insertion_score(self, node, a, b):
        vec, mism = self.parent(self.vec[a], self.vec[b])
        return (mism + self._popcount(self._miss(vec, self.vec[node])) + int(self.cost[a]) + int(self.cost[b]) +
                int(self.cost[node]) + self.const_cost)


def crc(vector):
    return zlib.crc32(np.ascontiguousarray(vector, dtype="<u4").tobytes()) & 0xFFFFFFFF


def informative_string(flags):
    return "".join("1" if f else "0" for f in flags)
