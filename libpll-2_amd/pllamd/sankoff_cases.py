"""Seeded weighted-parsimony (Sankoff) cases shared by tools/gen_sankoff_golden.py, the tests and
tools/sankoff_timing.py - plumbing, like the rest of this package; the product is the C/HIP library.

A case is an alignment (workload.random_states, seed 8, 15 % mutations; DNA cases additionally carry IUPAC ambiguity
codes and gaps in about a tenth of their cells), a character map, a rooted tree over all tips given as
(parent, child1, child2) score indices, and the cost matrices it is run under. The module also carries a NumPy
restatement of build / score / reconstruct / insertion (`Model`), checked against the golden file by the CPU tests,
which the GPU tests use where no reference library is at hand.

Index plan of a case: score buffers 0 .. tips-1 are the tips, tips .. 2 tips - 2 the inner nodes of the rooted tree,
2 tips .. the directional vectors of the insertion tree (parsimony_cases.directional_ops with that base), the last two
are spare. Ancestral buffers: one per inner node, at the node's score index.
"""
import zlib
from dataclasses import dataclass

import numpy as np

from . import workload as W

ALIGNMENT_SEED, MUTATE_PCT = 8, 15
AMBIGUOUS = np.frombuffer(b"RYSWKMBDHVN-", dtype=np.uint8)


@dataclass(frozen=True)
class SankoffCase:
    name: str
    tips: int
    sites: int
    states: int
    tree: str = "random"  # "random" joins, "caterpillar" or "balanced"

    @property
    def score_buffers(self):
        return 4 * self.tips

    @property
    def ancestral_buffers(self):
        return self.tips

    @property
    def buffers(self):
        return self.tips + self.score_buffers

    @property
    def spare(self):
        return self.buffers - 2, self.buffers - 1

    @property
    def insertion_base(self):
        return 2 * self.tips

    @property
    def matrices(self):
        return ("unit", "tv", "real") if self.states == 4 else ("unit", "real")


CASES = [
    SankoffCase("dna_8x1", 8, 1, 4),
    SankoffCase("dna_8x63", 8, 63, 4),
    SankoffCase("dna_8x64", 8, 64, 4),
    SankoffCase("dna_8x65", 8, 65, 4),
    SankoffCase("dna_9x257_caterpillar", 9, 257, 4, "caterpillar"),
    SankoffCase("dna_16x300_balanced", 16, 300, 4, "balanced"),
    SankoffCase("bin_8x70", 8, 70, 2),
    SankoffCase("s5_12x130", 12, 130, 5),
    SankoffCase("aa_33x130", 33, 130, 20),
    SankoffCase("s61_10x70", 10, 70, 61),
    SankoffCase("s64_8x65", 8, 65, 64),
]
BY_NAME = {c.name: c for c in CASES}
CASE_MATRICES = [(c, m) for c in CASES for m in c.matrices]
CASE_MATRIX_IDS = [f"{c.name}-{m}" for c, m in CASE_MATRICES]


def symbols(states):
    return {4: W.NT_CHARS, 20: W.AA_CHARS, 2: b"01"}.get(states, bytes(range(48, 48 + states)))


def charmap(lib, states):
    """uint64[256] character -> state mask: the library's own map where it has one, workload.map_generic otherwise"""
    name = {4: "pll_map_nt", 20: "pll_map_aa", 2: "pll_map_bin"}.get(states)
    if name:
        return np.array(lib.state_map(name), dtype=np.uint64)
    return W.map_generic(states)


def alignment(case):
    """list of `tips` byte strings of `sites` characters"""
    st = W.random_states(case.tips, case.sites, case.states, ALIGNMENT_SEED, MUTATE_PCT)
    chars = np.frombuffer(symbols(case.states), dtype=np.uint8)[st]
    if case.states == 4:
        rng = np.random.Generator(np.random.PCG64(ALIGNMENT_SEED + 1))
        hit = rng.random(chars.shape) < 0.1
        chars = np.where(hit, AMBIGUOUS[rng.integers(0, len(AMBIGUOUS), size=chars.shape)], chars)
    return [row.astype(np.uint8).tobytes() for row in chars]


def matrix(name, states):
    """float64[states][states] cost matrix: entry [k][n] is the cost of state k below state n"""
    if name == "unit":  # the matrix of examples/parsimony/npr-pars.c
        return 1.0 - np.eye(states)
    if name == "tv":  # transitions (A<->G, C<->T) 1, transversions 2
        assert states == 4
        m = np.full((4, 4), 2.0)
        m[0, 2] = m[2, 0] = m[1, 3] = m[3, 1] = 1.0
        np.fill_diagonal(m, 0.0)
        return m
    if name == "real":  # asymmetric
        m = np.random.Generator(np.random.PCG64(5)).uniform(0.5, 3.0, size=(states, states))
        np.fill_diagonal(m, 0.0)
        return m
    raise KeyError(name)


def tree_ops(case):
    """(ops, root): ops that combine all tips into one root, children before parents; parents take the score indices
    tips, tips + 1, ..."""
    nxt, ops = case.tips, []
    if case.tree == "caterpillar":
        top = 0
        for leaf in range(1, case.tips):
            ops.append((nxt, top, leaf))
            top, nxt = nxt, nxt + 1
        return ops, top
    if case.tree == "balanced":
        level = list(range(case.tips))
        while len(level) > 1:
            up = []
            for i in range(0, len(level) - 1, 2):
                ops.append((nxt, level[i], level[i + 1]))
                up.append(nxt)
                nxt += 1
            if len(level) % 2:
                up.append(level[-1])
            level = up
        return ops, level[0]
    return random_join_ops(range(case.tips), nxt, case.tips * 1000 + case.sites)


def random_join_ops(leaves, first_parent, seed):
    """(ops, root): join two random subtrees until one remains; parents take first_parent, first_parent + 1, ..."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pool, nxt, ops = list(leaves), first_parent, []
    while len(pool) > 1:
        i, j = sorted(rng.choice(len(pool), size=2, replace=False))
        b = pool.pop(j)
        a = pool.pop(i)
        ops.append((nxt, a, b))
        pool.append(nxt)
        nxt += 1
    return ops, pool[0]


def reconstruct_ops(ops, root, tips):
    """(node score, node ancestral, parent score, parent ancestral) rows in preorder, the root first; tips get none.
    The first row's parent fields repeat the node's: the reference does not read them."""
    children = {p: (a, b) for p, a, b in ops}
    rows, stack = [(root, root, root, root)], [root]
    while stack:
        p = stack.pop()
        for c in children[p]:
            if c >= tips:
                rows.append((c, c, p, p))
                stack.append(c)
    return rows


def levels(ops):
    """number of dependency levels of a list in which every entry only reads what earlier entries wrote"""
    depth = {}
    for p, a, b in ops:
        depth[p] = max(depth.get(a, 0), depth.get(b, 0)) + 1
    return max(depth.values()) if depth else 0


# ---- NumPy restatement (src/parsimony.c:24-67, :204-383) ----------------------------------------------------------

class Model:
    """Executes the calls in order on arrays of its own: sb[buffer] is float64[sites][states], anc[buffer] uint32[sites]"""

    def __init__(self, case, cost_matrix):
        self.case = case
        self.m = np.ascontiguousarray(cost_matrix, dtype=np.float64)
        self.sb = np.zeros((case.buffers, case.sites, case.states))
        self.anc = np.zeros((case.tips + case.ancestral_buffers, case.sites), dtype=np.uint32)

    def set_sequence(self, index, cmap, seq):
        inf = self.m.max() + 1.0
        masks = np.asarray(cmap, dtype=np.uint64)[np.frombuffer(bytes(seq), dtype=np.uint8)]
        assert masks.all()
        bits = (masks[:, None] >> np.arange(self.case.states, dtype=np.uint64)[None, :]) & np.uint64(1)
        self.sb[index] = np.where(bits.astype(bool), 0.0, inf)

    def combine(self, a, b):
        """a, b: [sites][states] -> the parent's buffer: min over k of (child[k] + m[k][n]) of each child, added"""
        return (a[:, :, None] + self.m[None, :, :]).min(axis=1) + (b[:, :, None] + self.m[None, :, :]).min(axis=1)

    @staticmethod
    def total(buf):
        """the reference's sum: site after site (cumsum adds in order; np.sum would add pairwise)"""
        return float(np.cumsum(buf.min(axis=1))[-1])

    def build(self, ops):
        for p, a, b in ops:
            self.sb[p] = self.combine(self.sb[a], self.sb[b])
        return self.score(ops[-1][0])

    def score(self, index):
        return self.total(self.sb[index])

    def tables(self, cmap):
        cmap = [int(x) for x in cmap]
        revmap = [0] * 256
        for i in range(256):
            if bin(cmap[i]).count("1") == 1:
                revmap[cmap[i].bit_length() - 1] = i
        return np.array(revmap, dtype=np.uint32), cmap

    def reconstruct(self, cmap, rows, stats=None):
        """stats: a two-element list that receives [parent's character kept, own minimum taken] counts"""
        revmap, cmap = self.tables(cmap)
        sites = np.arange(self.case.sites)
        for i, (ns, na, ps, pa) in enumerate(rows):
            first_min = self.sb[ns].argmin(axis=1)  # the first of equal minima, like the reference's strict <
            own = revmap[first_min]
            if i == 0:
                self.anc[na] = own
                continue
            pchar = self.anc[pa].copy()
            pstate = np.array([(cmap[c] & -cmap[c]).bit_length() - 1 for c in pchar])
            keep = self.sb[ns][sites, first_min] + 1.0 > self.sb[ps][sites, pstate]
            self.anc[na] = np.where(keep, pchar, own)
            if stats is not None:
                stats[0] += int(keep.sum())
                stats[1] += int((~keep).sum())

    def insertion_score(self, node, a, b):
        return self.total(self.combine(self.combine(self.sb[a], self.sb[b]), self.sb[node]))


def crc(array, dtype):
    return zlib.crc32(np.ascontiguousarray(array, dtype=dtype).tobytes()) & 0xFFFFFFFF
