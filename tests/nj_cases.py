"""What the neighbour-joining tests share - TEST INFRASTRUCTURE: the matrices, and pllamd/nj.py's answer for each, computed
once and left read-only.

additive(n)   the path lengths of nj.random_tree(n): every branch a multiple of 1/64 in [1/64, 1/2], so sums, halves and
              (on a cherry) the division of the length formula are exact in binary64
noisy(n)      additive(n) x (1 +- 5 % uniform), symmetric: distances up to 11.2 at 600 nodes
ones(n)       every distance 1: every pair ties in the first join
balanced(L)   nj.balanced_tree(L), 3 * 2^L tips: all cherries tie in every round of joins
"""
import functools

import numpy as np

from pllamd import nj

# no join; one join = the four-node rule alone; ...; below, at and above a wave; past the 256 threads of a workgroup; 600:
# several search workgroups at the default rows per workgroup
COUNTS = (3, 4, 5, 8, 9, 33, 64, 65, 130, 257, 600)
FLAGS = {"nj": 0, "bionj": nj.BIONJ}
BALANCED_LEVELS = (1, 3, 6)  # 6, 24 and 192 tips

# test_nj_host.py::test_the_inputs_keep_their_gaps measures both on this host and asserts them:
# the worst |length(binary64) - length(long double)| of pllamd/nj.py over noisy(n), n in COUNTS, both flags ...
# (measured: 2.348e-12, at 600 nodes under NJ, where the distances reach 11.2; 1.4e-15 and less up to 9 nodes) ...
WORST_RESTATEMENT_DEVIATION = 2.35e-12
# ... and the least (second-best Q - best Q) / max |Q| over every join of those runs (measured: 7.5e-7, at 600 nodes, NJ)
LEAST_GAP = 1e-9


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def additive(n):
    parent, length = nj.random_tree(n, np.random.default_rng(1000 + n))
    return _frozen(nj.tree_distances(parent, length))


@functools.lru_cache(maxsize=None)
def noisy(n):
    rng = np.random.default_rng(2000 + n)
    up = np.triu(additive(n) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(n, n))), 1)
    return _frozen(up + up.T)


@functools.lru_cache(maxsize=None)
def ones(n):
    return _frozen(np.ones((n, n)) - np.eye(n))


@functools.lru_cache(maxsize=None)
def balanced(levels):
    return _frozen(nj.balanced_tree(levels))


MATRICES = {"additive": additive, "noisy": noisy, "ones": ones, "balanced": balanced}

# rows of the triangle per search workgroup (PLL_AMD_NJ_ROWS) -> the (kind, n, flag) run under it in a child process. One
# row: 599 search workgroups at the first step of 600 nodes, so the last arrival's loop over the partials takes a third
# step of its 256 threads, then a second, then one, as the matrix shrinks, and the ties of ones(600) are settled across all
# of them. Three rows: the last workgroup's list of rows ends early (598 = 3 x 199 + 1 rows at 599 nodes, ...).
ROW_RUNS = {1: (("noisy", 600, "nj"), ("noisy", 600, "bionj"), ("ones", 600, "nj"), ("balanced", 6, "nj")),
            3: (("noisy", 257, "nj"), ("noisy", 257, "bionj"), ("noisy", 600, "nj"), ("noisy", 600, "bionj"))}
EXACT_KINDS = ("additive", "ones", "balanced")


def search_workgroups(nodes, rows):
    """the search workgroups of every step of a join of `nodes` nodes: ceil((r - 1) / rows), r = nodes .. 4
    (include/pll_amd_device.h: rows 0 .. r-2 of the triangle hold pairs)"""
    return [(r - 1 + rows - 1) // rows for r in range(nodes, 3, -1)]


@functools.lru_cache(maxsize=None)
def expected(kind, n, flag, long_double=False):
    """(parent, length) of pllamd/nj.py for MATRICES[kind](n) under FLAGS[flag]"""
    parent, length = nj.nj_tree(MATRICES[kind](n), FLAGS[flag], np.longdouble if long_double else np.float64)
    return _frozen(parent), _frozen(length)
