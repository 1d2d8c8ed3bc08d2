"""What the quartet tests share - TEST INFRASTRUCTURE: from an insertion_cases.Layout the call sequence of a caller that
scores all three pairings around EVERY inner edge with one pll_gpu_quartet_loglikelihoods call (INTEGRATION.md,
"Scoring every NNI at once").

All four ends of every quartet are read in one launch, so each must stand in HBM oriented towards its quartet's inner
edge at once: the caller runs the rooted full traversal and the upward operations of the insertion tests
(Layout.full_ops / Layout.upward) and names, for the record q on the far side of each of the four outer branches, the
upward slot where q is the root-side record of its edge and q's own slot otherwise. The reference's per-edge path - two
operations into two spare nodes and an edge log-likelihood per value - takes Layout.tmp and Layout.cherry as the spare
slots."""
import numpy as np

import insertion_cases as IC
from pllamd import driver


def outer(p):
    """the records of the inner edge p's four outer branches, in the order of e0..e3"""
    return (p.next, p.next.next, p.back.next, p.back.next.next)


def quartet_rows(lay, slot, edges=None):
    """one row per inner edge, in tree.inner_edges() order: ((clv, scaler, matrix) of e0..e3, the inner matrix)"""
    def directed(x):
        return slot[x.uid] if x.uid in slot else lay.end(x)

    rows = []
    for p in (lay.tree.inner_edges() if edges is None else edges):
        ends = tuple(directed(q.back) + (q.pm,) for q in outer(p))
        rows.append(ends + (p.pm,))
    return rows


def prepare(bed):
    """full traversal + upward CLVs; the quartet row of every inner edge"""
    bed.update(bed.lay.full_ops())
    ops, slot = bed.lay.upward()
    bed.update(ops)
    return quartet_rows(bed.lay, slot)


def batched(bed, rows):
    return driver.quartet_loglikelihoods(bed.lib, bed.p, rows, bed.fi)


def per_edge(bed, rows, own=None):
    """[Q, 3] through the two spare slots; own (a list) receives per value (first node, second node): whether that node
    rescaled anywhere beyond its children's counts - scale_buffer[tmp] minus the children's buffers"""
    lay = bed.lay

    def rescaled(tmp, children):
        count = bed.scaler(tmp[1]).astype(np.int64)
        for clv, sc, _ in children:
            if sc >= 0 and clv >= lay.tips:
                count -= bed.scaler(sc)
        return bool((count > 0).any())

    def after(i, a, first, second):
        own.append((rescaled(lay.tmp, first), rescaled(lay.cherry, second)))

    return driver.quartet_loglikelihoods_per_edge(bed.lib, bed.p, rows, bed.fi, lay.tmp, lay.cherry, after if own is not None else None)


def pair_tips(lay, rows):
    """the number of tip ends in each pair of each arrangement of each row, flattened"""
    out = []
    for r in rows:
        for (x, y), (z, w) in driver.QUARTET_PAIRS:
            out += [(r[x][0] < lay.tips) + (r[y][0] < lay.tips), (r[z][0] < lay.tips) + (r[w][0] < lay.tips)]
    return out
