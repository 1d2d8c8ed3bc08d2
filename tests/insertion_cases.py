"""What the insertion tests share - TEST INFRASTRUCTURE: from a UTree the call sequence of a caller that scores the
insertion of a subtree into EVERY edge with one pll_gpu_insertion_loglikelihoods call ("Scoring every
regraft edge at once"), and a partition per library that can take it.

All candidates are read in one launch, so both ends of every edge must stand in HBM at once, and an inner node's one
CLV slot holds one orientation. The caller therefore
  * roots a full traversal at one edge: every CLV then points towards that edge (the "downward" CLVs);
  * computes, for every other edge, the CLV of its root-side end pointing AWAY from the root (the "upward" CLV) into a
    spare slot, with ordinary operations: parent = the spare slot, children = the upward CLV of the edge above (or the
    far end of the root edge) and the sibling's downward CLV - one pll_update_partials list, parents before children;
  * writes the half-length matrix of every edge into a spare matrix slot with one pll_update_prob_matrices;
  * scores all edges with one call.

Index plan (`Layout`): the tree's own tips 0 .. T-1, `extra` further tips (query sequences), the tree's inner nodes,
2T-4 upward slots, one slot for a query cherry, one tmp slot (the per-edge path and the reference need it); scalers
alike without the tips; matrices: the 2T-3 edges, their halves, the query's pendant edge, the two edges of the query
cherry."""
import ctypes as C

import numpy as np

from pllamd import api, driver, workload as W
from utree import UTree

NONE = api.SCALE_BUFFER_NONE


class Layout:
    def __init__(self, tree, extra=2):
        self.tree, self.T, self.extra = tree, tree.tips, extra
        T = self.T
        self.tips = T + extra
        self.inner0 = self.tips                  # the tree's inner node with UTree clv c sits at c + extra
        self.up0 = self.tips + (T - 2)           # upward slots
        self.cherry = (self.up0 + 2 * T - 4, (T - 2) + 2 * T - 4)
        self.tmp = (self.cherry[0] + 1, self.cherry[1] + 1)
        self.clv_buffers = (T - 2) + (2 * T - 4) + 2
        self.scale_buffers = self.clv_buffers
        self.edges = 2 * T - 3
        self.pm_pendant = 2 * self.edges
        self.pm_cherry = (self.pm_pendant + 1, self.pm_pendant + 2)
        self.prob_matrices = self.pm_pendant + 3
        self.root = tree.inner_edges()[0]

    def end(self, r):
        """(clv, scaler) of record r's own slot"""
        return (r.clv + self.extra, r.scaler) if r.inner else (r.clv, NONE)

    def half(self, pm):
        return self.edges + pm

    def full_ops(self):
        """the rooted full traversal, in the partition's numbering"""
        self.tree.forget()
        e = self.extra
        fix = lambda clv: clv + e if clv >= self.T else clv
        return [(fix(p), ps, fix(a), am, asc, fix(b), bm, bsc) for p, ps, a, am, asc, b, bm, bsc in self.tree.ops_for(self.root)]

    def upward(self):
        """(ops, {uid of record q: (clv, scaler) that holds q's node oriented towards q.back}) for the root-side record
        q of every edge; the ops fill the upward slots, parents before children"""
        ops, slot, n = [], {}, 0
        # the two ends of the root edge already point at each other
        slot[self.root.uid] = self.end(self.root)
        slot[self.root.back.uid] = self.end(self.root.back)
        todo = [self.root, self.root.back]
        while todo:
            x = todo.pop()  # x's own slot points towards the root; what lies beyond x.back is known: slot[x.back.uid]
            if not x.inner:
                continue
            for q, sib in ((x.next, x.next.next), (x.next.next, x.next)):
                # x's node towards q.back: what comes in over x's edge and over the sibling's
                far, s = slot[x.back.uid], self.end(sib.back)
                clv, sc = self.up0 + n, (self.T - 2) + n
                n += 1
                ops.append((clv, sc, far[0], x.pm, far[1], s[0], sib.pm, s[1]))
                slot[q.uid] = (clv, sc)
                todo.append(q.back)
        assert n == 2 * self.T - 4
        return ops, slot

    def candidates(self, slot):
        """one row per edge in tree.edges() order: (child1 clv, scaler, matrix, child2 clv, scaler, matrix), both matrices
        the edge's half-length one; child1 = the end away from the root (its own slot), child2 = the root-side end"""
        rows = []
        for r in self.tree.edges():
            if r is self.root or r.back is self.root:
                a, b = self.end(self.root), self.end(self.root.back)
            else:
                q = r if r.uid in slot else r.back   # the root-side record of the edge
                a, b = self.end(q.back), slot[q.uid]
            h = self.half(r.pm)
            rows.append((a[0], a[1], h, b[0], b[1], h))
        return rows

    def branches(self, pendant=0.1, cherry=(0.07, 0.13)):
        pairs = list(self.tree.branches())
        pairs += [(self.half(pm), x / 2.0) for pm, x in self.tree.branches()]
        pairs += [(self.pm_pendant, pendant), (self.pm_cherry[0], cherry[0]), (self.pm_cherry[1], cherry[1])]
        return pairs


def alignment(states, rows, sites, seed=8, mutate_pct=15):
    st = W.random_states(rows, sites, states, seed, mutate_pct)
    if states == 4:
        return W.states_to_sequences(st, W.NT_CHARS), W.map_nt(), W.GTR_DNA["exch"], W.GTR_DNA["freqs"]
    ex, fr = W.synthetic_exch(states)
    if states == 20:
        return W.states_to_sequences(st, W.AA_CHARS), W.map_aa(), ex, fr
    return W.states_to_sequences(st, bytes(range(48, 48 + states))), W.map_generic(states), ex, fr


class Bed:
    """one library's partition for a Layout"""

    def __init__(self, lib, lay, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, rate_matrices=1, freqs_indices=None,
                 pattern_weights=None, prop_invar=0.0):
        self.lib, self.lay, self.states, self.sites, self.rate_cats, self.attrs = lib, lay, states, sites, rate_cats, attrs
        self.p = lib.pll_partition_create(lay.tips, lay.clv_buffers, states, sites, rate_matrices, lay.prob_matrices, rate_cats,
                                          lay.scale_buffers, attrs | api.ARCH_AVX2)
        assert self.p, (lib.errno(), lib.errmsg())
        self.part = self.p.contents
        e = np.ascontiguousarray(exch, dtype=np.float64)
        r = np.ascontiguousarray(W.gamma_rates_mean(0.7, rate_cats), dtype=np.float64)
        for m in range(rate_matrices):
            f = np.roll(np.asarray(freqs, dtype=np.float64), m)  # a second frequency set: the first, rotated
            f = np.ascontiguousarray(f / f.sum())
            lib.pll_set_frequencies(self.p, m, api.dptr(f))
            lib.pll_set_subst_params(self.p, m, api.dptr(e))
        lib.pll_set_category_rates(self.p, api.dptr(r))
        self.cmap = (C.c_ulonglong * 256)(*[int(x) for x in cmap])
        for i, s in enumerate(seqs):
            assert lib.pll_set_tip_states(self.p, i, self.cmap, s), (lib.errno(), lib.errmsg())
        if pattern_weights is not None:
            w = np.ascontiguousarray(pattern_weights, dtype=np.uint32)
            lib.pll_set_pattern_weights(self.p, api.uptr(w))
        self.fi = np.ascontiguousarray(freqs_indices if freqs_indices is not None else np.zeros(rate_cats), dtype=np.uint32)
        if prop_invar > 0.0:
            assert lib.pll_update_invariant_sites(self.p), (lib.errno(), lib.errmsg())
            for m in range(rate_matrices):
                assert lib.pll_update_invariant_sites_proportion(self.p, m, float(prop_invar)), (lib.errno(), lib.errmsg())
        self.matrices(lay.branches())

    def close(self):
        if self.p:
            self.lib.pll_partition_destroy(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def matrices(self, pairs):
        idx = np.ascontiguousarray([m for m, _ in pairs], dtype=np.uint32)
        bl = np.ascontiguousarray([x for _, x in pairs], dtype=np.float64)
        assert self.lib.pll_update_prob_matrices(self.p, api.uptr(self.fi), api.uptr(idx), api.dptr(bl), len(pairs))

    def update(self, ops):
        if ops:
            self.lib.pll_update_partials(self.p, api.make_ops(ops), len(ops))

    def lnl(self, edge):
        return self.lib.pll_compute_edge_loglikelihood(self.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(self.fi), None)

    def prepare(self):
        """full traversal + upward CLVs; returns the candidate rows of every edge"""
        self.update(self.lay.full_ops())
        ops, slot = self.lay.upward()
        self.update(ops)
        return self.lay.candidates(slot)

    def query_cherry(self, tip_a, tip_b):
        """the two extra tips joined in the cherry slot: an inner subtree end with a scaler"""
        c = self.lay.cherry
        self.update([(c[0], c[1], tip_a, self.lay.pm_cherry[0], NONE, tip_b, self.lay.pm_cherry[1], NONE)])
        return (c[0], c[1], self.lay.pm_pendant)

    def batched(self, subtree, rows):
        return driver.insertion_loglikelihoods(self.lib, self.p, subtree, rows, self.fi)

    def per_edge(self, subtree, rows, own_rescales=None):
        """the per-edge path through the tmp slot; own_rescales (a list) receives, per candidate, whether the inserted node
        rescaled anywhere beyond its children's counts - scale_buffer[tmp] minus the children's buffers"""
        tmp = self.lay.tmp
        out = np.empty(len(rows))
        for i, c in enumerate(rows):
            out[i] = driver.insertion_loglikelihoods_per_edge(self.lib, self.p, subtree, [c], self.fi, tmp)[0]
            if own_rescales is not None:
                own = self.scaler(tmp[1]).astype(np.int64)
                for clv, sc in ((c[0], c[1]), (c[3], c[4])):
                    if sc >= 0 and clv >= self.lay.tips:
                        own -= self.scaler(sc)
                own_rescales.append(bool((own > 0).any()))
        return out

    def scaler(self, index):
        if self.lib.is_amd:
            assert self.lib.pll_gpu_sync_scaler(self.p, index)
        per = self.rate_cats if (self.attrs & api.RATE_SCALERS) else 1
        return api.as_np(self.part.scale_buffer[index], self.sites * per, np.uint32).copy()

    def write_scaler(self, index, counts):
        """the caller's own counts into scale_buffer[index], as driver.Session.write_scaler does it"""
        old = self.scaler(index)  # (settles the device side)
        new = np.ascontiguousarray(counts, dtype=np.uint32).reshape(old.shape)
        api.as_np(self.part.scale_buffer[index], new.size, np.uint32)[:] = new
        if self.lib.is_amd:
            self.lib.pll_gpu_invalidate(self.p, api.DIRTY_SCALER, index)

    def clv_bytes(self, index):
        assert self.lib.pll_gpu_sync_clv(self.p, index)
        n = self.sites * self.rate_cats * self.part.states_padded
        return api.as_np(self.part.clv[index], n, np.float64).tobytes()


def make(states, taxa, sites, rate_cats, seed_tree=7, extra=2):
    """(layout, sequences, charmap, exchangeabilities, frequencies) of one placement case"""
    tree = UTree(taxa, np.random.Generator(np.random.PCG64(seed_tree)))
    lay = Layout(tree, extra)
    seqs, cmap, exch, freqs = alignment(states, taxa + extra, sites)
    return lay, seqs, cmap, exch, freqs


def close(got, exp, rtol):
    """|d| <= rtol * max(|lnL|, 1), elementwise"""
    got, exp = np.asarray(got), np.asarray(exp)
    return np.isfinite(got).all() and bool((np.abs(got - exp) <= rtol * np.maximum(np.abs(exp), 1.0)).all())


def worst(got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    return float(np.max(np.abs(got - exp) / np.maximum(np.abs(exp), 1.0)))
