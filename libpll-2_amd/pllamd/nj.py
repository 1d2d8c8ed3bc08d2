"""Neighbour-joining and BIONJ trees from a distance matrix, on the host: the executable statement of what pll_gpu_nj_tree
and pll_gpu_distance_tree (include/pll_amd.h) compute. numpy only - usable with no device. The kernels
(csrc/hip/kernels_nj.h) perform the same operations in the same order, so in binary64 this is what they return.

The tree: tips are 0 .. n-1 in input order, the inner node made by join s is n + s, the last inner node 2n - 3 joins the
three nodes that remain; parent[v] / length[v] are v's parent and the branch to it, parent[2n - 3] = -1, length[2n - 3] = 0.

With r active nodes, r > 3 (every product rounded before it is added, brackets as written):
    R_i  = sum_k d_ik                          first: added one term at a time, k = 0, 1, ...; then carried forward
    Q_ij = (r-2) d_ij - (R_i + R_j)            the minimal one is joined; i = the node of the pair with the smaller label
    l_i  = d_ij / 2 + (R_i - R_j) / (2 (r-2)),   l_j = d_ij - l_i
    NJ:     d_uk = ((d_ik + d_jk) - d_ij) / 2,   R_u = ((R_i + R_j) - r d_ij) / 2
    BIONJ:  V starts as D;  lambda = 1/2 + (sum_{k != i,j} (V_jk - V_ik)) / (2 (r-2) V_ij) clamped to [0, 1], 1/2 where V_ij = 0
            d_uk = (d_jk - l_j) + lambda ((d_ik - l_i) - (d_jk - l_j))      = lambda (d_ik - l_i) + (1 - lambda) (d_jk - l_j)
            V_uk = (lambda V_ik + (1 - lambda) V_jk) - (lambda (1 - lambda)) V_ij
            R_u  = B + lambda (A - B),  A = (R_i - d_ij) - (r-2) l_i,  B = (R_j - d_ij) - (r-2) l_j
            (the weighted means of d and R in the form that is exact where both sides agree: on an additive matrix of
            dyadic lengths BIONJ then keeps D and R exact whatever lambda is, and joins what NJ joins)
    R_k  <- ((R_k - d_ik) - d_jk) + d_uk       the row sums are carried forward, not recomputed
    three nodes a, b, c:  l_a = ((d_ab + d_ac) - d_bc) / 2, likewise b and c.
Ties: among equal minimal Q the pair whose (smaller label, larger label) comes first lexicographically. Four nodes left:
Q_ab = Q_cd for every split, so only the three pairs that contain the active node with the smallest label are searched.

The active nodes live in slots 0 .. r-1: the new node takes the slot of i and the last slot moves into the slot of j (when
i is the last slot the new node takes j's and nothing moves). Only BIONJ's sum over k sees the slot order: it is added as
the kernel adds it (sum_order below).
"""
import numpy as np

BIONJ = 1


def launch_count(n):
    """launches of pll_gpu_nj_tree at n nodes (include/pll_amd_device.h states the rule)"""
    return 1 if n == 3 else 2 * (n - 3) + 2


def sum_order(terms, dtype):
    """the sum of terms[0 .. r) in the kernel's order: 256 running sums (k = t, t + 256, ...), each 64 of them added by
    halving (l takes l + 32, then l + 16, ...), the four results in order"""
    r = len(terms)
    rows = -(-r // 256)
    padded = np.zeros(rows * 256, dtype=dtype)
    padded[:r] = terms
    part = np.zeros(256, dtype=dtype)
    for row in padded.reshape(rows, 256):
        part = part + row
    w = part.reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[:, :off] + w[:, off:2 * off]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def nj_tree(distances, flags=0, dtype=np.float64, trace=None):
    """-> (parent int32 [2n - 2], length dtype [2n - 2]) of the [n, n] matrix, of which only [x][y], x < y, is read.
    flags: 0 = NJ, BIONJ. dtype: np.float64 is the definition; np.longdouble serves the tests as a second opinion.
    trace: a list that receives per join (best Q, second-best Q among the pairs searched or None, max |Q| over them)."""
    T = dtype
    src = np.asarray(distances, dtype=T)
    n = src.shape[0]
    assert src.shape == (n, n) and n >= 3
    up = np.triu(src, 1)
    D = up + up.T
    bionj = bool(flags & BIONJ)
    V = D.copy() if bionj else None
    R = np.zeros(n, dtype=T)
    for k in range(n):
        R = R + D[k]
    label = np.arange(n)
    parent = np.full(2 * n - 2, -1, dtype=np.int32)
    length = np.zeros(2 * n - 2, dtype=T)
    half, two = T(0.5), T(2)
    r, step = n, 0
    while r > 3:
        lab = label[:r]
        rm2 = T(r - 2)
        Q = rm2 * D[:r, :r] - (R[:r, None] + R[None, :r])
        search = np.triu(np.ones((r, r), dtype=bool), 1)
        if r == 4:
            only = int(np.argmin(lab))
            mine = np.zeros(r, dtype=bool)
            mine[only] = True
            search &= mine[:, None] | mine[None, :]
        qs = Q[search]
        qmin = qs.min()
        if trace is not None:
            rest = np.sort(qs)
            trace.append((qmin, rest[1] if len(rest) > 1 else None, np.abs(qs).max()))
        at = np.flatnonzero(search & (Q == qmin))
        a, b = at // r, at % r
        lo, hi = np.minimum(lab[a], lab[b]), np.maximum(lab[a], lab[b])
        first = int(np.argmin(lo.astype(np.int64) * (2 * n) + hi))  # (smaller label, larger label), lexicographically
        a, b = int(a[first]), int(b[first])
        si, sj = (a, b) if lab[a] < lab[b] else (b, a)

        dij, ri, rj = D[si, sj], R[si], R[sj]
        len_i = half * dij + (ri - rj) / (two * rm2)
        len_j = dij - len_i
        dI, dJ = D[si, :r].copy(), D[sj, :r].copy()
        others = np.ones(r, dtype=bool)
        others[[si, sj]] = False
        if bionj:
            vI, vJ, vij = V[si, :r].copy(), V[sj, :r].copy(), V[si, sj]
            lam = half
            if vij != 0:
                total = sum_order(np.where(others, vJ - vI, T(0)), T)
                lam = half + total / ((two * rm2) * vij)
                if not lam >= 0:
                    lam = T(0)
                if lam > 1:
                    lam = T(1)
            mu = T(1) - lam
            du = (dJ - len_j) + lam * ((dI - len_i) - (dJ - len_j))
            vu = (lam * vI + mu * vJ) - (lam * mu) * vij
            ru_i, ru_j = (ri - dij) - rm2 * len_i, (rj - dij) - rm2 * len_j
            ru = ru_j + lam * (ru_i - ru_j)
        else:
            du = half * ((dI + dJ) - dij)
            ru = half * ((ri + rj) - T(r) * dij)
        rn = ((R[:r] - dI) - dJ) + du

        u = n + step
        parent[lab[si]] = parent[lab[sj]] = u
        length[lab[si]], length[lab[sj]] = len_i, len_j
        last = r - 1
        su = sj if si == last else si
        move = si != last and sj != last
        ks = np.flatnonzero(others)
        kn = ks.copy()
        if move:
            kn[ks == last] = sj
            for M in (D, V) if bionj else (D,):
                M[sj, :r] = M[last, :r]
                M[:r, sj] = M[:r, last]
                M[sj, sj] = 0
            label[sj] = label[last]
        D[su, kn] = du[ks]
        D[kn, su] = du[ks]
        D[su, su] = 0
        if bionj:
            V[su, kn] = vu[ks]
            V[kn, su] = vu[ks]
            V[su, su] = 0
        R[kn] = rn[ks]
        R[su] = ru
        label[su] = u
        r, step = r - 1, step + 1

    root = 2 * n - 3
    d01, d02, d12 = D[0, 1], D[0, 2], D[1, 2]
    parent[label[:3]] = root
    length[label[0]] = half * ((d01 + d02) - d12)
    length[label[1]] = half * ((d01 + d12) - d02)
    length[label[2]] = half * ((d02 + d12) - d01)
    parent[root] = -1
    length[root] = 0
    return parent, length


def tree_distances(parent, length, dtype=np.float64):
    """[n, n] path lengths between the tips of a tree in the format above (a parent's label exceeds its children's)"""
    nodes = len(parent)
    n = (nodes + 2) // 2
    P = np.zeros((nodes, nodes), dtype=dtype)
    done = [nodes - 1]
    for v in range(nodes - 2, -1, -1):
        p = int(parent[v])
        assert p > v
        row = P[p, done] + dtype(length[v])
        P[v, done] = row
        P[done, v] = row
        done.append(v)
    return P[:n, :n]


def random_tree(n, rng, unit=1.0 / 64, longest=32):
    """(parent, length) of a random tree of n tips in the format above: random pairs joined until three nodes remain; every
    branch a multiple of `unit` in [unit, longest * unit] - sums and halves of such lengths are exact in binary64"""
    parent = np.full(2 * n - 2, -1, dtype=np.int32)
    length = np.zeros(2 * n - 2)
    active = list(range(n))
    for s in range(n - 3):
        i, j = sorted(rng.choice(len(active), size=2, replace=False))
        a, b = active[i], active[j]
        del active[j], active[i]
        parent[a] = parent[b] = n + s
        active.append(n + s)
    parent[active] = 2 * n - 3
    length[:-1] = rng.integers(1, longest + 1, size=2 * n - 3) * unit
    return parent, length


def balanced_tree(levels, unit=1.0 / 64):
    """the distance matrix of 3 * 2^levels tips: three balanced binary subtrees of that depth around one node, every branch
    `unit` long - all cherries tie in every round of joins"""
    n = 3 << levels
    D = np.zeros((n, n))
    per = 1 << levels
    for x in range(n):
        for y in range(n):
            if x == y:
                continue
            if x // per != y // per:
                D[x, y] = 2 * (levels + 1) * unit
            else:
                D[x, y] = 2 * ((x ^ y).bit_length()) * unit
    return D
