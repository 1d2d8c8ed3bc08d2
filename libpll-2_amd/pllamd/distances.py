"""The maximum-likelihood distance between two tips, on the host: the executable statement of what
pll_gpu_pairwise_distances (include/pll_amd.h) computes for one pair. numpy only - usable with no device.

Both ends are tips given by codes, so a site's sumtable row depends on its pair of codes (a, b) alone:
    row[k][j] = U[a][k][j] * W[b][k][j],   U[a][k][j] = sum_{i in a} pi_i Vinv[i][j],   W[b][k][j] = sum_{i in b} V[j][i]
with (V, Vinv, pi) of rate category k's matrix params_indices[k]. The alignment enters through the counts
n[a][b] = the summed pattern weight of the sites where the pair shows (a, b); an evaluation at t is a sum over the code pairs
that occur, and the iteration is newton.Bracket's.
"""
import numpy as np

from . import newton


def encode(sequences, charmap, states):
    """(codes [tips, sites] uint8, masks [ncodes] uint64) of sequences (bytes) under a 256-entry character -> state-mask map.
    4 states: the code is the mask (16 codes); otherwise a code per distinct mask that occurs, in increasing mask order -
    any numbering serves: the counts are indexed by it and nothing else is."""
    cmap = np.asarray(charmap, dtype=np.uint64)
    m = np.stack([cmap[np.frombuffer(s, dtype=np.uint8)] for s in sequences])
    assert (m != 0).all(), "a character without a state mask"
    if states == 4:
        return m.astype(np.uint8), np.arange(16, dtype=np.uint64)
    masks, codes = np.unique(m, return_inverse=True)
    assert len(masks) <= 256
    return codes.reshape(m.shape).astype(np.uint8), masks


def code_pair_counts(codes_a, codes_b, weights, ncodes):
    """n[a][b] as int64 [ncodes, ncodes]: exact, whatever the order of the sites"""
    a, b = np.asarray(codes_a, dtype=np.int64), np.asarray(codes_b, dtype=np.int64)
    n = np.zeros((ncodes, ncodes), dtype=np.int64)
    np.add.at(n, (a, b), np.asarray(weights, dtype=np.int64))
    return n


def p_distance(counts, masks, states):
    """sum of n[a][b] over code pairs with disjoint state sets / sum over code pairs where neither code is the all-states
    set; 0 where the latter is 0. Two integer sums, one division."""
    masks = np.asarray(masks, dtype=np.uint64)
    full = np.uint64((1 << states) - 1)
    disjoint = (masks[:, None] & masks[None, :]) == 0
    informative = (masks[:, None] != full) & (masks[None, :] != full)
    differ, compared = int(counts[disjoint].sum()), int(counts[informative].sum())
    return differ / compared if compared else 0.0


def code_vectors(masks, states, eigenvecs, inv_eigenvecs, freqs, params_indices):
    """(U, W), each [ncodes, rate_cats, states]; eigenvecs / inv_eigenvecs [rate_matrices][states][>= states] as the
    partition stores them (row i of inv_eigenvecs = state i, row j of eigenvecs = eigen index j), freqs [rate_matrices][states].
    The state sum runs in increasing state order."""
    S, R = states, len(params_indices)
    U, W = np.zeros((len(masks), R, S)), np.zeros((len(masks), R, S))
    for c, mask in enumerate(int(x) for x in masks):
        for k, m in enumerate(params_indices):
            V, Vinv, pi = np.asarray(eigenvecs[m])[:S, :S], np.asarray(inv_eigenvecs[m])[:S, :S], np.asarray(freqs[m])[:S]
            for i in range(S):
                if (mask >> i) & 1:
                    U[c, k] += pi[i] * Vinv[i]
                    W[c, k] += V[:, i]
    return U, W


def derivatives(counts, U, W, eigenvals, rates, rate_weights, params_indices, t):
    """(d_f, dd_f) of -lnL at t for a count table: per code pair that occurs the site's (L, L', L'') as
    pll_compute_likelihood_derivatives forms them (no invariant sites), weighted with n[a][b]"""
    S = U.shape[2]
    d_f = dd_f = 0.0
    for a, b in zip(*np.nonzero(counts)):
        lk = np.zeros(3)
        for k, m in enumerate(params_indices):
            lam = np.asarray(eigenvals[m])[:S] * rates[k]
            e = np.exp(lam * t)
            row = U[a, k] * W[b, k]
            lk += rate_weights[k] * np.array([np.dot(row, e), np.dot(row, lam * e), np.dot(row, lam * lam * e)])
        d1 = -lk[1] / lk[0]
        d_f += counts[a, b] * d1
        dd_f += counts[a, b] * (d1 * d1 - lk[2] / lk[0])
    return float(d_f), float(dd_f)


def ml_distance(counts, U, W, eigenvals, rates, rate_weights, params_indices, t_start, t_min, t_max, tolerance, max_iters):
    """-> (t, status, trace): the recipe of newton.host_newton on the count table; trace = the evaluations (t, d_f, dd_f),
    t = the last point evaluated"""
    t = min(max(float(t_start), float(t_min)), float(t_max))
    br = newton.Bracket(float(t_min), float(t_max))
    trace = []
    for _ in range(max_iters):
        d, dd = derivatives(counts, U, W, eigenvals, rates, rate_weights, params_indices, t)
        trace.append((t, d, dd))
        status, nxt = br.step(t, d, dd, tolerance)
        if status is not None:
            return t, status, trace
        t = nxt
    return trace[-1][0], newton.MAXITER, trace
