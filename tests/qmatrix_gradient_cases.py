"""What the model-gradient tests share - TEST INFRASTRUCTURE: a numpy restatement of the definitions of
pll_gpu_qmatrix_gradient (include/pll_amd.h) and of the library's Q construction, with an eigen-decomposition of its own
(np.linalg.eigh of the symmetrised Q: the library's vectors are not used), fed with the REFERENCE's CLVs and scaling
counts of an insertion_cases.Bed and the rows of gradient_cases.prepare.

Besides each output the restatement returns the same sum with every term's absolute value (abs_q, abs_root): entries of d_q
are signed sums that cancel, so a tolerance for them scales with that sum."""
import numpy as np

from pllamd import api

MAXDIFF = 4  # PLL_SCALE_RATE_MAXDIFF


def exch_matrix(subst, states):
    """symmetric [S, S] exchangeabilities relative to the last one: s_p = subst[p] / subst[last]"""
    s = np.zeros((states, states))
    iu = np.triu_indices(states, 1)
    s[iu] = np.asarray(subst, dtype=np.float64) / subst[-1]
    return s + s.T


def q_matrix(subst, freqs):
    """a_xy = s_xy pi_y (x != y), a_xx = -sum_y a_xy, mean = 2 sum_{x<y} s_xy pi_x pi_y, Q = a / mean"""
    pi = np.asarray(freqs, dtype=np.float64)
    s = exch_matrix(subst, len(pi))
    a = s * pi[None, :]
    a -= np.diag(a.sum(axis=1))
    mean = float(np.sum(s * np.outer(pi, pi)))
    return a / mean


def eigensystem(q, freqs):
    """(lam, U, U^-1) with Q = U diag(lam) U^-1, from the symmetric D^1/2 Q D^-1/2"""
    pi = np.asarray(freqs, dtype=np.float64)
    r = np.sqrt(pi)
    sym = q * r[:, None] / r[None, :]
    lam, e = np.linalg.eigh((sym + sym.T) / 2.0)
    return lam, e / r[:, None], e.T * r[None, :]


def phi(lam, tau):
    """Phi[i][j] = tau e^{lam_j tau} g((lam_i - lam_j) tau), g(x) = expm1(x) / x, g(0) = 1 - written without positive
    exponents: tau e^{max tau} g(-|lam_i - lam_j| tau), the same number"""
    x = -np.abs(lam[:, None] - lam[None, :]) * tau
    safe = np.where(x == 0.0, 1.0, x)
    g = np.where(x == 0.0, 1.0, np.expm1(safe) / safe)
    return tau * np.exp(np.maximum(lam[:, None], lam[None, :]) * tau) * g


class Model:
    """the model of one partition: what the definitions name"""

    def __init__(self, freqs, subst, rates, weights, pinv, mi, pw, invariant=None, per_rate=False):
        self.freqs = [np.asarray(f, dtype=np.float64) for f in freqs]
        self.subst = [np.asarray(s, dtype=np.float64) for s in subst]
        self.rates, self.weights = np.asarray(rates, dtype=np.float64), np.asarray(weights, dtype=np.float64)
        self.pinv, self.mi = np.asarray(pinv, dtype=np.float64), [int(x) for x in mi]
        self.pw, self.invariant, self.per_rate = np.asarray(pw, dtype=np.float64), invariant, per_rate
        self.S, self.R, self.M, self.sites = len(self.freqs[0]), len(self.rates), len(self.freqs), len(self.pw)
        self.q = [q_matrix(self.subst[m], self.freqs[m]) for m in range(self.M)]
        self.eig = [eigensystem(self.q[m], self.freqs[m]) for m in range(self.M)]

    @classmethod
    def from_bed(cls, bed, params_indices):
        """read from the partition's host fields"""
        part = bed.part
        S, R, M, sites = int(part.states), int(part.rate_cats), int(part.rate_matrices), int(part.sites)
        return cls([api.as_np(part.frequencies[m], S, np.float64).copy() for m in range(M)],
                   [api.as_np(part.subst_params[m], S * (S - 1) // 2, np.float64).copy() for m in range(M)],
                   api.as_np(part.rates, R, np.float64).copy(), api.as_np(part.rate_weights, R, np.float64).copy(),
                   api.as_np(part.prop_invar, M, np.float64).copy(), params_indices,
                   api.as_np(part.pattern_weights, sites, np.uint32).astype(np.float64),
                   api.as_np(part.invariant, sites, np.int32).copy() if part.invariant else None, bool(bed.attrs & api.RATE_SCALERS))


def read_ends(bed, rows):
    """{(clv, scaler): (clv [sites, R, S], per-rate counts [sites, R] or None)} of every end the rows name, from a
    partition whose tips are dense (the reference's, attributes without PLL_ATTRIB_PATTERN_TIP)"""
    part = bed.part
    S, R, sp, sites = int(part.states), int(part.rate_cats), int(part.states_padded), int(part.sites)
    per_rate = bool(bed.attrs & api.RATE_SCALERS)
    out = {}
    for p, ps, c, cs, _ in rows:
        for key in ((p, ps), (c, cs)):
            if key in out:
                continue
            clv = api.as_np(part.clv[key[0]], sites * R * sp, np.float64).reshape(sites, R, sp)[:, :, :S].copy()
            counts = None
            if per_rate and key[1] >= 0 and key[0] >= int(part.tips):
                counts = bed.scaler(key[1]).astype(np.int64).reshape(sites, R)
            out[key] = (clv, counts)
    return out


def restate(model, ends, rows):
    """d_q [M, S, S], d_root [M, S], abs_q, abs_root of the definitions, and L [count, sites]"""
    S, R, M = model.S, model.R, model.M
    W = np.zeros((M, S, S))
    Wabs = np.zeros((M, S, S))
    G = np.zeros((M, S, S))
    Gabs = np.zeros((M, S, S))
    Ls = []
    for b, (p, ps, c, cs, t) in enumerate(rows):
        pclv, pcnt = ends[(p, ps)]
        cclv, ccnt = ends[(c, cs)]
        f = np.ones((model.sites, R))
        if model.per_rate:
            s = np.zeros((model.sites, R), dtype=np.int64)
            for cnt in (pcnt, ccnt):
                if cnt is not None:
                    s = s + cnt
            f = np.ldexp(1.0, (-256 * np.minimum(s - s.min(axis=1, keepdims=True), MAXDIFF)).astype(np.int64))
        A, B, c0, taus = [], [], [], []
        L = np.zeros(model.sites)
        for k in range(R):
            m = model.mi[k]
            lam, U, Ui = model.eig[m]
            pi, pinv = model.freqs[m], model.pinv[m]
            tau = model.rates[k] * t / (1.0 - pinv)
            Ak = (pclv[:, k, :] * pi[None, :]) @ U
            Bk = cclv[:, k, :] @ Ui.T
            ck = np.sum(Ak * Bk * np.exp(lam * tau)[None, :], axis=1) * f[:, k]
            if pinv > 0.0:
                inv = model.invariant
                isl = np.where(inv >= 0, pi[np.maximum(inv, 0)] * pinv, 0.0) if inv is not None else 0.0
                ck = ck * (1.0 - pinv) + isl
            L += model.weights[k] * ck
            A.append(Ak), B.append(Bk), taus.append(tau)
        Ls.append(L)
        for k in range(R):
            m = model.mi[k]
            lam = model.eig[m][0]
            g = model.pw * model.weights[k] * (1.0 - model.pinv[m]) * f[:, k] / L
            H = (A[k] * g[:, None]).T @ B[k]
            Habs = (np.abs(A[k]) * np.abs(g)[:, None]).T @ np.abs(B[k])
            ph = phi(lam, taus[k])
            W[m] += ph * H
            Wabs[m] += np.abs(ph) * Habs
            if b == 0:
                e = np.exp(lam * taus[k])[None, :]
                G[m] += e * H
                Gabs[m] += e * Habs
    d_q, abs_q = np.zeros((M, S, S)), np.zeros((M, S, S))
    d_root, abs_root = np.zeros((M, S)), np.zeros((M, S))
    for m in range(M):
        _, U, Ui = model.eig[m]
        pi = model.freqs[m]
        d_q[m] = -(Ui.T @ W[m] @ U.T)
        abs_q[m] = np.abs(Ui).T @ Wabs[m] @ np.abs(U).T
        d_root[m] = -np.einsum("ix,ij,xj->x", Ui, G[m], U) / pi
        abs_root[m] = np.einsum("ix,ij,xj->x", np.abs(Ui), Gabs[m], np.abs(U)) / pi
    return {"d_q": d_q, "d_root": d_root, "abs_q": abs_q, "abs_root": abs_root, "L": np.array(Ls)}


def chain_rule(subst, freqs, d_q, d_root=None, h=None):
    """d_subst, d_freqs by a numeric Jacobian of q_matrix (central differences at step h relative to each parameter):
    d F / d theta = sum_xy d_q[x][y] dQ[x][y] / d theta, plus d_root for the frequencies"""
    subst, freqs = np.asarray(subst, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
    h = 2.0 ** -20 if h is None else h
    d_subst, d_freqs = np.zeros(len(subst)), np.zeros(len(freqs))
    for p in range(len(subst)):
        e = np.zeros(len(subst))
        e[p] = h * subst[p]
        d_subst[p] = np.sum(d_q * (q_matrix(subst + e, freqs) - q_matrix(subst - e, freqs))) / (2.0 * e[p])
    for x in range(len(freqs)):
        e = np.zeros(len(freqs))
        e[x] = h * freqs[x]
        d_freqs[x] = np.sum(d_q * (q_matrix(subst, freqs + e) - q_matrix(subst, freqs - e))) / (2.0 * e[x])
    if d_root is not None:
        d_freqs = d_freqs + d_root
    return d_subst, d_freqs


def blocks_by_rule(states, rate_cats, sites):
    """the workgroups per branch: the cutting rule of include/pll_amd_device.h, pllgpu_qmatrix_gradient"""
    tiles = (sites + 63) // 64
    if states == 4 and rate_cats == 4:
        w = (tiles + 4 * 64 - 1) // (4 * 64)
        return (tiles + 4 * w - 1) // (4 * w)
    pad = (states + 15) // 16 * 16
    m = min(64, max(4, 16384 // (pad * pad)))
    w = (tiles + m - 1) // m
    return (tiles + w - 1) // w


def per_launch_by_rule(states, rate_cats, sites, count, used_matrices=1, root=True):
    v = used_matrices * states * states * (2 if root else 1)
    return min(count, 8192, max(1, (4 << 20) // (v * blocks_by_rule(states, rate_cats, sites))))


def launches_by_rule(states, rate_cats, sites, count, used_matrices=1, root=True):
    q = per_launch_by_rule(states, rate_cats, sites, count, used_matrices, root)
    return 3 * ((count + q - 1) // q) + 1
