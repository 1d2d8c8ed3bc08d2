"""What the ancestral-state tests share - TEST INFRASTRUCTURE: the tolerance of a table of marginal state probabilities
and the numpy restatement that stands in for the reference where it ignores per-rate scaling counts.

Tolerance: every entry within RTOL (1e-10) relative of the expected one - every term of an entry is non-negative, nothing
cancels -, an entry expected as exactly 0 is 0, every row sums to 1 within 1e-12.

With PLL_ATTRIB_RATE_SCALERS the library honours the per-rate scaling counts of both ends, the reference does not
(src/likelihood.c:711-743): there the expected values are `restated`, a numpy restatement of

    a[n][j] = sum_k w_k pi_f(k)[j] x_k[n][j] (P_k y_k[n])[j] 2^(-256 min(count_k[n] - min_k count[n], 4)),   a[n] /= sum_j a[n][j]

fed with the REFERENCE's CLVs, tip codes, matrices and scaler vectors (read from its partition's host memory; nothing
comes from the library under test)."""
import numpy as np

from compare import RTOL
from pllamd import api

SUMTOL = 1e-12


def assert_table(got, exp, what):
    """got against exp under the tolerance of this file; returns the worst relative error"""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert np.isfinite(exp).all(), (what, "the expected table has non-finite rows", np.argwhere(~np.isfinite(exp).all(1))[:5])
    assert np.isfinite(got).all(), (what, "non-finite rows", np.argwhere(~np.isfinite(got).all(1))[:5])
    zero = exp == 0
    assert (got[zero] == 0).all(), (what, "an entry expected as exactly 0 is not")
    rel = np.zeros_like(exp)
    rel[~zero] = np.abs(got[~zero] - exp[~zero]) / exp[~zero]
    worst = float(rel.max()) if rel.size else 0.0
    assert worst <= RTOL, (what, worst, np.unravel_index(int(rel.argmax()), rel.shape))
    rows = np.abs(got.sum(1) - 1.0)
    assert rows.max() <= SUMTOL, (what, "row sum", float(rows.max()))
    return worst


def _part_arrays(lib, p, node, nscaler, other, oscaler, matrix):
    """what the formula reads, from the HOST memory of partition p (the reference's): x, y [sites][rates][states],
    P [rates][states][states], and the per-rate counts of both ends summed [sites][rates] (None without RATE_SCALERS)"""
    part = p.contents
    s, sp, r, n = part.states, part.states_padded, part.rate_cats, part.sites
    per_rate = bool(part.attributes & api.RATE_SCALERS)

    def clv(idx):
        if idx < part.tips and (part.attributes & api.PATTERN_TIP):
            codes = api.as_np(part.tipchars[idx], n, np.uint8)
            if s == 4:
                masks = codes.astype(np.uint64)
            else:
                masks = api.as_np(part.tipmap, part.maxstates, np.uint64)[codes]
            y = ((masks[:, None] >> np.arange(s, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64)
            return np.repeat(y[:, None, :], r, axis=1)
        return api.as_np(part.clv[idx], n * r * sp, np.float64).reshape(n, r, sp)[:, :, :s].copy()

    def counts(idx):
        if idx < 0:
            return np.zeros((n, r if per_rate else 1), dtype=np.int64)
        return api.as_np(part.scale_buffer[idx], n * (r if per_rate else 1), np.uint32).reshape(n, -1).astype(np.int64)

    pm = api.as_np(part.pmatrix[matrix], r * s * sp, np.float64).reshape(r, s, sp)[:, :, :s].copy()
    other_is_codes = other < part.tips and bool(part.attributes & api.PATTERN_TIP)
    cn, co = counts(nscaler), (counts(-1) if other_is_codes else counts(oscaler))
    return clv(node), clv(other), pm, (cn + co) if per_rate else None, (cn, co)


def restated(lib, p, edge, fi):
    """the formula of the module docstring on partition p's host arrays"""
    part = p.contents
    x, y, pm, rs, _ = _part_arrays(lib, p, *edge)
    s, sp, r = part.states, part.states_padded, part.rate_cats
    v = x * np.einsum("kij,nkj->nki", pm, y)
    if rs is not None:
        ex = np.minimum(rs - rs.min(1, keepdims=True), 4)
        v = v * np.ldexp(1.0, (-256 * ex).astype(np.int64))[:, :, None]
    w = api.as_np(part.rate_weights, r, np.float64)
    pi = np.stack([api.as_np(part.frequencies[int(f)], sp, np.float64)[:s] for f in fi])
    a = np.einsum("k,kj,nkj->nj", w, pi, v)
    return a / a.sum(1, keepdims=True)
