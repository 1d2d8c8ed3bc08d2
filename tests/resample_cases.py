"""What the resampling tests share - TEST INFRASTRUCTURE on top of insertion_cases / quartet_cases: the replicates'
weights, the reference values of pll_gpu_quartet_resampled_loglikelihoods and the call itself.

Reference: the reference library's per-edge path with a persite_lnl buffer per value (driver.quartet_persite_per_edge) on
a partition whose pattern weights are all 1 gives u, the per-site log-likelihoods before any weight; the resampled value of
(quartet i, replicate b, arrangement a) is math.fsum(w_b[n] * u[i, a, n]) - the exact sum of the rounded products."""
import math

import numpy as np

import quartet_cases as QC
from pllamd import driver


def weights(sites, replicates):
    """RELL replicates: `sites` draws over the sites, uniformly - rows of site counts that add up to `sites`"""
    rng = np.random.Generator(np.random.PCG64(11))
    w = rng.multinomial(sites, np.full(sites, 1.0 / sites), size=replicates).astype(np.uint32)
    if sites >= 64:  # a condition on the inputs: every replicate drops a site and repeats one
        assert (w.min(axis=1) == 0).all() and (w.max(axis=1) >= 2).all()
    return w


def resampled_from(u, w):
    """[Q, B, 3] from u [Q, 3, sites] and w [B, sites]: fsum of the rounded products"""
    u, wd = np.asarray(u), np.asarray(w, dtype=np.float64)
    out = np.empty((u.shape[0], wd.shape[0], 3))
    for i in range(u.shape[0]):
        for a in range(3):
            for b in range(wd.shape[0]):
                out[i, b, a] = math.fsum((wd[b] * u[i, a]).tolist())
    return out


def persite_per_edge(bed, rows, own=None):
    """(lnl [Q, 3], persite [Q, 3, sites]) through the two spare slots; own as quartet_cases.per_edge fills it"""
    lay = bed.lay

    def rescaled(tmp, children):
        count = bed.scaler(tmp[1]).astype(np.int64)
        for clv, sc, _ in children:
            if sc >= 0 and clv >= lay.tips:
                count -= bed.scaler(sc)
        return bool((count > 0).any())

    def after(i, a, first, second):
        own.append((rescaled(lay.tmp, first), rescaled(lay.cherry, second)))

    return driver.quartet_persite_per_edge(bed.lib, bed.p, rows, bed.fi, lay.tmp, lay.cherry, after if own is not None else None)


def call(bed, rows, w, want_persite=True):
    """(lnl, resampled, persite) from one call"""
    return driver.quartet_resampled_loglikelihoods(bed.lib, bed.p, rows, bed.fi, w, want_persite)


def prepare(bed):
    return QC.prepare(bed)


def stage2_bound(persite_u, w):
    """[Q, B, 3]: (sites + 3) 2^-53 sum_n w |u| - the worst case of ANY summation order of rounded or fused products
    (n - 1 additions and one rounding per product, first order, with room for the second)"""
    u, wd = np.abs(np.asarray(persite_u)), np.asarray(w, dtype=np.float64)
    mag = np.einsum("ian,bn->iba", u, wd)
    return (u.shape[2] + 3) * 2.0 ** -53 * mag
