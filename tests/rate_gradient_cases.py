"""What the rate-gradient tests share - TEST INFRASTRUCTURE: the expected values of pll_gpu_branch_category_derivatives,
derived from the REFERENCE alone, their tolerance, the restatement of pll_gpu_rate_gradient's two sums and the cutting
rule of include/pll_amd_device.h (pllgpu_branch_category_derivatives).

The per-category oracle. For a branch at its length, with the branch's matrix in a matrix slot:

    post[n][k] = category_common.expected(...)["posterior"]   the reference's persite_lnl under one-hot category weights
    q_k[n]     = the reference's d_f from pll_update_sumtable (once per branch) + pll_compute_likelihood_derivatives under
                 the unit category row e_k and the unit pattern-weight vector e_n: one-hot weights make that -c1_k / c0_k.
                 The vector is handed over as 2 e_n and the result halved (both exact): the reference's AVX2 kernel takes
                 four neighbouring weights whose bitwise OR is 1 as four ones ("assumption: no zero weights",
                 src/core_derivatives_avx2.c:1766-1773), so under e_n itself it returns the sum over the site's block of four
    exp[k]     = sum_n pw[n] post[n][k] q_k[n]                 = sum_n pw[n] (- w_k c1_k[n] / lk0[n])
    A[k]       = sum_n pw[n] post[n][k] |q_k[n]|               the scale of the tolerance: a category's sum may cancel

A value passes within DTOL A[k] + 4e-15 sum(pw) (deriv_common.DTOL). The likelihood code and the derivative code treat a
scaled invariant site differently (finish_site's rule), so the oracle is used only where they coincide: prop_invar > 0
only where the ends carry no scaling counts (asserted here from the reference's scale buffers), scaled ends only with
prop_invar = 0."""
import ctypes as C

import numpy as np

import category_common as CC
import gradient_cases as GC
from deriv_common import DTOL
from pllamd import api, driver

FLOOR = 4e-15


def edge_rows(bed):
    """GC.prepare's rows (full traversal + upward CLVs) and, per row, the matrix slot that holds the edge at its own length"""
    rows = GC.prepare(bed)
    return rows, [r.pm for r in bed.lay.tree.edges()]


def _aligned(n):
    raw = np.zeros(n + 8, dtype=np.float64)
    off = (-raw.ctypes.data // 8) % 8
    return raw[off:off + n]


def oracle(ref_lib, bed, rows, matrices, weights=None):
    """(exp [count, R], A [count, R], d_f [count]) of the rows from the reference's partition behind `bed` (module
    docstring); d_f is the reference's own under the real weights. The partition's weights and pattern weights are put back."""
    p, part = bed.p, bed.p.contents
    n, r = int(part.sites), int(part.rate_cats)
    fi = bed.fi
    pinv = api.as_np(part.prop_invar, part.rate_matrices, np.float64)
    if (pinv > 0).any():
        for pclv, psc, cclv, csc, _ in rows:
            assert not CC.summed_counts(p, (pclv, psc, cclv, csc, 0)).any(), "prop_invar > 0 on ends that carry scaling counts"
    own = api.as_np(part.rate_weights, r, np.float64).copy()
    w = own if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    pw = api.as_np(part.pattern_weights, n, np.uint32).copy()
    table = _aligned(n * r * int(part.states_padded))
    exp, scale, d_f = np.zeros((len(rows), r)), np.zeros((len(rows), r)), np.zeros(len(rows))
    d1, d2 = C.c_double(0), C.c_double(0)
    try:
        for i, ((pclv, psc, cclv, csc, t), m) in enumerate(zip(rows, matrices)):
            ref_lib.pll_set_category_weights(p, api.dptr(w))
            post = CC.expected(ref_lib, p, (pclv, psc, cclv, csc, m), fi, weights=w)["posterior"]
            assert ref_lib.pll_update_sumtable(p, int(pclv), int(cclv), int(psc), int(csc), api.uptr(fi), api.dptr(table))
            ref_lib.pll_set_category_weights(p, api.dptr(w))
            ref_lib.pll_set_pattern_weights(p, api.uptr(pw))
            assert ref_lib.pll_compute_likelihood_derivatives(p, int(psc), int(csc), float(t), api.uptr(fi), api.dptr(table), C.byref(d1), C.byref(d2))
            d_f[i] = d1.value
            q = np.zeros((n, r))
            e_n = np.zeros(n, dtype=np.uint32)
            for k in range(r):
                e_k = np.zeros(r)
                e_k[k] = 1.0
                ref_lib.pll_set_category_weights(p, api.dptr(e_k))
                for s in range(n):
                    e_n[s] = 2
                    ref_lib.pll_set_pattern_weights(p, api.uptr(e_n))
                    e_n[s] = 0
                    assert ref_lib.pll_compute_likelihood_derivatives(p, int(psc), int(csc), float(t), api.uptr(fi), api.dptr(table), C.byref(d1),
                                                                      C.byref(d2))
                    q[s, k] = 0.5 * d1.value
            assert np.isfinite(post).all() and np.isfinite(q).all() and np.isfinite(d_f[i]), "the reference's own values are not finite"
            exp[i] = (pw[:, None] * post * q).sum(0)
            scale[i] = (pw[:, None] * post * np.abs(q)).sum(0)
    finally:
        ref_lib.pll_set_pattern_weights(p, api.uptr(pw))
        ref_lib.pll_set_category_weights(p, api.dptr(own))
    return exp, scale, d_f


def bound(scale, weight_sum):
    return DTOL * np.asarray(scale) + FLOOR * weight_sum


def worst(got, exp, scale, weight_sum):
    """the largest |d| / (DTOL A + 4e-15 sum(pw)): at most 1 where the values pass"""
    return float(np.max(np.abs(np.asarray(got) - exp) / bound(scale, weight_sum)))


def assert_categories(got_cat, exp, scale, d_f, weight_sum, what):
    """every d_cat against the oracle, and sum_k d_cat against the reference's d_f within DTOL sum_k A + 4e-15 sum(pw); the
    worst fractions of the two bounds"""
    got_cat = np.asarray(got_cat)
    assert got_cat.shape == exp.shape and np.isfinite(got_cat).all(), what
    w_cat = worst(got_cat, exp, scale, weight_sum)
    w_sum = worst(got_cat.sum(1), d_f, scale.sum(1), weight_sum)
    print(f"{what}: d_cat worst {w_cat:.3f} of the bound, sum_k d_cat against d_f worst {w_sum:.3f}")
    assert w_cat <= 1.0, (what, "d_cat", w_cat)
    assert w_sum <= 1.0, (what, "sum over the categories", w_sum)
    return w_cat, w_sum


def sum_identity(got_cat, ref_d_f, weight_sum):
    """the worst fraction of the bound of sum_k d_cat[i][k] against the reference's d_f[i] where no per-category oracle was
    run: sum_k A[i][k] >= |d_f[i]| (the triangle inequality), so DTOL |d_f| + 4e-15 sum(pw) asks no less than
    DTOL sum_k A + 4e-15 sum(pw)"""
    ref_d_f = np.asarray(ref_d_f)
    return worst(np.asarray(got_cat).sum(1), ref_d_f, np.abs(ref_d_f), weight_sum)


def restated(d_cat, d_f, lengths, rates):
    """(d_rates, d_scale) as the header defines them: each product rounded, then added in list order, left to right"""
    d_cat, d_f = np.asarray(d_cat, dtype=np.float64), np.asarray(d_f, dtype=np.float64)
    rates = np.asarray(rates, dtype=np.float64)
    acc, scale = np.zeros(len(rates)), np.float64(0.0)
    for i, t in enumerate(np.asarray(lengths, dtype=np.float64)):
        acc = acc + (t / rates) * d_cat[i]
        scale = scale + t * d_f[i]
    return acc, float(scale)


def blocks_by_rule(states, rate_cats, sites):
    """B of include/pll_amd_device.h: the workgroups per branch"""
    tiles = (sites + 63) // 64
    if states == 4 and rate_cats == 4:
        w = (tiles + 4095) // 4096
        return (tiles + 4 * w - 1) // (4 * w)
    w = (tiles + 1023) // 1024
    return (tiles + w - 1) // w


def per_launch_by_rule(states, rate_cats, sites, count):
    """Q of pllgpu_branch_category_derivatives: R + 2 partial sums per workgroup"""
    return min(count, 8192, max(1, (4 << 20) // ((rate_cats + 2) * blocks_by_rule(states, rate_cats, sites))))


def launches_by_rule(states, rate_cats, sites, count, contraction=False):
    q = per_launch_by_rule(states, rate_cats, sites, count)
    return (count + q - 1) // q + (1 if contraction else 0)


def category_derivatives(bed, rows, **kw):
    return driver.branch_category_derivatives(bed.lib, bed.p, rows, bed.fi, **kw)


def rate_gradient(bed, rows, **kw):
    return driver.rate_gradient(bed.lib, bed.p, rows, bed.fi, **kw)
