"""What the rate-category tests share - TEST INFRASTRUCTURE: the expected values of
pll_gpu_edge_category_posteriors / pll_gpu_category_weights_em, derived from the REFERENCE alone, and the tolerances.

With one_k the reference's persite_lnl under pll_set_category_weights(e_k) (the k-th unit row) and full the one under the
real weights w, both with pattern weights 1:

    posterior[n][k] = w_k exp(one_k[n] - full[n])          (the same prop_invar for every category)
    cat_lnl[n][k]   = one_k[n]                             (prop_invar 0; at a variable site otherwise: - log(1 - pinv))
                      - 256 ln2 (s - c - 4) where the count s[n][k] of the pair exceeds the site's smallest c[n] by more
                      than the cap 4, from the integers in the reference's scale buffers
    weight_sums[k]  = sum_n pw[n] posterior[n][k]
    site_rates[n]   = sum_k (posterior[n][k] - I[n][k] / L[n]) r_k,   I = w_k pinv pi_f(k)[inv_n] at an invariant site,
                      L[n] = exp(full[n]) there (finish_site takes the logarithm of the whole sum at such a site)
    lnl             = the reference's pll_compute_edge_loglikelihood under w and the real pattern weights

Tolerances (the project's): a log value within RTOL max(1, |exp|); a probability or sum within RTOL relative, an entry
expected as exactly 0 is 0; rows of posterior sum to 1 within SUMTOL.
A site rate is the difference P - Q of two sums the reference gives to RTOL relative each, P = sum_k posterior r_k and
Q = sum_k (I / L) r_k: it passes within RTOL (P + Q), which is RTOL relative wherever Q = 0 - every site without an
invariant share. At a scaled invariant site P and Q agree to 77 digits and more (the variable share is 2^-256 and below):
there the reference says that the rate is 0 to within RTOL (P + Q) and nothing finer."""
import numpy as np

from ancestral_common import SUMTOL, assert_table
from compare import RTOL
from pllamd import api

OUTPUTS = ("cat_lnl", "posterior", "site_rates", "weight_sums", "lnl")
LOG_THRESHOLD = -256.0 * np.log(2.0)
CAP = 4  # PLL_SCALE_RATE_MAXDIFF
BASE_WEIGHTS = (0.1, 0.2, 0.3, 0.4)


def weights_for(rate_cats):
    """the non-uniform weights of the tests, cycled to rate_cats"""
    return np.array([BASE_WEIGHTS[k % 4] for k in range(rate_cats)])


def pattern_weights_for(sites):
    return (1 + (np.arange(sites) * 7 % 5 == 0) + 2 * (np.arange(sites) % 11 == 3)).astype(np.uint32)


def call(lib, p, edge, fi, want=OUTPUTS):
    """pll_gpu_edge_category_posteriors -> dict of the outputs in `want` (lnl as a float)"""
    part = p.contents
    n, r = part.sites, part.rate_cats
    shapes = {"cat_lnl": (n, r), "posterior": (n, r), "site_rates": (n,), "weight_sums": (r,), "lnl": (1,)}
    out = {k: np.full(shapes[k], -7.0) for k in OUTPUTS if k in want}
    ok = lib.pll_gpu_edge_category_posteriors(p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(fi),
                                              *[api.dptr(out[k]) if k in out else None for k in OUTPUTS])
    assert ok, (edge, want, lib.errno(), lib.errmsg())
    if "lnl" in out:
        out["lnl"] = float(out["lnl"][0])
    return out


def em(lib, p, edge, fi, start, steps):
    r = p.contents.rate_cats
    w, lnl = np.full((steps + 1, r), -7.0), np.full(steps + 1, -7.0)
    s = None if start is None else np.ascontiguousarray(start, dtype=np.float64)
    ok = lib.pll_gpu_category_weights_em(p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(fi), None if s is None else api.dptr(s), steps,
                                         api.dptr(w), api.dptr(lnl))
    assert ok, (edge, steps, lib.errno(), lib.errmsg())
    return w, lnl


def _persite(lib, p, edge, fi):
    ps = np.zeros(p.contents.sites)
    v = lib.pll_compute_edge_loglikelihood(p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(fi), api.dptr(ps))
    return v, ps


def summed_counts(p, edge):
    """s[n][k]: the counts of both ends added, from the partition's scale buffers (an end given by codes under
    PLL_ATTRIB_PATTERN_TIP or without a scaler counts 0); [sites][rate_cats]"""
    part = p.contents
    n, r = part.sites, part.rate_cats
    per = r if part.attributes & api.RATE_SCALERS else 1
    s = np.zeros((n, r), dtype=np.int64)
    for clv, scaler in ((edge[0], edge[1]), (edge[2], edge[3])):
        if scaler < 0 or (clv < part.tips and (part.attributes & api.PATTERN_TIP)):
            continue
        s += api.as_np(part.scale_buffer[scaler], n * per, np.uint32).reshape(n, per).astype(np.int64)
    return s


def expected(ref_lib, p, edge, fi, weights=None, rates=None):
    """the expected outputs from the reference's partition p (module docstring) under `weights` (default: the partition's
    own); the partition's weights and pattern weights are put back"""
    part = p.contents
    n, r, sp = part.sites, part.rate_cats, part.states_padded
    own = api.as_np(part.rate_weights, r, np.float64).copy()
    w = own if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    pw = api.as_np(part.pattern_weights, n, np.uint32).copy()
    ones = np.ones(n, dtype=np.uint32)
    one = np.zeros((n, r))
    try:
        ref_lib.pll_set_pattern_weights(p, api.uptr(ones))
        for k in range(r):
            e_k = np.zeros(r)
            e_k[k] = 1.0
            ref_lib.pll_set_category_weights(p, api.dptr(e_k))
            one[:, k] = _persite(ref_lib, p, edge, fi)[1]
        ref_lib.pll_set_category_weights(p, api.dptr(w))
        full = _persite(ref_lib, p, edge, fi)[1]
        ref_lib.pll_set_pattern_weights(p, api.uptr(pw))
        lnl = _persite(ref_lib, p, edge, fi)[0]
    finally:
        ref_lib.pll_set_pattern_weights(p, api.uptr(pw))
        ref_lib.pll_set_category_weights(p, api.dptr(own))
    assert np.isfinite(full).all() and np.isfinite(lnl), "the reference's own values are not finite"
    exp = {"lnl": float(lnl), "one": one, "full": full}
    exp["posterior"] = w[None, :] * np.exp(one - full[:, None])
    exp["weight_sums"] = (pw[:, None] * exp["posterior"]).sum(0)
    # cat_lnl
    pinv = np.array([api.as_np(part.prop_invar, part.rate_matrices, np.float64)[int(f)] for f in fi])
    assert (pinv == pinv[0]).all(), "the identity needs one prop_invar for every category"
    s = summed_counts(p, edge)
    over = np.maximum(s - s.min(1, keepdims=True) - CAP, 0)
    cat = one + over * LOG_THRESHOLD
    inv = api.as_np(part.invariant, n, np.int32) if pinv[0] > 0 else np.full(n, -1)
    exp["invariant"] = inv >= 0
    exp["scaled"] = s.min(1) > 0
    exp["over_cap"] = over > 0
    exp["at_cap"] = (s - s.min(1, keepdims=True)) >= CAP  # the reference mixes l 2^-1024 there: a subnormal number
    if pinv[0] > 0:
        cat = cat - np.log1p(-pinv[0])
        cat[inv >= 0] = np.nan  # not available from the reference at an invariant site
    exp["cat_lnl"] = cat
    # site rates
    if rates is not None:
        share = np.zeros((n, r))
        if pinv[0] > 0:
            pi = np.stack([api.as_np(part.frequencies[int(f)], sp, np.float64) for f in fi])  # [rates][states_padded]
            hit = inv >= 0
            share[hit] = w[None, :] * pinv[None, :] * pi[:, inv[hit]].T / np.exp(full[hit])[:, None]
        rr = np.asarray(rates, dtype=np.float64)
        exp["site_rates"] = (exp["posterior"] - share) @ rr
        exp["site_rates_scale"] = (exp["posterior"] + share) @ rr
    return exp


def worst_log(got, exp):
    ok = np.isfinite(exp)
    return float(np.max(np.abs(got[ok] - exp[ok]) / np.maximum(1.0, np.abs(exp[ok])))) if ok.any() else 0.0


def worst_rel(got, exp):
    nz = exp != 0
    return float(np.max(np.abs(got[nz] - exp[nz]) / np.abs(exp[nz]))) if nz.any() else 0.0


def assert_outputs(got, exp, what, pattern_weights=None):
    """every output in `got` against `exp` under the tolerances of this file -> the worst figures, by output"""
    fig = {}
    if "cat_lnl" in got:
        assert np.isfinite(got["cat_lnl"]).all(), (what, "cat_lnl")
        fig["cat_lnl"] = worst_log(got["cat_lnl"], exp["cat_lnl"])
    if "posterior" in got:
        fig["posterior"] = worst_rel(got["posterior"], exp["posterior"])
        fig["row_sum"] = float(np.abs(got["posterior"].sum(1) - 1.0).max())
    if "site_rates" in got and "site_rates" in exp:
        assert np.isfinite(got["site_rates"]).all() and (got["site_rates"] >= 0).all(), (what, "site_rates")
        fig["site_rates"] = float(np.max(np.abs(got["site_rates"] - exp["site_rates"]) / exp["site_rates_scale"]))
    if "weight_sums" in got:
        fig["weight_sums"] = worst_rel(got["weight_sums"], exp["weight_sums"])
    if "lnl" in got:
        fig["lnl"] = abs(got["lnl"] - exp["lnl"]) / max(1.0, abs(exp["lnl"]))
    print("categories", what, " ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    if "posterior" in got:
        assert_table(got["posterior"], exp["posterior"], (what, "posterior"))
        assert fig["row_sum"] <= SUMTOL, (what, "row sum", fig["row_sum"])
    if "weight_sums" in fig:
        assert np.isfinite(got["weight_sums"]).all() and ((got["weight_sums"] == 0) | (exp["weight_sums"] != 0)).all(), (what, "weight_sums")
        assert fig["weight_sums"] <= RTOL, (what, "weight_sums", fig["weight_sums"])
    for k in ("cat_lnl", "lnl", "site_rates"):
        if k in fig:
            assert fig[k] <= RTOL, (what, k, fig[k])
    return fig
