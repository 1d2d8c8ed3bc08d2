"""CPU (no GPU): pll_gpu_branch_category_derivatives and pll_gpu_rate_gradient are declared, exported and bound with their
device entry, the device header states the R + 2 cutting rule, the arithmetic of the definitions and of the tests' oracle
holds on a two-taxon toy in plain numpy, and everything the calls decide before a device is needed - the zero-count rule,
the checks in their stated order, the refusals, the rate check - on host-only partitions (PLL_AMD_HOST_ONLY=1). A failed
call leaves every output as it found it."""
import os
import re

import numpy as np
import pytest
from scipy.linalg import expm

import rate_gradient_cases as RG
from pllamd import api, workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIPS, INNER, SITES, MATRICES = 7, 6, 20, 9  # (below 16 sites site repeats are switched off)
SENTINEL = -12345.5
SEQ = b"ACGTACGTACGTACGTACGT"
GOOD = [(TIPS, 0, TIPS + 1, 1, 0.1), (TIPS + 2, 2, 0, -1, 0.25), (3, 4, TIPS + 5, -1, 0.0), (TIPS + 4, -1, TIPS + 3, 5, 1.5)]
INVALID, UNSUPPORTED, UNAVAILABLE = api.ERROR_PARAM_INVALID, api.ERROR_GPU_UNSUPPORTED, api.ERROR_GPU_UNAVAILABLE


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


# ---- declared, exported, bound ---------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    assert re.search(r"\bint pll_gpu_branch_category_derivatives\(", hdr) and re.search(r"\bint pll_gpu_rate_gradient\(", hdr)
    assert hdr.index("int pll_gpu_branch_derivatives(") < hdr.index("int pll_gpu_branch_category_derivatives(") < hdr.index("int pll_gpu_rate_gradient(")
    assert getattr(amd_lib.dll, "pll_gpu_branch_category_derivatives") and getattr(amd_lib.dll, "pll_gpu_rate_gradient")
    assert len(amd_lib.pll_gpu_branch_category_derivatives.argtypes) == 7 and len(amd_lib.pll_gpu_rate_gradient.argtypes) == 8
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert re.search(r"\bint pllgpu_branch_category_derivatives\(", dev) and getattr(amd_lib.dll, "pllgpu_branch_category_derivatives")


def test_the_device_header_states_the_cutting_rule():
    dev = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "pll_amd_device.h")).read())
    assert "Q = min(count, PLLGPU_BRANCH_MAX, max(1, floor(PLLGPU_INSERTION_MAX_SLOTS / ((R + 2) B))))" in dev
    assert "Q = min(count, PLLGPU_BRANCH_MAX, max(1, floor(PLLGPU_INSERTION_MAX_SLOTS / (2 B))))" in dev  # the old entry keeps its own
    assert re.search(r"#define PLLGPU_BRANCH_MAX 8192\b", dev) and re.search(r"#define PLLGPU_INSERTION_MAX_SLOTS \(?4u? ?<< ?20\)?|#define PLLGPU_INSERTION_MAX_SLOTS 4194304", dev)
    # ... and the helper restates it: one workgroup, sixteen workgroups, the 4 x 4 form
    assert RG.per_launch_by_rule(4, 33, 33, 1 << 30) == 8192
    assert RG.per_launch_by_rule(4, 33, 961, 1 << 30) == (4 << 20) // (35 * 16) == 7489
    assert RG.per_launch_by_rule(4, 4, 100000, 125) == 125 and RG.launches_by_rule(4, 4, 100000, 125, contraction=True) == 2
    assert RG.launches_by_rule(4, 33, 961, 7490) == 2 and RG.launches_by_rule(4, 33, 961, 7489) == 1


# ---- the arithmetic on a toy -----------------------------------------------------------------------------------------
def _toy(pinv, seed=5, sites=23, cats=4):
    """two taxa joined by one branch: Q (GTR, normalised), its eigensystem, tip vectors, weights, rates"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pi = np.asarray(W.GTR_DNA["freqs"], dtype=np.float64)
    ex = np.asarray(W.GTR_DNA["exch"], dtype=np.float64)
    q = np.zeros((4, 4))
    q[np.triu_indices(4, 1)] = ex
    q = (q + q.T) * pi[None, :]
    np.fill_diagonal(q, -q.sum(1))
    q /= -(pi * np.diag(q)).sum()
    sq = np.sqrt(pi)
    lam, u = np.linalg.eigh(sq[:, None] * q / sq[None, :])
    v, vinv = u / sq[:, None], u.T * sq[None, :]  # Q = v diag(lam) vinv
    assert np.allclose(v @ np.diag(lam) @ vinv, q, atol=1e-13)
    x = np.eye(4)[rng.integers(0, 4, sites)]
    y = np.eye(4)[np.where(rng.random(sites) < 0.4, x.argmax(1), rng.integers(0, 4, sites))]
    inv = np.where(x.argmax(1) == y.argmax(1), x.argmax(1), -1)
    w = np.array([0.1, 0.2, 0.3, 0.4])[:cats]
    pw = (1 + np.arange(sites) % 3).astype(np.float64)
    return dict(pi=pi, q=q, lam=lam, v=v, vinv=vinv, x=x, y=y, inv=inv, w=w / w.sum(), pw=pw, rates=W.gamma_rates_mean(0.7, cats), pinv=pinv, t=0.37)


def _toy_terms(m, rates=None, t=None):
    """(c0, c1) [sites, cats] as the kernels form them: the table row contracted with (e, l e), after the pinv step"""
    rates = m["rates"] if rates is None else rates
    t = m["t"] if t is None else t
    row = ((m["x"] * m["pi"]) @ m["v"]) * (m["y"] @ m["vinv"].T)  # [sites, j]
    ki = rates / (1.0 - m["pinv"])
    e = np.exp(m["lam"][None, :] * ki[:, None] * t)              # [cats, j]
    c0 = row @ e.T
    c1 = row @ (m["lam"][None, :] * ki[:, None] * e).T
    isl = np.where(m["inv"] >= 0, m["pi"][np.maximum(m["inv"], 0)] * m["pinv"], 0.0)
    return c0 * (1.0 - m["pinv"]) + isl[:, None], c1 * (1.0 - m["pinv"])


def _toy_lnl(m, rates, t):
    """the same likelihood with no eigensystem: transition matrices by scipy's expm"""
    site = np.zeros(len(m["x"]))
    for k, r in enumerate(rates):
        p = expm(m["q"] * (r * t / (1.0 - m["pinv"])))
        lk = np.einsum("ni,i,ij,nj->n", m["x"], m["pi"], p, m["y"])
        site += m["w"][k] * ((1.0 - m["pinv"]) * lk + np.where(m["inv"] >= 0, m["pi"][np.maximum(m["inv"], 0)] * m["pinv"], 0.0))
    return float((m["pw"] * np.log(site)).sum())


@pytest.mark.parametrize("pinv", [0.0, 0.2])
def test_the_definitions_on_a_toy(pinv):
    m = _toy(pinv)
    c0, c1 = _toy_terms(m)
    lk0, lk1 = c0 @ m["w"], c1 @ m["w"]
    d_f = float((m["pw"] * (-lk1 / lk0)).sum())
    d_cat = (m["pw"][:, None] * (-(m["w"][None, :] * c1) / lk0[:, None])).sum(0)
    assert abs(d_cat.sum() - d_f) <= 1e-13 * np.abs(d_cat).sum()
    # the oracle's arithmetic: posterior x (the derivative under one-hot weights) is the same number
    post, q = m["w"][None, :] * c0 / lk0[:, None], -c1 / c0
    assert np.allclose(post.sum(1), 1.0, atol=1e-14)
    oracle = (m["pw"][:, None] * post * q).sum(0)
    scale = (m["pw"][:, None] * post * np.abs(q)).sum(0)
    assert (np.abs(oracle - d_cat) <= 1e-13 * scale).all()
    # d_f is the derivative of -lnL with respect to the length ...
    h = 1e-5
    fd = -(_toy_lnl(m, m["rates"], m["t"] + h) - _toy_lnl(m, m["rates"], m["t"] - h)) / (2 * h)
    assert abs(fd - d_f) <= 1e-7 * abs(d_f)
    # ... (t / r_k) d_cat[k] the derivative with respect to r_k, 1 / (1 - pinv) included, and t d_f the one with respect to a
    # multiplier of the length
    d_rates, d_scale = RG.restated(d_cat[None, :], [d_f], [m["t"]], m["rates"])
    for k in range(len(m["rates"])):
        step = np.zeros(len(m["rates"]))
        step[k] = 1e-5 * m["rates"][k]
        fd = -(_toy_lnl(m, m["rates"] + step, m["t"]) - _toy_lnl(m, m["rates"] - step, m["t"])) / (2 * step[k])
        assert abs(fd - d_rates[k]) <= 1e-7 * abs(d_rates[k]) + 1e-9, (k, fd, d_rates[k])
    fd = -(_toy_lnl(m, m["rates"], m["t"] * (1 + h)) - _toy_lnl(m, m["rates"], m["t"] * (1 - h))) / (2 * h)
    assert abs(fd - d_scale) <= 1e-7 * abs(d_scale)


def test_the_restatement_adds_in_list_order():
    """left to right, each product rounded first: not numpy's pairwise sum, not a fused multiply-add"""
    rng = np.random.Generator(np.random.PCG64(9))
    cat, d, t, rates = rng.normal(size=(300, 3)) * 1e3, rng.normal(size=300), rng.uniform(0.01, 2, 300), np.array([0.3, 1.0, 2.2])
    got, scale = RG.restated(cat, d, t, rates)
    for k in range(3):
        acc = 0.0
        for i in range(300):
            acc += float(np.float64(t[i]) / np.float64(rates[k])) * float(cat[i, k])
        assert acc == got[k]
    acc = 0.0
    for i in range(300):
        acc += float(t[i]) * float(d[i])
    assert acc == scale


# ---- the checks that need no device ----------------------------------------------------------------------------------
def _partition(lib, attrs=0):
    p = lib.pll_partition_create(TIPS, INNER, 4, SITES, 1, MATRICES, 4, INNER, attrs | api.ARCH_AVX2)
    assert p, (lib.errno(), lib.errmsg())
    nt = lib.state_map("pll_map_nt")
    for t in range(TIPS):
        assert lib.pll_set_tip_states(p, t, nt, SEQ), (lib.errno(), lib.errmsg())
    return p


def _outputs(n=4):
    return {"d_cat": np.full((n, 4), SENTINEL), "d_f": np.full(n, SENTINEL), "dd_f": np.full(n, SENTINEL), "d_rates": np.full(4, SENTINEL),
            "d_scale": np.full(1, SENTINEL)}


def _untouched(out):
    return all((v == SENTINEL).all() for v in out.values())


def _with(row, field, value, rows=GOOD):
    rows = [list(r) for r in rows]
    rows[row][field] = value
    return rows


def _both(lib, p, rows, pi, out, null_list=False):
    """(status, errno, message) of each of the two calls on the same input, every output asked for"""
    br = None if null_list else api.make_branches(rows)
    res = []
    lib.pll_gpu_branch_category_derivatives(p, br, len(rows), api.uptr(pi), api.dptr(out["d_cat"]), api.dptr(out["d_f"]), api.dptr(out["dd_f"]))
    res.append((lib.errno(), lib.errmsg()))
    lib.pll_gpu_rate_gradient(p, br, len(rows), api.uptr(pi), api.dptr(out["d_rates"]), api.dptr(out["d_scale"]), api.dptr(out["d_cat"]),
                              api.dptr(out["d_f"]))
    res.append((lib.errno(), lib.errmsg()))
    return res


ZERO_RATE = np.array([0.0, 0.5, 1.0, 2.5])
EVERYTHING = api.SITE_REPEATS  # (the two refusals exclude each other: pll_partition_create takes no partition with both)
ASC = api.AB_FLAG | api.AB_LEWIS
# an index and a length wrong in one row (the list is checked row by row, the index first) and two code tips in another
ALL_WRONG = _with(1, 4, -1.0, _with(2, 2, 5, _with(1, 0, TIPS + INNER)))
ORDER = [  # (what, attributes, rows, NULL list, code, a word of the message): each case carries every later fault it can
    ("NULL list", EVERYTHING, ALL_WRONG, True, INVALID, "NULL"),
    ("index out of range", EVERYTHING, ALL_WRONG, False, INVALID, "index out of range"),
    ("negative length", EVERYTHING, _with(0, 4, -1.0, _with(2, 2, 5)), False, INVALID, "length"),
    ("two code-tip ends", EVERYTHING, _with(2, 2, 5), False, INVALID, "tips given by codes"),
    ("NULL list, ascertainment bias", ASC, ALL_WRONG, True, INVALID, "NULL"),
    ("index out of range, ascertainment bias", ASC, ALL_WRONG, False, INVALID, "index out of range"),
    ("two code-tip ends, ascertainment bias", ASC, _with(2, 2, 5), False, INVALID, "tips given by codes"),
    ("site repeats", EVERYTHING, GOOD, False, UNSUPPORTED, "SITE_REPEATS"),
    ("ascertainment bias", ASC, GOOD, False, UNSUPPORTED, "ascertainment"),
    ("ascertainment bias (Stamatakis)", api.AB_FLAG | api.AB_STAMATAKIS, GOOD, False, UNSUPPORTED, "ascertainment"),
]


@pytest.mark.parametrize("case", ORDER, ids=[c[0] for c in ORDER])
def test_the_checks_in_their_order(amd_lib, case):
    _, attrs, rows, null_list, code, word = case
    p = _partition(amd_lib, attrs)
    try:
        amd_lib.pll_set_category_rates(p, api.dptr(ZERO_RATE))  # (the last fault in the order, on every case)
        out = _outputs()
        for errno, msg in _both(amd_lib, p, rows, np.zeros(4, dtype=np.uint32), out, null_list=null_list):
            assert errno == code and word in msg, (errno, msg)
        assert _untouched(out)
    finally:
        amd_lib.pll_partition_destroy(p)


def test_every_output_null_comes_first(amd_lib, capfd):
    p = _partition(amd_lib, EVERYTHING)
    try:
        amd_lib.pll_set_category_rates(p, api.dptr(ZERO_RATE))
        pi = np.zeros(4, dtype=np.uint32)
        assert amd_lib.pll_gpu_branch_category_derivatives(p, None, 4, api.uptr(pi), None, None, None) == 0
        assert amd_lib.errno() == INVALID and "every output is NULL" in amd_lib.errmsg()
        assert "pll_gpu_branch_category_derivatives" in capfd.readouterr().err  # the usual line on stderr
        assert amd_lib.pll_gpu_rate_gradient(p, None, 4, api.uptr(pi), None, None, None, None) == 0
        assert amd_lib.errno() == INVALID and "every output is NULL" in amd_lib.errmsg()
        assert "pll_gpu_rate_gradient" in capfd.readouterr().err
        assert amd_lib.pll_gpu_rate_gradient(None, None, 4, api.uptr(pi), None, None, None, None) == 0 and amd_lib.errno() == INVALID
    finally:
        amd_lib.pll_partition_destroy(p)


def test_any_one_output_is_enough(amd_lib):
    """each output alone passes the NULL check: the call gets as far as the missing device"""
    p = _partition(amd_lib)
    try:
        amd_lib.pll_set_category_rates(p, api.dptr(np.array([0.5, 1.0, 1.5, 2.5])))
        pi, br = np.zeros(4, dtype=np.uint32), api.make_branches(GOOD)
        for which in ("d_cat", "d_f", "dd_f"):
            out = _outputs()
            args = [api.dptr(out[k]) if k == which else None for k in ("d_cat", "d_f", "dd_f")]
            assert amd_lib.pll_gpu_branch_category_derivatives(p, br, 4, api.uptr(pi), *args) == 0
            assert amd_lib.errno() == UNAVAILABLE and _untouched(out), which
        for which in ("d_rates", "d_scale", "d_cat", "d_f"):
            out = _outputs()
            args = [api.dptr(out[k]) if k == which else None for k in ("d_rates", "d_scale", "d_cat", "d_f")]
            assert amd_lib.pll_gpu_rate_gradient(p, br, 4, api.uptr(pi), *args) == 0
            assert amd_lib.errno() == UNAVAILABLE and _untouched(out), which
    finally:
        amd_lib.pll_partition_destroy(p)


@pytest.mark.parametrize("rate", [0.0, -0.5, float("nan"), float("inf")])
def test_a_rate_that_is_not_positive_and_finite(amd_lib, rate):
    """refused where d_rates is asked for - after the refusals, before the device is asked for; with d_rates NULL, and in
    pll_gpu_branch_category_derivatives, the same partition gets as far as the missing device"""
    p = _partition(amd_lib)
    try:
        rates = np.array([0.5, 1.0, rate, 2.5])
        amd_lib.pll_set_category_rates(p, api.dptr(rates))
        pi, br = np.zeros(4, dtype=np.uint32), api.make_branches(GOOD)
        out = _outputs()
        assert amd_lib.pll_gpu_rate_gradient(p, br, 4, api.uptr(pi), api.dptr(out["d_rates"]), api.dptr(out["d_scale"]), api.dptr(out["d_cat"]),
                                             api.dptr(out["d_f"])) == 0
        assert amd_lib.errno() == INVALID and "category rate 2" in amd_lib.errmsg(), amd_lib.errmsg()
        assert amd_lib.pll_gpu_rate_gradient(p, br, 4, api.uptr(pi), None, api.dptr(out["d_scale"]), api.dptr(out["d_cat"]), api.dptr(out["d_f"])) == 0
        assert amd_lib.errno() == UNAVAILABLE
        assert amd_lib.pll_gpu_branch_category_derivatives(p, br, 4, api.uptr(pi), api.dptr(out["d_cat"]), api.dptr(out["d_f"]), None) == 0
        assert amd_lib.errno() == UNAVAILABLE
        assert _untouched(out)
    finally:
        amd_lib.pll_partition_destroy(p)


def test_zero_count(amd_lib):
    """no launch, nothing of the list read, outputs untouched - except d_rates and d_scale: sums over no branch"""
    p = _partition(amd_lib, EVERYTHING)
    try:
        out = _outputs()
        bad = api.make_branches(ALL_WRONG)
        assert amd_lib.pll_gpu_branch_category_derivatives(p, None, 0, None, None, None, None) == 1
        assert amd_lib.pll_gpu_branch_category_derivatives(p, bad, 0, None, api.dptr(out["d_cat"]), api.dptr(out["d_f"]), api.dptr(out["dd_f"])) == 1
        assert _untouched(out)
        assert amd_lib.pll_gpu_rate_gradient(p, None, 0, None, None, None, None, None) == 1
        assert amd_lib.pll_gpu_rate_gradient(p, bad, 0, None, api.dptr(out["d_rates"]), api.dptr(out["d_scale"]), api.dptr(out["d_cat"]),
                                             api.dptr(out["d_f"])) == 1
        assert (out["d_rates"] == 0.0).all() and (out["d_scale"] == 0.0).all()
        assert (out["d_cat"] == SENTINEL).all() and (out["d_f"] == SENTINEL).all() and (out["dd_f"] == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_params_indices(amd_lib):
    p = _partition(amd_lib)
    try:
        out = _outputs()
        for errno, msg in _both(amd_lib, p, GOOD, np.array([0, 0, 1, 0], dtype=np.uint32), out):
            assert errno == INVALID and "params_indices[2]" in msg
        br = api.make_branches(GOOD)
        assert amd_lib.pll_gpu_rate_gradient(p, br, 4, None, api.dptr(out["d_rates"]), None, None, None) == 0
        assert amd_lib.errno() == INVALID and "NULL" in amd_lib.errmsg()
        assert _untouched(out)
    finally:
        amd_lib.pll_partition_destroy(p)
