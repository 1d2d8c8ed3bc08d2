"""CPU (no GPU): pll_gpu_qmatrix_gradient, pll_gpu_subst_gradient_from_dq and pll_gpu_subst_gradient are declared, exported
and bound with their device entry, the device header states the cutting rule, the Phi / eigen form of the definitions agrees
with scipy's Frechet derivative of expm (GTR and JC69, whose three equal eigenvalues take the degenerate branch), the
definitions agree with central differences of a two-taxon toy's log-likelihood, the chain rule of
pll_gpu_subst_gradient_from_dq agrees with a numeric Jacobian of the restated Q construction, and everything the calls
decide before a device is needed - the zero-count rule, the checks in their stated order, the refusals - holds on host-only
partitions (PLL_AMD_HOST_ONLY=1). A failed call leaves every output as it found it."""
import os
import re

import numpy as np
import pytest
from scipy.linalg import expm, expm_frechet

import qmatrix_gradient_cases as QC
from pllamd import api, workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIPS, INNER, SITES, MATRICES = 7, 6, 20, 9  # (below 16 sites site repeats are switched off)
SENTINEL = -12345.5
SEQ = b"ACGTACGTACGTACGTACGT"
GOOD = [(TIPS, 0, TIPS + 1, 1, 0.1), (TIPS + 2, 2, 0, -1, 0.25), (3, 4, TIPS + 5, -1, 0.0), (TIPS + 4, -1, TIPS + 3, 5, 1.5)]
INVALID, UNSUPPORTED, UNAVAILABLE = api.ERROR_PARAM_INVALID, api.ERROR_GPU_UNSUPPORTED, api.ERROR_GPU_UNAVAILABLE
JC = (np.ones(6), np.full(4, 0.25))
GTR = (np.asarray(W.GTR_DNA["exch"], dtype=np.float64), np.asarray(W.GTR_DNA["freqs"], dtype=np.float64))


@pytest.fixture(autouse=True)
def host_only(monkeypatch, amd_lib):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")
    # the restatement checked below is the restatement of THIS library's call: no call, no test
    assert getattr(amd_lib.dll, "pll_gpu_qmatrix_gradient") and getattr(amd_lib.dll, "pll_gpu_subst_gradient_from_dq")


# ---- 1: declared, exported, bound ------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    names = ("pll_gpu_qmatrix_gradient", "pll_gpu_subst_gradient_from_dq", "pll_gpu_subst_gradient")
    at = [hdr.index(f"int {n}(") for n in ("pll_gpu_rate_gradient",) + names]
    assert at == sorted(at), "declared after pll_gpu_rate_gradient, in the issue's order"
    for n in names:
        assert getattr(amd_lib.dll, n) and len(getattr(amd_lib, n).argtypes) == 6, n
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert re.search(r"\bint pllgpu_qmatrix_gradient\(", dev) and getattr(amd_lib.dll, "pllgpu_qmatrix_gradient")
    for text in ("A_i(n,k)", "H_bk[i][j]", "Phi_bk[i][j]", "W_m[i][j]", "d_q[m][x][y]", "d_root[m][x]", "expm1"):
        assert text in hdr, text


def test_the_device_header_states_the_cutting_rule():
    dev = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "pll_amd_device.h")).read())
    assert "Q = min(count, PLLGPU_BRANCH_MAX, max(1, floor(PLLGPU_INSERTION_MAX_SLOTS / (V B))))" in dev
    assert "M = min(PLLGPU_QGRADIENT_MAX_BLOCKS, max(4, floor(16384 / P^2)))" in dev and "3 ceil(count / Q) + 1 launches" in dev
    assert re.search(r"#define PLLGPU_QGRADIENT_MAX_BLOCKS 64\b", dev)
    # ... and the helper restates it
    assert QC.blocks_by_rule(4, 4, 100000) == 56 and QC.blocks_by_rule(20, 4, 20000) == 16 and QC.blocks_by_rule(61, 2, 100000) == 4
    assert QC.blocks_by_rule(5, 4, 65) == 2 and QC.blocks_by_rule(4, 4, 300) == 2
    assert QC.per_launch_by_rule(61, 2, 65, 1 << 30) == (4 << 20) // (2 * 3721 * 2) == 281
    assert QC.launches_by_rule(61, 2, 65, 281) == 4 and QC.launches_by_rule(61, 2, 65, 282) == 7
    assert QC.launches_by_rule(4, 4, 100000, 125) == 4


# ---- 2: Phi against scipy's Frechet derivative -----------------------------------------------------------------------
@pytest.mark.parametrize("model", [GTR, JC], ids=["gtr", "jc69"])
@pytest.mark.parametrize("tau", [0.0, 1e-9, 0.37, 25.0])
def test_phi_is_the_frechet_derivative_of_expm(model, tau):
    """d exp(Q tau) in direction E: U (Phi o (U^-1 E U)) U^-1, for symmetric Phi; observed agreement 5e-16"""
    subst, freqs = model
    q = QC.q_matrix(subst, freqs)
    lam, u, ui = QC.eigensystem(q, freqs)
    assert np.allclose(u @ np.diag(lam) @ ui, q, atol=1e-14) and np.allclose(u @ ui, np.eye(4), atol=1e-14)
    if model is JC:
        assert np.sum(np.abs(lam - lam[0]) < 1e-12) == 3, "JC69 has three equal eigenvalues"
    ph = QC.phi(lam, tau)
    assert np.isfinite(ph).all() and np.allclose(np.diag(ph), tau * np.exp(lam * tau), rtol=1e-15, atol=0)
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(4):
        e = rng.normal(size=(4, 4))
        got = u @ (ph * (ui @ e @ u)) @ ui
        exp = expm_frechet(q * tau, e * tau, compute_expm=False) if tau > 0 else np.zeros((4, 4))
        assert np.abs(got - exp).max() <= 1e-13 * max(np.abs(exp).max(), tau), (tau, np.abs(got - exp).max())


# ---- 3: the definitions on a two-taxon toy ---------------------------------------------------------------------------
def _toy(pinv, seed=5, sites=23):
    rng = np.random.Generator(np.random.PCG64(seed))
    subst, freqs = GTR
    x = np.eye(4)[rng.integers(0, 4, sites)]
    y = np.eye(4)[np.where(rng.random(sites) < 0.4, x.argmax(1), rng.integers(0, 4, sites))]
    inv = np.where(x.argmax(1) == y.argmax(1), x.argmax(1), -1)
    w = np.array([0.1, 0.2, 0.3, 0.4])
    pw = (1 + np.arange(sites) % 3).astype(np.float64)
    model = QC.Model([freqs], [subst], W.gamma_rates_mean(0.7, 4), w, [pinv], [0, 0, 0, 0], pw, invariant=inv)
    # CLVs per category: the tip vectors, and on the child side a soft vector so that nothing is special
    px = np.repeat(x[:, None, :], 4, axis=1)
    cy = np.repeat(y[:, None, :], 4, axis=1) * 0.9 + 0.025
    ends = {(0, -1): (px, None), (1, -1): (cy, None)}
    return model, ends, [(0, -1, 1, -1, 0.37)]


def _toy_lnl(model, ends, rows, q=None, freqs=None):
    """the same likelihood with no eigensystem: transition matrices by scipy's expm; the root sum with `freqs`"""
    q = model.q[0] if q is None else q
    pi = model.freqs[0] if freqs is None else freqs
    (p, ps, c, cs, t), = rows
    site = np.zeros(model.sites)
    for k in range(model.R):
        pm = expm(q * (model.rates[k] * t / (1.0 - model.pinv[0])))
        lk = np.einsum("ni,i,ij,nj->n", ends[(p, ps)][0][:, k, :], pi, pm, ends[(c, cs)][0][:, k, :])
        isl = np.where(model.invariant >= 0, model.freqs[0][np.maximum(model.invariant, 0)] * model.pinv[0], 0.0)
        site += model.weights[k] * ((1.0 - model.pinv[0]) * lk + isl)
    return float((model.pw * np.log(site)).sum())


@pytest.mark.parametrize("pinv", [0.0, 0.2])
def test_the_definitions_on_a_toy(pinv):
    """d_q[x][y] against central differences of -lnL in Q[x][y] alone, d_root[x] against those in the root sum's pi_x
    alone: agreement to the differences' own error (observed 2e-9 relative to the largest entry)"""
    model, ends, rows = _toy(pinv)
    r = QC.restate(model, ends, rows)
    h = 1e-5
    fd = np.zeros((4, 4))
    for x in range(4):
        for y in range(4):
            e = np.zeros((4, 4))
            e[x, y] = h
            fd[x, y] = -(_toy_lnl(model, ends, rows, q=model.q[0] + e) - _toy_lnl(model, ends, rows, q=model.q[0] - e)) / (2 * h)
    assert np.abs(fd - r["d_q"][0]).max() <= 1e-7 * np.abs(fd).max(), (fd, r["d_q"][0])
    if pinv == 0.0:
        for x in range(4):
            e = np.zeros(4)
            e[x] = h
            f = -(_toy_lnl(model, ends, rows, freqs=model.freqs[0] + e) - _toy_lnl(model, ends, rows, freqs=model.freqs[0] - e)) / (2 * h)
            assert abs(f - r["d_root"][0][x]) <= 1e-7 * np.abs(r["d_root"][0]).max(), (x, f, r["d_root"][0])
    # Euler: Q enters through Q tau only, so sum_xy d_q Q = the derivative with respect to a multiplier of the length
    f = -(_toy_lnl(model, ends, rows, q=model.q[0] * (1 + h)) - _toy_lnl(model, ends, rows, q=model.q[0] * (1 - h))) / (2 * h)
    assert abs(np.sum(r["d_q"][0] * model.q[0]) - f) <= 1e-7 * abs(f)
    assert (r["abs_q"] >= np.abs(r["d_q"]) * (1 - 1e-12)).all()


# ---- 4: the chain rule -----------------------------------------------------------------------------------------------
def _model_partition(lib, states, subst, freqs):
    p = lib.pll_partition_create(4, 2, states, 20, 2, 5, 4, 2, api.ARCH_AVX2)
    assert p, (lib.errno(), lib.errmsg())
    for m in range(2):
        lib.pll_set_frequencies(p, m, api.dptr(np.ascontiguousarray(freqs[m])))
        lib.pll_set_subst_params(p, m, api.dptr(np.ascontiguousarray(subst[m])))
    return p


@pytest.mark.parametrize("states", [4, 20])
def test_from_dq_is_the_chain_rule(amd_lib, states):
    """against a numeric Jacobian of the restated Q construction at two step sizes: |got - X| <= 2 |D_h - D_h/2| + 1e-10
    scale, X the Richardson value (test_gpu_rate_gradient.py, section 8), scale = sum_xy |d_q| |Q| / theta; observed below
    0.02 of the bound"""
    rng = np.random.Generator(np.random.PCG64(11 + states))
    n = states * (states - 1) // 2
    subst = [rng.uniform(0.3, 3.0, n) for _ in range(2)]  # (the last entry is not 1: the division is exercised)
    freqs = [f / f.sum() for f in (rng.uniform(0.5, 1.5, states) for _ in range(2))]
    p = _model_partition(amd_lib, states, subst, freqs)
    try:
        for m in range(2):
            d_q, d_root = rng.normal(size=(states, states)), rng.normal(size=states)
            got_s, got_f = np.full(n, SENTINEL), np.full(states, SENTINEL)
            assert amd_lib.pll_gpu_subst_gradient_from_dq(p, m, api.dptr(d_q), api.dptr(d_root), api.dptr(got_s), api.dptr(got_f)) == 1
            h = 2.0 ** -12
            s1, f1 = QC.chain_rule(subst[m], freqs[m], d_q, d_root, h)
            s2, f2 = QC.chain_rule(subst[m], freqs[m], d_q, d_root, h / 2)
            xs, xf = (4 * s2 - s1) / 3, (4 * f2 - f1) / 3
            scale = np.sum(np.abs(d_q) * np.abs(QC.q_matrix(subst[m], freqs[m])))
            bs = 2 * np.abs(s1 - s2) + 1e-10 * scale / subst[m]
            bf = 2 * np.abs(f1 - f2) + 1e-10 * (scale / freqs[m] + np.abs(d_root))
            print(f"{states} states, set {m}: worst {np.max(np.abs(got_s - xs) / bs):.3f} / {np.max(np.abs(got_f - xf) / bf):.3f} of the bound")
            assert (np.abs(got_s - xs) <= bs).all() and (np.abs(got_f - xf) <= bf).all()
            assert (bs < 1e-4 * np.abs(xs).max()).all() and (bf < 1e-4 * np.abs(xf).max()).all(), "the bound could hide a wrong factor"
            assert abs(np.dot(subst[m], got_s)) <= 1e-12 * np.dot(subst[m], np.abs(got_s))
            # each output alone, and without d_root
            only_s, only_f = np.full(n, SENTINEL), np.full(states, SENTINEL)
            assert amd_lib.pll_gpu_subst_gradient_from_dq(p, m, api.dptr(d_q), None, api.dptr(only_s), None) == 1
            assert amd_lib.pll_gpu_subst_gradient_from_dq(p, m, api.dptr(d_q), None, None, api.dptr(only_f)) == 1
            assert only_s.tobytes() == got_s.tobytes() and np.abs(only_f + d_root - got_f).max() <= 1e-13 * np.abs(got_f).max()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_from_dq_refusals(amd_lib, capfd):
    n = 6
    subst, freqs = [np.array([1.0, 2.0, 0.5, 1.5, 3.0, 1.0]), np.array([1.0, 2.0, 0.5, 1.5, 3.0, 0.0])], [GTR[1], np.array([0.5, 0.5 - 1e-7, 1e-7, 0.0])]
    p = _model_partition(amd_lib, 4, subst, [freqs[0], freqs[0]])
    q = _model_partition(amd_lib, 4, [subst[0], subst[0]], [freqs[0], freqs[1]])
    try:
        d_q, out_s, out_f = np.ones((4, 4)), np.full(n, SENTINEL), np.full(4, SENTINEL)
        call = amd_lib.pll_gpu_subst_gradient_from_dq
        for part, m, args, word in [(None, 0, (api.dptr(d_q), None, api.dptr(out_s), api.dptr(out_f)), "NULL"),
                                    (p, 0, (None, None, api.dptr(out_s), api.dptr(out_f)), "NULL"),
                                    (p, 0, (api.dptr(d_q), None, None, None), "no output"),
                                    (p, 2, (api.dptr(d_q), None, api.dptr(out_s), api.dptr(out_f)), "out of range"),
                                    (p, 1, (api.dptr(d_q), None, api.dptr(out_s), api.dptr(out_f)), "last substitution parameter"),
                                    (q, 1, (api.dptr(d_q), None, api.dptr(out_s), api.dptr(out_f)), "PLL_EIGEN_MINFREQ")]:
            assert call(part, m, *args) == 0 and amd_lib.errno() == INVALID and word in amd_lib.errmsg(), (word, amd_lib.errmsg())
            assert "pll_gpu_subst_gradient_from_dq" in capfd.readouterr().err
            assert (out_s == SENTINEL).all() and (out_f == SENTINEL).all()
        assert call(q, 0, api.dptr(d_q), None, api.dptr(out_s), api.dptr(out_f)) == 1  # needs no device
    finally:
        amd_lib.pll_partition_destroy(p)
        amd_lib.pll_partition_destroy(q)


# ---- 5: the checks that need no device -------------------------------------------------------------------------------
def _partition(lib, attrs=0, rate_matrices=1):
    p = lib.pll_partition_create(TIPS, INNER, 4, SITES, rate_matrices, MATRICES, 4, INNER, attrs | api.ARCH_AVX2)
    assert p, (lib.errno(), lib.errmsg())
    nt = lib.state_map("pll_map_nt")
    for t in range(TIPS):
        assert lib.pll_set_tip_states(p, t, nt, SEQ), (lib.errno(), lib.errmsg())
    for m in range(rate_matrices):
        lib.pll_set_frequencies(p, m, api.dptr(np.ascontiguousarray(GTR[1])))
        lib.pll_set_subst_params(p, m, api.dptr(np.ascontiguousarray(GTR[0])))
    return p


def _outputs(m=1):
    return {"d_q": np.full((m, 4, 4), SENTINEL), "d_root": np.full((m, 4), SENTINEL), "d_subst": np.full((m, 6), SENTINEL),
            "d_freqs": np.full((m, 4), SENTINEL)}


def _untouched(out):
    return all((v == SENTINEL).all() for v in out.values())


def _with(row, field, value, rows=GOOD):
    rows = [list(r) for r in rows]
    rows[row][field] = value
    return rows


def _both(lib, p, rows, pi, out, null_list=False, root=True):
    """(errno, message) of each of the two device calls on the same input, every output asked for"""
    br = None if null_list else api.make_branches(rows)
    res = []
    assert lib.pll_gpu_qmatrix_gradient(p, br, len(rows), api.uptr(pi), api.dptr(out["d_q"]), api.dptr(out["d_root"]) if root else None) == 0
    res.append((lib.errno(), lib.errmsg()))
    assert lib.pll_gpu_subst_gradient(p, br, len(rows), api.uptr(pi), api.dptr(out["d_subst"]), api.dptr(out["d_freqs"]) if root else None) == 0
    res.append((lib.errno(), lib.errmsg()))
    return res


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
        if not attrs & api.AB_FLAG:  # (the last fault in the order, wherever a partition can carry it)
            assert amd_lib.pll_update_invariant_sites_proportion(p, 0, 0.2)
        out = _outputs()
        for errno, msg in _both(amd_lib, p, rows, np.zeros(4, dtype=np.uint32), out, null_list=null_list):
            assert errno == code and word in msg, (errno, msg)
        assert _untouched(out)
    finally:
        amd_lib.pll_partition_destroy(p)


def test_null_outputs_and_partition(amd_lib, capfd):
    p = _partition(amd_lib, EVERYTHING)
    try:
        pi, br, out = np.zeros(4, dtype=np.uint32), api.make_branches(ALL_WRONG), _outputs()
        assert amd_lib.pll_gpu_qmatrix_gradient(p, br, 4, api.uptr(pi), None, api.dptr(out["d_root"])) == 0
        assert amd_lib.errno() == INVALID and "d_q is NULL" in amd_lib.errmsg()
        assert "pll_gpu_qmatrix_gradient" in capfd.readouterr().err  # the usual line on stderr
        assert amd_lib.pll_gpu_subst_gradient(p, br, 4, api.uptr(pi), None, None) == 0
        assert amd_lib.errno() == INVALID and "every output is NULL" in amd_lib.errmsg()
        assert "pll_gpu_subst_gradient" in capfd.readouterr().err
        assert amd_lib.pll_gpu_qmatrix_gradient(None, br, 4, api.uptr(pi), api.dptr(out["d_q"]), None) == 0 and amd_lib.errno() == INVALID
        assert amd_lib.pll_gpu_subst_gradient(None, br, 4, api.uptr(pi), api.dptr(out["d_subst"]), None) == 0 and amd_lib.errno() == INVALID
        assert amd_lib.pll_gpu_qmatrix_gradient(p, api.make_branches(GOOD), 4, None, api.dptr(out["d_q"]), None) == 0
        assert amd_lib.errno() == INVALID and "NULL" in amd_lib.errmsg()
        assert _untouched(out)
    finally:
        amd_lib.pll_partition_destroy(p)


def test_the_frequency_part_with_invariant_sites_is_refused(amd_lib):
    """after the refusals, before the device is asked for; d_q and d_subst alone get as far as the missing device; a
    prop_invar of a rate matrix that no category uses does not count"""
    p = _partition(amd_lib, rate_matrices=2)
    try:
        assert amd_lib.pll_update_invariant_sites_proportion(p, 1, 0.2)
        br, out = api.make_branches(GOOD), _outputs(2)
        for pi, code in ((np.array([0, 0, 1, 0], dtype=np.uint32), UNSUPPORTED), (np.zeros(4, dtype=np.uint32), UNAVAILABLE)):
            for errno, msg in _both(amd_lib, p, GOOD, pi, out):
                assert errno == code and (code == UNAVAILABLE or "prop_invar" in msg), (errno, msg)
            for errno, msg in _both(amd_lib, p, GOOD, pi, out, root=False):
                assert errno == UNAVAILABLE, (errno, msg)
        assert _untouched(out)
    finally:
        amd_lib.pll_partition_destroy(p)


def test_what_the_chain_rule_asks_comes_first_in_subst_gradient(amd_lib):
    p = _partition(amd_lib, EVERYTHING, rate_matrices=2)
    try:
        amd_lib.pll_set_frequencies(p, 1, api.dptr(np.array([0.5, 0.5 - 1e-7, 1e-7, 0.0])))
        out, pi = _outputs(2), np.array([0, 1, 0, 0], dtype=np.uint32)
        args = (api.uptr(pi), api.dptr(out["d_subst"]), api.dptr(out["d_freqs"]))
        assert amd_lib.pll_gpu_subst_gradient(p, api.make_branches(ALL_WRONG), 4, *args) == 0
        assert amd_lib.errno() == INVALID and "PLL_EIGEN_MINFREQ" in amd_lib.errmsg()
        amd_lib.pll_set_frequencies(p, 1, api.dptr(np.ascontiguousarray(GTR[1])))
        amd_lib.pll_set_subst_params(p, 1, api.dptr(np.array([1.0, 2.0, 0.5, 1.5, 3.0, 0.0])))
        assert amd_lib.pll_gpu_subst_gradient(p, api.make_branches(ALL_WRONG), 4, *args) == 0
        assert amd_lib.errno() == INVALID and "last substitution parameter" in amd_lib.errmsg()
        # a set that no category uses is not looked at; pll_gpu_qmatrix_gradient does not look at all
        pi0 = np.zeros(4, dtype=np.uint32)
        assert amd_lib.pll_gpu_subst_gradient(p, api.make_branches(GOOD), 4, api.uptr(pi0), api.dptr(out["d_subst"]), None) == 0
        assert amd_lib.errno() == UNSUPPORTED
        assert amd_lib.pll_gpu_qmatrix_gradient(p, api.make_branches(GOOD), 4, api.uptr(pi), api.dptr(out["d_q"]), None) == 0
        assert amd_lib.errno() == UNSUPPORTED
        assert _untouched(out)
    finally:
        amd_lib.pll_partition_destroy(p)


@pytest.mark.parametrize("states,cats,code", [(61, 4, UNSUPPORTED), (61, 2, UNAVAILABLE), (20, 4, UNAVAILABLE), (20, 5, UNSUPPORTED), (4, 9, UNAVAILABLE)])
def test_a_shape_beyond_the_lds_of_a_workgroup(amd_lib, states, cats, code):
    """PLLGPU_QGRADIENT_LDS_BYTES against PLLGPU_QGRADIENT_LDS_MAX, asked before the device is: a shape that fits gets as
    far as the missing device"""
    p = amd_lib.pll_partition_create(4, 3, states, 20, 1, 5, cats, 3, api.ARCH_AVX2)
    assert p, (amd_lib.errno(), amd_lib.errmsg())
    try:
        d_q, pi = np.full((states, states), SENTINEL), np.zeros(cats, dtype=np.uint32)
        br = api.make_branches([(4, 0, 5, 1, 0.1)])
        assert amd_lib.pll_gpu_qmatrix_gradient(p, br, 1, api.uptr(pi), api.dptr(d_q), None) == 0
        assert amd_lib.errno() == code and (code == UNAVAILABLE or "LDS" in amd_lib.errmsg()), amd_lib.errmsg()
        assert (d_q == SENTINEL).all()
        pad = (states + 15) // 16 * 16
        assert (8 * (4 * cats * states + 256 + 64 * cats + 130 * cats * pad) > 160 * 1024) == (code == UNSUPPORTED)
    finally:
        amd_lib.pll_partition_destroy(p)


def test_zero_count(amd_lib):
    """no launch, nothing of the list read: every output is a sum over no branch"""
    p = _partition(amd_lib, EVERYTHING, rate_matrices=2)
    try:
        out, bad = _outputs(2), api.make_branches(ALL_WRONG)
        assert amd_lib.pll_gpu_qmatrix_gradient(p, None, 0, None, None, None) == 1
        assert amd_lib.pll_gpu_subst_gradient(p, None, 0, None, None, None) == 1
        assert _untouched(out)
        assert amd_lib.pll_gpu_qmatrix_gradient(p, bad, 0, None, api.dptr(out["d_q"]), None) == 1
        assert (out["d_q"] == 0.0).all() and (out["d_root"] == SENTINEL).all()
        assert amd_lib.pll_gpu_qmatrix_gradient(p, bad, 0, None, api.dptr(out["d_q"]), api.dptr(out["d_root"])) == 1
        assert amd_lib.pll_gpu_subst_gradient(p, bad, 0, None, api.dptr(out["d_subst"]), api.dptr(out["d_freqs"])) == 1
        assert all((v == 0.0).all() for v in out.values())
    finally:
        amd_lib.pll_partition_destroy(p)


def test_params_indices(amd_lib):
    p = _partition(amd_lib)
    try:
        out = _outputs()
        for errno, msg in _both(amd_lib, p, GOOD, np.array([0, 0, 1, 0], dtype=np.uint32), out):
            assert errno == INVALID and "params_indices[2]" in msg
        for errno, msg in _both(amd_lib, p, GOOD, np.zeros(4, dtype=np.uint32), out):
            assert errno == UNAVAILABLE  # a good call gets as far as the missing device
        assert _untouched(out)
    finally:
        amd_lib.pll_partition_destroy(p)
