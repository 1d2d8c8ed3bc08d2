"""CPU (no GPU): pll_gpu_quartet_loglikelihoods is declared, exported and bound, and everything it decides before a
device is needed - the zero-count shortcut, the index checks over the WHOLE list, the refusals in their stated order, the
answer of a partition with no device behind it - on host-only partitions (PLL_AMD_HOST_ONLY=1). A failed call leaves
lnl as it found it."""
import os
import re

import numpy as np
import pytest

from pllamd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIPS, INNER, SITES, MATRICES = 7, 6, 20, 9  # (below 16 sites site repeats are switched off)
SENTINEL = -12345.5
SEQ = b"ACGTACGTACGTACGTACGT"

# ((clv, scaler, matrix) of e0..e3, inner matrix): inner and tip ends mixed, a scaler named for a tip
GOOD = [
    ((TIPS, 0, 1), (TIPS + 1, 1, 2), (0, -1, 3), (TIPS + 2, 2, 4), 8),
    ((0, -1, 0), (1, -1, 1), (2, 3, 2), (3, -1, 3), 4),
    ((TIPS + 5, 5, 5), (TIPS + 4, -1, 6), (TIPS + 3, 3, 7), (6, -1, 8), 0),
]


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


def _partition(lib, attrs=0, states=4, rate_cats=4):
    p = lib.pll_partition_create(TIPS, INNER, states, SITES, 1, MATRICES, rate_cats, INNER, attrs | api.ARCH_AVX2)
    assert p, (lib.errno(), lib.errmsg())
    nt = lib.state_map("pll_map_nt")
    for t in range(TIPS):
        assert lib.pll_set_tip_states(p, t, nt, SEQ), (lib.errno(), lib.errmsg())
    return p


def _call(lib, p, lnl, rows=GOOD, fi=None, count=None):
    fi = np.zeros(4, dtype=np.uint32) if fi is None else fi
    return lib.pll_gpu_quartet_loglikelihoods(p, api.make_quartets(rows), len(rows) if count is None else count, api.uptr(fi), api.dptr(lnl))


def _refused(lib, code, attrs=0, **kw):
    p = _partition(lib, attrs)
    try:
        lnl = np.full(9, SENTINEL)
        assert _call(lib, p, lnl, **kw) == 0
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        assert (lnl == SENTINEL).all()
    finally:
        lib.pll_partition_destroy(p)


def _with(row, end, field, value):
    """GOOD with one field replaced: end 0..3 and field 0..2 (clv, scaler, matrix), or end 4 = the inner matrix"""
    rows = [[list(e) for e in r[:4]] + [r[4]] for r in GOOD]
    if end == 4:
        rows[row][4] = value
    else:
        rows[row][end][field] = value
    return rows


def test_symbol_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    assert re.search(r"\bint pll_gpu_quartet_loglikelihoods\(", hdr)
    assert re.search(r"\}\s*pll_gpu_quartet_t;", hdr)
    assert getattr(amd_lib.dll, "pll_gpu_quartet_loglikelihoods")
    assert amd_lib.pll_gpu_quartet_loglikelihoods.argtypes and len(amd_lib.pll_gpu_quartet_loglikelihoods.argtypes) == 5
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert re.search(r"\bint pllgpu_quartet_loglikelihoods\(", dev) and getattr(amd_lib.dll, "pllgpu_quartet_loglikelihoods")


def test_the_struct_mirror():
    import ctypes as C
    assert C.sizeof(api.Quartet) == 52
    assert [getattr(api.Quartet, f).offset for f in ("clv_index", "scaler_index", "matrix_index", "inner_matrix_index")] == [0, 16, 32, 48]
    q = api.make_quartets(GOOD)[2]
    assert list(q.clv_index) == [TIPS + 5, TIPS + 4, TIPS + 3, 6] and list(q.scaler_index) == [5, -1, 3, -1]
    assert list(q.matrix_index) == [5, 6, 7, 8] and q.inner_matrix_index == 0


def test_zero_count_succeeds_and_leaves_lnl(amd_lib):
    p = _partition(amd_lib)
    try:
        lnl = np.full(9, SENTINEL)
        f = amd_lib.pll_gpu_quartet_loglikelihoods
        assert _call(amd_lib, p, lnl, count=0) == 1
        assert f(p, None, 0, None, None) == 1
        assert f(p, api.make_quartets(_with(0, 0, 0, TIPS + INNER)), 0, None, api.dptr(lnl)) == 1  # nothing of the list is read
        assert (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


BAD = {
    "e0 clv": (1, 0, 0, TIPS + INNER),
    "e1 clv max": (1, 1, 0, 0xFFFFFFFF),
    "e2 scaler": (1, 2, 1, INNER),
    "e3 scaler below -1": (1, 3, 1, -2),
    "e0 matrix": (1, 0, 2, MATRICES),
    "e3 matrix": (1, 3, 2, MATRICES + 1),
    "e2 clv": (1, 2, 0, TIPS + INNER + 7),
    "inner matrix": (1, 4, 0, MATRICES),
}


@pytest.mark.parametrize("what", list(BAD))
def test_a_field_out_of_range_in_the_middle_of_the_list(amd_lib, what):
    row, end, field, value = BAD[what]
    _refused(amd_lib, api.ERROR_PARAM_INVALID, rows=_with(row, end, field, value))


@pytest.mark.parametrize("end", [0, 3, 4])
def test_a_bad_index_in_the_last_quartet_is_caught(amd_lib, end):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, rows=_with(len(GOOD) - 1, end, 2, MATRICES + 3))


def test_freqs_indices_out_of_range(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, fi=np.array([0, 0, 1, 0], dtype=np.uint32))


@pytest.mark.parametrize("which", ["partition", "quartets", "freqs_indices", "lnl"])
def test_each_null_argument(amd_lib, which):
    p = _partition(amd_lib)
    try:
        lnl = np.full(9, SENTINEL)
        fi = np.zeros(4, dtype=np.uint32)
        args = {"partition": p, "quartets": api.make_quartets(GOOD), "freqs_indices": api.uptr(fi), "lnl": api.dptr(lnl)}
        args[which] = None
        assert amd_lib.pll_gpu_quartet_loglikelihoods(args["partition"], args["quartets"], 3, args["freqs_indices"], args["lnl"]) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_unsupported_partitions_are_refused(amd_lib, attrs):
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=attrs)


@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_an_index_error_comes_before_a_refusal(amd_lib, attrs):
    """the order of the checks: a bad index on a partition that would be refused anyway is PARAM_INVALID"""
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, rows=_with(2, 1, 0, TIPS + INNER))
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, fi=np.array([0, 0, 0, 1], dtype=np.uint32))


def test_a_null_argument_comes_before_an_index_error(amd_lib):
    p = _partition(amd_lib)
    try:
        fi = np.array([0, 5, 0, 0], dtype=np.uint32)
        assert amd_lib.pll_gpu_quartet_loglikelihoods(p, api.make_quartets(_with(0, 0, 0, TIPS + INNER)), 3, api.uptr(fi), None) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_a_refusal_comes_before_the_missing_device(amd_lib):
    """host-only partitions have no device either: UNSUPPORTED, not UNAVAILABLE"""
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=api.SITE_REPEATS)


def test_host_only_partition_is_refused_and_lnl_untouched(amd_lib, capfd):
    p = _partition(amd_lib)
    try:
        lnl = np.full(9, SENTINEL)
        assert _call(amd_lib, p, lnl) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert (lnl == SENTINEL).all()
        assert "pll_gpu_quartet_loglikelihoods" in capfd.readouterr().err  # the usual line on stderr
    finally:
        amd_lib.pll_partition_destroy(p)
