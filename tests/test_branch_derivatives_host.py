"""CPU (no GPU): pll_gpu_branch_derivatives is declared, exported and bound, and everything it decides before a device is
needed - the zero-count shortcut, the checks over the WHOLE list, the refusals in their stated order, the answer of a
partition with no device behind it - on host-only partitions (PLL_AMD_HOST_ONLY=1). A failed call leaves d_f and dd_f as it
found them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pllamd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIPS, INNER, SITES, MATRICES = 7, 6, 20, 9  # (below 16 sites site repeats are switched off)
SENTINEL = -12345.5
SEQ = b"ACGTACGTACGTACGTACGT"

# (parent clv, parent scaler, child clv, child scaler, length): inner and tip ends mixed, a scaler named for a tip
GOOD = [
    (TIPS, 0, TIPS + 1, 1, 0.1),
    (TIPS + 2, 2, 0, -1, 0.25),
    (3, 4, TIPS + 5, -1, 0.0),
    (TIPS + 4, -1, TIPS + 3, 5, 1.5),
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


def _call(lib, p, d, dd, rows=GOOD, pi=None, count=None):
    pi = np.zeros(4, dtype=np.uint32) if pi is None else pi
    return lib.pll_gpu_branch_derivatives(p, api.make_branches(rows), len(rows) if count is None else count, api.uptr(pi), api.dptr(d),
                                          api.dptr(dd))


def _refused(lib, code, attrs=0, **kw):
    p = _partition(lib, attrs)
    try:
        d, dd = np.full(len(GOOD), SENTINEL), np.full(len(GOOD), SENTINEL)
        assert _call(lib, p, d, dd, **kw) == 0
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        assert (d == SENTINEL).all() and (dd == SENTINEL).all()
    finally:
        lib.pll_partition_destroy(p)


def _with(row, field, value):
    """GOOD with one field of one row replaced"""
    rows = [list(r) for r in GOOD]
    rows[row][field] = value
    return rows


def test_symbol_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    assert re.search(r"\bint pll_gpu_branch_derivatives\(", hdr)
    assert re.search(r"\}\s*pll_gpu_branch_t;", hdr)
    assert getattr(amd_lib.dll, "pll_gpu_branch_derivatives")
    assert amd_lib.pll_gpu_branch_derivatives.argtypes and len(amd_lib.pll_gpu_branch_derivatives.argtypes) == 6
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert re.search(r"\bint pllgpu_branch_derivatives\(", dev) and getattr(amd_lib.dll, "pllgpu_branch_derivatives")
    assert re.search(r"#define PLLGPU_BRANCH_MAX 8192\b", dev)


def test_the_struct_mirror():
    assert C.sizeof(api.Branch) == 24
    fields = ("parent_clv_index", "parent_scaler_index", "child_clv_index", "child_scaler_index", "branch_length")
    assert [getattr(api.Branch, f).offset for f in fields] == [0, 4, 8, 12, 16]
    b = api.make_branches(GOOD)[1]
    assert (b.parent_clv_index, b.parent_scaler_index, b.child_clv_index, b.child_scaler_index, b.branch_length) == (TIPS + 2, 2, 0, -1, 0.25)
    abi = open(os.path.join(ROOT, "libpll-2_amd", "csrc", "host", "abi_check.c")).read()
    assert "sizeof(pll_gpu_branch_t) == 24" in abi and "AT(pll_gpu_branch_t, branch_length, 16)" in abi


def test_zero_count_succeeds_and_leaves_the_outputs(amd_lib):
    p = _partition(amd_lib)
    try:
        d, dd = np.full(4, SENTINEL), np.full(4, SENTINEL)
        f = amd_lib.pll_gpu_branch_derivatives
        assert _call(amd_lib, p, d, dd, count=0) == 1
        assert f(p, None, 0, None, None, None) == 1
        assert f(p, api.make_branches(_with(0, 0, TIPS + INNER)), 0, None, api.dptr(d), api.dptr(dd)) == 1  # nothing of the list is read
        assert (d == SENTINEL).all() and (dd == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


BAD = {
    "parent clv": (1, 0, TIPS + INNER),
    "parent clv max": (1, 0, 0xFFFFFFFF),
    "child clv": (2, 2, TIPS + INNER + 7),
    "parent scaler": (1, 1, INNER),
    "parent scaler below -1": (2, 1, -2),
    "child scaler": (1, 3, INNER + 3),
    "child scaler below -1": (2, 3, -7),
    "negative length": (1, 4, -0.01),
    "nan length": (2, 4, float("nan")),
    "infinite length": (1, 4, float("inf")),
    "two code tips": (2, 2, 5),
}


@pytest.mark.parametrize("what", list(BAD))
def test_a_field_out_of_range_in_the_middle_of_the_list(amd_lib, what):
    row, field, value = BAD[what]
    _refused(amd_lib, api.ERROR_PARAM_INVALID, rows=_with(row, field, value))


@pytest.mark.parametrize("what", list(BAD))
def test_a_bad_field_in_the_last_row_is_caught(amd_lib, what):
    _, field, value = BAD[what]
    rows = [list(r) for r in GOOD]
    if what == "two code tips":
        rows[-1][0] = 2  # (the last row's parent becomes a tip as well)
    rows[-1][field] = value
    _refused(amd_lib, api.ERROR_PARAM_INVALID, rows=rows)


def test_two_code_tips_are_refused_under_pattern_tip_too(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=api.PATTERN_TIP, rows=_with(1, 0, 4))


def test_params_indices_out_of_range(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, pi=np.array([0, 0, 1, 0], dtype=np.uint32))


@pytest.mark.parametrize("which", ["partition", "branches", "params_indices", "d_f"])
def test_each_null_argument(amd_lib, which):
    p = _partition(amd_lib)
    try:
        d, dd = np.full(4, SENTINEL), np.full(4, SENTINEL)
        pi = np.zeros(4, dtype=np.uint32)
        args = {"partition": p, "branches": api.make_branches(GOOD), "params_indices": api.uptr(pi), "d_f": api.dptr(d)}
        args[which] = None
        assert amd_lib.pll_gpu_branch_derivatives(args["partition"], args["branches"], 4, args["params_indices"], args["d_f"], api.dptr(dd)) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert (d == SENTINEL).all() and (dd == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_a_null_dd_f_is_no_error(amd_lib):
    """dd_f may be NULL: the call gets as far as the missing device"""
    p = _partition(amd_lib)
    try:
        d = np.full(4, SENTINEL)
        pi = np.zeros(4, dtype=np.uint32)
        assert amd_lib.pll_gpu_branch_derivatives(p, api.make_branches(GOOD), 4, api.uptr(pi), api.dptr(d), None) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE and (d == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


UNSUPPORTED = {"site_repeats": api.SITE_REPEATS, "asc_bias_lewis": api.AB_FLAG | api.AB_LEWIS, "asc_bias_stamatakis": api.AB_FLAG | api.AB_STAMATAKIS}


@pytest.mark.parametrize("attrs", list(UNSUPPORTED.values()), ids=list(UNSUPPORTED))
def test_unsupported_partitions_are_refused(amd_lib, attrs):
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=attrs)


@pytest.mark.parametrize("attrs", list(UNSUPPORTED.values()), ids=list(UNSUPPORTED))
def test_an_index_error_comes_before_a_refusal(amd_lib, attrs):
    """the order of the checks: a bad field on a partition that would be refused anyway is PARAM_INVALID"""
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, rows=_with(3, 2, TIPS + INNER))
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, rows=_with(0, 4, -1.0))
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, pi=np.array([0, 0, 0, 1], dtype=np.uint32))


def test_a_null_argument_comes_before_an_index_error(amd_lib):
    p = _partition(amd_lib)
    try:
        pi = np.array([0, 5, 0, 0], dtype=np.uint32)
        dd = np.full(4, SENTINEL)
        assert amd_lib.pll_gpu_branch_derivatives(p, api.make_branches(_with(0, 0, TIPS + INNER)), 4, api.uptr(pi), None, api.dptr(dd)) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
        assert (dd == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_a_refusal_comes_before_the_missing_device(amd_lib):
    """host-only partitions have no device either: UNSUPPORTED, not UNAVAILABLE"""
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=api.SITE_REPEATS)


def test_host_only_partition_is_refused_and_the_outputs_untouched(amd_lib, capfd):
    p = _partition(amd_lib)
    try:
        d, dd = np.full(4, SENTINEL), np.full(4, SENTINEL)
        assert _call(amd_lib, p, d, dd) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert (d == SENTINEL).all() and (dd == SENTINEL).all()
        assert "pll_gpu_branch_derivatives" in capfd.readouterr().err  # the usual line on stderr
    finally:
        amd_lib.pll_partition_destroy(p)
