"""CPU (no GPU): pll_gpu_insertion_loglikelihoods is declared, exported and bound, and everything it decides before a
device is needed - the count == 0 shortcut, the index checks over the WHOLE candidate list, the refusals, the answer
of a partition with no device behind it - on host-only partitions (PLL_AMD_HOST_ONLY=1). A failed call leaves lnl as
it found it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from pllamd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIPS, INNER, SITES, MATRICES = 5, 6, 20, 9  # (below 16 sites site repeats are switched off)
SENTINEL = -12345.5


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


def _partition(lib, attrs=0, states=4, rate_cats=4):
    p = lib.pll_partition_create(TIPS, INNER, states, SITES, 1, MATRICES, rate_cats, INNER, attrs | api.ARCH_AVX2)
    assert p, (lib.errno(), lib.errmsg())
    return p


def _call(lib, p, subtree, rows, lnl, count=None, fi=None):
    fi = np.zeros(4, dtype=np.uint32) if fi is None else fi
    return lib.pll_gpu_insertion_loglikelihoods(p, subtree[0], subtree[1], subtree[2], api.make_insertions(rows),
                                                len(rows) if count is None else count, api.uptr(fi), api.dptr(lnl))


GOOD = [(TIPS, 0, 1, TIPS + 1, 1, 2), (0, -1, 3, TIPS + 2, 2, 4), (1, -1, 5, 2, -1, 6)]
SUBTREE = (4, -1, 8)


def test_symbol_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    assert re.search(r"\bpll_gpu_insertion_loglikelihoods\(", hdr) and "pll_gpu_insertion_t" in hdr
    assert getattr(amd_lib.dll, "pll_gpu_insertion_loglikelihoods")
    assert amd_lib.pll_gpu_insertion_loglikelihoods.argtypes
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert "pllgpu_insertion_loglikelihoods(" in dev and getattr(amd_lib.dll, "pllgpu_insertion_loglikelihoods")


def test_struct_layout():
    assert C.sizeof(api.Insertion) == 24
    assert [getattr(api.Insertion, f).offset for f, _ in api.Insertion._fields_] == [0, 4, 8, 12, 16, 20]
    src = open(os.path.join(ROOT, "libpll-2_amd", "csrc", "host", "abi_check.c")).read()
    assert "sizeof(pll_gpu_insertion_t) == 24" in src


def test_host_only_partition_is_refused_and_lnl_untouched(amd_lib, capfd):
    p = _partition(amd_lib)
    try:
        lnl = np.full(3, SENTINEL)
        assert _call(amd_lib, p, SUBTREE, GOOD, lnl) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert (lnl == SENTINEL).all()
        assert "pll_gpu_insertion_loglikelihoods" in capfd.readouterr().err  # the usual line on stderr
    finally:
        amd_lib.pll_partition_destroy(p)


BAD = {
    "child1 clv": (0, 0, TIPS + INNER),
    "child1 scaler": (1, 1, INNER),
    "child1 scaler below -1": (1, 1, -2),
    "child1 matrix": (2, 2, MATRICES),
    "child2 clv": (1, 3, TIPS + INNER + 7),
    "child2 scaler": (2, 4, INNER + 3),
    "child2 matrix": (0, 5, MATRICES + 1),
}


@pytest.mark.parametrize("what", list(BAD))
def test_an_index_out_of_range_anywhere_in_the_list(amd_lib, what):
    row, field, value = BAD[what]
    rows = [list(r) for r in GOOD]
    rows[row][field] = value
    p = _partition(amd_lib)
    try:
        lnl = np.full(3, SENTINEL)
        assert _call(amd_lib, p, SUBTREE, rows, lnl) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID, what
        assert (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


@pytest.mark.parametrize("subtree", [(TIPS + INNER, -1, 8), (4, INNER, 8), (4, -1, MATRICES)], ids=["clv", "scaler", "matrix"])
def test_a_subtree_end_out_of_range(amd_lib, subtree):
    p = _partition(amd_lib)
    try:
        lnl = np.full(3, SENTINEL)
        assert _call(amd_lib, p, subtree, GOOD, lnl) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_null_arguments_and_freqs_indices(amd_lib):
    p = _partition(amd_lib)
    try:
        lnl = np.full(3, SENTINEL)
        fi = np.zeros(4, dtype=np.uint32)
        f = amd_lib.pll_gpu_insertion_loglikelihoods
        assert f(p, 4, -1, 8, None, 3, api.uptr(fi), api.dptr(lnl)) == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert f(p, 4, -1, 8, api.make_insertions(GOOD), 3, api.uptr(fi), None) == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert _call(amd_lib, p, SUBTREE, GOOD, lnl, fi=np.array([0, 0, 1, 0], dtype=np.uint32)) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_count_zero_succeeds(amd_lib):
    p = _partition(amd_lib)
    try:
        lnl = np.full(3, SENTINEL)
        assert _call(amd_lib, p, SUBTREE, GOOD, lnl, count=0) == 1
        assert amd_lib.pll_gpu_insertion_loglikelihoods(p, 4, -1, 8, None, 0, None, None) == 1
        assert (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_unsupported_partitions_are_refused(amd_lib, attrs):
    p = _partition(amd_lib, attrs)
    try:
        lnl = np.full(3, SENTINEL)
        assert _call(amd_lib, p, SUBTREE, GOOD, lnl) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNSUPPORTED
        assert (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)
