"""CPU (no GPU): pll_gpu_placement_loglikelihoods is declared, exported and bound, and everything it decides before a
device is needed - the two zero-count shortcuts, the index checks over the WHOLE of both lists, the refusals, the
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

GOOD = [(TIPS, 0, 1, TIPS + 1, 1, 2), (0, -1, 3, TIPS + 2, 2, 4), (1, -1, 5, 2, -1, 6)]
QUERIES = [4, 5, 6]
PENDANT = 8


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


def _call(lib, p, lnl, queries=QUERIES, pendant=PENDANT, rows=GOOD, fi=None, qcount=None, count=None):
    fi = np.zeros(4, dtype=np.uint32) if fi is None else fi
    q = np.ascontiguousarray(queries, dtype=np.uint32)
    return lib.pll_gpu_placement_loglikelihoods(p, api.uptr(q), len(q) if qcount is None else qcount, pendant, api.make_insertions(rows),
                                                len(rows) if count is None else count, api.uptr(fi), api.dptr(lnl))


def _refused(lib, code, attrs=0, **kw):
    p = _partition(lib, attrs)
    try:
        lnl = np.full(9, SENTINEL)
        assert _call(lib, p, lnl, **kw) == 0
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        assert (lnl == SENTINEL).all()
    finally:
        lib.pll_partition_destroy(p)


def test_symbol_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    assert re.search(r"\bint pll_gpu_placement_loglikelihoods\(", hdr)
    assert getattr(amd_lib.dll, "pll_gpu_placement_loglikelihoods")
    assert amd_lib.pll_gpu_placement_loglikelihoods.argtypes and len(amd_lib.pll_gpu_placement_loglikelihoods.argtypes) == 8
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert re.search(r"\bint pllgpu_placement_loglikelihoods\(", dev) and getattr(amd_lib.dll, "pllgpu_placement_loglikelihoods")


def test_zero_counts_succeed_and_leave_lnl(amd_lib):
    p = _partition(amd_lib)
    try:
        lnl = np.full(9, SENTINEL)
        f = amd_lib.pll_gpu_placement_loglikelihoods
        assert _call(amd_lib, p, lnl, qcount=0) == 1
        assert _call(amd_lib, p, lnl, count=0) == 1
        assert f(p, None, 0, PENDANT, api.make_insertions(GOOD), 3, None, None) == 1
        q = np.ascontiguousarray(QUERIES, dtype=np.uint32)
        assert f(p, api.uptr(q), 3, PENDANT, None, 0, None, None) == 1
        assert f(p, None, 0, PENDANT, None, 0, None, None) == 1
        assert (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


@pytest.mark.parametrize("bad", [TIPS, TIPS + 1, TIPS + INNER + 5, 0xFFFFFFFF], ids=["tips", "inner", "beyond_nodes", "max"])
def test_a_query_index_that_is_no_tip(amd_lib, bad):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, queries=[4, bad, 6])


@pytest.mark.parametrize("pendant", [MATRICES, MATRICES + 40])
def test_the_pendant_matrix_out_of_range(amd_lib, pendant):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, pendant=pendant)


BAD = {
    "child1 clv": (1, 0, TIPS + INNER),
    "child1 scaler": (1, 1, INNER),
    "child1 scaler below -1": (1, 1, -2),
    "child1 matrix": (1, 2, MATRICES),
    "child2 clv": (1, 3, TIPS + INNER + 7),
    "child2 scaler": (1, 4, INNER + 3),
    "child2 matrix": (1, 5, MATRICES + 1),
}


@pytest.mark.parametrize("what", list(BAD))
def test_a_candidate_field_out_of_range_in_the_middle_of_the_list(amd_lib, what):
    row, field, value = BAD[what]
    rows = [list(r) for r in GOOD]
    rows[row][field] = value
    _refused(amd_lib, api.ERROR_PARAM_INVALID, rows=rows)


def test_freqs_indices_out_of_range(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, fi=np.array([0, 0, 1, 0], dtype=np.uint32))


@pytest.mark.parametrize("which", ["partition", "query_tip_indices", "candidates", "freqs_indices", "lnl"])
def test_each_null_argument(amd_lib, which):
    p = _partition(amd_lib)
    try:
        lnl = np.full(9, SENTINEL)
        q = np.ascontiguousarray(QUERIES, dtype=np.uint32)
        fi = np.zeros(4, dtype=np.uint32)
        args = {"partition": p, "query_tip_indices": api.uptr(q), "candidates": api.make_insertions(GOOD), "freqs_indices": api.uptr(fi),
                "lnl": api.dptr(lnl)}
        args[which] = None
        assert amd_lib.pll_gpu_placement_loglikelihoods(args["partition"], args["query_tip_indices"], 3, PENDANT, args["candidates"], 3,
                                                        args["freqs_indices"], args["lnl"]) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID
        assert (lnl == SENTINEL).all()
    finally:
        amd_lib.pll_partition_destroy(p)


@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_unsupported_partitions_are_refused(amd_lib, attrs):
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=attrs)


def test_an_index_error_comes_before_a_refusal(amd_lib):
    """the order of the checks: a bad index on a partition that would be refused anyway is PARAM_INVALID"""
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=api.SITE_REPEATS, queries=[4, TIPS, 6])


def test_host_only_partition_is_refused_and_lnl_untouched(amd_lib, capfd):
    p = _partition(amd_lib)
    try:
        lnl = np.full(9, SENTINEL)
        assert _call(amd_lib, p, lnl) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert (lnl == SENTINEL).all()
        assert "pll_gpu_placement_loglikelihoods" in capfd.readouterr().err  # the usual line on stderr
    finally:
        amd_lib.pll_partition_destroy(p)
