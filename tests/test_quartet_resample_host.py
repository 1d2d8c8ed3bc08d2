"""CPU (no GPU): pll_gpu_quartet_resampled_loglikelihoods is declared, exported and bound, and everything it decides
before a device is needed - the zero-count shortcut, the argument checks, the index checks over the WHOLE list, the
refusals in their stated order, the answer of a partition with no device behind it - on host-only partitions
(PLL_AMD_HOST_ONLY=1). A failed call leaves lnl, resampled and persite as it found them."""
import os
import re

import numpy as np
import pytest

from pllamd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIPS, INNER, SITES, MATRICES = 7, 6, 20, 9  # (below 16 sites site repeats are switched off)
REPLICATES = 3
SENTINEL = -12345.5
SEQ = b"ACGTACGTACGTACGTACGT"
NAME = "pll_gpu_quartet_resampled_loglikelihoods"

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


class Buffers:
    """the three outputs filled with a sentinel, and the weights of REPLICATES replicates"""

    def __init__(self):
        self.lnl = np.full(3 * len(GOOD), SENTINEL)
        self.resampled = np.full(3 * len(GOOD) * REPLICATES, SENTINEL)
        self.persite = np.full(3 * len(GOOD) * SITES, SENTINEL)
        self.weights = np.ones((REPLICATES, SITES), dtype=np.uint32)

    def untouched(self):
        return bool((self.lnl == SENTINEL).all() and (self.resampled == SENTINEL).all() and (self.persite == SENTINEL).all())


def _call(lib, p, b, rows=GOOD, fi=None, count=None, replicates=REPLICATES, **null):
    """the call with every argument given; null=dict(name=True) passes NULL for that argument"""
    fi = np.zeros(4, dtype=np.uint32) if fi is None else fi
    args = {"quartets": api.make_quartets(rows), "freqs_indices": api.uptr(fi), "weights": api.uptr(b.weights), "lnl": api.dptr(b.lnl),
            "resampled": api.dptr(b.resampled), "persite": api.dptr(b.persite)}
    for name in null:
        assert name in args
        args[name] = None
    return getattr(lib, NAME)(p, args["quartets"], len(rows) if count is None else count, args["freqs_indices"], args["weights"], replicates,
                              args["lnl"], args["resampled"], args["persite"])


def _refused(lib, code, attrs=0, **kw):
    p = _partition(lib, attrs)
    try:
        b = Buffers()
        assert _call(lib, p, b, **kw) == 0
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        assert b.untouched()
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
    assert re.search(r"\bint " + NAME + r"\(", hdr)
    assert getattr(amd_lib.dll, NAME)
    fn = getattr(amd_lib, NAME)
    assert fn.argtypes and len(fn.argtypes) == 9
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert re.search(r"\bint pllgpu_quartet_resampled_loglikelihoods\(", dev) and getattr(amd_lib.dll, "pllgpu_quartet_resampled_loglikelihoods")
    assert re.search(r"#define PLLGPU_RESAMPLE_MAX_BYTES\b", dev)


def test_zero_count_succeeds_and_writes_nothing(amd_lib):
    p = _partition(amd_lib)
    try:
        b = Buffers()
        assert _call(amd_lib, p, b, count=0) == 1
        assert getattr(amd_lib, NAME)(p, None, 0, None, None, 0, None, None, None) == 1
        assert getattr(amd_lib, NAME)(p, None, 0, None, None, REPLICATES, None, None, None) == 1
        assert _call(amd_lib, p, b, rows=_with(0, 0, 0, TIPS + INNER), count=0) == 1  # nothing of the list is read
        assert b.untouched()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_null_partition(amd_lib):
    b = Buffers()
    assert _call(amd_lib, None, b) == 0
    assert amd_lib.errno() == api.ERROR_PARAM_INVALID and b.untouched()


@pytest.mark.parametrize("which", ["quartets", "freqs_indices"])
def test_null_list_arguments(amd_lib, which):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, **{which: True})


@pytest.mark.parametrize("which", ["weights", "resampled"])
def test_replicates_need_weights_and_resampled(amd_lib, which):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, **{which: True})


def test_all_three_outputs_null(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, replicates=0, lnl=True, resampled=True, persite=True)
    _refused(amd_lib, api.ERROR_PARAM_INVALID, replicates=0, weights=True, lnl=True, resampled=True, persite=True)


BAD = {
    "e0 clv": (1, 0, 0, TIPS + INNER),
    "e1 clv max": (1, 1, 0, 0xFFFFFFFF),
    "e2 scaler": (1, 2, 1, INNER),
    "e3 scaler below -1": (1, 3, 1, -2),
    "e0 matrix": (1, 0, 2, MATRICES),
    "e3 matrix": (1, 3, 2, MATRICES + 1),
    "inner matrix": (1, 4, 0, MATRICES),
    "last quartet": (len(GOOD) - 1, 4, 0, MATRICES + 3),
}


@pytest.mark.parametrize("what", list(BAD))
def test_a_field_out_of_range_anywhere_in_the_list(amd_lib, what):
    row, end, field, value = BAD[what]
    _refused(amd_lib, api.ERROR_PARAM_INVALID, rows=_with(row, end, field, value))


def test_freqs_indices_out_of_range(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, fi=np.array([0, 0, 1, 0], dtype=np.uint32))


@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_unsupported_partitions_are_refused(amd_lib, attrs):
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=attrs)
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=attrs, replicates=0, weights=True, resampled=True)  # the per-site form alike


@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_argument_and_index_errors_come_before_a_refusal(amd_lib, attrs):
    """the order of the checks: on a partition that would be refused anyway each of these is PARAM_INVALID"""
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, rows=_with(2, 1, 0, TIPS + INNER))
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, fi=np.array([0, 0, 0, 1], dtype=np.uint32))
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, weights=True)
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, resampled=True)
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, replicates=0, lnl=True, resampled=True, persite=True)


def test_a_null_argument_comes_before_an_index_error(amd_lib):
    p = _partition(amd_lib)
    try:
        b = Buffers()
        fi = np.array([0, 5, 0, 0], dtype=np.uint32)
        assert _call(amd_lib, p, b, rows=_with(0, 0, 0, TIPS + INNER), fi=fi, resampled=True) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
        assert b.untouched()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_a_refusal_comes_before_the_missing_device(amd_lib):
    """host-only partitions have no device either: UNSUPPORTED, not UNAVAILABLE"""
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=api.SITE_REPEATS)


@pytest.mark.parametrize("replicates", [REPLICATES, 0])
def test_host_only_partition_is_refused_and_outputs_untouched(amd_lib, capfd, replicates):
    p = _partition(amd_lib)
    try:
        b = Buffers()
        assert _call(amd_lib, p, b, replicates=replicates) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert b.untouched()
        assert NAME in capfd.readouterr().err  # the usual line on stderr
    finally:
        amd_lib.pll_partition_destroy(p)


def test_the_existing_call_keeps_its_messages(amd_lib, capfd):
    """both calls share their checks: each names itself in what it reports"""
    p = _partition(amd_lib)
    try:
        lnl = np.full(9, SENTINEL)
        fi = np.zeros(4, dtype=np.uint32)
        assert amd_lib.pll_gpu_quartet_loglikelihoods(p, api.make_quartets(_with(1, 2, 0, TIPS + INNER)), 3, api.uptr(fi), api.dptr(lnl)) == 0
        assert amd_lib.errmsg() == "pll_gpu_quartet_loglikelihoods: quartet 1 has an index out of range"
        assert "pll_gpu_quartet_loglikelihoods:" in capfd.readouterr().err
        b = Buffers()
        assert _call(amd_lib, p, b, rows=_with(1, 2, 0, TIPS + INNER)) == 0
        assert amd_lib.errmsg() == NAME + ": quartet 1 has an index out of range"
    finally:
        amd_lib.pll_partition_destroy(p)
