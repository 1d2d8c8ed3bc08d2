"""CPU (no GPU): pll_gpu_edge_category_posteriors and pll_gpu_category_weights_em are declared, exported and bound, and
everything they decide before a device is needed - the NULL and start-weight checks, the index checks, the refusals in
their stated order, the answer of a partition with no device behind it - on host-only partitions
(PLL_AMD_HOST_ONLY=1). A failed call leaves every output as it found it."""
import os
import re

import numpy as np
import pytest

from pllamd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIPS, INNER, SITES, MATRICES, RATES = 7, 6, 20, 9, 4  # (below 16 sites site repeats are switched off)
SENTINEL = -12345.5
SEQ = b"ACGTACGTACGTACGTACGT"
STEPS = 3
GOOD = (TIPS, 0, TIPS + 1, 1, 2)  # (parent, parent scaler, child, child scaler, matrix)
CALLS = ("posteriors", "em")


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


def _partition(lib, attrs=0):
    p = lib.pll_partition_create(TIPS, INNER, 4, SITES, 1, MATRICES, RATES, INNER, attrs | api.ARCH_AVX2)
    assert p, (lib.errno(), lib.errmsg())
    nt = lib.state_map("pll_map_nt")
    for t in range(TIPS):
        assert lib.pll_set_tip_states(p, t, nt, SEQ), (lib.errno(), lib.errmsg())
    return p


class Outputs:
    """the outputs of one call, filled with the sentinel"""

    def __init__(self, which):
        self.which = which
        if which == "posteriors":
            shapes = {"cat_lnl": SITES * RATES, "posterior": SITES * RATES, "site_rates": SITES, "weight_sums": RATES, "lnl": 1}
        else:
            shapes = {"weights_out": (STEPS + 1) * RATES, "lnl_out": STEPS + 1}
        self.arrays = {k: np.full(n, SENTINEL) for k, n in shapes.items()}

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.arrays.values())


def _call(lib, which, p, edge=GOOD, fi="default", out=None, null=(), start="default", steps=STEPS):
    """-> (status, outputs); `null`: names of outputs passed as NULL"""
    out = out or Outputs(which)
    fi = np.zeros(RATES, dtype=np.uint32) if isinstance(fi, str) else fi
    ptr = {k: (None if k in null else api.dptr(a)) for k, a in out.arrays.items()}
    head = (p, edge[0], edge[1], edge[2], edge[3], edge[4], None if fi is None else api.uptr(fi))
    if which == "posteriors":
        rc = lib.pll_gpu_edge_category_posteriors(*head, ptr["cat_lnl"], ptr["posterior"], ptr["site_rates"], ptr["weight_sums"], ptr["lnl"])
    else:
        s = np.array([0.1, 0.2, 0.3, 0.4]) if isinstance(start, str) else start
        rc = lib.pll_gpu_category_weights_em(*head, None if s is None else api.dptr(s), steps, ptr["weights_out"], ptr["lnl_out"])
    return rc, out


def _refused(lib, which, code, attrs=0, **kw):
    p = _partition(lib, attrs)
    try:
        rc, out = _call(lib, which, p, **kw)
        assert rc == 0
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        assert out.untouched()
    finally:
        lib.pll_partition_destroy(p)


def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    for name, nargs in (("pll_gpu_edge_category_posteriors", 12), ("pll_gpu_category_weights_em", 11)):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert getattr(amd_lib.dll, name)
        assert getattr(amd_lib, name).argtypes and len(getattr(amd_lib, name).argtypes) == nargs, name
    assert re.search(r"#define PLL_GPU_EM_MAX_STEPS 1024\b", hdr)
    for name in ("pllgpu_edge_category_posteriors", "pllgpu_category_weights_em"):
        assert re.search(r"\bint %s\(" % name, dev) and getattr(amd_lib.dll, name), name
    assert re.search(r"#define PLLGPU_EM_MAX_STEPS 1024\b", dev)


@pytest.mark.parametrize("which", CALLS)
def test_null_partition_and_null_freqs_indices(amd_lib, which):
    rc, out = _call(amd_lib, which, None)
    assert rc == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID and out.untouched()
    _refused(amd_lib, which, api.ERROR_PARAM_INVALID, fi=None)


def test_all_five_outputs_null(amd_lib):
    _refused(amd_lib, "posteriors", api.ERROR_PARAM_INVALID, null=("cat_lnl", "posterior", "site_rates", "weight_sums", "lnl"))


def test_null_weights_out(amd_lib):
    _refused(amd_lib, "em", api.ERROR_PARAM_INVALID, null=("weights_out",))


def test_too_many_steps(amd_lib):
    _refused(amd_lib, "em", api.ERROR_PARAM_INVALID, steps=1025)


@pytest.mark.parametrize("start", [(0.1, -0.2, 0.3, 0.8), (0.1, np.nan, 0.3, 0.4), (0.1, np.inf, 0.3, 0.4), (0.0, 0.0, 0.0, 0.0)],
                         ids=["negative", "nan", "inf", "sum0"])
def test_bad_start_weights(amd_lib, start):
    _refused(amd_lib, "em", api.ERROR_PARAM_INVALID, start=np.array(start, dtype=np.float64))


def test_null_start_reads_the_partitions_weights(amd_lib):
    """the partition's own row is checked like a caller's"""
    p = _partition(amd_lib)
    try:
        w = np.array([0.5, -0.5, 0.5, 0.5])
        amd_lib.pll_set_category_weights(p, api.dptr(w))
        rc, out = _call(amd_lib, "em", p, start=None)
        assert rc == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID and out.untouched()
        w = np.array([0.1, 0.2, 0.3, 0.4])
        amd_lib.pll_set_category_weights(p, api.dptr(w))
        rc, out = _call(amd_lib, "em", p, start=None)
        assert rc == 0 and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE and out.untouched()
    finally:
        amd_lib.pll_partition_destroy(p)


BAD = {
    "parent clv": (TIPS + INNER, 0, TIPS + 1, 1, 2),
    "child clv max": (TIPS, 0, 0xFFFFFFFF, 1, 2),
    "parent scaler": (TIPS, INNER, TIPS + 1, 1, 2),
    "child scaler": (TIPS, 0, TIPS + 1, INNER + 3, 2),
    "parent scaler below -1": (TIPS, -2, TIPS + 1, 1, 2),
    "child scaler below -1": (TIPS, 0, TIPS + 1, -5, 2),
    "matrix": (TIPS, 0, TIPS + 1, 1, MATRICES),
}


@pytest.mark.parametrize("which", CALLS)
@pytest.mark.parametrize("what", list(BAD))
def test_an_index_out_of_range(amd_lib, which, what):
    _refused(amd_lib, which, api.ERROR_PARAM_INVALID, edge=BAD[what])


@pytest.mark.parametrize("which", CALLS)
def test_freqs_indices_out_of_range(amd_lib, which):
    _refused(amd_lib, which, api.ERROR_PARAM_INVALID, fi=np.array([0, 0, 1, 0], dtype=np.uint32))


@pytest.mark.parametrize("which", CALLS)
def test_both_ends_pattern_tips(amd_lib, which):
    _refused(amd_lib, which, api.ERROR_PARAM_INVALID, attrs=api.PATTERN_TIP, edge=(0, -1, 1, -1, 2))


@pytest.mark.parametrize("which", CALLS)
@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_unsupported_partitions_are_refused(amd_lib, which, attrs):
    _refused(amd_lib, which, api.ERROR_GPU_UNSUPPORTED, attrs=attrs)


@pytest.mark.parametrize("which", CALLS)
@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_an_index_error_comes_before_a_refusal(amd_lib, which, attrs):
    """the order of the checks: a bad index on a partition that would be refused anyway is PARAM_INVALID"""
    _refused(amd_lib, which, api.ERROR_PARAM_INVALID, attrs=attrs, edge=BAD["child clv max"])
    _refused(amd_lib, which, api.ERROR_PARAM_INVALID, attrs=attrs, fi=np.array([0, 0, 0, 1], dtype=np.uint32))


@pytest.mark.parametrize("which", CALLS)
def test_a_null_argument_comes_before_an_index_error(amd_lib, which):
    p = _partition(amd_lib)
    try:
        null = ("cat_lnl", "posterior", "site_rates", "weight_sums", "lnl") if which == "posteriors" else ("weights_out",)
        rc, out = _call(amd_lib, which, p, edge=BAD["parent clv"], null=null)
        assert rc == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_a_start_weight_error_comes_before_a_refusal(amd_lib):
    _refused(amd_lib, "em", api.ERROR_PARAM_INVALID, attrs=api.SITE_REPEATS, start=np.array([0.1, -0.2, 0.3, 0.8]))


@pytest.mark.parametrize("which", CALLS)
def test_a_refusal_comes_before_the_missing_device(amd_lib, which):
    """host-only partitions have no device either: UNSUPPORTED, not UNAVAILABLE"""
    _refused(amd_lib, which, api.ERROR_GPU_UNSUPPORTED, attrs=api.SITE_REPEATS)


@pytest.mark.parametrize("which", CALLS)
def test_host_only_partition_is_refused_and_outputs_untouched(amd_lib, which, capfd):
    p = _partition(amd_lib)
    try:
        rc, out = _call(amd_lib, which, p)
        assert rc == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert out.untouched()
        name = "pll_gpu_edge_category_posteriors" if which == "posteriors" else "pll_gpu_category_weights_em"
        assert name in capfd.readouterr().err  # the usual line on stderr
        # each output alone, and steps == 0, get as far
        for only in out.arrays:
            rc, o = _call(amd_lib, which, p, null=tuple(k for k in out.arrays if k != only and k != "weights_out"), steps=0 if which == "em" else STEPS)
            assert rc == 0 and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE and o.untouched()
    finally:
        amd_lib.pll_partition_destroy(p)
