"""CPU (no GPU): the ancestral-state entry points are declared, exported and bound, and the argument checks that need
no device answer with the reference's codes (host-only partitions, PLL_AMD_HOST_ONLY=1)."""
import os
import re

import numpy as np
import pytest

from pllamd import api, driver, workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pll_compute_node_ancestral", "pll_compute_node_ancestral_extbuf", "pll_gpu_node_ancestral_async")


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\bint " + name + r"\(pll_partition_t \*partition,", hdr), name
        assert getattr(amd_lib.dll, name)
        assert getattr(amd_lib, name).restype is not None  # api.py gave it a prototype
    # the reference's declarations are cited like every other one
    assert "src/pll.h:799-806" in hdr and "src/pll.h:808-818" in hdr
    assert "pllgpu_node_ancestral(" in open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert amd_lib.dll.pllgpu_node_ancestral


def _calls(lib, p, e, fi, out, bufs):
    plain = lambda part, o: lib.pll_compute_node_ancestral(part, e[0], e[1], e[2], e[3], e[4], fi, o)
    ext = lambda part, o, b: lib.pll_compute_node_ancestral_extbuf(part, e[0], e[1], e[2], e[3], e[4], fi, o, *b)
    asyn = lambda part, o: lib.pll_gpu_node_ancestral_async(part, e[0], e[1], e[2], e[3], e[4], fi, o)
    return plain, ext, asyn


def test_argument_checks_without_a_device(amd_lib):
    case = W.make_case("anc", 4, 8, 50, seed=1)
    fi = api.uptr(np.zeros(4, dtype=np.uint32))
    out = np.zeros((50, 4))
    temp_clv, temp_scaler, ident = np.zeros(50 * 16), np.zeros(200, dtype=np.uint32), np.zeros(80)
    bufs = (api.dptr(temp_clv), api.uptr(temp_scaler), api.dptr(ident))
    with driver.Session(amd_lib, case) as s:
        e = case.edges[0]
        plain, ext, asyn = _calls(amd_lib, s.p, e, fi, out, bufs)
        # NULL partition / output
        for call in (lambda: plain(None, api.dptr(out)), lambda: plain(s.p, None), lambda: ext(None, api.dptr(out), bufs),
                     lambda: ext(s.p, None, bufs), lambda: asyn(None, 1), lambda: asyn(s.p, None)):
            assert call() == 0 and amd_lib.errno() == 113
            assert amd_lib.errmsg() == "Parameter value is NULL!"
        # NULL scratch buffers of the _extbuf form
        for k in range(3):
            b = list(bufs)
            b[k] = None
            assert ext(s.p, api.dptr(out), b) == 0 and amd_lib.errno() == 113 and amd_lib.errmsg() == "NULL buffer pointer"
        # indices out of range
        nodes, mats, scs = case.tips + case.clv_buffers, case.prob_matrices, case.scale_buffers
        for bad in ((nodes, e[1], e[2], e[3], e[4]), (e[0], e[1], nodes, e[3], e[4]), (e[0], e[1], e[2], e[3], mats),
                    (e[0], scs, e[2], e[3], e[4]), (e[0], e[1], e[2], scs, e[4])):
            assert amd_lib.pll_compute_node_ancestral(s.p, *bad, fi, api.dptr(out)) == 0 and amd_lib.errno() == 113, bad
        assert amd_lib.pll_compute_node_ancestral(s.p, e[0], e[1], e[2], e[3], e[4], None, api.dptr(out)) == 0 and amd_lib.errno() == 113
        # everything in order, but no device behind the partition: refused loudly, nothing computed on the host
        assert plain(s.p, api.dptr(out)) == 0 and amd_lib.errno() == 900
        assert ext(s.p, api.dptr(out), bufs) == 0 and amd_lib.errno() == 900
        assert asyn(s.p, 1) == 0 and amd_lib.errno() == 900
        assert not out.any() and not temp_clv.any() and not temp_scaler.any() and not ident.any()


def test_site_repeats_and_pattern_tip_nodes_are_refused(amd_lib):
    fi = api.uptr(np.zeros(4, dtype=np.uint32))
    out = np.zeros((50, 4))
    case = W.make_case("anc_rep", 4, 8, 50, attributes=api.SITE_REPEATS, seed=1)
    with driver.Session(amd_lib, case) as s:
        e = case.edges[0]
        assert amd_lib.pll_compute_node_ancestral(s.p, e[0], e[1], e[2], e[3], e[4], fi, api.dptr(out)) == 0
        assert amd_lib.errno() == 130  # PLL_ERROR_EINVAL
        assert amd_lib.errmsg() == "Site repeats are not compatible with ancestral state reconstruction!"
        assert amd_lib.pll_gpu_node_ancestral_async(s.p, e[0], e[1], e[2], e[3], e[4], fi, 1) == 0 and amd_lib.errno() == 130
    case = W.make_case("anc_tip", 4, 8, 50, attributes=api.PATTERN_TIP, seed=1)
    with driver.Session(amd_lib, case) as s:
        e = case.edges[0]
        # the node's end is a pattern tip: no CLV to read (the reference dereferences NULL)
        assert amd_lib.pll_compute_node_ancestral(s.p, 0, -1, e[0], e[1], 0, fi, api.dptr(out)) == 0 and amd_lib.errno() == 113
        # the other end may be one
        assert amd_lib.pll_compute_node_ancestral(s.p, e[0], e[1], 0, -1, 0, fi, api.dptr(out)) == 0 and amd_lib.errno() == 900
