"""CPU (no GPU): everything the host layer of libpll_amd.so decides about pll_gpu_nj_trees and
pll_gpu_bootstrap_distance_trees before a device is needed - the symbols and the struct mirror, every
PLL_ERROR_PARAM_INVALID refusal in the order include/pll_amd.h states, outputs untouched behind a refusal, and
replicates == 0.

The refusals of pll_gpu_bootstrap_distance_trees are checked on a host-only partition (PLL_AMD_HOST_ONLY): behind the last
check of the list stands the device, so a call that passes them all reports PLL_ERROR_GPU_UNAVAILABLE there. The refusal of
pattern weights that add up to 0 stands behind the device check and is made in tests/test_gpu_bootstrap_trees.py.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import distance_cases as DC
import nj_cases as NC
from pllamd import api, driver, workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.5
FIELDS = ("parent", "length", "distances", "status", "weights")


def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    assert re.search(r"\bint pll_gpu_nj_trees\(", hdr) and re.search(r"\bint pll_gpu_bootstrap_distance_trees\(", hdr)
    assert re.search(r"\}\s*pll_gpu_bootstrap_trees_t;", hdr)
    assert len(amd_lib.pll_gpu_nj_trees.argtypes) == 7 and len(amd_lib.pll_gpu_bootstrap_distance_trees.argtypes) == 10
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    for name in ("pllgpu_nj_trees", "pllgpu_bootstrap_distance_trees", "pllgpu_nj_scratch_bytes"):
        assert re.search(r"\b%s\(" % name, dev) and getattr(amd_lib.dll, name)
    assert re.search(r"#define PLLGPU_NJ_BATCH_MAX_BYTES ", dev) and re.search(r"#define PLLGPU_BOOTSTRAP_MAX_BYTES ", dev)
    assert "PLL_AMD_NJ_BATCH_BYTES" in dev and "PLL_AMD_BOOTSTRAP_BYTES" in dev


def test_the_struct_mirror_against_a_c_program(tmp_path):
    """sizeof and offsetof of pll_gpu_bootstrap_trees_t as a C compiler sees the header, against the ctypes mirror"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pll_amd.h"\nint main(void)\n{\n'
                   '  printf("%zu", sizeof(pll_gpu_bootstrap_trees_t));\n'
                   + "".join('  printf(" %%zu", offsetof(pll_gpu_bootstrap_trees_t, %s));\n' % f for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert [name for name, _ in api.BootstrapTrees._fields_] == list(FIELDS)
    assert seen == [C.sizeof(api.BootstrapTrees)] + [getattr(api.BootstrapTrees, f).offset for f in FIELDS] == [40, 0, 8, 16, 24, 32]
    abi = open(os.path.join(ROOT, "libpll-2_amd", "csrc", "host", "abi_check.c")).read()
    assert "sizeof(pll_gpu_bootstrap_trees_t) == 40" in abi and "AT(pll_gpu_bootstrap_trees_t, weights, 32)" in abi


# ---- pll_gpu_nj_trees ------------------------------------------------------------------------------------------------
def _batch(n=5, reps=4):
    return np.stack([NC.noisy(n) if b % 2 else NC.additive(n) for b in range(reps)])


def _trees_refused(lib, matrices, flags=0, code=api.ERROR_PARAM_INVALID):
    with pytest.raises(RuntimeError) as err:
        api.nj_trees(lib, matrices, flags, fill=SENTINEL)
    assert lib.errno() == code, (lib.errno(), lib.errmsg())
    assert (err.value.outputs["parent"] == int(SENTINEL)).all() and (err.value.outputs["length"] == SENTINEL).all()
    return str(err.value)


@pytest.mark.parametrize("which", ["distances", "parent", "length"])
def test_nj_trees_each_null_argument(amd_lib, capfd, which):
    d = np.ascontiguousarray(_batch())
    parent, length = np.full((4, 8), 77, dtype=np.int32), np.full((4, 8), SENTINEL)
    args = {"distances": api.dptr(d), "parent": parent.ctypes.data_as(C.POINTER(C.c_int)), "length": api.dptr(length)}
    args[which] = None
    for reps in (4, 0):  # the NULL check stands before "replicates == 0 succeeds"
        assert amd_lib.pll_gpu_nj_trees(args["distances"], 5, reps, 0, -1, args["parent"], args["length"]) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
        assert (parent == 77).all() and (length == SENTINEL).all()
    assert "pll_gpu_nj_trees" in capfd.readouterr().err  # the usual line on stderr


def test_nj_trees_count_flags_and_entries_in_that_order(amd_lib):
    bad = _batch().copy()
    bad[3, 0, 1] = -1.0
    assert "at least 3" in _trees_refused(amd_lib, bad[:, :2, :2], flags=6)  # count before flags
    assert "flag" in _trees_refused(amd_lib, bad, flags=6)                   # flags before the entries
    assert "flag" in _trees_refused(amd_lib, _batch(), flags=0x80000001)
    assert "[3][0][1]" in _trees_refused(amd_lib, bad)
    for n in (1, 2):
        assert "at least 3" in _trees_refused(amd_lib, np.zeros((2, n, n)))


@pytest.mark.parametrize("value", [-1e-300, -1.0, float("nan"), float("inf"), -float("inf")])
def test_nj_trees_refuses_an_entry_of_any_matrix(amd_lib, value):
    """a negative or non-finite entry in replicate 3 of 4 (and in the others) refuses the whole call, all outputs untouched"""
    for b, x, y in ((3, 0, 1), (0, 2, 8), (1, 7, 8), (3, 7, 8)):
        m = _batch(9).copy()
        m[b, x, y] = value
        assert f"[{b}][{x}][{y}]" in _trees_refused(amd_lib, m)


def test_nj_trees_reads_only_the_upper_triangles_in_its_checks(amd_lib):
    m = _batch().copy()
    m[:, np.tril_indices(5)[0], np.tril_indices(5)[1]] = np.nan
    if not amd_lib.pll_gpu_available():
        _trees_refused(amd_lib, m, code=api.ERROR_GPU_UNAVAILABLE)
    else:
        parent, _ = api.nj_trees(amd_lib, m)
        assert np.array_equal(parent[1], NC.expected("noisy", 5, "nj")[0])


def test_nj_trees_without_replicates_succeeds_and_writes_nothing(amd_lib):
    d = np.full((1, 5, 5), np.nan)  # (nothing of it is read)
    parent, length = np.full(8, 77, dtype=np.int32), np.full(8, SENTINEL)
    ptr = parent.ctypes.data_as(C.POINTER(C.c_int))
    for flags in (0, api.NJ_BIONJ):
        assert amd_lib.pll_gpu_nj_trees(api.dptr(d), 5, 0, flags, -1, ptr, api.dptr(length)) == 1
    assert (parent == 77).all() and (length == SENTINEL).all()
    # ... behind the count and flag checks
    assert amd_lib.pll_gpu_nj_trees(api.dptr(d), 2, 0, 0, -1, ptr, api.dptr(length)) == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID
    assert amd_lib.pll_gpu_nj_trees(api.dptr(d), 5, 0, 2, -1, ptr, api.dptr(length)) == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID


# ---- pll_gpu_bootstrap_distance_trees --------------------------------------------------------------------------------
SEQ = [b"ACGTACGTACGTACGTACGT", b"ACGTACGAACGTRCGTACGT", b"ACGTTCGTAC-TACGTACGT", b"ACCTACGTACGTACGTANGT", b"ACGTACGTACGTACGTACGA"]
GOOD = dict(t_start=0.1, t_min=1e-6, t_max=100.0, tolerance=1e-6, max_iters=32, matrix_index=-1)
REPS = 3


def _tips(lib, attrs=0, **kw):
    return DC.Tips(lib, 4, 4, SEQ, W.map_nt(), W.GTR_DNA["exch"], W.GTR_DNA["freqs"], attrs=attrs, **kw)


def _untouched(outputs):
    return all((a == np.asarray(SENTINEL).astype(a.dtype)).all() for a in outputs.values())


def _refused(lib, code, tips=(0, 1, 2, 3, 4), flags=0, options=None, **kw):
    with _tips(lib, **kw) as b:
        with pytest.raises(RuntimeError) as err:
            api.bootstrap_distance_trees(lib, b.p, tips, b.pi, driver.newton_options(**dict(GOOD, **(options or {}))), flags, 7, 0, REPS,
                                         fill=SENTINEL)
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        assert set(err.value.outputs) == set(FIELDS) and _untouched(err.value.outputs)
        return str(err.value)


def test_bootstrap_checks_in_their_order_on_a_host_only_partition(amd_lib, monkeypatch):
    """the checks of pll_gpu_distance_tree in its order - the list, the options, the tips' codes, the refusals, then count
    and flags - each met with a later one wrong too"""
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")
    inv, uns = api.ERROR_PARAM_INVALID, api.ERROR_GPU_UNSUPPORTED
    assert "is no tip" in _refused(amd_lib, inv, tips=(0, 5, 2), flags=2, options=dict(tolerance=0.0))
    assert "options" in _refused(amd_lib, inv, options=dict(tolerance=0.0, matrix_index=0), flags=2)
    assert "matrix_index" in _refused(amd_lib, inv, options=dict(matrix_index=0), dense=(1,))
    assert "not given by codes" in _refused(amd_lib, inv, dense=(1,), tips=(0, 1), flags=2)
    assert "prop_invar" in _refused(amd_lib, uns, prop_invar=0.2, flags=2)
    _refused(amd_lib, uns, attrs=api.SITE_REPEATS, tips=(0, 1))
    # every check of the distances passes (a host-only partition has no device): the missing device is reported
    _refused(amd_lib, api.ERROR_GPU_UNAVAILABLE)
    _refused(amd_lib, api.ERROR_GPU_UNAVAILABLE, flags=api.NJ_BIONJ)
    _refused(amd_lib, api.ERROR_GPU_UNAVAILABLE, tips=(0, 1), flags=2)
    assert "at least 3" in _refused(amd_lib, inv, tips=())


@pytest.mark.parametrize("which", ["partition", "out", "parent", "length", "tips", "params_indices", "options"])
def test_bootstrap_each_null_argument(amd_lib, monkeypatch, which):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")
    with _tips(amd_lib) as b:
        tips = np.arange(5, dtype=np.uint32)
        parent, length = np.full((REPS, 8), 77, dtype=np.int32), np.full((REPS, 8), SENTINEL)
        rec = api.BootstrapTrees(parent=None if which == "parent" else parent.ctypes.data_as(C.POINTER(C.c_int)),
                                 length=None if which == "length" else api.dptr(length))
        opt = driver.newton_options(**GOOD)
        args = {"partition": b.p, "tips": api.uptr(tips), "params_indices": api.uptr(b.pi), "options": C.byref(opt), "out": C.byref(rec)}
        if which in args:
            args[which] = None
        # (the first check - partition, out, parent, length - comes before anything else is looked at: tips[1] is no tip)
        tips[1] = 99 if which in ("partition", "out", "parent", "length") else 1
        assert amd_lib.pll_gpu_bootstrap_distance_trees(args["partition"], args["tips"], 5, args["params_indices"], args["options"], 0, 7, 0, REPS,
                                                        args["out"]) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
        assert (parent == 77).all() and (length == SENTINEL).all()


def test_bootstrap_without_replicates_succeeds_and_writes_nothing(amd_lib, monkeypatch):
    """after the first check and before every other: a list that names no tip, options out of range, two tips"""
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")
    with _tips(amd_lib) as b:
        opt = driver.newton_options(**dict(GOOD, tolerance=0.0))
        out = api.bootstrap_distance_trees(amd_lib, b.p, (0, 9), b.pi, opt, 6, 7, 0, 0, fill=SENTINEL)
        assert set(out) == set(FIELDS) and all(a.shape[0] == 0 for a in out.values())
        tips = np.array([0, 9], dtype=np.uint32)
        parent, length = np.full(8, 77, dtype=np.int32), np.full(8, SENTINEL)
        rec = api.BootstrapTrees(parent=parent.ctypes.data_as(C.POINTER(C.c_int)), length=api.dptr(length))
        assert amd_lib.pll_gpu_bootstrap_distance_trees(b.p, api.uptr(tips), 2, api.uptr(b.pi), C.byref(opt), 6, 7, 0, 0, C.byref(rec)) == 1
        assert (parent == 77).all() and (length == SENTINEL).all()
        # ... but not before the first
        rec.length = None
        assert amd_lib.pll_gpu_bootstrap_distance_trees(b.p, api.uptr(tips), 2, api.uptr(b.pi), C.byref(opt), 6, 7, 0, 0, C.byref(rec)) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID
