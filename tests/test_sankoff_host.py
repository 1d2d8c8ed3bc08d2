"""CPU (no GPU): the weighted-parsimony entry points are declared, exported and bound; pll_parsimony_create and
pll_set_parsimony_sequence leave the host fields the reference leaves (tests/golden/sankoff.json, and the live reference
where it is built); every out-of-range index of every call is refused before the device is asked for; a host-only
structure refuses the device calls; the two kinds of structure refuse each other's calls; pll_parsimony_destroy frees
an own structure, a foreign one and NULL.

The NumPy restatement that the GPU tests lean on (pllamd.sankoff_cases.Model) is checked here against the same file:
every score, score-buffer CRC, ancestral CRC and insertion score the reference recorded."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from pllamd import api, driver, parsimony_cases as PC, sankoff_cases as SC
import sankoff_common as K

ROOT = K.ROOT
GOLDEN = K.golden()
REFERENCE_SYMBOLS = ("pll_parsimony_create", "pll_set_parsimony_sequence", "pll_parsimony_build", "pll_parsimony_score",
                     "pll_parsimony_reconstruct", "pll_parsimony_destroy")
NEW_SYMBOLS = ("pll_gpu_parsimony_invalidate", "pll_gpu_parsimony_insertion_scores", "pll_gpu_sync_parsimony",
               "pll_gpu_synchronize_parsimony", "pll_gpu_fastparsimony_last_launch_count")
DEVICE_SYMBOLS = ("pllgpu_spars_create", "pllgpu_spars_destroy", "pllgpu_spars_upload", "pllgpu_spars_download",
                  "pllgpu_spars_download_ancestral", "pllgpu_spars_build", "pllgpu_spars_score", "pllgpu_spars_reconstruct",
                  "pllgpu_spars_insertion_scores", "pllgpu_spars_last_launch_count", "pllgpu_spars_synchronize")
NEG_INF = -math.inf


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


@pytest.fixture(scope="module")
def ref_or_none():
    p = os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so")
    return api.PllLib(p) if os.path.exists(p) else None


def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    for name in REFERENCE_SYMBOLS + NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert getattr(amd_lib.dll, name)
        assert getattr(amd_lib, name).argtypes, name  # api.py gave it a prototype
    for cite in ("src/pll.h:502-508", "src/pll.h:2535-2559", "src/parsimony.c:117-202", "src/parsimony.c:204-284",
                 "src/parsimony.c:286-307", "src/parsimony.c:309-383", "src/parsimony.c:24-67"):
        assert cite in hdr, cite
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    for name in DEVICE_SYMBOLS:
        assert name + "(" in dev and getattr(amd_lib.dll, name), name


def test_struct_sizes():
    assert C.sizeof(api.ParsRecOp) == 16 and api.ParsRecOp.parent_ancestral_index.offset == 12
    src = open(os.path.join(ROOT, "libpll-2_amd", "csrc", "host", "abi_check.c")).read()
    assert "sizeof(pll_pars_recop_t) == 16" in src


def _fields(st):
    return [int(x) for x in (st.tips, st.states, st.sites, st.score_buffers, st.ancestral_buffers, st.inner_nodes, st.attributes,
                             st.packedvector_count, st.const_cost, st.informative_count)]


@pytest.mark.parametrize("case,mname", SC.CASE_MATRICES, ids=SC.CASE_MATRIX_IDS)
def test_create_and_tips_equal_the_reference(amd_lib, ref_or_none, case, mname):
    exp = GOLDEN[case.name][mname]
    with K.session(amd_lib, case, mname) as s:
        st = s.s
        assert _fields(st) == exp["fields"]
        assert st.alignment == 0 and not st.packedvector and not st.node_cost and not st.informative
        m = SC.matrix(mname, case.states)
        assert (api.as_np(st.score_matrix, case.states ** 2, np.float64) == m.ravel()).all()
        # every score buffer and every ancestral buffer is allocated and zero; no ancestral buffer below `tips`
        assert all(not s.buffer(i).any() for i in range(case.buffers))
        assert all(not st.anc_states[t] for t in range(case.tips))
        assert all(not s.ancestral(i).any() for i in range(case.tips, case.tips + case.ancestral_buffers))
        K.set_tips(s, amd_lib, case)
        assert [SC.crc(s.buffer(t), "<f8") for t in range(case.tips)] == exp["tip_crc"]
        # inf = the largest entry + 1, zero where the character allows the state
        assert set(np.unique(s.buffer(0))) <= {0.0, m.max() + 1.0}
        if ref_or_none is not None:
            with K.session(ref_or_none, case, mname) as rs:
                assert _fields(rs.s) == _fields(st)
                K.set_tips(rs, ref_or_none, case)
                assert all((rs.buffer(t) == s.buffer(t)).all() for t in range(case.tips))


def test_illegal_character(amd_lib, capfd):
    case = SC.BY_NAME["dna_8x63"]
    with K.session(amd_lib, case, "unit") as s:
        cmap = SC.charmap(amd_lib, 4)
        assert s.set_sequence(0, cmap, b"ACGT" + b"!" + b"A" * (case.sites - 5)) == 0
        assert amd_lib.errno() == api.ERROR_TIPDATA_ILLEGALSTATE == 114
        assert amd_lib.errmsg() == 'Illegal state code in tip "!"'
        C.CDLL(None).fflush(None)  # the library's own printf is what capfd sees
        assert 'Illegal state code in tip "!"\n' in capfd.readouterr().out


def test_create_refusals(amd_lib):
    m = np.zeros((65, 65))
    for args in ((4, 0, 10, api.dptr(m), 2, 2), (4, 65, 10, api.dptr(m), 2, 2), (0, 4, 10, api.dptr(m), 2, 2), (4, 4, 0, api.dptr(m), 2, 2),
                 (4, 4, 10, None, 2, 2)):
        assert not amd_lib.pll_parsimony_create(*args)
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID, args
    for states in (1, 64):
        p = amd_lib.pll_parsimony_create(3, states, 5, api.dptr(m), 1, 1)
        assert p and p.contents.states == states
        amd_lib.pll_parsimony_destroy(p)


def test_every_out_of_range_index_is_refused(amd_lib):
    case = SC.BY_NAME["dna_8x63"]
    nbuf, lo, hi = case.buffers, case.tips, case.tips + case.ancestral_buffers
    with K.session(amd_lib, case, "unit") as s:
        cmap = K.set_tips(s, amd_lib, case)
        before = [s.buffer(i) for i in range(nbuf)]

        def refused(call, expect=None):
            api.C.c_int.in_dll(amd_lib.dll, "pll_errno").value = 0
            got = call()
            assert amd_lib.errno() == api.ERROR_PARAM_INVALID, (got, amd_lib.errmsg())
            if expect is not None:
                assert got == expect

        refused(lambda: s.set_sequence(nbuf, cmap, b"A" * case.sites), 0)
        for bad in ((nbuf, 0, 1), (8, nbuf, 1), (8, 0, nbuf)):
            refused(lambda: s.build([(8, 0, 1), bad]), NEG_INF)
        refused(lambda: amd_lib.pll_parsimony_build(s.pars, api.make_pars_ops([(8, 0, 1)]), 0), NEG_INF)
        refused(lambda: amd_lib.pll_parsimony_build(s.pars, None, 1), NEG_INF)
        refused(lambda: s.score(nbuf), NEG_INF)
        good = (8, 8, 8, 8)
        for bad in ((nbuf, 9, 8, 8), (9, lo - 1, 8, 8), (9, hi, 8, 8), (9, 9, nbuf, 8), (9, 9, 8, lo - 1), (9, 9, 8, hi)):
            refused(lambda: s.reconstruct(cmap, [good, bad]))
        refused(lambda: s.reconstruct(cmap, [(nbuf, 8, 0, 0)]))
        refused(lambda: s.reconstruct(cmap, [(8, hi, 0, 0)]))
        refused(lambda: amd_lib.pll_parsimony_reconstruct(s.pars, None, api.make_pars_recops([good]), 1))
        refused(lambda: amd_lib.pll_parsimony_reconstruct(s.pars, s._map(cmap), None, 1))
        out = np.full(2, 7.5)
        for node, edges in ((nbuf, [0, 1, 2, 3]), (0, [nbuf, 1, 2, 3]), (0, [0, 1, 2, nbuf])):
            e = np.array(edges, dtype=np.uint32)
            refused(lambda: amd_lib.pll_gpu_parsimony_insertion_scores(s.pars, node, api.uptr(e), 2, api.dptr(out)), 0)
        refused(lambda: amd_lib.pll_gpu_parsimony_insertion_scores(s.pars, 0, None, 2, api.dptr(out)), 0)
        refused(lambda: amd_lib.pll_gpu_parsimony_invalidate(s.pars, nbuf), 0)
        refused(lambda: amd_lib.pll_gpu_sync_parsimony(s.pars, max(nbuf, hi)), 0)
        assert (out == 7.5).all()
        assert all((s.buffer(i) == before[i]).all() for i in range(nbuf))
        assert all(not s.ancestral(i).any() for i in range(lo, hi))


def test_device_calls_refuse_a_host_only_structure(amd_lib):
    case = SC.BY_NAME["dna_8x63"]
    ops, root = SC.tree_ops(case)
    with K.session(amd_lib, case, "unit") as s:
        cmap = K.set_tips(s, amd_lib, case)
        assert s.build(ops) == NEG_INF and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert s.score(0) == NEG_INF and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        api.C.c_int.in_dll(amd_lib.dll, "pll_errno").value = 0
        s.reconstruct(cmap, SC.reconstruct_ops(ops, root, case.tips))
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert all(not s.ancestral(i).any() for i in range(case.tips, case.tips + case.ancestral_buffers))
        e, out = np.array([0, 1], dtype=np.uint32), np.full(1, 7.5)
        assert amd_lib.pll_gpu_parsimony_insertion_scores(s.pars, 2, api.uptr(e), 1, api.dptr(out)) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE and out[0] == 7.5
        assert amd_lib.pll_gpu_sync_parsimony(s.pars, -1) == 0 and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert amd_lib.pll_gpu_synchronize_parsimony(s.pars) == 0 and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert amd_lib.pll_gpu_fastparsimony_last_launch_count(s.pars) == 0
        assert amd_lib.pll_gpu_parsimony_invalidate(s.pars, 0) == 1  # bookkeeping alone


def test_the_two_kinds_refuse_each_other(amd_lib):
    fcase = PC.BY_NAME["dna_8x300_tail"]
    seqs, weights = PC.alignment(fcase)
    case = SC.BY_NAME["dna_8x63"]
    with driver.ParsimonySession(amd_lib, 4, seqs, PC.charmap(amd_lib, fcase), weights, api.PATTERN_TIP) as fast, \
            K.session(amd_lib, case, "unit") as weighted:
        cmap = (C.c_ulonglong * 256)(*[int(x) for x in SC.charmap(amd_lib, 4)])
        op, rop = api.make_pars_ops([(8, 0, 1)]), api.make_pars_recops([(8, 8, 8, 8)])
        e, out, uout = np.array([0, 1], dtype=np.uint32), np.full(1, 7.5), np.full(1, 77, dtype=np.uint32)
        calls = [
            lambda: amd_lib.pll_set_parsimony_sequence(fast.pars, 0, cmap, b"A" * fcase.sites),
            lambda: amd_lib.pll_parsimony_build(fast.pars, op, 1),
            lambda: amd_lib.pll_parsimony_score(fast.pars, 0),
            lambda: amd_lib.pll_parsimony_reconstruct(fast.pars, cmap, rop, 1),
            lambda: amd_lib.pll_gpu_parsimony_insertion_scores(fast.pars, 2, api.uptr(e), 1, api.dptr(out)),
            lambda: amd_lib.pll_gpu_parsimony_invalidate(fast.pars, 0),
            lambda: amd_lib.pll_fastparsimony_update_vectors(weighted.pars, op, 1),
            lambda: amd_lib.pll_fastparsimony_edge_score(weighted.pars, 0, 1),
            lambda: amd_lib.pll_fastparsimony_root_score(weighted.pars, 0),
            lambda: amd_lib.pll_gpu_fastparsimony_edge_scores(weighted.pars, api.uptr(e), 1, api.uptr(uout)),
            lambda: amd_lib.pll_gpu_fastparsimony_insertion_scores(weighted.pars, 2, api.uptr(e), 1, api.uptr(uout)),
        ]
        for i, call in enumerate(calls):
            api.C.c_int.in_dll(amd_lib.dll, "pll_errno").value = 0
            call()
            assert amd_lib.errno() == api.ERROR_PARAM_INVALID, i
        assert out[0] == 7.5 and uout[0] == 77
        # a structure the library has never seen
        foreign = api.Parsimony()
        assert amd_lib.pll_parsimony_score(C.byref(foreign), 0) == NEG_INF and amd_lib.errno() == api.ERROR_PARAM_INVALID


def test_destroy_own_foreign_and_null(amd_lib):
    m = np.zeros((4, 4))
    amd_lib.pll_parsimony_destroy(amd_lib.pll_parsimony_create(4, 4, 10, api.dptr(m), 3, 2))
    amd_lib.pll_parsimony_destroy(amd_lib.pll_parsimony_create(4, 4, 10, api.dptr(m), 0, 0))
    # what another library's pll_parsimony_create leaves
    libc = C.CDLL(None)
    libc.calloc.restype = C.c_void_p
    libc.calloc.argtypes = [C.c_size_t, C.c_size_t]
    raw = libc.calloc(1, C.sizeof(api.Parsimony))
    st = C.cast(raw, api.ParsimonyP).contents
    st.tips, st.states, st.sites, st.score_buffers, st.ancestral_buffers = 4, 4, 10, 3, 2
    st.score_matrix = C.cast(libc.calloc(16, 8), api.c_double_p)
    sb = libc.calloc(7, C.sizeof(C.c_void_p))
    for i in range(7):
        C.cast(sb, C.POINTER(C.c_void_p))[i] = libc.calloc(40, 8)
    st.sbuffer = C.cast(sb, C.POINTER(api.c_double_p))
    an = libc.calloc(6, C.sizeof(C.c_void_p))
    for i in range(4, 6):
        C.cast(an, C.POINTER(C.c_void_p))[i] = libc.calloc(10, 4)
    st.anc_states = C.cast(an, C.POINTER(api.c_uint_p))
    amd_lib.pll_parsimony_destroy(raw)
    amd_lib.pll_parsimony_destroy(None)


@pytest.mark.parametrize("case,mname", SC.CASE_MATRICES, ids=SC.CASE_MATRIX_IDS)
def test_numpy_model_reproduces_the_reference(amd_lib, case, mname):
    """the stand-in the GPU tests use computes what the reference recorded, bit for bit"""
    exp = GOLDEN[case.name][mname]
    model, cmap = K.model(amd_lib, case, mname)
    ops, root = SC.tree_ops(case)
    assert [SC.crc(model.sb[t], "<f8") for t in range(case.tips)] == exp["tip_crc"]
    assert model.build(ops).hex() == exp["score"]
    assert {str(p): SC.crc(model.sb[p], "<f8") for p, _, _ in ops} == exp["buffer_crc"]
    model.reconstruct(cmap, SC.reconstruct_ops(ops, root, case.tips))
    assert {str(p): SC.crc(model.anc[p], "<u4") for p, _, _ in ops} == exp["anc_crc"]
    dops, edges = K.insertion_tree(case)
    model.build(dops)
    assert [model.insertion_score(case.tips - 1, a, b).hex() for a, b in edges] == exp["insertion_scores"]
