"""CPU (no GPU): the fast-parsimony entry points are declared, exported and bound; pll_fastparsimony_init's host work -
site classification and tip packing - equals the reference's for every case and attribute set of
tests/golden/fastparsimony.json (host-only partitions, PLL_AMD_HOST_ONLY=1); pll_parsimony_destroy frees a
structure another library made; the device calls refuse a structure with no device behind it.

The NumPy restatement of the Fitch step that the GPU tests use where no reference library is at hand
(pllamd.parsimony_cases.Model) is checked here against the same file: every node cost, vector CRC and score the
reference recorded."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from pllamd import api, driver, parsimony_cases as PC
from utree import UTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "fastparsimony.json")))
REFERENCE_SYMBOLS = ("pll_fastparsimony_init", "pll_fastparsimony_update_vectors", "pll_fastparsimony_update_vector",
                     "pll_fastparsimony_update_vector_4x4", "pll_fastparsimony_edge_score", "pll_fastparsimony_edge_score_4x4",
                     "pll_fastparsimony_root_score", "pll_parsimony_destroy")
NEW_SYMBOLS = ("pll_gpu_sync_parsimony", "pll_gpu_fastparsimony_edge_scores", "pll_gpu_fastparsimony_insertion_scores",
               "pll_gpu_fastparsimony_last_launch_count", "pll_gpu_synchronize_parsimony")
CASE_SETS = [(c, label, attrs) for c in PC.CASES for label, attrs in PC.attribute_sets(c)]
CASE_SET_IDS = [f"{c.name}-{label}" for c, label, _ in CASE_SETS]


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


def _session(lib, case, attrs):
    seqs, weights = PC.alignment(case)
    return driver.ParsimonySession(lib, case.states, seqs, PC.charmap(lib, case), weights, attrs)


def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    for name in REFERENCE_SYMBOLS + NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", hdr), name
        assert getattr(amd_lib.dll, name)
        assert getattr(amd_lib, name).argtypes, name  # api.py gave it a prototype
    # the reference's declarations are cited like every other one
    for cite in ("src/pll.h:468-492", "src/pll.h:495-500", "src/pll.h:186", "src/pll.h:2574", "src/pll.h:2576",
                 "src/pll.h:2580", "src/pll.h:2583", "src/pll.h:2559"):
        assert cite in hdr, cite
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    for name in ("pllgpu_pars_create", "pllgpu_pars_destroy", "pllgpu_pars_upload", "pllgpu_pars_download", "pllgpu_pars_update",
                 "pllgpu_pars_edge_scores", "pllgpu_pars_insertion_scores", "pllgpu_pars_synchronize"):
        assert name + "(" in dev and getattr(amd_lib.dll, name)
    # the vector-ISA names of the reference are not part of the surface, like those of the core functions
    for name in ("pll_fastparsimony_update_vector_avx2", "pll_fastparsimony_edge_score_4x4_sse"):
        assert not hasattr(amd_lib.dll, name)


def test_struct_sizes():
    assert C.sizeof(api.Parsimony) == 104 and C.sizeof(api.ParsBuildOp) == 12
    assert api.Parsimony.packedvector.offset == 32 and api.Parsimony.informative_count.offset == 64
    assert api.Parsimony.anc_states.offset == 96
    src = open(os.path.join(ROOT, "libpll-2_amd", "csrc", "host", "abi_check.c")).read()
    assert "sizeof(pll_parsimony_t) == 104" in src and "sizeof(pll_pars_buildop_t) == 12" in src


@pytest.mark.parametrize("case,label,attrs", CASE_SETS, ids=CASE_SET_IDS)
def test_init_fields_and_tip_vectors_equal_the_reference(amd_lib, case, label, attrs):
    exp = GOLDEN[case.name][label]
    with _session(amd_lib, case, attrs) as s:
        st = s.s
        assert (st.tips, st.inner_nodes, st.sites, st.states) == (case.tips, case.tips - 1, case.sites, case.states)
        assert st.attributes == attrs
        assert st.packedvector_count == exp["packedvector_count"]
        assert st.const_cost == exp["const_cost"]
        assert st.informative_count == exp["informative_count"]
        assert PC.informative_string(s.informative()) == exp["informative"]
        assert [PC.crc(s.vector(t)) for t in range(case.tips)] == exp["tip_crc"]
        # inner mirrors are allocated and zero-filled, costs are zero
        for n in range(case.tips, s.nodes):
            assert not s.vector(n).any()
        assert not s.costs().any()


def test_padding_words_are_all_ones(amd_lib):
    case = PC.BY_NAME["dna_8x31_one_word"]
    with _session(amd_lib, case, api.PATTERN_TIP | api.ARCH_AVX2) as s:
        assert s.words == 8
        for t in range(case.tips):
            v = s.vector(t)
            assert (v[:, 1:] == 0xFFFFFFFF).all()
            used = GOLDEN[case.name]["tip"]["informative_count"]  # unweighted: one bit per informative site
            assert ((v[:, 0] >> np.uint32(used)) == (0xFFFFFFFF >> used)).all()


@pytest.mark.parametrize("case", PC.CASES, ids=[c.name for c in PC.CASES])
def test_numpy_model_reproduces_the_reference(amd_lib, case):
    """the stand-in the GPU tests use when the reference library is absent computes what the reference recorded"""
    exp = GOLDEN[case.name]["tip"]
    ops, edge = PC.traversal(case)
    with _session(amd_lib, case, api.PATTERN_TIP) as s:
        model = PC.Model([s.vector(t) for t in range(case.tips)], case.nodes, s.s.const_cost)
    model.update(ops)
    assert [int(x) for x in model.cost[:case.tips + len(ops)]] == exp["node_cost"]
    assert {str(p): PC.crc(model.vec[p]) for p, _, _ in ops} == exp["vector_crc"]
    assert model.edge_score(*edge) == exp["edge_score"] and model.root_score(edge[0]) == exp["root_score"]
    if case.tips - 1 >= 4:
        tree = UTree(case.tips - 1, np.random.default_rng(case.seed + 1000))
        dops, edges = PC.directional_ops(tree, case.tips)
        model.update(dops)
        assert [model.insertion_score(case.tips - 1, a, b) for a, b in edges] == exp["insertion_scores"]


def test_init_refusals(amd_lib):
    case = PC.BY_NAME["s61_12x200"]
    seqs, _ = PC.alignment(case)
    with pytest.raises(RuntimeError, match=r"\[129\] Use PLL_ATTRIB_PATTERN_TIP for more than 20 states\."):
        driver.ParsimonySession(amd_lib, case.states, seqs, PC.charmap(amd_lib, case), None, 0)
    case = PC.BY_NAME["dna_8x31_one_word"]
    seqs, _ = PC.alignment(case)
    with pytest.raises(RuntimeError, match=r"\[902\]"):
        driver.ParsimonySession(amd_lib, case.states, seqs, PC.charmap(amd_lib, case), None, api.SITE_REPEATS)


def test_destroy_frees_a_foreign_structure(amd_lib):
    """what another library's pll_parsimony_create leaves: calloc'd struct, weighted-parsimony buffers, no fast fields"""
    libc = C.CDLL(None)
    libc.calloc.restype = C.c_void_p
    libc.calloc.argtypes = [C.c_size_t, C.c_size_t]
    tips, score_buffers, anc_buffers = 4, 3, 2
    raw = libc.calloc(1, C.sizeof(api.Parsimony))
    st = C.cast(raw, api.ParsimonyP).contents
    st.tips, st.inner_nodes, st.states, st.sites = tips, tips - 1, 4, 10
    st.score_buffers, st.ancestral_buffers = score_buffers, anc_buffers
    st.score_matrix = C.cast(libc.calloc(16, 8), api.c_double_p)
    sb = libc.calloc(score_buffers + tips, C.sizeof(C.c_void_p))
    for i in range(score_buffers + tips):
        C.cast(sb, C.POINTER(C.c_void_p))[i] = libc.calloc(40, 8)
    st.sbuffer = C.cast(sb, C.POINTER(api.c_double_p))
    an = libc.calloc(anc_buffers + tips, C.sizeof(C.c_void_p))
    for i in range(tips, anc_buffers + tips):
        C.cast(an, C.POINTER(C.c_void_p))[i] = libc.calloc(10, 4)
    st.anc_states = C.cast(an, C.POINTER(api.c_uint_p))
    amd_lib.pll_parsimony_destroy(raw)  # under tools/host_asan.sh: no invalid or double free
    amd_lib.pll_parsimony_destroy(None)


def test_device_calls_refuse_a_host_only_structure(amd_lib):
    case = PC.BY_NAME["dna_8x300_tail"]
    ops, edge = PC.traversal(case)
    with _session(amd_lib, case, api.PATTERN_TIP) as s:
        before = [s.vector(n) for n in range(s.nodes)]
        s.update(ops)
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert s.edge_score(*edge) == api.UINT_MAX and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert s.root_score(edge[0]) == api.UINT_MAX and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert amd_lib.pll_gpu_sync_parsimony(s.pars, -1) == 0 and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        pairs = np.array([[0, 1]], dtype=np.uint32)
        out = np.full(1, 0xDEADBEEF, dtype=np.uint32)
        assert amd_lib.pll_gpu_fastparsimony_edge_scores(s.pars, api.uptr(pairs), 1, api.uptr(out)) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert amd_lib.pll_gpu_fastparsimony_insertion_scores(s.pars, 2, api.uptr(pairs), 1, api.uptr(out)) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert out[0] == 0xDEADBEEF and not s.costs().any()
        assert all((s.vector(n) == before[n]).all() for n in range(s.nodes))
    # a structure the library has never seen: PLL_ERROR_PARAM_INVALID
    foreign = api.Parsimony()
    assert amd_lib.pll_fastparsimony_edge_score(C.byref(foreign), 0, 1) == api.UINT_MAX
    assert amd_lib.errno() == api.ERROR_PARAM_INVALID
