"""CPU (no GPU): pllamd/nj.py, the definition of pll_gpu_nj_tree / pll_gpu_distance_tree, and everything the host layer of
libpll_amd.so decides before a device is needed.

The definition. On additive matrices of random trees whose branch lengths are multiples of 1/64 every operation of NJ is
exact (on a cherry (R_i - R_j) / (2 (r-2)) = (l_i - l_j) / 2), so the tree read back from parent / length reproduces every
input distance EXACTLY, 4 .. 600 nodes; BIONJ's weighted means are evaluated in the form that is exact where both sides
agree, so it keeps the same exact D and R and joins what NJ joins. The tie rule and the four-node rule are checked against
an independent statement of the algorithm in exact rational arithmetic on labels (no slots, no floating point), which also
confirms the joins of the noisy inputs up to 9 nodes.

test_the_inputs_keep_their_gaps is a condition on the inputs of tests/test_gpu_nj.py: at every join of every noisy case the
second-best Q exceeds the best by at least 1e-9 max |Q| (measured: 7.5e-7 at least), the binary64 and long-double
restatements give the same parent, and their lengths differ by at most nj_cases.WORST_RESTATEMENT_DEVIATION (measured:
2.348e-12 at 600 nodes, where distances reach 11.2 and the carried row sums 3000) - the figure the GPU test's bound is 16 x of.
"""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import distance_cases as DC
import nj_cases as NC
from pllamd import api, driver, nj, workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.5


# ---- the algorithm once more: exact rationals, a dict on labels ---------------------------------------------------
def exact_tree(matrix, bionj=False):
    n = len(matrix)
    F = lambda x: Fraction(float(x))
    d = {(x, y): F(matrix[min(x, y)][max(x, y)]) for x in range(n) for y in range(n) if x != y}
    v = dict(d)
    active = list(range(n))
    parent, length = [-1] * (2 * n - 2), [Fraction(0)] * (2 * n - 2)
    step = 0
    while len(active) > 3:
        r = len(active)
        R = {x: sum(d[x, k] for k in active if k != x) for x in active}
        pairs = [(x, y) for x in active for y in active if x < y]
        if r == 4:
            pairs = [p for p in pairs if min(active) in p]
        i, j = min(pairs, key=lambda p: ((r - 2) * d[p] - R[p[0]] - R[p[1]], p[0], p[1]))
        li = d[i, j] / 2 + (R[i] - R[j]) / (2 * (r - 2))
        lj = d[i, j] - li
        u = n + step
        parent[i] = parent[j] = u
        length[i], length[j] = li, lj
        rest = [k for k in active if k not in (i, j)]
        lam = Fraction(1, 2)
        if bionj and v[i, j] != 0:
            lam = min(Fraction(1), max(Fraction(0), lam + sum(v[j, k] - v[i, k] for k in rest) / (2 * (r - 2) * v[i, j])))
        for k in rest:
            if bionj:
                d[u, k] = d[k, u] = lam * (d[i, k] - li) + (1 - lam) * (d[j, k] - lj)
                v[u, k] = v[k, u] = lam * v[i, k] + (1 - lam) * v[j, k] - lam * (1 - lam) * v[i, j]
            else:
                d[u, k] = d[k, u] = (d[i, k] + d[j, k] - d[i, j]) / 2
        active = rest + [u]
        step += 1
    a, b, c = active
    root = 2 * n - 3
    for x, y, z in ((a, b, c), (b, a, c), (c, a, b)):
        parent[x], length[x] = root, (d[x, y] + d[x, z] - d[y, z]) / 2
    return parent, length


SMALL = (3, 4, 5, 8, 9)


@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_the_definition_against_exact_arithmetic(flag):
    """ties (all ones, the balanced tree), the four-node rule (every run passes through it; at 4 nodes it is all there is) and
    ordinary joins: the same parent as the rational statement, lengths within 1e-13"""
    cases = [("ones", n) for n in SMALL + (6, 12)] + [("balanced", 1), ("balanced", 2)]
    cases += [("additive", n) for n in SMALL] + [("noisy", n) for n in SMALL]
    for kind, n in cases:
        m = NC.MATRICES[kind](n)
        parent, length = nj.nj_tree(m, NC.FLAGS[flag])
        ep, el = exact_tree(m, flag == "bionj")
        assert list(parent) == ep, (kind, n, list(parent), ep)
        assert max(abs(float(x) - float(y)) for x, y in zip(length, el)) <= 1e-13, (kind, n)


def test_the_tie_rule_on_labels():
    """all ones, six nodes: (0,1) first; then (2,3): the first pair among those of minimal Q; then four nodes remain - 4, 5,
    6, 7 - and only the pairs of node 4 are searched"""
    parent, length = nj.nj_tree(NC.ones(6))
    assert list(parent) == [6, 6, 7, 7, 8, 8, 9, 9, 9, -1]
    assert list(length) == [0.5] * 6 + [0.0] * 4
    # a permutation of the input permutes the labels of a tie-free tree and nothing else: the rule is on labels, not slots
    m = NC.noisy(9)
    perm = np.array([4, 7, 0, 8, 2, 6, 1, 3, 5])
    _, length_p = nj.nj_tree(m[np.ix_(perm, perm)])
    _, length_0 = nj.nj_tree(m)
    assert np.abs(length_p[:9] - length_0[perm]).max() <= 1e-14


def test_the_balanced_tree_is_joined_cherry_by_cherry():
    for levels in NC.BALANCED_LEVELS:
        m = NC.balanced(levels)
        n = len(m)
        parent, length = NC.expected("balanced", levels, "nj")
        assert [int(parent[2 * c]) for c in range(n // 2)] == [int(parent[2 * c + 1]) for c in range(n // 2)] == list(range(n, n + n // 2))
        assert np.array_equal(nj.tree_distances(parent, length), m)


def test_the_four_node_rule():
    """Q_ab = Q_cd for every split of four nodes: whichever split the matrix holds, the pair that contains node 0 is joined"""
    for partner in (1, 2, 3):
        others = [x for x in (1, 2, 3) if x != partner]
        m = np.zeros((4, 4))
        for x in range(4):
            for y in range(4):
                if x != y:
                    m[x, y] = 0.25 if {x, y} in ({0, partner}, set(others)) else 0.75
        parent, length = nj.nj_tree(m)
        assert parent[0] == parent[partner] == 4 and parent[others[0]] == parent[others[1]] == parent[4] == 5
        assert np.array_equal(nj.tree_distances(parent, length), m)


@pytest.mark.parametrize("n", [c for c in NC.COUNTS if c >= 4])
def test_additive_matrices_are_reproduced_exactly(n):
    m = NC.additive(n)
    parent, length = NC.expected("additive", n, "nj")
    assert parent[-1] == -1 and length[-1] == 0 and (parent[:-1] >= n).all() and (parent[:-1] > np.arange(2 * n - 3)).all()
    assert np.array_equal(nj.tree_distances(parent, length), m)
    parent_b, length_b = NC.expected("additive", n, "bionj")
    assert np.array_equal(parent_b, parent)
    assert np.array_equal(nj.tree_distances(parent_b, length_b), m)


def test_only_the_upper_triangle_is_read():
    m = NC.noisy(9).copy()
    expect = nj.nj_tree(m, nj.BIONJ)
    m[np.tril_indices(9)] = np.nan
    got = nj.nj_tree(m, nj.BIONJ)
    assert np.array_equal(got[0], expect[0]) and got[1].tobytes() == expect[1].tobytes()


def test_the_inputs_keep_their_gaps():
    worst, least = 0.0, 1.0
    for n in NC.COUNTS:
        for flag in NC.FLAGS:
            trace = []
            parent, length = nj.nj_tree(NC.noisy(n), NC.FLAGS[flag], trace=trace)
            assert np.array_equal(parent, NC.expected("noisy", n, flag)[0]) and length.tobytes() == NC.expected("noisy", n, flag)[1].tobytes()
            parent_l, length_l = NC.expected("noisy", n, flag, True)
            assert length_l.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18  # a second opinion, not a second copy
            assert np.array_equal(parent, parent_l), (n, flag)
            assert len(trace) == n - 3
            for best, second, largest in trace:
                assert second is not None and second - best >= NC.LEAST_GAP * largest, (n, flag, best, second, largest)
                least = min(least, float((second - best) / largest))
            worst = max(worst, float(np.abs(length - length_l).max()))
    print(f"least gap {least:.3g} of max |Q|; worst |binary64 - long double| length {worst:.4g}")
    assert worst <= NC.WORST_RESTATEMENT_DEVIATION


def test_the_launch_rule():
    assert [nj.launch_count(n) for n in (3, 4, 5, 600)] == [1, 4, 6, 1196]
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert "2 (count - 3) + 2" in dev and re.search(r"#define PLLGPU_NJ_ROWS \d+u", dev)


def test_the_row_runs_stride_the_partial_loop():
    """conditions on nj_cases.ROW_RUNS (tests/test_gpu_nj.py): the last arrival reduces the partials with 256 threads, so the
    runs must hold a step with more than 512 search workgroups, one in (256, 512] and one in (64, 256] - and the default of
    8 rows never leaves the first stride at these sizes, nor do the nine nodes over two rows"""
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert "#define PLLGPU_NJ_ROWS 8u" in dev
    assert max(NC.search_workgroups(600, 8)) == 75 and max(NC.search_workgroups(9, 2)) == 4
    assert NC.search_workgroups(9, 2) == [4, 4, 3, 3, 2, 2] and NC.search_workgroups(5, 1) == [4, 3]
    for rows, runs in NC.ROW_RUNS.items():
        counts = set()
        for kind, n, flag in runs:
            assert flag in NC.FLAGS
            nodes = len(NC.MATRICES[kind](n))
            counts |= set(NC.search_workgroups(nodes, rows))
        if rows == 1:
            assert max(counts) == 599
            assert any(c > 512 for c in counts) and any(256 < c <= 512 for c in counts) and any(64 < c <= 256 for c in counts)
        else:
            # a last workgroup with fewer rows than the others, past one stride of the partial loop or not
            assert any((r - 1) % rows for kind, n, flag in runs for r in range(4, n + 1))
            assert max(counts) == 200 and 86 in counts
    assert len(NC.balanced(6)) == 192


# ---- the host layer of libpll_amd.so ---------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    assert re.search(r"\bint pll_gpu_nj_tree\(", hdr) and re.search(r"\bint pll_gpu_distance_tree\(", hdr)
    assert re.search(r"#define PLL_GPU_NJ_BIONJ 1u", hdr) and api.NJ_BIONJ == nj.BIONJ == 1
    assert "the NJ tree itself" not in hdr
    assert len(amd_lib.pll_gpu_nj_tree.argtypes) == 6 and len(amd_lib.pll_gpu_distance_tree.argtypes) == 9
    assert amd_lib.pll_gpu_nj_last_launch_count.restype is C.c_uint and amd_lib.pll_gpu_nj_last_device_ms.restype is C.c_double
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    for name in ("pllgpu_nj_tree", "pllgpu_distance_tree", "pllgpu_nj_last_launch_count"):
        assert re.search(r"\b%s\(" % name, dev) and getattr(amd_lib.dll, name)


def _nj_refused(lib, matrix, flags=0, code=api.ERROR_PARAM_INVALID):
    with pytest.raises(RuntimeError) as err:
        driver.nj_tree(lib, matrix, flags, fill=SENTINEL)
    assert lib.errno() == code, (lib.errno(), lib.errmsg())
    assert (err.value.outputs["parent"] == int(SENTINEL)).all() and (err.value.outputs["length"] == SENTINEL).all()
    return str(err.value)


@pytest.mark.parametrize("which", ["distances", "parent", "length"])
def test_nj_tree_each_null_argument(amd_lib, capfd, which):
    d = np.ascontiguousarray(NC.noisy(5))
    parent, length = np.full(8, 77, dtype=np.int32), np.full(8, SENTINEL)
    args = {"distances": api.dptr(d), "parent": parent.ctypes.data_as(C.POINTER(C.c_int)), "length": api.dptr(length)}
    args[which] = None
    assert amd_lib.pll_gpu_nj_tree(args["distances"], 5, 0, -1, args["parent"], args["length"]) == 0
    assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
    assert (parent == 77).all() and (length == SENTINEL).all()
    assert "pll_gpu_nj_tree" in capfd.readouterr().err  # the usual line on stderr


def test_nj_tree_refuses_fewer_than_three_nodes_and_unknown_flags(amd_lib):
    for n in (1, 2):
        assert "at least 3" in _nj_refused(amd_lib, np.zeros((n, n)))
    d, parent, length = np.zeros(1), np.full(1, 77, dtype=np.int32), np.full(1, SENTINEL)
    assert amd_lib.pll_gpu_nj_tree(api.dptr(d), 0, 0, -1, parent.ctypes.data_as(C.POINTER(C.c_int)), api.dptr(length)) == 0
    assert amd_lib.errno() == api.ERROR_PARAM_INVALID and parent[0] == 77 and length[0] == SENTINEL
    assert "flag" in _nj_refused(amd_lib, NC.noisy(5), flags=2)
    assert "flag" in _nj_refused(amd_lib, NC.noisy(5), flags=0x80000001)


@pytest.mark.parametrize("value", [-1e-300, -1.0, float("nan"), float("inf"), -float("inf")])
def test_nj_tree_refuses_an_entry_that_is_negative_or_not_finite(amd_lib, value):
    for x, y in ((0, 1), (2, 8), (7, 8)):
        m = NC.noisy(9).copy()
        m[x, y] = value
        assert f"[{x}][{y}]" in _nj_refused(amd_lib, m)


def test_nj_tree_ignores_the_lower_triangle_and_the_diagonal_in_its_checks(amd_lib):
    """only [x][y], x < y, is read: what stands elsewhere cannot be refused - the call gets as far as the device"""
    m = NC.noisy(5).copy()
    m[np.tril_indices(5)] = np.nan
    if not amd_lib.pll_gpu_available():
        _nj_refused(amd_lib, m, code=api.ERROR_GPU_UNAVAILABLE)
    else:
        parent, length = driver.nj_tree(amd_lib, m)
        assert np.array_equal(parent, NC.expected("noisy", 5, "nj")[0])


def test_the_order_of_nj_tree_checks(amd_lib):
    m = NC.noisy(5).copy()
    m[0, 1] = -1.0
    assert "at least 3" in _nj_refused(amd_lib, m[:2, :2], flags=6)  # count before flags
    assert "flag" in _nj_refused(amd_lib, m, flags=6)                # flags before the entries


SEQ = [b"ACGTACGTACGTACGTACGT", b"ACGTACGAACGTRCGTACGT", b"ACGTTCGTAC-TACGTACGT", b"ACCTACGTACGTACGTANGT", b"ACGTACGTACGTACGTACGA"]
GOOD = dict(t_start=0.1, t_min=1e-6, t_max=100.0, tolerance=1e-6, max_iters=32, matrix_index=-1)


def _tips(lib, attrs=0, **kw):
    return DC.Tips(lib, 4, 4, SEQ, W.map_nt(), W.GTR_DNA["exch"], W.GTR_DNA["freqs"], attrs=attrs, **kw)


def _tree_refused(lib, code, tips=(0, 1, 2, 3, 4), flags=0, options=None, **kw):
    with _tips(lib, **kw) as b:
        with pytest.raises(RuntimeError) as err:
            driver.distance_tree(lib, b.p, tips, b.pi, driver.newton_options(**dict(GOOD, **(options or {}))), flags, fill=SENTINEL)
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        out = err.value.outputs
        assert (out["parent"] == int(SENTINEL)).all() and (out["length"] == SENTINEL).all() and (out["distances"] == SENTINEL).all()
        return str(err.value)


def test_distance_tree_checks_on_a_host_only_partition(amd_lib, monkeypatch):
    """the checks of pll_gpu_pairwise_distances in their order, then count and flags, with a host-only partition behind them"""
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")
    inv, uns = api.ERROR_PARAM_INVALID, api.ERROR_GPU_UNSUPPORTED
    assert "is no tip" in _tree_refused(amd_lib, inv, tips=(0, 5, 2), flags=2)
    assert "options" in _tree_refused(amd_lib, inv, options=dict(tolerance=0.0), flags=2)
    assert "matrix_index" in _tree_refused(amd_lib, inv, options=dict(matrix_index=0))
    assert "not given by codes" in _tree_refused(amd_lib, inv, dense=(1,), tips=(0, 1))
    assert "prop_invar" in _tree_refused(amd_lib, uns, prop_invar=0.2, flags=2)
    _tree_refused(amd_lib, uns, attrs=api.SITE_REPEATS, tips=(0, 1))
    # every check of the distances passes (a host-only partition has no device): the missing device is reported
    _tree_refused(amd_lib, api.ERROR_GPU_UNAVAILABLE)
    _tree_refused(amd_lib, api.ERROR_GPU_UNAVAILABLE, flags=api.NJ_BIONJ)
    for tips in ((), (0,), (0, 1)):
        if tips:
            _tree_refused(amd_lib, api.ERROR_GPU_UNAVAILABLE, tips=tips)
        else:
            assert "at least 3" in _tree_refused(amd_lib, inv, tips=tips)


@pytest.mark.parametrize("which", ["partition", "parent", "length", "tips", "params_indices", "options"])
def test_distance_tree_each_null_argument(amd_lib, monkeypatch, which):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")
    with _tips(amd_lib) as b:
        tips = np.arange(5, dtype=np.uint32)
        parent, length = np.full(8, 77, dtype=np.int32), np.full(8, SENTINEL)
        opt = driver.newton_options(**GOOD)
        args = {"partition": b.p, "tips": api.uptr(tips), "params_indices": api.uptr(b.pi), "options": C.byref(opt),
                "parent": parent.ctypes.data_as(C.POINTER(C.c_int)), "length": api.dptr(length)}
        args[which] = None
        assert amd_lib.pll_gpu_distance_tree(args["partition"], args["tips"], 5, args["params_indices"], args["options"], 0, args["parent"],
                                             args["length"], None) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
        assert (parent == 77).all() and (length == SENTINEL).all()
