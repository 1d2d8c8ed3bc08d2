"""CPU (no GPU): the safeguarded Newton recipe of pllamd.newton, driven through the reference library, behaves on the
test cases as tests/test_gpu_newton.py assumes; the new call refuses to run without a device; struct sizes."""
import ctypes as C

import numpy as np
import pytest

import newton_cases as NC
from pllamd import api, driver, newton, workload as W


@pytest.fixture(scope="module", params=NC.IDS)
def ref(request, ref_lib):
    cid = request.param
    with NC.prepared(ref_lib, cid) as s:
        yield cid, s


def test_tip_edge_converges_to_a_stationary_point(ref):
    """5-15 evaluations from every start, and the answer is a stationary point of the reference's own derivative"""
    cid, s = ref
    edge = NC.tip_edge(cid)
    st = NC.table(s, edge)
    for t0 in NC.T_STARTS:
        t, status, trace = newton.host_newton(s, edge, st, t0, **NC.bounds(cid))
        print(cid, t0, "->", t, status, len(trace))
        assert status == newton.CONVERGED, (cid, t0, status, trace)
        assert 5 <= len(trace) <= 15, (cid, t0, len(trace))
        assert NC.T_MIN < t < NC.T_MAX and t == trace[-1][0]
        assert abs(s.derivatives(edge, st, t)[0]) < NC.tolerance(cid)


def test_inner_edge_ends_at_t_min(ref):
    cid, s = ref
    if not NC.balanced(cid):
        return  # the statement is about case.edges[0] of the balanced trees
    edge = NC.inner_edge(cid)
    st = NC.table(s, edge)
    for t0 in NC.T_STARTS:
        t, status, trace = newton.host_newton(s, edge, st, t0, **NC.bounds(cid))
        assert status == newton.AT_MIN and t == NC.T_MIN, (cid, t0, status, t)
        assert len(trace) == (1 if t0 == NC.T_MIN else 2), (cid, t0, trace)


def test_max_iters_reports_the_last_point_evaluated(ref):
    cid, s = ref
    edge = NC.tip_edge(cid)
    st = NC.table(s, edge)
    full = newton.host_newton(s, edge, st, 5.0, **NC.bounds(cid))[2]
    t, status, trace = newton.host_newton(s, edge, st, 5.0, **NC.bounds(cid, max_iters=3))
    assert status == newton.MAXITER and trace == full[:3] and t == full[2][0]


def test_refused_without_a_device(amd_lib, monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")
    case = W.make_case("t", 4, 4, 32)
    with driver.Session(amd_lib, case, api.ARCH_AVX2) as s:
        st = s.new_sumtable()
        opt = api.Newton(0.1, 1e-6, 100.0, 1e-6, 64, -1)
        res = api.NewtonResult(-1.0, -2.0, -3.0, 7, 8, 9)
        before = bytes(res)
        trace = np.full(3 * 64, -5.0)
        fi = np.zeros(case.rate_cats, dtype=np.uint32)
        ok = amd_lib.pll_gpu_optimize_branch_length(s.p, 0, -1, api.uptr(fi), api.dptr(st), C.byref(opt), C.byref(res), api.dptr(trace))
        assert ok == 0 and amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE == 900
        assert bytes(res) == before and (trace == -5.0).all()
        with pytest.raises(RuntimeError, match="900"):
            s.optimize_branch((0, 0, 1, -1), st, 0.1, 1e-6, 100.0, 1e-6)


def test_struct_sizes():
    assert C.sizeof(api.Newton) == 40 and C.sizeof(api.NewtonResult) == 40
