"""GPU: pll_gpu_optimize_branch_length - the safeguarded Newton iteration of pllamd.newton run on the device in one
call - against the reference's derivatives, this library's own per-call derivatives, the recipe replayed on the host
and the reference's answer, on the smallest shapes that reach each launch path (newton_cases.py)."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

import newton_cases as NC
from deriv_common import close
from pllamd import api, driver, newton, workload as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=NC.IDS)
def dev(request, amd_lib):
    """one device session per case, the tip edge optimised from every start"""
    cid = request.param
    with NC.prepared(amd_lib, cid) as s:
        edge = NC.tip_edge(cid)
        st = NC.table(s, edge)
        runs = {t0: s.optimize_branch(edge, st, t0, **NC.bounds(cid)) for t0 in NC.T_STARTS}
        launches = amd_lib.pll_gpu_last_launch_count(s.p)
        yield SimpleNamespace(cid=cid, case=NC.make(cid), s=s, edge=edge, st=st, runs=runs, launches=launches)


def replay(trace, t_min, t_max, tolerance, max_iters):
    """the recipe on the host from the device's own (t_i, d_i, dd_i): -> (status, [(next point, was it a Newton step)])"""
    br = newton.Bracket(t_min, t_max)
    nexts = []
    for i, (t, d, dd) in enumerate(trace):
        status, nxt = br.step(t, d, dd, tolerance)
        if status is not None:
            return status, nexts, i + 1
        nexts.append((nxt, br.newton))
    return (newton.MAXITER if len(trace) == max_iters else None), nexts, len(trace)


def assert_follows_recipe(res, trace, t_min, t_max, tolerance, max_iters):
    status, nexts, used = replay([tuple(r) for r in trace], t_min, t_max, tolerance, max_iters)
    assert used == len(trace) == res.iterations and status == res.status, (status, used, res.status, res.iterations)
    for i in range(len(trace) - 1):
        want, is_newton = nexts[i]
        got = trace[i + 1][0]
        if is_newton:  # a division and a subtraction: half an ulp each, doubled in case the division is not correctly rounded
            assert abs(got - want) <= 2 * np.spacing(abs(want)), (i, got, want)
        else:          # lo / hi / 2*t / midpoint: exact
            assert got == want, (i, got, want)
    assert (res.t, res.d_f, res.dd_f) == tuple(trace[-1])
    assert res.host_waits == math.ceil(res.iterations / 8)


def test_rows_are_the_per_call_derivatives_bit_for_bit(dev):
    for t0, (res, trace) in dev.runs.items():
        assert res.iterations == len(trace) >= 1
        for t, d, dd in trace:
            assert dev.s.derivatives(dev.edge, dev.st, t) == (d, dd), (dev.cid, t0, t)


def test_steps_statuses_and_round_trips_follow_the_recipe(dev):
    for t0, (res, trace) in dev.runs.items():
        print(dev.cid, t0, "->", res.t, res.status, res.iterations, res.host_waits)
        assert trace[0][0] == t0
        assert_follows_recipe(res, trace, **NC.bounds(dev.cid))
    # the launches of the last call: one per evaluation enqueued (two with the diag pre-kernel), one publish per batch
    res = dev.runs[NC.T_STARTS[-1]][0]
    per_eval = 2 if dev.case.rate_cats * dev.case.states > 1024 else 1
    assert dev.launches == per_eval * min(8 * res.host_waits, NC.MAX_ITERS) + res.host_waits


def test_derivatives_and_answer_are_the_reference_s(dev, ref_lib):
    with NC.prepared(ref_lib, dev.cid) as r:
        rst = NC.table(r, dev.edge)
        tol = NC.tolerance(dev.cid)
        for t0, (res, trace) in dev.runs.items():
            for t, d, dd in trace:
                e1, e2 = r.derivatives(dev.edge, rst, t)
                print(dev.cid, t0, t, d, e1, dd, e2)
                assert close(d, e1, sites=dev.case.sites) and close(dd, e2, sites=dev.case.sites), (dev.cid, t0, t, d, e1, dd, e2)
            t_ref, status_ref, trace_ref = newton.host_newton(r, dev.edge, rst, t0, **NC.bounds(dev.cid))
            assert res.status == status_ref == newton.CONVERGED
            # both points satisfy |d| < tolerance on a curve whose slope there is dd
            assert abs(res.t - t_ref) <= 2.5 * tol / trace_ref[-1][2], (dev.cid, t0, res.t, t_ref)


def test_inner_edge_ends_at_t_min(dev):
    if not NC.balanced(dev.cid):
        return  # the statement is about case.edges[0] of the balanced trees
    edge = NC.inner_edge(dev.cid)
    st = NC.table(dev.s, edge)
    for t0 in NC.T_STARTS:
        res, trace = dev.s.optimize_branch(edge, st, t0, **NC.bounds(dev.cid))
        assert res.status == newton.AT_MIN and res.t == NC.T_MIN and res.iterations <= 2, (dev.cid, t0, res.status, res.t, res.iterations)
        assert res.host_waits == 1
        assert_follows_recipe(res, trace, **NC.bounds(dev.cid))


def test_max_iters_cuts_the_same_run_short(dev):
    full = dev.runs[5.0][1]
    res, trace = dev.s.optimize_branch(dev.edge, dev.st, 5.0, **NC.bounds(dev.cid, max_iters=3))
    assert res.status == newton.MAXITER and res.iterations == 3 and res.host_waits == 1
    assert trace.tobytes() == full[:3].tobytes()
    assert res.t == full[2][0]
    assert_follows_recipe(res, trace, **NC.bounds(dev.cid, max_iters=3))


def test_same_call_twice_is_identical(dev):
    a, ta = dev.s.optimize_branch(dev.edge, dev.st, 0.1, **NC.bounds(dev.cid))
    b, tb = dev.s.optimize_branch(dev.edge, dev.st, 0.1, **NC.bounds(dev.cid))
    assert bytes(a) == bytes(b) and ta.tobytes() == tb.tobytes()
    assert bytes(a) == bytes(dev.runs[0.1][0]) and ta.tobytes() == dev.runs[0.1][1].tobytes()


# ---- the transition matrix behind the chain ---------------------------------------------------------
def _update_matrix(s, m, t):
    pi = np.zeros(s.case.rate_cats, dtype=np.uint32)
    one = np.array([m], dtype=np.uint32)
    bl = np.array([float(t)])
    assert s.lib.pll_update_prob_matrices(s.p, api.uptr(pi), api.uptr(one), api.dptr(bl), 1)


def _matrices(s):
    c = s.case
    if s.lib.is_amd:
        assert s.lib.pll_gpu_sync_pmatrix(s.p, -1)
    return [api.as_np(s.part.pmatrix[i], c.rate_cats * c.states * s.sp, np.float64).copy() for i in range(c.prob_matrices)]


@pytest.mark.parametrize("cid", ["dna-16x777", "aa-16x200", "codon-8x100"])
def test_matrix_index_leaves_the_matrix_of_the_answer(amd_lib, ref_lib, cid):
    t0 = 5.0
    with NC.prepared(amd_lib, cid) as s, NC.prepared(ref_lib, cid) as r:
        edge = NC.tip_edge(cid)
        m = NC.make(cid).edges[0][4]
        across = edge + (m,)
        st = NC.table(s, edge)
        _update_matrix(s, m, t0)
        lnl_start = s.edge_lnl(across, persite=False)[0]

        # matrix_index = -1: no matrix moves
        before = _matrices(s)
        res_none, _ = s.optimize_branch(edge, st, t0, **NC.bounds(cid))
        assert s.edge_lnl(across, persite=False)[0] == lnl_start
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, _matrices(s)))

        res, _ = s.optimize_branch(edge, st, t0, matrix_index=m, **NC.bounds(cid))
        assert bytes(res) == bytes(res_none) and res.status == newton.CONVERGED
        assert amd_lib.pll_gpu_last_launch_count(s.p) == 8 * res.host_waits + res.host_waits + 1
        lnl_end = s.edge_lnl(across, persite=False)[0]   # with no further call in between
        after = _matrices(s)
        _update_matrix(r, m, res.t)
        exp = _matrices(r)
        assert np.abs(after[m] - exp[m]).max() <= 1e-12, np.abs(after[m] - exp[m]).max()
        assert all(a.tobytes() == b.tobytes() for i, (a, b) in enumerate(zip(before, after)) if i != m)
        lnl_ref = r.edge_lnl(across, persite=False)[0]
        print(cid, "lnL", lnl_start, "->", lnl_end, "reference", lnl_ref)
        assert lnl_end >= lnl_start
        assert abs(lnl_end - lnl_ref) <= 1e-10 * abs(lnl_ref)


# ---- refusals ---------------------------------------------------------------------------------------
def _raw_call(s, st, opt, partition=True, params=True, sumtable=True, options=True, result=True, fi=None):
    """-> (return value, errno, result and trace untouched?)"""
    res = api.NewtonResult(-1.0, -2.0, -3.0, 7, 8, 9)
    before = bytes(res)
    trace = np.full(3 * 64, -5.0)
    fi = np.zeros(s.case.rate_cats, dtype=np.uint32) if fi is None else np.asarray(fi, dtype=np.uint32)
    ok = s.lib.pll_gpu_optimize_branch_length(
        s.p if partition else None, 0, -1, api.uptr(fi) if params else None, api.dptr(st) if sumtable else None,
        C.byref(opt) if options else None, C.byref(res) if result else None, api.dptr(trace))
    return ok, s.lib.errno(), bytes(res) == before and bool((trace == -5.0).all())


def test_refusals_leave_result_and_trace_alone(amd_lib):
    cid = "dna-16x130"
    inf, nan = float("inf"), float("nan")
    with NC.prepared(amd_lib, cid) as s:
        edge = NC.tip_edge(cid)
        st = NC.table(s, edge)
        nmat = s.case.prob_matrices

        def good(**kw):
            d = dict(t_start=0.1, t_min=1e-6, t_max=100.0, tolerance=1e-6, max_iters=64, matrix_index=-1)
            d.update(kw)
            return api.Newton(**d)

        assert _raw_call(s, st, good())[0] == 1
        invalid = [dict(partition=False), dict(params=False), dict(sumtable=False), dict(options=False), dict(result=False),
                   dict(fi=[0, 0, 1, 0])]
        for kw in invalid:
            assert _raw_call(s, st, good(), **kw) == (0, api.ERROR_PARAM_INVALID, True), kw
        for kw in (dict(t_min=-1e-3), dict(t_min=2.0, t_max=1.0), dict(t_min=nan), dict(t_max=nan), dict(t_max=inf),
                   dict(t_min=inf, t_max=inf), dict(t_start=nan), dict(tolerance=0.0), dict(tolerance=-1.0), dict(tolerance=nan),
                   dict(max_iters=0), dict(max_iters=65), dict(matrix_index=nmat), dict(matrix_index=-2)):
            assert _raw_call(s, st, good(**kw)) == (0, api.ERROR_PARAM_INVALID, True), kw
        assert _raw_call(s, st, good(t_min=0.0, t_max=0.0, max_iters=1, matrix_index=nmat - 1))[0] == 1  # the edges of the valid range

        # a recycled handle fails as it does for the per-call path (test_gpu_derivatives.py::test_sumtable_handles)
        more = [NC.table(s, edge) for _ in range(16)]
        ok, errno, untouched = _raw_call(s, st, good())
        assert (ok, errno, untouched) == (0, api.ERROR_GPU_RUNTIME, True) and "recycled" in amd_lib.errmsg()
        assert _raw_call(s, more[-1], good())[0] == 1


def test_lewis_correction_is_unsupported(amd_lib):
    case = W.make_case("lewis", 4, 16, 200, seed=5, asc_type=1, asc_weights=[5, 4, 6, 2])
    eig = W.eigensystem(case.model["exch"], case.freqs[0])
    e = case.edges[0]
    with driver.Session(amd_lib, case, api.ARCH_AVX2) as s:
        s.inject_eigen(eig, case.model["rates"])
        s.update_partials()
        st = NC.table(s, (e[0], e[1], case.tips - 1, -1))
        assert _raw_call(s, st, api.Newton(0.1, 1e-6, 100.0, 1e-6, 64, -1)) == (0, api.ERROR_GPU_UNSUPPORTED, True)
