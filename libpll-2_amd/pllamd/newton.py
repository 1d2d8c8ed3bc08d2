"""The safeguarded Newton iteration for one branch length, on the host: the executable statement of the recipe that
pll_gpu_optimize_branch_length (include/pll_amd.h) runs on the device. It evaluates the derivatives through
Session.derivatives - one pll_compute_likelihood_derivatives per step - so it drives any library with the libpll ABI.

d / dd are d_f / dd_f, the derivatives of -lnL. A bracket [lo, hi] with d < 0 at lo and d > 0 at hi closes in as points
are evaluated; an end that has not been evaluated yet is "open" (it is t_min or t_max itself). A Newton step that
leaves the bracket goes to the open end it crossed, or bisects once that end is closed.
"""
from . import api

CONVERGED, AT_MIN, AT_MAX, STALLED, MAXITER = (api.NEWTON_CONVERGED, api.NEWTON_AT_MIN, api.NEWTON_AT_MAX,
                                                  api.NEWTON_STALLED, api.NEWTON_MAXITER)


class Bracket:
    """what the iteration carries from one evaluation to the next, besides t"""

    def __init__(self, t_min, t_max):
        self.t_min, self.t_max = t_min, t_max
        self.lo, self.hi = t_min, t_max
        self.lo_open = self.hi_open = True

    def step(self, t, d, dd, tolerance):
        """after the evaluation (d, dd) at t: (terminal status or None, the next point; t itself with a status)"""
        if abs(d) < tolerance:
            return CONVERGED, t
        if d > 0:
            if t == self.t_min:
                return AT_MIN, t
            self.hi, self.hi_open = t, False
        else:
            if t == self.t_max:
                return AT_MAX, t
            self.lo, self.lo_open = t, False
        lo, hi = self.lo, self.hi
        self.newton = dd > 0                     # (for tests: which branch produced the candidate)
        cand = t - d / dd if dd > 0 else (lo if d > 0 else 2 * t)
        if not cand > lo:                        # also a NaN
            cand = lo if self.lo_open else 0.5 * (lo + hi)
            self.newton = False
        elif not cand < hi:
            cand = hi if self.hi_open else 0.5 * (lo + hi)
            self.newton = False
        if cand == t:
            return STALLED, t
        return None, cand


def host_newton(session, edge, sumtable, t_start, t_min, t_max, tolerance, max_iters):
    """-> (t, status, trace): trace = the evaluations as (t, d_f, dd_f); t = the last point evaluated"""
    t = min(max(float(t_start), float(t_min)), float(t_max))
    br = Bracket(float(t_min), float(t_max))
    trace = []
    for _ in range(max_iters):
        d, dd = session.derivatives(edge, sumtable, t)
        trace.append((t, d, dd))
        status, nxt = br.step(t, d, dd, tolerance)
        if status is not None:
            return t, status, trace
        t = nxt
    return trace[-1][0], MAXITER, trace
