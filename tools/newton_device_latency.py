"""Latency of one branch-length optimisation, on the shapes of tools/newton_latency.py: (a) the recipe of pllamd.newton
driven through the per-call API (one pll_compute_likelihood_derivatives per step, each a launch, a poll and a step on
the host) against (b) pll_gpu_optimize_branch_length (the iteration on the device, one poll per batch of evaluations).
Both start at t = 5.0 on the same table and must do the same number of evaluations. Alternating rounds; per shape the
median over the rounds and their spread go to profiles/newton_on_device.json. With --batches the new call is also
timed at other batch sizes (PLL_AMD_NEWTON_BATCH, read when a partition is created)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libpll-2_amd"))
from pllamd import api, driver, newton, workload as W  # noqa: E402

SHAPES = ((4, 1000), (4, 100000), (20, 10000), (61, 2000))
T_START, T_MIN, T_MAX = 5.0, 1e-6, 100.0


def open_session(lib, states, sites):
    case = W.make_case("nr", states, 16, sites, seed=2)
    e = case.edges[0]
    edge = (e[0], e[1], case.tips - 1, -1)  # a tip edge: an interior optimum
    s = driver.Session(lib, case, api.ARCH_AVX2)
    s.inject_eigen(W.eigensystem(case.model["exch"], case.freqs[0]), case.model["rates"])
    s.update_partials()
    st = s.new_sumtable()
    s.update_sumtable(edge, st)
    return s, edge, st, dict(t_min=T_MIN, t_max=T_MAX, tolerance=1e-8 * sites, max_iters=api.NEWTON_MAX_ITERS)


def time_calls(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e6 * (time.perf_counter() - t0) / reps


def summary(us):
    return dict(median_us=round(statistics.median(us), 2), min_us=round(min(us), 2), max_us=round(max(us), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="*", default=[4, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_on_device.json"))
    a = ap.parse_args()
    lib = api.PllLib()
    if not lib.pll_gpu_available():
        raise SystemExit("no MI355X visible: nothing to measure")
    rows = []
    for states, sites in SHAPES:
        os.environ.pop("PLL_AMD_NEWTON_BATCH", None)
        s, edge, st, kw = open_session(lib, states, sites)
        others = {}
        for b in a.batches:
            os.environ["PLL_AMD_NEWTON_BATCH"] = str(b)
            others[b] = open_session(lib, states, sites)
        os.environ.pop("PLL_AMD_NEWTON_BATCH", None)

        def per_call():
            return newton.host_newton(s, edge, st, T_START, **kw)

        def on_device(sess=s, e=edge, tab=st):
            return sess.optimize_branch(e, tab, T_START, **kw)

        t_a, status_a, trace_a = per_call()
        res, trace_b = on_device()
        launches = lib.pll_gpu_last_launch_count(s.p)
        assert status_a == res.status == newton.CONVERGED and len(trace_a) == res.iterations, (status_a, res.status, len(trace_a), res.iterations)
        for _ in range(20):  # warm-up of both
            per_call()
            on_device()
        us_a, us_b = [], []
        us_other = {b: [] for b in others}
        for _ in range(a.rounds):
            us_a.append(time_calls(per_call, a.reps))
            us_b.append(time_calls(on_device, a.reps))
            for b, (so, eo, sto, _) in others.items():
                us_other[b].append(time_calls(lambda: on_device(so, eo, sto), a.reps))
        row = dict(states=states, sites=sites, t_start=T_START, t=res.t, evaluations=res.iterations, launches=launches,
                   host_waits=res.host_waits, batch=8, per_call=summary(us_a), on_device=summary(us_b),
                   ratio=round(statistics.median(us_a) / statistics.median(us_b), 2),
                   per_call_spread_us=round(max(us_a) - min(us_a), 2),
                   faster_by_more_than_the_spread=bool(statistics.median(us_a) - statistics.median(us_b) > max(us_a) - min(us_a)))
        for b, (so, eo, sto, _) in others.items():
            r2, _ = on_device(so, eo, sto)
            assert r2.iterations == res.iterations and r2.t == res.t
            row[f"on_device_batch_{b}"] = dict(summary(us_other[b]), host_waits=r2.host_waits, launches=lib.pll_gpu_last_launch_count(so.p))
            so.close()
        s.close()
        rows.append(row)
        print(json.dumps(row))
    with open(a.out, "w") as f:
        json.dump(dict(tool="tools/newton_device_latency.py", rounds=a.rounds, reps_per_round=a.reps,
                       note="host wall time per optimisation through ctypes; every call is synchronous", shapes=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
