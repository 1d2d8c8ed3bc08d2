"""What the gradient of -lnL with respect to the substitution parameters and the frequencies costs: (a) ONE
pll_gpu_subst_gradient call over all 125 edges of the seeded 64-taxon tree (and pll_gpu_qmatrix_gradient alone, its device
part), (b) pll_gpu_branch_derivatives on the same list in the same process - the same bytes read, the floor - and (c) what
the library offers without it: central differences, 2 x (free parameters) evaluations of the log-likelihood, each
pll_set_subst_params + pll_update_eigen + pll_update_prob_matrices of all 125 branches + the full traversal +
pll_compute_edge_loglikelihood - profiles/qmatrix_gradient.json.

Shapes: those of profiles/rate_gradient.json - 64 taxa x 100k sites, DNA (4 states x 4 rates, 5 free exchangeabilities), and
64 taxa x 20k sites, 20 states x 4 rates (189). OUTSIDE the timed regions: the rooted full traversal and the "upward" CLVs of
every edge (tests/gradient_cases.py), and a one-row call that launches what they hold back. Timed: (a) and (b) with device
events on the partition's stream (pll_gpu_timer_start / _stop around the synchronous call: launches and the copy back) and
with the host clock, alternating within a repetition; (c) ONE evaluation with the host clock (its eigen-decomposition is
host work), multiplied by 2 x (free parameters). The achieved rates divide stage 1's reads and arithmetic by the device time
of the whole pll_gpu_qmatrix_gradient call (stage 2 and the copy back included: a lower bound for the kernel):
bytes = both ends of every branch (8 S R per site of a CLV end, 1 per site of a code end), matrix-pipe FLOPs = 2 P^2 R per
site and branch (P = states padded to 16; the 4 x 4 form has none), all fp64 FLOPs = that (unpadded for 4 x 4) plus the two
contractions, 2 S^2 R per site and CLV end. Checked, not timed: sum_xy d_q Q = d_scale of pll_gpu_rate_gradient to 1e-9
relative. Nothing is asserted on time.

Usage: python tools/qmatrix_gradient_probe.py [--out profiles/qmatrix_gradient.json] [--reps 10] [--shapes dna,aa] [--no-json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "libpll-2_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import gradient_cases as GC  # noqa: E402
import insertion_cases as IC  # noqa: E402
import qmatrix_gradient_cases as QC  # noqa: E402
from pllamd import api, driver  # noqa: E402

SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000), "aa": dict(states=20, rate_cats=4, taxa=64, sites=20000)}
PEAK = dict(hbm_bytes_per_s=8.0e12, fp64_matrix_flops=78.6e12)  # the MI355X figures README.md and DESIGN.md section 5 quote


def run_shape(lib, name, reps):
    sh = SHAPES[name]
    S, R, sites = sh["states"], sh["rate_cats"], sh["sites"]
    lay, seqs, cmap, exch, freqs = IC.make(S, sh["taxa"], sites, R)
    with IC.Bed(lib, lay, S, sites, R, 0, seqs, cmap, exch, freqs) as b:
        branches = list(lay.tree.branches())
        root = lay.end(lay.root) + lay.end(lay.root.back) + (lay.root.pm,)
        full_ops = lay.full_ops()
        subst = np.ascontiguousarray(exch, dtype=np.float64)

        def lnl_at(params):
            """set params + the eigensystem + all P matrices + full traversal + edge log-likelihood"""
            lib.pll_set_subst_params(b.p, 0, api.dptr(np.ascontiguousarray(params)))
            assert lib.pll_update_eigen(b.p, 0)
            b.matrices(branches)
            b.update(full_ops)
            return b.lnl(root)

        rows = GC.prepare(b)
        n = len(rows)
        assert n == 2 * sh["taxa"] - 3
        pi, arr = api.uptr(b.fi), api.make_branches(rows)
        old = np.empty((2, n))
        M = 1
        d_q, d_root = np.empty((M, S, S)), np.empty((M, S))
        d_subst, d_freqs = np.empty((M, S * (S - 1) // 2)), np.empty((M, S))
        calls = {
            "branch_derivatives": lambda: lib.pll_gpu_branch_derivatives(b.p, arr, n, pi, api.dptr(old[0]), api.dptr(old[1])),
            "qmatrix_gradient": lambda: lib.pll_gpu_qmatrix_gradient(b.p, arr, n, pi, api.dptr(d_q), api.dptr(d_root)),
            "subst_gradient": lambda: lib.pll_gpu_subst_gradient(b.p, arr, n, pi, api.dptr(d_subst), api.dptr(d_freqs)),
        }
        names = list(calls)
        dev = {k: [] for k in names}
        host = {k: [] for k in names}
        t_eval, launches = [], 0
        for rep in range(reps + 2):  # two warm-up rounds
            assert GC.prepare(b) == rows
            assert lib.pll_gpu_branch_derivatives(b.p, arr, 1, pi, api.dptr(old[0]), None), (lib.errno(), lib.errmsg())
            for k in names[rep % 3:] + names[:rep % 3]:  # which call goes first rotates
                s0 = time.perf_counter()
                assert lib.pll_gpu_timer_start(b.p)
                ok = calls[k]()
                ms = lib.pll_gpu_timer_stop(b.p)
                s1 = time.perf_counter()
                assert ok, (k, lib.errno(), lib.errmsg())
                if k == "qmatrix_gradient":
                    launches = int(lib.pll_gpu_last_launch_count(b.p))
                if rep >= 2:
                    dev[k].append(ms * 1e3)
                    host[k].append((s1 - s0) * 1e6)
            e = np.zeros(len(subst))
            e[0] = 2.0 ** -10 * subst[0]
            t0 = time.perf_counter()
            lnl_at(subst + e)
            t1 = time.perf_counter()
            lnl_at(subst)
            b.matrices(lay.branches())
            if rep >= 2:
                t_eval.append((t1 - t0) * 1e6)
        q_model = QC.q_matrix(subst, np.asarray(freqs, dtype=np.float64) / np.sum(freqs))
        d_scale = driver.rate_gradient(lib, b.p, rows, b.fi, want_rates=False, want_cat=False, want_d=False)["d_scale"]
    euler = float(np.sum(d_q[0] * q_model))
    assert abs(euler - d_scale) <= 1e-9 * abs(d_scale), (euler, d_scale)
    tips = lay.tips
    clv_ends = sum((r[0] >= tips) + (r[2] >= tips) for r in rows)
    code_ends = 2 * n - clv_ends
    pad = (S + 15) // 16 * 16
    bytes_read = float(clv_ends) * sites * R * S * 8 + float(code_ends) * sites
    matrix_flops = 0.0 if (S, R) == (4, 4) else 2.0 * pad * pad * R * sites * n
    outer_flops = matrix_flops if matrix_flops else 2.0 * S * S * R * sites * n
    all_flops = outer_flops + 2.0 * S * S * R * sites * clv_ends
    med = statistics.median
    t = med(dev["qmatrix_gradient"]) * 1e-6
    q = lambda x: dict(median=round(med(x), 2), min=round(min(x), 2), max=round(max(x), 2))
    free = S * (S - 1) // 2 - 1
    fd = 2 * free * med(t_eval)
    res = dict(shape=sh, branches=n, launches=launches, workgroups_per_branch=QC.blocks_by_rule(S, R, sites),
               device_us={k: q(v) for k, v in dev.items()}, host_us={k: q(v) for k, v in host.items()},
               one_evaluation_us=q(t_eval), free_parameters=free, likelihood_evaluations=2 * free, finite_differences_us=round(fd, 1),
               subst_gradient_over_branch_derivatives=round(med(host["subst_gradient"]) / med(host["branch_derivatives"]), 3),
               finite_differences_over_subst_gradient=round(fd / med(host["subst_gradient"]), 1),
               stage1=dict(bytes_read=bytes_read, fp64_flops=all_flops, matrix_pipe_flops=matrix_flops,
                           achieved_bytes_per_s=float(f"{bytes_read / t:.4g}"), achieved_fp64_flops=float(f"{all_flops / t:.4g}"),
                           achieved_matrix_pipe_flops=float(f"{matrix_flops / t:.4g}"),
                           fraction_of_hbm=round(bytes_read / t / PEAK["hbm_bytes_per_s"], 3),
                           fraction_of_matrix_pipe=round(matrix_flops / t / PEAK["fp64_matrix_flops"], 4)))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qmatrix_gradient.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="dna,aa")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps, "peaks": PEAK,
           "clock": "device events on the partition's stream and the host clock around the synchronous calls, rotating; medians, min, max in us"}
    for name in a.shapes.split(","):
        res[name] = run_shape(lib, name, a.reps)
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
