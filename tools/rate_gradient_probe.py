"""What the gradient of -lnL with respect to the category rates and the branch-length multiplier costs: ONE
pll_gpu_rate_gradient call with every output over all 125 edges of the seeded 64-taxon tree, (a) against
pll_gpu_branch_derivatives on the same list in the same process - the same bytes read, R more sums kept - and (b) against
what the library offers without it for the same rate_cats numbers: 2 * rate_cats evaluations of the log-likelihood (central
differences), each pll_set_category_rates + pll_update_prob_matrices of all 125 branches + the full traversal +
pll_compute_edge_loglikelihood - profiles/rate_gradient.json.

Shapes: 64 taxa x 100k sites, DNA (4 states x 4 rates), and 64 taxa x 20k sites, 20 states x 4 rates; the tree and the
alignment come from seeds (tests/insertion_cases.py), nothing is read from disk. OUTSIDE the timed regions of (a): the
rooted full traversal and the "upward" CLVs of every edge into spare slots (tests/gradient_cases.py); they are timed on their
own, together with a synchronous one-row call that launches what they hold back (`prepare_us`: what a caller adds to the one
call when its CLVs are not oriented yet). Timed, host clock around the
synchronous calls, the variants alternating within a repetition, `--reps` repetitions after two warm-up rounds. The
finite-difference loop leaves the rates as they were and the traversal is run again before the next repetition. Checked, not
timed: d_f of the new call equals pll_gpu_branch_derivatives' bit for bit; sum_k r_k d_rates[k] equals d_scale to 1e-10
relative. Reported, not asserted: the largest relative difference between -d_rates and the central differences (step
2^-10 r_k) of the log-likelihoods of the same library. Nothing is asserted on time.

Usage: python tools/rate_gradient_probe.py [--out profiles/rate_gradient.json] [--reps 20] [--shapes dna,aa] [--no-json]"""
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
from pllamd import api, workload as W  # noqa: E402

SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000), "aa": dict(states=20, rate_cats=4, taxa=64, sites=20000)}


def run_shape(lib, name, reps):
    sh = SHAPES[name]
    R = sh["rate_cats"]
    lay, seqs, cmap, exch, freqs = IC.make(sh["states"], sh["taxa"], sh["sites"], R)
    with IC.Bed(lib, lay, sh["states"], sh["sites"], R, 0, seqs, cmap, exch, freqs) as b:
        rates = np.ascontiguousarray(W.gamma_rates_mean(0.7, R), dtype=np.float64)
        branches = list(lay.tree.branches())
        root = lay.end(lay.root) + lay.end(lay.root.back) + (lay.root.pm,)
        full_ops = lay.full_ops()

        def lnl_at(r):
            """set rates + all P matrices + full traversal + edge log-likelihood"""
            lib.pll_set_category_rates(b.p, api.dptr(np.ascontiguousarray(r)))
            b.matrices(branches)
            b.update(full_ops)
            return b.lnl(root)

        rows = GC.prepare(b)
        assert len(rows) == 2 * sh["taxa"] - 3
        pi, arr, n = api.uptr(b.fi), api.make_branches(rows), len(rows)
        old = np.empty((2, n))
        d_rates, d_scale, d_cat, d_f = np.empty(R), np.empty(1), np.empty((n, R)), np.empty(n)
        fd = np.empty(R)
        t_old, t_new, t_fd, t_prep, launches = [], [], [], [], (0, 0)
        for rep in range(reps + 2):  # two warm-up rounds
            t0 = time.perf_counter()
            rows_again = GC.prepare(b)
            # what the traversal holds back is launched by the next call that reads CLVs: by this synchronous one-row call,
            # inside `prepare_us` and outside the clocks of (a)
            assert lib.pll_gpu_branch_derivatives(b.p, arr, 1, pi, api.dptr(old[0]), None), (lib.errno(), lib.errmsg())
            t1 = time.perf_counter()
            assert rows_again == rows
            order = (0, 1) if rep % 2 == 0 else (1, 0)  # which of the two calls of (a) goes first alternates
            span = [0.0, 0.0]
            for which in order:
                s0 = time.perf_counter()
                if which == 0:
                    ok = lib.pll_gpu_branch_derivatives(b.p, arr, n, pi, api.dptr(old[0]), api.dptr(old[1]))
                else:
                    ok = lib.pll_gpu_rate_gradient(b.p, arr, n, pi, api.dptr(d_rates), api.dptr(d_scale), api.dptr(d_cat), api.dptr(d_f))
                span[which] = time.perf_counter() - s0
                assert ok, (lib.errno(), lib.errmsg())
                if which == 1:
                    launches = int(lib.pll_gpu_last_launch_count(b.p))
            t2 = time.perf_counter()
            for k in range(R):
                h = 2.0 ** -10 * rates[k]
                e = np.zeros(R)
                e[k] = h
                fd[k] = (lnl_at(rates + e) - lnl_at(rates - e)) / (2.0 * h)
            t3 = time.perf_counter()
            lib.pll_set_category_rates(b.p, api.dptr(rates))
            b.matrices(lay.branches())
            if rep >= 2:
                t_prep.append((t1 - t0) * 1e6)
                t_old.append(span[0] * 1e6)
                t_new.append(span[1] * 1e6)
                t_fd.append((t3 - t2) * 1e6)
    assert d_f.tobytes() == old[0].tobytes(), "d_f differs from pll_gpu_branch_derivatives"
    # sum_k r_k d_rates[k] = sum_i t_i sum_k d_cat[i][k] = d_scale up to rounding: the contraction against itself
    identity = abs(float(np.dot(rates, d_rates)) - d_scale[0]) / abs(d_scale[0])
    assert identity < 1e-10, (d_rates, d_scale)
    rel = float(np.max(np.abs(-d_rates - fd) / np.abs(fd)))
    q = lambda x: dict(median=round(statistics.median(x), 2), min=round(min(x), 2), max=round(max(x), 2))
    med = statistics.median
    res = dict(shape=sh, branches=n, launches=launches, branch_derivatives_us=q(t_old), rate_gradient_us=q(t_new),
               finite_differences_us=q(t_fd), prepare_us=q(t_prep), likelihood_evaluations=2 * R,
               rate_gradient_over_branch_derivatives=round(med(t_new) / med(t_old), 3),
               finite_differences_over_rate_gradient=round(med(t_fd) / med(t_new), 1),
               finite_differences_over_prepare_plus_rate_gradient=round(med(t_fd) / (med(t_new) + med(t_prep)), 1),
               worst_relative_difference_from_central_differences=float(f"{rel:.3g}"))
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_gradient.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="dna,aa")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps,
           "clock": "host clock around the synchronous calls, the variants alternating; medians, min, max in us"}
    for name in a.shapes.split(","):
        res[name] = run_shape(lib, name, a.reps)
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
