"""What the branch supports of a tree cost: ONE pll_gpu_quartet_resampled_loglikelihoods call over all 61 inner edges of the
seeded 64-taxon tree (183 values) under 100 and 1000 resampled weight vectors, against what a caller could do before the call
existed - pll_set_pattern_weights + pll_gpu_quartet_loglikelihoods once per replicate - profiles/quartet_resample.json.

Shapes: 64 taxa x 100k sites, DNA (4 states x 4 rates), and 64 taxa x 10k sites, 20 states x 4 rates; tree and alignment
come from seeds (tests/insertion_cases.py), the replicates are RELL resamples (`sites` uniform draws per row). OUTSIDE the
timed regions: the rooted full traversal and the "upward" CLVs (tests/quartet_cases.py). Timed, host clock around the
synchronous calls, the two variants alternating in one process, `--reps` repetitions after two warm-up rounds, medians: the
new call (lnl + resampled, no per-site copy); the per-replicate loop, on min(replicates, 50) replicates and scaled to the
replicate count where that is fewer (`baseline_scaled`). The partition's pattern weights are put back after every loop.
Every resampled value of the timed replicates is compared with the per-replicate one (1e-10 relative).

Inside the new call, by stream events (pll_gpu_resample_last_times): the upload of the weights, the quartet launch (stage 1),
contraction + reduction (stage 2); stage 2's fp64 rate = 2 x values x replicates x sites / its time.

Usage: python tools/quartet_resample_probe.py [--out profiles/quartet_resample.json] [--reps 10] [--shapes dna,aa] [--replicates 100,1000]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "libpll-2_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import insertion_cases as IC  # noqa: E402
import quartet_cases as QC  # noqa: E402
from pllamd import api  # noqa: E402

RTOL = 1e-10
BASELINE_MAX = 50
SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000), "aa": dict(states=20, rate_cats=4, taxa=64, sites=10000)}


def rell_weights(sites, replicates):
    rng = np.random.Generator(np.random.PCG64(11))
    w = np.empty((replicates, sites), dtype=np.uint32)
    for b in range(replicates):
        w[b] = np.bincount(rng.integers(0, sites, sites), minlength=sites)
    return w


def run(lib, b, rows, replicates, reps):
    sites, nq = b.sites, len(rows)
    w = rell_weights(sites, replicates)
    ones = np.ones(sites, dtype=np.uint32)
    nb = min(replicates, BASELINE_MAX)
    fi, arr = api.uptr(b.fi), api.make_quartets(rows)
    lnl, res = np.empty((nq, 3)), np.empty((nq, replicates, 3))
    base, one = np.empty((nq, nb, 3)), np.empty((nq, 3))
    ms = np.zeros(3)
    t_new, t_base, phases, launches = [], [], [], 0
    for rep in range(reps + 2):  # two warm-up rounds
        t0 = time.perf_counter()
        ok = lib.pll_gpu_quartet_resampled_loglikelihoods(b.p, arr, nq, fi, api.uptr(w), replicates, api.dptr(lnl), api.dptr(res), None)
        t1 = time.perf_counter()
        assert ok, (lib.errno(), lib.errmsg())
        launches = int(lib.pll_gpu_last_launch_count(b.p))
        assert lib.pll_gpu_resample_last_times(b.p, api.dptr(ms))
        t2 = time.perf_counter()
        for k in range(nb):
            lib.pll_set_pattern_weights(b.p, api.uptr(w[k]))
            assert lib.pll_gpu_quartet_loglikelihoods(b.p, arr, nq, fi, api.dptr(one))
            base[:, k, :] = one
        t3 = time.perf_counter()
        lib.pll_set_pattern_weights(b.p, api.uptr(ones))
        if rep >= 2:
            t_new.append((t1 - t0) * 1e3)
            t_base.append((t3 - t2) * 1e3 * replicates / nb)
            phases.append(ms.copy())
    worst = float(np.max(np.abs(res[:, :nb, :] - base) / np.maximum(np.abs(base), 1.0)))
    assert worst <= RTOL, worst
    q = lambda x: dict(median=round(statistics.median(x), 3), min=round(min(x), 3), max=round(max(x), 3))
    ph = np.median(np.array(phases), axis=0)
    flops = 2.0 * 3 * nq * replicates * sites
    out = dict(replicates=replicates, launches=launches, call_ms=q(t_new), baseline_ms=q(t_base), baseline_replicates_timed=nb,
               baseline_scaled=nb < replicates, ratio_of_medians=round(statistics.median(t_base) / statistics.median(t_new), 2),
               upload_ms=round(float(ph[0]), 3), stage1_ms=round(float(ph[1]), 3), stage2_ms=round(float(ph[2]), 3),
               upload_bytes=int(w.nbytes), stage2_fp64_tflops=round(flops / (float(ph[2]) * 1e-3) / 1e12, 2), worst_rel_diff=worst)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quartet_resample.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="dna,aa")
    ap.add_argument("--replicates", default="100,1000")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps,
           "clock": "host clock around the synchronous calls, the call and the per-replicate loop alternating; medians, min, max in ms; "
                    "upload / stage1 / stage2: stream events inside the call, medians"}
    for name in a.shapes.split(","):
        sh = SHAPES[name]
        lay, seqs, cmap, exch, freqs = IC.make(sh["states"], sh["taxa"], sh["sites"], sh["rate_cats"])
        with IC.Bed(lib, lay, sh["states"], sh["sites"], sh["rate_cats"], 0, seqs, cmap, exch, freqs) as b:
            rows = QC.prepare(b)
            assert len(rows) == sh["taxa"] - 3
            res[name] = dict(shape=sh, quartets=len(rows), values=3 * len(rows), runs=[run(lib, b, rows, int(r), a.reps) for r in a.replicates.split(",")])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
