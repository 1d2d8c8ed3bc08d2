"""What the maximum-likelihood distances between all pairs of sequences cost: (a) ONE pll_gpu_pairwise_distances call over the
whole list and (b) the per-pair path this library offered before it - pll_update_sumtable on the two tips, then
pll_gpu_optimize_branch_length, once per pair - in the same run - profiles/pairwise_distances.json.

Inputs: all pairs of 64 taxa x 100k DNA sites (4 states x 4 rates), 64 taxa x 20k sites x 20 states x 4 rates, and 1024 taxa
x 10k DNA sites; workload.random_states at 15 % mutation (seed 8), no ambiguity, pattern weights 1. Options: t_start 0.1,
bounds [1e-6, 100], tolerance 1e-8 x sites, at most 32 evaluations. (a) runs on a PLL_ATTRIB_PATTERN_TIP partition, (b) on a
plain one of the same data (pll_update_sumtable gives one of two code tips a dense CLV: the partitions must differ); at
1024 taxa (b) is timed on a sample of 2000 pairs (PCG64 seed 5) and scaled to all pairs.
Timed with device events on the partition's stream (pll_gpu_timer_start / _stop around the synchronous calls: launches and
the copy back) and with the host clock. The split: the same call with max_iters = 1 is the histogram plus ONE evaluation per
pair; the full call minus that is the rest of the iteration. The histogram's rate divides the code-row bytes a call reads
(2 x sites per pair; the pattern weights, 4 bytes per site and pair, come on top and are listed) by the device time of the
max_iters = 1 call - a lower bound: that time holds the code vectors' launch, an evaluation and the copy back as well.
Checked, not timed: the distances of (a) and (b) agree to 1e-6 relative on the pairs (b) ran. Nothing is asserted on time.

Usage: python tools/pairwise_distances_timing.py [--out profiles/pairwise_distances.json] [--reps 5] [--shapes dna,aa,dna1024] [--no-json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "libpll-2_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import distance_cases as DC  # noqa: E402
import insertion_cases as IC  # noqa: E402
from pllamd import api, driver  # noqa: E402

SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000, sample=0),
          "aa": dict(states=20, rate_cats=4, taxa=64, sites=20000, sample=0),
          "dna1024": dict(states=4, rate_cats=4, taxa=1024, sites=10000, sample=2000)}
# HBM: the MI355X figure README.md and DESIGN.md quote; L2: rows that every workgroup shares, read at 16.8-18.8 TB/s chip-wide
PEAK = dict(hbm_bytes_per_s=8.0e12, l2_bytes_per_s=16.8e12)


def timed(lib, p, call):
    s0 = time.perf_counter()
    assert lib.pll_gpu_timer_start(p)
    out = call()
    ms = lib.pll_gpu_timer_stop(p)
    return out, ms * 1e3, (time.perf_counter() - s0) * 1e6


def run_shape(lib, name, reps):
    sh = SHAPES[name]
    S, R, taxa, sites = sh["states"], sh["rate_cats"], sh["taxa"], sh["sites"]
    seqs, cmap, exch, freqs = IC.alignment(S, taxa, sites)
    pairs = DC.pairs(taxa)
    tol = 1e-8 * sites
    full, one = driver.newton_options(0.1, 1e-6, 100.0, tol, 32), driver.newton_options(0.1, 1e-6, 100.0, tol, 1)
    tips = list(range(taxa))
    dev = {"full": [], "one_evaluation": []}
    host = {"full": [], "one_evaluation": []}
    with DC.Tips(lib, S, R, seqs, cmap, exch, freqs, attrs=api.PATTERN_TIP) as b:
        for rep in range(reps + 2):  # two warm-up rounds
            for key, opt in (("full", full), ("one_evaluation", one)):
                out, d_us, h_us = timed(lib, b.p, lambda: b.distances(tips, opt))
                if key == "full":
                    batched, launches = out, b.launches()
                if rep >= 2:
                    dev[key].append(d_us)
                    host[key].append(h_us)
    iters = np.array([batched["iterations"][x, y] for x, y in pairs])
    status = np.array([batched["status"][x, y] for x, y in pairs])

    # (b) the per-pair path, on a partition of its own
    sample = pairs
    if sh["sample"]:
        pick = np.random.Generator(np.random.PCG64(5)).choice(len(pairs), size=sh["sample"], replace=False)
        sample = [pairs[i] for i in sorted(pick)]
    res_t = np.empty(len(sample))
    waits = 0
    with DC.Tips(lib, S, R, seqs, cmap, exch, freqs) as b:
        opt, res = driver.newton_options(0.1, 1e-6, 100.0, tol, 32), api.NewtonResult()

        def per_pair():
            nonlocal waits
            waits = 0
            for i, (x, y) in enumerate(sample):
                st = b.table(x, y)
                assert lib.pll_gpu_optimize_branch_length(b.p, DC.NONE, DC.NONE, api.uptr(b.pi), api.dptr(st), C.byref(opt), C.byref(res), None), \
                    (lib.errno(), lib.errmsg())
                res_t[i] = res.t
                waits += res.host_waits

        per_pair()  # warm-up (and every tip dense)
        s0 = time.perf_counter()
        per_pair()
        pair_us = (time.perf_counter() - s0) * 1e6
    got = np.array([batched["distance"][x, y] for x, y in sample])
    assert np.allclose(got, res_t, rtol=1e-6, atol=1e-9), float(np.max(np.abs(got - res_t)))
    med = statistics.median
    q = lambda x: dict(median=round(med(x), 1), min=round(min(x), 1), max=round(max(x), 1))
    n = len(pairs)
    t1 = med(dev["one_evaluation"]) * 1e-6
    code_bytes, weight_bytes = 2.0 * sites * n, 4.0 * sites * n
    per_pair_all = pair_us * n / len(sample)
    out = dict(shape=sh, pairs=n, launches=launches, layout="one pair per workgroup (no blocked layout was tried)",
               device_us={k: q(v) for k, v in dev.items()}, host_us={k: q(v) for k, v in host.items()},
               iteration_after_the_first_evaluation_us=round(med(dev["full"]) - med(dev["one_evaluation"]), 1),
               evaluations_per_pair=dict(mean=round(float(iters.mean()), 2), max=int(iters.max())),
               status_counts={str(s): int((status == s).sum()) for s in np.unique(status)},
               per_pair_path=dict(pairs_timed=len(sample), host_us=round(pair_us, 1), us_per_pair=round(pair_us / len(sample), 2),
                                  host_waits=waits, host_us_scaled_to_all_pairs=round(per_pair_all, 1)),
               per_pair_path_over_one_call=round(per_pair_all / med(host["full"]), 1),
               histogram=dict(code_row_bytes=code_bytes, pattern_weight_bytes=weight_bytes,
                              code_row_bytes_per_s=float(f"{code_bytes / t1:.4g}"), all_bytes_per_s=float(f"{(code_bytes + weight_bytes) / t1:.4g}"),
                              code_rows_fraction_of_hbm=round(code_bytes / t1 / PEAK["hbm_bytes_per_s"], 4),
                              all_bytes_fraction_of_l2=round((code_bytes + weight_bytes) / t1 / PEAK["l2_bytes_per_s"], 4)))
    print(name, json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_distances.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default="dna,aa,dna1024")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps, "peaks": PEAK,
           "clock": "device events on the partition's stream and the host clock around the synchronous calls; medians, min, max in us; "
                    "the per-pair path with the host clock alone (one pass after a warm-up pass)"}
    for name in a.shapes.split(","):
        res[name] = run_shape(lib, name, a.reps)
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
