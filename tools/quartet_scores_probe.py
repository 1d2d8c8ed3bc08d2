"""What ranking the NNI neighbourhood of a tree costs: ONE pll_gpu_quartet_loglikelihoods call over all 61 inner edges of
the seeded 64-taxon tree (183 values) against the same values through the per-edge path of the same library (per value one
pll_update_partials with two operations into two spare nodes + pll_compute_edge_loglikelihood) - profiles/quartet_scores.json.

Shapes: 64 taxa x 100k sites, DNA (4 states x 4 rates), and 64 taxa x 10k sites, 20 states x 4 rates; the tree and the
alignment come from seeds (tests/insertion_cases.py), nothing is read from disk. OUTSIDE both timed regions: the rooted
full traversal and the "upward" CLVs of every edge into spare slots (tests/quartet_cases.py). Timed, host clock around the
synchronous calls, the two variants alternating, `--reps` repetitions after two warm-up rounds: the batched call; the
per-edge loop (operation arrays built beforehand: two library calls per value inside the clock). Every batched value is
compared with the per-edge one (1e-10 relative), and the run fails unless the batched call's median is faster than the
per-edge path's fastest repetition.

Bytes per site, derived: `batched` = what one quartet reads for all three values (its four ends and their scalers);
`per_edge` = what the three values move through the per-edge path (per value: two operations read two ends each and write
a spare CLV and scaler, the edge evaluation reads both spare nodes back). Share of the 8 TB/s peak from the batched call's
median (host clock: launch and wait included; the kernel's own durations come from a separate
`rocprofv3 --kernel-trace --stats` pass over `--reps 3 --no-json`).

Usage: python tools/quartet_scores_probe.py [--out profiles/quartet_scores.json] [--reps 20] [--shapes dna,aa] [--no-json]"""
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
from pllamd import api, driver  # noqa: E402

PEAK = 8.0e12
RTOL = 1e-10
SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000), "aa": dict(states=20, rate_cats=4, taxa=64, sites=10000)}


def traffic(bed, rows):
    """(bytes one batched call reads, bytes the per-edge path moves) over all rows"""
    lay = bed.lay
    clv = ((bed.sites + 63) // 64) * 64 * bed.states * bed.rate_cats * 8
    tip, sc = bed.sites, bed.sites * 4
    size = lambda e: (tip if e[0] < lay.tips else clv) + (sc if e[1] >= 0 and e[0] >= lay.tips else 0)
    batched = sum(size(e) for r in rows for e in r[:4])
    # per value: both operations read their two ends and write a spare node, the evaluation reads both spare nodes
    per_edge = sum(3 * sum(size(e) for e in r[:4]) + 3 * 4 * (clv + sc) for r in rows)
    return batched, per_edge


def run_shape(lib, name, reps):
    sh = SHAPES[name]
    lay, seqs, cmap, exch, freqs = IC.make(sh["states"], sh["taxa"], sh["sites"], sh["rate_cats"])
    with IC.Bed(lib, lay, sh["states"], sh["sites"], sh["rate_cats"], 0, seqs, cmap, exch, freqs) as b:
        rows = QC.prepare(b)
        assert len(rows) == sh["taxa"] - 3
        fi = api.uptr(b.fi)
        arr = api.make_quartets(rows)
        t1_, t2_ = lay.tmp, lay.cherry
        ops = []
        for r in rows:
            for (x, y), (z, w) in driver.QUARTET_PAIRS:
                ops.append((api.make_ops([(t1_[0], t1_[1], r[x][0], r[x][2], r[x][1], r[y][0], r[y][2], r[y][1]),
                                          (t2_[0], t2_[1], r[z][0], r[z][2], r[z][1], r[w][0], r[w][2], r[w][1])]), int(r[4])))
        got, exp = np.empty(3 * len(rows)), np.empty(3 * len(rows))
        tb, ts, launches = [], [], 0
        for rep in range(reps + 2):  # two warm-up rounds
            t0 = time.perf_counter()
            ok = lib.pll_gpu_quartet_loglikelihoods(b.p, arr, len(rows), fi, api.dptr(got))
            t1 = time.perf_counter()
            assert ok, (lib.errno(), lib.errmsg())
            launches = int(lib.pll_gpu_last_launch_count(b.p))
            t2 = time.perf_counter()
            for i, (two, inner) in enumerate(ops):
                lib.pll_update_partials(b.p, two, 2)
                exp[i] = lib.pll_compute_edge_loglikelihood(b.p, t1_[0], t1_[1], t2_[0], t2_[1], inner, fi, None)
            t3 = time.perf_counter()
            if rep >= 2:
                tb.append((t1 - t0) * 1e6)
                ts.append((t3 - t2) * 1e6)
        batched_bytes, per_edge_bytes = traffic(b, rows)
    worst = float(np.max(np.abs(got - exp) / np.maximum(np.abs(exp), 1.0)))
    assert worst <= RTOL, worst
    q = lambda x: dict(median=round(statistics.median(x), 2), min=round(min(x), 2), max=round(max(x), 2))
    res = dict(shape=sh, quartets=len(rows), values=len(got), launches=launches, batched_us=q(tb), per_edge_us=q(ts), worst_rel_diff=worst,
               us_per_value_batched=round(statistics.median(tb) / len(got), 3), us_per_value_per_edge=round(statistics.median(ts) / len(got), 3),
               ratio_of_medians=round(statistics.median(ts) / statistics.median(tb), 2),
               bytes_per_site_per_quartet_batched=round(batched_bytes / len(rows) / sh["sites"], 1),
               bytes_per_site_per_quartet_per_edge=round(per_edge_bytes / len(rows) / sh["sites"], 1),
               share_of_peak_batched=round(batched_bytes / (statistics.median(tb) * 1e-6) / PEAK, 4))
    print(name, json.dumps(res), flush=True)
    assert statistics.median(tb) < min(ts), f"{name}: the batched call's median {statistics.median(tb):.1f} us is not below the per-edge path's fastest repetition {min(ts):.1f} us"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quartet_scores.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="dna,aa")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps, "peak_bytes_per_s": PEAK,
           "clock": "host clock around the synchronous calls, batched and per-edge alternating; medians, min, max in us"}
    for name in a.shapes.split(","):
        res[name] = run_shape(lib, name, a.reps)
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
