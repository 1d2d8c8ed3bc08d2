"""What scoring Q query sequences against every edge of a tree costs: ONE pll_gpu_placement_loglikelihoods call against
pll_gpu_insertion_loglikelihoods looped over the queries in the same process - profiles/placement_scores.json.

Shapes: 64 taxa x 100k sites, DNA (4 states x 4 rates), all 125 edges, Q in {1, 8, 64, 512}; 64 taxa x 10k sites,
20 states x 4 rates, all 125 edges, Q in {1, 8, 64}. The tree, the alignment and the query sequences come from seeds
(tests/insertion_cases.py: make(..., extra=64)), nothing is read from disk; the partition is PLL_ATTRIB_PATTERN_TIP,
so a tip costs the host one byte per site. 64 query tips are set; Q = 512 names each of them eight times (the call
allows it, and a row's bytes do not depend on what else is in the list). Outside the timed regions: the full traversal,
the upward CLVs and the half-length matrices of every edge (Bed.prepare).

Timed, host clock around the synchronous calls, the two variants alternating, `--reps` repetitions after two warm-up
rounds: the new call over Q x 125 pairs; the existing call once per query over the same 125 candidates. Every value of
the new call is compared with the loop's, byte for byte. Per Q: median, min and max of both in us, the time per
(query, candidate) pair, and the two requirements - Q = 1: the new call's median is no slower than the loop's slowest
repetition; Q >= 8: the new call's median time per pair is below the loop's fastest repetition per pair.

Bytes per pair and site, derived (not measured): a candidate with two inner ends reads 2 x (S x R x 8 B + 4 B of
scaling counts) per site; the loop reads that and the query's byte for every pair; the new call reads it once per
chunk of QCH queries (include/pll_amd_device.h: PLLGPU_PLACEMENT_CHUNK_*) plus one byte per pair.

The kernels' own durations come from a separate `rocprofv3 --kernel-trace --stats` pass over `--reps 3 --no-json`.

Usage: python tools/placement_scores_probe.py [--out profiles/placement_scores.json] [--reps 20] [--shapes dna,aa] [--no-json]"""
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
from pllamd import api  # noqa: E402

SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000, queries=(1, 8, 64, 512), chunk=16),
          "aa": dict(states=20, rate_cats=4, taxa=64, sites=10000, queries=(1, 8, 64), chunk=4)}
TIPS = 64  # query tips set in the partition


def measure(b, tips, rows, reps):
    lib, p, lay = b.lib, b.p, b.lay
    arr, fi = api.make_insertions(rows), api.uptr(b.fi)
    q = np.ascontiguousarray(tips, dtype=np.uint32)
    got, exp = np.empty((len(q), len(rows))), np.empty((len(q), len(rows)))
    tn, tl, launches = [], [], 0
    for rep in range(reps + 2):  # two warm-up rounds
        t0 = time.perf_counter()
        ok = lib.pll_gpu_placement_loglikelihoods(p, api.uptr(q), len(q), lay.pm_pendant, arr, len(rows), fi, api.dptr(got))
        t1 = time.perf_counter()
        assert ok, (lib.errno(), lib.errmsg())
        launches = int(lib.pll_gpu_last_launch_count(p))
        for r, tip in enumerate(q):
            assert lib.pll_gpu_insertion_loglikelihoods(p, int(tip), IC.NONE, lay.pm_pendant, arr, len(rows), fi, api.dptr(exp[r]))
        t2 = time.perf_counter()
        if rep >= 2:
            tn.append((t1 - t0) * 1e6)
            tl.append((t2 - t1) * 1e6)
    assert got.tobytes() == exp.tobytes(), "the new call and the loop differ"
    pairs = len(q) * len(rows)
    s = lambda x: dict(median=round(statistics.median(x), 2), min=round(min(x), 2), max=round(max(x), 2))
    new, loop = s(tn), s(tl)
    rec = dict(queries=len(q), candidates=len(rows), launches=launches, placement_us=new, loop_us=loop,
               ns_per_pair_placement=round(new["median"] * 1e3 / pairs, 2), ns_per_pair_loop_median=round(loop["median"] * 1e3 / pairs, 2),
               ns_per_pair_loop_fastest=round(loop["min"] * 1e3 / pairs, 2), ratio_of_medians=round(loop["median"] / new["median"], 2))
    rec["requirement"] = ("median <= the loop's slowest repetition" if len(q) == 1 else "median per pair < the loop's fastest repetition per pair")
    rec["met"] = bool(new["median"] <= loop["max"]) if len(q) == 1 else bool(new["median"] < loop["min"])
    return rec


def run_shape(lib, name, reps):
    sh = SHAPES[name]
    lay, seqs, cmap, exch, freqs = IC.make(sh["states"], sh["taxa"], sh["sites"], sh["rate_cats"], extra=TIPS)
    out = []
    with IC.Bed(lib, lay, sh["states"], sh["sites"], sh["rate_cats"], api.PATTERN_TIP, seqs, cmap, exch, freqs) as b:
        rows = b.prepare()
        for nq in sh["queries"]:
            tips = [lay.T + (i % TIPS) for i in range(nq)]
            rec = measure(b, tips, rows, reps)
            out.append(rec)
            print(f"{name} Q={nq}: placement {rec['placement_us']['median']} us, loop {rec['loop_us']['median']} us "
                  f"[{rec['loop_us']['min']}, {rec['loop_us']['max']}], x{rec['ratio_of_medians']}, {rec['launches']} launch(es), "
                  f"requirement met: {rec['met']}", flush=True)
    clv = sh["states"] * sh["rate_cats"] * 8 + 4
    per_pair = lambda nq: round((-(-nq // sh["chunk"]) * 2 * clv + nq) / nq, 2)
    return dict(shape={k: sh[k] for k in ("states", "rate_cats", "taxa", "sites")}, chunk=sh["chunk"], results=out,
                derived_bytes_per_pair_and_site=dict(loop=2 * clv + 1, placement={str(nq): per_pair(nq) for nq in sh["queries"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placement_scores.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="dna,aa")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps,
           "clock": "host clock around the synchronous calls, the new call and the loop alternating; medians, min, max in us"}
    for name in a.shapes.split(","):
        res[name] = run_shape(lib, name, a.reps)
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
