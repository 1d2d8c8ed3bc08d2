"""What the gradient over all branches of a tree costs: ONE pll_gpu_branch_derivatives call over all 125 edges of the seeded
64-taxon tree against the same values through the per-edge path of the same library (per edge pll_update_sumtable into one
caller-owned table + pll_compute_likelihood_derivatives) - profiles/branch_derivatives.json.

Shapes: 64 taxa x 100k sites, DNA (4 states x 4 rates), and 64 taxa x 20k sites, 20 states x 4 rates; the tree and the
alignment come from seeds (tests/insertion_cases.py), nothing is read from disk. OUTSIDE both timed regions: the rooted
full traversal and the "upward" CLVs of every edge into spare slots (tests/gradient_cases.py). Timed, host clock around the
synchronous calls, the two variants alternating, `--reps` repetitions after two warm-up rounds: the batched call; the
per-edge loop (two library calls per edge inside the clock). Every batched value is compared with the per-edge one
(deriv_common.close: 1e-10 relative + 4e-15 per site). Nothing is asserted on time: the figures are reported as measured.

Bytes per site, derived: `batched` = what one branch reads (its two ends: 256 B at 4 x 4 for two inner ends, a byte for an
end given by codes; the pattern weight once per branch); `per_edge` = the same ends, plus the table written and read back
(128 B each at 4 x 4). Share of the 8 TB/s peak from the batched call's median (host clock: descriptor upload, launch, copy
back and wait included), once from the bytes as derived and, for 4 x 4, once with every end taken as a CLV (256 B per site
and branch plus the weight).

Usage: python tools/branch_derivatives_probe.py [--out profiles/branch_derivatives.json] [--reps 20] [--shapes dna,aa]
       [--resources FILE.json] [--no-json]      (--resources: the compiler's resource summary of the kernels, embedded as is)"""
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
import gradient_cases as GC  # noqa: E402
import insertion_cases as IC  # noqa: E402
from pllamd import api  # noqa: E402

PEAK = 8.0e12
SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000), "aa": dict(states=20, rate_cats=4, taxa=64, sites=20000)}


def traffic(bed, rows):
    """(bytes one batched call reads, bytes the per-edge path moves) over all rows; no scaler is read in per-site mode"""
    lay = bed.lay
    clv = ((bed.sites + 63) // 64) * 64 * bed.states * bed.rate_cats * 8
    size = lambda clv_index: bed.sites if clv_index < lay.tips else clv
    weights = bed.sites * 4
    batched = sum(size(r[0]) + size(r[2]) + weights for r in rows)
    per_edge = batched + sum(2 * clv for r in rows)  # the table: written, read back
    return batched, per_edge


def run_shape(lib, name, reps):
    sh = SHAPES[name]
    lay, seqs, cmap, exch, freqs = IC.make(sh["states"], sh["taxa"], sh["sites"], sh["rate_cats"])
    with IC.Bed(lib, lay, sh["states"], sh["sites"], sh["rate_cats"], 0, seqs, cmap, exch, freqs) as b:
        rows = GC.prepare(b)
        assert len(rows) == 2 * sh["taxa"] - 3
        pi = api.uptr(b.fi)
        arr = api.make_branches(rows)
        n = b.sites * b.rate_cats * b.part.states_padded
        raw = np.zeros(n + 8)
        table = raw[(-raw.ctypes.data // 8) % 8:][:n]
        tp = api.dptr(table)
        got, exp = np.empty((2, len(rows))), np.empty((len(rows), 2))
        d1, d2 = C.c_double(0), C.c_double(0)
        tb, ts, launches = [], [], 0
        for rep in range(reps + 2):  # two warm-up rounds
            t0 = time.perf_counter()
            ok = lib.pll_gpu_branch_derivatives(b.p, arr, len(rows), pi, api.dptr(got[0]), api.dptr(got[1]))
            t1 = time.perf_counter()
            assert ok, (lib.errno(), lib.errmsg())
            launches = int(lib.pll_gpu_last_launch_count(b.p))
            t2 = time.perf_counter()
            for i, (p, ps, c, cs, t) in enumerate(rows):
                lib.pll_update_sumtable(b.p, p, c, ps, cs, pi, tp)
                lib.pll_compute_likelihood_derivatives(b.p, ps, cs, t, pi, tp, C.byref(d1), C.byref(d2))
                exp[i] = d1.value, d2.value
            t3 = time.perf_counter()
            if rep >= 2:
                tb.append((t1 - t0) * 1e6)
                ts.append((t3 - t2) * 1e6)
        lib.pll_gpu_release_sumtable(b.p, tp)
        batched_bytes, per_edge_bytes = traffic(b, rows)
    worst = GC.worst(got.T, exp, sh["sites"])
    assert GC.close(got.T, exp, sh["sites"]), worst
    q = lambda x: dict(median=round(statistics.median(x), 2), min=round(min(x), 2), max=round(max(x), 2))
    res = dict(shape=sh, branches=len(rows), launches=launches, batched_us=q(tb), per_edge_us=q(ts), worst_share_of_the_bound=round(worst, 4),
               us_per_branch_batched=round(statistics.median(tb) / len(rows), 3), us_per_branch_per_edge=round(statistics.median(ts) / len(rows), 3),
               ratio_of_medians=round(statistics.median(ts) / statistics.median(tb), 2),
               bytes_per_site_per_branch_batched=round(batched_bytes / len(rows) / sh["sites"], 1),
               bytes_per_site_per_branch_per_edge=round(per_edge_bytes / len(rows) / sh["sites"], 1),
               share_of_peak_batched=round(batched_bytes / (statistics.median(tb) * 1e-6) / PEAK, 4))
    if name == "dna":
        # the nominal figure: every end taken as a CLV (256 B per site and branch) plus the pattern weight; no scaler is read
        nominal = len(rows) * sh["sites"] * (256 + 4)
        res["share_of_peak_batched_at_256B_per_site"] = round(nominal / (statistics.median(tb) * 1e-6) / PEAK, 4)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_derivatives.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="dna,aa")
    ap.add_argument("--resources", default=None)
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps, "peak_bytes_per_s": PEAK,
           "clock": "host clock around the synchronous calls, batched and per-edge alternating; medians, min, max in us"}
    for name in a.shapes.split(","):
        res[name] = run_shape(lib, name, a.reps)
    if a.resources:
        with open(a.resources) as f:
            res["kernel_resources"] = json.load(f)
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
