"""What the bootstrap of a distance tree costs: (a) ONE pll_gpu_bootstrap_distance_trees call for all replicates and (b) the
host loop this library offered before it - pll_gpu_draw_replicate_weights once, then pll_set_pattern_weights +
pll_gpu_distance_tree per replicate - in the same run; and pll_gpu_nj_trees on 1000 matrices of 64 taxa next to 1000 calls of
pll_gpu_nj_tree and to pllamd/nj.py on this host - profiles/bootstrap_trees.json.

Inputs: workload.random_states at 15 % mutation (seed 8), no ambiguity, pattern weights 1, PLL_ATTRIB_PATTERN_TIP; NJ
(flags 0); t_start 0.1, bounds [1e-6, 100], tolerance 1e-8 x sites, at most 32 evaluations; seed 11, rows from 0.
(a) is timed with device events on the partition's stream (pll_gpu_timer_start / _stop around the synchronous call: every
chunk's launches and copies back) and with the host clock: medians of --reps rounds after two warm-up rounds. Its split -
draw, distance launches, joins - is that of the call's FIRST chunk (pll_gpu_bootstrap_last_times), whose replicates are
listed. (b) is timed with the host clock: the median of three passes after one warm-up pass. The rate at which the distance
launches read the weight rows divides 4 x sites bytes per (pair, replicate) of the first chunk by its distance time - the
code rows (2 x sites per pair and replicate) are listed beside it.
The matrices of the NJ comparison are nj_probe.matrix's recipe under 1000 seeds; nj.py runs one pass over the first 100 and
is scaled.
Checked, not timed: every row of (a) has the words of (b), and every tree of pll_gpu_nj_trees those of pll_gpu_nj_tree.
Nothing is asserted on time.

Usage: python tools/bootstrap_trees_timing.py [--out profiles/bootstrap_trees.json] [--reps 5] [--cases ...] [--no-json]"""
import argparse
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
from pllamd import api, driver, nj  # noqa: E402

CASES = {"dna64x100k_r100": (4, 64, 100000, 100), "dna64x100k_r1000": (4, 64, 100000, 1000), "dna64x10k_r1000": (4, 64, 10000, 1000),
         "dna1024x10k_r100": (4, 1024, 10000, 100), "aa64x20k_r100": (20, 64, 20000, 100)}
SEED = 11
BUDGET = 1 << 30  # PLLGPU_BOOTSTRAP_MAX_BYTES
L2_RATE_OF_THE_SINGLE_CALL = 4.653e12  # profiles/pairwise_distances.json, dna: all bytes per second


def q(x):
    return dict(median=round(statistics.median(x), 1), min=round(min(x), 1), max=round(max(x), 1))


def run_case(lib, name, reps):
    states, taxa, sites, replicates = CASES[name]
    seqs, cmap, exch, freqs = IC.alignment(states, taxa, sites)
    opt = driver.newton_options(0.1, 1e-6, 100.0, 1e-8 * sites, 32)
    tips = list(range(taxa))
    wstride = (sites + 3) // 4 * 4
    per_replicate = 4 * wstride + 48 * taxa * taxa + int(lib.pllgpu_nj_scratch_bytes(taxa, 0))
    first_chunk = min(replicates, 65535, max(1, BUDGET // per_replicate))
    out = dict(states=states, rate_cats=4, taxa=taxa, sites=sites, replicates=replicates, bytes_per_replicate=per_replicate,
               replicates_of_the_first_chunk=first_chunk, chunks=-(-replicates // first_chunk))
    with DC.Tips(lib, states, 4, seqs, cmap, exch, freqs, attrs=api.PATTERN_TIP) as b:
        dev, host, split = [], [], []
        for rep in range(reps + 2):  # two warm-up rounds
            s0 = time.perf_counter()
            assert lib.pll_gpu_timer_start(b.p)
            fused = api.bootstrap_distance_trees(lib, b.p, tips, b.pi, opt, 0, SEED, 0, replicates, want=())
            ms = lib.pll_gpu_timer_stop(b.p)
            h = (time.perf_counter() - s0) * 1e6
            three = np.zeros(3)
            assert lib.pll_gpu_bootstrap_last_times(b.p, api.dptr(three))
            if rep >= 2:
                dev.append(ms * 1e3)
                host.append(h)
                split.append(three * 1e3)
        out["one_call"] = dict(device_us=q(dev), host_us=q(host), launches=b.launches(),
                               first_chunk_us={k: q([s[i] for s in split]) for i, k in enumerate(("draw", "distances", "join"))})
        pairs = taxa * (taxa - 1) // 2
        t_dist = statistics.median([s[1] for s in split]) * 1e-6
        weight_bytes, code_bytes = 4.0 * sites * pairs * first_chunk, 2.0 * sites * pairs * first_chunk
        out["weight_rows"] = dict(bytes_read_by_the_first_chunk=weight_bytes, bytes_per_s=float(f"{weight_bytes / t_dist:.4g}"),
                                  code_row_bytes=code_bytes, all_bytes_per_s=float(f"{(weight_bytes + code_bytes) / t_dist:.4g}"),
                                  over_the_single_call_rate=round((weight_bytes + code_bytes) / t_dist / L2_RATE_OF_THE_SINGLE_CALL, 3))

        # (b) the host loop, on the same partition; its weights are put back
        own = np.ones(sites, dtype=np.uint32)

        def loop():
            rows = driver.draw_replicate_weights(lib, b.p, SEED, 0, replicates)
            trees = []
            for row in rows:
                lib.pll_set_pattern_weights(b.p, api.uptr(row))
                trees.append(driver.distance_tree(lib, b.p, tips, b.pi, opt, 0, want_distances=False)[:2])
            lib.pll_set_pattern_weights(b.p, api.uptr(own))
            return trees

        passes = []
        for rep in range(4):  # one warm-up pass
            s0 = time.perf_counter()
            trees = loop()
            if rep:
                passes.append((time.perf_counter() - s0) * 1e6)
        for r, (parent, length) in enumerate(trees):
            assert np.array_equal(fused["parent"][r], parent) and fused["length"][r].tobytes() == length.tobytes(), r
        out["host_loop"] = dict(host_us=q(passes), us_per_replicate=round(statistics.median(passes) / replicates, 1))
        out["host_loop_over_one_call"] = round(statistics.median(passes) / statistics.median(host), 2)
    print(name, json.dumps(out), flush=True)
    return out


def matrices(n, count):
    out = []
    for s in range(count):
        rng = np.random.default_rng(7000 + s)
        parent, length = nj.random_tree(n, rng)
        up = np.triu(nj.tree_distances(parent, length) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(n, n))), 1)
        out.append(up + up.T)
    return np.stack(out)


def run_nj(lib, reps, taxa=64, count=1000):
    m = matrices(taxa, count)
    out = dict(taxa=taxa, matrices=count)
    for flag, bits in (("nj", 0), ("bionj", nj.BIONJ)):
        dev, host = [], []
        for rep in range(reps + 2):
            s0 = time.perf_counter()
            batched = api.nj_trees(lib, m, bits)
            h = (time.perf_counter() - s0) * 1e6
            if rep >= 2:
                host.append(h)
                dev.append(lib.pll_gpu_nj_last_device_ms() * 1e3)
        rec = dict(one_call=dict(device_us=q(dev), host_us=q(host), launches=int(lib.pll_gpu_nj_last_launch_count()),
                                 device_us_per_tree=round(statistics.median(dev) / count, 3)))
        passes, dev_single = [], []
        for rep in range(3):  # one warm-up pass
            s0 = time.perf_counter()
            singles = []
            for x in m:
                singles.append(driver.nj_tree(lib, x, bits))
                if rep:
                    dev_single.append(lib.pll_gpu_nj_last_device_ms() * 1e3)
            if rep:
                passes.append((time.perf_counter() - s0) * 1e6)
        for r, (parent, length) in enumerate(singles):
            assert np.array_equal(batched[0][r], parent) and batched[1][r].tobytes() == length.tobytes(), r
        rec["per_tree_calls"] = dict(host_us=q(passes), device_us_per_tree=round(statistics.median(dev_single), 1),
                                     host_us_per_tree=round(statistics.median(passes) / count, 1))
        rec["per_tree_device_over_one_call_device"] = round(statistics.median(dev_single) * count / statistics.median(dev), 1)
        rec["per_tree_host_over_one_call_host"] = round(statistics.median(passes) / statistics.median(host), 1)
        s0 = time.perf_counter()
        for x in m[:100]:
            nj.nj_tree(x, bits)
        numpy_us = (time.perf_counter() - s0) * 1e6 * count / 100
        rec["numpy_restatement_wall_us_scaled"] = round(numpy_us, 1)
        rec["numpy_over_one_call_host"] = round(numpy_us / statistics.median(host), 1)
        out[flag] = rec
    print("nj_trees", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bootstrap_trees.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES) + ",nj_trees")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps,
           "clock": "device events on the call's stream and the host clock around the synchronous calls; medians, min, max in us; the "
                    "loops with the host clock (median of three passes after a warm-up pass)"}
    for name in a.cases.split(","):
        res[name] = run_nj(lib, a.reps) if name == "nj_trees" else run_case(lib, name, a.reps)
        if not a.no_json:  # (written after every case: a run that ends early keeps what it measured)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
