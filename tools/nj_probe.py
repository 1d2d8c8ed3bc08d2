"""What a neighbour-joining / BIONJ tree costs on the device - profiles/nj_tree.json.

(a) pll_gpu_nj_tree on a matrix of 64, 1024 and 4096 taxa, both flags: the device time of the join's launches (events on the
call's own stream, pll_gpu_nj_last_device_ms: from the first launch to the last, without the copy of the matrix up and of
the tree back) and the host clock around the whole call. (b) pll_gpu_distance_tree, distances and join in one call, on the same
taxon counts x 10k DNA sites (1k sites at 4096 taxa): device events on the partition's stream (pll_gpu_timer_start / _stop) and the host clock, next to
pll_gpu_pairwise_distances alone on the same list. (c) The comparator: the wall clock of pllamd/nj.py, the numpy statement
of the same algorithm, on this host - not the code under test (4096 taxa only with --numpy-4096: minutes).

Inputs: nj.random_tree's additive matrix x (1 +- 5 % uniform), seed 7. Bytes scanned: a join at r active nodes reads the
upper triangle of the r x r block once, 8 r (r - 1) / 2 bytes; the sum over r = 4 .. n divided by the device time is the rate
the searches sustain at least (the joins' rows, the row sums and labels come on top). Checked, not timed: parent equals
nj.py's where nj.py ran. Nothing is asserted on time.

Usage: python tools/nj_probe.py [--out profiles/nj_tree.json] [--reps 5] [--taxa 64,1024,4096] [--numpy-4096] [--no-json]"""
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

FLAGS = {"nj": 0, "bionj": nj.BIONJ}
SITES = 10000


def matrix(n):
    rng = np.random.default_rng(7)
    parent, length = nj.random_tree(n, rng)
    up = np.triu(nj.tree_distances(parent, length) * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, size=(n, n))), 1)
    return up + up.T


def scanned_bytes(n):
    return sum(8 * r * (r - 1) // 2 for r in range(4, n + 1))


def q(x):
    return dict(median=round(statistics.median(x), 1), min=round(min(x), 1), max=round(max(x), 1))


def run_matrix(lib, n, reps, with_numpy):
    m = matrix(n)
    out = dict(taxa=n, launches=nj.launch_count(n), scanned_bytes=scanned_bytes(n))
    for flag, bits in FLAGS.items():
        dev, host = [], []
        for rep in range(reps + 2):  # two warm-up rounds
            s0 = time.perf_counter()
            tree = driver.nj_tree(lib, m, bits)
            h = (time.perf_counter() - s0) * 1e6
            if rep >= 2:
                host.append(h)
                dev.append(lib.pll_gpu_nj_last_device_ms() * 1e3)
        assert lib.pll_gpu_nj_last_launch_count() == out["launches"]
        rec = dict(device_us=q(dev), host_us=q(host), us_per_join=round(statistics.median(dev) / max(n - 3, 1), 2),
                   scanned_bytes_per_s=float(f"{out['scanned_bytes'] / (statistics.median(dev) * 1e-6):.4g}"))
        if with_numpy:
            s0 = time.perf_counter()
            exp = nj.nj_tree(m, bits)
            rec["numpy_restatement_wall_us"] = round((time.perf_counter() - s0) * 1e6, 1)
            rec["numpy_over_device_call_host_clock"] = round(rec["numpy_restatement_wall_us"] / statistics.median(host), 1)
            assert np.array_equal(exp[0], tree[0])
            rec["bit_for_bit_the_restatement"] = bool(exp[1].tobytes() == tree[1].tobytes())
        out[flag] = rec
    print("matrix", json.dumps(out), flush=True)
    return out


def run_fused(lib, taxa, reps):
    sites = SITES if taxa <= 1024 else SITES // 10
    seqs, cmap, exch, freqs = IC.alignment(4, taxa, sites)
    opt = driver.newton_options(0.1, 1e-6, 100.0, 1e-8 * sites, 32)
    tips = list(range(taxa))
    out = dict(taxa=taxa, sites=sites, states=4, rate_cats=4)

    def timed(p, call):
        s0 = time.perf_counter()
        assert lib.pll_gpu_timer_start(p)
        res = call()
        ms = lib.pll_gpu_timer_stop(p)
        return res, ms * 1e3, (time.perf_counter() - s0) * 1e6

    with DC.Tips(lib, 4, 4, seqs, cmap, exch, freqs, attrs=api.PATTERN_TIP) as b:
        calls = {"distances_alone": lambda: b.distances(tips, opt, want=())}
        for flag, bits in FLAGS.items():
            calls["tree_" + flag] = lambda bits=bits: driver.distance_tree(lib, b.p, tips, b.pi, opt, bits, want_distances=False)
        for name, call in calls.items():
            dev, host = [], []
            for rep in range(reps + 2):
                _, d, h = timed(b.p, call)
                if rep >= 2:
                    dev.append(d)
                    host.append(h)
            out[name] = dict(device_us=q(dev), host_us=q(host), launches=b.launches())
    print("fused", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nj_tree.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--taxa", default="64,1024,4096")
    ap.add_argument("--numpy-4096", action="store_true")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    taxa = [int(t) for t in a.taxa.split(",")]
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps,
           "clock": "device events (the call's own stream for pll_gpu_nj_tree, the partition's for the fused call) and the host clock "
                    "around the synchronous calls; medians, min, max in us; pllamd/nj.py with the host clock, one pass",
           "matrix": [run_matrix(lib, n, a.reps, n < 4096 or a.numpy_4096) for n in taxa],
           "fused": [run_fused(lib, n, a.reps) for n in taxa]}
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
