"""What drawing the RELL weights on the device saves: pll_gpu_quartet_rell_loglikelihoods against
pll_gpu_quartet_resampled_loglikelihoods with the same rows uploaded from the host, over all 61 inner edges of the seeded
64-taxon tree x 100k DNA sites x 1000 replicates, in one run on one device - profiles/quartet_rell.json.

Tree, alignment and the untimed preparation are tools/quartet_resample_probe.py's. Timed, host clock around the synchronous
calls, the two calls alternating in one process, `--reps` repetitions after two warm-up rounds, medians: the host-weights
call (lnl + resampled; its rows are the ones the rell call returned once, so both compute the same values and every output
is compared bit for bit) and the rell call (lnl + resampled, no rows copied back). Inside each call, by stream events
(pll_gpu_resample_last_times): what puts the weights in place - the upload, or the draw -, the quartet launch, contraction +
reduction. The prefix sums of the pattern weights (k_rell_cdf, once per change of the weights): the host time of a one-row
pll_gpu_draw_replicate_weights directly after pll_set_pattern_weights less that of the next one.

Every candidate of k_rell_draw's range H (sites per workgroup, PLL_AMD_RELL_RANGE, read when the partition is created) runs
in a partition of its own; `kept_range` names the library's default. For context, not as a gate: the host time of
numpy.random.Generator.multinomial for the same 1000 rows, once.

Usage: python tools/quartet_rell_probe.py [--out profiles/quartet_rell.json] [--reps 10] [--replicates 1000] [--ranges 16384,32768]"""
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

SHAPE = dict(states=4, rate_cats=4, taxa=64, sites=100000)
KEPT = 32768  # kernels_rell.h: kRellRange
SEED = 20261020


def q(x):
    return dict(median=round(statistics.median(x), 3), min=round(min(x), 3), max=round(max(x), 3))


def run(lib, b, rows, replicates, reps):
    sites, nq = b.sites, len(rows)
    fi, arr = api.uptr(b.fi), api.make_quartets(rows)
    w = driver.draw_replicate_weights(lib, b.p, SEED, 0, replicates)
    assert (w.sum(axis=1) == sites).all()
    lnl_h, res_h = np.empty((nq, 3)), np.empty((nq, replicates, 3))
    lnl_d, res_d = np.empty((nq, 3)), np.empty((nq, replicates, 3))
    ms = np.zeros(3)
    t_host, t_dev, ph_host, ph_dev, launches = [], [], [], [], 0
    for rep in range(reps + 2):  # two warm-up rounds
        t0 = time.perf_counter()
        ok = lib.pll_gpu_quartet_resampled_loglikelihoods(b.p, arr, nq, fi, api.uptr(w), replicates, api.dptr(lnl_h), api.dptr(res_h), None)
        t1 = time.perf_counter()
        assert ok, (lib.errno(), lib.errmsg())
        assert lib.pll_gpu_resample_last_times(b.p, api.dptr(ms))
        up = ms.copy()
        t2 = time.perf_counter()
        ok = lib.pll_gpu_quartet_rell_loglikelihoods(b.p, arr, nq, fi, SEED, replicates, api.dptr(lnl_d), api.dptr(res_d), None, None)
        t3 = time.perf_counter()
        assert ok, (lib.errno(), lib.errmsg())
        launches = int(lib.pll_gpu_last_launch_count(b.p))
        assert lib.pll_gpu_resample_last_times(b.p, api.dptr(ms))
        if rep >= 2:
            t_host.append((t1 - t0) * 1e3)
            t_dev.append((t3 - t2) * 1e3)
            ph_host.append(up)
            ph_dev.append(ms.copy())
    assert lnl_h.tobytes() == lnl_d.tobytes() and res_h.tobytes() == res_d.tobytes(), "the two calls differ"
    # the prefix sums: a one-row draw after a change of the weights against the next one
    ones, one_row = np.ones(sites, dtype=np.uint32), np.empty((1, sites), dtype=np.uint32)
    cdf = []
    for _ in range(reps):
        lib.pll_set_pattern_weights(b.p, api.uptr(ones))
        t0 = time.perf_counter()
        assert lib.pll_gpu_draw_replicate_weights(b.p, SEED, 0, 1, api.uptr(one_row))
        t1 = time.perf_counter()
        assert lib.pll_gpu_draw_replicate_weights(b.p, SEED, 0, 1, api.uptr(one_row))
        t2 = time.perf_counter()
        cdf.append(((t1 - t0) - (t2 - t1)) * 1e3)
    ph, pd = np.median(np.array(ph_host), axis=0), np.median(np.array(ph_dev), axis=0)
    out = dict(replicates=replicates, rell_launches=launches, host_weights_call_ms=q(t_host), rell_call_ms=q(t_dev),
               upload_ms=round(float(ph[0]), 3), draw_ms=round(float(pd[0]), 3), upload_bytes=int(w.nbytes),
               host_weights_stage1_ms=round(float(ph[1]), 3), host_weights_stage2_ms=round(float(ph[2]), 3),
               rell_stage1_ms=round(float(pd[1]), 3), rell_stage2_ms=round(float(pd[2]), 3),
               cdf_rebuild_ms=q(cdf), same_bits=True,
               draw_below_upload=bool(pd[0] < ph[0]), call_below_call=bool(statistics.median(t_dev) < statistics.median(t_host)))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quartet_rell.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--replicates", type=int, default=1000)
    ap.add_argument("--ranges", default="16384,32768")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    sh = SHAPE
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps, "shape": sh, "kept_range": KEPT,
           "clock": "host clock around the synchronous calls, the two calls alternating; medians, min, max in ms; upload / draw / "
                    "stage1 / stage2: stream events inside the call, medians"}
    lay, seqs, cmap, exch, freqs = IC.make(sh["states"], sh["taxa"], sh["sites"], sh["rate_cats"])
    res["ranges"] = {}
    for h in a.ranges.split(","):
        os.environ["PLL_AMD_RELL_RANGE"] = h  # read when the partition's context is created
        with IC.Bed(lib, lay, sh["states"], sh["sites"], sh["rate_cats"], 0, seqs, cmap, exch, freqs) as b:
            rows = QC.prepare(b)
            assert len(rows) == sh["taxa"] - 3
            res["quartets"] = len(rows)
            res["ranges"][h] = run(lib, b, rows, a.replicates, a.reps)
    del os.environ["PLL_AMD_RELL_RANGE"]
    t0 = time.perf_counter()
    np.random.Generator(np.random.PCG64(11)).multinomial(sh["sites"], np.full(sh["sites"], 1.0 / sh["sites"]), size=a.replicates)
    res["numpy_multinomial_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
