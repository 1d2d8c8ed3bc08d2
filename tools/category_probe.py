"""What the rate-category calls cost: pll_gpu_edge_category_posteriors and pll_gpu_category_weights_em on the root edge of a
balanced 64-taxon tree against what they replace in the same library - rate_cats one-hot pll_set_category_weights +
pll_compute_edge_loglikelihood(persite) calls plus one with the real weights - profiles/category_posteriors.json.

Shapes: 64 taxa x 100k sites, DNA (4 states x 4 rates), and 64 taxa x 20k sites, 20 states x 4 rates (pllamd.workload
make_case: seeded, nothing is read from disk). OUTSIDE every timed region: the full traversal. Timed by device events on
the partition's stream (pll_gpu_timer_start / _stop around the synchronous calls, so uploads, copies back and waits are
inside), in one process, after two warm-up rounds, the legs alternating within every repetition:
  all          the posteriors call with all five outputs
  sums         ... with weight_sums + lnl only
  em0, em20    the EM call with 0 and with 20 steps; per step = (em20 - em0) / 20
  loop         what `all` replaces: rate_cats + 1 weight settings and per-site evaluations (unchanged entry points)
  edge         one plain pll_compute_edge_loglikelihood on the same edge: the floor of stage A
The posteriors of `all` are compared with those formed from the loop's per-site values (w_k exp(one_k - full), 1e-10
relative). Nothing is asserted on time: the figures are reported as measured.

Usage: python tools/category_probe.py [--out profiles/category_posteriors.json] [--reps 20] [--shapes dna,aa] [--no-json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "libpll-2_amd"), ROOT]
import numpy as np  # noqa: E402
from pllamd import api, driver, workload as W  # noqa: E402

SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000), "aa": dict(states=20, rate_cats=4, taxa=64, sites=20000)}
EM_STEPS = 20
WEIGHTS = (0.1, 0.2, 0.3, 0.4)


def timed(lib, p, fn):
    """milliseconds between two events on the partition's stream around fn()"""
    assert lib.pll_gpu_timer_start(p)
    fn()
    return lib.pll_gpu_timer_stop(p)


def run_shape(lib, name, reps):
    sh = SHAPES[name]
    case = W.make_case(name, sh["states"], sh["taxa"], sh["sites"], rate_cats=sh["rate_cats"], seed=5)
    case.rate_weights = np.array(WEIGHTS)
    r, n = sh["rate_cats"], sh["sites"]
    with driver.Session(lib, case) as s:
        rates = np.ascontiguousarray(case.model["rates"], dtype=np.float64)
        lib.pll_set_category_rates(s.p, api.dptr(rates))
        s.update_partials()
        edge = tuple(case.edges[0])
        w = np.ascontiguousarray(case.rate_weights, dtype=np.float64)
        one, full = np.zeros((r, n)), np.zeros(n)
        units = np.eye(r)
        keep = {}

        # every leg writes into arrays made (and touched) once, as the loop's are
        out = {"cat_lnl": np.zeros((n, r)), "posterior": np.zeros((n, r)), "site_rates": np.zeros(n), "weight_sums": np.zeros(r), "lnl": np.zeros(1)}
        sums = {"weight_sums": np.zeros(r), "lnl": np.zeros(1)}
        em = {steps: (np.zeros((steps + 1, r)), np.zeros(steps + 1)) for steps in (0, EM_STEPS)}
        names = ("cat_lnl", "posterior", "site_rates", "weight_sums", "lnl")

        def posteriors(arrays):
            ok = lib.pll_gpu_edge_category_posteriors(s.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(s._fi),
                                                      *[api.dptr(arrays[k]) if k in arrays else None for k in names])
            assert ok, (lib.errno(), lib.errmsg())

        def leg_all():
            posteriors(out)
            keep["all"] = dict(out, lnl=float(out["lnl"][0]))

        def leg_sums():
            posteriors(sums)

        def leg_em(steps):
            ok = lib.pll_gpu_category_weights_em(s.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(s._fi), None, steps,
                                                 api.dptr(em[steps][0]), api.dptr(em[steps][1]))
            assert ok, (lib.errno(), lib.errmsg())
            keep["em%d" % steps] = em[steps]

        def leg_loop():
            fi = api.uptr(s._fi)
            for k in range(r):
                lib.pll_set_category_weights(s.p, api.dptr(units[k]))
                lib.pll_compute_edge_loglikelihood(s.p, edge[0], edge[1], edge[2], edge[3], edge[4], fi, api.dptr(one[k]))
            lib.pll_set_category_weights(s.p, api.dptr(w))
            keep["loop_lnl"] = lib.pll_compute_edge_loglikelihood(s.p, edge[0], edge[1], edge[2], edge[3], edge[4], fi, api.dptr(full))

        def leg_edge():
            keep["edge_lnl"] = s.edge_lnl(edge, persite=False)[0]

        legs = {"all": leg_all, "sums": leg_sums, "em0": lambda: leg_em(0), "em20": lambda: leg_em(EM_STEPS), "loop": leg_loop, "edge": leg_edge}
        ms = {k: [] for k in legs}
        for rep in range(reps + 2):  # two warm-up rounds
            for k, fn in legs.items():
                t = timed(lib, s.p, fn)
                if rep >= 2:
                    ms[k].append(t * 1e3)
        launches = {}
        for k in ("all", "sums", "em0", "em20"):
            legs[k]()
            launches[k] = int(lib.pll_gpu_last_launch_count(s.p))
    post = w[None, :] * np.exp(one.T - full[:, None])  # pattern weights are 1 here
    worst = float(np.max(np.abs(keep["all"]["posterior"] - post) / post))
    assert worst <= 1e-10, worst
    assert abs(keep["all"]["lnl"] - keep["loop_lnl"]) <= 1e-10 * abs(keep["loop_lnl"])
    q = lambda x: dict(median=round(statistics.median(x), 2), min=round(min(x), 2), max=round(max(x), 2))
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = dict(shape=sh, edge=list(edge), launches=launches, us={k: q(v) for k, v in ms.items()},
               em_us_per_step=round((med["em20"] - med["em0"]) / EM_STEPS, 2),
               loop_over_all=round(med["loop"] / med["all"], 2), edge_over_em_step=round(med["edge"] / ((med["em20"] - med["em0"]) / EM_STEPS), 2),
               table_bytes=8 * r * ((n + 63) // 64) * 64 + 4 * n, clv_bytes_both_ends=2 * 8 * r * sh["states"] * ((n + 63) // 64) * 64,
               worst_posterior_rel_err_against_the_loop=worst, em_lnl_first_last=[float(keep["em20"][1][0]), float(keep["em20"][1][-1])])
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "category_posteriors.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="dna,aa")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps,
           "clock": "device events on the partition's stream around the synchronous calls, the legs alternating; medians, min, max in us"}
    for name in a.shapes.split(","):
        res[name] = run_shape(lib, name, a.reps)
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
