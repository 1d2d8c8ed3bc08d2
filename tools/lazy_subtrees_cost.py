#!/usr/bin/env python3
"""What leaving a loop costs with lazy subtrees (profiles/dna_tree_lazy_subtrees.md): a caller runs k steps without
reading a CLV, then reads a level-2 CLV - one of the 56 that the deep form of the tree launch leaves unstored from the
second step on - which stores all of them with one seven-op group launch. With k = 1 the deep form is never entered and
the read pays what it paid before: the launch that stores the 32 tip x tip parents.

Times, on the flagship shape (4 states, 4 rates, 64-taxon balanced tree), per repetition and between two waits for the
stream:
  k steps           k x (pll_update_partials (full traversal) + pll_compute_edge_loglikelihood at the root edge)
  k steps+read      ... + pll_gpu_sync_clv of one level-2 CLV (a download of sites x 128 B)
for every k of --k, and prints one JSON line. --root names the tree whose library is measured (a clean export of another
commit, built), default this one; PLL_AMD_LAZY_SUBTREES=0/1 selects the form where the library knows the switch."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--sites", type=int, default=100000)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 5])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.root), "libpll-2_amd"))
    from pllamd import api, driver, workload as W

    lib = api.PllLib()
    if not lib.pll_gpu_available():
        raise SystemExit("no MI355X visible")
    case = W.make_case("c2", 4, 64, args.sites, seed=1, generator="xorshift64")
    e = case.edges[0]
    cherry_parents = {op[0] for op in case.op_batches[0] if op[2] < case.tips and op[5] < case.tips}
    level_2 = [op for op in case.op_batches[0] if op[2] in cherry_parents and op[5] in cherry_parents][0]
    pending = getattr(lib, "pll_gpu_pending_clvs", None)
    with driver.Session(lib, case, api.ARCH_AVX2) as s:
        def step():
            s.update_partials()
            return s.edge_lnl(e, persite=False)[0]

        def read():
            if not lib.pll_gpu_sync_clv(s.p, level_2[0]):
                raise SystemExit(f"pll_gpu_sync_clv: {lib.errmsg()}")

        out = {"root": os.path.abspath(args.root), "sites": args.sites, "reps": args.reps,
               "lazy_subtrees": os.environ.get("PLL_AMD_LAZY_SUBTREES", "default"), "unit": "us"}
        for k in args.k:
            for name, after in (("%d steps" % k, ()), ("%d steps+read" % k, (read,))):
                times, unstored = [], None
                for r in range(args.warmup + args.reps):
                    read()  # every repetition starts like a caller who has just read: nothing pending
                    lib.pll_gpu_synchronize(s.p)
                    t0 = time.perf_counter()
                    for _ in range(k):
                        lnl = step()
                    if pending is not None:
                        unstored = int(pending(s.p))
                    for fn in after:
                        fn()
                    lib.pll_gpu_synchronize(s.p)
                    dt = time.perf_counter() - t0
                    if r >= args.warmup:
                        times.append(dt * 1e6)
                out[name] = {"min": round(min(times), 1), "median": round(statistics.median(times), 1), "max": round(max(times), 1),
                             "pending_after_steps": unstored}
        out["lnl"] = lnl
    print(json.dumps(out))


if __name__ == "__main__":
    main()
