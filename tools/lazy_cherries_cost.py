#!/usr/bin/env python3
"""The paying case of lazy cherries (profiles/dna_tree_lazy_cherries.md): what a caller who DOES read a tip x tip parent
right after a step pays for the launch that stores the 32 of them on demand - and what the callers who do not read one
but change matrices between two steps pay (nothing but one small copy of the matrices the cherries read).

Times, on the flagship shape (4 states, 4 rates, 64-taxon balanced tree), per repetition and between two waits for the
stream:
  step              pll_update_partials (full traversal) + pll_compute_edge_loglikelihood at the root edge
  step+read         ... + pll_gpu_sync_clv of one cherry parent (a download of sites x 128 B)
  step+derivatives  ... + pll_update_sumtable and pll_compute_likelihood_derivatives at an edge between two cherry parents
  matrices+step     pll_update_prob_matrices of every matrix, then the step: one round of a model-parameter loop
  step+matrix+edge  the step, pll_update_prob_matrices of the root edge's matrix, the root edge again: a branch-length move
and prints one JSON line. --root names the tree whose library is measured (a clean export of another commit, built),
default this one; PLL_AMD_LAZY_CHERRIES=0/1 selects the form where the library knows the switch."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--sites", type=int, default=100000)
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
    cherries = [op for op in case.op_batches[0] if op[2] < case.tips and op[5] < case.tips]
    a, b = cherries[0], cherries[1]
    cherry_edge = (a[0], a[1], b[0], b[1])
    pending = getattr(lib, "pll_gpu_pending_clvs", None)
    with driver.Session(lib, case, api.ARCH_AVX2) as s:
        s.set_model(case.model["exch"], case.freqs, case.model["rates"])
        st = s.new_sumtable()

        def step():
            s.update_partials()
            return s.edge_lnl(e, persite=False)[0]

        def read():
            if not lib.pll_gpu_sync_clv(s.p, a[0]):
                raise SystemExit(f"pll_gpu_sync_clv: {lib.errmsg()}")

        def derivatives():
            s.update_sumtable(cherry_edge, st)
            return s.derivatives(cherry_edge, st, 0.13)

        nmat = case.prob_matrices
        pi = np.zeros(case.rate_cats, dtype=np.uint32)
        every = np.arange(nmat, dtype=np.uint32)
        brlen = np.ascontiguousarray(W.branch_lengths(nmat))
        one, one_len = np.array([e[4]], dtype=np.uint32), np.array([brlen[e[4]]])

        def matrices(idx=every, bl=brlen):
            if not lib.pll_update_prob_matrices(s.p, api.uptr(pi), api.uptr(idx), api.dptr(bl), len(idx)):
                raise SystemExit(f"pll_update_prob_matrices: {lib.errmsg()}")

        def matrix_and_edge():
            matrices(one, one_len)
            return s.edge_lnl(e, persite=False)[0]

        matrices()
        legs = {"step": ((), ()), "step+read": ((), (read,)), "step+derivatives": ((), (derivatives,)),
                "matrices+step": ((matrices,), ()), "step+matrix+edge": ((), (matrix_and_edge,))}
        out = {"root": os.path.abspath(args.root), "sites": args.sites, "reps": args.reps,
               "lazy_cherries": os.environ.get("PLL_AMD_LAZY_CHERRIES", "default"), "unit": "us"}
        for name, (before, after) in legs.items():
            times = []
            for r in range(args.warmup + args.reps):
                lib.pll_gpu_synchronize(s.p)
                t0 = time.perf_counter()
                for fn in before:
                    fn()
                lnl = step()
                for fn in after:
                    last = fn()
                lib.pll_gpu_synchronize(s.p)
                dt = time.perf_counter() - t0
                if r >= args.warmup:
                    times.append(dt * 1e6)
            out[name] = {"min": round(min(times), 1), "median": round(statistics.median(times), 1), "max": round(max(times), 1)}
            if after and after[0] is derivatives:
                out["derivatives"] = list(last)
        out["lnl"] = lnl
        if pending is not None:
            step()
            out["pending_after_step"] = int(pending(s.p))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
