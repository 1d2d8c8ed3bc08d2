"""What scoring an SPR neighbourhood costs: ONE pll_gpu_insertion_loglikelihoods call against the same candidates through
the per-edge path of the same library (pll_update_partials with one operation into a spare node +
pll_compute_edge_loglikelihood, per candidate) - profiles/insertion_scores.json.

Shapes: 64 taxa x 100k sites, DNA (4 states x 4 rates), and 64 taxa x 10k sites, 20 states x 4 rates; the tree and the
alignment come from seeds, nothing is read from disk. Candidates: for each of `--points` prune points the regraft edges
within `--radius` nodes (UTree.spr_targets). Per prune point, OUTSIDE both timed regions: a partial traversal towards
the pruned edge, the matrix of the edge that closes the gap, the half-length matrices of the candidate edges, and the
"upward" CLVs of the candidate edges in the pruned tree, into spare slots (one pll_update_partials list). Timed, host
clock around the synchronous calls, the two variants alternating, `--reps` repetitions after a warm-up: the batched
call over all candidates and over the first 8; the per-edge loop over the same lists (operation arrays built
beforehand: two library calls per candidate inside the clock). Every batched value is compared with the per-edge one.

Bytes, both ways, because re-reads served by a cache would flatter the figure: `distinct` = every CLV and scaler the
list names once; `per_candidate` = what each candidate reads, added up. Share of the 8 TB/s peak for each, from the
batched call's median (host clock: launch and wait included; the kernel's own durations come from a separate
`rocprofv3 --kernel-trace --stats` pass over `--reps 3 --no-json`).

Usage: python tools/insertion_scores_probe.py [--out profiles/insertion_scores.json] [--reps 20] [--points 20] [--radius 6]
                                               [--shapes dna,aa] [--no-json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "libpll-2_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from pllamd import api, workload as W  # noqa: E402
from utree import UTree  # noqa: E402

PEAK = 8.0e12
SHAPES = {"dna": dict(states=4, rate_cats=4, taxa=64, sites=100000), "aa": dict(states=20, rate_cats=4, taxa=64, sites=10000)}
NONE = api.SCALE_BUFFER_NONE


class Search:
    """a partition with spare slots for one neighbourhood at a time"""

    def __init__(self, lib, shape, seed):
        self.lib = lib
        s, r, t, n = shape["states"], shape["rate_cats"], shape["taxa"], shape["sites"]
        self.tree = UTree(t, np.random.Generator(np.random.PCG64(seed)))
        self.T, self.sites, self.states, self.rate_cats = t, n, s, r
        self.spare = 2 * t  # upward slots / half-length matrices of one neighbourhood at most
        self.up0, self.up_sc0 = t + (t - 2), t - 2
        self.tmp = (self.up0 + self.spare, self.up_sc0 + self.spare)
        self.pm_half0 = 2 * t - 3
        self.pm_joined = self.pm_half0 + self.spare
        buffers = (t - 2) + self.spare + 1
        self.p = lib.pll_partition_create(t, buffers, s, n, 1, self.pm_joined + 1, r, buffers, api.ARCH_AVX2)
        assert self.p, (lib.errno(), lib.errmsg())
        st = W.random_states(t, n, s, seed + 1, 15)
        if s == 4:
            seqs, cmap, exch, freqs = W.states_to_sequences(st, W.NT_CHARS), W.map_nt(), W.GTR_DNA["exch"], W.GTR_DNA["freqs"]
        else:
            ex, fr = W.synthetic_exch(s)
            seqs, cmap, exch, freqs = W.states_to_sequences(st, W.AA_CHARS), W.map_aa(), ex, fr
        lib.pll_set_frequencies(self.p, 0, api.dptr(np.ascontiguousarray(freqs, dtype=np.float64)))
        lib.pll_set_subst_params(self.p, 0, api.dptr(np.ascontiguousarray(exch, dtype=np.float64)))
        lib.pll_set_category_rates(self.p, api.dptr(np.ascontiguousarray(W.gamma_rates_mean(0.7, r), dtype=np.float64)))
        import ctypes as C
        cm = (C.c_ulonglong * 256)(*[int(x) for x in cmap])
        for i, q in enumerate(seqs):
            assert lib.pll_set_tip_states(self.p, i, cm, q)
        self.fi = np.zeros(r, dtype=np.uint32)
        self.matrices(self.tree.branches())

    def close(self):
        self.lib.pll_partition_destroy(self.p)

    def matrices(self, pairs):
        idx = np.ascontiguousarray([m for m, _ in pairs], dtype=np.uint32)
        bl = np.ascontiguousarray([x for _, x in pairs], dtype=np.float64)
        assert self.lib.pll_update_prob_matrices(self.p, api.uptr(self.fi), api.uptr(idx), api.dptr(bl), len(pairs))

    @staticmethod
    def end(r):
        return (r.clv, r.scaler) if r.inner else (r.clv, NONE)

    def neighbourhood(self, p, radius):
        """everything a caller prepares for the regraft edges around prune point p; returns (subtree end, candidate rows)"""
        tree = self.tree
        ops = tree.ops_for(p)  # every CLV now points towards the pruned edge
        u, v = p.next.back, p.next.next.back
        pairs = [(self.pm_joined, u.length + v.length)]
        up_ops, rows, n = [], [], 0
        # what lies beyond x.back, seen from x: (clv, scaler, matrix); the gap is closed by the joined edge
        todo = [(u, self.end(v) + (self.pm_joined,), 1), (v, self.end(u) + (self.pm_joined,), 1)]
        while todo:
            x, far, d = todo.pop()
            if not x.inner or d >= radius or n + 2 > self.spare:
                continue
            for q, sib in ((x.next, x.next.next), (x.next.next, x.next)):
                s = self.end(sib.back)
                clv, sc, half = self.up0 + n, self.up_sc0 + n, self.pm_half0 + n
                n += 1
                up_ops.append((clv, sc, far[0], far[2], far[1], s[0], sib.pm, s[1]))
                pairs.append((half, q.length / 2.0))
                a = self.end(q.back)
                rows.append((a[0], a[1], half, clv, sc, half))
                todo.append((q.back, (clv, sc, q.pm), d + 1))
        self.matrices(pairs)
        both = ops + up_ops
        if both:
            self.lib.pll_update_partials(self.p, api.make_ops(both), len(both))
        sub = self.end(p.back) + (p.pm,)
        return sub, rows

    def batched(self, sub, rows, arr, out):
        ok = self.lib.pll_gpu_insertion_loglikelihoods(self.p, sub[0], sub[1], sub[2], arr, len(rows), api.uptr(self.fi), api.dptr(out))
        assert ok, (self.lib.errno(), self.lib.errmsg())

    def per_edge(self, sub, op_arrays, out):
        lib, p, tmp, fi = self.lib, self.p, self.tmp, api.uptr(self.fi)
        for i, arr in enumerate(op_arrays):
            lib.pll_update_partials(p, arr, 1)
            out[i] = lib.pll_compute_edge_loglikelihood(p, tmp[0], tmp[1], sub[0], sub[1], sub[2], fi, None)

    def traffic(self, sub, rows):
        clv = ((self.sites + 63) // 64) * 64 * self.states * self.rate_cats * 8
        tip, sc = self.sites, self.sites * 4
        size = lambda node, scaler: (tip if node < self.T else clv) + (sc if scaler >= 0 and node >= self.T else 0)
        ends = [(r[0], r[1]) for r in rows] + [(r[3], r[4]) for r in rows]
        per_candidate = sum(size(*e) for e in ends) + len(rows) * size(sub[0], sub[1])
        distinct = sum(size(*e) for e in set(ends) | {(sub[0], sub[1])})
        return distinct, per_candidate


def measure(search, sub, rows, reps):
    arr = api.make_insertions(rows)
    ops = [api.make_ops([(search.tmp[0], search.tmp[1], c[0], c[2], c[1], c[3], c[5], c[4])]) for c in rows]
    got, exp = np.empty(len(rows)), np.empty(len(rows))
    tb, ts, launches = [], [], 0
    for rep in range(reps + 2):  # two warm-up rounds
        t0 = time.perf_counter()
        search.batched(sub, rows, arr, got)
        t1 = time.perf_counter()
        launches = int(search.lib.pll_gpu_last_launch_count(search.p))
        search.per_edge(sub, ops, exp)
        t2 = time.perf_counter()
        if rep >= 2:
            tb.append((t1 - t0) * 1e6)
            ts.append((t2 - t1) * 1e6)
    worst = float(np.max(np.abs(got - exp) / np.maximum(np.abs(exp), 1.0)))
    assert worst <= 1e-10, worst
    q = lambda x: dict(median=round(statistics.median(x), 2), min=round(min(x), 2), max=round(max(x), 2))
    return dict(candidates=len(rows), batched_us=q(tb), per_edge_us=q(ts), worst_rel_diff=worst,
                launches=launches)


def run_shape(lib, name, reps, points, radius, seed=31):
    search = Search(lib, SHAPES[name], seed)
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    tree = search.tree
    records = [r for n in tree.inner_nodes for r in (n, n.next, n.next.next)]
    out = []
    try:
        while len(out) < points:
            p = records[int(rng.integers(0, len(records)))]
            if len(tree.spr_targets(p, radius)) < 8:
                continue
            sub, rows = search.neighbourhood(p, radius)
            full = measure(search, sub, rows, reps)
            eight = measure(search, sub, rows[:8], reps)
            distinct, per_candidate = search.traffic(sub, rows)
            sec = full["batched_us"]["median"] * 1e-6
            full.update(bytes_distinct=distinct, bytes_per_candidate=per_candidate,
                        share_of_peak_distinct=round(distinct / sec / PEAK, 4), share_of_peak_per_candidate=round(per_candidate / sec / PEAK, 4))
            out.append(dict(all=full, first_8=eight))
            print(f"{name} point {len(out)}: {full['candidates']} candidates, batched {full['batched_us']['median']} us, "
                  f"per edge {full['per_edge_us']['median']} us; first 8: {eight['batched_us']['median']} vs {eight['per_edge_us']['median']} us", flush=True)
    finally:
        search.close()
    med = lambda f: round(statistics.median(f(x) for x in out), 3)
    return dict(shape=SHAPES[name], points=out, summary=dict(
        candidates_median=med(lambda x: x["all"]["candidates"]),
        us_per_candidate_batched=med(lambda x: x["all"]["batched_us"]["median"] / x["all"]["candidates"]),
        us_per_candidate_per_edge=med(lambda x: x["all"]["per_edge_us"]["median"] / x["all"]["candidates"]),
        us_per_candidate_batched_at_8=med(lambda x: x["first_8"]["batched_us"]["median"] / 8),
        us_per_candidate_per_edge_at_8=med(lambda x: x["first_8"]["per_edge_us"]["median"] / 8),
        share_of_peak_distinct=med(lambda x: x["all"]["share_of_peak_distinct"]),
        share_of_peak_per_candidate=med(lambda x: x["all"]["share_of_peak_per_candidate"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "insertion_scores.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=20)
    ap.add_argument("--radius", type=int, default=6)
    ap.add_argument("--shapes", default="dna,aa")
    ap.add_argument("--no-json", action="store_true")
    a = ap.parse_args()
    lib = api.PllLib()
    assert lib.pll_gpu_available(), "no MI355X visible"
    res = {"what": __doc__.split("\n\n")[0].replace("\n", " "), "reps": a.reps, "radius": a.radius, "peak_bytes_per_s": PEAK,
           "clock": "host clock around the synchronous calls, batched and per-edge alternating; medians, min, max in us"}
    for name in a.shapes.split(","):
        res[name] = run_shape(lib, name, a.reps, a.points, a.radius)
        print(name, json.dumps(res[name]["summary"]), flush=True)
    if not a.no_json:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
