"""What the fast-parsimony entry points cost, call for call and batched, against the reference's AVX2 path on one core of
the same host (profiles/fastparsimony.json). Shapes: DNA, 64 and 128 taxa x 100k and 1M sites, and 20 states, 64 taxa x
50k sites; seeded alignments with a mutation rate of 0.6, so nearly every site is informative (the counts are recorded).

Per shape, one child process per library, each under its own `timeout`:
  (a) one pll_fastparsimony_update_vector + one pll_fastparsimony_edge_score, call by call;
  (b) a full traversal: pll_fastparsimony_update_vectors over the tips-2 operations towards one edge + its edge score;
  (c) the scores of inserting one taxon into every edge of a tree over the other taxa: ONE
      pll_gpu_fastparsimony_insertion_scores call, and the per-edge pattern update_vector + edge_score
      (src/stepwise.c:507-512) - on the reference only the latter exists;
  and, GPU only, the update kernel's rate: a level of tips/2 independent cherries as one launch, `reps` launches
  between two synchronisations, bytes = 3 x states x words x 4 per operation, against the bare store stream of
  profiles/r6_store_ceiling.txt.
Times are host-clock medians over `--rounds` rounds; every timed GPU section ends in a synchronisation (a score is
one; updates are followed by pll_gpu_synchronize_parsimony).

Usage: python tools/fastparsimony_timing.py [--out profiles/fastparsimony.json] [--rounds 5] [--shapes a,b]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "libpll-2_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
from pllamd import api, driver, parsimony_cases as PC  # noqa: E402
from utree import UTree  # noqa: E402

STORE_CEILING_BYTES_PER_S = 6.92e12  # profiles/r6_store_ceiling.txt: a bare store stream on one MI355X
SHAPES = {
    "dna_64x100k": dict(states=4, tips=64, sites=100000),
    "dna_128x100k": dict(states=4, tips=128, sites=100000),
    "dna_64x1m": dict(states=4, tips=64, sites=1000000),
    "dna_128x1m": dict(states=4, tips=128, sites=1000000),
    "aa_64x50k": dict(states=20, tips=64, sites=50000),
}


def sequences(shape, seed=21):
    """one ancestral state per site, a tip copies it unless a draw falls below 0.6 (bytes, not doubles: 128 x 1M)"""
    rng = np.random.default_rng(seed)
    sym = np.frombuffer(PC.NT if shape["states"] == 4 else PC.AA, dtype=np.uint8)
    tips, sites, states = shape["tips"], shape["sites"], shape["states"]
    ancestral = rng.integers(0, states, size=sites, dtype=np.uint8)
    out = []
    for _ in range(tips):
        mutate = rng.integers(0, 256, size=sites, dtype=np.uint8) < 154
        drawn = rng.integers(0, states, size=sites, dtype=np.uint8)
        out.append(sym[np.where(mutate, drawn, ancestral)].tobytes())
    return out


def step(name, which, rounds):
    shape = SHAPES[name]
    gpu = which == "gpu"
    lib = api.PllLib() if gpu else api.PllLib(os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so"))
    tips, states = shape["tips"], shape["states"]
    cmap = np.array(lib.state_map("pll_map_nt" if states == 4 else "pll_map_aa"), dtype=np.uint64)
    t0 = time.perf_counter()
    s = driver.ParsimonySession(lib, states, sequences(shape), cmap, None, api.PATTERN_TIP | api.ARCH_AVX2)
    setup_s = time.perf_counter() - t0
    try:
        s.drop_partition()
        nodes, words = s.nodes, s.words
        full = UTree(tips, np.random.default_rng(5))
        trav, trav_edge = PC.postorder_ops(full, full.tip_recs[0], tips)
        sub = UTree(tips - 1, np.random.default_rng(6))
        dops, edges = PC.directional_ops(sub, tips)
        node, spare = tips - 1, nodes - 1
        sync = (lambda: lib.pll_gpu_synchronize_parsimony(s.pars)) if gpu else (lambda: 1)
        us = lambda t, n: (time.perf_counter() - t) * 1e6 / n
        trav_arr, one = api.make_pars_ops(trav), api.make_pars_ops([(spare, 0, 1)])
        cherries = api.make_pars_ops([(tips + i, 2 * i, 2 * i + 1) for i in range(tips // 2)])
        big = words >= 10000
        res = {k: [] for k in ("a_update_plus_edge_score", "b_full_traversal_plus_edge_score", "c_insertion_per_edge_all_edges")}
        if gpu:
            res.update({"c_insertion_batched_all_edges": [], "level_of_cherries_one_launch": [], "single_update_async": []})
        s.update(trav)
        s.edge_score(*trav_edge)  # warm: code objects, argument blocks
        for _ in range(rounds):
            n = 100 if big else 300
            t = time.perf_counter()
            for _i in range(n):
                lib.pll_fastparsimony_update_vector(s.pars, one)
                lib.pll_fastparsimony_edge_score(s.pars, spare, 2)
            res["a_update_plus_edge_score"].append(us(t, n))
            n = 10 if big else 30
            t = time.perf_counter()
            for _i in range(n):
                lib.pll_fastparsimony_update_vectors(s.pars, trav_arr, len(trav))
                lib.pll_fastparsimony_edge_score(s.pars, *trav_edge)
            res["b_full_traversal_plus_edge_score"].append(us(t, n))
            s.update(dops)
            sync()
            t = time.perf_counter()
            per_edge = s.insertion_scores_per_edge(node, edges, spare)
            res["c_insertion_per_edge_all_edges"].append(us(t, 1))
            if gpu:
                n = 10 if big else 30
                t = time.perf_counter()
                for _i in range(n):
                    batched = s.insertion_scores(node, edges)
                res["c_insertion_batched_all_edges"].append(us(t, n))
                assert (batched == per_edge).all()
                n = 20 if big else 100
                sync()
                t = time.perf_counter()
                for _i in range(n):
                    lib.pll_fastparsimony_update_vectors(s.pars, cherries, tips // 2)
                sync()
                res["level_of_cherries_one_launch"].append(us(t, n))
                assert lib.pll_gpu_fastparsimony_last_launch_count(s.pars) == 1
                t = time.perf_counter()
                for _i in range(n):
                    lib.pll_fastparsimony_update_vector(s.pars, one)
                sync()
                res["single_update_async"].append(us(t, n))
        med = lambda v: round(statistics.median(v), 2)
        out = {"library": "libpll_amd.so on one MI355X" if gpu else "reference, AVX2, one core", "tips": tips, "states": states,
               "sites": shape["sites"], "informative_sites": int(s.s.informative_count), "packedvector_count": int(words),
               "bytes_per_operation": 3 * states * words * 4, "edges_scored": len(edges), "traversal_ops": len(trav),
               "setup_s_partition_tips_and_init": round(setup_s, 2),
               "us": {k: {"median": med(v), "min": round(min(v), 2)} for k, v in res.items()},
               "score_of_the_traversal": s.edge_score(*trav_edge), "insertion_scores_crc": PC.crc(per_edge)}
        if gpu:
            level_bytes = (tips // 2) * out["bytes_per_operation"]
            rate = level_bytes / (min(res["level_of_cherries_one_launch"]) * 1e-6)
            out["update_kernel"] = {"level_bytes": level_bytes, "bytes_per_s": round(rate, -6),
                                    "fraction_of_store_ceiling": round(rate / STORE_CEILING_BYTES_PER_S, 3),
                                    "note": "host clock over back-to-back launches of one level, launch overhead included"}
        print(json.dumps(out))
    finally:
        s.close()


def child(args, seconds):
    cmd = ["timeout", "-k", "10", str(seconds), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {args} ended with status {r.returncode}: nothing more is started")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastparsimony.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--step", nargs=2, metavar=("SHAPE", "gpu|ref"))
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    if a.step:
        return step(a.step[0], a.step[1], a.rounds)
    have_ref = not a.no_reference and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so"))
    result = {"what": "fast parsimony, call for call and batched; tools/fastparsimony_timing.py",
              "store_ceiling_bytes_per_s": STORE_CEILING_BYTES_PER_S, "shapes": {}}
    for name in a.shapes.split(","):
        entry = {"gpu": child(["--step", name, "gpu", "--rounds", str(a.rounds)], 300)}
        if have_ref:
            entry["reference"] = child(["--step", name, "ref", "--rounds", str(a.rounds)], 300)
            g, r = entry["gpu"], entry["reference"]
            assert g["score_of_the_traversal"] == r["score_of_the_traversal"] and g["insertion_scores_crc"] == r["insertion_scores_crc"]
            entry["reference_over_gpu"] = {
                "a_update_plus_edge_score": round(r["us"]["a_update_plus_edge_score"]["median"] / g["us"]["a_update_plus_edge_score"]["median"], 2),
                "b_full_traversal_plus_edge_score": round(r["us"]["b_full_traversal_plus_edge_score"]["median"] / g["us"]["b_full_traversal_plus_edge_score"]["median"], 2),
                "c_per_edge_reference_over_batched_gpu": round(r["us"]["c_insertion_per_edge_all_edges"]["median"] / g["us"]["c_insertion_batched_all_edges"]["median"], 2),
                "c_per_edge_reference_over_per_edge_gpu": round(r["us"]["c_insertion_per_edge_all_edges"]["median"] / g["us"]["c_insertion_per_edge_all_edges"]["median"], 2),
            }
        result["shapes"][name] = entry
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # after every shape: a later step that ends early loses nothing
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result["shapes"], indent=1))


if __name__ == "__main__":
    main()
