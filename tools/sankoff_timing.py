"""What weighted (Sankoff) parsimony costs on the device against the reference's pll_parsimony_build on one core of the
same host (profiles/sankoff_scores.json). Shapes: 64 taxa x 100 000 DNA sites and 64 taxa x 20 000 sites at 20 states,
both under the `unit` matrix; a 65th sequence is the taxon that gets inserted.

Per shape, one child process per library, each under its own `timeout`:
  (a) one pll_parsimony_build of a random rooted tree over the 64 taxa (63 operations) - its score included;
  (b) the scores of inserting the 65th taxon into all 125 edges of a random unrooted tree over the 64: ONE
      pll_gpu_parsimony_insertion_scores call; on the reference - and, for comparison, on the device - the pattern the
      call is defined by, pll_parsimony_build({{t1, a, b}, {t2, t1, node}}, 2) per edge.
Times are host-clock medians over `--rounds` rounds; every timed call is synchronous. Bytes are what the launches have to
move by construction (two child buffers read and one parent written per operation; three buffers read per candidate),
quoted against the HBM peak.

Usage: python tools/sankoff_timing.py [--out profiles/sankoff_scores.json] [--rounds 5] [--shapes a,b]"""
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
from pllamd import api, driver, parsimony_cases as PC, sankoff_cases as SC, workload as W  # noqa: E402
from utree import UTree  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X data sheet
TAXA = 64
SHAPES = {
    "dna_64x100k": dict(states=4, sites=100000),
    "aa_64x20k": dict(states=20, sites=20000),
}


def step(name, which, rounds):
    shape = SHAPES[name]
    gpu = which == "gpu"
    lib = api.PllLib() if gpu else api.PllLib(os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so"))
    states, sites = shape["states"], shape["sites"]
    case = SC.SankoffCase(name, TAXA + 1, sites, states)
    cmap = SC.charmap(lib, states)
    seqs = W.states_to_sequences(W.random_states(TAXA + 1, sites, states, SC.ALIGNMENT_SEED, SC.MUTATE_PCT), SC.symbols(states))
    ops, root = SC.random_join_ops(range(TAXA), TAXA + 1, 5)
    dops, edges = PC.directional_ops(UTree(TAXA, np.random.default_rng(6)), case.insertion_base)
    assert len(ops) == TAXA - 1 and len(edges) == 2 * TAXA - 3
    t0 = time.perf_counter()
    s = driver.SankoffSession(lib, case.tips, states, sites, SC.matrix("unit", states), case.score_buffers, 0)
    try:
        for t, seq in enumerate(seqs):
            assert s.set_sequence(t, cmap, seq) == 1
        setup_s = time.perf_counter() - t0
        us = lambda t, n: (time.perf_counter() - t) * 1e6 / n
        res = {"a_build_plus_score": [], "b_insertion_per_edge_all_edges": []}
        if gpu:
            res["b_insertion_batched_all_edges"] = []
        score = s.build(ops)  # warm: code objects, argument blocks, the tips' upload
        s.build(dops)
        for _ in range(rounds):
            n = 5 if gpu else 1
            t = time.perf_counter()
            for _i in range(n):
                assert s.build(ops) == score
            res["a_build_plus_score"].append(us(t, n))
            t = time.perf_counter()
            per_edge = s.insertion_scores_per_edge(TAXA, edges, case.spare)
            res["b_insertion_per_edge_all_edges"].append(us(t, 1))
            if gpu:
                t = time.perf_counter()
                for _i in range(n):
                    batched = s.insertion_scores(TAXA, edges)
                res["b_insertion_batched_all_edges"].append(us(t, n))
                assert s.launches() == 1 and (batched == per_edge).all()  # `unit`: integers, no rounding anywhere
        buffer_bytes = -(-sites // 64) * 64 * states * 8
        med = lambda v: round(statistics.median(v), 2)
        out = {"library": "libpll_amd.so on one MI355X" if gpu else "reference, one core", "taxa": TAXA, "states": states, "sites": sites,
               "matrix": "unit", "build_ops": len(ops), "build_levels": SC.levels(ops), "edges_scored": len(edges),
               "setup_s_create_and_tips": round(setup_s, 2), "score_of_the_build": score, "insertion_scores_crc": SC.crc(per_edge, "<f8"),
               "us": {k: {"median": med(v), "min": round(min(v), 2)} for k, v in res.items()}}
        if gpu:
            build_bytes, ins_bytes = 3 * len(ops) * buffer_bytes, 3 * len(edges) * buffer_bytes
            out["bytes"] = {
                "score_buffer": buffer_bytes, "build_all_launches": build_bytes, "build_per_launch_mean": build_bytes // SC.levels(ops),
                "insertion_one_launch": ins_bytes,
                "build_fraction_of_hbm_peak": round(build_bytes / (min(res["a_build_plus_score"]) * 1e-6) / HBM_PEAK_BYTES_PER_S, 4),
                "insertion_fraction_of_hbm_peak": round(ins_bytes / (min(res["b_insertion_batched_all_edges"]) * 1e-6) / HBM_PEAK_BYTES_PER_S, 4),
                "note": "host clock over whole synchronous calls: launch overhead, the score launch and the copy back included"}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sankoff_scores.json"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--step", nargs=2, metavar=("SHAPE", "gpu|ref"))
    ap.add_argument("--no-reference", action="store_true")
    a = ap.parse_args()
    if a.step:
        return step(a.step[0], a.step[1], a.rounds)
    have_ref = not a.no_reference and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so"))
    result = {"what": "weighted parsimony: one build + score, and all insertion edges in one call; tools/sankoff_timing.py",
              "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S, "shapes": {}}
    for name in a.shapes.split(","):
        entry = {"gpu": child(["--step", name, "gpu", "--rounds", str(a.rounds)], 300)}
        if have_ref:
            entry["reference"] = child(["--step", name, "ref", "--rounds", str(max(1, a.rounds // 2))], 400)
            g, r = entry["gpu"], entry["reference"]
            assert g["score_of_the_build"] == r["score_of_the_build"] and g["insertion_scores_crc"] == r["insertion_scores_crc"]
            entry["reference_over_gpu"] = {
                "a_build_plus_score": round(r["us"]["a_build_plus_score"]["median"] / g["us"]["a_build_plus_score"]["median"], 1),
                "b_per_edge_reference_over_batched_gpu": round(
                    r["us"]["b_insertion_per_edge_all_edges"]["median"] / g["us"]["b_insertion_batched_all_edges"]["median"], 1),
                "b_per_edge_reference_over_per_edge_gpu": round(
                    r["us"]["b_insertion_per_edge_all_edges"]["median"] / g["us"]["b_insertion_per_edge_all_edges"]["median"], 1),
            }
        result["shapes"][name] = entry
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # after every shape: a later step that ends early loses nothing
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result["shapes"], indent=1))


if __name__ == "__main__":
    main()
