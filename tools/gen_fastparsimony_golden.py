#!/usr/bin/env python3
"""Write tests/golden/fastparsimony.json from the REFERENCE build (oracle/_ref/libpll_ref.so, made by `make -C oracle
ref` where the reference sources are present).

For every case of pllamd/parsimony_cases.py and every attribute set the tests cover, the reference's
pll_fastparsimony_init / update_vectors / edge_score / root_score are run and recorded: the init fields, every node
cost after the traversal, a CRC-32 of every packed vector, the edge and root scores, and the scores of inserting the last
tip into every edge of a seeded random tree over the other tips (update_vector into a spare index followed by
edge_score, src/stepwise.c:507-512). Integers only; the file regenerates bit-identically.

    python tools/gen_fastparsimony_golden.py            # rewrite the file
    python tools/gen_fastparsimony_golden.py --check    # compare with the file, exit 1 on any difference
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libpll-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pllamd import api, driver, parsimony_cases as PC  # noqa: E402
from utree import UTree  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fastparsimony.json")
# the attribute sets the issue lists as giving identical scores on the reference; only packedvector_count differs
EXTRA_SETS = [("sse_tip", api.ARCH_SSE | api.PATTERN_TIP), ("avx_tip", api.ARCH_AVX | api.PATTERN_TIP), ("avx2_clv", api.ARCH_AVX2)]


def insertion_tree(case):
    """seeded random tree over tips 0 .. tips-2 (None below four of them)"""
    if case.tips - 1 < 4:
        return None
    return UTree(case.tips - 1, np.random.default_rng(case.seed + 1000))


def record(lib, case, attrs):
    seqs, weights = PC.alignment(case)
    ops, edge = PC.traversal(case)
    with driver.ParsimonySession(lib, case.states, seqs, PC.charmap(lib, case), weights, attrs) as s:
        rec = {
            "packedvector_count": int(s.s.packedvector_count),
            "const_cost": int(s.s.const_cost),
            "informative_count": int(s.s.informative_count),
            "informative": PC.informative_string(s.informative()),
            "tip_crc": [PC.crc(s.vector(t)) for t in range(case.tips)],
        }
        s.update(ops)
        written = sorted({o[0] for o in ops})
        rec["node_cost"] = [int(x) for x in s.costs()[:case.tips + len(ops)]]
        rec["vector_crc"] = {str(n): PC.crc(s.vector(n)) for n in written}
        rec["edge_score"] = s.edge_score(*edge)
        rec["root_score"] = s.root_score(edge[0])
        tree = insertion_tree(case)
        if tree is None:
            rec["insertion_scores"] = []
        else:
            dops, edges = PC.directional_ops(tree, case.tips)
            s.update(dops)
            rec["insertion_scores"] = [int(x) for x in s.insertion_scores_per_edge(case.tips - 1, edges, case.nodes - 1)]
    return rec


def generate(lib):
    out = {}
    for case in PC.CASES:
        sets = PC.attribute_sets(case)
        entry = {label: record(lib, case, attrs) for label, attrs in sets}
        # scores do not depend on the attribute set: assert it here, on the reference, once
        for label, attrs in EXTRA_SETS:
            if case.pattern_tip_only and not attrs & api.PATTERN_TIP:
                continue
            other = record(lib, case, attrs)
            for key in ("const_cost", "informative", "node_cost", "edge_score", "root_score", "insertion_scores"):
                assert other[key] == entry["tip"][key], (case.name, label, key)
        for label, _ in sets[1:]:
            for key in ("const_cost", "informative", "node_cost", "edge_score", "root_score", "insertion_scores"):
                assert entry[label][key] == entry["tip"][key], (case.name, label, key)
        out[case.name] = entry
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    ref = os.path.join(ROOT, "oracle", "_ref", "libpll_ref.so")
    if not os.path.exists(ref):
        sys.exit(f"{ref} not built: the golden file comes from the reference alone")
    text = json.dumps(generate(api.PllLib(ref)), indent=0, sort_keys=True, separators=(",", ":")) + "\n"
    if args.check:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("fastparsimony.json:", "identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT} ({len(text)} bytes)")


if __name__ == "__main__":
    main()
