#!/usr/bin/env python3
"""Write tests/golden/sankoff.json from the REFERENCE build (oracle/_ref/libpll_ref.so, made by `make -C oracle ref`
where the reference sources are present).

For every case of pllamd/sankoff_cases.py and every cost matrix it is run under, the reference's pll_parsimony_create /
pll_set_parsimony_sequence / build / reconstruct are run and recorded: the fields after create, the CRC-32 of every tip
buffer, the build score (hex float) and the CRC-32 of every inner node's score buffer, the CRC-32 of every inner node's
anc_states, and the score (hex float) of inserting the last tip into every edge of a seeded random tree over the other
tips - pll_parsimony_build({{t1, a, b}, {t2, t1, node}}, 2) with two spare buffers. Recorded results only; the file
regenerates bit-identically.

    python tools/gen_sankoff_golden.py            # rewrite the file
    python tools/gen_sankoff_golden.py --check    # compare with the file, exit 1 on any difference
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libpll-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from pllamd import api, sankoff_cases as SC  # noqa: E402
from sankoff_common import insertion_tree, session  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sankoff.json")


def record(lib, case, matrix_name):
    seqs, cmap = SC.alignment(case), SC.charmap(lib, case.states)
    ops, root = SC.tree_ops(case)
    with session(lib, case, matrix_name) as s:
        st = s.s
        rec = {"fields": [int(x) for x in (st.tips, st.states, st.sites, st.score_buffers, st.ancestral_buffers, st.inner_nodes, st.attributes,
                                           st.packedvector_count, st.const_cost, st.informative_count)]}
        for t, seq in enumerate(seqs):
            assert s.set_sequence(t, cmap, seq) == 1
        rec["tip_crc"] = [SC.crc(s.buffer(t), "<f8") for t in range(case.tips)]
        rec["score"] = s.build(ops).hex()
        s.sync()
        rec["buffer_crc"] = {str(p): SC.crc(s.buffer(p), "<f8") for p, _, _ in ops}
        s.reconstruct(cmap, SC.reconstruct_ops(ops, root, case.tips))
        rec["anc_crc"] = {str(p): SC.crc(s.ancestral(p), "<u4") for p, _, _ in ops}
        dops, edges = insertion_tree(case)
        s.build(dops)
        rec["insertion_scores"] = [float(x).hex() for x in s.insertion_scores_per_edge(case.tips - 1, edges, case.spare)]
    return rec


def generate(lib):
    return {case.name: {m: record(lib, case, m) for m in case.matrices} for case in SC.CASES}


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
        print("sankoff.json:", "identical" if same else "DIFFERENT")
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print(f"wrote {OUT} ({len(text)} bytes)")


if __name__ == "__main__":
    main()
