"""Child process of tests/test_gpu_nj.py: pll_gpu_nj_tree with whatever PLL_AMD_NJ_ROWS the parent put into the environment
(the variable is read when a call starts; a fresh process keeps the parent's own environment out of it).

Without arguments: nj_cases.noisy(9) under both flags; one JSON line: per flag the bytes of parent and length in hex and the
launches. With arguments kind:n:flag (nj_cases.MATRICES[kind](n) under nj_cases.FLAGS[flag]), the runs of the list: one JSON
line, per argument the same three."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libpll-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nj_cases as NC  # noqa: E402
from pllamd import api, driver  # noqa: E402


def main(items):
    lib = api.PllLib()
    out = {}
    runs = [(item,) + tuple(item.split(":")) for item in items] or [(flag, "noisy", "9", flag) for flag in NC.FLAGS]
    for key, kind, n, flag in runs:
        parent, length = driver.nj_tree(lib, NC.MATRICES[kind](int(n)), NC.FLAGS[flag])
        out[key] = [parent.tobytes().hex(), length.tobytes().hex(), int(lib.pll_gpu_nj_last_launch_count())]
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
