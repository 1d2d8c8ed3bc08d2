"""Child process of tests/test_gpu_nj.py: pll_gpu_nj_tree on nj_cases.noisy(9) under both flags, with whatever
PLL_AMD_NJ_ROWS the parent put into the environment (the variable is read when a call starts; a fresh process keeps the
parent's own environment out of it). Prints one JSON line: per flag the bytes of parent and length in hex and the launches."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libpll-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nj_cases as NC  # noqa: E402
from pllamd import api, driver  # noqa: E402


def main():
    lib = api.PllLib()
    out = {}
    for flag, bits in NC.FLAGS.items():
        parent, length = driver.nj_tree(lib, NC.noisy(9), bits)
        out[flag] = [parent.tobytes().hex(), length.tobytes().hex(), int(lib.pll_gpu_nj_last_launch_count())]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
