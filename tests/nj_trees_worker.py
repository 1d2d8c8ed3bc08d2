"""Child process of tests/test_gpu_nj_trees.py: pll_gpu_nj_trees with whatever PLL_AMD_NJ_ROWS / PLL_AMD_NJ_BATCH_BYTES the
parent put into the environment (both are read when a call starts; a fresh process keeps the parent's own environment out
of it). Also the home of the batches both sides build.

Arguments n:replicates:flag, ...: batch(n, replicates) under nj_cases.FLAGS[flag]; one JSON line, per argument the bytes of
parent and length in hex and the launches."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libpll-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nj_cases as NC  # noqa: E402


def permuted(matrix, seed):
    """the same distances under other labels: another order of joins over the slots"""
    perm = np.random.default_rng(seed).permutation(len(matrix))
    return matrix[np.ix_(perm, perm)]


def batch(n, replicates):
    """[replicates, n, n]: noisy and additive matrices by turns, from the third on under permuted labels - no two alike, so
    the replicates of a batch join different slots at every step"""
    kinds = (NC.noisy, NC.additive)
    return np.stack([kinds[b % 2](n) if b < 2 else permuted(kinds[b % 2](n), 10 * n + b) for b in range(replicates)])


def main(items):
    from pllamd import api

    lib = api.PllLib()
    out = {}
    for item in items:
        n, replicates, flag = item.split(":")
        parent, length = api.nj_trees(lib, batch(int(n), int(replicates)), NC.FLAGS[flag])
        out[item] = [parent.tobytes().hex(), length.tobytes().hex(), int(lib.pll_gpu_nj_last_launch_count())]
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
