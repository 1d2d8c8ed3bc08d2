"""Child process of tests/test_gpu_bootstrap_trees.py: pll_gpu_bootstrap_distance_trees with whatever
PLL_AMD_BOOTSTRAP_BYTES / PLL_AMD_DISTANCE_PAIRS the parent put into the environment (both are read when the partition's
device context is made; a fresh process keeps the parent's own environment out of it). Also the home of the beds both
sides build.

Arguments shape:flag, ...: rows FIRST .. FIRST + REPLICATES - 1 of SEED on bed(shape); one JSON line, per argument the bytes
of every output in hex and the launches of the call (the first on its partition: the prefix sums are formed)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libpll-2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import distance_cases as DC  # noqa: E402
import nj_cases as NC  # noqa: E402

SEED, FIRST, REPLICATES = 20240607, 3, 5
OUTPUTS = ("parent", "length", "distances", "status", "weights")

# name -> (states, rate categories, tips, sites, pattern weights). 1029 sites: rows of 1032 words on the device, and the
# four-sites-per-thread loop of the distance kernel has a tail of one site.
SHAPES = {"dna": (4, 4, 9, 1029, "mixed"), "dna-ones": (4, 4, 9, 1029, None), "aa": (20, 4, 6, 203, "mixed"), "codon": (61, 4, 4, 64, "mixed")}


def pattern_weights(kind, sites):
    """zeros, small weights and one large one (the general draw), or None: all ones (the draw's short cut)"""
    if kind is None:
        return None
    w = np.arange(sites, dtype=np.uint32) % 3
    w[5] = 400
    return w


def bed(lib, shape, **kw):
    states, rate_cats, tips, sites, kind = SHAPES[shape]
    seqs, cmap, exch, freqs = DC.sequences(states, tips, sites)
    return DC.Tips(lib, states, rate_cats, seqs, cmap, exch, freqs, pattern_weights=pattern_weights(kind, sites), **kw)


def options(shape):
    from pllamd import driver

    return driver.newton_options(0.1, 1e-6, 100.0, 1e-8 * SHAPES[shape][3], 32)


def main(items):
    from pllamd import api

    lib = api.PllLib()
    out = {}
    for item in items:
        shape, flag = item.split(":")
        with bed(lib, shape) as b:
            got = api.bootstrap_distance_trees(lib, b.p, range(b.tips), b.pi, options(shape), NC.FLAGS[flag], SEED, FIRST, REPLICATES)
            out[item] = [got[name].tobytes().hex() for name in OUTPUTS] + [b.launches()]
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1:])
