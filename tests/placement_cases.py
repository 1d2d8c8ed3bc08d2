"""What the placement tests share - TEST INFRASTRUCTURE on top of insertion_cases: the inputs of a case (a Layout with
`extra` query tips), the expected [query][candidate] matrix from the reference, computed once per case and shared, and
the cutting rule of pll_gpu_placement_loglikelihoods restated from include/pll_amd_device.h."""
import functools
import os
import re

import numpy as np

import insertion_cases as IC
from pllamd import driver

# the rule's constants as include/pll_amd_device.h defines them
_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pll_amd_device.h")).read()
_define = lambda name: eval(re.search(r"#define %s +(.+)" % name, _HDR).group(1).replace("u", ""))
CHUNK_DNA, CHUNK_TILED = _define("PLLGPU_PLACEMENT_CHUNK_DNA"), _define("PLLGPU_PLACEMENT_CHUNK_TILED")
MAX_CANDS, MAX_SLOTS = _define("PLLGPU_INSERTION_MAX_CANDS"), _define("PLLGPU_INSERTION_MAX_SLOTS")


def launches(states, rate_cats, sites, queries, count):
    """the header's rule: B workgroups per pair, C candidates and Q queries per launch"""
    tiles = -(-sites // 64)
    if states == 4 and rate_cats == 4:
        w = -(-tiles // 4096)
        blocks, chunk = -(-tiles // (4 * w)), CHUNK_DNA
    else:
        w = -(-tiles // 1024)
        blocks, chunk = -(-tiles // w), CHUNK_TILED
    if queries == 1:  # the insertion call's own cut
        return -(-count // min(count, MAX_CANDS, max(1, MAX_SLOTS // blocks)))
    c = min(count, MAX_CANDS, max(1, MAX_SLOTS // (blocks * chunk)))
    q = min(queries, chunk * min(65535, max(1, (MAX_SLOTS // (blocks * c)) // chunk)))
    return -(-count // c) * -(-queries // q)


@functools.lru_cache(maxsize=None)
def case(states, rate_cats, taxa, sites, extra):
    return IC.make(states, taxa, sites, rate_cats, extra=extra)


def bed(lib, dims, attrs, extra, **kw):
    states, rate_cats, taxa, sites = dims
    lay, seqs, cmap, exch, freqs = case(states, rate_cats, taxa, sites, extra)
    return IC.Bed(lib, lay, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, **kw)


def sequences(dims, extra):
    states, rate_cats, taxa, sites = dims
    return case(states, rate_cats, taxa, sites, extra)[1]


def query(lay, tip):
    """tip as the subtree end of the existing call: no scaler, the pendant matrix"""
    return (tip, IC.NONE, lay.pm_pendant)


def placement(b, tips, rows):
    return driver.placement_loglikelihoods(b.lib, b.p, tips, b.lay.pm_pendant, rows, b.fi)


def extra_rows(lay, rows):
    """candidates no edge of a tree gives: both ends tips, a tip as child2 of an inner child1, and an end that is itself
    a query tip (the second extra tip)"""
    inner = next(r for r in rows if r[0] >= lay.tips and r[3] >= lay.tips)
    return [(0, IC.NONE, lay.half(0), 1, IC.NONE, lay.half(1)), (inner[0], inner[1], inner[2], 2, IC.NONE, lay.half(2)),
            (lay.T + 1, IC.NONE, lay.half(3), inner[3], inner[4], inner[5])]


def reference(ref, dims, attrs, extra, offsets, more_rows=False, kw=()):
    """(expected [len(offsets)][candidates] from the reference: per query tip lay.T + offset the per-edge path over
    every edge; whether each candidate's inserted node rescales on its own). Cached per case."""
    return _reference(id(ref), dims, attrs, extra, tuple(offsets), more_rows, kw, _lib=ref)


_CACHE = {}


def _reference(key, dims, attrs, extra, offsets, more_rows, kw, _lib):
    k = (key, dims, attrs, extra, offsets, more_rows, kw)
    if k not in _CACHE:
        with bed(_lib, dims, attrs, extra, **dict(kw)) as b:
            rows = b.prepare()
            if more_rows:
                rows = rows + extra_rows(b.lay, rows)
            own = []
            exp = np.stack([b.per_edge(query(b.lay, b.lay.T + q), rows, own if i == 0 else None) for i, q in enumerate(offsets)])
        exp.setflags(write=False)
        _CACHE[k] = (exp, tuple(own))
    return _CACHE[k]
