"""What the long-walk tests share - TEST INFRASTRUCTURE: the smallest site counts at which a wave (4 x 4) or a workgroup
(every other shape) of a batched call walks a second 64-site tile, the walk restated from the rule that
include/pll_amd_device.h states, and the inputs: UTree(5, PCG64(7)) through insertion_cases.make - 7 edges, 2 inner
edges, 2 extra tips - with the last site, the only site of the last tile, at pattern weight LAST_WEIGHT and every other
site at 1, in both libraries."""
import functools

import numpy as np

import insertion_cases as IC
from placement_cases import _define
from pllamd import api

QG_MAX_BLOCKS = _define("PLLGPU_QGRADIENT_MAX_BLOCKS")
TAXA = 5
LAST_WEIGHT = 50
# shape: (states, rate categories, taxa, sites)
SIZES = {"4x4": (4, 4, TAXA, 262145), "20x4": (20, 4, TAXA, 65537), "5x3": (5, 3, TAXA, 65537)}
BOTH = ("4x4", "20x4")  # where a test runs at two sizes only
# the model gradient's long walks: (states, rate categories, sites)
QG_SIZES = [(4, 4, 16385), (20, 4, 1025), (20, 4, 3137), (5, 4, 4097), (61, 2, 257), (4, 8, 4097)]


def walk(states, rate_cats, sites):
    """(T, w, B) of the batched calls: T = ceil(sites / 64); 4 x 4: w = ceil(T / 4096), B = ceil(T / (4 w)); every other
    shape: w = ceil(T / 1024), B = ceil(T / w)"""
    tiles = -(-sites // 64)
    if states == 4 and rate_cats == 4:
        w = -(-tiles // 4096)
        return tiles, w, -(-tiles // (4 * w))
    w = -(-tiles // 1024)
    return tiles, w, -(-tiles // w)


def qg_walk(states, rate_cats, sites):
    """(T, w, B) of pllgpu_qmatrix_gradient: 4 x 4: w = ceil(T / (4 MAX_BLOCKS)), B = ceil(T / (4 w)); every other shape:
    P = states rounded up to 16, M = min(MAX_BLOCKS, max(4, floor(16384 / P^2))), w = ceil(T / M), B = ceil(T / w)"""
    tiles = -(-sites // 64)
    if states == 4 and rate_cats == 4:
        w = -(-tiles // (4 * QG_MAX_BLOCKS))
        return tiles, w, -(-tiles // (4 * w))
    pad = -(-states // 16) * 16
    m = min(QG_MAX_BLOCKS, max(4, 16384 // (pad * pad)))
    w = -(-tiles // m)
    return tiles, w, -(-tiles // w)


def last_workgroup(states, rate_cats, sites, rule=walk):
    """(tiles the last workgroup holds, tiles a full one holds, sites of the very last tile)"""
    tiles, w, blocks = rule(states, rate_cats, sites)
    full = 4 * w if states == 4 and rate_cats == 4 else w
    return tiles - (blocks - 1) * full, full, sites - 64 * (tiles - 1)


@functools.lru_cache(maxsize=None)
def case(states, rate_cats, taxa, sites, extra=2):
    return IC.make(states, taxa, sites, rate_cats, extra=extra)


def pattern_weights(sites, last=LAST_WEIGHT):
    w = np.ones(sites, dtype=np.uint32)
    w[-1] = last
    return w


def weight_sum(sites, last=LAST_WEIGHT):
    return sites - 1 + last


def bed(lib, dims, attrs=0, last=LAST_WEIGHT, **kw):
    """one library's partition of a size; last = None leaves every pattern weight at 1"""
    states, rate_cats, taxa, sites = dims
    lay, seqs, cmap, exch, freqs = case(states, rate_cats, taxa, sites)
    if last is not None:
        kw["pattern_weights"] = pattern_weights(sites, last)
    return IC.Bed(lib, lay, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, **kw)


def drop_last_site(b):
    """the last site's pattern weight set to 0 in the partition behind b (the reference's): what a lost tile would give"""
    b.lib.pll_set_pattern_weights(b.p, api.uptr(pattern_weights(b.sites, 0)))
