"""What the long-walk tests share - TEST INFRASTRUCTURE: the smallest site counts at which a wave (4 x 4) or a workgroup
(every other shape) of a batched call walks a second 64-site tile, the walk restated from the rule that
include/pll_amd_device.h states, and the inputs: UTree(5, PCG64(7)) through insertion_cases.make - 7 edges, 2 inner
edges, 2 extra tips - with the last site, the only site of the last tile, at pattern weight LAST_WEIGHT and every other
site at 1, in both libraries.
Below them the same for the two calls that leave a table per site (test_gpu_table_walk.py): TABLE_SIZES, the three stages'
walks restated (table_walk, mix_walk, reduce_rounds) and TableBed, a partition of 4 tips and 2 inner CLVs - the batched
calls' layout keeps 18 CLVs, 2.4 GB per library at a million sites."""
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


# ---- the calls that leave a table per site: pll_compute_node_ancestral, pll_gpu_edge_category_posteriors / _em --------------
TABLE_BLOCKS = 4096  # kTableBlocks (pllgpu.hip)
MIX_BLOCKS = 1024  # the grid of k_category_mix ends here
REDUCE_DOUBLES = 7 * 1025  # kCategoryReduceDoubles (kernels_category.h)
# shape: (states, rate categories, sites) - the smallest site counts of their walk length but 5 x 3, which walks three tiles
TABLE_SIZES = {"4x4": (4, 4, 1048577), "20x4": (20, 4, 262145), "4x8": (4, 8, 262145), "5x3": (5, 3, 524353)}
TABLE_SMALLEST = ("4x4", "20x4", "4x8")


def table_walk(states, rate_cats, sites):
    """(T, w, B) of stage A of the per-site table calls (include/pll_amd_device.h, "The launch rule"): T = ceil(sites / 64);
    4 x 4: w = ceil(T / 16384), B = ceil(T / (4 w)); every other shape: w = ceil(T / 4096), B = ceil(T / w)"""
    tiles = -(-sites // 64)
    if states == 4 and rate_cats == 4:
        w = -(-tiles // (4 * TABLE_BLOCKS))
        return tiles, w, -(-tiles // (4 * w))
    w = -(-tiles // TABLE_BLOCKS)
    return tiles, w, -(-tiles // w)


def mix_walk(sites):
    """(256-site tiles, workgroups) of k_category_mix: B = min(ceil(sites / 256), 1024), walked with stride B"""
    tiles = -(-sites // 256)
    return tiles, min(tiles, MIX_BLOCKS)


def reduce_rounds(rate_cats, workgroups):
    """rounds of k_category_reduce over the rate_cats + 1 values of `workgroups` partials each: per = min(R + 1,
    7175 // (nparts | 1)) values a round"""
    per = min(rate_cats + 1, REDUCE_DOUBLES // (workgroups | 1))
    return -(-(rate_cats + 1) // per)


def written_sites(states, rate_cats, sites):
    """where the tests write scaling counts: sites 0, 63, 64 (the first site of a walker's second tile), the last site of
    workgroup 0's walk and the last site"""
    _, full, _ = last_workgroup(states, rate_cats, sites, rule=table_walk)
    return [0, 63, 64, 64 * full - 1, sites - 1]


class TableLayout:
    """the smallest partition with an inner edge and a tip edge: tips 0-3, inner CLVs 4 and 5 with scalers 0 and 1, matrix m
    on the branch above tip m, matrix 4 between the inner nodes (what insertion_cases.Bed asks of a layout)"""
    tips, clv_buffers, scale_buffers, prob_matrices = 4, 2, 2, 5
    OPS = [(4, 0, 0, 0, IC.NONE, 1, 1, IC.NONE), (5, 1, 2, 2, IC.NONE, 3, 3, IC.NONE)]
    INNER = (4, 0, 5, 1, 4)
    TIP = (4, 0, 0, IC.NONE, 0)

    @staticmethod
    def branches():
        return [(0, 0.11), (1, 0.23), (2, 0.08), (3, 0.31), (4, 0.17)]


@functools.lru_cache(maxsize=None)
def table_alignment(states, sites):
    return IC.alignment(states, TableLayout.tips, sites)


class TableBed(IC.Bed):
    """one library's partition of a TABLE_SIZES entry, the traversal done: category rates gamma_rates_mean(0.7, R) (Bed's),
    category weights `weights`, pattern weights 1 but LAST_WEIGHT at the last site"""

    def __init__(self, lib, dims, attrs, weights):
        states, rate_cats, sites = dims
        seqs, cmap, exch, freqs = table_alignment(states, sites)
        super().__init__(lib, TableLayout, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, pattern_weights=pattern_weights(sites))
        self.weights = np.ascontiguousarray(weights, dtype=np.float64)
        lib.pll_set_category_weights(self.p, api.dptr(self.weights))
        self.update(TableLayout.OPS)
