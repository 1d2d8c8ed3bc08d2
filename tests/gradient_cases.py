"""What the branch-gradient tests share - TEST INFRASTRUCTURE: from an insertion_cases.Layout the call sequence of a caller
that asks for the derivatives of EVERY branch with one pll_gpu_branch_derivatives call ("The gradient of
every branch at once").

Both ends of every branch are read in one launch, so each must stand in HBM oriented towards its branch at once: the caller
runs the rooted full traversal and the upward operations of the insertion tests (Bed.prepare) and names, per edge, the
root-side (upward) end as the parent, the end away from the root as the child and the tree's own length of that edge."""
import numpy as np

import insertion_cases as IC
from deriv_common import DTOL
from pllamd import driver


def branch_rows(lay, candidates, factor=1.0):
    """one row per edge in tree.edges() order: (parent clv, parent scaler, child clv, child scaler, length x factor); the
    candidates are Layout.candidates' rows: child1 = the end away from the root, child2 = the root-side end"""
    edges = lay.tree.edges()
    assert len(edges) == len(candidates) == 2 * lay.T - 3
    return [(c[3], c[4], c[0], c[1], factor * r.length) for r, c in zip(edges, candidates)]


def prepare(bed, factors=(1.0,)):
    """full traversal + upward CLVs; the rows of every edge, once per length factor (factor-major)"""
    cands = bed.prepare()
    return [row for f in factors for row in branch_rows(bed.lay, cands, f)]


def flipped(rows):
    """every row the other way round: parent and child exchanged"""
    return [(c, cs, p, ps, t) for p, ps, c, cs, t in rows]


def batched(bed, rows, **kw):
    return driver.branch_derivatives(bed.lib, bed.p, rows, bed.fi, **kw)


def per_edge(bed, rows):
    """[count, 2] through pll_update_sumtable + pll_compute_likelihood_derivatives, either library"""
    return driver.branch_derivatives_per_edge(bed.lib, bed.p, rows, bed.fi)


def close(got, exp, sites):
    """deriv_common.close for every d_f and every dd_f: |d| <= DTOL |exp| + 4e-15 sites"""
    got, exp = np.asarray(got), np.asarray(exp)
    return got.shape == exp.shape and np.isfinite(got).all() and bool((np.abs(got - exp) <= DTOL * np.abs(exp) + 4e-15 * sites).all())


def worst(got, exp, sites):
    """the largest |d| / (DTOL |exp| + 4e-15 sites): at most 1 where close() holds"""
    got, exp = np.asarray(got), np.asarray(exp)
    return float(np.max(np.abs(got - exp) / (DTOL * np.abs(exp) + 4e-15 * sites)))


def launches_by_rule(states, rate_cats, sites, count):
    """the cutting rule of include/pll_amd_device.h, pllgpu_branch_derivatives"""
    tiles = (sites + 63) // 64
    if states == 4 and rate_cats == 4:
        w = (tiles + 4095) // 4096
        blocks = (tiles + 4 * w - 1) // (4 * w)
    else:
        w = (tiles + 1023) // 1024
        blocks = (tiles + w - 1) // w
    per_launch = min(count, 8192, max(1, (4 << 20) // (2 * blocks)))
    return (count + per_launch - 1) // per_launch
