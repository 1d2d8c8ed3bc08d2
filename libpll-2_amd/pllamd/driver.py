"""Issue the libpll call sequence of one test case against a library with the libpll ABI.

`run_case` is the Python rendering of what the reference's own tests do in C
(test/src/00010_NMDU_lkcalc.c:33-175): create partition, set model arrays and tip data, update
partials, evaluate edge log-likelihoods, read CLVs back. Because it talks ABI only, parity
tests call it once per library under comparison.
"""
import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import api


@dataclass
class Case:
    name: str
    states: int
    rate_cats: int
    tips: int
    sites: int
    pmatrix: np.ndarray  # [prob_matrices][rate][states][states] float64, row = parent state
    freqs: np.ndarray  # [rate_matrices][states]
    op_batches: List[List[Tuple[int, ...]]]  # one inner list per pll_update_partials call
    edges: List[Tuple[int, int, int, int, int]]  # (parent, pscaler, child, cscaler, matrix)
    charmap: Optional[np.ndarray] = None  # uint64[256] char -> state mask
    sequences: Optional[List[bytes]] = None
    tip_clvs: Optional[np.ndarray] = None  # [tips][sites][states]
    attributes: int = 0  # PATTERN_TIP / RATE_SCALERS / SITE_REPEATS / AB_* (no arch bits)
    clv_buffers: int = 0
    scale_buffers: int = 0
    rate_weights: Optional[np.ndarray] = None
    pattern_weights: Optional[np.ndarray] = None
    prop_invar: Optional[np.ndarray] = None
    freqs_indices: Optional[np.ndarray] = None
    roots: List[Tuple[int, int]] = field(default_factory=list)  # (clv, scaler) root lnL
    dump_clvs: Optional[Sequence[int]] = None  # default: every op parent
    update_repeats: int = 1
    # optional model description for the derivative tests: exch (upper triangle), rates (category
    # rates), and the list of branch lengths at which derivatives are evaluated
    model: Optional[dict] = None
    # ascertainment-bias correction: attributes must carry api.AB_FLAG (extra per-state entries);
    # asc_type 0 none, 1 Lewis, 2 Felsenstein, 3 Stamatakis (PLL_ATTRIB_AB_* >> 5), set through
    # pll_set_asc_bias_type; asc_weights[states] through pll_set_asc_state_weights
    asc_type: int = 0
    asc_weights: Optional[np.ndarray] = None

    def __post_init__(self):
        self.pmatrix = np.ascontiguousarray(self.pmatrix, dtype=np.float64)
        self.freqs = np.ascontiguousarray(np.atleast_2d(self.freqs), dtype=np.float64)
        if not self.clv_buffers:
            self.clv_buffers = max(self.tips - 2, 1)
        if self.rate_weights is None:
            self.rate_weights = np.full(self.rate_cats, 1.0 / self.rate_cats)
        if self.pattern_weights is None:
            self.pattern_weights = np.ones(self.sites, dtype=np.uint32)
        if self.prop_invar is None:
            self.prop_invar = np.zeros(self.freqs.shape[0])
        if self.freqs_indices is None:
            self.freqs_indices = np.zeros(self.rate_cats, dtype=np.uint32)

    @property
    def asc_alloc(self):
        return bool(self.attributes & (api.AB_FLAG | (7 << 5)))

    @property
    def entries_alloc(self):
        """site entries per (uncompressed) CLV: the sites plus one extra entry per state"""
        return self.sites + (self.states if self.asc_alloc else 0)

    @property
    def prob_matrices(self):
        return self.pmatrix.shape[0]

    @property
    def rate_matrices(self):
        return self.freqs.shape[0]


def states_padded_for(states, arch):
    if arch & (api.ARCH_AVX | api.ARCH_AVX2):
        return (states + 3) & ~3
    if arch & api.ARCH_SSE:
        return (states + 1) & ~1
    return states


def insertion_loglikelihoods(lib, partition, subtree, candidates, freqs_indices):
    """pll_gpu_insertion_loglikelihoods: subtree = (clv, scaler, matrix) of the end that is inserted, candidates = rows
    in pll_gpu_insertion_t field order (child1 clv, scaler, matrix, child2 clv, scaler, matrix); one log-likelihood
    per candidate, all from one call. libpll_amd.so only."""
    rows = list(candidates)
    out = np.full(len(rows), np.nan)
    fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
    if not lib.pll_gpu_insertion_loglikelihoods(partition, int(subtree[0]), int(subtree[1]), int(subtree[2]),
                                                api.make_insertions(rows), len(rows), api.uptr(fi), api.dptr(out)):
        raise RuntimeError(f"pll_gpu_insertion_loglikelihoods: [{lib.errno()}] {lib.errmsg()}")
    return out


def placement_loglikelihoods(lib, partition, query_tips, pendant_matrix, candidates, freqs_indices):
    """pll_gpu_placement_loglikelihoods: every query tip of query_tips inserted into every candidate (rows in
    pll_gpu_insertion_t field order) across the one pendant matrix; a [Q, E] array from one call. libpll_amd.so only."""
    rows = list(candidates)
    tips = np.ascontiguousarray(query_tips, dtype=np.uint32)
    out = np.full((len(tips), len(rows)), np.nan)
    fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
    if not lib.pll_gpu_placement_loglikelihoods(partition, api.uptr(tips), len(tips), int(pendant_matrix), api.make_insertions(rows),
                                                len(rows), api.uptr(fi), api.dptr(out)):
        raise RuntimeError(f"pll_gpu_placement_loglikelihoods: [{lib.errno()}] {lib.errmsg()}")
    return out


def insertion_loglikelihoods_per_edge(lib, partition, subtree, candidates, freqs_indices, tmp):
    """the same values the way every libpll offers them: per candidate one pll_update_partials with a single operation
    into the spare node tmp = (clv, scaler), then pll_compute_edge_loglikelihood between tmp and the subtree end"""
    fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
    out = np.empty(len(candidates))
    for i, c in enumerate(candidates):
        lib.pll_update_partials(partition, api.make_ops([(tmp[0], tmp[1], c[0], c[2], c[1], c[3], c[5], c[4])]), 1)
        out[i] = lib.pll_compute_edge_loglikelihood(partition, tmp[0], tmp[1], int(subtree[0]), int(subtree[1]), int(subtree[2]),
                                                    api.uptr(fi), None)
    return out


def quartet_loglikelihoods(lib, partition, quartets, freqs_indices):
    """pll_gpu_quartet_loglikelihoods: quartets = rows ((clv, scaler, matrix) of e0, of e1, of e2, of e3, inner matrix);
    a [Q, 3] array from one call, column a = arrangement a: ((e0,e1),(e2,e3)), ((e0,e2),(e1,e3)), ((e0,e3),(e1,e2)).
    libpll_amd.so only."""
    rows = list(quartets)
    out = np.full((len(rows), 3), np.nan)
    fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
    if not lib.pll_gpu_quartet_loglikelihoods(partition, api.make_quartets(rows), len(rows), api.uptr(fi), api.dptr(out)):
        raise RuntimeError(f"pll_gpu_quartet_loglikelihoods: [{lib.errno()}] {lib.errmsg()}")
    return out


QUARTET_PAIRS = (((0, 1), (2, 3)), ((0, 2), (1, 3)), ((0, 3), (1, 2)))


def quartet_loglikelihoods_per_edge(lib, partition, quartets, freqs_indices, tmp1, tmp2, after_value=None):
    """the same values the way every libpll offers them: per value one pll_update_partials with two operations into the
    spare nodes tmp1 / tmp2 = (clv, scaler), then pll_compute_edge_loglikelihood between them over the inner matrix.
    after_value(i, a, (x, y), (z, w)), if given, runs after each value while both spare nodes still hold it."""
    fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
    rows = list(quartets)
    out = np.empty((len(rows), 3))
    for i, r in enumerate(rows):
        for a, ((x, y), (z, w)) in enumerate(QUARTET_PAIRS):
            ops = [(tmp1[0], tmp1[1], r[x][0], r[x][2], r[x][1], r[y][0], r[y][2], r[y][1]),
                   (tmp2[0], tmp2[1], r[z][0], r[z][2], r[z][1], r[w][0], r[w][2], r[w][1])]
            lib.pll_update_partials(partition, api.make_ops(ops), 2)
            out[i, a] = lib.pll_compute_edge_loglikelihood(partition, tmp1[0], tmp1[1], tmp2[0], tmp2[1], int(r[4]), api.uptr(fi), None)
            if after_value is not None:
                after_value(i, a, (r[x], r[y]), (r[z], r[w]))
    return out


def quartet_resampled_loglikelihoods(lib, partition, quartets, freqs_indices, weights, want_persite=False):
    """pll_gpu_quartet_resampled_loglikelihoods: quartets as for quartet_loglikelihoods, weights a [replicates, sites]
    array of site weights (None or zero rows: no replicates). Returns (lnl [Q, 3], resampled [Q, replicates, 3] or None,
    persite [Q, 3, sites] or None) from one call. libpll_amd.so only."""
    rows = list(quartets)
    sites = int(partition.contents.sites)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32).reshape(-1, sites)
    reps = 0 if w is None else len(w)
    lnl = np.full((len(rows), 3), np.nan)
    res = np.full((len(rows), reps, 3), np.nan) if reps else None
    per = np.full((len(rows), 3, sites), np.nan) if want_persite else None
    fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
    if not lib.pll_gpu_quartet_resampled_loglikelihoods(partition, api.make_quartets(rows), len(rows), api.uptr(fi),
                                                        api.uptr(w) if reps else None, reps, api.dptr(lnl),
                                                        api.dptr(res) if reps else None, api.dptr(per) if want_persite else None):
        raise RuntimeError(f"pll_gpu_quartet_resampled_loglikelihoods: [{lib.errno()}] {lib.errmsg()}")
    return lnl, res, per


def quartet_rell_loglikelihoods(lib, partition, quartets, freqs_indices, seed, replicates, want_persite=False, want_weights=False):
    """pll_gpu_quartet_rell_loglikelihoods: quartet_resampled_loglikelihoods with rows 0 .. replicates - 1 of `seed` drawn on
    the device (pllamd.rell is their definition). Returns (lnl [Q, 3], resampled [Q, replicates, 3] or None, persite
    [Q, 3, sites] or None, weights uint32 [replicates, sites] or None) from one call. libpll_amd.so only."""
    rows = list(quartets)
    sites, reps = int(partition.contents.sites), int(replicates)
    lnl = np.full((len(rows), 3), np.nan)
    res = np.full((len(rows), reps, 3), np.nan) if reps else None
    per = np.full((len(rows), 3, sites), np.nan) if want_persite else None
    w = np.full((reps, sites), 0xFFFFFFFF, dtype=np.uint32) if want_weights and reps else None
    fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
    if not lib.pll_gpu_quartet_rell_loglikelihoods(partition, api.make_quartets(rows), len(rows), api.uptr(fi), int(seed), reps, api.dptr(lnl),
                                                   api.dptr(res) if reps else None, api.dptr(per) if want_persite else None,
                                                   api.uptr(w) if w is not None else None):
        raise RuntimeError(f"pll_gpu_quartet_rell_loglikelihoods: [{lib.errno()}] {lib.errmsg()}")
    return lnl, res, per, w


def draw_replicate_weights(lib, partition, seed, first, replicates):
    """pll_gpu_draw_replicate_weights: rows [first, first + replicates) of `seed` for the partition's pattern weights, a
    uint32 [replicates, sites] array (pllamd.rell.replicate_weights is their definition). libpll_amd.so only."""
    sites = int(partition.contents.sites)
    w = np.full((int(replicates), sites), 0xFFFFFFFF, dtype=np.uint32)
    if not lib.pll_gpu_draw_replicate_weights(partition, int(seed), int(first), int(replicates), api.uptr(w) if len(w) else None):
        raise RuntimeError(f"pll_gpu_draw_replicate_weights: [{lib.errno()}] {lib.errmsg()}")
    return w


def quartet_persite_per_edge(lib, partition, quartets, freqs_indices, tmp1, tmp2, after_value=None):
    """the reference path of quartet_loglikelihoods_per_edge with a persite_lnl buffer per value: (lnl [Q, 3],
    persite [Q, 3, sites]) - each row what pll_compute_edge_loglikelihood stores, the partition's pattern weights
    included. after_value as in quartet_loglikelihoods_per_edge. Either library."""
    fi = np.ascontiguousarray(freqs_indices, dtype=np.uint32)
    rows = list(quartets)
    sites = int(partition.contents.sites)
    out = np.empty((len(rows), 3))
    per = np.full((len(rows), 3, sites), np.nan)
    for i, r in enumerate(rows):
        for a, ((x, y), (z, w)) in enumerate(QUARTET_PAIRS):
            ops = [(tmp1[0], tmp1[1], r[x][0], r[x][2], r[x][1], r[y][0], r[y][2], r[y][1]),
                   (tmp2[0], tmp2[1], r[z][0], r[z][2], r[z][1], r[w][0], r[w][2], r[w][1])]
            lib.pll_update_partials(partition, api.make_ops(ops), 2)
            out[i, a] = lib.pll_compute_edge_loglikelihood(partition, tmp1[0], tmp1[1], tmp2[0], tmp2[1], int(r[4]), api.uptr(fi),
                                                           api.dptr(per[i, a]))
            if after_value is not None:
                after_value(i, a, (r[x], r[y]), (r[z], r[w]))
    return out, per


def branch_derivatives(lib, partition, rows, params_indices, want_dd=True):
    """pll_gpu_branch_derivatives: rows (parent clv, parent scaler, child clv, child scaler, t); a [count, 2] array
    (d_f, dd_f of -lnL) from one call - column 1 stays NaN with want_dd=False (dd_f = NULL). libpll_amd.so only."""
    rows = list(rows)
    d, dd = np.full(len(rows), np.nan), np.full(len(rows), np.nan)
    pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
    if not lib.pll_gpu_branch_derivatives(partition, api.make_branches(rows), len(rows), api.uptr(pi), api.dptr(d),
                                          api.dptr(dd) if want_dd else None):
        raise RuntimeError(f"pll_gpu_branch_derivatives: [{lib.errno()}] {lib.errmsg()}")
    return np.stack([d, dd], axis=1)


def branch_category_derivatives(lib, partition, rows, params_indices, want_d=True, want_dd=True):
    """pll_gpu_branch_category_derivatives: rows as branch_derivatives; (d_cat [count, rate_cats], d_f [count], dd_f [count]) from
    one call - d_f / dd_f stay NaN where not asked for (NULL). libpll_amd.so only."""
    rows = list(rows)
    R = int(partition.contents.rate_cats)
    cat, d, dd = np.full((len(rows), R), np.nan), np.full(len(rows), np.nan), np.full(len(rows), np.nan)
    pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
    if not lib.pll_gpu_branch_category_derivatives(partition, api.make_branches(rows), len(rows), api.uptr(pi), api.dptr(cat),
                                                   api.dptr(d) if want_d else None, api.dptr(dd) if want_dd else None):
        raise RuntimeError(f"pll_gpu_branch_category_derivatives: [{lib.errno()}] {lib.errmsg()}")
    return cat, d, dd


def rate_gradient(lib, partition, rows, params_indices, want_rates=True, want_scale=True, want_cat=True, want_d=True):
    """pll_gpu_rate_gradient: rows as branch_derivatives; a dict d_rates [rate_cats], d_scale (float), d_cat [count, rate_cats],
    d_f [count] from one call - NaN where not asked for (NULL). d_rates / d_scale are gradients of -lnL only where the rows
    name every branch of the tree once, each end oriented towards its branch. libpll_amd.so only."""
    rows = list(rows)
    R = int(partition.contents.rate_cats)
    rates, scale = np.full(R, np.nan), np.full(1, np.nan)
    cat, d = np.full((len(rows), R), np.nan), np.full(len(rows), np.nan)
    pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
    if not lib.pll_gpu_rate_gradient(partition, api.make_branches(rows), len(rows), api.uptr(pi), api.dptr(rates) if want_rates else None,
                                     api.dptr(scale) if want_scale else None, api.dptr(cat) if want_cat else None,
                                     api.dptr(d) if want_d else None):
        raise RuntimeError(f"pll_gpu_rate_gradient: [{lib.errno()}] {lib.errmsg()}")
    return {"d_rates": rates, "d_scale": float(scale[0]), "d_cat": cat, "d_f": d}


def qmatrix_gradient(lib, partition, rows, params_indices, want_root=True):
    """pll_gpu_qmatrix_gradient: rows as branch_derivatives; (d_q [rate_matrices, states, states], d_root [rate_matrices,
    states]) of -lnL from one call - d_root stays NaN with want_root=False (NULL). libpll_amd.so only."""
    rows = list(rows)
    part = partition.contents
    M, S = int(part.rate_matrices), int(part.states)
    d_q, d_root = np.full((M, S, S), np.nan), np.full((M, S), np.nan)
    pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
    if not lib.pll_gpu_qmatrix_gradient(partition, api.make_branches(rows), len(rows), api.uptr(pi), api.dptr(d_q),
                                        api.dptr(d_root) if want_root else None):
        raise RuntimeError(f"pll_gpu_qmatrix_gradient: [{lib.errno()}] {lib.errmsg()}")
    return d_q, d_root


def subst_gradient(lib, partition, rows, params_indices, want_subst=True, want_freqs=True):
    """pll_gpu_subst_gradient: rows as branch_derivatives; (d_subst [rate_matrices, states (states - 1) / 2], d_freqs
    [rate_matrices, states]) of -lnL - NaN where not asked for (NULL). Gradients only where the rows name every branch of the
    tree once, each end oriented towards its branch. libpll_amd.so only."""
    rows = list(rows)
    part = partition.contents
    M, S = int(part.rate_matrices), int(part.states)
    d_subst, d_freqs = np.full((M, S * (S - 1) // 2), np.nan), np.full((M, S), np.nan)
    pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
    if not lib.pll_gpu_subst_gradient(partition, api.make_branches(rows), len(rows), api.uptr(pi), api.dptr(d_subst) if want_subst else None,
                                      api.dptr(d_freqs) if want_freqs else None):
        raise RuntimeError(f"pll_gpu_subst_gradient: [{lib.errno()}] {lib.errmsg()}")
    return d_subst, d_freqs


DISTANCE_OUTPUTS = ("distance", "p_distance", "d_f", "dd_f", "status", "iterations")


def newton_options(t_start, t_min, t_max, tolerance, max_iters, matrix_index=-1):
    """pll_gpu_newton_t from its fields"""
    return api.Newton(float(t_start), float(t_min), float(t_max), float(tolerance), int(max_iters), int(matrix_index))


def pairwise_distances(lib, partition, tips, params_indices, options, want=DISTANCE_OUTPUTS, fill=None):
    """pll_gpu_pairwise_distances: tips = the tip indices of the list, options = an api.Newton (newton_options). A dict of
    [count, count] arrays: `distance` always, the others of `want` (p_distance, d_f, dd_f float64; status int32; iterations
    uint32) - the rest is handed over as NULL. `fill`: what every array holds before the call, cast to its type (tests: outputs stay untouched
    on a failure; the arrays then travel in the exception's `outputs`). libpll_amd.so only."""
    tips = np.ascontiguousarray(tips, dtype=np.uint32)
    n = len(tips)
    pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
    dtypes = {"status": np.int32, "iterations": np.uint32}
    out = {name: np.full((n, n), 0.0 if fill is None else fill).astype(dtypes.get(name, np.float64))
           for name in DISTANCE_OUTPUTS if name == "distance" or name in want}
    rec = api.Distances()
    for name, a in out.items():
        setattr(rec, name, a.ctypes.data_as(dict(api.Distances._fields_)[name]))
    if not lib.pll_gpu_pairwise_distances(partition, api.uptr(tips), n, api.uptr(pi), C.byref(options), C.byref(rec)):
        err = RuntimeError(f"pll_gpu_pairwise_distances: [{lib.errno()}] {lib.errmsg()}")
        err.outputs = out
        raise err
    return out


def nj_tree(lib, distances, flags=0, device=-1, fill=None):
    """pll_gpu_nj_tree: (parent int32 [2n - 2], length float64 [2n - 2]) of the [n, n] matrix `distances` (only [x][y],
    x < y, is read); flags 0 = NJ, api.NJ_BIONJ. `fill`: what both outputs hold before the call (tests: outputs stay
    untouched on a failure; they then travel in the exception's `outputs`). libpll_amd.so only."""
    d = np.ascontiguousarray(distances, dtype=np.float64)
    n = d.shape[0]
    assert d.shape == (n, n)
    parent = np.full(max(2 * n - 2, 1), 0 if fill is None else fill, dtype=np.int32)
    length = np.full(max(2 * n - 2, 1), 0.0 if fill is None else fill, dtype=np.float64)
    if not lib.pll_gpu_nj_tree(api.dptr(d), n, int(flags), int(device), parent.ctypes.data_as(C.POINTER(C.c_int)), api.dptr(length)):
        err = RuntimeError(f"pll_gpu_nj_tree: [{lib.errno()}] {lib.errmsg()}")
        err.outputs = {"parent": parent, "length": length}
        raise err
    return parent, length


def distance_tree(lib, partition, tips, params_indices, options, flags=0, want_distances=True, fill=None):
    """pll_gpu_distance_tree: (parent, length, distances or None) of the tips of the list - pairwise_distances and nj_tree
    in one call, the matrix staying on the device unless want_distances. libpll_amd.so only."""
    tips = np.ascontiguousarray(tips, dtype=np.uint32)
    n = len(tips)
    pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
    parent = np.full(max(2 * n - 2, 1), 0 if fill is None else fill, dtype=np.int32)
    length = np.full(max(2 * n - 2, 1), 0.0 if fill is None else fill, dtype=np.float64)
    dist = np.full((n, n), 0.0 if fill is None else fill, dtype=np.float64) if want_distances else None
    if not lib.pll_gpu_distance_tree(partition, api.uptr(tips), n, api.uptr(pi), C.byref(options), int(flags),
                                     parent.ctypes.data_as(C.POINTER(C.c_int)), api.dptr(length), api.dptr(dist) if want_distances else None):
        err = RuntimeError(f"pll_gpu_distance_tree: [{lib.errno()}] {lib.errmsg()}")
        err.outputs = {"parent": parent, "length": length, "distances": dist}
        raise err
    return parent, length, dist


def branch_derivatives_per_edge(lib, partition, rows, params_indices, sumtable=None):
    """the same values the way every libpll offers them: per row pll_update_sumtable into one caller-owned table, then
    pll_compute_likelihood_derivatives at the row's length. The table (sites * rate_cats * states_padded doubles, 64-byte
    aligned as the reference's kernels store into it) is allocated here unless the caller brings one."""
    rows = list(rows)
    pi = np.ascontiguousarray(params_indices, dtype=np.uint32)
    part = partition.contents
    own = sumtable is None
    if own:
        n = int(part.sites) * int(part.rate_cats) * int(part.states_padded)
        raw = np.zeros(n + 8, dtype=np.float64)
        off = (-raw.ctypes.data // 8) % 8
        sumtable = raw[off:off + n]
    out = np.empty((len(rows), 2))
    d1, d2 = C.c_double(0), C.c_double(0)
    for i, (pclv, psc, cclv, csc, t) in enumerate(rows):
        if not lib.pll_update_sumtable(partition, int(pclv), int(cclv), int(psc), int(csc), api.uptr(pi), api.dptr(sumtable)):
            raise RuntimeError(f"pll_update_sumtable: [{lib.errno()}] {lib.errmsg()}")
        if not lib.pll_compute_likelihood_derivatives(partition, int(psc), int(csc), float(t), api.uptr(pi), api.dptr(sumtable),
                                                      C.byref(d1), C.byref(d2)):
            raise RuntimeError(f"pll_compute_likelihood_derivatives: [{lib.errno()}] {lib.errmsg()}")
        out[i] = d1.value, d2.value
    if own and lib.is_amd:
        lib.pll_gpu_release_sumtable(partition, api.dptr(sumtable))  # the handle dies with this array
    return out


class Session:
    """A live partition built from a Case (kept open so benches can re-run the hot path)."""

    def __init__(self, lib: api.PllLib, case: Case, arch: int = api.ARCH_AVX2):
        self.lib, self.case, self.arch = lib, case, arch
        c = case
        p = lib.pll_partition_create(c.tips, c.clv_buffers, c.states, c.sites, c.rate_matrices,
                                     c.prob_matrices, c.rate_cats, c.scale_buffers,
                                     c.attributes | arch)
        if not p:
            raise RuntimeError(f"pll_partition_create failed: [{lib.errno()}] {lib.errmsg()}")
        self.p = p
        self.part = p.contents
        self.sp = self.part.states_padded
        try:
            self._load_inputs()
        except Exception:
            lib.pll_partition_destroy(p)
            self.p = None
            raise
        self._op_arrays = [api.make_ops(b) for b in c.op_batches]
        self._fi = np.ascontiguousarray(c.freqs_indices, dtype=np.uint32)

    # ------------------------------------------------------------------------------
    def _load_inputs(self):
        lib, c, part, sp = self.lib, self.case, self.part, self.sp
        for m in range(c.rate_matrices):
            f = np.ascontiguousarray(c.freqs[m], dtype=np.float64)
            lib.pll_set_frequencies(self.p, m, api.dptr(f))
        rw = np.ascontiguousarray(c.rate_weights, dtype=np.float64)
        lib.pll_set_category_weights(self.p, api.dptr(rw))
        pw = np.ascontiguousarray(c.pattern_weights, dtype=np.uint32)
        lib.pll_set_pattern_weights(self.p, api.uptr(pw))
        # transition matrices are written straight into the partition's block, padded stride
        r, s = c.rate_cats, c.states
        for i in range(c.prob_matrices):
            dst = api.as_np(part.pmatrix[i], r * s * sp, np.float64).reshape(r, s, sp)
            dst[:, :, :s] = c.pmatrix[i]
            dst[:, :, s:] = 0.0
        if lib.is_amd:
            lib.pll_gpu_invalidate(self.p, api.DIRTY_PMATRIX, -1)
        # tip data
        if c.sequences is not None:
            cmap = (C.c_ulonglong * 256)(*[int(x) for x in c.charmap])
            for t, seq in enumerate(c.sequences):
                assert len(seq) == c.sites
                if not lib.pll_set_tip_states(self.p, t, cmap, seq):
                    raise RuntimeError(f"pll_set_tip_states: [{lib.errno()}] {lib.errmsg()}")
        else:
            for t in range(c.tips):
                a = np.ascontiguousarray(c.tip_clvs[t], dtype=np.float64)
                if not lib.pll_set_tip_clv(self.p, t, api.dptr(a), 0):
                    raise RuntimeError(f"pll_set_tip_clv: [{lib.errno()}] {lib.errmsg()}")
        if c.asc_weights is not None:
            w = np.ascontiguousarray(c.asc_weights, dtype=np.uint32)
            lib.pll_set_asc_state_weights(self.p, api.uptr(w))
        if c.asc_type:
            if not lib.pll_set_asc_bias_type(self.p, c.asc_type << 5):
                raise RuntimeError(f"pll_set_asc_bias_type: [{lib.errno()}] {lib.errmsg()}")
        for m in range(c.rate_matrices):
            if c.prop_invar[m] > 0:
                if not lib.pll_update_invariant_sites_proportion(self.p, m, float(c.prop_invar[m])):
                    raise RuntimeError(f"invariant sites: [{lib.errno()}] {lib.errmsg()}")

    # ------------------------------------------------------------------------------
    def update_partials(self, update_repeats=None):
        ur = self.case.update_repeats if update_repeats is None else update_repeats
        for arr, batch in zip(self._op_arrays, self.case.op_batches):
            if ur == 1:
                self.lib.pll_update_partials(self.p, arr, len(batch))
            else:
                self.lib.pll_update_partials_rep(self.p, arr, len(batch), ur)

    def edge_lnl(self, edge, persite=True):
        c = self.case
        ps = np.zeros(c.sites) if persite else None
        v = self.lib.pll_compute_edge_loglikelihood(
            self.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(self._fi),
            api.dptr(ps) if persite else None)
        return v, ps

    def root_lnl(self, root, persite=True):
        c = self.case
        ps = np.zeros(c.sites) if persite else None
        v = self.lib.pll_compute_root_loglikelihood(
            self.p, root[0], root[1], api.uptr(self._fi), api.dptr(ps) if persite else None)
        return v, ps

    def pending_clvs(self):
        """pll_gpu_pending_clvs (libpll_amd.so only): CLVs the last step formed and has not stored on the device"""
        return int(self.lib.pll_gpu_pending_clvs(self.p)) if self.lib.is_amd else 0

    def node_ancestral(self, edge):
        """marginal state probabilities [sites, states] of the node edge[0] (scaler edge[1]) towards the other
        end edge[2] (scaler edge[3]) across matrix edge[4]"""
        c = self.case
        out = np.zeros((c.sites, c.states))
        ok = self.lib.pll_compute_node_ancestral(
            self.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(self._fi), api.dptr(out))
        if not ok:
            raise RuntimeError(f"pll_compute_node_ancestral: [{self.lib.errno()}] {self.lib.errmsg()}")
        return out

    CATEGORY_OUTPUTS = ("cat_lnl", "posterior", "site_rates", "weight_sums", "lnl")

    def edge_categories(self, edge, want=CATEGORY_OUTPUTS):
        """pll_gpu_edge_category_posteriors on edge = (parent, pscaler, child, cscaler, matrix): a dict of the outputs
        named in `want` - cat_lnl and posterior [sites, rate_cats], site_rates [sites], weight_sums [rate_cats], lnl"""
        c = self.case
        shapes = {"cat_lnl": (c.sites, c.rate_cats), "posterior": (c.sites, c.rate_cats), "site_rates": (c.sites,),
                  "weight_sums": (c.rate_cats,), "lnl": (1,)}
        unknown = set(want) - set(shapes)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        out = {k: np.zeros(shapes[k]) for k in self.CATEGORY_OUTPUTS if k in want}
        ok = self.lib.pll_gpu_edge_category_posteriors(
            self.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(self._fi),
            *[api.dptr(out[k]) if k in out else None for k in self.CATEGORY_OUTPUTS])
        if not ok:
            raise RuntimeError(f"pll_gpu_edge_category_posteriors: [{self.lib.errno()}] {self.lib.errmsg()}")
        if "lnl" in out:
            out["lnl"] = float(out["lnl"][0])
        return out

    def category_weights_em(self, edge, start, steps):
        """pll_gpu_category_weights_em: (weights [steps + 1, rate_cats], lnl [steps + 1]); start None = the partition's
        rate_weights"""
        c = self.case
        w = np.zeros((steps + 1, c.rate_cats))
        lnl = np.zeros(steps + 1)
        s = None if start is None else np.ascontiguousarray(start, dtype=np.float64)
        ok = self.lib.pll_gpu_category_weights_em(
            self.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(self._fi),
            None if s is None else api.dptr(s), steps, api.dptr(w), api.dptr(lnl))
        if not ok:
            raise RuntimeError(f"pll_gpu_category_weights_em: [{self.lib.errno()}] {self.lib.errmsg()}")
        return w, lnl

    def insertion_lnls(self, subtree, candidates):
        """log-likelihood of inserting subtree = (clv, scaler, matrix) into every candidate edge, one call"""
        return insertion_loglikelihoods(self.lib, self.p, subtree, candidates, self._fi)

    def entries(self, clv_index):
        return self.lib.pll_get_sites_number(self.p, clv_index)

    def read_clv(self, clv_index, expand=True):
        """CLV as [sites or entries][rate][states] (padding stripped). With site repeats and
        expand=True the class-compressed CLV is expanded through site_id."""
        c, sp = self.case, self.sp
        if self.lib.is_amd:
            if not self.lib.pll_gpu_sync_clv(self.p, clv_index):
                raise RuntimeError(f"pll_gpu_sync_clv: [{self.lib.errno()}] {self.lib.errmsg()}")
        n = self.entries(clv_index)
        raw = api.as_np(self.part.clv[clv_index], n * c.rate_cats * sp, np.float64)
        a = raw.reshape(n, c.rate_cats, sp)[:, :, :c.states].copy()
        sid = self.lib.pll_get_site_id(self.p, clv_index)
        if expand and sid:
            ids = api.as_np(sid, c.sites, np.uint32)
            a = a[ids]
        return a

    def set_asc_type(self, asc_type):
        if not self.lib.pll_set_asc_bias_type(self.p, asc_type << 5):
            raise RuntimeError(f"pll_set_asc_bias_type: [{self.lib.errno()}] {self.lib.errmsg()}")

    def read_scaler(self, scaler_index, clv_index=None, expand=True):
        c = self.case
        if scaler_index < 0:
            return None
        if self.lib.is_amd:
            self.lib.pll_gpu_sync_scaler(self.p, scaler_index)
        n = self.entries(clv_index) if clv_index is not None else c.entries_alloc
        per = c.rate_cats if (c.attributes & api.RATE_SCALERS) else 1
        a = api.as_np(self.part.scale_buffer[scaler_index], n * per, np.uint32).reshape(n, per).copy()
        if clv_index is not None and expand:
            sid = self.lib.pll_get_site_id(self.p, clv_index)
            if sid:
                a = a[api.as_np(sid, c.sites, np.uint32)]
        return a

    def write_scaler(self, scaler_index, clv_index, counts):
        """the caller's own scaling counts into partition->scale_buffer[scaler_index] - [entries] or [entries][rates] with
        PLL_ATTRIB_RATE_SCALERS, entries = pll_get_sites_number of the node the buffer belongs to. read_scaler first
        settles the device side (whatever pll_update_partials holds back is launched, the host copy becomes current);
        afterwards libpll_amd.so is told that the host copy is the newer one"""
        cur = self.read_scaler(scaler_index, clv_index, expand=False)
        new = np.ascontiguousarray(counts, dtype=np.uint32).reshape(cur.shape)
        api.as_np(self.part.scale_buffer[scaler_index], new.size, np.uint32)[:] = new.ravel()
        if self.lib.is_amd:
            self.lib.pll_gpu_invalidate(self.p, api.DIRTY_SCALER, scaler_index)

    # ---- branch-length derivatives ---------------------------------
    def set_model(self, exch, freqs, rates):
        """substitution parameters, frequencies and category rates through the model setters; the
        library computes its own eigensystem on demand (pll_update_eigen)"""
        c = self.case
        e = np.ascontiguousarray(exch, dtype=np.float64)
        for m in range(c.rate_matrices):
            f = np.ascontiguousarray(np.atleast_2d(freqs)[m], dtype=np.float64)
            self.lib.pll_set_frequencies(self.p, m, api.dptr(f))
            self.lib.pll_set_subst_params(self.p, m, api.dptr(e))
        r = np.ascontiguousarray(rates, dtype=np.float64)
        self.lib.pll_set_category_rates(self.p, api.dptr(r))

    def update_eigen(self):
        for m in range(self.case.rate_matrices):
            if not self.lib.pll_update_eigen(self.p, m):
                raise RuntimeError(f"pll_update_eigen: [{self.lib.errno()}] {self.lib.errmsg()}")

    def read_eigen(self):
        c, sp, part = self.case, self.sp, self.part
        out = {"eigenvecs": [], "inv_eigenvecs": [], "eigenvals": []}
        for m in range(c.rate_matrices):
            out["eigenvecs"].append(api.as_np(part.eigenvecs[m], c.states * sp, np.float64).reshape(c.states, sp)[:, :c.states].copy())
            out["inv_eigenvecs"].append(api.as_np(part.inv_eigenvecs[m], c.states * sp, np.float64).reshape(c.states, sp)[:, :c.states].copy())
            out["eigenvals"].append(api.as_np(part.eigenvals[m], c.states, np.float64).copy())
        return {k: np.stack(v) for k, v in out.items()}

    def inject_eigen(self, eig, rates):
        """write a given eigensystem into the partition's arrays (callers may do that: the arrays are
        public) and mark it valid, so both libraries work in the same eigenbasis"""
        c, sp, part = self.case, self.sp, self.part
        for m in range(c.rate_matrices):
            for name in ("eigenvecs", "inv_eigenvecs"):
                dst = api.as_np(getattr(part, name)[m], c.states * sp, np.float64).reshape(c.states, sp)
                dst[:, :] = 0.0
                dst[:, :c.states] = eig[name][m]
            api.as_np(part.eigenvals[m], sp, np.float64)[:c.states] = eig["eigenvals"][m]
            part.eigen_decomp_valid[m] = 1
        r = np.ascontiguousarray(rates, dtype=np.float64)
        self.lib.pll_set_category_rates(self.p, api.dptr(r))
        if self.lib.is_amd:
            self.lib.pll_gpu_invalidate(self.p, api.DIRTY_EIGEN, -1)

    def new_sumtable(self):
        """caller-owned table, aligned like pll_aligned_alloc(.., partition->alignment) in the
        reference's tests (its AVX kernels use aligned stores)"""
        n = self.case.entries_alloc * self.case.rate_cats * self.sp
        raw = np.zeros(n + 8, dtype=np.float64)
        off = (-raw.ctypes.data // 8) % 8  # doubles up to the next 64-byte boundary
        return raw[off:off + n]

    def update_sumtable(self, edge, sumtable):
        ok = self.lib.pll_update_sumtable(self.p, edge[0], edge[2], edge[1], edge[3], api.uptr(self._fi), api.dptr(sumtable))
        if not ok:
            raise RuntimeError(f"pll_update_sumtable: [{self.lib.errno()}] {self.lib.errmsg()}")

    def read_sumtable(self, sumtable):
        """[sites (+ states with ascertainment bias)][rate][states]; the AMD library keeps the table
        in HBM until asked for it"""
        c = self.case
        if self.lib.is_amd:
            if not self.lib.pll_gpu_sync_sumtable(self.p, api.dptr(sumtable)):
                raise RuntimeError(f"pll_gpu_sync_sumtable: [{self.lib.errno()}] {self.lib.errmsg()}")
        return sumtable.reshape(c.entries_alloc, c.rate_cats, self.sp)[:, :, :c.states].copy()

    def derivatives(self, edge, sumtable, t):
        d1, d2 = C.c_double(0), C.c_double(0)
        ok = self.lib.pll_compute_likelihood_derivatives(self.p, edge[1], edge[3], float(t), api.uptr(self._fi),
                                                         api.dptr(sumtable), C.byref(d1), C.byref(d2))
        if not ok:
            raise RuntimeError(f"pll_compute_likelihood_derivatives: [{self.lib.errno()}] {self.lib.errmsg()}")
        return d1.value, d2.value

    def optimize_branch(self, edge, sumtable, t_start, t_min, t_max, tolerance, max_iters=api.NEWTON_MAX_ITERS,
                        matrix_index=-1):
        """pll_gpu_optimize_branch_length (libpll_amd.so only): the whole safeguarded Newton iteration of pllamd.newton
        in one call. Returns (result, trace): the api.NewtonResult and the evaluations as rows (t, d_f, dd_f)."""
        opt = api.Newton(float(t_start), float(t_min), float(t_max), float(tolerance), int(max_iters), int(matrix_index))
        res = api.NewtonResult()
        trace = np.full((max(int(max_iters), 1), 3), np.nan)
        ok = self.lib.pll_gpu_optimize_branch_length(self.p, edge[1], edge[3], api.uptr(self._fi), api.dptr(sumtable),
                                                     C.byref(opt), C.byref(res), api.dptr(trace))
        if not ok:
            raise RuntimeError(f"pll_gpu_optimize_branch_length: [{self.lib.errno()}] {self.lib.errmsg()}")
        return res, trace[:res.iterations].copy()

    def close(self):
        if self.p:
            self.lib.pll_partition_destroy(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ParsimonySession:
    """A pll_parsimony_t built from an alignment (pll_fastparsimony_init, src/fast_parsimony.c:523-555) and the calls
    that drive it. ABI only, like Session: the same sequence runs on libpll_amd.so and on the reference; the batched
    calls and the mirror refresh exist on libpll_amd.so alone."""

    def __init__(self, lib: api.PllLib, states, sequences, charmap, weights=None, attributes=0):
        self.lib, self.states = lib, int(states)
        tips, sites = len(sequences), len(sequences[0])
        # parsimony reads the tips only: one CLV buffer, one of everything else
        self.partition = lib.pll_partition_create(tips, 1, states, sites, 1, 1, 1, 0, attributes)
        if not self.partition:
            raise RuntimeError(f"pll_partition_create failed: [{lib.errno()}] {lib.errmsg()}")
        self.pars = None
        try:
            cmap = (C.c_ulonglong * 256)(*[int(x) for x in charmap])
            for t, seq in enumerate(sequences):
                if not lib.pll_set_tip_states(self.partition, t, cmap, bytes(seq)):
                    raise RuntimeError(f"pll_set_tip_states: [{lib.errno()}] {lib.errmsg()}")
            if weights is not None:
                w = np.ascontiguousarray(weights, dtype=np.uint32)
                lib.pll_set_pattern_weights(self.partition, api.uptr(w))
            self.pars = lib.pll_fastparsimony_init(self.partition)
            if not self.pars:
                raise RuntimeError(f"pll_fastparsimony_init failed: [{lib.errno()}] {lib.errmsg()}")
        except Exception:
            self.close()
            raise
        self.s = self.pars.contents
        self.nodes = self.s.tips + 3 * self.s.inner_nodes
        self.words = self.s.packedvector_count

    def drop_partition(self):
        """the structure is independent of the partition it came from"""
        if self.partition:
            self.lib.pll_partition_destroy(self.partition)
            self.partition = None

    def update(self, ops, per_op=False):
        """run (parent, child1, child2) rows; returns the kernel launches the call(s) took (libpll_amd.so) or None"""
        ops = list(ops)
        arr = api.make_pars_ops(ops)
        count = getattr(self.lib, "pll_gpu_fastparsimony_last_launch_count", None)
        launches = 0
        if per_op:
            for i in range(len(ops)):
                self.lib.pll_fastparsimony_update_vector(self.pars, C.byref(arr[i]))
                launches += count(self.pars) if count else 0
        else:
            self.lib.pll_fastparsimony_update_vectors(self.pars, arr, len(ops))
            launches = count(self.pars) if count else 0
        return launches if count else None

    def edge_score(self, a, b):
        return int(self.lib.pll_fastparsimony_edge_score(self.pars, a, b))

    def root_score(self, n):
        return int(self.lib.pll_fastparsimony_root_score(self.pars, n))

    def edge_scores(self, pairs):
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        out = np.full(len(pairs), 0xDEADBEEF, dtype=np.uint32)
        if not self.lib.pll_gpu_fastparsimony_edge_scores(self.pars, api.uptr(pairs), len(pairs), api.uptr(out)):
            raise RuntimeError(f"pll_gpu_fastparsimony_edge_scores: [{self.lib.errno()}] {self.lib.errmsg()}")
        return out

    def insertion_scores(self, node, edges):
        edges = np.ascontiguousarray(edges, dtype=np.uint32).reshape(-1, 2)
        out = np.full(len(edges), 0xDEADBEEF, dtype=np.uint32)
        if not self.lib.pll_gpu_fastparsimony_insertion_scores(self.pars, node, api.uptr(edges), len(edges), api.uptr(out)):
            raise RuntimeError(f"pll_gpu_fastparsimony_insertion_scores: [{self.lib.errno()}] {self.lib.errmsg()}")
        return out

    def insertion_scores_per_edge(self, node, edges, spare):
        """the reference's pattern (src/stepwise.c:507-512): update_vector({spare, a, b}) then edge_score(spare, node)"""
        out = []
        for a, b in edges:
            op = api.make_pars_ops([(spare, a, b)])
            self.lib.pll_fastparsimony_update_vector(self.pars, op)
            out.append(self.edge_score(spare, node))
        return np.array(out, dtype=np.uint32)

    def sync(self, node=-1):
        if self.lib.is_amd and not self.lib.pll_gpu_sync_parsimony(self.pars, node):
            raise RuntimeError(f"pll_gpu_sync_parsimony: [{self.lib.errno()}] {self.lib.errmsg()}")

    def vector(self, node):
        """host copy of a node's packed vector, [states][packedvector_count] (call sync() first on libpll_amd.so)"""
        n = self.states * self.words
        if n == 0:
            return np.zeros((self.states, 0), dtype=np.uint32)
        return api.as_np(self.s.packedvector[node], n, np.uint32).reshape(self.states, self.words).copy()

    def costs(self):
        return api.as_np(self.s.node_cost, self.nodes, np.uint32).copy()

    def informative(self):
        return api.as_np(self.s.informative, self.s.sites, np.int32).copy()

    def close(self):
        if self.pars:
            self.lib.pll_parsimony_destroy(self.pars)
            self.pars = None
        self.drop_partition()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SankoffSession:
    """A pll_parsimony_t made by pll_parsimony_create (src/parsimony.c:117-202) and the calls that drive it. ABI only,
    like ParsimonySession: the same sequence runs on libpll_amd.so and on the reference; the batched call, the mirror
    refresh and the launch count exist on libpll_amd.so alone."""

    def __init__(self, lib: api.PllLib, tips, states, sites, matrix, score_buffers, ancestral_buffers):
        self.lib, self.tips, self.states, self.sites = lib, int(tips), int(states), int(sites)
        self.buffers, self.ancestral_buffers = self.tips + int(score_buffers), int(ancestral_buffers)
        m = np.ascontiguousarray(matrix, dtype=np.float64)
        self.pars = lib.pll_parsimony_create(tips, states, sites, api.dptr(m), score_buffers, ancestral_buffers)
        if not self.pars:
            raise RuntimeError(f"pll_parsimony_create failed: [{lib.errno()}] {lib.errmsg()}")
        self.s = self.pars.contents

    @staticmethod
    def _map(charmap):
        return (C.c_ulonglong * 256)(*[int(x) for x in charmap])

    def set_sequence(self, index, charmap, seq):
        return int(self.lib.pll_set_parsimony_sequence(self.pars, index, self._map(charmap), bytes(seq)))

    def launches(self):
        count = getattr(self.lib, "pll_gpu_fastparsimony_last_launch_count", None)
        return int(count(self.pars)) if count else None

    def build(self, ops, per_op=False):
        """run (parent, child1, child2) rows; returns the score of the last row's parent"""
        ops = list(ops)
        arr = api.make_pars_ops(ops)
        if not per_op:
            return float(self.lib.pll_parsimony_build(self.pars, arr, len(ops)))
        for i in range(len(ops)):
            score = float(self.lib.pll_parsimony_build(self.pars, C.byref(arr[i]), 1))
        return score

    def score(self, index):
        return float(self.lib.pll_parsimony_score(self.pars, index))

    def reconstruct(self, charmap, rows):
        rows = list(rows)
        self.lib.pll_parsimony_reconstruct(self.pars, self._map(charmap), api.make_pars_recops(rows), len(rows))

    def insertion_scores(self, node, edges):
        edges = np.ascontiguousarray(edges, dtype=np.uint32).reshape(-1, 2)
        out = np.full(len(edges), np.nan)
        if not self.lib.pll_gpu_parsimony_insertion_scores(self.pars, node, api.uptr(edges), len(edges), api.dptr(out)):
            raise RuntimeError(f"pll_gpu_parsimony_insertion_scores: [{self.lib.errno()}] {self.lib.errmsg()}")
        return out

    def insertion_scores_per_edge(self, node, edges, spare):
        """what the batched call is defined by: pll_parsimony_build({{t1, a, b}, {t2, t1, node}}, 2)"""
        t1, t2 = spare
        return np.array([self.build([(t1, a, b), (t2, t1, node)]) for a, b in edges])

    def sync(self, node=-1):
        if self.lib.is_amd and not self.lib.pll_gpu_sync_parsimony(self.pars, node):
            raise RuntimeError(f"pll_gpu_sync_parsimony: [{self.lib.errno()}] {self.lib.errmsg()}")

    def buffer(self, index):
        """host copy of a score buffer, [sites][states] (call sync() first on libpll_amd.so)"""
        return api.as_np(self.s.sbuffer[index], self.sites * self.states, np.float64).reshape(self.sites, self.states).copy()

    def ancestral(self, index):
        return api.as_np(self.s.anc_states[index], self.sites, np.uint32).copy()

    def close(self):
        if self.pars:
            self.lib.pll_parsimony_destroy(self.pars)
            self.pars = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def run_case(lib: api.PllLib, case: Case, arch: int = api.ARCH_AVX2):
    """Full sequence; returns {'clv': {idx: arr}, 'scaler': {idx: arr}, 'lnl': [...],
    'persite': [...], 'root_lnl': [...], 'root_persite': [...]}. CLVs are scaler-free raw values;
    use `normalised` to compare across implementations whose scaling decisions may differ."""
    out = {"clv": {}, "scaler": {}, "lnl": [], "persite": [], "root_lnl": [], "root_persite": []}
    with Session(lib, case, arch) as s:
        s.update_partials()
        parents = {}
        for batch in case.op_batches:
            for op in batch:
                parents[op[0]] = op[1]
        dump = case.dump_clvs if case.dump_clvs is not None else sorted(parents)
        for idx in dump:
            out["clv"][idx] = s.read_clv(idx)
            sc = parents.get(idx, -1)
            if sc >= 0:
                out["scaler"][idx] = s.read_scaler(sc, idx)
        for e in case.edges:
            v, ps = s.edge_lnl(e)
            out["lnl"].append(v)
            out["persite"].append(ps)
        for r in case.roots:
            v, ps = s.root_lnl(r)
            out["root_lnl"].append(v)
            out["root_persite"].append(ps)
    return out


def normalised(clv, scaler):
    """(mantissa-like value, exponent) pairs that are invariant to WHEN a site was rescaled:
    returns clv * 2^(-256*scaler) as (frexp mantissa, integer exponent) arrays."""
    m, e = np.frexp(clv)
    e = e.astype(np.int64)
    if scaler is not None:
        sc = scaler.astype(np.int64)
        if sc.shape[1] == 1:
            e = e - 256 * sc[:, :, None]
        else:
            e = e - 256 * sc[:, :, None]
    e = np.where(clv == 0, 0, e)
    return m, e


def rel_err_normalised(a, sa, b, sb):
    """max relative difference between two (clv, scaler) pairs after undoing the scaling."""
    ma, ea = normalised(a, sa)
    mb, eb = normalised(b, sb)
    # bring to common exponent: values equal iff ma*2^ea == mb*2^eb
    d = np.clip(ea - eb, -64, 64)
    va = np.ldexp(ma, d)  # a expressed at b's exponent
    denom = np.maximum(np.abs(mb), 1e-300)
    err = np.abs(va - mb) / denom
    err = np.where((a == 0) & (b == 0), 0.0, err)
    return float(err.max()) if err.size else 0.0
