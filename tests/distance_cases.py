"""What the pairwise-distance tests share - TEST INFRASTRUCTURE: the inputs (insertion_cases.alignment with the ambiguity
treatment of workload.make_case), a partition that holds nothing but tips, the per-pair path of either library
(pll_update_sumtable on the two tips + pll_compute_likelihood_derivatives) and the cutting rule of
include/pll_amd_device.h restated."""
import ctypes as C

import numpy as np

import insertion_cases as IC
from pllamd import api, distances, driver, newton, workload as W

NONE = api.SCALE_BUFFER_NONE
T_POINTS = (0.05, 0.3, 1.2)
MAX_PAIRS = 1 << 20  # PLLGPU_DISTANCE_MAX_PAIRS
MAX_CODES = 128      # PLLGPU_DISTANCE_MAX_CODES


def ambiguate(seqs, states, sites, seed=1, gap_pct=10, partial_pct=10):
    """workload.make_case's treatment: gap_pct % of every sequence become '-' (all states), then partial_pct % a partial
    ambiguity character of the alphabet - the same pools and generators"""
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    out = []
    for sq in seqs:
        a = np.frombuffer(sq, dtype=np.uint8).copy()
        a[rng.integers(0, 100, size=sites) < gap_pct] = ord("-")
        out.append(a)
    pool = np.frombuffer({4: b"RYSWKMBDHV", 20: b"BZJ"}.get(states, b"!#$"), dtype=np.uint8)
    rng = np.random.Generator(np.random.PCG64(seed + 78))
    for a in out:
        hit = rng.integers(0, 100, size=sites) < partial_pct
        a[hit] = pool[rng.integers(0, len(pool), size=int(hit.sum()))]
    return [a.tobytes() for a in out]


def sequences(states, tips, sites, seed=8, mutate_pct=15):
    """(sequences, charmap, exchangeabilities, frequencies): insertion_cases.alignment at 15 % mutation, 10 % '-' and 10 %
    partial ambiguity characters"""
    seqs, cmap, exch, freqs = IC.alignment(states, tips, sites, seed, mutate_pct)
    return ambiguate(seqs, states, sites), cmap, exch, freqs


def unrelated(states, sites, seed):
    """one sequence of independent uniform states (no ancestor in common with anything)"""
    st = np.random.Generator(np.random.PCG64(seed)).integers(0, states, size=(1, sites)).astype(np.uint8)
    alphabet = {4: W.NT_CHARS, 20: W.AA_CHARS}.get(states, bytes(range(48, 48 + states)))
    return W.states_to_sequences(st, alphabet)[0]


class Tips:
    """one library's partition of tips alone: the model of insertion_cases.Bed (gamma rates of alpha 0.7, a second rate
    matrix = the first with rotated frequencies)"""

    def __init__(self, lib, states, rate_cats, seqs, cmap, exch, freqs, attrs=0, rate_matrices=1, params_indices=None, pattern_weights=None,
                 rate_weights=None, prop_invar=0.0, dense=()):
        self.lib, self.states, self.rate_cats, self.attrs = lib, states, rate_cats, attrs
        self.tips, self.sites = len(seqs), len(seqs[0])
        self.p = lib.pll_partition_create(self.tips, 1, states, self.sites, rate_matrices, 1, rate_cats, 1, attrs | api.ARCH_AVX2)
        assert self.p, (lib.errno(), lib.errmsg())
        self.part = self.p.contents
        e = np.ascontiguousarray(exch, dtype=np.float64)
        self.rates = np.ascontiguousarray(W.gamma_rates_mean(0.7, rate_cats), dtype=np.float64)
        self.freqs = []
        for m in range(rate_matrices):
            f = np.roll(np.asarray(freqs, dtype=np.float64), m)
            f = np.ascontiguousarray(f / f.sum())
            self.freqs.append(f)
            lib.pll_set_frequencies(self.p, m, api.dptr(f))
            lib.pll_set_subst_params(self.p, m, api.dptr(e))
        lib.pll_set_category_rates(self.p, api.dptr(self.rates))
        self.rate_weights = np.full(rate_cats, 1.0 / rate_cats) if rate_weights is None else np.ascontiguousarray(rate_weights, dtype=np.float64)
        if rate_weights is not None:
            lib.pll_set_category_weights(self.p, api.dptr(self.rate_weights))
        self.cmap = (C.c_ulonglong * 256)(*[int(x) for x in cmap])
        for i, s in enumerate(seqs):
            if i in dense:  # every state possible, with different weights: no indicator vector, so a dense CLV
                clv = np.ascontiguousarray(0.25 + 0.5 * ((np.arange(self.sites * states) % 7) / 7.0))
                assert lib.pll_set_tip_clv(self.p, i, api.dptr(clv), 0), (lib.errno(), lib.errmsg())
            else:
                assert lib.pll_set_tip_states(self.p, i, self.cmap, s), (lib.errno(), lib.errmsg())
        self.weights = np.ones(self.sites, dtype=np.uint32)
        if pattern_weights is not None:
            self.weights = np.ascontiguousarray(pattern_weights, dtype=np.uint32)
            lib.pll_set_pattern_weights(self.p, api.uptr(self.weights))
        self.pi = np.ascontiguousarray(params_indices if params_indices is not None else np.zeros(rate_cats), dtype=np.uint32)
        if prop_invar > 0.0:
            assert lib.pll_update_invariant_sites(self.p), (lib.errno(), lib.errmsg())
            for m in range(rate_matrices):
                assert lib.pll_update_invariant_sites_proportion(self.p, m, float(prop_invar)), (lib.errno(), lib.errmsg())
        for m in range(rate_matrices):  # (the reference reads whatever eigensystem is stored)
            assert lib.pll_update_eigen(self.p, m), (lib.errno(), lib.errmsg())
        n = self.sites * rate_cats * int(self.part.states_padded)
        raw = np.zeros(n + 8, dtype=np.float64)
        off = (-raw.ctypes.data // 8) % 8
        self._raw, self.sumtable, self._table_used = raw, raw[off:off + n], False

    def close(self):
        if self.p:
            if self.lib.is_amd and self._table_used:  # the handle dies with this array
                self.lib.pll_gpu_release_sumtable(self.p, api.dptr(self.sumtable))
            self.lib.pll_partition_destroy(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def weight_sum(self):
        return int(self.weights.astype(np.int64).sum())

    def eigen(self):
        """(eigenvecs, inv_eigenvecs, eigenvals) per rate matrix, as the partition stores them"""
        S, sp = self.states, int(self.part.states_padded)
        ev = [api.as_np(self.part.eigenvecs[m], S * sp, np.float64).reshape(S, sp)[:, :S].copy() for m in range(len(self.freqs))]
        iev = [api.as_np(self.part.inv_eigenvecs[m], S * sp, np.float64).reshape(S, sp)[:, :S].copy() for m in range(len(self.freqs))]
        lam = [api.as_np(self.part.eigenvals[m], S, np.float64).copy() for m in range(len(self.freqs))]
        return ev, iev, lam

    # ---- the per-pair path every libpll offers: x in the parent (left) role, y in the child (right) role
    def table(self, x, y):
        self._table_used = True
        if not self.lib.pll_update_sumtable(self.p, int(x), int(y), NONE, NONE, api.uptr(self.pi), api.dptr(self.sumtable)):
            raise RuntimeError(f"pll_update_sumtable: [{self.lib.errno()}] {self.lib.errmsg()}")
        return self.sumtable

    def derivatives(self, edge, sumtable, t):
        """(d_f, dd_f) at t on the table of the last table(): the evaluation newton.host_newton drives"""
        d1, d2 = C.c_double(0), C.c_double(0)
        if not self.lib.pll_compute_likelihood_derivatives(self.p, NONE, NONE, float(t), api.uptr(self.pi), api.dptr(sumtable), C.byref(d1),
                                                           C.byref(d2)):
            raise RuntimeError(f"pll_compute_likelihood_derivatives: [{self.lib.errno()}] {self.lib.errmsg()}")
        return d1.value, d2.value

    def pair_derivatives(self, x, y, ts=T_POINTS):
        st = self.table(x, y)
        return [self.derivatives(None, st, t) for t in ts]

    def pair_newton(self, x, y, t_start, t_min, t_max, tolerance, max_iters):
        """the recipe driven with this library's per-pair derivatives: (t, status, trace)"""
        return newton.host_newton(self, None, self.table(x, y), t_start, t_min, t_max, tolerance, max_iters)

    # ---- the call under test
    def distances(self, tips, options, **kw):
        return driver.pairwise_distances(self.lib, self.p, tips, self.pi, options, **kw)

    def launches(self):
        return int(self.lib.pll_gpu_last_launch_count(self.p))


def pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def restated(seqs, cmap, states, weights):
    """pllamd/distances.py's view of the inputs: (codes [tips, sites], masks, weights)"""
    codes, masks = distances.encode(seqs, np.asarray(cmap, dtype=np.uint64), states)
    return codes, masks, np.asarray(weights, dtype=np.int64)


def p_distance_by_sites(seq_a, seq_b, cmap, states, weights):
    """the definition, site by site: (sum of the weights where the two state sets are disjoint, ... where neither is the
    all-states set), as integers"""
    full = (1 << states) - 1
    differ = compared = 0
    for ca, cb, w in zip(seq_a, seq_b, weights):
        ma, mb = int(cmap[ca]), int(cmap[cb])
        if ma & mb == 0:
            differ += int(w)
        if ma != full and mb != full:
            compared += int(w)
    return differ, compared


COUNT_BUDGET = 36 * 1024  # "up to 36 KB of them": the private count tables of a workgroup
LDS_MAX = 158 * 1024      # PLLGPU_DISTANCE_LDS_MAX


def codes_in_use(states, seqs, cmap):
    """C of include/pll_amd_device.h: 16 for 4 states, else a code per distinct state mask that the tips show"""
    if states == 4:
        return 16
    return len(distances.encode(seqs, np.asarray(cmap, dtype=np.uint64), states)[1])


def copies_by_rule(states, rate_cats, ncodes):
    """the count tables a workgroup keeps, by the text of include/pll_amd_device.h: the diag table of 32 R S bytes and at
    least one table of 4 (C^2 | 1) bytes must fit PLLGPU_DISTANCE_LDS_MAX with C <= PLLGPU_DISTANCE_MAX_CODES (else None: the
    call is refused); where there is room 2, 4, ... 256 tables, up to 36 KB of them"""
    diag, table = 32 * rate_cats * states, 4 * ((ncodes * ncodes) | 1)
    if ncodes > MAX_CODES or diag + table > LDS_MAX:
        return None
    room = min(max(COUNT_BUDGET, table), LDS_MAX - diag)
    copies = 1
    while copies < 256 and 2 * copies * table <= room:
        copies *= 2
    return copies


def lds_bytes_by_rule(states, rate_cats, ncodes):
    """dynamic LDS of a launch by the same text: the diag table and copies_by_rule tables (None: refused)"""
    copies = copies_by_rule(states, rate_cats, ncodes)
    return None if copies is None else 32 * rate_cats * states + copies * 4 * ((ncodes * ncodes) | 1)


# ---- inputs with exactly C codes ---------------------------------------------------------------------------------------
def code_masks(states, ncodes, seed=5):
    """ncodes distinct non-empty state masks in increasing order: the singletons (all of them from ncodes >= states on), the
    all-states mask, then random proper subsets of 2 .. states - 1 states"""
    masks = [1 << i for i in range(min(states, ncodes))]
    if ncodes > states:
        masks.append((1 << states) - 1)
    rng = np.random.Generator(np.random.PCG64(seed + 1000 * states + ncodes))
    seen = set(masks)
    while len(masks) < ncodes:
        bits = rng.integers(0, 2, size=states)
        m = sum(1 << i for i in range(states) if bits[i])
        if 2 <= int(bits.sum()) < states and m not in seen:
            seen.add(m)
            masks.append(m)
    return sorted(masks)


def generated(states, ncodes, tips, sites, seed=5):
    """(sequences, charmap, exchangeabilities, frequencies) that show exactly ncodes codes. The character map gives the
    bytes 1 .. ncodes the masks of code_masks in increasing order, so a byte b is code b - 1 under distances.encode (masks in
    increasing order) and under either attribute set of the library (plain: the order in which tip 0 shows them; PATTERN_TIP:
    the order of the bytes). Site s < ncodes of tip x shows byte 1 + (s + rot[x]) % ncodes, rot = 0, ncodes - 1, 1, 2: every
    tip runs through all codes, and the pairs (0, 1) and (0, 2) meet in the corner cells (0, C-1) and (C-1, 0) of the table.
    Site ncodes shows the last code in every tip: the corner (C-1, C-1). The rest are random."""
    assert states != 4 and tips <= 4 and sites > ncodes > 2
    cmap = np.zeros(256, dtype=np.uint64)
    cmap[1:ncodes + 1] = np.array(code_masks(states, ncodes, seed), dtype=np.uint64)
    rng = np.random.Generator(np.random.PCG64(seed + 31 * ncodes + states))
    seqs = []
    for x in range(tips):
        run = 1 + (np.arange(ncodes) + (0, ncodes - 1, 1, 2)[x]) % ncodes
        rest = rng.integers(1, ncodes + 1, size=sites - ncodes - 1)
        seqs.append(np.concatenate([run, [ncodes], rest]).astype(np.uint8).tobytes())
    ex, fr = W.synthetic_exch(states)
    return seqs, cmap, ex, fr


# (shape, codes, sites) of tests/test_gpu_distance_tables.py; four tips, except three at 61 states
TABLE_SHAPES = {"5x3": (5, 3), "20x4": (20, 4), "61x49": (61, 49), "61x50": (61, 50)}
TABLE_CASES = [("5x3", 5, 300), ("5x3", 8, 300), ("20x4", 68, 300), ("20x4", 96, 300), ("20x4", 127, 300), ("20x4", 128, 300),
               ("61x49", 127, 160)]
TABLE_REFUSED = [("61x50", 127, 160), ("20x4", 129, 300)]


def table_tips(shape):
    return 3 if shape.startswith("61") else 4


def table_case(shape, ncodes, sites):
    return generated(TABLE_SHAPES[shape][0], ncodes, table_tips(shape), sites)


class Restated:
    """pllamd/distances.py in the place of a library's per-pair path, on the model of an open Tips (either library: the
    eigensystem is read from the partition) - the expectation where the reference cannot take the input (a byte >= 128)"""
    sumtable = None

    def __init__(self, bed, seqs, cmap):
        self.codes, self.masks, self.w = restated(seqs, cmap, bed.states, bed.weights)
        ev, iev, lam = bed.eigen()
        self.U, self.Wv = distances.code_vectors(self.masks, bed.states, ev, iev, bed.freqs, bed.pi)
        self.model = (lam, bed.rates.copy(), bed.rate_weights.copy(), bed.pi.copy())
        self.states, self.n = bed.states, None

    def table(self, x, y):
        self.n = distances.code_pair_counts(self.codes[x], self.codes[y], self.w, len(self.masks))

    def derivatives(self, edge, sumtable, t):
        return distances.derivatives(self.n, self.U, self.Wv, *self.model, t)

    def pair_derivatives(self, x, y, ts=T_POINTS):
        self.table(x, y)
        return [self.derivatives(None, None, t) for t in ts]

    def pair_newton(self, x, y, t_start, t_min, t_max, tolerance, max_iters):
        self.table(x, y)
        return newton.host_newton(self, None, None, t_start, t_min, t_max, tolerance, max_iters)

    def p_distance(self, x, y):
        self.table(x, y)
        return distances.p_distance(self.n, self.masks, self.states)


WEIGHT_SITES, HEAVY, SECOND = 1027, 5, 700


def weights_case(states):
    """(sequences, charmap, exchangeabilities, frequencies, weights) of four tips at 1027 sites whose weights add up to
    2^32 - 1: arange % 4, site 5 = 2^31, site 700 = the rest; tips 0 and 1 show at site 700 what they show at site 5, so that
    one cell of their table counts more than 2^31, from two threads (quads 1 and 175) with different private tables"""
    seqs, cmap, exch, freqs = sequences(states, 4, WEIGHT_SITES)
    seqs = [bytearray(s) for s in seqs]
    for x in (0, 1):
        seqs[x][SECOND] = seqs[x][HEAVY]
    w = np.arange(WEIGHT_SITES, dtype=np.int64) % 4
    w[HEAVY], w[SECOND] = 1 << 31, 0
    w[SECOND] = (1 << 32) - 1 - int(w.sum())
    return [bytes(s) for s in seqs], cmap, exch, freqs, w.astype(np.uint32)


def launches_by_rule(count, max_pairs=MAX_PAIRS):
    """the cutting rule of include/pll_amd_device.h, pllgpu_pairwise_distances: one launch for the code vectors, then whole
    rows of the pair matrix"""
    if count < 2:
        return 0
    rows = max(1, min(65535, max_pairs // count))
    return 1 + (count - 1 + rows - 1) // rows
