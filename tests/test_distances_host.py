"""CPU (no GPU): pll_gpu_pairwise_distances is declared, exported and bound, and everything it decides before a device is
needed - the checks, the refusals in their stated order (a doubly wrong input reports the earlier fault), the answer of a
partition with no device behind it - on host-only partitions (PLL_AMD_HOST_ONLY=1); a failed call leaves every output as it
found it. And pllamd/distances.py, the numpy restatement of one pair, against the reference: counts -> (d_f, dd_f) equal
the reference's pll_update_sumtable on the two tips + pll_compute_likelihood_derivatives within gradient_cases.close
(1e-10 |exp| + 4e-15 W, W = the weight sum); its p-distance equals a direct per-site loop exactly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distance_cases as DC
import gradient_cases as GC
from pllamd import api, distances, driver, workload as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.5
TIPS, SITES = 5, 20
SEQ = [b"ACGTACGTACGTACGTACGT", b"ACGTACGAACGTRCGTACGT", b"ACGTTCGTAC-TACGTACGT", b"ACCTACGTACGTACGTANGT", b"ACGTACGTACGTACGTACGA"]
GOOD = dict(t_start=0.1, t_min=1e-6, t_max=100.0, tolerance=1e-6, max_iters=32, matrix_index=-1)


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


def _tips(lib, attrs=0, states=4, rate_cats=4, **kw):
    if states == 4:
        return DC.Tips(lib, 4, rate_cats, SEQ, W.map_nt(), W.GTR_DNA["exch"], W.GTR_DNA["freqs"], attrs=attrs, **kw)
    seqs, cmap, exch, freqs = DC.sequences(states, TIPS, SITES)
    return DC.Tips(lib, states, rate_cats, seqs, cmap, exch, freqs, attrs=attrs, **kw)


def _refused(lib, code, attrs=0, tips=(0, 1, 2, 3, 4), pi=None, options=None, make=None, **kw):
    with (make(lib) if make else _tips(lib, attrs, **kw)) as b:
        if pi is not None:
            b.pi = np.ascontiguousarray(pi, dtype=np.uint32)
        with pytest.raises(RuntimeError) as err:
            b.distances(tips, driver.newton_options(**dict(GOOD, **(options or {}))), fill=SENTINEL)
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        for name, a in err.value.outputs.items():
            assert (a == np.array(SENTINEL).astype(a.dtype)).all(), name
        return str(err.value)


def test_symbol_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    assert re.search(r"\bint pll_gpu_pairwise_distances\(", hdr) and re.search(r"\}\s*pll_gpu_distances_t;", hdr)
    assert getattr(amd_lib.dll, "pll_gpu_pairwise_distances")
    assert len(amd_lib.pll_gpu_pairwise_distances.argtypes) == 6
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    assert re.search(r"\bint pllgpu_pairwise_distances\(", dev) and getattr(amd_lib.dll, "pllgpu_pairwise_distances")
    assert re.search(r"#define PLLGPU_DISTANCE_MAX_CODES %d\b" % DC.MAX_CODES, dev)
    assert re.search(r"#define PLLGPU_DISTANCE_MAX_PAIRS \(1u << 20\)", dev) and DC.MAX_PAIRS == 1 << 20
    assert DC.MAX_CODES >= 64  # what a 61-state alignment with ambiguity codes produces must be served


def test_the_struct_mirror():
    assert C.sizeof(api.Distances) == 48
    assert [getattr(api.Distances, f).offset for f in driver.DISTANCE_OUTPUTS] == [0, 8, 16, 24, 32, 40]
    abi = open(os.path.join(ROOT, "libpll-2_amd", "csrc", "host", "abi_check.c")).read()
    assert "sizeof(pll_gpu_distances_t) == 48" in abi and "AT(pll_gpu_distances_t, iterations, 40)" in abi


@pytest.mark.parametrize("which", ["partition", "out", "distance", "tips", "params_indices", "options"])
def test_each_null_argument(amd_lib, which):
    with _tips(amd_lib) as b:
        d = np.full((TIPS, TIPS), SENTINEL)
        tips = np.arange(TIPS, dtype=np.uint32)
        rec = api.Distances(distance=None if which == "distance" else api.dptr(d))
        opt = driver.newton_options(**GOOD)
        args = {"partition": b.p, "tips": api.uptr(tips), "params_indices": api.uptr(b.pi), "options": C.byref(opt), "out": C.byref(rec)}
        if which in args:
            args[which] = None
        assert amd_lib.pll_gpu_pairwise_distances(args["partition"], args["tips"], TIPS, args["params_indices"], args["options"], args["out"]) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
        assert (d == SENTINEL).all()


def test_only_distance_is_mandatory(amd_lib):
    """the other five may be NULL: the call gets as far as the missing device"""
    with _tips(amd_lib) as b:
        with pytest.raises(RuntimeError) as err:
            b.distances(range(TIPS), driver.newton_options(**GOOD), want=(), fill=SENTINEL)
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE and list(err.value.outputs) == ["distance"]


BAD_OPTIONS = {
    "negative t_min": dict(t_min=-1e-3),
    "t_min above t_max": dict(t_min=2.0, t_max=1.0),
    "infinite t_max": dict(t_max=float("inf")),
    "nan t_start": dict(t_start=float("nan")),
    "zero tolerance": dict(tolerance=0.0),
    "nan tolerance": dict(tolerance=float("nan")),
    "no iteration": dict(max_iters=0),
    "too many iterations": dict(max_iters=api.NEWTON_MAX_ITERS + 1),
    "a matrix slot": dict(matrix_index=0),
    "matrix_index below -1": dict(matrix_index=-2),
}


@pytest.mark.parametrize("what", list(BAD_OPTIONS))
def test_options_out_of_range(amd_lib, what):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, options=BAD_OPTIONS[what])


def test_a_tip_index_out_of_range_anywhere_in_the_list(amd_lib):
    for tips in ((TIPS, 1, 2), (0, TIPS, 2), (0, 1, 0xFFFFFFFF)):
        assert "is no tip" in _refused(amd_lib, api.ERROR_PARAM_INVALID, tips=tips)


def test_params_indices_out_of_range(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, pi=[0, 0, 1, 0])


def test_a_dense_tip_is_refused(amd_lib):
    assert "not given by codes" in _refused(amd_lib, api.ERROR_PARAM_INVALID, dense=(3,))


def test_a_partition_without_tip_codes_is_refused(amd_lib, monkeypatch):
    monkeypatch.setenv("PLL_AMD_NO_TIP_CODES", "1")
    assert "not given by codes" in _refused(amd_lib, api.ERROR_PARAM_INVALID)


UNSUPPORTED = {"site_repeats": api.SITE_REPEATS, "asc_bias_lewis": api.AB_FLAG | api.AB_LEWIS,
               "asc_bias_stamatakis": api.AB_FLAG | api.AB_STAMATAKIS}


@pytest.mark.parametrize("attrs", list(UNSUPPORTED.values()), ids=list(UNSUPPORTED))
def test_unsupported_partitions_are_refused(amd_lib, attrs):
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=attrs)


def test_invariant_sites_are_refused(amd_lib):
    assert "prop_invar" in _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, prop_invar=0.2)


def _many_codes(lib, attrs=api.PATTERN_TIP):
    """20 states under a character map of 200 distinct state sets: more codes than a workgroup's table may hold"""
    cmap = np.zeros(256, dtype=np.uint64)
    cmap[1:201] = np.arange(1, 201, dtype=np.uint64)
    seq = bytes(range(1, 201))
    ex, fr = W.synthetic_exch(20)
    return DC.Tips(lib, 20, 4, [seq, seq[::-1], seq], cmap, ex, fr, attrs=attrs)


@pytest.mark.parametrize("attrs", [api.PATTERN_TIP, 0], ids=["pattern_tip", "plain"])
def test_an_over_long_code_table_is_refused(amd_lib, attrs):
    assert "tip codes" in _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, tips=(0, 1, 2), make=lambda lib: _many_codes(lib, attrs))


def test_a_weight_sum_beyond_32_bits_is_refused(amd_lib):
    w = np.ones(SITES, dtype=np.uint32)
    w[3] = w[11] = 1 << 31
    assert "add up" in _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, pattern_weights=w)


def test_the_order_of_the_checks(amd_lib):
    """a doubly wrong input reports the earlier fault"""
    inv, uns = api.ERROR_PARAM_INVALID, api.ERROR_GPU_UNSUPPORTED
    w = np.ones(SITES, dtype=np.uint32)
    w[0] = w[1] = 1 << 31
    assert "is no tip" in _refused(amd_lib, inv, tips=(0, TIPS), options=dict(max_iters=0))
    assert "options" in _refused(amd_lib, inv, options=dict(tolerance=-1.0, matrix_index=3))
    assert "matrix_index" in _refused(amd_lib, inv, options=dict(matrix_index=0), pi=[0, 0, 0, 7])
    assert "params_indices" in _refused(amd_lib, inv, pi=[0, 0, 0, 7], dense=(1,))
    assert "not given by codes" in _refused(amd_lib, inv, dense=(1,), attrs=api.AB_FLAG | api.AB_LEWIS)
    assert "not given by codes" in _refused(amd_lib, inv, dense=(1,), prop_invar=0.1)
    _refused(amd_lib, inv, attrs=api.SITE_REPEATS, options=dict(t_min=-1.0))
    assert "SITE_REPEATS" in _refused(amd_lib, uns, attrs=api.SITE_REPEATS, prop_invar=0.1)
    assert "ascertainment" in _refused(amd_lib, uns, attrs=api.AB_FLAG | api.AB_LEWIS, pattern_weights=w)
    assert "prop_invar" in _refused(amd_lib, uns, prop_invar=0.1, pattern_weights=w)
    assert "tip codes" in _refused(amd_lib, uns, tips=(0, 1, 2), make=lambda lib: _with_weights(_many_codes(lib), 1 << 31))


def _with_weights(bed, value):
    w = np.full(bed.sites, value, dtype=np.uint32)
    bed.lib.pll_set_pattern_weights(bed.p, api.uptr(w))
    return bed


def test_a_refusal_comes_before_the_missing_device(amd_lib):
    """host-only partitions have no device either: UNSUPPORTED, not UNAVAILABLE"""
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, prop_invar=0.3)


@pytest.mark.parametrize("count", [1, 2, TIPS])
def test_host_only_partition_is_refused_and_the_outputs_untouched(amd_lib, capfd, count):
    """no device: PLL_ERROR_GPU_UNAVAILABLE, for one tip as for many"""
    _refused(amd_lib, api.ERROR_GPU_UNAVAILABLE, tips=tuple(range(count)))
    assert "pll_gpu_pairwise_distances" in capfd.readouterr().err  # the usual line on stderr


def test_zero_count_succeeds_and_reads_nothing(amd_lib):
    with _tips(amd_lib) as b:
        d = np.full(4, SENTINEL)
        rec = api.Distances(distance=api.dptr(d))
        assert amd_lib.pll_gpu_pairwise_distances(b.p, None, 0, None, None, C.byref(rec)) == 1
        assert (d == SENTINEL).all()
        assert amd_lib.pll_gpu_pairwise_distances(b.p, None, 0, None, None, None) == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID


# ---- the edges of the count tables: the rule restated, and conditions on the inputs of test_gpu_distance_tables.py --------
def test_the_header_still_states_the_rule():
    dev = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "pll_amd_device.h")).read())
    assert "PLLGPU_DISTANCE_LDS_BYTES = 32 R states + 4 (C^2 | 1) <= PLLGPU_DISTANCE_LDS_MAX" in dev
    assert "a workgroup keeps 2, 4, ... 256 such tables, up to 36 KB of them" in dev and DC.COUNT_BUDGET == 36 * 1024
    assert re.search(r"#define PLLGPU_DISTANCE_LDS_MAX \(158ul \* 1024ul\)", dev) and DC.LDS_MAX == 158 * 1024
    assert re.search(r"#define PLLGPU_DISTANCE_LDS_BYTES\(S, R, C\) \(32ul \* \(R\) \* \(S\) \+ 4ul \* \(\(\(C\) \* \(C\)\) \| 1ul\)\)", dev)
    hip = open(os.path.join(ROOT, "libpll-2_amd", "csrc", "hip", "pllgpu.hip")).read()
    assert "constexpr size_t kDistCountBytes = 36 * 1024;" in hip
    # the figures the issue of these tests was written with
    assert DC.lds_bytes_by_rule(20, 4, 127) == 67076 and DC.lds_bytes_by_rule(61, 49, 127) == 160164 <= DC.LDS_MAX == 161792
    assert DC.copies_by_rule(61, 50, 127) is None and DC.copies_by_rule(20, 4, 129) is None
    assert [DC.copies_by_rule(20, 4, c) for c in (67, 68, 95, 96, 128)] == [2, 1, 1, 1, 1]
    assert 4 * ((95 * 95) | 1) <= DC.COUNT_BUDGET < 4 * ((96 * 96) | 1)


@pytest.mark.parametrize("shape,ncodes,sites", DC.TABLE_CASES + DC.TABLE_REFUSED)
def test_the_generated_inputs_show_exactly_their_codes(shape, ncodes, sites):
    """exactly C codes, a byte b being code b - 1; some pair has a count in each corner cell of the table"""
    states = DC.TABLE_SHAPES[shape][0]
    seqs, cmap, _, _ = DC.table_case(shape, ncodes, sites)
    tips = DC.table_tips(shape)
    assert len(seqs) == tips and all(len(s) == sites for s in seqs) and sites <= 300
    codes, masks, w = DC.restated(seqs, cmap, states, np.ones(sites))
    assert len(masks) == ncodes == DC.codes_in_use(states, seqs, cmap) and (np.diff(masks.astype(object)) > 0).all()
    assert all((codes[x] == np.frombuffer(seqs[x], dtype=np.uint8) - 1).all() for x in range(tips))
    assert all(set(codes[x][:ncodes]) == set(range(ncodes)) for x in range(tips))
    assert sum(int(m) & (int(m) - 1) == 0 for m in masks) == min(states, ncodes)
    assert ((1 << states) - 1 in [int(m) for m in masks]) == (ncodes > states)
    corners = {(0, ncodes - 1): False, (ncodes - 1, 0): False, (ncodes - 1, ncodes - 1): False}
    for x, y in DC.pairs(tips):
        n = distances.code_pair_counts(codes[x], codes[y], w, ncodes)
        for cell in corners:
            corners[cell] |= bool(n[cell] > 0)
    assert all(corners.values()), corners


@pytest.mark.parametrize("shape,ncodes,sites", [c for c in DC.TABLE_CASES + DC.TABLE_REFUSED if c[1] <= 127])
def test_the_restatement_against_the_reference_at_the_table_edges(ref_lib, shape, ncodes, sites):
    """(a byte >= 128 cannot go through the reference, which indexes its character map with a signed char)"""
    states, rate_cats = DC.TABLE_SHAPES[shape]
    seqs, cmap, exch, freqs = DC.table_case(shape, ncodes, sites)
    codes, masks, w = DC.restated(seqs, cmap, states, np.ones(sites))
    with DC.Tips(ref_lib, states, rate_cats, seqs, cmap, exch, freqs) as b:
        ev, iev, lam = b.eigen()
        U, Wv = distances.code_vectors(masks, states, ev, iev, b.freqs, b.pi)
        worst = 0.0
        for x, y in DC.pairs(len(seqs)):
            n = distances.code_pair_counts(codes[x], codes[y], w, ncodes)
            exp = np.array(b.pair_derivatives(x, y))
            got = np.array([distances.derivatives(n, U, Wv, lam, b.rates, b.rate_weights, b.pi, t) for t in DC.T_POINTS])
            worst = max(worst, GC.worst(got, exp, sites))
            assert GC.close(got, exp, sites), (shape, ncodes, x, y, GC.worst(got, exp, sites))
    print(f"{shape} {ncodes} codes: the restatement's worst deviation is {worst:.3f} of the bound")


def _generated_tips(shape, ncodes, sites, attrs):
    states, rate_cats = DC.TABLE_SHAPES[shape]
    return lambda lib: DC.Tips(lib, states, rate_cats, *DC.table_case(shape, ncodes, sites), attrs=attrs)


@pytest.mark.parametrize("attrs", [api.PATTERN_TIP, 0], ids=["pattern_tip", "plain"])
def test_the_limits_of_the_code_table_on_the_host(amd_lib, attrs):
    """128 codes, and 61 x 49 at 127 codes, get as far as the missing device; 129 codes and 61 x 50 at 127 codes are refused"""
    tips = (0, 1, 2)
    for shape, ncodes, sites in (("20x4", 127, 300), ("20x4", 128, 300), ("61x49", 127, 160)):
        _refused(amd_lib, api.ERROR_GPU_UNAVAILABLE, tips=tips, make=_generated_tips(shape, ncodes, sites, attrs))
    for shape, ncodes, sites in DC.TABLE_REFUSED:
        assert "tip codes" in _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, tips=tips, make=_generated_tips(shape, ncodes, sites, attrs))


def test_every_size_class_of_the_count_tables_is_run():
    """copies_by_rule over all cases of both GPU files: every number of tables the code can choose with these alphabets,
    and dynamic LDS on both sides of 64 KB; a changed constant cannot silently move a case out of its class"""
    import test_gpu_distances as old
    classes, lds = set(), set()
    for shape, tips, sites in {(c[0], c[2], c[3]) for c in old.CASES}:
        states, rate_cats = old.SHAPES[shape]
        seqs, cmap, _, _ = DC.sequences(states, tips, sites)
        ncodes = DC.codes_in_use(states, seqs, cmap)
        classes.add(DC.copies_by_rule(states, rate_cats, ncodes))
        lds.add(DC.lds_bytes_by_rule(states, rate_cats, ncodes))
    assert classes >= {2, 8, 32, 64} and max(lds) <= 64 * 1024
    by_case = {c: DC.copies_by_rule(*DC.TABLE_SHAPES[c[0]], c[1]) for c in DC.TABLE_CASES}
    assert by_case[("5x3", 5, 300)] == 256 and by_case[("5x3", 8, 300)] == 128
    assert all(by_case[c] == 1 for c in DC.TABLE_CASES if c[1] >= 68)
    assert classes | set(by_case.values()) >= {1, 2, 8, 32, 64, 128, 256}
    for shape, ncodes, _ in DC.TABLE_CASES:
        over = DC.lds_bytes_by_rule(*DC.TABLE_SHAPES[shape], ncodes) > 64 * 1024
        assert over == (ncodes >= 127), (shape, ncodes)
    assert DC.lds_bytes_by_rule(20, 4, 96) <= 64 * 1024 < DC.lds_bytes_by_rule(20, 4, 127)
    # both sides of the 158 KB limit
    assert DC.lds_bytes_by_rule(61, 49, 127) <= DC.LDS_MAX and all(DC.copies_by_rule(*DC.TABLE_SHAPES[s], c) is None for s, c, _ in DC.TABLE_REFUSED)
    assert 32 * 50 * 61 + 4 * ((127 * 127) | 1) > DC.LDS_MAX


@pytest.mark.parametrize("states,rate_cats", [(4, 4), (20, 4)])
def test_the_heavy_weights_meet_in_one_cell_from_two_tables(ref_lib, states, rate_cats):
    """conditions on distance_cases.weights_case: the weights add up to 2^32 - 1 (2^32 is refused), the pair (0, 1) has a cell
    above 2^31 whose two heavy sites lie in the quads of two threads with different private tables - and with W = 2^32 - 1
    the restatement stays within gradient_cases.close of the reference"""
    seqs, cmap, exch, freqs, weights = DC.weights_case(states)
    assert weights.dtype == np.uint32 and int(weights.astype(np.int64).sum()) == (1 << 32) - 1
    assert int(weights[DC.HEAVY]) == 1 << 31 and int(weights[DC.SECOND]) == 2147482109
    codes, masks, w = DC.restated(seqs, cmap, states, weights)
    n = distances.code_pair_counts(codes[0], codes[1], w, len(masks))
    cell = (codes[0][DC.HEAVY], codes[1][DC.HEAVY])
    assert cell == (codes[0][DC.SECOND], codes[1][DC.SECOND]) and int(n[cell]) > 1 << 31
    copies = DC.copies_by_rule(states, rate_cats, DC.codes_in_use(states, seqs, cmap))
    assert copies > 1 and (DC.HEAVY // 4) % copies != (DC.SECOND // 4) % copies and DC.SECOND // 4 < 256 <= DC.WEIGHT_SITES // 4
    with DC.Tips(ref_lib, states, rate_cats, seqs, cmap, exch, freqs, pattern_weights=weights) as b:
        r = DC.Restated(b, seqs, cmap)
        for x, y in DC.pairs(4):
            exp, got = np.array(b.pair_derivatives(x, y)), np.array(r.pair_derivatives(x, y))
            assert GC.close(got, exp, b.weight_sum), (x, y, GC.worst(got, exp, b.weight_sum))
            differ, compared = DC.p_distance_by_sites(seqs[x], seqs[y], cmap, states, weights)
            assert r.p_distance(x, y) == differ / compared


# ---- pllamd/distances.py against the reference -------------------------------------------------------------------
SHAPES ={"4x4": (4, 4), "5x3": (5, 3), "20x4": (20, 4)}
REF_TIPS, REF_SITES = 6, 130


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_restatement_against_the_reference(ref_lib, shape):
    states, rate_cats = SHAPES[shape]
    seqs, cmap, exch, freqs = DC.sequences(states, REF_TIPS, REF_SITES)
    weights = np.arange(REF_SITES, dtype=np.uint32) % 4
    codes, masks, w = DC.restated(seqs, cmap, states, weights)
    with DC.Tips(ref_lib, states, rate_cats, seqs, cmap, exch, freqs, pattern_weights=weights) as b:
        ev, iev, lam = b.eigen()
        U, Wv = distances.code_vectors(masks, states, ev, iev, b.freqs, b.pi)
        worst = 0.0
        for x, y in DC.pairs(REF_TIPS):
            n = distances.code_pair_counts(codes[x], codes[y], w, len(masks))
            assert int(n.sum()) == b.weight_sum
            exp = np.array(b.pair_derivatives(x, y))
            got = np.array([distances.derivatives(n, U, Wv, lam, b.rates, b.rate_weights, b.pi, t) for t in DC.T_POINTS])
            worst = max(worst, GC.worst(got, exp, b.weight_sum))
            assert GC.close(got, exp, b.weight_sum), (shape, x, y, GC.worst(got, exp, b.weight_sum))
            differ, compared = DC.p_distance_by_sites(seqs[x], seqs[y], cmap, states, weights)
            assert compared > 0 and distances.p_distance(n, masks, states) == differ / compared
    print(f"{shape}: the restatement's worst deviation is {worst:.3f} of the bound")


def test_the_p_distance_of_nothing_comparable_is_zero():
    masks = np.arange(16, dtype=np.uint64)
    n = np.zeros((16, 16), dtype=np.int64)
    n[15, 3] = n[2, 15] = 7
    assert distances.p_distance(n, masks, 4) == 0.0
    n[1, 2], n[1, 3], n[4, 4] = 2, 5, 3  # disjoint, overlapping, equal
    assert distances.p_distance(n, masks, 4) == 2 / 10


def test_the_restated_iteration_stops_where_the_slope_is_small(ref_lib):
    """distances.ml_distance drives newton.Bracket on a count table: same status and trace length as the recipe driven with the
    reference's own derivatives, and the reference's slope at its answer is within twice the tolerance"""
    states, rate_cats = 4, 4
    seqs, cmap, exch, freqs = DC.sequences(states, 3, REF_SITES)
    codes, masks, w = DC.restated(seqs, cmap, states, np.ones(REF_SITES))
    with DC.Tips(ref_lib, states, rate_cats, seqs, cmap, exch, freqs) as b:
        ev, iev, lam = b.eigen()
        U, Wv = distances.code_vectors(masks, states, ev, iev, b.freqs, b.pi)
        tol = 1e-8 * REF_SITES
        for x, y in DC.pairs(3):
            n = distances.code_pair_counts(codes[x], codes[y], w, len(masks))
            t, status, trace = distances.ml_distance(n, U, Wv, lam, b.rates, b.rate_weights, b.pi, 0.1, 1e-6, 100.0, tol, 32)
            t_ref, status_ref, trace_ref = b.pair_newton(x, y, 0.1, 1e-6, 100.0, tol, 32)
            assert status == status_ref == api.NEWTON_CONVERGED and abs(len(trace) - len(trace_ref)) <= 1
            assert abs(b.derivatives(None, b.table(x, y), t)[0]) <= 2 * tol
