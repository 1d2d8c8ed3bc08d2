"""GPU: pll_gpu_draw_replicate_weights and pll_gpu_quartet_rell_loglikelihoods.

The rows the device draws are held to pllamd/rell.py - the definition of DESIGN.md section 5.11 in integer arithmetic - bit
for bit; the log-likelihoods under them to pll_gpu_quartet_resampled_loglikelihoods with the same rows uploaded, bit for
bit, and to the reference within compare.RTOL for every value, as tests/test_gpu_quartet_resample.py holds that call.
Shapes, trees, helpers and the reference values are that file's and test_gpu_quartets' (shared, computed once)."""
import numpy as np
import pytest

import insertion_cases as IC
import quartet_cases as QC
import resample_cases as RC
import test_gpu_quartet_resample as RQ
from compare import RTOL
from pllamd import api, driver, rell

pytestmark = pytest.mark.gpu

SHAPES = RQ.SHAPES
SEED = 0x9E3779B97F4A7C15


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    RQ._REF = ref_lib


def own_weights(sites):
    """OWN_WEIGHTS-style weights 1..5 with every sixth site (3, 9, ...) of weight 0"""
    return tuple(int(1 + (7 * n) % 5) if n % 6 != 3 else 0 for n in range(sites))


def _rell(bed, rows, replicates, seed=SEED, want_persite=True, want_weights=True):
    return driver.quartet_rell_loglikelihoods(bed.lib, bed.p, rows, bed.fi, seed, replicates, want_persite, want_weights)


def _same(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _check_rows(amd_lib, sites, kind):
    p = own_weights(sites) if kind == "own" else (1,) * sites
    kw = dict(pattern_weights=p) if kind == "own" else {}
    with RQ._bed(amd_lib, (4, 4, 20, sites), 0, **kw) as b:
        for first, replicates in ((0, 1), (3, 17), (0, 100)):
            got = driver.draw_replicate_weights(amd_lib, b.p, SEED, first, replicates)
            exp = rell.replicate_weights(p, SEED, first, replicates)
            assert got.shape == exp.shape and got.dtype == exp.dtype
            assert got.tobytes() == exp.tobytes(), (sites, kind, first, replicates, np.argwhere(got != exp)[:4].tolist())
            assert (got.sum(axis=1, dtype=np.uint64) == sum(p)).all()
            if sites >= 64 and kind == "ones":  # the input condition resample_cases.weights asserts
                assert (got.min(axis=1) == 0).all() and (got.max(axis=1) >= 2).all()
            if kind == "own":
                assert (got[:, np.array(p) == 0] == 0).all()


@pytest.mark.parametrize("kind", ["ones", "own"])
@pytest.mark.parametrize("sites", [1, 3, 63, 64, 65, 257, 2500])
def test_the_device_draws_the_definition(amd_lib, sites, kind):
    """site counts around the 4-word row padding and the 64-site tile, one and several draws per thread; 1, 17 and 100
    rows from different first rows; every weight 1 (the site is r itself) and weights 0..5 (the search over the cdf)"""
    _check_rows(amd_lib, sites, kind)


@pytest.mark.parametrize("kind", ["ones", "own"])
@pytest.mark.parametrize("sites", [65, 257, 2500])
def test_the_device_draws_the_definition_over_several_ranges(amd_lib, monkeypatch, sites, kind):
    """PLL_AMD_RELL_RANGE=64: 2, 5 and 40 workgroups per row, the last one short (1, 1 and 4 sites)"""
    monkeypatch.setenv("PLL_AMD_RELL_RANGE", "64")
    _check_rows(amd_lib, sites, kind)


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_same_bits_as_the_uploaded_rows(amd_lib, shape):
    dims = SHAPES[shape]
    with RQ._bed(amd_lib, dims, 0) as b:
        rows = RQ._rows(b)
        lnl, res, per, w = _rell(b, rows, 17)
        assert w.tobytes() == rell.replicate_weights([1] * dims[3], SEED, 0, 17).tobytes()
        assert _same((lnl, res, per), RC.call(b, rows, w))
        assert lnl.tobytes() == QC.batched(b, rows).tobytes()


@pytest.mark.parametrize("shape,attrs", RQ.EVERY_EDGE)
def test_every_inner_edge_against_the_reference(amd_lib, shape, attrs):
    dims = SHAPES[shape]
    lnl_exp, u_exp, _ = RQ._reference(dims, RQ.ATTRS[attrs])
    with RQ._bed(amd_lib, dims, RQ.ATTRS[attrs]) as b:
        lnl, res, per, w = _rell(b, RQ._rows(b), 17)
    assert w.tobytes() == rell.replicate_weights([1] * dims[3], SEED, 0, 17).tobytes()
    exp = RC.resampled_from(u_exp, w)
    print(f"{shape} {attrs}: lnl worst {IC.worst(lnl, lnl_exp):.2e}, resampled worst {IC.worst(res, exp):.2e}, persite worst {IC.worst(per, u_exp):.2e}")
    RQ._check_all((lnl, res, per), lnl_exp, u_exp, w, f"{shape} {attrs}")


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_chunks_change_no_bit(amd_lib, monkeypatch, shape):
    """the cut of tests/test_gpu_quartet_resample.py - 20000 bytes of scratch, 17 quartets x 65 sites x 40 replicates: 9 quartet
    chunks, 2 replicate chunks - changes no output, the returned weights included; a draw launch per replicate chunk"""
    states, rate_cats = SHAPES[shape][:2]
    dims = (states, rate_cats, 20, 65)
    with RQ._bed(amd_lib, dims, 0) as b:
        rows = RQ._rows(b)
        whole = _rell(b, rows, 40)  # (launches the prefix sums and what the upward operations held back as well)
        assert _same(_rell(b, rows, 40), whole)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 4  # the draw, the quartets, the contraction, its reduction
    assert whole[3].tobytes() == rell.replicate_weights([1] * 65, SEED, 0, 40).tobytes()
    monkeypatch.setenv("PLL_AMD_RESAMPLE_SCRATCH", "20000")
    with RQ._bed(amd_lib, dims, 0) as b:
        rows = RQ._rows(b)
        assert _same(_rell(b, rows, 40), whole)
        assert _same(_rell(b, rows, 40), whole)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        assert launches == 2 * (1 + 9 * 3), launches
        sums_only = _rell(b, rows, 40, want_persite=False, want_weights=False)
        assert sums_only[1].tobytes() == whole[1].tobytes() and sums_only[2] is None and sums_only[3] is None
        # ... and the rows alone, cut by the same scratch (20000 // (4 * 68) = 73 rows per chunk)
        alone = driver.draw_replicate_weights(amd_lib, b.p, SEED, 0, 100)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 2
        assert alone.tobytes() == rell.replicate_weights([1] * 65, SEED, 0, 100).tobytes()


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_values_are_independent(amd_lib, shape):
    dims = SHAPES[shape]
    with RQ._bed(amd_lib, dims, 0) as b:
        rows = RQ._rows(b)[:40]
        whole = _rell(b, rows, 17)
        assert _same(_rell(b, rows, 17), whole)
        for k in (0, 9, 16):
            assert driver.draw_replicate_weights(amd_lib, b.p, SEED, k, 1).tobytes() == whole[3][k:k + 1].tobytes(), k
        fewer = _rell(b, rows, 5)
        assert fewer[3].tobytes() == whole[3][:5].tobytes() and fewer[1].tobytes() == np.ascontiguousarray(whole[1][:, :5]).tobytes()
        perm = np.random.Generator(np.random.PCG64(3)).permutation(len(rows))
        shuffled = _rell(b, [rows[i] for i in perm], 17)
        assert all(x.tobytes() == y[perm].tobytes() for x, y in zip(shuffled[:3], whole[:3]))
        assert shuffled[3].tobytes() == whole[3].tobytes()
        other = _rell(b, rows, 17, seed=SEED + 1)
        assert all(x.tobytes() != y.tobytes() for x, y in zip(other[3], whole[3])), "the seed does not show"
        assert other[0].tobytes() == whole[0].tobytes()
        lnl0, res0, per0, w0 = _rell(b, rows, 0)
        assert res0 is None and w0 is None and per0.tobytes() == whole[2].tobytes() and lnl0.tobytes() == whole[0].tobytes()
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 1


def test_weights_follow_the_partition(amd_lib):
    """after pll_set_pattern_weights the next draw uses the new weights (total changes: 130 -> 343 -> 130)"""
    dims = RQ.SMALL["4x4"]
    sites = dims[3]
    new = np.array(own_weights(sites), dtype=np.uint32)
    assert int(new.sum()) != sites
    with RQ._bed(amd_lib, dims, 0) as b:
        rows = RQ._rows(b)
        first = _rell(b, rows, 5)
        assert first[3].tobytes() == rell.replicate_weights([1] * sites, SEED, 0, 5).tobytes()
        amd_lib.pll_set_pattern_weights(b.p, api.uptr(new))
        got = driver.draw_replicate_weights(amd_lib, b.p, SEED, 0, 5)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 2  # the prefix sums again, the draw
        assert got.tobytes() == rell.replicate_weights(new, SEED, 0, 5).tobytes()
        assert (got.sum(axis=1) == new.sum()).all()
        second = _rell(b, rows, 5)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 4  # (kept: no upload since)
        assert second[3].tobytes() == got.tobytes()
        assert _same(second[:3], RC.call(b, rows, got))
        assert second[1].tobytes() != first[1].tobytes()
        amd_lib.pll_set_pattern_weights(b.p, api.uptr(np.ones(sites, dtype=np.uint32)))
        assert _same(_rell(b, rows, 5), first)


def test_a_sum_out_of_range_is_refused(amd_lib):
    """total == 0 and total >= 2^32: PARAM_INVALID from both calls, outputs untouched; replicates == 0 does not ask"""
    dims = RQ.SMALL["4x4"]
    sites = dims[3]
    for p in (np.zeros(sites, dtype=np.uint32), np.array([2 ** 31, 2 ** 31] + [0] * (sites - 2), dtype=np.uint32)):
        with RQ._bed(amd_lib, dims, 0, pattern_weights=p) as b:
            rows = RQ._rows(b)
            w = np.full((3, sites), 7, dtype=np.uint32)
            assert amd_lib.pll_gpu_draw_replicate_weights(b.p, SEED, 0, 3, api.uptr(w)) == 0
            assert amd_lib.errno() == api.ERROR_PARAM_INVALID and (w == 7).all()
            lnl, res = np.full((len(rows), 3), -1.5), np.full((len(rows), 3, 3), -1.5)
            fi = np.ascontiguousarray(b.fi, dtype=np.uint32)
            assert amd_lib.pll_gpu_quartet_rell_loglikelihoods(b.p, api.make_quartets(rows), len(rows), api.uptr(fi), SEED, 3, api.dptr(lnl),
                                                               api.dptr(res), None, api.uptr(w)) == 0
            assert amd_lib.errno() == api.ERROR_PARAM_INVALID and (w == 7).all() and (lnl == -1.5).all() and (res == -1.5).all()
            assert _rell(b, rows, 0, want_persite=False)[0].tobytes() == QC.batched(b, rows).tobytes()


def test_nothing_is_written(amd_lib):
    """tests/test_gpu_quartet_resample.py's test with the rell call: CLVs and scalers of nodes the list names and of a spare
    slot it does not name are byte-identical after the call, the partition's pattern weights are what they were, and the
    operation list of before still replays"""
    dims = SHAPES["4x4"]
    own = tuple(int(x) for x in 1 + (np.arange(dims[3]) * 7) % 5)
    with RQ._bed(amd_lib, dims, 0, pattern_weights=own) as b:
        lay = b.lay
        b.query_cherry(lay.T, lay.T + 1)  # the spare slot the list does not name
        b.update(lay.full_ops())
        up_ops, slot = lay.upward()
        rows = QC.quartet_rows(lay, slot)
        b.update(up_ops)
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1  # (the control: the list does replay when nothing happens)
        inner_ends = [(e[0], e[1]) for r in rows for e in r[:4] if e[0] >= lay.tips]
        named = inner_ends[:3] + inner_ends[-2:]
        assert all(s >= 0 for _, s in named) and lay.cherry not in inner_ends and lay.tmp not in inner_ends
        watch = named + [lay.cherry]
        before = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        got = _rell(b, rows, 17)
        assert all(np.isfinite(x).all() for x in got[:3])
        assert got[3].tobytes() == rell.replicate_weights(own, SEED, 0, 17).tobytes()
        after = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        assert before == after
        assert api.as_np(b.part.pattern_weights, dims[3], np.uint32).tolist() == list(own)
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1
        assert QC.batched(b, rows).tobytes() == got[0].tobytes()  # (the device's pattern weights are the partition's still)
        assert _same(_rell(b, rows, 17), got)
