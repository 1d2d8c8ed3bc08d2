"""GPU: pll_gpu_placement_loglikelihoods - every query tip x every candidate edge in one call - against the reference,
live, and against pll_gpu_insertion_loglikelihoods of the same library, bit for bit.

Expected values: per query tip, the reference's own per-edge path (insertion_cases.Bed.per_edge: pll_update_partials
with one operation into a spare node, then pll_compute_edge_loglikelihood between it and the query tip across the
pendant matrix). Bound, for EVERY (query, candidate): |d| <= compare.RTOL (1e-10) * max(|lnL|, 1). In addition every
row equals b.batched((lay.T + q, NONE, lay.pm_pendant), rows) of the same library byte for byte: the call is defined as
that value.

Inputs: insertion_cases.make(..., extra=Q) - Q query tips beside the tree's own. The large trees are there so that the
inserted node rescales ON ITS OWN; the reference alone, on a CPU over exactly these inputs (extra = 8), gives
(candidates that rescale / candidates):

    shape    plain / PATTERN_TIP    RATE_SCALERS
    4x4      530 / 597              597 / 597
    4x2      411 / 597              411 / 597
    5x3      210 / 597              391 / 597
    20x4     291 / 397              329 / 397
    61x4     108 / 317              177 / 317

and every case asserts at least a quarter, recomputed from the reference in the test - a condition on the inputs."""
import numpy as np
import pytest

import insertion_cases as IC
import placement_cases as PC
from compare import RTOL
from pllamd import api

pytestmark = pytest.mark.gpu

SHAPES = {"4x4": (4, 4, 300, 200), "4x2": (4, 2, 300, 65), "5x3": (5, 3, 300, 33), "20x4": (20, 4, 200, 33), "61x4": (61, 4, 160, 17)}
ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP, "rate_scalers": api.RATE_SCALERS}
SMALL = {"4x4": (4, 4, 20, 130), "5x3": (5, 3, 20, 130), "20x4": (20, 4, 20, 130)}


def _check(got, exp, what):
    assert got.shape == exp.shape, what
    assert np.isfinite(got).all(), what
    print(f"{what}: worst {IC.worst(got, exp):.2e} over {got.size} pairs")
    assert IC.close(got, exp, RTOL), (what, IC.worst(got, exp))


def _same_as_insertion_call(b, tips, rows, got):
    for r, t in enumerate(tips):
        assert b.batched(PC.query(b.lay, t), rows).tobytes() == got[r].tobytes(), ("row of query tip", t)


@pytest.mark.parametrize("attrs", list(ATTRS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_query_into_every_edge(amd_lib, ref_lib, shape, attrs):
    dims = SHAPES[shape]
    offsets = (0, 3, 7) if shape == "61x4" else tuple(range(8))  # (the reference takes seconds per query at 61 states)
    exp, own = PC.reference(ref_lib, dims, ATTRS[attrs], 8, offsets)
    assert exp.shape == (len(offsets), 2 * dims[2] - 3)
    print(f"{shape} {attrs}: {sum(own)} of {len(own)} candidates rescale on their own")
    assert sum(own) >= 0.25 * len(own), "the inputs do not exercise the inserted node's scaling"
    with PC.bed(amd_lib, dims, ATTRS[attrs], 8) as b:
        rows = b.prepare()
        tips = [b.lay.T + q for q in offsets]
        got = PC.placement(b, tips, rows)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        _check(got, exp, f"{shape} {attrs}")
        _same_as_insertion_call(b, tips, rows, got)
    assert (got[0] != got[1]).all(), "two queries give the same value somewhere: the query axis is not tested"
    assert launches == PC.launches(dims[0], dims[1], dims[3], len(tips), len(rows)) == 1


@pytest.mark.parametrize("shape", list(SMALL))
def test_query_counts_around_the_chunk(amd_lib, ref_lib, shape):
    """one past every power of two up to 64: the leading Q rows of the Q = 65 result, bit for bit"""
    dims = SMALL[shape]
    exp, _ = PC.reference(ref_lib, dims, 0, 65, range(65))
    assert exp.shape == (65, 37)
    with PC.bed(amd_lib, dims, 0, 65) as b:
        rows = b.prepare()
        tips = [b.lay.T + q for q in range(65)]
        full = PC.placement(b, tips, rows)
        _check(full, exp, f"{shape}, 65 queries")
        for q in (1, 2, 3, 5, 9, 17, 33, 65):
            assert PC.placement(b, tips[:q], rows).tobytes() == full[:q].tobytes(), q
        _same_as_insertion_call(b, tips, rows, full)


@pytest.mark.parametrize("sites", [1, 63, 64, 65, 257, 2500])
@pytest.mark.parametrize("shape", ["4x4", "5x3"])
def test_site_counts_around_the_tile(amd_lib, ref_lib, monkeypatch, shape, sites):
    """site counts around the 64-site tile and the workgroup; candidate sublists are bit-equal slices. 2500 sites span
    more workgroups than there are XCDs: there the fenced hand-off equals the default bit for bit"""
    dims = SHAPES[shape][:2] + (20, sites)
    exp, _ = PC.reference(ref_lib, dims, 0, 5, range(5))
    with PC.bed(amd_lib, dims, 0, 5) as b:
        rows = b.prepare()
        tips = [b.lay.T + q for q in range(5)]
        full = PC.placement(b, tips, rows)
        _check(full, exp, f"{shape}, {sites} sites")
        _same_as_insertion_call(b, tips, rows, full)
        for count in (1, 2, 33):
            assert PC.placement(b, tips, rows[:count]).tobytes() == full[:, :count].tobytes(), count
    if sites == 2500:
        monkeypatch.setenv("PLL_AMD_FENCED_HANDOFF", "1")
        with PC.bed(amd_lib, dims, 0, 5) as b:
            rows = b.prepare()
            fenced = PC.placement(b, tips, rows)
        assert fenced.tobytes() == full.tobytes()


def test_a_list_longer_than_one_launch(amd_lib, ref_lib):
    """more candidates than one launch carries descriptors for (16384; include/pll_amd_device.h states the cutting rule),
    two queries so that the call is not the insertion call's: the second launch's values land behind the first's in
    every query's row, each with the bits it has in a short list"""
    dims = (4, 4, 20, 65)
    exp, _ = PC.reference(ref_lib, dims, 0, 2, range(2))
    with PC.bed(amd_lib, dims, 0, 2) as b:
        rows = b.prepare()
        assert len(rows) == 37
        tips = [b.lay.T, b.lay.T + 1]
        short = PC.placement(b, tips, rows)
        _check(short, exp, "the short list")
        times = 16384 // len(rows) + 1
        got = PC.placement(b, tips, rows * times)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        assert launches == PC.launches(dims[0], dims[1], dims[3], len(tips), len(rows) * times) == 2
        for q in range(len(tips)):
            assert got[q].tobytes() == np.tile(short[q], times).tobytes(), q


MODEL = {
    "invariant_sites": dict(prop_invar=0.3),
    "two_frequency_sets": dict(rate_matrices=2, freqs_indices=(0, 1, 0, 1)),
    "pattern_weights": dict(pattern_weights=tuple(1 + (np.arange(130) * 7) % 5)),
}


@pytest.mark.parametrize("what", list(MODEL))
@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_model_features(amd_lib, ref_lib, shape, attrs, what):
    dims = SMALL[shape]
    kw = tuple(sorted(MODEL[what].items()))
    exp, _ = PC.reference(ref_lib, dims, ATTRS[attrs], 3, range(3), kw=kw)
    plain, _ = PC.reference(ref_lib, dims, ATTRS[attrs], 3, range(3))
    assert not IC.close(plain, exp, 1e-6), "the feature does not change the values: nothing is tested"
    with PC.bed(amd_lib, dims, ATTRS[attrs], 3, **dict(kw)) as b:
        rows = b.prepare()
        tips = [b.lay.T + q for q in range(3)]
        got = PC.placement(b, tips, rows)
        _check(got, exp, what)
        _same_as_insertion_call(b, tips, rows, got)


@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
def test_a_tile_too_large_for_lds(amd_lib, ref_lib, attrs):
    """20 states x 16 rates: R x S = 320 values per lane do not fit beside the per-query parts, so pass 2 forms the
    products again, once per chunk - the other path through k_placement_tiled; more rates than waves"""
    dims = (20, 16, 20, 65)
    exp, _ = PC.reference(ref_lib, dims, ATTRS[attrs], 3, range(3))
    with PC.bed(amd_lib, dims, ATTRS[attrs], 3) as b:
        rows = b.prepare()
        tips = [b.lay.T + q for q in range(3)]
        got = PC.placement(b, tips, rows)
        _check(got, exp, "two-pass path")
        _same_as_insertion_call(b, tips, rows, got)


@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_pairs_are_independent(amd_lib, shape, attrs):
    """lnl[q][i] has the same bits in lists shuffled in both directions, with a query named twice, alone, and twice
    in a row"""
    dims = SHAPES[shape]
    with PC.bed(amd_lib, dims, ATTRS[attrs], 8) as b:
        rows = b.prepare()
        tips = np.array([b.lay.T + q for q in range(8)])
        full = PC.placement(b, tips, rows)
        assert np.isfinite(full).all()
        assert PC.placement(b, tips, rows).tobytes() == full.tobytes()
        rng = np.random.Generator(np.random.PCG64(3))
        qperm, cperm = rng.permutation(len(tips)), rng.permutation(len(rows))
        shuffled = PC.placement(b, tips[qperm], [rows[i] for i in cperm])
        assert shuffled.tobytes() == full[np.ix_(qperm, cperm)].tobytes()
        twice = PC.placement(b, [tips[2], tips[5], tips[2]], rows)
        assert twice.tobytes() == full[[2, 5, 2]].tobytes()
        for q, i in ((0, 0), (3, 1), (7, len(rows) // 2), (4, len(rows) - 1)):
            assert PC.placement(b, [tips[q]], [rows[i]]).tobytes() == full[q:q + 1, i:i + 1].tobytes(), (q, i)


@pytest.mark.parametrize("attrs", ["plain", "pattern_tip"], ids=["compact_tips", "pattern_tip"])
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_end_kinds(amd_lib, ref_lib, shape, attrs):
    """both ends, one end (as child1 and as child2) or no end of a candidate a tip; an end that is itself a query"""
    dims = SMALL[shape]
    exp, _ = PC.reference(ref_lib, dims, ATTRS[attrs], 3, range(3), more_rows=True)
    with PC.bed(amd_lib, dims, ATTRS[attrs], 3) as b:
        rows = b.prepare()
        rows = rows + PC.extra_rows(b.lay, rows)
        tips = [b.lay.T + q for q in range(3)]
        kinds = [(r[0] < b.lay.tips) + (r[3] < b.lay.tips) for r in rows]
        assert set(kinds) == {0, 1, 2} and rows[-1][0] in tips
        got = PC.placement(b, tips, rows)
        _check(got, exp, "mixed kinds")
        _same_as_insertion_call(b, tips, rows, got)


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_held_work_is_launched_first(amd_lib, ref_lib, shape):
    """a full traversal directly followed by the call that names the two nodes the traversal ends in - what
    pll_update_partials holds back for the next log-likelihood call - and the edge log-likelihood afterwards"""
    dims = SMALL[shape]
    exp, _ = PC.reference(ref_lib, dims, 0, 3, range(3))
    with PC.bed(ref_lib, dims, 0, 3) as r:
        r.update(r.lay.full_ops())
        root = r.lay.end(r.lay.root) + r.lay.end(r.lay.root.back) + (r.lay.root.pm,)
        exp_root = r.lnl(root)
    with PC.bed(amd_lib, dims, 0, 3) as b:
        lay = b.lay
        index = next(i for i, e in enumerate(lay.tree.edges()) if e is lay.root or e.back is lay.root)
        a, c = lay.end(lay.root), lay.end(lay.root.back)
        h = lay.half(lay.root.pm)
        b.update(lay.full_ops())
        got = PC.placement(b, [lay.T, lay.T + 1, lay.T + 2], [(a[0], a[1], h, c[0], c[1], h)])
        _check(got, exp[:, index:index + 1], "candidate at the edge the traversal ends in")
        v = b.lnl(root)
        assert abs(v - exp_root) <= RTOL * max(abs(exp_root), 1.0), (v, exp_root)


def test_nothing_is_written(amd_lib):
    """CLVs and scalers of nodes the list names and of a spare slot it does not name are byte-identical after the call,
    and the operation list of before still replays"""
    dims = SHAPES["4x4"]
    with PC.bed(amd_lib, dims, 0, 8) as b:
        lay = b.lay
        for k in (3, 2, 1, 0):  # the spare slot the list does not name; every query tip's codes reach the device here, so
            b.query_cherry(lay.T + 2 * k, lay.T + 2 * k + 1)  # that the control below finds nothing left to upload
        b.update(lay.full_ops())
        up_ops, slot = lay.upward()
        rows = lay.candidates(slot)
        b.update(up_ops)
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1  # (the control: the list does replay when nothing happens)
        named = [(r[0], r[1]) for r in rows if r[0] >= lay.tips][:3] + [(r[3], r[4]) for r in rows[-2:]]
        watch = named + [lay.cherry]
        before = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        tips = [lay.T + q for q in range(8)]
        got = PC.placement(b, tips, rows)
        assert np.isfinite(got).all()
        after = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        assert before == after
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1
        assert PC.placement(b, tips, rows).tobytes() == got.tobytes()


def test_a_query_tip_not_held_as_codes(amd_lib, ref_lib):
    """a query tip overwritten with a dense CLV (pll_set_tip_clv) is refused with lnl untouched; set again with
    pll_set_tip_states it is served"""
    dims = SMALL["4x4"]
    exp, _ = PC.reference(ref_lib, dims, 0, 3, range(3))
    with PC.bed(amd_lib, dims, 0, 3) as b:
        rows = b.prepare()
        tips = np.array([b.lay.T + q for q in range(3)], dtype=np.uint32)
        seq = PC.sequences(dims, 3)[b.lay.T + 1]
        masks = np.array([int(b.cmap[ch]) for ch in bytes(seq)], dtype=np.uint64)
        # (an indicator vector of zeros and ones would be taken as codes again: a sequencing-error model instead)
        dense = np.ascontiguousarray(((masks[:, None] >> np.arange(4, dtype=np.uint64)) & 1).astype(np.float64) * 0.97 + 0.01)
        assert amd_lib.pll_set_tip_clv(b.p, int(tips[1]), api.dptr(dense), 0)
        lnl = np.full((3, len(rows)), -12345.5)
        assert amd_lib.pll_gpu_placement_loglikelihoods(b.p, api.uptr(tips), 3, b.lay.pm_pendant, api.make_insertions(rows), len(rows),
                                                        api.uptr(b.fi), api.dptr(lnl)) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNSUPPORTED, (amd_lib.errno(), amd_lib.errmsg())
        assert "pll_set_tip_states" in amd_lib.errmsg()
        assert (lnl == -12345.5).all()
        assert amd_lib.pll_set_tip_states(b.p, int(tips[1]), b.cmap, seq)
        _check(PC.placement(b, tips, rows), exp, "after pll_set_tip_states")
