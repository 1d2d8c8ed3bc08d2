"""GPU: pll_gpu_insertion_loglikelihoods against the reference, live.

The value per candidate is the reference's own: one pll_update_partials with a single operation into a spare tmp node,
then pll_compute_edge_loglikelihood between tmp and the subtree end (insertion_cases.Bed.per_edge; both libraries get
the tmp slot, only the per-edge path uses it). Tolerance: |d| <= RTOL * max(|lnL|, 1), compare.RTOL = 1e-10, for EVERY
candidate; the same candidates through this library's own per-edge path meet the same bound (bit-identity with that
path is not asked for: the sum over sites is partitioned differently).

Placement matrix: a query sequence (one extra tip) is inserted into every edge of UTree(taxa, PCG64(7)) over
W.random_states(taxa + 2, sites, states, seed 8, mutate 15 %) and W.gamma_rates_mean(0.7, R). The trees are large enough
that the inserted node rescales ON ITS OWN, beyond its children's counts - otherwise the test would pass without ever
taking the scaling path. The reference alone, run on a CPU over exactly these inputs, gives (candidates whose inserted
node rescales at some site or rate: scale_buffer[tmp] minus the children's buffers):

    states x rates   taxa x sites   candidates   per site   per rate
    4 x 4            300 x 200      597          597        597
    4 x 2 (generic)  300 x 65       597          385        385
    5 x 3            300 x 33       597          303        379
    20 x 4           200 x 33       397          271        317
    61 x 4           160 x 17       317          160        208

and every case asserts that at least a quarter of its candidates do (a fifth for 5 x 3 per site) - a condition on the
inputs, recomputed from the reference in the test, not a tolerance. (A 64-taxon tree rescales nothing.)"""
import functools

import numpy as np
import pytest

import insertion_cases as IC
from compare import RTOL
from pllamd import api

pytestmark = pytest.mark.gpu

SHAPES = {"4x4": (4, 4, 300, 200), "4x2": (4, 2, 300, 65), "5x3": (5, 3, 300, 33), "20x4": (20, 4, 200, 33), "61x4": (61, 4, 160, 17)}
ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP, "rate_scalers": api.RATE_SCALERS}
SMALL = {"4x4": (4, 4, 20, 130), "20x4": (20, 4, 20, 130)}
_REF = None  # the reference library of the session (functools.cache keys must be hashable)


def _bar(shape, attrs):
    return 0.2 if (shape == "5x3" and not (ATTRS[attrs] & api.RATE_SCALERS)) else 0.25


@functools.lru_cache(maxsize=None)
def _case(states, rate_cats, taxa, sites):
    return IC.make(states, taxa, sites, rate_cats)


def _bed(lib, dims, attrs, **kw):
    states, rate_cats, taxa, sites = dims
    lay, seqs, cmap, exch, freqs = _case(*dims)
    return IC.Bed(lib, lay, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, **kw)


def _query(lay):
    """the first extra tip over the pendant matrix"""
    return (lay.T, IC.NONE, lay.pm_pendant)


def _extra_rows(lay, rows):
    """candidates no edge of a tree gives: both ends tips, and a tip as child2 of an inner child1"""
    inner = next(r for r in rows if r[0] >= lay.tips and r[3] >= lay.tips)
    return [(0, IC.NONE, lay.half(0), 1, IC.NONE, lay.half(1)), (inner[0], inner[1], inner[2], 2, IC.NONE, lay.half(2))]


@functools.lru_cache(maxsize=None)
def _reference(dims, attrs, subtree="tip", extra_rows=False, kw=()):
    """(expected lnL per candidate, own-rescale flag per candidate), computed once per case and shared"""
    with _bed(_REF, dims, attrs, **dict(kw)) as b:
        sub = b.query_cherry(b.lay.T, b.lay.T + 1) if subtree == "cherry" else _query(b.lay)
        rows = b.prepare()
        if extra_rows:
            rows = rows + _extra_rows(b.lay, rows)
        own = []
        exp = b.per_edge(sub, rows, own)
    exp.setflags(write=False)
    return exp, tuple(own)


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    global _REF
    _REF = ref_lib


def _check(got, exp, what):
    assert np.isfinite(got).all(), what
    assert IC.close(got, exp, RTOL), (what, IC.worst(got, exp))


@pytest.mark.parametrize("attrs", list(ATTRS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_placement_into_every_edge(amd_lib, shape, attrs):
    dims = SHAPES[shape]
    exp, own = _reference(dims, ATTRS[attrs])
    assert len(exp) == 2 * dims[2] - 3
    print(f"{shape} {attrs}: {sum(own)} of {len(own)} candidates rescale on their own")
    assert sum(own) >= _bar(shape, attrs) * len(own), "the inputs do not exercise the inserted node's scaling"
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = b.prepare()
        got = b.batched(_query(b.lay), rows)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        seq = b.per_edge(_query(b.lay), rows)
    print(f"{shape} {attrs}: batched worst {IC.worst(got, exp):.2e}, per-edge worst {IC.worst(seq, exp):.2e}, {launches} launch(es)")
    _check(got, exp, "batched call against the reference")
    _check(seq, exp, "per-edge path against the reference")
    assert 1 <= launches <= 3


@pytest.mark.parametrize("attrs", list(ATTRS))
@pytest.mark.parametrize("shape", list(SMALL))
def test_inner_subtree_end(amd_lib, shape, attrs):
    """the subtree end is an inner CLV with a scaler: a cherry of the two extra tips in a spare slot"""
    dims = SMALL[shape]
    exp, _ = _reference(dims, ATTRS[attrs], subtree="cherry")
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        sub = b.query_cherry(b.lay.T, b.lay.T + 1)
        rows = b.prepare()
        _check(b.batched(sub, rows), exp, "cherry as the subtree end")


@pytest.mark.parametrize("attrs", ["plain", "pattern_tip"], ids=["compact_tips", "pattern_tip"])
@pytest.mark.parametrize("shape", list(SMALL))
def test_tip_and_inner_ends(amd_lib, shape, attrs):
    """both ends, one end (as child1 and as child2) or no end of a candidate a tip; launches counted"""
    dims = SMALL[shape]
    exp, _ = _reference(dims, ATTRS[attrs], extra_rows=True)
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = b.prepare()
        rows = rows + _extra_rows(b.lay, rows)
        tips = b.lay.tips
        kinds = [(r[0] < tips) + (r[3] < tips) for r in rows]
        assert set(kinds) == {0, 1, 2}
        got = b.batched(_query(b.lay), rows)
        assert 1 <= amd_lib.pll_gpu_last_launch_count(b.p) <= 3
        _check(got, exp, "mixed kinds")
        for kind in (0, 1, 2):
            some = [i for i, k in enumerate(kinds) if k == kind]
            assert amd_lib.pll_gpu_synchronize(b.p)
            part = b.batched(_query(b.lay), [rows[i] for i in some])
            assert amd_lib.pll_gpu_last_launch_count(b.p) == 1, kind
            assert part.tobytes() == got[some].tobytes(), kind


MODEL = {
    "invariant_sites": dict(prop_invar=0.3),
    "two_frequency_sets": dict(rate_matrices=2, freqs_indices=(0, 1, 0, 1)),
    "pattern_weights": dict(pattern_weights=tuple(1 + (np.arange(130) * 7) % 5)),
}


@pytest.mark.parametrize("what", list(MODEL))
@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape", list(SMALL))
def test_model_features(amd_lib, shape, attrs, what):
    dims = SMALL[shape]
    kw = tuple(sorted(MODEL[what].items()))
    exp, _ = _reference(dims, ATTRS[attrs], kw=kw)
    plain, _ = _reference(dims, ATTRS[attrs])
    assert not IC.close(plain, exp, 1e-6), "the feature does not change the values: nothing is tested"
    with _bed(amd_lib, dims, ATTRS[attrs], **dict(kw)) as b:
        rows = b.prepare()
        _check(b.batched(_query(b.lay), rows), exp, what)


@pytest.mark.parametrize("sites", [1, 63, 64, 65, 257, 2500])
@pytest.mark.parametrize("shape", ["4x4", "5x3"])
def test_geometry_edges(amd_lib, monkeypatch, shape, sites):
    """site counts around the 64-site tile and the workgroup; candidate counts 1, 2, 33, all. 2500 sites span more
    workgroups than there are XCDs: there the fenced hand-off equals the default bit for bit"""
    states, rate_cats = SHAPES[shape][:2]
    dims = (states, rate_cats, 20, sites)
    exp, _ = _reference(dims, 0)
    assert len(exp) == 37
    with _bed(amd_lib, dims, 0) as b:
        rows = b.prepare()
        full = b.batched(_query(b.lay), rows)
        _check(full, exp, "all candidates")
        for count in (1, 2, 33):
            part = b.batched(_query(b.lay), rows[:count])
            assert part.tobytes() == full[:count].tobytes(), count
    if sites == 2500:
        monkeypatch.setenv("PLL_AMD_FENCED_HANDOFF", "1")
        with _bed(amd_lib, dims, 0) as b:
            rows = b.prepare()
            fenced = b.batched(_query(b.lay), rows)
        assert fenced.tobytes() == full.tobytes()


def test_a_list_longer_than_one_launch(amd_lib):
    """more candidates than one launch carries descriptors for (16384; include/pll_amd_device.h states the cutting rule):
    the second launch's values land behind the first's, each with the bits it has in a short list"""
    dims = (4, 4, 20, 65)
    exp, _ = _reference(dims, 0)
    with _bed(amd_lib, dims, 0) as b:
        rows = b.prepare()
        assert len(rows) == 37
        short = b.batched(_query(b.lay), rows)
        _check(short, exp, "the short list")
        times = 16384 // len(rows) + 1
        got = b.batched(_query(b.lay), rows * times)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 2
        assert got.tobytes() == np.tile(short, times).tobytes()


@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
def test_a_tile_too_large_for_lds(amd_lib, attrs):
    """20 states x 16 rates: the inserted node's tile (R x S = 320 > 288 values per lane) does not fit the 144 KB the kernel
    may keep, so it forms the products twice instead - the other path through k_insertion_tiled; more rates than waves"""
    dims = (20, 16, 20, 65)
    exp, _ = _reference(dims, ATTRS[attrs])
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = b.prepare()
        _check(b.batched(_query(b.lay), rows), exp, "two-pass path")


@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_candidates_are_independent(amd_lib, shape, attrs):
    """lnl[i] has the same bits alone, in a shuffled list and twice in a row"""
    dims = SHAPES[shape]
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = b.prepare()
        sub = _query(b.lay)
        full = b.batched(sub, rows)
        assert b.batched(sub, rows).tobytes() == full.tobytes()
        perm = np.random.Generator(np.random.PCG64(3)).permutation(len(rows))
        shuffled = b.batched(sub, [rows[i] for i in perm])
        assert shuffled.tobytes() == full[perm].tobytes()
        for i in (0, 1, len(rows) // 2, len(rows) - 1):
            assert b.batched(sub, [rows[i]]).tobytes() == full[i:i + 1].tobytes(), i
            assert b.batched(sub, [rows[i], rows[i]]).tobytes() == full[[i, i]].tobytes(), i


@pytest.mark.parametrize("shape", list(SMALL))
def test_held_work_is_launched_first(amd_lib, shape):
    """a full traversal directly followed by the batched call that names the two nodes the traversal ends in - what
    pll_update_partials holds back for the next log-likelihood call - and the edge log-likelihood afterwards"""
    dims = SMALL[shape]
    exp, _ = _reference(dims, 0)
    with _bed(_REF, dims, 0) as r:
        r.update(r.lay.full_ops())
        root = r.lay.end(r.lay.root) + r.lay.end(r.lay.root.back) + (r.lay.root.pm,)
        exp_root = r.lnl(root)
    with _bed(amd_lib, dims, 0) as b:
        lay = b.lay
        index = next(i for i, e in enumerate(lay.tree.edges()) if e is lay.root or e.back is lay.root)
        a, c = lay.end(lay.root), lay.end(lay.root.back)
        h = lay.half(lay.root.pm)
        b.update(lay.full_ops())
        got = b.batched(_query(lay), [(a[0], a[1], h, c[0], c[1], h)])
        _check(got, exp[index:index + 1], "candidate at the edge the traversal ends in")
        v = b.lnl(root)
        assert abs(v - exp_root) <= RTOL * max(abs(exp_root), 1.0), (v, exp_root)


def test_nothing_is_written(amd_lib):
    """CLVs and scalers of nodes the list names and of a spare slot it does not name are byte-identical after the call,
    and the operation list of before still replays"""
    dims = SHAPES["4x4"]
    with _bed(amd_lib, dims, 0) as b:
        lay = b.lay
        b.query_cherry(lay.T, lay.T + 1)  # the spare slot the list does not name
        b.update(lay.full_ops())
        up_ops, slot = lay.upward()
        rows = lay.candidates(slot)
        b.update(up_ops)
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1  # (the control: the list does replay when nothing happens)
        named = [(r[0], r[1]) for r in rows if r[0] >= lay.tips][:3] + [(r[3], r[4]) for r in rows[-2:]]
        watch = named + [lay.cherry]
        before = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        got = b.batched(_query(lay), rows)
        assert np.isfinite(got).all()
        after = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        assert before == after
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1
        assert b.batched(_query(lay), rows).tobytes() == got.tobytes()
