"""GPU: pll_gpu_quartet_loglikelihoods against the reference, live.

The three values per quartet are the reference's own: per arrangement one pll_update_partials with two operations into
two spare nodes, then pll_compute_edge_loglikelihood between them (quartet_cases.per_edge; both libraries get the spare
slots, only the per-edge path uses them). Tolerance: |d| <= RTOL * max(|lnL|, 1), compare.RTOL = 1e-10, for EVERY value;
the same values through this library's own per-edge path meet the same bound (bit-identity with that path is not asked
for).

Every inner edge of UTree(taxa, PCG64(7)) over W.random_states(taxa + 2, sites, states, seed 8, mutate 15 %) and
W.gamma_rates_mean(0.7, R) - the insertion tests' inputs. The trees are large enough that the two nodes rescale ON THEIR
OWN, beyond their children's counts - otherwise the test would pass without ever taking a node's scaling path. The
reference alone, run on a CPU over exactly these inputs, gives (values in which a node rescales at some site or rate:
scale_buffer[tmp] minus the children's buffers):

    shape    attribute       values   some node   first node   second node
    4 x 4    plain           891      730         419          311
    4 x 4    pattern_tip     891      730         419          311
    4 x 4    rate_scalers    891      886         498          392
    4 x 2    plain           891      473         274          199
    4 x 2    rate_scalers    891      528         304          224
    5 x 3    plain           891      426         252          174
    5 x 3    rate_scalers    891      637         366          271
    20 x 4   plain           591      329         185          144
    20 x 4   rate_scalers    591      501         273          228
    61 x 4   plain           471      192         111          81
    61 x 4   rate_scalers    471      319         182          137

and every case asserts that some node does in at least a quarter of its values and each of the two nodes in at least a
tenth - a condition on the inputs, recomputed from the reference in the test, not a tolerance. (A 20-taxon tree rescales
nothing.) 61 x 4 with pattern_tip is left out of this matrix (the reference needs 17 s for it); test_ends_of_every_kind
covers that combination on a small tree."""
import functools

import numpy as np
import pytest

import insertion_cases as IC
import quartet_cases as QC
from compare import RTOL
from pllamd import api
from utree import UTree

pytestmark = pytest.mark.gpu

SHAPES = {"4x4": (4, 4, 300, 200), "4x2": (4, 2, 300, 65), "5x3": (5, 3, 300, 33), "20x4": (20, 4, 200, 33), "61x4": (61, 4, 160, 17)}
ATTRS = {"plain": 0, "pattern_tip": api.PATTERN_TIP, "rate_scalers": api.RATE_SCALERS}
EVERY_EDGE = [(s, a) for s in SHAPES for a in ATTRS if not (s == "61x4" and a == "pattern_tip")]
SMALL = {"4x4": (4, 4, 20, 130), "20x4": (20, 4, 20, 130)}
_REF = None  # the reference library of the session (functools.cache keys must be hashable)


@functools.lru_cache(maxsize=None)
def _case(states, rate_cats, taxa, sites):
    return IC.make(states, taxa, sites, rate_cats)


def _bed(lib, dims, attrs, lay=None, **kw):
    states, rate_cats, taxa, sites = dims
    own_lay, seqs, cmap, exch, freqs = _case(*dims)
    return IC.Bed(lib, lay or own_lay, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, **kw)


def _extra_rows(lay, rows):
    """quartets no tree gives: all four ends tips, and a pair that is (inner, tip) in that order"""
    pm = [lay.tree.tip_recs[t].pm for t in range(5)]
    inner = next(r for r in rows if r[0][0] >= lay.tips)
    return [((0, IC.NONE, pm[0]), (1, IC.NONE, pm[1]), (2, IC.NONE, pm[2]), (3, IC.NONE, pm[3]), rows[0][4]),
            (inner[0], (4, IC.NONE, pm[4]), inner[2], inner[3], inner[4])]


@functools.lru_cache(maxsize=None)
def _reference(dims, attrs, extra_rows=False, kw=()):
    """(expected [Q, 3], per value (first node rescales, second node rescales)), computed once per case and shared"""
    with _bed(_REF, dims, attrs, **dict(kw)) as b:
        rows = QC.prepare(b)
        if extra_rows:
            rows = rows + _extra_rows(b.lay, rows)
        own = []
        exp = QC.per_edge(b, rows, own)
    exp.setflags(write=False)
    return exp, tuple(own)


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    global _REF
    _REF = ref_lib


def _check(got, exp, what):
    assert np.isfinite(got).all(), what
    assert IC.close(got, exp, RTOL), (what, IC.worst(got, exp))


@pytest.mark.parametrize("shape,attrs", EVERY_EDGE)
def test_every_inner_edge(amd_lib, shape, attrs):
    dims = SHAPES[shape]
    exp, own = _reference(dims, ATTRS[attrs])
    assert exp.shape == (dims[2] - 3, 3)
    some, first, second = sum(a or b for a, b in own), sum(a for a, _ in own), sum(b for _, b in own)
    print(f"{shape} {attrs}: of {len(own)} values a node rescales on its own in {some}, the first in {first}, the second in {second}")
    assert some >= 0.25 * len(own), "the inputs do not exercise the nodes' scaling"
    assert first >= 0.1 * len(own), "the inputs do not exercise the first node's scaling"
    assert second >= 0.1 * len(own), "the inputs do not exercise the second node's scaling"
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = QC.prepare(b)
        got = QC.batched(b, rows)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        seq = QC.per_edge(b, rows)
    print(f"{shape} {attrs}: batched worst {IC.worst(got, exp):.2e}, per-edge worst {IC.worst(seq, exp):.2e}, {launches} launch(es)")
    _check(got, exp, "batched call against the reference")
    _check(seq, exp, "per-edge path against the reference")
    assert 1 <= launches <= 3


KINDS = [(s, a) for s in SMALL for a in ("plain", "pattern_tip")] + [("61x4", "pattern_tip")]


@pytest.mark.parametrize("shape,attrs", KINDS, ids=[f"{s}-{'compact_tips' if a == 'plain' else a}" for s, a in KINDS])
def test_ends_of_every_kind(amd_lib, shape, attrs):
    """pairs of two inner ends, of a tip and an inner end (in both orders) and of two tips, compact or pattern tips"""
    dims = SMALL[shape] if shape in SMALL else (61, 4, 20, 17)
    exp, _ = _reference(dims, ATTRS[attrs], extra_rows=True)
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = QC.prepare(b)
        rows = rows + _extra_rows(b.lay, rows)
        assert set(QC.pair_tips(b.lay, rows)) == {0, 1, 2}
        assert all(r[0][0] < b.lay.tips and r[1][0] < b.lay.tips and r[2][0] < b.lay.tips and r[3][0] < b.lay.tips for r in rows[-2:-1])
        assert rows[-1][0][0] >= b.lay.tips and rows[-1][1][0] < b.lay.tips
        got = QC.batched(b, rows)
        assert 1 <= amd_lib.pll_gpu_last_launch_count(b.p) <= 3
        _check(got, exp, "mixed kinds")


@pytest.mark.parametrize("shape", list(SMALL))
def test_nni_correspondence(amd_lib, shape):
    """arrangement 0 is the tree itself, arrangement 2 the tree after UTree.nni(p, 0), arrangement 1 after nni(p, 1):
    the reference's full-traversal log-likelihood of a fresh copy of the moved tree"""
    dims = SMALL[shape]
    picks = (0, 5, 11, 16)

    def moved_lnl(index, kind):
        tree = UTree(dims[2], np.random.Generator(np.random.PCG64(7)))
        if kind is not None:
            tree.nni(tree.inner_edges()[index], kind)
            tree.check()
        lay = IC.Layout(tree)
        with _bed(_REF, dims, 0, lay=lay) as r:
            r.update(lay.full_ops())
            return r.lnl(lay.end(lay.root) + lay.end(lay.root.back) + (lay.root.pm,))

    unmoved = moved_lnl(0, None)
    with _bed(amd_lib, dims, 0) as b:
        rows = QC.prepare(b)
        assert len(rows) == 17
        got = QC.batched(b, [rows[i] for i in picks])
    for row, i in zip(got, picks):
        exp = np.array([unmoved, moved_lnl(i, 1), moved_lnl(i, 0)])
        print(f"{shape} inner edge {i}: {row} against {exp}")
        _check(row, exp, f"inner edge {i}")
        assert abs(exp[1] - exp[0]) > 1e-6 and abs(exp[2] - exp[0]) > 1e-6 and abs(exp[1] - exp[2]) > 1e-6


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
        _check(QC.batched(b, QC.prepare(b)), exp, what)


@pytest.mark.parametrize("sites", [1, 63, 64, 65, 257, 2500])
@pytest.mark.parametrize("shape", ["4x4", "5x3"])
def test_geometry_edges(amd_lib, monkeypatch, shape, sites):
    """site counts around the 64-site tile and the workgroup; the first 1 and 2 quartets of the list alone. 2500 sites span
    more workgroups than there are XCDs: there the fenced hand-off equals the default bit for bit"""
    states, rate_cats = SHAPES[shape][:2]
    dims = (states, rate_cats, 20, sites)
    exp, _ = _reference(dims, 0)
    assert exp.shape == (17, 3)
    with _bed(amd_lib, dims, 0) as b:
        rows = QC.prepare(b)
        full = QC.batched(b, rows)
        _check(full, exp, "all quartets")
        for count in (1, 2):
            part = QC.batched(b, rows[:count])
            assert part.tobytes() == full[:count].tobytes(), count
    if sites == 2500:
        monkeypatch.setenv("PLL_AMD_FENCED_HANDOFF", "1")
        with _bed(amd_lib, dims, 0) as b:
            fenced = QC.batched(b, QC.prepare(b))
        assert fenced.tobytes() == full.tobytes()


@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
def test_two_tiles_too_large_for_lds(amd_lib, attrs):
    """20 states x 16 rates: two tiles of R x S = 320 values per lane do not fit the LDS the kernel may keep, so it forms
    the products twice instead - the other path through k_quartet_tiled; more rates than waves"""
    dims = (20, 16, 20, 65)
    exp, _ = _reference(dims, ATTRS[attrs])
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        _check(QC.batched(b, QC.prepare(b)), exp, "recompute path")


@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_quartets_are_independent(amd_lib, shape, attrs):
    """a quartet's three values have the same bits alone, duplicated, in a shuffled list and twice in a row"""
    dims = SHAPES[shape]
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = QC.prepare(b)
        full = QC.batched(b, rows)
        assert QC.batched(b, rows).tobytes() == full.tobytes()
        perm = np.random.Generator(np.random.PCG64(3)).permutation(len(rows))
        shuffled = QC.batched(b, [rows[i] for i in perm])
        assert shuffled.tobytes() == full[perm].tobytes()
        for i in (0, 1, len(rows) // 2, len(rows) - 1):
            assert QC.batched(b, [rows[i]]).tobytes() == full[i:i + 1].tobytes(), i
            assert QC.batched(b, [rows[i], rows[i]]).tobytes() == full[[i, i]].tobytes(), i


def test_a_list_longer_than_one_launch(amd_lib):
    """more quartets than one launch carries descriptors for (8192; include/pll_amd_device.h states the cutting rule): the
    second launch's values land behind the first's, each with the bits it has in a short list"""
    dims = (4, 4, 20, 65)
    exp, _ = _reference(dims, 0)
    with _bed(amd_lib, dims, 0) as b:
        rows = QC.prepare(b)
        short = QC.batched(b, rows)
        _check(short, exp, "the short list")
        times = 8192 // len(rows) + 1
        got = QC.batched(b, rows * times)
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 2
        assert got.tobytes() == np.tile(short, (times, 1)).tobytes()


def _root_row(lay):
    """a quartet that names the two nodes a full traversal ends in, paired with two tips"""
    t0, t1 = lay.tree.tip_recs[0], lay.tree.tip_recs[1]
    root = lay.root
    return (lay.end(root) + (root.pm,), (0, IC.NONE, t0.pm), lay.end(root.back) + (root.back.next.pm,), (1, IC.NONE, t1.pm), root.pm)


@pytest.mark.parametrize("shape", list(SMALL))
def test_held_work_is_launched_first(amd_lib, shape):
    """a full traversal directly followed by the batched call that names the two nodes the traversal ends in - what
    pll_update_partials holds back for the next log-likelihood call - and the edge log-likelihood afterwards"""
    dims = SMALL[shape]
    with _bed(_REF, dims, 0) as r:
        r.update(r.lay.full_ops())
        row = _root_row(r.lay)
        exp = QC.per_edge(r, [row])
        root = r.lay.end(r.lay.root) + r.lay.end(r.lay.root.back) + (r.lay.root.pm,)
        exp_root = r.lnl(root)
    with _bed(amd_lib, dims, 0) as b:
        b.update(b.lay.full_ops())
        got = QC.batched(b, [row])
        _check(got, exp, "the quartet over the two nodes the traversal ends in")
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
        rows = QC.quartet_rows(lay, slot)
        b.update(up_ops)
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1  # (the control: the list does replay when nothing happens)
        inner_ends = [(e[0], e[1]) for r in rows for e in r[:4] if e[0] >= lay.tips]
        named = inner_ends[:3] + inner_ends[-2:]
        assert all(s >= 0 for _, s in named) and lay.cherry not in inner_ends and lay.tmp not in inner_ends
        watch = named + [lay.cherry]
        before = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        got = QC.batched(b, rows)
        assert np.isfinite(got).all()
        after = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        assert before == after
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1
        assert QC.batched(b, rows).tobytes() == got.tobytes()
