"""GPU: pll_gpu_quartet_resampled_loglikelihoods against the reference, live.

Per value (quartet i, arrangement a) the reference's per-edge path - pll_update_partials with two operations into two
spare nodes, pll_compute_edge_loglikelihood with a persite_lnl buffer - on a partition whose pattern weights are all 1
gives u, the per-site log-likelihoods; the expected resampled value of replicate b is math.fsum(w_b[n] * u[n])
(resample_cases). Weights: Generator(PCG64(11)).multinomial(sites, uniform, size=replicates); from 64 sites on every row
is asserted to drop a site and to repeat one. Tolerance against the reference, for EVERY lnl, resampled value and per-site
entry: |d| <= RTOL * max(|v|, 1), compare.RTOL = 1e-10. The contraction alone is held to its own derived bound
(test_the_contraction_alone), lnl to bit-identity with pll_gpu_quartet_loglikelihoods.

Shapes, trees and the scaling conditions are test_gpu_quartets' (its docstring has the table): the trees are large enough
that the two nodes rescale on their own, and every case asserts from the reference that they do."""
import functools

import numpy as np
import pytest

import insertion_cases as IC
import quartet_cases as QC
import resample_cases as RC
import test_gpu_quartets as TQ
from compare import RTOL
from pllamd import api

pytestmark = pytest.mark.gpu

SHAPES, ATTRS, SMALL = TQ.SHAPES, TQ.ATTRS, TQ.SMALL
EVERY_EDGE = [(s, a) for s in SHAPES for a in ("plain", "rate_scalers")] + [("4x4", "pattern_tip")]
OWN_WEIGHTS = tuple(int(x) for x in 1 + (np.arange(130) * 7) % 5)
_REF = None  # the reference library of the session (functools.cache keys must be hashable)


@pytest.fixture(autouse=True)
def _reference_library(ref_lib):
    global _REF
    _REF = ref_lib


def _bed(lib, dims, attrs, **kw):
    states, rate_cats, taxa, sites = dims
    lay, seqs, cmap, exch, freqs = TQ._case(*dims)
    return IC.Bed(lib, lay, states, sites, rate_cats, attrs, seqs, cmap, exch, freqs, **kw)


def _rows(bed, extra_rows=False):
    rows = QC.prepare(bed)
    return rows + TQ._extra_rows(bed.lay, rows) if extra_rows else rows


@functools.lru_cache(maxsize=None)
def _reference(dims, attrs, extra_rows=False, kw=()):
    """(lnl [Q, 3], persite [Q, 3, sites], per value (first node rescales, second node rescales)) of the reference,
    computed once per case and shared; with kw = () the partition's pattern weights are 1 and persite is u"""
    with _bed(_REF, dims, attrs, **dict(kw)) as b:
        own = []
        lnl, per = RC.persite_per_edge(b, _rows(b, extra_rows), own)
    lnl.setflags(write=False)
    per.setflags(write=False)
    return lnl, per, tuple(own)


def _check(got, exp, what):
    assert np.isfinite(got).all(), what
    assert IC.close(got, exp, RTOL), (what, IC.worst(got, exp))


def _check_all(got, lnl_exp, u_exp, w, what, persite_exp=None):
    """all three outputs of one call against the reference: u_exp from a partition of weights 1"""
    lnl, res, per = got
    _check(lnl, lnl_exp, what + ": lnl")
    _check(per, u_exp if persite_exp is None else persite_exp, what + ": persite")
    _check(res, RC.resampled_from(u_exp, w), what + ": resampled")


@pytest.mark.parametrize("shape,attrs", EVERY_EDGE)
def test_every_inner_edge(amd_lib, shape, attrs):
    dims = SHAPES[shape]
    lnl_exp, u_exp, own = _reference(dims, ATTRS[attrs])
    assert lnl_exp.shape == (dims[2] - 3, 3)
    some, first, second = sum(a or b for a, b in own), sum(a for a, _ in own), sum(b for _, b in own)
    assert some >= 0.25 * len(own), "the inputs do not exercise the nodes' scaling"
    assert first >= 0.1 * len(own), "the inputs do not exercise the first node's scaling"
    assert second >= 0.1 * len(own), "the inputs do not exercise the second node's scaling"
    w = RC.weights(dims[3], 17)  # one past an MFMA tile of 16
    with _bed(amd_lib, dims, ATTRS[attrs]) as b:
        rows = _rows(b)
        got = RC.call(b, rows, w)
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        plain = QC.batched(b, rows)
    exp = RC.resampled_from(u_exp, w)
    print(f"{shape} {attrs}: lnl worst {IC.worst(got[0], lnl_exp):.2e}, resampled worst {IC.worst(got[1], exp):.2e}, "
          f"persite worst {IC.worst(got[2], u_exp):.2e}, {launches} launch(es)")
    _check_all(got, lnl_exp, u_exp, w, f"{shape} {attrs}")
    assert got[0].tobytes() == plain.tobytes(), "lnl is not what pll_gpu_quartet_loglikelihoods returns"
    assert 3 <= launches <= 5  # the quartet launch, the contraction, its reduction - and what the upward operations held back


@pytest.mark.parametrize("dims", [SHAPES["4x4"], SHAPES["20x4"], (4, 4, 20, 2500), (5, 3, 20, 257)], ids=["4x4", "20x4", "4x4-2500", "5x3-257"])
def test_the_contraction_alone(amd_lib, dims):
    """stage 2 against its own input: with partition weights 1 persite is u, and the sum of w u in any order of rounded or
    fused products lies within (sites + 3) 2^-53 sum w |u| of the exact one. 2500 sites: more than one split"""
    w = RC.weights(dims[3], 17)
    with _bed(amd_lib, dims, 0) as b:
        _, res, per = RC.call(b, _rows(b), w)
    exact = RC.resampled_from(per, w)
    bound = RC.stage2_bound(per, w)
    assert np.isfinite(res).all() and (bound > 0).all()
    print(f"{dims}: worst |d| / bound {np.max(np.abs(res - exact) / bound):.3f}")
    assert (np.abs(res - exact) <= bound).all()


@pytest.mark.parametrize("own_weights", [False, True], ids=["weights_1", "own_weights"])
@pytest.mark.parametrize("shape", list(SMALL))
def test_the_definition_through_pll_set_pattern_weights(amd_lib, shape, own_weights):
    """resampled[i, b, a] is what the reference's per-edge path returns after pll_set_pattern_weights(w_b); the partition's
    own weights do not enter it, while persite and lnl carry them"""
    dims = SMALL[shape]
    kw = dict(pattern_weights=OWN_WEIGHTS) if own_weights else {}
    w = RC.weights(dims[3], 3)
    with _bed(_REF, dims, 0, **kw) as r:
        rows = _rows(r)
        lnl_exp, per_exp = RC.persite_per_edge(r, rows)
        exp = np.empty((len(rows), 3, 3))
        for k in range(3):
            _REF.pll_set_pattern_weights(r.p, api.uptr(w[k]))
            exp[:, k, :] = QC.per_edge(r, rows)
    for k in range(3):
        assert np.abs(exp[:, k, :] - lnl_exp).min() > 1e-6 and np.abs(exp[:, k, :] - exp[:, (k + 1) % 3, :]).min() > 1e-6, "nothing is tested"
    with _bed(amd_lib, dims, 0, **kw) as b:
        lnl, res, per = RC.call(b, _rows(b), w)
        assert api.as_np(b.part.pattern_weights, dims[3], np.uint32).tolist() == (list(OWN_WEIGHTS) if own_weights else [1] * dims[3])
    _check(res, exp, "resampled")
    _check(lnl, lnl_exp, "lnl")
    _check(per, per_exp, "persite")
    if own_weights:
        plain_lnl, u, _ = _reference(dims, 0)
        assert not IC.close(lnl, plain_lnl, 1e-6) and not IC.close(per, u, 1e-6), "the partition's weights do not show"
        _check(res, RC.resampled_from(u, w), "resampled against the unweighted per-site values")


GEOMETRY = [(s, 17) for s in (1, 63, 64, 65, 257, 2500)] + [(65, r) for r in (1, 15, 16, 100)]


@pytest.mark.parametrize("sites,replicates", GEOMETRY)
@pytest.mark.parametrize("shape", ["4x4", "5x3"])
def test_geometry_edges(amd_lib, shape, sites, replicates):
    """site counts around the 64-site tile, the 16-site block of the contraction and its split (2500); replicate counts
    around the 16-column tile; ends of every kind: four tips, (inner, tip)"""
    states, rate_cats = SHAPES[shape][:2]
    dims = (states, rate_cats, 20, sites)
    lnl_exp, u_exp, _ = _reference(dims, 0, extra_rows=True)
    assert lnl_exp.shape == (19, 3)
    w = RC.weights(sites, replicates)
    with _bed(amd_lib, dims, 0) as b:
        rows = _rows(b, extra_rows=True)
        assert set(QC.pair_tips(b.lay, rows)) == {0, 1, 2}
        got = RC.call(b, rows, w)
        assert got[1].shape == (19, replicates, 3)
        _check_all(got, lnl_exp, u_exp, w, f"{shape} {sites} x {replicates}")
        assert got[0].tobytes() == QC.batched(b, rows).tobytes()


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_values_are_independent(amd_lib, shape):
    """a quartet alone, doubled and in a shuffled list, a replicate row alone, the call twice: the same bits; and
    replicates == 0 gives the same per-site bits"""
    dims = SHAPES[shape]
    w = RC.weights(dims[3], 17)
    with _bed(amd_lib, dims, 0) as b:
        rows = _rows(b)[:40]
        lnl, res, per = RC.call(b, rows, w)
        again = RC.call(b, rows, w)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (lnl, res, per)))
        perm = np.random.Generator(np.random.PCG64(3)).permutation(len(rows))
        shuffled = RC.call(b, [rows[i] for i in perm], w)
        assert all(x.tobytes() == y[perm].tobytes() for x, y in zip(shuffled, (lnl, res, per)))
        for i in (0, len(rows) // 2, len(rows) - 1):
            alone = RC.call(b, [rows[i]], w)
            assert all(x.tobytes() == y[i:i + 1].tobytes() for x, y in zip(alone, (lnl, res, per))), i
            twice = RC.call(b, [rows[i], rows[i]], w)
            assert all(x.tobytes() == y[[i, i]].tobytes() for x, y in zip(twice, (lnl, res, per))), i
        for k in (0, 9, 16):
            _, one, _ = RC.call(b, rows, w[k:k + 1], want_persite=False)
            assert one.tobytes() == np.ascontiguousarray(res[:, k:k + 1, :]).tobytes(), k
        lnl0, res0, per0 = RC.call(b, rows, None)
        assert res0 is None and per0.tobytes() == per.tobytes() and lnl0.tobytes() == lnl.tobytes()
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 1


@pytest.mark.parametrize("shape", ["4x4", "20x4"])
def test_chunks_change_no_bit(amd_lib, monkeypatch, shape):
    """PLL_AMD_RESAMPLE_SCRATCH lowered until 17 quartets x 65 sites x 40 replicates need several quartet chunks AND two
    replicate chunks (include/pll_amd_device.h has the rule: 20000 bytes -> 2 quartets, 29 replicates per chunk): every
    output has the bits of the uncut call, from more launches"""
    states, rate_cats = SHAPES[shape][:2]
    dims = (states, rate_cats, 20, 65)
    w = RC.weights(65, 40)
    with _bed(amd_lib, dims, 0) as b:
        rows = _rows(b)
        whole = RC.call(b, rows, w)  # (launches what the upward operations held back as well)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(RC.call(b, rows, w), whole))
        assert amd_lib.pll_gpu_last_launch_count(b.p) == 3
    monkeypatch.setenv("PLL_AMD_RESAMPLE_SCRATCH", "20000")
    with _bed(amd_lib, dims, 0) as b:
        rows = _rows(b)
        cut = RC.call(b, rows, w)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(cut, whole))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(RC.call(b, rows, w), whole))
        launches = amd_lib.pll_gpu_last_launch_count(b.p)
        assert launches == 2 * 9 * 3, launches  # 2 replicate chunks x 9 quartet chunks x (quartets, contraction, reduction)
        sums_only = RC.call(b, rows, w, want_persite=False)
        assert sums_only[1].tobytes() == whole[1].tobytes() and sums_only[2] is None


MODEL = {"invariant_sites": dict(prop_invar=0.3), "two_frequency_sets": dict(rate_matrices=2, freqs_indices=(0, 1, 0, 1))}


@pytest.mark.parametrize("what", list(MODEL))
@pytest.mark.parametrize("attrs", ["plain", "rate_scalers"])
@pytest.mark.parametrize("shape", list(SMALL))
def test_model_features(amd_lib, shape, attrs, what):
    dims = SMALL[shape]
    kw = tuple(sorted(MODEL[what].items()))
    lnl_exp, u_exp, _ = _reference(dims, ATTRS[attrs], kw=kw)
    plain, _, _ = _reference(dims, ATTRS[attrs])
    assert not IC.close(plain, lnl_exp, 1e-6), "the feature does not change the values: nothing is tested"
    w = RC.weights(dims[3], 5)
    with _bed(amd_lib, dims, ATTRS[attrs], **dict(kw)) as b:
        _check_all(RC.call(b, _rows(b), w), lnl_exp, u_exp, w, what)


def test_nothing_is_written(amd_lib):
    """CLVs and scalers of nodes the list names and of a spare slot it does not name are byte-identical after the call, the
    partition's pattern weights are what they were, and the operation list of before still replays"""
    dims = SHAPES["4x4"]
    own = tuple(int(x) for x in 1 + (np.arange(dims[3]) * 7) % 5)
    w = RC.weights(dims[3], 17)
    with _bed(amd_lib, dims, 0, pattern_weights=own) as b:
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
        got = RC.call(b, rows, w)
        assert all(np.isfinite(x).all() for x in got)
        after = [(b.clv_bytes(c), b.scaler(s).tobytes()) for c, s in watch]
        assert before == after
        assert api.as_np(b.part.pattern_weights, dims[3], np.uint32).tolist() == list(own)
        b.update(up_ops)
        assert amd_lib.pll_gpu_last_update_replayed(b.p) == 1
        assert QC.batched(b, rows).tobytes() == got[0].tobytes()  # (the device's pattern weights are the partition's still)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(RC.call(b, rows, w), got))


@pytest.mark.parametrize("shape", list(SMALL))
def test_held_work_is_launched_first(amd_lib, shape):
    """a full traversal directly followed by the call over the two nodes the traversal ends in - what pll_update_partials
    holds back for the next log-likelihood call - and the edge log-likelihood afterwards"""
    dims = SMALL[shape]
    w = RC.weights(dims[3], 5)
    with _bed(_REF, dims, 0) as r:
        r.update(r.lay.full_ops())
        row = TQ._root_row(r.lay)
        lnl_exp, u_exp = RC.persite_per_edge(r, [row])
        root = r.lay.end(r.lay.root) + r.lay.end(r.lay.root.back) + (r.lay.root.pm,)
        exp_root = r.lnl(root)
    with _bed(amd_lib, dims, 0) as b:
        b.update(b.lay.full_ops())
        _check_all(RC.call(b, [row], w), lnl_exp, u_exp, w, "the quartet over the two nodes the traversal ends in")
        v = b.lnl(root)
        assert abs(v - exp_root) <= RTOL * max(abs(exp_root), 1.0), (v, exp_root)
