"""GPU: pll_gpu_bootstrap_distance_trees against its definition, word for word. Row b of every output is what the sequence
    row FIRST + b of pll_gpu_draw_replicate_weights(seed) -> pll_set_pattern_weights(that row) -> pll_gpu_distance_tree
returns on the same partition (status: that of pll_gpu_pairwise_distances under the same row), the partition's own weights
restored afterwards. Every one of those calls is pinned to the reference and to pllamd/rell.py, distances.py and nj.py by its
own tests; no tolerance appears here.

Shapes (bootstrap_trees_worker.SHAPES): DNA 4 x 4 at 9 tips x 1029 sites - rows 1032 words apart on the device, a tail in
the four-sites-per-thread loop - once with weights that hold zeros and one large value (the general draw) and once with all
weights 1 (the draw's short cut); 20 x 4 at 6 tips x 203 sites; 61 x 4 at 4 tips x 64 sites (one join: the four-node rule).
Five replicates from row 3, both flags.

Fresh child processes: PLL_AMD_BOOTSTRAP_BYTES for chunks of 2 + 2 + 1; PLL_AMD_DISTANCE_PAIRS = 2 x tips, where every
replicate's distance launches are cut over rows (and so over replicates), and = 2 matrices, where a launch holds two
replicates. The bits are the default run's and the launches those of the rule include/pll_amd_device.h states.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bootstrap_trees_worker as BW
import distance_cases as DC
import nj_cases as NC
from pllamd import api, driver, nj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "bootstrap_trees_worker.py")
SEED, FIRST, REPS = BW.SEED, BW.FIRST, BW.REPLICATES


def _current_weights(b):
    return api.as_np(b.part.pattern_weights, b.sites, np.uint32).copy()


def by_definition(b, shape, flags, first, replicates, seed=SEED):
    """the three-step sequence, replicate by replicate, on the bed itself; its weights are put back"""
    lib, opt, tips = b.lib, BW.options(shape), range(b.tips)
    own = _current_weights(b)
    rows = driver.draw_replicate_weights(lib, b.p, seed, first, replicates)
    out = {"parent": [], "length": [], "distances": [], "status": [], "weights": rows}
    try:
        for row in rows:
            lib.pll_set_pattern_weights(b.p, api.uptr(np.ascontiguousarray(row)))
            parent, length, dist = driver.distance_tree(lib, b.p, tips, b.pi, opt, flags)
            status = b.distances(tips, opt, want=("status",))["status"]
            for name, a in zip(("parent", "length", "distances", "status"), (parent, length, dist, status)):
                out[name].append(a)
    finally:
        lib.pll_set_pattern_weights(b.p, api.uptr(own))
    return {name: np.stack(a) if isinstance(a, list) else a for name, a in out.items()}


def _same_words(got, exp, names=BW.OUTPUTS):
    for name in names:
        assert got[name].dtype == exp[name].dtype and got[name].shape == exp[name].shape, name
        assert got[name].tobytes() == exp[name].tobytes(), name


def launches_by_rule(count, replicates, per_chunk=None, max_pairs=DC.MAX_PAIRS, prefix_sums=True):
    """include/pll_amd_device.h, pllgpu_bootstrap_distance_trees: the prefix sums (when formed) and the code vectors once,
    then per chunk one draw, the pair launches cut over replicates first and then over rows, and the join"""
    per_chunk = min(replicates, 65535) if per_chunk is None else per_chunk
    rows = max(1, min(65535, max_pairs // count))
    total = (1 if prefix_sums else 0) + 1
    for r0 in range(0, replicates, per_chunk):
        n = min(per_chunk, replicates - r0)
        if rows >= count - 1:
            m = max(1, min(65535, max_pairs // (count * (count - 1))))
            pair_launches = (n + m - 1) // m
        else:
            pair_launches = n * ((count - 1 + rows - 1) // rows)
        total += 1 + pair_launches + nj.launch_count(count)
    return total


@pytest.mark.parametrize("shape", list(BW.SHAPES))
@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_every_row_equals_the_definition(amd_lib, flag, shape):
    with BW.bed(amd_lib, shape) as b:
        exp = by_definition(b, shape, NC.FLAGS[flag], FIRST, REPS)
        assert (exp["weights"].sum(axis=1) == b.weight_sum).all() and len({w.tobytes() for w in exp["weights"]}) == REPS
        # (the definition's last step uploaded the partition's weights again: the prefix sums are formed once more)
        got = api.bootstrap_distance_trees(amd_lib, b.p, range(b.tips), b.pi, BW.options(shape), NC.FLAGS[flag], SEED, FIRST, REPS)
        assert b.launches() == launches_by_rule(b.tips, REPS)
        _same_words(got, exp)
        assert (got["distances"] == got["distances"].transpose(0, 2, 1)).all() and (got["distances"][:, np.arange(b.tips), np.arange(b.tips)] == 0).all()
        if b.tips > 4:  # the replicates are different trees, not one tree five times
            assert len({p.tobytes() + l.tobytes() for p, l in zip(got["parent"], got["length"])}) > 1
        # a second call forms no prefix sums and gives the same words
        again = api.bootstrap_distance_trees(amd_lib, b.p, range(b.tips), b.pi, BW.options(shape), NC.FLAGS[flag], SEED, FIRST, REPS)
        assert b.launches() == launches_by_rule(b.tips, REPS, prefix_sums=False)
        _same_words(again, got)


@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_rows_are_numbered_absolutely(amd_lib, flag):
    """a call for rows 3..7 gives rows 3..7 of a call for rows 0..7; a sub-list in another order has its own labels"""
    with BW.bed(amd_lib, "dna") as b:
        opt = BW.options("dna")
        part = api.bootstrap_distance_trees(amd_lib, b.p, range(b.tips), b.pi, opt, NC.FLAGS[flag], SEED, FIRST, REPS)
        whole = api.bootstrap_distance_trees(amd_lib, b.p, range(b.tips), b.pi, opt, NC.FLAGS[flag], SEED, 0, FIRST + REPS)
        _same_words(part, {name: a[FIRST:] for name, a in whole.items()})
        order = [5, 0, 7, 2]
        sub = api.bootstrap_distance_trees(amd_lib, b.p, order, b.pi, opt, NC.FLAGS[flag], SEED, FIRST, 2)
        assert sub["weights"].tobytes() == part["weights"][:2].tobytes()
        for r in range(2):
            parent, length = nj.nj_tree(sub["distances"][r], NC.FLAGS[flag])
            assert np.array_equal(sub["parent"][r], parent) and sub["length"][r].tobytes() == length.tobytes()


def _child(items, **env):
    run = subprocess.run([sys.executable, WORKER] + items, env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def _default_run(lib, shape, flag):
    with BW.bed(lib, shape) as b:
        got = api.bootstrap_distance_trees(lib, b.p, range(b.tips), b.pi, BW.options(shape), NC.FLAGS[flag], SEED, FIRST, REPS)
        assert b.launches() == launches_by_rule(b.tips, REPS)
        return [got[name].tobytes().hex() for name in BW.OUTPUTS], b.tips, b.sites


@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_chunks_of_two_two_and_one_give_the_same_bits(amd_lib, flag):
    item = f"dna:{flag}"
    words, tips, sites = _default_run(amd_lib, "dna", flag)
    wstride = (sites + 3) // 4 * 4
    per_replicate = 4 * wstride + 48 * tips * tips + int(amd_lib.pllgpu_nj_scratch_bytes(tips, NC.FLAGS[flag]))
    child = _child([item], PLL_AMD_BOOTSTRAP_BYTES=str(2 * per_replicate + per_replicate // 2))
    assert child[item] == words + [launches_by_rule(tips, REPS, per_chunk=2)]
    assert launches_by_rule(tips, REPS, per_chunk=2) == 2 + 3 * (1 + 1 + nj.launch_count(tips))


@pytest.mark.parametrize("pairs,pair_launches", [(2 * 9, 5 * 4), (2 * 9 * 8, 3)])
def test_the_distance_launches_cut_over_replicates_and_rows(amd_lib, pairs, pair_launches):
    """9 tips, 5 replicates in one chunk. 18 workgroups per launch: two rows of one replicate's pair matrix, four launches
    per replicate. 144: two replicates' matrices, launches of 2 + 2 + 1 replicates."""
    items = [f"dna:{flag}" for flag in NC.FLAGS]
    child = _child(items, PLL_AMD_DISTANCE_PAIRS=str(pairs))
    for item, flag in zip(items, NC.FLAGS):
        words, tips, _ = _default_run(amd_lib, "dna", flag)
        assert launches_by_rule(tips, REPS, max_pairs=pairs) == 2 + 1 + pair_launches + nj.launch_count(tips)
        assert child[item] == words + [launches_by_rule(tips, REPS, max_pairs=pairs)], item


def test_both_cuts_at_once(amd_lib):
    item = "aa:bionj"
    words, tips, sites = _default_run(amd_lib, "aa", "bionj")
    per_replicate = 4 * ((sites + 3) // 4 * 4) + 48 * tips * tips + int(amd_lib.pllgpu_nj_scratch_bytes(tips, api.NJ_BIONJ))
    child = _child([item], PLL_AMD_BOOTSTRAP_BYTES=str(2 * per_replicate + 8), PLL_AMD_DISTANCE_PAIRS=str(3 * tips))
    expect = launches_by_rule(tips, REPS, per_chunk=2, max_pairs=3 * tips)
    assert expect == 2 + 3 + 5 * 2 + 3 * nj.launch_count(tips)
    assert child[item] == words + [expect]


def _inner_clv(b):
    lib = b.lib
    mi, bl = np.zeros(1, dtype=np.uint32), np.array([0.1])
    assert lib.pll_update_prob_matrices(b.p, api.uptr(b.pi), api.uptr(mi), api.dptr(bl), 1), (lib.errno(), lib.errmsg())
    lib.pll_update_partials(b.p, api.make_ops([(b.tips, DC.NONE, 0, 0, DC.NONE, 1, 0, DC.NONE)]), 1)


def _edge_lnl(b):
    fi = np.zeros(b.rate_cats, dtype=np.uint32)
    return b.lib.pll_compute_edge_loglikelihood(b.p, b.tips, DC.NONE, 2, DC.NONE, 0, api.uptr(fi), None)


def _download(b):
    assert b.lib.pll_gpu_sync_clv(b.p, b.tips)
    return api.as_np(b.part.clv[b.tips], b.sites * b.rate_cats * int(b.part.states_padded), np.float64).tobytes()


@pytest.mark.parametrize("shape", ["dna", "aa"])
def test_the_partition_is_untouched(amd_lib, shape):
    with BW.bed(amd_lib, shape) as b:
        opt, tips = BW.options(shape), range(b.tips)
        _inner_clv(b)
        lnl_before, clv_before, weights_before = _edge_lnl(b), _download(b), _current_weights(b)
        dist_before = b.distances(tips, opt)
        drawn_before = driver.draw_replicate_weights(amd_lib, b.p, SEED + 1, 2, 3)
        for flag in NC.FLAGS.values():
            api.bootstrap_distance_trees(amd_lib, b.p, tips, b.pi, opt, flag, SEED, FIRST, REPS)
        assert _current_weights(b).tobytes() == weights_before.tobytes() == b.weights.tobytes()
        assert _edge_lnl(b) == lnl_before and _download(b) == clv_before
        dist_after = b.distances(tips, opt)
        assert all(dist_after[name].tobytes() == dist_before[name].tobytes() for name in driver.DISTANCE_OUTPUTS)
        assert driver.draw_replicate_weights(amd_lib, b.p, SEED + 1, 2, 3).tobytes() == drawn_before.tobytes()
        # and the tree of the partition's own weights is still the tree of its own weights
        parent, length, dist = driver.distance_tree(amd_lib, b.p, tips, b.pi, opt, 0)
        assert dist.tobytes() == dist_before["distance"].tobytes()


WANTS = [tuple(n for n, keep in zip(api.BOOTSTRAP_OPTIONAL, (d, s, w)) if keep) for d in (0, 1) for s in (0, 1) for w in (0, 1)]


@pytest.mark.parametrize("want", WANTS, ids=lambda w: "+".join(w) or "none")
def test_optional_outputs_may_be_null(amd_lib, want):
    """every subset of distances, status and weights: what is asked for has the full call's words"""
    with BW.bed(amd_lib, "aa") as b:
        full = api.bootstrap_distance_trees(amd_lib, b.p, range(b.tips), b.pi, BW.options("aa"), api.NJ_BIONJ, SEED, FIRST, REPS)
        got = api.bootstrap_distance_trees(amd_lib, b.p, range(b.tips), b.pi, BW.options("aa"), api.NJ_BIONJ, SEED, FIRST, REPS, want=want)
        assert set(got) == {"parent", "length"} | set(want)
        _same_words(got, full, names=list(got))


def _refused(lib, b, shape, code, flags=0, tips=None):
    with pytest.raises(RuntimeError) as err:
        api.bootstrap_distance_trees(lib, b.p, range(b.tips) if tips is None else tips, b.pi, BW.options(shape), flags, SEED, FIRST, REPS, fill=7)
    assert lib.errno() == code, (lib.errno(), lib.errmsg())
    assert set(err.value.outputs) == set(BW.OUTPUTS) and all((a == 7).all() for a in err.value.outputs.values())
    return str(err.value)


def test_refusals_with_a_device(amd_lib):
    with BW.bed(amd_lib, "dna", attrs=api.SITE_REPEATS) as b:
        _refused(amd_lib, b, "dna", api.ERROR_GPU_UNSUPPORTED)
    with BW.bed(amd_lib, "dna", prop_invar=0.2) as b:
        assert "prop_invar" in _refused(amd_lib, b, "dna", api.ERROR_GPU_UNSUPPORTED)
    with BW.bed(amd_lib, "dna") as b:
        # count and flags stand behind every check of the distances, the device included
        assert "at least 3" in _refused(amd_lib, b, "dna", api.ERROR_PARAM_INVALID, tips=(0, 1))
        assert "flag" in _refused(amd_lib, b, "dna", api.ERROR_PARAM_INVALID, flags=2)
        # weights that add up to 0: the refusal of pll_gpu_draw_replicate_weights, last
        zeros = np.zeros(b.sites, dtype=np.uint32)
        amd_lib.pll_set_pattern_weights(b.p, api.uptr(zeros))
        assert "add up to 0" in _refused(amd_lib, b, "dna", api.ERROR_PARAM_INVALID)
        assert "flag" in _refused(amd_lib, b, "dna", api.ERROR_PARAM_INVALID, flags=2)
        amd_lib.pll_set_pattern_weights(b.p, api.uptr(b.weights))
        got = api.bootstrap_distance_trees(amd_lib, b.p, (0, 1, 2), b.pi, BW.options("dna"), 0, SEED, 0, 2)
        assert (got["parent"] == [3, 3, 3, -1]).all() and b.launches() == launches_by_rule(3, 2)
