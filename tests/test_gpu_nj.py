"""GPU: pll_gpu_nj_tree and pll_gpu_distance_tree against pllamd/nj.py, the definition.

Both flags at nj_cases.COUNTS = 3, 4, 5, 8, 9, 33, 64, 65, 130, 257, 600 nodes: no join, one join (the four-node rule
alone), below, at and above a wave, past the 256 threads of a workgroup, and 600, where several search workgroups run at the
default rows per workgroup.

Exact inputs (additive matrices of dyadic branch lengths, all ones, the balanced dyadic tree): parent and length bit for bit
nj.py's under NJ. Noisy inputs (additive x (1 +- 5 %)): parent identical to nj.py's and |length - expected| <= B,
    B = 16 x 2.35e-12 = 3.76e-11,
16 x the worst deviation between the binary64 and long-double restatements over these same cases, measured on the CPU by
tests/test_nj_host.py::test_the_inputs_keep_their_gaps (2.348e-12, at 600 nodes, where the distances reach 11.2; at most
1.4e-15 up to 9 nodes); the factor 16 allows the device another order of adding the row sums than either restatement's.
The kernels add in nj.py's order, so the observed fraction of the bound, which every case prints, is expected to be 0.

Several workgroups and the ticket at 9 nodes: PLL_AMD_NJ_ROWS=2 in a fresh child process must give the default run's bits.
Hundreds of them (nj_cases.ROW_RUNS): one row per workgroup at 600 nodes is 599 search workgroups, so the last arrival's
loop over the partials takes up to three steps; three rows per workgroup leave the last workgroup fewer rows than the others.
The fused call is also run with its distance launches cut into pieces (PLL_AMD_DISTANCE_PAIRS).
The fused call at 9 tips x 130 sites, 4 x 4 and 20 x 4 (distance_cases): pll_gpu_distance_tree equals pll_gpu_nj_tree fed
with the distance array of pll_gpu_pairwise_distances bit for bit, distances_out equals that array, and an inner CLV of the
partition computed before the call has, downloaded after it, the bytes of the same CLV of a partition that made no such call.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import distance_cases as DC
import nj_cases as NC
from pllamd import api, driver, nj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 16 * NC.WORST_RESTATEMENT_DEVIATION


def _same_bits(got, exp):
    return np.array_equal(got[0], exp[0]) and got[1].tobytes() == exp[1].tobytes()


@pytest.mark.parametrize("n", NC.COUNTS)
@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_noisy_matrices(amd_lib, flag, n):
    exp_parent, exp_length = NC.expected("noisy", n, flag)
    parent, length = driver.nj_tree(amd_lib, NC.noisy(n), NC.FLAGS[flag])
    assert amd_lib.pll_gpu_nj_last_launch_count() == nj.launch_count(n) == (1 if n == 3 else 2 * (n - 3) + 2)
    assert np.array_equal(parent, exp_parent)
    worst = float(np.abs(length - exp_length).max())
    print(f"{flag} {n} nodes: worst |length - expected| {worst:.3g} = {worst / BOUND:.3g} of the bound {BOUND:.3g}")
    assert np.isfinite(length).all() and worst <= BOUND


@pytest.mark.parametrize("n", NC.COUNTS)
def test_exact_matrices_bit_for_bit(amd_lib, n):
    for kind in ("additive", "ones"):
        got = driver.nj_tree(amd_lib, NC.MATRICES[kind](n), 0)
        assert _same_bits(got, NC.expected(kind, n, "nj")), (kind, n)
    # BIONJ keeps an additive matrix exact too (nj.py): the same parent as NJ, every input distance reproduced
    parent, length = driver.nj_tree(amd_lib, NC.additive(n), api.NJ_BIONJ)
    assert np.array_equal(parent, NC.expected("additive", n, "nj")[0])
    assert np.array_equal(nj.tree_distances(parent, length), NC.additive(n))


@pytest.mark.parametrize("levels", NC.BALANCED_LEVELS)
def test_the_balanced_tree_bit_for_bit(amd_lib, levels):
    assert _same_bits(driver.nj_tree(amd_lib, NC.balanced(levels), 0), NC.expected("balanced", levels, "nj"))


def test_only_the_upper_triangle_is_read_and_the_outputs_are_a_function_of_the_input(amd_lib):
    m = NC.noisy(65).copy()
    first = driver.nj_tree(amd_lib, m, api.NJ_BIONJ)
    m[np.tril_indices(65)] = np.nan
    assert _same_bits(driver.nj_tree(amd_lib, m, api.NJ_BIONJ), first)


def test_several_search_workgroups_give_the_same_bits(amd_lib):
    """nine nodes, two rows of the triangle per workgroup: four search workgroups at r = 9, the ticket and the last arrival's
    reduction - in a fresh child process, since the variable is read from the process environment"""
    env = dict(os.environ, PLL_AMD_NJ_ROWS="2")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nj_rows_worker.py")], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    child = json.loads(run.stdout.strip().splitlines()[-1])
    for flag, bits in NC.FLAGS.items():
        parent, length = driver.nj_tree(amd_lib, NC.noisy(9), bits)
        assert child[flag] == [parent.tobytes().hex(), length.tobytes().hex(), nj.launch_count(9)], flag
        assert _same_bits((parent, length), NC.expected("noisy", 9, flag))


@pytest.mark.parametrize("rows", list(NC.ROW_RUNS))
def test_hundreds_of_search_workgroups_give_the_same_bits(amd_lib, rows):
    """nj_cases.ROW_RUNS in one fresh child process per value of PLL_AMD_NJ_ROWS: at one row per workgroup 600 nodes start with
    599 search workgroups, so the last arrival's loop over the partials takes three steps, later two, later one, and the ties
    of the all-ones matrix are settled across all of them; at three rows the last workgroup's rows end early. Every result is
    the default run's, bit for bit, in as many launches, and nj.py's (tests/test_nj_host.py holds the workgroup counts)"""
    items = [f"{kind}:{n}:{flag}" for kind, n, flag in NC.ROW_RUNS[rows]]
    env = dict(os.environ, PLL_AMD_NJ_ROWS=str(rows))
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nj_rows_worker.py")] + items, env=env, capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    child = json.loads(run.stdout.strip().splitlines()[-1])
    assert list(child) == items
    for item, (kind, n, flag) in zip(items, NC.ROW_RUNS[rows]):
        matrix = NC.MATRICES[kind](n)
        parent, length = driver.nj_tree(amd_lib, matrix, NC.FLAGS[flag])
        assert amd_lib.pll_gpu_nj_last_launch_count() == nj.launch_count(len(matrix))
        assert child[item] == [parent.tobytes().hex(), length.tobytes().hex(), nj.launch_count(len(matrix))], item
        exp_parent, exp_length = NC.expected(kind, n, flag)
        assert np.array_equal(parent, exp_parent), item
        if kind in NC.EXACT_KINDS:
            assert length.tobytes() == exp_length.tobytes(), item
        else:
            worst = float(np.abs(length - exp_length).max())
            print(f"{rows} rows, {item}: worst |length - expected| {worst:.3g} = {worst / BOUND:.3g} of the bound {BOUND:.3g}")
            assert np.isfinite(length).all() and worst <= BOUND


def test_refusals_with_a_device(amd_lib):
    with pytest.raises(RuntimeError) as err:
        driver.nj_tree(amd_lib, NC.noisy(5), 0, device=4096, fill=7)
    assert amd_lib.errno() != 0 and (err.value.outputs["parent"] == 7).all() and (err.value.outputs["length"] == 7).all()
    assert amd_lib.pll_gpu_nj_last_launch_count() == 0


SHAPES = {"4x4": (4, 4), "20x4": (20, 4)}
TIPS, SITES = 9, 130


def _bed(lib, shape):
    states, rate_cats = SHAPES[shape]
    seqs, cmap, exch, freqs = DC.sequences(states, TIPS, SITES)
    return DC.Tips(lib, states, rate_cats, seqs, cmap, exch, freqs)


def _inner_clv(b):
    """the one inner CLV of the partition from tips 0 and 1 over matrix 0, left on the device"""
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


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_the_fused_call(amd_lib, flag, shape):
    opt = driver.newton_options(0.1, 1e-6, 100.0, 1e-8 * SITES, 32)
    with _bed(amd_lib, shape) as plain:
        _inner_clv(plain)
        clv_before = _download(plain)
    with _bed(amd_lib, shape) as b:
        _inner_clv(b)
        lnl_before = _edge_lnl(b)
        dist = b.distances(range(TIPS), opt, want=())["distance"]
        distance_launches = b.launches()
        assert distance_launches == DC.launches_by_rule(TIPS)
        parent, length, dist_out = driver.distance_tree(amd_lib, b.p, range(TIPS), b.pi, opt, NC.FLAGS[flag])
        assert b.launches() == distance_launches + nj.launch_count(TIPS)
        assert dist_out.tobytes() == dist.tobytes()
        assert _same_bits((parent, length), driver.nj_tree(amd_lib, dist, NC.FLAGS[flag]))
        assert _same_bits((parent, length), nj.nj_tree(dist, NC.FLAGS[flag]))
        # without distances_out: the same tree
        again = driver.distance_tree(amd_lib, b.p, range(TIPS), b.pi, opt, NC.FLAGS[flag], want_distances=False)
        assert again[2] is None and _same_bits(again[:2], (parent, length))
        # a sub-list in another order: its own labels
        order = [5, 0, 7, 2]
        sub = driver.distance_tree(amd_lib, b.p, order, b.pi, opt, NC.FLAGS[flag])
        assert (sub[2] == sub[2].T).all() and (np.diag(sub[2]) == 0).all()
        assert _same_bits(sub[:2], nj.nj_tree(sub[2], NC.FLAGS[flag]))
        # the partition: untouched
        assert _edge_lnl(b) == lnl_before
        assert _download(b) == clv_before
        # and the distances after the tree are the distances before it
        assert b.distances(range(TIPS), opt, want=())["distance"].tobytes() == dist.tobytes()


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_the_fused_call_with_the_distances_cut_into_several_launches(amd_lib, flag, shape, monkeypatch):
    """PLL_AMD_DISTANCE_PAIRS = 2 x tips when the partition is created: two rows of the pair matrix per launch, the join
    behind the last of them - the uncut call's parent, length and distances, bit for bit, in the launches of both rules"""
    opt = driver.newton_options(0.1, 1e-6, 100.0, 1e-8 * SITES, 32)
    with _bed(amd_lib, shape) as b:
        parent, length, dist = driver.distance_tree(amd_lib, b.p, range(TIPS), b.pi, opt, NC.FLAGS[flag])
        assert b.launches() == DC.launches_by_rule(TIPS) + nj.launch_count(TIPS) == 2 + nj.launch_count(TIPS)
    monkeypatch.setenv("PLL_AMD_DISTANCE_PAIRS", str(2 * TIPS))
    with _bed(amd_lib, shape) as b:
        cut = driver.distance_tree(amd_lib, b.p, range(TIPS), b.pi, opt, NC.FLAGS[flag])
        assert b.launches() == DC.launches_by_rule(TIPS, 2 * TIPS) + nj.launch_count(TIPS) == 5 + nj.launch_count(TIPS)
        assert _same_bits(cut[:2], (parent, length)) and cut[2].tobytes() == dist.tobytes()
        assert b.distances(range(TIPS), opt, want=())["distance"].tobytes() == dist.tobytes()
        assert b.launches() == 5
    assert _same_bits((parent, length), nj.nj_tree(dist, NC.FLAGS[flag]))


def test_the_fused_call_refuses_with_a_device(amd_lib):
    opt = driver.newton_options(0.1, 1e-6, 100.0, 1e-6, 32)
    with _bed(amd_lib, "4x4") as b:
        for tips, flags in (((0, 1), 0), ((0, 1, 2), 2)):
            with pytest.raises(RuntimeError) as err:
                driver.distance_tree(amd_lib, b.p, tips, b.pi, opt, flags, fill=7)
            assert amd_lib.errno() == api.ERROR_PARAM_INVALID
            assert all((a == 7).all() for a in err.value.outputs.values())
        parent, length, dist = driver.distance_tree(amd_lib, b.p, (0, 1, 2), b.pi, opt, 0)
        assert list(parent) == [3, 3, 3, -1] and b.launches() == DC.launches_by_rule(3) + 1
        assert _same_bits((parent, length), nj.nj_tree(dist))
