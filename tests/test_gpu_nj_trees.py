"""GPU: pll_gpu_nj_trees against pll_gpu_nj_tree, matrix by matrix - parent identical, length identical as 64-bit words.
No tolerance: the batched call is the single call's kernels with the replicate as a second grid dimension, and the single
call is pinned to pllamd/nj.py by tests/test_gpu_nj.py.

Shapes: 3 nodes (the three-node step alone), 4 (the four-node rule), 5, 9 and 64 with 1, 2 and 7 replicates, 600 with 3
(several search workgroups per replicate at the default rows per workgroup, one ticket per replicate and step). Within a
batch no two matrices are alike (nj_trees_worker.batch: noisy and additive ones by turns, under permuted labels), so the
replicates join different slots at every step. One batch holds the same matrix twice around the all-ones matrix, which is
all ties. On the additive matrices of dyadic lengths the bits are also pllamd/nj.py's.

Fresh child processes: PLL_AMD_NJ_ROWS=2 (nine nodes x 5 replicates: four search workgroups and one ticket per replicate)
and PLL_AMD_NJ_BATCH_BYTES for chunks of 2 + 2 + 1 give the default run's bits; the launches of one chunk are the single
tree's whatever the number of replicates, those of three chunks three times as many.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import nj_cases as NC
import nj_trees_worker as TW
from pllamd import api, driver, nj

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "nj_trees_worker.py")


def _rows_equal_the_single_call(lib, matrices, flags, got):
    parent, length = got
    assert parent.shape == length.shape == (len(matrices), 2 * matrices.shape[1] - 2)
    for b, m in enumerate(matrices):
        one_parent, one_length = driver.nj_tree(lib, m, flags)
        assert np.array_equal(parent[b], one_parent), b
        assert length[b].tobytes() == one_length.tobytes(), b


@pytest.mark.parametrize("n,replicates", [(n, r) for n in (3, 4, 5, 9, 64) for r in (1, 2, 7)] + [(600, 3)])
@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_every_tree_equals_the_single_call(amd_lib, flag, n, replicates):
    matrices = TW.batch(n, replicates)
    got = api.nj_trees(amd_lib, matrices, NC.FLAGS[flag])
    # one chunk: the single tree's launches, whatever the number of replicates
    assert amd_lib.pll_gpu_nj_last_launch_count() == nj.launch_count(n) == (1 if n == 3 else 2 * (n - 3) + 2)
    _rows_equal_the_single_call(amd_lib, matrices, NC.FLAGS[flag], got)
    if replicates > 2 and n > 4:  # different trees side by side, not one tree several times
        assert not np.array_equal(got[0][0], got[0][2])


@pytest.mark.parametrize("n", (9, 64))
@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_a_matrix_of_ties_between_two_copies_of_one_matrix(amd_lib, flag, n):
    matrices = np.stack([NC.noisy(n), NC.ones(n), NC.noisy(n)])
    parent, length = api.nj_trees(amd_lib, matrices, NC.FLAGS[flag])
    assert np.array_equal(parent[0], parent[2]) and length[0].tobytes() == length[2].tobytes()
    _rows_equal_the_single_call(amd_lib, matrices, NC.FLAGS[flag], (parent, length))
    if flag == "nj":
        exp = NC.expected("ones", n, "nj")
        assert np.array_equal(parent[1], exp[0]) and length[1].tobytes() == exp[1].tobytes()


@pytest.mark.parametrize("n", (4, 9, 64, 65))
def test_additive_matrices_bit_for_bit_the_definition(amd_lib, n):
    """dyadic branch lengths: every operation of NJ is exact, under any labels"""
    matrices = np.stack([NC.additive(n), TW.permuted(NC.additive(n), 1), NC.ones(n), TW.permuted(NC.additive(n), 2)])
    parent, length = api.nj_trees(amd_lib, matrices, 0)
    for b, m in enumerate(matrices):
        exp_parent, exp_length = nj.nj_tree(m, 0)
        assert np.array_equal(parent[b], exp_parent) and length[b].tobytes() == exp_length.tobytes(), b
        if b != 2:
            assert np.array_equal(nj.tree_distances(parent[b], length[b]), m)


def _child(items, **env):
    run = subprocess.run([sys.executable, WORKER] + items, env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_several_search_workgroups_per_replicate_give_the_same_bits(amd_lib):
    """nine nodes x 5 replicates at two rows of the triangle per workgroup: four search workgroups per replicate at r = 9,
    the last of ITS replicate reduces that replicate's partials"""
    items = [f"9:5:{flag}" for flag in NC.FLAGS]
    child = _child(items, PLL_AMD_NJ_ROWS="2")
    for item, flag in zip(items, NC.FLAGS):
        parent, length = api.nj_trees(amd_lib, TW.batch(9, 5), NC.FLAGS[flag])
        assert child[item] == [parent.tobytes().hex(), length.tobytes().hex(), nj.launch_count(9)], flag


@pytest.mark.parametrize("flag", list(NC.FLAGS))
def test_chunks_of_two_two_and_one_give_the_same_bits(amd_lib, flag):
    """a budget of two and a half replicates (a matrix of 8 x 81 bytes and the working set each): 5 replicates run as
    2 + 2 + 1, three times the launches of one tree"""
    per_replicate = 8 * 81 + int(amd_lib.pllgpu_nj_scratch_bytes(9, NC.FLAGS[flag]))
    item = f"9:5:{flag}"
    child = _child([item], PLL_AMD_NJ_BATCH_BYTES=str(2 * per_replicate + per_replicate // 2))
    parent, length = api.nj_trees(amd_lib, TW.batch(9, 5), NC.FLAGS[flag])
    assert amd_lib.pll_gpu_nj_last_launch_count() == 2 * 6 + 2
    assert child[item] == [parent.tobytes().hex(), length.tobytes().hex(), 3 * (2 * 6 + 2)]


def test_a_bad_entry_in_the_last_replicate_refuses_the_whole_call(amd_lib):
    matrices = TW.batch(9, 4).copy()
    matrices[3, 2, 7] = -0.5
    with pytest.raises(RuntimeError) as err:
        api.nj_trees(amd_lib, matrices, 0, fill=7)
    assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "[3][2][7]" in str(err.value)
    assert (err.value.outputs["parent"] == 7).all() and (err.value.outputs["length"] == 7).all()
    # a device that does not exist: refused behind the entries, outputs untouched, no launch counted
    with pytest.raises(RuntimeError) as err:
        api.nj_trees(amd_lib, TW.batch(9, 4), 0, device=4096, fill=7)
    assert amd_lib.errno() != 0 and (err.value.outputs["parent"] == 7).all() and (err.value.outputs["length"] == 7).all()
    assert amd_lib.pll_gpu_nj_last_launch_count() == 0
