"""What tests/test_sankoff_host.py, tests/test_gpu_sankoff.py and tools/gen_sankoff_golden.py share: the golden file, the
insertion tree of a case and a session over a case."""
import json
import os

import numpy as np

from pllamd import driver, parsimony_cases as PC, sankoff_cases as SC
from utree import UTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "sankoff.json")


def golden():
    with open(GOLDEN_PATH) as f:
        return json.load(f)


def insertion_tree(case):
    """seeded random tree over tips 0 .. tips-2: (ops of every directional vector, the facing vectors of every edge), the
    inner vectors at score indices from case.insertion_base on"""
    tree = UTree(case.tips - 1, np.random.default_rng(case.tips + 2000))
    return PC.directional_ops(tree, case.insertion_base)


def session(lib, case, matrix_name):
    return driver.SankoffSession(lib, case.tips, case.states, case.sites, SC.matrix(matrix_name, case.states), case.score_buffers,
                                 case.ancestral_buffers)


def set_tips(s, lib, case):
    cmap = SC.charmap(lib, case.states)
    for t, seq in enumerate(SC.alignment(case)):
        assert s.set_sequence(t, cmap, seq) == 1
    return cmap


def model(lib, case, matrix_name):
    m = SC.Model(case, SC.matrix(matrix_name, case.states))
    cmap = SC.charmap(lib, case.states)
    for t, seq in enumerate(SC.alignment(case)):
        m.set_sequence(t, cmap, seq)
    return m, cmap
