"""shared pieces of the Newton branch-length tests (test_newton_recipe.py on the CPU, test_gpu_newton.py on the
device): the cases - the smallest shapes at which each launch path of the derivative kernels can go wrong - the edge
that is optimised, the bounds, and a session prepared up to the sumtable"""
import contextlib
import functools

from pllamd import api, driver, workload as W

T_MIN, T_MAX, MAX_ITERS = 1e-6, 100.0, api.NEWTON_MAX_ITERS
T_STARTS = (1e-6, 0.1, 5.0)

# id -> make_case keywords
CASES = {
    "dna-16x130": dict(states=4, tips=16, sites=130, seed=171),                      # one workgroup, partial last tile
    "dna-16x777": dict(states=4, tips=16, sites=777, seed=172),                      # 13 tiles: 4 workgroups, the ticket
    "dna-8x262209": dict(states=4, tips=8, sites=262209, seed=173),                  # 4097 tiles: tiles_per_wave = 2, 513 workgroups
    "dna-tip-32x777": dict(states=4, tips=32, sites=777, attributes=api.PATTERN_TIP, ambiguity_pct=5, seed=72),
    "dna-rep-32x900": dict(states=4, tips=32, sites=900, attributes=api.SITE_REPEATS, mutate_pct=5, seed=73),
    "dna-8cat-rs-16x130": dict(states=4, tips=16, sites=130, rate_cats=8, attributes=api.RATE_SCALERS, seed=74),
    "dna-cat256-rs-x70": dict(states=4, tips=256, sites=70, tree="caterpillar", brlen_scale=4, attributes=api.RATE_SCALERS, seed=75),
    "dna-pinv-16x400": dict(states=4, tips=16, sites=400, pinv=0.3, mutate_pct=4, seed=76),
    "dna-stamatakis-16x200": dict(states=4, tips=16, sites=200, asc_type=3, asc_weights=[3, 1, 4, 1], seed=176),
    "aa-16x200": dict(states=20, tips=16, sites=200, seed=77),                       # generic kernel
    "codon-8x100": dict(states=61, tips=8, sites=100, seed=80),                      # wide kernel
    "codon-17cat-8x70": dict(states=61, tips=8, sites=70, rate_cats=17, seed=181),   # 1037 > 1024 diag entries: the pre-kernel
}
IDS = list(CASES)


@functools.lru_cache(maxsize=None)
def make(cid):
    return W.make_case(cid, **CASES[cid])


def balanced(cid):
    return CASES[cid].get("tree", "balanced") == "balanced"


def tip_edge(cid):
    """(parent, parent scaler, tip, no scaler): star-like alignments give tip edges an interior optimum"""
    e = make(cid).edges[0]
    return (e[0], e[1], make(cid).tips - 1 if balanced(cid) else 0, -1)


def inner_edge(cid):
    """case.edges[0]: its optimum is at zero, so the iteration ends at t_min"""
    e = make(cid).edges[0]
    return (e[0], e[1], e[2], e[3])


def tolerance(cid):
    return 1e-8 * make(cid).sites


def bounds(cid, **over):
    kw = dict(t_min=T_MIN, t_max=T_MAX, tolerance=tolerance(cid), max_iters=MAX_ITERS)
    kw.update(over)
    return kw


@contextlib.contextmanager
def prepared(lib, cid):
    """a session with the shared eigenbasis injected and the partials computed"""
    case = make(cid)
    eig = W.eigensystem(case.model["exch"], case.freqs[0])
    with driver.Session(lib, case, api.ARCH_AVX2) as s:
        s.inject_eigen(eig, case.model["rates"])
        s.update_partials()
        yield s


def table(s, edge):
    st = s.new_sumtable()
    s.update_sumtable(edge, st)
    return st
