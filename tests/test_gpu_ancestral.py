"""GPU: marginal ancestral states (pll_compute_node_ancestral, pll_compute_node_ancestral_extbuf,
pll_gpu_node_ancestral_async) against the reference build.

Tolerance everywhere: every entry within RTOL (1e-10) relative of the expected one - every term of an entry is
non-negative, nothing cancels -, an entry expected as exactly 0 is 0, every row sums to 1 within 1e-12.

With PLL_ATTRIB_RATE_SCALERS the library honours the per-rate scaling counts of both ends, the reference does not
(src/likelihood.c:711-743): there the expected values are `restated`, a numpy restatement of

    a[n][j] = sum_k w_k pi_f(k)[j] x_k[n][j] (P_k y_k[n])[j] 2^(-256 min(count_k[n] - min_k count[n], 4)),   a[n] /= sum_j a[n][j]

fed with the REFERENCE's CLVs, tip codes, matrices and scaler vectors (read from its partition's host memory; nothing
comes from the library under test). The golden sweep pins that restatement to the reference on every case whose ends
carry no counts."""
import ctypes as C
import glob
import json
import os

import numpy as np
import pytest

from ancestral_common import SUMTOL, _part_arrays, assert_table, restated
from pllamd import api, driver, fixtures, workload as W
from utree import UTree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _golden_cases():
    """every case of tests/golden/*.npz that names an edge (`edges`, or the `deriv_edges` of the derivative fixtures; the
    two root-only cases name none) but the site-repeats ones (refused: test_error_paths)"""
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))):
        name = os.path.basename(path)[:-4]
        if name.startswith("model_"):
            continue  # a substitution model, not a case
        meta = json.loads(bytes(np.load(path)["meta"]).decode())
        if not (meta["attributes"] & api.SITE_REPEATS) and (meta["edges"] or meta["extra"].get("deriv_edges")):
            out.append(name)
    return out


def _case_edges(case, extra):
    """(node, node scaler, other, other scaler, matrix): the case's edges; a derivative fixture names (parent, scaler,
    child, scaler) and forms its own matrices per branch length - here its edge goes with the case's matrix 0"""
    return [tuple(e) for e in case.edges] or [tuple(de[0]) + (0,) for de in extra["deriv_edges"]]


def _call(lib, p, edge, fi, sites, states):
    out = np.full((sites, states), -7.0)
    ok = lib.pll_compute_node_ancestral(p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(fi), api.dptr(out))
    return ok, out


def _ends_unscaled(lib, p, edge):
    _, _, _, _, (cn, co) = _part_arrays(lib, p, *edge)
    return not cn.any() and not co.any()


# ---- 1. golden sweep -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _golden_cases())
def test_golden_sweep(amd_lib, ref_lib, name):
    case, _, extra = fixtures.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    fi = np.ascontiguousarray(case.freqs_indices, dtype=np.uint32)
    worst, done = 0.0, 0
    with driver.Session(amd_lib, case) as a, driver.Session(ref_lib, case) as r:
        a.update_partials()
        r.update_partials()
        for e in _case_edges(case, extra):
            for edge in (e, (e[2], e[3], e[0], e[1], e[4])):
                what = (name, edge)
                if (case.attributes & api.PATTERN_TIP) and edge[0] < case.tips:
                    # the node's end has no CLV: the reference dereferences NULL, the library refuses
                    ok, _ = _call(amd_lib, a.p, edge, fi, case.sites, case.states)
                    assert not ok and amd_lib.errno() == 113, what
                    continue
                ok, exp = _call(ref_lib, r.p, edge, fi, case.sites, case.states)
                assert ok, (what, ref_lib.errno(), ref_lib.errmsg())
                assert np.isfinite(exp).all(), (what, "the reference's own result has non-finite rows")
                ok, got = _call(amd_lib, a.p, edge, fi, case.sites, case.states)
                assert ok, (what, amd_lib.errno(), amd_lib.errmsg())
                model = restated(ref_lib, r.p, edge, fi)
                if not (case.attributes & api.RATE_SCALERS) or _ends_unscaled(ref_lib, r.p, edge):
                    worst = max(worst, assert_table(got, exp, what))
                    assert_table(model, exp, (what, "restatement against the reference"))
                else:
                    worst = max(worst, assert_table(got, model, (what, "per-rate counts: against the restatement")))
                got2 = a.node_ancestral(edge)
                assert np.array_equal(got, got2), (what, "Session.node_ancestral")
                done += 1
    assert done, name
    print(f"ancestral {name}: {done} tables, worst rel err {worst:.2e}")


# ---- trees that rescale --------------------------------------------------------------------------------------------
class Driven:
    """one library's partition over a UTree (per-site or per-rate scalers on every inner node)"""

    def __init__(self, lib, tree, states, sites, attrs, seqs, cmap, exch, freqs, rates):
        self.lib, self.states, self.sites = lib, states, sites
        t = tree.tips
        self.p = lib.pll_partition_create(t, t - 2, states, sites, 1, 2 * t - 3, len(rates), t - 2, attrs | api.ARCH_AVX2)
        assert self.p, (lib.errno(), lib.errmsg())
        f = np.ascontiguousarray(freqs, dtype=np.float64)
        e = np.ascontiguousarray(exch, dtype=np.float64)
        r = np.ascontiguousarray(rates, dtype=np.float64)
        lib.pll_set_frequencies(self.p, 0, api.dptr(f))
        lib.pll_set_subst_params(self.p, 0, api.dptr(e))
        lib.pll_set_category_rates(self.p, api.dptr(r))
        cm = (C.c_ulonglong * 256)(*[int(x) for x in cmap])
        for i, s in enumerate(seqs):
            assert lib.pll_set_tip_states(self.p, i, cm, s), (lib.errno(), lib.errmsg())
        self.fi = np.zeros(len(rates), dtype=np.uint32)
        pairs = tree.branches()
        idx = np.ascontiguousarray([m for m, _ in pairs], dtype=np.uint32)
        bl = np.ascontiguousarray([x for _, x in pairs], dtype=np.float64)
        assert lib.pll_update_prob_matrices(self.p, api.uptr(self.fi), api.uptr(idx), api.dptr(bl), len(pairs))

    def update(self, ops):
        if ops:
            self.lib.pll_update_partials(self.p, api.make_ops(ops), len(ops))

    def ancestral(self, edge):
        ok, out = _call(self.lib, self.p, edge, self.fi, self.sites, self.states)
        assert ok, (edge, self.lib.errno(), self.lib.errmsg())
        return out

    def close(self):
        self.lib.pll_partition_destroy(self.p)


def _alignment(states, tips, sites, seed):
    st = W.random_states(tips, sites, states, seed, 15)
    if states == 4:
        return W.states_to_sequences(st, W.NT_CHARS), W.map_nt(), W.GTR_DNA["exch"], W.GTR_DNA["freqs"]
    ex, fr = W.synthetic_exch(states)
    return W.states_to_sequences(st, W.AA_CHARS), W.map_aa(), ex, fr


def _tips_behind(tree, rec):
    return sum(1 for q in tree.subtree_records(rec) if not q.inner)


def _deep_records(tree, rng, count, least):
    """`count` records of inner nodes, each with at least `least` tips in the subtree its CLV summarises"""
    cand = [r for r in tree.records() if r.inner and _tips_behind(tree, r) >= least]
    assert len(cand) >= count, len(cand)
    return [cand[int(i)] for i in rng.choice(len(cand), size=count, replace=False)]


def _tree_pair(amd_lib, ref_lib, states, tips, sites, attrs, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    tree = UTree(tips, rng)
    seqs, cmap, exch, freqs = _alignment(states, tips, sites, seed + 1)
    rates = W.gamma_rates_mean(0.7, 4)
    return rng, tree, [Driven(lib, tree, states, sites, attrs, seqs, cmap, exch, freqs, rates) for lib in (amd_lib, ref_lib)]


@pytest.mark.parametrize("states,tips,sites,least", [(4, 600, 700, 250), (20, 200, 300, 90)], ids=["dna600", "aa200"])
def test_scaled_trees(amd_lib, ref_lib, states, tips, sites, least):
    """per-site scalers on trees deep enough to rescale: ten inner nodes, each after the partial traversal that turns
    the CLVs towards it; the counts cancel in the ratio, so the kernel never reads them"""
    rng, tree, (a, r) = _tree_pair(amd_lib, ref_lib, states, tips, sites, 0, 8100 + states)
    worst = 0.0
    try:
        for rec in _deep_records(tree, rng, 10, least):
            ops = tree.ops_for(rec)
            a.update(ops)
            r.update(ops)
            edge = tree.edge_args(rec)
            sc = api.as_np(r.p.contents.scale_buffer[edge[1]], sites, np.uint32)
            assert sc.any(), ("the reference did not rescale at the evaluated node", edge)
            worst = max(worst, assert_table(a.ancestral(edge), r.ancestral(edge), (states, edge)))
    finally:
        a.close()
        r.close()
    print(f"ancestral, scaled tree, {states} states {tips} taxa: worst rel err {worst:.2e}")


@pytest.mark.parametrize("states,tips,sites,least", [(4, 600, 700, 250), (20, 200, 300, 90)], ids=["dna600", "aa200"])
def test_rate_scalers_on_a_tree_that_rescales(amd_lib, ref_lib, states, tips, sites, least):
    """PLL_ATTRIB_RATE_SCALERS with counts that differ between the categories of a site: the library honours them, the
    expected values are the restatement on the reference's CLVs and scaler vectors"""
    rng, tree, (a, r) = _tree_pair(amd_lib, ref_lib, states, tips, sites, api.RATE_SCALERS, 8300 + states)
    worst, uneven = 0.0, 0
    try:
        for rec in _deep_records(tree, rng, 10, least):
            ops = tree.ops_for(rec)
            a.update(ops)
            r.update(ops)
            edge = tree.edge_args(rec)
            sc = api.as_np(r.p.contents.scale_buffer[edge[1]], sites * 4, np.uint32).reshape(sites, 4)
            assert sc.any(), ("the reference did not rescale at the evaluated node", edge)
            uneven += int((sc.max(1) != sc.min(1)).sum())
            worst = max(worst, assert_table(a.ancestral(edge), restated(ref_lib, r.p, edge, r.fi), (states, edge)))
        assert uneven, "no site whose categories carry different counts: the case shows nothing"
    finally:
        a.close()
        r.close()
    print(f"ancestral, per-rate scalers, {states} states {tips} taxa: {uneven} uneven sites, worst rel err {worst:.2e}")


# ---- 4. the _extbuf form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("states,attrs", [(4, 0), (4, api.PATTERN_TIP), (20, 0)])
def test_extbuf_same_bits_and_buffers_untouched(amd_lib, states, attrs):
    case = W.make_case("extbuf", states, 16, 333, attributes=attrs, seed=31)
    fi = np.zeros(4, dtype=np.uint32)
    with driver.Session(amd_lib, case) as s:
        s.update_partials()
        sp = s.sp
        for edge in (case.edges[0], (case.edges[0][2], case.edges[0][3], case.edges[0][0], case.edges[0][1], case.edges[0][4])):
            ok, plain = _call(amd_lib, s.p, edge, fi, case.sites, states)
            assert ok
            temp_clv = np.full(case.sites * 4 * sp, -3.25)
            temp_scaler = np.full(case.sites * 4, 0xABCD1234, dtype=np.uint32)
            ident = np.full(4 * states * sp + sp * sp, -5.5)
            out = np.full((case.sites, states), -7.0)
            assert amd_lib.pll_compute_node_ancestral_extbuf(s.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(fi), api.dptr(out),
                                                             api.dptr(temp_clv), api.uptr(temp_scaler), api.dptr(ident))
            assert np.array_equal(out, plain)
            assert (temp_clv == -3.25).all() and (temp_scaler == 0xABCD1234).all() and (ident == -5.5).all()


# ---- 5. the stream-ordered form ------------------------------------------------------------------------------------
@pytest.mark.parametrize("states", [4, 20])
def test_async_three_nodes_one_synchronisation(amd_lib, states):
    hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")  # the runtime the library itself is linked against
    sites = 5000
    case = W.make_case("async", states, 16, sites, seed=95)
    n = sites * states
    dev = C.c_void_p()
    assert hip.hipMalloc(C.byref(dev), C.c_size_t(3 * n * 8)) == 0
    try:
        fi = np.zeros(4, dtype=np.uint32)
        with driver.Session(amd_lib, case) as s:
            s.update_partials()
            e = case.edges[0]
            last = case.op_batches[-1][-1]  # (parent, pscaler, child1, matrix1, cscaler1, child2, ...): a third orientation
            edges = [tuple(e), (e[2], e[3], e[0], e[1], e[4]), (last[0], last[1], last[2], last[4], last[3])]
            sync = []
            for edge in edges:
                ok, t = _call(amd_lib, s.p, edge, fi, sites, states)
                assert ok
                sync.append(t)
            for i, edge in enumerate(edges):
                before = amd_lib.pll_gpu_last_launch_count(s.p)
                assert amd_lib.pll_gpu_node_ancestral_async(s.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(fi),
                                                            C.c_void_p(dev.value + i * n * 8))
                assert amd_lib.pll_gpu_last_launch_count(s.p) - before == 1
            assert amd_lib.pll_gpu_synchronize(s.p)
            host = np.zeros(3 * n)
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, C.c_size_t(3 * n * 8), 2) == 0  # hipMemcpyDeviceToHost
            for i in range(3):
                assert np.array_equal(host[i * n:(i + 1) * n].reshape(sites, states), sync[i]), i
            assert not np.array_equal(sync[0], sync[1])
            # the synchronous path still works afterwards
            ok, again = _call(amd_lib, s.p, edges[0], fi, sites, states)
            assert ok and np.array_equal(again, sync[0])
            assert not amd_lib.pll_gpu_node_ancestral_async(s.p, e[0], e[1], e[2], e[3], e[4], api.uptr(fi), None)
            assert amd_lib.errno() == 113
    finally:
        hip.hipFree(dev)


# ---- 6. sizes that are not tile multiples ----------------------------------------------------------------------------
@pytest.mark.parametrize("sites", [1, 63, 64, 65, 100003])
@pytest.mark.parametrize("states", [4, 20])
def test_sites_off_the_tile(amd_lib, ref_lib, states, sites):
    tips = 8 if sites > 1000 else 16
    for attrs in (0, api.PATTERN_TIP):
        case = W.make_case("sizes", states, tips, sites, attributes=attrs, seed=40 + states)
        fi = np.zeros(4, dtype=np.uint32)
        with driver.Session(amd_lib, case) as a, driver.Session(ref_lib, case) as r:
            a.update_partials()
            r.update_partials()
            e = case.edges[0]
            last = case.op_batches[-1][0]  # an op over tips where there is one: the other end as tip codes
            for edge in (tuple(e), (e[2], e[3], e[0], e[1], e[4]), (last[0], last[1], last[2], last[4], last[3])):
                if attrs and edge[0] < tips:
                    continue
                ok, exp = _call(ref_lib, r.p, edge, fi, sites, states)
                assert ok
                guard = np.full(sites * states + 64, -7.0)  # nothing is written past the table
                assert amd_lib.pll_compute_node_ancestral(a.p, edge[0], edge[1], edge[2], edge[3], edge[4], api.uptr(fi), api.dptr(guard))
                assert (guard[sites * states:] == -7.0).all()
                assert_table(guard[:sites * states].reshape(sites, states), exp, (states, sites, attrs, edge))


@pytest.mark.parametrize("states", [2, 64])
def test_other_state_counts(amd_lib, ref_lib, states):
    for attrs, rate_cats, sites in ((0, 4, 130), (api.PATTERN_TIP, 4, 65), (0, 1, 70), (api.PATTERN_TIP, 3, 1)):
        case = W.make_case("states", states, 8, sites, rate_cats=rate_cats, attributes=attrs, seed=50 + states)
        fi = np.zeros(rate_cats, dtype=np.uint32)
        with driver.Session(amd_lib, case) as a, driver.Session(ref_lib, case) as r:
            a.update_partials()
            r.update_partials()
            e = case.edges[0]
            last = case.op_batches[-1][0]
            for edge in (tuple(e), (e[2], e[3], e[0], e[1], e[4]), (last[0], last[1], last[2], last[4], last[3])):
                if attrs and edge[0] < case.tips:
                    continue
                ok, exp = _call(ref_lib, r.p, edge, fi, sites, states)
                assert ok
                ok, got = _call(amd_lib, a.p, edge, fi, sites, states)
                assert ok, (amd_lib.errno(), amd_lib.errmsg())
                assert_table(got, exp, (states, attrs, rate_cats, sites, edge))


# ---- 7. error paths --------------------------------------------------------------------------------------------------
def test_error_paths(amd_lib, ref_lib):
    fi = np.zeros(4, dtype=np.uint32)
    both = {}
    # site repeats: refused by both, the same way
    case = W.make_case("err_rep", 4, 8, 100, attributes=api.SITE_REPEATS, seed=3)
    for key, lib in (("amd", amd_lib), ("ref", ref_lib)):
        with driver.Session(lib, case) as s:
            s.update_partials()
            e = case.edges[0]
            ok, _ = _call(lib, s.p, e, fi, 100, 4)
            both[key] = (ok, lib.errno(), lib.errmsg())
    assert both["amd"] == both["ref"] == (0, 130, "Site repeats are not compatible with ancestral state reconstruction!")

    case = W.make_case("err", 4, 8, 100, seed=3)
    sp = 4
    temp_clv, temp_scaler, ident = np.zeros(100 * 4 * sp), np.zeros(100 * 4, dtype=np.uint32), np.zeros(4 * 4 * sp + sp * sp)
    out = np.zeros((100, 4))
    res = {}
    for key, lib in (("amd", amd_lib), ("ref", ref_lib)):
        with driver.Session(lib, case) as s:
            s.update_partials()
            e = case.edges[0]
            got = []
            # the _extbuf form checks its pointers in the reference too
            for args in ((None, api.dptr(temp_clv), api.uptr(temp_scaler), api.dptr(ident)),
                         (api.dptr(out), None, api.uptr(temp_scaler), api.dptr(ident)),
                         (api.dptr(out), api.dptr(temp_clv), None, api.dptr(ident)),
                         (api.dptr(out), api.dptr(temp_clv), api.uptr(temp_scaler), None)):
                ok = lib.pll_compute_node_ancestral_extbuf(s.p, e[0], e[1], e[2], e[3], e[4], api.uptr(fi), *args)
                got.append((ok, lib.errno(), lib.errmsg()))
            ok = lib.pll_compute_node_ancestral_extbuf(None, e[0], e[1], e[2], e[3], e[4], api.uptr(fi), api.dptr(out),
                                                       api.dptr(temp_clv), api.uptr(temp_scaler), api.dptr(ident))
            got.append((ok, lib.errno(), lib.errmsg()))
            res[key] = got
    assert res["amd"] == res["ref"]
    assert [g[:2] for g in res["amd"]] == [(0, 113)] * 5
    assert res["amd"][0][2] == "Parameter value is NULL!" and res["amd"][1][2] == "NULL buffer pointer"

    # where the reference would crash (it dereferences what it is given) the library fails
    with driver.Session(amd_lib, case) as s:
        s.update_partials()
        e = case.edges[0]
        assert not amd_lib.pll_compute_node_ancestral(None, e[0], e[1], e[2], e[3], e[4], api.uptr(fi), api.dptr(out))
        assert amd_lib.errno() == 113
        assert not amd_lib.pll_compute_node_ancestral(s.p, e[0], e[1], e[2], e[3], e[4], api.uptr(fi), None)
        assert amd_lib.errno() == 113
        nodes, mats, scs = 8 + case.clv_buffers, case.prob_matrices, case.scale_buffers
        for bad in ((nodes, e[1], e[2], e[3], e[4]), (e[0], e[1], nodes, e[3], e[4]), (e[0], e[1], e[2], e[3], mats),
                    (e[0], scs, e[2], e[3], e[4]), (e[0], e[1], e[2], scs, e[4])):
            ok, _ = _call(amd_lib, s.p, bad, fi, 100, 4)
            assert not ok and amd_lib.errno() == 113, bad
        ok, good = _call(amd_lib, s.p, e, fi, 100, 4)
        assert ok and abs(good.sum(1) - 1).max() <= SUMTOL
