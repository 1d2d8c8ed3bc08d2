"""GPU: every entry point that reads a scale buffer, driven with scaling counts the CALLER wrote (scaler_cases.py: the
count tables, the shapes and which kernel family each reaches, why written counts are sound inputs).

partition->scale_buffer[i] is written on the host and handed over with pll_gpu_invalidate(PLL_GPU_DIRTY_SCALER, i)
(driver.Session.write_scaler); the CLVs stay as the traversal left them. The expected values come from the reference
build running live on the same arrays, with two restatements where the reference is known to deviate under
PLL_ATTRIB_RATE_SCALERS: the root log-likelihood (scaler_cases.root_restated; the reference reads the per-rate vector
as if it were per site, src/core_likelihood.c:197) and the ancestral states (ancestral_common.restated; the reference
ignores the per-rate counts, src/likelihood.c:711-743). test_scaler_counts_host.py pins both restatements and the tables
to the reference on the CPU.

Tolerances are the project's: compare.RTOL with |d| <= RTOL max(|v|, 1) for log-likelihoods, deriv_common.close for
derivatives, ancestral_common.assert_table for state probabilities, integer equality for scale buffers. Every test
asserts, from the arrays it wrote, that every pattern class of the count tables occurs (and occurs among the invariant
and among the variable sites where the case has invariant sites).

Invariant sites: 2^-256 is about 1e-77, so the VALUE the count of an invariant site is capped at (4 against 5 and above)
cannot be seen at 1e-10; what is seen, at order 1, is whether the invariant term is added inside the logarithm and which
count is taken.

Left out: ascertainment-bias entries under PLL_ATTRIB_RATE_SCALERS - the reference reads the [entry][rate] array as if it
were per site there (src/likelihood.c:219, :241, :376-379), so it supplies no expected value; the per-site cases are here."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest

import insertion_cases as IC
import scaler_cases as SC
from ancestral_common import assert_table, restated
from compare import RTOL
from deriv_common import close
from pllamd import api, driver, workload as W
from utree import UTree

pytestmark = pytest.mark.gpu

ALL_ATTRS = dict(SC.ATTRS, **SC.REPEATS)
CONFIGS = [(shape, attrs) for shape in SC.SHAPES for attrs in SC.ATTRS] + [(shape, attrs) for shape in SC.REPEAT_SHAPES for attrs in SC.REPEATS]
NONE = api.SCALE_BUFFER_NONE


@contextlib.contextmanager
def _open(lib, case):
    """a session with the shared eigenbasis injected (the derivative calls need one) and the full traversal done"""
    with driver.Session(lib, case) as s:
        s.inject_eigen(W.eigensystem(case.model["exch"], case.freqs[0]), case.model["rates"])
        s.update_partials()
        yield s


@contextlib.contextmanager
def _pair(amd_lib, ref_lib, case):
    with _open(amd_lib, case) as a, _open(ref_lib, case) as r:
        yield SimpleNamespace(case=case, a=a, r=r, both=(a, r))


@pytest.fixture(scope="module", params=CONFIGS, ids=lambda c: "-".join(c))
def pair(request, amd_lib, ref_lib):
    """one session per library for a shape x attribute word, shared by the tests below: each of them writes every scale
    buffer it reads, so none depends on what another left behind"""
    shape, attrs = request.param
    with _pair(amd_lib, ref_lib, SC.make(shape, ALL_ATTRS[attrs])) as ns:
        ns.shape, ns.attrs = shape, attrs
        yield ns


def _ends(edge):
    return ((edge[0], edge[1]), (edge[2], edge[3]))


def _edges(case):
    """the inner-inner root edge and a tip edge, each in both orientations"""
    return [SC.root_edge(case), SC.flip(SC.root_edge(case)), SC.tip_edge(case), SC.flip(SC.tip_edge(case))]


def _write_node(ns, clv, scaler, second=False, on=True):
    """the count table of one end (or zeros) into its scaler, in both libraries; -> the array as written. The pattern
    classes are asserted on the table itself, among the invariant and the variable sites where the case has both"""
    counts = SC.counts_for(ns.r, ns.case, clv, second=second)
    real = len(counts) - (ns.case.states if ns.case.asc_alloc else 0)
    SC.assert_covered(counts[:real], what=(clv, "second end" if second else "first end"))
    if ns.case.prop_invar.max() > 0:
        inv = SC.invariant_sites(ns.r)
        SC.assert_covered(counts[:real], among=inv, what=(clv, "invariant sites"))
        SC.assert_covered(counts[:real], among=~inv, what=(clv, "variable sites"))
    if not on:
        counts = np.zeros_like(counts)
    for s in ns.both:
        SC.write_scaler(s, scaler, clv, counts)
    return counts


def _write_ends(ns, edge, parent=True, child=True):
    """_write_node for either end of the edge; None for an end without a scaler. The second end's table starts three
    places further on in the cycle"""
    return [_write_node(ns, clv, scaler, bool(second), on) if scaler >= 0 else None
            for second, ((clv, scaler), on) in enumerate(zip(_ends(edge), (parent, child)))]


def _per_site(r, clv, counts):
    """per-entry counts of a node as per-site counts (through the class map under site repeats), without the
    ascertainment entries"""
    sid = r.lib.pll_get_site_id(r.p, clv)
    c = np.asarray(counts, dtype=np.int64)
    return c[api.as_np(sid, r.case.sites, np.uint32)] if sid else c[:r.case.sites]


def _assert_edge(ns, edge, what):
    va, pa = ns.a.edge_lnl(edge)
    vr, pr = ns.r.edge_lnl(edge)
    assert np.isfinite(vr) and np.isfinite(pr).all(), (what, "the reference's own value is not finite")
    assert IC.close(pa, pr, RTOL), (what, "per site", IC.worst(pa, pr), int(np.argmax(np.abs(pa - pr))))
    assert IC.close(va, vr, RTOL), (what, va, vr)
    total = ns.a.edge_lnl(edge, persite=False)[0]
    assert IC.close(total, vr, RTOL), (what, "without the per-site vector", total, vr)
    return pa


def _variants(edge):
    """(name, counts on the parent end, on the child end, the edge as evaluated)"""
    out = [("both", True, True, edge)]
    if edge[1] >= 0 and edge[3] >= 0:
        out += [("parent only", True, False, edge), ("child only", False, True, edge)]
    if edge[1] >= 0:
        out.append(("parent end without a scaler", True, True, (edge[0], NONE, edge[2], edge[3], edge[4])))
    if edge[3] >= 0:
        out.append(("child end without a scaler", True, True, (edge[0], edge[1], edge[2], NONE, edge[4])))
    return out


def _check_edges(ns):
    case = ns.case
    w = np.asarray(case.pattern_weights, dtype=np.float64)
    for edge in _edges(case):
        _write_ends(ns, edge, False, False)
        before = _assert_edge(ns, edge, (edge, "no counts"))
        for name, on_p, on_c, used in _variants(edge):
            cp, cc = _write_ends(ns, edge, on_p, on_c)
            after = _assert_edge(ns, used, (edge, name))
            if not SC.per_rate(case) and case.prop_invar.max() == 0 and not case.asc_type:
                # exact, and independent of the reference: the counts of the ends that were passed, per site
                total = np.zeros(case.sites)
                for (clv, scaler), counts in zip(_ends(used), (cp, cc)):
                    if scaler >= 0:
                        total += _per_site(ns.r, clv, counts)
                assert total.any() or name != "both"
                assert IC.close(after - before, w * total * SC.LOG_THRESHOLD, RTOL), (edge, name, "the shift by the written counts")


# ---- a. the upload round trip ------------------------------------------------------------------------------------------
def test_written_counts_survive_sync_and_evaluation(pair):
    case, a = pair.case, pair.a
    if case.attributes & api.SITE_REPEATS:
        e = SC.root_edge(case)
        assert a.entries(e[0]) < case.sites and a.entries(e[2]) < case.sites, "the evaluated nodes are not class-compressed"
        assert (a.entries(e[0]), a.entries(e[2])) == (pair.r.entries(e[0]), pair.r.entries(e[2]))
    for edge in (SC.root_edge(case), SC.tip_edge(case)):
        written = _write_ends(pair, edge)
        for (clv, scaler), counts in zip(_ends(edge), written):
            if scaler >= 0:  # pll_gpu_sync_scaler must not bring the device's older copy back
                assert np.array_equal(a.read_scaler(scaler, clv, expand=False), counts.reshape(len(counts), -1)), (edge, clv, "after sync")
        assert np.isfinite(a.edge_lnl(edge)[0])
        assert np.isfinite(a.root_lnl((edge[0], edge[1]))[0])
        for (clv, scaler), counts in zip(_ends(edge), written):
            if scaler >= 0:
                assert np.array_equal(a.read_scaler(scaler, clv, expand=False), counts.reshape(len(counts), -1)), (edge, clv, "after the evaluation")


# ---- b. edge log-likelihood ----------------------------------------------------------------------------------------------
def test_edge_loglikelihood(pair):
    _check_edges(pair)


def _route_run(lib, case):
    """full traversal; counts into the scalers of the inner children of the two top ops; those two ops again and the
    root edge evaluated DIRECTLY - the ends are then formed inside the evaluation's own launch where the library holds
    them back - once for the total and, after the two ops once more, for the per-site values"""
    _, top = SC.top_ops(case)
    with driver.Session(lib, case) as s:
        s.update_partials()
        written = {}
        for op in top:
            for second, (clv, scaler) in enumerate(((op[2], op[4]), (op[5], op[7]))):
                assert scaler >= 0 and clv >= case.tips
                written[scaler] = SC.counts_for(s, case, clv, second=bool(second))
                SC.assert_covered(written[scaler], what=("route", clv))
                SC.write_scaler(s, scaler, clv, written[scaler])
        arr = api.make_ops(top)
        lib.pll_update_partials(s.p, arr, len(top))
        launches = lib.pll_gpu_last_launch_count(s.p) if lib.is_amd else None  # of the call that may hold its ops back
        total = s.edge_lnl(SC.root_edge(case), persite=False)[0]
        lib.pll_update_partials(s.p, arr, len(top))
        again, persite = s.edge_lnl(SC.root_edge(case))
        ends = [s.read_scaler(op[1], op[0], expand=False) for op in top]
    return total, again, persite, ends, launches


@pytest.mark.parametrize("attrs", list(ALL_ATTRS))
def test_edge_loglikelihood_when_the_ends_are_formed_inside_the_evaluation(amd_lib, ref_lib, monkeypatch, attrs):
    """4 states x 4 rates: pll_update_partials holds the last ops back for the evaluation that follows (chain and tail
    forms of k_edge_dna); PLL_AMD_NO_TAIL_FUSION=1 launches them on their own. Bit-identical, and the reference's.
    That the two routes ARE two is asserted from the launch count of the call with the two top ops: fewer where they are
    held (ops that gather through class maps never are: hold_tail) than with the switch"""
    case = SC.make("dna", ALL_ATTRS[attrs])
    exp = _route_run(ref_lib, case)
    held = _route_run(amd_lib, case)
    monkeypatch.setenv("PLL_AMD_NO_TAIL_FUSION", "1")
    plain = _route_run(amd_lib, case)
    assert exp[3][0].any() and exp[3][1].any()
    for got, route in ((held, "held"), (plain, "PLL_AMD_NO_TAIL_FUSION=1")):
        assert IC.close(got[0], exp[0], RTOL) and IC.close(got[1], exp[1], RTOL), (route, got[0], got[1], exp[0])
        assert IC.close(got[2], exp[2], RTOL), (route, IC.worst(got[2], exp[2]))
        for g, e in zip(got[3], exp[3]):
            assert np.array_equal(g, e), (route, "the scale buffers of the two ends")
    assert held[0] == plain[0] and held[1] == plain[1] and held[2].tobytes() == plain[2].tobytes()
    assert plain[4] > 0, plain[4]
    if not (case.attributes & api.SITE_REPEATS):
        assert held[4] < plain[4], ("nothing of the two top ops was held back", held[4], plain[4])


# ---- c. root log-likelihood ----------------------------------------------------------------------------------------------
def _check_roots(ns):
    case = ns.case
    e = SC.root_edge(case)
    for second, (clv, scaler) in enumerate(_ends(e)):
        for on in (False, True):
            counts = _write_node(ns, clv, scaler, bool(second), on)
            va, pa = ns.a.root_lnl((clv, scaler))
            if SC.per_rate(case):
                vr, pr = SC.root_restated(ns.r, clv, counts, per_rate_counts=True)
            else:
                vr, pr = ns.r.root_lnl((clv, scaler))
            assert np.isfinite(vr)
            assert IC.close(pa, pr, RTOL), (clv, on, "per site", IC.worst(pa, pr))
            assert IC.close(va, vr, RTOL), (clv, on, va, vr)
            assert IC.close(ns.a.root_lnl((clv, scaler), persite=False)[0], vr, RTOL), (clv, on)


def test_root_loglikelihood(pair):
    _check_roots(pair)


# ---- d. invariant sites --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs", list(SC.ATTRS))
@pytest.mark.parametrize("shape", SC.PINV_SHAPES)
def test_invariant_sites(amd_lib, ref_lib, shape, attrs):
    """a scaled site that is also an invariant site (the terminv > 0 branch of finish_site): edge and root values"""
    case = SC.make(shape, SC.ATTRS[attrs], pinv=0.3)
    with _pair(amd_lib, ref_lib, case) as ns:
        inv = SC.invariant_sites(ns.r)
        assert inv.any() and not inv.all()
        _check_edges(ns)
        _check_roots(ns)


# ---- e. traversal propagation --------------------------------------------------------------------------------------------
def _propagate(s, case, zero=False):
    """counts into the scalers of the cherry parents, then every op above them -> ({parent: its scale buffer}, lnL)"""
    cherries = SC.cherry_parents(case)
    upper = [op for op in case.op_batches[0] if (op[0], op[1]) not in cherries]
    assert len(cherries) == case.tips // 2 and len(upper) == case.tips // 2 - 2
    written = []
    for i, (clv, scaler) in enumerate(cherries):  # (a class-compressed cherry parent may hold fewer entries than the cycle has places)
        counts = SC.counts_for(s, case, clv, shift=SC.SECOND_END_SHIFT * i)
        written.append(counts)
        SC.write_scaler(s, scaler, clv, np.zeros_like(counts) if zero else counts)
    SC.assert_covered(np.concatenate(written), what="the cherry parents together")
    s.lib.pll_update_partials(s.p, api.make_ops(upper), len(upper))
    lnl = s.edge_lnl(SC.root_edge(case), persite=False)[0]
    return {op[0]: s.read_scaler(op[1], op[0], expand=False) for op in upper}, lnl


def _assert_propagated(got, exp, what):
    for node, e in exp[0].items():
        assert e.any(), (what, node, "the reference's parent carries no counts: the case shows nothing")
        assert np.array_equal(got[0][node], e), (what, node, np.argwhere(got[0][node] != e)[:5])
    assert IC.close(got[1], exp[1], RTOL), (what, got[1], exp[1])


def test_counts_propagate_through_the_traversal(pair, amd_lib, monkeypatch):
    """every parent above the cherries adds its children's counts (through the class maps under site repeats): integer
    equality with the reference, on the default route and with one launch per level (PLL_AMD_NO_FUSE=1)"""
    case = pair.case
    try:
        exp = _propagate(pair.r, case)
        _assert_propagated(_propagate(pair.a, case), exp, "default route")
        monkeypatch.setenv("PLL_AMD_NO_FUSE", "1")
        with driver.Session(amd_lib, case) as s:
            s.update_partials()
            _assert_propagated(_propagate(s, case), exp, "PLL_AMD_NO_FUSE=1")
    finally:
        for s in pair.both:
            _propagate(s, case, zero=True)


# ---- f. derivatives ------------------------------------------------------------------------------------------------------
def _derivatives(s, edge):
    st = s.new_sumtable()
    s.update_sumtable(edge[:4], st)
    return st, [s.derivatives(edge[:4], st, t) for t in SC.BRLENS]


def _check_derivatives(ns, edges):
    case = ns.case
    for edge in edges:
        _write_ends(ns, edge, False, False)
        _, plain = _derivatives(ns.a, edge)
        _, plain_ref = _derivatives(ns.r, edge)
        written = _write_ends(ns, edge)
        assert any(c is not None and c.any() for c in written)
        _, got = _derivatives(ns.a, edge)
        _, exp = _derivatives(ns.r, edge)
        for t, g, e in zip(SC.BRLENS, got, exp):
            assert close(g[0], e[0], sites=case.sites) and close(g[1], e[1], sites=case.sites), (edge, t, g, e)
        if SC.per_rate(case):  # the counts enter through the sumtable (k_sumtable_excess)
            assert all(g != p for g, p in zip(got, plain)) and all(e != p for e, p in zip(exp, plain_ref)), (edge, "the counts change nothing")
        elif not case.asc_type:  # per-site counts cancel in L'/L, and the invariant term does not see them either
            assert got == plain, (edge, got, plain)


def test_derivatives(pair):
    e = SC.root_edge(pair.case)
    _check_derivatives(pair, [e, SC.flip(e), SC.tip_edge(pair.case)])


def test_optimize_branch_length_with_per_rate_counts(amd_lib, ref_lib):
    """pll_gpu_optimize_branch_length on a sumtable built over written per-rate counts: the trace rows are the per-call
    derivatives bit for bit, and the reference's within deriv_common.close. The tip edge, as in test_gpu_newton.py: its
    iterates stay where every site's term is O(1), which is what the absolute floor of `close` (4e-15 per site) stands
    for. (Across the root edge the written counts move the optimum to t = 0.0106, where the sites' terms are O(1/t) and
    cancel to d_f = -9.2e-4: there the reference's own kernels differ by 4e-12 - ARCH_CPU -9.245923134746e-4 against
    ARCH_AVX2 -9.245923094800e-4 - seven times that floor, so the point says nothing about a third implementation.)"""
    case = SC.make("dna", api.RATE_SCALERS)
    with _pair(amd_lib, ref_lib, case) as ns:
        edge = SC.tip_edge(case)
        _write_ends(ns, edge)
        st, _ = _derivatives(ns.a, edge)
        rst, _ = _derivatives(ns.r, edge)
        res, trace = ns.a.optimize_branch(edge[:4], st, 0.1, 1e-6, 100.0, 1e-8 * case.sites)
        assert res.iterations == len(trace) >= 2
        for t, d, dd in trace:
            assert ns.a.derivatives(edge[:4], st, t) == (d, dd), (edge, t)
            e1, e2 = ns.r.derivatives(edge[:4], rst, t)
            assert close(d, e1, sites=case.sites) and close(dd, e2, sites=case.sites), (edge, t, d, e1, dd, e2)


# ---- g. ancestral states -------------------------------------------------------------------------------------------------
def test_ancestral_states(pair):
    case = pair.case
    if case.attributes & api.SITE_REPEATS:
        return  # refused by both libraries (test_gpu_ancestral.py::test_error_paths)
    fi = np.ascontiguousarray(case.freqs_indices, dtype=np.uint32)
    for edge in _edges(case):
        if (case.attributes & api.PATTERN_TIP) and edge[0] < case.tips:
            continue  # the node's end has no CLV
        _write_ends(pair, edge, False, False)
        plain = pair.a.node_ancestral(edge)
        assert_table(plain, pair.r.node_ancestral(edge), (edge, "no counts"))
        _write_ends(pair, edge)
        got = pair.a.node_ancestral(edge)
        if SC.per_rate(case):
            assert_table(got, restated(pair.r.lib, pair.r.p, edge, fi), (edge, "per-rate counts: against the restatement"))
            if edge[0] >= case.tips:  # (a tip's own row is its indicator whatever the other end's counts are)
                assert not np.array_equal(got, plain), (edge, "the counts change nothing")
        else:  # the counts cancel in the ratio
            assert np.array_equal(got, plain), edge
            assert_table(got, pair.r.node_ancestral(edge), edge)


# ---- h. insertion --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attrs", ["plain", "tip", "rs"])
@pytest.mark.parametrize("shape", ["dna", "aa"])
def test_insertion_loglikelihoods(amd_lib, ref_lib, shape, attrs):
    """written counts in both ends of every candidate and in the inserted end (a cherry of the two extra tips): the
    batched call and the library's own per-edge path against the reference's per-edge path"""
    states, rates, sites = SC.SHAPES[shape]
    lay = IC.Layout(UTree(8, np.random.Generator(np.random.PCG64(7))), 2)
    seqs, cmap, exch, freqs = IC.alignment(states, 8 + 2, sites)
    per = rates if SC.ATTRS[attrs] & api.RATE_SCALERS else None
    out = {}
    for lib in (ref_lib, amd_lib):
        with IC.Bed(lib, lay, states, sites, rates, SC.ATTRS[attrs], seqs, cmap, exch, freqs) as b:
            sub = b.query_cherry(lay.T, lay.T + 1)
            rows = b.prepare()
            slots = sorted({r[1] for r in rows if r[1] >= 0} | {r[4] for r in rows if r[4] >= 0} | {sub[1]})
            assert len(slots) >= 2 * lay.T - 4 and lay.tmp[1] not in slots
            for slot in slots:
                counts = SC.table(sites, per, shift=slot)
                SC.assert_covered(counts, what=("slot", slot))
                b.write_scaler(slot, counts)
            out[lib.is_amd] = (b.batched(sub, rows) if lib.is_amd else None, b.per_edge(sub, rows))
    exp = out[False][1]
    assert np.isfinite(exp).all() and len(exp) == 2 * lay.T - 3
    assert IC.close(out[True][0], exp, RTOL), ("batched", IC.worst(out[True][0], exp))
    assert IC.close(out[True][1], exp, RTOL), ("per edge", IC.worst(out[True][1], exp))


# ---- i. ascertainment entries --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("asc_type", [1, 2, 3], ids=["lewis", "felsenstein", "stamatakis"])
def test_ascertainment_entries(amd_lib, ref_lib, asc_type):
    """per-site scalers, counts on all sites + states entries, the four entries behind the sites carrying (0, 2, 5, 1)"""
    case = SC.make("dna", 0, asc_type=asc_type)
    with _pair(amd_lib, ref_lib, case) as ns:
        e = SC.root_edge(case)
        cp, cc = _write_ends(ns, e)
        assert tuple(cp[case.sites:]) == SC.ASC_EXTRA and tuple(cc[case.sites:]) == SC.ASC_EXTRA and len(cp) == case.sites + 4
        _check_edges(ns)
        _check_roots(ns)
        if asc_type in (1, 3):
            _check_derivatives(ns, [e, SC.flip(e), SC.tip_edge(case)])
        if asc_type == 3:  # the other two types are refused by pll_gpu_optimize_branch_length
            edge = SC.tip_edge(case)
            _write_ends(ns, edge)
            st, _ = _derivatives(ns.a, edge)
            rst, _ = _derivatives(ns.r, edge)
            res, trace = ns.a.optimize_branch(edge[:4], st, 0.1, 1e-6, 100.0, 1e-8 * case.sites)
            assert res.iterations == len(trace) >= 1
            for t, d, dd in trace:
                assert ns.a.derivatives(edge[:4], st, t) == (d, dd), t
                e1, e2 = ns.r.derivatives(edge[:4], rst, t)
                assert close(d, e1, sites=case.sites) and close(dd, e2, sites=case.sites), (t, d, e1, dd, e2)
