"""CPU (no GPU): the inputs and expected values of test_gpu_scaler_counts.py are sound - against the reference build alone
(oracle/_ref/libpll_ref.so), before any device time is spent.

  * the count tables of scaler_cases.py hold every pattern class for every shape, among the invariant and among the
    variable sites where a case has invariant sites, and the site-repeats cases do evaluate class-compressed nodes;
  * the numpy restatement of the root log-likelihood (scaler_cases.root_restated) equals the reference under per-site
    scalers, with written counts, within compare.RTOL - per-rate it replaces the reference, which reads the per-rate
    vector as if it were per site (src/core_likelihood.c:197);
  * the reference, given written per-site counts, shifts every per-site log-likelihood by exactly
    -w_n (c_parent[n] + c_child[n]) 256 ln 2."""
import numpy as np
import pytest

import insertion_cases as IC
import scaler_cases as SC
from compare import RTOL
from pllamd import api, driver

ALL = [(shape, attrs) for shape in SC.SHAPES for attrs in SC.ATTRS] + [(shape, attrs) for shape in SC.REPEAT_SHAPES for attrs in SC.REPEATS]
ALL_ATTRS = dict(SC.ATTRS, **SC.REPEATS)


def test_pattern_rows_hold_what_they_claim():
    SC.assert_rows4_properties()
    for rates in (None, 3, 4, 8):
        first, second = SC.table(40, rates), SC.table(40, rates, SC.SECOND_END_SHIFT)
        SC.assert_covered(first)
        SC.assert_covered(second)
        assert not np.array_equal(first, second), "the two ends of an edge must carry different tables"


@pytest.mark.parametrize("shape,attrs", ALL, ids=lambda v: str(v))
def test_tables_cover_every_shape(ref_lib, shape, attrs):
    case = SC.make(shape, ALL_ATTRS[attrs])
    with driver.Session(ref_lib, case) as r:
        r.update_partials()
        for edge in (SC.root_edge(case), SC.tip_edge(case)):
            for second, (clv, scaler) in enumerate(((edge[0], edge[1]), (edge[2], edge[3]))):
                if scaler < 0:
                    continue
                counts = SC.counts_for(r, case, clv, second=bool(second))
                assert counts.shape[0] == r.entries(clv)
                SC.assert_covered(counts, what=(shape, attrs, clv))
        if case.attributes & api.SITE_REPEATS:
            e = SC.root_edge(case)
            assert r.entries(e[0]) < case.sites and r.entries(e[2]) < case.sites, "the evaluated nodes are not class-compressed"


@pytest.mark.parametrize("shape", SC.PINV_SHAPES)
@pytest.mark.parametrize("attrs", ["plain", "rs"])
def test_tables_cover_invariant_and_variable_sites(ref_lib, shape, attrs):
    case = SC.make(shape, SC.ATTRS[attrs], pinv=0.3)
    with driver.Session(ref_lib, case) as r:
        r.update_partials()
        inv = SC.invariant_sites(r)
        assert inv.any() and not inv.all()
        e = SC.root_edge(case)
        for second, clv in enumerate((e[0], e[2])):
            counts = SC.counts_for(r, case, clv, second=bool(second))
            SC.assert_covered(counts, among=inv, what=(shape, attrs, "invariant sites"))
            SC.assert_covered(counts, among=~inv, what=(shape, attrs, "variable sites"))


@pytest.mark.parametrize("shape,pinv", [(s, 0.0) for s in SC.SHAPES] + [(s, 0.3) for s in SC.PINV_SHAPES], ids=lambda v: str(v))
def test_root_restatement_equals_the_reference_per_site(ref_lib, shape, pinv):
    case = SC.make(shape, 0, pinv=pinv)
    with driver.Session(ref_lib, case) as r:
        r.update_partials()
        e = SC.root_edge(case)
        for counts in (np.zeros(case.sites, dtype=np.uint32), SC.counts_for(r, case, e[0])):
            SC.write_scaler(r, e[1], e[0], counts)
            exp, exp_site = r.root_lnl((e[0], e[1]))
            got, got_site = SC.root_restated(r, e[0], counts, per_rate_counts=False)
            assert IC.close(got_site, exp_site, RTOL), (shape, IC.worst(got_site, exp_site))
            assert IC.close(got, exp, RTOL), (shape, got, exp)


@pytest.mark.parametrize("shape,pinv", [(s, 0.0) for s in SC.SHAPES] + [(s, 0.3) for s in SC.PINV_SHAPES], ids=lambda v: str(v))
def test_root_restatement_per_rate_with_equal_counts_is_the_per_site_value(ref_lib, shape, pinv):
    """per-rate counts that are the same in every category of a site are per-site counts: the restatement fed with them
    (per_rate_counts=True, on a RATE_SCALERS partition) gives what the reference gives for a per-site partition"""
    plain, rs = SC.make(shape, 0, pinv=pinv), SC.make(shape, api.RATE_SCALERS, pinv=pinv)
    with driver.Session(ref_lib, plain) as r, driver.Session(ref_lib, rs) as q:
        r.update_partials()
        q.update_partials()
        e = SC.root_edge(plain)
        counts = SC.counts_for(r, plain, e[0])
        SC.write_scaler(r, e[1], e[0], counts)
        exp, exp_site = r.root_lnl((e[0], e[1]))
        wide = np.repeat(counts[:, None], rs.rate_cats, axis=1)
        SC.write_scaler(q, e[1], e[0], wide)
        got, got_site = SC.root_restated(q, e[0], wide, per_rate_counts=True)
        assert IC.close(got_site, exp_site, RTOL) and IC.close(got, exp, RTOL), (shape, got, exp)


@pytest.mark.parametrize("attrs", ["plain", "tip"])
@pytest.mark.parametrize("shape", list(SC.SHAPES))
def test_reference_shifts_per_site_values_by_the_written_counts(ref_lib, shape, attrs):
    case = SC.make(shape, SC.ATTRS[attrs])
    w = np.asarray(case.pattern_weights, dtype=np.float64)
    with driver.Session(ref_lib, case) as r:
        r.update_partials()
        for edge in (SC.root_edge(case), SC.flip(SC.root_edge(case)), SC.tip_edge(case)):
            before = r.edge_lnl(edge)[1]
            total = np.zeros(case.sites)
            saved = {}
            for second, (clv, scaler) in enumerate(((edge[0], edge[1]), (edge[2], edge[3]))):
                if scaler < 0:
                    continue
                saved[scaler] = (clv, r.read_scaler(scaler, clv, expand=False))
                counts = SC.counts_for(r, case, clv, second=bool(second))
                SC.write_scaler(r, scaler, clv, counts)
                total += counts
            assert total.any()
            after = r.edge_lnl(edge)[1]
            assert IC.close(after - before, w * total * SC.LOG_THRESHOLD, RTOL), (shape, attrs, edge)
            for scaler, (clv, old) in saved.items():
                SC.write_scaler(r, scaler, clv, old)
