"""CPU (no GPU): the replicate weights of pll_gpu_draw_replicate_weights / pll_gpu_quartet_rell_loglikelihoods.

pllamd/rell.py is their definition in integer arithmetic: its generator against the published
known-answer vectors of Philox-4x32-10, its vectorised form against a draw-by-draw one in Python ints, the properties the
definition promises, and a goodness-of-fit test of one fixed seed whose bound is derived, not tuned.

Through the C API on host-only partitions (PLL_AMD_HOST_ONLY=1), as tests/test_quartet_resample_host.py does for the
existing call: both symbols are declared, exported and bound; every refusal in its documented order; a failed call leaves
lnl, resampled, persite and replicate_weights as it found them."""
import os
import re

import numpy as np
import pytest

import test_quartet_resample_host as H
from pllamd import api, rell

ROOT = H.ROOT
TIPS, INNER, SITES, MATRICES, REPLICATES, SENTINEL, GOOD = H.TIPS, H.INNER, H.SITES, H.MATRICES, H.REPLICATES, H.SENTINEL, H.GOOD
NAME = "pll_gpu_quartet_rell_loglikelihoods"
DRAW = "pll_gpu_draw_replicate_weights"
W_SENTINEL = 0xABCDEF01
SEED = 0x0123456789ABCDEF
MIXED = [1 + (7 * n) % 5 if n % 6 else 0 for n in range(40)]  # weights 1..5 and some zeros


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setenv("PLL_AMD_HOST_ONLY", "1")


# ---- the definition -------------------------------------------------------------------------------------------------
KAT = [  # Random123's kat_vectors for philox4x32-10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,out", KAT)
def test_the_generator_is_philox4x32_10(counter, key, out):
    assert tuple(int(x) for x in rell.philox4x32_10(counter, key)) == out


def test_the_constants_are_the_published_ones():
    assert (rell.M0, rell.M1, rell.W0, rell.W1) == (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)


@pytest.mark.parametrize("p", [[1] * 9, MIXED, [0, 0, 5, 0], [3]], ids=["ones", "mixed", "one_pattern", "one_site"])
def test_the_vectorised_form_is_the_draw_by_draw_one(p):
    assert rell.replicate_weights(p, SEED, 3, 4).tobytes() == rell.replicate_weights_slow(p, SEED, 3, 4).tobytes()


def test_the_high_half_product():
    rng = np.random.Generator(np.random.PCG64(5))
    for total in (1, 2, 3, 100000, 2 ** 32 - 1):
        hi, lo = rng.integers(0, 2 ** 32, 50, dtype=np.uint64), rng.integers(0, 2 ** 32, 50, dtype=np.uint64)
        hi[:2], lo[:2] = (0, 2 ** 32 - 1), (0, 2 ** 32 - 1)
        exp = [((int(h) << 32 | int(l)) * total) >> 64 for h, l in zip(hi, lo)]
        assert rell.scaled(hi, lo, total).tolist() == exp


def test_rows_add_up_and_zero_weights_stay_zero():
    w = rell.replicate_weights(MIXED, SEED, 0, 25)
    assert w.dtype == np.uint32 and w.shape == (25, len(MIXED))
    assert (w.sum(axis=1, dtype=np.uint64) == sum(MIXED)).all()
    zero = np.array(MIXED) == 0
    assert zero.any() and (w[:, zero] == 0).all() and (w[:, ~zero].sum(axis=0) > 0).all()


@pytest.mark.parametrize("p", [[1] * 70, MIXED], ids=["ones", "mixed"])
def test_a_row_depends_on_its_absolute_number_alone(p):
    long = rell.replicate_weights(p, SEED, 0, 12)
    assert rell.replicate_weights(p, SEED, 5, 4).tobytes() == long[5:9].tobytes()
    assert rell.replicate_weights(p, SEED, 11, 1).tobytes() == long[11:].tobytes()
    assert len({r.tobytes() for r in long}) == 12, "rows repeat"
    other = rell.replicate_weights(p, SEED + 1, 0, 12)
    assert all(a.tobytes() != b.tobytes() for a, b in zip(long, other)), "the seed does not show"
    high = rell.replicate_weights(p, SEED ^ (1 << 40), 0, 12)
    assert all(a.tobytes() != b.tobytes() for a, b in zip(long, high)), "the seed's high half does not show"


def test_unit_weights_take_the_general_path():
    """total == sites with every weight 1: the site is r itself - the shortcut the device takes"""
    sites = 300
    w = rell.replicate_weights([1] * sites, SEED, 2, 3)
    for k in range(3):
        hi, lo = rell.draw_words(SEED, 2 + k, sites)
        assert np.bincount(rell.scaled(hi, lo, sites).astype(np.int64), minlength=sites).tolist() == w[k].tolist()
    # ... and equal sums alone do not make the shortcut valid
    p = [2, 0] * (sites // 2)
    assert sum(p) == sites and (rell.replicate_weights(p, SEED, 2, 3)[:, 1::2] == 0).all()


def test_sums_out_of_range_are_refused():
    for p in ([0, 0, 0], [], [2 ** 31, 2 ** 31]):
        with pytest.raises(ValueError):
            rell.replicate_weights(p, SEED, 0, 1)


def test_goodness_of_fit():
    """64 patterns of weights 1 + (7 n) % 5, 200 replicates pooled: Pearson's statistic against p / total is chi-square
    with 63 degrees of freedom under the definition (mean dof, variance 2 dof); the bound is dof + 6 sqrt(2 dof)"""
    p = np.array([1 + (7 * n) % 5 for n in range(64)], dtype=np.float64)
    w = rell.replicate_weights(p.astype(np.uint32), 20261020, 0, 200)
    draws = 200 * p.sum()
    assert w.sum() == draws
    exp = draws * p / p.sum()
    stat = float((((w.sum(axis=0) - exp) ** 2) / exp).sum())
    dof = 63
    print(f"Pearson statistic {stat:.2f}, bound {dof + 6 * np.sqrt(2 * dof):.2f}")
    assert stat <= dof + 6 * np.sqrt(2 * dof)


# ---- the C API without a device -------------------------------------------------------------------------------------
class Buffers(H.Buffers):
    def __init__(self):
        super().__init__()
        self.weights = np.full((REPLICATES, SITES), W_SENTINEL, dtype=np.uint32)  # an output here

    def untouched(self):
        return super().untouched() and bool((self.weights == W_SENTINEL).all())


def _call(lib, p, b, rows=GOOD, fi=None, count=None, replicates=REPLICATES, seed=SEED, **null):
    fi = np.zeros(4, dtype=np.uint32) if fi is None else fi
    args = {"quartets": api.make_quartets(rows), "freqs_indices": api.uptr(fi), "weights": api.uptr(b.weights), "lnl": api.dptr(b.lnl),
            "resampled": api.dptr(b.resampled), "persite": api.dptr(b.persite)}
    for name in null:
        assert name in args
        args[name] = None
    return getattr(lib, NAME)(p, args["quartets"], len(rows) if count is None else count, args["freqs_indices"], seed, replicates,
                              args["lnl"], args["resampled"], args["persite"], args["weights"])


def _refused(lib, code, attrs=0, **kw):
    p = H._partition(lib, attrs)
    try:
        b = Buffers()
        assert _call(lib, p, b, **kw) == 0
        assert lib.errno() == code, (lib.errno(), lib.errmsg())
        assert b.untouched()
    finally:
        lib.pll_partition_destroy(p)


def test_symbols_declared_exported_and_bound(amd_lib):
    hdr = open(os.path.join(ROOT, "include", "pll_amd.h")).read()
    dev = open(os.path.join(ROOT, "include", "pll_amd_device.h")).read()
    for name, nargs in ((NAME, 10), (DRAW, 5)):
        assert re.search(r"\bint " + name + r"\(", hdr)
        assert getattr(amd_lib.dll, name)
        fn = getattr(amd_lib, name)
        assert fn.argtypes and len(fn.argtypes) == nargs
    for name in ("pllgpu_quartet_rell_loglikelihoods", "pllgpu_replicate_weights_draw"):
        assert re.search(r"\bint " + name + r"\(", dev) and getattr(amd_lib.dll, name)


def test_zero_count_succeeds_and_writes_nothing(amd_lib):
    p = H._partition(amd_lib)
    try:
        b = Buffers()
        assert _call(amd_lib, p, b, count=0) == 1
        assert getattr(amd_lib, NAME)(p, None, 0, None, SEED, 0, None, None, None, None) == 1
        assert getattr(amd_lib, NAME)(p, None, 0, None, SEED, REPLICATES, None, None, None, None) == 1
        assert _call(amd_lib, p, b, rows=H._with(0, 0, 0, TIPS + INNER), count=0) == 1  # nothing of the list is read
        assert b.untouched()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_null_partition(amd_lib):
    b = Buffers()
    assert _call(amd_lib, None, b) == 0
    assert amd_lib.errno() == api.ERROR_PARAM_INVALID and b.untouched()


@pytest.mark.parametrize("which", ["quartets", "freqs_indices"])
def test_null_list_arguments(amd_lib, which):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, **{which: True})


def test_replicates_need_resampled_and_not_the_weights(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, resampled=True)
    p = H._partition(amd_lib)
    try:
        b = Buffers()
        assert _call(amd_lib, p, b, resampled=True) == 0 and "resampled is NULL" in amd_lib.errmsg()
        assert _call(amd_lib, p, b, weights=True) == 0  # replicate_weights is optional: the call gets as far as the device
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE and b.untouched()
    finally:
        amd_lib.pll_partition_destroy(p)


def test_all_three_outputs_null(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, replicates=0, lnl=True, resampled=True, persite=True)
    _refused(amd_lib, api.ERROR_PARAM_INVALID, replicates=0, weights=True, lnl=True, resampled=True, persite=True)


@pytest.mark.parametrize("what", list(H.BAD))
def test_a_field_out_of_range_anywhere_in_the_list(amd_lib, what):
    row, end, field, value = H.BAD[what]
    _refused(amd_lib, api.ERROR_PARAM_INVALID, rows=H._with(row, end, field, value))


def test_freqs_indices_out_of_range(amd_lib):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, fi=np.array([0, 0, 1, 0], dtype=np.uint32))


@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_unsupported_partitions_are_refused(amd_lib, attrs):
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=attrs)
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=attrs, replicates=0, weights=True, resampled=True)


@pytest.mark.parametrize("attrs", [api.SITE_REPEATS, api.AB_FLAG | api.AB_LEWIS], ids=["site_repeats", "asc_bias"])
def test_argument_and_index_errors_come_before_a_refusal(amd_lib, attrs):
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, rows=H._with(2, 1, 0, TIPS + INNER))
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, fi=np.array([0, 0, 0, 1], dtype=np.uint32))
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, resampled=True)
    _refused(amd_lib, api.ERROR_PARAM_INVALID, attrs=attrs, replicates=0, lnl=True, resampled=True, persite=True)


def test_a_null_argument_comes_before_an_index_error(amd_lib):
    p = H._partition(amd_lib)
    try:
        b = Buffers()
        fi = np.array([0, 5, 0, 0], dtype=np.uint32)
        assert _call(amd_lib, p, b, rows=H._with(0, 0, 0, TIPS + INNER), fi=fi, resampled=True) == 0
        assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
        assert b.untouched()
    finally:
        amd_lib.pll_partition_destroy(p)


@pytest.mark.parametrize("replicates", [REPLICATES, 0])
def test_the_missing_device_comes_last(amd_lib, capfd, replicates):
    """after every refusal (host-only partitions have no device either: UNSUPPORTED first), UNAVAILABLE; outputs untouched"""
    _refused(amd_lib, api.ERROR_GPU_UNSUPPORTED, attrs=api.SITE_REPEATS, replicates=replicates)
    p = H._partition(amd_lib)
    try:
        b = Buffers()
        assert _call(amd_lib, p, b, replicates=replicates) == 0
        assert amd_lib.errno() == api.ERROR_GPU_UNAVAILABLE
        assert b.untouched()
        assert NAME in capfd.readouterr().err  # the usual line on stderr
    finally:
        amd_lib.pll_partition_destroy(p)


def test_the_call_names_itself(amd_lib):
    p = H._partition(amd_lib)
    try:
        b = Buffers()
        assert _call(amd_lib, p, b, rows=H._with(1, 2, 0, TIPS + INNER)) == 0
        assert amd_lib.errmsg() == NAME + ": quartet 1 has an index out of range"
    finally:
        amd_lib.pll_partition_destroy(p)


# ---- pll_gpu_draw_replicate_weights ---------------------------------------------------------------------------------
def _draw(lib, p, w, replicates=REPLICATES, first=0):
    return getattr(lib, DRAW)(p, SEED, first, replicates, None if w is None else api.uptr(w))


def test_draw_checks_in_their_order(amd_lib, capfd):
    w = np.full((REPLICATES, SITES), W_SENTINEL, dtype=np.uint32)
    assert _draw(amd_lib, None, w) == 0 and amd_lib.errno() == api.ERROR_PARAM_INVALID
    for attrs, code in ((0, api.ERROR_GPU_UNAVAILABLE), (api.SITE_REPEATS, api.ERROR_GPU_UNSUPPORTED),
                        (api.AB_FLAG | api.AB_LEWIS, api.ERROR_GPU_UNSUPPORTED)):
        p = H._partition(amd_lib, attrs)
        try:
            assert _draw(amd_lib, p, None, replicates=0) == 1  # no rows: nothing is checked further, nothing is launched
            assert _draw(amd_lib, p, w, replicates=0) == 1
            assert _draw(amd_lib, p, None) == 0  # NULL weights before a refusal
            assert amd_lib.errno() == api.ERROR_PARAM_INVALID and "NULL" in amd_lib.errmsg()
            capfd.readouterr()
            assert _draw(amd_lib, p, w) == 0
            assert amd_lib.errno() == code, (amd_lib.errno(), amd_lib.errmsg())
            assert DRAW in capfd.readouterr().err
        finally:
            amd_lib.pll_partition_destroy(p)
    assert (w == W_SENTINEL).all()
