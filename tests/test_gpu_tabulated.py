"""GPU tests of the tabulated distribution (RIMPHONY_TABULATED = 4): every coefficient, normalisation and calc_f value
carries the bits of the table oracle (tests/support/liboracle_tab.so), whatever the batch size and whoever evaluates a
request; misuse is refused as include/rimphony_hip.h says.  Every test runs under a time limit of its own: a launch that
does not end takes the process down instead of holding the device."""
import contextlib
import faulthandler
import os
import sys

import numpy as np
import pytest

import tab_bind
from rimphony_amd import workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_det.npz")
ST_NONFINITE, ST_NORM_FAIL = 16, 32
TAB = 4


@contextlib.contextmanager
def time_limit(seconds):
    """Ends the process (with a traceback of every thread) if the body -- GPU work that may block inside the runtime,
    where no Python exception can reach -- is still running after `seconds`."""
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def fix():
    return np.load(FIXTURE)


def install(ctx, fix):
    ctx.set_tables(float(fix["gamma_lo"]), float(fix["gamma_hi"]), fix["tables"])
    assert tab_bind.set_tables(float(fix["gamma_lo"]), float(fix["gamma_hi"]), fix["tables"]) == 0


def env_context(**env):
    """A context created with the given environment (the knobs are read when a context is created)."""
    from rimphony_amd import api
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def check_status(out, st):
    assert (((st & ST_NONFINITE) != 0) == np.isnan(out)).all()
    assert ((st & ST_NORM_FAIL) == 0).all()


def test_fixture_rows_bit_identical(gpu_ctx, fix):
    """All 8 slots of the committed rows: values (NaN pattern included), status and per-coefficient sample counts."""
    with time_limit(600):
        install(gpu_ctx, fix)
        out, st, work = gpu_ctx.compute_batch(TAB, fix["s"], fix["theta"], [fix["index"]], 0xFF, want_status=True, want_work=True)
    print("rows", len(out), "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    assert len(out) >= 256
    assert np.isfinite(fix["values"]).any(axis=0).all()
    assert same_bits(out, fix["values"]).all()
    assert (work.astype(np.uint64) == fix["work"]).all()
    check_status(out, st)


def test_further_rows_against_live_oracle(gpu_ctx, fix):
    with time_limit(600):
        install(gpu_ctx, fix)
        _, _, s, th, _ = workload.make_batch("cfg3_thermal_8", 24, start=8100000)
        index = ((np.arange(24) // 3) % 2).astype(np.float64)
        out, st, work = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
    ref, ref_work = tab_bind.batch(s, th, index)
    assert same_bits(out, ref).all()
    assert (work.astype(np.uint64) == ref_work).all()
    check_status(out, st)


def test_norm_and_calc_f_bit_identical(gpu_ctx, fix):
    with time_limit(300):
        install(gpu_ctx, fix)
        index = np.array([0.0, 1.0, 1.0, 0.0, 2.0, 0.5, -1.0, np.nan])
        norm = gpu_ctx.norm_batch(TAB, [index])
        ref = tab_bind.batch_norm(index)
        assert same_bits(norm, ref).all()
        assert np.isfinite(norm[:4]).all() and np.isnan(norm[4:]).all()
        rng = np.random.default_rng(11)
        lo, hi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
        gamma = np.concatenate([np.exp(rng.uniform(np.log(lo), np.log(hi), 5000)), [lo, hi, 0.5 * lo, 2 * hi, np.nan]])
        cx = rng.uniform(-1, 1, len(gamma))
        for table in (0.0, 1.0):
            for nrm in (1.0, None):
                got = gpu_ctx.calc_f_batch(TAB, [table], gamma, cx, nrm)
                want = tab_bind.dev_calc_f(TAB, [table], ref[int(table)] if nrm is None else nrm, gamma, cx)
                for g, w in zip(got, want):
                    assert same_bits(g, w).all()
        assert (got[0][-3:-1] == 0).all() and (got[1][-3:-1] == 0).all() and (got[2] == 0).all()


def test_batch_size_and_cooperative_tail_change_no_bit(gpu_ctx, fix):
    """Two launches of different n, and a context without the cooperative tail (RIMPHONY_NO_ASSIST=1): same bits, same
    status words, same sample counts."""
    n_small = 40
    with time_limit(600):
        install(gpu_ctx, fix)
        big = gpu_ctx.compute_batch(TAB, fix["s"], fix["theta"], [fix["index"]], 0xFF, want_status=True, want_work=True)
        sl = slice(100, 100 + n_small)
        small = gpu_ctx.compute_batch(TAB, fix["s"][sl], fix["theta"][sl], [fix["index"][sl]], 0xFF, want_status=True, want_work=True)
        solo_ctx = env_context(RIMPHONY_NO_ASSIST="1")
        try:
            solo_ctx.set_tables(float(fix["gamma_lo"]), float(fix["gamma_hi"]), fix["tables"])
            solo = solo_ctx.compute_batch(TAB, fix["s"][sl], fix["theta"][sl], [fix["index"][sl]], 0xFF, want_status=True, want_work=True)
        finally:
            solo_ctx.close()
    for other in (small, solo):
        assert same_bits(big[0][sl], other[0]).all()
        assert (big[1][sl] == other[1]).all()
        assert (big[2][sl] == other[2]).all()


def test_tabulated_power_law_within_one_percent_of_kind_0(gpu_ctx, fix):
    """On the committed rows of the golden file's (s, theta) list: a 2048-node table of gamma^-2.5 exp(-gamma / 1e10) over
    [1, 1e12] against the analytic kind, the reference's fixture tolerance of 1 % (tests/symphony.rs:82)."""
    gold = np.loadtxt(os.path.join(ROOT, "tests", "golden", "symphony-powerlaw.txt"))
    rows = fix["pl_rows"]
    s, th, n = gold[rows, 0].copy(), gold[rows, 1].copy(), len(rows)
    g = tab_bind.nodes(1.0, 1e12, 2048)
    with time_limit(600):
        gpu_ctx.set_tables(1.0, 1e12, tab_bind.log_n_powerlaw(g, 2.5, 1e10))
        tab = gpu_ctx.compute_batch(TAB, s, th, [np.zeros(n)], 0xFF)
        ref = gpu_ctx.compute_batch(0, s, th, [np.full(n, 2.5), np.ones(n), np.full(n, 1e12), np.full(n, 1e10)], 0xFF)
    assert np.isfinite(tab).all() and np.isfinite(ref).all()
    rel = np.abs(tab / ref - 1.0)
    print("max rel per slot", rel.max(axis=0))
    assert rel.max() < 0.01


def test_misuse(gpu_ctx, fix):
    from rimphony_amd import api, capi
    s, th = fix["s"][:6].copy(), fix["theta"][:6].copy()
    with time_limit(600):
        # no tables: EINVAL from the batch, the norm and the calc_f entries
        gpu_ctx.set_tables(1.0, 2.0, None)
        for call in (lambda: gpu_ctx.compute_batch(TAB, s, th, [np.zeros(6)], 0xFF),
                     lambda: gpu_ctx.norm_batch(TAB, [np.zeros(6)]),
                     lambda: gpu_ctx.calc_f_batch(TAB, [0.0], np.array([2.0]), np.array([0.1]), 1.0),
                     lambda: api.compute_batch_multi([gpu_ctx._get()], TAB, s, th, [np.zeros(6)], 0xFF)):
            with pytest.raises(capi.RimphonyError, match="invalid argument"):
                call()
        # a bad index: NaN and ST_NORM_FAIL on that row only
        install(gpu_ctx, fix)
        index = np.array([1.0, 2.0, 1.0, 0.5, 1.0, np.nan])
        out, st = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True)
        bad = np.array([False, True, False, True, False, True])
        assert np.isnan(out[bad]).all() and ((st[bad] & ST_NORM_FAIL) != 0).all()
        assert ((st[~bad] & ST_NORM_FAIL) == 0).all()
        good, _ = tab_bind.batch(s, th, np.ones(6))
        assert same_bits(out[~bad], good[~bad]).all() and np.isfinite(out[~bad]).any()
        # replacing the table set changes the next call's results
        first = gpu_ctx.compute_batch(TAB, s, th, [np.zeros(6)], 0x03)
        gpu_ctx.set_tables(float(fix["gamma_lo"]), float(fix["gamma_hi"]), fix["tables"][::-1].copy())
        second = gpu_ctx.compute_batch(TAB, s, th, [np.zeros(6)], 0x03)
        assert not same_bits(first[:, :2], second[:, :2]).all()
        install(gpu_ctx, fix)
        assert same_bits(gpu_ctx.compute_batch(TAB, s, th, [np.ones(6)], 0x03)[:, :2], second[:, :2]).all()
        # F32_INTEGRAND: not supported, with or without the measurement hook
        with pytest.raises(capi.RimphonyError, match="not supported"):
            gpu_ctx.compute_batch(TAB, s, th, [np.zeros(6)], 0xFF, precision=api.PRECISION_F32_INTEGRAND)
        hook = env_context(RIMPHONY_F32_VARIANT="1")
        try:
            hook.set_tables(float(fix["gamma_lo"]), float(fix["gamma_hi"]), fix["tables"])
            with pytest.raises(capi.RimphonyError, match="not supported"):
                hook.compute_batch(TAB, s, th, [np.zeros(6)], 0xFF, precision=api.PRECISION_F32_INTEGRAND)
        finally:
            hook.close()
        # the high-frequency closed forms exist for kinds 0 and 1 only
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.highfreq_batch(TAB, s, th, [np.zeros(6)])
        # compute_batch_multi with one context (each context uses its own table set)
        index = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 1.0])
        one, ost = api.compute_batch_multi([gpu_ctx._get()], TAB, s, th, [index], 0xFF, want_status=True)
        ref, rst = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True)
        assert same_bits(one, ref).all() and (ost == rst).all()


def test_routing_knobs_change_no_bit(gpu_ctx, fix):
    """RIMPHONY_FARADAY_GROUP=1 falls back to the one-wave-per-coefficient kernel for this kind, RIMPHONY_SYM_SOLO=1 selects
    the kernel it runs on anyway: same bits."""
    sl = slice(0, 16)
    with time_limit(600):
        install(gpu_ctx, fix)
        want = gpu_ctx.compute_batch(TAB, fix["s"][sl], fix["theta"][sl], [fix["index"][sl]], 0xFF, want_status=True)
        ctx = env_context(RIMPHONY_FARADAY_GROUP="1", RIMPHONY_SYM_SOLO="1")
        try:
            ctx.set_tables(float(fix["gamma_lo"]), float(fix["gamma_hi"]), fix["tables"])
            got = ctx.compute_batch(TAB, fix["s"][sl], fix["theta"][sl], [fix["index"][sl]], 0xFF, want_status=True)
        finally:
            ctx.close()
    assert same_bits(want[0], got[0]).all() and (want[1] == got[1]).all()


def test_tabulated_distribution_object(gpu_ctx, fix):
    """api.TabulatedDistribution: calc_f, calc_f_derivatives and full_calculation on its own table."""
    from rimphony_amd import api
    with time_limit(300):
        d = api.TabulatedDistribution(float(fix["gamma_lo"]), float(fix["gamma_hi"]), fix["tables"][1])
        d.ctx = gpu_ctx._get()
        d.norm = 1.0
        assert tab_bind.set_tables(d.gamma_lo, d.gamma_hi, d.log_n) == 0
        f, dfdg, _ = tab_bind.dev_calc_f(TAB, [0.0], 1.0, np.array([37.5]))
        assert d.calc_f(37.5, 0.3) == f[0]
        assert d.calc_f_derivatives(37.5, 0.3) == (dfdg[0], 0.0)
        calc = d.full_calculation(gpu_ctx._get())
        s, th = float(fix["s"][1]), float(fix["theta"][1])
        ref, _ = tab_bind.batch([s], [th], [0.0])
        assert same_bits(calc.compute_all_dimensionless(s, th), ref[0]).all()
