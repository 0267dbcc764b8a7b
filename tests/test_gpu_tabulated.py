"""GPU tests of the tabulated distribution (RIMPHONY_TABULATED = 4): every coefficient, normalisation and calc_f value
carries the bits of the table oracle (tests/support/liboracle_tab.so), whatever the batch size and whoever evaluates a
request; so does every seam below the coefficients (integrand, gamma integral, n integral, derivative probe, gamma
contribution, the Faraday elements and outer integrands), on every table geometry from 8 to 65536 nodes and on hostile
rows; misuse is refused as include/rimphony_hip.h says.  (What the oracle's spline, f and normalisation are held to:
test_tabulated_reference.py.)  Every test runs under a time limit of its own: a launch that does not end takes the
process down instead of holding the device.  The oracle's side of a comparison is computed BEFORE the launch, so that a
reference that does not end shows on the CPU."""
import contextlib
import ctypes
import faulthandler
import math
import os
import sys

import numpy as np
import pytest

import tab_bind
from rimphony_amd import workload
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs

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


# ---- the seams below the coefficients, kind 4 --------------------------------------------------------------------------
EDGE_LO, EDGE_HI = 1.01, 1e4


def install_edge(ctx, n_nodes):
    """the three-table set of tab_bind.edge_tables over [1.01, 1e4] in the context and in the oracle"""
    t = tab_bind.edge_tables(EDGE_LO, EDGE_HI, n_nodes)
    assert tab_bind.set_tables(EDGE_LO, EDGE_HI, t) == 0
    ctx.set_tables(EDGE_LO, EDGE_HI, t)
    return t


def mismatch(name, got, ref, extra=None):
    ok = same_bits(got, ref)
    if not ok.all():
        i = int(np.flatnonzero(~ok.ravel())[0])
        pytest.fail("%s: %d of %d differ; first at %d: got %r, oracle %r%s" % (
            name, (~ok).sum(), ok.size, i, np.ravel(got)[i], np.ravel(ref)[i], "" if extra is None else " | " + str(extra(i))))


def oracle_dist(table):
    d, st = tab_bind.mkdist(table)
    assert st == 0 and np.isfinite(d.norm)
    return d


def test_gamma_integrand_seam(gpu_ctx):
    """integrand_kernel_n<4>: 1000 (n, gamma) inside the kinematic range per trial, one trial per table of the 64-node set,
    with (s, theta) chosen so that the samples lie on both sides of gamma_hi (theta = 0.3: gamma+ reaches 1e5) and of
    gamma_lo (theta = 1.5: the harmonics next to the first have gamma below 1.01): outside the table the integrand is
    the oracle's exact 0 (or its NaN)."""
    L = tab_bind.load()
    rng = np.random.default_rng(404)
    below = above = 0
    with time_limit(120):
        install_edge(gpu_ctx, 64)
        for table, s, th, coeff, stokes in ((0, 100.0, 0.3, 0, 0), (1, 100.0, 1.5, 1, 1), (2, 100.0, 0.3, 0, 2)):
            d = oracle_dist(table)
            n, g = harmonic_samples(rng, s, th, 1000)
            below += int((g < EDGE_LO).sum())
            above += int((g > EDGE_HI).sum())
            ref = np.array([L.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
            assert (np.isfinite(ref) & (ref != 0)).sum() >= len(ref) // 2
            outside = ref[(g < EDGE_LO) | (g > EDGE_HI)]
            assert ((outside == 0) | np.isnan(outside)).all()
            got = gpu_ctx.gamma_integrand_batch(TAB, [float(table)], coeff, stokes, s, th, n, g)
            mismatch("gamma_integrand table %d" % table, got, ref, lambda i: (s, th, coeff, stokes, n[i], g[i]))
    assert below >= 10 and above >= 10, (below, above)


SYM_POINTS = ((0, 30.0, 0.9), (1, 200.0, 0.6), (2, 12.0, 1.2))      # (table, s, theta)
SYM_COMBOS = ((0, 0, 0), (1, 1, 0), (0, 2, 1))                      # (coeff, stokes, negative lobe)


@pytest.mark.parametrize("n_nodes", [64, 65536])
def test_gamma_integral_seam(gpu_ctx, n_nodes):
    """gamma_integral_kernel<4>: the first 16 harmonics and 32 further out, per table; also on the 65536-node set."""
    L = tab_bind.load()
    rng = np.random.default_rng(405)
    with time_limit(120):
        install_edge(gpu_ctx, n_nodes)
        for (table, s, th), (coeff, stokes, lobe) in zip(SYM_POINTS, SYM_COMBOS):
            d = oracle_dist(table)
            nmin = s * abs(math.sin(th))
            n = np.concatenate([np.floor(nmin + 1) + np.arange(16), nmin + 17 + np.exp(rng.uniform(0, 10, 32))])
            ref = np.array([L.rimo_gamma_integral(d, coeff, stokes, lobe, s, th, v) for v in n])
            assert (np.isfinite(ref) & (ref != 0)).sum() > len(n) // 2
            got = gpu_ctx.gamma_integral_batch(TAB, [float(table)], coeff, stokes, lobe, s, th, n)
            mismatch("gamma_integral table %d" % table, got, ref, lambda i: (s, th, n[i], lobe))


def test_n_integral_seam(gpu_ctx):
    """n_integral_kernel<4>: the outer QAG over n on 32 ranges [n_lo, n_hi] per table."""
    rng = np.random.default_rng(406)
    with time_limit(120):
        install_edge(gpu_ctx, 64)
        for (table, s, th), (coeff, stokes, lobe) in zip(SYM_POINTS, SYM_COMBOS):
            d = oracle_dist(table)
            lo = s * math.sin(th) + 31. + rng.uniform(0., 50., 32)
            hi = lo * rng.uniform(1.05, 3., 32)
            ref = np.array([tab_bind.n_integral(d, coeff, stokes, lobe, s, th, a, b) for a, b in zip(lo, hi)])
            assert np.isfinite(ref).sum() > 16
            got = gpu_ctx.n_integral_batch(TAB, [float(table)], coeff, stokes, lobe, s, th, lo, hi)
            mismatch("n_integral table %d" % table, got, ref, lambda i: (coeff, stokes, lo[i], hi[i]))


def test_deriv_probe_seam(gpu_ctx):
    """deriv_probe_kernel<4>: gsl::deriv_central of the gamma integral at 32 starts per table, integer ones near the first
    harmonics and fractional ones in the tail."""
    L = tab_bind.load()
    rng = np.random.default_rng(407)
    with time_limit(120):
        install_edge(gpu_ctx, 64)
        for (table, s, th), (coeff, stokes, lobe) in zip(SYM_POINTS, SYM_COMBOS):
            d = oracle_dist(table)
            n0 = np.floor(s * math.sin(th) + 31. + rng.uniform(0., 400., 32))
            n0[16:] = n0[16:] * rng.uniform(1.5, 40., 16)
            ref = np.array([L.rimo_symphony_deriv_probe(ctypes.byref(d), coeff, stokes, lobe, s, th, float(x)) for x in n0])
            assert np.isfinite(ref).sum() >= 16
            got = gpu_ctx.deriv_probe_batch(TAB, [float(table)], coeff, stokes, lobe, s, th, n0)
            mismatch("deriv_probe table %d" % table, got, ref, lambda i: (coeff, stokes, n0[i]))


def test_gamma_contribution_seam(gpu_ctx):
    """gamma_contribution_kernel<4>: the fully discrete sum (few harmonics) and the 31-discrete + QAG-over-n branch."""
    L = tab_bind.load()
    rng = np.random.default_rng(408)
    with time_limit(120):
        install_edge(gpu_ctx, 64)
        for table, s, th, glo, ghi, coeff, stokes in ((0, 8., 0.9, 1.5, 30., 0, 0), (2, 400., 0.6, 3., 40., 1, 1), (1, 400., 0.6, 3., 40., 0, 0)):
            d = oracle_dist(table)
            gam = np.exp(rng.uniform(math.log(glo), math.log(ghi), 12))
            ref = np.array([L.rimo_gamma_contribution(ctypes.byref(d), coeff, stokes, s, th, float(x)) for x in gam])
            assert np.isfinite(ref).sum() >= 6
            got = gpu_ctx.gamma_contribution_batch(TAB, [float(table)], coeff, stokes, s, th, gam)
            mismatch("gamma_contribution table %d" % table, got, ref, lambda i: (s, coeff, stokes, gam[i]))


HEY_POINTS = ((2.0, 0.9), (60.0, 1.1))        # sigma0 = s sin(theta) < 3: the J/Y branch; and the large-order branches


@pytest.mark.parametrize("table", [0, 1, 2])
def test_faraday_element_seam(gpu_ctx, table):
    """hey_element_kernel<4>: 512 (fixed, v) per (stokes, quasi-resonant or not) at both points."""
    L = tab_bind.load()
    rng = np.random.default_rng(410 + table)
    with time_limit(120):
        install_edge(gpu_ctx, 64)
        d = oracle_dist(table)
        for s, th in HEY_POINTS:
            for stokes in (1, 2):
                for qr in (0, 1):
                    fixed, v = hey_seam_inputs(rng, s, th, qr, 512)
                    ref = np.array([L.rimo_hey_element(ctypes.byref(d), stokes, s, th, qr, float(a), float(b)) for a, b in zip(fixed, v)])
                    assert np.isfinite(ref).sum() > 256
                    got = gpu_ctx.hey_element_batch(TAB, [float(table)], stokes, s, th, qr, fixed, v)
                    mismatch("hey_element table %d s %g stokes %d qr %d" % (table, s, stokes, qr), got, ref, lambda i: (fixed[i], v[i]))


@pytest.mark.parametrize("table", [0, 1, 2])
def test_faraday_outer_seam(gpu_ctx, table):
    """hey_outer_kernel<4>: 24 abscissae per (stokes, quasi-resonant or not) at both points, one inner QAG each."""
    L = tab_bind.load()
    rng = np.random.default_rng(420 + table)
    with time_limit(120):
        install_edge(gpu_ctx, 64)
        d = oracle_dist(table)
        for s, th in HEY_POINTS:
            for stokes in (1, 2):
                for qr in (0, 1):
                    u = hey_outer_abscissae(rng, s, th, qr, 24)
                    ref = np.array([L.rimo_hey_outer_integrand(ctypes.byref(d), stokes, s, th, qr, float(x)) for x in u])
                    assert np.isfinite(ref).sum() > 12
                    got = gpu_ctx.hey_outer_batch(TAB, [float(table)], stokes, s, th, qr, u)
                    mismatch("hey_outer table %d s %g stokes %d qr %d" % (table, s, stokes, qr), got, ref, lambda i: u[i])


# ---- table geometries and hostile rows, whole coefficients -------------------------------------------------------------
def check_rows(ctx, s, th, index, ref, ref_work, ref_norm):
    """All eight slots of the rows against the oracle's values and sample counts; NaN <=> ST_NONFINITE in every slot;
    ST_NORM_FAIL in every slot of exactly the rows whose normalisation is NaN (include/rimphony_hip.h)."""
    out, st, work = ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
    mismatch("coefficients", out, ref, lambda i: (s[i // 8], th[i // 8], index[i // 8], i % 8))
    assert (work.astype(np.uint64) == ref_work).all(), (work, ref_work)
    assert (((st & ST_NONFINITE) != 0) == np.isnan(out)).all()
    assert (((st & ST_NORM_FAIL) != 0) == np.isnan(ref_norm)[:, None]).all()
    return out


@pytest.mark.parametrize("n_nodes", [8, 64, 65536])
def test_node_counts(gpu_ctx, n_nodes):
    """The smallest set the library takes, a middling one and the largest, three tables each (row offsets 0, 1 and 2):
    four rows, all eight coefficients, the normalisations, and calc_f on every node (every 16th of 65536) and both ends
    of the table exactly, and on the doubles next to the ends on either side."""
    index = np.array([2.0, 0.0, 1.0, 2.0])
    s, th = np.array([1.5, 10.0, 300.0, 3000.0]), np.array([0.3, 0.8, 1.2, 1.5])
    gam = tab_bind.nodes(EDGE_LO, EDGE_HI, n_nodes)[:: 16 if n_nodes > 4096 else 1]
    gam = np.concatenate([gam, [EDGE_LO, EDGE_HI, np.nextafter(EDGE_LO, 0.), np.nextafter(EDGE_LO, 2.), np.nextafter(EDGE_HI, 0.),
                                np.nextafter(EDGE_HI, np.inf)]])
    with time_limit(180):
        install_edge(gpu_ctx, n_nodes)
        ref, ref_work = tab_bind.batch(s, th, index, nthreads=16)
        ref_norm = tab_bind.batch_norm(np.array([0.0, 1.0, 2.0]))
        assert np.isfinite(ref).all() and np.isfinite(ref_norm).all()          # nothing passes as NaN == NaN
        ref_f = [tab_bind.dev_calc_f(TAB, [float(k)], ref_norm[k], gam) for k in range(3)]
        check_rows(gpu_ctx, s, th, index, ref, ref_work, ref_norm[index.astype(int)])
        mismatch("norm", gpu_ctx.norm_batch(TAB, [np.array([0.0, 1.0, 2.0])]), ref_norm)
        for k in range(3):
            got = gpu_ctx.calc_f_batch(TAB, [float(k)], gam, np.zeros_like(gam), None)
            for name, g, w in zip(("f", "dfdg", "dfdcx"), got, ref_f[k]):
                mismatch("%s table %d" % (name, k), g, w, lambda i: gam[i])
            assert (got[0][:-4] > 0).any() and got[0][-4] == 0 and got[0][-1] == 0 and got[1][-4] == 0 and got[1][-1] == 0


_NAN, _INF = float("nan"), float("inf")
HOSTILE_S = [0.0, -1.0, _NAN, _INF, 1e-300, 1e-5, 1e8, 1e12]
HOSTILE_THETA = [0.0, -0.5, math.pi / 2, math.pi / 2 + 0.3, 3.0, math.pi, _NAN, _INF, 1e-8, 1e-3]
HOSTILE_ROWS = [(v, 0.8) for v in HOSTILE_S] + [(10.0, v) for v in HOSTILE_THETA]
HOSTILE_FINITE = [(1e8, 0.8), (10.0, math.pi / 2 + 0.3), (10.0, 3.0)]         # legitimate inputs: all eight slots finite


@pytest.mark.parametrize("row", range(len(HOSTILE_ROWS)), ids=["s=%r,theta=%.4g" % r for r in HOSTILE_ROWS])
def test_hostile_s_and_theta(gpu_ctx, row):
    """What test_gpu_parity.py::test_hostile_parameter_values_terminate_and_match gives kinds 0...3: zero, negative, NaN,
    infinite and extreme s and theta, one at a time around (10, 0.8), on table 0 of the 64-node set (one row per case, so
    that a failure names its row).  The launch ends and every slot carries the oracle's bits, status and sample counts.

    theta = pi/2 exactly (cos theta = 6.1e-17) is the row that found a fault: every gamma integral of the discrete
    harmonics has gamma- = gamma+ to an ulp there and z is rounding noise (2.2e9 for n = 11), where the oracle, like the
    reference, still gets J_n(z) from the complete pkgw_bessel_j and sym_bessel_pair had no value.  Values and status
    agreed (NaN either way), the sample counts did not: 2046 / 3968 against the oracle's 1426 / 2728.  sym_eval_pair
    now evaluates a request with a NaN sample again through the complete functions."""
    s, th = np.array([HOSTILE_ROWS[row][0]]), np.array([HOSTILE_ROWS[row][1]])
    index = np.zeros(1)
    with time_limit(120):
        install_edge(gpu_ctx, 64)
        ref, ref_work = tab_bind.batch(s, th, index, nthreads=16)
        if HOSTILE_ROWS[row] in HOSTILE_FINITE:
            assert np.isfinite(ref).all()
        check_rows(gpu_ctx, s, th, index, ref, ref_work, tab_bind.batch_norm(index))


def extreme_tables():
    """8 nodes over [1, 1e3]: values of either sign up to 600 (normalisation 1e-258), a constant 700 (normalisation
    7.85e-309, a subnormal the device must not flush), a constant -800 (the integral of n underflows to 0: normalisation
    inf, every coefficient NaN) and a step from 0 to -50 between nodes 3 and 4."""
    j = np.arange(8)
    return np.stack([600. * np.cos(j), np.full(8, 700.), np.full(8, -800.), np.where(j < 4, 0., -50.)])


def test_extreme_tables(gpu_ctx):
    t = extreme_tables()
    index = np.arange(4, dtype=np.float64)
    s, th = np.full(4, 10.0), np.full(4, 0.8)
    with time_limit(180):
        assert tab_bind.set_tables(1.0, 1e3, t) == 0
        gpu_ctx.set_tables(1.0, 1e3, t)
        ref_norm = tab_bind.batch_norm(index)
        ref, ref_work = tab_bind.batch(s, th, index, nthreads=16)
        assert 0 < ref_norm[0] < 1e-250 and 0 < ref_norm[1] < 2.2250738585072014e-308 and ref_norm[2] == np.inf and np.isfinite(ref_norm[3])
        assert np.isfinite(ref[[0, 1, 3]]).all() and np.isnan(ref[2]).all()
        mismatch("norm", gpu_ctx.norm_batch(TAB, [index]), ref_norm)
        check_rows(gpu_ctx, s, th, index, ref, ref_work, ref_norm)
