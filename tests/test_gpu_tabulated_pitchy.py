"""GPU tests of the tabulated distribution with a sin^k xi prefactor per table (rimphony_ctx_set_tables_pitchy): the
coefficients, normalisations (with P integrated on the device), calc_f values and every seam carry the bits of the sin^k
table oracle (tests/support/liboracle_tabpitchy.so); scheduling changes no bit; no state survives a change of form; the
table agrees with the device's own analytic pitchy power law; misuse is refused and leaves the previous set in place.
(What the oracle is held to: test_tabulated_pitchy_host.py.)  Every test runs under a time limit of its own, and the
oracle's side of a comparison is computed before the launch."""
import contextlib
import ctypes
import faulthandler
import math
import os
import sys

import numpy as np
import pytest

import tab_bind
import tab_pitch_bind as tp
import tab_pitchy_bind as ty
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL = -1
ST_NONFINITE, ST_NORM_FAIL = 16, 32
TAB = 4
ENTRY = "rimphony_ctx_set_tables_pitchy"


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


def mismatch(name, got, ref, extra=None):
    ok = same_bits(got, ref)
    if not ok.all():
        i = int(np.flatnonzero(~ok.ravel())[0])
        pytest.fail("%s: %d of %d differ; first at %d: got %r, oracle %r%s" % (
            name, (~ok).sum(), ok.size, i, np.ravel(got)[i], np.ravel(ref)[i], "" if extra is None else " | " + str(extra(i))))


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


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "tabulated_pitchy_det.npz"))


def install(ctx, which, oracle=True):
    """set A (0) or B (1) in the context and, if asked, in the oracle"""
    lo, hi, t, g, k = ty.fixture_set(which)
    if oracle:
        assert ty.set_tables(lo, hi, t, g, k) == 0
    if ctx is not None:
        ctx.set_tables(lo, hi, t, g, sin_k=k)


def raw_set(ctx, glo, ghi, log_n, log_g, sin_k, n_mu=None):
    """rimphony_ctx_set_tables_pitchy as a C caller reaches it -> its return code"""
    dp = ctypes.POINTER(ctypes.c_double)
    log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
    if log_g is not None:
        log_g = np.ascontiguousarray(np.atleast_2d(log_g), dtype=np.float64)
    if n_mu is None:
        n_mu = 0 if log_g is None else log_g.shape[1]
    if sin_k is not None:
        sin_k = np.ascontiguousarray(sin_k, dtype=np.float64)
    return ctx.lib.rimphony_ctx_set_tables_pitchy(ctx.handle, log_n.shape[0], log_n.shape[1], float(glo), float(ghi),
                                                  log_n.ctypes.data_as(dp), n_mu, None if log_g is None else log_g.ctypes.data_as(dp),
                                                  None if sin_k is None else sin_k.ctypes.data_as(dp))


# ---- 1. the fixture's rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A: no g", "B: 8-node rows"])
def test_fixture_rows_bit_identical(gpu_ctx, fix, which):
    """All 8 slots of the committed rows: values (NaN pattern included), per-coefficient sample counts, and the status words,
    of which the fixture holds what the values imply: ST_NONFINITE exactly where a value is NaN, ST_NORM_FAIL nowhere."""
    with time_limit(300):
        install(gpu_ctx, which, oracle=False)
        out, st, work = gpu_ctx.compute_batch(TAB, fix["s"], fix["theta"], [fix["index"]], 0xFF, want_status=True, want_work=True)
    print("set", "AB"[which], "rows", len(out), "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    assert len(out) == 24 and (np.bincount(fix["index"].astype(int)) >= 6).all()
    want = fix["values"][which]
    assert np.isfinite(want).any(axis=0).all()                      # every slot finite on at least one row
    mismatch("coefficients", out, want, lambda i: (fix["s"][i // 8], fix["theta"][i // 8], fix["index"][i // 8], i % 8))
    assert (work.astype(np.uint64) == fix["work"][which]).all()
    assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which]).all()
    assert not same_bits(fix["values"][0], fix["values"][1]).all(axis=1).any()      # the two sets differ on every row


# ---- 2. norm, P and calc_f ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_norm_and_calc_f_bit_identical(gpu_ctx, fix, which):
    """rimphony_batch_norm_device (bad indices included; set B: P by the device's quadrature) and rimphony_calc_f_batch on
    256 (gamma, mu) pairs per table: mu = +-1 and 0, a mu a rounding beyond +-1, NaN, gamma at and outside both table ends."""
    rng = np.random.default_rng(12)
    lo, hi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
    gamma = np.concatenate([np.exp(rng.uniform(np.log(lo), np.log(hi), 242)),
                            [lo, hi, np.nextafter(lo, 0.), np.nextafter(hi, np.inf), 0.5 * lo, 2 * hi, 3.0, 3.0, 3.0, 3.0, 3.0, 50.0,
                             np.nan, 3.0]])
    mu = np.concatenate([rng.uniform(-1, 1, 242),
                         [0.3, -0.3, 0.3, 0.3, 0.3, 0.3, -1.0, 1.0, 0.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), -0.0,
                          0.3, np.nan]])
    assert len(gamma) == 256 and len(mu) == 256
    index = np.array([0.0, 1.0, 2.0, 2.0, 3.0, 0.5, -1.0, np.nan])
    with time_limit(120):
        install(gpu_ctx, which)
        ref_norm = ty.batch_norm(index)
        assert np.isfinite(ref_norm[:4]).all() and np.isnan(ref_norm[4:]).all()
        mismatch("norm", gpu_ctx.norm_batch(TAB, [index]), ref_norm)
        for table in (0, 1, 2):
            for nrm in (1.0, None):
                want = ty.dev_calc_f([float(table)], ref_norm[table] if nrm is None else nrm, gamma, mu)
                got = gpu_ctx.calc_f_batch(TAB, [float(table)], gamma, mu, nrm)
                for name, g, w in zip(("f", "dfdg", "dfdcx"), got, want):
                    mismatch("%s table %d" % (name, table), g, w, lambda i: (gamma[i], mu[i]))
            outside = (gamma < lo) | (gamma > hi)
            assert (got[0][outside] == 0).all() and (got[1][outside] == 0).all() and (got[2][outside] == 0).all()
            k = ty.fixture_set(which)[4][table]
            inside = ~outside & np.isfinite(gamma) & (np.abs(mu) < 1)
            if k == 0 and which == 0:
                assert (got[2][inside] == 0).all()                          # sin^0 and no g: isotropic
            else:
                assert (got[2][inside] != 0).sum() >= 200                   # a live d f / d mu


# ---- 3. the seams -------------------------------------------------------------------------------------------------------
SEAM_TABLE = {0: 0, 1: 2}              # one table of each set: k = 0.5 without g; k = 3.0 with the wavy row
SYM_POINTS = ((30.0, 0.9), (12.0, 1.2))
SYM_COMBOS = ((1, 1, 0), (0, 2, 1))    # (coeff, stokes, negative lobe)
HEY_POINTS = ((2.0, 0.9), (60.0, 1.1))


def seam_dist(table):
    d, st = ty.mkdist(table)
    assert st == 0 and np.isfinite(d.norm)
    return d


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_symphony_seams(gpu_ctx, which):
    """integrand_kernel_n<7> (emission and absorption, whose d f / d mu term takes the general form), gamma_integral_kernel<7>,
    n_integral_kernel<7>, deriv_probe_kernel<7> and gamma_contribution_kernel<7>."""
    L = ty.load()
    rng = np.random.default_rng(700 + which)
    table = SEAM_TABLE[which]
    par = [float(table)]
    with time_limit(240):
        install(gpu_ctx, which)
        d = seam_dist(table)
        for s, th, coeff, stokes in ((100.0, 0.3, 1, 0), (100.0, 1.5, 1, 1), (30.0, 0.9, 1, 2), (30.0, 0.9, 0, 0)):
            n, g = harmonic_samples(rng, s, th, 200)
            ref = np.array([L.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
            assert (np.isfinite(ref) & (ref != 0)).sum() >= len(ref) // 2
            got = gpu_ctx.gamma_integrand_batch(TAB, par, coeff, stokes, s, th, n, g)
            mismatch("gamma_integrand", got, ref, lambda i: (s, th, coeff, stokes, n[i], g[i]))
        for (s, th), (coeff, stokes, lobe) in zip(SYM_POINTS, SYM_COMBOS):
            nmin = s * abs(math.sin(th))
            n = np.concatenate([np.floor(nmin + 1) + np.arange(8), nmin + 9 + np.exp(rng.uniform(0, 8, 8))])
            ref = np.array([L.rimo_gamma_integral(d, coeff, stokes, lobe, s, th, v) for v in n])
            assert (np.isfinite(ref) & (ref != 0)).sum() > len(n) // 2
            got = gpu_ctx.gamma_integral_batch(TAB, par, coeff, stokes, lobe, s, th, n)
            mismatch("gamma_integral", got, ref, lambda i: (s, th, n[i], lobe))
            lo = s * math.sin(th) + 31. + rng.uniform(0., 50., 16)
            hi = lo * rng.uniform(1.05, 3., 16)
            ref = np.array([ty.n_integral(d, coeff, stokes, lobe, s, th, a, b) for a, b in zip(lo, hi)])
            assert np.isfinite(ref).sum() > 8
            got = gpu_ctx.n_integral_batch(TAB, par, coeff, stokes, lobe, s, th, lo, hi)
            mismatch("n_integral", got, ref, lambda i: (coeff, stokes, lo[i], hi[i]))
            n0 = np.floor(s * math.sin(th) + 31. + rng.uniform(0., 400., 16))
            n0[8:] = n0[8:] * rng.uniform(1.5, 40., 8)
            ref = np.array([L.rimo_symphony_deriv_probe(ctypes.byref(d), coeff, stokes, lobe, s, th, float(x)) for x in n0])
            assert np.isfinite(ref).sum() >= 8
            got = gpu_ctx.deriv_probe_batch(TAB, par, coeff, stokes, lobe, s, th, n0)
            mismatch("deriv_probe", got, ref, lambda i: (coeff, stokes, n0[i]))
        for s, th, glo, ghi, coeff, stokes in ((8., 0.9, 1.5, 30., 0, 0), (400., 0.6, 3., 40., 1, 1)):
            gam = np.exp(rng.uniform(math.log(glo), math.log(ghi), 8))
            ref = np.array([L.rimo_gamma_contribution(ctypes.byref(d), coeff, stokes, s, th, float(x)) for x in gam])
            assert np.isfinite(ref).sum() >= 4
            got = gpu_ctx.gamma_contribution_batch(TAB, par, coeff, stokes, s, th, gam)
            mismatch("gamma_contribution", got, ref, lambda i: (s, coeff, stokes, gam[i]))


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_faraday_seams(gpu_ctx, which):
    """hey_element_kernel<7> and hey_outer_kernel<7>, quasi-resonant or not, stokes Q and V: the mu term of d f / d sigma
    (dev_heyvaerts.h) with both of its parts."""
    L = ty.load()
    rng = np.random.default_rng(710 + which)
    table = SEAM_TABLE[which]
    with time_limit(180):
        install(gpu_ctx, which)
        d = seam_dist(table)
        for s, th in HEY_POINTS:
            for stokes in (1, 2):
                for qr in (0, 1):
                    fixed, v = hey_seam_inputs(rng, s, th, qr, 64)
                    ref = np.array([L.rimo_hey_element(ctypes.byref(d), stokes, s, th, qr, float(a), float(b)) for a, b in zip(fixed, v)])
                    assert np.isfinite(ref).sum() > 32
                    got = gpu_ctx.hey_element_batch(TAB, [float(table)], stokes, s, th, qr, fixed, v)
                    mismatch("hey_element s %g stokes %d qr %d" % (s, stokes, qr), got, ref, lambda i: (fixed[i], v[i]))
                    u = hey_outer_abscissae(rng, s, th, qr, 6)
                    ref = np.array([L.rimo_hey_outer_integrand(ctypes.byref(d), stokes, s, th, qr, float(x)) for x in u])
                    assert np.isfinite(ref).sum() >= 3
                    got = gpu_ctx.hey_outer_batch(TAB, [float(table)], stokes, s, th, qr, u)
                    mismatch("hey_outer s %g stokes %d qr %d" % (s, stokes, qr), got, ref, lambda i: u[i])


# ---- 4. scheduling ------------------------------------------------------------------------------------------------------
def test_scheduling_changes_no_bit(gpu_ctx, fix):
    """The 24 rows, a 10-row slice of them, and a context without the cooperative tail (RIMPHONY_NO_ASSIST=1): same bits,
    same status words, same sample counts."""
    s, th, index = fix["s"], fix["theta"], fix["index"]
    sl = slice(7, 17)
    lo, hi, t, g, k = ty.fixture_set(1)
    with time_limit(300):
        install(gpu_ctx, 1, oracle=False)
        big = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        part = gpu_ctx.compute_batch(TAB, s[sl].copy(), th[sl].copy(), [index[sl].copy()], 0xFF, want_status=True, want_work=True)
        solo_ctx = env_context(RIMPHONY_NO_ASSIST="1")
        try:
            solo_ctx.set_tables(lo, hi, t, g, sin_k=k)
            solo = solo_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        finally:
            solo_ctx.close()
    mismatch("all rows", big[0], fix["values"][1])
    assert same_bits(big[0][sl], part[0]).all() and (big[1][sl] == part[1]).all() and (big[2][sl] == part[2]).all()
    assert same_bits(big[0], solo[0]).all() and (big[1] == solo[1]).all() and (big[2] == solo[2]).all()


# ---- 5. a change of form ------------------------------------------------------------------------------------------------
def test_no_state_survives_a_change_of_form(gpu_ctx, fix):
    """sin^k (set B), then pitch, then isotropic, then 2-D, then sin^k (set A): after each install the first 6 committed
    rows of that form's fixture come back bit for bit, sample counts included."""
    import tab2d_bind as t2
    pitch = np.load(os.path.join(GOLDEN, "tabulated_pitch_det.npz"))
    iso = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))
    two = np.load(os.path.join(GOLDEN, "tabulated_2d_det.npz"))
    n_nodes, n_mu = (int(x) for x in two["geometry"][0])
    steps = (
        ("sin^k B", lambda: install(gpu_ctx, 1, oracle=False), fix, fix["values"][1], fix["work"][1]),
        ("pitch", lambda: gpu_ctx.set_tables(float(pitch["gamma_lo"]), float(pitch["gamma_hi"]), pitch["tables"], tp.edge_pitch(8)),
         pitch, pitch["values"][0], pitch["work"][0]),
        ("isotropic", lambda: gpu_ctx.set_tables(float(iso["gamma_lo"]), float(iso["gamma_hi"]), iso["tables"]),
         iso, iso["values"], iso["work"]),
        ("2-D", lambda: gpu_ctx.set_tables_2d(float(two["gamma_lo"]), float(two["gamma_hi"]), t2.edge_tables_2d(n_nodes, n_mu, two["cols_0"])),
         two, two["values"][0], two["work"][0]),
        ("sin^k A", lambda: install(gpu_ctx, 0, oracle=False), fix, fix["values"][0], fix["work"][0]),
    )
    got = []
    with time_limit(300):
        for name, put, f, values, work in steps:
            put()
            got.append(gpu_ctx.compute_batch(TAB, f["s"][:6].copy(), f["theta"][:6].copy(), [f["index"][:6].copy()], 0xFF,
                                             want_status=True, want_work=True))
    for (name, put, f, values, work), (out, st, w) in zip(steps, got):
        mismatch(name, out, values[:6])
        assert (w.astype(np.uint64) == work[:6]).all(), name
        assert np.isfinite(out).any()


# ---- 6. against the device's own analytic pitchy power law --------------------------------------------------------------
def test_against_the_device_kind_2(gpu_ctx):
    """The 2048-node table of gamma^-2.5 exp(-gamma / 1e10) over [1, 1e12] with k = 1.0 and no g against RIMPHONY_PITCHY_PL
    (p = 2.5, k = 1.0) on the 16 committed pl_rows, all eight slots: 4 x the figure recorded on the CPU oracles."""
    rows = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))["pl_rows"]
    gold = np.loadtxt(os.path.join(GOLDEN, "symphony-powerlaw.txt"))
    s, th, n = gold[rows, 0].copy(), gold[rows, 1].copy(), len(rows)
    g = tab_bind.nodes(1.0, 1e12, 2048)
    with time_limit(300):
        gpu_ctx.set_tables(1.0, 1e12, tab_bind.log_n_powerlaw(g, 2.5, 1e10), sin_k=1.0)
        tab = gpu_ctx.compute_batch(TAB, s, th, [np.zeros(n)], 0xFF)
        ref = gpu_ctx.compute_batch(2, s, th, [np.full(n, 2.5), np.ones(n), np.ones(n), np.full(n, 1e12), np.full(n, 1e10)], 0xFF)
    assert n == 16 and np.isfinite(tab).all() and np.isfinite(ref).all()
    rel = np.abs(tab / ref - 1.0)
    print("max rel per slot", rel.max(axis=0), "recorded", ty.MEASURED_KIND2[1.0])
    assert rel.max() <= 4.0 * ty.MEASURED_KIND2[1.0]


# ---- 7. misuse ----------------------------------------------------------------------------------------------------------
def test_misuse_on_a_live_context(gpu_ctx, fix):
    from rimphony_amd import api, capi
    lo, hi, t, g, k = ty.fixture_set(1)
    s, th, index = fix["s"][:6].copy(), fix["theta"][:6].copy(), fix["index"][:6].copy()
    nan_g = g.copy()
    nan_g[1, 5] = np.nan
    with time_limit(300):
        # kind 4 with no set installed
        gpu_ctx.set_tables(1.0, 2.0, None)
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)
        install(gpu_ctx, 1, oracle=False)
        before = gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)
        mismatch("before", before[:, :2], fix["values"][1][:6, :2])
        for bad in (-0.5, np.nan, np.inf, -np.inf, 100.00000000000001):
            assert raw_set(gpu_ctx, lo, hi, t, g, [0.5, bad, 2.0]) == EINVAL, bad
            assert raw_set(gpu_ctx, lo, hi, t, None, [0.5, bad, 2.0]) == EINVAL, bad
        assert raw_set(gpu_ctx, lo, hi, t, g, k, n_mu=0) == EINVAL
        assert raw_set(gpu_ctx, lo, hi, t, None, k, n_mu=8) == EINVAL
        assert raw_set(gpu_ctx, lo, hi, t, nan_g, k) == EINVAL
        assert raw_set(gpu_ctx, lo, hi, t[:, :7], g, k) == EINVAL
        for wrong in ([0.5, 1.0], np.zeros(4)):
            with pytest.raises(ValueError):
                gpu_ctx.set_tables(lo, hi, t, g, sin_k=wrong)                   # a wrong length: the mirror's check
        with pytest.raises(ValueError):
            gpu_ctx.set_tables(lo, hi, t, g, sin_k=-1.0)
        after = gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)
        assert same_bits(before, after).all()                                   # the previous set is still in place
        # a bad index: NaN and ST_NORM_FAIL on that row only
        bad_index = np.array([0.0, 3.0, 2.0, 0.5, 0.0, np.nan])
        out, st = gpu_ctx.compute_batch(TAB, s, th, [bad_index], 0x03, want_status=True)
        bad = np.array([False, True, False, True, False, True])
        assert np.isnan(out[bad][:, :2]).all() and ((st[bad][:, :2] & ST_NORM_FAIL) != 0).all()
        assert ((st[~bad] & ST_NORM_FAIL) == 0).all() and np.isfinite(out[~bad][:, :2]).all()
        with pytest.raises(capi.RimphonyError, match="not supported"):
            gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, precision=api.PRECISION_F32_INTEGRAND)
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.highfreq_batch(TAB, s, th, [index])
        # sin_k = NULL is the pitch entry: the pitch fixture's rows
        pitch = np.load(os.path.join(GOLDEN, "tabulated_pitch_det.npz"))
        capi.check(raw_set(gpu_ctx, float(pitch["gamma_lo"]), float(pitch["gamma_hi"]), pitch["tables"], tp.edge_pitch(8), None), ENTRY)
        out = gpu_ctx.compute_batch(TAB, pitch["s"][:6].copy(), pitch["theta"][:6].copy(), [pitch["index"][:6].copy()], 0xFF)
        mismatch("sin_k = NULL", out, pitch["values"][0][:6])
        # n_tables = 0 clears the set
        assert raw_set(gpu_ctx, 1.0, 2.0, np.zeros((0, 8)), None, None) == 0
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)
