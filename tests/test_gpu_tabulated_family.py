"""GPU tests of the tabulated distribution as a FAMILY of energy tables with a real index per row
(rimphony_ctx_set_tables_family): the coefficients, status words, sample counts, normalisations, calc_f values and the
integrand / gamma-integral / Heyvaerts seams carry the bits of the family oracle (tests/support/liboracle_tabfamily.so), on
the group kernel and one wave per coefficient; a row at an integer index carries the bits of the same table installed through
the plain entries; no state survives a change of form; misuse is refused and leaves the previous set in place.  (What the
oracle is held to: test_tabulated_family_host.py.)  Every test runs under a time limit of its own, and the oracle's side of
a comparison is computed before the launch or taken from the fixture (tools/make_tabulated_family_fixture.py)."""
import contextlib
import ctypes
import faulthandler
import math
import os
import sys

import numpy as np
import pytest

import tab_family_bind as tf
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL = -1
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
    return np.load(os.path.join(GOLDEN, "tabulated_family_det.npz"))


def install(ctx, which, oracle=True):
    """set A (0) or B (1) in the context and, if asked, in the oracle"""
    lo, hi, t, k = tf.fixture_set(which)
    if oracle:
        assert tf.set_tables(lo, hi, t, k) == 0
    if ctx is not None:
        ctx.set_tables_family(lo, hi, t, k)


def raw_set(ctx, glo, ghi, log_n, sin_k):
    """rimphony_ctx_set_tables_family as a C caller reaches it -> its return code"""
    dp = ctypes.POINTER(ctypes.c_double)
    log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
    if sin_k is not None:
        sin_k = np.ascontiguousarray(sin_k, dtype=np.float64)
    return ctx.lib.rimphony_ctx_set_tables_family(ctx.handle, log_n.shape[0], log_n.shape[1], float(glo), float(ghi),
                                                  log_n.ctypes.data_as(dp), None if sin_k is None else sin_k.ctypes.data_as(dp))


def check_rows(ctx, fix, which):
    out, st, work = ctx.compute_batch(TAB, fix["s"], fix["theta"], [fix["x"][which].copy()], 0xFF, want_status=True, want_work=True)
    print("set", "AB"[which], "rows", len(out), "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    want = fix["values"][which]
    assert len(out) == 24 and np.isfinite(want).any(axis=0).all()           # every slot finite on at least one row
    mismatch("coefficients", out, want, lambda i: (fix["s"][i // 8], fix["theta"][i // 8], fix["x"][which][i // 8], i % 8))
    assert (work.astype(np.uint64) == fix["work"][which]).all()
    assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which]).all()


# ---- 1. the fixture's rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A: isotropic", "B: sin_k"])
def test_fixture_rows_bit_identical(gpu_ctx, fix, which):
    """All 8 slots of the committed rows on the default path: values (NaN pattern included), per-coefficient sample counts
    and the status words -- ST_NONFINITE where a value is NaN, ST_NORM_FAIL with it where the index names no table."""
    with time_limit(300):
        install(gpu_ctx, which, oracle=False)
        check_rows(gpu_ctx, fix, which)
    bad = ~((fix["x"][which] >= 0) & (fix["x"][which] <= (2 if which == 0 else 1)))
    assert bad.sum() == (6 if which == 0 else 12) and (fix["status"][which][bad] == (ST_NONFINITE | ST_NORM_FAIL)).all()


@pytest.mark.parametrize("which", [0, 1], ids=["A: isotropic", "B: sin_k"])
def test_fixture_rows_one_wave_per_coefficient(fix, which):
    """The same rows with RIMPHONY_TAB_GROUP=0: no bit, status word or sample count depends on where the Symphony slots run."""
    lo, hi, t, k = tf.fixture_set(which)
    with time_limit(300):
        ctx = env_context(RIMPHONY_TAB_GROUP="0")
        try:
            ctx.set_tables_family(lo, hi, t, k)
            check_rows(ctx, fix, which)
        finally:
            ctx.close()


# ---- 2. norm, calc_f and the seams at fractional x -----------------------------------------------------------------------
FRAC_X = {0: (0.25, 1.5, 2.0 - 2.0 ** -52), 1: (0.25, 0.5, 1.0 - 2.0 ** -52)}


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_norm_and_calc_f_bit_identical(gpu_ctx, fix, which):
    """rimphony_batch_norm_device on the fixture's indices (the bad ones included) and rimphony_calc_f_batch on 256
    (gamma, mu) pairs per row: mu = +-1 and 0, a mu a rounding beyond +-1, NaN, gamma at and outside both table ends."""
    rng = np.random.default_rng(14)
    lo, hi = tf.EDGE_LO, tf.EDGE_HI
    gamma = np.concatenate([np.exp(rng.uniform(np.log(lo), np.log(hi), 242)),
                            [lo, hi, np.nextafter(lo, 0.), np.nextafter(hi, np.inf), 0.5 * lo, 2 * hi, 3.0, 3.0, 3.0, 3.0, 3.0, 50.0,
                             np.nan, 3.0]])
    mu = np.concatenate([rng.uniform(-1, 1, 242),
                         [0.3, -0.3, 0.3, 0.3, 0.3, 0.3, -1.0, 1.0, 0.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), -0.0,
                          0.3, np.nan]])
    x = np.concatenate([tf.fixture_x(which), FRAC_X[which], [-0.0, -1e-300, np.inf, -np.inf]])
    with time_limit(120):
        install(gpu_ctx, which)
        ref_norm = tf.batch_norm(x)
        mismatch("norm", gpu_ctx.norm_batch(TAB, [x]), ref_norm, lambda i: x[i])
        mismatch("norm, the fixture's", ref_norm[:8], fix["norm"][which][:8])
        assert np.isfinite(ref_norm[8:12]).all() and np.isnan(ref_norm[12:]).all()
        for xr in FRAC_X[which]:
            nrm_x = float(tf.batch_norm(np.array([xr]))[0])
            for nrm in (1.0, None):
                want = tf.dev_calc_f(xr, nrm_x if nrm is None else nrm, gamma, mu)
                got = gpu_ctx.calc_f_batch(TAB, [xr], gamma, mu, nrm)
                for name, g, w in zip(("f", "dfdg", "dfdcx"), got, want):
                    mismatch("%s x %r" % (name, xr), g, w, lambda i: (gamma[i], mu[i]))
            outside = (gamma < lo) | (gamma > hi)
            assert (got[0][outside] == 0).all() and (got[1][outside] == 0).all() and (got[2][outside] == 0).all()
            inside = ~outside & np.isfinite(gamma) & (np.abs(mu) < 1)
            assert (got[0][inside] > 0).sum() >= 200
            if which == 0:
                assert (got[2][inside] == 0).all()                          # isotropic
            else:
                assert (got[2][inside] != 0).sum() >= 200                   # a live d f / d mu


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_symphony_and_faraday_seams(gpu_ctx, which):
    """integrand_kernel_n and gamma_integral_kernel of the form (emission and absorption), hey_element_kernel and
    hey_outer_kernel (quasi-resonant or not, stokes Q and V), at a fractional index."""
    L = tf.load()
    rng = np.random.default_rng(720 + which)
    xr = FRAC_X[which][0] if which else FRAC_X[which][1]
    par = [xr]
    with time_limit(240):
        install(gpu_ctx, which)
        d, st = tf.mkdist(xr)
        assert st == 0 and np.isfinite(d.norm)
        for s, th, coeff, stokes in ((100.0, 0.3, 1, 0), (30.0, 0.9, 1, 2), (30.0, 0.9, 0, 0)):
            n, g = harmonic_samples(rng, s, th, 200)
            ref = np.array([L.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
            assert (np.isfinite(ref) & (ref != 0)).sum() >= len(ref) // 2
            got = gpu_ctx.gamma_integrand_batch(TAB, par, coeff, stokes, s, th, n, g)
            mismatch("gamma_integrand", got, ref, lambda i: (s, th, coeff, stokes, n[i], g[i]))
        for (s, th), (coeff, stokes, lobe) in zip(((30.0, 0.9), (12.0, 1.2)), ((1, 1, 0), (0, 2, 1))):
            nmin = s * abs(math.sin(th))
            n = np.concatenate([np.floor(nmin + 1) + np.arange(8), nmin + 9 + np.exp(rng.uniform(0, 8, 8))])
            ref = np.array([L.rimo_gamma_integral(d, coeff, stokes, lobe, s, th, v) for v in n])
            assert (np.isfinite(ref) & (ref != 0)).sum() > len(n) // 2
            got = gpu_ctx.gamma_integral_batch(TAB, par, coeff, stokes, lobe, s, th, n)
            mismatch("gamma_integral", got, ref, lambda i: (s, th, n[i], lobe))
        for s, th in ((2.0, 0.9), (60.0, 1.1)):
            for stokes in (1, 2):
                for qr in (0, 1):
                    fixed, v = hey_seam_inputs(rng, s, th, qr, 64)
                    ref = np.array([L.rimo_hey_element(ctypes.byref(d), stokes, s, th, qr, float(a), float(b)) for a, b in zip(fixed, v)])
                    assert np.isfinite(ref).sum() > 32
                    got = gpu_ctx.hey_element_batch(TAB, par, stokes, s, th, qr, fixed, v)
                    mismatch("hey_element s %g stokes %d qr %d" % (s, stokes, qr), got, ref, lambda i: (fixed[i], v[i]))
                    u = hey_outer_abscissae(rng, s, th, qr, 6)
                    ref = np.array([L.rimo_hey_outer_integrand(ctypes.byref(d), stokes, s, th, qr, float(a)) for a in u])
                    assert np.isfinite(ref).sum() >= 3
                    got = gpu_ctx.hey_outer_batch(TAB, par, stokes, s, th, qr, u)
                    mismatch("hey_outer s %g stokes %d qr %d" % (s, stokes, qr), got, ref, lambda i: u[i])


# ---- 3. integer rows are the plain forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_integer_rows_are_the_plain_form(gpu_ctx, fix, which):
    """The same context after set_tables / set_tables(sin_k=...) of the same tables: coefficients, status words, sample
    counts, normalisations and calc_f of the rows at integer indices, as uint64."""
    lo, hi, t, k = tf.fixture_set(which)
    nt = t.shape[0]
    s, th = fix["s"][:2 * nt].copy(), fix["theta"][:2 * nt].copy()
    index = np.tile(np.arange(nt, dtype=np.float64), 2)
    gamma = np.exp(np.linspace(np.log(lo), np.log(hi), 100))
    mu = np.linspace(-0.95, 0.95, 100)
    with time_limit(300):
        install(gpu_ctx, which, oracle=False)
        fam = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        fam_norm = gpu_ctx.norm_batch(TAB, [index])
        fam_f = [gpu_ctx.calc_f_batch(TAB, [float(i)], gamma, mu, None) for i in range(nt)]
        gpu_ctx.set_tables(lo, hi, t, sin_k=k)
        plain = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        plain_norm = gpu_ctx.norm_batch(TAB, [index])
        plain_f = [gpu_ctx.calc_f_batch(TAB, [float(i)], gamma, mu, None) for i in range(nt)]
    assert np.isfinite(fam[0]).mean() > 0.8
    mismatch("coefficients", fam[0], plain[0])
    assert (fam[1] == plain[1]).all() and (fam[2] == plain[2]).all()
    mismatch("norm", fam_norm, plain_norm)
    for a, b in zip(fam_f, plain_f):
        for name, g, w in zip(("f", "dfdg", "dfdcx"), a, b):
            assert np.isfinite(g).all()
            mismatch(name, g, w)


# ---- 4. a change of form ------------------------------------------------------------------------------------------------
def test_no_state_survives_a_change_of_form(gpu_ctx, fix):
    """2-D, family B, family A, isotropic, family B: after each install the first 6 committed rows of that form's fixture
    come back bit for bit, sample counts included."""
    import tab2d_bind as t2
    iso = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))
    two = np.load(os.path.join(GOLDEN, "tabulated_2d_det.npz"))
    n_nodes, n_mu = (int(v) for v in two["geometry"][0])

    def rows(f, index):
        return f["s"][:6].copy(), f["theta"][:6].copy(), index[:6].copy()

    steps = (
        ("2-D", lambda: gpu_ctx.set_tables_2d(float(two["gamma_lo"]), float(two["gamma_hi"]), t2.edge_tables_2d(n_nodes, n_mu, two["cols_0"])),
         rows(two, two["index"]), two["values"][0], two["work"][0]),
        ("family B", lambda: install(gpu_ctx, 1, oracle=False), rows(fix, fix["x"][1]), fix["values"][1], fix["work"][1]),
        ("family A", lambda: install(gpu_ctx, 0, oracle=False), rows(fix, fix["x"][0]), fix["values"][0], fix["work"][0]),
        ("isotropic", lambda: gpu_ctx.set_tables(float(iso["gamma_lo"]), float(iso["gamma_hi"]), iso["tables"]),
         rows(iso, iso["index"]), iso["values"], iso["work"]),
        ("family B again", lambda: install(gpu_ctx, 1, oracle=False), rows(fix, fix["x"][1]), fix["values"][1], fix["work"][1]),
    )
    got = []
    with time_limit(300):
        for name, put, (s, th, index), values, work in steps:
            put()
            got.append(gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True))
    for (name, put, r, values, work), (out, st, w) in zip(steps, got):
        mismatch(name, out, values[:6])
        assert (w.astype(np.uint64) == work[:6]).all(), name
        assert np.isfinite(out).any()


# ---- 5. refusals and the set read back -----------------------------------------------------------------------------------
def test_refusals_and_the_blob(gpu_ctx, fix):
    from rimphony_amd import capi
    lo, hi, t, k = tf.fixture_set(1)
    s, th, x = fix["s"][:6].copy(), fix["theta"][:6].copy(), fix["x"][1][:6].copy()
    nan_t = t.copy()
    nan_t[1, 3] = np.inf
    with time_limit(300):
        for which in (0, 1):
            install(gpu_ctx, which)
            assert gpu_ctx.tables_blob().tobytes() == tf.blob().tobytes() and len(tf.blob()) > 8
        before = gpu_ctx.compute_batch(TAB, s, th, [x], 0x03)
        mismatch("before", before[:, :2], fix["values"][1][:6, :2])
        assert raw_set(gpu_ctx, lo, hi, t[:, :7], k) == EINVAL
        assert raw_set(gpu_ctx, lo, hi, np.zeros((2, 65537)), k) == EINVAL
        assert raw_set(gpu_ctx, 0.99, hi, t, k) == EINVAL
        assert raw_set(gpu_ctx, lo, hi, nan_t, k) == EINVAL
        assert raw_set(gpu_ctx, lo, hi, nan_t, None) == EINVAL
        for bad in (-0.5, np.nan, 100.00000000000001):
            assert raw_set(gpu_ctx, lo, hi, t, [0.5, bad]) == EINVAL, bad
        assert gpu_ctx.tables_blob().tobytes() == tf.blob().tobytes()
        after = gpu_ctx.compute_batch(TAB, s, th, [x], 0x03)
        assert same_bits(before, after).all()                                   # the previous set is still in place
        # the plain entries keep refusing a non-integer index
        gpu_ctx.set_tables(lo, hi, t, sin_k=k)
        out, st = gpu_ctx.compute_batch(TAB, s, th, [np.array([0.0, 0.25, 1.0, 0.5, 1.0, 0.0])], 0x03, want_status=True)
        bad = np.array([False, True, False, True, False, False])
        assert np.isnan(out[bad][:, :2]).all() and ((st[bad][:, :2] & ST_NORM_FAIL) != 0).all() and np.isfinite(out[~bad][:, :2]).all()
        # n_tables = 0 clears the set
        assert raw_set(gpu_ctx, 1.0, 2.0, np.zeros((0, 8)), None) == 0
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.compute_batch(TAB, s, th, [x], 0x03)
