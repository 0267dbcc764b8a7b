"""GPU tests of the tabulated distribution as a family of 2-D surfaces blended CUBICALLY across its tables
(rimphony_ctx_set_tables_2d_family_cubic): the coefficients, status words, sample counts, normalisations, calc_f values and the
integrand / gamma-integral / Heyvaerts seams carry the bits of the form's oracle (tests/support/liboracle_tab2dfamilycubic.so),
on the group kernel and one wave per coefficient; a row at an integer index carries the bits of the same table installed through
set_tables_2d_nodes; the rows of a batch each read their own line, neighbours on different stencils; no state survives a change
of form; misuse is refused and leaves the previous set in place; a row whose blended k overshoots is a NaN row.  (What the
oracle is held to: test_tabulated_2d_family_cubic_host.py.)  Every test runs under a time limit of its own, and the oracle's side
of a comparison is computed before the launch or taken from the fixture (tools/make_tabulated_2d_family_cubic_fixture.py)."""
import contextlib
import ctypes
import faulthandler
import math
import os
import sys

import numpy as np
import pytest

import tab2d_family_bind as tf
import tab2d_family_cubic_bind as tc
import tab2d_nodes_bind as tn
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
    return np.load(os.path.join(GOLDEN, "tabulated_2d_family_cubic_det.npz"))


def install(ctx, which, oracle=True):
    """set A (0) or B (1) in the context and, if asked, in the oracle"""
    gamma, mu, t, k, ends, param = tc.fixture_set(which)
    if oracle:
        assert tc.set_tables(gamma, mu, t, k, ends, param) == 0
    if ctx is not None:
        ctx.set_tables_2d_family(gamma, mu, t, k, ends, blend="cubic", param=param)


def raw_set(ctx, gamma, mu, log_n, sin_k, ends=(0, 0), param=None, shape=None):
    """rimphony_ctx_set_tables_2d_family_cubic as a C caller reaches it -> its return code"""
    keep, a = tf.call_args(gamma, mu, log_n, sin_k, shape)
    param = None if param is None else np.ascontiguousarray(param, dtype=np.float64)
    return ctx.lib.rimphony_ctx_set_tables_2d_family_cubic(ctx.handle, *a, int(ends[0]), int(ends[1]), tc._dp(param))


def check_rows(ctx, fix, which, tiles=1):
    s, th, x = (np.tile(fix[k], tiles) for k in ("s", "theta", "x"))
    out, st, work = ctx.compute_batch(TAB, s, th, [x.copy()], 0xFF, want_status=True, want_work=True)
    print("set", "AB"[which], "rows", len(out), "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    want = np.tile(fix["values"][which], (tiles, 1))
    assert len(out) == 24 * tiles and np.isfinite(want).any(axis=0).all()           # every slot finite on at least one row
    mismatch("coefficients", out, want, lambda i: (s[i // 8], th[i // 8], x[i // 8], i % 8))
    assert (work.astype(np.uint64) == np.tile(fix["work"][which], (tiles, 1))).all()
    assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == np.tile(fix["status"][which], (tiles, 1))).all()


# ---- 1. the fixture's rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A: plain", "B: sin_k"])
def test_fixture_rows_bit_identical(gpu_ctx, fix, which):
    """All 8 slots of the committed rows on the default path: values (NaN pattern included), per-coefficient sample counts
    and the status words -- ST_NONFINITE where a value is NaN, ST_NORM_FAIL with it where the index names no table."""
    with time_limit(300):
        install(gpu_ctx, which, oracle=False)
        check_rows(gpu_ctx, fix, which)
    bad = ~tc.valid_x(fix["x"])
    assert bad.sum() == tc.BAD_X and (fix["status"][which][bad] == (ST_NONFINITE | ST_NORM_FAIL)).all()
    assert np.isfinite(fix["values"][which][~bad]).mean() >= 0.8


@pytest.mark.parametrize("which", [0, 1], ids=["A: plain", "B: sin_k"])
def test_fixture_rows_one_wave_per_coefficient(fix, which):
    """The same rows with RIMPHONY_TAB_GROUP=0: no bit, status word or sample count depends on where the Symphony slots run."""
    gamma, mu, t, k, ends, param = tc.fixture_set(which)
    with time_limit(300):
        ctx = env_context(RIMPHONY_TAB_GROUP="0")
        try:
            ctx.set_tables_2d_family(gamma, mu, t, k, ends, blend="cubic", param=param)
            check_rows(ctx, fix, which)
        finally:
            ctx.close()


# ---- 2. norm, calc_f and the seams at fractional x -----------------------------------------------------------------------
SEAM_X = (0.37, 2.25, 4.75)         # the stencil clamped low, interior, clamped high


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_norm_and_calc_f_bit_identical(gpu_ctx, fix, which):
    """rimphony_batch_norm_device on the fixture's indices (the bad ones included) and rimphony_calc_f_batch at three fractional
    x, one per stencil position, on 256 (gamma, mu) pairs: mu = +-1 and 0, a mu a rounding beyond +-1, NaN, gamma at and
    outside both table ends."""
    rng = np.random.default_rng(18)
    gamma_n = tc.fixture_nodes(which)[0]
    lo, hi = float(gamma_n[0]), float(gamma_n[-1])
    gamma = np.concatenate([np.exp(rng.uniform(np.log(lo), np.log(hi), 242)),
                            [lo, hi, np.nextafter(lo, 0.), np.nextafter(hi, np.inf), 0.5 * (1.0 + lo), 2 * hi, 3.0, 3.0, 3.0, 3.0, 3.0, 50.0,
                             np.nan, 3.0]])
    mu = np.concatenate([rng.uniform(-1, 1, 242),
                         [0.3, -0.3, 0.3, 0.3, 0.3, 0.3, -1.0, 1.0, 0.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), -0.0,
                          0.3, np.nan]])
    x = fix["x"].copy()
    valid = tc.valid_x(x)
    with time_limit(120):
        install(gpu_ctx, which)
        mismatch("norm", gpu_ctx.norm_batch(TAB, [x]), fix["norm"][which], lambda i: x[i])
        assert np.isfinite(fix["norm"][which][valid]).all() and np.isnan(fix["norm"][which][~valid]).all()
        for xr in SEAM_X:
            nrm_x = float(tc.batch_norm(np.array([xr]))[0])
            for nrm in (1.0, None):
                want = tc.dev_calc_f(xr, nrm_x if nrm is None else nrm, gamma, mu)
                got = gpu_ctx.calc_f_batch(TAB, [xr], gamma, mu, nrm)
                for name, g, w in zip(("f", "dfdg", "dfdcx"), got, want):
                    mismatch("%s x %r" % (name, xr), g, w, lambda i: (gamma[i], mu[i]))
            outside = (gamma < lo) | (gamma > hi)
            assert outside.sum() == 4 and (got[0][outside] == 0).all() and (got[1][outside] == 0).all() and (got[2][outside] == 0).all()
            inside = ~outside & np.isfinite(gamma) & (np.abs(mu) < 1)
            assert (got[0][inside] > 0).sum() >= 200 and (got[2][inside] != 0).sum() >= 200     # a live d f / d mu
            ends = np.isin(np.abs(mu), [1.0, np.nextafter(1.0, 2.0)]) & ~outside
            assert ends.sum() == 4 and (np.isnan(got[2][ends]).all() if which else np.isfinite(got[2][ends]).all())


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_symphony_and_faraday_seams(gpu_ctx, which):
    """integrand_kernel_n and gamma_integral_kernel of the form (emission and absorption), hey_element_kernel and
    hey_outer_kernel (quasi-resonant or not, stokes Q and V), at a fractional index: A on an interior stencil, B on the one
    clamped at the high end."""
    L = tc.load()
    rng = np.random.default_rng(750 + which)
    xr = SEAM_X[2] if which else SEAM_X[1]
    par = [xr]
    with time_limit(240):
        install(gpu_ctx, which)
        d, st = tc.mkdist(xr)
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


# ---- 3. integer rows are the plain form ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_integer_rows_are_the_plain_form(gpu_ctx, fix, which):
    """The same context after set_tables_2d_nodes(..., sin_k, ends) of the same tables: coefficients, status words, sample
    counts, normalisations and calc_f of the rows at integer indices, as uint64."""
    gamma_n, mu_n, t, k, ends, param = tc.fixture_set(which)
    nt = t.shape[0]
    s, th = fix["s"][:2 * nt].copy(), fix["theta"][:2 * nt].copy()
    index = np.tile(np.arange(nt, dtype=np.float64), 2)
    gamma = np.exp(np.linspace(np.log(gamma_n[0]), np.log(gamma_n[-1]), 102))[1:-1]
    mu = np.linspace(-0.95, 0.95, 100)
    with time_limit(300):
        install(gpu_ctx, which, oracle=False)
        fam = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        fam_norm = gpu_ctx.norm_batch(TAB, [index])
        fam_f = [gpu_ctx.calc_f_batch(TAB, [float(i)], gamma, mu, None) for i in range(nt)]
        gpu_ctx.set_tables_2d_nodes(gamma_n, mu_n, t, k, ends)
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


# ---- 4. the rows of one batch and the growth of the line array ---------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_many_rows_each_read_their_own_line(gpu_ctx, fix, which):
    """A 24-row batch, then one batch of the same rows tiled 16 times, 384 rows, in the same context, after a LINEAR family of
    as many rows has sized the line array for its narrower lines: the array grows, and every tile carries the fixture's bits --
    a line indexed, strided or sized wrongly gives a row another row's weights.  Neighbouring rows of the fixture use
    different stencils (x = 0.37, 1.5, 2.25, 3.5, 4.75: base tables 0, 0, 1, 2, 2)."""
    assert [tc.numpy_weights(None, tc.N_TABLES, v)[0] for v in tc.FRAC_X] == [0, 0, 1, 2, 2]
    gamma, mu, t, k, ends, param = tc.fixture_set(which)
    with time_limit(300):
        gpu_ctx.set_tables_2d_family(gamma, mu, t, k, ends)
        x = np.tile(np.where(tc.valid_x(fix["x"]), fix["x"], 0.0), 16)
        gpu_ctx.compute_batch(TAB, np.tile(fix["s"], 16), np.tile(fix["theta"], 16), [x], 0x01)
        install(gpu_ctx, which, oracle=False)
        check_rows(gpu_ctx, fix, which, tiles=16)
        check_rows(gpu_ctx, fix, which)


# ---- 5. a change of form ------------------------------------------------------------------------------------------------
def test_no_state_survives_a_change_of_form(gpu_ctx, fix):
    """Linear family -> cubic family -> plain nodes -> cubic: after each install the first 6 committed rows of that form's
    fixture come back bit for bit, sample counts included."""
    lin = np.load(os.path.join(GOLDEN, "tabulated_2d_family_det.npz"))
    nod = np.load(os.path.join(GOLDEN, "tabulated_2d_nodes_det.npz"))

    def rows(f, index):
        return f["s"][:6].copy(), f["theta"][:6].copy(), index[:6].copy()

    def put_linear():
        gamma, mu, t, k, ends = tf.fixture_set(1)
        gpu_ctx.set_tables_2d_family(gamma, mu, t, k, ends)

    steps = (
        ("linear family B", put_linear, rows(lin, lin["x"][1]), lin["values"][1], lin["work"][1]),
        ("cubic family B", lambda: install(gpu_ctx, 1, oracle=False), rows(fix, fix["x"]), fix["values"][1], fix["work"][1]),
        ("2-D nodes", lambda: gpu_ctx.set_tables_2d_nodes(nod["gamma_k"], nod["mu_k"], nod["tables_k"], nod["k_k"]),
         rows(nod, nod["index"]), nod["values"][1], nod["work"][1]),
        ("cubic family A", lambda: install(gpu_ctx, 0, oracle=False), rows(fix, fix["x"]), fix["values"][0], fix["work"][0]),
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


# ---- 6. refusals and the set read back -----------------------------------------------------------------------------------
def test_refusals_and_the_blob(gpu_ctx, fix):
    from rimphony_amd import capi
    gamma, mu, t, k, ends, param = tc.fixture_set(1)
    s, th, x = fix["s"][:6].copy(), fix["theta"][:6].copy(), fix["x"][:6].copy()
    with time_limit(300):
        for which in (0, 1):
            install(gpu_ctx, which)
            assert gpu_ctx.tables_blob().tobytes() == tc.blob().tobytes() and len(tc.blob()) > 8
        before = gpu_ctx.compute_batch(TAB, s, th, [x], 0x03)
        mismatch("before", before[:, :2], fix["values"][1][:6, :2])
        for n in (1, 2, 3):
            assert raw_set(gpu_ctx, gamma, mu, t[:n], k[:n], ends, param[:n]) == EINVAL, n
        for bad in ([0.0, 1.0, 2.0, 1.5, 3.0, 4.0], [0.0, 1.0, np.nan, 3.0, 4.0, 5.0], [0.0, 1.0, 1.0, 2.0, 3.0, 4.0],
                    [0.0, 1.0, 2.0, 3.0, 4.0, np.inf]):
            assert raw_set(gpu_ctx, gamma, mu, t, k, ends, bad) == EINVAL, bad
        for name, (g, m, tt, kk, shape) in tn.refused_cases(gamma, mu, t, k).items():
            assert raw_set(gpu_ctx, g, m, tt, kk, ends, None, shape) == EINVAL, name
        for bad_ends in ((2, 0), (0, -1), (0, 2)):
            assert raw_set(gpu_ctx, gamma, mu, t, k, bad_ends, param) == EINVAL, bad_ends
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d_family(gamma, mu, t, k, ends, blend="linear", param=param)
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d_family(gamma, mu, t, k, ends, blend="cubic", param=param[:5])
        assert gpu_ctx.tables_blob().tobytes() == tc.blob().tobytes()
        after = gpu_ctx.compute_batch(TAB, s, th, [x], 0x03)
        assert same_bits(before, after).all()                                   # the previous set is still in place
        # n_tables = 0 clears the set
        assert raw_set(gpu_ctx, None, None, np.zeros((0, 8, 8)), None) == 0
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.compute_batch(TAB, s, th, [x], 0x03)


# ---- 7. the k overshoot --------------------------------------------------------------------------------------------------------
def test_k_overshoot_is_a_nan_row(gpu_ctx):
    """sin_k = (0, 0, 3, 0, 0, 0) on the knots 0 .. 5: the row at x = 0.5 blends k to -0.9375 and is a NaN row with
    RIMPHONY_ST_NORM_FAIL in every slot; the rows at the knots and at x = 1.5 around it carry the oracle's bits."""
    gamma, mu, t, k, ends, param = tc.overshoot_set()
    assert tc.set_tables(gamma, mu, t, k, ends, param) == 0
    x = np.array([tc.OVERSHOOT_X, 0.0, 1.0, 2.0, 1.5, tc.OVERSHOOT_X])
    s, th = np.full(6, 30.0), np.full(6, 0.9)
    want, want_work = tc.batch(s, th, x, 0xFF)
    want_norm = tc.batch_norm(x)
    bad = np.array([True, False, False, False, False, True])
    assert np.isnan(want[bad]).all() and np.isfinite(want[~bad]).mean() > 0.8 and np.isnan(want_norm[bad]).all()
    with time_limit(120):
        gpu_ctx.set_tables_2d_family(gamma, mu, t, k, ends, blend="cubic", param=param)
        out, st, work = gpu_ctx.compute_batch(TAB, s, th, [x], 0xFF, want_status=True, want_work=True)
        nrm = gpu_ctx.norm_batch(TAB, [x])
    mismatch("coefficients", out, want)
    mismatch("norm", nrm, want_norm)
    assert (work.astype(np.uint64) == want_work).all()
    assert ((st[bad] & (ST_NONFINITE | ST_NORM_FAIL)) == (ST_NONFINITE | ST_NORM_FAIL)).all()
    assert ((st[~bad] & ST_NORM_FAIL) == 0).all()
