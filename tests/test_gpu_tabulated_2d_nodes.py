"""GPU tests of the tabulated distribution as 2-D sets on gamma nodes and mu nodes of the caller's choosing
(rimphony_ctx_set_tables_2d_nodes), plain and with a sin^k xi prefactor: the coefficients, the normalisations integrated on
the device -- every mu cell with its own centre and half width, the end cells of a sin^k set under their substitution --,
calc_f values and the seams carry the bits of the form's table oracle (tests/support/liboracle_tab2dnodes.so); routing and
scheduling change no bit; no state survives a change of form; a refused set leaves the previous one in place.  Every test
runs under a time limit of its own, and the oracle's side of a comparison is computed before the launch.  The oracle's
normalisations of the fixture's sets are the fixture's record of them; the GPU integrates its own."""
import contextlib
import ctypes
import faulthandler
import os
import sys

import numpy as np
import pytest

import tab_grid_bind as tg
import tab2d_nodes_bind as tn
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL = -1
ST_NONFINITE, ST_NORM_FAIL = 16, 32
TAB = 4
SETS = pytest.mark.parametrize("which", [0, 1], ids=["P: 32 log-gm1 x 9 graded, plain", "K: 24 jittered x 12 in xi, k 0.5 2.5"])


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
    return np.load(os.path.join(GOLDEN, "tabulated_2d_nodes_det.npz"))


def fixture_set(fix, which):
    """(gamma, mu, log_n, sin_k) of set P (sin_k None) or K"""
    if which == 0:
        return fix["gamma_p"], fix["mu_p"], fix["tables_p"], None
    return fix["gamma_k"], fix["mu_k"], fix["tables_k"], fix["k_k"]


def install(ctx, fix, which, oracle=True):
    """set P (0) or K (1) of the fixture in the context and, if asked, in the oracle (with the recorded normalisations)"""
    gamma, mu, t, k = fixture_set(fix, which)
    if oracle:
        assert tn.set_tables(gamma, mu, t, k, with_norm=False) == 0 and tn.put_norms(fix["norms"][which]) == 0
    if ctx is not None:
        ctx.set_tables_2d_nodes(gamma, mu, t, k)


def raw_set(ctx, gamma, mu, log_n, sin_k, shape=None):
    """the C entry as a C caller reaches it -> its return code; shape: what the call states"""
    dp = ctypes.POINTER(ctypes.c_double)
    nt, nn, nmu, gamma, mu, log_n, sin_k = tn._args(gamma, mu, log_n, sin_k, shape)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    return ctx.lib.rimphony_ctx_set_tables_2d_nodes(ctx.handle, nt, nn, ptr(gamma), nmu, ptr(mu), ptr(log_n), ptr(sin_k))


def first_rows(ctx, f, n=6, mask=0xFF):
    return ctx.compute_batch(TAB, f["s"][:n].copy(), f["theta"][:n].copy(), [f["index"][:n].copy()], mask, want_status=True, want_work=True)


# ---- 1. the fixture's rows ----------------------------------------------------------------------------------------------
@SETS
def test_fixture_rows_bit_identical(gpu_ctx, fix, which):
    """All 8 slots of the committed rows under the default routing and with RIMPHONY_TAB_GROUP=0 in a context of its own:
    values (NaN pattern included), per-coefficient sample counts, ST_NONFINITE exactly where a value is NaN, ST_NORM_FAIL
    nowhere; the same bits both ways."""
    want = fix["values"][which]
    assert len(fix["s"]) == 24 and (np.bincount(fix["index"].astype(int)) >= 6).all() and (np.isfinite(want).sum(axis=0) >= 12).all()
    assert not same_bits(fix["values"][0], fix["values"][1]).all(axis=1).any()      # the two sets differ on every row
    with time_limit(300):
        install(gpu_ctx, fix, which, oracle=False)
        runs = {"default": first_rows(gpu_ctx, fix, 24)}
        solo = env_context(RIMPHONY_TAB_GROUP="0")
        try:
            install(solo, fix, which, oracle=False)
            runs["one wave per coefficient"] = first_rows(solo, fix, 24)
        finally:
            solo.close()
    for name, (out, st, work) in runs.items():
        print("set", "PK"[which], name, "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
        mismatch(name, out, want, lambda i: (fix["s"][i // 8], fix["theta"][i // 8], fix["index"][i // 8], i % 8))
        assert (work.astype(np.uint64) == fix["work"][which]).all(), name
        assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which]).all(), name


# ---- 2. norm and calc_f -------------------------------------------------------------------------------------------------
@SETS
def test_norm_and_calc_f_bit_identical(gpu_ctx, fix, which):
    """The tables' normalisations as the device integrated them, bad indices (2.0, 0.5, -1, NaN -> NaN) included, and
    rimphony_calc_f_batch on 256 (gamma, mu) pairs per table: every mu node and one ulp either side of it, mu = +-1 and a
    rounding beyond (set P extrapolates its end cell, set K gives NaN: the square root), +-0, NaN in either argument, gamma at
    both ends of the table and outside them."""
    rng = np.random.default_rng(1213 + which)
    nodes, mun, tables, k = fixture_set(fix, which)
    lo, hi = nodes[0], nodes[-1]
    mu_special = np.concatenate([mun, np.nextafter(mun, 2.0), np.nextafter(mun, -2.0), [0.0, -0.0]])
    n_sp = len(mu_special)
    tail_g = [lo, hi, 0.5 * (1. + lo), 2 * hi, np.nextafter(lo, 0.), np.nextafter(hi, np.inf), np.nan, 3.0, np.nan, 50.0]
    tail_m = [0.3, -0.3, 0.3, 0.3, 0.3, -0.3, 0.3, np.nan, np.nan, 0.3]
    n_rand = 256 - n_sp - len(tail_g)
    gamma = np.concatenate([np.exp(rng.uniform(np.log(1.05 * lo), np.log(0.9 * hi), n_sp + n_rand)), tail_g])
    mu = np.concatenate([mu_special, rng.uniform(-1, 1, n_rand), tail_m])
    assert len(gamma) == 256 and len(mu) == 256
    beyond = np.abs(mu) > 1.0
    assert beyond.sum() == 2
    index = np.array([0.0, 1.0, 1.0, 2.0, 0.5, -1.0, np.nan])
    with time_limit(120):
        install(gpu_ctx, fix, which)
        ref_norm = tn.batch_norm(index)
        assert np.isfinite(ref_norm[:3]).all() and np.isnan(ref_norm[3:]).all() and (ref_norm[:2] == fix["norms"][which]).all()
        want = {(table, nrm): tn.dev_calc_f([float(table)], ref_norm[table] if nrm is None else nrm, gamma, mu)
                for table in (0, 1) for nrm in (1.0, None)}
        mismatch("norm", gpu_ctx.norm_batch(TAB, [index]), ref_norm)
        for (table, nrm), w in want.items():
            got = gpu_ctx.calc_f_batch(TAB, [float(table)], gamma, mu, nrm)
            for name, g, r in zip(("f", "dfdg", "dfdcx"), got, w):
                mismatch("%s table %d" % (name, table), g, r, lambda i: (gamma[i], mu[i]))
            outside = (gamma < lo) | (gamma > hi)
            assert outside.sum() >= 4
            assert (got[0][outside] == 0).all() and (got[1][outside] == 0).all() and (got[2][outside] == 0).all()
            assert np.isnan(got[0][np.isnan(gamma)]).all() and np.isnan(got[0][np.isnan(mu) & ~outside]).all()
            ends = (np.abs(mu) == 1.0) & ~outside
            assert ends.sum() == 2
            if k is None:
                # the plain function: the end cell extrapolates a rounding beyond +-1, and the ends are ordinary points
                assert (np.isfinite(got[0][beyond]) & (got[0][beyond] > 0)).all() and np.isfinite(got[2][beyond]).all()
                assert np.isfinite(got[2][ends]).all()
            else:
                assert np.isnan(got[0][beyond]).all() and np.isnan(got[2][beyond]).all()
                assert np.isnan(got[2][ends]).all()                                         # d f / d mu at |mu| = 1
            inside = ~outside & np.isfinite(gamma) & np.isfinite(mu) & ~beyond
            assert (np.isfinite(got[0][inside]) & (got[0][inside] >= 0)).all() and (got[0][inside] > 0).sum() >= 150


# ---- 3. the seams -------------------------------------------------------------------------------------------------------
def seam_dist(table):
    d, st = tn.mkdist(table)
    assert st == 0 and np.isfinite(d.norm)
    return d


@SETS
def test_symphony_seams(gpu_ctx, fix, which):
    """integrand_kernel_n and gamma_integral_kernel of the form, one point, on table 0"""
    import math
    L = tn.load()
    rng = np.random.default_rng(1200 + which)
    table, par = 0, [0.0]
    s, th, coeff, stokes, lobe = 30.0, 0.9, 1, 1, 0
    with time_limit(240):
        install(gpu_ctx, fix, which)
        d = seam_dist(table)
        n, g = harmonic_samples(rng, s, th, 200)
        ref = np.array([L.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
        assert (np.isfinite(ref) & (ref != 0)).sum() >= len(ref) // 2
        nmin = s * abs(math.sin(th))
        n2 = np.concatenate([np.floor(nmin + 1) + np.arange(8), nmin + 9 + np.exp(rng.uniform(0, 8, 8))])
        ref2 = np.array([L.rimo_gamma_integral(d, coeff, stokes, lobe, s, th, v) for v in n2])
        assert (np.isfinite(ref2) & (ref2 != 0)).sum() > len(n2) // 2
        mismatch("gamma_integrand", gpu_ctx.gamma_integrand_batch(TAB, par, coeff, stokes, s, th, n, g), ref, lambda i: (n[i], g[i]))
        mismatch("gamma_integral", gpu_ctx.gamma_integral_batch(TAB, par, coeff, stokes, lobe, s, th, n2), ref2, lambda i: n2[i])


@SETS
def test_faraday_seams(gpu_ctx, fix, which):
    """hey_element_kernel and hey_outer_kernel of the form, one point, quasi-resonant or not, stokes Q and V."""
    L = tn.load()
    rng = np.random.default_rng(1210 + which)
    table = 0
    s, th = 2.0, 0.9
    with time_limit(180):
        install(gpu_ctx, fix, which)
        d = seam_dist(table)
        for stokes in (1, 2):
            for qr in (0, 1):
                fixed, v = hey_seam_inputs(rng, s, th, qr, 64)
                u = hey_outer_abscissae(rng, s, th, qr, 4)
                ref = np.array([L.rimo_hey_element(ctypes.byref(d), stokes, s, th, qr, float(a), float(b)) for a, b in zip(fixed, v)])
                ref_o = np.array([L.rimo_hey_outer_integrand(ctypes.byref(d), stokes, s, th, qr, float(x)) for x in u])
                assert np.isfinite(ref).sum() > 32 and np.isfinite(ref_o).sum() >= 2
                got = gpu_ctx.hey_element_batch(TAB, [float(table)], stokes, s, th, qr, fixed, v)
                mismatch("hey_element stokes %d qr %d" % (stokes, qr), got, ref, lambda i: (fixed[i], v[i]))
                got = gpu_ctx.hey_outer_batch(TAB, [float(table)], stokes, s, th, qr, u)
                mismatch("hey_outer stokes %d qr %d" % (stokes, qr), got, ref_o, lambda i: u[i])


# ---- 4. scheduling ------------------------------------------------------------------------------------------------------
def test_scheduling_changes_no_bit(gpu_ctx, fix):
    """One row alone against the batch, and the batch without the cooperative tail (RIMPHONY_NO_ASSIST=1): same bits, same
    status words, same sample counts."""
    s, th, index = fix["s"], fix["theta"], fix["index"]
    with time_limit(300):
        for which in (0, 1):
            install(gpu_ctx, fix, which, oracle=False)
            out, st, work = first_rows(gpu_ctx, fix, 24)
            mismatch("batch", out, fix["values"][which])
            for row in (1, 8):                                       # one row of each table
                o1, s1, w1 = gpu_ctx.compute_batch(TAB, s[row:row + 1].copy(), th[row:row + 1].copy(), [index[row:row + 1].copy()], 0xFF,
                                                   want_status=True, want_work=True)
                mismatch("row %d alone" % row, o1[0], out[row])
                assert (s1[0] == st[row]).all() and (w1[0] == work[row]).all()
            ctx = env_context(RIMPHONY_NO_ASSIST="1")
            try:
                install(ctx, fix, which, oracle=False)
                o2, s2, w2 = first_rows(ctx, fix, 24)
            finally:
                ctx.close()
            mismatch("no assist", o2, out)
            assert (s2 == st).all() and (w2 == work).all()


# ---- 5. a change of form ------------------------------------------------------------------------------------------------
@SETS
def test_no_state_survives_a_change_of_form(gpu_ctx, fix, which):
    """2-D, new, 2-D; given nodes, new, given nodes; 2-D on given nodes, new, cleared, 2-D on given nodes: the second visit of a
    form returns the bits of the first (the first 6 committed rows of its fixture, sample counts included), the new form returns
    its own in between, and a batch on the cleared context is refused."""
    import tab2d_bind as t2
    from rimphony_amd import capi
    two = np.load(os.path.join(GOLDEN, "tabulated_2d_det.npz"))
    grid = np.load(os.path.join(GOLDEN, "tabulated_grid_det.npz"))
    two_grid = np.load(os.path.join(GOLDEN, "tabulated_2d_grid_det.npz"))
    n_nodes, n_mu = (int(x) for x in two["geometry"][0])
    forms = {
        "2-D": (lambda: gpu_ctx.set_tables_2d(float(two["gamma_lo"]), float(two["gamma_hi"]), t2.edge_tables_2d(n_nodes, n_mu, two["cols_0"])),
                two, two["values"][0], two["work"][0]),
        "given nodes": (lambda: gpu_ctx.set_tables_grid(*tg.fixture_set(0)), grid, grid["values"][0], grid["work"][0]),
        "2-D on given nodes": (lambda: gpu_ctx.set_tables_2d_grid(two_grid["gamma_a"], two_grid["tables_a"]), two_grid,
                               two_grid["values"][0], two_grid["work"][0]),
    }
    with time_limit(300):
        for name, (put_other, f, values, work) in forms.items():
            put_other()
            first = first_rows(gpu_ctx, f)
            install(gpu_ctx, fix, which, oracle=False)
            own = first_rows(gpu_ctx, fix)
            if name == "2-D on given nodes":
                gpu_ctx.set_tables_2d_nodes(None, None, None)
                with pytest.raises(capi.RimphonyError, match="invalid argument"):
                    first_rows(gpu_ctx, fix, mask=0x03)
            put_other()
            again = first_rows(gpu_ctx, f)
            mismatch(name + ", first visit", first[0], values[:6])
            assert (first[2].astype(np.uint64) == work[:6]).all() and np.isfinite(first[0]).any()
            mismatch(name + ", the new form in between", own[0], fix["values"][which][:6])
            assert (own[2].astype(np.uint64) == fix["work"][which][:6]).all()
            mismatch(name + ", second visit", again[0], first[0])
            assert (again[1] == first[1]).all() and (again[2] == first[2]).all()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
@SETS
def test_refusals_through_the_c_entry(gpu_ctx, fix, which):
    """What test_tabulated_2d_nodes_host.py::test_refusals has the host check refuse, through the C entry itself:
    RIMPHONY_EINVAL, and the fixture's set, installed before, still computes its bits."""
    gamma, mu, t, k = fixture_set(fix, which)
    bad = tn.refused_cases(gamma, mu, t, k)
    with time_limit(120):
        install(gpu_ctx, fix, which, oracle=False)
        codes = {name: raw_set(gpu_ctx, *args) for name, args in bad.items()}
        out, st, work = first_rows(gpu_ctx, fix)
    assert codes == {name: EINVAL for name in bad}
    mismatch("after the refusals", out, fix["values"][which][:6])
    assert (work.astype(np.uint64) == fix["work"][which][:6]).all()


# ---- 7. the objects -----------------------------------------------------------------------------------------------------
@SETS
def test_distribution_objects_carry_the_batch_bits(gpu_ctx, fix, which):
    """TabulatedDistribution2DNodes, without and with sin_k: three rows of table 0 through full_calculation() return the bits
    of the batch."""
    from rimphony_amd import api
    gamma, mu, t, k = fixture_set(fix, which)
    rows = np.flatnonzero(fix["index"] == 0)[:3]
    with time_limit(120):
        dist = api.TabulatedDistribution2DNodes(gamma, mu, t[0], sin_k=None if k is None else float(k[0]))
        calc = dist.full_calculation(gpu_ctx)
        obj = np.stack([calc.compute_all_dimensionless(float(fix["s"][r]), float(fix["theta"][r])) for r in rows])
    # (the table alone in its set: its normalisation is the same quadrature on the same words but for the table's place)
    mismatch("object", obj, fix["values"][which][rows])
