"""GPU tests of the tabulated distribution as 2-D sets on given gamma nodes (rimphony_ctx_set_tables_2d_grid): the
coefficients, the normalisations integrated on the device, calc_f values and the seams carry the bits of the form's table
oracle (tests/support/liboracle_tab2dgrid.so); routing and scheduling change no bit; no state survives a change of form; a
refused set leaves the previous one in place; the cold table the form exists for carries the oracle's bits, so the accuracy
measured on the CPU (test_tabulated_2d_grid_host.py) is the product's.  Every test runs under a time limit of its own, and
the oracle's side of a comparison is computed before the launch.  The oracle's normalisations of the fixture's sets are the
fixture's record of them (set B's quadrature takes the CPU ten seconds); the GPU integrates its own."""
import contextlib
import ctypes
import faulthandler
import os
import sys

import numpy as np
import pytest

import tab_bind
import tab_grid_bind as tg
import tab2d_grid_bind as tq
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL = -1
ST_NONFINITE, ST_NORM_FAIL = 16, 32
TAB = 4
SETS = pytest.mark.parametrize("which", [0, 1], ids=["A: 64 log-gm1 x 8", "B: 16 jitter x 1024"])


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
    return np.load(os.path.join(GOLDEN, "tabulated_2d_grid_det.npz"))


def fixture_set(fix, which):
    return (fix["gamma_a"], fix["tables_a"]) if which == 0 else (fix["gamma_b"], fix["tables_b"])


def install(ctx, fix, which, oracle=True):
    """set A (0) or B (1) of the fixture in the context and, if asked, in the oracle (with the recorded normalisations)"""
    gamma, t = fixture_set(fix, which)
    if oracle:
        assert tq.set_tables(gamma, t, with_norm=False) == 0 and tq.put_norms(fix["norms"][which]) == 0
    if ctx is not None:
        ctx.set_tables_2d_grid(gamma, t)


def raw_set(ctx, gamma, log_n, shape=None):
    """rimphony_ctx_set_tables_2d_grid as a C caller reaches it -> its return code; shape: what the call states"""
    dp = ctypes.POINTER(ctypes.c_double)
    nt, nn, nmu, gamma, log_n = tq._args(gamma, log_n, shape)
    return ctx.lib.rimphony_ctx_set_tables_2d_grid(ctx.handle, nt, nn, None if gamma is None else gamma.ctypes.data_as(dp), nmu,
                                                   None if log_n is None else log_n.ctypes.data_as(dp))


def first_rows(ctx, f, n=6, mask=0xFF):
    return ctx.compute_batch(TAB, f["s"][:n].copy(), f["theta"][:n].copy(), [f["index"][:n].copy()], mask, want_status=True, want_work=True)


# ---- 1. the fixture's rows ----------------------------------------------------------------------------------------------
@SETS
def test_fixture_rows_bit_identical(gpu_ctx, fix, which):
    """All 8 slots of the committed rows under the default routing and with RIMPHONY_TAB_GROUP=0 in a context of its own:
    values (NaN pattern included), per-coefficient sample counts, ST_NONFINITE exactly where a value is NaN, ST_NORM_FAIL
    nowhere; the same bits both ways."""
    want = fix["values"][which]
    assert (np.bincount(fix["index"].astype(int)) >= 6).all() and (np.isfinite(want).sum(axis=0) >= 12).all()
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
        print("set", "AB"[which], name, "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
        mismatch(name, out, want, lambda i: (fix["s"][i // 8], fix["theta"][i // 8], fix["index"][i // 8], i % 8))
        assert (work.astype(np.uint64) == fix["work"][which]).all(), name
        assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which]).all(), name


# ---- 2, 3. norm and calc_f ----------------------------------------------------------------------------------------------
@SETS
def test_norm_and_calc_f_bit_identical(gpu_ctx, fix, which):
    """The tables' normalisations as the device integrated them, bad indices (3.0, 0.5, -1, NaN -> NaN) included, and
    rimphony_calc_f_batch on 256 (gamma, mu) pairs per table: every node and one ulp either side of it, both ends and outside
    them, mu = +-1 and 0, a mu a rounding beyond +-1, NaN in either argument."""
    rng = np.random.default_rng(912 + which)
    nodes = fixture_set(fix, which)[0]
    lo, hi = nodes[0], nodes[-1]
    gamma = np.concatenate([nodes, np.nextafter(nodes, 0.), np.nextafter(nodes, np.inf),
                            np.exp(rng.uniform(np.log(lo), np.log(hi), 242 - 3 * len(nodes))),
                            [lo, hi, 0.5 * (1. + lo), 2 * hi, 3.0, 3.0, 3.0, 3.0, 3.0, 50.0, np.nan, 3.0, np.nan, 1.0]])
    mu = np.concatenate([rng.uniform(-1, 1, 242),
                         [0.3, -0.3, 0.3, 0.3, -1.0, 1.0, 0.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), -0.0, 0.3, np.nan,
                          np.nan, 0.3]])
    assert len(gamma) == 256 and len(mu) == 256
    index = np.array([0.0, 1.0, 2.0, 2.0, 3.0, 0.5, -1.0, np.nan])
    with time_limit(120):
        install(gpu_ctx, fix, which)
        ref_norm = tq.batch_norm(index)
        assert np.isfinite(ref_norm[:4]).all() and np.isnan(ref_norm[4:]).all() and (ref_norm[:3] == fix["norms"][which]).all()
        want = {(table, nrm): tq.dev_calc_f([float(table)], ref_norm[table] if nrm is None else nrm, gamma, mu)
                for table in (0, 1, 2) for nrm in (1.0, None)}
        mismatch("norm", gpu_ctx.norm_batch(TAB, [index]), ref_norm)
        for (table, nrm), w in want.items():
            got = gpu_ctx.calc_f_batch(TAB, [float(table)], gamma, mu, nrm)
            for name, g, r in zip(("f", "dfdg", "dfdcx"), got, w):
                mismatch("%s table %d" % (name, table), g, r, lambda i: (gamma[i], mu[i]))
            outside = (gamma < lo) | (gamma > hi)
            assert outside.sum() >= 4
            assert (got[0][outside] == 0).all() and (got[1][outside] == 0).all() and (got[2][outside] == 0).all()
            assert np.isnan(got[0][np.isnan(gamma)]).all() and np.isnan(got[0][np.isnan(mu) & ~outside]).all()
            inside = ~outside & np.isfinite(gamma) & np.isfinite(mu)
            assert (np.isfinite(got[0][inside]) & (got[0][inside] >= 0)).all() and (got[0][inside] > 0).sum() >= 150


# ---- 4. the seams -------------------------------------------------------------------------------------------------------
def seam_dist(table):
    d, st = tq.mkdist(table)
    assert st == 0 and np.isfinite(d.norm)
    return d


@SETS
def test_symphony_seams(gpu_ctx, fix, which):
    """integrand_kernel_n<9> and gamma_integral_kernel<9>, one point, on table 2 (curved, non-separable)"""
    import math
    L = tq.load()
    rng = np.random.default_rng(900 + which)
    table, par = 2, [2.0]
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
    """hey_element_kernel<9> and hey_outer_kernel<9>, one point, quasi-resonant or not, stokes Q and V."""
    L = tq.load()
    rng = np.random.default_rng(910 + which)
    table = 2
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


# ---- 5. scheduling ------------------------------------------------------------------------------------------------------
def test_scheduling_changes_no_bit(gpu_ctx, fix):
    """One row alone against the batch, and the batch without the cooperative tail (RIMPHONY_NO_ASSIST=1): same bits, same
    status words, same sample counts."""
    s, th, index = fix["s"], fix["theta"], fix["index"]
    with time_limit(300):
        for which in (0, 1):
            install(gpu_ctx, fix, which, oracle=False)
            out, st, work = first_rows(gpu_ctx, fix, 24)
            mismatch("batch", out, fix["values"][which])
            for row in (1, 8, 15):                                   # one row of each table
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


# ---- 6. a change of form ------------------------------------------------------------------------------------------------
def test_no_state_survives_a_change_of_form(gpu_ctx, fix):
    """2-D, new, 2-D; given nodes, new, given nodes; isotropic, new, cleared, isotropic: the second visit of a form returns the
    bits of the first (the first 6 committed rows of its fixture, sample counts included), the new form returns its own in
    between, and a batch on the cleared context is refused."""
    import tab2d_bind as t2
    from rimphony_amd import capi
    iso = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))
    two = np.load(os.path.join(GOLDEN, "tabulated_2d_det.npz"))
    grid = np.load(os.path.join(GOLDEN, "tabulated_grid_det.npz"))
    n_nodes, n_mu = (int(x) for x in two["geometry"][0])
    forms = {
        "2-D": (lambda: gpu_ctx.set_tables_2d(float(two["gamma_lo"]), float(two["gamma_hi"]), t2.edge_tables_2d(n_nodes, n_mu, two["cols_0"])),
                two, two["values"][0], two["work"][0]),
        "given nodes": (lambda: gpu_ctx.set_tables_grid(*tg.fixture_set(0)), grid, grid["values"][0], grid["work"][0]),
        "isotropic": (lambda: gpu_ctx.set_tables(float(iso["gamma_lo"]), float(iso["gamma_hi"]), iso["tables"]), iso, iso["values"], iso["work"]),
    }
    with time_limit(300):
        for name, (put, f, values, work) in forms.items():
            which = 0 if name == "given nodes" else 1
            put()
            first = first_rows(gpu_ctx, f)
            install(gpu_ctx, fix, which, oracle=False)
            own = first_rows(gpu_ctx, fix)
            if name == "isotropic":
                gpu_ctx.set_tables_2d_grid(None, None)
                with pytest.raises(capi.RimphonyError, match="invalid argument"):
                    first_rows(gpu_ctx, fix, mask=0x03)
            put()
            again = first_rows(gpu_ctx, f)
            mismatch(name + ", first visit", first[0], values[:6])
            assert (first[2].astype(np.uint64) == work[:6]).all() and np.isfinite(first[0]).any()
            mismatch(name + ", the new form in between", own[0], fix["values"][which][:6])
            assert (own[2].astype(np.uint64) == fix["work"][which][:6]).all()
            mismatch(name + ", second visit", again[0], first[0])
            assert (again[1] == first[1]).all() and (again[2] == first[2]).all()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_entry(gpu_ctx, fix):
    """Everything test_tabulated_2d_grid_host.py::test_refusals has the host check refuse, through
    rimphony_ctx_set_tables_2d_grid itself: RIMPHONY_EINVAL, and set A, installed before, still computes its bits."""
    g = tg.grid("jitter")
    t = tq.surfaces_at(g, 16)
    bad = {"null gamma": (None, t, (3, 64, 16)), "null log_n": (g, None, (3, 64, 16))}
    for name, v in (("NaN", np.nan), ("inf", np.inf), ("-inf", -np.inf)):
        gb, tb = g.copy(), t.copy()
        gb[3], tb[1, 5, 3] = v, v
        bad["gamma " + name], bad["value " + name] = (gb, t, None), (g, tb, None)
    low, same, swapped, close = g.copy(), g.copy(), g.copy(), g.copy()
    low[0] = np.nextafter(1.0, 0.0)
    same[21] = same[20]
    swapped[[20, 21]] = swapped[[21, 20]]
    close[30] = np.nextafter(close[29], np.inf)
    assert close[29] > 3 and close[29] < close[30] < close[31] and tq.rim_log(close[29:31])[0] == tq.rim_log(close[29:31])[1]
    many, g1025 = tab_bind.nodes(1.01, 1e4, 65537), tab_bind.nodes(1.01, 1e4, 1025)
    bad.update({"gamma_0 < 1": (low, t, None), "equal nodes": (same, t, None), "swapped nodes": (swapped, t, None),
                "equal logarithms": (close, t, None), "7 gamma nodes": (g[:7], t[:, :7], None),
                "65537 gamma nodes": (many, np.zeros((1, 65537, 8)), None), "7 mu nodes": (g, t[:, :, :7], None),
                "1025 mu nodes": (g[:16], np.zeros((1, 16, 1025)), None), "over 2^20 nodes": (g1025, np.zeros((1, 1025, 1024)), None)})
    with time_limit(120):
        install(gpu_ctx, fix, 0, oracle=False)
        codes = {name: raw_set(gpu_ctx, *args) for name, args in bad.items()}
        out, st, work = first_rows(gpu_ctx, fix)
    assert codes == {name: EINVAL for name in bad}
    mismatch("after the refusals", out, fix["values"][0][:6])
    assert (work.astype(np.uint64) == fix["work"][0][:6]).all()


# ---- 8. the case the form is for ----------------------------------------------------------------------------------------
def test_cold_table_rows_carry_the_oracle_bits(gpu_ctx):
    """T = 0.1 Juettner on [1 + 1e-6, 31], 512 nodes uniform in ln(gamma - 1) x 8 mu nodes, the six rows of
    test_tabulated_2d_grid_host.py: the GPU returns the CPU oracle's bits, normalisation included, so the accuracy measured
    there is the product's.  The same rows through TabulatedDistribution2DGrid.full_calculation() agree."""
    from rimphony_amd import api
    gamma = tg.cold_grid(512)
    log_n = tq.cold_table(gamma)
    with time_limit(300):
        assert tq.set_tables(gamma, log_n) == 0
        ref, ref_work = tq.batch(tg.COLD_S, tg.COLD_THETA, np.zeros(6))
        ref_norm = tq.batch_norm([0.0])
        gpu_ctx.set_tables_2d_grid(gamma, log_n)
        norm = gpu_ctx.norm_batch(TAB, [np.zeros(1)])
        out, st, work = gpu_ctx.compute_batch(TAB, tg.COLD_S, tg.COLD_THETA, [np.zeros(6)], 0xFF, want_status=True, want_work=True)
        calc = api.TabulatedDistribution2DGrid(gamma, log_n).full_calculation(gpu_ctx)
        obj = np.stack([calc.compute_all_dimensionless(float(s), float(th)) for s, th in zip(tg.COLD_S, tg.COLD_THETA)])
    print("NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    mismatch("norm", norm, ref_norm)
    mismatch("cold table", out, ref)
    assert (work.astype(np.uint64) == ref_work).all()
    assert np.isfinite(out).sum() >= 46 and not (st & ST_NORM_FAIL).any()
    mismatch("TabulatedDistribution2DGrid", obj, out)
