"""GPU tests of the tabulated distribution on given gamma nodes (rimphony_ctx_set_tables_grid): the coefficients,
normalisations (with P integrated on the device), calc_f values and every seam carry the bits of the grid table oracle
(tests/support/liboracle_tabgrid.so); scheduling changes no bit; no state survives a change of form; a refused set leaves
the previous one in place; the cold Juettner table the form exists for carries the oracle's bits, so the accuracy measured
on the CPU (test_tabulated_grid_host.py) is the product's.  Every test runs under a time limit of its own, and the
oracle's side of a comparison is computed before the launch."""
import contextlib
import ctypes
import faulthandler
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import tab_bind
import tab_grid_bind as tg
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
    return np.load(os.path.join(GOLDEN, "tabulated_grid_det.npz"))


def install(ctx, which, oracle=True):
    """set A (0) or B (1) in the context and, if asked, in the oracle"""
    gamma, t, g, k = tg.fixture_set(which)
    if oracle:
        assert tg.set_tables(gamma, t, g, k) == 0
    if ctx is not None:
        ctx.set_tables_grid(gamma, t, g, k)


def raw_set(ctx, gamma, log_n, log_g, sin_k):
    """rimphony_ctx_set_tables_grid as a C caller reaches it -> its return code"""
    dp = ctypes.POINTER(ctypes.c_double)
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
    if log_g is not None:
        log_g = np.ascontiguousarray(np.atleast_2d(log_g), dtype=np.float64)
    if sin_k is not None:
        sin_k = np.ascontiguousarray(sin_k, dtype=np.float64)
    return ctx.lib.rimphony_ctx_set_tables_grid(ctx.handle, log_n.shape[0], len(gamma), gamma.ctypes.data_as(dp), log_n.ctypes.data_as(dp),
                                                0 if log_g is None else log_g.shape[1], None if log_g is None else log_g.ctypes.data_as(dp),
                                                None if sin_k is None else sin_k.ctypes.data_as(dp))


# ---- 7. the fixture's rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A: log-gm1, no g", "B: jitter, 8-node rows"])
def test_fixture_rows_bit_identical(gpu_ctx, fix, which):
    """All 8 slots of the committed rows: values (NaN pattern included), per-coefficient sample counts, and the status words,
    of which the fixture holds what the values imply: ST_NONFINITE exactly where a value is NaN, ST_NORM_FAIL nowhere."""
    with time_limit(300):
        install(gpu_ctx, which, oracle=False)
        out, st, work = gpu_ctx.compute_batch(TAB, fix["s"], fix["theta"], [fix["index"]], 0xFF, want_status=True, want_work=True)
    print("set", "AB"[which], "rows", len(out), "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    assert len(out) == 24 and (np.bincount(fix["index"].astype(int)) >= 6).all()
    want = fix["values"][which]
    assert (np.isfinite(want).sum(axis=0) >= 12).all()              # every slot finite on at least half the rows
    mismatch("coefficients", out, want, lambda i: (fix["s"][i // 8], fix["theta"][i // 8], fix["index"][i // 8], i % 8))
    assert (work.astype(np.uint64) == fix["work"][which]).all()
    assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which]).all()
    assert not same_bits(fix["values"][0], fix["values"][1]).all(axis=1).any()      # the two sets differ on every row


# ---- 8. norm, P and calc_f ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_norm_and_calc_f_bit_identical(gpu_ctx, which):
    """rimphony_batch_norm_device (bad indices included; set B: P by the device's quadrature) and rimphony_calc_f_batch on
    256 (gamma, mu) pairs per table: every node and one ulp either side of it, both table ends and outside them, mu = +-1 and
    0, a mu a rounding beyond +-1, NaN in either argument."""
    rng = np.random.default_rng(812 + which)
    nodes = tg.fixture_set(which)[0]
    lo, hi = nodes[0], nodes[-1]
    gamma = np.concatenate([nodes, np.nextafter(nodes, 0.), np.nextafter(nodes, np.inf), np.exp(rng.uniform(np.log(lo), np.log(hi), 50)),
                            [lo, hi, 0.5 * (1. + lo), 2 * hi, 3.0, 3.0, 3.0, 3.0, 3.0, 50.0, np.nan, 3.0, np.nan, 1.0]])
    mu = np.concatenate([rng.uniform(-1, 1, 242),
                         [0.3, -0.3, 0.3, 0.3, -1.0, 1.0, 0.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), -0.0, 0.3, np.nan,
                          np.nan, 0.3]])
    assert len(gamma) == 256 and len(mu) == 256
    index = np.array([0.0, 1.0, 2.0, 2.0, 3.0, 0.5, -1.0, np.nan])
    with time_limit(120):
        install(gpu_ctx, which)
        ref_norm = tg.batch_norm(index)
        assert np.isfinite(ref_norm[:4]).all() and np.isnan(ref_norm[4:]).all()
        mismatch("norm", gpu_ctx.norm_batch(TAB, [index]), ref_norm)
        for table in (0, 1, 2):
            for nrm in (1.0, None):
                want = tg.dev_calc_f([float(table)], ref_norm[table] if nrm is None else nrm, gamma, mu)
                got = gpu_ctx.calc_f_batch(TAB, [float(table)], gamma, mu, nrm)
                for name, g, w in zip(("f", "dfdg", "dfdcx"), got, want):
                    mismatch("%s table %d" % (name, table), g, w, lambda i: (gamma[i], mu[i]))
            outside = (gamma < lo) | (gamma > hi)
            assert outside.sum() >= 4
            assert (got[0][outside] == 0).all() and (got[1][outside] == 0).all() and (got[2][outside] == 0).all()
            assert np.isnan(got[0][np.isnan(gamma)]).all()
            inside = ~outside & np.isfinite(gamma) & (np.abs(mu) < 1)
            assert (np.isfinite(got[0][inside]) & (got[0][inside] >= 0)).all() and (got[0][inside] > 0).sum() >= 150


# ---- 9. the seams -------------------------------------------------------------------------------------------------------
SEAM_TABLE = {0: 0, 1: 2}              # one table of each set: k = 0.5 without g; k = 3.0 with the wavy row


def seam_dist(table):
    d, st = tg.mkdist(table)
    assert st == 0 and np.isfinite(d.norm)
    return d


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_symphony_seams(gpu_ctx, which):
    """integrand_kernel_n<8>, gamma_integral_kernel<8>, n_integral_kernel<8>, deriv_probe_kernel<8> and
    gamma_contribution_kernel<8>, one point each."""
    L = tg.load()
    rng = np.random.default_rng(900 + which)
    table = SEAM_TABLE[which]
    par = [float(table)]
    s, th, coeff, stokes, lobe = 30.0, 0.9, 1, 1, 0
    with time_limit(240):
        install(gpu_ctx, which)
        d = seam_dist(table)
        n, g = harmonic_samples(rng, s, th, 200)
        ref = np.array([L.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
        assert (np.isfinite(ref) & (ref != 0)).sum() >= len(ref) // 2
        mismatch("gamma_integrand", gpu_ctx.gamma_integrand_batch(TAB, par, coeff, stokes, s, th, n, g), ref, lambda i: (n[i], g[i]))
        nmin = s * abs(math.sin(th))
        n = np.concatenate([np.floor(nmin + 1) + np.arange(8), nmin + 9 + np.exp(rng.uniform(0, 8, 8))])
        ref = np.array([L.rimo_gamma_integral(d, coeff, stokes, lobe, s, th, v) for v in n])
        assert (np.isfinite(ref) & (ref != 0)).sum() > len(n) // 2
        mismatch("gamma_integral", gpu_ctx.gamma_integral_batch(TAB, par, coeff, stokes, lobe, s, th, n), ref, lambda i: n[i])
        lo = s * math.sin(th) + 31. + rng.uniform(0., 50., 8)
        hi = lo * rng.uniform(1.05, 3., 8)
        ref = np.array([tg.n_integral(d, coeff, stokes, lobe, s, th, a, b) for a, b in zip(lo, hi)])
        assert np.isfinite(ref).sum() > 4
        mismatch("n_integral", gpu_ctx.n_integral_batch(TAB, par, coeff, stokes, lobe, s, th, lo, hi), ref, lambda i: (lo[i], hi[i]))
        n0 = np.floor(s * math.sin(th) + 31. + rng.uniform(0., 400., 8))
        ref = np.array([L.rimo_symphony_deriv_probe(ctypes.byref(d), coeff, stokes, lobe, s, th, float(x)) for x in n0])
        assert np.isfinite(ref).sum() >= 4
        mismatch("deriv_probe", gpu_ctx.deriv_probe_batch(TAB, par, coeff, stokes, lobe, s, th, n0), ref, lambda i: n0[i])
        gam = np.exp(rng.uniform(math.log(1.5), math.log(30.), 8))
        ref = np.array([L.rimo_gamma_contribution(ctypes.byref(d), 0, 0, 8., 0.9, float(x)) for x in gam])
        assert np.isfinite(ref).sum() >= 4
        mismatch("gamma_contribution", gpu_ctx.gamma_contribution_batch(TAB, par, 0, 0, 8., 0.9, gam), ref, lambda i: gam[i])


@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_faraday_seams(gpu_ctx, which):
    """hey_element_kernel<8> and hey_outer_kernel<8>, one point, quasi-resonant or not, stokes Q and V."""
    L = tg.load()
    rng = np.random.default_rng(910 + which)
    table = SEAM_TABLE[which]
    s, th = 2.0, 0.9
    with time_limit(180):
        install(gpu_ctx, which)
        d = seam_dist(table)
        for stokes in (1, 2):
            for qr in (0, 1):
                fixed, v = hey_seam_inputs(rng, s, th, qr, 64)
                ref = np.array([L.rimo_hey_element(ctypes.byref(d), stokes, s, th, qr, float(a), float(b)) for a, b in zip(fixed, v)])
                assert np.isfinite(ref).sum() > 32
                got = gpu_ctx.hey_element_batch(TAB, [float(table)], stokes, s, th, qr, fixed, v)
                mismatch("hey_element stokes %d qr %d" % (stokes, qr), got, ref, lambda i: (fixed[i], v[i]))
                u = hey_outer_abscissae(rng, s, th, qr, 4)
                ref = np.array([L.rimo_hey_outer_integrand(ctypes.byref(d), stokes, s, th, qr, float(x)) for x in u])
                assert np.isfinite(ref).sum() >= 2
                got = gpu_ctx.hey_outer_batch(TAB, [float(table)], stokes, s, th, qr, u)
                mismatch("hey_outer stokes %d qr %d" % (stokes, qr), got, ref, lambda i: u[i])


# ---- 10. scheduling -----------------------------------------------------------------------------------------------------
def test_scheduling_changes_no_bit(gpu_ctx, fix):
    """The fixture's rows on the group kernel (RIMPHONY_TAB_GROUP=1), one wave per coefficient (=0), the default, and
    without the cooperative tail (RIMPHONY_NO_ASSIST=1): same bits, same status words, same sample counts."""
    s, th, index = fix["s"], fix["theta"], fix["index"]
    runs = {}
    with time_limit(300):
        for which in (0, 1):
            install(gpu_ctx, which, oracle=False)
            runs["default", which] = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
            for name, env in (("group", {"RIMPHONY_TAB_GROUP": "1"}), ("solo", {"RIMPHONY_TAB_GROUP": "0"}),
                              ("no assist", {"RIMPHONY_NO_ASSIST": "1"})):
                ctx = env_context(**env)
                try:
                    install(ctx, which, oracle=False)
                    runs[name, which] = ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
                finally:
                    ctx.close()
    for (name, which), (out, st, work) in runs.items():
        mismatch("%s set %s" % (name, "AB"[which]), out, fix["values"][which])
        assert (work.astype(np.uint64) == fix["work"][which]).all(), (name, which)
        assert (st == runs["default", which][1]).all(), (name, which)


# ---- 11. a change of form -----------------------------------------------------------------------------------------------
def test_no_state_survives_a_change_of_form(gpu_ctx, fix):
    """uniform, then grid (set A), then 2-D, then grid (set B), then cleared: after each install the first 6 committed rows of
    that form's fixture come back bit for bit, sample counts included, and a batch after clearing is refused.  A refused
    rimphony_ctx_set_tables_grid -- nodes that do not increase, nodes whose logarithms coincide -- leaves the previous set
    computing its own bits."""
    import tab2d_bind as t2
    from rimphony_amd import capi
    iso = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))
    two = np.load(os.path.join(GOLDEN, "tabulated_2d_det.npz"))
    n_nodes, n_mu = (int(x) for x in two["geometry"][0])
    steps = (
        ("uniform", lambda: gpu_ctx.set_tables(float(iso["gamma_lo"]), float(iso["gamma_hi"]), iso["tables"]),
         iso, iso["values"], iso["work"]),
        ("grid A", lambda: install(gpu_ctx, 0, oracle=False), fix, fix["values"][0], fix["work"][0]),
        ("2-D", lambda: gpu_ctx.set_tables_2d(float(two["gamma_lo"]), float(two["gamma_hi"]), t2.edge_tables_2d(n_nodes, n_mu, two["cols_0"])),
         two, two["values"][0], two["work"][0]),
        ("grid B", lambda: install(gpu_ctx, 1, oracle=False), fix, fix["values"][1], fix["work"][1]),
    )
    gamma, t, g, k = tg.fixture_set(1)
    swapped = gamma.copy()
    swapped[[20, 21]] = swapped[[21, 20]]
    close = gamma.copy()
    close[30] = np.nextafter(close[29], np.inf)
    assert close[29] < close[30] < close[31] and math.log(close[29]) == math.log(close[30])
    got = []
    with time_limit(300):
        for name, put, f, values, work in steps:
            put()
            got.append(gpu_ctx.compute_batch(TAB, f["s"][:6].copy(), f["theta"][:6].copy(), [f["index"][:6].copy()], 0xFF,
                                             want_status=True, want_work=True))
        refused = [raw_set(gpu_ctx, swapped, t, g, k), raw_set(gpu_ctx, close, t, g, k)]
        after = gpu_ctx.compute_batch(TAB, fix["s"][:6].copy(), fix["theta"][:6].copy(), [fix["index"][:6].copy()], 0xFF)
        gpu_ctx.set_tables_grid(None, None)
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.compute_batch(TAB, fix["s"][:6].copy(), fix["theta"][:6].copy(), [fix["index"][:6].copy()], 0x03)
    for (name, put, f, values, work), (out, st, w) in zip(steps, got):
        mismatch(name, out, values[:6])
        assert (w.astype(np.uint64) == work[:6]).all(), name
        assert np.isfinite(out).any()
    assert refused == [EINVAL, EINVAL]
    mismatch("after the refusals", after, fix["values"][1][:6])


# ---- 12. the case the form is for ---------------------------------------------------------------------------------------
def test_cold_juettner_rows_carry_the_oracle_bits(gpu_ctx):
    """T = 0.1 Juettner on [1 + 1e-6, 31], 512 nodes uniform in ln(gamma - 1), the six rows of test_tabulated_grid_host.py:
    the GPU returns the CPU oracle's bits, so the accuracy measured there is the product's.  The same rows through
    TabulatedDistributionGrid.from_function(...).full_calculation() agree with Context.set_tables_grid + compute_batch."""
    from rimphony_amd import api
    gamma = tg.cold_grid(512)
    log_n = tab_bind.log_n_juettner(gamma, tg.COLD_T)
    with time_limit(300):
        assert tg.set_tables(gamma, log_n) == 0
        ref, ref_work = tg.batch(tg.COLD_S, tg.COLD_THETA, np.zeros(6))
        gpu_ctx.set_tables_grid(gamma, log_n)
        out, st, work = gpu_ctx.compute_batch(TAB, tg.COLD_S, tg.COLD_THETA, [np.zeros(6)], 0xFF, want_status=True, want_work=True)
        dist = api.TabulatedDistributionGrid.from_function(lambda x: np.exp(tab_bind.log_n_juettner(x, tg.COLD_T)), gamma)
        calc = dist.full_calculation(gpu_ctx)
        obj = np.stack([calc.compute_all_dimensionless(float(s), float(th)) for s, th in zip(tg.COLD_S, tg.COLD_THETA)])
    print("NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    mismatch("cold Juettner", out, ref)
    assert (work.astype(np.uint64) == ref_work).all()
    assert np.isfinite(out).sum() >= 44
    mismatch("from_function", obj, out)


# ---- 13. the C++ mirror -------------------------------------------------------------------------------------------------
def test_cxx_mirror_builds_and_runs(tmp_path, gpu_ctx, fix):
    """rimphony.hpp's Context::set_tables_grid and TabulatedDistributionGrid compile and compute one row equal to the Python
    path: the program reads the nodes and the table as hexadecimal floats and prints the row likewise."""
    exe = tmp_path / "grid_row"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "support", "cxx_grid_row.cpp"),
                    "-L", os.path.join(ROOT, "rimphony_amd"), "-lrimphony_hip", "-Wl,-rpath," + os.path.join(ROOT, "rimphony_amd"),
                    "-o", str(exe)], check=True)
    gamma, t, g, k = tg.fixture_set(0)
    table, s, th = 0, float(fix["s"][0]), float(fix["theta"][0])
    assert fix["index"][0] == table
    data = tmp_path / "table.txt"
    data.write_text("%d\n%s\n%s\n%s %s %s\n" % (len(gamma), " ".join(float(x).hex() for x in gamma), " ".join(float(x).hex() for x in t[table]),
                                                float(k[table]).hex(), s.hex(), th.hex()))
    with time_limit(120):
        r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [np.array([float.fromhex(x) for x in line.split()]) for line in r.stdout.strip().splitlines()]
    assert len(rows) == 2 and len(rows[0]) == 8
    mismatch("Context::set_tables_grid + BatchCalculator", rows[0], fix["values"][0][0])
    mismatch("TabulatedDistributionGrid", rows[1], fix["values"][0][0])
