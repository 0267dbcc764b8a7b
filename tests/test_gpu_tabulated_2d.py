"""GPU tests of the tabulated distribution on 2-D table sets, ln n(gamma, mu) on a grid (rimphony_ctx_set_tables_2d): the
coefficients, the per-table normalisations, calc_f values and the seams carry the bits of the 2-D oracle
(tests/support/liboracle_tab2d.so); an isotropic or a pitch set gives the same bits before and after a 2-D set has used the
context; misuse is refused and leaves the previous set in place.  (What the oracle's surface is held to:
test_tabulated_2d_host.py.)  Every test runs under a time limit of its own, and the oracle's side of a comparison is
computed before the launch."""
import contextlib
import ctypes
import faulthandler
import math
import os
import sys

import numpy as np
import pytest

import tab2d_bind as t2
import tab_pitch_bind as tp
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_2d_det.npz")
PITCH_FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_pitch_det.npz")
EINVAL = -1
ST_NONFINITE, ST_NORM_FAIL = 16, 32
TAB = 4
ENTRY = "rimphony_ctx_set_tables_2d"


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
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def pitch_fix():
    return np.load(PITCH_FIXTURE)


def tables_of(fix, which):
    """the fixture's three-table set of geometry `which`, rebuilt from the stored gamma-node columns"""
    n_nodes, n_mu = (int(x) for x in fix["geometry"][which])
    return t2.edge_tables_2d(n_nodes, n_mu, fix["cols_%d" % which])


_oracle_has = [None]


def install(ctx, fix, which, oracle=True):
    """the fixture's set of geometry `which` in the context and, unless it holds it already, in the oracle"""
    glo, ghi, t = float(fix["gamma_lo"]), float(fix["gamma_hi"]), tables_of(fix, which)
    if oracle and _oracle_has[0] != which:
        assert t2.set_tables(glo, ghi, t) == 0
        _oracle_has[0] = which
    if ctx is not None:
        ctx.set_tables_2d(glo, ghi, t)


def raw_set(ctx, glo, ghi, log_n, shape=None):
    """rimphony_ctx_set_tables_2d as a C caller reaches it -> its return code.  shape: the (n_tables, n_nodes, n_mu) the
    call states (default: log_n's own); the buffer covers it"""
    dp = ctypes.POINTER(ctypes.c_double)
    t = t2.as_set(log_n) if shape is None else np.ascontiguousarray(log_n, dtype=np.float64)
    nt, nn, nmu = t.shape if shape is None else shape
    return ctx.lib.rimphony_ctx_set_tables_2d(ctx.handle, nt, nn, float(glo), float(ghi), nmu, t.ctypes.data_as(dp))


def refusals(t):
    """(log_n, shape, gamma_lo, gamma_hi) of every set the entry refuses; t: a good [3][16][16] set over [1.01, 1e4]"""
    nan_t, inf_t = t.copy(), t.copy()
    nan_t[1, 5, 3], inf_t[2, 0, 15] = np.nan, -np.inf
    big = np.zeros(1025 * 1024)
    return ((t, (3, 16, 7), 1.01, 1e4), (big, (1, 16, 1025), 1.01, 1e4), (t, (3, 7, 16), 1.01, 1e4),
            (big, (1, 1025, 1024), 1.01, 1e4),                # one gamma node's worth over 2^20 nodes
            (nan_t, None, 1.01, 1e4), (inf_t, None, 1.01, 1e4),
            (t, None, 0.5, 1e4), (t, None, 10.0, 10.0), (t, None, 10.0, 5.0))


@pytest.mark.parametrize("which", [0, 1], ids=["64x8", "16x1024"])
def test_fixture_rows_bit_identical(gpu_ctx, fix, which):
    """All 8 slots of the committed rows: values (NaN pattern included), per-coefficient sample counts, and the status words,
    of which the fixture holds what the values imply: ST_NONFINITE exactly where a value is NaN, ST_NORM_FAIL nowhere."""
    with time_limit(300):
        install(gpu_ctx, fix, which, oracle=False)
        out, st, work = gpu_ctx.compute_batch(TAB, fix["s"], fix["theta"], [fix["index"]], 0xFF, want_status=True, want_work=True)
    print(fix["geometry"][which], "rows", len(out), "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    assert len(out) == 24
    want = fix["values"][which]
    assert np.isfinite(want).any(axis=0).all() and np.isfinite(want).mean() >= 0.9
    mismatch("coefficients", out, want, lambda i: (fix["s"][i // 8], fix["theta"][i // 8], fix["index"][i // 8], i % 8))
    assert (work.astype(np.uint64) == fix["work"][which]).all()
    assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which]).all()
    # the geometry is in the numbers: the rows of the two sets differ
    assert not same_bits(fix["values"][0], fix["values"][1]).all(axis=1).any()


def test_norm_and_calc_f_bit_identical(gpu_ctx, fix):
    """rimphony_batch_norm_device (bad indices included) against the oracle's installation-time quadrature, and
    rimphony_calc_f_batch on 256 (gamma, mu) pairs per table: mu = +-1, 0 and -0, a mu a rounding beyond +-1, gamma at and
    outside both table ends."""
    rng = np.random.default_rng(12)
    lo, hi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
    gamma = np.concatenate([np.exp(rng.uniform(np.log(lo), np.log(hi), 244)),
                            [lo, hi, np.nextafter(lo, 0.), np.nextafter(hi, np.inf), 0.5 * lo, 2 * hi, 3.0, 3.0, 3.0, 3.0, 3.0, 50.0]])
    mu = np.concatenate([rng.uniform(-1, 1, 244),
                         [0.3, -0.3, 0.3, 0.3, 0.3, 0.3, -1.0, 1.0, 0.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), -0.0]])
    assert len(gamma) == 256 and len(mu) == 256
    index = np.array([0.0, 1.0, 2.0, 2.0, 3.0, 0.5, -1.0, np.nan])
    for which in (0, 1):
        with time_limit(120):
            install(None, fix, which)
            ref_norm = t2.batch_norm(index)
            assert np.isfinite(ref_norm[:4]).all() and np.isnan(ref_norm[4:]).all()
            assert same_bits(ref_norm[:3], fix["norm"][which]).all()
            want = {(table, nrm): t2.dev_calc_f([float(table)], ref_norm[table] if nrm is None else nrm, gamma, mu)
                    for table in (0, 1, 2) for nrm in (1.0, None)}
            install(gpu_ctx, fix, which)
            mismatch("norm geometry %d" % which, gpu_ctx.norm_batch(TAB, [index]), ref_norm)
            for table in (0, 1, 2):
                for nrm in (1.0, None):
                    got = gpu_ctx.calc_f_batch(TAB, [float(table)], gamma, mu, nrm)
                    for name, g, w in zip(("f", "dfdg", "dfdcx"), got, want[(table, nrm)]):
                        mismatch("%s table %d geometry %d" % (name, table, which), g, w, lambda i: (gamma[i], mu[i]))
                inside = (gamma >= lo) & (gamma <= hi)
                assert (got[0][~inside] == 0).all() and (got[1][~inside] == 0).all() and (got[2][~inside] == 0).all()
                assert (got[0][inside] > 0).sum() >= 200
                if table == 1:
                    assert (got[2] == 0).all()                                  # no mu dependence
                else:
                    assert (got[2][inside] != 0).sum() >= 200                   # a live d f / d mu


LIVE_TABLES = (0, 2)           # the tables of the set that depend on mu


def live_dist(table):
    d, st = t2.mkdist(table)
    assert st == 0 and np.isfinite(d.norm)
    return d


def test_gamma_integrand_seam(gpu_ctx, fix):
    """integrand_kernel_n<6>: absorption, whose d f / d mu term takes the general form, in Stokes I, Q and V, and emission."""
    L = t2.load()
    rng = np.random.default_rng(604)
    cases = ((0, 100.0, 0.3, 1, 0), (2, 100.0, 1.5, 1, 1), (2, 30.0, 0.9, 1, 2), (0, 30.0, 0.9, 0, 0))
    with time_limit(120):
        install(None, fix, 0)
        refs = []
        for table, s, th, coeff, stokes in cases:
            d = live_dist(table)
            n, g = harmonic_samples(rng, s, th, 200)
            ref = np.array([L.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
            assert (np.isfinite(ref) & (ref != 0)).sum() >= len(ref) // 2
            refs.append((n, g, ref))
        install(gpu_ctx, fix, 0)
        for (table, s, th, coeff, stokes), (n, g, ref) in zip(cases, refs):
            got = gpu_ctx.gamma_integrand_batch(TAB, [float(table)], coeff, stokes, s, th, n, g)
            mismatch("gamma_integrand table %d" % table, got, ref, lambda i: (s, th, coeff, stokes, n[i], g[i]))


def test_gamma_integral_seam(gpu_ctx, fix):
    """gamma_integral_kernel<6>: the first 8 harmonics and 8 further out, on the set with 1024 mu nodes."""
    L = t2.load()
    rng = np.random.default_rng(605)
    cases = (((0, 30.0, 0.9), (1, 0, 0)), ((2, 12.0, 1.2), (1, 2, 1)))
    with time_limit(120):
        install(None, fix, 1)
        refs = []
        for (table, s, th), (coeff, stokes, lobe) in cases:
            d = live_dist(table)
            nmin = s * abs(math.sin(th))
            n = np.concatenate([np.floor(nmin + 1) + np.arange(8), nmin + 9 + np.exp(rng.uniform(0, 8, 8))])
            ref = np.array([L.rimo_gamma_integral(d, coeff, stokes, lobe, s, th, v) for v in n])
            assert (np.isfinite(ref) & (ref != 0)).sum() > len(n) // 2
            refs.append((n, ref))
        install(gpu_ctx, fix, 1)
        for ((table, s, th), (coeff, stokes, lobe)), (n, ref) in zip(cases, refs):
            got = gpu_ctx.gamma_integral_batch(TAB, [float(table)], coeff, stokes, lobe, s, th, n)
            mismatch("gamma_integral table %d" % table, got, ref, lambda i: (s, th, n[i], lobe))


HEY_POINTS = ((2.0, 0.9), (60.0, 1.1))        # as test_gpu_tabulated.py: the J/Y branch, and the large-order branches


@pytest.mark.parametrize("table", LIVE_TABLES)
def test_faraday_seams(gpu_ctx, fix, table):
    """hey_element_kernel<6> and hey_outer_kernel<6>, quasi-resonant or not, Stokes Q and V: the mu term of d f / d sigma."""
    L = t2.load()
    rng = np.random.default_rng(610 + table)
    with time_limit(180):
        install(None, fix, 0)
        d = live_dist(table)
        refs = []
        for s, th in HEY_POINTS:
            for stokes in (1, 2):
                for qr in (0, 1):
                    fixed, v = hey_seam_inputs(rng, s, th, qr, 64)
                    ref_e = np.array([L.rimo_hey_element(ctypes.byref(d), stokes, s, th, qr, float(a), float(b)) for a, b in zip(fixed, v)])
                    assert np.isfinite(ref_e).sum() > 32
                    u = hey_outer_abscissae(rng, s, th, qr, 6)
                    ref_o = np.array([L.rimo_hey_outer_integrand(ctypes.byref(d), stokes, s, th, qr, float(x)) for x in u])
                    assert np.isfinite(ref_o).sum() >= 3
                    refs.append((s, th, stokes, qr, fixed, v, ref_e, u, ref_o))
        install(gpu_ctx, fix, 0)
        for s, th, stokes, qr, fixed, v, ref_e, u, ref_o in refs:
            got = gpu_ctx.hey_element_batch(TAB, [float(table)], stokes, s, th, qr, fixed, v)
            mismatch("hey_element table %d s %g stokes %d qr %d" % (table, s, stokes, qr), got, ref_e, lambda i: (fixed[i], v[i]))
            got = gpu_ctx.hey_outer_batch(TAB, [float(table)], stokes, s, th, qr, u)
            mismatch("hey_outer table %d s %g stokes %d qr %d" % (table, s, stokes, qr), got, ref_o, lambda i: u[i])


@pytest.mark.parametrize("around", ["isotropic", "pitch"])
def test_no_state_survives(gpu_ctx, fix, pitch_fix, around):
    """One context: an isotropic (or a pitch) set, then a 2-D set, then the first set again.  The third results are the
    first, bit for bit -- and the committed ones of the pitch fixture --; the second are the 2-D fixture's."""
    s, th, index = fix["s"], fix["theta"], fix["index"]
    ps, pth, pindex = pitch_fix["s"], pitch_fix["theta"], pitch_fix["index"]
    glo, ghi = float(pitch_fix["gamma_lo"]), float(pitch_fix["gamma_hi"])
    G = tp.edge_pitch(8) if around == "pitch" else None
    with time_limit(300):
        gpu_ctx.set_tables(glo, ghi, pitch_fix["tables"], G)
        first = gpu_ctx.compute_batch(TAB, ps, pth, [pindex], 0xFF, want_status=True, want_work=True)
        norm1 = gpu_ctx.norm_batch(TAB, [np.arange(3.0)])
        install(gpu_ctx, fix, 0, oracle=False)
        second = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        gpu_ctx.set_tables(glo, ghi, pitch_fix["tables"], G)
        third = gpu_ctx.compute_batch(TAB, ps, pth, [pindex], 0xFF, want_status=True, want_work=True)
        norm3 = gpu_ctx.norm_batch(TAB, [np.arange(3.0)])
    assert same_bits(first[0], third[0]).all() and (first[1] == third[1]).all() and (first[2] == third[2]).all()
    assert same_bits(norm1, norm3).all() and np.isfinite(norm1).all()
    if around == "pitch":
        mismatch("the pitch fixture's rows", first[0], pitch_fix["values"][0])
    else:
        assert np.isfinite(first[0]).mean() >= 0.9
    mismatch("second", second[0], fix["values"][0])
    assert (second[2].astype(np.uint64) == fix["work"][0]).all()


def test_batch_size_and_cooperative_tail_change_no_bit(gpu_ctx, fix):
    """One row against all rows, and a context without the cooperative tail (RIMPHONY_NO_ASSIST=1): same bits, same status
    words, same sample counts."""
    glo, ghi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
    s, th, index = fix["s"], fix["theta"], fix["index"]
    with time_limit(300):
        install(gpu_ctx, fix, 0, oracle=False)
        big = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        ones = [gpu_ctx.compute_batch(TAB, s[i:i + 1], th[i:i + 1], [index[i:i + 1]], 0xFF, want_status=True, want_work=True)
                for i in (0, 17)]
        solo_ctx = env_context(RIMPHONY_NO_ASSIST="1")
        try:
            solo_ctx.set_tables_2d(glo, ghi, tables_of(fix, 0))
            solo = solo_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        finally:
            solo_ctx.close()
    mismatch("all rows", big[0], fix["values"][0])
    for i, one in zip((0, 17), ones):
        assert same_bits(big[0][i:i + 1], one[0]).all() and (big[1][i:i + 1] == one[1]).all() and (big[2][i:i + 1] == one[2]).all(), i
    assert same_bits(big[0], solo[0]).all() and (big[1] == solo[1]).all() and (big[2] == solo[2]).all()


def test_misuse_on_a_live_context(gpu_ctx, fix):
    from rimphony_amd import api, capi
    s, th, index = fix["s"][:6].copy(), fix["theta"][:6].copy(), fix["index"][:6].copy()
    good = t2.edge_tables_2d(16, 16)
    with time_limit(300):
        install(gpu_ctx, fix, 0, oracle=False)
        before = gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)
        mismatch("before", before[:, :2], fix["values"][0][:6, :2])
        for log_n, shape, glo, ghi in refusals(good):
            assert raw_set(gpu_ctx, glo, ghi, log_n, shape) == EINVAL, (shape, glo, ghi)
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
        # n_tables = 0 clears the set
        assert raw_set(gpu_ctx, 1.0, 2.0, np.zeros((0, 8, 8))) == 0
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)


def test_tabulated_distribution_2d_object(gpu_ctx, fix):
    """api.TabulatedDistribution2D: calc_f, calc_f_derivatives and full_calculation give the bits of the raw entry (and of
    the oracle) on one point."""
    from rimphony_amd import api, capi
    glo, ghi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
    table = tables_of(fix, 0)[2]
    with time_limit(300):
        assert t2.set_tables(glo, ghi, table) == 0
        _oracle_has[0] = None
        f, dfdg, dfdcx = t2.dev_calc_f([0.0], 1.0, np.array([37.5]), np.array([0.3]))
        s, th = float(fix["s"][1]), float(fix["theta"][1])
        ref, _ = t2.batch([s], [th], [0.0])
        capi.check(raw_set(gpu_ctx, glo, ghi, table), ENTRY)
        raw = gpu_ctx.compute_batch(TAB, np.array([s]), np.array([th]), [np.zeros(1)], 0xFF)
        gpu_ctx.set_tables_2d(glo, ghi, None)
        d = api.TabulatedDistribution2D(glo, ghi, table)
        d.ctx = gpu_ctx._get()
        d.norm = 1.0
        assert d.calc_f(37.5, 0.3) == f[0] and f[0] > 0
        assert d.calc_f_derivatives(37.5, 0.3) == (dfdg[0], dfdcx[0]) and dfdcx[0] != 0
        got = d.full_calculation(gpu_ctx._get()).compute_all_dimensionless(s, th)
    assert np.isfinite(ref).all()
    assert same_bits(got, raw[0]).all() and same_bits(got, ref[0]).all()
