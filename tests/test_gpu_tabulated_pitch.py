"""GPU tests of the tabulated distribution with a pitch-angle factor g(cos xi) (rimphony_ctx_set_tables_pitch): the
coefficients, normalisations, calc_f values and the seams that d f / d cos xi reaches carry the bits of the pitch oracle
(tests/support/liboracle_tabpitch.so); an isotropic set gives the same bits through either entry and after a pitch set has
used the context; misuse is refused and leaves the previous set in place.  (What the oracle's spline, g and P are held to:
test_tabulated_pitch_host.py.)  Every test runs under a time limit of its own, and the oracle's side of a comparison is
computed before the launch."""
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
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_pitch_det.npz")
ISO_FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_det.npz")
EDGE_LO, EDGE_HI = 1.01, 1e4
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
    return np.load(FIXTURE)


@pytest.fixture(scope="module")
def iso_fix():
    return np.load(ISO_FIXTURE)


def install(ctx, fix, n_mu):
    """the fixture's set with pitch rows of n_mu nodes, in the context and in the oracle"""
    glo, ghi, G = float(fix["gamma_lo"]), float(fix["gamma_hi"]), tp.edge_pitch(n_mu)
    assert tp.set_tables(glo, ghi, fix["tables"], G) == 0
    ctx.set_tables(glo, ghi, fix["tables"], G)


def raw_set(ctx, glo, ghi, log_n, log_g, n_mu=None):
    """rimphony_ctx_set_tables_pitch as a C caller reaches it -> its return code"""
    dp = ctypes.POINTER(ctypes.c_double)
    log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
    if log_g is not None:
        log_g = np.ascontiguousarray(np.atleast_2d(log_g), dtype=np.float64)
    if n_mu is None:
        n_mu = 0 if log_g is None else log_g.shape[1]
    return ctx.lib.rimphony_ctx_set_tables_pitch(ctx.handle, log_n.shape[0], log_n.shape[1], float(glo), float(ghi),
                                                 log_n.ctypes.data_as(dp), n_mu, None if log_g is None else log_g.ctypes.data_as(dp))


@pytest.mark.parametrize("which", [0, 1], ids=["n_mu=8", "n_mu=4096"])
def test_fixture_rows_bit_identical(gpu_ctx, fix, which):
    """All 8 slots of the committed rows: values (NaN pattern included), per-coefficient sample counts, and the status words,
    of which the fixture holds what the values imply: ST_NONFINITE exactly where a value is NaN, ST_NORM_FAIL nowhere."""
    n_mu = int(fix["n_mu"][which])
    with time_limit(300):
        install(gpu_ctx, fix, n_mu)
        out, st, work = gpu_ctx.compute_batch(TAB, fix["s"], fix["theta"], [fix["index"]], 0xFF, want_status=True, want_work=True)
    print("n_mu", n_mu, "rows", len(out), "NaN per slot", np.isnan(out).sum(axis=0), "samples", int(work.sum()))
    assert len(out) == 24
    want = fix["values"][which]
    assert np.isfinite(want).any(axis=0).all() and np.isfinite(want).mean() >= 0.9
    mismatch("coefficients", out, want, lambda i: (fix["s"][i // 8], fix["theta"][i // 8], fix["index"][i // 8], i % 8))
    assert (work.astype(np.uint64) == fix["work"][which]).all()
    assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which]).all()
    # the pitch factor is in the numbers: the rows of the G = 0 table apart, the two geometries or the isotropic set differ
    assert not same_bits(fix["values"][0][16:], fix["values"][1][16:]).all()


def test_norm_and_calc_f_bit_identical(gpu_ctx, fix):
    """rimphony_batch_norm_device (bad indices included) and rimphony_calc_f_batch on 256 (gamma, mu) pairs per table: mu = +-1
    and 0, a mu a rounding beyond +-1, gamma at and outside both table ends."""
    rng = np.random.default_rng(12)
    lo, hi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
    gamma = np.concatenate([np.exp(rng.uniform(np.log(lo), np.log(hi), 244)),
                            [lo, hi, np.nextafter(lo, 0.), np.nextafter(hi, np.inf), 0.5 * lo, 2 * hi, 3.0, 3.0, 3.0, 3.0, 3.0, 50.0]])
    mu = np.concatenate([rng.uniform(-1, 1, 244),
                         [0.3, -0.3, 0.3, 0.3, 0.3, 0.3, -1.0, 1.0, 0.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), -0.0]])
    assert len(gamma) == 256 and len(mu) == 256
    index = np.array([0.0, 1.0, 2.0, 2.0, 3.0, 0.5, -1.0, np.nan])
    for n_mu in (8, 4096):
        with time_limit(120):
            install(gpu_ctx, fix, n_mu)
            ref_norm = tp.batch_norm(index)
            assert np.isfinite(ref_norm[:4]).all() and np.isnan(ref_norm[4:]).all()
            mismatch("norm n_mu %d" % n_mu, gpu_ctx.norm_batch(TAB, [index]), ref_norm)
            for table in (0, 1, 2):
                for nrm in (1.0, None):
                    want = tp.dev_calc_f([float(table)], ref_norm[table] if nrm is None else nrm, gamma, mu)
                    got = gpu_ctx.calc_f_batch(TAB, [float(table)], gamma, mu, nrm)
                    for name, g, w in zip(("f", "dfdg", "dfdcx"), got, want):
                        mismatch("%s table %d n_mu %d" % (name, table, n_mu), g, w, lambda i: (gamma[i], mu[i]))
                inside = (gamma >= lo) & (gamma <= hi)
                assert (got[0][~inside] == 0).all() and (got[1][~inside] == 0).all() and (got[2][~inside] == 0).all()
                if table == 1:
                    assert (got[2] == 0).all()                                  # G = 0
                else:
                    assert (got[2][inside] != 0).sum() >= 200                   # a live d f / d mu


PITCH_TABLES = (0, 2)          # the tables of the set whose G is not 0


def pitch_dist(table):
    d, st = tp.mkdist(table)
    assert st == 0 and np.isfinite(d.norm)
    return d


def test_gamma_integrand_seam_with_absorption(gpu_ctx, fix):
    """integrand_kernel_n<4> with a pitch row: emission and, above all, absorption, whose d f / d mu term takes the general
    form (beta cos theta - mu) / (gamma - 1 / gamma) and no longer the isotropic shortcut."""
    L = tp.load()
    rng = np.random.default_rng(504)
    with time_limit(120):
        install(gpu_ctx, fix, 8)
        for table, s, th, coeff, stokes in ((0, 100.0, 0.3, 1, 0), (2, 100.0, 1.5, 1, 1), (2, 30.0, 0.9, 1, 2), (0, 30.0, 0.9, 0, 0)):
            d = pitch_dist(table)
            n, g = harmonic_samples(rng, s, th, 200)
            ref = np.array([L.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
            assert (np.isfinite(ref) & (ref != 0)).sum() >= len(ref) // 2
            got = gpu_ctx.gamma_integrand_batch(TAB, [float(table)], coeff, stokes, s, th, n, g)
            mismatch("gamma_integrand table %d" % table, got, ref, lambda i: (s, th, coeff, stokes, n[i], g[i]))


def test_gamma_integral_seam(gpu_ctx, fix):
    """gamma_integral_kernel<4> with a pitch row: the first 8 harmonics and 8 further out."""
    L = tp.load()
    rng = np.random.default_rng(505)
    with time_limit(120):
        install(gpu_ctx, fix, 4096)
        for (table, s, th), (coeff, stokes, lobe) in zip(((0, 30.0, 0.9), (2, 12.0, 1.2)), ((1, 0, 0), (1, 2, 1))):
            d = pitch_dist(table)
            nmin = s * abs(math.sin(th))
            n = np.concatenate([np.floor(nmin + 1) + np.arange(8), nmin + 9 + np.exp(rng.uniform(0, 8, 8))])
            ref = np.array([L.rimo_gamma_integral(d, coeff, stokes, lobe, s, th, v) for v in n])
            assert (np.isfinite(ref) & (ref != 0)).sum() > len(n) // 2
            got = gpu_ctx.gamma_integral_batch(TAB, [float(table)], coeff, stokes, lobe, s, th, n)
            mismatch("gamma_integral table %d" % table, got, ref, lambda i: (s, th, n[i], lobe))


HEY_POINTS = ((2.0, 0.9), (60.0, 1.1))        # as test_gpu_tabulated.py: the J/Y branch, and the large-order branches


@pytest.mark.parametrize("table", PITCH_TABLES)
def test_faraday_seams(gpu_ctx, fix, table):
    """hey_element_kernel<4> and hey_outer_kernel<4> with a pitch row, quasi-resonant or not, stokes Q and V: the mu term of
    d f / d sigma (dev_heyvaerts.h), which no isotropic table reaches."""
    L = tp.load()
    rng = np.random.default_rng(510 + table)
    with time_limit(180):
        install(gpu_ctx, fix, 8)
        d = pitch_dist(table)
        for s, th in HEY_POINTS:
            for stokes in (1, 2):
                for qr in (0, 1):
                    fixed, v = hey_seam_inputs(rng, s, th, qr, 64)
                    ref = np.array([L.rimo_hey_element(ctypes.byref(d), stokes, s, th, qr, float(a), float(b)) for a, b in zip(fixed, v)])
                    assert np.isfinite(ref).sum() > 32
                    got = gpu_ctx.hey_element_batch(TAB, [float(table)], stokes, s, th, qr, fixed, v)
                    mismatch("hey_element table %d s %g stokes %d qr %d" % (table, s, stokes, qr), got, ref, lambda i: (fixed[i], v[i]))
                    u = hey_outer_abscissae(rng, s, th, qr, 6)
                    ref = np.array([L.rimo_hey_outer_integrand(ctypes.byref(d), stokes, s, th, qr, float(x)) for x in u])
                    assert np.isfinite(ref).sum() >= 3
                    got = gpu_ctx.hey_outer_batch(TAB, [float(table)], stokes, s, th, qr, u)
                    mismatch("hey_outer table %d s %g stokes %d qr %d" % (table, s, stokes, qr), got, ref, lambda i: u[i])


def iso_rows(iso_fix):
    sl = slice(0, 24)
    return iso_fix["s"][sl], iso_fix["theta"][sl], iso_fix["index"][sl], iso_fix["values"][sl], iso_fix["work"][sl]


def test_both_entries_agree_on_an_isotropic_set(gpu_ctx, iso_fix):
    """rimphony_ctx_set_tables and rimphony_ctx_set_tables_pitch with log_g = NULL, n_mu = 0: the committed isotropic rows,
    bit for bit, through either."""
    from rimphony_amd import capi
    s, th, index, want, want_work = iso_rows(iso_fix)
    glo, ghi = float(iso_fix["gamma_lo"]), float(iso_fix["gamma_hi"])
    with time_limit(300):
        gpu_ctx.set_tables(glo, ghi, iso_fix["tables"])
        old = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        capi.check(raw_set(gpu_ctx, glo, ghi, iso_fix["tables"], None), "rimphony_ctx_set_tables_pitch")
        new = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
    mismatch("old entry", old[0], want)
    mismatch("new entry", new[0], want)
    assert (old[1] == new[1]).all() and (old[2] == new[2]).all() and (old[2].astype(np.uint64) == want_work).all()


def test_no_pitch_state_survives(gpu_ctx, fix, iso_fix):
    """One context: isotropic, then the same gamma tables with pitch rows, then isotropic again.  The third results are the
    first, bit for bit; the second are not."""
    s, th, index = fix["s"], fix["theta"], fix["index"]
    glo, ghi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
    with time_limit(300):
        gpu_ctx.set_tables(glo, ghi, fix["tables"])
        first = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        norm1 = gpu_ctx.norm_batch(TAB, [np.arange(3.0)])
        install(gpu_ctx, fix, 8)
        second = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        gpu_ctx.set_tables(glo, ghi, fix["tables"])
        third = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        norm3 = gpu_ctx.norm_batch(TAB, [np.arange(3.0)])
    assert tab_bind.set_tables(glo, ghi, fix["tables"]) == 0
    ref, ref_work = tab_bind.batch(s, th, index, nthreads=16)
    mismatch("first", first[0], ref)
    mismatch("third", third[0], ref)
    assert (first[1] == third[1]).all() and (first[2] == third[2]).all() and (first[2].astype(np.uint64) == ref_work).all()
    assert same_bits(norm1, norm3).all()
    mismatch("second", second[0], fix["values"][0])
    differs = ~same_bits(first[0], second[0]).all(axis=1)
    assert differs[index != 1].all()                    # every row of a table with G != 0 moved


def test_batch_size_and_cooperative_tail_change_no_bit(gpu_ctx, fix):
    """One row against all rows, and a context without the cooperative tail (RIMPHONY_NO_ASSIST=1): same bits, same status
    words, same sample counts on the pitch rows."""
    glo, ghi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
    s, th, index = fix["s"], fix["theta"], fix["index"]
    with time_limit(300):
        install(gpu_ctx, fix, 8)
        big = gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        ones = [gpu_ctx.compute_batch(TAB, s[i:i + 1], th[i:i + 1], [index[i:i + 1]], 0xFF, want_status=True, want_work=True)
                for i in (0, 17)]
        solo_ctx = env_context(RIMPHONY_NO_ASSIST="1")
        try:
            solo_ctx.set_tables(glo, ghi, fix["tables"], tp.edge_pitch(8))
            solo = solo_ctx.compute_batch(TAB, s, th, [index], 0xFF, want_status=True, want_work=True)
        finally:
            solo_ctx.close()
    mismatch("all rows", big[0], fix["values"][0])
    for i, one in zip((0, 17), ones):
        assert same_bits(big[0][i:i + 1], one[0]).all() and (big[1][i:i + 1] == one[1]).all() and (big[2][i:i + 1] == one[2]).all(), i
    assert same_bits(big[0], solo[0]).all() and (big[1] == solo[1]).all() and (big[2] == solo[2]).all()


def test_misuse_on_a_live_context(gpu_ctx, fix):
    from rimphony_amd import api, capi
    glo, ghi, t = float(fix["gamma_lo"]), float(fix["gamma_hi"]), fix["tables"]
    s, th, index = fix["s"][:6].copy(), fix["theta"][:6].copy(), fix["index"][:6].copy()
    good = tp.edge_pitch(16)
    nan_g, inf_g = good.copy(), good.copy()
    nan_g[1, 5], inf_g[2, 0] = np.nan, -np.inf
    with time_limit(300):
        install(gpu_ctx, fix, 8)
        before = gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)
        mismatch("before", before[:, :2], fix["values"][0][:6, :2])
        for log_g, n_mu in ((good[:, :7], None), (nan_g, None), (inf_g, None), (good, 0), (None, 16), (good, 65537)):
            assert raw_set(gpu_ctx, glo, ghi, t, log_g, n_mu) == EINVAL
        with pytest.raises(ValueError):
            gpu_ctx.set_tables(glo, ghi, t, good[:2])                           # a wrong row count: the mirror's check
        after = gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)
        assert same_bits(before, after).all()                                   # the previous set is still in place
        # a bad index on a pitch set: NaN and ST_NORM_FAIL on that row only
        bad_index = np.array([0.0, 3.0, 2.0, 0.5, 0.0, np.nan])
        out, st = gpu_ctx.compute_batch(TAB, s, th, [bad_index], 0x03, want_status=True)
        bad = np.array([False, True, False, True, False, True])
        assert np.isnan(out[bad][:, :2]).all() and ((st[bad][:, :2] & ST_NORM_FAIL) != 0).all()
        assert ((st[~bad] & ST_NORM_FAIL) == 0).all() and np.isfinite(out[~bad][:, :2]).all()
        with pytest.raises(capi.RimphonyError, match="not supported"):
            gpu_ctx.compute_batch(TAB, s, th, [index], 0xFF, precision=api.PRECISION_F32_INTEGRAND)
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.highfreq_batch(TAB, s, th, [index])
        # n_tables = 0 clears the set through the new entry too
        assert raw_set(gpu_ctx, 1.0, 2.0, np.zeros((0, 8)), None) == 0
        with pytest.raises(capi.RimphonyError, match="invalid argument"):
            gpu_ctx.compute_batch(TAB, s, th, [index], 0x03)


def test_tabulated_distribution_object_with_log_g(gpu_ctx, fix):
    """api.TabulatedDistribution(..., log_g=...): calc_f, calc_f_derivatives and full_calculation give the bits of the raw
    entry (and of the oracle) on one point."""
    from rimphony_amd import api, capi
    glo, ghi = float(fix["gamma_lo"]), float(fix["gamma_hi"])
    G = tp.log_g_beam(64, 0.8, 1.5)
    with time_limit(300):
        assert tp.set_tables(glo, ghi, fix["tables"][0], G) == 0
        f, dfdg, dfdcx = tp.dev_calc_f([0.0], 1.0, np.array([37.5]), np.array([0.3]))
        s, th = float(fix["s"][1]), float(fix["theta"][1])
        ref, _ = tp.batch([s], [th], [0.0])
        capi.check(raw_set(gpu_ctx, glo, ghi, fix["tables"][0], G), "rimphony_ctx_set_tables_pitch")
        raw = gpu_ctx.compute_batch(TAB, np.array([s]), np.array([th]), [np.zeros(1)], 0xFF)
        gpu_ctx.set_tables(glo, ghi, None)
        d = api.TabulatedDistribution(glo, ghi, fix["tables"][0], log_g=G)
        d.ctx = gpu_ctx._get()
        d.norm = 1.0
        assert d.calc_f(37.5, 0.3) == f[0] and f[0] > 0
        assert d.calc_f_derivatives(37.5, 0.3) == (dfdg[0], dfdcx[0]) and dfdcx[0] != 0
        got = d.full_calculation(gpu_ctx._get()).compute_all_dimensionless(s, th)
    assert np.isfinite(ref).all()
    assert same_bits(got, raw[0]).all() and same_bits(got, ref[0]).all()
