"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on the
same seeded inputs.  Bar: BIT-EXACT (the oracle build shares the deterministic
elementary functions and the GK31 reduction tree with the kernels; DESIGN.md
"Rounding contract").  north_star's stated tolerance is 1e-6 relative; where a
test cannot be bit-exact it says so and uses that tolerance.
"""
import ctypes
import math

import numpy as np
import pytest

import oracle_bind
from rimphony_amd import workload
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6   # north_star: <= 1e-6 max relative error


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def report_mismatch(name, got, ref, extra=None):
    ok = same_bits(got, ref)
    if ok.all():
        return
    bad = np.flatnonzero(~ok.ravel())
    g, r = np.ravel(got)[bad], np.ravel(ref)[bad]
    with np.errstate(all="ignore"):
        rel = np.abs(g - r) / np.abs(r)
    msg = "%s: %d of %d differ; max rel %.3e; first idx %d got %r ref %r" % (
        name, len(bad), ok.size, np.nanmax(rel) if len(rel) else 0.0, bad[0], g[0], r[0])
    if extra is not None:
        msg += " | " + str(extra(bad[0]))
    pytest.fail(msg)


def test_bessel_bit_exact(gpu_ctx, oracle):
    rng = np.random.default_rng(11)
    N = 60000
    u = rng.random(N)
    n = np.where(u < 0.2, rng.integers(0, 31, N).astype(float),
                 np.exp(rng.uniform(math.log(30), math.log(1e14), N)))
    n = np.where(rng.random(N) < 0.5, np.floor(n), n)
    eta = rng.uniform(-12, 0, N)
    x = n * (1 - 10.0 ** eta)
    x = np.where(rng.random(N) < 0.05, n * (1 + 10.0 ** rng.uniform(-12, -3, N)), x)
    x = np.where(rng.random(N) < 0.08, n * (1 + 10.0 ** rng.uniform(-4, 1, N)), x)      # x > n up to 11 n: Meissel "second"
    x = np.where(rng.random(N) < 0.02, n, x)
    x = np.where(rng.random(N) < 0.02, 0.0, x)
    x = np.where((n < 30) & (rng.random(N) < 0.1), np.exp(rng.uniform(math.log(3e4), math.log(1e9), N)), x)   # Hankel branch
    j, dj = gpu_ctx.bessel_batch(n, x)
    rj = np.array([oracle.rimo_bessel_j(a, b) for a, b in zip(n, x)])
    rdj = np.array([oracle.rimo_bessel_dj(a, b) for a, b in zip(n, x)])
    report_mismatch("bessel_j", j, rj, lambda i: (n[i], x[i]))
    report_mismatch("bessel_dj", dj, rdj, lambda i: (n[i], x[i]))


def test_bessel_hostile_arguments(gpu_ctx, oracle):
    """pkgw_bessel_j / pkgw_bessel_dj on every pair of a grid of awkward orders and arguments (zero, negative,
    fractional below 30, 1e15 and beyond, subnormal, NaN, +-inf; x from 0 to 1e300, negative, NaN, inf): the device
    function returns what the oracle returns, NaNs included."""
    import itertools
    nan, inf = float("nan"), float("inf")
    ns = [0., 1., 2., 5., 29., 30., 31., 12.5, 30.5, 100., 1e3, 1e6, 1e15, 1e16, 1e300, -1., -30., -100.5, nan, inf, -inf,
          1e-320, 0.5]
    xs = [0., -0., 1e-320, 1e-300, 1e-10, 0.5, 1., 5., 17., 29.9, 30., 31., 100., 1e3, 5e4, 5.1e4, 1e6, 1e15, 1e55, 1e56,
          1e300, -1., -100., -1e-320, -30., -1e6, nan, inf, -inf]
    pairs = np.array(list(itertools.product(ns, xs)))
    n, x = pairs[:, 0].copy(), pairs[:, 1].copy()
    j, dj = gpu_ctx.bessel_batch(n, x)
    rj = np.array([oracle.rimo_bessel_j(a, b) for a, b in zip(n, x)])
    rdj = np.array([oracle.rimo_bessel_dj(a, b) for a, b in zip(n, x)])
    report_mismatch("bessel_j hostile", j, rj, lambda i: (n[i], x[i]))
    report_mismatch("bessel_dj hostile", dj, rdj, lambda i: (n[i], x[i]))


def test_scalar_bessel_seam(gpu_ctx, oracle):
    """pkgw_bessel_j / pkgw_bessel_dj, the reference's own FFI seam (leung-bessel/src/lib.rs:36-42), as exported
    by the library: same bits as the batch entry point and the oracle, NaN conventions included."""
    from rimphony_amd import capi
    lib = capi.load()
    for n, x in [(2., 1.5), (29., 28.5), (100., 99.), (1e6, 999000.), (30.5, 10.), (12.5, 3.), (50., 50.), (40., -1.)]:
        rj, rdj = oracle.rimo_bessel_j(n, x), oracle.rimo_bessel_dj(n, x)
        j, dj = lib.pkgw_bessel_j(n, x), lib.pkgw_bessel_dj(n, x)
        assert (j == rj or (math.isnan(j) and math.isnan(rj))), (n, x, j, rj)
        assert (dj == rdj or (math.isnan(dj) and math.isnan(rdj))), (n, x, dj, rdj)
    # the reference's own smoke values (leung-bessel/src/lib.rs:82-86, assert_approx_eq at 1e-6)
    assert abs(lib.pkgw_bessel_j(0., 0.) - 1.) < 1e-6
    assert abs(lib.pkgw_bessel_j(5., 5.) - 0.2611405) < 1e-6
    assert abs(lib.pkgw_bessel_j(0., 17.) + 0.1698543) < 1e-6


def _kind_params(rng, kind):
    if kind == 0:
        return [rng.uniform(1.5, 4), float(np.exp(rng.uniform(0, math.log(30)))), 1e12, 1e10]
    if kind == 1:
        return [float(np.exp(rng.uniform(math.log(.1), math.log(100))))]
    if kind == 2:
        return [rng.uniform(1.5, 4), rng.uniform(0, 3), 1., 1e12, 1e10]
    return [rng.uniform(1.5, 4.5), float(np.exp(rng.uniform(1, 3))), rng.uniform(0, 3), 1e10]


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_gamma_integrand_bit_exact(gpu_ctx, oracle, kind):
    rng = np.random.default_rng(100 + kind)
    for trial in range(6):
        par = _kind_params(rng, kind)
        d, st = oracle_bind.mkdist(oracle, kind, par)
        assert st == 0
        s = float(np.exp(rng.uniform(math.log(.1), math.log(1e6))))
        th = float(rng.uniform(0.01, 1.55))
        coeff, stokes = int(rng.integers(0, 2)), int(rng.integers(0, 3))
        n, g = harmonic_samples(rng, s, th, 3000)
        got = gpu_ctx.gamma_integrand_batch(kind, par, coeff, stokes, s, th, n, g)
        ref = np.array([oracle.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
        report_mismatch("gamma_integrand kind %d" % kind, got, ref, lambda i: (par, s, th, coeff, stokes, n[i], g[i]))


def test_integrand_with_bessel_values_next_to_underflow(gpu_ctx, oracle):
    """Inside the integrand the kernels return Bessel values below 2.2e-294 as signed zeros (dev_bessel.h exp_factor,
    TINY_ZERO) where the oracle keeps the reference's exp(log|f| + e) (bessel.c:44-48): every product of such a value
    underflows, so the samples must still be the oracle's bits.  Dense gamma sweeps over whole integration ranges, so
    that hundreds of samples have J_n or J_{n+1} between 1e-323 and 2.2e-294."""
    rng = np.random.default_rng(77)
    hit = 0
    for kind, par, s, th, n in ((0, [2.5, 1., 1e12, 1e10], 40., 0.8, 2000.5), (1, [8.0], 300., 1.1, 5000.),
                                (0, [3.2, 1., 1e12, 1e10], 5., 0.3, 1500.25), (3, [3.3, 6.0, 0.8, 1e10], 90., 0.6, 3000.)):
        d, st = oracle_bind.mkdist(oracle, kind, par)
        assert st == 0
        nos = n / s
        root = math.sqrt(nos * nos - math.sin(th) ** 2)
        gm = (nos - abs(math.cos(th)) * root) / math.sin(th) ** 2
        gp = (nos + abs(math.cos(th)) * root) / math.sin(th) ** 2
        g = np.sort(gm + (gp - gm) * rng.random(12000))
        nn = np.full_like(g, n)
        for coeff, stokes in ((0, 0), (1, 2)):
            got = gpu_ctx.gamma_integrand_batch(kind, par, coeff, stokes, s, th, nn, g)
            ref = np.array([oracle.rimo_gamma_integrand(d, coeff, stokes, s, th, n, float(x)) for x in g])
            report_mismatch("integrand next to underflow, kind %d" % kind, got, ref, lambda i: (par, s, th, coeff, stokes, n, g[i]))
        # how many of these samples had a Bessel value in the band the kernels flush (symphony.rs:398-437 kinematics)
        beta = np.sqrt(1. - 1. / (g * g))
        cos_xi = (s * g - n) / (s * g * beta * math.cos(th))
        with np.errstate(invalid="ignore"):
            z = s * beta * math.sin(th) * g * np.sqrt(1. - cos_xi * cos_xi)
        z = z[np.isfinite(z)][::8]
        for order in (n, n + 1.):
            j = np.abs(np.array([oracle.rimo_bessel_j(order, float(x)) for x in z]))
            hit += int(((j > 0) & (j < 2.2e-294)).sum())
    assert hit > 100, hit


def test_qag_selftest_bit_exact(gpu_ctx, oracle):
    """Wave-cooperative QAG vs the oracle's GSL-order QAG on +-*/sqrt integrands:
    result, error estimate, status AND subinterval count must agree, including
    cases that end in EROUND / ESING / EMAXITER."""
    rng = np.random.default_rng(5)
    N = 4000
    fam = rng.integers(0, 4, N).astype(np.int32)
    a = rng.uniform(-3, 1, N)
    b = a + np.exp(rng.uniform(-2, 3, N))
    p0 = a + (b - a) * rng.uniform(-0.2, 1.2, N)
    p1 = np.exp(rng.uniform(-4, 6, N))
    for (epsabs, epsrel, limit) in [(0., 1e-3, 1000), (0., 1e-8, 1000), (1e-10, 0., 50), (0., 1e-12, 200), (0., 1e-13, 700)]:
        res, err, qst, size = gpu_ctx.qag_selftest(fam, p0, p1, a, b, epsabs, epsrel, limit)
        ref = [oracle_bind.qag_selftest(oracle, fam[i], p0[i], p1[i], a[i], b[i], epsabs, epsrel, limit) for i in range(N)]
        rst = np.array([r[0] for r in ref]); rres = np.array([r[1] for r in ref])
        rerr = np.array([r[2] for r in ref]); rsz = np.array([r[3] for r in ref])
        # lists longer than the 256-entry LDS store spill to global memory: every size up to the
        # GSL limit must agree
        assert (qst == rst).all(), (epsrel, np.flatnonzero(qst != rst)[:5])
        assert (size == rsz).all()
        report_mismatch("qag result eps=%g" % epsrel, res, rres)
        report_mismatch("qag abserr eps=%g" % epsrel, err, rerr)
    # long subinterval lists (beyond the LDS store): triangle waves with many kinks
    M = 64
    fam = np.full(M, 4, dtype=np.int32)
    a = rng.uniform(-1, 0, M); b = a + rng.uniform(2, 6, M)
    p0 = rng.uniform(20, 120, M); p1 = np.exp(rng.uniform(-2, 2, M))
    res, err, qst, size = gpu_ctx.qag_selftest(fam, p0, p1, a, b, 0., 1e-6, 5000)
    ref = [oracle_bind.qag_selftest(oracle, 4, p0[i], p1[i], a[i], b[i], 0., 1e-6, 5000) for i in range(M)]
    rsz = np.array([r[3] for r in ref])
    assert rsz.max() > 300, rsz.max()      # well past the 256-entry LDS part
    assert (qst == np.array([r[0] for r in ref])).all() and (size == rsz).all()
    report_mismatch("qag long-list result", res, np.array([r[1] for r in ref]))
    report_mismatch("qag long-list abserr", err, np.array([r[2] for r in ref]))


def qag_past_half_inputs():
    """Family 4 (triangle waves with many kinks), the shape of the long-list leg above, 256 cases."""
    rng = np.random.default_rng(6)
    M = 256
    a = rng.uniform(-1, 0, M); b = a + rng.uniform(2, 6, M)
    p0 = rng.uniform(20, 120, M); p1 = np.exp(rng.uniform(-2, 2, M))
    return np.full(M, 4, dtype=np.int32), p0, p1, a, b


@pytest.mark.parametrize("epsrel,limit,min_between", [(1e-6, 200, 0), (1e-6, 400, 10), (1e-8, 1000, 10)])
def test_qag_selftest_past_half_the_limit(gpu_ctx, oracle, epsrel, limit, min_between):
    """GSL's qpsrt keeps its order list fully sorted only while the workspace holds fewer than limit / 2 + 2 intervals;
    beyond, it sorts the top limit + 1 - last entries only, and the kernels go on picking by argmax over (error, stamp).
    Limits small enough that many cases end AT the limit (status 11, every pick of the second half made in that regime) and,
    on two of the three legs, others converge strictly between limit / 2 + 2 and the limit: result, error estimate, status
    and size are the oracle's, whose qpsrt is qpsrt.c's (oracle/rimo_quad.c)."""
    fam, p0, p1, a, b = qag_past_half_inputs()
    ref = [oracle_bind.qag_selftest(oracle, 4, p0[i], p1[i], a[i], b[i], 0., epsrel, limit) for i in range(len(a))]
    rst = np.array([r[0] for r in ref]); rsz = np.array([r[3] for r in ref])
    at_limit = int((rst == 11).sum())
    between = int(((rsz > limit // 2 + 2) & (rsz < limit)).sum())
    print("limit %d: %d cases end at the limit, %d strictly between limit/2 + 2 and the limit" % (limit, at_limit, between))
    assert at_limit >= 60 and between >= min_between, (at_limit, between)
    res, err, qst, size = gpu_ctx.qag_selftest(fam, p0, p1, a, b, 0., epsrel, limit)
    assert (qst == rst).all(), np.flatnonzero(qst != rst)[:5]
    assert (size == rsz).all(), np.flatnonzero(size != rsz)[:5]
    report_mismatch("qag past half the limit, result", res, np.array([r[1] for r in ref]))
    report_mismatch("qag past half the limit, abserr", err, np.array([r[2] for r in ref]))


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_norm_bit_exact(gpu_ctx, oracle, kind):
    cfg = {0: "cfg2_powerlaw_8", 1: "cfg3_thermal_8", 2: "cfg4_pitchypl_8", 3: "cfg5_pitchykappa_8"}[kind]
    _, _, s, th, params = workload.make_batch(cfg, 300)
    got = gpu_ctx.norm_batch(kind, params)
    ref = oracle_bind.batch_norm(oracle, kind, params)
    assert np.isfinite(ref).all()
    report_mismatch("norm kind %d" % kind, got, ref)


@pytest.mark.parametrize("kind,stokes,coeff", [(0, 0, 0), (0, 2, 1), (2, 1, 0), (3, 2, 0), (1, 0, 1)])
def test_gamma_integral_bit_exact(gpu_ctx, oracle, kind, stokes, coeff):
    rng = np.random.default_rng(300 + kind * 10 + stokes)
    par = _kind_params(rng, kind)
    d, st = oracle_bind.mkdist(oracle, kind, par)
    for (s, th) in [(3.0, 0.7), (250.0, 1.2), (4000.0, 0.2)]:
        nmin = s * abs(math.sin(th))
        n = np.concatenate([np.floor(nmin + 1) + np.arange(30), nmin + 31 + np.exp(rng.uniform(0, 10, 60))])
        for lobe in ([0, 1] if stokes == 2 else [0]):
            got = gpu_ctx.gamma_integral_batch(kind, par, coeff, stokes, lobe, s, th, n)
            ref = np.array([oracle.rimo_gamma_integral(d, coeff, stokes, lobe, s, th, v) for v in n])
            report_mismatch("gamma_integral", got, ref, lambda i: (par, s, th, n[i], lobe))


def _symphony_parity(gpu_ctx, oracle, cfg, n, mask):
    kind, _, s, th, params = workload.make_batch(cfg, n)
    got, status = gpu_ctx.compute_batch(kind, s, th, params, mask, want_status=True)
    ref = oracle_bind.batch(oracle, kind, s, th, params, mask, nthreads=16)
    sel = [k for k in range(8) if mask & (1 << k)]
    g, r = got[:, sel], ref[:, sel]
    # NaN pattern must match exactly
    assert (np.isnan(g) == np.isnan(r)).all()
    ok = same_bits(g, r)
    with np.errstate(all="ignore"):
        rel = np.abs(g - r) / np.abs(r)
    rel = np.where(ok, 0.0, rel)
    assert np.nanmax(rel) <= REL_TOL, "max rel err %.3e (tolerance %.1e)" % (np.nanmax(rel), REL_TOL)
    # the design goal is bit-exactness; report it as the stronger check
    assert ok.all(), "%d of %d coefficients not bit-identical (max rel %.3e)" % ((~ok).sum(), ok.size, np.nanmax(rel))
    unsel = [k for k in range(8) if not mask & (1 << k)]
    assert np.isnan(got[:, unsel]).all()
    return got, status


def test_symphony_powerlaw_jI_aI(gpu_ctx, oracle):
    """BASELINE config 2 (power law, j_I/alpha_I), first 96 points."""
    _symphony_parity(gpu_ctx, oracle, "cfg2_powerlaw_jI_aI", 96, 0x03)


def test_symphony_powerlaw_all_six(gpu_ctx, oracle):
    _symphony_parity(gpu_ctx, oracle, "cfg2_powerlaw_8", 48, 0x3F)


@pytest.mark.parametrize("cfg", ["cfg3_thermal_8", "cfg4_pitchypl_8", "cfg5_pitchykappa_8"])
def test_symphony_other_distributions(gpu_ctx, oracle, cfg):
    _symphony_parity(gpu_ctx, oracle, cfg, 24, 0x3F)


@pytest.mark.parametrize("cfg,n", [("cfg2_powerlaw_8", 64), ("cfg3_thermal_8", 48), ("cfg4_pitchypl_8", 48),
                                   ("cfg5_pitchykappa_8", 48)])
def test_faraday_bit_exact(gpu_ctx, oracle, cfg, n):
    """Heyvaerts rho_Q / rho_V (slots 6, 7) against the oracle."""
    _symphony_parity(gpu_ctx, oracle, cfg, n, 0xC0)


def test_endless_thermal_marching_loops_end_at_once_with_the_caps_status(gpu_ctx, oracle):
    """Cold, high-frequency thermal points whose quasi-resonant part is exactly 0: the reference's marching loop never ends
    there (heyvaerts.rs:156-185 tests keep_going only once qr_val != 0); this build applies its step cap as soon as the
    loop is PROVABLY endless (dev_heyvaerts.h hey_qr_is_endless).  Row 51111 of the thermal table is one (found as the
    longest chain of the table, profiles/r4_launch_tails.txt): both Faraday slots NaN with status CHUNK_CAP | NONFINITE, after
    a few hundred thousand samples instead of the four million the 4096-step cap took, and the oracle agrees -- values,
    and sample counts (the work counters would show a loop that ran on)."""
    kind, mask, s, th, params = workload.make_batch("cfg3_thermal_8", 4, start=51109)
    out, st, work = gpu_ctx.compute_batch(kind, s, th, params, 0xC0, want_status=True, want_work=True)
    assert np.isnan(out[2, 6:]).all() and (st[2, 6:] == (4 | 16)).all(), (out[2], st[2])
    assert (work[2, 6:] < 1000000).all() and (work[2, 6:] > 100000).all(), work[2]
    ref, ctr = oracle_bind.batch(oracle, kind, s, th, params, 0xC0, nthreads=4, want_counters=True)
    report_mismatch("thermal rows around an endless loop", out[:, 6:], ref[:, 6:])
    assert int(work[:, 6:].sum()) == ctr["integrand_evals"]


def test_faraday_known_answers_on_gpu(gpu_ctx):
    """The reference's four 1 % Faraday fixtures through the HIP path (power_law.rs:209-240,
    thermal_juettner.rs:174-210)."""
    from rimphony_amd import api
    pl = api.PowerLawDistribution(2.5).gamma_limits(10., 1e12, 1e10).full_calculation(gpu_ctx)
    assert abs(pl.compute_dimensionless(api.Coefficient.Faraday, api.Stokes.Q, 1e4, 0.25 * math.pi) / 1.89e-9 - 1) < 0.01
    assert abs(pl.compute_dimensionless(api.Coefficient.Faraday, api.Stokes.V, 1e4, 0.25 * math.pi) / 5.28e-8 - 1) < 0.01
    tj = api.ThermalJuettnerDistribution(10.).full_calculation(gpu_ctx)
    assert abs(tj.compute_dimensionless(api.Coefficient.Faraday, api.Stokes.Q, 4e4, 0.4) / 4.8081e-11 - 1) < 0.01
    tj = api.ThermalJuettnerDistribution(0.1).full_calculation(gpu_ctx)
    assert abs(tj.compute_dimensionless(api.Coefficient.Faraday, api.Stokes.V, 40., 0.5) / 3.064e-4 - 1) < 0.01
    assert math.isnan(pl.compute_dimensionless(api.Coefficient.Faraday, api.Stokes.I, 1e4, 0.5))   # lib.rs:239-240


def test_all_eight_slots_one_call(gpu_ctx, oracle):
    """compute_all_dimensionless semantics: all 8 slots in the order of lib.rs:176-177."""
    _symphony_parity(gpu_ctx, oracle, "cfg4_pitchypl_8", 12, 0xFF)


def test_golden_file_on_gpu(gpu_ctx):
    """The reference's own fixture (tests/symphony-powerlaw.txt, Symphony-C values, 1 %,
    reference tests/symphony.rs:29-112) evaluated through the HIP path: every row, all six coefficients."""
    import os
    rows = np.loadtxt(os.path.join(os.path.dirname(__file__), "golden", "symphony-powerlaw.txt"))
    n = len(rows)
    s, th, p = rows[:, 0], rows[:, 1], rows[:, 2]
    out = gpu_ctx.compute_batch(0, s, th, [p, np.ones(n), 1e12 * np.ones(n), 1e10 * np.ones(n)], 0x3F)
    nu = 1e9
    cgs = out[:, :6].copy()
    cgs[:, [0, 2, 4]] *= nu
    cgs[:, [1, 3, 5]] /= nu
    rel = np.abs(cgs / rows[:, 3:9] - 1)
    assert not np.isnan(rel).any()
    # same single exception as the oracle's pin (tests/test_oracle.py::test_golden_file_full): alpha_V of row 159
    bad = np.argwhere(rel >= 0.01)
    assert len(bad) <= 1 and (len(bad) == 0 or (tuple(bad[0]) == (159, 5) and rel[159, 5] < 0.014)), bad


def test_golden_rows_bit_exact_vs_oracle(gpu_ctx, oracle):
    """The golden file's parameter rows reach corners the synthetic tables avoid (theta down to 0.0027, s from
    0.07 to 9433): every 4th row, six coefficients, HIP path against the oracle bit for bit."""
    import os
    rows = np.loadtxt(os.path.join(os.path.dirname(__file__), "golden", "symphony-powerlaw.txt"))[::4]
    n = len(rows)
    s, th, p = rows[:, 0].copy(), rows[:, 1].copy(), rows[:, 2].copy()
    params = [p, np.ones(n), 1e12 * np.ones(n), 1e10 * np.ones(n)]
    got = gpu_ctx.compute_batch(0, s, th, params, 0x3F)
    ref = oracle_bind.batch(oracle, 0, s, th, params, 0x3F, nthreads=16)
    report_mismatch("golden rows vs oracle", got[:, :6], ref[:, :6], extra=lambda i: rows[i // 6, :3])


@pytest.mark.parametrize("cfg,n", [("cfg2_powerlaw_8", 64), ("cfg3_thermal_8", 32), ("cfg4_pitchypl_8", 32),
                                   ("cfg5_pitchykappa_8", 24)])
def test_small_angle_corner(gpu_ctx, oracle, cfg, n):
    """The corner the synthetic tables leave out (theta < 0.05, where the harmonics run to huge n):
    theta log-uniform in [1e-3, 0.05], all eight slots, bit for bit."""
    kind, _, s, _, params = workload.make_batch(cfg, n, start=900000)
    u = workload.uniform01(99, np.arange(n), 1)
    th = np.exp(np.log(1e-3) + u * (np.log(0.05) - np.log(1e-3)))
    got, st = gpu_ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True)
    ref = oracle_bind.batch(oracle, kind, s, th, params, 0xFF, nthreads=16)
    report_mismatch("small-angle corner " + cfg, got, ref, extra=lambda i: (s[i // 8], th[i // 8]))


def test_reference_benchmark_cases(gpu_ctx, oracle):
    """The five rows of the Latin square of benches/powerlaw.rs:28-45 (its sixteen benchmark functions compute one
    coefficient each on these rows): all eight slots, bit for bit."""
    SS, TH, PS = [1e0, 1e1, 1e2, 1e3, 1e4], [0.05, 0.430, 0.810, 1.190, 1.5707], [1.5, 1.75, 2.5, 3.25, 4.]
    LATIN = [1, 4, 2, 3, 0, 3, 1, 0, 4, 2, 0, 3, 1, 2, 4, 2, 0, 4, 1, 3, 4, 2, 3, 0, 1]
    s = np.array([SS[LATIN[5 * r + 2]] for r in range(5)])
    th = np.array([TH[LATIN[5 * r + 3]] for r in range(5)])
    p = np.array([PS[LATIN[5 * r + 4]] for r in range(5)])
    params = [p, np.ones(5), 1e12 * np.ones(5), 1e10 * np.ones(5)]
    got = gpu_ctx.compute_batch(0, s, th, params, 0xFF)
    ref = oracle_bind.batch(oracle, 0, s, th, params, 0xFF, nthreads=5)
    report_mismatch("benches/powerlaw.rs rows", got, ref, extra=lambda i: (s[i // 8], th[i // 8], p[i // 8]))
    assert np.isfinite(got[0]).all()          # row 0 carries all eight benchmark functions


def test_empty_and_unselected(gpu_ctx):
    out = gpu_ctx.compute_batch(0, np.zeros(0), np.zeros(0), [np.zeros(0)] * 4, 0x3F)
    assert out.shape == (0, 8)
    out, st = gpu_ctx.compute_batch(0, [10.0], [0.8], [[2.5], [1.0], [1e12], [1e10]], 0x01, want_status=True)
    assert np.isfinite(out[0, 0]) and np.isnan(out[0, 1:]).all()
    assert st[0, 0] == 0 and (st[0, 1:] & 64).all()


def test_any_coefficient_mask_selects_the_same_bits(gpu_ctx):
    """A slot's value does not depend on which other slots are selected: every single-bit mask, a few mixed ones
    and the empty mask on 24 pitchy-power-law points against the columns of the 0xFF table; unselected slots are
    NaN with status NOT_COMPUTED (64)."""
    kind, _, s, th, params = workload.make_batch("cfg4_pitchypl_8", 24, start=31000)
    full, st_full = gpu_ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True)
    for mask in [1 << k for k in range(8)] + [0x00, 0xC0, 0x3F, 0x55, 0xAA, 0x81]:
        out, st = gpu_ctx.compute_batch(kind, s, th, params, mask, want_status=True)
        sel = [k for k in range(8) if mask & (1 << k)]
        uns = [k for k in range(8) if not mask & (1 << k)]
        assert same_bits(out[:, sel], full[:, sel]).all(), hex(mask)
        assert (st[:, sel] == st_full[:, sel]).all(), hex(mask)
        assert np.isnan(out[:, uns]).all() and ((st[:, uns] & 64) != 0).all(), hex(mask)


def test_results_independent_of_batch_composition(gpu_ctx):
    """A point's result must not depend on what else is in the batch (interleaved
    sharding across GPUs relies on this)."""
    kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_jI_aI", 64)
    full = gpu_ctx.compute_batch(kind, s, th, params, mask)
    sub = slice(1, 64, 2)
    part = gpu_ctx.compute_batch(kind, s[sub], th[sub], [p[sub] for p in params], mask)
    assert same_bits(full[sub][:, :2], part[:, :2]).all()


def test_sharded_table_equals_whole_table_at_bench_size(gpu_ctx):
    """Size-independent property at the bench's launch size (65536 rows of BASELINE configs[1]): the table
    computed in one launch and the table assembled from the two interleaved shards a 2-GPU job would compute
    (row i -> rank i mod 2) are the same bits, NaN rows included."""
    from rimphony_amd import sharding
    n = 65536
    kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_jI_aI", n, start=131072)
    whole = gpu_ctx.compute_batch(kind, s, th, params, mask)
    merged = np.empty_like(whole)
    for rank in range(2):
        mine = sharding.shard_indices(n, rank, 2)
        merged[mine] = gpu_ctx.compute_batch(kind, s[mine], th[mine], [p[mine] for p in params], mask)
    assert same_bits(whole[:, :2], merged[:, :2]).all()
    assert np.isfinite(whole[:, :2]).mean() > 0.999


def test_full_size_table_properties(gpu_ctx, oracle):
    """BASELINE configs[1] at its full size (all 1e6 rows of the table, j_I and alpha_I, one launch), checked
    through properties that do not need the oracle on every row:
      * every selected slot is a positive finite number or NaN with a non-zero status word, never anything else
        (power-law j_I and alpha_I are positive: all 200 golden rows are), unselected slots are NaN;
      * 16384 rows drawn from all over the table and recomputed in a launch of their own have the same bits
        (a row's result depends on nothing but the row);
      * 64 of those rows agree bit for bit with the CPU oracle."""
    n = 1_000_000
    kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_jI_aI", n)
    out, st = gpu_ctx.compute_batch(kind, s, th, params, mask, want_status=True)
    sel = out[:, :2]
    nan = np.isnan(sel)
    assert ((sel > 0) & np.isfinite(sel) | nan).all()
    assert (st[:, :2][nan] != 0).all() and (st[:, :2][~nan] == 0).all()
    assert nan.mean() < 2e-3, nan.mean()
    assert np.isnan(out[:, 2:]).all()
    rng = np.random.default_rng(20250614)
    rows = np.sort(rng.choice(n, 16384, replace=False))
    again = gpu_ctx.compute_batch(kind, s[rows], th[rows], [p[rows] for p in params], mask)
    assert same_bits(sel[rows], again[:, :2]).all()
    few = rows[:: len(rows) // 64][:64]
    ref = oracle_bind.batch(oracle, kind, s[few], th[few], [p[few] for p in params], mask, nthreads=16)
    report_mismatch("full-size table vs oracle", sel[few], ref[:, :2])


@pytest.mark.parametrize("cfg", ["cfg2_powerlaw_8", "cfg3_thermal_8", "cfg4_pitchypl_8", "cfg5_pitchykappa_8"])
def test_all_eight_table_properties(gpu_ctx, cfg):
    """The same properties for the eight-coefficient configurations on 16384 rows each.  (Their full sizes are minutes, not
    hours, of one GPU -- configs[2]'s 1e7 thermal rows about 5 minutes, a GPU's 1.25e6-row share of configs[3] about 2 --
    which is still too long for a test: the full-size runs are tools/full_size_run.py, profiles/r4_full_size_*.txt, with
    the same properties checked tile by tile.)  NaN <=> the NONFINITE status bit in every slot, j_I and alpha_I positive where
    finite for the isotropic distributions, and
    2048 scattered rows recomputed alone give the same bits in all eight slots."""
    n = 16384
    kind, mask, s, th, params = workload.make_batch(cfg, n, start=500000)
    out, st = gpu_ctx.compute_batch(kind, s, th, params, mask, want_status=True)
    nan = np.isnan(out)
    assert (np.isfinite(out) | nan).all()
    # RIMPHONY_ST_NONFINITE (16) marks exactly the NaN slots; the other bits record failed inner quadratures, which do
    # not always reach the result (a failed step-size probe of the Faraday chunk marching, for instance)
    assert ((st & 16) != 0)[nan].all() and ((st & 16) == 0)[~nan].all() and ((st & 64) == 0).all()
    if kind in (0, 1):          # isotropic distributions: j_I, alpha_I > 0 (anisotropic ones can have alpha_I < 0)
        assert (out[:, :2][~nan[:, :2]] > 0).all()
    # failed quadratures (the reference's NaN) are a few per cent of the cold-thermal and pitchy slots; the sweeps in
    # profiles/r1_parity_sweep.txt show the oracle fails on exactly the same ones
    assert nan[:, :2].mean() < 0.05 and nan.mean() < 0.15, (nan[:, :2].mean(), nan.mean())
    rows = np.sort(np.random.default_rng(7).choice(n, 2048, replace=False))
    again = gpu_ctx.compute_batch(kind, s[rows], th[rows], [p[rows] for p in params], mask)
    assert same_bits(out[rows], again).all()


def test_pitchy_k0_equals_power_law_on_gpu(gpu_ctx):
    """pitchy_pl.rs:142-201 (k = 0 makes the pitch-angle factor 1): the reference's 5 x 3 choice table plus 256
    rows of the cfg 2 table, all EIGHT coefficients -- the Faraday pair included, as in the reference's k_zero_rq /
    k_zero_rv.  The two distributions order the operations of f and df/dgamma differently and normalise through
    different closed forms, so the bar is north_star's 1e-6 relative, not bit equality."""
    SS, TH, PS = [1e0, 1e1, 1e2, 1e3, 1e4], [0.05, 0.430, 0.810, 1.190, 1.5707], [1.5, 1.75, 2.5, 3.25, 4.]
    CH = [1, 4, 2, 3, 1, 0, 0, 3, 1, 2, 0, 4, 4, 2, 3]
    pts = [(SS[CH[b]], TH[CH[b + 1]], PS[CH[b + 2]]) for b in range(0, 15, 3)]
    _, _, s2, th2, par2 = workload.make_batch("cfg2_powerlaw_8", 256, start=42000)
    s = np.concatenate([[q[0] for q in pts], s2])
    th = np.concatenate([[q[1] for q in pts], th2])
    p = np.concatenate([[q[2] for q in pts], par2[0]])
    gmin = np.concatenate([np.ones(len(pts)), par2[1]])
    n = len(s)
    gmax, gc = 1e12 * np.ones(n), 1e10 * np.ones(n)
    a = gpu_ctx.compute_batch(0, s, th, [p, gmin, gmax, gc], 0xFF)
    b = gpu_ctx.compute_batch(2, s, th, [p, np.zeros(n), gmin, gmax, gc], 0xFF)
    assert (np.isnan(a) == np.isnan(b)).mean() > 0.99      # a failed quadrature may differ on a borderline row
    both = np.isfinite(a) & np.isfinite(b)
    assert both[:len(pts), :6].all()
    with np.errstate(all="ignore"):
        rel = np.abs(a / b - 1)
    assert rel[both].max() < REL_TOL, rel[both].max()


def test_cooperative_tail_changes_no_bit(gpu_ctx):
    """The assist board only changes WHO evaluates a gamma-integral / inner integral: a context created with
    RIMPHONY_NO_ASSIST=1 (one wave per task to the end) must return the same bits, status words included, for
    all eight coefficients -- on a batch small enough that most of it runs in the cooperative regime."""
    import os
    from rimphony_amd import api
    kind, mask, s, th, params = workload.make_batch("cfg4_pitchypl_8", 96, start=5000)
    coop, st_coop = gpu_ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True)
    old = os.environ.get("RIMPHONY_NO_ASSIST")
    os.environ["RIMPHONY_NO_ASSIST"] = "1"
    try:
        solo_ctx = api.Context(0)
    finally:
        if old is None:
            del os.environ["RIMPHONY_NO_ASSIST"]
        else:
            os.environ["RIMPHONY_NO_ASSIST"] = old
    solo, st_solo = solo_ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True)
    solo_ctx.close()
    assert same_bits(coop, solo).all()
    assert (st_coop == st_solo).all()


def test_hostile_parameter_values_terminate_and_match(gpu_ctx, oracle):
    """A drop-in gets whatever arrays the caller has: zero / negative / NaN / infinite / out-of-range values of every
    power-law input, one at a time around a sane point (theta beyond pi/2, gamma_min > gamma_max, cutoff 0 ...).
    The reference has no input validation -- such points run through the same arithmetic and mostly end as NaN.
    The launch must end (a persistent kernel that spins on a bad point would hang the caller) and every slot,
    status word included, must carry the oracle's bits."""
    nan, inf = float("nan"), float("inf")
    base = dict(s=10.0, th=0.8, p=2.5, gmin=1.0, gmax=1e12, gc=1e10)
    hostile = dict(
        s=[0.0, -1.0, nan, inf, 1e-300, 1e-5, 1e8, 1e12],
        th=[0.0, -0.5, math.pi / 2, math.pi / 2 + 0.3, 3.0, math.pi, nan, inf, 1e-8, 1e-3],
        p=[0.0, -2.0, nan, inf, 50.0, 1.0, 0.5],
        gmin=[0.0, -1.0, 0.5, nan, 1e13, 1.0000001],
        gmax=[0.5, 1.0, nan, inf, 2.0],
        gc=[0.0, -1.0, nan, inf, 1e-3, 1.0])
    pts = []
    for key, vals in hostile.items():
        for v in vals:
            c = dict(base)
            c[key] = v
            pts.append(c)
    col = lambda k: np.array([c[k] for c in pts])
    s, th = col("s"), col("th")
    params = [col("p"), col("gmin"), col("gmax"), col("gc")]
    got, st = gpu_ctx.compute_batch(0, s, th, params, 0xFF, want_status=True)
    ref = oracle_bind.batch(oracle, 0, s, th, params, 0xFF, nthreads=16)
    report_mismatch("hostile inputs", got, ref, extra=lambda i: pts[i // 8])
    nanslot = np.isnan(got)
    assert ((st & 16) != 0)[nanslot].all() and ((st & 16) == 0)[~nanslot].all()
    assert np.isfinite(got[len(hostile["s"]) + 3]).all()      # theta = pi/2 + 0.3 is a legitimate angle


@pytest.mark.parametrize("kind", [1, 2, 3])
def test_hostile_parameter_values_other_distributions(gpu_ctx, oracle, kind):
    """The same for thermal (T), pitchy power law (k) and pitchy kappa (kappa, width, k, cutoff)."""
    nan, inf = float("nan"), float("inf")
    if kind == 1:
        rows = [[T] for T in [0.0, -1.0, nan, inf, 1e-3, 1e-2, 1e4, 1e8]]
    elif kind == 2:
        rows = [[2.5, k, 1.0, 1e12, 1e10] for k in [-1.0, -3.0, nan, inf, 50.0, 0.0]]
    else:
        rows = [[kap, 5.0, 1.0, 1e10] for kap in [0.0, -1.0, nan, inf, 0.5, 100.0]]
        rows += [[3.0, w, 1.0, 1e10] for w in [0.0, -1.0, nan, inf, 1e-3, 1e6]]
        rows += [[3.0, 5.0, k, 1e10] for k in [-1.0, nan, inf, 50.0]]
        rows += [[3.0, 5.0, 1.0, gc] for gc in [0.0, -1.0, nan, inf, 1.0]]
        # the kappa term leaves the domain of the kernels' restricted power function here (1^inf; a negative base
        # with an integer exponent, which powf defines): dist_prepare routes such points to the general rim_pow
        rows += [[-3.0, 5.0, 1.0, 1e10], [-inf, 5.0, 1.0, 1e10], [1e-200, -2.5, 1.0, 1e10], [inf, -1.0, 1.0, 1e10],
                 [inf, inf, 1.0, 1e10], [1e200, 1e200, 1.0, 1e10]]
    n = len(rows)
    params = [np.array([r[j] for r in rows]) for j in range(len(rows[0]))]
    s, th = np.full(n, 10.0), np.full(n, 0.8)
    got, st = gpu_ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True)
    ref = oracle_bind.batch(oracle, kind, s, th, params, 0xFF, nthreads=16)
    report_mismatch("hostile inputs, kind %d" % kind, got, ref, extra=lambda i: rows[i // 8])
    nanslot = np.isnan(got)
    assert ((st & 16) != 0)[nanslot].all() and ((st & 16) == 0)[~nanslot].all()


def test_api_misuse_is_an_error_code_not_a_crash(gpu_ctx):
    """Error convention of the boundary: negative return on misuse, never an abort."""
    import ctypes
    from rimphony_amd import capi
    lib = capi.load()
    h = gpu_ctx.handle
    one = (ctypes.c_double * 1)(1.0)
    pp = (ctypes.c_void_p * 4)(None, None, None, None)
    out = (ctypes.c_double * 8)()
    # distribution kind out of range, null arrays, null context
    assert lib.rimphony_batch_compute_device(h, 7, 1, one, one, pp, 0xFF, out, None, None) < 0
    assert lib.rimphony_batch_compute_device(h, 0, 1, None, None, pp, 0xFF, out, None, None) < 0
    assert lib.rimphony_batch_compute_device(None, 0, 1, one, one, pp, 0xFF, out, None, None) < 0
    assert lib.rimphony_highfreq_batch_device(h, 2, 1, one, one, pp, out, None) < 0        # no HF form for pitchy_pl
    assert lib.rimphony_dist_nparams(-1) < 0
    lib.rimphony_strerror.restype = ctypes.c_char_p
    assert lib.rimphony_strerror(-1) and lib.rimphony_strerror(-4)
    # the context is still usable afterwards
    got = gpu_ctx.compute_batch(0, [10.0], [0.8], [[2.5], [1.0], [1e12], [1e10]], 0x03)
    assert np.isfinite(got[0, :2]).all()


def test_n_integral_diagnostic_bit_exact(gpu_ctx, oracle):
    """diagnostic_symphony_n_integral (lib.rs:254-260): the outer QAG over n of the gamma-integral on [n_lo, n_hi]."""
    rng = np.random.default_rng(31)
    params = [2.8, 1.0, 1e12, 1e10]
    s, th = 30., 0.9
    d, st = oracle_bind.mkdist(oracle, 0, params)
    assert st == 0
    n_minus = s * math.sin(th)
    lo = n_minus + 31. + rng.uniform(0., 50., 24)
    hi = lo * rng.uniform(1.05, 3., 24)
    for coeff, stokes, lobe in ((0, 0, 0), (1, 1, 0), (0, 2, 1)):
        got = gpu_ctx.n_integral_batch(0, params, coeff, stokes, lobe, s, th, lo, hi)
        ref = np.array([oracle_bind.n_integral(oracle, d, coeff, stokes, lobe, s, th, a, b) for a, b in zip(lo, hi)])
        report_mismatch("n_integral", got, ref, lambda i: (coeff, stokes, lo[i], hi[i]))
        assert np.isfinite(ref).sum() > 12


def test_deriv_central_seam_bit_exact(gpu_ctx, oracle):
    """gsl::deriv_central (gsl.rs:233-257 -> gsl_deriv_central: central_deriv with h, then the optimal-step refinement) as
    n_integration drives it (symphony.rs:238-240): the derivative-probe phases of the state machine against the oracle's
    rimo_deriv_central on the oracle's gamma-integral, bit for bit.  The inputs include abscissae where the refinement is
    taken (round-off below truncation error) and where it is not."""
    rng = np.random.default_rng(33)
    cases = ((0, [2.8, 1.0, 1e12, 1e10], 30., 0.9), (1, [8.0], 200., 0.6), (3, [3.0, 5.0, 1.5, 1e10], 12., 1.2))
    for kind, params, s, th in cases:
        d, st = oracle_bind.mkdist(oracle, kind, params)
        assert st == 0
        n_minus = s * math.sin(th)
        n0 = np.floor(n_minus + 31. + rng.uniform(0., 400., 20))
        n0[10:] = n0[10:] * rng.uniform(1.5, 40., 10)          # non-integer starts further out in the tail
        for coeff, stokes, lobe in ((0, 0, 0), (1, 1, 0), (0, 2, 1)):
            got = gpu_ctx.deriv_probe_batch(kind, params, coeff, stokes, lobe, s, th, n0)
            ref = np.array([oracle.rimo_symphony_deriv_probe(ctypes.byref(d), coeff, stokes, lobe, s, th, float(x)) for x in n0])
            report_mismatch("deriv_central", got, ref, lambda i: (kind, coeff, stokes, n0[i]))
            assert np.isfinite(ref).sum() >= 10


def test_gamma_contribution_diagnostic_bit_exact(gpu_ctx, oracle):
    """diagnostic_symphony_gamma_contribution (lib.rs:288-296): fully discrete sums (few harmonics) and the
    31-discrete + QAG-over-n branch (more than 1000 harmonics)."""
    rng = np.random.default_rng(32)
    params = [2.8, 1.0, 1e12, 1e10]
    d, st = oracle_bind.mkdist(oracle, 0, params)
    assert st == 0
    for s, th, glo, ghi in ((8., 0.9, 1.5, 30.), (400., 0.6, 3., 40.)):
        gam = np.exp(rng.uniform(math.log(glo), math.log(ghi), 12))
        for coeff, stokes in ((0, 0), (1, 1)):
            got = gpu_ctx.gamma_contribution_batch(0, params, coeff, stokes, s, th, gam)
            ref = np.array([oracle.rimo_gamma_contribution(ctypes.byref(d), coeff, stokes, s, th, float(x)) for x in gam])
            report_mismatch("gamma_contribution", got, ref, lambda i: (s, coeff, stokes, gam[i]))
            assert np.isfinite(ref).sum() >= 6


HEY_SEAM_POINTS = [   # (kind, params, s, theta): sigma0 = s sin(theta) spans the J/Y branch (< 3) and the large-order branches
    (1, [10.], 4e4, 0.4), (1, [0.3], 1.5, 0.6), (0, [2.5, 1., 1e12, 1e10], 2.0, 0.9), (0, [3.1, 1., 1e12, 1e10], 60., 1.1),
    (2, [2.8, 1.2, 1., 1e12, 1e10], 25., 0.7), (3, [3.3, 6.0, 0.8, 1e10], 9., 0.5),
]


@pytest.mark.parametrize("case", range(len(HEY_SEAM_POINTS)))
def test_heyvaerts_elements_bit_exact(gpu_ctx, oracle, case):
    """h_qr / h_nr / f_qr / f_nr_element (heyvaerts.rs:302-468), the inner integrands of the Faraday double integral,
    sample by sample against the oracle's restatement."""
    kind, par, s, th = HEY_SEAM_POINTS[case]
    rng = np.random.default_rng(700 + case)
    d, st = oracle_bind.mkdist(oracle, kind, par)
    assert st == 0
    for stokes in (1, 2):
        for qr in (0, 1):
            fixed, v = hey_seam_inputs(rng, s, th, qr, 1536)
            got = gpu_ctx.hey_element_batch(kind, par, stokes, s, th, qr, fixed, v)
            ref = np.array([oracle.rimo_hey_element(ctypes.byref(d), stokes, s, th, qr, float(a), float(b)) for a, b in zip(fixed, v)])
            report_mismatch("hey_element case %d stokes %d qr %d" % (case, stokes, qr), got, ref, lambda i: (fixed[i], v[i]))
            assert np.isfinite(ref).sum() > 1000


@pytest.mark.parametrize("case", range(len(HEY_SEAM_POINTS)))
def test_heyvaerts_outer_integrands_bit_exact(gpu_ctx, oracle, case):
    """nr_outer_integrand / qr_outer_integrand (heyvaerts.rs:213-250, 262-296): one inner QAG per abscissa, the wave-level
    quadrature of the Faraday kernel, against the oracle (NaN where the inner integral fails; exactly 0 where the sigma
    range is empty)."""
    kind, par, s, th = HEY_SEAM_POINTS[case]
    rng = np.random.default_rng(800 + case)
    d, st = oracle_bind.mkdist(oracle, kind, par)
    assert st == 0
    n = 40
    for stokes in (1, 2):
        for qr in (0, 1):
            u = hey_outer_abscissae(rng, s, th, qr, n)
            got = gpu_ctx.hey_outer_batch(kind, par, stokes, s, th, qr, u)
            ref = np.array([oracle.rimo_hey_outer_integrand(ctypes.byref(d), stokes, s, th, qr, float(x)) for x in u])
            report_mismatch("hey_outer case %d stokes %d qr %d" % (case, stokes, qr), got, ref, lambda i: u[i])
            assert np.isfinite(ref).sum() > n // 2


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_distribution_function_seam_bit_exact(gpu_ctx, oracle, kind):
    """DistributionFunction::calc_f / calc_f_derivatives (lib.rs:111-146) through the C ABI against the oracle's
    restatement, bit for bit, with the distribution's own normalisation and with norm = 1."""
    rng = np.random.default_rng(50 + kind)
    par = {0: [2.7, 3.0, 1e7, 1e5], 1: [4.0], 2: [3.1, 1.4, 2.0, 1e8, 1e6], 3: [3.3, 6.0, 0.8, 1e4]}[kind]
    n = 512
    gamma = np.exp(rng.uniform(math.log(1.0001), math.log(2e7), n))
    cos_xi = rng.uniform(-0.99, 0.99, n)
    d, st = oracle_bind.mkdist(oracle, kind, par)
    assert st == 0
    for norm in (None, 1.0):
        if norm is not None:
            d.norm = norm
        f, dg, dc = gpu_ctx.calc_f_batch(kind, par, gamma, cos_xi, norm)
        rf = np.array([oracle.rimo_calc_f(d, g, c) for g, c in zip(gamma, cos_xi)])
        rdg, rdc = np.empty(n), np.empty(n)
        a, b = ctypes.c_double(), ctypes.c_double()
        for i in range(n):
            oracle.rimo_calc_f_derivatives(d, gamma[i], cos_xi[i], ctypes.byref(a), ctypes.byref(b))
            rdg[i], rdc[i] = a.value, b.value
        report_mismatch("calc_f kind %d" % kind, f, rf)
        report_mismatch("dfdg kind %d" % kind, dg, rdg)
        report_mismatch("dfdcx kind %d" % kind, dc, rdc)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_distribution_function_seam_hostile_arguments(gpu_ctx, oracle, kind):
    """calc_f / calc_f_derivatives on every pair of awkward gammas (0, below 1, 1, beyond gamma_max, negative, NaN,
    inf, subnormal) and pitch-angle cosines (+-1, beyond 1, NaN, inf): the oracle's bits (tools/calc_f_hostile.py)."""
    import itertools
    nan, inf = float("nan"), float("inf")
    gs = [0., -0., 0.5, 1., 1.0000000000000002, 1.5, 10., 1e6, 1e12, 1e13, 1e100, 1e300, inf, -1., -inf, nan, 1e-320]
    cs = [-1., 1., 0., -0., 0.5, -0.5, 0.9999999999999999, 1.5, -1.5, nan, inf, 1e-320]
    par = {0: [2.7, 1.0, 1e12, 1e10], 1: [4.0], 2: [3.1, 1.4, 1.0, 1e12, 1e10], 3: [3.3, 6.0, 0.8, 1e10]}[kind]
    pairs = np.array(list(itertools.product(gs, cs)))
    g, c = pairs[:, 0].copy(), pairs[:, 1].copy()
    d, st = oracle_bind.mkdist(oracle, kind, par)
    f, dg, dc = gpu_ctx.calc_f_batch(kind, par, g, c, None)
    rf = np.array([oracle.rimo_calc_f(d, a, b) for a, b in zip(g, c)])
    rdg, rdc = np.empty(len(g)), np.empty(len(g))
    x, y = ctypes.c_double(), ctypes.c_double()
    for i in range(len(g)):
        oracle.rimo_calc_f_derivatives(d, g[i], c[i], ctypes.byref(x), ctypes.byref(y))
        rdg[i], rdc[i] = x.value, y.value
    report_mismatch("calc_f hostile kind %d" % kind, f, rf, lambda i: (g[i], c[i]))
    report_mismatch("dfdg hostile kind %d" % kind, dg, rdg, lambda i: (g[i], c[i]))
    report_mismatch("dfdcx hostile kind %d" % kind, dc, rdc, lambda i: (g[i], c[i]))


@pytest.mark.parametrize("which", ["pitchy_pl", "pitchy_kappa"])
def test_reference_derivative_tests_on_gpu(gpu_ctx, which):
    """pitchy_pl.rs:203-238 and pitchy_kappa.rs:135-173 as the reference writes them -- a distribution object,
    `norm = 1` ("fake this"), calc_f_derivatives against forward differences of calc_f with EPS 1e-6, TOL 1e-4,
    100 random draws -- with calc_f evaluated by the HIP library."""
    from rimphony_amd import api
    rng = np.random.default_rng(3)
    EPS, TOL = 1e-6, 1e-4
    for _ in range(100):
        if which == "pitchy_pl":
            dist = api.PitchyPowerLawDistribution(2. + 3. * rng.random(), 0. + 3. * rng.random())
        else:
            dist = api.PitchyKappaDistribution(1.5 + 3. * rng.random(), math.exp(1. + 2. * rng.random()), 3. * rng.random())
        dist.ctx = gpu_ctx
        dist.norm = 1.                                   # fake this
        gamma, cos_xi = 1.1 + 1e3 * rng.random(), 0.01 + 0.98 * rng.random()
        analytic_dfdg, analytic_dfdcx = dist.calc_f_derivatives(gamma, cos_xi)
        f0 = dist.calc_f(gamma, cos_xi)
        numeric_dfdg = (dist.calc_f(gamma + EPS, cos_xi) - f0) / EPS
        numeric_dfdcx = (dist.calc_f(gamma, cos_xi + EPS) - f0) / EPS
        assert abs((analytic_dfdg - numeric_dfdg) / numeric_dfdg) < TOL, (gamma, cos_xi, analytic_dfdg, numeric_dfdg)
        assert abs((analytic_dfdcx - numeric_dfdcx) / numeric_dfdcx) < TOL, (gamma, cos_xi, analytic_dfdcx, numeric_dfdcx)


def test_cxx_mirror_builds_and_runs(tmp_path, gpu_ctx):
    """The header-only C++ mirror of the reference API (rimphony_amd/cxx/rimphony.hpp) over the C ABI: the
    counterpart of examples/one-powerlaw-direct.rs (j_I within 1e-3 of Symphony's printed value), a
    high-frequency closed form and one derivative check through the DistributionFunction trait; the program exits
    0 when all hold."""
    import os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "one_powerlaw_direct"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(root, "include"),
                    os.path.join(root, "rimphony_amd", "cxx", "one_powerlaw_direct.cpp"),
                    "-L", os.path.join(root, "rimphony_amd"), "-lrimphony_hip",
                    "-Wl,-rpath," + os.path.join(root, "rimphony_amd"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ours = float(r.stdout.split("Ours:")[1].split()[0])
    pl = gpu_ctx.compute_batch(0, [1e9 / (4.80320680e-10 * 1e3 / (2 * math.pi * 9.1093826e-28 * 2.99792458e10))], [0.9],
                               [[2.5], [1.0], [1e12], [1e10]], 0x01)
    assert abs(ours / (pl[0, 0] * 1e9) - 1.) < 1e-5          # printed with %e: 7 significant digits
