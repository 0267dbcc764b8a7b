"""The pitch-angle factor g(cos xi) of the tabulated distribution without a GPU: the C entry
rimphony_ctx_set_tables_pitch and its mirrors, what the host check refuses, the layout of a pitch set next to an isotropic
one, the spline G = ln g, g, G' and P = 1/2 int g dmu against a reference written from the mathematics (mpmath, 40
digits), the isotropic limit G = 0, consistent derivatives, and all eight coefficients of an exponential beam against an
ANALYTIC distribution (tests/support/beam_oracle.cpp) that shares no code with the tables.  The library's side is the
pitch oracle (tests/support/liboracle_tabpitch.so): the host build of the device functions and of rim_tab_build_pitch.
CPU only.

Every bound marked MEASURED is 4 x a figure measured on the host build against the reference named there (every test
prints its figure, `pytest -s`)."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

import tab_bind
import tab_pitch_bind as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_det.npz")
GOLD = os.path.join(ROOT, "tests", "golden", "symphony-powerlaw.txt")
mp = mpmath.mp
U52 = 2.0 ** -52
MARGIN = 4.0
EDGE_LO, EDGE_HI = 1.01, 1e4
ENTRY = "rimphony_ctx_set_tables_pitch"


def ulps(a, b):
    return abs(a - b) / np.spacing(abs(b))


# ---- 1. the entry and its mirrors ----------------------------------------------------------------------------------------
def test_entry_in_library_header_and_mirrors():
    from rimphony_amd import _build, capi
    _build.build_hip()
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, ENTRY)
    fn = getattr(lib, ENTRY)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                   ctypes.c_size_t, ctypes.c_void_p]
    assert fn(None, 0, 0, 1.0, 2.0, None, 0, None) == -1            # a null context is refused before anything is touched
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    assert re.search(r"int rimphony_ctx_set_tables_pitch\(rimphony_ctx \*ctx, size_t n_tables, size_t n_nodes, double gamma_lo, "
                     r"double gamma_hi,\s+const double \*log_n, size_t n_mu, const double \*log_g\);", hdr)
    assert ENTRY in capi.SYMBOLS
    rs = open(os.path.join(ROOT, "rimphony-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn rimphony_ctx_set_tables_pitch\(", rs)
    hpp = open(os.path.join(ROOT, "rimphony_amd", "cxx", "rimphony.hpp")).read()
    assert ENTRY in hpp and re.search(r"TabulatedDistribution\(double gamma_lo, double gamma_hi, std::vector<double> log_n, "
                                      r"std::vector<double> log_g\)", hpp)


# ---- 2. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    """Each through api.check_pitch_tables and through the library's own host check (rim_tab_check_pitch, reached as the
    pitch oracle reaches it); a refused set leaves the oracle's previous one in place.  The wrong row count has no form in
    the C entry -- log_g is a bare pointer read as [n_tables][n_mu] -- so that one is the Python mirror's alone."""
    from rimphony_amd import api
    good_n = np.linspace(0.0, -30.0, 16)
    good_g = tp.log_g_beam(16, 0.5, 0.25)
    t, g = api.check_pitch_tables(1.0, 1e3, good_n, good_g)
    assert t.shape == (1, 16) and g.shape == (1, 16)
    assert api.check_pitch_tables(1.0, 1e3, good_n)[1] is None and api.check_pitch_tables(1.0, 1e3, good_n, None, 0)[1] is None
    assert tp.set_tables(1.0, 1e3, good_n, good_g) == 0
    before = tp.blob()
    nan_g, inf_g = good_g.copy(), good_g.copy()
    nan_g[5], inf_g[0] = np.nan, -np.inf
    for log_g, n_mu in ((good_g[:7], None),             # n_mu of 7
                        (nan_g, None), (inf_g, None),   # a NaN, a -inf
                        (good_g, 0),                    # log_g given with n_mu = 0
                        (None, 16)):                    # n_mu given with log_g = NULL
        with pytest.raises(ValueError):
            api.check_pitch_tables(1.0, 1e3, good_n, log_g, n_mu)
        assert tp.set_tables(1.0, 1e3, good_n, log_g, n_mu) == -1
        assert np.array_equal(tp.blob(), before)
    with pytest.raises(ValueError):
        api.check_pitch_tables(1.0, 1e3, good_n, np.stack([good_g, good_g]))       # two pitch rows for one table
    with pytest.raises(ValueError):
        api.TabulatedDistribution(1.0, 1e3, good_n, nan_g)
    # what check_tables refuses is refused with a good log_g too
    with pytest.raises(ValueError):
        api.check_pitch_tables(10.0, 5.0, good_n, good_g)
    assert tp.set_tables(10.0, 5.0, good_n, good_g) == -1
    d = api.TabulatedDistribution.from_function(lambda x: x ** -2.5 * np.exp(-30.0 / x - x / 500.0), 1.0, 1e4, 64,
                                                pitch_fn=lambda mu: np.exp(0.8 * mu - 1.5 * mu * mu))
    assert d.log_n.shape == (1, 64) and d.log_g.shape == (1, 257)
    assert np.abs(d.log_g[0] - tp.log_g_beam(257, 0.8, 1.5)).max() < 1e-15
    assert api.TabulatedDistribution(1.0, 1e3, good_n).log_g is None


# ---- 3. layout ----------------------------------------------------------------------------------------------------------
def test_layout_next_to_the_isotropic_set():
    """Without log_g the blob is tab_bind's, byte for byte (length 8 + 2 n_tables n_nodes, header word 7 = 0); with log_g
    everything from word 8 through the gamma rows is unchanged, word 7 holds n_mu and one pitch row per table follows: {n_mu - 2,
    1 / h, h, P}, then (G_j, M_j) pairs."""
    t = tab_bind.edge_tables(EDGE_LO, EDGE_HI, 64)
    assert tab_bind.set_tables(EDGE_LO, EDGE_HI, t) == 0
    iso = tab_bind.blob()
    assert len(iso) == 8 + 2 * 3 * 64 and iso[7] == 0
    assert tp.set_tables(EDGE_LO, EDGE_HI, t) == 0
    assert tp.blob().tobytes() == iso.tobytes()
    for n_mu in (8, 33):
        G = tp.edge_pitch(n_mu)
        assert tp.set_tables(EDGE_LO, EDGE_HI, t, G) == 0
        b = tp.blob()
        assert len(b) == len(iso) + 3 * (4 + 2 * n_mu)
        assert b[:7].tobytes() == iso[:7].tobytes() and b[7] == n_mu
        assert b[8:len(iso)].tobytes() == iso[8:].tobytes()
        h = 2.0 / (n_mu - 1)
        for k in range(3):
            head, Gk, Mk = tp.pitch_row(b, k)
            assert head[0] == n_mu - 2 and head[1] == 1.0 / h and head[2] == h
            assert (Gk == G[k]).all()
        assert np.abs(tp.pitch_row(b, 0)[2] - 1.0).max() < 1e-14        # a straight line has its slope at every node
        assert (tp.pitch_row(b, 1)[2] == 0).all()


# ---- 4. an independent reference --------------------------------------------------------------------------------------
class RefPitch:
    """The natural cubic spline through (mu_j, G_j), mu_j = -1 + j h, h = 2 / (n - 1), by its SECOND derivatives S_j (the
    library solves for the slopes): S_0 = S_last = 0, S_{j-1} + 4 S_j + S_{j+1} = 6 (G_{j+1} - 2 G_j + G_{j-1}) / h^2, a dense
    solve in mpmath at 40 digits; on [mu_j, mu_{j+1}], a = mu_{j+1} - mu, b = mu - mu_j:
    G = (S_j a^3 + S_{j+1} b^3) / (6 h) + (G_j / h - S_j h / 6) a + (G_{j+1} / h - S_{j+1} h / 6) b."""

    def __init__(self, G):
        mp.dps = 40
        self.y = y = [mp.mpf(float(v)) for v in G]
        self.n = n = len(G)
        self.h = h = mp.mpf(2) / (n - 1)
        A, rhs = mp.zeros(n - 2, n - 2), mp.zeros(n - 2, 1)
        for i in range(n - 2):
            A[i, i] = 4
            if i > 0:
                A[i, i - 1] = 1
            if i < n - 3:
                A[i, i + 1] = 1
            rhs[i] = 6 * (y[i + 2] - 2 * y[i + 1] + y[i]) / h ** 2
        sol = mp.lu_solve(A, rhs)
        self.S = [mp.mpf(0)] + [sol[i] for i in range(n - 2)] + [mp.mpf(0)]

    def slopes(self):
        y, S, h, n = self.y, self.S, self.h, self.n
        m = [(y[j + 1] - y[j]) / h - h * (2 * S[j] + S[j + 1]) / 6 for j in range(n - 1)]
        m.append((y[n - 1] - y[n - 2]) / h + h * (2 * S[n - 1] + S[n - 2]) / 6)
        return m

    def spline(self, mu):
        """(G, dG/dmu) at the mpf mu in [-1, 1]"""
        h = self.h
        j = min(max(int(mp.floor((mu + 1) / h)), 0), self.n - 2)
        a, b = -1 + (j + 1) * h - mu, mu - (-1 + j * h)
        Sj, Sk, yj, yk = self.S[j], self.S[j + 1], self.y[j], self.y[j + 1]
        val = (Sj * a ** 3 + Sk * b ** 3) / (6 * h) + (yj / h - Sj * h / 6) * a + (yk / h - Sk * h / 6) * b
        der = (-Sj * a ** 2 + Sk * b ** 2) / (2 * h) - (yj / h - Sj * h / 6) + (yk / h - Sk * h / 6)
        return val, der

    def pitch_integral(self):
        """P = 1/2 int exp(G) dmu: Gauss-Legendre, 20 points per node interval"""
        xs, ws = np.polynomial.legendre.leggauss(20)
        total = mp.mpf(0)
        for j in range(self.n - 1):
            for x, w in zip(xs, ws):
                mu = -1 + (j + (mp.mpf(float(x)) + 1) / 2) * self.h
                total += mp.mpf(float(w)) * mp.exp(self.spline(mu)[0])
        return total * self.h / 2 / 2


def wavy_row(n_mu):
    """a row that is neither a line nor a parabola: the spline's second derivatives all differ"""
    mu = tp.mu_nodes(n_mu)
    return 0.8 * mu - 1.5 * mu * mu + 0.4 * np.sin(3.0 * mu)


# Measured on the host build against RefPitch, rows (G = 1.0 mu, G = 0.8 mu - 1.5 mu^2, wavy_row) of each n_mu:
#   slope: max over rows and nodes of |M_j - M_ref_j| / max(|dG| / h)
#   g:     max over rows and 400 mu of |g / g_ref - 1| / ((1 + |G|) 2^-52), g = f gamma^2 beta at norm 1 on a table with n = 1
#   dG:    max over rows and the same mu of |dfdcx / f - G'_ref| / max(|dG| / h), in units of 2^-52
#   P:     max over rows of |P / P_ref - 1|.  P_ref is a 20-point Gauss-Legendre rule per interval, the library's a 31-point
#          Kronrod rule: both integrate the cubic-exponential to far below a rounding, so this is summation rounding.
MEASURED = {
    8: dict(slope=4.3e-16, g=2.3, dG=6.2, P=2.4e-16),
    64: dict(slope=4.0e-16, g=1.7, dG=3.7, P=1.4e-16),
}


def check(name, got, measured):
    print(name, "measured", got, "recorded", measured)
    assert measured is not None, "no figure recorded for %s: measured %r" % (name, got)
    assert got <= MARGIN * measured, (name, got, measured)


@pytest.mark.parametrize("n_mu", [8, 64])
def test_pitch_spline_against_mpmath(n_mu):
    rows = np.stack([tp.log_g_beam(n_mu, 1.0), tp.log_g_beam(n_mu, 0.8, 1.5), wavy_row(n_mu)])
    # a gamma table with n = 1: H = 0, so that f gamma^2 beta at norm 1 is g alone
    flat = np.zeros((3, 8))
    assert tp.set_tables(1.0, 1e3, flat, rows) == 0
    b = tp.blob()
    rng = np.random.default_rng(77 + n_mu)
    mu = np.concatenate([rng.uniform(-1, 1, 394), [-1.0, 1.0, 0.0, -0.5, np.nextafter(1.0, 0), np.nextafter(-1.0, 0)]])
    gamma = np.full(len(mu), 2.0)
    g2b = mp.mpf(4) * mp.sqrt(mp.mpf(3) / 4)
    worst = dict(slope=0.0, g=0.0, dG=0.0, P=0.0)
    for k in range(3):
        ref = RefPitch(rows[k])
        head, Gk, Mk = tp.pitch_row(b, k)
        scale = float(np.abs(np.diff(rows[k])).max() / (2.0 / (n_mu - 1)))
        want = ref.slopes()
        worst["slope"] = max(worst["slope"], max(float(abs(mp.mpf(float(Mk[j])) - want[j])) for j in range(n_mu)) / scale)
        f, _, dfdcx = tp.dev_calc_f([float(k)], 1.0, gamma, mu)
        assert (f > 0).all()
        for i in range(len(mu)):
            Gr, dGr = ref.spline(mp.mpf(float(mu[i])))
            g_err = abs(mp.mpf(float(f[i])) * g2b / mp.exp(Gr) - 1)
            worst["g"] = max(worst["g"], float(g_err) / ((1 + abs(float(Gr))) * U52))
            d_err = abs(mp.mpf(float(dfdcx[i])) / mp.mpf(float(f[i])) - dGr)
            worst["dG"] = max(worst["dG"], float(d_err) / scale / U52)
        worst["P"] = max(worst["P"], float(abs(mp.mpf(float(head[3])) / ref.pitch_integral() - 1)))
    for key in ("slope", "g", "dG", "P"):
        check("n_mu %d %s" % (n_mu, key), worst[key], MEASURED[n_mu][key])
    # the straight line: P = sinh(1), and a NaN mu gives NaN
    assert abs(tp.pitch_row(b, 0)[0][3] / np.sinh(1.0) - 1) < 1e-14
    f, a, c = tp.dev_calc_f([1.0], 1.0, np.array([2.0]), np.array([np.nan]))
    assert np.isnan(f[0]) and np.isnan(a[0]) and np.isnan(c[0])


# ---- 5. G = 0 -------------------------------------------------------------------------------------------------------------
def test_zero_pitch_row_is_the_isotropic_table():
    t = tab_bind.edge_tables(EDGE_LO, EDGE_HI, 64)
    rng = np.random.default_rng(5)
    gamma = np.concatenate([np.exp(rng.uniform(np.log(EDGE_LO), np.log(EDGE_HI), 2000)), [EDGE_LO, EDGE_HI, 1.0, 2e4]])
    mu = np.concatenate([rng.uniform(-1, 1, 2000), [-1.0, 1.0, 0.0, 0.3]])
    assert tab_bind.set_tables(EDGE_LO, EDGE_HI, t) == 0
    iso = [tab_bind.dev_calc_f(4, [float(k)], 1.0, gamma, mu) for k in range(3)]
    iso_norm = tab_bind.batch_norm([0.0, 1.0, 2.0])
    for n_mu in (8, 257):
        assert tp.set_tables(EDGE_LO, EDGE_HI, t, np.zeros((3, n_mu))) == 0
        b = tp.blob()
        norm = tp.batch_norm([0.0, 1.0, 2.0])
        for k in range(3):
            f, dfdg, dfdcx = tp.dev_calc_f([float(k)], 1.0, gamma, mu)
            assert f.tobytes() == iso[k][0].tobytes() and dfdg.tobytes() == iso[k][1].tobytes()
            assert (f[:2000] > 0).any() and (dfdcx == 0).all()     # (the Juettner table underflows to f = 0 at the top)
            P = tp.pitch_row(b, k)[0][3]
            print("n_mu", n_mu, "table", k, "P - 1 in ulp", ulps(P, 1.0), "norm in ulp", ulps(norm[k], iso_norm[k]))
            assert ulps(P, 1.0) <= 4 and ulps(norm[k], iso_norm[k]) <= 4


# ---- 6. derivatives -----------------------------------------------------------------------------------------------------
# Measured with the one-sided difference quotient of step 1e-6: max over the draws of |analytic - numeric| / |numeric|, the
# reference's form, and for d f / d mu also of |analytic - numeric| / (f max|G'|) ("dfdcx_scaled").  What is measured is the
# truncation error of the quotient, 1e-6 / 2 x |f'' / f'|, not an error of the derivative.  G' = 0.8 - 3 mu has a zero at
# mu0 = 0.8 / 3, where the relative form has a pole (the reference's sin^k factor has none in its range of draws): it is
# taken over the draws with |mu - mu0| >= 0.02, where 1e-6 / 2 x |G'' / G'| <= 2.5e-5; the scaled form covers every draw.
MEASURED_FD = dict(dfdg=2.7e-6, dfdcx=2.2e-5, dfdcx_scaled=4.0e-7)
FD_MU0, FD_KEEP = 0.8 / 3.0, 0.02


def test_derivatives_of_a_curved_pitch_row():
    """The finite-difference check of pitchy_pl.rs:203-238 (norm 1, step 1e-6, gamma = 1.1 + 1e3 u, cos xi = 0.01 + 0.98 u,
    100 draws) on the rolled power-law table with G = 0.8 mu - 1.5 mu^2 on 64 nodes, for both derivatives; the bounds are
    4 x the measured figures, all below the reference's own 1e-4."""
    EPS = 1e-6
    rng = np.random.default_rng(6)
    t = tab_bind.edge_tables(EDGE_LO, EDGE_HI, 2048)[:1]
    assert tp.set_tables(EDGE_LO, EDGE_HI, t, tp.log_g_beam(64, 0.8, 1.5)) == 0
    gamma = 1.1 + 1e3 * rng.random(100)
    cx = 0.01 + 0.98 * rng.random(100)
    f0, dfdg, dfdcx = tp.dev_calc_f([0.0], 1.0, gamma, cx)
    f1, _, _ = tp.dev_calc_f([0.0], 1.0, gamma + EPS, cx)
    f2, _, _ = tp.dev_calc_f([0.0], 1.0, gamma, cx + EPS)
    assert (f0 > 1e-250).all() and (dfdcx != 0).all()
    assert (dfdcx[cx < FD_MU0] > 0).all() and (dfdcx[cx > FD_MU0] < 0).all()      # the sign of G' = 0.8 - 3 mu
    num_g, num_c = (f1 - f0) / EPS, (f2 - f0) / EPS
    away = np.abs(cx - FD_MU0) >= FD_KEEP
    assert away.sum() >= 90
    check("dfdg", np.abs((dfdg - num_g) / num_g).max(), MEASURED_FD["dfdg"])
    check("dfdcx", np.abs((dfdcx[away] - num_c[away]) / num_c[away]).max(), MEASURED_FD["dfdcx"])
    check("dfdcx_scaled", (np.abs(dfdcx - num_c) / (f0 * 3.8)).max(), MEASURED_FD["dfdcx_scaled"])
    assert MARGIN * max(MEASURED_FD.values()) < 1e-4


# ---- 7., 8. against the analytic beam --------------------------------------------------------------------------------
PL_P, PL_CUT, PL_LO, PL_HI, PL_NODES = 2.5, 1e10, 1.0, 1e12, 2048      # the table of test_tabulated_power_law_against_kind_0


def beam_rows(a, b):
    """The rows of the golden file's (s, theta) list among the 16 committed pl_rows at which the ANALYTIC oracle alone
    returns eight finite values, and those values"""
    rows = np.load(FIXTURE)["pl_rows"]
    assert len(rows) == 16
    gold = np.loadtxt(GOLD)
    s, th = gold[rows, 0].copy(), gold[rows, 1].copy()
    ref = tp.beam_batch(s, th, [PL_P, PL_LO, PL_HI, PL_CUT, a, b])
    keep = np.isfinite(ref).all(axis=1)
    return s[keep], th[keep], ref[keep]


def table_rows(s, th, log_g):
    g = tab_bind.nodes(PL_LO, PL_HI, PL_NODES)
    assert tp.set_tables(PL_LO, PL_HI, tab_bind.log_n_powerlaw(g, PL_P, PL_CUT), log_g) == 0
    return tp.batch(s, th, np.zeros(len(s)))[0]


MEASURED_BEAM = {1.0: 3.3e-14, -0.7: 1.7e-14}


@pytest.mark.parametrize("a", [1.0, -0.7])
def test_straight_line_beam_against_the_analytic_oracle(a):
    """G = a mu on 8 nodes -- which the spline reproduces exactly -- on the 2048-node table of gamma^-2.5 exp(-gamma / 1e10)
    over [1, 1e12], all eight slots, against liboracle_beam; both signs of a, so that a mirrored mu or a wrong sign of
    d f / d mu shows.  Measured maximum relative difference: 3.3e-14 (a = +1), 1.7e-14 (a = -0.7); all 16 rows are finite in
    the analytic oracle for either sign.  (The isotropic table against kind 0 measured 3.5e-13.)"""
    s, th, ref = beam_rows(a, 0.0)
    print("a", a, "rows kept", len(s), "of 16")
    assert len(s) >= 12
    tab = table_rows(s, th, tp.log_g_beam(8, a))
    assert np.isfinite(tab).all() and np.isfinite(ref).all()
    rel = np.abs(tab / ref - 1.0)
    print("a", a, "max rel per slot", rel.max(axis=0))
    check("beam a = %g" % a, rel.max(), MEASURED_BEAM[a])


MEASURED_CURVED = {64: 1.23e-4, 1024: 3.4e-9}


def test_curved_beam_converges_to_the_analytic_oracle():
    """G = 0.8 mu - 1.5 mu^2 on 64 and on 1024 nodes against liboracle_beam on 4 of the rows above: the finer table agrees
    better than the coarser one.  Measured: 1.23e-4 on 64 nodes, 3.4e-9 on 1024 -- the natural end condition G'' = 0 at
    mu = +-1 against G'' = -3: an error of the spline of the table, not of its evaluation."""
    s, th, ref = beam_rows(0.8, 1.5)
    assert len(s) >= 4
    s, th, ref = s[:4], th[:4], ref[:4]
    worst = {}
    for n_mu in (64, 1024):
        tab = table_rows(s, th, tp.log_g_beam(n_mu, 0.8, 1.5))
        assert np.isfinite(tab).all()
        worst[n_mu] = np.abs(tab / ref - 1.0).max()
        print("n_mu", n_mu, "max rel per slot", np.abs(tab / ref - 1.0).max(axis=0))
    assert worst[1024] < worst[64]
    for n_mu in (64, 1024):
        check("curved n_mu %d" % n_mu, worst[n_mu], MEASURED_CURVED[n_mu])
