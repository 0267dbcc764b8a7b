"""2-D table sets of the tabulated distribution, ln n(gamma, mu) on a grid, without a GPU: the C entry
rimphony_ctx_set_tables_2d and its mirrors, what the host check refuses, the layout next to the two older forms, the
tensor-product natural spline S, S_u, S_mu against a reference written from the mathematics (mpmath, 40 digits), a bilinear
surface reproduced exactly, a separable table against the pitch oracle, and all eight coefficients of a tilted power law
against an ANALYTIC distribution (tests/support/tilt_oracle.cpp) that shares no code with the tables.  The library's side
is the 2-D oracle (tests/support/liboracle_tab2d.so): the host build of the device functions and of rim_tab_build_2d.
CPU only.

The bounds of tests 6 and 7 are 10 x a figure measured here on the host build (profiles/tabulated_2d_vs_analytic.txt;
every test prints its figure, `pytest -s`)."""
import ctypes
import hashlib
import os
import re

import mpmath
import numpy as np
import pytest

import tab_bind
import tab_pitch_bind as tp
import tab2d_bind as t2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISO_FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_det.npz")
PITCH_FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_pitch_det.npz")
FIXTURE_2D = os.path.join(ROOT, "tests", "golden", "tabulated_2d_det.npz")
GOLD = os.path.join(ROOT, "tests", "golden", "symphony-powerlaw.txt")
mp = mpmath.mp
U52 = 2.0 ** -52
EDGE_LO, EDGE_HI = t2.EDGE_LO, t2.EDGE_HI
ENTRY = "rimphony_ctx_set_tables_2d"


def check(name, got, measured, margin):
    print(name, "measured", got, "recorded", measured)
    assert measured is not None, "no figure recorded for %s: measured %r" % (name, got)
    assert got <= margin * measured, (name, got, measured)


# ---- 1. the entry and its mirrors ----------------------------------------------------------------------------------------
def test_entry_in_library_header_and_mirrors():
    from rimphony_amd import _build, api, capi
    _build.build_hip()
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, ENTRY)
    fn = getattr(lib, ENTRY)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, ctypes.c_size_t,
                   ctypes.c_void_p]
    assert fn(None, 0, 0, 1.0, 2.0, 0, None) == -1            # a null context is refused before anything is touched
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    assert re.search(r"int rimphony_ctx_set_tables_2d\(rimphony_ctx \*ctx, size_t n_tables, size_t n_nodes, double gamma_lo, "
                     r"double gamma_hi,\s+size_t n_mu, const double \*log_n\);", hdr)
    assert ENTRY in capi.SYMBOLS
    rs = open(os.path.join(ROOT, "rimphony-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn rimphony_ctx_set_tables_2d\(", rs)
    hpp = open(os.path.join(ROOT, "rimphony_amd", "cxx", "rimphony.hpp")).read()
    assert ENTRY in hpp and "void set_tables_2d(" in hpp and "class TabulatedDistribution2D" in hpp
    assert hasattr(api.Context, "set_tables_2d") and hasattr(api, "TabulatedDistribution2D") and hasattr(api, "check_tables_2d")


# ---- 2. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_without_a_gpu():
    """Each through api.check_tables_2d and through the library's own host check (rim_tab_check_2d, reached as the 2-D oracle
    reaches it); a refused set leaves the oracle's previous one in place."""
    from rimphony_amd import api
    good = t2.edge_tables_2d(16, 16)
    t = api.check_tables_2d(EDGE_LO, EDGE_HI, good)
    assert t.shape == (3, 16, 16) and api.check_tables_2d(EDGE_LO, EDGE_HI, good[0]).shape == (1, 16, 16)
    assert t2.set_tables(EDGE_LO, EDGE_HI, good, with_norm=False) == 0
    before = t2.blob()
    nan_t, inf_t = good.copy(), good.copy()
    nan_t[1, 5, 3], inf_t[2, 0, 15] = np.nan, -np.inf
    cases = ((good[:, :, :7], EDGE_LO, EDGE_HI),                    # n_mu of 7
             (np.zeros((1, 16, 1025)), EDGE_LO, EDGE_HI),           # n_mu of 1025
             (good[:, :7, :], EDGE_LO, EDGE_HI),                    # n_nodes of 7
             (np.zeros((1, 1025, 1024)), EDGE_LO, EDGE_HI),         # one gamma node's worth over 2^20 nodes per table
             (nan_t, EDGE_LO, EDGE_HI), (inf_t, EDGE_LO, EDGE_HI),  # a NaN, a -inf
             (good, 0.5, EDGE_HI), (good, 10.0, 10.0), (good, 10.0, 5.0))
    for log_n, lo, hi in cases:
        with pytest.raises(ValueError):
            api.check_tables_2d(lo, hi, log_n)
        assert t2.check(lo, hi, log_n) == -1
        assert t2.set_tables(lo, hi, log_n, with_norm=False) == -1
        assert np.array_equal(t2.blob(), before)
    # the cap itself is accepted: 1024 x 1024 nodes
    assert t2.check(EDGE_LO, EDGE_HI, np.zeros((1, 1024, 1024))) == 0
    assert api.check_tables_2d(EDGE_LO, EDGE_HI, np.zeros((1024, 1024))).shape == (1, 1024, 1024)
    with pytest.raises(ValueError):
        api.TabulatedDistribution2D(EDGE_LO, EDGE_HI, nan_t[1])
    with pytest.raises(ValueError):
        api.TabulatedDistribution2D(EDGE_LO, EDGE_HI, good)         # a set where one table is expected
    d = api.TabulatedDistribution2D.from_function(
        lambda g, mu: g ** (-2.5 + 0.3 * mu) * np.exp(-30.0 / g - g / 500.0 + 0.5 * mu), EDGE_LO, EDGE_HI)
    assert d.log_n.shape == (1, 512, 65)
    assert np.abs(d.log_n[0] - t2.table_tilted(512, 65)).max() < 1e-12


# ---- 3. layout ----------------------------------------------------------------------------------------------------------
# sha256 of the laid-out sets of the two older forms, recorded on the commit before the 2-D form existed: the committed
# tables of tabulated_pitch_det.npz over [1.01, 1e4], isotropic and with tab_pitch_bind.edge_pitch(33)
OLD_BLOBS = dict(iso="804c88bfa1190ca08f2bbc679c8bf2521a1cf2f6e59ad11f4cb4706163d99ac7",
                 pitch="4084b2451b16a2e26c19604bcc9f15c3c7e6dd01fc46374caea13a8752a2e32c")


def test_layout_next_to_the_older_forms():
    """An isotropic and a pitch set through the old builders are what they were, byte for byte.  A 2-D set: header word 7 =
    -n_mu, a header of 8 words per table {n_mu - 2, 1 / h_mu, h_mu, norm, 0, 0, 0, 0}, then [n_tables][n_nodes][n_mu][4] with
    the table's values in word 0 of every node."""
    pf = np.load(PITCH_FIXTURE)
    glo, ghi, tables = float(pf["gamma_lo"]), float(pf["gamma_hi"]), pf["tables"]
    assert tab_bind.set_tables(glo, ghi, tables) == 0
    iso = tab_bind.blob()
    assert tp.set_tables(glo, ghi, tables) == 0
    assert tp.blob().tobytes() == iso.tobytes() and iso[7] == 0
    assert tp.set_tables(glo, ghi, tables, tp.edge_pitch(33)) == 0
    pitch = tp.blob()
    assert pitch[7] == 33
    got = dict(iso=hashlib.sha256(iso.tobytes()).hexdigest(), pitch=hashlib.sha256(pitch.tobytes()).hexdigest())
    print(got)
    assert got == OLD_BLOBS
    for n_nodes, n_mu in ((64, 8), (16, 1024)):
        t = t2.edge_tables_2d(n_nodes, n_mu)
        assert t2.set_tables(EDGE_LO, EDGE_HI, t, with_norm=False) == 0
        b = t2.blob()
        assert len(b) == 8 + 3 * 8 + 3 * n_nodes * n_mu * 4
        assert b[0] == 3 and b[1] == n_nodes and b[2] == EDGE_LO and b[3] == EDGE_HI and b[7] == -n_mu
        h, hm = b[6], 2.0 / (n_mu - 1)
        assert b[5] == 1.0 / h and abs(h * (n_nodes - 1) / np.log(EDGE_HI / EDGE_LO) - 1) < 1e-15
        for k in range(3):
            head = t2.table_header(b, k)
            assert head[0] == n_mu - 2 and head[1] == 1.0 / hm and head[2] == hm and (head[3:] == 0).all()
            nodes = t2.table_nodes(b, k)
            assert nodes.shape == (n_nodes, n_mu, 4) and (nodes[:, :, 0] == t[k]).all()
        assert (t2.table_nodes(b, 1)[:, :, 2:] == 0).all()          # no mu dependence: S_mu = S_umu = 0 at every node
        assert (t2.table_nodes(b, 0)[:, :, 3] != 0).all()           # the tilt: a cross derivative everywhere
    # with the normalisations: word 3 of each table header, and nothing else moves
    assert t2.set_tables(EDGE_LO, EDGE_HI, t2.edge_tables_2d(64, 8), with_norm=False) == 0
    bare = t2.blob()
    assert t2.set_tables(EDGE_LO, EDGE_HI, t2.edge_tables_2d(64, 8)) == 0
    full = t2.blob()
    differs = np.flatnonzero(bare != full)
    assert differs.tolist() == [8 + 3, 16 + 3, 24 + 3] and (full[differs] > 0).all()
    assert (t2.batch_norm([0.0, 1.0, 2.0]) == full[differs]).all()


# ---- 4. an independent reference --------------------------------------------------------------------------------------
class RefSpline:
    """The natural cubic spline through (x_j, y_j), x_j = x0 + j h, by its SECOND derivatives (the library solves for the
    slopes): a dense solve in mpmath at 40 digits, as test_tabulated_pitch_host.RefPitch."""

    def __init__(self, y, x0, h):
        self.y, self.n, self.x0, self.h = list(y), len(y), x0, h
        n = self.n
        A, rhs = mp.zeros(n - 2, n - 2), mp.zeros(n - 2, 1)
        for i in range(n - 2):
            A[i, i] = 4
            if i > 0:
                A[i, i - 1] = 1
            if i < n - 3:
                A[i, i + 1] = 1
            rhs[i] = 6 * (self.y[i + 2] - 2 * self.y[i + 1] + self.y[i]) / h ** 2
        sol = mp.lu_solve(A, rhs)
        self.S = [mp.mpf(0)] + [sol[i] for i in range(n - 2)] + [mp.mpf(0)]

    def eval(self, x):
        """(value, derivative) at the mpf x; beyond the ends the end cubic goes on"""
        h = self.h
        j = min(max(int(mp.floor((x - self.x0) / h)), 0), self.n - 2)
        a, b = self.x0 + (j + 1) * h - x, x - (self.x0 + j * h)
        Sj, Sk, yj, yk = self.S[j], self.S[j + 1], self.y[j], self.y[j + 1]
        val = (Sj * a ** 3 + Sk * b ** 3) / (6 * h) + (yj / h - Sj * h / 6) * a + (yk / h - Sk * h / 6) * b
        der = (-Sj * a ** 2 + Sk * b ** 2) / (2 * h) - (yj / h - Sj * h / 6) + (yk / h - Sk * h / 6)
        return val, der


class RefSurface:
    """The tensor-product natural cubic spline through a grid, without the Hermite form: S(u, mu) is the natural spline in
    mu through the values at u of the natural splines in u through the columns; S_u the same through their derivatives."""

    def __init__(self, table, u_lo, u_hi):
        mp.dps = 40
        n_nodes, n_mu = table.shape
        self.hu = (u_hi - u_lo) / (n_nodes - 1)
        self.hm = mp.mpf(2) / (n_mu - 1)
        self.cols = [RefSpline([mp.mpf(float(v)) for v in table[:, j]], u_lo, self.hu) for j in range(n_mu)]

    def eval(self, u, mu):
        """(S, S_u, S_mu) at the mpf (u, mu)"""
        at_u = [c.eval(u) for c in self.cols]
        s, s_mu = RefSpline([v for v, _ in at_u], mp.mpf(-1), self.hm).eval(mu)
        s_u, _ = RefSpline([d for _, d in at_u], mp.mpf(-1), self.hm).eval(mu)
        return s, s_u, s_mu


def wavy_table(n_nodes, n_mu, lo, hi):
    """neither separable nor polynomial"""
    u = np.linspace(np.log(lo), np.log(hi), n_nodes)[:, None]
    mu = np.linspace(-1.0, 1.0, n_mu)[None, :]
    return -2.2 * u + 0.4 * np.sin(1.3 * u) * np.cos(2.0 * mu) + 0.25 * u * mu - 0.6 * mu * mu + 0.3 * np.sin(3.0 * mu + 0.5 * u)


# What test_tabulated_pitch_host.py holds the pitch spline to on 8 nodes (its MEASURED[8] x its MARGIN of 4), in its units:
# the value to 2.3 x 4 units of (1 + |S|) 2^-52, a derivative to 6.2 x 4 units of 2^-52 x the steepest chord of the table
# along that axis.
TOL_VALUE, TOL_DERIV = 4 * 2.3, 4 * 6.2


@pytest.mark.parametrize("shape", [(8, 8), (9, 12)])
def test_surface_against_mpmath(shape):
    """S, S_u, S_mu of tab_bicubic at random interior points, on nodes, on cell edges and at mu = +-1 (and a rounding beyond)
    against RefSurface.  The reference is evaluated at u = ln gamma of the double gamma, so rim_log's rounding of u is part
    of what is measured."""
    n_nodes, n_mu = shape
    lo, hi = 1.5, 4.0e3
    table = wavy_table(n_nodes, n_mu, lo, hi)
    assert t2.set_tables(lo, hi, table, with_norm=False) == 0
    mp.dps = 40
    u_lo, u_hi = mp.log(mp.mpf(lo)), mp.log(mp.mpf(hi))
    ref = RefSurface(table, u_lo, u_hi)
    rng = np.random.default_rng(100 * n_nodes + n_mu)
    un = np.linspace(np.log(lo), np.log(hi), n_nodes)
    mun = np.linspace(-1.0, 1.0, n_mu)
    gam, mus = [], []
    for _ in range(60):                                             # interior
        gam.append(np.exp(rng.uniform(np.log(lo), np.log(hi)))), mus.append(rng.uniform(-1, 1))
    for i in range(0, n_nodes, 3):                                  # nodes
        for j in range(0, n_mu, 3):
            gam.append(min(max(np.exp(un[i]), lo), hi)), mus.append(mun[j])
    for k in range(12):                                             # cell edges: one coordinate on a node line
        gam.append(min(max(np.exp(un[k % n_nodes]), lo), hi)), mus.append(rng.uniform(-1, 1))
        gam.append(np.exp(rng.uniform(np.log(lo), np.log(hi)))), mus.append(mun[k % n_mu])
    for m in (-1.0, 1.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)):     # mu = +-1 and a rounding beyond
        for _ in range(4):
            gam.append(np.exp(rng.uniform(np.log(lo), np.log(hi)))), mus.append(m)
    gam, mus = np.array(gam), np.array(mus)
    s, su, sm = t2.bicubic(0, gam, mus)
    scale_u = float(np.abs(np.diff(table, axis=0)).max() / float(ref.hu))
    scale_m = float(np.abs(np.diff(table, axis=1)).max() / float(ref.hm))
    worst = dict(S=0.0, S_u=0.0, S_mu=0.0)
    for i in range(len(gam)):
        r, ru, rm = ref.eval(mp.log(mp.mpf(float(gam[i]))), mp.mpf(float(mus[i])))
        worst["S"] = max(worst["S"], float(abs(mp.mpf(float(s[i])) - r)) / ((1 + abs(float(r))) * U52))
        worst["S_u"] = max(worst["S_u"], float(abs(mp.mpf(float(su[i])) - ru)) / scale_u / U52)
        worst["S_mu"] = max(worst["S_mu"], float(abs(mp.mpf(float(sm[i])) - rm)) / scale_m / U52)
    print(shape, "points", len(gam), worst, "bounds", TOL_VALUE, TOL_DERIV)
    assert worst["S"] <= TOL_VALUE and worst["S_u"] <= TOL_DERIV and worst["S_mu"] <= TOL_DERIV
    # a NaN gives NaN
    for g, m in ((np.nan, 0.3), (30.0, np.nan)):
        v = t2.bicubic(0, np.array([g]), np.array([m]))
        assert np.isnan(v[0][0]) and np.isnan(v[1][0]) and np.isnan(v[2][0])


# ---- 5. a bilinear surface ----------------------------------------------------------------------------------------------
def test_bilinear_surface_is_reproduced():
    """ln n = c - p u + a mu + q u mu on 8 x 8 nodes at 1000 random points.  The node values carry a rounding of up to half
    an ulp of the largest |S| each, and a slope is a difference of them over the spacing: the value is held to 4 ulp of
    max |S|, a derivative to 8 ulp of max |S| over the spacing of its axis."""
    lo, hi = 1.0, 1e3
    c, p, a, q = 1.0, 2.5, 0.7, 0.3
    u = np.linspace(np.log(lo), np.log(hi), 8)[:, None]
    mu = np.linspace(-1.0, 1.0, 8)[None, :]
    table = c - p * u + a * mu + q * u * mu
    assert t2.set_tables(lo, hi, table, with_norm=False) == 0
    rng = np.random.default_rng(5)
    g = np.exp(rng.uniform(np.log(lo), np.log(hi), 1000))
    m = rng.uniform(-1, 1, 1000)
    s, su, sm = t2.bicubic(0, g, m)
    mp.dps = 40
    ulp = float(np.spacing(np.abs(table).max()))
    hu, hm = float(u[1, 0] - u[0, 0]), 2.0 / 7
    worst = [0.0, 0.0, 0.0]
    for i in range(1000):
        ui, mi = mp.log(mp.mpf(float(g[i]))), mp.mpf(float(m[i]))
        worst[0] = max(worst[0], float(abs(mp.mpf(float(s[i])) - (c - p * ui + a * mi + q * ui * mi))) / ulp)
        worst[1] = max(worst[1], float(abs(mp.mpf(float(su[i])) - (-p + q * mi))) / (ulp / hu))
        worst[2] = max(worst[2], float(abs(mp.mpf(float(sm[i])) - (a + q * ui))) / (ulp / hm))
    print("bilinear: S, S_u, S_mu in ulp of max|S| (over the spacing)", worst)
    assert worst[0] <= 4 and worst[1] <= 8 and worst[2] <= 8


# ---- 6. a separable table against the pitch oracle --------------------------------------------------------------------
PL_P, PL_CUT, PL_LO, PL_HI, PL_NODES = 2.5, 1e10, 1.0, 1e12, 2048      # the table of the pitch host test
SEP_NMU = 64


def golden_rows():
    rows = np.load(ISO_FIXTURE)["pl_rows"]
    assert len(rows) == 16
    gold = np.loadtxt(GOLD)
    return gold[rows, 0].copy(), gold[rows, 1].copy()


# largest relative distance measured here between the 2-D oracle and the pitch oracle on the same separable content
# (profiles/tabulated_2d_vs_analytic.txt); the bounds are 10 x these
MEASURED_SEP = dict(f=1.5e-14, dfdg=9.2e-14, dfdcx=1.5e-13, norm=1.2e-16, coefficients=6.3e-13)


def test_separable_table_against_the_pitch_oracle():
    """log_n[i][j] = y_i + G_j, y the 2048-node table of gamma^-2.5 exp(-gamma / 1e10) over [1, 1e12] and G = 0.8 mu - 1.5
    mu^2 on 64 nodes, against liboracle_tabpitch with (y, G): the same function in other arithmetic.  calc_f, both
    derivatives, the normalisation, and all eight coefficients on the rows of the golden file's list at which the pitch
    oracle alone is finite in every slot; there the NaN patterns agree, that is, the 2-D oracle is finite too."""
    g = tab_bind.nodes(PL_LO, PL_HI, PL_NODES)
    y, G = tab_bind.log_n_powerlaw(g, PL_P, PL_CUT), tp.log_g_beam(SEP_NMU, 0.8, 1.5)
    s, th = golden_rows()
    assert tp.set_tables(PL_LO, PL_HI, y, G) == 0
    ref_norm = tp.batch_norm([0.0])[0]
    rng = np.random.default_rng(66)
    gam = np.exp(rng.uniform(np.log(1.001), np.log(1e11), 2000))
    mu = rng.uniform(-1, 1, 2000)
    ref_f = tp.dev_calc_f([0.0], ref_norm, gam, mu)
    ref = tp.batch(s, th, np.zeros(len(s)))[0]
    keep = np.isfinite(ref).all(axis=1)
    print("rows kept", keep.sum(), "of 16")
    assert keep.sum() >= 12
    assert t2.set_tables(PL_LO, PL_HI, y[:, None] + G[None, :]) == 0
    norm = t2.batch_norm([0.0])[0]
    got_f = t2.dev_calc_f([0.0], norm, gam, mu)
    got = t2.batch(s[keep], th[keep], np.zeros(keep.sum()))[0]
    assert np.isfinite(got).all()
    check("norm", abs(norm / ref_norm - 1), MEASURED_SEP["norm"], 10)
    # d f / d mu = f G' has a zero at mu0 = 0.8 / 3: relative to f max|G'| there, as the pitch host test does
    check("f", np.abs(got_f[0] / ref_f[0] - 1).max(), MEASURED_SEP["f"], 10)
    check("dfdg", np.abs(got_f[1] / ref_f[1] - 1).max(), MEASURED_SEP["dfdg"], 10)
    check("dfdcx", (np.abs(got_f[2] - ref_f[2]) / (np.abs(ref_f[0]) * 3.8)).max(), MEASURED_SEP["dfdcx"], 10)
    rel = np.abs(got / ref[keep] - 1)
    print("max rel per slot", rel.max(axis=0))
    check("coefficients", rel.max(), MEASURED_SEP["coefficients"], 10)


# ---- 7. the tilted power law against the analytic oracle -------------------------------------------------------------
TILT_NMU = 8
MEASURED_TILT = {(0.3, 0.0): 2.5e-14, (0.3, 0.8): 4.9e-14, (-0.3, 0.0): 2.2e-14, (-0.3, 0.8): 7.5e-13}


def tilt_table(q, a):
    u = np.log(tab_bind.nodes(PL_LO, PL_HI, PL_NODES))[:, None]
    mu = np.linspace(-1.0, 1.0, TILT_NMU)[None, :]
    return -PL_P * u + q * u * mu + a * mu - np.exp(u) / PL_CUT


def tilt_rows(q, a):
    """the golden rows at which the ANALYTIC oracle alone is finite in every slot, and its values there"""
    s, th = golden_rows()
    ref = t2.tilt_batch(s, th, [PL_P, PL_LO, PL_HI, PL_CUT, a, q])
    keep = np.isfinite(ref).all(axis=1)
    return s[keep], th[keep], ref[keep]


def table_rows(s, th, table):
    assert t2.set_tables(PL_LO, PL_HI, table) == 0
    return t2.batch(s, th, np.zeros(len(s)))[0]


@pytest.mark.parametrize("q,a", sorted(MEASURED_TILT))
def test_tilted_power_law_against_the_analytic_oracle(q, a):
    """ln n = -2.5 u + q u mu + a mu - gamma / 1e10 on 2048 x 8 nodes over [1, 1e12] -- bilinear but for the cutoff, so the
    spline reproduces the mu dependence exactly -- against liboracle_tilt, all eight slots; both signs of q, with and without
    the beam."""
    s, th, ref = tilt_rows(q, a)
    print("q", q, "a", a, "rows kept", len(s), "of 16")
    assert len(s) >= 12
    tab = table_rows(s, th, tilt_table(q, a))
    assert np.isfinite(tab).all()
    rel = np.abs(tab / ref - 1.0)
    print("q", q, "a", a, "max rel per slot", rel.max(axis=0))
    check("tilt q = %g a = %g" % (q, a), rel.max(), MEASURED_TILT[(q, a)], 10)


def test_the_cross_term_is_in_the_numbers():
    """q = 0.3 against q = 0 (a = 0): at least one coefficient of every row moves by more than 1 %."""
    s, th, _ = tilt_rows(0.3, 0.0)
    with_q = table_rows(s, th, tilt_table(0.3, 0.0))
    without = table_rows(s, th, tilt_table(0.0, 0.0))
    both = np.isfinite(with_q) & np.isfinite(without)
    moved = np.where(both, np.abs(with_q / without - 1.0), 0.0).max(axis=1)
    print("largest move per row", moved)
    assert (moved > 0.01).all()


# ---- 8. derivatives -----------------------------------------------------------------------------------------------------
FD_MU0, FD_KEEP = 0.8 / 3.0, 0.02


def test_derivatives_of_the_curved_table():
    """The finite-difference check of pitchy_pl.rs:203-238 (norm 1, step 1e-6, gamma = 1.1 + 1e3 u, cos xi = 0.01 + 0.98 u,
    100 draws, relative tolerance 1e-4) on table (2), 64 x 16 nodes, for both derivatives.  d f / d mu = f (0.8 - 3 mu) w has
    a zero at mu0 = 0.8 / 3, where the relative form has a pole (the reference's sin^k factor has none in its range of
    draws): as in test_tabulated_pitch_host.py it is taken over the draws with |mu - mu0| >= 0.02, and the form relative to
    f max|S_mu| covers every draw."""
    EPS, TOL = 1e-6, 1e-4
    rng = np.random.default_rng(6)
    assert t2.set_tables(EDGE_LO, EDGE_HI, t2.table_growing(64, 16), with_norm=False) == 0
    gamma = 1.1 + 1e3 * rng.random(100)
    cx = 0.01 + 0.98 * rng.random(100)
    f0, dfdg, dfdcx = t2.dev_calc_f([0.0], 1.0, gamma, cx)
    f1, _, _ = t2.dev_calc_f([0.0], 1.0, gamma + EPS, cx)
    f2, _, _ = t2.dev_calc_f([0.0], 1.0, gamma, cx + EPS)
    assert (f0 > 1e-250).all() and (dfdcx != 0).all()
    num_g, num_c = (f1 - f0) / EPS, (f2 - f0) / EPS
    away = np.abs(cx - FD_MU0) >= FD_KEEP
    assert away.sum() >= 90
    err_g = np.abs((dfdg - num_g) / num_g).max()
    err_c = np.abs((dfdcx[away] - num_c[away]) / num_c[away]).max()
    err_cs = (np.abs(dfdcx - num_c) / (f0 * 3.8)).max()
    print("dfdg", err_g, "dfdcx", err_c, "dfdcx scaled", err_cs)
    assert err_g < TOL and err_c < TOL and err_cs < TOL


# ---- 9. the curved table converges ---------------------------------------------------------------------------------------
def test_curved_table_converges_to_its_closed_form():
    """Table (2) on 64 x 16 and on 512 x 128 nodes against liboracle_tilt with the table's own formula, all eight slots on the
    first rows of the 2-D fixture's table-2 block at which the analytic oracle is finite: the finer grid is closer by at
    least 10 x.  (What separates them is the natural end condition and the curvature between nodes: an error of the spline
    of the table, not of its evaluation.)"""
    fx = np.load(FIXTURE_2D)
    s, th = fx["s"][16:24], fx["theta"][16:24]
    par, extra = t2.GROW_CLOSED
    ref = t2.tilt_batch(s, th, par, extra)
    keep = np.isfinite(ref).all(axis=1)
    assert keep.sum() >= 4
    s, th, ref = s[keep][:4], th[keep][:4], ref[keep][:4]
    worst = {}
    for shape in ((64, 16), (512, 128)):
        tab = table_rows_edge(s, th, t2.table_growing(*shape))
        assert np.isfinite(tab).all()
        worst[shape] = np.abs(tab / ref - 1.0).max()
        print(shape, "max rel per slot", np.abs(tab / ref - 1.0).max(axis=0))
    print("distances", worst)
    assert worst[(512, 128)] * 10 <= worst[(64, 16)]


def table_rows_edge(s, th, table):
    assert t2.set_tables(EDGE_LO, EDGE_HI, table) == 0
    return t2.batch(s, th, np.zeros(len(s)))[0]
