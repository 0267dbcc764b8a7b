"""The tabulated distribution's host functions against a reference written from the mathematics, not from tab_spline.h or
dev_symphony.h: the natural cubic spline through (u_j, y_j), u = ln gamma, in its SECOND-derivative form (the library
solves for the slopes), as a dense linear solve in mpmath at 40 digits for the small tables and a numpy.longdouble
Thomas solve for 2048 and 65536 nodes; f = norm e^H / (gamma^2 beta) and df/dgamma = f (H'/gamma - 1/gamma -
gamma/(gamma^2 - 1)) of DESIGN.md section 1 evaluated in mpmath from that spline; the normalisation 1 / (4 pi int
e^(H(u) + u) du) by a 20-point Gauss-Legendre rule per node interval.  What is compared is the laid-out table set
(tab_bind.blob), tab_bind.dev_calc_f and tab_bind.batch_norm, i.e. rim_tab_build, dist_prepare<4>, tab_spline,
tab_calc_f_both and the integrand of norm_kernel<4> as the GPU compiles them.  Two mutated copies of those sources, which
every straight-line table passes, must fail the same comparisons.  CPU only.

Every bound below is 4 x a figure measured against this reference (the 4 covers another libm's logarithm in the node
positions and the samples); the figures are in MEASURED, next to the cases."""
import os
import shutil
import subprocess

import mpmath
import numpy as np
import pytest

import tab_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
mp = mpmath.mp
U52 = 2.0 ** -52
F_FLOOR = 1e-290            # below it the host's f is on its way to the subnormals: not compared
MARGIN = 4.0

# name -> (gamma_lo, gamma_hi, n_nodes, tables)
CASES = {
    "edge8": (1.01, 5e3, 8, None), "edge64": (1.01, 1e4, 64, None), "edge2048": (1.01, 1e4, 2048, None),
    "edge65536": (1.01, 1e4, 65536, None),
    "wiggle9": (tab_bind.WIGGLE_LO, tab_bind.WIGGLE_HI, tab_bind.WIGGLE_NODES, "wiggle"),
    "juettner2048": (1.01, 2e3, 2048, "juettner"),
}

# Measured on the host build against the reference (every test prints its figure, `pytest -s`); the tests bound by
# MARGIN x these.
#   slope: max over the case's tables and nodes of |m_j - m_ref_j| / (max|dy| / h)
#   kf:    per table, max of |f / f_ref - 1| / ((1 + |H|) 2^-52)
#   kd:    per table, max of what is left of the df/dgamma error after the slope term, in the same unit (f_errors)
MEASURED = {
    "edge8": dict(slope=5.4e-16, kf=[2.1, 22.6, 2.8], kd=[1.6, 7.8, 2.5]),
    "edge64": dict(slope=2.4e-16, kf=[4.0, 12.6, 4.9], kd=[4.0, 7.1, 4.9]),
    "edge2048": dict(slope=4.0e-16, kf=[4.0, 11.0, 5.7], kd=[3.8, 7.2, 5.6]),
    "edge65536": dict(slope=5.4e-16, kf=[4.0, 15.0, 5.7], kd=[3.8, 6.6, 5.6]),
    "wiggle9": dict(slope=2.3e-16, kf=[11.5], kd=[28.8]),
    "juettner2048": dict(slope=3.2e-16, kf=[14.5], kd=[2.6]),
}
NORM_BOUND = 1e-8           # the epsrel norm_kernel<4> and the table oracle give QAG


def case_tables(name):
    glo, ghi, nn, which = CASES[name]
    if which == "wiggle":
        t = tab_bind.wiggle_table()[None, :]
    elif which == "juettner":
        t = tab_bind.log_n_juettner(tab_bind.nodes(glo, ghi, nn), 10.)[None, :]
    else:
        t = tab_bind.edge_tables(glo, ghi, nn)
    return glo, ghi, np.ascontiguousarray(t)


def _mpf(x):
    """a numpy.longdouble as an mpf, exactly"""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


class RefSpline:
    """The natural cubic spline through (u_j, y_j), u_j = ln gamma_lo + j h, by its second derivatives M_j:
    M_0 = M_last = 0, M_{j-1} + 4 M_j + M_{j+1} = 6 (y_{j+1} - 2 y_j + y_{j-1}) / h^2; on [u_j, u_{j+1}], with a = u_{j+1} - u,
    b = u - u_j: S = (M_j a^3 + M_{j+1} b^3) / (6 h) + (y_j / h - M_j h / 6) a + (y_{j+1} / h - M_{j+1} h / 6) b."""

    def __init__(self, gamma_lo, gamma_hi, y):
        mp.dps = 40
        self.y = [mp.mpf(float(v)) for v in y]
        self.n = n = len(y)
        self.glo, self.ghi = float(gamma_lo), float(gamma_hi)
        self.ulo = mp.log(mp.mpf(self.glo))
        self.h = (mp.log(mp.mpf(self.ghi)) - self.ulo) / (n - 1)
        if n <= 64:
            A = mp.zeros(n - 2, n - 2)
            rhs = mp.zeros(n - 2, 1)
            for i in range(n - 2):
                A[i, i] = 4
                if i > 0:
                    A[i, i - 1] = 1
                if i < n - 3:
                    A[i, i + 1] = 1
                rhs[i] = 6 * (self.y[i + 2] - 2 * self.y[i + 1] + self.y[i]) / self.h ** 2
            sol = mp.lu_solve(A, rhs)
            self.M = [mp.mpf(0)] + [sol[i] for i in range(n - 2)] + [mp.mpf(0)]
        else:
            ld = np.longdouble
            assert np.finfo(ld).eps < 1e-18                 # an extended type: 2000 times finer than the code under test
            yl = np.asarray(y, dtype=ld)
            hl = (np.log(ld(self.ghi)) - np.log(ld(self.glo))) / ld(n - 1)
            d = 6 * (yl[2:] - 2 * yl[1:-1] + yl[:-2]) / (hl * hl)
            m = n - 2
            c = np.zeros(m, dtype=ld)
            g = np.zeros(m, dtype=ld)
            c[0], g[0] = ld(1) / 4, d[0] / 4
            for i in range(1, m):
                den = 4 - c[i - 1]
                c[i] = 1 / den
                g[i] = (d[i] - g[i - 1]) / den
            x = np.zeros(m, dtype=ld)
            x[-1] = g[-1]
            for i in range(m - 2, -1, -1):
                x[i] = g[i] - c[i] * x[i + 1]
            self.M_ld, self.y_ld, self.h_ld = np.concatenate([[ld(0)], x, [ld(0)]]), yl, hl
            self.M = [_mpf(v) for v in self.M_ld]

    def slopes(self):
        y, M, h, n = self.y, self.M, self.h, self.n
        m = [(y[j + 1] - y[j]) / h - h * (2 * M[j] + M[j + 1]) / 6 for j in range(n - 1)]
        m.append((y[n - 1] - y[n - 2]) / h + h * (2 * M[n - 1] + M[n - 2]) / 6)
        return m

    def slopes_ld(self):
        """the same in numpy.longdouble, for the tables solved in it"""
        y, M, h = self.y_ld, self.M_ld, self.h_ld
        m = (y[1:] - y[:-1]) / h - h * (2 * M[:-1] + M[1:]) / 6
        return np.concatenate([m, [(y[-1] - y[-2]) / h + h * (2 * M[-1] + M[-2]) / 6]])

    def spline(self, u):
        """(H, dH/du) at u (an mpf inside the table)"""
        h = self.h
        j = min(max(int(mp.floor((u - self.ulo) / h)), 0), self.n - 2)
        a, b = self.ulo + (j + 1) * h - u, u - (self.ulo + j * h)
        Mj, Mk, yj, yk = self.M[j], self.M[j + 1], self.y[j], self.y[j + 1]
        val = (Mj * a ** 3 + Mk * b ** 3) / (6 * h) + (yj / h - Mj * h / 6) * a + (yk / h - Mk * h / 6) * b
        der = (-Mj * a ** 2 + Mk * b ** 2) / (2 * h) - (yj / h - Mj * h / 6) + (yk / h - Mk * h / 6)
        return val, der

    def f(self, gamma, norm):
        """(f, df/dgamma, H, H', the sum of the magnitudes of the three terms of the derivative's bracket) at the double
        `gamma` inside the table, for the double `norm`: DESIGN.md section 1"""
        g = mp.mpf(float(gamma))
        H, dH = self.spline(mp.log(g))
        beta = mp.sqrt(1 - 1 / (g * g))
        f = mp.mpf(float(norm)) * mp.exp(H) / (g * g * beta)
        dfdg = f * (dH / g - 1 / g - g / (g * g - 1))
        return f, dfdg, H, dH, (abs(dH) + 1) / g + g / (g * g - 1)

    def norm(self):
        """1 / (4 pi int n dgamma), n dgamma = e^(H(u) + u) du: Gauss-Legendre, 20 points per node interval"""
        xs, ws = np.polynomial.legendre.leggauss(20)
        if self.n <= 64:
            total = mp.mpf(0)
            for j in range(self.n - 1):
                for x, w in zip(xs, ws):
                    u = self.ulo + (j + (mp.mpf(float(x)) + 1) / 2) * self.h
                    total += mp.mpf(float(w)) * mp.exp(self.spline(u)[0] + u)
            return 1 / (4 * mp.pi * total * self.h / 2)
        ld = np.longdouble
        M, y, h, ulo = self.M_ld, self.y_ld, self.h_ld, np.log(ld(self.glo))
        b = ((xs.astype(ld) + 1) / 2 * h)[None, :]
        a = h - b
        Mj, Mk, yj, yk = M[:-1, None], M[1:, None], y[:-1, None], y[1:, None]
        val = (Mj * a ** 3 + Mk * b ** 3) / (6 * h) + (yj / h - Mj * h / 6) * a + (yk / h - Mk * h / 6) * b
        u = ulo + np.arange(self.n - 1, dtype=ld)[:, None] * h + b
        total = (np.exp(val + u) * ws.astype(ld)[None, :]).sum()
        return 1 / (4 * mp.pi * _mpf(total) * _mpf(h) / 2)


_refs = {}


def ref_of(name, table):
    """the reference spline of one table of a case, solved once per session"""
    if (name, table) not in _refs:
        glo, ghi, t = case_tables(name)
        _refs[name, table] = RefSpline(glo, ghi, t[table])
    return _refs[name, table]


def _dy_over_h(y, glo, ghi):
    return float(np.abs(np.diff(y)).max() / ((np.log(ghi) - np.log(glo)) / (len(y) - 1)))


def slope_error(lib, name):
    """max over tables and nodes of |blob slope - reference slope| / (max|dy| / h)"""
    glo, ghi, t = case_tables(name)
    assert lib.set_tables(glo, ghi, t) == 0
    b = lib.blob()
    nt, nn = t.shape
    assert len(b) == 8 + 2 * nt * nn and b[0] == nt and b[1] == nn and b[2] == glo and b[3] == ghi
    pairs = b[8:].reshape(nt, nn, 2)
    assert (pairs[:, :, 0] == t).all()
    worst = 0.
    for k in range(nt):
        ref = ref_of(name, k)
        if nn <= 64:
            want = ref.slopes()
            err = max(abs(mp.mpf(float(pairs[k, j, 1])) - want[j]) for j in range(nn))
        else:
            err = np.abs(pairs[k, :, 1].astype(np.longdouble) - ref.slopes_ld()).max()
        worst = max(worst, float(err) / _dy_over_h(t[k], glo, ghi))
    return worst


def sample_gammas(name):
    """4000 log-uniform gammas, every interior node, both ends, and the doubles next to both ends inside the table.
    (Of a table over [1, ...] the end gamma = 1 has beta = 0: test_table_ends.  Of the 65536-node tables every 64th
    interior node is taken here and every one in test_every_interior_node_of_the_largest_tables.)"""
    glo, ghi, t = case_tables(name)
    nn = t.shape[1]
    rng = np.random.default_rng(4000 + nn)
    rand = np.exp(rng.uniform(np.log(glo), np.log(ghi), 4000))
    interior = tab_bind.nodes(glo, ghi, nn)[1:-1]
    if nn > 4096:
        interior = interior[::64]
    ends = [glo, np.nextafter(glo, np.inf), np.nextafter(ghi, 0.), ghi]
    return np.concatenate([rand[(rand > glo) & (rand < ghi)], interior, [g for g in ends if g > 1.]])


def f_errors(lib, name):
    """(kf, kd, share of samples below F_FLOOR), each a list with one entry per table of the case: the host's f and
    df/dgamma at sample_gammas(), with the host's own normalisation of the table (so that f has its physical size), against
    the reference.

    f:    |f / f_ref - 1| in units of (1 + |H|) 2^-52 -- e^H carries |H| ulps of H.
    dfdg: the error is taken relative to |f| times the SUM of the magnitudes of the three terms of the bracket
          H'/gamma - 1/gamma - gamma/(gamma^2 - 1), not to df/dgamma itself, which passes through 0 where f peaks.  The
          part of it that the node slopes' own error explains -- MARGIN x MEASURED slope x max|dy|/h, the bound of
          test_node_slopes, as an error of H' -- is taken off first; what is left is in the same unit as kf."""
    glo, ghi, t = case_tables(name)
    assert lib.set_tables(glo, ghi, t) == 0
    norms = lib.batch_norm(np.arange(len(t), dtype=np.float64))
    gam = sample_gammas(name)
    kfs, kds, lows = [], [], []
    for k in range(len(t)):
        kf = kd = 0.
        low = 0
        ref = ref_of(name, k)
        f, dfdg, dfdcx = lib.dev_calc_f(4, [float(k)], norms[k], gam)
        assert (dfdcx == 0).all()
        slope_abs = MARGIN * MEASURED[name]["slope"] * _dy_over_h(t[k], glo, ghi)
        for i, g in enumerate(gam):
            rf, rd, H, dH, mag = ref.f(g, norms[k])
            if rf < F_FLOOR:
                low += 1
                continue
            unit = (1 + float(abs(H))) * U52
            kf = max(kf, float(abs(mp.mpf(float(f[i])) / rf - 1)) / unit)
            ed = float(abs(mp.mpf(float(dfdg[i])) - rd) / (rf * mag))
            kd = max(kd, max(ed - slope_abs / (float(g) * float(mag)), 0.) / unit)
        kfs.append(kf)
        kds.append(kd)
        lows.append(low / len(gam))
    return kfs, kds, lows


def fails_the_comparison(lib, name):
    """(slopes fail, f or dfdg fails) of `lib` on a case, by the bounds of test_node_slopes and test_f_and_dfdg"""
    kf, kd, _ = f_errors(lib, name)
    return (slope_error(lib, name) > MARGIN * MEASURED[name]["slope"],
            any(a > MARGIN * b for a, b in zip(kf, MEASURED[name]["kf"])) or any(a > MARGIN * b for a, b in zip(kd, MEASURED[name]["kd"])))


@pytest.fixture(scope="module")
def lib():
    tab_bind.load()
    return tab_bind._lib


@pytest.mark.parametrize("name", list(CASES))
def test_node_slopes(lib, name):
    """The slopes rim_tab_build lays out against the reference's, in units of max|dy|/h of the table.  Measured: 2.3e-16 to
    5.4e-16 at every node count from 8 to 65536 (MEASURED).  A double-precision reference shows 6e-12 at 65536 nodes; that
    is the reference's error, not the library's."""
    err = slope_error(lib, name)
    print(name, "slope error / (max|dy|/h) = %.3e" % err)
    assert err <= MARGIN * MEASURED[name]["slope"]


@pytest.mark.parametrize("name", list(CASES))
def test_f_and_dfdg(lib, name):
    """calc_f<4> and calc_f_derivatives<4> of the host build against the reference: f_errors.  Measured K: 2.1 to 5.7 on the
    rolled power laws (largest |H| 82), 11 to 23 on the Juettner shapes (largest |H| 635; the worst samples sit at
    gamma = 90, where H = ln(gamma^2 beta) - gamma/T passes through 0 and carries the ulps of its two terms, not of
    itself), 11.5 (f) and 29 (df/dgamma) on the wiggle table over [1, 1e6] (at gamma = 1.008, from beta = sqrt(1 -
    1/gamma^2)).
    Samples whose reference f is below 1e-290 are left out, at most 5 % of a table's: none on the rolled and the wiggle
    tables, none on the Juettner table over [1.01, 2e3], 4.7 % to 4.8 % on the Juettner table of the three-table sets over
    [1.01, 1e4] (gamma > 6500; |H| up to 635 is still compared).  Over [1.01, 1e4] with 8 nodes the share was 5.7 %, over
    the limit: the 8-node set of this file ends at 5e3 (share 0)."""
    kf, kd, low = f_errors(lib, name)
    print(name, "kf", kf, "kd", kd, "excluded share", low)
    juettner = [CASES[name][3] == "juettner" or (CASES[name][3] is None and k == 1) for k in range(len(kf))]
    for k in range(len(kf)):
        assert low[k] <= (0.05 if juettner[k] else 0.)
        assert kf[k] <= MARGIN * MEASURED[name]["kf"][k]
        assert kd[k] <= MARGIN * MEASURED[name]["kd"][k]


@pytest.mark.parametrize("name", list(CASES))
def test_normalisation(lib, name):
    """batch_norm (QAG with epsrel 1e-8 over the host build's e^H) against the reference's Gauss-Legendre sum: 1e-8.
    Measured: 3.2e-9 worst (64 nodes, Juettner table), 1e-12 at 65536 nodes."""
    glo, ghi, t = case_tables(name)
    assert lib.set_tables(glo, ghi, t) == 0
    got = lib.batch_norm(np.arange(len(t), dtype=np.float64))
    worst = 0.
    for k in range(len(t)):
        want = ref_of(name, k).norm()
        assert np.isfinite(got[k]) and got[k] > 0
        worst = max(worst, float(abs(mp.mpf(float(got[k])) / want - 1)))
    print(name, "norm rel = %.3e" % worst)
    assert worst < NORM_BOUND


def test_every_interior_node_of_the_largest_tables(lib):
    """All 65534 interior nodes of the 65536-node set, each table: at a node H = y_j whatever the slopes are, so f there
    needs no spline -- norm e^(y_j + m_j du) / (gamma^2 beta) in numpy.longdouble, du = ln gamma - u_j the distance of the
    double gamma from its node (1e-16; m_j the reference's slope), and df/dgamma from m_j.  Same units and bounds as
    test_f_and_dfdg.  Whichever of the two intervals next to the node the host picks for such a gamma, it must return
    this."""
    name = "edge65536"
    ld = np.longdouble
    glo, ghi, t = case_tables(name)
    nn = t.shape[1]
    assert lib.set_tables(glo, ghi, t) == 0
    norms = lib.batch_norm(np.arange(len(t), dtype=np.float64))
    gam = tab_bind.nodes(glo, ghi, nn)[1:-1]
    g = gam.astype(ld)
    h = (np.log(ld(ghi)) - np.log(ld(glo))) / ld(nn - 1)
    du = np.log(g) - (np.log(ld(glo)) + np.arange(1, nn - 1, dtype=ld) * h)
    assert np.abs(du).max() < 1e-14
    for k in range(len(t)):
        ref = ref_of(name, k)
        y = t[k].astype(ld)
        m = ref.slopes_ld()[1:-1]
        H = y[1:-1] + m * du
        rf = ld(norms[k]) * np.exp(H) / (g * g * np.sqrt(1 - 1 / (g * g)))
        mag = (np.abs(m) + 1) / g + g / (g * g - 1)
        rd = rf * (m / g - 1 / g - g / (g * g - 1))
        f, dfdg, _ = lib.dev_calc_f(4, [float(k)], norms[k], gam)
        keep = rf >= F_FLOOR
        assert keep.mean() >= 0.95
        unit = (1 + np.abs(H)) * U52
        kf = (np.abs(f.astype(ld) / rf - 1) / unit)[keep].max()
        slope_abs = MARGIN * MEASURED[name]["slope"] * _dy_over_h(t[k], glo, ghi)
        ed = np.abs(dfdg.astype(ld) - rd) / (rf * mag)
        kd = (np.maximum(ed - slope_abs / (g * mag), 0) / unit)[keep].max()
        print("table", k, "kf %.3f kd %.3f kept %.4f" % (kf, kd, keep.mean()))
        assert kf <= MARGIN * MEASURED[name]["kf"][k]
        assert kd <= MARGIN * MEASURED[name]["kd"][k]


@pytest.mark.parametrize("name", list(CASES))
def test_table_ends(lib, name):
    """gamma_lo and gamma_hi belong to the table (compared in test_f_and_dfdg); the doubles next to them outside, and
    anything further out, give exactly 0 in f and both derivatives.  A table that starts at gamma = 1 has beta = 0 there:
    f = +inf and df/dgamma = -inf, the limits of the formulas."""
    glo, ghi, t = case_tables(name)
    assert lib.set_tables(glo, ghi, t) == 0
    out = np.array([np.nextafter(glo, 0.), np.nextafter(ghi, np.inf), 0.5 * glo, 2. * ghi, 0., -3., 1e300, np.inf, -np.inf])
    inside = np.array([glo, np.nextafter(glo, np.inf), np.nextafter(ghi, 0.), ghi])
    for k in range(len(t)):
        for norm in (1.0, 3.5e-5):
            f, a, b = lib.dev_calc_f(4, [float(k)], norm, out)
            for v in (f, a, b):
                assert (v == 0).all() and not np.signbit(v).any()
            f, a, b = lib.dev_calc_f(4, [float(k)], norm, inside)
            assert (b == 0).all()
            if glo == 1.:
                assert f[0] == np.inf and a[0] == -np.inf
                f, a = f[1:], a[1:]
            assert (f >= 0).all() and np.isfinite(f).all() and np.isfinite(a).all()      # (0: e^H underflows at the top)


def test_third_table_is_the_table_alone(lib):
    """Table 2 of a three-table set (row offset 2 n_nodes 2) against the same table as a one-table set: slopes,
    normalisation, f and df/dgamma bit for bit, at 8, 64 and 2048 nodes."""
    for name in ("edge8", "edge64", "edge2048"):
        glo, ghi, t = case_tables(name)
        nn = t.shape[1]
        gam = sample_gammas(name)
        assert lib.set_tables(glo, ghi, t) == 0
        in_set = (lib.blob()[8:].reshape(3, nn, 2)[2].copy(), lib.batch_norm([2.0]), lib.dev_calc_f(4, [2.0], 1.0, gam))
        assert lib.set_tables(glo, ghi, t[2]) == 0
        alone = (lib.blob()[8:].reshape(1, nn, 2)[0].copy(), lib.batch_norm([0.0]), lib.dev_calc_f(4, [0.0], 1.0, gam))
        bits = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
        assert (bits(in_set[0]) == bits(alone[0])).all()
        assert np.isfinite(alone[1]).all() and (bits(in_set[1]) == bits(alone[1])).all()
        for a, b in zip(in_set[2], alone[2]):
            assert (bits(a) == bits(b)).all()
        assert (in_set[2][0] > 0).any()


# ---- the comparisons above on mutated copies of the sources -----------------------------------------------------------
MUTANTS = {
    # the last node's slope is the last chord's: no coupling to its neighbour (a "not-a-natural" end)
    "end_condition": ("rimphony_amd/csrc/tab_spline.h", "row[2 * last + 1] = dp[last];", "row[2 * last + 1] = (y[last] - y[last - 1]) / h;"),
    # the last interval is extrapolated from its neighbour's cubic
    "last_interval": ("rimphony_amd/csrc/dev_symphony.h", "d.par[4] = (double) (nn - 2);", "d.par[4] = (double) (nn - 3);"),
}


@pytest.fixture(scope="module")
def private_build(tmp_path_factory):
    """build(tag, edit) -> TabLib of a table oracle built from a copy of the sources tab_oracle.cpp compiles (its own
    file, rimphony_amd/csrc/*.h, oracle/rimo.h), with `edit` = (file, old, new) applied to the copy.  The oracle's C
    files include neither edited header: their objects are compiled once, from the tree."""
    from rimphony_amd import _build
    base = tmp_path_factory.mktemp("tab_private")
    objs = []
    for c in _build.TAB_ORACLE_C:
        o = str(base / (c[:-2] + ".o"))
        subprocess.run(["gcc"] + _build.ORACLE_CFLAGS + ["-std=gnu11", "-c", os.path.join(_build.ORACLE_DIR, c), "-o", o], check=True)
        objs.append(o)

    def build(tag, edit):
        tree = base / tag
        (tree / "tests" / "support").mkdir(parents=True)
        (tree / "oracle").mkdir()
        shutil.copy(os.path.join(ROOT, "tests", "support", "tab_oracle.cpp"), tree / "tests" / "support")
        shutil.copy(os.path.join(ROOT, "oracle", "rimo.h"), tree / "oracle")
        shutil.copytree(os.path.join(ROOT, "rimphony_amd", "csrc"), tree / "rimphony_amd" / "csrc",
                        ignore=lambda d, names: [n for n in names if not n.endswith(".h")])
        if edit is not None:
            path, old, new = edit
            src = (tree / path).read_text()
            assert src.count(old) == 1, old
            (tree / path).write_text(src.replace(old, new))
        o, out = str(tree / "tab_oracle.o"), str(tree / "liboracle_tab.so")
        subprocess.run(["g++"] + _build.ORACLE_CFLAGS + ["-std=c++17", "-c", str(tree / "tests" / "support" / "tab_oracle.cpp"), "-o", o], check=True)
        subprocess.run(["g++", "-shared", "-fopenmp", "-Wl,-z,defs"] + objs + [o, "-o", out, "-lm"], check=True)
        return tab_bind.TabLib(out)
    return build


def _straight_line_is_exact(lib):
    """the pin of test_tabulated_host.py::test_straight_line_table_is_the_power_law, on one table"""
    glo, ghi, p = 1.0, float(np.exp(60.0 / 2.5)), 2.5
    assert lib.set_tables(glo, ghi, tab_bind.log_n_powerlaw(tab_bind.nodes(glo, ghi, 64), p)) == 0
    gamma = np.exp(np.random.default_rng(1).uniform(np.log(1.0001), np.log(ghi * 0.9999), 2000))
    f4, _, _ = lib.dev_calc_f(4, [0.0], 1.0, gamma)
    f0, _, _ = lib.dev_calc_f(0, [p, glo, ghi, np.inf], 1.0, gamma)
    return np.abs(f4 / f0 - 1.0).max() < 1e-12


def test_private_build_of_the_unchanged_sources_passes(private_build):
    """The control of the two tests below: the same route with no edit passes the comparisons."""
    lib = private_build("unchanged", None)
    for name in ("wiggle9", "edge8"):
        assert fails_the_comparison(lib, name) == (False, False)
    assert _straight_line_is_exact(lib)


def test_mutant_end_condition_is_caught(private_build):
    """rim_tab_build with the last node's slope taken from the last chord alone: a straight-line table cannot tell (it
    passes the power-law pin), the slope comparison does, on every curved table, and so does f in the last intervals."""
    lib = private_build("end_condition", MUTANTS["end_condition"])
    assert _straight_line_is_exact(lib)
    for name in ("wiggle9", "edge8"):
        slopes_fail, f_fails = fails_the_comparison(lib, name)
        assert slopes_fail and f_fails, name


def test_mutant_last_interval_is_caught(private_build):
    """dist_prepare<4> with the last interval's index one short, so that the top interval is evaluated with its
    neighbour's cubic: the table set itself is the unchanged one (slopes pass) and a straight line is still exact; the
    comparison of f fails."""
    lib = private_build("last_interval", MUTANTS["last_interval"])
    assert _straight_line_is_exact(lib)
    for name in ("wiggle9", "edge8"):
        slopes_fail, f_fails = fails_the_comparison(lib, name)
        assert not slopes_fail and f_fails, name
