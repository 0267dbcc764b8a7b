"""The tabulated distribution on given gamma nodes (rimphony_ctx_set_tables_grid) without a GPU: the host build of what the
kernels inline (tests/support/liboracle_tabgrid.so: rim_tab_check_grid, rim_tab_build_grid, dist_prepare<8>,
tab_spline_grid with its interval search, tab_calc_f_both<8>) against

  1. a reference written from the mathematics: the natural cubic spline on non-uniform nodes in its SECOND-derivative form
     (the library solves for the slopes), a dense mpmath solve at 40 digits for 8 and 64 nodes and a numpy.longdouble
     Thomas solve for 2048; f and df/dgamma from it in mpmath;
  2. numpy.searchsorted on the u_j of the laid-out set, for the interval search;
  3. the analytic power law (kind 0) on a straight-line table;
  4. the uniform form with the sin^k entry (rim_tab_build_pitchy) on the same content;
  5. the analytic thermal kind on the cold Juettner table the form exists for, next to what uniform nodes give today;
  6. the refusals of the C ABI.

Every bound that is not set from outside is MARGIN = 4 x a figure measured here (MEASURED; every test prints its own): the
4 covers another libm in the node positions and the samples, as in test_tabulated_reference.py."""
import os

import mpmath
import numpy as np
import pytest

import oracle_bind
import tab_bind
import tab_grid_bind as tg
import tab_pitchy_bind as tpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
mp = mpmath.mp
U52 = 2.0 ** -52
F_FLOOR = 1e-290
MARGIN = 4.0

REF_GRIDS = ("jitter8", "log-gm1", "jitter", "gap", "uniform", "log-gm1-2048")

# Measured on the host build (`pytest -s` prints every figure); the tests bound by MARGIN x these.
#   slope: max over the three tables and the nodes of |m_j - m_ref_j| / max_j |dy_j / h_j|
#   kf:    max over the three tables of |f / f_ref - 1| in units of (1 + |H| + |H' u|) 2^-52 + 2^-52 / (gamma^2 - 1): e^H
#          carries |H| ulps of H and |H' u| of u = rim_log(gamma); beta = sqrt(1 - 1 / gamma^2) is formed in doubles (as in
#          every tabulated form and in the analytic power law), and at gamma - 1 = 1e-6 it keeps 11 digits
#   kd:    max of |dfdg - ref| / (f_ref x the sum of the magnitudes of the three terms of the bracket), in that unit plus
#          2^-52 gamma^2 / (gamma^2 - 1) x the share of the term gamma / (gamma^2 - 1) in that sum: gamma^2 - 1 likewise
MEASURED = {
    "jitter8": dict(slope=2.4e-16, kf=1.0, kd=0.5),
    "log-gm1": dict(slope=5.3e-16, kf=0.4, kd=0.5),
    "jitter": dict(slope=3.3e-16, kf=0.7, kd=1.0),
    "gap": dict(slope=5.0e-16, kf=5.4, kd=4.1),
    "uniform": dict(slope=3.6e-16, kf=0.6, kd=0.5),
    "log-gm1-2048": dict(slope=7.7e-16, kf=0.7, kd=0.4),
}
# item 3: max over the 16 pl_rows and 8 slots of |grid table / analytic kind 0 - 1|
MEASURED_LINE = 4.0e-14
UNIFORM_LINE = 3.5e-13          # the uniform form's figure for the same content (README)
# item 4: max over 12 rows and 8 slots of |grid form / sin^k form - 1| per case
MEASURED_TWO_FORMS = {"no g, k = 0": 4.2e-15, "no g, k = 1.5": 2.9e-15, "8-node rows, k = 0.3": 3.3e-15}


def _mpf(x):
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))


class RefSplineGrid:
    """The natural cubic spline through (u_j, y_j) by its second derivatives M_j.  The u_j are the DOUBLES the library
    forms, rim_log(gamma_j): the data define the spline, and on a grid uniform in ln(gamma - 1) the steps h_j = u_{j+1} - u_j
    near gamma = 1 are differences of rounded logarithms, a hundred times coarser relative to h_j than 2^-52 (at 2048 nodes
    h / u = 0.011), which belongs to the input and not to the solve.  Samples are taken at the exact ln gamma.
    M_0 = M_last = 0,
    h_{j-1} M_{j-1} + 2 (h_{j-1} + h_j) M_j + h_j M_{j+1} = 6 ((y_{j+1} - y_j) / h_j - (y_j - y_{j-1}) / h_{j-1});
    on [u_j, u_{j+1}], with h = h_j, a = u_{j+1} - u, b = u - u_j:
    S = (M_j a^3 + M_{j+1} b^3) / (6 h) + (y_j / h - M_j h / 6) a + (y_{j+1} / h - M_{j+1} h / 6) b."""

    def __init__(self, u, y):
        mp.dps = 40
        self.n = n = len(y)
        self.y = [mp.mpf(float(v)) for v in y]
        self.u = [mp.mpf(float(v)) for v in u]
        self.h = h = [self.u[j + 1] - self.u[j] for j in range(n - 1)]
        self.u_f = np.array([float(v) for v in self.u])
        if n <= 64:
            A = mp.zeros(n - 2, n - 2)
            rhs = mp.zeros(n - 2, 1)
            for i in range(n - 2):
                j = i + 1
                A[i, i] = 2 * (h[j - 1] + h[j])
                if i > 0:
                    A[i, i - 1] = h[j - 1]
                if i < n - 3:
                    A[i, i + 1] = h[j]
                rhs[i] = 6 * ((self.y[j + 1] - self.y[j]) / h[j] - (self.y[j] - self.y[j - 1]) / h[j - 1])
            sol = mp.lu_solve(A, rhs)
            self.M = [mp.mpf(0)] + [sol[i] for i in range(n - 2)] + [mp.mpf(0)]
        else:
            ld = np.longdouble
            assert np.finfo(ld).eps < 1e-18
            ul = np.asarray(u, dtype=ld)
            yl = np.asarray(y, dtype=ld)
            hl = ul[1:] - ul[:-1]
            d = 6 * ((yl[2:] - yl[1:-1]) / hl[1:] - (yl[1:-1] - yl[:-2]) / hl[:-1])
            m = n - 2
            c = np.zeros(m, dtype=ld)
            g = np.zeros(m, dtype=ld)
            b0 = 2 * (hl[0] + hl[1])
            c[0], g[0] = hl[1] / b0, d[0] / b0
            for i in range(1, m):
                den = 2 * (hl[i] + hl[i + 1]) - hl[i] * c[i - 1]
                c[i] = hl[i + 1] / den
                g[i] = (d[i] - hl[i] * g[i - 1]) / den
            x = np.zeros(m, dtype=ld)
            x[-1] = g[-1]
            for i in range(m - 2, -1, -1):
                x[i] = g[i] - c[i] * x[i + 1]
            self.M = [_mpf(v) for v in np.concatenate([[ld(0)], x, [ld(0)]])]

    def slopes(self):
        y, M, h, n = self.y, self.M, self.h, self.n
        m = [(y[j + 1] - y[j]) / h[j] - h[j] * (2 * M[j] + M[j + 1]) / 6 for j in range(n - 1)]
        m.append((y[n - 1] - y[n - 2]) / h[n - 2] + h[n - 2] * (2 * M[n - 1] + M[n - 2]) / 6)
        return m

    def spline(self, u):
        j = min(max(int(np.searchsorted(self.u_f, float(u), side="right")) - 1, 0), self.n - 2)
        while j > 0 and self.u[j] > u:
            j -= 1
        while j < self.n - 2 and self.u[j + 1] <= u:
            j += 1
        h = self.h[j]
        a, b = self.u[j + 1] - u, u - self.u[j]
        Mj, Mk, yj, yk = self.M[j], self.M[j + 1], self.y[j], self.y[j + 1]
        val = (Mj * a ** 3 + Mk * b ** 3) / (6 * h) + (yj / h - Mj * h / 6) * a + (yk / h - Mk * h / 6) * b
        der = (-Mj * a ** 2 + Mk * b ** 2) / (2 * h) - (yj / h - Mj * h / 6) + (yk / h - Mk * h / 6)
        return val, der

    def f(self, gamma, norm):
        g = mp.mpf(float(gamma))
        H, dH = self.spline(mp.log(g))
        beta = mp.sqrt(1 - 1 / (g * g))
        f = mp.mpf(float(norm)) * mp.exp(H) / (g * g * beta)
        dfdg = f * (dH / g - 1 / g - g / (g * g - 1))
        # the last term is formed from gamma^2 - 1 in doubles: the rounding of gamma^2 is gamma^2 / (gamma^2 - 1) ulps of it
        return f, dfdg, abs(H) + abs(dH * mp.log(g)), (abs(dH) + 1) / g + g / (g * g - 1), g * g / (g * g - 1) * g / (g * g - 1)


_refs = {}


def ref_of(name, table):
    if (name, table) not in _refs:
        g = tg.grid(name)
        _refs[name, table] = RefSplineGrid(tg.rim_log(g), tg.edge_tables_at(g)[table])
    return _refs[name, table]


def slope_error(name, slopes_of=None):
    """max over tables and nodes of |slope - reference slope| / max_j |dy_j / h_j|; slopes_of(u, y) replaces the laid-out set's"""
    g = tg.grid(name)
    t = tg.edge_tables_at(g)
    assert tg.set_tables(g, t) == 0
    B = tg.Blob(tg.blob())
    assert B.n_tables == 3 and B.n_nodes == len(g) and (B.nodes[:, :, 1] == t).all()
    worst = 0.
    for k in range(3):
        want = ref_of(name, k).slopes()
        have = B.nodes[k, :, 2] if slopes_of is None else slopes_of(B.u, t[k])
        err = max(abs(mp.mpf(float(have[j])) - want[j]) for j in range(len(g)))
        worst = max(worst, float(err) / float(np.abs(np.diff(t[k]) / np.diff(B.u)).max()))
    return worst


def sample_gammas(name):
    """every node, one ulp either side of every node, 200 seeded gamma (of the 2048-node grid every 16th node)"""
    g = tg.grid(name)
    nodes = g if len(g) <= 64 else g[::16]
    rng = np.random.default_rng(5000 + len(g))
    rand = np.exp(rng.uniform(np.log(np.log(g[0])), np.log(np.log(g[-1])), 200))     # uniform in ln ln gamma: down to gamma - 1 = 1e-6
    gam = np.concatenate([nodes, np.nextafter(nodes, 0.), np.nextafter(nodes, np.inf), np.exp(rand)])
    return gam[(gam >= g[0]) & (gam <= g[-1])]


def f_errors(name):
    g = tg.grid(name)
    t = tg.edge_tables_at(g)
    assert tg.set_tables(g, t) == 0
    norms = tg.batch_norm(np.arange(3, dtype=np.float64))
    gam = sample_gammas(name)
    kf = kd = 0.
    compared = 0
    for k in range(3):
        ref = ref_of(name, k)
        f, dfdg, dfdcx = tg.dev_calc_f([float(k)], norms[k], gam, np.full(len(gam), 0.3))
        for i, x in enumerate(gam):
            rf, rd, H, mag, cond = ref.f(x, norms[k])
            if rf < F_FLOOR:
                continue
            compared += 1
            unit = (1 + float(H)) * U52 + U52 / (float(x) * float(x) - 1.0)
            kf = max(kf, float(abs(mp.mpf(float(f[i])) / rf - 1)) / unit)
            kd = max(kd, float(abs(mp.mpf(float(dfdg[i])) - rd) / (rf * mag)) / (unit + U52 * float(cond / mag)))
    return kf, kd, compared / (3 * len(gam))


# ---- 1. the independent reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", REF_GRIDS)
def test_node_slopes(name):
    err = slope_error(name)
    print(name, "slope error / max|dy/h| = %.3e" % err)
    assert err <= MARGIN * MEASURED[name]["slope"]


@pytest.mark.parametrize("name", REF_GRIDS)
def test_f_and_dfdg(name):
    """calc_f<8> and calc_f_derivatives<8> of the host build (no g, no prefactor: the factor is 1) at every node, one ulp
    either side of every node and 200 seeded gamma per table, against the reference.  Samples whose reference f is below
    1e-290 are left out (the Juettner shape above gamma = 6500; most on the "gap" grid, whose nodes crowd at the top: 11 %)."""
    kf, kd, share = f_errors(name)
    print(name, "kf %.1f kd %.1f compared share %.3f" % (kf, kd, share))
    assert share >= 0.8
    assert kf <= MARGIN * MEASURED[name]["kf"]
    assert kd <= MARGIN * MEASURED[name]["kd"]


def test_mutated_sweep_fails_on_jitter_and_passes_on_uniform():
    """A copy of the library's sweep with h_{j-1} and h_j swapped in the right-hand side (tab_grid_oracle.cpp) is another
    spline on jittered nodes -- the slope test must tell, and does by fourteen orders of magnitude -- and the library's own
    where the steps are equal.  On exactly equal steps (u_j = j / 8) it returns the library's bits.  The steps of the
    "uniform" grid are differences of rounded logarithms and differ among themselves by up to 2 x 2^-52 u_last / h = 2.8e-14
    of h, which the swap moves from one side of a node to the other: there the mutated sweep stays within that figure of
    the reference (measured: 1.7e-15, against the library's 3.6e-16), which is not the 4 x 3.6e-16 of test_node_slopes."""
    good_j = slope_error("jitter", lambda u, y: tg.slopes(u, y, False))
    bad_j = slope_error("jitter", lambda u, y: tg.slopes(u, y, True))
    bad_u = slope_error("uniform", lambda u, y: tg.slopes(u, y, True))
    print("jitter: library %.3e mutated %.3e; uniform: mutated %.3e" % (good_j, bad_j, bad_u))
    assert good_j <= MARGIN * MEASURED["jitter"]["slope"]
    assert bad_j > MARGIN * MEASURED["jitter"]["slope"]
    u = tg.rim_log(tg.grid("uniform"))
    assert bad_u <= 2 * U52 * u[-1] / (u[1] - u[0])
    exact = np.arange(64) / 8.0
    y = tg.edge_tables_at(np.exp(exact) + 0.01)[0]
    assert (tg.slopes(exact, y, True) == tg.slopes(exact, y, False)).all()


# ---- 2. the lookup ------------------------------------------------------------------------------------------------------
# the most node words a bisection may read on each grid: ceil(log2(most nodes between two guide words + 1))
@pytest.mark.parametrize("name", tg.GRIDS + ("log-gm1-2048",))
def test_interval_is_searchsorted(name):
    """tabo_grid_interval -- dist_prepare<8> and tab_grid_interval of the host build -- equals numpy.searchsorted on the u_j
    read back from the laid-out set (side="right", - 1, clamped to [0, n - 2]) at every node, the doubles either side of it,
    both table ends and one step outside them, 10 000 seeded gamma, and NaN (interval 0, NaN values, every read in
    bounds).  The guide words are what the definition says."""
    g = tg.grid(name)
    t = tg.edge_tables_at(g)
    assert tg.set_tables(g, t) == 0
    B = tg.Blob(tg.blob())
    n = len(g)
    assert B.cells >= n and B.cells & (B.cells - 1) == 0 and (np.diff(B.u) > 0).all()
    cell = np.clip(np.floor((B.u - B.u0) * B.inv_cell), 0, B.cells - 1).astype(int)
    want_guide = [min(max(int((cell < c).sum()) - 1, 0), n - 2) for c in range(B.cells + 1)]
    assert (B.guide == want_guide).all()
    rng = np.random.default_rng(77)
    probe = np.concatenate([g, np.nextafter(g, 0.), np.nextafter(g, np.inf),
                            [g[0], g[-1], np.nextafter(g[0], 0.), np.nextafter(g[-1], np.inf), 1.0, 2 * g[-1]],
                            np.exp(np.exp(rng.uniform(np.log(np.log(g[0])), np.log(np.log(g[-1])), 5000))),
                            np.exp(rng.uniform(np.log(g[0]), np.log(g[-1]), 5000))])
    got, reads = tg.intervals(probe)
    want = np.clip(np.searchsorted(B.u, tg.rim_log(probe), side="right") - 1, 0, n - 2)
    bad = np.flatnonzero(got != want)
    print(name, "cells", B.cells, "probes", len(probe), "most node words read by a bisection", reads,
          "most nodes between two guide words", int(np.diff(B.guide.astype(int)).max()))
    assert len(bad) == 0, (probe[bad[:4]], got[bad[:4]], want[bad[:4]])
    assert reads <= int(np.ceil(np.log2(n)))
    j, _ = tg.interval(float("nan"))
    assert j == 0
    h, d = tg.spline(0, np.array([np.nan]))
    assert np.isnan(h).all() and np.isnan(d).all()
    f, a, b = tg.dev_calc_f([0.0], 1.0, np.array([np.nan]), np.array([0.3]))
    assert np.isnan(f).all() and np.isnan(a).all()


# ---- 3. a straight line comes back --------------------------------------------------------------------------------------
def test_straight_line_against_kind_0(oracle):
    """gamma^-2.5 exp(-gamma / 1e10) at the nodes of a 2048-node grid uniform in ln(gamma - 1) over [1 + 1e-6, 1e12] against
    the analytic power law with the same limits, on the 16 pl_rows of tests/golden/tabulated_det.npz, all 8 slots."""
    rows = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))["pl_rows"]
    gold = np.loadtxt(os.path.join(GOLDEN, "symphony-powerlaw.txt"))
    s, th, n = gold[rows, 0].copy(), gold[rows, 1].copy(), len(rows)
    g = tg.log_gm1_nodes(1e-6, 1e12 - 1.0, 2048)
    g[-1] = 1e12
    assert tg.set_tables(g, tab_bind.log_n_powerlaw(g, 2.5, 1e10)) == 0
    tab, _ = tg.batch(s, th, np.zeros(n), 0xFF, 8)
    ref = oracle_bind.batch(oracle, 0, s, th, [np.full(n, 2.5), np.full(n, g[0]), np.full(n, 1e12), np.full(n, 1e10)], 0xFF, 8)
    assert n == 16 and np.isfinite(tab).all() and np.isfinite(ref).all()
    rel = np.abs(tab / ref - 1.0)
    print("max rel per slot", rel.max(axis=0), "worst %.2e" % rel.max(), "the uniform form's", UNIFORM_LINE)
    assert rel.max() <= MARGIN * MEASURED_LINE


# ---- 4. same content, two forms -----------------------------------------------------------------------------------------
TWO_FORMS = {"no g, k = 0": (None, 0.0), "no g, k = 1.5": (None, 1.5), "8-node rows, k = 0.3": (8, 0.3)}


def two_forms_rows():
    from rimphony_amd import workload
    _, _, s, theta, _ = workload.make_batch("cfg2_powerlaw_8", 12, start=7100000)
    return s, theta, np.tile(np.arange(3, dtype=np.float64), 4)


@pytest.mark.parametrize("case", list(TWO_FORMS))
def test_same_content_two_forms(case):
    """The "uniform" grid through rim_tab_build_grid against the same tables through rim_tab_build_pitchy: both take the
    general terms, so what differs is the rounding of t (and of the slopes' sweep).  All 8 slots on 12 rows; NaN patterns
    equal."""
    n_mu, k = TWO_FORMS[case]
    g = tg.grid("uniform")
    t = tg.edge_tables_at(g)
    assert (t == tab_bind.edge_tables(tg.EDGE_LO, tg.EDGE_HI, 64)).all()
    rows = None if n_mu is None else tpy.set_b_rows(n_mu)
    ks = np.full(3, k)
    s, theta, index = two_forms_rows()
    assert tg.set_tables(g, t, rows, ks) == 0
    a, _ = tg.batch(s, theta, index, 0xFF, 8)
    assert tpy.set_tables(tg.EDGE_LO, tg.EDGE_HI, t, rows, ks) == 0
    b, _ = tpy.batch(s, theta, index, 0xFF, 8)
    assert (np.isnan(a) == np.isnan(b)).all()               # the same NaN pattern, hence the same status words
    fin = np.isfinite(a)
    assert fin.sum() >= 0.8 * a.size
    rel = np.abs(a[fin] / b[fin] - 1.0)
    print(case, "worst |grid / sin^k - 1| = %.2e over %d of %d coefficients" % (rel.max(), fin.sum(), a.size))
    assert rel.max() <= MARGIN * MEASURED_TWO_FORMS[case]


# ---- 5. the case this is for --------------------------------------------------------------------------------------------
def cold_figures(oracle):
    """per slot: worst |table / analytic thermal kind - 1| over the six rows for the 512- and 4096-node tables uniform in
    ln gamma and the 512-node table uniform in ln(gamma - 1), with the number of coefficients finite on both sides"""
    s, th = tg.COLD_S, tg.COLD_THETA
    ref = oracle_bind.batch(oracle, 1, s, th, [np.full(6, tg.COLD_T)], 0xFF, 8)
    out = {}
    for nn in (512, 4096):
        g = tab_bind.nodes(tg.COLD_LO, tg.COLD_HI, nn)
        assert tab_bind.set_tables(tg.COLD_LO, tg.COLD_HI, tab_bind.log_n_juettner(g, tg.COLD_T)) == 0
        out["uniform %d" % nn] = tab_bind.batch(s, th, np.zeros(6), 0xFF, 8)[0]
    g = tg.cold_grid(512)
    assert tg.set_tables(g, tab_bind.log_n_juettner(g, tg.COLD_T)) == 0
    out["grid 512"] = tg.batch(s, th, np.zeros(6), 0xFF, 8)[0]
    fig = {}
    for name, v in out.items():
        both = np.isfinite(v) & np.isfinite(ref)
        rel = np.where(both, np.abs(v / np.where(both, ref, 1.0) - 1.0), 0.0)
        fig[name] = (rel.max(axis=0), int(both.sum()))
    return fig


def test_cold_juettner_beats_4096_uniform_nodes(oracle):
    """T = 0.1 Juettner on [1 + 1e-6, 31], rows s = 3, 10, 20, 30, 50, 100: in every slot the 512-node table uniform in
    ln(gamma - 1) is closer to the analytic thermal kind than the 4096-node table uniform in ln gamma, which the test computes
    itself, over the coefficients finite on both sides -- at most 4 of 48 may be missing."""
    fig = cold_figures(oracle)
    for name, (rel, count) in fig.items():
        print("%-13s finite %2d of 48; j_I a_I j_Q a_Q j_V a_V rho_Q rho_V:" % (name, count), " ".join("%.1e" % x for x in rel))
    assert fig["grid 512"][1] >= 44
    assert (fig["grid 512"][0] < fig["uniform 4096"][0]).all()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------
def test_refusals():
    g = tg.grid("jitter")
    t = tg.edge_tables_at(g)
    rows = tpy.set_b_rows(8)
    k = np.array(tg.SET_B_K)
    assert tg.check(g, t, rows, k) == 0 and tg.check(g, t) == 0 and tg.check(g[:8], t[:, :8]) == 0
    assert tg.check(None, t, n_nodes=64) == -1 and tg.check(g, None, n_tables=3) == -1          # a null pointer
    for bad in (np.nan, np.inf, -np.inf):
        for arr in ("gamma", "log_n", "log_g", "sin_k"):
            args = dict(gamma=g.copy(), log_n=t.copy(), log_g=rows.copy(), sin_k=k.copy())
            args[arr].flat[3 if arr != "sin_k" else 1] = bad
            assert tg.check(**args) == -1, (arr, bad)
    low = g.copy()
    low[0] = np.nextafter(1.0, 0.0)
    assert tg.check(low, t) == -1                                                               # gamma[0] < 1
    one = g.copy()
    one[0] = 1.0
    assert tg.check(one, t) == 0
    assert tg.check(g[:7], t[:, :7]) == -1                                                      # too few nodes
    many = tab_bind.nodes(1.01, 1e4, 65537)
    assert tg.check(many, np.zeros((1, 65537))) == -1 and tg.check(many[:65536], np.zeros((1, 65536))) == 0
    same = g.copy()
    same[21] = same[20]
    swapped = g.copy()
    swapped[[20, 21]] = swapped[[21, 20]]
    assert tg.check(same, t) == -1 and tg.check(swapped, t) == -1                               # not strictly increasing
    close = g.copy()
    close[30] = np.nextafter(close[29], np.inf)
    assert close[29] < close[30] < close[31] and tg.rim_log(close[29:31])[0] == tg.rim_log(close[29:31])[1]
    assert tg.check(close, t) == -1                                                             # logarithms coincide
    # what rim_tab_check_pitchy refuses for log_g, n_mu and sin_k
    assert tg.check(g, t, rows, k, n_mu=0) == -1 and tg.check(g, t, None, k, n_mu=8) == -1
    assert tg.check(g, t, rows[:, :7], k) == -1
    for badk in (-0.5, 100.00000000000001):
        assert tg.check(g, t, rows, np.array([0.5, badk, 2.0])) == -1
    # a refusal leaves the previous set in place
    assert tg.set_tables(g, t, rows, k) == 0
    before = tg.blob()
    assert tg.set_tables(close, t, rows, k) == -1 and (tg.blob() == before).all()


# ---- the entry through every layer --------------------------------------------------------------------------------------
def test_entry_in_library_header_and_mirrors():
    import ctypes
    import re
    from rimphony_amd import _build, api, capi
    entry = "rimphony_ctx_set_tables_grid"
    _build.build_hip()
    lib = ctypes.CDLL(capi.LIB_PATH)
    fn = getattr(lib, entry)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                   ctypes.c_void_p]
    assert fn(None, 0, 0, None, None, 0, None, None) == -1          # a null context is refused before anything is touched
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    assert re.search(r"int rimphony_ctx_set_tables_grid\(rimphony_ctx \*ctx, size_t n_tables, size_t n_nodes, const double \*gamma, "
                     r"const double \*log_n,\s+size_t n_mu, const double \*log_g, const double \*sin_k\);", hdr)
    assert entry in capi.SYMBOLS
    assert re.search(r"pub fn rimphony_ctx_set_tables_grid\(", open(os.path.join(ROOT, "rimphony-hip-sys", "src", "lib.rs")).read())
    hpp = open(os.path.join(ROOT, "rimphony_amd", "cxx", "rimphony.hpp")).read()
    assert entry in hpp and "void set_tables_grid(" in hpp and "class TabulatedDistributionGrid" in hpp
    assert hasattr(api.Context, "set_tables_grid")
    g = api.grid_nodes_log_gm1(1.0 + 1e-6, 31.0, 512)
    assert g[0] == 1.0 + 1e-6 and g[-1] == 31.0 and (np.diff(g) > 0).all()
    assert np.allclose(np.diff(np.log(g - 1.0)), np.log(30.0 / 1e-6) / 511, rtol=1e-6)
    d = api.TabulatedDistributionGrid.from_function(lambda x: x ** -2.0, g, pitch_fn=np.exp, n_mu=9, sin_k=0.5)
    assert d.sin_k.tolist() == [0.5] and d.log_g.shape == (1, 9) and d.log_n.shape == (1, 512) and d.gamma_hi == 31.0
    for bad in (g[::-1], np.r_[0.5, g[1:]], g[:7], np.r_[g[:5], np.nan, g[6:]]):
        with pytest.raises(ValueError):
            api.check_grid_tables(bad, np.zeros(len(bad)))
    with pytest.raises(ValueError):
        api.check_grid_tables(g, np.zeros(511))


def test_grid_group_kernel_resources_leave_room_for_its_grid(tmp_path):
    """The budget test_tabulated_group_host.py applies to rimphony_tab_group.hip, applied to the form's own unit,
    rimphony_tab_grid_group.hip: compiled alone for gfx950 it reports exactly one SymGroupProblem kernel, resident
    RIM_GROUP_WAVES times per SIMD and with an LDS block that fits 4 x that many times into a CU's 160 KB with one 512-byte
    granule to spare.  The unit is a source of the library and of the two build recipes."""
    import re
    import subprocess
    from rimphony_amd import _build
    csrc = os.path.join(ROOT, "rimphony_amd", "csrc")
    unit = os.path.join(csrc, "rimphony_tab_grid_group.hip")
    assert unit in _build.hip_sources()
    for recipe in ("build_variant.sh", "build_prof.sh"):
        for line in open(os.path.join(ROOT, "tools", recipe)):
            assert ("rimphony_tab.hip" in line) == ("rimphony_tab_grid_group.hip" in line), (recipe, line)
    hipcc = _build.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-c", unit, "-o", str(tmp_path / "g.o"),
                                           "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    waves = int(re.search(r"#define RIM_GROUP_WAVES (\d+)", open(os.path.join(csrc, "group_launch.h")).read()).group(1))
    names = []
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        name = b.split()[0]
        if "SymGroupProblem" not in name:
            continue
        names.append(name)
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(name, "occupancy", occ, "LDS", lds, "VGPRs", re.search(r"VGPRs: (\d+)", b).group(1),
              "scratch", re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert occ >= waves, (name, occ)
        assert 4 * waves * ((lds + 511) // 512 * 512) <= 160 * 1024 - 512, (name, lds)
    assert names == ["_Z12group_kernelI15SymGroupProblemILi8EEEv9GroupArgs"]
