"""2-D table sets on given gamma nodes (rimphony_ctx_set_tables_2d_grid) without a GPU: the host build of what the kernels
inline (tests/support/liboracle_tab2dgrid.so: rim_tab_check_2d_grid, rim_tab_build_2d_grid, dist_prepare<9>,
tab_bicubic_grid with its interval search, tab_calc_f_both<9>) against

  1. a reference written from the mathematics: the tensor-product natural cubic spline on non-uniform u nodes WITHOUT the
     Hermite form -- splines in u through the columns (second-derivative form, dense mpmath solves at 40 digits), then a
     spline in mu through their values;
  2. the same comparison on a mutated copy of the sources, which must fail on jittered nodes and pass on uniform ones;
  3. numpy.searchsorted, for the interval search;
  4. the analytic tilted power law (liboracle_tilt.so) on a surface bilinear in (u, mu);
  5. the 2-D form on uniform nodes and the given-nodes form on a separable table: the same content through two forms;
  6. the analytic thermal kind on the cold Juettner table the form exists for;
  7. finite differences, for both derivatives;
  8. the refusals of the C ABI; 9. the entry through every layer; 10. the units' kernels and resources.
(11., the group kernel on the wave emulator, is test_wave_emu_tabulated_2d_grid.py.)

Every bound that is not set from outside is a margin (4 in item 1, 10 in items 4 to 6) times a figure measured here on the host
build (the MEASURED* constants; every test prints its own figure, `pytest -s`; profiles/tabulated_2d_grid_vs_analytic.txt)."""
import ctypes
import os
import re
import shutil
import subprocess

import mpmath
import numpy as np
import pytest

import oracle_bind
import tab_bind
import tab2d_bind as t2
import tab_grid_bind as tg
import tab2d_grid_bind as tq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "rimphony_amd", "csrc")
mp = mpmath.mp
U52 = 2.0 ** -52
ENTRY = "rimphony_ctx_set_tables_2d_grid"


def check(name, got, measured, margin):
    print(name, "measured %.3e" % got, "recorded", measured)
    assert got <= margin * measured, (name, got, measured)


# ---- 1. the independent reference ---------------------------------------------------------------------------------------
class RefSpline:
    """The natural cubic spline through (x_j, y_j) on any increasing nodes by its SECOND derivatives M_j (the library solves
    for slopes): M_0 = M_last = 0, h_{j-1} M_{j-1} + 2 (h_{j-1} + h_j) M_j + h_j M_{j+1} = 6 (s_j - s_{j-1}), a dense solve in
    mpmath at 40 digits.  Beyond the ends the end cubic goes on."""

    def __init__(self, x, y):
        self.x, self.y, self.n = list(x), list(y), len(y)
        n, x, y = self.n, self.x, self.y
        self.h = h = [x[j + 1] - x[j] for j in range(n - 1)]
        A, rhs = mp.zeros(n - 2, n - 2), mp.zeros(n - 2, 1)
        for i in range(n - 2):
            j = i + 1
            A[i, i] = 2 * (h[j - 1] + h[j])
            if i > 0:
                A[i, i - 1] = h[j - 1]
            if i < n - 3:
                A[i, i + 1] = h[j]
            rhs[i] = 6 * ((y[j + 1] - y[j]) / h[j] - (y[j] - y[j - 1]) / h[j - 1])
        sol = mp.lu_solve(A, rhs)
        self.M = [mp.mpf(0)] + [sol[i] for i in range(n - 2)] + [mp.mpf(0)]

    def eval(self, x):
        j = 0
        while j < self.n - 2 and self.x[j + 1] <= x:
            j += 1
        h = self.h[j]
        a, b = self.x[j + 1] - x, x - self.x[j]
        Mj, Mk, yj, yk = self.M[j], self.M[j + 1], self.y[j], self.y[j + 1]
        val = (Mj * a ** 3 + Mk * b ** 3) / (6 * h) + (yj / h - Mj * h / 6) * a + (yk / h - Mk * h / 6) * b
        der = (-Mj * a ** 2 + Mk * b ** 2) / (2 * h) - (yj / h - Mj * h / 6) + (yk / h - Mk * h / 6)
        return val, der


class RefSurface:
    """S(u, mu): the natural spline in mu through the values at u of the natural splines in u through the columns; S_u the
    same through their derivatives.  The u nodes are the DOUBLES the library forms, rim_log(gamma_i): the data define the
    spline.  Samples are taken at the exact ln gamma."""

    def __init__(self, u, table):
        mp.dps = 40
        n_nodes, n_mu = table.shape
        un = [mp.mpf(float(v)) for v in u]
        self.mun = [mp.mpf(-1) + 2 * mp.mpf(j) / (n_mu - 1) for j in range(n_mu)]
        self.cols = [RefSpline(un, [mp.mpf(float(v)) for v in table[:, j]]) for j in range(n_mu)]

    def eval(self, u, mu):
        at_u = [c.eval(u) for c in self.cols]
        s, s_mu = RefSpline(self.mun, [v for v, _ in at_u]).eval(mu)
        s_u, _ = RefSpline(self.mun, [d for _, d in at_u]).eval(mu)
        return s, s_u, s_mu


def wavy_at(gamma, n_mu):
    """neither separable nor polynomial (the surface of test_tabulated_2d_host.py at the given nodes)"""
    u = np.log(gamma)[:, None]
    mu = np.linspace(-1.0, 1.0, n_mu)[None, :]
    return -2.2 * u + 0.4 * np.sin(1.3 * u) * np.cos(2.0 * mu) + 0.25 * u * mu - 0.6 * mu * mu + 0.3 * np.sin(3.0 * mu + 0.5 * u)


def ref_nodes(kind, n_nodes):
    """jittered nodes over [1.01, 1e4], or nodes uniform in ln gamma there"""
    return tg.jitter_nodes(n_nodes) if kind == "jitter" else tab_bind.nodes(tg.EDGE_LO, tg.EDGE_HI, n_nodes)


def surface_points(g, n_mu, seed):
    """interior points, nodes and one ulp either side, cell edges, mu = +-1 and a rounding beyond"""
    rng = np.random.default_rng(seed)
    mun = np.linspace(-1.0, 1.0, n_mu)
    lo, hi = np.log(g[0]), np.log(g[-1])
    gam, mus = [], []
    for _ in range(60):
        gam.append(np.exp(rng.uniform(lo, hi))), mus.append(rng.uniform(-1, 1))
    for i in range(len(g)):
        for j in range(0, n_mu, 3):
            for x in (g[i], np.nextafter(g[i], 0.0), np.nextafter(g[i], np.inf)):
                gam.append(x), mus.append(mun[j])
    for k in range(12):
        gam.append(g[k % len(g)]), mus.append(rng.uniform(-1, 1))
        gam.append(np.exp(rng.uniform(lo, hi))), mus.append(mun[k % n_mu])
    for m in (-1.0, 1.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0)):
        for _ in range(4):
            gam.append(np.exp(rng.uniform(lo, hi))), mus.append(m)
    gam, mus = np.array(gam), np.array(mus)
    keep = (gam >= g[0]) & (gam <= g[-1])
    return gam[keep], mus[keep]


_refs = {}


def surface_errors(lib, kind, shape):
    """worst |S - ref| in units of (1 + |S|) 2^-52, and of S_u, S_mu in units of 2^-52 x the steepest chord of the table over
    its spacing along that axis, for tab_bicubic_grid of `lib` on the wavy surface"""
    n_nodes, n_mu = shape
    g = ref_nodes(kind, n_nodes)
    table = wavy_at(g, n_mu)
    assert lib.set_tables(g, table, with_norm=False) == 0
    u = tq.rim_log(g)
    if (kind, shape) not in _refs:
        _refs[kind, shape] = RefSurface(u, table)
    ref = _refs[kind, shape]
    gam, mus = surface_points(g, n_mu, 100 * n_nodes + n_mu)
    s, su, sm = lib.bicubic(0, gam, mus)
    scale_u = float((np.abs(np.diff(table, axis=0)) / np.diff(u)[:, None]).max())
    scale_m = float(np.abs(np.diff(table, axis=1)).max() / (2.0 / (n_mu - 1)))
    worst = dict(S=0.0, S_u=0.0, S_mu=0.0)
    for i in range(len(gam)):
        r, ru, rm = ref.eval(mp.log(mp.mpf(float(gam[i]))), mp.mpf(float(mus[i])))
        worst["S"] = max(worst["S"], float(abs(mp.mpf(float(s[i])) - r)) / ((1 + abs(float(r))) * U52))
        worst["S_u"] = max(worst["S_u"], float(abs(mp.mpf(float(su[i])) - ru)) / scale_u / U52)
        worst["S_mu"] = max(worst["S_mu"], float(abs(mp.mpf(float(sm[i])) - rm)) / scale_m / U52)
    return worst, len(gam)


MARGIN = 4.0
# measured on the host build, in the units of surface_errors; the class the 2-D and the given-nodes forms are held to (a few
# 2^-52 of the steepest chord over the spacing)
MEASURED_SURFACE = {
    ("jitter", (8, 8)): dict(S=1.3, S_u=4.4, S_mu=1.8),
    ("jitter", (9, 12)): dict(S=1.2, S_u=5.3, S_mu=2.6),
    ("uniform", (8, 8)): dict(S=0.9, S_u=5.0, S_mu=3.2),
    ("uniform", (9, 12)): dict(S=1.0, S_u=4.6, S_mu=1.8),
}
SHAPES = [(8, 8), (9, 12)]


def passes_the_comparison(lib, kind, shape):
    worst, count = surface_errors(lib, kind, shape)
    print(kind, shape, "points", count, {k: "%.2f" % v for k, v in worst.items()}, "recorded", MEASURED_SURFACE[kind, shape])
    return all(worst[k] <= MARGIN * MEASURED_SURFACE[kind, shape][k] for k in worst)


@pytest.mark.parametrize("shape", SHAPES)
def test_surface_against_mpmath_on_jittered_nodes(shape):
    assert passes_the_comparison(tq._tab(), "jitter", shape)
    for g, m in ((np.nan, 0.3), (30.0, np.nan)):                    # a NaN gives NaN
        v = tq.bicubic(0, np.array([g]), np.array([m]))
        assert np.isnan(v[0][0]) and np.isnan(v[1][0]) and np.isnan(v[2][0])


# ---- 2. a mutated copy ----------------------------------------------------------------------------------------------------
# rim_tab_build_2d_grid with h_{i-1} and h_i swapped in the right-hand side of the S_umu sweep (the third family only)
SWEEP_CALL = """            for (size_t i = 0; i < n_nodes; i++) y[i] = nodes[(i * n_mu + j) * 4 + 2];
            rim_tab_spline_row_grid(y.data(), n_nodes, h.data(), ih.data(), m.data(), cp.data(), dp.data());
"""
SWEEP_MUTATED = """            for (size_t i = 0; i < n_nodes; i++) y[i] = nodes[(i * n_mu + j) * 4 + 2];
            {
                const size_t last = n_nodes - 1;
                cp[0] = 0.5;
                dp[0] = 3. * ((y[1] - y[0]) / h[0]) / 2.;
                for (size_t i = 1; i < last; i++) {
                    const double sl = (y[i] - y[i - 1]) / h[i - 1], sr = (y[i + 1] - y[i]) / h[i];
                    const double rhs = 3. * (sl * ih[i] + sr * ih[i - 1]);
                    const double den = 2. * (ih[i - 1] + ih[i]) - ih[i - 1] * cp[i - 1];
                    cp[i] = ih[i] / den;
                    dp[i] = (rhs - ih[i - 1] * dp[i - 1]) / den;
                }
                m[last] = (3. * ((y[last] - y[last - 1]) / h[last - 1]) - dp[last - 1]) / (2. - cp[last - 1]);
                for (size_t i = last; i-- > 0;) m[i] = dp[i] - cp[i] * m[i + 1];
            }
"""


@pytest.fixture(scope="module")
def private_build(tmp_path_factory):
    """build(tag, edit) -> Tab2DGridLib of an oracle built from a copy of the sources tab2d_grid_oracle.cpp compiles, with
    `edit` = (file, old, new) applied to the copy (the route of test_tabulated_reference.py)."""
    from rimphony_amd import _build
    base = tmp_path_factory.mktemp("tab2dgrid_private")
    objs = []
    for c in _build.TAB_ORACLE_C:
        o = str(base / (c[:-2] + ".o"))
        subprocess.run(["gcc"] + _build.ORACLE_CFLAGS + ["-std=gnu11", "-c", os.path.join(_build.ORACLE_DIR, c), "-o", o], check=True)
        objs.append(o)

    def build(tag, edit):
        tree = base / tag
        (tree / "tests" / "support").mkdir(parents=True)
        (tree / "oracle").mkdir()
        shutil.copy(os.path.join(ROOT, "tests", "support", "tab2d_grid_oracle.cpp"), tree / "tests" / "support")
        shutil.copy(os.path.join(ROOT, "oracle", "rimo.h"), tree / "oracle")
        shutil.copytree(CSRC, tree / "rimphony_amd" / "csrc", ignore=lambda d, names: [n for n in names if not n.endswith(".h")])
        if edit is not None:
            path, old, new = edit
            src = (tree / path).read_text()
            assert src.count(old) == 1, old
            (tree / path).write_text(src.replace(old, new))
        o, out = str(tree / "tab2d_grid_oracle.o"), str(tree / "liboracle_tab2dgrid.so")
        subprocess.run(["g++"] + _build.ORACLE_CFLAGS + ["-std=c++17", "-c", str(tree / "tests" / "support" / "tab2d_grid_oracle.cpp"),
                        "-o", o], check=True)
        subprocess.run(["g++", "-shared", "-fopenmp", "-Wl,-z,defs"] + objs + [o, "-o", out, "-lm"], check=True)
        return tq.Tab2DGridLib(out)
    return build


def test_mutated_sweep_fails_on_jitter_and_passes_on_uniform(private_build):
    """The S_umu sweep with h_{i-1} and h_i swapped in its right-hand side is another surface on jittered nodes -- the
    comparison of item 1 must tell -- and the library's own where the steps are equal: on nodes uniform in ln gamma it passes
    every comparison the library passes there, with the library's own recorded figures.  The control, a private build with no
    edit, passes on both."""
    same = private_build("unchanged", None)
    bad = private_build("swapped", ("rimphony_amd/csrc/tab_spline.h", SWEEP_CALL, SWEEP_MUTATED))
    for shape in SHAPES:
        assert passes_the_comparison(same, "jitter", shape) and passes_the_comparison(same, "uniform", shape)
        assert passes_the_comparison(tq._tab(), "uniform", shape)
        assert passes_the_comparison(bad, "uniform", shape)
        assert not passes_the_comparison(bad, "jitter", shape)


# ---- 3. the lookup --------------------------------------------------------------------------------------------------------
LOOKUP_GRIDS = {"set A": lambda: tq.fixture_grid(0), "set B": lambda: tq.fixture_grid(1), "log-gm1-2048": lambda: tg.grid("log-gm1-2048")}


@pytest.mark.parametrize("name", list(LOOKUP_GRIDS))
def test_interval_is_searchsorted(name):
    """dist_prepare<9> and tab_2d_grid_interval of the host build equal numpy.searchsorted on the u_i read back from the
    laid-out set (side="right", - 1, clamped to [0, n - 2]) at every node, the doubles either side, both ends and one step
    outside them, 10 000 seeded gamma, and NaN (interval 0, NaN values, every read in bounds).  The guide is what the
    definition says, and the u-node words are (u_i, 1 / (u_{i+1} - u_i))."""
    g = LOOKUP_GRIDS[name]()
    n = len(g)
    assert tq.set_tables(g, np.zeros((1, n, 8)), with_norm=False) == 0
    B = tq.Blob(tq.blob())
    assert B.size == len(tq.blob()) and B.n_nodes == n and B.n_mu == 8
    assert B.cells >= n and B.cells & (B.cells - 1) == 0 and (np.diff(B.u) > 0).all()
    assert (B.u == tq.rim_log(g)).all() and B.u0 == B.u[0]
    assert (B.unodes[:-1, 1] == 1.0 / np.diff(B.u)).all() and B.unodes[-1, 1] == 0
    cell = np.clip(np.floor((B.u - B.u0) * B.inv_cell), 0, B.cells - 1).astype(int)
    want_guide = [min(max(int((cell < c).sum()) - 1, 0), n - 2) for c in range(B.cells + 1)]
    assert (B.guide == want_guide).all()
    rng = np.random.default_rng(77)
    probe = np.concatenate([g, np.nextafter(g, 0.), np.nextafter(g, np.inf),
                            [g[0], g[-1], np.nextafter(g[0], 0.), np.nextafter(g[-1], np.inf), 1.0, 2 * g[-1]],
                            np.exp(np.exp(rng.uniform(np.log(np.log(g[0])), np.log(np.log(g[-1])), 5000))),
                            np.exp(rng.uniform(np.log(g[0]), np.log(g[-1]), 5000))])
    got, reads = tq.intervals(probe)
    want = np.clip(np.searchsorted(B.u, tq.rim_log(probe), side="right") - 1, 0, n - 2)
    bad = np.flatnonzero(got != want)
    print(name, "cells", B.cells, "probes", len(probe), "most node words read by a bisection", reads,
          "most nodes between two guide words", int(np.diff(B.guide.astype(int)).max()))
    assert len(bad) == 0, (probe[bad[:4]], got[bad[:4]], want[bad[:4]])
    assert reads <= int(np.ceil(np.log2(n)))
    assert tq.intervals([np.nan])[0][0] == 0
    v = tq.bicubic(0, np.array([np.nan]), np.array([0.3]))
    assert np.isnan(v[0]).all() and np.isnan(v[1]).all() and np.isnan(v[2]).all()
    f, a, b = tq.dev_calc_f([0.0], 1.0, np.array([np.nan]), np.array([0.3]))
    assert np.isnan(f).all() and np.isnan(a).all() and np.isnan(b).all()


def test_layout_of_the_fixture_sets():
    """word 0 of every node is the table's value, mu fastest (set B has many more mu than gamma nodes: a swapped stride
    cannot pass), the table headers sit where a 2-D set has them, and the normalisations are all that the installation adds"""
    for which in (0, 1):
        g, t = tq.fixture_set(which)
        assert tq.set_tables(g, t, with_norm=False) == 0
        bare = tq.blob()
        B = tq.Blob(bare)
        n_mu = t.shape[2]
        hm = 2.0 / (n_mu - 1)
        assert (B.n_tables, B.n_nodes, B.n_mu) == t.shape and B.gamma_lo == g[0] and B.gamma_hi == g[-1]
        assert (B.nodes[:, :, :, 0] == t).all()
        for k in range(3):
            assert (B.headers[k] == [n_mu - 2, 1.0 / hm, hm, 0, 0, 0, 0, 0]).all()
            assert (t2.table_header(bare, k) == B.headers[k]).all()
        assert (B.nodes[:, :, :, 3] != 0).all()                     # none separable: a cross derivative everywhere
    assert tq.set_tables(*tq.fixture_set(0)) == 0
    full = tq.blob()
    g, t = tq.fixture_set(0)
    assert tq.set_tables(g, t, with_norm=False) == 0
    differs = np.flatnonzero(tq.blob() != full)
    assert differs.tolist() == [8 + 3, 16 + 3, 24 + 3] and (full[differs] > 0).all()


# ---- 4. a bilinear surface against the analytic oracle ------------------------------------------------------------------
PL_P, PL_CUT, PL_LO, PL_HI, PL_NODES, TILT_NMU = 2.5, 1e10, 1.0 + 1e-6, 1e12, 2048, 8
# worst |table / analytic - 1| over the rows kept and 8 slots; the 2-D form's worst figure for the same content is 7.5e-13
MEASURED_TILT = {(0.3, 0.0): 1.7e-14, (0.3, 0.8): 2.1e-14, (-0.3, 0.0): 4.5e-15, (-0.3, 0.8): 1.3e-13}


def pl_nodes():
    g = tg.log_gm1_nodes(PL_LO - 1.0, PL_HI - 1.0, PL_NODES)
    g[0], g[-1] = PL_LO, PL_HI
    return g


def golden_rows():
    rows = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))["pl_rows"]
    gold = np.loadtxt(os.path.join(GOLDEN, "symphony-powerlaw.txt"))
    assert len(rows) == 16
    return gold[rows, 0].copy(), gold[rows, 1].copy()


@pytest.mark.parametrize("q,a", sorted(MEASURED_TILT))
def test_tilted_power_law_against_the_analytic_oracle(q, a):
    """ln n = -2.5 u + q u mu + a mu - gamma / 1e10 on 2048 nodes uniform in ln(gamma - 1) over [1 + 1e-6, 1e12] x 8 mu nodes --
    bilinear in (u, mu) but for the cutoff -- against liboracle_tilt on the 16 pl_rows, all eight slots, over the rows at which
    the ANALYTIC oracle alone is finite in every slot."""
    g = pl_nodes()
    u, mu = np.log(g)[:, None], np.linspace(-1.0, 1.0, TILT_NMU)[None, :]
    s, th = golden_rows()
    ref = t2.tilt_batch(s, th, [PL_P, PL_LO, PL_HI, PL_CUT, a, q])
    keep = np.isfinite(ref).all(axis=1)
    print("q", q, "a", a, "rows kept", keep.sum(), "of 16")
    assert keep.sum() >= 12
    assert tq.set_tables(g, -PL_P * u + q * u * mu + a * mu - g[:, None] / PL_CUT) == 0
    tab = tq.batch(s[keep], th[keep], np.zeros(keep.sum()))[0]
    assert np.isfinite(tab).all()
    rel = np.abs(tab / ref[keep] - 1.0)
    print("max rel per slot", rel.max(axis=0))
    check("tilt q = %g a = %g" % (q, a), rel.max(), MEASURED_TILT[(q, a)], 10)


# ---- 5. the same content through two forms ------------------------------------------------------------------------------
# Worst relative distance between the two forms.  `norm` and the four figures after it are of the quantities as the forms
# return them; the `shape_*` figures are the same with the normalisation divided out (f and its derivatives with norm 1, a
# coefficient over its own form's normalisation).  Against the 2-D form everything agrees to rounding.  Against the
# given-nodes form the normalisations differ by 4.7e-10 and everything else carries that factor: there P = 1/2 int g dmu is
# the given-nodes form's ADAPTIVE quadrature to eps_rel 1e-8 over the kinks of the pitch row's spline (the sin^k family's
# installation), where this form takes the Kronrod rule on every mu cell, as the 2-D and the pitch forms do -- a property of
# the other side's P, within its tolerance.  With it divided out the agreement is rounding-level there too.
MEASURED_TWO_FORMS = {
    "2-D form": dict(norm=3.4e-16, f=5.8e-14, dfdg=1.1e-13, dfdcx=3.9e-14, coefficients=2.3e-15,
                     shape_f=5.8e-14, shape_dfdg=1.1e-13, shape_dfdcx=4.0e-14, shape_coefficients=2.0e-15),
    "given-nodes form": dict(norm=4.8e-10, f=4.8e-10, dfdg=4.8e-10, dfdcx=4.7e-10, coefficients=4.8e-10,
                             shape_f=7.4e-15, shape_dfdg=1.5e-12, shape_dfdcx=1.8e-14, shape_coefficients=1.3e-15),
}


def two_forms_rows():
    from rimphony_amd import workload
    _, _, s, theta, _ = workload.make_batch("cfg2_powerlaw_8", 12, start=7100000)
    return s, theta


def compare_forms(case, got, ref, dfdcx_scale):
    """got, ref: (norm, (f, dfdg, dfdcx) with that norm, coefficients) of the new form and of the other one"""
    M = MEASURED_TWO_FORMS[case]
    check(case + " norm", abs(got[0] / ref[0] - 1), M["norm"], 10)
    live = ref[1][0] > 1e-290
    assert live.sum() >= 0.9 * len(live)
    assert (np.isnan(got[2]) == np.isnan(ref[2])).all()             # the same NaN pattern, hence the same status words
    fin = np.isfinite(ref[2])
    assert fin.sum() >= 0.8 * fin.size
    for prefix, gn, rn in (("", 1.0, 1.0), ("shape_", got[0], ref[0])):
        gf, rf = [v[live] / gn for v in got[1]], [v[live] / rn for v in ref[1]]
        check(case + " " + prefix + "f", np.abs(gf[0] / rf[0] - 1).max(), M[prefix + "f"], 10)
        check(case + " " + prefix + "dfdg", np.abs(gf[1] / rf[1] - 1).max(), M[prefix + "dfdg"], 10)
        # d f / d mu = f S_mu may pass through zero: relative to f max|S_mu|
        check(case + " " + prefix + "dfdcx", (np.abs(gf[2] - rf[2]) / (np.abs(rf[0]) * dfdcx_scale)).max(), M[prefix + "dfdcx"], 10)
        rel = np.abs((got[2][fin] / gn) / (ref[2][fin] / rn) - 1.0)
        check(case + " " + prefix + "coefficients", rel.max(), M[prefix + "coefficients"], 10)


def test_uniform_nodes_against_the_2d_form():
    """table (2) of tab2d_bind -- curved and non-separable -- on 64 x 16 nodes uniform in ln gamma through rim_tab_build_2d and
    through rim_tab_build_2d_grid: the normalisation, f, both derivatives at 2000 seeded points and all eight coefficients on
    12 rows.  What differs is the rounding of t_u and of the sweeps."""
    n_nodes, n_mu = 64, 16
    g = tab_bind.nodes(t2.EDGE_LO, t2.EDGE_HI, n_nodes)
    g[0], g[-1] = t2.EDGE_LO, t2.EDGE_HI
    table = t2.table_growing(n_nodes, n_mu)
    s, th = two_forms_rows()
    rng = np.random.default_rng(55)
    gam, mu = np.exp(rng.uniform(np.log(1.02), np.log(9e3), 2000)), rng.uniform(-1, 1, 2000)
    assert t2.set_tables(t2.EDGE_LO, t2.EDGE_HI, table) == 0
    rn = t2.batch_norm([0.0])[0]
    ref = (rn, t2.dev_calc_f([0.0], rn, gam, mu), t2.batch(s, th, np.zeros(12))[0])
    assert tq.set_tables(g, table) == 0
    gn = tq.batch_norm([0.0])[0]
    got = (gn, tq.dev_calc_f([0.0], gn, gam, mu), tq.batch(s, th, np.zeros(12))[0])
    compare_forms("2-D form", got, ref, abs(t2.GROW_C1) + 2 * abs(t2.GROW_C2))


def test_separable_table_against_the_given_nodes_form():
    """log_n[i][j] = y_i + G_j on the 64 jittered nodes, y the rolled power law of the edge tables and G = 0.8 mu - 1.5 mu^2 on 16
    nodes, through the new entry and through rim_tab_build_grid with (gamma, y, G): the same function in other arithmetic."""
    import tab_pitch_bind as tp
    g = tg.grid("jitter")
    y, G = tg.edge_tables_at(g)[0], tp.log_g_beam(16, 0.8, 1.5)
    s, th = two_forms_rows()
    rng = np.random.default_rng(56)
    gam, mu = np.exp(rng.uniform(np.log(1.02), np.log(9e3), 2000)), rng.uniform(-1, 1, 2000)
    assert tg.set_tables(g, y, G) == 0
    rn = tg.batch_norm([0.0])[0]
    ref = (rn, tg.dev_calc_f([0.0], rn, gam, mu), tg.batch(s, th, np.zeros(12))[0])
    assert tq.set_tables(g, y[:, None] + G[None, :]) == 0
    gn = tq.batch_norm([0.0])[0]
    got = (gn, tq.dev_calc_f([0.0], gn, gam, mu), tq.batch(s, th, np.zeros(12))[0])
    compare_forms("given-nodes form", got, ref, 3.8)


# ---- 6. the case the form exists for ------------------------------------------------------------------------------------
# per slot (j_I a_I j_Q a_Q j_V a_V rho_Q rho_V): worst |table / analytic thermal kind - 1| over the six rows
#   the given-nodes form, 512 nodes uniform in ln(gamma - 1) (test_tabulated_grid_host.py prints it; README table, last row)
GRID_FORM_COLD = (2.6e-8, 7.9e-8, 2.5e-8, 2.8e-8, 2.5e-8, 2.8e-8, 1.6e-7, 1.8e-7)
#   the new form on the same nodes x 8 mu nodes, measured here
MEASURED_COLD = (2.6e-8, 7.9e-8, 2.5e-8, 2.8e-8, 2.5e-8, 2.8e-8, 1.6e-7, 1.8e-7)
#   the non-separable variant, 512 against 4096 nodes of the same family: worst over the coefficients finite on both
MEASURED_COLD_Q = 1.6e-7


def cold_rows(table_of):
    """the six rows through the new form on cold_grid(n): table_of(gamma) -> [n][8]"""
    def run(n):
        g = tg.cold_grid(n)
        assert tq.set_tables(g, table_of(g)) == 0
        return tq.batch(tg.COLD_S, tg.COLD_THETA, np.zeros(6), 0xFF, 8)[0]
    return run


def test_cold_juettner_beats_4096_uniform_nodes(oracle):
    """T = 0.1 Juettner on [1 + 1e-6, 31], constant in mu, rows s = 3, 10, 20, 30, 50, 100, against the analytic thermal kind: in
    every slot the new form on 512 nodes uniform in ln(gamma - 1) x 8 is closer than the 2-D form on 4096 uniform nodes x 8, and
    within 10 x of what the given-nodes form measured on this case; at least 46 of 48 coefficients finite on each table."""
    s, th = tg.COLD_S, tg.COLD_THETA
    ref = oracle_bind.batch(oracle, 1, s, th, [np.full(6, tg.COLD_T)], 0xFF, 8)
    assert np.isfinite(ref).all()
    g4 = tab_bind.nodes(tg.COLD_LO, tg.COLD_HI, 4096)
    assert t2.set_tables(tg.COLD_LO, tg.COLD_HI, tq.cold_table(g4)) == 0
    out = {"2-D 4096": t2.batch(s, th, np.zeros(6), 0xFF, 8)[0], "2-D grid 512": cold_rows(tq.cold_table)(512)}
    fig = {}
    for name, v in out.items():
        fin = np.isfinite(v)
        fig[name] = np.where(fin, np.abs(np.where(fin, v, 1.0) / ref - 1.0), 0.0).max(axis=0)
        print("%-13s finite %2d of 48; j_I a_I j_Q a_Q j_V a_V rho_Q rho_V:" % (name, fin.sum()), " ".join("%.1e" % x for x in fig[name]))
        assert fin.sum() >= 46
    assert (fig["2-D grid 512"] < fig["2-D 4096"]).all()
    assert (fig["2-D grid 512"] <= 10 * np.array(GRID_FORM_COLD)).all()
    assert (fig["2-D grid 512"] <= 10 * np.array(MEASURED_COLD)).all()


def test_cold_core_with_a_tilt_converges():
    """the same core with ln n + 0.3 (gamma - 1) mu, non-separable: 512 nodes against 4096 nodes of the same family, all slots"""
    run = cold_rows(lambda g: tq.cold_table(g, tq.COLD_Q))
    coarse, fine = run(512), run(4096)
    both = np.isfinite(coarse) & np.isfinite(fine)
    assert both.sum() >= 44 and (np.isfinite(coarse) == np.isfinite(fine)).all()
    rel = np.abs(coarse[both] / fine[both] - 1.0).max()
    check("cold core with a tilt, 512 against 4096 nodes", rel, MEASURED_COLD_Q, 10)
    flat = cold_rows(tq.cold_table)(512)
    moved = np.where(both, np.abs(coarse / np.where(both, flat, 1.0) - 1.0), 0.0).max(axis=1)
    assert (moved > 0.01).all()                                     # the tilt is in the numbers of every row


# ---- 7. derivatives -------------------------------------------------------------------------------------------------------
def test_derivatives_by_finite_differences():
    """The finite-difference check of pitchy_pl.rs:203-238 (norm 1, step 1e-6, gamma = 1.1 + 1e3 u, cos xi = 0.01 + 0.98 u, 100
    draws, relative tolerance 1e-4) on the curved surface, table (2), on 64 jittered nodes x 16, for both derivatives.
    d f / d mu = f (0.8 - 3 mu) w has a zero at mu0 = 0.8 / 3: the relative form is taken over the draws at least 0.02 from it,
    and the form relative to f max|S_mu| covers every draw."""
    EPS, TOL, MU0 = 1e-6, 1e-4, 0.8 / 3.0
    rng = np.random.default_rng(6)
    g = tg.grid("jitter")
    assert tq.set_tables(g, tq.surfaces_at(g, 16)[2], with_norm=False) == 0
    gamma = 1.1 + 1e3 * rng.random(100)
    cx = 0.01 + 0.98 * rng.random(100)
    f0, dfdg, dfdcx = tq.dev_calc_f([0.0], 1.0, gamma, cx)
    f1, _, _ = tq.dev_calc_f([0.0], 1.0, gamma + EPS, cx)
    f2, _, _ = tq.dev_calc_f([0.0], 1.0, gamma, cx + EPS)
    assert (f0 > 1e-250).all() and (dfdcx != 0).all()
    num_g, num_c = (f1 - f0) / EPS, (f2 - f0) / EPS
    away = np.abs(cx - MU0) >= 0.02
    assert away.sum() >= 90
    err_g = np.abs((dfdg - num_g) / num_g).max()
    err_c = np.abs((dfdcx[away] - num_c[away]) / num_c[away]).max()
    err_cs = (np.abs(dfdcx - num_c) / (f0 * 3.8)).max()
    print("dfdg", err_g, "dfdcx", err_c, "dfdcx scaled", err_cs)
    assert err_g < TOL and err_c < TOL and err_cs < TOL


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    from rimphony_amd import api
    g = tg.grid("jitter")
    t = tq.surfaces_at(g, 16)
    assert tq.check(g, t) == 0 and tq.check(g[:8], t[:, :8]) == 0 and tq.check(g, t[:, :, :8]) == 0
    assert api.check_tables_2d_grid(g, t)[1].shape == (3, 64, 16) and api.check_tables_2d_grid(g, t[0])[1].shape == (1, 64, 16)
    assert tq.set_tables(g, t, with_norm=False) == 0
    before = tq.blob()

    def refused(gamma, log_n, shape=None, python_too=True):
        assert tq.check(gamma, log_n, shape) == -1
        assert tq.set_tables(gamma, log_n, shape, with_norm=False) == -1
        assert np.array_equal(tq.blob(), before)                    # the previous set is intact
        if python_too:
            with pytest.raises(ValueError):
                api.check_tables_2d_grid(gamma, log_n)

    refused(None, t, python_too=False)                              # null pointers
    refused(g, None, shape=(3, 64, 16), python_too=False)
    for bad in (np.nan, np.inf, -np.inf):                           # a non-finite gamma or value
        gb, tb = g.copy(), t.copy()
        gb[3], tb[1, 5, 3] = bad, bad
        refused(gb, t)
        refused(g, tb)
    low = g.copy()
    low[0] = np.nextafter(1.0, 0.0)
    refused(low, t)                                                 # gamma_0 < 1
    one = g.copy()
    one[0] = 1.0
    assert tq.check(one, t) == 0
    same, swapped = g.copy(), g.copy()
    same[21] = same[20]
    swapped[[20, 21]] = swapped[[21, 20]]
    refused(same, t)                                                # nodes not increasing
    refused(swapped, t)
    close = g.copy()
    close[30] = np.nextafter(close[29], np.inf)
    assert close[29] > 3 and close[29] < close[30] < close[31] and tq.rim_log(close[29:31])[0] == tq.rim_log(close[29:31])[1]
    refused(close, t, python_too=False)                             # equal logarithms: the library alone judges that
    refused(g[:7], t[:, :7])                                        # too few gamma nodes
    many = tab_bind.nodes(1.01, 1e4, 65537)
    refused(many, np.zeros((1, 65537, 8)))                          # too many
    refused(g, t[:, :, :7])                                         # too few mu nodes
    refused(g[:16], np.zeros((1, 16, 1025)))                        # too many
    g1025 = tab_bind.nodes(1.01, 1e4, 1025)
    refused(g1025, np.zeros((1, 1025, 1024)))                       # n_nodes n_mu > 2^20
    assert tq.check(g1025[:1024], np.zeros((1, 1024, 1024))) == 0   # the cap itself is accepted
    assert tq.check(many[:65536], np.zeros((1, 65536, 16))) == 0
    with pytest.raises(ValueError):
        api.check_tables_2d_grid(g, t[:, :32])                      # rows that do not match the nodes
    with pytest.raises(ValueError):
        api.TabulatedDistribution2DGrid(g, t)                       # a set where one table is expected


# ---- 9. the entry through every layer -----------------------------------------------------------------------------------
def test_entry_in_library_header_and_mirrors():
    from rimphony_amd import _build, api, capi
    _build.build_hip()
    lib = ctypes.CDLL(capi.LIB_PATH)
    fn = getattr(lib, ENTRY)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert fn(None, 0, 0, None, 0, None) == -1                      # a null context is refused before anything is touched
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    m = re.search(r"int rimphony_ctx_set_tables_2d_grid\(rimphony_ctx \*ctx, size_t n_tables, size_t n_nodes,\s+const double \*gamma, "
                  r"size_t n_mu,\s+const double \*log_n\);", hdr)
    assert m
    assert ENTRY in capi.SYMBOLS
    rs = open(os.path.join(ROOT, "rimphony-hip-sys", "src", "lib.rs")).read()
    decl = re.search(r"pub fn rimphony_ctx_set_tables_2d_grid\(([^)]*)\)", rs)
    assert decl and len([a for a in decl.group(1).split(",") if a.strip()]) == m.group(0).count(",") + 1 == 6
    hpp = open(os.path.join(ROOT, "rimphony_amd", "cxx", "rimphony.hpp")).read()
    assert ENTRY in hpp and "void set_tables_2d_grid(" in hpp and "class TabulatedDistribution2DGrid" in hpp
    assert hasattr(api.Context, "set_tables_2d_grid") and hasattr(api, "TabulatedDistribution2DGrid")
    g = api.grid_nodes_log_gm1(1.0 + 1e-6, 31.0, 512)
    d = api.TabulatedDistribution2DGrid.from_function(lambda x, mu: x ** (-2.5 + 0.3 * mu), g)
    assert d.log_n.shape == (1, 512, 65) and d.gamma_lo == 1.0 + 1e-6 and d.gamma_hi == 31.0
    assert np.abs(d.log_n[0] - (-2.5 + 0.3 * np.linspace(-1, 1, 65)[None, :]) * np.log(g)[:, None]).max() < 1e-12
    assert api.TabulatedDistribution2DGrid.from_function(lambda x, mu: x ** -2.0 + 0 * mu, g, n_mu=9).log_n.shape == (1, 512, 9)


# ---- 10. the units ----------------------------------------------------------------------------------------------------------
def resource_report(tmp_path, unit):
    from rimphony_amd import _build
    hipcc = _build.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-c", os.path.join(CSRC, unit), "-o", str(tmp_path / (unit + ".o")),
                                           "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for b in re.split(r"remark: Function Name: ", r.stderr)[1:]:
        out[b.split()[0]] = dict(occ=int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1)),
                                 lds=int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)),
                                 vgprs=int(re.search(r"VGPRs: (\d+)", b).group(1)),
                                 scratch=int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)))
    print(unit, out)
    return out


def test_units_are_sources_of_every_build():
    from rimphony_amd import _build
    for unit in ("rimphony_tab_2d_grid.hip", "rimphony_tab_2d_grid_group.hip"):
        assert os.path.join(CSRC, unit) in _build.hip_sources()
        for recipe in ("build_variant.sh", "build_prof.sh"):
            for line in open(os.path.join(ROOT, "tools", recipe)):
                assert ("rimphony_tab.hip" in line) == (unit in line), (recipe, line)


def test_unit_defines_exactly_its_kernels(tmp_path):
    """rimphony_tab_2d_grid.hip, compiled alone for gfx950, defines the installation kernel, the two persistent kernels and the
    two unit seams of kind 9, by mangled name, and the persistent ones keep the family's budgets: 80 / 96 VGPRs at 6 / 5 waves
    per SIMD."""
    rep = resource_report(tmp_path, "rimphony_tab_2d_grid.hip")
    sym, hey = "_Z11coop_kernelI15SymphonyProblemILi9ELi0EEEv7SymArgs", "_Z11coop_kernelI16HeyvaertsProblemILi9EEEv7SymArgs"
    assert sorted(rep) == sorted(["_Z28tab2d_grid_table_norm_kernelPdS_", sym, hey, "_Z18integrand_kernel_nILi9EEv9PointArgsPKdmS2_S2_Pd",
                                  "_Z21gamma_integral_kernelILi9EEv9PointArgsPKdmS2_PdS3_"])
    assert rep[sym]["vgprs"] <= 80 and rep[sym]["occ"] >= 6 and rep[hey]["vgprs"] <= 96 and rep[hey]["occ"] >= 5


def test_group_kernel_resources_leave_room_for_its_grid(tmp_path):
    """The bound of test_grid_group_kernel_resources_leave_room_for_its_grid on the form's group unit: exactly one
    SymGroupProblem kernel, resident RIM_GROUP_WAVES times per SIMD, its LDS block 4 x that many times in a CU's 160 KB with one
    512-byte granule to spare -- and no larger than the family's 7648 bytes."""
    rep = resource_report(tmp_path, "rimphony_tab_2d_grid_group.hip")
    waves = int(re.search(r"#define RIM_GROUP_WAVES (\d+)", open(os.path.join(CSRC, "group_launch.h")).read()).group(1))
    assert list(rep) == ["_Z12group_kernelI15SymGroupProblemILi9EEEv9GroupArgs"]
    k = rep["_Z12group_kernelI15SymGroupProblemILi9EEEv9GroupArgs"]
    assert k["occ"] >= waves and k["vgprs"] <= 96 and k["lds"] <= 7648
    assert 4 * waves * ((k["lds"] + 511) // 512 * 512) <= 160 * 1024 - 512
