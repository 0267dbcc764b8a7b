"""ctypes binding of the table oracle for FAMILIES of 2-D surfaces on given gamma and mu nodes, a real index per row
(tests/support/liboracle_tab2dfamily.so: the CPU oracle's calculators on top of the host build of the family's device functions
and of rim_tab_check_2d_family / rim_tab_build_2d_family), with the sets the tests, the tools and the fixture share.  Test
infrastructure only."""
import ctypes
import os
import re
from ctypes import POINTER, c_double, c_int, c_size_t

import numpy as np

import tab2d_nodes_bind as tn
import tab_bind
import tab_grid_bind as tg

_lib = None
NATURAL, NOT_A_KNOT = 0, 1
HDR, T_HDR, T_NORM = 8, 8, 3            # dev_symphony.h: TAB_HDR_DOUBLES, TAB_2D_HDR, TAB_2D_NORM


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_set_tables_2d_family.restype = c_int
    L.tabo_set_tables_2d_family.argtypes = [c_size_t, c_size_t, dp, c_size_t, dp, dp, dp, c_int, c_int]
    L.tabo_row_line.restype = c_int
    L.tabo_row_line.argtypes = [c_double, dp, dp, dp, dp]
    return L


def call_args(gamma, mu, log_n, sin_k, shape=None):
    """(arrays to keep alive, the first seven arguments of the C entry); shape: what the call states (default: log_n's own)"""
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    gamma, mu, log_n, sin_k = c(gamma), c(mu), c(log_n), c(sin_k)
    if log_n is not None and log_n.ndim == 2:
        log_n = log_n[None]
    nt, nn, nmu = log_n.shape if shape is None else shape
    return (gamma, mu, log_n, sin_k), [int(nt), int(nn), _dp(gamma), int(nmu), _dp(mu), _dp(log_n), _dp(sin_k)]


class Tab2DFamilyLib(tab_bind.TabLib):
    """tab_bind.TabLib on the 2-D family oracle: set_tables(gamma, mu, log_n, sin_k, ends); blob, batch, batch_norm, dev_calc_f
    and mkdist are inherited, `index` being the real index x of a row."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.tabo_set_tables = L.tabo_set_tables_2d_family       # (tab_bind declares the name; _declare declares the entry again)
        self.L = _declare(tab_bind._declare(L))

    def set_tables(self, gamma, mu, log_n, sin_k=None, ends=(0, 0), shape=None):
        """0, or -1 where rimphony_ctx_set_tables_2d_family answers RIMPHONY_EINVAL.  sin_k is passed as it is."""
        keep, a = call_args(gamma, mu, log_n, sin_k, shape)
        return self.L.tabo_set_tables_2d_family(*a, int(ends[0]), int(ends[1]))


def _tab():
    """The tree's oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = Tab2DFamilyLib(_build.build_tab2d_family_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma, mu, log_n, sin_k=None, ends=(0, 0), shape=None):
    return _tab().set_tables(gamma, mu, log_n, sin_k, ends, shape)


def blob():
    return _tab().blob()


def batch(s, theta, x, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the family last given to set_tables(), rows at the real indices x"""
    return _tab().batch(s, theta, x, mask, nthreads)


def batch_norm(x):
    return _tab().batch_norm(x)


def dev_calc_f(x, norm, gamma, cos_xi):
    """(f, dfdg, dfdcx) of the host build of calc_f / calc_f_derivatives of the family's form for the row at x"""
    return _tab().dev_calc_f(4, [x], norm, gamma, cos_xi)


def mkdist(x):
    return _tab().mkdist(x)


def row_line(x):
    """(w, k, the distance to table b in doubles, the three mu geometry words) of the line of a row at x"""
    w, k, d = c_double(), c_double(), c_double()
    geo = np.zeros(3)
    assert load().tabo_row_line(float(x), ctypes.byref(w), ctypes.byref(k), ctypes.byref(d), _dp(geo)) == 0
    return w.value, k.value, d.value, geo


# ---- the sets the tests and the fixture share ------------------------------------------------------------------------
# A: 3 tables (an interior pair and the clamped last table), no prefactor, 16 gamma nodes uniform in ln(gamma - 1) x 8 mu nodes
#    uniform in xi, natural ends.
# B: 2 tables with sin_k = (0.5, 2.5), 16 gamma nodes x 8 jittered mu nodes, not-a-knot ends along mu.
# The surfaces: not separable, curved along both axes, different per table, tapered at both gamma ends as
# tab2d_bind.edge_tables_2d tapers its own (a g1 / gamma and a gamma / g2 term).  No node word is zero.
SET_NODES, SET_NMU = 16, 8
SET_B_K = (0.5, 2.5)
SET_ENDS = ((NATURAL, NATURAL), (NATURAL, NOT_A_KNOT))
SET_GM1 = (1e-2, 1e4)                   # gamma - 1 at the first and the last node
N_TABLES = (3, 2)


def family_surfaces(gamma, mu, n_tables):
    """[n_tables][n_nodes][n_mu]: table t is a rolled power law of index 2.5 + 0.5 t with a tilt that grows with gamma and a
    curvature in mu that changes sign along gamma, both depending on t"""
    gamma = np.asarray(gamma, dtype=np.float64)
    u, g = np.log(gamma)[None, :, None], gamma[None, :, None]
    m = np.asarray(mu, dtype=np.float64)[None, None, :]
    t = np.arange(n_tables, dtype=np.float64)[:, None, None]
    w = (u - u[0, 0, 0]) / (u[0, -1, 0] - u[0, 0, 0])
    return np.ascontiguousarray(-(2.5 + 0.5 * t) * u - (0.3 + 0.2 * t) / (g - 1.0) ** 0.5 - g / (500.0 - 150.0 * t)
                                + (0.3 - 0.25 * t) * u * m + (0.5 + 0.1 * t) * m + (0.4 * t - 0.9 * w + 0.35) * m * m - 0.01)


def fixture_nodes(which):
    if which == 0:
        return tg.log_gm1_nodes(SET_GM1[0], SET_GM1[1], SET_NODES), tn.mu_uniform_in_xi(SET_NMU)
    return tg.log_gm1_nodes(SET_GM1[0], SET_GM1[1], SET_NODES), tn.mu_jitter(SET_NMU)


def fixture_set(which):
    """(gamma, mu, log_n, sin_k, ends) of set A (0) or B (1)"""
    gamma, mu = fixture_nodes(which)
    return gamma, mu, family_surfaces(gamma, mu, N_TABLES[which]), (None if which == 0 else np.array(SET_B_K)), SET_ENDS[which]


BAD_X = 6


def fixture_x(which):
    """the 24 real indices of the fixture rows: every integer, interior fractions in each pair, last - 2^-52, -0.0 and six bad
    values: -1e-300, just above the last table, NaN, +-inf and a large value"""
    last = float(N_TABLES[which] - 1)
    bad = [-1e-300, np.nextafter(last, np.inf), np.nan, np.inf, -np.inf, 1e300]
    if which == 0:
        good = [0.0, 1.0, 2.0, 0.25, 0.5, 0.8125, 1.25, 1.5, 1.9375, last - 2.0 ** -52, -0.0, 0.0625, 1.0625, 0.375, 1.75, 1.0, 0.6875, 2.0]
    else:
        good = [0.0, 1.0, 0.25, 0.5, 0.8125, 0.125, 0.375, 0.9375, last - 2.0 ** -52, -0.0, 0.0625, 0.625, 0.75, 1.0, 0.6875, 0.0, 0.4375,
                0.5625]
    x = np.array(good + bad)
    assert len(x) == 24
    return x


def valid_x(which, x):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= N_TABLES[which] - 1)


# ---- the exactness content: two surfaces bilinear in (ln gamma, mu), a tilted power law each ---------------------------------
# ln n = -p u + q u mu + a mu - gamma / cut: tilt_oracle's closed form with par = {p, gmin, gmax, cut, a, q}
EX_LO, EX_HI, EX_NODES, EX_NMU, EX_CUT = 1.0 + 1e-6, 1e12, 2048, 8, 1e10
# Table 0 is the first content of the plain nodes form's own comparison (p = 2.5, a = 0.8, q = 0.3:
# profiles/tabulated_2d_nodes_accuracy.txt); table 1 differs in index and tilt but keeps the sign of a: where a + q u passes
# through zero the V coefficients of the closed form are differences of nearly equal terms (alpha_V 1e-5 of alpha_I at theta
# near pi / 2), and the PLAIN form on such a surface is itself 3e-12 from the closed form -- a property of that content, which
# says nothing about the blend.
EX_P, EX_A, EX_Q = (2.5, 3.5), (0.8, 0.4), (0.3, 0.1)
EX_K = (0.0, 3.0)
EX_X = (0.1, 0.25, 0.5, 0.75, 0.9)


def exact_family():
    """(gamma, mu, log_n [2][2048][8]): 2048 nodes uniform in ln(gamma - 1) over [1 + 1e-6, 1e12] x 8 jittered mu nodes, the
    nodes of the plain form's own comparison with the closed form"""
    g = tg.log_gm1_nodes(EX_LO - 1.0, EX_HI - 1.0, EX_NODES)
    g[0], g[-1] = EX_LO, EX_HI
    mu = tn.mu_jitter(EX_NMU)
    u = np.log(g)[:, None]
    t = [-p * u + q * u * mu[None, :] + a * mu[None, :] - g[:, None] / EX_CUT for p, a, q in zip(EX_P, EX_A, EX_Q)]
    return g, mu, np.stack(t)


def golden_rows():
    """(s, theta) of the 16 committed power-law rows the analytic comparisons of the plain forms use"""
    golden = os.path.join(tab_bind.ROOT, "tests", "golden")
    rows = np.load(os.path.join(golden, "tabulated_det.npz"))["pl_rows"]
    gold = np.loadtxt(os.path.join(golden, "symphony-powerlaw.txt"))
    assert len(rows) == 16
    return gold[rows, 0].copy(), gold[rows, 1].copy()


def exact_par(x):
    """the closed form's parameters at index x in [0, 1]: every one of them linear in x, as ln n is"""
    lin = lambda v: v[0] + x * (v[1] - v[0])
    return [lin(EX_P), EX_LO, EX_HI, EX_CUT, lin(EX_A), lin(EX_Q)], lin(EX_K)


def read_accuracy(name="tabulated_2d_family_accuracy.txt"):
    """the figures of a profiles/*_accuracy.txt as {name: value}"""
    path = os.path.join(tab_bind.ROOT, "profiles", name)
    out = {}
    for line in open(path):
        m = re.match(r"^  (\w+) = (\S+)$", line.rstrip("\n"))
        if m:
            out[m.group(1)] = float(m.group(2))
    return out


# ---- the measurements the host tests assert and tools/tab_2d_family_accuracy.py records ---------------------------------------
LIN_X = {0: (0.25, 0.8125, 1.5, 1.9375), 1: (0.125, 0.5, 0.9375)}


def _rel(got, ref):
    both = np.isfinite(got) & np.isfinite(ref) & (ref != 0)
    return float(np.abs(got[both] / ref[both] - 1.0).max()), int(both.sum())


def measure_linearity(which, nthreads=16):
    """The family of fixture set `which` at the fractional indices LIN_X against the PLAIN nodes oracle (tab2d_ends_bind)
    installed with ln n -- and k -- blended on the host, t_a + w (t_b - t_a): the worst relative difference of f over 2000
    seeded (gamma, mu) inside the table, of d f / d gamma and d f / d mu relative to |reference| + |f| (d f / d mu passes
    through zero), and of the eight coefficients on the fixture's first 12 (s, theta) over the slots finite in both.
    -> dict(f=, dfdg=, dfdcx=, coefficients=)"""
    import tab2d_ends_bind as te
    gamma_n, mu_n, t, k, ends = fixture_set(which)
    src = np.load(os.path.join(tab_bind.ROOT, "tests", "golden", "tabulated_pitchy_det.npz"))
    s, th = src["s"][:12].copy(), src["theta"][:12].copy()
    rng = np.random.default_rng(2026 + which)
    gamma = np.exp(rng.uniform(np.log(gamma_n[0]), np.log(gamma_n[-1]), 2000))
    mu = rng.uniform(-0.999, 0.999, 2000)
    worst = dict(f=0.0, dfdg=0.0, dfdcx=0.0, coefficients=0.0)
    for x in LIN_X[which]:
        a = int(x)
        w = x - a
        assert set_tables(gamma_n, mu_n, t, k, ends) == 0
        nrm = float(batch_norm(np.array([x]))[0])
        got = dev_calc_f(x, nrm, gamma, mu)
        coeff = batch(s, th, np.full(len(s), x), 0xFF, nthreads)[0]
        blended = t[a] + w * (t[a + 1] - t[a])
        kb = None if k is None else [k[a] + w * (k[a + 1] - k[a])]
        assert te.set_tables(gamma_n, mu_n, blended, kb, ends) == 0
        pn = float(te.batch_norm(np.zeros(1))[0])
        ref = te.dev_calc_f([0.0], pn, gamma, mu)
        ref_coeff = te.batch(s, th, np.zeros(len(s)), 0xFF, nthreads)[0]
        assert (ref[0] > 0).all() and np.isfinite(got[0]).all()
        worst["f"] = max(worst["f"], float(np.abs(got[0] / ref[0] - 1.0).max()))
        for name, i in (("dfdg", 1), ("dfdcx", 2)):
            worst[name] = max(worst[name], float((np.abs(got[i] - ref[i]) / (np.abs(ref[i]) + np.abs(ref[0]))).max()))
        r, n = _rel(coeff, ref_coeff)
        assert n >= 0.8 * coeff.size, n
        worst["coefficients"] = max(worst["coefficients"], r)
    return worst


def measure_exactness(with_k, nthreads=16):
    """Two surfaces bilinear in (ln gamma, mu) with different index and tilt (exact_family) as a family, with_k: sin_k = EX_K,
    at the five interior indices EX_X against the analytic tilted power law at the blended parameters (liboracle_tilt; with_k:
    liboracle_pitchy_tilt at the blended k), on the 16 pl_rows over the rows at which the ANALYTIC oracle alone is finite in
    every slot: the worst |table / analytic - 1| over those rows and the eight coefficients"""
    import tab2d_bind as t2
    import tab2d_pitchy_bind as tp
    g, mu, t = exact_family()
    s, th = golden_rows()
    assert set_tables(g, mu, t, np.array(EX_K) if with_k else None) == 0
    worst = 0.0
    for x in EX_X:
        par, k = exact_par(x)
        ref = tp.ptilt_batch(s, th, par, k, nthreads=nthreads) if with_k else t2.tilt_batch(s, th, par, nthreads=nthreads)
        keep = np.isfinite(ref).all(axis=1)
        assert keep.sum() >= 12, (x, keep.sum())
        tab = batch(s[keep], th[keep], np.full(keep.sum(), x), 0xFF, nthreads)[0]
        assert np.isfinite(tab).all()
        rel = float(np.abs(tab / ref[keep] - 1.0).max())
        print("exactness", "sin_k" if with_k else "plain", "x", x, "rows", int(keep.sum()), "max rel", rel)
        worst = max(worst, rel)
    return worst


# a Juettner shape whose anisotropy depends on T, spaced in 1 / T: ln n is NOT linear in 1 / T, so the blend has an error, which
# falls as the tables get closer
JT_INV = (0.1, 0.2)
JT_LO, JT_HI, JT_NODES, JT_NMU = 1.01, 1e3, 256, 16


def juettner_surface(inv_t, g, mu):
    """ln n of n = gamma^2 beta exp(-(gamma - 1)(1 + a(T) mu^2) / T), a(T) = 0.3 + 0.002 T^2: a(T) / T is not linear in 1 / T"""
    temp = 1.0 / inv_t
    a = 0.3 + 0.002 * temp * temp
    return np.log(g * np.sqrt(g * g - 1.0))[:, None] - (g[:, None] - 1.0) * (1.0 + a * mu[None, :] ** 2) * inv_t


def measure_juettner(n_tables, nthreads=16):
    """n_tables tables equally spaced in 1 / T over JT_INV, evaluated at the middle of every pair against a table built directly
    at that 1 / T (the plain nodes oracle), not-a-knot ends along mu: the worst relative error of the eight coefficients on the
    fixture's first 8 (s, theta), over the slots finite in both"""
    import tab2d_ends_bind as te
    g = tab_bind.nodes(JT_LO, JT_HI, JT_NODES)
    mu = np.linspace(-1.0, 1.0, JT_NMU)
    ends = (NATURAL, NOT_A_KNOT)
    inv = np.linspace(JT_INV[0], JT_INV[1], n_tables)
    src = np.load(os.path.join(tab_bind.ROOT, "tests", "golden", "tabulated_pitchy_det.npz"))
    s, th = src["s"][:8].copy(), src["theta"][:8].copy()
    assert set_tables(g, mu, np.stack([juettner_surface(v, g, mu) for v in inv]), None, ends) == 0
    worst = 0.0
    for a in range(n_tables - 1):
        got = batch(s, th, np.full(len(s), a + 0.5), 0xFF, nthreads)[0]
        assert te.set_tables(g, mu, juettner_surface(0.5 * (inv[a] + inv[a + 1]), g, mu), None, ends) == 0
        ref = te.batch(s, th, np.zeros(len(s)), 0xFF, nthreads)[0]
        r, n = _rel(got, ref)
        assert n >= 0.75 * got.size, n
        worst = max(worst, r)
        # (the family oracle keeps its own set: the plain oracle's install does not touch it)
    return worst
