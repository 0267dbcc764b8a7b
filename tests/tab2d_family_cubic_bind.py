"""ctypes binding of the table oracle for families of 2-D surfaces blended CUBICALLY across their tables
(tests/support/liboracle_tab2dfamilycubic.so: the CPU oracle's calculators on top of the host build of the form's device
functions and of rim_tab_check_2d_family_cubic / rim_tab_build_2d_family_cubic), with the sets the tests, the tools and the
fixture share and the measurements the host tests assert.  Test infrastructure only."""
import ctypes
import os
from ctypes import POINTER, c_double, c_int, c_size_t

import numpy as np

import tab2d_family_bind as tf
import tab2d_nodes_bind as tn
import tab_bind
import tab_grid_bind as tg

_lib = None
NATURAL, NOT_A_KNOT = 0, 1
read_accuracy = tf.read_accuracy
ACCURACY = "tabulated_2d_family_cubic_accuracy.txt"


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_set_tables_2d_family_cubic.restype = c_int
    L.tabo_set_tables_2d_family_cubic.argtypes = [c_size_t, c_size_t, dp, c_size_t, dp, dp, dp, c_int, c_int, dp]
    L.tabo_row_line.restype = c_int
    L.tabo_row_line.argtypes = [c_double, dp, dp, dp, dp, dp]
    return L


class Tab2DFamilyCubicLib(tab_bind.TabLib):
    """tab_bind.TabLib on the oracle of the cubic family: set_tables(gamma, mu, log_n, sin_k, ends, param); blob, batch,
    batch_norm, dev_calc_f and mkdist are inherited, `index` being the real index x of a row."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.tabo_set_tables = L.tabo_set_tables_2d_family_cubic     # (tab_bind declares the name; _declare declares the entry again)
        self.L = _declare(tab_bind._declare(L))

    def set_tables(self, gamma, mu, log_n, sin_k=None, ends=(0, 0), param=None, shape=None):
        """0, or -1 where rimphony_ctx_set_tables_2d_family_cubic answers RIMPHONY_EINVAL.  sin_k and param are passed as
        they are (the caller states the number of tables: a param of another length is the caller's to refuse)."""
        keep, a = tf.call_args(gamma, mu, log_n, sin_k, shape)
        param = None if param is None else np.ascontiguousarray(param, dtype=np.float64)
        return self.L.tabo_set_tables_2d_family_cubic(*a, int(ends[0]), int(ends[1]), _dp(param))


def _tab():
    """The tree's oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = Tab2DFamilyCubicLib(_build.build_tab2d_family_cubic_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma, mu, log_n, sin_k=None, ends=(0, 0), param=None, shape=None):
    return _tab().set_tables(gamma, mu, log_n, sin_k, ends, param, shape)


def blob():
    return _tab().blob()


def batch(s, theta, x, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the family last given to set_tables(), rows at the real indices x"""
    return _tab().batch(s, theta, x, mask, nthreads)


def batch_norm(x):
    return _tab().batch_norm(x)


def dev_calc_f(x, norm, gamma, cos_xi):
    """(f, dfdg, dfdcx) of the host build of calc_f / calc_f_derivatives of the form for the row at x"""
    return _tab().dev_calc_f(4, [x], norm, gamma, cos_xi)


def mkdist(x):
    return _tab().mkdist(x)


def row_line(x):
    """(w, k, the table stride in doubles, the four weights, the stencil's base table, p) of the line of a row at x"""
    w, k, d = c_double(), c_double(), c_double()
    geo, cubic = np.zeros(3), np.zeros(6)
    assert load().tabo_row_line(float(x), ctypes.byref(w), ctypes.byref(k), ctypes.byref(d), _dp(geo), _dp(cubic)) == 0
    return w.value, k.value, d.value, cubic[:4].copy(), int(cubic[4]), float(cubic[5])


# ---- the rule, written again in numpy: what the host tests hold the oracle's weights to -----------------------------------------
def knots(param, n_tables):
    return np.arange(n_tables, dtype=np.float64) if param is None else np.asarray(param, dtype=np.float64)


def numpy_weights(param, n_tables, x):
    """(s, L [4], p) of a valid row at x: the stencil's base table, the Lagrange weights on the knots s .. s + 3 and the row's
    parameter.  Products and quotients in numpy's own order: equal to the oracle's to a few roundings, not bit for bit."""
    c = knots(param, n_tables)
    a = int(x)
    b = min(a + 1, n_tables - 1)
    p = c[a] + (x - a) * (c[b] - c[a])
    s = min(max(a - 1, 0), n_tables - 4)
    k = c[s:s + 4]
    L = np.array([np.prod([(p - k[j]) / (k[i] - k[j]) for j in range(4) if j != i]) for i in range(4)])
    return s, L, p


# ---- the sets the tests and the fixture share ------------------------------------------------------------------------
# Both: 6 tables -- the stencil is clamped at the low end (a = 0), interior (a = 1 .. 3) and clamped at the high end (a = 4) -- on
# 24 gamma nodes uniform in ln(gamma - 1), so not in ln gamma, x 8 mu nodes.
# A: no prefactor, mu nodes uniform in xi, natural ends, knots increasing and unevenly spaced.
# B: sin_k per table, jittered mu nodes, not-a-knot ends along mu, knots decreasing.
# The surfaces are smooth, non-polynomial functions of a variable v of the knot (A: v = c; B: v = 0.6 (9 - c)): not separable,
# curved along both axes, tapered at both gamma ends as tab2d_family_bind.family_surfaces tapers its own.  No node word is zero.
SET_NODES, SET_NMU, N_TABLES = 24, 8, 6
SET_PARAM = ((0.0, 0.7, 1.1, 2.0, 2.6, 4.0), (9.0, 7.5, 6.8, 5.0, 4.1, 3.0))
SET_B_K = (0.5, 1.0, 1.4, 2.0, 2.3, 2.5)
SET_ENDS = ((NATURAL, NATURAL), (NATURAL, NOT_A_KNOT))
SET_GM1 = (1e-2, 1e4)


def surfaces(gamma, mu, v):
    """[len(v)][n_nodes][n_mu]: a rolled power law whose index, low-energy taper, cutoff, tilt and curvature in mu all depend
    on v, none of them polynomially in all terms (1 / (500 + 80 v), exp(-0.3 v))"""
    gamma = np.asarray(gamma, dtype=np.float64)
    u, g = np.log(gamma)[None, :, None], gamma[None, :, None]
    m = np.asarray(mu, dtype=np.float64)[None, None, :]
    v = np.asarray(v, dtype=np.float64)[:, None, None]
    w = (u - u[0, 0, 0]) / (u[0, -1, 0] - u[0, 0, 0])
    return np.ascontiguousarray(-(2.5 + 0.3 * v + 0.04 * v * v) * u - (0.3 + 0.1 * v) / (g - 1.0) ** 0.5 - g / (500.0 + 80.0 * v)
                                + (0.3 - 0.12 * v) * u * m + (0.5 + 0.4 * np.exp(-0.3 * v)) * m + (0.2 * v - 0.9 * w + 0.35) * m * m - 0.01)


def fixture_nodes(which):
    gamma = tg.log_gm1_nodes(SET_GM1[0], SET_GM1[1], SET_NODES)
    return gamma, (tn.mu_uniform_in_xi(SET_NMU) if which == 0 else tn.mu_jitter(SET_NMU))


def fixture_v(which):
    c = np.array(SET_PARAM[which])
    return c if which == 0 else 0.6 * (9.0 - c)


def fixture_set(which):
    """(gamma, mu, log_n, sin_k, ends, param) of set A (0) or B (1)"""
    gamma, mu = fixture_nodes(which)
    return (gamma, mu, surfaces(gamma, mu, fixture_v(which)), (None if which == 0 else np.array(SET_B_K)), SET_ENDS[which],
            np.array(SET_PARAM[which]))


INT_X = (0.0, -0.0, 1.0, 5.0)
FRAC_X = (0.37, 1.5, 2.25, 3.5, 4.75)           # one per table interval
BAD_X_VALUES = (-1e-3, 5.0000001, np.nan, np.inf)
BAD_X = len(BAD_X_VALUES)


def fixture_x():
    """the 24 real indices of the fixture rows, the same for both sets: the integers, one fraction per table interval, the four
    invalid values, then the fractions and the remaining integers again on other (s, theta)"""
    x = np.array(INT_X + FRAC_X + BAD_X_VALUES + FRAC_X + (2.0, 3.0, 4.0, 1.0, 5.0, 0.37))
    assert len(x) == 24
    return x


def valid_x(x):
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= N_TABLES - 1)


# the k overshoot: sin_k = (0, 0, 3, 0, 0, 0) on the knots 0 .. 5; at x = 0.5 the weights are (0.3125, 0.9375, -0.3125, 0.0625)
# and the blended k is -0.9375
OVERSHOOT_K, OVERSHOOT_X = (0.0, 0.0, 3.0, 0.0, 0.0, 0.0), 0.5


def overshoot_set():
    gamma, mu, t, k, ends, param = fixture_set(1)
    return gamma, mu, t, np.array(OVERSHOOT_K), ends, None


def fixture_rows():
    """(s, theta) of the 24 fixture rows: those of tests/golden/tabulated_pitchy_det.npz"""
    src = np.load(os.path.join(tab_bind.ROOT, "tests", "golden", "tabulated_pitchy_det.npz"))
    return src["s"].copy(), src["theta"].copy()


def _rel(got, ref):
    both = np.isfinite(got) & np.isfinite(ref) & (ref != 0)
    return float(np.abs(got[both] / ref[both] - 1.0).max()), int(both.sum())


# ---- the measurements the host tests assert and tools/tab_2d_family_cubic_accuracy.py records ---------------------------------
def measure_independence(which, nthreads=16):
    """The cubic family of fixture set `which` at the fractional rows FRAC_X against the PLAIN nodes oracle (tab2d_ends_bind)
    installed with ln n -- and k -- blended on the host with numpy_weights, which shares no text with the oracle: the worst
    relative difference of f over 2000 seeded (gamma, mu) inside the table, of d f / d gamma and d f / d mu relative to
    |reference| + |f|, and of the eight coefficients on the fixture's first 12 (s, theta) over the slots finite in both.
    -> dict(f=, dfdg=, dfdcx=, coefficients=)"""
    import tab2d_ends_bind as te
    gamma_n, mu_n, t, k, ends, param = fixture_set(which)
    s, th = (v[:12].copy() for v in fixture_rows())
    rng = np.random.default_rng(2027 + which)
    gamma = np.exp(rng.uniform(np.log(gamma_n[0]), np.log(gamma_n[-1]), 2000))
    mu = rng.uniform(-0.999, 0.999, 2000)
    worst = dict(f=0.0, dfdg=0.0, dfdcx=0.0, coefficients=0.0)
    assert set_tables(gamma_n, mu_n, t, k, ends, param) == 0
    for x in FRAC_X:
        nrm = float(batch_norm(np.array([x]))[0])
        got = dev_calc_f(x, nrm, gamma, mu)
        coeff = batch(s, th, np.full(len(s), x), 0xFF, nthreads)[0]
        base, L, p = numpy_weights(param, len(t), x)
        blended = np.tensordot(L, t[base:base + 4], axes=1)
        kb = None if k is None else [float(np.dot(L, k[base:base + 4]))]
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


# the exactness content: five surfaces ln n = -p u + q u mu + a mu - gamma / cut with p, a, q (and k) CUBIC polynomials in unevenly
# spaced knots: a 4-point Lagrange cubic reproduces them, so the row at x is the closed form at the polynomials' values.  a and q
# keep their sign (tab2d_family_bind: where a + q u passes through zero the V coefficients of the closed form cancel).
EX_PARAM = (0.0, 0.6, 1.0, 1.9, 2.5)
EX_POLY = dict(p=(2.5, 0.3, 0.1, -0.02), a=(0.8, -0.2, 0.05, -0.01), q=(0.3, -0.1, 0.02, 0.002), k=(0.5, 0.8, -0.1, 0.02))
EX_X = (0.4, 1.5, 2.3, 3.6)             # the stencil clamped low, interior (twice), clamped high


def _poly(name, c):
    c0, c1, c2, c3 = EX_POLY[name]
    return c0 + c * (c1 + c * (c2 + c * c3))


def exact_family():
    """(gamma, mu, log_n [5][2048][8], sin_k [5]) on the nodes of tab2d_family_bind.exact_family"""
    g, mu, unused = tf.exact_family()
    u = np.log(g)[:, None]
    c = np.array(EX_PARAM)
    t = [-_poly("p", v) * u + _poly("q", v) * u * mu[None, :] + _poly("a", v) * mu[None, :] - g[:, None] / tf.EX_CUT for v in c]
    return g, mu, np.stack(t), _poly("k", c)


def exact_par(x):
    """the closed form's parameters {p, gmin, gmax, cut, a, q} and k of the row at index x"""
    c = np.array(EX_PARAM)
    a = int(x)
    v = c[a] + (x - a) * (c[a + 1] - c[a])
    return [_poly("p", v), tf.EX_LO, tf.EX_HI, tf.EX_CUT, _poly("a", v), _poly("q", v)], _poly("k", v)


def measure_exactness(with_k, nthreads=16):
    """exact_family as a cubic family, with_k: with its sin_k, at the off-knot indices EX_X against the analytic tilted power
    law at the polynomials' values (liboracle_tilt; with_k: liboracle_pitchy_tilt), on the 16 pl_rows over the rows at which
    the ANALYTIC oracle alone is finite in every slot: the worst |table / analytic - 1| over those rows and the eight
    coefficients"""
    import tab2d_bind as t2
    import tab2d_pitchy_bind as tp
    g, mu, t, k = exact_family()
    s, th = tf.golden_rows()
    assert set_tables(g, mu, t, k if with_k else None, (0, 0), np.array(EX_PARAM)) == 0
    worst = 0.0
    for x in EX_X:
        par, kx = exact_par(x)
        ref = tp.ptilt_batch(s, th, par, kx, nthreads=nthreads) if with_k else t2.tilt_batch(s, th, par, nthreads=nthreads)
        keep = np.isfinite(ref).all(axis=1)
        assert keep.sum() >= 12, (x, keep.sum())
        tab = batch(s[keep], th[keep], np.full(keep.sum(), x), 0xFF, nthreads)[0]
        assert np.isfinite(tab).all()
        rel = float(np.abs(tab / ref[keep] - 1.0).max())
        print("exactness", "sin_k" if with_k else "plain", "x", x, "rows", int(keep.sum()), "max rel", rel)
        worst = max(worst, rel)
    return worst


def measure_juettner(n_tables, nthreads=16):
    """tab2d_family_bind.measure_juettner with the cubic blend: the same surface, nodes, ends and rows, n_tables tables equally
    spaced in 1 / T with 1 / T as the knots, the row in the middle of every pair against a table built directly at that 1 / T"""
    import tab2d_ends_bind as te
    g = tab_bind.nodes(tf.JT_LO, tf.JT_HI, tf.JT_NODES)
    mu = np.linspace(-1.0, 1.0, tf.JT_NMU)
    ends = (NATURAL, NOT_A_KNOT)
    inv = np.linspace(tf.JT_INV[0], tf.JT_INV[1], n_tables)
    src = np.load(os.path.join(tab_bind.ROOT, "tests", "golden", "tabulated_pitchy_det.npz"))
    s, th = src["s"][:8].copy(), src["theta"][:8].copy()
    assert set_tables(g, mu, np.stack([tf.juettner_surface(v, g, mu) for v in inv]), None, ends, inv) == 0
    worst = 0.0
    for a in range(n_tables - 1):
        got = batch(s, th, np.full(len(s), a + 0.5), 0xFF, nthreads)[0]
        assert te.set_tables(g, mu, tf.juettner_surface(0.5 * (inv[a] + inv[a + 1]), g, mu), None, ends) == 0
        ref = te.batch(s, th, np.zeros(len(s)), 0xFF, nthreads)[0]
        r, n = _rel(got, ref)
        assert n >= 0.75 * got.size, n
        worst = max(worst, r)
    return worst
