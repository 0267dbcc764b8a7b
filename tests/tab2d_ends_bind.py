"""ctypes binding of the table oracle for 2-D sets of any of the six forms with a choice of the spline's ends per axis
(tests/support/liboracle_tab2dends.so: the CPU oracle's calculators on top of the host build of the tabulated
distribution's device functions, of rim_tab_check_ends / rim_tab_build_2d* with their trailing arguments and of
tab_install.h), and the node sets and surfaces the tests, the tools and the fixture share.  Test infrastructure only.

A call names its form as the C entries do: gamma None -> nodes uniform in ln gamma from gamma_lo to gamma_hi, mu None -> nodes
uniform in mu, sin_k None -> no prefactor.  ends: a pair (ends_gamma, ends_mu) of 0 (natural) or 1 (not-a-knot)."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_longlong, c_size_t

import numpy as np

import tab_bind

_lib = None
NATURAL, NOT_A_KNOT = 0, 1
GLO, GHI = 1.01, 1e4                    # the range of the sets on nodes uniform in ln gamma
HDR, T_HDR, T_NORM, T_ENDS = 8, 8, 3, 7     # dev_symphony.h: TAB_HDR_DOUBLES, TAB_2D_HDR, TAB_2D_NORM, TAB_2D_ENDS
FORMS = ("uniform", "grid", "nodes")
SHAPES = [(1, 8, 8), (3, 9, 11), (5, 70, 13), (1, 300, 8), (1, 8, 1024)]


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    head = [c_size_t, c_size_t, dp, c_double, c_double, c_size_t, dp, dp, dp]
    L.tabo_check_2d_ends.restype = c_int
    L.tabo_check_2d_ends.argtypes = head + [c_int, c_int]
    L.tabo_set_tables_2d_ends.restype = c_int
    L.tabo_set_tables_2d_ends.argtypes = head + [c_int, c_int, c_int]
    L.tabo_build_2d_without_ends.restype = c_longlong
    L.tabo_build_2d_without_ends.argtypes = head + [dp, c_size_t]
    L.tabo_lines_2d_ends.restype = c_longlong
    L.tabo_lines_2d_ends.argtypes = head + [c_int, c_int, dp, c_size_t]
    L.tabo_put_norms.restype = c_int
    L.tabo_put_norms.argtypes = [c_size_t, dp]
    L.tabo_form.restype = c_int
    L.tabo_form.argtypes = []
    L.tabo_bicubic.restype = c_int
    L.tabo_bicubic.argtypes = [c_double, c_size_t, dp, dp, dp, dp, dp]
    return L


def _args(gamma, mu, log_n, sin_k, shape, gamma_lo, gamma_hi):
    """the first nine arguments of every entry; shape: what the call states (default: log_n's own)"""
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    gamma, mu, log_n = c(gamma), c(mu), c(log_n)
    if log_n is not None and log_n.ndim == 2:
        log_n = log_n[None]
    nt, nn, nmu = log_n.shape if shape is None else shape
    if sin_k is not None:
        sin_k = c(np.broadcast_to(np.asarray(sin_k, dtype=np.float64), (int(nt),)))
    keep = (gamma, mu, log_n, sin_k)
    return keep, [int(nt), int(nn), _dp(gamma), float(gamma_lo), float(gamma_hi), int(nmu), _dp(mu), _dp(log_n), _dp(sin_k)]


class Tab2DEndsLib(tab_bind.TabLib):
    """tab_bind.TabLib on this oracle; blob, batch, batch_norm, dev_calc_f and mkdist are inherited."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.tabo_set_tables = L.tabo_set_tables_2d_ends       # (tab_bind declares the name; _declare declares the entry again)
        self.L = _declare(tab_bind._declare(L))

    def set_tables(self, gamma, mu, log_n, sin_k=None, ends=(0, 0), shape=None, with_norm=True, gamma_lo=GLO, gamma_hi=GHI):
        """0, or -1 where rimphony_ctx_set_tables_2d_ends answers RIMPHONY_EINVAL"""
        keep, a = _args(gamma, mu, log_n, sin_k, shape, gamma_lo, gamma_hi)
        return self.L.tabo_set_tables_2d_ends(*a, int(ends[0]), int(ends[1]), int(with_norm))

    def check(self, gamma, mu, log_n, sin_k=None, ends=(0, 0), shape=None, gamma_lo=GLO, gamma_hi=GHI):
        keep, a = _args(gamma, mu, log_n, sin_k, shape, gamma_lo, gamma_hi)
        return self.L.tabo_check_2d_ends(*a, int(ends[0]), int(ends[1]))

    def _sized(self, fn, a, tail):
        size = fn(*a, *tail, None, 0)
        assert size > 0, size
        out = np.zeros(size)
        assert fn(*a, *tail, _dp(out), size) == size
        return out

    def without_ends(self, gamma, mu, log_n, sin_k=None, gamma_lo=GLO, gamma_hi=GHI):
        """the set as the builders lay it out where their trailing arguments are left out, normalisations 0"""
        keep, a = _args(gamma, mu, log_n, sin_k, None, gamma_lo, gamma_hi)
        return self._sized(self.L.tabo_build_2d_without_ends, a, ())

    def lines(self, gamma, mu, log_n, sin_k=None, ends=(0, 0), gamma_lo=GLO, gamma_hi=GHI):
        """the set as the device entry solves it, line by line through the host build of tab_install.h, normalisations 0"""
        keep, a = _args(gamma, mu, log_n, sin_k, None, gamma_lo, gamma_hi)
        return self._sized(self.L.tabo_lines_2d_ends, a, (int(ends[0]), int(ends[1])))

    def put_norms(self, norms):
        norms = np.ascontiguousarray(norms, dtype=np.float64)
        return self.L.tabo_put_norms(len(norms), _dp(norms))

    def bicubic(self, index, gamma, mu):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        s, su, sm = np.zeros_like(gamma), np.zeros_like(gamma), np.zeros_like(gamma)
        assert self.L.tabo_bicubic(float(index), len(gamma), _dp(gamma), _dp(mu), _dp(s), _dp(su), _dp(sm)) == 0
        return s, su, sm


def _tab():
    """The tree's oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = Tab2DEndsLib(_build.build_tab2d_ends_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma, mu, log_n, sin_k=None, ends=(0, 0), **kw):
    return _tab().set_tables(gamma, mu, log_n, sin_k, ends, **kw)


def check(gamma, mu, log_n, sin_k=None, ends=(0, 0), **kw):
    return _tab().check(gamma, mu, log_n, sin_k, ends, **kw)


def without_ends(gamma, mu, log_n, sin_k=None, **kw):
    return _tab().without_ends(gamma, mu, log_n, sin_k, **kw)


def lines(gamma, mu, log_n, sin_k=None, ends=(0, 0), **kw):
    return _tab().lines(gamma, mu, log_n, sin_k, ends, **kw)


def put_norms(norms):
    """the tables' normalisations from a record (the fixture's) into a set installed with_norm=False"""
    return _tab().put_norms(norms)


def blob():
    return _tab().blob()


def form():
    return load().tabo_form()


def batch(s, theta, index, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the table set last given to set_tables()"""
    return _tab().batch(s, theta, index, mask, nthreads)


def batch_norm(index):
    return _tab().batch_norm(index)


def dev_calc_f(par, norm, gamma, cos_xi):
    """(f, dfdg, dfdcx) of the host build of calc_f / calc_f_derivatives of the installed form for table par[0]"""
    return _tab().dev_calc_f(4, par, norm, gamma, cos_xi)


def bicubic(index, gamma, mu):
    """(S, dS/du, dS/dmu) of the host build of the installed form's bicubic for table `index`"""
    return _tab().bicubic(index, gamma, mu)


def mkdist(index):
    return _tab().mkdist(index)


def node_data(b, shape):
    """the node data of a laid-out set of any form, [n_tables][n_nodes][n_mu][4] = {S, S_u, S_mu, S_umu}: its last words"""
    nt, nn, nmu = shape
    return b[-4 * nt * nn * nmu:].reshape(nt, nn, nmu, 4)


def ends_words(b):
    """TAB_2D_ENDS of every table header of a laid-out set"""
    return b[HDR + T_HDR * np.arange(int(b[0])) + T_ENDS]


def norm_at(n_tables):
    return HDR + T_HDR * np.arange(n_tables) + T_NORM


# ---- the node sets ---------------------------------------------------------------------------------------------------------
def mu_jitter(n, seed=20261020):
    """n nodes uniform in mu, each interior one moved by a seeded +-30 % of the spacing; the ends exactly -1 and +1"""
    m = np.linspace(-1.0, 1.0, n)
    r = np.random.default_rng(seed + n).uniform(-0.3, 0.3, n)
    r[0] = r[-1] = 0.0
    m = m + r * (m[1] - m[0])
    m[0], m[-1] = -1.0, 1.0
    return m


def gamma_jitter(n, seed=20261020):
    """n nodes uniform in ln gamma over [GLO, GHI], each interior one moved by a seeded +-30 % of the spacing"""
    u = np.linspace(np.log(GLO), np.log(GHI), n)
    r = np.random.default_rng(seed + 7 * n).uniform(-0.3, 0.3, n)
    r[0] = r[-1] = 0.0
    return np.exp(u + r * (u[1] - u[0]))


def nodes_of(form_name, n_nodes, n_mu):
    """(gamma, mu) as the entry of the form takes them -- None where the form places its own nodes -- and (gamma, mu) where the
    nodes lie.  form_name: "uniform", "grid" (jittered gamma nodes) or "nodes" (jittered gamma and mu nodes)."""
    if form_name == "uniform":
        return None, None, np.exp(np.linspace(np.log(GLO), np.log(GHI), n_nodes)), np.linspace(-1.0, 1.0, n_mu)
    gamma = gamma_jitter(n_nodes)
    if form_name == "grid":
        return gamma, None, gamma, np.linspace(-1.0, 1.0, n_mu)
    mu = mu_jitter(n_mu)
    return gamma, mu, gamma, mu


def u_of(gamma, g_at):
    """ln gamma scaled to [-1, 1] over the nodes g_at: the variable the test polynomials are written in"""
    lo, hi = np.log(g_at[0]), np.log(g_at[-1])
    return (2.0 * np.log(gamma) - (lo + hi)) / (hi - lo)


def smooth_tables(shape, g_at, mu_at, seed=0, jitter=0.0):
    """ln n of a power law per table, rolled off at both ends of the nodes, tilted in mu more the higher gamma and CURVED in mu
    (a bi-Maxwellian's -a(gamma) mu^2), each value moved by a seeded +-jitter"""
    nt = shape[0]
    u, g, m = np.log(g_at)[None, :, None], g_at[None, :, None], mu_at[None, None, :]
    p = (2.0 + 0.5 * np.arange(nt))[:, None, None]
    t = -p * u + 0.05 * u * m + 0.7 * m - 0.3 * u * m * m - 2.0 / g - 5.0 * g / g_at[-1]
    rng = np.random.default_rng(20261020 + seed)
    return np.ascontiguousarray(t * (1.0 + rng.uniform(-jitter, jitter, shape)))


# ---- the fixture (tests/golden/tabulated_2d_ends_det.npz, tools/make_tabulated_2d_ends_fixture.py) ---------------------------
FIXTURE_K = (None, (0.5, 2.0))
FIXTURE_ENDS = (NOT_A_KNOT, NOT_A_KNOT)


def bimaxwellian(g_at, mu_at, theta_e, a):
    """ln n of n = gamma^2 beta exp(-(gamma - 1)(1 + a mu^2) / theta_e): quadratic in mu with a coefficient that grows with
    gamma, so not separable"""
    g, m = g_at[:, None], mu_at[None, :]
    return np.log(g * np.sqrt(g * g - 1.0)) - (g - 1.0) * (1.0 + a * m * m) / theta_e


def fixture_set(which):
    """(gamma, gamma_lo, gamma_hi, mu, log_n, sin_k): set 0 is 64 x 16 on uniform nodes over [1.01, 300], two bi-Maxwellians
    (theta_e 3 and 10, a 0.5 and -0.3); set 1 is 40 x 12 on jittered gamma and mu nodes over [GLO, GHI] with sin_k = 0.5, 2.0,
    two surfaces of smooth_tables"""
    if which == 0:
        lo, hi = 1.01, 300.0
        g_at, mu_at = np.exp(np.linspace(np.log(lo), np.log(hi), 64)), np.linspace(-1.0, 1.0, 16)
        t = np.stack([bimaxwellian(g_at, mu_at, 3.0, 0.5), bimaxwellian(g_at, mu_at, 10.0, -0.3)])
        return None, lo, hi, None, t, None
    gamma, mu, g_at, mu_at = nodes_of("nodes", 40, 12)
    return gamma, GLO, GHI, mu, smooth_tables((2, 40, 12), g_at, mu_at), np.array(FIXTURE_K[1])



# ---- the measurements the host tests assert and tools/tab_2d_ends_accuracy.py records -----------------------------------------
CUBIC_SHAPES = [(8, 8), (9, 11)]
P3, Q3 = (0.3, -0.8, 0.5, 0.9), (-0.2, 0.7, -0.6, 0.4)      # coefficients of 1, x, x^2, x^3
R3, T3 = (1.0, -2.0, 0.4, -0.7), (0.0, 0.5, -1.1, 0.8)


def _poly(c, x):
    return c[0] + x * (c[1] + x * (c[2] + x * c[3]))


def _dpoly(c, x):
    return c[1] + x * (2.0 * c[2] + x * 3.0 * c[3])


def cubic_surface(gamma, mu, g_at):
    """(S, S_u, S_mu) of S = P(x) Q(mu) + R(x) + T(mu), x = ln gamma scaled to [-1, 1] over the nodes, P, Q, R, T of degree 3,
    at the points (gamma[i], mu[i]) or, for gamma [n][1] and mu [1][m], on their grid"""
    x = u_of(gamma, g_at)
    dxdu = 2.0 / (np.log(g_at[-1]) - np.log(g_at[0]))
    s = _poly(P3, x) * _poly(Q3, mu) + _poly(R3, x) + _poly(T3, mu)
    su = (_dpoly(P3, x) * _poly(Q3, mu) + _dpoly(R3, x)) * dxdu
    sm = _poly(P3, x) * _dpoly(Q3, mu) + _dpoly(T3, mu)
    return s, su, sm


def cubic_points(g_at, mu_at, n=200, seed=3):
    """n points off the nodes: a quarter of them in the end cells of the gamma nodes, a quarter in the end cells of the mu nodes,
    the others anywhere inside"""
    rng = np.random.default_rng(seed)
    u_at = np.log(g_at)
    u = rng.uniform(u_at[0], u_at[-1], n)
    m = rng.uniform(-1.0, 1.0, n)
    q = n // 4
    u[:q:2] = rng.uniform(u_at[0], u_at[1], len(u[:q:2]))
    u[1:q:2] = rng.uniform(u_at[-2], u_at[-1], len(u[1:q:2]))
    m[q:2 * q:2] = rng.uniform(mu_at[0], mu_at[1], len(m[q:2 * q:2]))
    m[q + 1:2 * q:2] = rng.uniform(mu_at[-2], mu_at[-1], len(m[q + 1:2 * q:2]))
    u = np.clip(u, u_at[0] + 1e-9, u_at[-1] - 1e-9)
    m = np.clip(m, -1.0 + 1e-9, 1.0 - 1e-9)
    return np.exp(u), m


def cubic_deviation(form_name, shape, ends):
    """The worst deviation of S, S_u and S_mu of the oracle's bicubic from the cubic surface over cubic_points, relative to
    max |S| at the nodes, for the set of `shape` = (n_nodes, n_mu) on the geometry `form_name` installed with `ends`"""
    nn, nmu = shape
    gamma, mu, g_at, mu_at = nodes_of(form_name, nn, nmu)
    t = cubic_surface(g_at[:, None], mu_at[None, :], g_at)[0]
    assert set_tables(gamma, mu, t, None, ends, with_norm=False) == 0
    pg, pm = cubic_points(g_at, mu_at)
    got = bicubic(0, pg, pm)
    want = cubic_surface(pg, pm, g_at)
    return max(np.abs(g - w).max() for g, w in zip(got, want)) / np.abs(t).max()


SCIPY_SHAPES = [(3, 9, 11), (1, 70, 13)]


def scipy_difference(shape, ends=(NOT_A_KNOT, NOT_A_KNOT)):
    """The worst difference between the S_u, S_mu and S_umu words of the set of `shape` on jittered gamma and mu nodes
    (smooth_tables, each value jittered by 2 %) and scipy's CubicSpline through the same lines, each line scaled by its own
    max |slope|.  S_umu: the spline along u through the S_mu column scipy gave."""
    from scipy.interpolate import CubicSpline
    bc = ("natural", "not-a-knot")
    gamma, mu, g_at, mu_at = nodes_of("nodes", shape[1], shape[2])
    t = smooth_tables(shape, g_at, mu_at, seed=shape[1], jitter=0.02)
    assert set_tables(gamma, mu, t, None, ends, with_norm=False) == 0
    nd = node_data(blob(), shape)
    u = np.log(g_at)
    su = CubicSpline(u, t, axis=1, bc_type=bc[ends[0]])(u, 1)
    sm = CubicSpline(mu_at, t, axis=2, bc_type=bc[ends[1]])(mu_at, 1)
    sum_ = CubicSpline(u, sm, axis=1, bc_type=bc[ends[0]])(u, 1)
    worst = 0.0
    for got, want, axis in ((nd[..., 1], su, 1), (nd[..., 2], sm, 2), (nd[..., 3], sum_, 1)):
        scale = np.abs(want).max(axis=axis, keepdims=True)
        worst = max(worst, (np.abs(got - want) / scale).max())
    return worst


NORM_A, NORM_NMU, NORM_NODES = 2.0, 16, 64


def norm_deviation(ends):
    """|N_iso / N / P - 1| for the table S = H(u) + a mu^2 (a = 2, 64 x 16 uniform nodes over [GLO, GHI], H a rolled power
    law) installed with `ends`: N its normalisation, N_iso that of S = H(u) on the same nodes, P = 1/2 int exp(a mu^2) dmu =
    1/2 sqrt(pi / a) erfi(sqrt a) from scipy.special"""
    from scipy.special import erfi
    g_at, mu_at = np.exp(np.linspace(np.log(GLO), np.log(GHI), NORM_NODES)), np.linspace(-1.0, 1.0, NORM_NMU)
    h = tab_bind.log_n_rolled_powerlaw(g_at)[:, None]
    one = np.array([0.0])
    assert set_tables(None, None, h + 0.0 * mu_at[None, :], None, ends) == 0
    n_iso = batch_norm(one)[0]
    assert set_tables(None, None, h + NORM_A * mu_at[None, :] ** 2, None, ends) == 0
    n = batch_norm(one)[0]
    p = 0.5 * np.sqrt(np.pi / NORM_A) * erfi(np.sqrt(NORM_A))
    return abs(n_iso / n / p - 1.0)
