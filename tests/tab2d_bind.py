"""ctypes binding of the 2-D table oracle (tests/support/liboracle_tab2d.so: the CPU oracle's calculators on top of the host
build of the tabulated distribution's device functions, table sets ln n(gamma, mu) on a grid) and of the analytic tilt
oracle (liboracle_tilt.so), with the tables the tests and the fixture share.  Test infrastructure only."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_size_t, c_uint32, c_uint64

import numpy as np

import tab_bind
from oracle_bind import Dist

_lib = None
_tilt = None


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    """the entries of liboracle_tab2d.so: tab_bind's, with tabo_set_tables_2d in the place of tabo_set_tables"""
    dp = POINTER(c_double)
    L.tabo_check_2d.restype = c_int
    L.tabo_check_2d.argtypes = [c_size_t, c_size_t, c_double, c_double, c_size_t, dp]
    L.tabo_set_tables_2d.restype = c_int
    L.tabo_set_tables_2d.argtypes = [c_size_t, c_size_t, c_double, c_double, c_size_t, dp, c_int]
    L.tabo_get_blob.restype = c_size_t
    L.tabo_get_blob.argtypes = [dp, c_size_t]
    L.tabo_batch.restype = c_int
    L.tabo_batch.argtypes = [c_size_t, dp, dp, dp, c_uint32, dp, POINTER(c_uint64), c_int]
    L.tabo_batch_norm.restype = c_int
    L.tabo_batch_norm.argtypes = [c_size_t, dp, dp]
    L.tabo_dev_calc_f.restype = c_int
    L.tabo_dev_calc_f.argtypes = [c_int, dp, c_double, c_size_t, dp, dp, dp, dp, dp]
    L.tabo_bicubic.restype = c_int
    L.tabo_bicubic.argtypes = [c_double, c_size_t, dp, dp, dp, dp, dp]
    # the calculators' seams (oracle/rimo.h), reached with a kind-4 rimo_dist: mkdist()
    L.rimo_dist_init.restype = c_int
    L.rimo_dist_init.argtypes = [POINTER(Dist), c_int, dp]
    L.rimo_gamma_integrand.restype = c_double
    L.rimo_gamma_integrand.argtypes = [POINTER(Dist), c_int, c_int, c_double, c_double, c_double, c_double]
    L.rimo_gamma_integral.restype = c_double
    L.rimo_gamma_integral.argtypes = [POINTER(Dist), c_int, c_int, c_int, c_double, c_double, c_double]
    L.rimo_hey_element.restype = c_double
    L.rimo_hey_element.argtypes = [POINTER(Dist), c_int, c_double, c_double, c_int, c_double, c_double]
    L.rimo_hey_outer_integrand.restype = c_double
    L.rimo_hey_outer_integrand.argtypes = [POINTER(Dist), c_int, c_double, c_double, c_int, c_double]
    return L


def as_set(log_n):
    """[n_tables][n_nodes][n_mu], contiguous float64: a 2-D array is one table"""
    t = np.asarray(log_n, dtype=np.float64)
    if t.ndim == 2:
        t = t[None]
    assert t.ndim == 3
    return np.ascontiguousarray(t)


class Tab2DLib(tab_bind.TabLib):
    """tab_bind.TabLib on the 2-D oracle: set_tables(gamma_lo, gamma_hi, log_n[, shape]) replaces the isotropic one, which
    this library does not have; blob, batch, batch_norm, dev_calc_f and mkdist are inherited."""

    def __init__(self, path):
        self.L = _declare(ctypes.CDLL(path))

    def set_tables(self, gamma_lo, gamma_hi, log_n, shape=None, with_norm=True):
        """0, or -1 where rimphony_ctx_set_tables_2d answers RIMPHONY_EINVAL.  shape: the (n_tables, n_nodes, n_mu) the call
        states (default: log_n's own) -- the misuse tests state one that the buffer merely covers."""
        t = as_set(log_n) if shape is None else np.ascontiguousarray(log_n, dtype=np.float64)
        nt, nn, nmu = t.shape if shape is None else shape
        return self.L.tabo_set_tables_2d(nt, nn, float(gamma_lo), float(gamma_hi), nmu, _dp(t), int(with_norm))

    def check(self, gamma_lo, gamma_hi, log_n, shape=None):
        t = as_set(log_n) if shape is None else np.ascontiguousarray(log_n, dtype=np.float64)
        nt, nn, nmu = t.shape if shape is None else shape
        return self.L.tabo_check_2d(nt, nn, float(gamma_lo), float(gamma_hi), nmu, _dp(t))

    def bicubic(self, index, gamma, mu):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        s, su, sm = np.zeros_like(gamma), np.zeros_like(gamma), np.zeros_like(gamma)
        assert self.L.tabo_bicubic(float(index), len(gamma), _dp(gamma), _dp(mu), _dp(s), _dp(su), _dp(sm)) == 0
        return s, su, sm


def _tab():
    """The tree's 2-D oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = Tab2DLib(_build.build_tab2d_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma_lo, gamma_hi, log_n, shape=None, with_norm=True):
    return _tab().set_tables(gamma_lo, gamma_hi, log_n, shape, with_norm)


def check(gamma_lo, gamma_hi, log_n, shape=None):
    return _tab().check(gamma_lo, gamma_hi, log_n, shape)


def blob():
    return _tab().blob()


def batch(s, theta, index, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the table set last given to set_tables()"""
    return _tab().batch(s, theta, index, mask, nthreads)


def batch_norm(index):
    return _tab().batch_norm(index)


def dev_calc_f(par, norm, gamma, cos_xi):
    """(f, dfdg, dfdcx) of the host build of calc_f<6> / calc_f_derivatives<6> for table par[0]"""
    return _tab().dev_calc_f(4, par, norm, gamma, cos_xi)


def bicubic(index, gamma, mu):
    """(S, dS/du, dS/dmu) of the host build of tab_bicubic for table `index`"""
    return _tab().bicubic(index, gamma, mu)


def mkdist(index):
    return _tab().mkdist(index)


# ---- layout of the laid-out set (dev_symphony.h: TAB_HDR_*, TAB_2D_*) ---------------------------------------------------
HDR, HDR_NMU, T_HDR, T_NORM = 8, 7, 8, 3


def table_header(blob_, table):
    """{n_mu - 2, 1 / h_mu, h_mu, norm, 4 spare words} of one table"""
    return blob_[HDR + table * T_HDR:HDR + (table + 1) * T_HDR]


def table_nodes(blob_, table):
    """[n_nodes][n_mu][4] = {S, S_u, S_mu, S_umu} of one table"""
    nt, nn, nmu = int(blob_[0]), int(blob_[1]), int(-blob_[HDR_NMU])
    base = HDR + nt * T_HDR + table * nn * nmu * 4
    return blob_[base:base + nn * nmu * 4].reshape(nn, nmu, 4)


# ---- the analytic tilt oracle -------------------------------------------------------------------------------------------
class TiltLib:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        dp = POINTER(c_double)
        L.tilto_set_extra.restype = None
        L.tilto_set_extra.argtypes = [c_double, c_double, c_double]
        L.tilto_batch.restype = c_int
        L.tilto_batch.argtypes = [c_size_t, dp, dp, dp, c_uint32, dp, c_int]
        L.tilto_norm.restype = c_double
        L.tilto_norm.argtypes = [dp]
        L.tilto_calc_f.restype = None
        L.tilto_calc_f.argtypes = [dp, c_double, c_size_t, dp, dp, dp, dp, dp]
        self.L = L


def tilt():
    global _tilt
    if _tilt is None:
        from rimphony_amd import _build
        _tilt = TiltLib(_build.build_tilt_oracle())
    return _tilt.L


def tilt_batch(s, theta, par, extra=(0.0, 0.0, 0.0), mask=0xFF, nthreads=8):
    """out [n][8] of the analytic distribution; par = {p, gamma_min, gamma_max, gamma_cutoff, a, q}, extra = (g1, c1, c2)"""
    s = np.ascontiguousarray(s, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    par = np.ascontiguousarray(par, dtype=np.float64)
    assert par.shape == (6,)
    out = np.zeros((len(s), 8))
    tilt().tilto_set_extra(*[float(x) for x in extra])
    assert tilt().tilto_batch(len(s), _dp(s), _dp(theta), _dp(par), mask, _dp(out), nthreads) == 0
    return out


def tilt_norm(par, extra=(0.0, 0.0, 0.0)):
    tilt().tilto_set_extra(*[float(x) for x in extra])
    return tilt().tilto_norm(_dp(np.ascontiguousarray(par, dtype=np.float64)))


def tilt_calc_f(par, norm, gamma, cos_xi, extra=(0.0, 0.0, 0.0)):
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    cos_xi = np.ascontiguousarray(cos_xi, dtype=np.float64)
    f, a, b = np.zeros_like(gamma), np.zeros_like(gamma), np.zeros_like(gamma)
    tilt().tilto_set_extra(*[float(x) for x in extra])
    tilt().tilto_calc_f(_dp(np.ascontiguousarray(par, dtype=np.float64)), float(norm), len(gamma), _dp(gamma), _dp(cos_xi),
                        _dp(f), _dp(a), _dp(b))
    return f, a, b


# ---- the tables the tests and the fixture share -------------------------------------------------------------------------
EDGE_LO, EDGE_HI = 1.01, 1e4
TILT_P, TILT_G1, TILT_G2, TILT_A, TILT_Q = 2.5, 30.0, 500.0, 0.5, 0.3
GROW_P, GROW_G1, GROW_G2, GROW_C1, GROW_C2 = 3.5, 10.0, 200.0, 0.8, -1.5
# the closed forms of tables 0 and 2 as the tilt oracle takes them: (par, extra)
TILT_CLOSED = ([TILT_P, EDGE_LO, EDGE_HI, TILT_G2, TILT_A, TILT_Q], (TILT_G1, 0.0, 0.0))
GROW_CLOSED = ([GROW_P, EDGE_LO, EDGE_HI, GROW_G2, 0.0, 0.0], (GROW_G1, GROW_C1, GROW_C2))


def columns(n_nodes, lo=EDGE_LO, hi=EDGE_HI):
    """[3][n_nodes] = (u, gamma, the Juettner column) at the gamma nodes: everything about a table that takes a logarithm or
    an exponential.  The fixture stores these, so that a table built from them is the same bits on every machine."""
    u = np.linspace(np.log(lo), np.log(hi), n_nodes)
    g = np.exp(u)
    return np.stack([u, g, tab_bind.log_n_juettner(g, 10.0)])


def _split(n_nodes, n_mu, cols):
    cols = columns(n_nodes) if cols is None else np.asarray(cols, dtype=np.float64)
    assert cols.shape == (3, n_nodes)
    return cols[0][:, None], cols[1][:, None], cols[2][:, None], np.linspace(-1.0, 1.0, n_mu)[None, :]


def table_tilted(n_nodes, n_mu, cols=None):
    """(0) a tilted rolled power law, ln n = -p u + q u mu + a mu - g1 / gamma - gamma / g2: bilinear in the middle"""
    u, g, _, mu = _split(n_nodes, n_mu, cols)
    return -TILT_P * u + TILT_Q * u * mu + TILT_A * mu - TILT_G1 / g - g / TILT_G2


def table_juettner(n_nodes, n_mu, cols=None):
    """(1) the T = 10 Juettner shape, no mu dependence"""
    _, _, j, mu = _split(n_nodes, n_mu, cols)
    return j + 0.0 * mu


def table_growing(n_nodes, n_mu, cols=None):
    """(2) a rolled power law plus (0.8 mu - 1.5 mu^2) (u - u_lo) / (u_hi - u_lo): an anisotropy that grows with energy,
    curved and non-separable"""
    u, g, _, mu = _split(n_nodes, n_mu, cols)
    w = (u - u[0]) / (u[-1] - u[0])
    return -GROW_P * u - GROW_G1 / g - g / GROW_G2 + (GROW_C1 * mu + GROW_C2 * mu * mu) * w


def edge_tables_2d(n_nodes, n_mu, cols=None):
    """the three-table set over [1.01, 1e4]; cols: columns(n_nodes), or the fixture's copy of them"""
    return np.stack([table_tilted(n_nodes, n_mu, cols), table_juettner(n_nodes, n_mu, cols), table_growing(n_nodes, n_mu, cols)])
