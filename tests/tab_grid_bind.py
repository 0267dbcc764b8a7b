"""ctypes binding of the table oracle for sets on given gamma nodes (tests/support/liboracle_tabgrid.so: the CPU oracle's
calculators on top of the host build of the tabulated distribution's device functions and of rim_tab_check_grid /
rim_tab_build_grid), with the grids and table sets the tests and the fixture share.  Test infrastructure only."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_longlong, c_size_t

import numpy as np

import tab_bind
import tab_pitchy_bind as tpy

_lib = None


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_set_tables_grid.restype = c_int
    L.tabo_set_tables_grid.argtypes = [c_size_t, c_size_t, dp, dp, c_size_t, dp, dp]
    L.tabo_check_grid.restype = c_int
    L.tabo_check_grid.argtypes = [c_size_t, c_size_t, dp, dp, c_size_t, dp, dp]
    L.tabo_grid_interval.restype = c_longlong
    L.tabo_grid_interval.argtypes = [c_double]
    L.tabo_grid_reads.restype = c_longlong
    L.tabo_grid_reads.argtypes = []
    L.tabo_log.restype = c_double
    L.tabo_log.argtypes = [c_double]
    L.tabo_grid_spline.restype = c_int
    L.tabo_grid_spline.argtypes = [c_double, c_size_t, dp, dp, dp]
    L.tabo_grid_slopes.restype = None
    L.tabo_grid_slopes.argtypes = [c_size_t, dp, dp, c_int, dp]
    L.tabo_p_intervals.restype = c_int
    L.tabo_p_intervals.argtypes = []
    L.tabo_table_k_p.restype = c_int
    L.tabo_table_k_p.argtypes = [c_double, dp, dp]
    return L


class TabGridLib(tab_bind.TabLib):
    """tab_bind.TabLib on the grid oracle: set_tables(gamma, log_n, log_g, sin_k); blob, batch, batch_norm, dev_calc_f and
    mkdist are inherited."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        # the shared entries (tabo_batch, the calculators' seams, ...) are declared as tab_bind declares them; its
        # tabo_set_tables, which this oracle does not have, is given the grid entry's name and declared again below
        L.tabo_set_tables = L.tabo_set_tables_grid
        self.L = _declare(tab_bind._declare(L))

    def set_tables(self, gamma, log_n, log_g=None, sin_k=None, n_mu=None, n_nodes=None):
        """0, or -1 where rimphony_ctx_set_tables_grid answers RIMPHONY_EINVAL.  n_nodes, n_mu: what the call states
        (default: the lengths of gamma and of a row of log_g)."""
        gamma = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.float64)
        log_n = None if log_n is None else np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
        if log_g is not None:
            log_g = np.ascontiguousarray(np.atleast_2d(log_g), dtype=np.float64)
        if n_mu is None:
            n_mu = 0 if log_g is None else log_g.shape[1]
        if n_nodes is None:
            n_nodes = len(gamma)
        n_tables = 1 if log_n is None else log_n.shape[0]
        if sin_k is not None:
            sin_k = np.ascontiguousarray(np.atleast_1d(sin_k), dtype=np.float64)
        return self.L.tabo_set_tables_grid(n_tables, int(n_nodes), _dp(gamma), _dp(log_n), int(n_mu), _dp(log_g), _dp(sin_k))


def _tab():
    """The tree's grid oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = TabGridLib(_build.build_tab_grid_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma, log_n, log_g=None, sin_k=None, n_mu=None, n_nodes=None):
    return _tab().set_tables(gamma, log_n, log_g, sin_k, n_mu, n_nodes)


def check(gamma, log_n, log_g=None, sin_k=None, n_mu=None, n_nodes=None, n_tables=None):
    """rim_tab_check_grid: 0 or -1; every argument is passed as given (None: a null pointer)"""
    gamma = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.float64)
    log_n = None if log_n is None else np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
    log_g = None if log_g is None else np.ascontiguousarray(np.atleast_2d(log_g), dtype=np.float64)
    sin_k = None if sin_k is None else np.ascontiguousarray(np.atleast_1d(sin_k), dtype=np.float64)
    if n_mu is None:
        n_mu = 0 if log_g is None else log_g.shape[1]
    if n_nodes is None:
        n_nodes = len(gamma)
    if n_tables is None:
        n_tables = log_n.shape[0]
    return load().tabo_check_grid(int(n_tables), int(n_nodes), _dp(gamma), _dp(log_n), int(n_mu), _dp(log_g), _dp(sin_k))


def blob():
    return _tab().blob()


def batch(s, theta, index, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the table set last given to set_tables()"""
    return _tab().batch(s, theta, index, mask, nthreads)


def batch_norm(index):
    return _tab().batch_norm(index)


def dev_calc_f(par, norm, gamma, cos_xi):
    """(f, dfdg, dfdcx) of the host build of calc_f<8> / calc_f_derivatives<8> for table par[0]"""
    return _tab().dev_calc_f(4, par, norm, gamma, cos_xi)


def mkdist(index):
    return _tab().mkdist(index)


def table_k_p(index):
    k, p = c_double(), c_double()
    assert load().tabo_table_k_p(float(index), ctypes.byref(k), ctypes.byref(p)) == 0
    return k.value, p.value


def interval(gamma):
    """(the interval the device function finds in table 0, the node words its bisection read)"""
    L = load()
    j = L.tabo_grid_interval(float(gamma))
    return j, L.tabo_grid_reads()


def intervals(gamma):
    L = load()
    out, reads = np.zeros(len(gamma), dtype=np.int64), 0
    for i, g in enumerate(np.asarray(gamma, dtype=np.float64)):
        out[i] = L.tabo_grid_interval(float(g))
        reads = max(reads, L.tabo_grid_reads())
    return out, reads


def rim_log(gamma):
    """u = rim_log(gamma) of detmath.h, as the lookup forms it"""
    L = load()
    return np.array([L.tabo_log(float(g)) for g in np.asarray(gamma, dtype=np.float64)])


def spline(index, gamma):
    """(H, dH/du) of table `index` through tab_spline_grid"""
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    h, d = np.zeros_like(gamma), np.zeros_like(gamma)
    assert load().tabo_grid_spline(float(index), len(gamma), _dp(gamma), _dp(h), _dp(d)) == 0
    return h, d


def slopes(u, y, mutated=False):
    u = np.ascontiguousarray(u, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    m = np.zeros_like(u)
    load().tabo_grid_slopes(len(u), _dp(u), _dp(y), int(mutated), _dp(m))
    return m


def n_integral(dist, coeff, stokes, negative_lobe, s, theta, n_lo, n_hi):
    """rimo_n_integral: the value, or NaN when the QAG reports an error (as tab_bind.n_integral)"""
    v = c_double()
    rc = load().rimo_n_integral(ctypes.byref(dist), coeff, stokes, negative_lobe, s, theta, n_lo, n_hi, ctypes.byref(v))
    return v.value if rc == 0 else float("nan")


class Blob:
    """The parts of a laid-out grid set (dev_symphony.h: tab_grid_*)"""

    def __init__(self, b):
        self.n_tables, self.n_nodes, self.cells = int(b[0]), int(b[1]), int(b[6])
        self.u0, self.inv_cell = b[4], b[5]
        gd = ((self.cells + 2) // 2 + 7) & ~7
        self.guide = b[8:8 + gd].view(np.uint32)[:self.cells + 1]
        self.nodes = b[8 + gd:8 + gd + self.n_tables * self.n_nodes * 4].reshape(self.n_tables, self.n_nodes, 4)
        self.u = self.nodes[0, :, 0]


# ---- the grids -------------------------------------------------------------------------------------------------------
EDGE_LO, EDGE_HI = 1.01, 1e4


def log_gm1_nodes(gm1_lo, gm1_hi, n):
    """n gamma uniform in ln(gamma - 1) over gamma - 1 in [gm1_lo, gm1_hi]"""
    return 1.0 + np.exp(np.linspace(np.log(gm1_lo), np.log(gm1_hi), n))


def jitter_nodes(n, seed=20261018):
    """n nodes uniform in ln gamma over [1.01, 1e4], each interior one moved by a seeded +-40 % of its spacing"""
    u = np.linspace(np.log(EDGE_LO), np.log(EDGE_HI), n)
    r = np.random.default_rng(seed + n).uniform(-0.4, 0.4, n)
    r[0] = r[-1] = 0.0
    return np.exp(u + r * (u[1] - u[0]))


def gap_nodes(n=64, at=20):
    """n nodes uniform in ln gamma but for interval `at`, which is 1000 times the others: it spans most guide cells"""
    w = np.ones(n - 1)
    w[at] = 1000.0
    u = np.log(EDGE_LO) + np.concatenate([[0.0], np.cumsum(w)]) * (np.log(EDGE_HI) - np.log(EDGE_LO)) / w.sum()
    return np.exp(u)


def grid(name):
    if name == "log-gm1":
        return log_gm1_nodes(1e-6, 1e4, 64)
    if name == "log-gm1-2048":
        return log_gm1_nodes(1e-6, 1e4, 2048)
    if name == "jitter8":
        return jitter_nodes(8)
    if name == "jitter":
        return jitter_nodes(64)
    if name == "gap":
        return gap_nodes()
    if name == "uniform":
        return tab_bind.nodes(EDGE_LO, EDGE_HI, 64)
    raise KeyError(name)


GRIDS = ("log-gm1", "jitter8", "jitter", "gap", "uniform")


def edge_tables_at(gamma):
    """The three shapes of tab_bind.edge_tables at the given nodes: rolled power laws and a T = 10 Juettner shape, all
    negligible at both ends of every grid here, so that the quadratures see no step"""
    return np.stack([tab_bind.log_n_rolled_powerlaw(gamma, 2.5, 30., 500.), tab_bind.log_n_juettner(gamma, 10.),
                     tab_bind.log_n_rolled_powerlaw(gamma, 3.5, 10., 200.)])


SET_A_K = (0.5, 2.0, 0.0)
SET_B_K = (1.5, 0.3, 3.0)


def fixture_set(which):
    """(gamma, log_n, log_g, sin_k) of set A (0: the log-gm1 grid, no g) or B (1: the 64-node jitter grid, pitch rows of 8
    nodes)"""
    if which == 0:
        g = grid("log-gm1")
        return g, edge_tables_at(g), None, np.array(SET_A_K)
    g = grid("jitter")
    return g, edge_tables_at(g), tpy.set_b_rows(), np.array(SET_B_K)


# ---- the case the form is for ----------------------------------------------------------------------------------------
COLD_T, COLD_LO, COLD_HI = 0.1, 1.0 + 1e-6, 31.0
COLD_S = np.array([3., 10., 20., 30., 50., 100.])
COLD_THETA = np.array([0.6, 1.0, 0.8, 1.3, 0.4, 0.9])


def cold_grid(n=512):
    g = log_gm1_nodes(COLD_LO - 1.0, COLD_HI - 1.0, n)
    g[0], g[-1] = COLD_LO, COLD_HI
    return g
