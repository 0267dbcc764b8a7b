"""ctypes binding of the table oracle for 2-D sets on given gamma nodes (tests/support/liboracle_tab2dgrid.so: the CPU
oracle's calculators on top of the host build of the tabulated distribution's device functions and of rim_tab_check_2d_grid /
rim_tab_build_2d_grid), with the grids and table sets the tests and the fixture share.  Test infrastructure only."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_longlong, c_size_t

import numpy as np

import tab_bind
import tab2d_bind as t2
import tab_grid_bind as tg

_lib = None


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_check_2d_grid.restype = c_int
    L.tabo_check_2d_grid.argtypes = [c_size_t, c_size_t, dp, c_size_t, dp]
    L.tabo_set_tables_2d_grid.restype = c_int
    L.tabo_set_tables_2d_grid.argtypes = [c_size_t, c_size_t, dp, c_size_t, dp, c_int]
    L.tabo_put_norms.restype = c_int
    L.tabo_put_norms.argtypes = [c_size_t, dp]
    L.tabo_bicubic.restype = c_int
    L.tabo_bicubic.argtypes = [c_double, c_size_t, dp, dp, dp, dp, dp]
    L.tabo_grid_interval.restype = c_longlong
    L.tabo_grid_interval.argtypes = [c_double]
    L.tabo_grid_reads.restype = c_longlong
    L.tabo_grid_reads.argtypes = []
    L.tabo_log.restype = c_double
    L.tabo_log.argtypes = [c_double]
    return L


def _args(gamma, log_n, shape):
    """(n_tables, n_nodes, n_mu, gamma, log_n) as the C entry takes them; shape: what the call states (default: log_n's own)"""
    gamma = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.float64)
    if log_n is not None:
        log_n = t2.as_set(log_n) if shape is None else np.ascontiguousarray(log_n, dtype=np.float64)
    nt, nn, nmu = log_n.shape if shape is None else shape
    return int(nt), int(nn), int(nmu), gamma, log_n


class Tab2DGridLib(tab_bind.TabLib):
    """tab_bind.TabLib on this oracle: set_tables(gamma, log_n[, shape]); blob, batch, batch_norm, dev_calc_f and mkdist are
    inherited.  A test of the tests binds a privately built copy with Tab2DGridLib(path)."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        # the shared entries are declared as tab_bind declares them; its tabo_set_tables, which this oracle does not have,
        # is given this entry's name and declared again by _declare
        L.tabo_set_tables = L.tabo_set_tables_2d_grid
        self.L = _declare(tab_bind._declare(L))

    def set_tables(self, gamma, log_n, shape=None, with_norm=True):
        """0, or -1 where rimphony_ctx_set_tables_2d_grid answers RIMPHONY_EINVAL"""
        nt, nn, nmu, gamma, log_n = _args(gamma, log_n, shape)
        return self.L.tabo_set_tables_2d_grid(nt, nn, _dp(gamma), nmu, _dp(log_n), int(with_norm))

    def put_norms(self, norms):
        norms = np.ascontiguousarray(norms, dtype=np.float64)
        return self.L.tabo_put_norms(len(norms), _dp(norms))

    def check(self, gamma, log_n, shape=None):
        nt, nn, nmu, gamma, log_n = _args(gamma, log_n, shape)
        return self.L.tabo_check_2d_grid(nt, nn, _dp(gamma), nmu, _dp(log_n))

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
        _lib = Tab2DGridLib(_build.build_tab2d_grid_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma, log_n, shape=None, with_norm=True):
    return _tab().set_tables(gamma, log_n, shape, with_norm)


def put_norms(norms):
    """the tables' normalisations from a record (the fixture's) into a set installed with_norm=False"""
    return _tab().put_norms(norms)


def check(gamma, log_n, shape=None):
    return _tab().check(gamma, log_n, shape)


def blob():
    return _tab().blob()


def batch(s, theta, index, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the table set last given to set_tables()"""
    return _tab().batch(s, theta, index, mask, nthreads)


def batch_norm(index):
    return _tab().batch_norm(index)


def dev_calc_f(par, norm, gamma, cos_xi):
    """(f, dfdg, dfdcx) of the host build of calc_f<9> / calc_f_derivatives<9> for table par[0]"""
    return _tab().dev_calc_f(4, par, norm, gamma, cos_xi)


def bicubic(index, gamma, mu):
    """(S, dS/du, dS/dmu) of the host build of tab_bicubic_grid for table `index`"""
    return _tab().bicubic(index, gamma, mu)


def mkdist(index):
    return _tab().mkdist(index)


def intervals(gamma):
    """(the intervals in u the device function finds, the most node words a bisection read)"""
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


class Blob:
    """The parts of a laid-out set (dev_symphony.h: tab_2d_grid_*)"""

    def __init__(self, b):
        self.n_tables, self.n_nodes, self.cells, self.n_mu = int(b[0]), int(b[1]), int(b[6]), int(-b[7])
        self.gamma_lo, self.gamma_hi, self.u0, self.inv_cell = b[2], b[3], b[4], b[5]
        at = 8
        self.headers = b[at:at + 8 * self.n_tables].reshape(self.n_tables, 8)
        at += 8 * self.n_tables
        gd = ((self.cells + 2) // 2 + 7) & ~7
        self.guide = b[at:at + gd].view(np.uint32)[:self.cells + 1]
        at += gd
        ud = (2 * self.n_nodes + 7) & ~7
        self.unodes = b[at:at + 2 * self.n_nodes].reshape(self.n_nodes, 2)
        self.u = self.unodes[:, 0]
        at += ud
        per = self.n_nodes * self.n_mu * 4
        self.size = at + self.n_tables * per
        self.nodes = b[at:self.size].reshape(self.n_tables, self.n_nodes, self.n_mu, 4)


# ---- the tables the tests and the fixture share -------------------------------------------------------------------------
def surfaces_at(gamma, n_mu):
    """The three shapes of tab2d_bind.edge_tables_2d at the given gamma nodes (none separable): the tilted rolled power law,
    a T = 10 Juettner shape with a beam that grows with energy, the rolled power law with a growing curved anisotropy.  All
    negligible at both ends of every grid here."""
    gamma = np.asarray(gamma, dtype=np.float64)
    u, g = np.log(gamma)[:, None], gamma[:, None]
    mu = np.linspace(-1.0, 1.0, n_mu)[None, :]
    w = (u - u[0]) / (u[-1] - u[0])
    tilted = -t2.TILT_P * u + t2.TILT_Q * u * mu + t2.TILT_A * mu - t2.TILT_G1 / g - g / t2.TILT_G2
    beam = tab_bind.log_n_juettner(gamma, 10.0)[:, None] + 0.6 * mu * w
    growing = -t2.GROW_P * u - t2.GROW_G1 / g - g / t2.GROW_G2 + (t2.GROW_C1 * mu + t2.GROW_C2 * mu * mu) * w
    return np.stack([tilted, beam, growing])


def fixture_grid(which):
    """the gamma nodes of set A (0: 64 nodes uniform in ln(gamma - 1) over gamma - 1 in [1e-6, 1e4]) or B (1: 16 jittered nodes)"""
    return tg.grid("log-gm1") if which == 0 else tg.jitter_nodes(16)


FIXTURE_NMU = (8, 1024)


def fixture_set(which):
    """(gamma, log_n) of set A (64 x 8 nodes) or B (16 x 1024 nodes)"""
    g = fixture_grid(which)
    return g, surfaces_at(g, FIXTURE_NMU[which])


# ---- the case the form is for -------------------------------------------------------------------------------------------
COLD_NMU, COLD_Q = 8, 0.3


def cold_table(gamma, q=0.0, n_mu=COLD_NMU):
    """the T = 0.1 Juettner shape at the given nodes, constant in mu for q = 0; else plus q (gamma - 1) mu"""
    mu = np.linspace(-1.0, 1.0, n_mu)[None, :]
    return tab_bind.log_n_juettner(gamma, tg.COLD_T)[:, None] + q * (gamma[:, None] - 1.0) * mu
