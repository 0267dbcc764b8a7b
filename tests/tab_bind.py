"""ctypes binding of the table oracle (tests/support/liboracle_tab.so: the CPU oracle's calculators on top of the host
build of the tabulated distribution's device functions) and the tables the tests share.  Test infrastructure only."""
import ctypes
import os
from ctypes import POINTER, c_double, c_int, c_size_t, c_uint32, c_uint64

import numpy as np

from oracle_bind import Counters, Dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def _dp(a):
    return a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_set_tables.restype = c_int
    L.tabo_set_tables.argtypes = [c_size_t, c_size_t, c_double, c_double, dp]
    L.tabo_get_blob.restype = c_size_t
    L.tabo_get_blob.argtypes = [dp, c_size_t]
    L.tabo_batch.restype = c_int
    L.tabo_batch.argtypes = [c_size_t, dp, dp, dp, c_uint32, dp, POINTER(c_uint64), c_int]
    L.tabo_batch_norm.restype = c_int
    L.tabo_batch_norm.argtypes = [c_size_t, dp, dp]
    L.tabo_dev_calc_f.restype = c_int
    L.tabo_dev_calc_f.argtypes = [c_int, dp, c_double, c_size_t, dp, dp, dp, dp, dp]
    # the calculators' seams (oracle/rimo.h), reached with a kind-4 rimo_dist: mkdist()
    L.rimo_dist_init.restype = c_int
    L.rimo_dist_init.argtypes = [POINTER(Dist), c_int, dp]
    L.rimo_gamma_integrand.restype = c_double
    L.rimo_gamma_integrand.argtypes = [POINTER(Dist), c_int, c_int, c_double, c_double, c_double, c_double]
    L.rimo_gamma_integral.restype = c_double
    L.rimo_gamma_integral.argtypes = [POINTER(Dist), c_int, c_int, c_int, c_double, c_double, c_double]
    L.rimo_n_integral.restype = c_int
    L.rimo_n_integral.argtypes = [POINTER(Dist), c_int, c_int, c_int, c_double, c_double, c_double, c_double, dp]
    L.rimo_symphony_deriv_probe.restype = c_double
    L.rimo_symphony_deriv_probe.argtypes = [POINTER(Dist), c_int, c_int, c_int, c_double, c_double, c_double]
    L.rimo_gamma_contribution.restype = c_double
    L.rimo_gamma_contribution.argtypes = [POINTER(Dist), c_int, c_int, c_double, c_double, c_double]
    L.rimo_hey_element.restype = c_double
    L.rimo_hey_element.argtypes = [POINTER(Dist), c_int, c_double, c_double, c_int, c_double, c_double]
    L.rimo_hey_outer_integrand.restype = c_double
    L.rimo_hey_outer_integrand.argtypes = [POINTER(Dist), c_int, c_double, c_double, c_int, c_double]
    return L


class TabLib:
    """One loaded table oracle.  The tests use the tree's own through the module-level functions below; a test of the
    tests binds a privately built one (a mutated copy) with TabLib(path)."""

    def __init__(self, path):
        self.L = _declare(ctypes.CDLL(path))

    def set_tables(self, gamma_lo, gamma_hi, log_n):
        log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
        return self.L.tabo_set_tables(log_n.shape[0], log_n.shape[1], float(gamma_lo), float(gamma_hi), _dp(log_n))

    def blob(self):
        out = np.zeros(self.L.tabo_get_blob(None, 0))
        self.L.tabo_get_blob(_dp(out), len(out))
        return out

    def batch(self, s, theta, index, mask=0xFF, nthreads=8):
        s = np.ascontiguousarray(s, dtype=np.float64)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        index = np.ascontiguousarray(index, dtype=np.float64)
        n = len(s)
        out = np.zeros((n, 8))
        work = np.zeros((n, 8), dtype=np.uint64)
        rc = self.L.tabo_batch(n, _dp(s), _dp(theta), _dp(index), mask, _dp(out), work.ctypes.data_as(POINTER(c_uint64)), nthreads)
        assert rc == 0
        return out, work

    def batch_norm(self, index):
        index = np.ascontiguousarray(index, dtype=np.float64)
        out = np.zeros(len(index))
        assert self.L.tabo_batch_norm(len(index), _dp(index), _dp(out)) == 0
        return out

    def dev_calc_f(self, kind, par, norm, gamma, cos_xi=None):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        cos_xi = np.zeros_like(gamma) if cos_xi is None else np.ascontiguousarray(cos_xi, dtype=np.float64)
        par = np.ascontiguousarray(par, dtype=np.float64)
        f, a, b = np.zeros_like(gamma), np.zeros_like(gamma), np.zeros_like(gamma)
        assert self.L.tabo_dev_calc_f(kind, _dp(par), float(norm), len(gamma), _dp(gamma), _dp(cos_xi), _dp(f), _dp(a), _dp(b)) == 0
        return f, a, b

    def mkdist(self, index):
        d = Dist()
        st = self.L.rimo_dist_init(ctypes.byref(d), 4, (c_double * 1)(float(index)))
        return d, st


def load():
    """The tree's table oracle, rebuilt first whenever one of its sources is newer (_build.build_tab_oracle checks the
    dependencies itself): a host test never runs against the library of an earlier state of the sources."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = TabLib(_build.build_tab_oracle())
    return _lib.L


def _tab():
    load()
    return _lib


def set_tables(gamma_lo, gamma_hi, log_n):
    """0, or -1 where rimphony_ctx_set_tables answers RIMPHONY_EINVAL"""
    return _tab().set_tables(gamma_lo, gamma_hi, log_n)


def blob():
    return _tab().blob()


def batch(s, theta, index, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the table set last given to set_tables()"""
    return _tab().batch(s, theta, index, mask, nthreads)


def batch_norm(index):
    return _tab().batch_norm(index)


def dev_calc_f(kind, par, norm, gamma, cos_xi=None):
    """(f, dfdg, dfdcx) of the host build of calc_f<kind> / calc_f_derivatives<kind>, kind 0 or 4"""
    return _tab().dev_calc_f(kind, par, norm, gamma, cos_xi)


def mkdist(index):
    """(Dist, status) of table `index` of the set last given to set_tables(): what the seam functions of load() take.
    The Dist only names the table; the set itself stays inside the library."""
    return _tab().mkdist(index)


def n_integral(dist, coeff, stokes, negative_lobe, s, theta, n_lo, n_hi):
    """rimo_n_integral: the value, or NaN when the QAG reports an error (as oracle_bind.n_integral)"""
    v = c_double()
    rc = load().rimo_n_integral(ctypes.byref(dist), coeff, stokes, negative_lobe, s, theta, n_lo, n_hi, ctypes.byref(v))
    return v.value if rc == 0 else float("nan")


# ---- the tables the tests and the fixture share ----------------------------------------------------------------------
def nodes(gamma_lo, gamma_hi, n_nodes):
    """gamma at the nodes: uniform in ln gamma"""
    return np.exp(np.linspace(np.log(gamma_lo), np.log(gamma_hi), n_nodes))


def log_n_powerlaw(gamma, p, gamma_cutoff=np.inf):
    return -p * np.log(gamma) - gamma / gamma_cutoff


def log_n_juettner(gamma, temperature):
    """n = gamma^2 beta exp(-gamma / T): the thermal distribution's f = norm exp(-gamma / T) in the n convention"""
    return np.log(gamma * np.sqrt(gamma * gamma - 1.)) - gamma / temperature


def log_n_rolled_powerlaw(gamma, p=2.5, g1=30., g2=500.):
    """gamma^-p with exponential roll-offs at both ends: negligible at the ends of a table over [1.01, 1e4]"""
    return -p * np.log(gamma) - g1 / gamma - gamma / g2


def edge_tables(gamma_lo, gamma_hi, n_nodes):
    """The three-table set of the edge tests, CPU and GPU: a rolled power law (2.5, 30, 500), a T = 10 Juettner shape, a
    rolled power law (3.5, 10, 200)"""
    g = nodes(gamma_lo, gamma_hi, n_nodes)
    return np.stack([log_n_rolled_powerlaw(g, 2.5, 30., 500.), log_n_juettner(g, 10.), log_n_rolled_powerlaw(g, 3.5, 10., 200.)])


WIGGLE_LO, WIGGLE_HI, WIGGLE_NODES = 1.0, 1e6, 9


def wiggle_table():
    """9 nodes of y = -2.2 u + sin 3u over [1, 1e6]: one and a half nodes per radian, so the spline between the nodes is
    far from the function and only a spline through the same nodes reproduces it"""
    u = np.linspace(np.log(WIGGLE_LO), np.log(WIGGLE_HI), WIGGLE_NODES)
    return -2.2 * u + np.sin(3. * u)
