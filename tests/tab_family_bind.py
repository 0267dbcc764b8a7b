"""ctypes binding of the table oracle for FAMILIES of energy tables, a real index per row (tests/support/liboracle_tabfamily.so:
the CPU oracle's calculators on top of the host build of the family's device functions and of rim_tab_check_family /
rim_tab_build_family), with the sets the tests and the fixture share.  Test infrastructure only."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_size_t, c_uint32, c_uint64

import numpy as np

import tab_bind
from oracle_bind import Dist

_lib = None


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_set_tables_family.restype = c_int
    L.tabo_set_tables_family.argtypes = [c_size_t, c_size_t, c_double, c_double, dp, dp]
    L.tabo_row_line.restype = c_int
    L.tabo_row_line.argtypes = [c_double, dp, dp, dp]
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
    L.rimo_hey_element.restype = c_double
    L.rimo_hey_element.argtypes = [POINTER(Dist), c_int, c_double, c_double, c_int, c_double, c_double]
    L.rimo_hey_outer_integrand.restype = c_double
    L.rimo_hey_outer_integrand.argtypes = [POINTER(Dist), c_int, c_double, c_double, c_int, c_double]
    return L


class TabFamilyLib(tab_bind.TabLib):
    """tab_bind.TabLib on the family oracle: set_tables(gamma_lo, gamma_hi, log_n, sin_k); blob, batch, batch_norm,
    dev_calc_f and mkdist are inherited, `index` being the real index x of a row."""

    def __init__(self, path):
        self.L = _declare(ctypes.CDLL(path))

    def set_tables(self, gamma_lo, gamma_hi, log_n, sin_k=None):
        """0, or -1 where rimphony_ctx_set_tables_family answers RIMPHONY_EINVAL.  sin_k is passed as it is."""
        log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
        if sin_k is not None:
            sin_k = np.ascontiguousarray(np.atleast_1d(sin_k), dtype=np.float64)
            assert len(sin_k) == log_n.shape[0]
        return self.L.tabo_set_tables_family(log_n.shape[0], log_n.shape[1], float(gamma_lo), float(gamma_hi), _dp(log_n), _dp(sin_k))


def _tab():
    """The tree's family oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = TabFamilyLib(_build.build_tab_family_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma_lo, gamma_hi, log_n, sin_k=None):
    return _tab().set_tables(gamma_lo, gamma_hi, log_n, sin_k)


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
    """(k, w, P) of the line of a row at x (a family with a prefactor)"""
    k, w, p = c_double(), c_double(), c_double()
    assert load().tabo_row_line(float(x), ctypes.byref(k), ctypes.byref(w), ctypes.byref(p)) == 0
    return k.value, w.value, p.value


# ---- the sets the tests and the fixture share ------------------------------------------------------------------------
# A: the three edge tables of tab_bind on 64 nodes, isotropic -- an interior table, a clamped last table.
# B: two rolled power laws on 8 nodes, the minimum row length, with sin_k.
EDGE_LO, EDGE_HI = 1.01, 1e4
SET_A_NODES, SET_B_NODES = 64, 8
SET_B_K = (0.5, 2.0)


def fixture_set(which):
    """(gamma_lo, gamma_hi, log_n, sin_k) of set A (0) or B (1)"""
    if which == 0:
        return EDGE_LO, EDGE_HI, tab_bind.edge_tables(EDGE_LO, EDGE_HI, SET_A_NODES), None
    g = tab_bind.nodes(EDGE_LO, EDGE_HI, SET_B_NODES)
    t = np.stack([tab_bind.log_n_rolled_powerlaw(g, 2.5, 30., 500.), tab_bind.log_n_rolled_powerlaw(g, 3.5, 10., 200.)])
    return EDGE_LO, EDGE_HI, t, np.array(SET_B_K)


def fixture_x(which):
    """the real indices the fixture rows draw from: {0, 0.25, 1, 1.5, 2 - 2^-52, last, one beyond last, NaN}; in set B, of two
    tables, 1.5 and 2 - 2^-52 lie beyond the last table as well"""
    last = 2.0 if which == 0 else 1.0
    return np.array([0.0, 0.25, 1.0, 1.5, 2.0 - 2.0 ** -52, last, np.nextafter(last, np.inf), np.nan])


# the two-table power-law family of the accuracy tests: gamma^-p exp(-gamma / 1e10), p = 2 and 3.5, 2048 nodes over [1, 1e12]
PL_LO, PL_HI, PL_NODES, PL_CUT = 1.0, 1e12, 2048, 1e10
PL_P = (2.0, 3.5)
PL_K = (0.0, 3.0)
PL_X = (0.0, 0.25, 0.5, 0.9, 1.0)


def powerlaw_family():
    g = tab_bind.nodes(PL_LO, PL_HI, PL_NODES)
    return np.stack([tab_bind.log_n_powerlaw(g, p, PL_CUT) for p in PL_P])


def read_accuracy():
    """the figures of profiles/tabulated_family_accuracy.txt as {name: value}"""
    import os
    import re
    path = os.path.join(tab_bind.ROOT, "profiles", "tabulated_family_accuracy.txt")
    out = {}
    for line in open(path):
        m = re.match(r"^  (\w+) = (\S+)$", line.rstrip("\n"))
        if m:
            out[m.group(1)] = float(m.group(2))
    return out
