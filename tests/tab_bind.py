"""ctypes binding of the table oracle (tests/support/liboracle_tab.so: the CPU oracle's calculators on top of the host
build of the tabulated distribution's device functions) and the tables the tests share.  Test infrastructure only."""
import ctypes
import os
from ctypes import POINTER, c_double, c_int, c_size_t, c_uint32, c_uint64

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    path = os.path.join(ROOT, "tests", "support", "liboracle_tab.so")
    if not os.path.exists(path):
        from rimphony_amd import _build
        _build.build_tab_oracle()
    L = ctypes.CDLL(path)
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
    _lib = L
    return L


def _dp(a):
    return a.ctypes.data_as(POINTER(c_double))


def set_tables(gamma_lo, gamma_hi, log_n):
    """0, or -1 where rimphony_ctx_set_tables answers RIMPHONY_EINVAL"""
    log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
    return load().tabo_set_tables(log_n.shape[0], log_n.shape[1], float(gamma_lo), float(gamma_hi), _dp(log_n))


def blob():
    L = load()
    out = np.zeros(L.tabo_get_blob(None, 0))
    L.tabo_get_blob(_dp(out), len(out))
    return out


def batch(s, theta, index, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the table set last given to set_tables()"""
    s = np.ascontiguousarray(s, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    index = np.ascontiguousarray(index, dtype=np.float64)
    n = len(s)
    out = np.zeros((n, 8))
    work = np.zeros((n, 8), dtype=np.uint64)
    rc = load().tabo_batch(n, _dp(s), _dp(theta), _dp(index), mask, _dp(out), work.ctypes.data_as(POINTER(c_uint64)), nthreads)
    assert rc == 0
    return out, work


def batch_norm(index):
    index = np.ascontiguousarray(index, dtype=np.float64)
    out = np.zeros(len(index))
    assert load().tabo_batch_norm(len(index), _dp(index), _dp(out)) == 0
    return out


def dev_calc_f(kind, par, norm, gamma, cos_xi=None):
    """(f, dfdg, dfdcx) of the host build of calc_f<kind> / calc_f_derivatives<kind>, kind 0 or 4"""
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    cos_xi = np.zeros_like(gamma) if cos_xi is None else np.ascontiguousarray(cos_xi, dtype=np.float64)
    par = np.ascontiguousarray(par, dtype=np.float64)
    f, a, b = np.zeros_like(gamma), np.zeros_like(gamma), np.zeros_like(gamma)
    assert load().tabo_dev_calc_f(kind, _dp(par), float(norm), len(gamma), _dp(gamma), _dp(cos_xi), _dp(f), _dp(a), _dp(b)) == 0
    return f, a, b


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
