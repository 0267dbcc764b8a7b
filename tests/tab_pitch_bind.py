"""ctypes binding of the pitch-table oracle (tests/support/liboracle_tabpitch.so: the CPU oracle's calculators on top of
the host build of the tabulated distribution's device functions, table sets with a pitch-angle factor g(cos xi)) and of
the analytic beam oracle (liboracle_beam.so), with the pitch rows the tests and the fixture share.  Test infrastructure
only."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_size_t, c_uint32, c_uint64

import numpy as np

import tab_bind
from oracle_bind import Dist

_lib = None
_beam = None


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    """the entries of liboracle_tabpitch.so: tab_bind's, with tabo_set_tables_pitch in the place of tabo_set_tables"""
    dp = POINTER(c_double)
    L.tabo_set_tables_pitch.restype = c_int
    L.tabo_set_tables_pitch.argtypes = [c_size_t, c_size_t, c_double, c_double, dp, c_size_t, dp]
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


class TabPitchLib(tab_bind.TabLib):
    """tab_bind.TabLib on the pitch oracle: set_tables(..., log_g) replaces the isotropic one, which this library does not
    have; blob, batch, batch_norm, dev_calc_f and mkdist are inherited."""

    def __init__(self, path):
        self.L = _declare(ctypes.CDLL(path))

    def set_tables(self, gamma_lo, gamma_hi, log_n, log_g=None, n_mu=None):
        """0, or -1 where rimphony_ctx_set_tables_pitch answers RIMPHONY_EINVAL.  n_mu: what the call states (default: the
        row length of log_g, 0 without one) -- the misuse tests give one that contradicts log_g."""
        log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
        if log_g is not None:
            log_g = np.ascontiguousarray(np.atleast_2d(log_g), dtype=np.float64)
        if n_mu is None:
            n_mu = 0 if log_g is None else log_g.shape[1]
        return self.L.tabo_set_tables_pitch(log_n.shape[0], log_n.shape[1], float(gamma_lo), float(gamma_hi), _dp(log_n),
                                            int(n_mu), _dp(log_g))


def _tab():
    """The tree's pitch oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = TabPitchLib(_build.build_tab_pitch_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma_lo, gamma_hi, log_n, log_g=None, n_mu=None):
    return _tab().set_tables(gamma_lo, gamma_hi, log_n, log_g, n_mu)


def blob():
    return _tab().blob()


def batch(s, theta, index, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the table set last given to set_tables()"""
    return _tab().batch(s, theta, index, mask, nthreads)


def batch_norm(index):
    return _tab().batch_norm(index)


def dev_calc_f(par, norm, gamma, cos_xi):
    """(f, dfdg, dfdcx) of the host build of calc_f<4> / calc_f_derivatives<4> for table par[0]"""
    return _tab().dev_calc_f(4, par, norm, gamma, cos_xi)


def mkdist(index):
    return _tab().mkdist(index)


# ---- layout of the laid-out set (dev_symphony.h: TAB_HDR_*, TAB_PITCH_*) ---------------------------------------------
HDR, HDR_NMU, PITCH_HDR, PITCH_P = 8, 7, 4, 3


def pitch_row(blob_, table):
    """(header [4] = {n_mu - 2, 1 / h, h, P}, G [n_mu], M [n_mu]) of one table's pitch row"""
    nt, nn, nmu = int(blob_[0]), int(blob_[1]), int(blob_[HDR_NMU])
    base = HDR + 2 * nt * nn + table * (PITCH_HDR + 2 * nmu)
    row = blob_[base + PITCH_HDR:base + PITCH_HDR + 2 * nmu]
    return blob_[base:base + PITCH_HDR], row[0::2], row[1::2]


# ---- the analytic beam oracle ---------------------------------------------------------------------------------------------
class BeamLib:
    def __init__(self, path):
        L = ctypes.CDLL(path)
        dp = POINTER(c_double)
        L.beamo_pitch_integral.restype = c_double
        L.beamo_pitch_integral.argtypes = [c_double, c_double]
        L.beamo_batch.restype = c_int
        L.beamo_batch.argtypes = [c_size_t, dp, dp, dp, c_uint32, dp, c_int]
        L.beamo_norm.restype = c_double
        L.beamo_norm.argtypes = [dp]
        L.beamo_calc_f.restype = None
        L.beamo_calc_f.argtypes = [dp, c_double, c_size_t, dp, dp, dp, dp, dp]
        self.L = L


def beam():
    global _beam
    if _beam is None:
        from rimphony_amd import _build
        _beam = BeamLib(_build.build_beam_oracle())
    return _beam.L


def beam_batch(s, theta, par, mask=0xFF, nthreads=8):
    """out [n][8] of the analytic beam; par = {p, gamma_min, gamma_max, gamma_cutoff, a, b}, one row or one per point"""
    s = np.ascontiguousarray(s, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    par = np.ascontiguousarray(np.broadcast_to(np.asarray(par, dtype=np.float64), (len(s), 6)))
    out = np.zeros((len(s), 8))
    assert beam().beamo_batch(len(s), _dp(s), _dp(theta), _dp(par), mask, _dp(out), nthreads) == 0
    return out


def beam_norm(par):
    return beam().beamo_norm(_dp(np.ascontiguousarray(par, dtype=np.float64)))


def beam_calc_f(par, norm, gamma, cos_xi):
    gamma = np.ascontiguousarray(gamma, dtype=np.float64)
    cos_xi = np.ascontiguousarray(cos_xi, dtype=np.float64)
    f, a, b = np.zeros_like(gamma), np.zeros_like(gamma), np.zeros_like(gamma)
    beam().beamo_calc_f(_dp(np.ascontiguousarray(par, dtype=np.float64)), float(norm), len(gamma), _dp(gamma), _dp(cos_xi),
                        _dp(f), _dp(a), _dp(b))
    return f, a, b


# ---- the pitch rows the tests and the fixture share ---------------------------------------------------------------------
def mu_nodes(n_mu):
    return np.linspace(-1.0, 1.0, n_mu)


def log_g_beam(n_mu, a, b=0.0):
    """G = a mu - b mu^2 at the nodes"""
    mu = mu_nodes(n_mu)
    return a * mu - b * mu * mu


def edge_pitch(n_mu):
    """The pitch rows of tab_bind.edge_tables' three tables: G = 1.0 mu, G = 0, G = 0.8 mu - 1.5 mu^2"""
    return np.stack([log_g_beam(n_mu, 1.0), np.zeros(n_mu), log_g_beam(n_mu, 0.8, 1.5)])
