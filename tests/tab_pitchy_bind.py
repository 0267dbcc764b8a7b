"""ctypes binding of the table oracle for sets with a sin^k xi prefactor (tests/support/liboracle_tabpitchy.so: the CPU
oracle's calculators on top of the host build of the tabulated distribution's device functions and of
rim_tab_check_pitchy / rim_tab_build_pitchy) and of the analytic sin^k beam oracle (liboracle_pitchy_beam.so), with the
two table sets the tests and the fixture share.  Test infrastructure only."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_size_t, c_uint32, c_uint64

import numpy as np

import tab_bind
import tab_pitch_bind as tp
from oracle_bind import Dist

_lib = None
_beam = None


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_set_tables_pitchy.restype = c_int
    L.tabo_set_tables_pitchy.argtypes = [c_size_t, c_size_t, c_double, c_double, dp, c_size_t, dp, dp]
    L.tabo_p_intervals.restype = c_int
    L.tabo_p_intervals.argtypes = []
    L.tabo_table_k_p.restype = c_int
    L.tabo_table_k_p.argtypes = [c_double, dp, dp]
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


class TabPitchyLib(tab_bind.TabLib):
    """tab_bind.TabLib on the sin^k oracle: set_tables(..., log_g, sin_k); blob, batch, batch_norm, dev_calc_f and mkdist
    are inherited."""

    def __init__(self, path):
        self.L = _declare(ctypes.CDLL(path))

    def set_tables(self, gamma_lo, gamma_hi, log_n, log_g=None, sin_k=None, n_mu=None):
        """0, or -1 where rimphony_ctx_set_tables_pitchy answers RIMPHONY_EINVAL.  sin_k is passed as it is (its length is
        the caller's matter, as in C); n_mu: what the call states (default: the row length of log_g, 0 without one)."""
        log_n = np.ascontiguousarray(np.atleast_2d(log_n), dtype=np.float64)
        if log_g is not None:
            log_g = np.ascontiguousarray(np.atleast_2d(log_g), dtype=np.float64)
        if n_mu is None:
            n_mu = 0 if log_g is None else log_g.shape[1]
        if sin_k is not None:
            sin_k = np.ascontiguousarray(np.atleast_1d(sin_k), dtype=np.float64)
            assert len(sin_k) == log_n.shape[0]
        return self.L.tabo_set_tables_pitchy(log_n.shape[0], log_n.shape[1], float(gamma_lo), float(gamma_hi), _dp(log_n),
                                             int(n_mu), _dp(log_g), _dp(sin_k))


def _tab():
    """The tree's sin^k oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = TabPitchyLib(_build.build_tab_pitchy_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma_lo, gamma_hi, log_n, log_g=None, sin_k=None, n_mu=None):
    return _tab().set_tables(gamma_lo, gamma_hi, log_n, log_g, sin_k, n_mu)


def blob():
    return _tab().blob()


def batch(s, theta, index, mask=0xFF, nthreads=8):
    """(out [n][8], work [n][8]) of the table set last given to set_tables()"""
    return _tab().batch(s, theta, index, mask, nthreads)


def batch_norm(index):
    return _tab().batch_norm(index)


def dev_calc_f(par, norm, gamma, cos_xi):
    """(f, dfdg, dfdcx) of the host build of calc_f<7> / calc_f_derivatives<7> for table par[0]"""
    return _tab().dev_calc_f(4, par, norm, gamma, cos_xi)


def mkdist(index):
    return _tab().mkdist(index)


def table_k_p(index):
    """(k, P) of the table's header"""
    k, p = c_double(), c_double()
    assert load().tabo_table_k_p(float(index), ctypes.byref(k), ctypes.byref(p)) == 0
    return k.value, p.value


def p_intervals():
    return load().tabo_p_intervals()


def n_integral(dist, coeff, stokes, negative_lobe, s, theta, n_lo, n_hi):
    """rimo_n_integral: the value, or NaN when the QAG reports an error (as tab_bind.n_integral)"""
    v = c_double()
    rc = load().rimo_n_integral(ctypes.byref(dist), coeff, stokes, negative_lobe, s, theta, n_lo, n_hi, ctypes.byref(v))
    return v.value if rc == 0 else float("nan")


# ---- the analytic sin^k beam oracle ----------------------------------------------------------------------------------
def beam():
    global _beam
    if _beam is None:
        from rimphony_amd import _build
        L = ctypes.CDLL(_build.build_pitchy_beam_oracle())
        dp = POINTER(c_double)
        L.pbeamo_pitch_integral.restype = c_double
        L.pbeamo_pitch_integral.argtypes = [c_double, c_double]
        L.pbeamo_batch.restype = c_int
        L.pbeamo_batch.argtypes = [c_size_t, dp, dp, dp, c_uint32, dp, c_int]
        L.pbeamo_norm.restype = c_double
        L.pbeamo_norm.argtypes = [dp]
        _beam = L
    return _beam


def beam_batch(s, theta, par, mask=0xFF, nthreads=8):
    """out [n][8] of the analytic sin^k beam; par = {p, gamma_min, gamma_max, gamma_cutoff, a, k}"""
    s = np.ascontiguousarray(s, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    par = np.ascontiguousarray(np.broadcast_to(np.asarray(par, dtype=np.float64), (len(s), 6)))
    out = np.zeros((len(s), 8))
    assert beam().pbeamo_batch(len(s), _dp(s), _dp(theta), _dp(par), mask, _dp(out), nthreads) == 0
    return out


# ---- the two sets the tests and the fixture share --------------------------------------------------------------------
EDGE_LO, EDGE_HI, EDGE_NODES, SET_B_NMU = 1.01, 1e4, 64, 8
SET_A_K = (0.5, 2.0, 0.0)
SET_B_K = (1.5, 0.3, 3.0)


def wavy_row(n_mu):
    """a row that is neither a line nor a parabola (test_tabulated_pitch_host.py's)"""
    mu = tp.mu_nodes(n_mu)
    return 0.8 * mu - 1.5 * mu * mu + 0.4 * np.sin(3.0 * mu)


def set_b_rows(n_mu=SET_B_NMU):
    return np.stack([tp.log_g_beam(n_mu, 0.8, 1.5), tp.log_g_beam(n_mu, 1.0), wavy_row(n_mu)])


def fixture_set(which):
    """(gamma_lo, gamma_hi, log_n, log_g, sin_k) of set A (0: no g) or B (1: pitch rows of 8 nodes)"""
    t = tab_bind.edge_tables(EDGE_LO, EDGE_HI, EDGE_NODES)
    if which == 0:
        return EDGE_LO, EDGE_HI, t, None, np.array(SET_A_K)
    return EDGE_LO, EDGE_HI, t, set_b_rows(), np.array(SET_B_K)


# ---- recorded figures two test files share ---------------------------------------------------------------------------
# max over the 16 pl_rows of tests/golden/tabulated_det.npz and 8 slots of |table / analytic - 1|: the 2048-node table of
# gamma^-2.5 exp(-gamma / 1e10) over [1, 1e12] times sin^k xi against the analytic pitchy power law (kind 2), measured on
# the CPU oracles (test_tabulated_pitchy_host.py); the GPU carries both oracles' bits, so its figure is the same one.
MEASURED_KIND2 = {0.5: 2.8e-13, 1.0: 7.0e-13, 2.5: 2.7e-13}
