"""ctypes binding of the table oracle for 2-D sets with a sin^k xi prefactor, on nodes uniform in ln gamma or given
(tests/support/liboracle_tab2dpitchy.so: the CPU oracle's calculators on top of the host build of the tabulated distribution's
device functions and of rim_tab_check_2d_pitchy / rim_tab_build_2d_pitchy and their _grid_ counterparts), of the analytic
tilted power law with sin^k (liboracle_pitchy_tilt.so), and the table sets the tests and the fixture share.  Test
infrastructure only."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_size_t, c_uint32

import numpy as np

import tab_bind
import tab2d_bind as t2
import tab_grid_bind as tg

_lib = None
_ptilt = None
KIND_UNIFORM, KIND_GRID = 10, 11


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_check_2d_pitchy.restype = c_int
    L.tabo_check_2d_pitchy.argtypes = [c_size_t, c_size_t, c_double, c_double, c_size_t, dp, dp]
    L.tabo_check_2d_grid_pitchy.restype = c_int
    L.tabo_check_2d_grid_pitchy.argtypes = [c_size_t, c_size_t, dp, c_size_t, dp, dp]
    L.tabo_set_tables_2d_pitchy.restype = c_int
    L.tabo_set_tables_2d_pitchy.argtypes = [c_size_t, c_size_t, c_double, c_double, c_size_t, dp, dp, c_int]
    L.tabo_set_tables_2d_grid_pitchy.restype = c_int
    L.tabo_set_tables_2d_grid_pitchy.argtypes = [c_size_t, c_size_t, dp, c_size_t, dp, dp, c_int]
    L.tabo_put_norms.restype = c_int
    L.tabo_put_norms.argtypes = [c_size_t, dp]
    L.tabo_form.restype = c_int
    L.tabo_form.argtypes = []
    L.tabo_bicubic.restype = c_int
    L.tabo_bicubic.argtypes = [c_double, c_size_t, dp, dp, dp, dp, dp]
    L.tabo_nbar.restype = c_int
    L.tabo_nbar.argtypes = [c_double, c_size_t, dp, dp]
    return L


def _args(log_n, sin_k, shape):
    """(n_tables, n_nodes, n_mu, log_n, sin_k) as the C entries take them; shape: what the call states (default: log_n's own)"""
    if log_n is not None:
        log_n = t2.as_set(log_n) if shape is None else np.ascontiguousarray(log_n, dtype=np.float64)
    nt, nn, nmu = log_n.shape if shape is None else shape
    if sin_k is not None:
        sin_k = np.ascontiguousarray(np.broadcast_to(np.asarray(sin_k, dtype=np.float64), (int(nt),)))
    return int(nt), int(nn), int(nmu), log_n, sin_k


class Tab2DPitchyLib(tab_bind.TabLib):
    """tab_bind.TabLib on this oracle.  set_tables(where, log_n, sin_k): `where` is (gamma_lo, gamma_hi) for the form on nodes
    uniform in ln gamma, or the array of gamma nodes for the form on given nodes; blob, batch, batch_norm, dev_calc_f and
    mkdist are inherited.  A test of the tests binds a privately built copy with Tab2DPitchyLib(path)."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.tabo_set_tables = L.tabo_set_tables_2d_pitchy      # (tab_bind declares the name; _declare declares the entry again)
        self.L = _declare(tab_bind._declare(L))

    @staticmethod
    def is_range(where):
        return isinstance(where, tuple) and len(where) == 2

    def set_tables(self, where, log_n, sin_k, shape=None, with_norm=True):
        """0, or -1 where the C entry answers RIMPHONY_EINVAL"""
        nt, nn, nmu, log_n, sin_k = _args(log_n, sin_k, shape)
        if self.is_range(where):
            return self.L.tabo_set_tables_2d_pitchy(nt, nn, float(where[0]), float(where[1]), nmu, _dp(log_n), _dp(sin_k), int(with_norm))
        gamma = None if where is None else np.ascontiguousarray(where, dtype=np.float64)
        return self.L.tabo_set_tables_2d_grid_pitchy(nt, nn, _dp(gamma), nmu, _dp(log_n), _dp(sin_k), int(with_norm))

    def check(self, where, log_n, sin_k, shape=None):
        nt, nn, nmu, log_n, sin_k = _args(log_n, sin_k, shape)
        if self.is_range(where):
            return self.L.tabo_check_2d_pitchy(nt, nn, float(where[0]), float(where[1]), nmu, _dp(log_n), _dp(sin_k))
        gamma = None if where is None else np.ascontiguousarray(where, dtype=np.float64)
        return self.L.tabo_check_2d_grid_pitchy(nt, nn, _dp(gamma), nmu, _dp(log_n), _dp(sin_k))

    def put_norms(self, norms):
        norms = np.ascontiguousarray(norms, dtype=np.float64)
        return self.L.tabo_put_norms(len(norms), _dp(norms))

    def bicubic(self, index, gamma, mu):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        s, su, sm = np.zeros_like(gamma), np.zeros_like(gamma), np.zeros_like(gamma)
        assert self.L.tabo_bicubic(float(index), len(gamma), _dp(gamma), _dp(mu), _dp(s), _dp(su), _dp(sm)) == 0
        return s, su, sm

    def nbar(self, index, gamma):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        out = np.zeros_like(gamma)
        assert self.L.tabo_nbar(float(index), len(gamma), _dp(gamma), _dp(out)) == 0
        return out


def _tab():
    """The tree's oracle, rebuilt first whenever one of its sources is newer."""
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        _lib = Tab2DPitchyLib(_build.build_tab2d_pitchy_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(where, log_n, sin_k, shape=None, with_norm=True):
    return _tab().set_tables(where, log_n, sin_k, shape, with_norm)


def check(where, log_n, sin_k, shape=None):
    return _tab().check(where, log_n, sin_k, shape)


def put_norms(norms):
    """the tables' normalisations from a record (the fixture's) into a set installed with_norm=False"""
    return _tab().put_norms(norms)


def blob():
    return _tab().blob()


def form():
    """the form of the installed set: KIND_UNIFORM or KIND_GRID"""
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


def nbar(index, gamma):
    """nbar(gamma) of table `index` as the normalisation integrates it (tab_2d_norm_integrand)"""
    return _tab().nbar(index, gamma)


def mkdist(index):
    return _tab().mkdist(index)


# ---- the analytic tilted power law with sin^k ------------------------------------------------------------------------------
def ptilt():
    global _ptilt
    if _ptilt is None:
        from rimphony_amd import _build
        L = ctypes.CDLL(_build.build_pitchy_tilt_oracle())
        dp = POINTER(c_double)
        L.ptilto_set_k.restype = None
        L.ptilto_set_k.argtypes = [c_double]
        L.ptilto_batch.restype = c_int
        L.ptilto_batch.argtypes = [c_size_t, dp, dp, dp, c_uint32, dp, c_int]
        L.ptilto_norm.restype = c_double
        L.ptilto_norm.argtypes = [dp]
        _ptilt = L
    return _ptilt


def ptilt_batch(s, theta, par, k, mask=0xFF, nthreads=8):
    """out [n][8] of the analytic distribution; par = {p, gamma_min, gamma_max, gamma_cutoff, a, q}, k the exponent"""
    s = np.ascontiguousarray(s, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    par = np.ascontiguousarray(par, dtype=np.float64)
    assert par.shape == (6,)
    out = np.zeros((len(s), 8))
    ptilt().ptilto_set_k(float(k))
    assert ptilt().ptilto_batch(len(s), _dp(s), _dp(theta), _dp(par), mask, _dp(out), nthreads) == 0
    return out


# ---- the tables the tests and the fixture share -------------------------------------------------------------------------
FIXTURE_K = ((0.5, 2.5), (1.0, 0.0))
FIXTURE_SHAPE = ((32, 8), (64, 9))
FIXTURE_RANGE = (1.01, 1e4)


def loss_cone_surfaces(gamma, n_mu):
    """Two smooth remainders at the given gamma nodes, neither separable, both tapered to nothing at both ends of [1.01, 1e4]
    and of the log-gm1 grid: a rolled power law with a tilt that grows with gamma, and a T = 10 Juettner shape with a curved
    anisotropy that grows with gamma -- what is left of a loss cone that deepens with energy once sin^k xi is divided out."""
    gamma = np.asarray(gamma, dtype=np.float64)
    u, g = np.log(gamma)[:, None], gamma[:, None]
    mu = np.linspace(-1.0, 1.0, n_mu)[None, :]
    w = (u - u[0]) / (u[-1] - u[0])
    tilted = -t2.TILT_P * u + t2.TILT_Q * u * mu + t2.TILT_A * mu - t2.TILT_G1 / g - g / t2.TILT_G2
    curved = tab_bind.log_n_juettner(gamma, 10.0)[:, None] + (0.6 * mu - 0.9 * mu * mu) * w
    return np.stack([tilted, curved])


def fixture_where(which):
    """set U (0): the range of 32 nodes uniform in ln gamma; set G (1): 64 nodes uniform in ln(gamma - 1)"""
    return FIXTURE_RANGE if which == 0 else tg.grid("log-gm1")


def fixture_set(which):
    """(where, log_n, sin_k) of set U (32 x 8 nodes uniform in ln gamma, k = 0.5, 2.5) or G (64 x 9 given nodes, k = 1, 0)"""
    n_nodes, n_mu = FIXTURE_SHAPE[which]
    where = fixture_where(which)
    if which == 0:
        g = tab_bind.nodes(where[0], where[1], n_nodes)
        g[0], g[-1] = where
    else:
        g = where
        assert len(g) == n_nodes
    return where, loss_cone_surfaces(g, n_mu), np.array(FIXTURE_K[which])
