"""ctypes binding of the table oracle for 2-D sets on gamma nodes and mu nodes of the caller's choosing, with or without a
sin^k xi prefactor (tests/support/liboracle_tab2dnodes.so: the CPU oracle's calculators on top of the host build of the
tabulated distribution's device functions and of rim_tab_check_2d_nodes / rim_tab_build_2d_nodes), and the node sets and
table sets the tests and the fixture share.  Test infrastructure only."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_longlong, c_size_t, c_ulonglong

import numpy as np

import tab_bind
import tab2d_bind as t2
import tab_grid_bind as tg

_lib = None
KIND_PLAIN, KIND_PITCHY = 12, 13


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _declare(L):
    dp = POINTER(c_double)
    L.tabo_check_2d_nodes.restype = c_int
    L.tabo_check_2d_nodes.argtypes = [c_size_t, c_size_t, dp, c_size_t, dp, dp, dp]
    L.tabo_set_tables_2d_nodes.restype = c_int
    L.tabo_set_tables_2d_nodes.argtypes = [c_size_t, c_size_t, dp, c_size_t, dp, dp, dp, c_int]
    L.tabo_put_norms.restype = c_int
    L.tabo_put_norms.argtypes = [c_size_t, dp]
    L.tabo_form.restype = c_int
    L.tabo_form.argtypes = []
    L.tabo_bicubic.restype = c_int
    L.tabo_bicubic.argtypes = [c_double, c_size_t, dp, dp, dp, dp, dp]
    L.tabo_mu_interval.restype = c_int
    L.tabo_mu_interval.argtypes = [c_size_t, dp, POINTER(c_longlong), POINTER(c_ulonglong)]
    L.tabo_nbar.restype = c_int
    L.tabo_nbar.argtypes = [c_double, c_size_t, dp, dp]
    return L


def _args(gamma, mu, log_n, sin_k, shape):
    """(n_tables, n_nodes, n_mu, gamma, mu, log_n, sin_k) as the C entry takes them; shape: what the call states (default:
    log_n's own)"""
    gamma = None if gamma is None else np.ascontiguousarray(gamma, dtype=np.float64)
    mu = None if mu is None else np.ascontiguousarray(mu, dtype=np.float64)
    if log_n is not None:
        log_n = t2.as_set(log_n) if shape is None else np.ascontiguousarray(log_n, dtype=np.float64)
    nt, nn, nmu = log_n.shape if shape is None else shape
    if sin_k is not None:
        sin_k = np.ascontiguousarray(np.broadcast_to(np.asarray(sin_k, dtype=np.float64), (int(nt),)))
    return int(nt), int(nn), int(nmu), gamma, mu, log_n, sin_k


class Tab2DNodesLib(tab_bind.TabLib):
    """tab_bind.TabLib on this oracle: set_tables(gamma, mu, log_n, sin_k[, shape]); blob, batch, batch_norm, dev_calc_f and
    mkdist are inherited.  A test of the tests binds a privately built copy with Tab2DNodesLib(path)."""

    def __init__(self, path):
        L = ctypes.CDLL(path)
        L.tabo_set_tables = L.tabo_set_tables_2d_nodes      # (tab_bind declares the name; _declare declares the entry again)
        self.L = _declare(tab_bind._declare(L))

    def set_tables(self, gamma, mu, log_n, sin_k=None, shape=None, with_norm=True):
        """0, or -1 where rimphony_ctx_set_tables_2d_nodes answers RIMPHONY_EINVAL"""
        nt, nn, nmu, gamma, mu, log_n, sin_k = _args(gamma, mu, log_n, sin_k, shape)
        return self.L.tabo_set_tables_2d_nodes(nt, nn, _dp(gamma), nmu, _dp(mu), _dp(log_n), _dp(sin_k), int(with_norm))

    def check(self, gamma, mu, log_n, sin_k=None, shape=None):
        nt, nn, nmu, gamma, mu, log_n, sin_k = _args(gamma, mu, log_n, sin_k, shape)
        return self.L.tabo_check_2d_nodes(nt, nn, _dp(gamma), nmu, _dp(mu), _dp(log_n), _dp(sin_k))

    def put_norms(self, norms):
        norms = np.ascontiguousarray(norms, dtype=np.float64)
        return self.L.tabo_put_norms(len(norms), _dp(norms))

    def bicubic(self, index, gamma, mu):
        gamma = np.ascontiguousarray(gamma, dtype=np.float64)
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        s, su, sm = np.zeros_like(gamma), np.zeros_like(gamma), np.zeros_like(gamma)
        assert self.L.tabo_bicubic(float(index), len(gamma), _dp(gamma), _dp(mu), _dp(s), _dp(su), _dp(sm)) == 0
        return s, su, sm

    def mu_intervals(self, mu):
        mu = np.ascontiguousarray(mu, dtype=np.float64)
        out, reads = np.zeros(len(mu), dtype=np.int64), np.zeros(len(mu), dtype=np.uint64)
        assert self.L.tabo_mu_interval(len(mu), _dp(mu), out.ctypes.data_as(POINTER(c_longlong)),
                                       reads.ctypes.data_as(POINTER(c_ulonglong))) == 0
        return out, reads

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
        _lib = Tab2DNodesLib(_build.build_tab2d_nodes_oracle())
    return _lib


def load():
    return _tab().L


def set_tables(gamma, mu, log_n, sin_k=None, shape=None, with_norm=True):
    return _tab().set_tables(gamma, mu, log_n, sin_k, shape, with_norm)


def check(gamma, mu, log_n, sin_k=None, shape=None):
    return _tab().check(gamma, mu, log_n, sin_k, shape)


def put_norms(norms):
    """the tables' normalisations from a record (the fixture's) into a set installed with_norm=False"""
    return _tab().put_norms(norms)


def blob():
    return _tab().blob()


def form():
    """the form of the installed set: KIND_PLAIN or KIND_PITCHY"""
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
    """(S, dS/du, dS/dmu) of the host build of tab_bicubic_nodes for table `index`"""
    return _tab().bicubic(index, gamma, mu)


def mu_intervals(mu):
    """(the mu intervals the device function finds, the mu node words each search read)"""
    return _tab().mu_intervals(mu)


def nbar(index, gamma):
    """nbar(gamma) of table `index` as the normalisation integrates it (tab_2d_norm_integrand)"""
    return _tab().nbar(index, gamma)


def mkdist(index):
    return _tab().mkdist(index)


class Blob:
    """The parts of a laid-out set (dev_symphony.h: tab_2d_nodes_*)"""

    def __init__(self, b):
        g = _grid_prefix(b)
        self.__dict__.update(g)
        at = self.mu_guide_at
        self.mu_cells = int(self.headers[0, 2])
        gd = ((self.mu_cells + 2) // 2 + 7) & ~7
        self.mu_guide = b[at:at + gd].view(np.uint32)[:self.mu_cells + 1]
        at += gd
        self.mu_nodes = b[at:at + 2 * self.n_mu].reshape(self.n_mu, 2)
        self.mu = self.mu_nodes[:, 0]
        at += (2 * self.n_mu + 7) & ~7
        per = self.n_nodes * self.n_mu * 4
        self.size = at + self.n_tables * per
        self.nodes = b[at:self.size].reshape(self.n_tables, self.n_nodes, self.n_mu, 4)


def _grid_prefix(b):
    """what a 2-D set on given gamma nodes has in front of its node data, which is where this form's mu guide begins"""
    n_tables, n_nodes, cells, n_mu = int(b[0]), int(b[1]), int(b[6]), int(-b[7])
    at = 8
    headers = b[at:at + 8 * n_tables].reshape(n_tables, 8)
    at += 8 * n_tables
    gd = ((cells + 2) // 2 + 7) & ~7
    guide = b[at:at + gd].view(np.uint32)[:cells + 1]
    at += gd
    unodes = b[at:at + 2 * n_nodes].reshape(n_nodes, 2)
    at += (2 * n_nodes + 7) & ~7
    return dict(n_tables=n_tables, n_nodes=n_nodes, cells=cells, n_mu=n_mu, headers=headers, guide=guide, unodes=unodes,
                u=unodes[:, 0], mu_guide_at=at)


# ---- the mu node sets ------------------------------------------------------------------------------------------------------
def mu_uniform(n):
    """-1 + j 2 / (n - 1): the nodes of the older 2-D forms (numpy.linspace forms them so, ends exact)"""
    return np.linspace(-1.0, 1.0, n)


def mu_uniform_in_xi(n):
    from rimphony_amd.api import mu_nodes_uniform_in_xi
    return mu_nodes_uniform_in_xi(n)


# set P's: 9 nodes, 16 guide cells of 1/8.  The last guide cell holds five of them, eleven guide cells hold none, and the
# last cell before mu = +1 is 5e-5 wide.
MU_P = np.array([-1.0, -0.5, 0.0, 0.5, 0.9, 0.95, 0.98, 0.99995, 1.0])


def mu_jitter(n, seed=20261019):
    """n nodes uniform in mu, each interior one moved by a seeded +-40 % of the spacing"""
    m = np.linspace(-1.0, 1.0, n)
    r = np.random.default_rng(seed + n).uniform(-0.4, 0.4, n)
    r[0] = r[-1] = 0.0
    m = m + r * (m[1] - m[0])
    m[0], m[-1] = -1.0, 1.0
    return m


def mu_crowded(n=1000, n_last=940):
    """n nodes of which n_last lie in the last of the 1024 guide cells, [1 - 2/1024, 1]: the bisection's worst case"""
    head = np.linspace(-1.0, 1.0 - 2.0 / 1024, n - n_last, endpoint=False)
    tail = np.linspace(1.0 - 2.0 / 1024, 1.0, n_last)
    return np.concatenate([head, tail])


def mu_graded_ring(n, mu0, w, frac=0.5, span=8.0):
    """n nodes for a ring at mu0 of width w: frac of them uniform across mu0 +- span w, the others uniform outside it"""
    n_in = int(round(frac * n))
    lo, hi = mu0 - span * w, mu0 + span * w
    n_out = n - n_in
    n_left = max(2, int(round(n_out * (lo + 1.0) / (2.0 - (hi - lo)))))
    n_right = n_out - n_left
    left = np.linspace(-1.0, lo, n_left, endpoint=False)
    mid = np.linspace(lo, hi, n_in, endpoint=False)
    right = np.linspace(hi, 1.0, n_right)
    m = np.concatenate([left, mid, right])
    assert len(m) == n and (np.diff(m) > 0).all()
    return m


# ---- the tables the tests and the fixture share -------------------------------------------------------------------------
FIXTURE_K = (None, (0.5, 2.5))


def surfaces(gamma, mu):
    """Two surfaces at the given gamma and mu nodes, neither separable, both tapered to nothing at both ends of the gamma
    nodes: a rolled power law with a tilt that grows with gamma, and a T = 10 Juettner shape with a curved anisotropy that
    grows with gamma (tab2d_pitchy_bind.loss_cone_surfaces on mu nodes of any kind)."""
    gamma = np.asarray(gamma, dtype=np.float64)
    u, g = np.log(gamma)[:, None], gamma[:, None]
    mu = np.asarray(mu, dtype=np.float64)[None, :]
    w = (u - u[0]) / (u[-1] - u[0])
    tilted = -t2.TILT_P * u + t2.TILT_Q * u * mu + t2.TILT_A * mu - t2.TILT_G1 / g - g / t2.TILT_G2
    curved = tab_bind.log_n_juettner(gamma, 10.0)[:, None] + (0.6 * mu - 0.9 * mu * mu) * w
    return np.stack([tilted, curved])


def fixture_nodes(which):
    """(gamma, mu) of set P (0: 32 gamma uniform in ln(gamma - 1) over gamma - 1 in [1e-6, 1e4], the 9 graded mu of MU_P) or
    set K (1: 24 jittered gamma, 12 mu uniform in xi)"""
    if which == 0:
        return tg.log_gm1_nodes(1e-6, 1e4, 32), MU_P.copy()
    return tg.jitter_nodes(24), mu_uniform_in_xi(12)


def fixture_set(which):
    """(gamma, mu, log_n, sin_k) of set P (plain: sin_k None) or set K (sin_k = 0.5, 2.5)"""
    gamma, mu = fixture_nodes(which)
    k = FIXTURE_K[which]
    return gamma, mu, surfaces(gamma, mu), None if k is None else np.array(k)


# ---- what the host check refuses ----------------------------------------------------------------------------------------
def refused_cases(gamma, mu, t, k):
    """name -> (gamma, mu, log_n, sin_k, shape) of calls that differ from the valid (gamma, mu, t, k) in one respect each and
    that rimphony_ctx_set_tables_2d_nodes must refuse with RIMPHONY_EINVAL; shape: what the call states where log_n cannot"""
    nn, nmu = len(gamma), len(mu)
    k1 = None if k is None else np.asarray(k)[:1]

    def mu_with(j, v):
        m = np.array(mu, dtype=np.float64)
        m[j] = v
        return m

    tb = np.array(t, dtype=np.float64)
    tb[1, 5, 3] = np.nan
    swapped_mu, swapped_g, low = mu_with(0, mu[0]), np.array(gamma), np.array(gamma)
    swapped_mu[[3, 4]] = swapped_mu[[4, 3]]
    swapped_g[[5, 6]] = swapped_g[[6, 5]]
    low[0] = np.nextafter(1.0, 0.0)
    wide_g = np.exp(np.linspace(0.01, 9.0, 2048))
    bad = {
        "null gamma": (None, mu, t, k, t.shape), "null mu": (gamma, None, t, k, t.shape), "null log_n": (gamma, mu, None, k, t.shape),
        "log_n NaN": (gamma, mu, tb, k, None),
        "mu NaN": (gamma, mu_with(2, np.nan), t, k, None), "mu inf": (gamma, mu_with(nmu - 1, np.inf), t, k, None),
        "mu[0] = -1 + 1e-16": (gamma, mu_with(0, -1.0 + 1e-16), t, k, None),
        "mu[last] = nextafter(1, 0)": (gamma, mu_with(nmu - 1, np.nextafter(1.0, 0.0)), t, k, None),
        "mu[0] = -1.5": (gamma, mu_with(0, -1.5), t, k, None),
        "two equal mu nodes": (gamma, mu_with(3, mu[4]), t, k, None), "mu nodes swapped": (gamma, swapped_mu, t, k, None),
        "7 mu nodes": (gamma, np.linspace(-1.0, 1.0, 7), t[:, :, :7], k, None),
        "1025 mu nodes": (gamma[:8], np.linspace(-1.0, 1.0, 1025), np.zeros((1, 8, 1025)), k1, None),
        "n_nodes n_mu over 2^20": (wide_g, np.linspace(-1.0, 1.0, 1024), np.zeros((1, 2048, 1024)), k1, None),
        "7 gamma nodes": (gamma[:7], mu, t[:, :7], k, None), "gamma nodes swapped": (swapped_g, mu, t, k, None),
        "gamma[0] < 1": (low, mu, t, k, None),
    }
    if k is not None:
        bad.update({"k negative": (gamma, mu, t, [0.5, -0.1], None), "k above 100": (gamma, mu, t, [100.5, 1.0], None),
                    "k NaN": (gamma, mu, t, [np.nan, 1.0], None), "k inf": (gamma, mu, t, [1.0, np.inf], None)})
    assert (-1.0 + 1e-16) != -1.0 and nn >= 8
    return bad
