"""Host-side mirror of rimphony's public API on top of the HIP C ABI.

Reference surface being mirrored (same names, argument meaning and error
behaviour; see src/lib.rs of pkgw/rimphony):

  Stokes, Coefficient                               lib.rs:74-107
  SynchrotronCalculator.compute_dimensionless       lib.rs:155-156
                       .compute_cgs                 lib.rs:163-173
                       .compute_all_dimensionless   lib.rs:178-191
                       .compute_all_cgs             lib.rs:196-209
  PowerLawDistribution(p).gamma_limits(..).full_calculation()          power_law.rs:71-111
  ThermalJuettnerDistribution(T).full_calculation()                    thermal_juettner.rs:45-72
  PitchyPowerLawDistribution(p, k).gamma_limits(..).full_calculation() pitchy_pl.rs:73-115
  PitchyKappaDistribution(kappa, width, k).gamma_cutoff(..)...         pitchy_kappa.rs:70-125
  TabulatedDistribution(gamma_lo, gamma_hi, log_n)  the open DistributionFunction trait (lib.rs:111-146) as data: a table
                                                    of ln n(gamma), spline-interpolated inside the integrand
  TabulatedFamily(gamma_lo, gamma_hi, log_n, ...)   a set of such tables with a continuous parameter: .at(value) is the member
                                                    between two stored tables, blended inside the integrand
  TabulatedFamily2D(gamma, mu, log_n, ...)          the same for surfaces ln n(gamma, mu) on given gamma and mu nodes

plus the batched compute() the north star adds: `compute_batch`.  PyTorch is
used only as plumbing (device buffers, the current HIP stream).  Everything is
evaluated by librimphony_hip.so on the GPU; there is no CPU path here.
"""
import ctypes
import enum
import math

import numpy as np
import torch

from . import capi

# lib.rs:55-67
PI = math.pi
TWO_PI = 2.0 * math.pi
MASS_ELECTRON = 9.1093826e-28
SPEED_LIGHT = 2.99792458e10
ELECTRON_CHARGE = 4.80320680e-10


class Stokes(enum.IntEnum):
    I = 0
    Q = 1
    V = 2


class Coefficient(enum.IntEnum):
    Emission = 0
    Absorption = 1
    Faraday = 2


POWER_LAW, THERMAL_JUETTNER, PITCHY_PL, PITCHY_KAPPA, TABULATED = 0, 1, 2, 3, 4
NPARAMS = {POWER_LAW: 4, THERMAL_JUETTNER: 1, PITCHY_PL: 5, PITCHY_KAPPA: 4, TABULATED: 1}
TAB_MIN_NODES, TAB_MAX_NODES = 8, 65536

# slot order of compute_all_dimensionless (lib.rs:176-177)
SLOTS = [
    (Coefficient.Emission, Stokes.I), (Coefficient.Absorption, Stokes.I),
    (Coefficient.Emission, Stokes.Q), (Coefficient.Absorption, Stokes.Q),
    (Coefficient.Emission, Stokes.V), (Coefficient.Absorption, Stokes.V),
    (Coefficient.Faraday, Stokes.Q), (Coefficient.Faraday, Stokes.V),
]
SLOTS_ALL = 0xFF
SLOTS_SYMPHONY = 0x3F
# `precision` of the batch entry points (include/rimphony_hip.h)
PRECISION_F64 = 0               # the reference's arithmetic; bit-identical to the oracle
PRECISION_F32_INTEGRAND = 1     # refused by the library (RIMPHONY_ENOTSUP): slower and lossier than F64, include/rimphony_hip.h


def slot_of(coeff, stokes):
    return SLOTS.index((Coefficient(coeff), Stokes(stokes)))


def check_param_count(kind, params):
    """The parameter arrays of a batch: one per parameter of the kind (TABULATED: one, the table index of each row)."""
    if kind not in NPARAMS:
        raise ValueError("unknown distribution kind %r" % (kind,))
    if len(params) != NPARAMS[kind]:
        raise ValueError("distribution kind %d takes %d parameter arrays, got %d" % (kind, NPARAMS[kind], len(params)))


def check_tables(gamma_lo, gamma_hi, log_n):
    """A table set as rimphony_ctx_set_tables accepts it -> contiguous float64 [n_tables][n_nodes]; ValueError for what the
    library refuses with RIMPHONY_EINVAL (include/rimphony_hip.h)."""
    t = np.ascontiguousarray(np.atleast_2d(np.asarray(log_n, dtype=np.float64)))
    if t.ndim != 2 or t.shape[0] < 1:
        raise ValueError("log_n: expected [n_nodes] or [n_tables][n_nodes]")
    if not TAB_MIN_NODES <= t.shape[1] <= TAB_MAX_NODES:
        raise ValueError("log_n: %d nodes, expected %d .. %d" % (t.shape[1], TAB_MIN_NODES, TAB_MAX_NODES))
    if not (math.isfinite(gamma_lo) and math.isfinite(gamma_hi) and 1.0 <= gamma_lo < gamma_hi):
        raise ValueError("expected 1 <= gamma_lo < gamma_hi, got %r, %r" % (gamma_lo, gamma_hi))
    if not np.isfinite(t).all():
        raise ValueError("log_n: every value must be finite (a table cannot hold n = 0: let it roll off instead)")
    return t


def check_pitch_tables(gamma_lo, gamma_hi, log_n, log_g=None, n_mu=None):
    """A table set as rimphony_ctx_set_tables_pitch accepts it -> (log_n, log_g), contiguous float64 [n_tables][n_nodes] and
    [n_tables][n_mu] (log_g None: an isotropic set, check_tables alone); ValueError for what the library refuses with
    RIMPHONY_EINVAL.  n_mu, if given, is the node count the caller means to state: it must be the row length of log_g, 0
    without one."""
    t = check_tables(gamma_lo, gamma_hi, log_n)
    if log_g is None:
        if n_mu:
            raise ValueError("n_mu = %d without log_g" % n_mu)
        return t, None
    g = np.ascontiguousarray(np.atleast_2d(np.asarray(log_g, dtype=np.float64)))
    if n_mu is not None and n_mu != g.shape[1]:
        raise ValueError("n_mu = %d, but log_g has %d nodes per row" % (n_mu, g.shape[1]))
    if g.ndim != 2 or g.shape[0] != t.shape[0]:
        raise ValueError("log_g: expected one row of ln g per table (%d), got shape %r" % (t.shape[0], g.shape))
    if not TAB_MIN_NODES <= g.shape[1] <= TAB_MAX_NODES:
        raise ValueError("log_g: %d nodes, expected %d .. %d" % (g.shape[1], TAB_MIN_NODES, TAB_MAX_NODES))
    if not np.isfinite(g).all():
        raise ValueError("log_g: every value must be finite (g = 0 cannot be held: floor ln g instead)")
    return t, g


TAB_MAX_SIN_K = 100.0


def check_sin_k(sin_k, n_tables):
    """The exponents of a set's sin^k xi prefactors as rimphony_ctx_set_tables_pitchy accepts them -> contiguous float64
    [n_tables] (a scalar serves every table); ValueError for what the library refuses with RIMPHONY_EINVAL."""
    k = np.asarray(sin_k, dtype=np.float64)
    if k.ndim == 0:
        k = np.full(n_tables, float(k))
    if k.ndim != 1 or k.shape[0] != n_tables:
        raise ValueError("sin_k: expected a scalar or one value per table (%d), got shape %r" % (n_tables, k.shape))
    if not (np.isfinite(k) & (k >= 0.0) & (k <= TAB_MAX_SIN_K)).all():
        raise ValueError("sin_k: every exponent must be finite and in [0, %g]" % TAB_MAX_SIN_K)
    return np.ascontiguousarray(k)


def grid_nodes_log_gm1(gamma_lo, gamma_hi, n_nodes):
    """n_nodes gamma uniform in ln(gamma - 1) from gamma_lo to gamma_hi (1 < gamma_lo < gamma_hi), the ends exactly those:
    as many nodes in every e-fold of gamma - 1, which is what a cold or mildly relativistic core needs
    (Context.set_tables_grid)."""
    if not (1.0 < gamma_lo < gamma_hi) or int(n_nodes) < 2:
        raise ValueError("grid_nodes_log_gm1: expected 1 < gamma_lo < gamma_hi and at least two nodes")
    gamma = 1.0 + np.exp(np.linspace(math.log(gamma_lo - 1.0), math.log(gamma_hi - 1.0), int(n_nodes)))
    gamma[0], gamma[-1] = gamma_lo, gamma_hi
    return gamma


def check_grid_tables(gamma, log_n, log_g=None):
    """A table set as rimphony_ctx_set_tables_grid accepts it -> (gamma, log_n, log_g), contiguous float64 [n_nodes],
    [n_tables][n_nodes] and [n_tables][n_mu] or None; ValueError for what the library refuses with RIMPHONY_EINVAL (the
    library itself judges whether the nodes' logarithms increase)."""
    g = np.ascontiguousarray(np.asarray(gamma, dtype=np.float64))
    if g.ndim != 1 or not TAB_MIN_NODES <= g.shape[0] <= TAB_MAX_NODES:
        raise ValueError("gamma: expected %d to %d nodes, got shape %r" % (TAB_MIN_NODES, TAB_MAX_NODES, g.shape))
    if not np.isfinite(g).all() or not g[0] >= 1.0 or not (np.diff(g) > 0.0).all():
        raise ValueError("gamma: the nodes must be finite and strictly increasing from gamma[0] >= 1")
    t, p = check_pitch_tables(float(g[0]), float(g[-1]), log_n, log_g)
    if t.shape[1] != g.shape[0]:
        raise ValueError("log_n: expected rows of %d values, one per node, got %d" % (g.shape[0], t.shape[1]))
    return g, t, p


TAB_2D_MIN_MU, TAB_2D_MAX_MU, TAB_2D_MAX_CELLS = 8, 1024, 1 << 20


def check_tables_2d(gamma_lo, gamma_hi, log_n):
    """A 2-D table set as rimphony_ctx_set_tables_2d accepts it -> contiguous float64 [n_tables][n_nodes][n_mu] (a 2-D
    array is one table); ValueError for what the library refuses with RIMPHONY_EINVAL (include/rimphony_hip.h)."""
    t = np.asarray(log_n, dtype=np.float64)
    if t.ndim == 2:
        t = t[None]
    if t.ndim != 3 or t.shape[0] < 1:
        raise ValueError("log_n: expected [n_nodes][n_mu] or [n_tables][n_nodes][n_mu]")
    t = np.ascontiguousarray(t)
    if not TAB_MIN_NODES <= t.shape[1] <= TAB_MAX_NODES:
        raise ValueError("log_n: %d gamma nodes, expected %d .. %d" % (t.shape[1], TAB_MIN_NODES, TAB_MAX_NODES))
    if not TAB_2D_MIN_MU <= t.shape[2] <= TAB_2D_MAX_MU:
        raise ValueError("log_n: %d mu nodes, expected %d .. %d" % (t.shape[2], TAB_2D_MIN_MU, TAB_2D_MAX_MU))
    if t.shape[1] * t.shape[2] > TAB_2D_MAX_CELLS:
        raise ValueError("log_n: %d x %d nodes per table, at most %d" % (t.shape[1], t.shape[2], TAB_2D_MAX_CELLS))
    if not (math.isfinite(gamma_lo) and math.isfinite(gamma_hi) and 1.0 <= gamma_lo < gamma_hi):
        raise ValueError("expected 1 <= gamma_lo < gamma_hi, got %r, %r" % (gamma_lo, gamma_hi))
    if not np.isfinite(t).all():
        raise ValueError("log_n: every value must be finite (a table cannot hold n = 0: floor ln n instead)")
    return t


def check_gamma_nodes(gamma):
    """The gamma nodes of a 2-D set on given nodes -> contiguous float64 [n_nodes]; ValueError for what the library refuses
    (it judges itself whether the nodes' logarithms increase)."""
    g = np.ascontiguousarray(np.asarray(gamma, dtype=np.float64))
    if g.ndim != 1 or not TAB_MIN_NODES <= g.shape[0] <= TAB_MAX_NODES:
        raise ValueError("gamma: expected %d to %d nodes, got shape %r" % (TAB_MIN_NODES, TAB_MAX_NODES, g.shape))
    if not np.isfinite(g).all() or not g[0] >= 1.0 or not (np.diff(g) > 0.0).all():
        raise ValueError("gamma: the nodes must be finite and strictly increasing from gamma[0] >= 1")
    return g


def check_mu_nodes(mu):
    """The mu nodes of a 2-D set on given mu nodes -> contiguous float64 [n_mu]; ValueError for what the library refuses."""
    m = np.ascontiguousarray(np.asarray(mu, dtype=np.float64))
    if m.ndim != 1 or not TAB_2D_MIN_MU <= m.shape[0] <= TAB_2D_MAX_MU:
        raise ValueError("mu: expected %d to %d nodes, got shape %r" % (TAB_2D_MIN_MU, TAB_2D_MAX_MU, m.shape))
    if not np.isfinite(m).all() or not (np.diff(m) > 0.0).all():
        raise ValueError("mu: the nodes must be finite and strictly increasing")
    if m[0] != -1.0 or m[-1] != 1.0:
        raise ValueError("mu: the first node must be -1 and the last +1 exactly")
    return m


def check_tables_2d_grid(gamma, log_n):
    """A 2-D table set on given nodes as rimphony_ctx_set_tables_2d_grid accepts it -> (gamma, log_n), contiguous float64
    [n_nodes] and [n_tables][n_nodes][n_mu] (a 2-D array is one table); ValueError for what the library refuses with
    RIMPHONY_EINVAL (the library itself judges whether the nodes' logarithms increase)."""
    g = check_gamma_nodes(gamma)
    t = check_tables_2d(float(g[0]), float(g[-1]), log_n)
    if t.shape[1] != g.shape[0]:
        raise ValueError("log_n: expected %d rows of mu nodes per table, one per gamma node, got %d" % (g.shape[0], t.shape[1]))
    return g, t


def mu_nodes_uniform_in_xi(n):
    """n mu nodes uniform in the pitch angle xi, mu_j = -cos(pi j / (n - 1)), the ends exactly -1 and +1: the nodes of a
    pitch-angle histogram with bins uniform in xi, densest where a grid uniform in mu is coarsest in angle
    (Context.set_tables_2d_nodes)."""
    n = int(n)
    if n < 2:
        raise ValueError("mu_nodes_uniform_in_xi: expected at least two nodes")
    mu = -np.cos(np.pi * np.arange(n) / (n - 1))
    mu[0], mu[-1] = -1.0, 1.0
    return mu


def check_tables_2d_nodes(gamma, mu, log_n):
    """A 2-D table set on given gamma and mu nodes as rimphony_ctx_set_tables_2d_nodes accepts it -> (gamma, mu, log_n),
    contiguous float64 [n_nodes], [n_mu] and [n_tables][n_nodes][n_mu] (a 2-D array is one table); ValueError for what the
    library refuses with RIMPHONY_EINVAL."""
    m = check_mu_nodes(mu)
    g, t = check_tables_2d_grid(gamma, log_n)
    if t.shape[2] != m.shape[0]:
        raise ValueError("log_n: expected rows of %d values, one per mu node, got %d" % (m.shape[0], t.shape[2]))
    return g, m, t


TAB_ENDS_NATURAL, TAB_ENDS_NOT_A_KNOT = 0, 1
_TAB_ENDS = {"natural": TAB_ENDS_NATURAL, "not-a-knot": TAB_ENDS_NOT_A_KNOT}


def check_ends(ends):
    """The ends of the spline of a 2-D set -> (ends_gamma, ends_mu), each TAB_ENDS_NATURAL or TAB_ENDS_NOT_A_KNOT, or None for
    None (the entries that know of no choice).  ends: "natural" or "not-a-knot" for both axes, or a pair (gamma_end, mu_end)
    of those names or values.  ValueError for anything else (include/rimphony_hip.h: rimphony_ctx_set_tables_2d_ends)."""
    if ends is None:
        return None

    def one(e):
        if isinstance(e, str):
            if e not in _TAB_ENDS:
                raise ValueError("ends: expected 'natural' or 'not-a-knot', got %r" % (e,))
            return _TAB_ENDS[e]
        if isinstance(e, (bool, float)) or e not in (TAB_ENDS_NATURAL, TAB_ENDS_NOT_A_KNOT):
            raise ValueError("ends: expected 'natural' or 'not-a-knot', got %r" % (e,))
        return int(e)

    if isinstance(ends, str):
        return one(ends), one(ends)
    try:
        eg, em = ends
    except (TypeError, ValueError):
        raise ValueError("ends: expected 'natural', 'not-a-knot' or a pair (gamma_end, mu_end), got %r" % (ends,))
    return one(eg), one(em)


class Context:
    """Owns a rimphony_ctx bound to one GPU."""

    def __init__(self, device=0):
        self.lib = capi.load()
        if not torch.cuda.is_available():
            raise capi.RimphonyError("no HIP device visible: rimphony_amd has no CPU fallback")
        self.device = int(device)
        h = ctypes.c_void_p()
        capi.check(self.lib.rimphony_ctx_create(self.device, ctypes.byref(h)), "rimphony_ctx_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None):
            self.lib.rimphony_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------
    def _dev(self):
        return torch.device("cuda", self.device)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self._dev()).cuda_stream)

    def _as_dev(self, x):
        t = torch.as_tensor(x, dtype=torch.float64)
        return t.to(self._dev()).contiguous()

    # -- tabulated distributions ---------------------------------------------------
    def set_tables(self, gamma_lo, gamma_hi, log_n, log_g=None, sin_k=None):
        """The context's table set for kind TABULATED: log_n [n_tables][n_nodes] (or [n_nodes]) = ln n(gamma) at nodes
        uniform in ln gamma from gamma_lo to gamma_hi, n = dN/dgamma up to a factor.  Replaces the previous set; None
        clears it.  Synchronous.  Let n roll off to a negligible value at both ends: a table that ends at a sizeable n is a
        step in f, like the power law's gamma limits (include/rimphony_hip.h).
        log_g [n_tables][n_mu] (or [n_mu]) gives each table a pitch-angle factor g(mu), mu = cos xi: ln g at nodes uniform in
        mu from -1 to +1, f = norm n g / (gamma^2 beta).  Only the shape of a row matters.  A ln g that diverges at the
        ends (sin^k xi) cannot be held in a row: give the exponent instead.
        sin_k (a scalar, or one value per table, each in [0, 100]) multiplies each table by sin^k xi, the pitchy kinds'
        own anisotropy, in closed form: f = norm n sin^k xi g / (gamma^2 beta), with or without log_g
        (include/rimphony_hip.h: rimphony_ctx_set_tables_pitchy)."""
        if log_n is None:
            capi.check(self.lib.rimphony_ctx_set_tables(self.handle, 0, 0, 1.0, 2.0, None), "rimphony_ctx_set_tables")
            return
        if sin_k is not None:
            t, g = check_pitch_tables(gamma_lo, gamma_hi, log_n, log_g)
            k = check_sin_k(sin_k, t.shape[0])
            dp = ctypes.POINTER(ctypes.c_double)
            capi.check(self.lib.rimphony_ctx_set_tables_pitchy(self.handle, t.shape[0], t.shape[1], float(gamma_lo), float(gamma_hi),
                                                               t.ctypes.data_as(dp), 0 if g is None else g.shape[1],
                                                               None if g is None else g.ctypes.data_as(dp), k.ctypes.data_as(dp)),
                       "rimphony_ctx_set_tables_pitchy")
            return
        if log_g is not None:
            t, g = check_pitch_tables(gamma_lo, gamma_hi, log_n, log_g)
            dp = ctypes.POINTER(ctypes.c_double)
            capi.check(self.lib.rimphony_ctx_set_tables_pitch(self.handle, t.shape[0], t.shape[1], float(gamma_lo), float(gamma_hi),
                                                              t.ctypes.data_as(dp), g.shape[1], g.ctypes.data_as(dp)),
                       "rimphony_ctx_set_tables_pitch")
            return
        t = check_tables(gamma_lo, gamma_hi, log_n)
        capi.check(self.lib.rimphony_ctx_set_tables(self.handle, t.shape[0], t.shape[1], float(gamma_lo), float(gamma_hi),
                                                    t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                   "rimphony_ctx_set_tables")

    def set_tables_family(self, gamma_lo, gamma_hi, log_n, sin_k=None):
        """The context's table set as a FAMILY: log_n [n_tables][n_nodes] as for set_tables, and the one parameter of a
        TABULATED row a real index x in [0, n_tables - 1].  Every sample blends the splines of tables floor(x) and
        floor(x) + 1 with the weight x - floor(x); the normalisation is per row, over the blended spline.  sin_k (a scalar, or
        one value per table, each in [0, 100]) gives each table a sin^k xi prefactor whose exponent is blended likewise.  A
        row at an integer x carries the bits of that table installed through set_tables; an x outside the range is a NaN
        row.  Replaces the previous set of any form; log_n None clears it.  Synchronous (include/rimphony_hip.h:
        rimphony_ctx_set_tables_family)."""
        if log_n is None:
            capi.check(self.lib.rimphony_ctx_set_tables_family(self.handle, 0, 0, 1.0, 2.0, None, None), "rimphony_ctx_set_tables_family")
            return
        t = check_tables(gamma_lo, gamma_hi, log_n)
        k = None if sin_k is None else check_sin_k(sin_k, t.shape[0])
        dp = ctypes.POINTER(ctypes.c_double)
        capi.check(self.lib.rimphony_ctx_set_tables_family(self.handle, t.shape[0], t.shape[1], float(gamma_lo), float(gamma_hi),
                                                           t.ctypes.data_as(dp), None if k is None else k.ctypes.data_as(dp)),
                   "rimphony_ctx_set_tables_family")

    def set_tables_grid(self, gamma, log_n, log_g=None, sin_k=None):
        """The context's table set on gamma nodes of the caller's choosing: gamma [n_nodes] strictly increasing from >= 1,
        shared by the tables; log_n [n_tables][n_nodes] (or [n_nodes]) = ln n at the nodes.  For what nodes uniform in
        ln gamma cannot resolve, a cold thermal core above all (grid_nodes_log_gm1 gives nodes uniform in ln(gamma - 1)).
        log_g and sin_k as for set_tables.  Replaces the previous set of any form; log_n None clears it.  Synchronous
        (include/rimphony_hip.h: rimphony_ctx_set_tables_grid)."""
        if log_n is None:
            capi.check(self.lib.rimphony_ctx_set_tables_grid(self.handle, 0, 0, None, None, 0, None, None), "rimphony_ctx_set_tables_grid")
            return
        g, t, p = check_grid_tables(gamma, log_n, log_g)
        k = None if sin_k is None else check_sin_k(sin_k, t.shape[0])
        dp = ctypes.POINTER(ctypes.c_double)
        capi.check(self.lib.rimphony_ctx_set_tables_grid(self.handle, t.shape[0], t.shape[1], g.ctypes.data_as(dp), t.ctypes.data_as(dp),
                                                         0 if p is None else p.shape[1], None if p is None else p.ctypes.data_as(dp),
                                                         None if k is None else k.ctypes.data_as(dp)),
                   "rimphony_ctx_set_tables_grid")

    def set_tables_2d(self, gamma_lo, gamma_hi, log_n, sin_k=None, ends=None):
        """The context's table set for kind TABULATED as surfaces: log_n [n_tables][n_nodes][n_mu] (a 2-D array is one
        table) = ln n(gamma, mu) at nodes uniform in ln gamma from gamma_lo to gamma_hi and uniform in mu = cos xi from -1
        to +1; f = norm exp(S) / (gamma^2 beta) with S the tensor-product natural cubic spline.  Replaces the previous set of
        any form; None clears it.  Synchronous: the normalisation of every table is integrated here, once
        (include/rimphony_hip.h: rimphony_ctx_set_tables_2d).
        sin_k (a scalar, or one value per table, each in [0, 100]) multiplies each table by sin^k xi in closed form, f =
        norm sin^k xi exp(S) / (gamma^2 beta): for a distribution that vanishes along the field, whose ln n no surface can
        hold.  log_n is then the smooth remainder, ln(n / sin^k xi) (rimphony_ctx_set_tables_2d_pitchy).
        ends chooses the ends of the spline: None or "natural" (S'' = 0 across the end nodes), "not-a-knot" (every cubic
        along an axis comes back as itself: for a surface curved at mu = +-1, a bi-Maxwellian say), or a pair (gamma_end,
        mu_end) (check_ends; rimphony_ctx_set_tables_2d_ends).  It costs nothing per sample."""
        ends = check_ends(ends)
        if log_n is None:
            capi.check(self.lib.rimphony_ctx_set_tables_2d(self.handle, 0, 0, 1.0, 2.0, 0, None), "rimphony_ctx_set_tables_2d")
            return
        if isinstance(log_n, torch.Tensor) and log_n.is_cuda:
            if not (math.isfinite(gamma_lo) and math.isfinite(gamma_hi) and 1.0 <= gamma_lo < gamma_hi):
                raise ValueError("expected 1 <= gamma_lo < gamma_hi, got %r, %r" % (gamma_lo, gamma_hi))
            self._set_tables_2d_device(None, float(gamma_lo), float(gamma_hi), None, log_n, sin_k, ends)
            return
        t = check_tables_2d(gamma_lo, gamma_hi, log_n)
        if ends is not None:
            self._set_tables_2d_ends(None, float(gamma_lo), float(gamma_hi), None, t, sin_k, ends)
            return
        if sin_k is not None:
            k = check_sin_k(sin_k, t.shape[0])
            dp = ctypes.POINTER(ctypes.c_double)
            capi.check(self.lib.rimphony_ctx_set_tables_2d_pitchy(self.handle, t.shape[0], t.shape[1], float(gamma_lo), float(gamma_hi),
                                                                  t.shape[2], t.ctypes.data_as(dp), k.ctypes.data_as(dp)),
                       "rimphony_ctx_set_tables_2d_pitchy")
            return
        capi.check(self.lib.rimphony_ctx_set_tables_2d(self.handle, t.shape[0], t.shape[1], float(gamma_lo), float(gamma_hi),
                                                       t.shape[2], t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))),
                   "rimphony_ctx_set_tables_2d")

    def set_tables_2d_grid(self, gamma, log_n, sin_k=None, ends=None):
        """The context's table set as surfaces on gamma nodes of the caller's choosing: gamma [n_nodes] strictly increasing
        from >= 1, shared by the tables; log_n [n_tables][n_nodes][n_mu] (a 2-D array is one table) = ln n(gamma_i, mu_j),
        the mu nodes uniform from -1 to +1.  What set_tables_2d holds, on the nodes set_tables_grid takes: a cold core under
        an anisotropic tail.  Replaces the previous set of any form; log_n None clears it.  Synchronous: the normalisation of
        every table is integrated here, once (include/rimphony_hip.h: rimphony_ctx_set_tables_2d_grid).  sin_k as for
        set_tables_2d (rimphony_ctx_set_tables_2d_grid_pitchy), and so ends."""
        ends = check_ends(ends)
        if log_n is None:
            capi.check(self.lib.rimphony_ctx_set_tables_2d_grid(self.handle, 0, 0, None, 0, None), "rimphony_ctx_set_tables_2d_grid")
            return
        if isinstance(log_n, torch.Tensor) and log_n.is_cuda:
            self._set_tables_2d_device(check_gamma_nodes(gamma), 1.0, 2.0, None, log_n, sin_k, ends)
            return
        g, t = check_tables_2d_grid(gamma, log_n)
        if ends is not None:
            self._set_tables_2d_ends(g, 1.0, 2.0, None, t, sin_k, ends)
            return
        dp = ctypes.POINTER(ctypes.c_double)
        if sin_k is not None:
            k = check_sin_k(sin_k, t.shape[0])
            capi.check(self.lib.rimphony_ctx_set_tables_2d_grid_pitchy(self.handle, t.shape[0], t.shape[1], g.ctypes.data_as(dp),
                                                                       t.shape[2], t.ctypes.data_as(dp), k.ctypes.data_as(dp)),
                       "rimphony_ctx_set_tables_2d_grid_pitchy")
            return
        capi.check(self.lib.rimphony_ctx_set_tables_2d_grid(self.handle, t.shape[0], t.shape[1], g.ctypes.data_as(dp), t.shape[2],
                                                            t.ctypes.data_as(dp)),
                   "rimphony_ctx_set_tables_2d_grid")

    # -- batched compute() -------------------------------------------------------
    def set_tables_2d_nodes(self, gamma, mu, log_n, sin_k=None, ends=None):
        """The context's table set as surfaces on gamma nodes AND mu nodes of the caller's choosing: gamma [n_nodes] strictly
        increasing from >= 1 and mu [n_mu] strictly increasing from exactly -1 to exactly +1, both shared by the tables;
        log_n [n_tables][n_nodes][n_mu] (a 2-D array is one table) = ln n(gamma_i, mu_j).  What set_tables_2d_grid holds, on
        mu nodes graded towards a beam, a ring or the edge of a loss cone, or uniform in xi (mu_nodes_uniform_in_xi).
        sin_k and ends as for set_tables_2d.  Replaces the previous set of any form; log_n None clears it.  Synchronous: the
        normalisation of every table is integrated here, once (include/rimphony_hip.h: rimphony_ctx_set_tables_2d_nodes)."""
        ends = check_ends(ends)
        if log_n is None:
            capi.check(self.lib.rimphony_ctx_set_tables_2d_nodes(self.handle, 0, 0, None, 0, None, None, None),
                       "rimphony_ctx_set_tables_2d_nodes")
            return
        if isinstance(log_n, torch.Tensor) and log_n.is_cuda:
            self._set_tables_2d_device(check_gamma_nodes(gamma), 1.0, 2.0, check_mu_nodes(mu), log_n, sin_k, ends)
            return
        g, m, t = check_tables_2d_nodes(gamma, mu, log_n)
        if ends is not None:
            self._set_tables_2d_ends(g, 1.0, 2.0, m, t, sin_k, ends)
            return
        k = None if sin_k is None else check_sin_k(sin_k, t.shape[0])
        dp = ctypes.POINTER(ctypes.c_double)
        capi.check(self.lib.rimphony_ctx_set_tables_2d_nodes(self.handle, t.shape[0], t.shape[1], g.ctypes.data_as(dp), t.shape[2],
                                                             m.ctypes.data_as(dp), t.ctypes.data_as(dp),
                                                             None if k is None else k.ctypes.data_as(dp)),
                   "rimphony_ctx_set_tables_2d_nodes")

    def set_tables_2d_family(self, gamma, mu, log_n, sin_k=None, ends=None, blend="linear", param=None):
        """The context's table set as a FAMILY of surfaces: gamma, mu and log_n [n_tables][n_nodes][n_mu] as for
        set_tables_2d_nodes, and the one parameter of a TABULATED row a real index x in [0, n_tables - 1].  Every sample finds
        its cell once, blends the cell's sixteen node words from tables floor(x) and floor(x) + 1 with the weight x - floor(x)
        and evaluates one bicubic; sin_k (a scalar, or one value per table, each in [0, 100]) gives each table a sin^k xi
        prefactor whose exponent is blended likewise; ends as for set_tables_2d.  The normalisation is per row, integrated over
        the blended surface with every batch -- its cost grows with the number of mu nodes
        (profiles/tabulated_2d_family_times.txt).  A row at an integer x carries the bits of that table installed through
        set_tables_2d_nodes; an x outside the range is a NaN row.  Replaces the previous set of any form; log_n None clears it.
        Synchronous; host arrays only (include/rimphony_hip.h: rimphony_ctx_set_tables_2d_family).

        blend="cubic" blends FOUR neighbouring tables with a 4-point Lagrange cubic in `param` -- one finite knot per table,
        strictly monotonic; None: the index itself --, and k likewise (rimphony_ctx_set_tables_2d_family_cubic).  At least four
        tables.  A row whose blended k overshoots [0, 100] is a NaN row: space sin_k smoothly.  Fourth order in the spacing
        of the tables where the linear blend is second order, for four runs of node words per sample instead of two
        (profiles/tabulated_2d_family_cubic_accuracy.txt, profiles/tabulated_2d_family_cubic_times.txt).  The linear blend
        has no knots: a param with blend="linear" is a ValueError."""
        if blend not in ("linear", "cubic"):
            raise ValueError("blend: expected 'linear' or 'cubic', got %r" % (blend,))
        if blend == "linear" and param is not None:
            raise ValueError("param: the linear blend has no knots (blend='cubic' takes them)")
        ends = check_ends(ends) or (TAB_ENDS_NATURAL, TAB_ENDS_NATURAL)
        if blend == "cubic":
            dp = ctypes.POINTER(ctypes.c_double)
            if log_n is None:
                capi.check(self.lib.rimphony_ctx_set_tables_2d_family_cubic(self.handle, 0, 0, None, 0, None, None, None, 0, 0, None),
                           "rimphony_ctx_set_tables_2d_family_cubic")
                return
            g, m, t = check_tables_2d_nodes(gamma, mu, log_n)
            k = None if sin_k is None else check_sin_k(sin_k, t.shape[0])
            if t.shape[0] < 4:
                raise ValueError("log_n: the cubic blend needs at least 4 tables, got %d" % t.shape[0])
            c = None if param is None else TabulatedFamily._check_param(param, t.shape[0])
            entry = self.lib.rimphony_ctx_set_tables_2d_family_cubic
            capi.check(entry(self.handle, t.shape[0], t.shape[1], g.ctypes.data_as(dp), t.shape[2], m.ctypes.data_as(dp),
                             t.ctypes.data_as(dp), None if k is None else k.ctypes.data_as(dp), ends[0], ends[1],
                             None if c is None else c.ctypes.data_as(dp)),
                       "rimphony_ctx_set_tables_2d_family_cubic")
            return
        if log_n is None:
            capi.check(self.lib.rimphony_ctx_set_tables_2d_family(self.handle, 0, 0, None, 0, None, None, None, 0, 0),
                       "rimphony_ctx_set_tables_2d_family")
            return
        g, m, t = check_tables_2d_nodes(gamma, mu, log_n)
        k = None if sin_k is None else check_sin_k(sin_k, t.shape[0])
        dp = ctypes.POINTER(ctypes.c_double)
        capi.check(self.lib.rimphony_ctx_set_tables_2d_family(self.handle, t.shape[0], t.shape[1], g.ctypes.data_as(dp), t.shape[2],
                                                              m.ctypes.data_as(dp), t.ctypes.data_as(dp),
                                                              None if k is None else k.ctypes.data_as(dp), ends[0], ends[1]),
                   "rimphony_ctx_set_tables_2d_family")

    def _set_tables_2d_ends(self, gamma, gamma_lo, gamma_hi, mu, t, sin_k, ends):
        """set_tables_2d, set_tables_2d_grid and set_tables_2d_nodes for a numpy log_n with a choice of ends: gamma, mu and
        t validated host arrays (gamma, mu None where the form places its own nodes), ends a pair from check_ends
        (include/rimphony_hip.h: rimphony_ctx_set_tables_2d_ends)."""
        k = None if sin_k is None else check_sin_k(sin_k, t.shape[0])
        dp = ctypes.POINTER(ctypes.c_double)
        rc = self.lib.rimphony_ctx_set_tables_2d_ends(
            self.handle, t.shape[0], t.shape[1], None if gamma is None else gamma.ctypes.data_as(dp), gamma_lo, gamma_hi, t.shape[2],
            None if mu is None else mu.ctypes.data_as(dp), t.ctypes.data_as(dp), None if k is None else k.ctypes.data_as(dp),
            ends[0], ends[1])
        capi.check(rc, "rimphony_ctx_set_tables_2d_ends")

    def _set_tables_2d_device(self, gamma, gamma_lo, gamma_hi, mu, log_n, sin_k, ends=None):
        """set_tables_2d, set_tables_2d_grid and set_tables_2d_nodes for a log_n that is a CUDA tensor: the same set, word for
        word, solved on the GPU from where the tensor lies, on the current stream (include/rimphony_hip.h:
        rimphony_ctx_set_tables_2d_device).  gamma, mu: validated host arrays or None; the tensor is held to the rules of
        _check_input, [n_nodes][n_mu] or [n_tables][n_nodes][n_mu] within the form's limits.  The library itself looks for a
        non-finite value.  Synchronous.  ends: None, or a pair from check_ends (rimphony_ctx_set_tables_2d_device_ends)."""
        if log_n.dim() not in (2, 3):
            raise ValueError("log_n: expected [n_nodes][n_mu] or [n_tables][n_nodes][n_mu]")
        self._check_input("log_n", log_n, log_n.numel())
        nt, nn, nmu = (1,) + tuple(log_n.shape) if log_n.dim() == 2 else tuple(log_n.shape)
        if nt < 1:
            raise ValueError("log_n: expected [n_nodes][n_mu] or [n_tables][n_nodes][n_mu]")
        if not TAB_MIN_NODES <= nn <= TAB_MAX_NODES:
            raise ValueError("log_n: %d gamma nodes, expected %d .. %d" % (nn, TAB_MIN_NODES, TAB_MAX_NODES))
        if not TAB_2D_MIN_MU <= nmu <= TAB_2D_MAX_MU:
            raise ValueError("log_n: %d mu nodes, expected %d .. %d" % (nmu, TAB_2D_MIN_MU, TAB_2D_MAX_MU))
        if nn * nmu > TAB_2D_MAX_CELLS:
            raise ValueError("log_n: %d x %d nodes per table, at most %d" % (nn, nmu, TAB_2D_MAX_CELLS))
        if gamma is not None and gamma.shape[0] != nn:
            raise ValueError("log_n: expected %d rows of mu nodes per table, one per gamma node, got %d" % (gamma.shape[0], nn))
        if mu is not None and mu.shape[0] != nmu:
            raise ValueError("log_n: expected rows of %d values, one per mu node, got %d" % (mu.shape[0], nmu))
        k = None if sin_k is None else check_sin_k(sin_k, nt)
        dp = ctypes.POINTER(ctypes.c_double)
        if ends is not None:
            rc = self.lib.rimphony_ctx_set_tables_2d_device_ends(
                self.handle, nt, nn, None if gamma is None else gamma.ctypes.data_as(dp), gamma_lo, gamma_hi, nmu,
                None if mu is None else mu.ctypes.data_as(dp), ctypes.c_void_p(log_n.data_ptr()),
                None if k is None else k.ctypes.data_as(dp), ends[0], ends[1], self._stream())
            capi.check(rc, "rimphony_ctx_set_tables_2d_device_ends")
            return
        rc = self.lib.rimphony_ctx_set_tables_2d_device(
            self.handle, nt, nn, None if gamma is None else gamma.ctypes.data_as(dp), gamma_lo, gamma_hi, nmu,
            None if mu is None else mu.ctypes.data_as(dp), ctypes.c_void_p(log_n.data_ptr()),
            None if k is None else k.ctypes.data_as(dp), self._stream())
        capi.check(rc, "rimphony_ctx_set_tables_2d_device")

    def tables_blob(self):
        """The installed table set as the kernels read it, a float64 numpy array (empty without a set): headers, guides,
        node words, spline words and normalisations, offsets instead of addresses -- two installs of the same numbers are
        equal word for word (include/rimphony_hip.h: rimphony_debug_tables)."""
        n = ctypes.c_size_t(0)
        rc = self.lib.rimphony_debug_tables(self.handle, None, 0, ctypes.byref(n))
        if n.value == 0:
            capi.check(rc, "rimphony_debug_tables")
            return np.zeros(0, dtype=np.float64)
        out = np.empty(n.value, dtype=np.float64)
        capi.check(self.lib.rimphony_debug_tables(self.handle, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n.value,
                                                  ctypes.byref(n)), "rimphony_debug_tables")
        return out

    def _check_input(self, name, t, n):
        """The C ABI takes raw device pointers and cannot see what they point to: refuse anything but a contiguous
        float64 tensor of n elements on this context's GPU (a strided view, a float32 tensor, a tensor on another
        device or a length-1 'broadcast' parameter would be read as garbage or out of bounds)."""
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: expected a torch.Tensor, got %s" % (name, type(t).__name__))
        if not t.is_cuda or t.device != self._dev():
            raise ValueError("%s: tensor is on %s, this context computes on %s" % (name, t.device, self._dev()))
        if t.dtype != torch.float64:
            raise TypeError("%s: dtype %s, expected float64" % (name, t.dtype))
        if t.numel() != n:
            raise ValueError("%s: %d elements, expected %d (one per parameter point; scalars are not broadcast)"
                             % (name, t.numel(), n))
        if not t.is_contiguous():
            raise ValueError("%s: not contiguous (pass t.contiguous())" % name)

    def compute_batch_device(self, kind, s, theta, params, coeff_mask=SLOTS_ALL, want_status=False, want_work=False,
                             precision=PRECISION_F64):
        """s, theta: CUDA float64 tensors [n]; params: list of CUDA float64 tensors [n].
        Returns (out [n, 8] CUDA tensor, status [n, 8] int32 CUDA tensor or None) -- and, with want_work, a third
        element: [n, 8] int64 integrand samples spent per coefficient.  Asynchronous on the current stream."""
        check_param_count(kind, params)
        if not isinstance(s, torch.Tensor):
            raise TypeError("s: expected a torch.Tensor, got %s" % type(s).__name__)
        n = s.numel()
        self._check_input("s", s, n)
        self._check_input("theta", theta, n)
        for k, p in enumerate(params):
            self._check_input("params[%d]" % k, p, n)
        out = torch.empty((n, 8), dtype=torch.float64, device=self._dev())
        status = torch.empty((n, 8), dtype=torch.int32, device=self._dev()) if want_status else None
        work = torch.empty((n, 8), dtype=torch.int64, device=self._dev()) if want_work else None
        pp = (ctypes.c_void_p * len(params))(*[ctypes.c_void_p(p.data_ptr()) for p in params])
        capi.check(self.lib.rimphony_batch_compute_device_ex(
            self.handle, kind, n, ctypes.c_void_p(s.data_ptr()), ctypes.c_void_p(theta.data_ptr()), pp,
            coeff_mask, int(precision), ctypes.c_void_p(out.data_ptr()),
            ctypes.c_void_p(status.data_ptr()) if want_status else None,
            ctypes.c_void_p(work.data_ptr()) if want_work else None, self._stream()),
            "rimphony_batch_compute_device_ex")
        if want_work:
            return out, status, work
        return out, status

    def compute_batch(self, kind, s, theta, params, coeff_mask=SLOTS_ALL, want_status=False, want_work=False,
                      precision=PRECISION_F64):
        """Host arrays in, numpy arrays out (synchronous)."""
        ds, dth = self._as_dev(s), self._as_dev(theta)
        dp = [self._as_dev(p) for p in params]
        res = self.compute_batch_device(kind, ds, dth, dp, coeff_mask, want_status, want_work, precision)
        torch.cuda.synchronize(self._dev())
        ret = [res[0].cpu().numpy()]
        if want_status:
            ret.append(res[1].cpu().numpy())
        if want_work:
            ret.append(res[2].cpu().numpy())
        return ret[0] if len(ret) == 1 else tuple(ret)

    def shared_mode(self):
        """False when this context owns its GPU (full persistent grids, cooperative tail); True when another context
        or process had the device first (rimphony_ctx_create in include/rimphony_hip.h)."""
        return bool(self.lib.rimphony_ctx_shared_mode(self.handle))

    def status_histogram(self, status):
        """status: the [n, 8] int32 CUDA tensor of a batch call -> numpy [8 slots, 8] counts: columns 0..6 = rows
        with RIMPHONY_ST_* bit b set, column 7 = rows with status 0."""
        if not (isinstance(status, torch.Tensor) and status.is_cuda and status.dtype == torch.int32 and status.is_contiguous()):
            raise TypeError("status: expected a contiguous int32 CUDA tensor")
        hist = (ctypes.c_uint64 * 64)()
        capi.check(self.lib.rimphony_status_histogram_device(self.handle, status.numel() // 8, ctypes.c_void_p(status.data_ptr()),
                                                              hist, self._stream()), "rimphony_status_histogram_device")
        return np.array(list(hist), dtype=np.int64).reshape(8, 8)

    DETMATH_OPS = {"exp": 0, "log": 1, "log10": 2, "pow": 3, "sqrt": 4, "log10_region": 5, "lgamma": 6, "sin": 7, "cos": 8,
                   "div_by": 9, "cbrt": 10, "rgamma": 11, "third_powers": 12,
                   "rqrt4": 13, "powexp": 14}

    def detmath_batch(self, op, x, y=None):
        """Unit seam: a leaf function of detmath.h evaluated on the device over host arrays."""
        dx = self._as_dev(x)
        dy = self._as_dev(y) if y is not None else None
        out = torch.empty_like(dx)
        capi.check(self.lib.rimphony_detmath_batch_device(
            self.handle, self.DETMATH_OPS[op], dx.numel(), ctypes.c_void_p(dx.data_ptr()),
            ctypes.c_void_p(dy.data_ptr()) if dy is not None else None, ctypes.c_void_p(out.data_ptr()), self._stream()),
            "rimphony_detmath_batch_device")
        torch.cuda.synchronize(self._dev())
        return out.cpu().numpy()

    def highfreq_batch(self, kind, s, theta, params):
        """High-frequency closed forms (power law / thermal only): host arrays in, [n, 2] = {rho_Q, rho_V} out."""
        ds, dth = self._as_dev(s), self._as_dev(theta)
        dp = [self._as_dev(p) for p in params]
        n = ds.numel()
        out = torch.empty((n, 2), dtype=torch.float64, device=self._dev())
        pp = (ctypes.c_void_p * len(dp))(*[ctypes.c_void_p(p.data_ptr()) for p in dp])
        capi.check(self.lib.rimphony_highfreq_batch_device(
            self.handle, kind, n, ctypes.c_void_p(ds.data_ptr()), ctypes.c_void_p(dth.data_ptr()), pp,
            ctypes.c_void_p(out.data_ptr()), self._stream()), "rimphony_highfreq_batch_device")
        torch.cuda.synchronize(self._dev())
        return out.cpu().numpy()

    def last_work(self):
        w = capi.Work()
        capi.check(self.lib.rimphony_last_work(self.handle, ctypes.byref(w)), "rimphony_last_work")
        return {"samples": int(w.samples), "passes": int(w.passes), "inner_qags": int(w.inner_qags),
                "faraday_samples": int(w.faraday_samples), "faraday_passes": int(w.faraday_passes),
                "faraday_inner_qags": int(w.faraday_inner_qags)}

    def last_tail(self):
        """Heaviest task of the last call per kernel (its chain of batches bounds the launch's tail) and the group
        kernel's sharing counters: include/rimphony_hip.h, rimphony_last_tail."""
        o = (ctypes.c_uint64 * 8)()
        capi.check(self.lib.rimphony_last_tail(self.handle, o), "rimphony_last_tail")
        return {"symphony_heaviest_batches": int(o[0]), "symphony_heaviest_row": int(o[1]),
                "faraday_heaviest_batches": int(o[2]), "faraday_heaviest_row": int(o[3]),
                "member_passes": int(o[4]), "stash_filed": int(o[5]),
                "faraday_member_passes": int(o[6]), "faraday_stash_filed": int(o[7])}

    def last_symphony_ms(self):
        ms = ctypes.c_float()
        capi.check(self.lib.rimphony_last_symphony_ms(self.handle, ctypes.byref(ms)), "rimphony_last_symphony_ms")
        return float(ms.value)

    def last_faraday_ms(self):
        ms = ctypes.c_float()
        capi.check(self.lib.rimphony_last_faraday_ms(self.handle, ctypes.byref(ms)), "rimphony_last_faraday_ms")
        return float(ms.value)

    def debug_counters(self):
        arr = (ctypes.c_uint64 * 32)()
        capi.check(self.lib.rimphony_debug_counters(self.handle, arr), "rimphony_debug_counters")
        return [int(v) for v in arr]

    def heartbeat(self, task=0):
        """Diagnostics: returns a ctypes pointer to 16 host-mapped uint64 words (see rimphony_hip.h)."""
        p = ctypes.POINTER(ctypes.c_uint64)()
        capi.check(self.lib.rimphony_debug_heartbeat(self.handle, int(task), ctypes.byref(p)),
                   "rimphony_debug_heartbeat")
        return p

    def norm_batch(self, kind, params):
        dp = [self._as_dev(p) for p in params]
        n = dp[0].numel()
        out = torch.empty(n, dtype=torch.float64, device=self._dev())
        pp = (ctypes.c_void_p * len(dp))(*[ctypes.c_void_p(p.data_ptr()) for p in dp])
        capi.check(self.lib.rimphony_batch_norm_device(self.handle, kind, n, pp, ctypes.c_void_p(out.data_ptr()),
                                                       self._stream()), "rimphony_batch_norm_device")
        torch.cuda.synchronize(self._dev())
        return out.cpu().numpy()

    # -- unit seams ----------------------------------------------------------------
    def bessel_batch(self, n, x):
        dn, dx = self._as_dev(n), self._as_dev(x)
        j = torch.empty_like(dn)
        dj = torch.empty_like(dn)
        capi.check(self.lib.rimphony_bessel_batch_device(
            self.handle, dn.numel(), ctypes.c_void_p(dn.data_ptr()), ctypes.c_void_p(dx.data_ptr()),
            ctypes.c_void_p(j.data_ptr()), ctypes.c_void_p(dj.data_ptr()), self._stream()),
            "rimphony_bessel_batch_device")
        torch.cuda.synchronize(self._dev())
        return j.cpu().numpy(), dj.cpu().numpy()

    def _seam(self, entry, kind, params, scalars, arrays, n_out=1):
        """One call of a per-point seam, rimphony_<entry>_batch_device(ctx, kind, params, *scalars, count, *arrays,
        *outputs, stream): the arrays to the device, n_out outputs of their length, the call, and the results back as
        numpy arrays (one array if n_out == 1, else a tuple)."""
        name = "rimphony_%s_batch_device" % entry
        dev = [self._as_dev(a) for a in arrays]
        outs = [torch.empty_like(dev[0]) for _ in range(n_out)]
        capi.check(getattr(self.lib, name)(
            self.handle, kind, (ctypes.c_double * len(params))(*params), *scalars, dev[0].numel(),
            *[ctypes.c_void_p(t.data_ptr()) for t in dev + outs], self._stream()), name)
        torch.cuda.synchronize(self._dev())
        res = tuple(t.cpu().numpy() for t in outs)
        return res[0] if n_out == 1 else res

    def gamma_integrand_batch(self, kind, params, coeff, stokes, s, theta, n, gamma):
        return self._seam("gamma_integrand", kind, params, (int(coeff), int(stokes), s, theta), (n, gamma))

    def gamma_integral_batch(self, kind, params, coeff, stokes, negative_lobe, s, theta, n):
        return self._seam("gamma_integral", kind, params, (int(coeff), int(stokes), int(negative_lobe), s, theta), (n,))

    def n_integral_batch(self, kind, params, coeff, stokes, negative_lobe, s, theta, n_lo, n_hi):
        """diagnostic_symphony_n_integral over arrays of [n_lo, n_hi] ranges of one parameter point."""
        return self._seam("n_integral", kind, params, (int(coeff), int(stokes), int(negative_lobe), s, theta), (n_lo, n_hi))

    def deriv_probe_batch(self, kind, params, coeff, stokes, negative_lobe, s, theta, n_start):
        """gsl::deriv_central as n_integration drives it (symphony.rs:238-240): d(gamma_integral)/dn at each n_start."""
        return self._seam("deriv_probe", kind, params, (int(coeff), int(stokes), int(negative_lobe), s, theta), (n_start,))

    def gamma_contribution_batch(self, kind, params, coeff, stokes, s, theta, gamma):
        """diagnostic_symphony_gamma_contribution over an array of gammas of one parameter point."""
        return self._seam("gamma_contribution", kind, params, (int(coeff), int(stokes), s, theta), (gamma,))

    def calc_f_batch(self, kind, params, gamma, cos_xi, norm=None):
        """DistributionFunction::calc_f and calc_f_derivatives (lib.rs:111-146) of one distribution over arrays:
        returns (f, dfdg, dfdcx).  norm=None uses the distribution's own normalisation."""
        return self._seam("calc_f", kind, params, (float("nan") if norm is None else float(norm),), (gamma, cos_xi), n_out=3)

    def hey_element_batch(self, kind, params, stokes, s, theta, qr, fixed, v):
        """Heyvaerts inner integrand (h/f element, quasi-resonant if qr) of one parameter point over arrays."""
        return self._seam("hey_element", kind, params, (int(stokes), s, theta, int(qr)), (fixed, v))

    def hey_outer_batch(self, kind, params, stokes, s, theta, qr, u):
        """Heyvaerts outer integrand (one inner integral per abscissa) of one parameter point over an array."""
        return self._seam("hey_outer", kind, params, (int(stokes), s, theta, int(qr)), (u,))

    def qag_selftest(self, family, p0, p1, a, b, epsabs, epsrel, limit):
        fam = torch.as_tensor(family, dtype=torch.int32).to(self._dev()).contiguous()
        d = [self._as_dev(v) for v in (p0, p1, a, b)]
        n = fam.numel()
        res = torch.empty(n, dtype=torch.float64, device=self._dev())
        err = torch.empty(n, dtype=torch.float64, device=self._dev())
        qst = torch.empty(n, dtype=torch.int32, device=self._dev())
        size = torch.empty(n, dtype=torch.int32, device=self._dev())
        capi.check(self.lib.rimphony_qag_selftest_device(
            self.handle, n, ctypes.c_void_p(fam.data_ptr()), *[ctypes.c_void_p(v.data_ptr()) for v in d],
            epsabs, epsrel, int(limit), ctypes.c_void_p(res.data_ptr()), ctypes.c_void_p(err.data_ptr()),
            ctypes.c_void_p(qst.data_ptr()), ctypes.c_void_p(size.data_ptr()), self._stream()),
            "rimphony_qag_selftest_device")
        torch.cuda.synchronize(self._dev())
        return res.cpu().numpy(), err.cpu().numpy(), qst.cpu().numpy(), size.cpu().numpy()


def compute_batch_multi(ctxs, kind, s, theta, params, coeff_mask=SLOTS_ALL, want_status=False, want_work=False):
    """The in-process multi-GPU batch (rimphony_batch_compute_multi): host arrays in, row i evaluated by
    ctxs[i mod len(ctxs)], numpy [n, 8] out (+ status, + work).  The table does not depend on len(ctxs)."""
    lib = capi.load()
    s = np.ascontiguousarray(s, dtype=np.float64)
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    params = [np.ascontiguousarray(p, dtype=np.float64) for p in params]
    n = s.size
    if theta.size != n or any(p.size != n for p in params):
        raise ValueError("s, theta and every parameter array must have one element per point")
    if len(params) != NPARAMS[kind]:
        raise ValueError("distribution kind %d takes %d parameter arrays" % (kind, NPARAMS[kind]))
    dp = ctypes.POINTER(ctypes.c_double)
    out = np.empty((n, 8), dtype=np.float64)
    status = np.empty((n, 8), dtype=np.int32) if want_status else None
    work = np.empty((n, 8), dtype=np.uint64) if want_work else None
    handles = (ctypes.c_void_p * len(ctxs))(*[c.handle for c in ctxs])
    pp = (dp * len(params))(*[p.ctypes.data_as(dp) for p in params])
    capi.check(lib.rimphony_batch_compute_multi(
        handles, len(ctxs), kind, n, s.ctypes.data_as(dp), theta.ctypes.data_as(dp), pp, coeff_mask, 0,
        out.ctypes.data_as(dp),
        status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if want_status else None,
        work.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)) if want_work else None), "rimphony_batch_compute_multi")
    ret = [out] + ([status] if want_status else []) + ([work] if want_work else [])
    return ret[0] if len(ret) == 1 else tuple(ret)


def compute_batch_multi_device(ctxs, kind, shards, coeff_mask=SLOTS_ALL, want_status=False, synchronize=True):
    """rimphony_batch_compute_multi_device: device buffers per context.  shards[r] = (s, theta, [params...]) as torch
    tensors on ctxs[r]'s device; returns the per-context [n_r, 8] output tensors (+ status tensors)."""
    import torch
    lib = capi.load()
    n_ctx = len(ctxs)
    dp = ctypes.POINTER(ctypes.c_double)
    np_k = NPARAMS[kind]
    outs, stats, keep = [], [], []
    n_local = (ctypes.c_size_t * n_ctx)()
    d_s, d_th, d_out = (ctypes.c_void_p * n_ctx)(), (ctypes.c_void_p * n_ctx)(), (ctypes.c_void_p * n_ctx)()
    d_par = (ctypes.POINTER(ctypes.c_void_p) * n_ctx)()
    d_st = (ctypes.c_void_p * n_ctx)()
    streams = (ctypes.c_void_p * n_ctx)()
    for r, (c, (s, th, params)) in enumerate(zip(ctxs, shards)):
        if len(params) != np_k:
            raise ValueError("distribution kind %d takes %d parameter arrays" % (kind, np_k))
        n = s.numel()
        n_local[r] = n
        out = torch.empty((n, 8), dtype=torch.float64, device=s.device)
        st = torch.empty((n, 8), dtype=torch.int32, device=s.device) if want_status else None
        arr = (ctypes.c_void_p * np_k)(*[p.data_ptr() for p in params])
        keep.append(arr)
        d_s[r], d_th[r], d_out[r] = s.data_ptr(), th.data_ptr(), out.data_ptr()
        d_par[r] = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
        d_st[r] = st.data_ptr() if want_status else None
        streams[r] = torch.cuda.current_stream(s.device).cuda_stream
        outs.append(out)
        stats.append(st)
    handles = (ctypes.c_void_p * n_ctx)(*[c.handle for c in ctxs])
    capi.check(lib.rimphony_batch_compute_multi_device(handles, n_ctx, kind, n_local, d_s, d_th, d_par, coeff_mask, 0, d_out,
                                                       d_st if want_status else None, None, streams, 1 if synchronize else 0),
               "rimphony_batch_compute_multi_device")
    return (outs, stats) if want_status else outs


class RcclComm:
    """An RCCL communicator made through the library's own own run-time-loaded librccl (rimphony_rccl_*): what a host that is not
    Python would use for the gather of the output table.  One per rank; rank 0 makes the 128-byte id."""

    def __init__(self, ctx, rank, world, unique_id):
        lib = capi.load()
        self.ctx, self.rank, self.world = ctx, rank, world
        self.handle = ctypes.c_void_p()
        capi.check(lib.rimphony_rccl_comm_create(ctx.handle, rank, world, unique_id, ctypes.byref(self.handle)),
                   "rimphony_rccl_comm_create")

    @staticmethod
    def available():
        return bool(capi.load().rimphony_rccl_available())

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        capi.check(capi.load().rimphony_rccl_unique_id(buf), "rimphony_rccl_unique_id")
        return buf

    def gather_table(self, shard, n_total, root=0, scratch=None):
        """shard: this rank's [m, 8] float64 device tensor (rows rank, rank + world, ... of the table); returns the
        [n_total, 8] table on the root, None elsewhere."""
        import torch
        table = torch.empty((n_total, 8), dtype=torch.float64, device=shard.device) if self.rank == root else None
        capi.check(capi.load().rimphony_rccl_gather_table(
            self.ctx.handle, self.handle, self.rank, self.world, root, n_total, ctypes.c_void_p(shard.data_ptr()),
            ctypes.c_void_p(table.data_ptr()) if table is not None else None,
            ctypes.c_void_p(scratch.data_ptr()) if scratch is not None else None,
            ctypes.c_void_p(torch.cuda.current_stream(shard.device).cuda_stream)), "rimphony_rccl_gather_table")
        return table

    def close(self):
        if self.handle:
            capi.load().rimphony_rccl_comm_destroy(self.handle)
            self.handle = ctypes.c_void_p()


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


# ---------------------------------------------------------------------------------
# distribution builders + calculators, named as in the reference
# ---------------------------------------------------------------------------------

class FullSynchrotronCalculator:
    """lib.rs:230-247.  One parameter point; every call is a 1-point batch."""

    def __init__(self, kind, params, ctx=None):
        self.kind = kind
        self.params = [float(p) for p in params]
        self.ctx = ctx or default_context()

    def _run(self, s, theta, mask):
        out = self.ctx.compute_batch(self.kind, [s], [theta], [[p] for p in self.params], mask)
        return out[0]

    def compute_dimensionless(self, coeff, stokes, s, theta):
        coeff, stokes = Coefficient(coeff), Stokes(stokes)
        if coeff == Coefficient.Faraday and stokes == Stokes.I:
            return float("nan")          # lib.rs:239-240
        k = slot_of(coeff, stokes)
        return float(self._run(s, theta, 1 << k)[k])

    def compute_cgs(self, coeff, stokes, nu, b, n_e, theta):
        nu_c = ELECTRON_CHARGE * b / (TWO_PI * MASS_ELECTRON * SPEED_LIGHT)
        val = self.compute_dimensionless(coeff, stokes, nu / nu_c, theta)
        if Coefficient(coeff) == Coefficient.Emission:
            return val * n_e * nu
        return val * n_e / nu

    def compute_all_dimensionless(self, s, theta):
        return np.array(self._run(s, theta, SLOTS_ALL))

    def compute_all_cgs(self, nu, b, n_e, theta):
        nu_c = ELECTRON_CHARGE * b / (TWO_PI * MASS_ELECTRON * SPEED_LIGHT)
        v = self.compute_all_dimensionless(nu / nu_c, theta)
        scale = np.array([n_e * nu if c == Coefficient.Emission else n_e / nu for c, _ in SLOTS])
        return v * scale


class HighFrequencyApproximation:
    """SynchrotronCalculator over the closed-form high-frequency approximations
    (power_law.rs:131-170, thermal_juettner.rs:92-142): (Faraday, Q) and (Faraday, V); anything else is NaN."""

    def __init__(self, kind, params, ctx=None):
        if kind not in (POWER_LAW, THERMAL_JUETTNER):
            raise ValueError("the reference defines high-frequency approximations for power_law and thermal_juettner only")
        self.kind = kind
        self.params = [float(p) for p in params]
        self.ctx = ctx or default_context()

    def compute_dimensionless(self, coeff, stokes, s, theta):
        if int(coeff) != int(Coefficient.Faraday) or int(stokes) == int(Stokes.I):
            return float("nan")
        out = self.ctx.highfreq_batch(self.kind, np.array([s], dtype=np.float64), np.array([theta], dtype=np.float64),
                                      [np.array([p], dtype=np.float64) for p in self.params])
        return float(out[0, 0 if int(stokes) == int(Stokes.Q) else 1])


class _DistributionFunction:
    """The DistributionFunction trait (lib.rs:111-146).  `norm` mirrors the public field of the reference's structs:
    None until set, in which case calc_f uses the normalisation full_calculation would compute."""
    norm = None
    ctx = None

    def _kind_params(self):
        raise NotImplementedError

    def _calc(self, gamma, cos_xi):
        kind, params = self._kind_params()
        g, c = np.atleast_1d(np.asarray(gamma, dtype=np.float64)), np.atleast_1d(np.asarray(cos_xi, dtype=np.float64))
        g, c = np.broadcast_arrays(g, c)
        out = (self.ctx or default_context()).calc_f_batch(kind, params, np.ascontiguousarray(g), np.ascontiguousarray(c),
                                                           self.norm)
        return out if np.ndim(gamma) or np.ndim(cos_xi) else tuple(float(v[0]) for v in out)

    def calc_f(self, gamma, cos_xi):
        return self._calc(gamma, cos_xi)[0]

    def calc_f_derivatives(self, gamma, cos_xi):
        _, dfdg, dfdcx = self._calc(gamma, cos_xi)
        return dfdg, dfdcx


class PowerLawDistribution(_DistributionFunction):
    def _kind_params(self):
        return POWER_LAW, [self.p, self.gamma_min, self.gamma_max, self.gamma_cutoff]

    def __init__(self, p):
        self.p, self.gamma_min, self.gamma_max, self.gamma_cutoff = float(p), 1.0, 1e12, 1e10

    def gamma_limits(self, gamma_min, gamma_max, gamma_cutoff):
        self.gamma_min, self.gamma_max, self.gamma_cutoff = float(gamma_min), float(gamma_max), float(gamma_cutoff)
        return self

    def full_calculation(self, ctx=None):
        return FullSynchrotronCalculator(POWER_LAW, [self.p, self.gamma_min, self.gamma_max, self.gamma_cutoff], ctx)

    def high_freq_approximation(self, ctx=None):
        return HighFrequencyApproximation(POWER_LAW, [self.p, self.gamma_min, self.gamma_max, self.gamma_cutoff], ctx)


class ThermalJuettnerDistribution(_DistributionFunction):
    def _kind_params(self):
        return THERMAL_JUETTNER, [self.t]

    def __init__(self, t):
        self.t = float(t)

    def full_calculation(self, ctx=None):
        return FullSynchrotronCalculator(THERMAL_JUETTNER, [self.t], ctx)

    def high_freq_approximation(self, ctx=None):
        return HighFrequencyApproximation(THERMAL_JUETTNER, [self.t], ctx)


class PitchyPowerLawDistribution(_DistributionFunction):
    def _kind_params(self):
        return PITCHY_PL, [self.p, self.k, self.gamma_min, self.gamma_max, self.gamma_cutoff]

    def __init__(self, p, k):
        self.p, self.k = float(p), float(k)
        self.gamma_min, self.gamma_max, self.gamma_cutoff = 1.0, 1e12, 1e10

    def gamma_limits(self, gamma_min, gamma_max, gamma_cutoff):
        self.gamma_min, self.gamma_max, self.gamma_cutoff = float(gamma_min), float(gamma_max), float(gamma_cutoff)
        return self

    def full_calculation(self, ctx=None):
        return FullSynchrotronCalculator(
            PITCHY_PL, [self.p, self.k, self.gamma_min, self.gamma_max, self.gamma_cutoff], ctx)


class PitchyKappaDistribution(_DistributionFunction):
    def _kind_params(self):
        return PITCHY_KAPPA, [self.kappa, self.width, self.k, self._gamma_cutoff]

    def __init__(self, kappa, width, k):
        self.kappa, self.width, self.k, self._gamma_cutoff = float(kappa), float(width), float(k), 1e10

    def gamma_cutoff(self, gamma_cutoff):
        self._gamma_cutoff = float(gamma_cutoff)
        return self

    def full_calculation(self, ctx=None):
        return FullSynchrotronCalculator(PITCHY_KAPPA, [self.kappa, self.width, self.k, self._gamma_cutoff], ctx)


class TabulatedDistribution(_DistributionFunction):
    """A distribution given as a table: log_n [n_nodes] = ln n(gamma) at nodes uniform in ln gamma from gamma_lo
    to gamma_hi (n = dN/dgamma up to a factor; f = norm n / (gamma^2 beta) inside the table, 0 outside).  The library
    interpolates with the natural cubic spline in (ln gamma, ln n).  Isotropic, unless log_g [n_mu] = ln g(mu) at nodes
    uniform in mu = cos xi from -1 to +1 gives it a pitch-angle factor: f = norm n g / (gamma^2 beta), the natural cubic
    spline in (mu, ln g) (Context.set_tables).  sin_k, a number in [0, 100], multiplies it by sin^k xi in closed form.
    The object installs its table as the context's table
    set whenever it computes, so two of them can share a context in turn; a batch over several tables uses
    Context.set_tables and kind TABULATED directly."""

    def __init__(self, gamma_lo, gamma_hi, log_n, log_g=None, sin_k=None):
        self.gamma_lo, self.gamma_hi = float(gamma_lo), float(gamma_hi)
        self.log_n, self.log_g = check_pitch_tables(
            self.gamma_lo, self.gamma_hi, np.asarray(log_n, dtype=np.float64).reshape(1, -1),
            None if log_g is None else np.asarray(log_g, dtype=np.float64).reshape(1, -1))
        self.sin_k = None if sin_k is None else check_sin_k(sin_k, 1)

    @classmethod
    def from_function(cls, fn, gamma_lo, gamma_hi, n_nodes=4096, pitch_fn=None, n_mu=257, sin_k=None):
        """Tabulate n(gamma) = fn(gamma) (vectorised, positive) on n_nodes nodes uniform in ln gamma and, if given,
        g(mu) = pitch_fn(mu) (vectorised, positive) on n_mu nodes uniform in mu from -1 to +1; sin_k as in the constructor."""
        gamma = np.exp(np.linspace(math.log(gamma_lo), math.log(gamma_hi), int(n_nodes)))
        gamma[0], gamma[-1] = gamma_lo, gamma_hi
        log_g = None
        if pitch_fn is not None:
            log_g = np.log(np.asarray(pitch_fn(np.linspace(-1.0, 1.0, int(n_mu))), dtype=np.float64))
        return cls(gamma_lo, gamma_hi, np.log(np.asarray(fn(gamma), dtype=np.float64)), log_g, sin_k)

    def _install(self, ctx):
        ctx.set_tables(self.gamma_lo, self.gamma_hi, self.log_n, self.log_g, self.sin_k)
        return ctx

    def _kind_params(self):
        return TABULATED, [0.0]

    def _calc(self, gamma, cos_xi):
        self._install(self.ctx or default_context())
        return super()._calc(gamma, cos_xi)

    def full_calculation(self, ctx=None):
        return _TabulatedCalculator(self, ctx)


class TabulatedDistribution2D(TabulatedDistribution):
    """A distribution given as a surface: log_n [n_nodes][n_mu] = ln n(gamma, mu) at nodes uniform in ln gamma from
    gamma_lo to gamma_hi and uniform in mu = cos xi from -1 to +1; f = norm exp(S(ln gamma, mu)) / (gamma^2 beta) inside
    the table, 0 outside, S the tensor-product natural cubic spline (Context.set_tables_2d).  It need not be a product
    n(gamma) g(mu).  sin_k, a number in [0, 100], multiplies it by sin^k xi in closed form: log_n is then the smooth
    remainder ln(n / sin^k xi).  ends chooses the ends of the spline as for Context.set_tables_2d: "not-a-knot" for a surface
    curved at mu = +-1.  Installs its table whenever it computes, as TabulatedDistribution does."""

    def __init__(self, gamma_lo, gamma_hi, log_n, sin_k=None, ends=None):
        self.gamma_lo, self.gamma_hi = float(gamma_lo), float(gamma_hi)
        log_n = np.asarray(log_n, dtype=np.float64)
        if log_n.ndim != 2:
            raise ValueError("log_n: expected one table, [n_nodes][n_mu]")
        self.log_n = check_tables_2d(self.gamma_lo, self.gamma_hi, log_n)
        self.sin_k = None if sin_k is None else check_sin_k(sin_k, 1)
        self.ends = check_ends(ends)

    @classmethod
    def from_function(cls, fn, gamma_lo, gamma_hi, n_nodes=512, n_mu=65, sin_k=None, ends=None):
        """Tabulate n(gamma, mu) = fn(gamma[:, None], mu[None, :]) (vectorised, positive) on n_nodes nodes uniform in
        ln gamma and n_mu nodes uniform in mu from -1 to +1.  With sin_k, fn gives the smooth remainder n / sin^k xi."""
        gamma = np.exp(np.linspace(math.log(gamma_lo), math.log(gamma_hi), int(n_nodes)))
        gamma[0], gamma[-1] = gamma_lo, gamma_hi
        mu = np.linspace(-1.0, 1.0, int(n_mu))
        n = np.broadcast_to(np.asarray(fn(gamma[:, None], mu[None, :]), dtype=np.float64), (int(n_nodes), int(n_mu)))
        return cls(gamma_lo, gamma_hi, np.log(n), sin_k, ends)

    def _install(self, ctx):
        ctx.set_tables_2d(self.gamma_lo, self.gamma_hi, self.log_n, self.sin_k, self.ends)
        return ctx


class TabulatedDistributionGrid(TabulatedDistribution):
    """A distribution given as a table on gamma nodes of its own: log_n [n_nodes] = ln n at the strictly increasing
    gamma [n_nodes] (Context.set_tables_grid); f = norm n sin^k xi g / (gamma^2 beta) between the end nodes, 0 outside, the
    natural cubic spline in (ln gamma, ln n) on the given nodes.  log_g and sin_k as for TabulatedDistribution.  Installs
    its table whenever it computes, as TabulatedDistribution does."""

    def __init__(self, gamma, log_n, log_g=None, sin_k=None):
        self.gamma, self.log_n, self.log_g = check_grid_tables(
            gamma, np.asarray(log_n, dtype=np.float64).reshape(1, -1),
            None if log_g is None else np.asarray(log_g, dtype=np.float64).reshape(1, -1))
        self.gamma_lo, self.gamma_hi = float(self.gamma[0]), float(self.gamma[-1])
        self.sin_k = None if sin_k is None else check_sin_k(sin_k, 1)

    @classmethod
    def from_function(cls, fn, gamma, pitch_fn=None, n_mu=257, sin_k=None):
        """Tabulate n(gamma) = fn(gamma) (vectorised, positive) at the given nodes and, if given, g(mu) = pitch_fn(mu)
        (vectorised, positive) on n_mu nodes uniform in mu from -1 to +1; sin_k as in the constructor."""
        gamma = np.asarray(gamma, dtype=np.float64)
        log_g = None
        if pitch_fn is not None:
            log_g = np.log(np.asarray(pitch_fn(np.linspace(-1.0, 1.0, int(n_mu))), dtype=np.float64))
        return cls(gamma, np.log(np.asarray(fn(gamma), dtype=np.float64)), log_g, sin_k)

    def _install(self, ctx):
        ctx.set_tables_grid(self.gamma, self.log_n, self.log_g, self.sin_k)
        return ctx


class TabulatedDistribution2DGrid(TabulatedDistribution):
    """A distribution given as a surface on gamma nodes of its own: log_n [n_nodes][n_mu] = ln n(gamma_i, mu_j) at the
    strictly increasing gamma [n_nodes] and at mu nodes uniform from -1 to +1 (Context.set_tables_2d_grid);
    f = norm exp(S(ln gamma, mu)) / (gamma^2 beta) between the end nodes, 0 outside, S the tensor-product natural cubic
    spline on the given nodes.  sin_k and ends as for TabulatedDistribution2D.  Installs its table whenever it computes, as
    TabulatedDistribution does."""

    def __init__(self, gamma, log_n, sin_k=None, ends=None):
        log_n = np.asarray(log_n, dtype=np.float64)
        if log_n.ndim != 2:
            raise ValueError("log_n: expected one table, [n_nodes][n_mu]")
        self.gamma, self.log_n = check_tables_2d_grid(gamma, log_n)
        self.gamma_lo, self.gamma_hi = float(self.gamma[0]), float(self.gamma[-1])
        self.sin_k = None if sin_k is None else check_sin_k(sin_k, 1)
        self.ends = check_ends(ends)

    @classmethod
    def from_function(cls, fn, gamma, n_mu=65, sin_k=None, ends=None):
        """Tabulate n(gamma, mu) = fn(gamma[:, None], mu[None, :]) (vectorised, positive) at the given gamma nodes and
        n_mu nodes uniform in mu from -1 to +1.  With sin_k, fn gives the smooth remainder n / sin^k xi."""
        gamma = np.asarray(gamma, dtype=np.float64)
        mu = np.linspace(-1.0, 1.0, int(n_mu))
        n = np.broadcast_to(np.asarray(fn(gamma[:, None], mu[None, :]), dtype=np.float64), (gamma.shape[0], int(n_mu)))
        return cls(gamma, np.log(n), sin_k, ends)

    def _install(self, ctx):
        ctx.set_tables_2d_grid(self.gamma, self.log_n, self.sin_k, self.ends)
        return ctx


class TabulatedDistribution2DNodes(TabulatedDistribution):
    """A distribution given as a surface on gamma nodes and mu nodes of its own: log_n [n_nodes][n_mu] = ln n(gamma_i,
    mu_j) at the strictly increasing gamma [n_nodes] and mu [n_mu], mu from exactly -1 to exactly +1
    (Context.set_tables_2d_nodes); f = norm exp(S(ln gamma, mu)) / (gamma^2 beta) between the end gamma nodes, 0 outside,
    S the tensor-product natural cubic spline on the given nodes.  sin_k and ends as for TabulatedDistribution2D.  Installs
    its table whenever it computes, as TabulatedDistribution does."""

    def __init__(self, gamma, mu, log_n, sin_k=None, ends=None):
        log_n = np.asarray(log_n, dtype=np.float64)
        if log_n.ndim != 2:
            raise ValueError("log_n: expected one table, [n_nodes][n_mu]")
        self.gamma, self.mu, self.log_n = check_tables_2d_nodes(gamma, mu, log_n)
        self.gamma_lo, self.gamma_hi = float(self.gamma[0]), float(self.gamma[-1])
        self.sin_k = None if sin_k is None else check_sin_k(sin_k, 1)
        self.ends = check_ends(ends)

    @classmethod
    def from_function(cls, fn, gamma, mu, sin_k=None, ends=None):
        """Tabulate n(gamma, mu) = fn(gamma[:, None], mu[None, :]) (vectorised, positive) at the given gamma and mu nodes.
        With sin_k, fn gives the smooth remainder n / sin^k xi."""
        gamma = np.asarray(gamma, dtype=np.float64)
        mu = np.asarray(mu, dtype=np.float64)
        n = np.broadcast_to(np.asarray(fn(gamma[:, None], mu[None, :]), dtype=np.float64), (gamma.shape[0], mu.shape[0]))
        return cls(gamma, mu, np.log(n), sin_k, ends)

    def _install(self, ctx):
        ctx.set_tables_2d_nodes(self.gamma, self.mu, self.log_n, self.sin_k, self.ends)
        return ctx


class TabulatedFamily:
    """A family of tabulated distributions with a continuous parameter: log_n [n_tables][n_nodes] = ln n(gamma) at nodes
    uniform in ln gamma from gamma_lo to gamma_hi, table i belonging to the value param[i] of whatever the tables were
    stored by (a time, a temperature, a magnetisation); sin_k optionally one sin^k xi exponent per table
    (Context.set_tables_family).  Between two tables the library blends ln n -- and k -- LINEARLY IN THE INDEX, and
    index() maps a value to the index piecewise linearly in param.  The blend is therefore exact where ln n is linear in
    param: a power law stored by p, sin^k xi stored by k.  ln n of a Juettner shape is linear in 1 / T, not in T: to be
    exact there, space param in 1 / T (param = 1 / T of each table) and ask for at(1 / T).  param None: the index itself.

    A batch over many rows installs the family once and passes x = family.index(values) as the one parameter array of kind
    TABULATED; at(value) is the one-point object with the reference's trait."""

    def __init__(self, gamma_lo, gamma_hi, log_n, sin_k=None, param=None):
        self.gamma_lo, self.gamma_hi = float(gamma_lo), float(gamma_hi)
        self.log_n = check_tables(self.gamma_lo, self.gamma_hi, log_n)
        n = self.log_n.shape[0]
        self.sin_k = None if sin_k is None else check_sin_k(sin_k, n)
        self.param = self._check_param(param, n)

    @staticmethod
    def _check_param(param, n):
        param = np.arange(n, dtype=np.float64) if param is None else np.ascontiguousarray(param, dtype=np.float64)
        if param.shape != (n,):
            raise ValueError("param: expected one value per table (%d), got shape %r" % (n, param.shape))
        d = np.diff(param)
        if not np.isfinite(param).all() or not ((d > 0).all() or (d < 0).all()):
            raise ValueError("param: expected finite, strictly monotonic values")
        return param

    @classmethod
    def from_function(cls, fn, gamma_lo, gamma_hi, param, n_nodes=4096, sin_k=None):
        """Tabulate n(gamma; a) = fn(gamma, a) (vectorised in gamma, positive) for every a of param on n_nodes nodes uniform
        in ln gamma; sin_k as in the constructor."""
        gamma = np.exp(np.linspace(math.log(gamma_lo), math.log(gamma_hi), int(n_nodes)))
        gamma[0], gamma[-1] = gamma_lo, gamma_hi
        param = np.atleast_1d(np.asarray(param, dtype=np.float64))
        log_n = np.stack([np.log(np.asarray(fn(gamma, float(a)), dtype=np.float64)) for a in param])
        return cls(gamma_lo, gamma_hi, log_n, sin_k, param)

    def index(self, values):
        """The real index of each value: piecewise linear in param.  ValueError for a value outside param (or a NaN)."""
        v = np.asarray(values, dtype=np.float64)
        lo, hi = min(self.param[0], self.param[-1]), max(self.param[0], self.param[-1])
        if not ((v >= lo) & (v <= hi)).all():
            raise ValueError("value outside the family's parameter range [%r, %r]" % (lo, hi))
        n = len(self.param)
        if n == 1:
            return np.zeros_like(v)
        if self.param[0] < self.param[-1]:
            return np.interp(v, self.param, np.arange(n, dtype=np.float64))
        return np.interp(v, self.param[::-1], np.arange(n, dtype=np.float64)[::-1])

    def _install(self, ctx):
        ctx.set_tables_family(self.gamma_lo, self.gamma_hi, self.log_n, self.sin_k)
        return ctx

    def at(self, value):
        """The member of the family at `value`: full_calculation, calc_f and calc_f_derivatives, as TabulatedDistribution."""
        return _FamilyMember(self, float(self.index(float(value))))


class TabulatedFamily2D(TabulatedFamily):
    """A family of tabulated SURFACES with a continuous parameter: log_n [n_tables][n_nodes][n_mu] = ln n(gamma_i, mu_j) on the
    gamma nodes and mu nodes of TabulatedDistribution2DNodes, table i belonging to param[i]; sin_k optionally one sin^k xi
    exponent per table; ends as for Context.set_tables_2d (Context.set_tables_2d_family).  Everything else is
    TabulatedFamily's: the blend is linear in the index, index() piecewise linear in param, at(value) the one-point object.
    blend="cubic": a 4-point Lagrange cubic in param across four neighbouring tables instead (at least four tables;
    Context.set_tables_2d_family); index(), at() and the row's parameter stay as they are."""

    def __init__(self, gamma, mu, log_n, sin_k=None, param=None, ends=None, blend="linear"):
        self.gamma, self.mu, self.log_n = check_tables_2d_nodes(gamma, mu, log_n)
        n = self.log_n.shape[0]
        self.sin_k = None if sin_k is None else check_sin_k(sin_k, n)
        self.ends = check_ends(ends)
        self.param = self._check_param(param, n)
        if blend not in ("linear", "cubic"):
            raise ValueError("blend: expected 'linear' or 'cubic', got %r" % (blend,))
        if blend == "cubic" and n < 4:
            raise ValueError("log_n: the cubic blend needs at least 4 tables, got %d" % n)
        self.blend = blend

    @classmethod
    def from_function(cls, fn, gamma, mu, param, sin_k=None, ends=None, blend="linear"):
        """Tabulate n(gamma, mu; a) = fn(gamma, mu, a) (vectorised over gamma [n_nodes][1] and mu [1][n_mu], positive) for
        every a of param at the given nodes; sin_k, ends and blend as in the constructor."""
        g = check_gamma_nodes(gamma)
        m = check_mu_nodes(mu)
        param = np.atleast_1d(np.asarray(param, dtype=np.float64))
        log_n = np.stack([np.log(np.broadcast_to(np.asarray(fn(g[:, None], m[None, :], float(a)), dtype=np.float64), (len(g), len(m))))
                          for a in param])
        return cls(g, m, log_n, sin_k, param, ends, blend)

    def _install(self, ctx):
        if self.blend == "cubic":
            ctx.set_tables_2d_family(self.gamma, self.mu, self.log_n, self.sin_k, self.ends, "cubic", self.param)
        else:
            ctx.set_tables_2d_family(self.gamma, self.mu, self.log_n, self.sin_k, self.ends)
        return ctx


class _FamilyMember(_DistributionFunction):
    def __init__(self, family, x):
        self.family, self.x = family, x

    def _install(self, ctx):
        return self.family._install(ctx)

    def _kind_params(self):
        return TABULATED, [self.x]

    def _calc(self, gamma, cos_xi):
        self._install(self.ctx or default_context())
        return super()._calc(gamma, cos_xi)

    def full_calculation(self, ctx=None):
        calc = _TabulatedCalculator(self, ctx)
        calc.params = [self.x]
        return calc


class _TabulatedCalculator(FullSynchrotronCalculator):
    def __init__(self, dist, ctx=None):
        super().__init__(TABULATED, [0.0], ctx)
        self.dist = dist

    def _run(self, s, theta, mask):
        self.dist._install(self.ctx)
        return super()._run(s, theta, mask)
