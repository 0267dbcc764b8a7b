"""The quantity the Symphony path approximates, written from the mathematics: a plain sum over harmonics of
one-dimensional integrals of exact J_n and J'_n.  Test infrastructure only; numpy, scipy and mpmath, nothing of the project.

For f(gamma, mu), mu = cos xi, normalised so that 2 pi int dmu int dgamma gamma sqrt(gamma^2 - 1) f = 1:

    coefficient(s, theta) = P * sum_{n >= floor(s |sin theta| + 1)} G(n)
    G(n) = int_{gamma-}^{gamma+} gamma^2 pol F dgamma
    gamma+- = (n/s +- |cos theta| sqrt((n/s)^2 - sin^2 theta)) / sin^2 theta
    beta = sqrt(1 - gamma^-2);  mu = (s gamma - n) / (s gamma beta cos theta)
    M = (cos theta - beta mu) / sin theta;  N = beta sin xi;  z = s gamma beta sin theta sin xi
    pol_I = (M J_n)^2 + (N J'_n)^2;  pol_Q = (M J_n)^2 - (N J'_n)^2;  pol_V = 2 (M J_n)(N J'_n)
    F = f (emission);  F = df/dgamma + (beta cos theta - mu) / (gamma - 1/gamma) df/dmu (absorption)
    P_j = (2 pi e)^2 / (c |cos theta|);  P_alpha = -(2 pi e)^2 / (2 m_e c |cos theta|)

The roots of 1 - mu^2 in gamma are gamma+-, so sin^2 xi = sin^2 theta (gamma - gamma-)(gamma+ - gamma) / ((gamma^2 - 1) cos^2 theta);
the quadrature carries the two distances exactly instead of forming 1 - mu^2.

Each lobe [gamma-, gamma+] is cut at its midpoint (the two halves are the V lobes of the project's seam), each half is
clipped to the distribution's hard gamma limits and to the gamma beyond which gamma^3 f is below 1e-22 of its peak, and
mapped by gamma = a + (b - a) T(v), T = S o S, S(v) = sin^2(pi v / 2): T is flat to fourth order at both ends, which removes
the (1 - mu^2)^(n + k/2 - 1) endpoint behaviour of the pitch-angle kinds and places nodes geometrically away from gamma-.
v in [0, 1] is integrated by composite Gauss-Legendre; the error estimate of a value is its difference from the value at
twice the points per panel and a cut-off 1.5 times as far.

Slots are ordered as compute_batch orders them: j_I, alpha_I, j_Q, alpha_Q, j_V, alpha_V."""
import math
import os

import numpy as np
from scipy import integrate, special

E, C, ME = 4.80320680e-10, 2.99792458e10, 9.1093826e-28
PANELS, POINTS = 8, 40            # composite Gauss-Legendre in v: panels per half lobe, points per panel
CAP_FRACTION = 1e-22
SLOTS = ((0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2))     # (coefficient, Stokes) of compute_batch's first six columns


def pitch_integral(k):
    """int_0^1 sin^k xi dmu"""
    return 0.5 * math.sqrt(math.pi) * math.gamma(1. + 0.5 * k) / math.gamma(1.5 + 0.5 * k)


class Distribution:
    """Any f(gamma, mu) with its two derivatives.  The callables take (gamma, mu, xp) with xp = numpy or mpmath.mp and
    return f without its normalisation; `norm` multiplies all three.  A caller that knows sin^2 xi = 1 - mu^2 without the
    cancellation passes it as a fourth argument.  [gamma_lo, gamma_hi] are hard limits outside which
    f = 0: the integrals are split there, so the callables are never asked beyond them."""

    def __init__(self, f, dfdg, dfdmu, norm, gamma_lo=1., gamma_hi=math.inf, name="f"):
        self.f, self.dfdg, self.dfdmu, self.norm = f, dfdg, dfdmu, float(norm)
        self.gamma_lo, self.gamma_hi, self.name = float(gamma_lo), float(gamma_hi), name
        self._cap = None

    def cap(self, stretch=1.):
        """gamma beyond which gamma^3 max_mu f stays below CAP_FRACTION of its peak (never beyond gamma_hi)."""
        if self._cap is None:
            lo = max(self.gamma_lo, 1. + 1e-9)
            g = lo + np.expm1(np.linspace(0., math.log(1e9), 200001))
            g = g[g <= self.gamma_hi] if math.isfinite(self.gamma_hi) else g
            with np.errstate(all="ignore"):
                w = np.maximum.reduce([np.abs(g ** 3 * self.f(g, np.full_like(g, m), np)) for m in (-0.9, -0.5, 0., 0.5, 0.9)])
            w = np.where(np.isfinite(w), w, 0.)
            big = np.flatnonzero(w >= CAP_FRACTION * w.max())
            # f still counts at a hard upper limit: the limit itself, not the last grid point below it
            self._cap = self.gamma_hi if big[-1] == len(g) - 1 else float(g[big[-1] + 1])
        c = self.gamma_lo + (self._cap - self.gamma_lo) * stretch
        return min(c, self.gamma_hi)


def normalisation(f, gamma_lo=1., gamma_hi=math.inf):
    """1 / (2 pi int dmu int dgamma gamma sqrt(gamma^2 - 1) f) for a general f(gamma, mu, xp)."""
    def inner(mu):
        v, _ = integrate.quad(lambda g: g * math.sqrt(g * g - 1.) * float(f(g, mu, np)), gamma_lo, gamma_hi,
                              epsabs=0., epsrel=1e-12, limit=500)
        return v
    v, _ = integrate.quad(inner, -1., 1., epsabs=0., epsrel=1e-12, limit=200)
    return 1. / (2. * math.pi * v)


def _energy_norm(h, k, gamma_lo, gamma_hi):
    """1 / (4 pi int_0^1 sin^k dmu int h(gamma) dgamma), h = gamma sqrt(gamma^2 - 1) x the energy factor of f"""
    pieces = [gamma_lo] + [gamma_lo + 10. ** j for j in range(16) if gamma_lo + 10. ** j < min(gamma_hi, 1e15)] + [gamma_hi]
    v = sum(integrate.quad(h, a, b, epsabs=0., epsrel=1e-12, limit=500)[0] for a, b in zip(pieces[:-1], pieces[1:]))
    return 1. / (4. * math.pi * pitch_integral(k) * v)


def _sin2(mu, sin2):
    return 1. - mu * mu if sin2 is None else sin2


def thermal_juettner(T):
    """f = exp(-gamma / T) / (4 pi T K_2(1/T))"""
    f = lambda g, mu, xp, sin2=None: xp.exp(-g / T)
    dfdg = lambda g, mu, xp, sin2=None: -xp.exp(-g / T) / T
    dfdmu = lambda g, mu, xp, sin2=None: 0. * g
    norm = 1. / (4. * math.pi * T * special.kve(2, 1. / T) * math.exp(-1. / T))
    return Distribution(f, dfdg, dfdmu, norm, name="thermal_juettner")


def pitchy_power_law(p, k, gamma_min, gamma_max, gamma_cutoff, name="pitchy_pl"):
    """f = sin^k xi gamma^-p exp(-gamma / gamma_c) / (gamma sqrt(gamma^2 - 1)) on [gamma_min, gamma_max]"""
    def f(g, mu, xp, sin2=None):
        return _sin2(mu, sin2) ** (0.5 * k) * g ** (-p) * xp.exp(-g / gamma_cutoff) / (g * xp.sqrt(g * g - 1.))

    def dfdg(g, mu, xp, sin2=None):
        return -f(g, mu, xp, sin2) * ((p + 1.) / g + g / (g * g - 1.) + 1. / gamma_cutoff)

    def dfdmu(g, mu, xp, sin2=None):
        if k == 0.:
            return 0. * g
        return -k * mu * _sin2(mu, sin2) ** (0.5 * k - 1.) * g ** (-p) * xp.exp(-g / gamma_cutoff) / (g * xp.sqrt(g * g - 1.))

    norm = _energy_norm(lambda g: g ** (-p) * math.exp(-g / gamma_cutoff), k, gamma_min, gamma_max)
    return Distribution(f, dfdg, dfdmu, norm, gamma_min, gamma_max, name)


def power_law(p, gamma_min, gamma_max, gamma_cutoff):
    return pitchy_power_law(p, 0., gamma_min, gamma_max, gamma_cutoff, name="power_law")


def pitchy_kappa(kappa, width, k, gamma_cutoff):
    """f = sin^k xi (1 + (gamma - 1) / (kappa w))^-(kappa + 1) exp(-gamma / gamma_c)"""
    def e(g, xp):
        return (1. + (g - 1.) / (kappa * width)) ** (-(kappa + 1.)) * xp.exp(-g / gamma_cutoff)

    def f(g, mu, xp, sin2=None):
        return _sin2(mu, sin2) ** (0.5 * k) * e(g, xp)

    def dfdg(g, mu, xp, sin2=None):
        return -f(g, mu, xp, sin2) * ((kappa + 1.) / (kappa * width + g - 1.) + 1. / gamma_cutoff)

    def dfdmu(g, mu, xp, sin2=None):
        if k == 0.:
            return 0. * g
        return -k * mu * _sin2(mu, sin2) ** (0.5 * k - 1.) * e(g, xp)

    norm = _energy_norm(lambda g: g * math.sqrt(g * g - 1.) * e(g, math), k, 1., math.inf)
    return Distribution(f, dfdg, dfdmu, norm, name="pitchy_kappa")


def tilted_juettner(T, a, gamma_lo, gamma_hi):
    """A non-separable surface through the general entry: f = exp(-gamma / T + a (gamma - 1) mu) on [gamma_lo, gamma_hi],
    a cold Juettner core whose temperature depends on the pitch angle."""
    f = lambda g, mu, xp, sin2=None: xp.exp(-g / T + a * (g - 1.) * mu)
    dfdg = lambda g, mu, xp, sin2=None: f(g, mu, xp) * (a * mu - 1. / T)
    dfdmu = lambda g, mu, xp, sin2=None: f(g, mu, xp) * a * (g - 1.)
    return Distribution(f, dfdg, dfdmu, normalisation(f, gamma_lo, gamma_hi), gamma_lo, gamma_hi, "tilted_juettner")


KINDS = ("power_law", "thermal_juettner", "pitchy_pl", "pitchy_kappa")


def make(kind, params):
    """The distribution of the project's kind number (or name) and parameter list."""
    kind = KINDS[kind] if isinstance(kind, (int, np.integer)) else kind
    params = [float(p) for p in params]
    return {"power_law": power_law, "thermal_juettner": thermal_juettner, "pitchy_pl": pitchy_power_law,
            "pitchy_kappa": pitchy_kappa}[kind](*params)


# ---- G(n), double precision ---------------------------------------------------------------------------------------

_nodes_cache = {}


def _nodes(points):
    """v, 1 - ... the map T, its complement and T' w on the composite Gauss-Legendre nodes of [0, 1]"""
    if points not in _nodes_cache:
        x, w = np.polynomial.legendre.leggauss(points)
        v = np.concatenate([(i + 0.5 * (x + 1.)) / PANELS for i in range(PANELS)])
        w = np.tile(0.5 * w / PANELS, PANELS)
        s1, c1 = np.sin(0.5 * np.pi * v) ** 2, np.cos(0.5 * np.pi * v) ** 2
        T, Tc = np.sin(0.5 * np.pi * s1) ** 2, np.sin(0.5 * np.pi * c1) ** 2
        dT = 0.5 * np.pi * np.sin(np.pi * s1) * 0.5 * np.pi * np.sin(np.pi * v)
        _nodes_cache[points] = (T, Tc, dT * w)
    return _nodes_cache[points]


def gamma_limits(s, theta, n):
    sn, cs = math.sin(theta), abs(math.cos(theta))
    nos = np.asarray(n, dtype=np.float64) / s
    root = np.sqrt(nos * nos - sn * sn)
    return (nos - cs * root) / (sn * sn), (nos + cs * root) / (sn * sn)


def harmonics(dist, s, theta, n, points=POINTS, stretch=1.):
    """G(n) for an array of real n >= s |sin theta|, as [len(n), 2 coefficients, 4]: I, Q, and the two halves of V
    (upper half lobe [mid, gamma+] first, as negative_lobe = 0 of the project's seam; V = their sum)."""
    n = np.atleast_1d(np.asarray(n, dtype=np.float64))[:, None]
    sth, cth = math.sin(theta), math.cos(theta)
    gm, gp = gamma_limits(s, theta, n)
    mid = 0.5 * (gm + gp)
    lo, hi = dist.gamma_lo, dist.cap(stretch)
    T, Tc, w = _nodes(points)
    out = np.zeros((len(n), 2, 4))
    for half, (a0, b0) in enumerate(((mid, gp), (gm, mid))):
        a, b = np.maximum(a0, lo), np.minimum(b0, hi)
        empty = b <= a
        a, b = np.where(empty, mid, a), np.where(empty, mid, b)
        g = a + (b - a) * T
        d_minus = (a - gm) + (b - a) * T
        d_plus = (gp - b) + (b - a) * Tc
        wt = (b - a) * w
        g2m1 = ((a - 1.) + (b - a) * T) * (g + 1.)        # (gamma - 1)(gamma + 1): gamma- = 1 when n = s
        with np.errstate(all="ignore"):
            sin2 = np.clip(sth * sth * d_minus * d_plus / (g2m1 * cth * cth), 0., 1.)
            sin_xi = np.sqrt(sin2)
            gb = np.sqrt(g2m1)
            mu = np.clip((s * g - n) / (s * gb * cth), -1., 1.)
            beta = gb / g
            z = s * gb * sth * sin_xi
            nn = np.broadcast_to(n, z.shape)
            mj = (cth - beta * mu) / sth * special.jv(nn, z)
            njp = beta * sin_xi * special.jvp(nn, z)
            f0 = dist.f(g, mu, np)
            f1 = dist.dfdg(g, mu, np) + (beta * cth - mu) * g / g2m1 * dist.dfdmu(g, mu, np)
        for c, F in enumerate((f0, f1)):
            # a node whose mu rounds to +-1 gives df/dmu = inf for k < 2; the integrand there is O(sin^(2n + k - 2) xi) -> 0
            F = np.where((wt > 0.) & np.isfinite(F), g * g * F * wt, 0.)
            i, q, v = (mj * mj + njp * njp) * F, (mj * mj - njp * njp) * F, 2. * mj * njp * F
            out[:, c, 0] += i.sum(axis=1)
            out[:, c, 1] += q.sum(axis=1)
            out[:, c, 2 + half] = v.sum(axis=1)
    return out * dist.norm


def harmonics_with_error(dist, s, theta, n, capped=True):
    """G(n) and the error estimate: the difference from twice the points per panel and a cut-off 1.5 times as far.
    capped=False integrates up to gamma+ or the hard limit: a single harmonic held on its own scale, however small it is
    beside the sum, must not lose its upper part."""
    a = harmonics(dist, s, theta, n, POINTS, 1. if capped else math.inf)
    b = harmonics(dist, s, theta, n, 2 * POINTS, 1.5 if capped else math.inf)
    return b, np.abs(a - b)


def prefactors(theta):
    tpe = 2. * math.pi * E
    ac = abs(math.cos(theta))
    return np.array([tpe * tpe / (C * ac), -tpe * tpe / (2. * ME * C * ac)])


def _slots(g):
    """[.., 2, 4] of harmonics() -> [.., 6] in slot order"""
    g = np.asarray(g)
    return np.stack([g[..., c, st] if st < 2 else g[..., c, 2] + g[..., c, 3] for c, st in SLOTS], axis=-1)


def coefficients(dist, s, theta, chunk=48, max_harmonics=6000, allow_truncated=False):
    """The harmonic sum for the six Symphony slots.  Ends after 40 consecutive harmonics whose terms are all below 1e-13 of
    the running sums, or, if allow_truncated, after max_harmonics (otherwise that is an error).  Returns (value[6], error estimate[6], number of harmonics, share[6] of the sum carried by n >= 30)."""
    n0 = int(math.floor(s * abs(math.sin(theta)) + 1.))
    total, err, high = np.zeros(6), np.zeros(6), np.zeros(6)
    small, count, n = 0, 0, n0
    while small < 40 and count < max_harmonics:
        ns = np.arange(n, n + chunk, dtype=np.float64)
        g, e = harmonics_with_error(dist, s, theta, ns)
        g, e = _slots(g), _slots(e)
        for i in range(chunk):
            total += g[i]
            err += e[i]
            if ns[i] >= 30.:
                high += g[i]
            count += 1
            # (leading harmonics may underflow to 0 before the sum has begun: those do not count as closing terms)
            small = small + 1 if total.any() and (np.abs(g[i]) <= 1e-13 * np.abs(total)).all() else 0
            if small >= 40:
                break
        n += chunk
    if small < 40 and not allow_truncated:
        raise RuntimeError("harmonic sum of %s at s = %g, theta = %g did not end" % (dist.name, s, theta))
    p = prefactors(theta)[[c for c, _ in SLOTS]]
    with np.errstate(all="ignore"):
        share = np.abs(high / total)
    return total * p, err * np.abs(p), count, share


# ---- the same at 40 digits (mpmath), to check the double-precision one ---------------------------------------------------

def harmonic_mp(dist, s, theta, n, digits=40):
    """G(n) as [2, 4] floats, every operation in mpmath at `digits` digits (tanh-sinh on the same pieces)."""
    from mpmath import mp
    with mp.workdps(digits):
        s_, th, n_ = mp.mpf(s), mp.mpf(theta), mp.mpf(n)
        sth, cth = mp.sin(th), mp.cos(th)
        nos = n_ / s_
        root = mp.sqrt(nos * nos - sth * sth)
        gm, gp = (nos - abs(cth) * root) / sth ** 2, (nos + abs(cth) * root) / sth ** 2
        mid = (gm + gp) / 2
        lo, hi = mp.mpf(dist.gamma_lo), mp.mpf(dist.cap(1.5))

        def integrand(c, st):
            def fn(g):
                g2m1 = g * g - 1
                gb = mp.sqrt(g2m1)
                sin2 = sth * sth * (g - gm) * (gp - g) / (g2m1 * cth * cth)
                if sin2 <= mp.mpf(10) ** (5 - digits):        # 1 - mu^2 is not resolved; the integrand is O(sin^2 xi) at most
                    return mp.mpf(0)
                sin_xi = mp.sqrt(sin2)
                mu = (s_ * g - n_) / (s_ * gb * cth)
                beta = gb / g
                z = s_ * gb * sth * sin_xi
                mj = (cth - beta * mu) / sth * mp.besselj(n_, z)
                njp = beta * sin_xi * mp.besselj(n_, z, derivative=1)
                pol = mj * mj + njp * njp if st == 0 else (mj * mj - njp * njp if st == 1 else 2 * mj * njp)
                if c == 0:
                    F = dist.f(g, mu, mp)
                else:
                    F = dist.dfdg(g, mu, mp) + (beta * cth - mu) / (g - 1 / g) * dist.dfdmu(g, mu, mp)
                return g * g * pol * F
            return fn

        out = np.zeros((2, 4))
        for half, (a0, b0) in enumerate(((mid, gp), (gm, mid))):
            a, b = max(a0, lo), min(b0, hi)
            if b <= a:
                continue
            cuts = [a + (b - a) * mp.mpf(t) for t in (0, 0.02, 0.1, 0.3, 0.6, 1)]
            for c in range(2):
                vals = [mp.quad(integrand(c, st), cuts) for st in range(3)]
                out[c, 0] += float(vals[0] * dist.norm)
                out[c, 1] += float(vals[1] * dist.norm)
                out[c, 2 + half] = float(vals[2] * dist.norm)
        return out


def coefficients_mp(dist, s, theta, digits=40, n_harmonics=None):
    """The harmonic sum from harmonic_mp: the first n_harmonics terms, or the same ending rule.  For cold points only
    (every harmonic costs seconds)."""
    n = int(math.floor(s * abs(math.sin(theta)) + 1.))
    total, small, count = np.zeros(6), 0, 0
    while small < 40 and (n_harmonics is None or count < n_harmonics):
        g = _slots(harmonic_mp(dist, s, theta, n, digits))
        total += g
        small = small + 1 if total.any() and (np.abs(g) <= 1e-13 * np.abs(total)).all() else 0
        n, count = n + 1, count + 1
    return total * prefactors(theta)[[c for c, _ in SLOTS]], count


# ---- the stored fixture (tools/make_exact_symphony_fixture.py) -----------------------------------------------------------

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_symphony.npz")


def load_fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def row_inputs(fix, rows):
    """s, theta and the parameter columns (as compute_batch takes them) of the given rows, all of one kind"""
    rows = np.asarray(rows)
    npar = int(fix["row_nparams"][rows[0]])
    return fix["row_s"][rows], fix["row_theta"][rows], [fix["row_params"][rows, j].copy() for j in range(npar)]


def group_inputs(fix, g):
    """kind, parameter list, s, theta of a single-harmonic group"""
    return int(fix["grp_kind"][g]), [float(v) for v in fix["grp_params"][g, :fix["grp_nparams"][g]]], float(fix["grp_s"][g]), float(fix["grp_theta"][g])


def deviation(got, exact):
    return np.abs(np.asarray(got) / exact - 1.)


def surface_inputs(fix):
    """(T, a, gamma_lo, gamma_hi, n_nodes, n_mu) of the stored tabulated surface"""
    T, a, lo, hi, nn, nmu = fix["surf_params"]
    return float(T), float(a), float(lo), float(hi), int(nn), int(nmu)
