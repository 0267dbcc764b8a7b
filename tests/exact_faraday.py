"""The quantity the Heyvaerts path approximates, written from the mathematics: the two-dimensional integrals of Heyvaerts'
non-resonant and quasi-resonant elements, by fixed Gauss-Legendre rules on exact Bessel functions.  Test infrastructure only;
numpy, scipy and mpmath, the distributions of tests/exact_symphony.py, nothing of the project.

For f(gamma, mu), mu = cos xi, at s = nu / nu_B and observer angle theta, with c = cos theta and

    sigma0 = s sin theta,  t = sigma0 sin theta,  x^2 = sigma^2 - pomega^2 - sigma0^2,  R = pomega^2 + sigma0^2
    gamma = (sigma - pomega c) / t
    (t p)^2 = (sigma c - pomega)^2 + sin^2 theta x^2          (p^2 = gamma^2 - 1, a sum of squares: no cancellation)
    mu = (sigma c - pomega) / (t p),  sin^2 xi = sin^2 theta x^2 / (t p)^2
    d mu / d sigma = sin^2 theta (c x^2 - sigma (sigma c - pomega)) / (t p)^3
    df/dsigma = df/dgamma / t + (d mu / d sigma) df/dmu

    rho_Q, rho_V = 2 e^2 (NR + QR) / (m_e sigma0^2)
    NR = int dpomega int_{sqrt R}^{R^(3/4) / sqrt 3} dsigma  E_nr           (empty where R < 9)
    QR = int_{sigma >= max(sigma0, sigma0^(3/2) / sqrt 3)} dsigma int_{|pomega| <= min(sqrt(3^(2/3) sigma^(4/3) - sigma0^2), sqrt(sigma^2 - sigma0^2))} dpomega  E_qr

Non-resonant elements, r = sigma^2 / R, a1 = 1/8 - 5 r / 24, a2 = 3/128 - 77 r / 576 + 385 r^2 / 3456, b = -5 sigma^2 x^2 / (12 R^2):

    Q:  (pi / c_l) (2 [(6 a2 - a1^2 + b) R^(-1/2) + a1 x^2 R^(-3/2) - x^4 R^(-5/2) / 8] - sigma0^2 (6 a2 - a1^2) R^(-3/2)) df/dsigma
    V:  -(2 pi / c_l) pomega [x^2 R^(-3/2) / 2 + (6 a2 + b - a1^2) / R + 3 a1 x^2 / (2 R^2)] df/dsigma

Quasi-resonant elements, g = (sqrt 8 / 3) (sigma - x)^(3/2) / sqrt x, q = (sigma - x) / x, D_nu = I_(-nu)(g) - I_nu(g) = (2 / pi) sin(nu pi) K_nu(g)
(the difference is taken from K_nu: the same function without the cancellation), S_nu = I_(-nu)(g) + I_nu(g):

    Q:  (1 / c_l) (pi^2 x^2 Y1 + pi^2 pomega^2 Y2 - pi (2 pomega^2 + sigma0^2) / sqrt R) df/dsigma
          g < 10:  Y1 = (4 / sqrt 27) q^2 D_(2/3) S_(2/3),  Y2 = (2 / sqrt 27) q D_(1/3) S_(1/3)
          else:    Y1 = J'_sigma(x) Y'_sigma(x),             Y2 = -J_sigma(x) Y_sigma(x)
    V:  -(2 pi / c_l) pomega (pi Y - 1) df/dsigma
          g < 10:  Y = g D_(2/3) S_(1/3) / sqrt 3;   else:  Y = -x J'_sigma(x) Y_sigma(x)

A distribution's hard gamma limits are straight lines in the (sigma, pomega) plane; df/dsigma is taken as 0 beyond them, with no
delta function on them, which is what the project computes.  The infinite ranges end at the line gamma = Distribution.cap.

Quadrature.  An inner integral is cut at the roots of g = 10 (quasi-resonant, sigma below 3.0...: the universal root of
g = 10 on the physical limit) and clipped to the gamma limits; each piece [a, b] is mapped by a + (b - a) F(v), F = T o T with
T = S o S, S = sin^2(pi v / 2), flat to sixteenth order at both ends: x^2 is linear in the distance from an end on the curve
x = 0, the elements carry non-integer powers of it down to x^(k - 2) of the pitch-angle kinds and x^(-2 sigma) of Y_sigma, and
the distance itself is carried exactly next to the node.  An outer integral is cut at every point where the inner one changes
its make-up -- pomega = +-sqrt(9 - sigma0^2), sigma = 3, the root named above, where x at pomega = 0 reaches the g = 10 value,
where a gamma limit meets an end of the inner range or the g = 10 curve, through the point gamma = 1 (pomega = s cos theta on
sigma = s, where mu has no limit) -- and at a geometric ladder of points; each piece
is mapped by T.  v in [0, 1] is integrated by composite Gauss-Legendre.  Nothing adapts and nothing marches.  The error estimate
of a value is its difference from the value at twice the points per panel and a cut-off 1.5 times as far.

An mpmath twin at 20 to 30 digits serves a handful of points: element_mp, inner_integral_mp and coefficients_mp, which state the
elements, every limit of the domain, the cuts and the final factor a second time.  full_kernel_coefficients is a recorded study,
not a reference for any test: the J_sigma / Y_sigma kernel over the whole domain, with and without its principal-value part.

Stokes parameters are numbered as in the project: 1 = Q, 2 = V; compute_batch's slots 6 and 7 are rho_Q and rho_V."""
import math
import os

import numpy as np
from scipy import optimize, special

from exact_symphony import C, E, ME, Distribution, make       # noqa: F401 (Distribution and make are part of this module's interface)

STOKES_Q, STOKES_V = 1, 2
SQRT3 = math.sqrt(3.)
T23 = 3. ** (2. / 3.)
G_CUT = 10.
INNER = (8, 24)          # panels, points per panel of an inner piece
OUTER = (2, 24)          # of an outer piece
LADDER = 2.              # ratio of the geometric ladder of outer cuts


def qr_g(sigma, x):
    return math.sqrt(8.) / 3. * (sigma - x) ** 1.5 / np.sqrt(x)


def _x_edge(sigma):
    """x on the physical limit pomega^2 + sigma0^2 = 3^(2/3) sigma^(4/3)"""
    return math.sqrt(sigma * sigma - T23 * sigma ** (4. / 3.))


SIGMA_G10 = optimize.brentq(lambda sg: qr_g(sg, _x_edge(sg)) - G_CUT, 3. + 1e-9, 4., xtol=1e-15, rtol=1e-15)


class Geometry:
    def __init__(self, s, theta):
        self.s, self.theta = float(s), float(theta)
        self.sth, self.cth = math.sin(theta), math.cos(theta)
        self.sigma0 = self.s * self.sth
        self.sigma0_sq = self.sigma0 * self.sigma0
        self.t = self.sigma0 * self.sth

    def gamma(self, sigma, pomega):
        return (sigma - pomega * self.cth) / self.t


# ---- the elements ----------------------------------------------------------------------------------------------------

def dfdsigma(dist, geo, sigma, pomega, x2, mu_term=True, xp=np):
    sc = sigma * geo.cth - pomega
    tp2 = sc * sc + geo.sth * geo.sth * x2
    tp = xp.sqrt(tp2)
    gamma = (sigma - pomega * geo.cth) / geo.t
    mu = sc / tp
    sin2 = geo.sth * geo.sth * x2 / tp2
    out = dist.norm * dist.dfdg(gamma, mu, xp, sin2) / geo.t
    if mu_term:
        dmu = geo.sth * geo.sth * (geo.cth * x2 - sigma * sc) / (tp2 * tp)
        out = out + dist.norm * dmu * dist.dfdmu(gamma, mu, xp, sin2)
    return out


def _nr_kernel(stokes, geo, sigma, pomega, x2):
    R = pomega * pomega + geo.sigma0_sq
    r = sigma * sigma / R
    a1 = 1. / 8. - 5. / 24. * r
    a2 = 3. / 128. - 77. / 576. * r + 385. / 3456. * r * r
    b = -5. / 12. * sigma * sigma * x2 / (R * R)
    if stokes == STOKES_Q:
        t1 = (6. * a2 - a1 * a1 + b) * R ** -0.5 + a1 * x2 * R ** -1.5 - x2 * x2 * R ** -2.5 / 8.
        return math.pi / C * (2. * t1 - geo.sigma0_sq * (6. * a2 - a1 * a1) * R ** -1.5)
    z = 0.5 * x2 * R ** -1.5 + (6. * a2 + b - a1 * a1) / R + 1.5 * a1 * x2 / (R * R)
    return -2. * math.pi / C * z * pomega


def _qr_kernel(stokes, geo, sigma, pomega, x2):
    """numpy only.  The two forms are evaluated where they apply."""
    sigma, pomega, x2 = np.broadcast_arrays(sigma, pomega, x2)
    x = np.sqrt(x2)
    with np.errstate(all="ignore"):
        g = qr_g(sigma, x)
    low = g < G_CUT
    y1, y2 = np.zeros(x.shape), np.zeros(x.shape)
    if low.any():
        gl, q = g[low], (sigma[low] - x[low]) / x[low]
        i13, i23 = special.iv(1. / 3., gl), special.iv(2. / 3., gl)
        d13 = SQRT3 / math.pi * special.kv(1. / 3., gl)          # (2 / pi) sin(pi / 3) K
        d23 = SQRT3 / math.pi * special.kv(2. / 3., gl)
        s13, s23 = d13 + 2. * i13, d23 + 2. * i23
        if stokes == STOKES_Q:
            y1[low] = 4. / math.sqrt(27.) * q * q * d23 * s23
            y2[low] = 2. / math.sqrt(27.) * q * d13 * s13
        else:
            y1[low] = gl * d23 * s13 / SQRT3
    high = ~low
    if high.any():
        sg, xh = sigma[high], x[high]
        with np.errstate(all="ignore"):
            if stokes == STOKES_Q:
                y1[high] = special.jvp(sg, xh) * special.yvp(sg, xh)
                y2[high] = -special.jv(sg, xh) * special.yv(sg, xh)
            else:
                y1[high] = -xh * special.jvp(sg, xh) * special.yv(sg, xh)
    if stokes == STOKES_Q:
        R = pomega * pomega + geo.sigma0_sq
        return (math.pi ** 2 * x2 * y1 + math.pi ** 2 * pomega * pomega * y2 - math.pi * (2. * pomega * pomega + geo.sigma0_sq) / np.sqrt(R)) / C
    return -2. * math.pi / C * pomega * (math.pi * y1 - 1.)


def element(dist, stokes, s, theta, qr, fixed, v, mu_term=True):
    """The inner integrand: the quasi-resonant element at sigma = fixed, pomega = v, or the non-resonant one at
    pomega = fixed, sigma = v.  0 beyond the distribution's hard limits."""
    geo = Geometry(s, theta)
    fixed, v = np.broadcast_arrays(np.asarray(fixed, dtype=np.float64), np.asarray(v, dtype=np.float64))
    sigma, pomega = (fixed, v) if qr else (v, fixed)
    x2 = sigma * sigma - pomega * pomega - geo.sigma0_sq
    kern = (_qr_kernel if qr else _nr_kernel)(stokes, geo, sigma, pomega, x2)
    gamma = geo.gamma(sigma, pomega)
    inside = (gamma >= dist.gamma_lo) & (gamma <= dist.gamma_hi)
    with np.errstate(all="ignore"):
        return np.where(inside, kern * dfdsigma(dist, geo, sigma, pomega, x2, mu_term), 0.)


# ---- the maps and rules ------------------------------------------------------------------------------------------------

_rule_cache = {}


def _S(v):
    return np.sin(0.5 * np.pi * v) ** 2


def _dT(v, vc):
    """T'(v) with vc = 1 - v known exactly"""
    return 0.25 * np.pi ** 2 * np.sin(np.pi * np.minimum(_S(v), _S(vc))) * np.sin(np.pi * np.minimum(v, vc))


def _rule(panels, points, depth):
    """(M, 1 - M, M' w) on the composite Gauss-Legendre nodes of [0, 1] for the map M = T (depth 1) or T o T (depth 2)"""
    key = (panels, points, depth)
    if key not in _rule_cache:
        x, w = np.polynomial.legendre.leggauss(points)
        half = 0.5 * (x + 1.)
        v = np.concatenate([(i + half) / panels for i in range(panels)])
        vc = np.concatenate([(panels - 1 - i + (1. - half)) / panels for i in range(panels)])
        w = np.tile(0.5 * w / panels, panels)
        m, mc, dm = _S(_S(v)), _S(_S(vc)), _dT(v, vc)
        if depth == 2:
            dm = dm * _dT(m, mc)
            m, mc = _S(_S(m)), _S(_S(mc))
        _rule_cache[key] = (m, mc, dm * w)
    return _rule_cache[key]


def _roots(fn, a, b, n=2001):
    """the sign changes of a vectorised fn on [a, b], from a grid uniform in the square root of the distance from a"""
    if not b > a:
        return []
    u = a + (b - a) * np.linspace(0., 1., n) ** 2
    with np.errstate(all="ignore"):
        f = fn(u)
    out = []
    for i in np.flatnonzero(np.isfinite(f[:-1]) & np.isfinite(f[1:]) & (np.sign(f[:-1]) * np.sign(f[1:]) < 0.)):
        out.append(optimize.brentq(lambda z: float(fn(np.array([z]))[0]), u[i], u[i + 1], xtol=1e-300, rtol=1e-15))
    return out


# ---- the inner integrals ---------------------------------------------------------------------------------------------------

def _x10(sigma):
    """x at which g(sigma, x) = 10 (g falls with x on (0, sigma)), by bisection"""
    lo, hi = np.zeros_like(sigma), sigma.copy()
    for _ in range(64):
        mid = 0.5 * (lo + hi)
        with np.errstate(all="ignore"):
            above = qr_g(sigma, mid) > G_CUT
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return 0.5 * (lo + hi)


def _qr_limits(geo, sigma):
    """(pomega_max, the value sqrt(sigma^2 - sigma0^2) on which x = 0, pomega at which g = 10 within [0, pomega_max])"""
    wq2 = np.maximum((sigma - geo.sigma0) * (sigma + geo.sigma0), 0.)
    wq = np.sqrt(wq2)
    wp2 = T23 * sigma ** (4. / 3.) - geo.sigma0_sq
    wmax = np.where(wp2 < wq2, np.sqrt(np.maximum(wp2, 0.)), wq)
    w10 = np.sqrt(np.maximum(wq2 - _x10(sigma) ** 2, 0.))
    w10 = np.where(sigma < SIGMA_G10, np.minimum(w10, wmax), wmax)
    return wmax, wq, w10


def _clip_pomega(geo, sigma, glo, ghi):
    """the range of pomega at fixed sigma on which glo <= gamma <= ghi"""
    c = geo.cth
    with np.errstate(all="ignore"):
        if c > 0.:
            return (sigma - ghi * geo.t) / c, (sigma - glo * geo.t) / c
        if c < 0.:
            return (sigma - glo * geo.t) / c, (sigma - ghi * geo.t) / c
    ok = (sigma >= glo * geo.t) & (sigma <= ghi * geo.t)
    return np.where(ok, -np.inf, np.inf), np.where(ok, np.inf, -np.inf)


def _inner_qr(dist, stokes, geo, sigma, points, ghi, mu_term=True):
    sigma = np.atleast_1d(np.asarray(sigma, dtype=np.float64))[:, None]
    wmax, wq, w10 = _qr_limits(geo, sigma)
    clo, chi = _clip_pomega(geo, sigma, dist.gamma_lo, ghi)
    M, Mc, w = _rule(INNER[0], points, 2)
    total = np.zeros(len(sigma))
    for a0, b0 in ((-wmax, -w10), (-w10, w10), (w10, wmax)):
        a, b = np.maximum(a0, clo), np.minimum(b0, chi)
        empty = ~(b > a)
        a, b = np.where(empty, a0, a), np.where(empty, a0, b)
        pomega = a + (b - a) * M
        x2 = ((wq - b) + (b - a) * Mc) * ((a + wq) + (b - a) * M)
        with np.errstate(all="ignore"):
            val = _qr_kernel(stokes, geo, sigma, pomega, x2) * dfdsigma(dist, geo, sigma, pomega, x2, mu_term)
        wt = (b - a) * w
        with np.errstate(all="ignore"):
            total += np.where((wt > 0.) & np.isfinite(val), val * wt, 0.).sum(axis=1)
    return total


def _inner_nr(dist, stokes, geo, pomega, points, ghi, mu_term=True):
    pomega = np.atleast_1d(np.asarray(pomega, dtype=np.float64))[:, None]
    smin = np.sqrt(pomega * pomega + geo.sigma0_sq)
    smax = smin ** 1.5 / SQRT3
    with np.errstate(all="ignore"):
        a, b = np.maximum(smin, dist.gamma_lo * geo.t + pomega * geo.cth), np.minimum(smax, ghi * geo.t + pomega * geo.cth)
    empty = ~(b > a) | ~(smax > smin)
    a, b = np.where(empty, smin, a), np.where(empty, smin, b)
    M, Mc, w = _rule(INNER[0], points, 2)
    sigma = a + (b - a) * M
    x2 = ((a - smin) + (b - a) * M) * (sigma + smin)
    with np.errstate(all="ignore"):
        val = _nr_kernel(stokes, geo, sigma, pomega, x2) * dfdsigma(dist, geo, sigma, pomega, x2, mu_term)
    wt = (b - a) * w
    with np.errstate(all="ignore"):
        return np.where((wt > 0.) & np.isfinite(val), val * wt, 0.).sum(axis=1)


def inner_integral(dist, stokes, s, theta, qr, u, mu_term=True):
    """One outer-integrand sample, the Faraday counterpart of a single harmonic: the integral of the element over pomega at
    sigma = u (qr) or over sigma at pomega = u, up to the distribution's hard limits only.  Returns (values, error estimates)
    for an array u."""
    geo = Geometry(s, theta)
    fn = _inner_qr if qr else _inner_nr
    a = fn(dist, stokes, geo, u, INNER[1], dist.gamma_hi, mu_term)
    b = fn(dist, stokes, geo, u, 2 * INNER[1], dist.gamma_hi, mu_term)
    return b, np.abs(a - b)


# ---- the outer integrals ---------------------------------------------------------------------------------------------------

def _ladder(origin, scale, end):
    """origin + scale (LADDER^j - 1) up to end (scale may be negative)"""
    out, j = [], 1
    while abs(scale) * (LADDER ** j - 1.) < abs(end - origin) and j < 200:
        out.append(origin + scale * (LADDER ** j - 1.))
        j += 1
    return out


def qr_outer_cuts(dist, geo, ghi):
    """sorted points at which the quasi-resonant outer integrand is cut, from its lower limit to where gamma > ghi everywhere"""
    lo = max(geo.sigma0, geo.sigma0 ** 1.5 / SQRT3)
    top = ghi * geo.t / (1. - abs(geo.cth)) * (1. + 1e-12) + 1e-12
    if not top > lo:
        return []
    cuts = [lo, top] + [z for z in (3., SIGMA_G10, geo.s) if lo < z < top]       # (sigma, pomega) = s (1, cos theta) is gamma = 1
    lims = [g for g in (dist.gamma_lo, ghi) if g > 1.]

    for lim in lims:          # where a gamma limit meets an end of the inner range (0) or the g = 10 curve (2)
        for sign in (-1., 1.):
            cuts += _roots(lambda sg: geo.gamma(sg, sign * _qr_limits(geo, sg)[0]) - lim, lo, top)
            if lo < SIGMA_G10:
                cuts += _roots(lambda sg: geo.gamma(sg, sign * _qr_limits(geo, sg)[2]) - lim, lo, min(top, SIGMA_G10))
    if lo < SIGMA_G10:        # where g = 10 is reached at pomega = 0
        cuts += _roots(lambda sg: _x10(sg) ** 2 - (sg - geo.sigma0) * (sg + geo.sigma0), lo, min(top, SIGMA_G10))
    cuts += _ladder(lo, 0.5 * geo.sigma0, top)
    return sorted(set(cuts))


def nr_outer_cuts(dist, geo, ghi):
    p = math.sqrt(ghi * ghi - 1.)
    left, right = geo.s * (ghi * geo.cth - p), geo.s * (ghi * geo.cth + p)
    cuts = [left, right, 0., geo.s * geo.cth]
    if geo.sigma0 < 3.:
        cuts += [-math.sqrt(9. - geo.sigma0_sq), math.sqrt(9. - geo.sigma0_sq)]
    smin = lambda w: np.sqrt(w * w + geo.sigma0_sq)
    for lim in (g for g in (dist.gamma_lo, ghi) if g > 1.):
        for curve in (smin, lambda w: smin(w) ** 1.5 / SQRT3):
            for a, b in ((left, 0.), (0., right)):
                cuts += _roots(lambda w: geo.gamma(curve(w), w) - lim, a, b)
    cuts += _ladder(0., geo.sigma0, right) + _ladder(0., -geo.sigma0, left)
    return sorted(z for z in set(cuts) if left <= z <= right)


def _outer(inner, cuts, points):
    """sum over the pieces between consecutive cuts of the T-mapped composite rule on inner(array of abscissae)"""
    if len(cuts) < 2:
        return 0.
    M, Mc, w = _rule(OUTER[0], points, 1)
    a, b = np.array(cuts[:-1])[:, None], np.array(cuts[1:])[:, None]
    u = np.where(M < 0.5, a + (b - a) * M, b - (b - a) * Mc)
    val = inner(u.ravel()).reshape(u.shape)
    return float((val * (b - a) * w).sum())


def parts(dist, stokes, s, theta, points=1, stretch=1., mu_term=True):
    """(NR, QR) at `points` times the standard points per panel and the cut-off `stretch` times as far"""
    geo = Geometry(s, theta)
    ghi = dist.cap(stretch)
    nr = _outer(lambda w: _inner_nr(dist, stokes, geo, w, points * INNER[1], ghi, mu_term), nr_outer_cuts(dist, geo, ghi), points * OUTER[1])
    qr = _outer(lambda sg: _inner_qr(dist, stokes, geo, sg, points * INNER[1], ghi, mu_term), qr_outer_cuts(dist, geo, ghi), points * OUTER[1])
    return nr, qr


def scale(s, theta):
    return 2. * E * E / (ME * (s * math.sin(theta)) ** 2)


def coefficients(dist, s, theta, mu_term=True):
    """(rho_Q, rho_V), their error estimates, and the (NR, QR) parts of each: arrays [2], [2], [2, 2]"""
    val, err, split = np.zeros(2), np.zeros(2), np.zeros((2, 2))
    for i, stokes in enumerate((STOKES_Q, STOKES_V)):
        a = parts(dist, stokes, s, theta, 1, 1., mu_term)
        b = parts(dist, stokes, s, theta, 2, 1.5, mu_term)
        val[i], err[i], split[i] = sum(b), abs(sum(a) - sum(b)), b
    return val * scale(s, theta), err * scale(s, theta), split * scale(s, theta)


# ---- recorded study: the J_sigma / Y_sigma kernel over the whole domain (no test asserts on it) -----------------------------

def _full_kernels(stokes, geo, sigma, pomega, x2):
    """(kernel with the true Y_sigma, its principal-value part without the factor cot(pi sigma)): the J/Y form of the
    quasi-resonant elements at every point of the domain.  Y_sigma = J_sigma cot(pi sigma) - J_(-sigma) / sin(pi sigma); the first
    term has a pole at every integer sigma and its integral over sigma is a principal value."""
    sigma, pomega, x2 = np.broadcast_arrays(sigma, pomega, x2)
    x = np.sqrt(x2)
    with np.errstate(all="ignore"):
        j, y, dj, dy = special.jv(sigma, x), special.yv(sigma, x), special.jvp(sigma, x), special.yvp(sigma, x)
        if stokes == STOKES_Q:
            R = pomega * pomega + geo.sigma0_sq
            full = (math.pi ** 2 * (x2 * dj * dy - pomega * pomega * j * y) - math.pi * (2. * pomega * pomega + geo.sigma0_sq) / np.sqrt(R)) / C
            pv = math.pi ** 2 * (x2 * dj * dj - pomega * pomega * j * j) / C
        else:
            full = -2. * math.pi / C * pomega * (-math.pi * x * dj * y - 1.)
            pv = 2. * math.pi ** 2 / C * pomega * x * dj * j
    return full, pv


def _full_inner(dist, stokes, geo, sigma, points, ghi):
    """the integrals over |pomega| <= sqrt(sigma^2 - sigma0^2) of both kernels times df/dsigma, and the sum of the weights
    |dominant term x df/dsigma| of nodes left out because J_sigma underflows or Y_sigma overflows: [n], [n], [n]"""
    sigma = np.atleast_1d(np.asarray(sigma, dtype=np.float64))[:, None]
    wq = np.sqrt(np.maximum((sigma - geo.sigma0) * (sigma + geo.sigma0), 0.))
    clo, chi = _clip_pomega(geo, sigma, dist.gamma_lo, ghi)
    a, b = np.maximum(-wq, clo), np.minimum(wq, chi)
    empty = ~(b > a)
    a, b = np.where(empty, -wq, a), np.where(empty, -wq, b)
    M, Mc, w = _rule(INNER[0], points, 2)
    pomega = a + (b - a) * M
    x2 = ((wq - b) + (b - a) * Mc) * ((a + wq) + (b - a) * M)
    with np.errstate(all="ignore"):
        full, pv = _full_kernels(stokes, geo, sigma, pomega, x2)
        d = dfdsigma(dist, geo, sigma, pomega, x2) * (b - a) * w
        ok = ((b - a) * w > 0.) & np.isfinite(full * d) & np.isfinite(pv * d)
        dominant = np.abs(pomega) / C * np.abs(d)
        return (np.where(ok, full * d, 0.).sum(axis=1), np.where(ok, pv * d, 0.).sum(axis=1),
                np.where(~ok & ((b - a) * w > 0.) & np.isfinite(dominant), dominant, 0.).sum(axis=1))


def full_kernel_parts(dist, stokes, s, theta, ghi, points=1):
    """(integral with the true Y_sigma, principal-value integral of the cot(pi sigma) term, weight left out) over
    sigma >= sigma0, gamma <= ghi.  The first on the pieces of a geometric ladder; the second cell by cell around every integer n:
    PV int cot(pi sigma) H dsigma = int_0^h cot(pi u) (H(n + u) - H(n - u)) du, h = 1/2 or the distance to sigma0, plus plain pieces."""
    geo = Geometry(s, theta)
    lo, top = geo.sigma0, ghi * geo.t / (1. - abs(geo.cth))
    inner = lambda sg: _full_inner(dist, stokes, geo, sg, points * INNER[1], ghi)
    M, Mc, w = _rule(OUTER[0], points * OUTER[1], 1)
    cuts = sorted(set([lo, top] + [z for z in [geo.s] + _ladder(lo, 0.5 * geo.sigma0, top) if lo < z < top]))
    a, b = np.array(cuts[:-1])[:, None], np.array(cuts[1:])[:, None]
    u = np.where(M < 0.5, a + (b - a) * M, b - (b - a) * Mc)
    f, _, lost = inner(u.ravel())
    full = float((f.reshape(u.shape) * (b - a) * w).sum())
    lost = float((lost.reshape(u.shape) * (b - a) * w).sum())
    # the principal value
    first = math.floor(lo) + 1.
    h0 = min(0.5, first - lo)
    plain = [(lo, first - 0.5)] if first - lo > 0.5 else [(first + h0, first + 0.5)]
    pv = 0.
    for pa, pb in plain:
        if pb > pa:
            up = np.where(M < 0.5, pa + (pb - pa) * M, pb - (pb - pa) * Mc)
            pv += float((inner(up)[1] / np.tan(math.pi * up) * (pb - pa) * w).sum())
    uu = h0 * M                                              # the first cell: the square-root start of H may lie at its end
    pv += float(((inner(first + uu)[1] - inner(first - np.where(M < 0.5, uu, h0 - h0 * Mc))[1]) / np.tan(math.pi * uu) * h0 * w).sum())
    n = np.arange(first + 1., math.floor(top - 0.5) + 1.)[:, None]
    x, wg = np.polynomial.legendre.leggauss(points * 12)
    ug = 0.25 * (x + 1.)
    for chunk in np.array_split(n, max(1, len(n) // 64)):
        if len(chunk):
            hp, hm = inner((chunk + ug).ravel())[1].reshape(len(chunk), -1), inner((chunk - ug).ravel())[1].reshape(len(chunk), -1)
            pv += float(((hp - hm) / np.tan(math.pi * ug) * 0.25 * wg).sum())
    return full, pv, lost


def full_kernel_coefficients(dist, s, theta, ghi):
    """(rho_Q, rho_V) with the J_sigma / Y_sigma kernel over the whole domain sigma^2 >= pomega^2 + sigma0^2, up to gamma = ghi:
    returns (with the principal-value term, without it, error estimates of both from twice the points, share of the weight left
    out), arrays [2] each.  A recorded study (tools/faraday_full_kernel_study.py); nothing asserts on it."""
    out = np.zeros((5, 2))
    for i, stokes in enumerate((STOKES_Q, STOKES_V)):
        f1, p1, _ = full_kernel_parts(dist, stokes, s, theta, ghi, 1)
        f2, p2, lost = full_kernel_parts(dist, stokes, s, theta, ghi, 2)
        out[:, i] = f2, f2 - p2, abs(f2 - f1), abs((f2 - p2) - (f1 - p1)), lost / abs(f2)
    out[:4] *= scale(s, theta)
    return out


def deviation(got, exact):
    return np.abs(np.asarray(got) / exact - 1.)


# ---- the same at 30 digits or more (mpmath), written apart from the above ----------------------------------------------------

def element_mp(dist, stokes, s, theta, qr, fixed, v, digits=30, mu_term=True):
    """The inner integrand with every operation in mpmath: I_(-nu) - I_nu as the literal difference, x^2, p^2 and 1 - mu^2 by
    their defining subtractions.  Returns an mpf (evaluate and convert inside mp.workdps(digits))."""
    from mpmath import mp
    s, theta, fixed, v = mp.mpf(s), mp.mpf(theta), mp.mpf(fixed), mp.mpf(v)
    sth, cth = mp.sin(theta), mp.cos(theta)
    sigma0 = s * sth
    t = sigma0 * sth
    sigma, pomega = (fixed, v) if qr else (v, fixed)
    x2 = sigma ** 2 - pomega ** 2 - sigma0 ** 2
    gamma = (sigma - pomega * cth) / t
    if x2 <= 0 or gamma < dist.gamma_lo or gamma > dist.gamma_hi:
        return mp.mpf(0)
    x = mp.sqrt(x2)
    p = mp.sqrt(gamma ** 2 - 1)
    mu = (sigma * cth - pomega) / (t * p)
    dfds = dist.dfdg(gamma, mu, mp) / t
    if mu_term:
        dfds += (cth / (t * p) - (sigma * cth - pomega) * gamma / (t ** 2 * p ** 3)) * dist.dfdmu(gamma, mu, mp)
    dfds *= mp.mpf(dist.norm)
    R = pomega ** 2 + sigma0 ** 2
    c_l = mp.mpf(C)
    if not qr:
        r = sigma ** 2 / R
        a1 = mp.mpf(1) / 8 - 5 * r / 24
        a2 = mp.mpf(3) / 128 - 77 * r / 576 + 385 * r ** 2 / 3456
        b = -5 * sigma ** 2 * x2 / (12 * R ** 2)
        if stokes == STOKES_Q:
            t1 = (6 * a2 - a1 ** 2 + b) / mp.sqrt(R) + a1 * x2 / R ** mp.mpf(1.5) - x2 ** 2 / R ** mp.mpf(2.5) / 8
            return mp.pi / c_l * (2 * t1 - sigma0 ** 2 * (6 * a2 - a1 ** 2) / R ** mp.mpf(1.5)) * dfds
        z = x2 / R ** mp.mpf(1.5) / 2 + (6 * a2 + b - a1 ** 2) / R + 3 * a1 * x2 / (2 * R ** 2)
        return -2 * mp.pi / c_l * z * pomega * dfds
    g = mp.sqrt(8) / 3 * (sigma - x) ** mp.mpf(1.5) / mp.sqrt(x)
    third = mp.mpf(1) / 3
    if g < G_CUT:
        m13, p13, m23, p23 = mp.besseli(-third, g), mp.besseli(third, g), mp.besseli(-2 * third, g), mp.besseli(2 * third, g)
        q = (sigma - x) / x
        if stokes == STOKES_Q:
            y1 = 4 / mp.sqrt(27) * q ** 2 * (m23 - p23) * (m23 + p23)
            y2 = 2 / mp.sqrt(27) * q * (m13 - p13) * (m13 + p13)
        else:
            y = g * (m23 - p23) * (m13 + p13) / mp.sqrt(3)
    else:
        j, y_, dj = mp.besselj(sigma, x), mp.bessely(sigma, x), mp.besselj(sigma, x, derivative=1)
        if stokes == STOKES_Q:
            y1, y2 = dj * mp.bessely(sigma, x, derivative=1), -j * y_
        else:
            y = -x * dj * y_
    if stokes == STOKES_Q:
        return (mp.pi ** 2 * x2 * y1 + mp.pi ** 2 * pomega ** 2 * y2 - mp.pi * (2 * pomega ** 2 + sigma0 ** 2) / mp.sqrt(R)) / c_l * dfds
    return -2 * mp.pi / c_l * pomega * (mp.pi * y - 1) * dfds


def _g_mp(sigma, x):
    from mpmath import mp
    return mp.sqrt(8) / 3 * (sigma - x) ** mp.mpf(1.5) / mp.sqrt(x)


def _x10_mp(sigma):
    """x in (0, sigma) at which g = 10, by bisection in mpmath (g falls with x)"""
    from mpmath import mp
    lo, hi = mp.mpf(0), mp.mpf(sigma)
    for _ in range(4 * mp.dps):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if _g_mp(sigma, mid) > G_CUT else (lo, mid)
    return (lo + hi) / 2


def _qr_limits_mp(s, theta, sigma):
    """(pomega_max, pomega at which g = 10 within [0, pomega_max]) at fixed sigma, stated again in mpmath"""
    from mpmath import mp
    sigma0 = mp.mpf(s) * mp.sin(mp.mpf(theta))
    sigma = mp.mpf(sigma)
    wq2 = sigma ** 2 - sigma0 ** 2
    wp2 = mp.cbrt(9) * mp.cbrt(sigma) ** 4 - sigma0 ** 2
    wmax = mp.sqrt(max(min(wq2, wp2), 0))
    x_end2 = wq2 - wmax ** 2                      # x^2 at pomega = +-pomega_max: 0 on the curve x = 0
    if x_end2 > 0 and _g_mp(sigma, mp.sqrt(x_end2)) < G_CUT:
        return wmax, wmax                         # the I form all the way
    w10_2 = wq2 - _x10_mp(sigma) ** 2
    return wmax, (mp.sqrt(w10_2) if w10_2 > 0 else mp.mpf(0))


def inner_integral_mp(dist, stokes, s, theta, qr, u, digits=30, mu_term=True, gamma_hi=None):
    """inner_integral of one abscissa by tanh-sinh quadrature of element_mp, with the limits of the inner range, the g = 10 cut
    and the gamma limits stated again in mpmath; each piece is cut in seven"""
    from mpmath import mp
    with mp.workdps(digits):
        s_, th, u_ = mp.mpf(s), mp.mpf(theta), mp.mpf(u)
        sigma0, cth = s_ * mp.sin(th), mp.cos(th)
        t = sigma0 * mp.sin(th)
        glo, ghi = mp.mpf(dist.gamma_lo), mp.mpf(dist.gamma_hi if gamma_hi is None else gamma_hi)
        if qr:
            wmax, w10 = _qr_limits_mp(s, theta, u)
            pieces = [(-wmax, -w10), (-w10, w10), (w10, wmax)]
            ends = sorted(((u_ - ghi * t) / cth, (u_ - glo * t) / cth)) if cth != 0 else (-mp.inf, mp.inf)
        else:
            smin = mp.sqrt(u_ ** 2 + sigma0 ** 2)
            pieces = [(smin, smin ** mp.mpf(1.5) / mp.sqrt(3))]
            ends = (glo * t + u_ * cth, ghi * t + u_ * cth)
        total = mp.mpf(0)
        for a, b in pieces:
            a, b = max(a, ends[0]), min(b, ends[1])
            if b > a:
                cuts = [a + (b - a) * mp.mpf(f) for f in (0, 0.001, 0.03, 0.3, 0.7, 0.97, 0.999, 1)]
                total += mp.quad(lambda v: element_mp(dist, stokes, s, theta, qr, u, v, digits, mu_term), cuts)
        return float(total)


def outer_pieces_mp(dist, s, theta, qr, gamma_hi, digits=20):
    """The pieces of the outer variable for coefficients_mp, with every limit stated again in mpmath.  For a distribution that is
    smooth in gamma alone (no pitch-angle factor, no hard limits inside): the limits and kinks of the domain only."""
    from mpmath import mp
    with mp.workdps(digits):
        s_, th, ghi = mp.mpf(s), mp.mpf(theta), mp.mpf(gamma_hi)
        sigma0, cth = s_ * mp.sin(th), mp.cos(th)
        t = sigma0 * mp.sin(th)
        if qr:
            lo = max(sigma0, sigma0 ** mp.mpf(1.5) / mp.sqrt(3))
            # gamma >= (sigma - |c| pomega_max) / t > ghi beyond this sigma
            top = mp.findroot(lambda sg: (sg - abs(cth) * _qr_limits_mp(s, theta, sg)[0]) / t - ghi, ghi * t / (1 - abs(cth)))
            cuts = [lo, top]
            if lo < 3:
                g10 = mp.findroot(lambda sg: _g_mp(sg, mp.sqrt(sg ** 2 - mp.cbrt(9) * mp.cbrt(sg) ** 4)) - G_CUT, mp.mpf("3.02"))
                all_jy = mp.findroot(lambda sg: _x10_mp(sg) ** 2 - (sg ** 2 - sigma0 ** 2), (lo, mp.mpf(3)), solver="anderson")
                cuts += [mp.mpf(3), g10, all_jy]
            j = 1
            while lo + sigma0 / 2 * (2 ** j - 1) < top:
                cuts.append(lo + sigma0 / 2 * (2 ** j - 1))
                j += 1
            cuts = sorted(c for c in cuts if lo <= c <= top)
            return [(float(a), float(b)) for a, b in zip(cuts[:-1], cuts[1:])]
        p = mp.sqrt(ghi ** 2 - 1)
        left, right = s_ * (ghi * cth - p), s_ * (ghi * cth + p)          # where gamma = ghi meets the curve x = 0
        cuts = [left, right]
        if sigma0 < 3:
            cuts += [-mp.sqrt(9 - sigma0 ** 2), mp.sqrt(9 - sigma0 ** 2)]
        else:
            cuts.append(mp.mpf(0))
        j = 1
        while sigma0 * (2 ** j - 1) < max(-left, right):
            cuts += [sigma0 * (2 ** j - 1), -sigma0 * (2 ** j - 1)]
            j += 1
        cuts = sorted(c for c in cuts if left <= c <= right)
        return [(float(a), float(b)) for a, b in zip(cuts[:-1], cuts[1:])
                if not (sigma0 < 3 and abs(a + b) / 2 < mp.sqrt(9 - sigma0 ** 2))]          # the empty non-resonant region


def _mp_sample(job):
    kind, params, stokes, s, theta, qr, u, digits, gamma_hi = job
    return inner_integral_mp(make(kind, params), stokes, s, theta, qr, u, digits, True, gamma_hi)


def coefficients_mp(kind, params, s, theta, digits=20, points=24, stretch=1.5, pool_map=map):
    """(rho_Q, rho_V) of make(kind, params) from the mpmath twin: inner integrals by inner_integral_mp, the outer domain by outer_pieces_mp, the factor
    2 e^2 / (m_e sigma0^2) in mpmath; per outer piece a Gauss-Legendre rule of `points` points under u = a + (b - a)(3 v^2 - 2 v^3),
    which makes the square-root starts of the outer integrand analytic.  Hundreds of inner integrals of seconds each: pass a
    process pool's map."""
    from mpmath import mp
    dist = make(kind, params)
    ghi = dist.cap(stretch)
    x, w = np.polynomial.legendre.leggauss(points)
    v = 0.5 * (x + 1.)
    jobs, weights = [], []
    for stokes in (STOKES_Q, STOKES_V):
        for qr in (0, 1):
            for a, b in outer_pieces_mp(dist, s, theta, qr, ghi, digits):
                for vi, wi in zip(v, w):
                    jobs.append((kind, list(params), stokes, s, theta, qr, a + (b - a) * (3. * vi * vi - 2. * vi ** 3), digits, ghi))
                    weights.append((stokes, 0.5 * wi * (b - a) * 6. * vi * (1. - vi)))
    vals = list(pool_map(_mp_sample, jobs))
    out = []
    with mp.workdps(digits):
        factor = 2 * mp.mpf(E) ** 2 / (mp.mpf(ME) * (mp.mpf(s) * mp.sin(mp.mpf(theta))) ** 2)
        for stokes in (STOKES_Q, STOKES_V):
            out.append(float(factor * mp.fsum(mp.mpf(val) * mp.mpf(wt) for val, (st, wt) in zip(vals, weights) if st == stokes)))
    return np.array(out)


# ---- the stored fixture (tools/make_exact_faraday_fixture.py) -----------------------------------------------------------------

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "exact_faraday.npz")
SLOTS = (6, 7)          # compute_batch's columns of rho_Q and rho_V; the mask of both
MASK = 0xC0


def load_fixture():
    with np.load(FIXTURE) as f:
        return {k: f[k] for k in f.files}


def row_params(fix, row):
    return [float(v) for v in fix["row_params"][row, :fix["row_nparams"][row]]]


def row_inputs(fix, rows):
    """s, theta and the parameter columns (as compute_batch takes them) of the given rows, all of one kind"""
    rows = np.asarray(rows)
    npar = int(fix["row_nparams"][rows[0]])
    return fix["row_s"][rows], fix["row_theta"][rows], [fix["row_params"][rows, j].copy() for j in range(npar)]
