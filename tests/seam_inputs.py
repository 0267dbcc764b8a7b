"""Input generators of the seam tests (test_gpu_parity.py for the analytic kinds, test_gpu_tabulated.py for kind 4):
samples inside the integration domains the reference integrates over.  Test infrastructure only."""
import math

import numpy as np


def gamma_limits(s, th, n):
    """gamma-, gamma+ of harmonic n (array): the kinematic range of the gamma integral (symphony.rs:398-437)"""
    nos = n / s
    root = np.sqrt(np.maximum(nos * nos - math.sin(th) ** 2, 0))
    gm = (nos - abs(math.cos(th)) * root) / math.sin(th) ** 2
    gp = (nos + abs(math.cos(th)) * root) / math.sin(th) ** 2
    return gm, gp


def harmonic_samples(rng, s, th, m):
    """m pairs (n, gamma): n from just above s |sin theta| + 1 to e^12 beyond it, half of them integers, gamma uniform in
    the kinematic range of its harmonic"""
    nmin = s * abs(math.sin(th))
    n = nmin + 1 + np.exp(rng.uniform(-3, 12, m))
    n = np.where(rng.random(m) < 0.5, np.floor(n), n)
    gm, gp = gamma_limits(s, th, n)
    return n, gm + (gp - gm) * rng.random(m)


def hey_qr_start(sigma0):
    """Where the quasi-resonant region begins: both pomega_max expressions of heyvaerts.rs:262-296 are real."""
    return max(sigma0, 3 ** -0.5 * sigma0 ** 1.5)


def hey_seam_inputs(rng, s, th, qr, n):
    """(fixed, v) inside the integration domains of heyvaerts.rs:213-296: non-resonant -- fixed = pomega, v = sigma in
    [sigma_min, sigma_max]; quasi-resonant -- fixed = sigma >= sigma0, v = pomega in [-pomega_max, pomega_max]."""
    sigma0 = s * math.sin(th)
    if not qr:
        pomega = rng.uniform(-1., 1., n) * np.exp(rng.uniform(math.log(3.), math.log(3e3), n)) * max(sigma0, 1.)
        smin = np.sqrt(pomega ** 2 + sigma0 ** 2)
        smax = np.maximum(3 ** -0.5 * smin ** 1.5, smin)
        return pomega, smin + (smax - smin) * rng.random(n)
    sigma = hey_qr_start(sigma0) * (1. + np.exp(rng.uniform(math.log(1e-3), math.log(3e2), n)))
    with np.errstate(invalid="ignore"):
        pmax = np.fmin(np.sqrt(3 ** (2. / 3.) * sigma ** (4. / 3.) - sigma0 ** 2), np.sqrt(sigma ** 2 - sigma0 ** 2))
    pmax = np.nan_to_num(pmax, nan=0.)
    return sigma, pmax * rng.uniform(-1., 1., n)


def hey_outer_abscissae(rng, s, th, qr, n):
    """n abscissae of the outer Faraday integrals: sigma beyond the start of the quasi-resonant region, or pomega of
    either sign"""
    sigma0 = s * math.sin(th)
    if qr:
        return hey_qr_start(sigma0) * (1. + np.exp(rng.uniform(math.log(1e-3), math.log(1e2), n)))
    return rng.uniform(-1., 1., n) * np.exp(rng.uniform(math.log(0.3), math.log(1e3), n)) * max(sigma0, 1.)
