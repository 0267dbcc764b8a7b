#!/usr/bin/env python3
"""What the ends of the spline of a 2-D table set do to its accuracy, measured with the table oracle of the choice of ends
(tests/support/liboracle_tab2dends.so: the host build of the library's own solver and of the device functions): the
measurement of profiles/tabulated_2d_ends_accuracy.txt.

1. What the host tests assert (tests/test_tabulated_2d_ends_host.py takes ten times these figures as its bounds): how well
   cubics come back, how far the solver is from scipy.interpolate.CubicSpline, how well the normalisation of a surface
   quadratic in mu meets its closed form -- each with natural ends beside it.
2. An anisotropic relativistic Maxwellian, n = gamma^2 beta exp(-(gamma - 1)(1 + 0.5 mu^2) / 3): ln n quadratic in mu with a
   coefficient that grows with gamma, so not separable.  256 gamma nodes uniform in ln(gamma - 1) from 1 + 1e-4 to 200, times
   8, 16 and 64 mu nodes uniform in mu, the ends along mu natural and not-a-knot (natural along gamma, where the table is what
   it is).  The worst error of f, df/dgamma and df/dmu against the closed form through the calc_f seam, and the eight
   coefficients at theta = 0.9, s = 3, 10, 30 against a 256 x 512 table with natural ends as the converged statement.
3. The coefficient comparison again with exp(1.5 mu) in place of mu^2: no polynomial, so not-a-knot ends are O(h^4) and not
   exact.

CPU only; about a minute.  usage: tab_2d_ends_accuracy.py > profiles/tabulated_2d_ends_accuracy.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_ends_bind as te  # noqa: E402
from rimphony_amd import api  # noqa: E402

THETA_E, ANISO = 3.0, 0.5
G_LO, G_HI, N_GAMMA = 1.0 + 1e-4, 200.0, 256
N_MU = (8, 16, 64)
REF_MU = 512
S_VALUES, THETA = (3.0, 10.0, 30.0), 0.9
SLOTS = ("j_I", "alpha_I", "j_Q", "alpha_Q", "j_V", "alpha_V", "rho_Q", "rho_V")
ENDS = (("natural", (te.NATURAL, te.NATURAL)), ("not-a-knot", (te.NATURAL, te.NOT_A_KNOT)))


def shape_quadratic(mu):
    return mu * mu


def shape_exponential(mu):
    return np.exp(1.5 * mu)


def log_n(gamma, mu, shape):
    g, m = gamma[:, None], mu[None, :]
    return np.log(g * np.sqrt(g * g - 1.0)) - (g - 1.0) * (1.0 + ANISO * shape(m)) / THETA_E


def install(gamma, n_mu, ends, shape):
    mu = np.linspace(-1.0, 1.0, n_mu)
    assert te.set_tables(gamma, None, log_n(gamma, mu, shape), None, ends) == 0


def calc_f_errors(gamma):
    """worst |f_tab / f - 1|, |df/dgamma_tab - df/dgamma| / f and |df/dmu_tab - df/dmu| / f of the installed quadratic table at
    4096 seeded points, gamma - 1 log-uniform in [1e-3, 150], a quarter of the mu in the end cells of the 8-node grid"""
    rng = np.random.default_rng(20261020)
    g = 1.0 + np.exp(rng.uniform(np.log(1e-3), np.log(150.0), 4096))
    m = rng.uniform(-1.0, 1.0, 4096)
    m[:512] = rng.uniform(-1.0, -1.0 + 2.0 / 7.0, 512)
    m[512:1024] = rng.uniform(1.0 - 2.0 / 7.0, 1.0, 512)
    f, dfdg, dfdm = te.dev_calc_f([0.0], 1.0, g, m)
    a = (1.0 + ANISO * m * m) / THETA_E
    exact = np.exp(-(g - 1.0) * a)
    return (np.abs(f / exact - 1.0).max(), np.abs(dfdg / exact + a).max(),
            np.abs(dfdm / exact + (g - 1.0) * 2.0 * ANISO * m / THETA_E).max())


def coefficients():
    s = np.array(S_VALUES)
    out, _ = te.batch(s, np.full(len(s), THETA), np.zeros(len(s)), 0xFF, 8)
    return out


def coefficient_table(gamma, shape, title):
    print(title)
    install(gamma, REF_MU, ENDS[0][1], shape)
    ref = coefficients()
    assert np.isfinite(ref).all(), ref
    print("  the worst relative difference over s = %s at theta = %g from the %d x %d table with natural ends, per slot"
          % (", ".join("%g" % v for v in S_VALUES), THETA, N_GAMMA, REF_MU))
    print("  %5s  %-10s  %s" % ("n_mu", "mu ends", "  ".join("%8s" % n for n in SLOTS)))
    for n_mu in N_MU:
        for name, ends in ENDS:
            install(gamma, n_mu, ends, shape)
            d = np.abs(coefficients() / ref - 1.0).max(axis=0)
            print("  %5d  %-10s  %s" % (n_mu, name, "  ".join("%8.1e" % v for v in d)))
    print()


def main():
    print("The ends of the spline of a 2-D table set: accuracy on the CPU oracle (tools/tab_2d_ends_accuracy.py)")
    print()
    print("1. what the host tests assert (tests/test_tabulated_2d_ends_host.py: ten times the worst figure of each block)")
    print("  cubics come back: S = P(u) Q(mu) + R(u) + T(mu), degree 3 each; the worst deviation of S, S_u, S_mu at 200 points")
    print("  off the nodes, relative to max |S|")
    print("  %-8s  %-7s  %12s  %12s" % ("geometry", "shape", "not-a-knot", "natural"))
    worst = 0.0
    for form in te.FORMS:
        for shape in te.CUBIC_SHAPES:
            nak, nat = te.cubic_deviation(form, shape, (1, 1)), te.cubic_deviation(form, shape, (0, 0))
            worst = max(worst, nak)
            print("  %-8s  %-7s  %12.2e  %12.2e" % (form, "%dx%d" % shape, nak, nat))
    print("  worst with not-a-knot ends: %.1e" % worst)
    print("  an independent solver: S_u, S_mu, S_umu on jittered gamma and mu nodes against scipy CubicSpline(bc_type='not-a-knot'),")
    print("  the worst difference relative to the line's max |slope|")
    worst = 0.0
    for shape in te.SCIPY_SHAPES:
        d = te.scipy_difference(shape)
        worst = max(worst, d)
        print("  %-12s  %.2e" % ("%dx%dx%d" % shape, d))
    print("  worst: %.1e" % worst)
    print("  the normalisation: S = H(u) + 2 mu^2 on %d x %d nodes, |N_iso / N / P - 1| with P = 1/2 int exp(2 mu^2) dmu from"
          % (te.NORM_NODES, te.NORM_NMU))
    print("  scipy.special.erfi (a figure of 0 is below one unit in the last place of the ratio, 2.2e-16)")
    for name, ends in (("not-a-knot on both axes", (1, 1)), ("not-a-knot along mu only", (0, 1)), ("natural", (0, 0))):
        print("  %-26s  %.2e" % (name, te.norm_deviation(ends)))
    print()
    gamma = api.grid_nodes_log_gm1(G_LO, G_HI, N_GAMMA)
    print("2. n = gamma^2 beta exp(-(gamma - 1)(1 + %g mu^2) / %g) on %d gamma nodes uniform in ln(gamma - 1) over [1 + 1e-4, %g]"
          % (ANISO, THETA_E, N_GAMMA, G_HI))
    print("  the worst error against the closed form at 4096 points (gamma - 1 in [1e-3, 150], mu in [-1, 1]), through calc_f with")
    print("  norm = 1: |f_tab / f - 1|, |d_gamma f_tab - d_gamma f| / f, |d_mu f_tab - d_mu f| / f")
    print("  %5s  %-10s  %10s  %10s  %10s" % ("n_mu", "mu ends", "f", "df/dgamma", "df/dmu"))
    for n_mu in N_MU:
        for name, ends in ENDS:
            install(gamma, n_mu, ends, shape_quadratic)
            print("  %5d  %-10s  %10.1e  %10.1e  %10.1e" % ((n_mu, name) + calc_f_errors(gamma)))
    print("  (the errors that not-a-knot ends leave are those of the spline along gamma, which the mu nodes do not touch)")
    print()
    coefficient_table(gamma, shape_quadratic, "  the eight coefficients of that table")
    coefficient_table(gamma, shape_exponential, "3. the same with exp(1.5 mu) in place of mu^2: n = gamma^2 beta exp(-(gamma - 1)(1 + %g exp(1.5 mu)) / %g)"
                      % (ANISO, THETA_E))


if __name__ == "__main__":
    main()
