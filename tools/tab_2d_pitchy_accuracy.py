#!/usr/bin/env python3
"""What the 2-D table forms with a sin^k xi prefactor measure against the analytic references on the CPU oracle: the figures of
profiles/tabulated_2d_pitchy_accuracy.txt, from which tests/test_tabulated_2d_pitchy_host.py takes its bounds (twice each).  Runs
the test module's own measuring functions.  CPU only; takes a few minutes.

usage: tab_2d_pitchy_accuracy.py [out]        (default: profiles/tabulated_2d_pitchy_accuracy.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_tabulated_2d_pitchy_host as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tabulated_2d_pitchy_accuracy.txt")
    lines = ["2-D table forms with a sin^k xi prefactor against analytic references, CPU oracle (tools/tab_2d_pitchy_accuracy.py).",
             "The GPU returns the oracle's bits (tests/test_gpu_tabulated_2d_pitchy.py), so these figures are the product's.",
             "Every figure is the worst |table / reference - 1| over the rows and the eight coefficients; the host tests bound",
             "each comparison by twice its figure, never above 1e-11.", "",
             "against analytic kind 2 (gamma^-2.5 exp(-gamma / 1e10) sin^k, 2048 x 8 nodes over [1, 1e12], 16 rows)"]
    for form, k in sorted(T.MEASURED_KIND2):
        lines.append("  %-12s k = %-4g  %.2e" % (form, k, T.measure_kind2(form, k)))
    lines += ["", "against the analytic tilted power law times sin^k (ln n bilinear in (u, mu), 2048 x 8 nodes, rows finite in the reference)"]
    for form, q, a, k in sorted(T.MEASURED_TILT):
        lines.append("  %-12s q = %-5g a = %-4g k = %-4g  %.2e" % (form, q, a, k, T.measure_tilt(form, q, a, k)))
    lines += ["", "a separable surface H(u) + G(mu), k = %g, against the separable forms (12 rows): coefficients with the" % T.SEPARABLE_K,
              "normalisations divided out, then the normalisations themselves (two quadrature requests of 1e-8 apart)"]
    for form in sorted(T.MEASURED_SEPARABLE):
        shape, norms = T.measure_separable(form)
        lines.append("  %-12s coefficients %.2e   normalisations %.2e" % (form, shape, norms))
    lines += ["", "nbar against scipy.integrate.quad (epsrel 1e-13) on the same spline surface, worst of three gamma"]
    for n_mu in T.NBAR_NMU:
        for k in T.NBAR_KS:
            lines.append("  n_mu = %-3d k = %-4g  %.2e" % (n_mu, k, T.nbar_errors(T.tp._tab(), k, n_mu)))
    lines += ["  (These figures are the reference's own error, whose tolerance is 1e-13 across the spline's knots: against an 80-point",
              "  Gauss-Legendre sum per mu cell in 30-digit arithmetic, the end cells under the same substitution, nbar is within 1.2e-15 at",
              "  k = 100 / 8 nodes, k = 0.5 / 8 nodes and k = 2.5 / 65 nodes, and scipy's value is 7e-15 ... 2.8e-13 off.  A build with the plain",
              "  rule on the end cells is 4.7e-6 off at k = 0.5 on 8 nodes: test_plain_rule_on_the_end_cells_misses_the_bound.)"]
    text = "\n".join(lines) + "\n"
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
