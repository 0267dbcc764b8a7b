#!/usr/bin/env python3
"""Writes profiles/tabulated_2d_family_cubic_accuracy.txt: what the CPU oracle of the families of 2-D surfaces blended cubically
across their tables (tests/support/liboracle_tab2dfamilycubic.so) measures -- the figures
tests/test_tabulated_2d_family_cubic_host.py bounds by twice their value.  The GPU returns the oracle's bits
(tests/test_gpu_tabulated_2d_family_cubic.py), so these figures are the product's.

  independence  the family at fractional x against the plain nodes form installed with ln n blended on the host, the weights
                computed in numpy
  exactness     five surfaces bilinear in (ln gamma, mu) whose coefficients are cubic polynomials in unevenly spaced knots,
                against the analytic tilted power law at the polynomials' values
  juettner      the Juettner shape of profiles/tabulated_2d_family_accuracy.txt, where neither blend is exact: 4 and 8 tables,
                next to the linear blend on the same tables

CPU only; a few minutes.  Usage: python tools/tab_2d_family_cubic_accuracy.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_family_bind as tf  # noqa: E402
import tab2d_family_cubic_bind as tc  # noqa: E402


def main():
    lines = ["Families of 2-D surfaces blended cubically across their tables, CPU oracle (tools/tab_2d_family_cubic_accuracy.py).",
             "The GPU returns the oracle's bits (tests/test_gpu_tabulated_2d_family_cubic.py), so these figures are the product's.",
             "The host tests bound each figure marked `name = value` by twice its value: the margin covers another libm.",
             "",
             "independence: the cubic family of fixture sets A and B (6 tables, 24 x 8 nodes, uneven knots) at x = 0.37, 1.5, 2.25, 3.5,",
             "4.75 against the PLAIN nodes form installed with ln n (and k) blended on the host, the Lagrange weights computed in numpy:",
             "worst relative difference of f, of d f / d gamma and d f / d mu relative to |reference| + |f|, over 2000 (gamma, mu), and",
             "of the eight coefficients on 12 rows.  The two differ by the rounding of the weights and of the blended table values"]
    for which in (0, 1):
        w = tc.measure_independence(which)
        for name in ("f", "dfdg", "dfdcx", "coefficients"):
            lines.append("  independence_%s_%s = %.3e" % ("AB"[which], name, w[name]))
    lines += ["",
              "exactness: five surfaces ln n = -p u + q u mu + a mu - gamma / 1e10 with p, a, q cubic polynomials in the knots",
              "(0, 0.6, 1, 1.9, 2.5) on 2048 x 8 jittered mu nodes, at x = 0.4, 1.5, 2.3, 3.6 -- the stencil clamped low, interior",
              "twice, clamped high -- against the analytic tilted power law at the polynomials' values -- with sin_k, k cubic in the",
              "knots too, times sin^k --: worst |table / analytic - 1| over the rows finite in the reference and the eight",
              "coefficients (the linear family on two such surfaces: 5.3e-14 and 1.0e-13, profiles/tabulated_2d_family_accuracy.txt)"]
    lines.append("  exactness_plain = %.3e" % tc.measure_exactness(False))
    lines.append("  exactness_sin_k = %.3e" % tc.measure_exactness(True))
    lines += ["",
              "where neither blend is exact: n = gamma^2 beta exp(-(gamma - 1)(1 + a(T) mu^2) / T), a(T) = 0.3 + 0.002 T^2, tables equally",
              "spaced in 1 / T over [0.1, 0.2] on 256 x 16 nodes, not-a-knot ends along mu, the knots 1 / T, the row in the middle of",
              "every pair against a table built directly at that 1 / T: worst relative error of the eight coefficients on 8 rows"]
    for n in (4, 8):
        cubic, linear = tc.measure_juettner(n), tf.measure_juettner(n)
        lines.append("  juettner_cubic_%d_tables = %.3e" % (n, cubic))
        lines.append("  (the linear blend on the same %d tables: %.3e, %.1f times as far)" % (n, linear, linear / cubic))
    out = os.path.join(ROOT, "profiles", "tabulated_2d_family_cubic_accuracy.txt")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
