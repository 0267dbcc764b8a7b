#!/usr/bin/env python3
"""Writes profiles/tabulated_2d_family_accuracy.txt: what the CPU oracle of the families of 2-D surfaces
(tests/support/liboracle_tab2dfamily.so) measures -- the figures tests/test_tabulated_2d_family_host.py bounds by twice their
value.  The GPU returns the oracle's bits (tests/test_gpu_tabulated_2d_family.py), so these figures are the product's.

  linearity   the family at fractional x against the plain nodes form installed with ln n blended on the host
  exactness   two surfaces bilinear in (ln gamma, mu) against the analytic tilted power law at the blended parameters
  juettner    a Juettner shape whose anisotropy depends on T, spaced in 1 / T, where the blend is not exact: 2, 4 and 8 tables

CPU only; a few minutes.  Usage: python tools/tab_2d_family_accuracy.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_family_bind as tf  # noqa: E402


def main():
    lines = ["Families of 2-D surfaces on given gamma and mu nodes, a real index per row, CPU oracle (tools/tab_2d_family_accuracy.py).",
             "The GPU returns the oracle's bits (tests/test_gpu_tabulated_2d_family.py), so these figures are the product's.",
             "The host tests bound each figure marked `name = value` by twice its value: the margin covers another libm.",
             "",
             "linearity: the family of fixture sets A and B at fractional x against the PLAIN nodes form installed with ln n (and k)",
             "blended on the host: worst relative difference of f, of d f / d gamma and d f / d mu relative to |reference| + |f|, over",
             "2000 (gamma, mu), and of the eight coefficients on 12 rows.  The two differ by the rounding of the blended table values"]
    for which in (0, 1):
        w = tf.measure_linearity(which)
        for name in ("f", "dfdg", "dfdcx", "coefficients"):
            lines.append("  linearity_%s_%s = %.3e" % ("AB"[which], name, w[name]))
    lines += ["",
              "exactness: two surfaces ln n = -p u + q u mu + a mu - gamma / 1e10 with (p, a, q) = (2.5, 0.8, 0.3) and (3.5, 0.4, 0.1) on",
              "2048 x 8 jittered mu nodes, at x = 0.1, 0.25, 0.5, 0.75, 0.9 against the analytic tilted power law at the blended",
              "(p, a, q) -- with sin_k = (0, 3) times sin^k at the blended k --: worst |table / analytic - 1| over the rows finite in",
              "the reference and the eight coefficients (the plain nodes form on one such surface: 8.0e-15 .. 4.5e-14,",
              "profiles/tabulated_2d_nodes_accuracy.txt)"]
    lines.append("  exactness_plain = %.3e" % tf.measure_exactness(False))
    lines.append("  exactness_sin_k = %.3e" % tf.measure_exactness(True))
    lines += ["",
              "where the blend is NOT exact: n = gamma^2 beta exp(-(gamma - 1)(1 + a(T) mu^2) / T), a(T) = 0.3 + 0.002 T^2, tables equally",
              "spaced in 1 / T over [0.1, 0.2] on 256 x 16 nodes, not-a-knot ends along mu, the row in the middle of every pair",
              "against a table built directly at that 1 / T: worst relative error of the eight coefficients on 8 rows"]
    for n in (2, 4, 8):
        lines.append("  juettner_%d_tables = %.3e" % (n, tf.measure_juettner(n)))
    lines.append("  (linear interpolation of ln n between neighbouring tables: twice the tables, about a quarter of the error)")
    out = os.path.join(ROOT, "profiles", "tabulated_2d_family_accuracy.txt")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
