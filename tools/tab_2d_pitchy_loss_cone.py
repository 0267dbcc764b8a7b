#!/usr/bin/env python3
"""The README's table for a loss cone whose shape changes with energy: the plain 2-D form with a floored ln n against the 2-D
form with a sin^k xi prefactor, both against the analytic distribution (tests/support/pitchy_tilt_oracle.cpp)

    n(gamma, mu) = sin^2 xi  gamma^(-2.5 + 0.3 mu) exp(-gamma / 1e10)       on [1 + 1e-6, 1e12],

on 2048 gamma nodes uniform in ln gamma, the 16 committed power-law rows, all eight coefficients.  The plain form tabulates
ln n = max(ln(1 - mu^2), ln 1e-6) + the rest on 65 and on 257 mu nodes; the form with a prefactor tabulates the rest on 8 mu
nodes with k = 2.  CPU oracles only; takes a few minutes.  Appends its table to profiles/tabulated_2d_pitchy_accuracy.txt if
asked to (--append)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_bind as t2  # noqa: E402
import tab2d_pitchy_bind as tp  # noqa: E402
import test_tabulated_2d_pitchy_host as T  # noqa: E402

K, Q, FLOOR = 2.0, 0.3, 1e-6


def worst(tab, ref, keep):
    fin = np.isfinite(tab[keep])
    rel = np.where(fin, np.abs(np.where(fin, tab[keep], 1.0) / ref[keep] - 1.0), 0.0)
    return rel[:, :6].max(), rel[:, 6].max(), rel[:, 7].max(), int(fin.sum()), int(fin.size)


def main():
    g = T.uniform_nodes(T.TILT_LO, T.PL_HI, T.PL_NODES)
    u = np.log(g)[:, None]
    s, th = T.pl_rows()
    ref = tp.ptilt_batch(s, th, [T.PL_P, T.TILT_LO, T.PL_HI, T.PL_CUT, 0.0, Q], K, nthreads=16)
    keep = np.isfinite(ref).all(axis=1)
    rest = lambda mu: -T.PL_P * u + Q * u * mu - g[:, None] / T.PL_CUT
    lines = ["", "a loss cone that changes with energy, n = sin^2 xi gamma^(-2.5 + 0.3 mu) exp(-gamma / 1e10), against the analytic oracle",
             "(tools/tab_2d_pitchy_loss_cone.py; 2048 gamma nodes, %d of 16 rows finite in the reference): worst |table / analytic - 1|" % keep.sum(),
             "  form                                  mu nodes   j, alpha of I, Q, V   rho_Q      rho_V      finite"]
    for n_mu in (65, 257):
        mu = np.linspace(-1.0, 1.0, n_mu)[None, :]
        floored = np.maximum(0.5 * K * np.log(np.maximum(1.0 - mu * mu, 1e-300)), np.log(FLOOR)) + rest(mu)
        assert t2.set_tables(T.TILT_LO, T.PL_HI, floored) == 0
        tab = t2.batch(s, th, np.zeros(len(s)), nthreads=16)[0]
        lines.append("  plain 2-D, ln n floored at ln 1e-6     %-9d  %.1e              %.1e    %.1e    %d of %d" % ((n_mu,) + worst(tab, ref, keep)))
    mu = np.linspace(-1.0, 1.0, 8)[None, :]
    assert tp.set_tables((T.TILT_LO, T.PL_HI), rest(mu), [K]) == 0
    tab = tp.batch(s, th, np.zeros(len(s)), nthreads=16)[0]
    lines.append("  2-D with sin^k xi, k = 2               %-9d  %.1e              %.1e    %.1e    %d of %d" % ((8,) + worst(tab, ref, keep)))
    text = "\n".join(lines) + "\n"
    print(text)
    if "--append" in sys.argv:
        open(os.path.join(ROOT, "profiles", "tabulated_2d_pitchy_accuracy.txt"), "a").write(text)


if __name__ == "__main__":
    main()
