#!/usr/bin/env python3
"""Writes tests/golden/tabulated_2d_ends_det.npz: the fixture of 2-D table sets whose splines have not-a-knot ends on both
axes, computed by the table oracle of the choice of ends (tests/support/liboracle_tab2dends.so -- the CPU oracle's calculators
on the host build of the device functions and of the builders, so the GPU is expected to return the same BITS).

The two sets are tab2d_ends_bind.fixture_set's and are built from that function again by whoever reads the fixture; the
fixture stores their tables as well, so that a change of that function shows as a difference and not as other bits.
  tables_0 [2][64][16], lo_hi_0 [2]              set 0: 64 x 16 nodes uniform in ln gamma over [1.01, 300] and in mu, two
                                                 bi-Maxwellians (ln n quadratic in mu, the coefficient growing with gamma)
  gamma_1 [40], mu_1 [12], tables_1 [2][40][12], k_1 [2]
                                                 set 1: 40 jittered gamma nodes, 12 jittered mu nodes, sin_k = 0.5 and 2.0
  s, theta, index [12]                           the rows, the same for both sets: s = 1 ... 100 spaced evenly in ln s, theta
                                                 = 0.3 ... 2.0 spaced evenly and dealt out so that s and theta do not rise
                                                 together, the tables in turn (0, 1, ...)
  values [2][12][8], work [2][12][8]             per set: coefficients (NaN where the quadratures fail) and integrand samples
  status [2][12][8]                              the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN
  norms [2][2]                                   the tables' normalisations
  f_gamma, f_mu [48], f_values [2][2][3][48]     calc_f: (gamma, mu) pairs inside the tables -- the end cells along mu
                                                 among them -- and per set and table f, df/dgamma and df/dmu there

CPU only; takes about a minute.  Usage: python tools/make_tabulated_2d_ends_fixture.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_ends_bind as te  # noqa: E402

ROWS = 12
ST_NONFINITE = 16


def rows():
    s = np.exp(np.linspace(np.log(1.0), np.log(100.0), ROWS))
    theta = np.linspace(0.3, 2.0, ROWS)[(np.arange(ROWS) * 5) % ROWS]       # 5 and 12 are coprime: a permutation
    return s, theta, (np.arange(ROWS) % 2).astype(np.float64)


def calc_f_points():
    rng = np.random.default_rng(20261020)
    gamma = np.exp(rng.uniform(np.log(1.2), np.log(250.0), 48))
    mu = rng.uniform(-1.0, 1.0, 48)
    mu[:8] = [-0.999, -0.95, -0.9, -0.88, 0.88, 0.9, 0.95, 0.999]           # the end cells of either set
    return gamma, mu


def main():
    s, theta, index = rows()
    f_gamma, f_mu = calc_f_points()
    values, work, norms, f_values, sets = [], [], [], [], []
    for which in (0, 1):
        gamma, lo, hi, mu, tables, k = te.fixture_set(which)
        sets.append((gamma, lo, hi, mu, tables, k))
        assert te.set_tables(gamma, mu, tables, k, te.FIXTURE_ENDS, gamma_lo=lo, gamma_hi=hi) == 0
        assert (te.ends_words(te.blob()) == 3).all()
        norms.append(te.batch_norm(np.arange(2, dtype=np.float64)))
        v, w = te.batch(s, theta, index, 0xFF, 8)
        values.append(v)
        work.append(w)
        f_values.append([np.stack(te.dev_calc_f([float(t)], norms[-1][t], f_gamma, f_mu)) for t in (0, 1)])
        print("set", which, "NaN per slot", np.isnan(v).sum(axis=0), " samples", int(w.sum()), " dearest row", int(w.sum(axis=1).max()))
    values, work, norms, f_values = np.stack(values), np.stack(work), np.stack(norms), np.array(f_values)
    finite = np.isfinite(values)
    assert np.isfinite(norms).all() and np.isfinite(f_values).all() and (f_values[:, :, 0] > 0.0).all()
    assert (finite.sum(axis=1) >= 8).all(), finite.sum(axis=1)          # every slot: at least 8 of 12 values per set
    status = np.where(finite, 0, ST_NONFINITE).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_2d_ends_det.npz")
    np.savez_compressed(out, tables_0=sets[0][4], lo_hi_0=np.array(sets[0][1:3]), gamma_1=sets[1][0], mu_1=sets[1][3],
                        tables_1=sets[1][4], k_1=sets[1][5], s=s, theta=theta, index=index, values=values, work=work, status=status,
                        norms=norms, f_gamma=f_gamma, f_mu=f_mu, f_values=f_values)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
