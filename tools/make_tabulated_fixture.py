#!/usr/bin/env python3
"""Writes tests/golden/tabulated_det.npz: the fixture of the tabulated distribution (kind 4), computed by the table
oracle (tests/support/liboracle_tab.so -- the CPU oracle's calculators on the host build of the device functions, so the
GPU is expected to return the same BITS).

  gamma_lo, gamma_hi, tables[2][N]   the table set: 0 a Juettner shape at T = 10, 1 gamma^-2.5 with exponential roll-offs
                                     at both ends (tests/tab_bind.py has the formulas)
  s, theta, index [256]              the rows: (s, theta) of the bench generator, the two tables in turn
  values [256][8], work [256][8]     coefficients (NaN where the quadratures fail) and integrand samples per coefficient
  pl_rows, tj_rows [16]              rows of tests/golden/symphony-powerlaw.txt -- whose (s, theta) are the comparison
                                     points -- at which a tabulated power law / Juettner distribution AND the analytic
                                     kind are finite in all eight slots (tests/test_tabulated_host.py says how they are
                                     used); chosen here, on the CPU, in file order
  pl_max_rel, tj_max_rel             the largest relative difference found on them (information; the tests measure again)

CPU only; takes a few minutes.  Usage: python tools/make_tabulated_fixture.py [--rows 256]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_bind  # noqa: E402
import tab_bind  # noqa: E402
from rimphony_amd import workload  # noqa: E402

# A Juettner shape has ln n ~ ln sqrt(gamma - 1) at the bottom, which nodes uniform in ln gamma only resolve when the table
# starts a few node spacings above gamma = 1; what lies below 1.01 is 1e-6 of the electrons at T = 10.  At the top both
# shapes have rolled off to nothing well before the table ends (a sum of zeros is no normalisation: a table far longer
# than its distribution ends in norm = inf).
FIX_GAMMA_LO, FIX_GAMMA_HI, FIX_NODES = 1.01, 1e4, 2048
CMP_NODES, CMP_P, CMP_T = 2048, 2.5, 10.0
CMP_TJ_LO, CMP_TJ_HI = 1.01, 2e3


def fixture_tables():
    g = tab_bind.nodes(FIX_GAMMA_LO, FIX_GAMMA_HI, FIX_NODES)
    return np.stack([tab_bind.log_n_juettner(g, 10.0), tab_bind.log_n_rolled_powerlaw(g)])


def comparison(which, s, theta, nthreads):
    """(tabulated, analytic) tables [n][8] of the CPU oracles for comparison `which` ('pl' or 'tj')"""
    L = oracle_bind.load("det")
    n = len(s)
    if which == "pl":
        g = tab_bind.nodes(1.0, 1e12, CMP_NODES)
        assert tab_bind.set_tables(1.0, 1e12, tab_bind.log_n_powerlaw(g, CMP_P, 1e10)) == 0
        ref = oracle_bind.batch(L, 0, s, theta, [np.full(n, CMP_P), np.ones(n), np.full(n, 1e12), np.full(n, 1e10)], 0xFF, nthreads)
    else:
        g = tab_bind.nodes(CMP_TJ_LO, CMP_TJ_HI, CMP_NODES)
        assert tab_bind.set_tables(CMP_TJ_LO, CMP_TJ_HI, tab_bind.log_n_juettner(g, CMP_T)) == 0
        ref = oracle_bind.batch(L, 1, s, theta, [np.full(n, CMP_T)], 0xFF, nthreads)
    tab, _ = tab_bind.batch(s, theta, np.zeros(n), 0xFF, nthreads)
    return tab, ref


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    assert a.rows >= 256

    gold = np.loadtxt(os.path.join(ROOT, "tests", "golden", "symphony-powerlaw.txt"))
    picks, worst = {}, {}
    for which in ("pl", "tj"):
        tab, ref = comparison(which, gold[:, 0].copy(), gold[:, 1].copy(), a.threads)
        ok = np.isfinite(tab).all(axis=1) & np.isfinite(ref).all(axis=1)
        rows = np.nonzero(ok)[0][:16]
        assert len(rows) == 16, (which, int(ok.sum()))
        picks[which] = rows.astype(np.int64)
        worst[which] = float(np.abs(tab[rows] / ref[rows] - 1.0).max())
        print(which, "finite rows:", int(ok.sum()), "of", len(ok), " max rel on the 16:", worst[which])

    tables = fixture_tables()
    assert tab_bind.set_tables(FIX_GAMMA_LO, FIX_GAMMA_HI, tables) == 0
    _, _, s, theta, _ = workload.make_batch("cfg2_powerlaw_8", a.rows, start=7000000)
    index = (np.arange(a.rows) % 2).astype(np.float64)
    values, work = tab_bind.batch(s, theta, index, 0xFF, a.threads)
    print("fixture: NaN per slot", np.isnan(values).sum(axis=0), " samples", int(work.sum()))
    out = os.path.join(ROOT, "tests", "golden", "tabulated_det.npz")
    np.savez_compressed(out, gamma_lo=FIX_GAMMA_LO, gamma_hi=FIX_GAMMA_HI, tables=tables, s=s, theta=theta, index=index,
                        values=values, work=work.astype(np.uint64), pl_rows=picks["pl"], tj_rows=picks["tj"],
                        pl_max_rel=worst["pl"], tj_max_rel=worst["tj"])
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
