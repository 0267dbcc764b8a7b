#!/usr/bin/env python3
"""Writes tests/golden/tabulated_pitchy_det.npz: the fixture of the tabulated distribution with a sin^k xi prefactor,
computed by the sin^k table oracle (tests/support/liboracle_tabpitchy.so -- the CPU oracle's calculators on the host
build of the device functions, so the GPU is expected to return the same BITS).

  gamma_lo, gamma_hi, tables[3][64]  the gamma tables: tab_bind.edge_tables (a rolled power law (2.5, 30, 500), the T = 10
                                     Juettner shape, a rolled power law (3.5, 10, 200)) over [1.01, 1e4]
  sin_k [2][3]                       the exponents of set A (no g) and set B (pitch rows of 8 nodes,
                                     tab_pitchy_bind.set_b_rows: G = 0.8 mu - 1.5 mu^2, G = 1.0 mu, the wavy row)
  s, theta, index [24]               the rows: (s, theta) of the bench generator, the tables in turn (0, 1, 2, 0, ...)
  values [2][24][8], work [2][24][8] per set: coefficients (NaN where the quadratures fail) and integrand samples
  status [2][24][8]                  the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN

CPU only; takes a minute or two.  Usage: python tools/make_tabulated_pitchy_fixture.py"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab_pitchy_bind as ty  # noqa: E402
from rimphony_amd import workload  # noqa: E402

ROWS_PER_TABLE = 8
ST_NONFINITE = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    n = 3 * ROWS_PER_TABLE
    _, _, s, theta, _ = workload.make_batch("cfg2_powerlaw_8", n, start=7100000)
    index = np.tile(np.arange(3, dtype=np.float64), ROWS_PER_TABLE)
    values, work, ks = [], [], []
    for which in (0, 1):
        lo, hi, tables, log_g, sin_k = ty.fixture_set(which)
        assert ty.set_tables(lo, hi, tables, log_g, sin_k) == 0
        v, w = ty.batch(s, theta, index, 0xFF, a.threads)
        print("set", "AB"[which], "NaN per slot", np.isnan(v).sum(axis=0), " samples", int(w.sum()))
        values.append(v)
        work.append(w)
        ks.append(sin_k)
    values, work = np.stack(values), np.stack(work).astype(np.uint64)
    finite = np.isfinite(values)
    # if either fails, choose other rows (the start of the generator above)
    assert finite.any(axis=1).all(), finite.any(axis=1)          # every slot finite on at least one row of each set
    assert finite.mean() >= 0.8, finite.mean()
    status = np.where(finite, 0, ST_NONFINITE).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_pitchy_det.npz")
    np.savez_compressed(out, gamma_lo=lo, gamma_hi=hi, tables=tables, sin_k=np.stack(ks), s=s, theta=theta, index=index,
                        values=values, work=work, status=status)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
