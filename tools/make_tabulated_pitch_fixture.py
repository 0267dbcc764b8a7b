#!/usr/bin/env python3
"""Writes tests/golden/tabulated_pitch_det.npz: the fixture of the tabulated distribution with a pitch-angle factor,
computed by the pitch-table oracle (tests/support/liboracle_tabpitch.so -- the CPU oracle's calculators on the host build
of the device functions, so the GPU is expected to return the same BITS).

  gamma_lo, gamma_hi, tables[3][64]  the gamma tables: tab_bind.edge_tables (a rolled power law (2.5, 30, 500), the T = 10
                                     Juettner shape, a rolled power law (3.5, 10, 200)) over [1.01, 1e4]
  n_mu [2]                           the two pitch geometries, 8 and 4096 nodes; the pitch rows themselves are
                                     tab_pitch_bind.edge_pitch(n_mu): G = 1.0 mu, G = 0, G = 0.8 mu - 1.5 mu^2
  s, theta, index [24]               the rows: 8 (s, theta) of the bench generator per table
  values [2][24][8], work [2][24][8] per geometry: coefficients (NaN where the quadratures fail) and integrand samples
  status [2][24][8]                  the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN

CPU only; takes a minute or two.  Usage: python tools/make_tabulated_pitch_fixture.py"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab_bind  # noqa: E402
import tab_pitch_bind  # noqa: E402
from rimphony_amd import workload  # noqa: E402

GAMMA_LO, GAMMA_HI, NODES = 1.01, 1e4, 64
N_MU = (8, 4096)
ROWS_PER_TABLE = 8
ST_NONFINITE = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    tables = tab_bind.edge_tables(GAMMA_LO, GAMMA_HI, NODES)
    n = 3 * ROWS_PER_TABLE
    _, _, s, theta, _ = workload.make_batch("cfg2_powerlaw_8", n, start=7100000)
    index = np.repeat(np.arange(3, dtype=np.float64), ROWS_PER_TABLE)
    values, work = [], []
    for n_mu in N_MU:
        assert tab_pitch_bind.set_tables(GAMMA_LO, GAMMA_HI, tables, tab_pitch_bind.edge_pitch(n_mu)) == 0
        v, w = tab_pitch_bind.batch(s, theta, index, 0xFF, a.threads)
        print("n_mu", n_mu, "NaN per slot", np.isnan(v).sum(axis=0), " samples", int(w.sum()))
        values.append(v)
        work.append(w)
    values, work = np.stack(values), np.stack(work).astype(np.uint64)
    finite = np.isfinite(values)
    # if either fails, choose other rows (the start of the generator above)
    assert finite.mean() >= 0.9, finite.mean()
    assert finite.any(axis=1).all(), finite.any(axis=1)
    status = np.where(finite, 0, ST_NONFINITE).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_pitch_det.npz")
    np.savez_compressed(out, gamma_lo=GAMMA_LO, gamma_hi=GAMMA_HI, tables=tables, n_mu=np.array(N_MU, dtype=np.int64),
                        s=s, theta=theta, index=index, values=values, work=work, status=status)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
