#!/usr/bin/env python3
"""Writes tests/golden/tabulated_2d_det.npz: the fixture of the tabulated distribution on 2-D table sets, ln n(gamma, mu)
on a grid, computed by the 2-D table oracle (tests/support/liboracle_tab2d.so -- the CPU oracle's calculators on the host
build of the device functions, so the GPU is expected to return the same BITS).

  gamma_lo, gamma_hi                 the range of the tables, [1.01, 1e4]
  geometry [2][2]                    (n_nodes, n_mu) of the two sets: 64 x 8, the smallest mu grid, and 16 x 1024, many more
                                     mu nodes than gamma nodes.  The tables themselves are not stored: they are
                                     tab2d_bind.edge_tables_2d(n_nodes, n_mu, cols) -- a tilted rolled power law, the T = 10
                                     Juettner shape, a rolled power law with an anisotropy that grows with energy
  cols_0 [3][64], cols_1 [3][16]     per geometry what the tables need of the gamma nodes (tab2d_bind.columns: u, gamma, the
                                     Juettner column), so that the tables are the same bits wherever they are rebuilt
  s, theta, index [24]               the rows: 8 (s, theta) of the bench generator per table
  values [2][24][8], work [2][24][8] per geometry: coefficients (NaN where the quadratures fail) and integrand samples
  status [2][24][8]                  the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN
  norm [2][3]                        the normalisations of the tables

CPU only; takes a minute or two.  Usage: python tools/make_tabulated_2d_fixture.py"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_bind  # noqa: E402
from rimphony_amd import workload  # noqa: E402

GEOMETRY = ((64, 8), (16, 1024))
ROWS_PER_TABLE = 8
ST_NONFINITE = 16
START = 7100000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--start", type=int, default=START, help="first row of the bench generator")
    a = ap.parse_args()
    n = 3 * ROWS_PER_TABLE
    _, _, s, theta, _ = workload.make_batch("cfg2_powerlaw_8", n, start=a.start)
    index = np.repeat(np.arange(3, dtype=np.float64), ROWS_PER_TABLE)
    values, work, norm, cols = [], [], [], []
    for n_nodes, n_mu in GEOMETRY:
        cols.append(tab2d_bind.columns(n_nodes))
        assert tab2d_bind.set_tables(tab2d_bind.EDGE_LO, tab2d_bind.EDGE_HI, tab2d_bind.edge_tables_2d(n_nodes, n_mu, cols[-1])) == 0
        v, w = tab2d_bind.batch(s, theta, index, 0xFF, a.threads)
        print(n_nodes, "x", n_mu, "NaN per slot", np.isnan(v).sum(axis=0), " samples", int(w.sum()))
        values.append(v)
        work.append(w)
        norm.append(tab2d_bind.batch_norm(np.arange(3.0)))
    values, work = np.stack(values), np.stack(work).astype(np.uint64)
    finite = np.isfinite(values)
    # if either fails, choose other rows (--start)
    assert finite.mean() >= 0.9, finite.mean()
    assert finite.any(axis=1).all(), finite.any(axis=1)
    status = np.where(finite, 0, ST_NONFINITE).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_2d_det.npz")
    np.savez_compressed(out, gamma_lo=tab2d_bind.EDGE_LO, gamma_hi=tab2d_bind.EDGE_HI,
                        geometry=np.array(GEOMETRY, dtype=np.int64), s=s, theta=theta, index=index, values=values, work=work,
                        status=status, norm=np.stack(norm), cols_0=cols[0], cols_1=cols[1])
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
