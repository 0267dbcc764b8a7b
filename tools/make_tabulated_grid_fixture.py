#!/usr/bin/env python3
"""Writes tests/golden/tabulated_grid_det.npz: the fixture of the tabulated distribution on given gamma nodes, computed by
the grid table oracle (tests/support/liboracle_tabgrid.so -- the CPU oracle's calculators on the host build of the device
functions, so the GPU is expected to return the same BITS).

  gamma_a [64], gamma_b [64]         the nodes of set A (uniform in ln(gamma - 1), gamma - 1 from 1e-6 to 1e4) and of set B
                                     (uniform in ln gamma over [1.01, 1e4], each interior node moved by a seeded +-40 % of
                                     the spacing): tab_grid_bind.grid("log-gm1"), grid("jitter")
  sin_k [2][3]                       the exponents of set A (no g) and set B (pitch rows of 8 nodes,
                                     tab_pitchy_bind.set_b_rows); the tables are tab_grid_bind.edge_tables_at(nodes)
  s, theta, index [24]               the rows: (s, theta) of the bench generator, the tables in turn (0, 1, 2, 0, ...)
  values [2][24][8], work [2][24][8] per set: coefficients (NaN where the quadratures fail) and integrand samples
  status [2][24][8]                  the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN

CPU only; takes a minute or two.  Usage: python tools/make_tabulated_grid_fixture.py"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab_grid_bind as tg  # noqa: E402
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
    values, work, ks, grids = [], [], [], []
    for which in (0, 1):
        gamma, tables, log_g, sin_k = tg.fixture_set(which)
        assert tg.set_tables(gamma, tables, log_g, sin_k) == 0
        v, w = tg.batch(s, theta, index, 0xFF, a.threads)
        print("set", "AB"[which], "NaN per slot", np.isnan(v).sum(axis=0), " samples", int(w.sum()))
        values.append(v)
        work.append(w)
        ks.append(sin_k)
        grids.append(gamma)
    values, work = np.stack(values), np.stack(work).astype(np.uint64)
    finite = np.isfinite(values)
    # if it fails, choose other rows (the start of the generator above): a wall of NaN must not hide a failure
    assert (finite.sum(axis=1) >= n // 2).all(), finite.sum(axis=1)     # every slot finite on at least half the rows of each set
    status = np.where(finite, 0, ST_NONFINITE).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_grid_det.npz")
    np.savez_compressed(out, gamma_a=grids[0], gamma_b=grids[1], sin_k=np.stack(ks), s=s, theta=theta, index=index,
                        values=values, work=work, status=status)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
