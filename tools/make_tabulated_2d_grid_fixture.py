#!/usr/bin/env python3
"""Writes tests/golden/tabulated_2d_grid_det.npz: the fixture of the tabulated distribution as 2-D sets on given gamma nodes,
computed by the form's table oracle (tests/support/liboracle_tab2dgrid.so -- the CPU oracle's calculators on the host build
of the device functions, so the GPU is expected to return the same BITS).

  gamma_a [64], tables_a [3][64][8]      set A: nodes uniform in ln(gamma - 1), gamma - 1 from 1e-6 to 1e4, x the smallest mu
                                         grid; about half the nodes lie in the first guide cell, so the bisection runs deep
  gamma_b [16], tables_b [3][16][1024]   set B: 16 jittered nodes x the largest mu grid, many more mu than gamma nodes
                                         (tab2d_grid_bind.fixture_set; three tables per set, none separable.  The tables are
                                         stored, so that a set built from them is the same bits on every machine)
  s, theta, index [24]                   the rows: (s, theta) of the bench generator, the tables in turn (0, 1, 2, 0, ...)
  values [2][24][8], work [2][24][8]     per set: coefficients (NaN where the quadratures fail) and integrand samples
  status [2][24][8]                      the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN
  norms [2][3]                           the tables' normalisations

CPU only; takes a few minutes.  Usage: python tools/make_tabulated_2d_grid_fixture.py"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_grid_bind as tq  # noqa: E402
from rimphony_amd import workload  # noqa: E402

ROWS_PER_TABLE = 8
ST_NONFINITE = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--start", type=int, default=7100000, help="first row of the bench generator")
    a = ap.parse_args()
    n = 3 * ROWS_PER_TABLE
    _, _, s, theta, _ = workload.make_batch("cfg2_powerlaw_8", n, start=a.start)
    index = np.tile(np.arange(3, dtype=np.float64), ROWS_PER_TABLE)
    values, work, sets, norms = [], [], [], []
    for which in (0, 1):
        gamma, tables = tq.fixture_set(which)
        assert tq.set_tables(gamma, tables) == 0
        v, w = tq.batch(s, theta, index, 0xFF, a.threads)
        print("set", "AB"[which], "NaN per slot", np.isnan(v).sum(axis=0), " samples", int(w.sum()))
        values.append(v)
        work.append(w)
        sets.append((gamma, tables))
        norms.append(tq.batch_norm(np.arange(3, dtype=np.float64)))
    values, work = np.stack(values), np.stack(work).astype(np.uint64)
    finite = np.isfinite(values)
    # if one fails, choose other rows (--start): a wall of NaN must not hide a failure, nor two sets that agree a swapped one
    assert (finite.sum(axis=1) >= n // 2).all(), finite.sum(axis=1)     # every slot finite on at least half the rows of each set
    differ = (values[0].view(np.uint64) != values[1].view(np.uint64)) & ~(np.isnan(values[0]) & np.isnan(values[1]))
    assert differ.any(axis=1).all(), differ.any(axis=1)                 # the two sets differ on every row
    assert np.isfinite(np.stack(norms)).all()
    status = np.where(finite, 0, ST_NONFINITE).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_2d_grid_det.npz")
    np.savez_compressed(out, gamma_a=sets[0][0], tables_a=sets[0][1], gamma_b=sets[1][0], tables_b=sets[1][1], s=s, theta=theta,
                        index=index, values=values, work=work, status=status, norms=np.stack(norms))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
