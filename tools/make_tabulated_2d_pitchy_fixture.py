#!/usr/bin/env python3
"""Writes tests/golden/tabulated_2d_pitchy_det.npz: the fixture of the tabulated distribution as 2-D sets with a sin^k xi
prefactor, computed by the form's table oracle (tests/support/liboracle_tab2dpitchy.so -- the CPU oracle's calculators on
the host build of the device functions, so the GPU is expected to return the same BITS).

  range_u [2], tables_u [2][32][8], k_u [2]     set U: 32 nodes uniform in ln gamma over [1.01, 1e4] x 8 mu nodes (two of the
                                                seven mu cells are end cells), k = 0.5 and 2.5
  gamma_g [64], tables_g [2][64][9], k_g [2]    set G: 64 given nodes uniform in ln(gamma - 1) x 9 mu nodes, k = 1 and 0 given
                                                explicitly
                                                (tab2d_pitchy_bind.fixture_set; two tables per set, none separable, tapered
                                                at both ends.  The tables are stored, so that a set built from them is the
                                                same bits on every machine)
  s, theta, index [24]                          the rows: seeded (s, theta), s log-uniform in [2, 12] and theta uniform in
                                                [0.4, 1.3] (the bench generator's rows cost the oracle seconds each), chosen
                                                so that every slot has at least 12 finite values per set and no row costs
                                                the oracle 50 ms per coefficient; the tables in turn (0, 1, 0, ...)
  values [2][24][8], work [2][24][8]            per set: coefficients (NaN where the quadratures fail) and integrand samples
  status [2][24][8]                             the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN
  norms [2][2]                                  the tables' normalisations

CPU only; takes about two minutes.  Usage: python tools/make_tabulated_2d_pitchy_fixture.py"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_pitchy_bind as tp  # noqa: E402

ROWS = 24
ST_NONFINITE = 16
ROW_SECONDS = 8 * 0.05          # what a row may cost the oracle: 50 ms per coefficient


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261019, help="seed of the candidate rows")
    ap.add_argument("--pool", type=int, default=96, help="candidate rows")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    s_all, th_all = np.exp(rng.uniform(np.log(2.0), np.log(12.0), a.pool)), rng.uniform(0.4, 1.3, a.pool)
    sets = [tp.fixture_set(which) for which in (0, 1)]
    # the candidates one by one on one thread, each on the table it would get: its cost and its values on both sets
    cost = np.zeros((2, a.pool))
    vals = np.zeros((2, a.pool, 8))
    wrk = np.zeros((2, a.pool, 8), dtype=np.uint64)
    norms = []
    for which, (where, tables, k) in enumerate(sets):
        assert tp.set_tables(where, tables, k) == 0
        norms.append(tp.batch_norm(np.arange(2, dtype=np.float64)))
        for i in range(a.pool):
            t0 = time.perf_counter()
            v, w = tp.batch(s_all[i:i + 1], th_all[i:i + 1], np.array([float(i % 2)]), 0xFF, 1)
            cost[which, i] = time.perf_counter() - t0
            vals[which, i], wrk[which, i] = v[0], w[0]
    cheap = (cost < ROW_SECONDS).all(axis=0)
    # rows in order, table 0 on even candidates and table 1 on odd ones; prefer rows finite in every slot, then fill up
    fin = np.isfinite(vals).all(axis=(0, 2))
    order = [i for i in range(a.pool) if cheap[i] and fin[i]] + [i for i in range(a.pool) if cheap[i] and not fin[i]]
    pick = {0: [], 1: []}
    for i in order:
        if len(pick[i % 2]) < ROWS // 2:
            pick[i % 2].append(i)
    assert len(pick[0]) == ROWS // 2 and len(pick[1]) == ROWS // 2, (len(pick[0]), len(pick[1]))
    rows = np.array([r for pair in zip(sorted(pick[0]), sorted(pick[1])) for r in pair])
    s, theta, index = s_all[rows].copy(), th_all[rows].copy(), (rows % 2).astype(np.float64)
    values, work = vals[:, rows], wrk[:, rows]
    finite = np.isfinite(values)
    for which in (0, 1):
        print("set", "UG"[which], "NaN per slot", np.isnan(values[which]).sum(axis=0), " samples", int(work[which].sum()),
              " slowest row %.0f ms" % (1e3 * cost[which, rows].max()))
    assert (finite.sum(axis=1) >= 12).all(), finite.sum(axis=1)         # every slot: at least 12 finite values per set
    assert (np.bincount(index.astype(int)) >= 6).all()
    differ = (values[0].view(np.uint64) != values[1].view(np.uint64)) & ~(np.isnan(values[0]) & np.isnan(values[1]))
    assert differ.any(axis=1).all(), differ.any(axis=1)                 # the two sets differ on every row
    assert np.isfinite(np.stack(norms)).all()
    status = np.where(finite, 0, ST_NONFINITE).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_2d_pitchy_det.npz")
    np.savez_compressed(out, range_u=np.array(sets[0][0]), tables_u=sets[0][1], k_u=sets[0][2], gamma_g=sets[1][0], tables_g=sets[1][1],
                        k_g=sets[1][2], s=s, theta=theta, index=index, values=values, work=work, status=status, norms=np.stack(norms))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
