#!/usr/bin/env python3
"""Writes tests/golden/tabulated_2d_nodes_det.npz: the fixture of the tabulated distribution as 2-D sets on gamma nodes and mu
nodes of the caller's choosing, computed by the form's table oracle (tests/support/liboracle_tab2dnodes.so -- the CPU oracle's
calculators on the host build of the device functions, so the GPU is expected to return the same BITS).

  gamma_p [32], mu_p [9], tables_p [2][32][9]   set P, plain: 32 gamma nodes uniform in ln(gamma - 1), 9 graded mu nodes -- five
                                                of them in the last of the 16 guide cells, eleven guide cells empty, the last
                                                cell before mu = +1 5e-5 wide
  gamma_k [24], mu_k [12], tables_k [2][24][12], k_k [2]
                                                set K: 24 jittered gamma nodes, 12 mu nodes uniform in xi, sin_k = 0.5 and 2.5
                                                (tab2d_nodes_bind.fixture_set; two tables per set, neither separable, tapered
                                                at both ends.  The nodes and tables are stored, so that a set built from them
                                                is the same bits on every machine)
  s, theta, index [24]                          the rows: seeded (s, theta), s log-uniform in [2, 12] and theta uniform in
                                                [0.4, 1.3], chosen as tools/make_tabulated_2d_pitchy_fixture.py chooses its
                                                rows: every slot has at least 12 finite values per set and no row is dear --
                                                here at most 1e6 integrand samples over its eight coefficients on either set,
                                                what 50 ms per coefficient buy that tool's oracle, counted and not timed, so
                                                that the choice does not depend on the machine; the tables in turn (0, 1, ...)
  values [2][24][8], work [2][24][8]            per set: coefficients (NaN where the quadratures fail) and integrand samples
  status [2][24][8]                             the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN
  norms [2][2]                                  the tables' normalisations

CPU only; takes about a minute.  Usage: python tools/make_tabulated_2d_nodes_fixture.py"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_nodes_bind as tn  # noqa: E402

ROWS = 24
ST_NONFINITE = 16
ROW_SAMPLES = 1000000           # what a row may cost the oracle: integrand samples over its eight coefficients


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20261019, help="seed of the candidate rows")
    ap.add_argument("--pool", type=int, default=96, help="candidate rows")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    s_all, th_all = np.exp(rng.uniform(np.log(2.0), np.log(12.0), a.pool)), rng.uniform(0.4, 1.3, a.pool)
    sets = [tn.fixture_set(which) for which in (0, 1)]
    # set P is what the issue asks of it
    mu_p = sets[0][1]
    per_cell = np.bincount(np.minimum(((mu_p + 1.0) * 8.0).astype(int), 15), minlength=16)
    assert len(mu_p) == 9 and per_cell.max() >= 4 and (per_cell == 0).sum() >= 3 and mu_p[-1] - mu_p[-2] < 1e-4
    # the candidates, each on the table it would get: its values and its cost in samples on both sets
    vals = np.zeros((2, a.pool, 8))
    wrk = np.zeros((2, a.pool, 8), dtype=np.uint64)
    norms = []
    for which, (gamma, mu, tables, k) in enumerate(sets):
        assert tn.set_tables(gamma, mu, tables, k) == 0
        norms.append(tn.batch_norm(np.arange(2, dtype=np.float64)))
        vals[which], wrk[which] = tn.batch(s_all, th_all, (np.arange(a.pool) % 2).astype(np.float64), 0xFF, 8)
    cheap = (wrk.sum(axis=2) <= ROW_SAMPLES).all(axis=0)
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
        print("set", "PK"[which], "NaN per slot", np.isnan(values[which]).sum(axis=0), " samples", int(work[which].sum()),
              " dearest row", int(work[which].sum(axis=1).max()))
    assert (finite.sum(axis=1) >= 12).all(), finite.sum(axis=1)         # every slot: at least 12 finite values per set
    assert (np.bincount(index.astype(int)) >= 6).all()
    differ = (values[0].view(np.uint64) != values[1].view(np.uint64)) & ~(np.isnan(values[0]) & np.isnan(values[1]))
    assert differ.any(axis=1).all(), differ.any(axis=1)                 # the two sets differ on every row
    assert np.isfinite(np.stack(norms)).all()
    status = np.where(finite, 0, ST_NONFINITE).astype(np.int32)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_2d_nodes_det.npz")
    np.savez_compressed(out, gamma_p=sets[0][0], mu_p=sets[0][1], tables_p=sets[0][2], gamma_k=sets[1][0], mu_k=sets[1][1],
                        tables_k=sets[1][2], k_k=sets[1][3], s=s, theta=theta, index=index, values=values, work=work, status=status,
                        norms=np.stack(norms))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
