#!/usr/bin/env python3
"""Writes tests/golden/tabulated_2d_family_cubic_det.npz: the fixture of the tabulated distribution as a family of 2-D surfaces
blended CUBICALLY across its tables, computed by that form's oracle (tests/support/liboracle_tab2dfamilycubic.so -- the CPU
oracle's calculators on the host build of the device functions, so the GPU is expected to return the same BITS).

  s, theta [24]                      the rows: (s, theta) of tests/golden/tabulated_pitchy_det.npz
  x [24]                             the real index of each row, the same for both sets (tab2d_family_cubic_bind.fixture_x):
                                     the integers 0, -0.0, 1, 5, one fraction per table interval, four invalid values, then
                                     the fractions and the other integers again
  values [2][24][8], work [2][24][8] per set: coefficients (NaN where the quadratures fail or the index names no table)
                                     and integrand samples.  Sets A and B of tab2d_family_cubic_bind.fixture_set: 6 tables on
                                     24 x 8 nodes; A without a prefactor, natural ends, knots increasing; B with sin_k per
                                     table, not-a-knot ends along mu, knots decreasing
  status [2][24][8]                  the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN, and
                                     RIMPHONY_ST_NORM_FAIL with it where the index names no table
  norm [2][24]                       the rows' normalisations

CPU only; takes under a minute.  Usage: python tools/make_tabulated_2d_family_cubic_fixture.py"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_family_cubic_bind as tc  # noqa: E402

ST_NONFINITE, ST_NORM_FAIL = 16, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    s, theta = tc.fixture_rows()
    assert len(s) == 24
    x = tc.fixture_x()
    valid = tc.valid_x(x)
    values, work, norms, status = [], [], [], []
    for which in (0, 1):
        gamma, mu, tables, sin_k, ends, param = tc.fixture_set(which)
        assert tc.set_tables(gamma, mu, tables, sin_k, ends, param) == 0
        nt = len(tables)
        assert (tc.blob()[-4 * tables.size - nt:-nt] != 0).all()            # no zero node word: the sign of one is not kept
        v, w = tc.batch(s, theta, x, 0xFF, a.threads)
        nrm = tc.batch_norm(x)
        assert (np.isfinite(nrm) == valid).all() and (~valid).sum() == tc.BAD_X
        print("set", "AB"[which], "valid rows", int(valid.sum()), "NaN per slot", np.isnan(v).sum(axis=0), " samples", int(w.sum()))
        finite = np.isfinite(v)
        # the conditions of the fixture; if one fails, choose other rows
        assert finite.any(axis=0).all(), finite.any(axis=0)         # every slot finite on at least one row
        assert not finite[~valid].any() and finite[valid].mean() >= 0.8, finite[valid].mean()
        st = np.where(finite, 0, ST_NONFINITE)
        st[~valid] |= ST_NORM_FAIL
        values.append(v); work.append(w); norms.append(nrm); status.append(st)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_2d_family_cubic_det.npz")
    np.savez_compressed(out, s=s, theta=theta, x=x, values=np.stack(values), work=np.stack(work).astype(np.uint64),
                        status=np.stack(status).astype(np.int32), norm=np.stack(norms))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
