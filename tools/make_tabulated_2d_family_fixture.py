#!/usr/bin/env python3
"""Writes tests/golden/tabulated_2d_family_det.npz: the fixture of the tabulated distribution as a FAMILY of 2-D surfaces on
given gamma and mu nodes with a real index per row, computed by the 2-D family oracle
(tests/support/liboracle_tab2dfamily.so -- the CPU oracle's calculators on the host build of the device functions, so the GPU
is expected to return the same BITS).

  s, theta [24]                      the rows: (s, theta) of tests/golden/tabulated_pitchy_det.npz
  x [2][24]                          per set the real index of each row (tab2d_family_bind.fixture_x): every integer,
                                     interior fractions in each pair, last - 2^-52, -0.0, and six bad values
  values [2][24][8], work [2][24][8] per set: coefficients (NaN where the quadratures fail or the index names no table)
                                     and integrand samples.  Set A: 3 tables, no prefactor, 16 gamma nodes uniform in
                                     ln(gamma - 1) x 8 mu nodes uniform in xi, natural ends; set B: 2 tables with sin_k =
                                     (0.5, 2.5), 16 x 8 jittered mu nodes, not-a-knot ends along mu
                                     (tab2d_family_bind.fixture_set)
  status [2][24][8]                  the status bits the values imply: RIMPHONY_ST_NONFINITE where a value is NaN, and
                                     RIMPHONY_ST_NORM_FAIL with it where the index names no table
  norm [2][24]                       the rows' normalisations

CPU only; takes under a minute.  Usage: python tools/make_tabulated_2d_family_fixture.py"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tab2d_family_bind as tf  # noqa: E402

ST_NONFINITE, ST_NORM_FAIL = 16, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    src = np.load(os.path.join(ROOT, "tests", "golden", "tabulated_pitchy_det.npz"))
    s, theta = src["s"].copy(), src["theta"].copy()
    assert len(s) == 24
    xs, values, work, norms, status = [], [], [], [], []
    for which in (0, 1):
        gamma, mu, tables, sin_k, ends = tf.fixture_set(which)
        assert tf.set_tables(gamma, mu, tables, sin_k, ends) == 0
        assert (tf.blob()[-4 * tables.size:] != 0).all()           # no zero node word: rim_fma(0, d, -0.0) is +0.0
        x = tf.fixture_x(which)
        v, w = tf.batch(s, theta, x, 0xFF, a.threads)
        nrm = tf.batch_norm(x)
        valid = tf.valid_x(which, x)
        assert (np.isfinite(nrm) == valid).all() and (~valid).sum() == tf.BAD_X
        print("set", "AB"[which], "valid rows", int(valid.sum()), "NaN per slot", np.isnan(v).sum(axis=0), " samples", int(w.sum()))
        finite = np.isfinite(v)
        # the conditions of the fixture; if one fails, choose other rows
        assert finite.any(axis=0).all(), finite.any(axis=0)         # every slot finite on at least one row
        assert not finite[~valid].any() and finite[valid].mean() >= 0.8, finite[valid].mean()
        st = np.where(finite, 0, ST_NONFINITE)
        st[~valid] |= ST_NORM_FAIL
        assert (st[~valid] == (ST_NONFINITE | ST_NORM_FAIL)).all()
        xs.append(x); values.append(v); work.append(w); norms.append(nrm); status.append(st)
    out = os.path.join(ROOT, "tests", "golden", "tabulated_2d_family_det.npz")
    np.savez_compressed(out, s=s, theta=theta, x=np.stack(xs), values=np.stack(values), work=np.stack(work).astype(np.uint64),
                        status=np.stack(status).astype(np.int32), norm=np.stack(norms))
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
