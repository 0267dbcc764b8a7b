#!/usr/bin/env python3
"""Recorded study (no test asserts on it): rho_Q, rho_V of the thermal kind from the J_sigma / Y_sigma kernel over the whole
(sigma, pomega) domain, tests/exact_faraday.full_kernel_coefficients, with and without the principal-value term, beside the
deterministic oracle and the converged integrals of Heyvaerts' two asymptotic elements.  T = 0.3, theta = 0.7, s = 3 ... 40,
gamma up to 1 + 32 T (exp(-32) of the weight is left beyond).  Replaces the section "full Bessel kernel" at the end of
profiles/exact_faraday_deviation.txt.  CPU only; the largest s takes about ten minutes on one core.

usage: python tools/faraday_full_kernel_study.py [--jobs N]"""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import exact_faraday as ef
import exact_symphony as ex

T, THETA, S = 0.3, 0.7, (3., 5., 10., 20., 40.)
HEAD = "\nfull Bessel kernel"


def point(s):
    dist = ex.make(1, [T])
    return ef.full_kernel_coefficients(dist, s, THETA, 1. + 32. * T), ef.coefficients(dist, s, THETA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=5)
    ap.add_argument("--table", default=os.path.join(ROOT, "profiles", "exact_faraday_deviation.txt"))
    args = ap.parse_args()
    import oracle_bind
    from rimphony_amd import _build
    _build.build_oracle()
    det = oracle_bind.load("det")
    oracle = oracle_bind.batch(det, 1, list(S), [THETA] * len(S), [np.full(len(S), T)], ef.MASK, 1)[:, 6:]
    with multiprocessing.Pool(args.jobs) as pool:
        res = pool.map(point, S[::-1], chunksize=1)[::-1]
    lines = [HEAD + " over the whole domain (tools/faraday_full_kernel_study.py): thermal_juettner, T = %g, theta = %g, gamma <= %g" % (T, THETA, 1. + 32. * T),
             "per s: rho_Q then rho_V: full form with the principal-value term, without it (Y_sigma -> -J_(-sigma) / sin(pi sigma)), their relative",
             "error estimates (twice the points), the share of the weight at nodes where J_sigma underflows; the converged Heyvaerts integrals;",
             "the ratios oracle / full form with, oracle / full form without, oracle / converged Heyvaerts integrals"]
    for s, o, (full, (hey, hey_err, _)) in zip(S, oracle, res):
        lines.append("s = %-3g sigma0 = %.3g" % (s, s * np.sin(THETA)))
        for k, name in enumerate(("rho_Q", "rho_V")):
            lines.append("    %s  with %+.10e  without %+.10e  (%.0e %.0e, left out %.0e)  heyvaerts %+.10e   oracle / with %.5f  / without %.5f  / heyvaerts %.8f" % (
                name, full[0, k], full[1, k], full[2, k] / abs(full[0, k]), full[3, k] / abs(full[1, k]), full[4, k], hey[k],
                o[k] / full[0, k], o[k] / full[1, k], o[k] / hey[k]))
    text = "\n".join(lines) + "\n"
    print(text)
    old = open(args.table).read()
    open(args.table, "w").write((old[:old.index(HEAD)] if HEAD in old else old) + text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
