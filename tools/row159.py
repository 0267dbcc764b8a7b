#!/usr/bin/env python3
"""Golden row 159, alpha_V: which side is off by 1.29 %?  

tests/golden/symphony-powerlaw.txt holds Symphony-C's values; the reference's own test accepts 1 % on a random 3 %
subset of its rows per run (tests/symphony.rs:29-112), so a single row outside 1 % can sit there unnoticed.  This tool
evaluates that coefficient three ways, CPU only:
  1. the rimphony algorithm as the reference parameterises it (both oracle flavours);
  2. the same algorithm with tightened numerical parameters (eps_rel 1e-6 / 1e-8 for both quadratures, the tail
     cut-off at 1e-8 of the running sum, 300 discrete harmonics), literal flavour -- does the rimphony ALGORITHM
     converge to its own default value or to Symphony-C's?
  3. an independent evaluation that shares nothing with the Leung expansions: the harmonic sum with scipy's exact
     J_n, J'_n (the n-integral replaced by the plain sum over n, each gamma-integral by the composite Gauss-Legendre
     rule of tests/exact_symphony.py) -- the mathematical value of the expression both codes approximate.
Section 3 sums up to 200 000 harmonics: seconds for a row with small s, well over ten minutes for row 159.
usage: python tools/row159.py [row] [slot]"""
import ctypes, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oracle_bind

row = int(sys.argv[1]) if len(sys.argv) > 1 else 159
slot = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rows = np.loadtxt(os.path.join(ROOT, "tests", "golden", "symphony-powerlaw.txt"))
s, th, p = rows[row, 0], rows[row, 1], rows[row, 2]
gold = rows[row, 3 + slot]
coeff, stokes = slot & 1, slot >> 1
nu = 1e9
scale = nu if coeff == 0 else 1. / nu
print("row %d: s = %.17g theta = %.17g p = %.17g   slot %d (coeff %d stokes %d)   Symphony-C value %.16e"
      % (row, s, th, p, slot, coeff, stokes, gold))


class Tuning(ctypes.Structure):
    _fields_ = [("epsrel_gamma", ctypes.c_double), ("epsrel_n", ctypes.c_double), ("tail_tolerance", ctypes.c_double),
                ("n_discrete", ctypes.c_int), ("max_chunks", ctypes.c_int), ("hey_max_steps", ctypes.c_int)]


def run(L, tuning=None):
    L.rimo_set_tuning.restype = None
    L.rimo_set_tuning.argtypes = [ctypes.POINTER(Tuning)]
    L.rimo_set_tuning(ctypes.byref(tuning) if tuning else None)
    d, st = oracle_bind.mkdist(L, 0, [p, 1.0, 1e12, 1e10])
    c = oracle_bind.Counters()
    v = L.rimo_compute_dimensionless(d, coeff, stokes, s, th, ctypes.byref(c)) * scale
    L.rimo_set_tuning(None)
    return v, c.integrand_evals, d


det, libm = oracle_bind.load("det"), oracle_bind.load("libm")
for name, L in (("deterministic flavour", det), ("literal (libm) flavour", libm)):
    v, ne, _ = run(L)
    print("1. rimphony algorithm, reference parameters, %-24s %.16e  rel. to Symphony-C %+.4e   (%d samples)"
          % (name + ":", v, v / gold - 1, ne))
for eg, en, tail, nd in ((1e-6, 1e-6, 1e8, 30), (1e-8, 1e-8, 1e8, 30), (1e-6, 1e-6, 1e8, 300), (1e-3, 1e-3, 1e5, 300)):
    v, ne, _ = run(libm, Tuning(eg, en, tail, nd, 1 << 20, 4096))
    print("2. tightened: eps_gamma %g eps_n %g tail 1/%g discrete %3d:            %.16e  rel. to Symphony-C %+.4e   (%d samples)"
          % (eg, en, tail, nd, v, v / gold - 1, ne))

# 3. independent: exact Bessel functions, plain harmonic sum (tests/exact_symphony.py)
import exact_symphony
dist = exact_symphony.power_law(p, 1.0, 1e12, 1e10)
values, errors, harmonics, _ = exact_symphony.coefficients(dist, s, th, max_harmonics=200000, allow_truncated=True)
truth = values[slot] * scale
print("3. exact J_n (scipy), plain sum over %d harmonics, error estimate %.1e:           %.16e  rel. to Symphony-C %+.4e"
      % (harmonics, errors[slot] / abs(values[slot]), truth, truth / gold - 1))
v, _, _ = run(libm)
print("   rimphony default vs exact: %+.4e ; Symphony-C vs exact: %+.4e" % (v / truth - 1, gold / truth - 1))
