"""Stored reference side of tools/check_literals.py and tools/check_formulas.py.

Both tools derive each quantity of the reference (a polynomial, a formula, a constant) from its source text and prove
the project's own version of it identical.  Where the reference sources are not at hand, they compare with what a run
against the sources stored instead (tests/golden/check_*.json):
  * for every symbolic quantity, its value at NPOINTS sample points, to DIGITS significant digits -- the value of each
    free symbol at sample point k is drawn from the symbol's NAME and k alone, so both sides are evaluated at the
    same points without sharing any expression (an undefined function application such as besseli(1/3, x) counts
    as one symbol);
  * for every plain datum (a constant's literal, the lobe table), the datum itself.
A sign flip or an altered coefficient changes the values at every point; the record run checks that the comparison
of values agrees with the symbolic one for every quantity.

    python tools/check_literals.py --record [REF]    where the reference is mounted: (re)write the stored side
    python tools/check_literals.py --golden          compare with the stored side even where the reference is mounted
"""
import hashlib
import json
import os

import mpmath as mp
import sympy as sp
from sympy.core.function import AppliedUndef

NPOINTS = 4
DIGITS = 60          # evaluation precision
STORED = 45          # significant digits kept
TOL = mp.mpf(10) ** -30


def _point(name, k):
    """Sample value of the symbol `name` at point k: a rational in [5/4, 13/4), fixed by (name, k)."""
    u = int.from_bytes(hashlib.sha256(("%s#%d" % (name, k)).encode()).digest()[:8], "little")
    return sp.Rational(5, 4) + sp.Rational(2 * (u % 1000003), 1000003)


def fingerprint(expr):
    """[(re, im)] of `expr` at the NPOINTS sample points, as decimal strings."""
    expr = sp.sympify(expr)
    apps = sorted(expr.atoms(AppliedUndef), key=str)
    if apps:
        expr = expr.xreplace({a: sp.Symbol("{%s}" % a) for a in apps})
    syms = sorted(expr.free_symbols, key=lambda s: s.name)
    out = []
    for k in range(NPOINTS):
        v = sp.N(expr.xreplace({s: _point(s.name, k) for s in syms}), DIGITS)
        re_, im_ = (sp.re(v), sp.im(v)) if v.is_finite is not False else (sp.nan, sp.nan)
        out.append([sp.N(re_, STORED).__str__(), sp.N(im_, STORED).__str__()])
    return out


def _close(a, b):
    with mp.workdps(DIGITS):
        for (ar, ai), (br, bi) in zip(a, b):
            if "nan" in (ar + ai + br + bi):
                if [ar, ai] != [br, bi]:
                    return False
                continue
            x, y = mp.mpc(mp.mpf(ar), mp.mpf(ai)), mp.mpc(mp.mpf(br), mp.mpf(bi))
            if abs(x - y) > TOL * max(abs(x), abs(y)):
                return False
    return len(a) == len(b) == NPOINTS


class Reference:
    """`mounted`: the reference's text is read (symbolic comparison); otherwise the stored side is used."""

    def __init__(self, ref_dir, store, argv):
        self.store = store
        self.record = "--record" in argv
        self.mounted = os.path.isdir(ref_dir) and "--golden" not in argv
        if self.record and not self.mounted:
            raise SystemExit("--record needs the reference sources (%s)" % ref_dir)
        self.data = {"values": {}, "data": {}}
        if not self.record:
            if not self.mounted and not os.path.exists(store):
                raise SystemExit("reference not mounted and no stored reference side (%s)" % store)
            if not self.mounted:
                self.data = json.load(open(store))
        self.disagreements = []
        self._seen = {}

    def key(self, name):
        """`name`, made unique in the order of the calls (a label may recur)."""
        n = self._seen.get(name, 0)
        self._seen[name] = n + 1
        return name if n == 0 else "%s #%d" % (name, n + 1)

    def datum(self, key, compute):
        """A plain datum of the reference: compute() where mounted (and recorded), else the stored value."""
        if self.mounted:
            v = compute()
            if self.record:
                self.data["data"][key] = v
            return v
        if key not in self.data["data"]:
            raise KeyError("no stored reference datum %r" % key)
        return self.data["data"][key]

    def compare(self, key, ours, ref, symbolic):
        """Where mounted: symbolic() decides (and a record run stores ref's values, checking that the values of the two
        sides agree as the symbolic comparison says).  Else: ours' values against the stored ones."""
        if self.mounted:
            ok = symbolic()
            if self.record:
                fr = fingerprint(ref)
                self.data["values"][key] = fr
                try:
                    agree = _close(fingerprint(ours), fr) == ok
                except Exception:            # a quantity missing on the project's side: DIFFERENT either way
                    agree = not ok
                if not agree:
                    self.disagreements.append(key)
            return ok
        if key not in self.data["values"]:
            return False
        try:
            return _close(fingerprint(ours), self.data["values"][key])
        except Exception:
            return False

    def has(self, key):
        return self.mounted or key in self.data["values"]

    def save(self):
        if not self.record:
            return
        if self.disagreements:
            raise SystemExit("values and symbolic comparison disagree for: %s" % "; ".join(self.disagreements))
        with open(self.store, "w") as f:
            json.dump(self.data, f, indent=0, sort_keys=True)
            f.write("\n")
        print("stored reference side: %s (%d quantities, %d data)" % (os.path.relpath(self.store), len(self.data["values"]),
                                                                       len(self.data["data"])))
