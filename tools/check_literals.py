#!/usr/bin/env python3
"""Cross-check of every coefficient table of the Leung Bessel evaluator and of the Heyvaerts elements against the
REFERENCE SOURCES, with sign and position.

Bit-exact parity tests compare the kernels with oracle/, which shares these tables' transcription (they were typed
once); a wrong sign or a swapped coefficient would pass every such test.  This tool closes that hole where the
reference is mounted (/root/reference; build container only -- it is never run on the GPU box and reads the reference
as DATA: no header stand-ins, nothing compiled):

  * each polynomial of leung-bessel/src/bessel.c (Meissel "first": V_n parts 1 and 2, the small-epsilon series, the
    1/(1+Z) series; Meissel "second": P_n and Q_n sums; the Debye epsilon expansion; exp_factor's Taylor series) is
    taken from the C source as TEXT, turned into an exact sympy expression (every literal an exact rational), and
    expanded;
  * the corresponding straight-line code of rimphony_amd/csrc/dev_bessel.h (Horner chains of rim_fma / rim_fma_k) and
    of oracle/rimo_bessel.c is executed symbolically the same way;
  * the two expanded polynomials must be IDENTICAL -- every coefficient of every monomial, sign included.
  The same for the non-resonant Faraday elements h_nr / f_nr and the quasi-resonant combinations of src/heyvaerts.rs
  (Rust method syntax rewritten to infix by regular expressions), the constants of heyvaerts.rs:28-33, the region
  intercepts and slope of bessel.c:313-316, and the At[m] table (bessel.c:171-174) against mpmath.

Where the reference is not mounted (or with --golden), the reference side is the one stored in
tests/golden/check_literals.json by `--record` (tools/ref_golden.py): the project's side is compared with its values.

Exit status 0 = everything identical.  usage: python tools/check_literals.py [--golden | --record] [/root/reference]"""
import os
import re
import sys

import sympy as sp

import ref_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
REF = _ARGS[0] if _ARGS else "/root/reference"
G = ref_golden.Reference(REF, os.path.join(ROOT, "tests", "golden", "check_literals.json"), sys.argv[1:])
Z = sp.S.Zero           # stands in for a reference quantity that is not derived here (the stored side is compared)
NUM = re.compile(r"(?<![\w.])(\d+\.?\d*(?:[eE][-+]?\d+)?|\.\d+(?:[eE][-+]?\d+)?)(?![\w.(])")
failures = []


def exact(text):
    """Arithmetic text -> the same text with every numeric literal an exact Rational."""
    return NUM.sub(lambda m: 'R("%s")' % m.group(1), text)


def ev(text, env):
    e = dict(env)
    e["R"] = sp.Rational
    return eval(exact(text), {"__builtins__": {}}, e)


def c_statement(src, name):
    """The right-hand side of `const double NAME = ...;` in C source text."""
    m = re.search(r"const\s+double\s+" + re.escape(name) + r"\s*=\s*(.*?);", src, re.S)
    if not m:
        raise SystemExit("reference statement %s not found" % name)
    return re.sub(r"//[^\n]*", "", m.group(1)).replace("\n", " ")


def run_chain(body, env):
    """Execute straight-line C/C++ assignments (const double x = ...; x = ...;) symbolically; returns the env."""
    e = {}
    e.update({"R": sp.Rational, "rim_fma": lambda a, b, c: a * b + c, "rim_fma_k": lambda a, b, c: a * b + c,
              "fma": lambda a, b, c: a * b + c, "FMA": lambda a, b, c: a * b + c,
              "rim_div_by": lambda a, b, binv: a / b, "rim_div_moderate": lambda a, b: a / b, "rim_head": lambda a: a,
              "rim_sqrt": sp.sqrt, "m_sqrt": sp.sqrt, "sqrt": sp.sqrt,
              "rim_pow15": lambda x: x ** sp.Rational(3, 2), "rim_pow25": lambda x: x ** sp.Rational(5, 2),
              "m_pow15": lambda x: x ** sp.Rational(3, 2), "m_pow25": lambda x: x ** sp.Rational(5, 2)})
    e.update(env)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    body = re.sub(r"//[^\n]*", "", body)
    for stmt in body.split(";"):
        stmt = stmt.strip().replace("\n", " ")
        stmt = re.split(r"[{}]", stmt)[-1].strip()          # drop a function head or a closing brace in front
        if not stmt or "=" not in stmt:
            continue
        stmt = re.sub(r"^(const\s+)?double\s+", "", stmt)
        lhs, rhs = stmt.split("=", 1)
        lhs = lhs.strip().lstrip("*")
        if not re.match(r"^\w+$", lhs):
            continue
        try:
            e[lhs] = eval(exact(rhs.strip()), {"__builtins__": {}}, e)
        except Exception:
            e.pop(lhs, None)          # a statement outside the arithmetic being checked (struct fields, calls)
    return e


def between(text, start, stop):
    i = text.index(start)
    j = text.index(stop, i)
    return text[i:j]


def same(name, ours, ref):
    def symbolic():
        d = sp.expand(sp.together(ours - ref))
        if d != 0:
            d = sp.simplify(d)
        return d == 0
    ok = G.compare(G.key(name), ours, ref, symbolic)
    print("%-62s %s" % (name, "identical" if ok else "DIFFERENT"))
    if not ok:
        failures.append(name)


def main():
    mounted = G.mounted
    if not mounted:
        print("reference side: stored values (tests/golden/check_literals.json)")
    bc = open(os.path.join(REF, "leung-bessel", "src", "bessel.c")).read() if mounted else None
    # (RIMPHONY_CHECK_DEV_BESSEL: another file in place of dev_bessel.h -- the test suite feeds a mutated copy to
    # show that a flipped sign is caught)
    dev = open(os.environ.get("RIMPHONY_CHECK_DEV_BESSEL") or os.path.join(ROOT, "rimphony_amd", "csrc", "dev_bessel.h")).read()
    orc = open(os.path.join(ROOT, "oracle", "rimo_bessel.c")).read()
    t1, t2, U, eps, Z_, ninv, n, x, z, ez, t3, t4, t10 = sp.symbols("t1 t2 U eps Z ninv n x z ez t3 t4 t10")
    At = sp.symbols("At0:16")

    # ---------------- Meissel "first" (bessel.c:94-149) ----------------
    ref_v1 = ref_v2 = ref_lg = ref_e2 = ref_iz = Z
    if mounted:
        first = between(bc, "BesselJ_Meissel_First(const double n", "/* The Debye")
        ref_v1 = ev(c_statement(first, "Vsum1"), {"U": U, "t1": t1})
        ref_v2 = ev(c_statement(first, "Vsum2"), {"ninv": ninv, "t2": t2})
        ref_lg = ev(c_statement(first, "loggamma_exp"), {"ninv": ninv, "t2": t2, "t3": t2 * t2})
        ref_e2 = ev(c_statement(first, "exp2").replace("sqrt(2.*eps)", "S"), {"n": n, "eps": eps, "S": sp.Symbol("S")})
        m = re.search(r"invZp1\s*=\s*(1 \+ .*?);", first, re.S)
        ref_iz = ev(m.group(1).replace("\n", " "), {"Z": Z_})

    # (oracle/rimo_bessel.c keeps these coefficients in tables walked by loops -- a structurally different
    # transcription; it is held to dev_bessel.h bit for bit by tests/test_host_side.py and the GPU parity tests, so
    # what is proved here for dev_bessel.h holds for it too)
    for label, text, fn in (("dev_bessel.h", dev, "RIM_DEV double meissel_first("),):
        body = between(text, fn, "exp_factor(factor, exp_val)")
        chain = between(body, "double v, ak;" if "double v, ak;" in body else "const double t = z * z;", "const double factor")
        e = run_chain(chain, {"t": t1, "U": U, "z": sp.sqrt(t1)})
        same("Meissel-first V_n part 1 (bessel.c:108-118)  vs %s" % label, e["vsum1"], ref_v1)
        small = between(body, "if (eps < 1e-4", "} else {")
        e = run_chain(small, {"eps": eps, "n": n, "rim_sqrt": lambda a: sp.Symbol("S"), "m_sqrt": lambda a: sp.Symbol("S"),
                              "o": None})
        same("Meissel-first small-eps series (bessel.c:131-135) vs %s" % label, e["exp2"], ref_e2)
        series = between(body, "if (Z < 1.e-3) {", "} else {" if label == "dev_bessel.h" else "else")
        e = run_chain(series.replace("invZp1 = q", "res = q"), {"Z": Z_})
        same("Meissel-first 1/(1+Z) series (bessel.c:143)      vs %s" % label, e.get("res", e.get("invZp1")), ref_iz)
    # order-only pieces hoisted into leung_order (dev) / computed in place (oracle)
    lo = between(dev, "RIM_DEV LeungOrder leung_order(double n)", "return o;")
    e = run_chain(lo.replace("o.", "o_"), {"n": n, "rim_log10": lambda a: sp.Symbol("L10"), "guard_pow10": lambda a: a,
                                           "rim_lgamma_pos": lambda a: sp.Symbol("LG"), "rim_log": lambda a: sp.Symbol("LOG"),
                                           "RIM_PI": sp.pi})
    same("Meissel-first V_n part 2 (bessel.c:121)             vs dev_bessel.h", e["o_vsum2"].subs(1 / n, ninv), ref_v2.subs(t2, ninv ** 2))
    same("log-gamma 1/n^k part (bessel.c:130)                 vs dev_bessel.h", e["loggamma_exp"].subs(1 / n, ninv), ref_lg.subs(t2, ninv ** 2))
    for nm, val in (("thr_lo", "0.174857"), ("thr_hi", "0.295966"), ("thr_plus_lo", "0.151550")):
        refv = {"thr_lo": "MINUS_ETA_A_INTERCEPT", "thr_hi": "MINUS_ETA_B_INTERCEPT", "thr_plus_lo": "PLUS_ETA_A_INTERCEPT"}[nm]
        want = Z
        if mounted:
            rm = re.search(r"const\s+double\s+" + refv + r"\s*=\s*([-\d.eE]+)", bc)
            # the slope literal as the reference writes it in its region test: "-0.6666666 * log10(n) + <intercept>"
            sl = re.search(r"(-?0\.6666666\d*)\s*\*\s*logn\s*\+\s*" + refv, bc)
            if sl is None:
                raise SystemExit("slope of the region test not found next to " + refv)
            want = sp.Rational(sl.group(1)) * sp.Symbol("L10") + sp.Rational(rm.group(1))
        ours = e["o_" + nm]
        same("region threshold %s (bessel.c:313-316)       vs dev_bessel.h" % nm.ljust(11), ours, want)
    pb = G.datum("PLUS_ETA_B_INTERCEPT",
                 lambda: re.search(r"const\s+double\s+PLUS_ETA_B_INTERCEPT\s*=\s*([-\d.eE]+)", bc).group(1))
    print("%-62s %s" % ("PLUS_ETA_B_INTERCEPT %s in dev_bessel.h bessel_j" % pb,
                        "present" if pb in between(dev, "RIM_DEV double bessel_j(", "RIM_DEV double bessel_dj(") else "MISSING"))
    if pb not in between(dev, "RIM_DEV double bessel_j(", "RIM_DEV double bessel_dj("):
        failures.append("PLUS_ETA_B_INTERCEPT")

    # ---------------- Meissel "second" (bessel.c:57-88) ----------------
    ref_p = ref_q = Z
    if mounted:
        second = between(bc, "BesselJ_Meissel_Second(const double n", "/* Meissel's \"first\"")
        ref_p = ev(c_statement(second, "exp_val"), {"t1": t1, "t2": t2})
        ref_q = ev(c_statement(second, "Qsum"), {"t1": t1, "t2": t2, "U": U})
    for label, text, fn in (("dev_bessel.h", dev, "RIM_DEV double meissel_second("),):
        if fn not in text:
            print("(no %s in %s)" % (fn, label))
            continue
        body = between(text, fn, "exp_factor(factor, exp_val)")
        chain = between(body, "const double t2 = U * U;", "const double factor")
        chain = re.sub(r"const double Qt[^;]*;", "", chain)
        e = run_chain(chain, {"t1": t1, "t2": t2, "U": U})
        same("Meissel-second P_n sum (bessel.c:66-71)              vs %s" % label, e["exp_val"], ref_p.subs(t2, U * U))
        same("Meissel-second Q_n sum (bessel.c:77-83)              vs %s" % label, e["Qsum"], ref_q.subs(t2, U * U))

    # ---------------- Debye epsilon expansion (bessel.c:159-213) ----------------
    ref_d = Z
    if mounted:
        deb = between(bc, "BesselJ_Debye_Eps_Exp(const double n", "#define MINUS_ETA_A_INTERCEPT" if "#define MINUS_ETA_A_INTERCEPT" in bc else "return t149;")
        env = {"At": list(At), "t3": t3, "t4": t4, "t10": t10, "z": z, "ez": ez, "x": x, "M_PI": sp.pi}
        env["t38"] = ev(c_statement(deb, "t38"), env)
        env["t44"] = x
        for nm in ("t70", "t93", "t107", "t114", "t146"):
            env[nm] = ev(c_statement(deb, nm), env)
        ref_d = ev(c_statement(deb, "t149"), env)
    atenv = {"RIM_AT%d" % k: At[k] for k in range(16)}
    atenv.update({"t3": t3, "t4": t4, "t10": t10, "z": z, "x": x, "ez": ez, "RIM_PI": sp.pi})
    body = between(dev, "RIM_DEV double debye_eps(double n, double x)", "// The same for two orders at one x")
    chain = between(body, "const double t146 = t10 * t10;", "return p /")
    e = run_chain("const double t146 = t10 * t10;" + chain, atenv)
    ours = e["p"] / (sp.pi * e["t146"] * sp.Rational("0.58354968672000000e17"))
    same("Debye epsilon expansion (bessel.c:183-211)            vs dev_bessel.h debye_eps", ours, ref_d)
    body = between(dev, "RIM_DEV void debye_eps_pair(", "// pkgw_bessel_j for n >= 30 given the hoisted order data")
    chain = between(body, "const double t146 = t10 * t10;", "const double den")
    atenv2 = dict(atenv)
    atenv2.update({"ez0": ez, "ez1": sp.Symbol("ez1")})
    e = run_chain("const double t146 = t10 * t10;" + chain, atenv2)
    same("   the same                                            vs dev_bessel.h debye_eps_pair (order 0)",
         e["p0"] / (sp.pi * e["t146"] * sp.Rational("0.58354968672000000e17")), ref_d)
    same("   the same                                            vs dev_bessel.h debye_eps_pair (order 1)",
         (e["p1"] / (sp.pi * e["t146"] * sp.Rational("0.58354968672000000e17"))).subs(sp.Symbol("ez1"), ez), ref_d)
    # At[m] = sin(pi M) 6^M Gamma(M), M = (m + 1) / 3: the reference fills the table at run time with libm
    # (bessel.c:171-174: sin(M_PI * M) * pow(6., M) * exp(lgamma(M))); leung_table.h freezes the doubles that expression
    # gives under glibc.  Python's math module calls the same libm: the literals must be those doubles, bit for bit
    # (and, for the record, how far libm's values are from the exact ones).
    import math
    import mpmath as mp
    mp.mp.dps = 40
    tab = open(os.path.join(ROOT, "rimphony_amd", "csrc", "leung_table.h")).read()
    worst, ok = 0., True
    for k in range(16):
        v = float(re.search(r"#define RIM_AT%-2d\s*\(([-\d.e+]+)\)" % k, tab).group(1))
        M = (k + 1) / 3.
        libm = math.sin(math.pi * M) * math.pow(6., M) * math.exp(math.lgamma(M))
        ok = ok and v == libm
        if k % 3 != 2:                      # integer M: sin(k pi) residue, never read by the expansion
            Mx = mp.mpf(k + 1) / 3
            exact_v = mp.sin(mp.pi * Mx) * mp.power(6, Mx) * mp.gamma(Mx)
            worst = max(worst, abs(float((mp.mpf(v) - exact_v) / exact_v)))
    print("%-62s %s (libm vs exact: max rel. %.2e)" % ("At[m] table (bessel.c:171-174) vs leung_table.h", "identical" if ok else "DIFFERENT", worst))
    if not ok:
        failures.append("At table")

    # ---------------- exp_factor Taylor series (bessel.c:22-51) ----------------
    fe = sp.Symbol("f_exp")
    refq = None
    ef_name = "exp_factor Taylor series (bessel.c:22-51)              vs dev_bessel.h"
    if mounted:
        ef = between(bc, "exp_factor(", "/* Meissel's \"second\"")
        for cand in re.findall(r"=\s*([^;]*40320[^;]*);|return\s+([^;]*40320[^;]*);", ef, re.S):
            txt = (cand[0] or cand[1]).replace("\n", " ")
            try:
                refq = ev(txt, {"f_exp": fe, "f_factor": sp.Symbol("F"), "x": fe})
                break
            except Exception:
                continue
    elif G.has(ef_name):
        refq = Z
    body = between(dev, "if (a < 1e-3) {", "}")
    e = run_chain(body.replace("return ", "res = "), {"f_exp": fe, "f_factor": sp.Symbol("F")})
    if refq is not None:
        same(ef_name, e["res"], refq)
    else:
        print("exp_factor series: reference expression not isolated (skipped)")

    # ---------------- heyvaerts.rs ----------------
    hv = open(os.path.join(REF, "src", "heyvaerts.rs")).read() if mounted else None
    dh = open(os.path.join(ROOT, "rimphony_amd", "csrc", "dev_heyvaerts.h")).read()
    oh = open(os.path.join(ROOT, "oracle", "rimo_heyvaerts.c")).read()
    for rust, ours in (("FOUR_OVER_SQRT_27", "RIM_FOUR_OVER_SQRT_27"), ("INVERSE_SQRT_3", "RIM_INVERSE_SQRT_3"),
                       ("SQRT_8_OVER_3", "RIM_SQRT_8_OVER_3"), ("THREE_TWO_THIRDS", "RIM_THREE_TWO_THIRDS"),
                       ("G_APPROXIMATION_CUTOFF", "RIM_G_APPROXIMATION_CUTOFF")):
        rv = G.datum("constant " + rust, lambda: re.search(r"const\s+" + rust + r":\s*f64\s*=\s*([-\d.eE]+)", hv).group(1))
        ov = re.search(r"#define\s+" + ours + r"\s+([-\d.eE]+)", dh).group(1)
        cv = re.search(r"#define\s+" + rust + r"\s+([-\d.eE]+)", oh)
        ok = float(rv) == float(ov) and (cv is None or float(cv.group(1)) == float(rv))
        print("%-62s %s" % ("constant %s = %s (heyvaerts.rs:28-33)" % (rust, rv), "identical" if ok else "DIFFERENT"))
        if not ok:
            failures.append(rust)

    def rust_fn(name):
        body = between(hv, "fn %s(&self) -> f64 {" % name, "\n    }\n")
        body = body[body.index("{") + 1:]
        body = re.sub(r"//[^\n]*", "", body)
        body = body.replace("self.", "").replace("f64::consts::PI", "PI")
        for _ in range(6):      # method calls -> infix / function calls, innermost first
            body = re.sub(r"(\w+)\.powi\((\d+)\)", r"((\1)**\2)", body)
            body = re.sub(r"\(([^()]*)\)\.powi\((\d+)\)", r"((\1)**\2)", body)
            body = re.sub(r"(\w+)\.powf\(([\d.]+)\)", r"POW(\1, \2)", body)
            body = re.sub(r"\(([^()]*)\)\.powf\(([\d.]+)\)", r"POW((\1), \2)", body)
            body = re.sub(r"(\w+)\.sqrt\(\)", r"SQRT(\1)", body)
            body = re.sub(r"\(([^()]*)\)\.sqrt\(\)", r"SQRT((\1))", body)
            body = re.sub(r"(\w+)\.bessel([ijy])\(([^()]*)\)", r"BESSEL\2(\1, \3)", body)
        return body

    sig, xx, po, s0sq, dfds, g = sp.symbols("sigma x pomega sigma0_sq dfds g")
    Bi, Bj, By = sp.Function("besseli"), sp.Function("besselj"), sp.Function("bessely")
    renv = {"sigma": sig, "x": xx, "pomega": po, "sigma0_sq": s0sq, "PI": sp.pi, "INVERSE_C": sp.Symbol("INVC"),
            "TWO_PI": 2 * sp.pi, "dfdsigma": lambda: dfds,
            "POW": lambda a, b: a ** sp.nsimplify(b), "SQRT": sp.sqrt,
            "BESSELi": lambda a, nu: Bi(sp.nsimplify(nu), a), "BESSELj": lambda a, nu: Bj(sp.nsimplify(nu), a),
            "BESSELy": lambda a, nu: By(sp.nsimplify(nu), a),
            "FOUR_OVER_SQRT_27": sp.Symbol("F427"), "INVERSE_SQRT_3": sp.Symbol("ISQ3"), "SQRT_8_OVER_3": sp.Symbol("S83")}

    def run_rust(name, branch=None):
        body = rust_fn(name)
        e = dict(renv)
        e["R"] = sp.Rational
        stmts, depth, cur = [], 0, ""
        for ch in body:                   # split on ';' outside braces (the if / else blocks hold statements too)
            if ch == "{":
                depth += 1
            elif ch == "}":
                depth -= 1
            if ch == ";" and depth == 0:
                stmts.append(cur)
                cur = ""
            else:
                cur += ch
        stmts.append(cur)
        last = None
        for st in stmts:
            st = st.strip().replace("\n", " ")
            if not st:
                continue
            mm = re.match(r"let\s+(\w+)\s*=\s*(.*)$", st, re.S)
            rhs = mm.group(2) if mm else st
            mi = re.match(r"if\s+g\s*<\s*G_APPROXIMATION_CUTOFF\s*\{(.*)\}\s*else\s*\{(.*)\}$", rhs.strip(), re.S)
            if mi:
                blk = mi.group(1 if branch == "small" else 2)
                sub = dict(e)
                val = None
                for s2 in re.split(r";", blk):
                    s2 = s2.strip()
                    if not s2:
                        continue
                    m2 = re.match(r"let\s+(\w+)\s*=\s*(.*)$", s2, re.S)
                    if m2:
                        sub[m2.group(1)] = eval(exact(m2.group(2)), {"__builtins__": {}}, sub)
                    else:
                        val = eval(exact(s2), {"__builtins__": {}}, sub)
                rhsv = val
            else:
                rhsv = eval(exact(rhs), {"__builtins__": {}}, e)
            if mm:
                e[mm.group(1)] = rhsv
            else:
                last = rhsv
        return last, e

    def run_dev(text, fn_start, fn_stop, branch=None, extra=None):
        body = between(text, fn_start, fn_stop)
        body = re.sub(r"RIM_PROF_\w+\([^;]*\);", "", body)
        body = re.sub(r"#if.*?#endif", "", body, flags=re.S)
        env = {"c": None, "pt": None, "RIM_PI": sp.pi, "RIM_INVERSE_C": sp.Symbol("INVC"), "INVERSE_C": sp.Symbol("INVC"),
               "RIM_FOUR_OVER_SQRT_27": sp.Symbol("F427"), "RIM_INVERSE_SQRT_3": sp.Symbol("ISQ3"),
               "RIM_SQRT_8_OVER_3": sp.Symbol("S83"), "FOUR_OVER_SQRT_27": sp.Symbol("F427"),
               "INVERSE_SQRT_3": sp.Symbol("ISQ3"), "SQRT_8_OVER_3": sp.Symbol("S83"), "TWO_PI": 2 * sp.pi}
        if extra:
            env.update(extra)
        body = body.replace("c.sigma", "sigma").replace("c.x", "x").replace("c.pomega", "pomega").replace("pt.sigma0_sq", "sigma0_sq")
        body = body.replace("st->sigma0_sq", "sigma0_sq").replace("st->sigma", "sigma").replace("st->x", "x").replace("st->pomega", "pomega")
        env.update({"sigma": sig, "x": xx, "pomega": po, "sigma0_sq": s0sq})
        body = re.sub(r"dfdsigma(<KIND>)?\([^)]*\)", "DFDS", body)
        env["DFDS"] = dfds
        body = body.replace("return ", "RESULT = ")
        return run_chain(body, env)

    # non-resonant elements: pure arithmetic
    nr_dev = between(dh, "RIM_DEV void nr_common(", "// want_h: the")
    nr_dev = nr_dev.replace("x_sq = c.x * c.x", "x_sq = x * x").replace("c.sigma", "sigma").replace("c.x", "x")
    common = run_chain(nr_dev, {"sigma": sig, "x": xx})
    # (round 3: the elements of dev_heyvaerts.h are the branches of hey_member, fed by hey_shared)
    member = between(dh, "RIM_DEV double hey_member(", "// The inner integrand of either regime")
    nr_q = member[member.index("const double u3 = u2 * u;"):member.index("const double z =")]
    nr_q = nr_q[:nr_q.rindex("}")]
    nr_v = member[member.index("const double z ="):]
    for fn, body in (("h_nr_element", nr_q), ("f_nr_element", nr_v)):
        ref = run_rust(fn)[0] if mounted else Z
        body = body.replace("sh.dfds", "dfdsigma()")
        e = run_dev("X;\n" + body + "\nEND", "X", "END", extra={k: common[k] for k in ("a1", "a2", "xa1p", "x_sq", "u", "u2")})
        same("%s (heyvaerts.rs:379-394 / 453-468)            vs dev_heyvaerts.h" % fn, e["RESULT"], ref)
        body = between(oh, "static double %s(const hey_state *st)" % fn, "\n}\n")
        e = run_dev(body + " ", "{", "return" if False else "\n", extra=None) if False else run_dev(oh, "static double %s(const hey_state *st)" % fn, "\n}\n")
        same("%s                                              vs oracle/rimo_heyvaerts.c" % fn, e["RESULT"], ref)

    # quasi-resonant elements, both branches, Bessel functions opaque
    gsym = sp.Symbol("S83") * (sig - xx) ** sp.Rational(3, 2) / sp.sqrt(xx)
    for fn in ("h_qr_element", "f_qr_element"):
        for branch in ("small", "large"):
            ref = run_rust(fn, branch)[0] if mounted else Z
            # oracle (a literal restatement: bessel calls in place)
            body = between(oh, "static double %s(const hey_state *st)" % fn, "\n}\n")
            body = re.sub(r"if \(g < G_APPROXIMATION_CUTOFF\) \{(.*?)\} else \{(.*?)\}",
                          lambda mo: mo.group(1 if branch == "small" else 2), body, flags=re.S)
            body = body.replace("double y;", "")
            env = {"rimo_bessel_i": lambda nu, a: Bi(sp.nsimplify(nu), a), "rimo_bessel_jnu": lambda nu, a: Bj(sp.nsimplify(nu), a),
                   "rimo_bessel_ynu": lambda nu, a: By(sp.nsimplify(nu), a)}
            # round 4: g comes from qr_g(st) (its literal branch is heyvaerts.rs:309, 406, checked here as that expression)
            # and the four Bessel values of the large-g branch from jy_set(), whose literal branch hands back exactly
            # these calls (oracle/rimo_heyvaerts.c jy_set)
            qr_g_src = between(oh, "static double qr_g(const hey_state *st)", "\n}\n")
            assert "return SQRT_8_OVER_3 * m_pow15(st->sigma - st->x) / m_sqrt(st->x);" in qr_g_src
            jy_src = between(oh, "static void jy_set(", "\n}\n")
            for line in ("*js = rimo_bessel_jnu(sigma, x);", "*jm1 = rimo_bessel_jnu(sigma - 1., x);", "*ys = rimo_bessel_ynu(sigma, x);",
                         "*ym1 = want_ym1 ? rimo_bessel_ynu(sigma - 1., x) : 0.;"):
                assert line in jy_src, line
            env.update({"st": None, "qr_g": lambda _st: gsym, "js": Bj(sig, xx), "ys": By(sig, xx), "jm1": Bj(sig - 1, xx), "ym1": By(sig - 1, xx)})
            body = body.replace("double js = 0., ys = 0., jm1 = 0., ym1 = 0.;", "").replace("double js, ys, jm1, ym1;", "")
            e = run_dev("X" + body + "\nEND", "X", "END", extra=env)
            same("%s, %s-g branch (heyvaerts.rs:302-373, 400-447) vs oracle/rimo_heyvaerts.c" % (fn, branch),
                 e["RESULT"].subs(sp.Symbol("g"), gsym) if False else e["RESULT"], ref)

    print()
    if failures:
        print("FAILED:", ", ".join(failures))
        return 1
    G.save()
    print("all tables identical to the reference sources")
    return 0


if __name__ == "__main__":
    sys.exit(main())
