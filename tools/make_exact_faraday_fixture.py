#!/usr/bin/env python3
"""Writes tests/golden/exact_faraday.npz and profiles/exact_faraday_deviation.txt.  CPU only, minutes on 8 cores.

The fixture pins the Faraday pair (rho_Q, rho_V: slots 6 and 7) of the four analytic kinds to tests/exact_faraday.py: the
two-dimensional integrals of Heyvaerts' elements by fixed Gauss-Legendre rules on scipy's Bessel functions.  Three layers:

  whole coefficients   ten rows (kind, parameters, s, theta) per kind.  Class A: sigma0 = s sin theta between 4 and 40, theta
                       below pi / 2, the marching loops end within a few chunks -- and warm enough that the chunks after the
                       first still carry 1e-4 of the value, so that a loop which stops early shows.  Class B: sigma0 < 3 (the J/Y branch and the
                       empty non-resonant region are live), theta > pi / 2, theta near 0.1, a hard gamma_max where the
                       distribution is still large (power-law kinds), k = 0.5 ... 3 (pitch-angle kinds; the value with
                       df/dmu = 0 is stored beside the value, so the share of the mu term is on record)
  inner integrals      single outer-integrand samples of two rows per kind, Q and V, non-resonant and quasi-resonant, the
                       latter on both sides of sigma = 3 and between 3 and 3.0197 (where g = 10 is crossed on the physical limit)
  one tabulated        the tilted_juettner surface of the Symphony fixture through TabulatedDistribution2DGrid.from_function and
  surface              the table oracle against the exact integrals of the same f(gamma, mu)

Every record stores the inputs, the exact value, its error estimate, the deterministic oracle's value as bits, both oracle
flavours' deviation from exact, and the bound 2 max(|det / exact - 1|, |libm / exact - 1|) + 100 x the relative error
estimate.  The bounds come from the CPU oracle alone.  The tool stops if a row breaks a condition of the fixture that it can
check and that does not depend on the machine: both flavours finite, the exact value's relative error estimate at most 1e-9
(coefficients) or 1e-8 (inner integrals).  A row that fails is replaced in ROWS.  Two conditions of a row it cannot hold that
way.  The deterministic oracle's time, under 50 ms per coefficient on one core, is measured and printed, with a warning for a
row above it, and is neither stored nor written to the table (the fixture must regenerate on a slower or busier machine).  "No
status bit set" is a property of the device path: the CPU oracle has no status, so only tests/test_gpu_exact_faraday.py
asserts it; a replacement row has to pass there before it is taken.

One coefficient pair of the mpmath twin (exact_faraday.coefficients_mp: its own domain limits, cuts and final factor) is stored
beside the double-precision value of the same point, and the oracle's values at the points of NAN_POINTS are recorded in the table.

usage: python tools/make_exact_faraday_fixture.py [--jobs N]"""
import argparse
import ctypes
import math
import multiprocessing
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import exact_faraday as ef
import exact_symphony as ex

PL, TJ, PPL, PK = 0, 1, 2, 3
SLOT_NAMES = ("rho_Q", "rho_V")

ROWS = [
    (TJ, [3.], 30., 0.4, "A"), (TJ, [10.], 30., 0.25, "A"), (TJ, [20.], 15., 0.3, "A"), (TJ, [20.], 20., 0.4, "A"), (TJ, [40.], 30., 0.25, "A"),
    (TJ, [1.], 12., 0.2, "B"), (TJ, [1.], 25., 0.1, "B"), (TJ, [3.], 10., 2.2, "B"), (TJ, [1.], 12., 2.95, "B"), (TJ, [0.3], 6., 2.7, "B"),
    (PK, [5., 10., 3., 100.], 20., 0.3, "A"), (PK, [5., 10., 3., 100.], 4.5, 1.1, "A"), (PK, [4., 8., 2.4, 100.], 6., 1.0, "A"),
    (PK, [3.5, 5., 1.3, 50.], 4.5, 1.1, "A"), (PK, [4., 8., 2.4, 100.], 10., 0.9, "A"),
    (PK, [5., 1., 2.4, 10.], 25., 0.1, "B"), (PK, [4., 2., 3., 20.], 12., 0.2, "B"), (PK, [4., 1.5, 0.5, 8.], 10., 2.2, "B"),
    (PK, [4., 2., 3., 20.], 6., 2.7, "B"), (PK, [3.5, 3., 1.3, 5.], 40., 0.1, "B"),
    (PL, [2.2, 1.5, 1000., 200.], 16., 1.35, "A"), (PL, [2.2, 1.5, 1000., 200.], 25., 1.0, "A"), (PL, [2.2, 1.2, 2000., 300.], 8., 1.4, "A"),
    (PL, [2.2, 1.2, 2000., 300.], 35., 1.1, "A"), (PL, [2.5, 1.2, 300., 100.], 6., 1.0, "A"),
    (PL, [3.5, 1.5, 20., 100.], 10., 2.2, "B"), (PL, [3., 1.05, 1000., 10.], 12., 0.2, "B"), (PL, [3., 1.05, 1000., 10.], 30., 0.09, "B"),
    (PL, [3., 1.05, 1000., 10.], 4., 2.5, "B"), (PL, [3., 1.2, 40., 30.], 5., 0.5, "B"),
    (PPL, [2.2, 2.4, 1.5, 1000., 200.], 8., 1.4, "A"), (PPL, [2.2, 0.5, 1.5, 1000., 200.], 16., 1.35, "A"),
    (PPL, [2.2, 3., 1.2, 2000., 300.], 5., 1.3, "A"), (PPL, [2.2, 3., 1.2, 2000., 300.], 25., 1.0, "A"),
    (PPL, [2.2, 2.4, 1.5, 1000., 200.], 35., 1.1, "A"),
    (PPL, [3., 2.4, 1.05, 1000., 10.], 5., 0.5, "B"), (PPL, [3., 1.3, 1.05, 1000., 10.], 40., 0.1, "B"),
    (PPL, [3., 0.5, 1.05, 1000., 10.], 10., 2.2, "B"), (PPL, [3.5, 3., 1.5, 20., 100.], 10., 2.2, "B"),
    (PPL, [3., 2.4, 1.05, 1000., 10.], 4., 2.5, "B"),
]
PITCH_COLUMN = {PPL: 1, PK: 2}
MAX_MS = 50.
# the rows whose outer-integrand samples are stored: per kind one of class A and one with sigma0 < 3
INNER_ROWS = [0, 5, 10, 16, 20, 26, 30, 35]
# the tilted_juettner surface of tools/make_exact_symphony_fixture.py, and two points: one per hemisphere
SURFACE_POINTS = [(8., 0.7), (10., 2.2)]
# the point of the mpmath twin: cold (a small domain), sigma0 < 3 (the J/Y form, the empty non-resonant region and every seam inside)
MP_POINT = (TJ, [0.15], 2., 1.1)
MP_DIGITS, MP_POINTS = 20, 24
# points met during the row search at which the oracle returns NaN: recorded in the table, not part of the fixture
NAN_POINTS = [(TJ, [10.], 2.5, 2.2), (PK, [3.5, 3., 1.3, 5.], 1., 1.0), (PL, [2.2, 3., 30., 100.], 3., 2.9)]


def inner_abscissae(s, theta):
    """(qr, u) of the stored samples of a row: five non-resonant pomega on both sides of 0, five quasi-resonant sigma -- below
    3, between 3 and the g = 10 root and beyond it when sigma0 < 3, else from the lower limit upwards"""
    s0 = s * math.sin(theta)
    nr = [-3. * s0, -1.5 * s0, 0.4 * s0, 2. * s0, 4. * s0] if s0 > 3. else [-9., -4., 3.1, 5., 12.]
    low = max(s0, s0 ** 1.5 / math.sqrt(3.))
    qr = [low * f for f in (1.001, 1.1, 1.5, 2.5, 5.)] if s0 > 3. else [0.5 * (s0 + 3.), 2.99, 0.5 * (3. + ef.SIGMA_G10), 3.5, 7.]
    return [(0, u) for u in nr] + [(1, u) for u in qr]


def coefficient_row(row):
    kind, par, s, theta, _ = row
    dist = ex.make(kind, par)
    val, err, split = ef.coefficients(dist, s, theta)
    nomu = ef.coefficients(dist, s, theta, mu_term=False)[0] if kind in PITCH_COLUMN else val
    return val, err, split, nomu


def inner_row(i):
    kind, par, s, theta, _ = ROWS[i]
    dist = ex.make(kind, par)
    out = []
    for stokes in (ef.STOKES_Q, ef.STOKES_V):
        for qr, u in inner_abscissae(s, theta):
            v, e = ef.inner_integral(dist, stokes, s, theta, qr, [u])
            out.append((i, stokes, qr, u, v[0], e[0]))
    return out


def surface_distribution():
    from make_exact_symphony_fixture import SURFACE
    return ex.tilted_juettner(*SURFACE[:4]), SURFACE


def surface_table():
    from rimphony_amd import api
    dist, (T, a, lo, hi, nn, nmu) = surface_distribution()
    return api.TabulatedDistribution2DGrid.from_function(
        lambda g, mu: g * np.sqrt(g * g - 1.) * dist.f(g, mu, np), api.grid_nodes_log_gm1(lo, hi, nn), nmu)


def surface_point(point):
    return ef.coefficients(surface_distribution()[0], *point)


def oracle_faraday(L, row):
    """(rho_Q, rho_V) of one row on one thread, and the milliseconds per coefficient"""
    import oracle_bind
    kind, par, s, theta, _ = row
    t0 = time.perf_counter()
    out = oracle_bind.batch(L, kind, [s], [theta], [np.array([p]) for p in par], 0xC0, 1)[0, 6:]
    return out, 0.5e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "exact_faraday.npz"))
    ap.add_argument("--table", default=os.path.join(ROOT, "profiles", "exact_faraday_deviation.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import oracle_bind
    from rimphony_amd import _build
    _build.build_oracle()
    det, libm = oracle_bind.load("det"), oracle_bind.load("libm")

    # the oracle first, alone on the machine: its time is printed, not stored
    o_det, o_libm, ms = np.zeros((len(ROWS), 2)), np.zeros((len(ROWS), 2)), np.zeros(len(ROWS))
    for i, row in enumerate(ROWS):
        o_det[i], ms[i] = oracle_faraday(det, row)
        ms[i] = min(ms[i], oracle_faraday(det, row)[1])
        o_libm[i], _ = oracle_faraday(libm, row)
    problems = ["row %d %r: oracle %r / %r" % (i, ROWS[i], o_det[i], o_libm[i]) for i in range(len(ROWS))
                if not (np.isfinite(o_det[i]).all() and np.isfinite(o_libm[i]).all())]
    print("deterministic oracle, ms per coefficient on one core, per row: " + " ".join("%.0f" % v for v in ms))
    for i in np.flatnonzero(ms >= MAX_MS):
        print("WARNING: row %d %r took %.0f ms per coefficient here; the rows are meant to stay under %g ms" % (i, ROWS[i], ms[i], MAX_MS))

    with multiprocessing.Pool(args.jobs) as pool:
        coeff = pool.map_async(coefficient_row, ROWS, chunksize=1)
        inner = pool.map_async(inner_row, INNER_ROWS, chunksize=1)
        surf = pool.map_async(surface_point, SURFACE_POINTS, chunksize=1)
        coeff, inner, surf = coeff.get(), inner.get(), surf.get()
        mp_value = ef.coefficients_mp(*MP_POINT, MP_DIGITS, MP_POINTS, pool_map=lambda f, jobs: pool.map(f, jobs, chunksize=4))
    mp_exact, mp_err, _ = ef.coefficients(ex.make(*MP_POINT[:2]), *MP_POINT[2:])

    lines = ["Deviation of the CPU oracle's Faraday pair from the converged Heyvaerts integrals (tests/exact_faraday.py), tools/make_exact_faraday_fixture.py",
             "bound = 2 max(|det / exact - 1|, |libm / exact - 1|) + 100 x relative error estimate of the exact value", "",
             "whole coefficients: kind, class, parameters, s, theta, sigma0; per slot exact, relative error estimate,",
             "|det/exact-1|, |libm/exact-1|, bound, quasi-resonant share of the value, share of the mu term (1 - value with df/dmu = 0 / value)"]
    rec = {k: [] for k in ("row", "slot", "exact", "err", "nomu", "qr_share", "det_bits", "dev_det", "dev_libm", "bound")}
    for i, (row, (val, err, split, nomu)) in enumerate(zip(ROWS, coeff)):
        kind, par, s, theta, cls = row
        lines.append("%-16s %s %-30s s = %-4g theta = %-5g sigma0 = %-6.3g" % (ex.KINDS[kind], cls, par, s, theta, s * math.sin(theta)))
        for k in range(2):
            dd, dl = abs(o_det[i, k] / val[k] - 1.), abs(o_libm[i, k] / val[k] - 1.)
            rel = err[k] / abs(val[k])
            bound = 2. * max(dd, dl) + 100. * rel
            if not (rel <= 1e-9 and np.isfinite(bound)):
                problems.append("row %d %r %s: exact %r, relative error estimate %.2e" % (i, row, SLOT_NAMES[k], val[k], rel))
            lines.append("    %-6s %+.15e %.1e  %.2e %.2e %.2e  qr %+.3f  mu %+.3e" % (
                SLOT_NAMES[k], val[k], rel, dd, dl, bound, split[k, 1] / val[k], 1. - nomu[k] / val[k]))
            for key, v in zip(rec, (i, k, val[k], err[k], nomu[k], split[k, 1] / val[k], o_det[i:i + 1, k].view(np.uint64)[0], dd, dl, bound)):
                rec[key].append(v)

    # ---- inner integrals
    irec = {k: [] for k in ("row", "stokes", "qr", "u", "exact", "err", "det_bits", "dev_det", "dev_libm", "bound")}
    lines += ["", "inner integrals (one outer-integrand sample each): row, stokes, quasi-resonant, abscissa; exact, relative error estimate, |det/exact-1|, |libm/exact-1|, bound"]
    for group in inner:
        for i, stokes, qr, u, val, err in group:
            kind, par, s, theta, _ = ROWS[i]
            od, ol = (L.rimo_hey_outer_integrand(ctypes.byref(oracle_bind.mkdist(L, kind, par)[0]), stokes, s, theta, qr, u) for L in (det, libm))
            rel = err / abs(val) if val != 0. else math.inf
            dd, dl = (abs(o / val - 1.) if val != 0. else math.inf for o in (od, ol))
            bound = 2. * max(dd, dl) + 100. * rel
            if not (rel <= 1e-8 and np.isfinite(bound) and np.isfinite(od) and np.isfinite(ol)):
                problems.append("inner integral row %d stokes %d qr %d u %r: exact %r (%.2e), oracle %r / %r" % (i, stokes, qr, u, val, rel, od, ol))
            lines.append("    row %2d %s %s u = %-22r %+.15e %.1e  %.2e %.2e %.2e" % (i, "QV"[stokes - 1], "qr" if qr else "nr", u, val, rel, dd, dl, bound))
            for key, v in zip(irec, (i, stokes, qr, u, val, err, np.array([od]).view(np.uint64)[0], dd, dl, bound)):
                irec[key].append(v)

    R = {k: np.array(v) for k, v in rec.items()}
    IN = {k: np.array(v) for k, v in irec.items()}
    lines += ["", "summary, whole coefficients: kind class slot: rows, max deviation (either flavour), max bound, max |share of the mu term|"]
    for kind in (TJ, PK, PL, PPL):
        for cls in "AB":
            rows = [i for i, r in enumerate(ROWS) if r[0] == kind and r[4] == cls]
            for k in range(2):
                m = np.isin(R["row"], rows) & (R["slot"] == k)
                lines.append("%-16s %s %-6s %2d rows  dev %.2e  bound %.2e  mu %.2e" % (
                    ex.KINDS[kind], cls, SLOT_NAMES[k], m.sum(), np.maximum(R["dev_det"][m], R["dev_libm"][m]).max(), R["bound"][m].max(),
                    np.abs(1. - R["nomu"][m] / R["exact"][m]).max()))
    lines += ["", "summary, inner integrals: kind, part: records, max deviation, median deviation"]
    ikind = np.array([ROWS[i][0] for i in IN["row"]])
    for kind in (TJ, PK, PL, PPL):
        for qr in (0, 1):
            d = np.maximum(IN["dev_det"], IN["dev_libm"])[(ikind == kind) & (IN["qr"] == qr)]
            lines.append("%-16s %s %3d records  max %.2e  median %.2e" % (ex.KINDS[kind], "qr" if qr else "nr", len(d), d.max(), np.median(d)))

    # ---- the tabulated surface through the table oracle
    import tab2d_grid_bind
    table = surface_table()
    assert tab2d_grid_bind.set_tables(table.gamma, table.log_n) == 0
    sp = np.array(SURFACE_POINTS)
    tab, _ = tab2d_grid_bind.batch(sp[:, 0].copy(), sp[:, 1].copy(), np.zeros(len(sp)), 0xC0)
    s_exact, s_err = np.array([r[0] for r in surf]), np.array([r[1] for r in surf])
    s_dev = np.abs(tab[:, 6:] / s_exact - 1.)
    s_bound = 2. * s_dev + 100. * s_err / np.abs(s_exact)
    if not (np.isfinite(s_bound).all() and (s_err <= 1e-9 * np.abs(s_exact)).all()):
        problems.append("tabulated surface: oracle %r exact %r error estimate %r" % (tab[:, 6:], s_exact, s_err))
    lines += ["", "tabulated surface f = exp(-gamma / T + a (gamma - 1) mu), (T, a, gamma_lo, gamma_hi, nodes, mu nodes) = %r:" % (surface_distribution()[1],),
              "table oracle's |value / exact - 1| for rho_Q, rho_V, then the bounds"]
    for pt, d, b in zip(SURFACE_POINTS, s_dev, s_bound):
        lines.append("  s = %g theta = %g  %.2e %.2e   %.2e %.2e" % (pt + tuple(d) + tuple(b)))
    mp_dev = np.abs(mp_exact / mp_value - 1.)
    if not (mp_dev <= 1e-8).all():
        problems.append("mpmath twin at %r: %r against %r" % (MP_POINT, mp_value, mp_exact))
    lines += ["", "mpmath twin (coefficients_mp, %d digits, %d points per outer piece) at %s %r s = %g theta = %g:" % ((MP_DIGITS, MP_POINTS, ex.KINDS[MP_POINT[0]]) + MP_POINT[1:]),
              "  rho_Q %+.12e  rho_V %+.12e   |double / twin - 1| = %.1e %.1e" % (tuple(mp_value) + tuple(mp_dev)),
              "", "points met during the row search at which the oracle returns NaN (both flavours: det, libm); the reference itself could not be run:"]
    for kind, par, s, theta in NAN_POINTS:
        od, ol = (oracle_bind.batch(L, kind, [s], [theta], [np.array([p]) for p in par], 0xC0, 1)[0, 6:] for L in (det, libm))
        lines.append("  %-16s %-22r s = %-4g theta = %-4g  rho_Q %r / %r   rho_V %r / %r" % (ex.KINDS[kind], par, s, theta, float(od[0]), float(ol[0]), float(od[1]), float(ol[1])))
    print("\n".join(lines))
    if problems:
        print("\nNOT WRITTEN, conditions broken:\n" + "\n".join(problems))
        return 1
    keep = ""
    if os.path.exists(args.table):          # the recorded study below the table is kept (tools/faraday_full_kernel_study.py writes it)
        old = open(args.table).read()
        keep = old[old.index("\nfull Bessel kernel"):] if "\nfull Bessel kernel" in old else ""
    open(args.table, "w").write("\n".join(lines) + "\n" + keep)

    f32 = np.float32
    np.savez_compressed(
        args.out,
        row_kind=np.array([r[0] for r in ROWS], dtype=np.int8),
        row_params=np.array([r[1] + [0.] * (5 - len(r[1])) for r in ROWS]),
        row_nparams=np.array([len(r[1]) for r in ROWS], dtype=np.int8),
        row_s=np.array([r[2] for r in ROWS]), row_theta=np.array([r[3] for r in ROWS]), row_class=np.array([r[4] for r in ROWS]),
        rec_row=R["row"].astype(np.int16), rec_slot=R["slot"].astype(np.int8), rec_exact=R["exact"], rec_err=R["err"], rec_nomu=R["nomu"],
        rec_qr_share=R["qr_share"].astype(f32), rec_det_bits=R["det_bits"].astype(np.uint64), rec_dev_det=R["dev_det"].astype(f32),
        rec_dev_libm=R["dev_libm"].astype(f32), rec_bound=R["bound"],
        in_row=IN["row"].astype(np.int16), in_stokes=IN["stokes"].astype(np.int8), in_qr=IN["qr"].astype(np.int8), in_u=IN["u"],
        in_exact=IN["exact"], in_err=IN["err"], in_det_bits=IN["det_bits"].astype(np.uint64), in_dev_det=IN["dev_det"].astype(f32),
        in_dev_libm=IN["dev_libm"].astype(f32), in_bound=IN["bound"],
        surf_params=np.array(surface_distribution()[1], dtype=np.float64), surf_s=sp[:, 0], surf_theta=sp[:, 1], surf_exact=s_exact, surf_err=s_err,
        surf_oracle_bits=np.ascontiguousarray(tab[:, 6:]).view(np.uint64), surf_dev=s_dev.astype(f32), surf_bound=s_bound,
        mp_kind=np.int8(MP_POINT[0]), mp_params=np.array(MP_POINT[1]), mp_s=MP_POINT[2], mp_theta=MP_POINT[3], mp_digits=MP_DIGITS,
        mp_points=MP_POINTS, mp_value=mp_value, mp_exact=mp_exact, mp_err=mp_err)
    print("wrote %s: %d coefficient records, %d inner-integral records, %d bytes" % (args.out, len(R["row"]), len(IN["u"]), os.path.getsize(args.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
