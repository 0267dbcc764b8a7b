#!/usr/bin/env python3
"""Writes tests/golden/exact_symphony.npz and profiles/exact_symphony_deviation.txt.  CPU only, minutes on 8 cores.

The fixture pins the Symphony path of the four analytic kinds to tests/exact_symphony.py: the plain harmonic sum of
one-dimensional integrals of exact J_n, J'_n.  Two layers:

  whole coefficients   rows (kind, parameters, s, theta) of class A ("exhausted": harmonics n >= 30 carry < 1e-14 of
                       every slot's sum, so the oracle's exact integer-order Bessel routine covers the whole sum) and
                       class B ("typical": the Leung expansions and the n-integral take part); one record per row and slot
  one tabulated        a non-separable surface through TabulatedDistribution2DGrid.from_function and the table oracle
  surface              against the exact sum of the same f(gamma, mu) at two class-A points
  single harmonics     G(n) of tests/exact_symphony.harmonics for the six (coefficient, Stokes) pairs, both lobes for V,
                       at two (s, theta) per kind: the integer orders below 30 and twenty orders from 30 up, half of them
                       non-integer

Every record stores the exact value, its error estimate, the deterministic oracle's value as bits, both oracle flavours'
deviation from exact, and the bound 2 max(|det / exact - 1|, |libm / exact - 1|) + 100 x the relative error estimate.
The bounds come from the CPU oracle alone.  A record for which either oracle flavour is not finite (or the exact value is
zero) is not written; it is printed here, and the tests leave nothing out at run time.

usage: python tools/make_exact_symphony_fixture.py [--jobs N]"""
import argparse
import math
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import exact_symphony as ex

PL, TJ, PPL, PK = 0, 1, 2, 3
SLOT_NAMES = ("j_I", "alpha_I", "j_Q", "alpha_Q", "j_V", "alpha_V")

# (kind, parameters, s, theta, class).  Class A needs a cold distribution AND few harmonics below 30 left out, i.e. small
# s |sin theta|.  The power-law kinds keep gamma_max <= 100 gamma_cutoff (beyond that the oracle's normalisation quadrature
# fails), gamma_min > 1 and, for a finite V, gamma_max beyond the lobe midpoint of the first harmonic of the n-integral.
ROWS = [
    (TJ, [0.3], 2., 0.6, "A"), (TJ, [0.25], 1.5, 2.4, "A"), (TJ, [0.2], 0.8, 1.3, "A"), (TJ, [0.35], 3., 0.4, "A"),
    (TJ, [0.3], 1.1, 2.0, "A"),
    (TJ, [1.], 3., 0.9, "B"), (TJ, [3.], 12., 1.2, "B"), (TJ, [2.], 8., 2.2, "B"), (TJ, [0.8], 40., 0.5, "B"),
    (TJ, [1.5], 1., 1.0, "B"),
    (PK, [4., 1.5, 1.7, 0.3], 2., 0.6, "A"), (PK, [3.5, 3., 0.6, 0.4], 1.5, 2.4, "A"), (PK, [4., 1.5, 2.4, 0.25], 0.8, 1.3, "A"),
    (PK, [5., 0.8, 1.7, 0.5], 1.1, 2.0, "A"), (PK, [3.5, 2., 3.1, 0.3], 3., 0.4, "A"),
    (PK, [4., 1.5, 1.7, 8.], 1., 1.0, "B"), (PK, [4., 1.5, 1.7, 8.], 10., 1.0, "B"), (PK, [3.5, 3., 0.6, 5.], 15., 0.5, "B"),
    (PK, [5., 1., 2.4, 10.], 4., 2.3, "B"), (PK, [4., 2., 1.3, 20.], 2., 1.9, "B"),
    (PL, [3., 1.02, 30., 0.3], 2.5, 1.4, "A"), (PL, [2.5, 1.02, 35., 0.35], 2.5, 1.75, "A"), (PL, [3.5, 1.02, 30., 0.3], 2.5, 1.0, "A"),
    (PL, [3., 1.02, 30., 0.4], 2.5, 2.2, "A"), (PL, [3., 1.05, 30., 0.3], 1.5, 0.6, "A"),
    (PL, [3., 1., 400., 8.], 4., 0.8, "B"), (PL, [2.5, 2., 1000., 10.], 8., 1.3, "B"), (PL, [3., 1.5, 40., 30.], 3., 2.2, "B"),
    (PL, [2.2, 1.2, 200., 5.], 20., 0.7, "B"), (PL, [3.5, 1., 100., 10.], 1.1, 1.1, "B"),
    (PPL, [3., 1.3, 1.02, 30., 0.3], 2.5, 1.4, "A"), (PPL, [2.5, 2.4, 1.02, 35., 0.35], 2.5, 1.75, "A"),
    (PPL, [3.5, 0.6, 1.02, 30., 0.3], 2.5, 1.0, "A"), (PPL, [3., 1.3, 1.02, 30., 0.4], 2.5, 2.2, "A"),
    (PPL, [3., 1.3, 1.05, 30., 0.3], 1.5, 0.6, "A"),
    (PPL, [3., 1.3, 1., 400., 8.], 4., 0.8, "B"), (PPL, [2.5, 2.4, 2., 1000., 10.], 8., 1.3, "B"),
    (PPL, [3., 0.6, 1.5, 40., 30.], 3., 2.2, "B"), (PPL, [2.2, 1.3, 1.2, 200., 5.], 20., 0.7, "B"),
    (PPL, [3.5, 2.4, 1., 100., 10.], 1.1, 1.1, "B"),
]

# the single-harmonic layer: (kind, parameters, s, theta), two per kind, one in each hemisphere and on each side of s = 10
HARMONIC_GROUPS = [
    (TJ, [1.], 3., 0.9), (TJ, [3.], 12., 2.0),
    (PK, [4., 1.5, 1.7, 8.], 3., 0.9), (PK, [3.5, 3., 0.6, 20.], 12., 2.0),
    (PL, [3., 1., 4000., 40.], 3., 0.9), (PL, [2.5, 1.02, 3000., 30.], 12., 2.0),
    (PPL, [3., 1.3, 1., 4000., 40.], 3., 0.9), (PPL, [2.5, 2.4, 1.02, 3000., 30.], 12., 2.0),
]
# one tabulated surface, f = exp(-gamma / T + a (gamma - 1) mu): (T, a, gamma_lo, gamma_hi, gamma nodes uniform in
# ln(gamma - 1), mu nodes) and two class-A points whose first lobe begins above gamma_lo; gamma_hi lies beyond the lobe
# midpoint of the first harmonic of the n-integral, or V is NaN as for the power-law kinds
SURFACE = (0.25, 0.5, 1.001, 24., 192, 65)
SURFACE_POINTS = [(2.5, 1.0), (2.5, 2.0)]

# (coefficient, Stokes, negative_lobe) of the seam; column of exact_symphony.harmonics
PAIRS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 1), (1, 1, 0, 1), (0, 2, 0, 2), (0, 2, 1, 3), (1, 2, 0, 2), (1, 2, 1, 3)]


def harmonic_orders(s, theta):
    """the integer orders from n_lo up to 29, then twenty orders from 30 to about 3000, every other one non-integer"""
    n_lo = math.floor(s * abs(math.sin(theta)) + 1.)
    low = np.arange(n_lo, 30, dtype=np.float64)
    high = np.round(30. * (100. ** (np.arange(20) / 19.)))
    high[1::2] += 0.37
    return np.concatenate([low, high])


def coefficient_row(row):
    kind, par, s, theta, _ = row
    return ex.coefficients(ex.make(kind, par), s, theta)


def harmonic_group(group):
    kind, par, s, theta = group
    n = harmonic_orders(s, theta)
    dist = ex.make(kind, par)
    val, err = ex.harmonics_with_error(dist, s, theta, n, capped=False)
    return n, val, err


def surface_table():
    """the surface as TabulatedDistribution2DGrid.from_function tabulates it: n = gamma sqrt(gamma^2 - 1) f"""
    from rimphony_amd import api
    T, a, lo, hi, nn, nmu = SURFACE
    dist = ex.tilted_juettner(T, a, lo, hi)
    return api.TabulatedDistribution2DGrid.from_function(
        lambda g, mu: g * np.sqrt(g * g - 1.) * dist.f(g, mu, np), api.grid_nodes_log_gm1(lo, hi, nn), nmu)


def surface_point(point):
    T, a, lo, hi, nn, nmu = SURFACE
    return ex.coefficients(ex.tilted_juettner(T, a, lo, hi), *point)


def oracle_coefficients(L, rows):
    import oracle_bind
    out = np.full((len(rows), 6), np.nan)
    for kind in range(4):
        idx = [i for i, r in enumerate(rows) if r[0] == kind]
        par = np.array([rows[i][1] for i in idx]).T
        out[idx] = oracle_bind.batch(L, kind, [rows[i][2] for i in idx], [rows[i][3] for i in idx], list(par), 0x3F, 8)[:, :6]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "exact_symphony.npz"))
    ap.add_argument("--table", default=os.path.join(ROOT, "profiles", "exact_symphony_deviation.txt"))
    args = ap.parse_args()
    import oracle_bind
    from rimphony_amd import _build
    _build.build_oracle()
    det, libm = oracle_bind.load("det"), oracle_bind.load("libm")

    with multiprocessing.Pool(args.jobs) as pool:
        coeff = pool.map_async(coefficient_row, ROWS, chunksize=1)
        harm = pool.map_async(harmonic_group, HARMONIC_GROUPS, chunksize=1)
        surf = pool.map_async(surface_point, SURFACE_POINTS, chunksize=1)
        coeff, harm, surf = coeff.get(), harm.get(), surf.get()

    lines = ["Deviation of the CPU oracle from the exact harmonic sum (tests/exact_symphony.py), tools/make_exact_symphony_fixture.py",
             "bound = 2 max(|det / exact - 1|, |libm / exact - 1|) + 100 x relative error estimate of the exact value", ""]
    with np.errstate(all="ignore"):
        # ---- whole coefficients
        o_det, o_libm = oracle_coefficients(det, ROWS), oracle_coefficients(libm, ROWS)
        rec = {k: [] for k in ("row", "slot", "exact", "err", "share", "det_bits", "dev_det", "dev_libm", "bound")}
        lines.append("whole coefficients: kind, class, parameters, s, theta, harmonics summed; per slot |det/exact-1| |libm/exact-1| bound share(n>=30)")
        for i, (row, (val, err, count, share)) in enumerate(zip(ROWS, coeff)):
            kind, par, s, theta, cls = row
            exhausted = bool((share < 1e-14).all())
            if exhausted != (cls == "A"):        # the class is what was measured; a row listed under the other one is said
                print("row %d %r listed as %s: shares of n >= 30 are %r" % (i, row, cls, share))
                cls = "A" if exhausted else "B"
                ROWS[i] = (kind, par, s, theta, cls)
            lines.append("%-16s %s %-28s s = %-5g theta = %-5g %5d harmonics" % (ex.KINDS[kind], cls, par, s, theta, count))
            for k in range(6):
                dd, dl = abs(o_det[i, k] / val[k] - 1.), abs(o_libm[i, k] / val[k] - 1.)
                bound = 2. * max(dd, dl) + 100. * err[k] / abs(val[k])
                if not (np.isfinite(o_det[i, k]) and np.isfinite(o_libm[i, k]) and np.isfinite(bound)):
                    msg = "    %-8s NOT WRITTEN: det %r libm %r exact %r" % (SLOT_NAMES[k], o_det[i, k], o_libm[i, k], val[k])
                    print(ex.KINDS[kind], cls, par, s, theta, msg)
                    lines.append(msg)
                    continue
                lines.append("    %-8s %.2e %.2e %.2e %.1e" % (SLOT_NAMES[k], dd, dl, bound, share[k]))
                for key, v in zip(rec, (i, k, val[k], err[k], share[k], o_det[i:i + 1, k].view(np.uint64)[0], dd, dl, bound)):
                    rec[key].append(v)

        # ---- single harmonics
        hrec = {k: [] for k in ("group", "pair", "n", "exact", "err", "det_bits", "dev_det", "dev_libm", "bound")}
        for gi, (group, (ns, val, err)) in enumerate(zip(HARMONIC_GROUPS, harm)):
            kind, par, s, theta = group
            dists = [oracle_bind.mkdist(L, kind, par)[0] for L in (det, libm)]
            for pi, (c, st, lobe, col) in enumerate(PAIRS):
                for j, n in enumerate(ns):
                    e, ee = val[j, c, col], err[j, c, col]
                    od, ol = (L.rimo_gamma_integral(d, c, st, lobe, s, theta, n) for L, d in zip((det, libm), dists))
                    dd, dl = abs(od / e - 1.), abs(ol / e - 1.)
                    bound = 2. * max(dd, dl) + 100. * ee / abs(e)
                    if not (np.isfinite(od) and np.isfinite(ol) and np.isfinite(bound) and abs(e) > 1e-290):
                        print("harmonic %s %r s %g theta %g pair %r n %g NOT WRITTEN: det %r libm %r exact %r" % (
                            ex.KINDS[kind], par, s, theta, (c, st, lobe), n, od, ol, e))
                        continue
                    for key, v in zip(hrec, (gi, pi, n, e, ee, np.array([od]).view(np.uint64)[0], dd, dl, bound)):
                        hrec[key].append(v)

    R = {k: np.array(v) for k, v in rec.items()}
    H = {k: np.array(v) for k, v in hrec.items()}
    lines += ["", "summary, whole coefficients: kind class slot: rows, max deviation (either flavour), max bound, 3rd smallest bound"]
    for kind in range(4):
        for cls in "AB":
            rows = [i for i, r in enumerate(ROWS) if r[0] == kind and r[4] == cls]
            for k in range(6):
                m = np.isin(R["row"], rows) & (R["slot"] == k)
                b = np.sort(R["bound"][m])
                dev = np.maximum(R["dev_det"][m], R["dev_libm"][m])
                lines.append("%-16s %s %-8s %2d rows  dev %.2e  bound %.2e  3rd smallest bound %s" % (
                    ex.KINDS[kind], cls, SLOT_NAMES[k], m.sum(), dev.max() if m.any() else math.nan,
                    b.max() if m.any() else math.nan, "%.2e" % b[2] if len(b) > 2 else "none"))
    lines += ["", "summary, single harmonics G(n): kind, orders: records, bound quantiles 50 % / 90 % / max, share of records with bound <= 1e-6"]
    hkind = np.array([g[0] for g in HARMONIC_GROUPS])[H["group"]]
    for kind in range(4):
        for name, m in (("n < 30 ", H["n"] < 30.), ("n >= 30", H["n"] >= 30.)):
            b = H["bound"][(hkind == kind) & m]
            lines.append("%-16s %s %4d records  %.2e / %.2e / %.2e   %.1f %% <= 1e-6" % (
                ex.KINDS[kind], name, len(b), np.quantile(b, 0.5), np.quantile(b, 0.9), b.max(), 100. * (b <= 1e-6).mean()))
    open(args.table, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[-60:]))

    # ---- the tabulated surface through the table oracle
    import tab2d_grid_bind
    table = surface_table()
    assert tab2d_grid_bind.set_tables(table.gamma, table.log_n) == 0
    sp = np.array(SURFACE_POINTS)
    tab, _ = tab2d_grid_bind.batch(sp[:, 0].copy(), sp[:, 1].copy(), np.zeros(len(sp)), 0x3F)
    s_exact, s_err = np.array([r[0] for r in surf]), np.array([r[1] for r in surf])
    assert all((r[3] < 1e-14).all() for r in surf), "the surface's points are not of class A"
    s_dev = np.abs(tab[:, :6] / s_exact - 1.)
    s_bound = 2. * s_dev + 100. * s_err / np.abs(s_exact)
    assert np.isfinite(s_bound).all()
    lines = ["", "tabulated surface f = exp(-gamma / T + a (gamma - 1) mu), (T, a, gamma_lo, gamma_hi, nodes, mu nodes) = %r:" % (SURFACE,),
             "table oracle's |value / exact - 1| per slot, then the bound"]
    for pt, d, b in zip(SURFACE_POINTS, s_dev, s_bound):
        lines += ["  s = %g theta = %g  " % pt + " ".join("%.2e" % v for v in d), "  " + " " * 22 + " ".join("%.2e" % v for v in b)]
    open(args.table, "a").write("\n".join(lines) + "\n")
    print("\n".join(lines))

    f32 = np.float32
    np.savez_compressed(
        args.out,
        row_kind=np.array([r[0] for r in ROWS], dtype=np.int8),
        row_params=np.array([r[1] + [0.] * (5 - len(r[1])) for r in ROWS]),
        row_nparams=np.array([len(r[1]) for r in ROWS], dtype=np.int8),
        row_s=np.array([r[2] for r in ROWS]), row_theta=np.array([r[3] for r in ROWS]),
        row_class=np.array([r[4] for r in ROWS]), row_harmonics=np.array([c[2] for c in coeff], dtype=np.int32),
        rec_row=R["row"].astype(np.int16), rec_slot=R["slot"].astype(np.int8), rec_exact=R["exact"], rec_err=R["err"],
        rec_share=R["share"].astype(f32), rec_det_bits=R["det_bits"].astype(np.uint64), rec_dev_det=R["dev_det"].astype(f32),
        rec_dev_libm=R["dev_libm"].astype(f32), rec_bound=R["bound"],
        grp_kind=np.array([g[0] for g in HARMONIC_GROUPS], dtype=np.int8),
        grp_params=np.array([g[1] + [0.] * (5 - len(g[1])) for g in HARMONIC_GROUPS]),
        grp_nparams=np.array([len(g[1]) for g in HARMONIC_GROUPS], dtype=np.int8),
        grp_s=np.array([g[2] for g in HARMONIC_GROUPS]), grp_theta=np.array([g[3] for g in HARMONIC_GROUPS]),
        pairs=np.array([p[:3] for p in PAIRS], dtype=np.int8),
        h_group=H["group"].astype(np.int8), h_pair=H["pair"].astype(np.int8), h_n=H["n"], h_exact=H["exact"],
        h_err=H["err"].astype(f32), h_det_bits=H["det_bits"].astype(np.uint64), h_dev_det=H["dev_det"].astype(f32),
        h_dev_libm=H["dev_libm"].astype(f32), h_bound=H["bound"],
        surf_params=np.array(SURFACE, dtype=np.float64), surf_s=sp[:, 0], surf_theta=sp[:, 1], surf_exact=s_exact, surf_err=s_err,
        surf_oracle_bits=np.ascontiguousarray(tab[:, :6]).view(np.uint64), surf_dev=s_dev.astype(f32), surf_bound=s_bound)
    print("wrote %s: %d coefficient records, %d harmonic records, %d bytes" % (args.out, len(R["row"]), len(H["n"]), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
