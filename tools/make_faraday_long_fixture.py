#!/usr/bin/env python3
"""Writes tests/golden/faraday_long_det.npz: rows of the bench tables whose Faraday outer quadratures grow LONG, computed by
the deterministic CPU oracle (oracle/liboracle.so through tests/oracle_bind.py), so that the GPU tests can hold the kernels
to the oracle's bits in every size class of the outer subinterval list:

      48  the rounds begin (RIM_ROUND_MIN_SIZE, heyvaerts_wave.h; pitchy-kappa only)
      64  the list leaves LDS (CAP_OUTER, rimphony_internal.h)
    2050  limit / 2 + 2 for the Faraday limit of 4096: GSL's qpsrt stops keeping its list fully sorted
    4096  the quadrature gives up (GSL_EMAXITER -> NaN)

  config, row [n]                  the table (a name of workload.CONFIGS) and the row index
  s, theta [n], params [n][5]      the row as workload.make_rows generates it (params padded with NaN), nparams [n]
  values [n][8]                    rimo_compute_dimensionless per slot (api.SLOTS order; NaN where a quadrature fails)
  integrand_evals [n][8]           the integrand samples of each slot
  status [n][8]                    the status word of each slot (uint8; the bits of include/rimphony_hip.h:74-80) as
                                   rimo_compute_dimensionless_st sets it from the oracle's own control flow
  max_outer_size, outer_qag_calls, inner_qag_calls [n][2]
                                   of the Faraday pair (slots 6, 7 = rho_Q, rho_V)
  cls [n]                          'mid' (seconds of CPU) or 'limit' (an outer list beyond limit / 2 + 2: a minute or two)
  notes                            what the scan of the pitchy power-law table found

The classes are asserted here, on what the oracle computed, not taken on trust.  The file is written with fixed zip
timestamps: the same oracle writes the same bytes.

CPU only; a few minutes on 16 threads.  Usage: python tools/make_faraday_long_fixture.py [--threads 16]"""
import argparse
import io
import os
import sys
import time
import zipfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_bind  # noqa: E402
from rimphony_amd import workload  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "faraday_long_det.npz")
# (coefficient, stokes) of the eight slots: rimphony_amd/api.py SLOTS (not imported: that module needs torch)
SLOTS = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 1), (2, 2)]
LIMIT, HALF, CAP_OUTER, ROUND_MIN = 4096, 4096 // 2 + 2, 64, 48
SCAN_CFG, SCAN_ROWS, SCAN_BLOCK = "cfg4_pitchypl_8", 4096, 256

ROWS = [
    # (config, row, class)                      what it exercises
    ("cfg5_pitchykappa_8", 305, "mid"),         # the list reaches exactly 48: the first size with rounds
    ("cfg5_pitchykappa_8", 78, "mid"),          # just past LDS
    ("cfg5_pitchykappa_8", 70, "mid"),          # spill
    ("cfg5_pitchykappa_8", 152, "mid"),         # spill, and a FINITE value: it depends on every pick of the run
    ("cfg5_pitchykappa_8", 12, "mid"),          # control: short lists
    ("cfg2_powerlaw_8", 1131095, "mid"),        # 45
    ("cfg2_powerlaw_8", 1131217, "mid"),        # 51
    ("cfg2_powerlaw_8", 1260884, "mid"),        # a long marching loop at theta ~ 0.05
    ("cfg3_thermal_8", 14905, "mid"),           # spill on the thermal kernel
    ("cfg3_thermal_8", 6078, "mid"),            # a long marching loop
    ("cfg4_pitchypl_8", 169, "mid"),            # 42, finite
    ("cfg4_pitchypl_8", 29920, "mid"),          # a long marching loop
    ("cfg5_pitchykappa_8", 11648, "limit"),     # runs to 4096
    ("cfg5_pitchykappa_8", 7887, "limit"),      # converges past limit / 2 + 2
    ("cfg2_powerlaw_8", 1132205, "limit"),      # runs to 4096
    ("cfg2_powerlaw_8", 1176506, "limit"),      # converges past limit / 2 + 2
]


def one_row(config, row):
    kind, _, s, theta, params = workload.make_rows(config, [row])
    return kind, float(s[0]), float(theta[0]), [float(p[0]) for p in params]


def compute(L, config, row, slot):
    """(value, Counters as a dict, status word) of one slot of one row"""
    kind, s, theta, params = one_row(config, row)
    d, st = oracle_bind.mkdist(L, kind, params)
    assert st == 0, (config, row)
    co, stk = SLOTS[slot]
    v, status, c = oracle_bind.compute_st(L, d, co, stk, s, theta)
    return v, c, status


def compute_rows(L, rows, slots, threads):
    """{(config, row, slot): (value, counters)}; the Faraday slots of the 'limit' rows are started first"""
    tasks = [(cfg, row, slot) for cfg, row, cls in rows for slot in slots]
    heavy = {(cfg, row) for cfg, row, cls in rows if cls == "limit"}
    tasks.sort(key=lambda t: not (t[2] >= 6 and (t[0], t[1]) in heavy))
    with ThreadPoolExecutor(threads) as pool:
        res = list(pool.map(lambda t: compute(L, *t), tasks))
    return dict(zip(tasks, res))


def scan(L, threads):
    """The first row of SCAN_CFG's first SCAN_ROWS whose Faraday pair has an outer list longer than CAP_OUTER (None: none),
    and the longest list seen."""
    longest = 0
    for start in range(0, SCAN_ROWS, SCAN_BLOCK):
        rows = [(SCAN_CFG, r, "mid") for r in range(start, start + SCAN_BLOCK)]
        res = compute_rows(L, rows, (6, 7), threads)
        size = {r: max(res[SCAN_CFG, r, 6][1]["max_outer_size"], res[SCAN_CFG, r, 7][1]["max_outer_size"]) for _, r, _ in rows}
        longest = max(longest, max(size.values()))
        hit = [r for r in sorted(size) if size[r] > CAP_OUTER]
        print("scan %s rows %d..%d: longest %d" % (SCAN_CFG, start, start + SCAN_BLOCK - 1, max(size.values())), flush=True)
        if hit:
            return hit[0], size[hit[0]], longest
    return None, 0, longest


def assemble(rows, res):
    n = len(rows)
    f = {"config": np.array([r[0] for r in rows]), "row": np.array([r[1] for r in rows], dtype=np.int64),
         "cls": np.array([r[2] for r in rows]), "s": np.zeros(n), "theta": np.zeros(n), "params": np.full((n, 5), np.nan),
         "nparams": np.zeros(n, dtype=np.int64), "values": np.zeros((n, 8)), "status": np.zeros((n, 8), dtype=np.uint8),
         "integrand_evals": np.zeros((n, 8), dtype=np.uint64),
         "max_outer_size": np.zeros((n, 2), dtype=np.uint64), "outer_qag_calls": np.zeros((n, 2), dtype=np.uint64),
         "inner_qag_calls": np.zeros((n, 2), dtype=np.uint64)}
    for i, (cfg, row, _) in enumerate(rows):
        _, f["s"][i], f["theta"][i], params = one_row(cfg, row)
        f["nparams"][i] = len(params)
        f["params"][i, :len(params)] = params
        for slot in range(8):
            v, c, status = res[cfg, row, slot]
            f["values"][i, slot] = v
            f["status"][i, slot] = status
            f["integrand_evals"][i, slot] = c["integrand_evals"]
            if slot >= 6:
                for name in ("max_outer_size", "outer_qag_calls", "inner_qag_calls"):
                    f[name][i, slot - 6] = c[name]
    return f


def check_classes(f):
    """The size classes the fixture exists for, on the computed data (tests/test_faraday_long_host.py asserts the same on
    the stored file)."""
    size, rho = f["max_outer_size"].astype(np.int64), f["values"][:, 6:]
    fin = np.isfinite(rho)
    i305 = int(np.flatnonzero((f["config"] == "cfg5_pitchykappa_8") & (f["row"] == 305))[0])
    assert size[i305].max() == ROUND_MIN, size[i305]
    assert (fin & (size > CAP_OUTER) & (size < HALF)).sum() >= 1
    assert (fin & (size > HALF) & (size < LIMIT)).sum() >= 2
    assert (~fin & (size == LIMIT)).sum() >= 2
    assert size.max() <= LIMIT
    # the class tag says where a row may run: a 'mid' row has no list past limit / 2 + 2
    mid = f["cls"] == "mid"
    assert (size[mid] < HALF).all() and (size[~mid].max(axis=1) > HALF).all()
    # the status words: NONFINITE <=> NaN in every slot, and a list that ran to the limit is an OUTER_FAIL
    assert (((f["status"] & 16) != 0) == np.isnan(f["values"])).all()
    assert ((f["status"][:, 6:] & 2) != 0)[size == LIMIT].all()


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the time of day)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    L = oracle_bind.load("det")
    t0 = time.time()
    rows = list(ROWS)
    hit, hit_size, longest = scan(L, a.threads)
    if hit is None:
        notes = "%s rows 0..%d: no Faraday outer list longer than %d (the longest is %d)" % (SCAN_CFG, SCAN_ROWS - 1, CAP_OUTER, longest)
    else:
        notes = "%s row %d is the first of rows 0..%d with a Faraday outer list longer than %d (%d)" % (
            SCAN_CFG, hit, SCAN_ROWS - 1, CAP_OUTER, hit_size)
        if (SCAN_CFG, hit) not in {(c, r) for c, r, _ in rows}:
            rows.insert(12, (SCAN_CFG, hit, "mid" if hit_size < HALF else "limit"))
    print(notes, " (%.0f s)" % (time.time() - t0), flush=True)
    res = compute_rows(L, rows, range(8), a.threads)
    f = assemble(rows, res)
    f["notes"] = np.array(notes)
    for i, (cfg, row, cls) in enumerate(rows):
        print("%-20s %8d %-5s size %4d / %4d  rho_Q %r rho_V %r  inner QAGs %d / %d" % (
            cfg, row, cls, f["max_outer_size"][i, 0], f["max_outer_size"][i, 1], f["values"][i, 6], f["values"][i, 7],
            f["inner_qag_calls"][i, 0], f["inner_qag_calls"][i, 1]))
    check_classes(f)
    write_npz(OUT, f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes in %.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
