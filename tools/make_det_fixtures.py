#!/usr/bin/env python3
"""Writes tests/golden/det_<cfg>.npz for the four eight-slot bench tables and profiles/det_fixture_census.txt: values, FULL
status words and per-slot work of the deterministic CPU oracle (oracle/liboracle.so, rimo_batch_st through
tests/oracle_bind.py), so that the GPU tests can hold every output word of compute() to the oracle on 2048 rows per table
without running the oracle.  The status word is the oracle's own: rimo_compute_dimensionless_st sets the reason bits of
include/rimphony_hip.h:74-80 where the restated reference's errors arise (oracle/rimo_symphony.c, rimo_heyvaerts.c).

  flavour                          rimo_build_flavour() of the library that computed the file
  start, n, mask                   the MAIN block: rows start .. start + n - 1 of workload.make_batch(cfg), the block of
                                   tests/golden/literal_<cfg>.npz (a launch the suite already makes)
  values [n][8], status [n][8] (uint8), work [n][8] (uint32 where it fits)
  extra_s, extra_theta [m], extra_params [m][nparams], extra_tag [m]
                                   the EXTRA block: rows given explicitly, off the bench tables (tags below)
  extra_values, extra_status, extra_work [m][8]

Tags of the extra rows:
  cut       power law / pitchy power law rows 0 .. of the table with gamma_max = 10 (even rows) or 100 (odd rows) and, for the
            power law, gamma_min = 1: the distribution ends inside the range the quadratures sample
  corner    48 rows per kind with theta log-uniform in [1e-3, 0.05] (tests/test_gpu_parity.py test_small_angle_corner)
  endless   thermal rows 51108 .. 51115: row 51111 is a provably endless marching loop (CHUNK_CAP)
  finite_nonzero, inner_only
            what the search found: rows of the table after the main block with a slot that is FINITE with a nonzero status
            word, or NaN with INNER_FAIL and neither OUTER_FAIL nor CHUNK_CAP; up to 16 rows per class and kind

The search looks at up to --search-rows further rows per kind within --search-minutes of wall time in total, the kinds in
turn block by block, Faraday slots first (they are cheap), and the census file records how far it looked.

The files are written with fixed zip timestamps: the same oracle writes the same bytes.  CPU only.
Usage: python tools/make_det_fixtures.py [--threads 8] [--search-minutes 20] [--search-rows 20000] [--n 2048]"""
import argparse
import io
import os
import sys
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_bind  # noqa: E402
from rimphony_amd import workload  # noqa: E402

CONFIGS = ("cfg2_powerlaw_8", "cfg3_thermal_8", "cfg4_pitchypl_8", "cfg5_pitchykappa_8")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CENSUS = os.path.join(ROOT, "profiles", "det_fixture_census.txt")
MAX_BYTES = 420 * 1000
CORNER_ROWS, CORNER_START, CUT_ROWS = 48, 900000, {"cfg2_powerlaw_8": 128, "cfg4_pitchypl_8": 192}
ENDLESS = (51108, 8)
SEARCH_BLOCK, PER_CLASS = 512, 16
ST_INNER, ST_OUTER, ST_CAP, ST_NONFINITE = 1, 2, 4, 16


def extra_rows(cfg):
    """(s, theta, params [m][np], tags) of the extra block's fixed rows of a config"""
    blocks = []
    if cfg in CUT_ROWS:
        m = CUT_ROWS[cfg]
        _, _, s, th, params = workload.make_batch(cfg, m)
        gmax = np.where(np.arange(m) % 2 == 0, 10., 100.)
        if cfg == "cfg2_powerlaw_8":
            params = [params[0], np.ones(m), gmax, params[3]]
        else:
            params = [params[0], params[1], params[2], gmax, params[4]]
        blocks.append((s, th, params, "cut"))
    _, _, s, _, params = workload.make_batch(cfg, CORNER_ROWS, start=CORNER_START)
    u = workload.uniform01(99, np.arange(CORNER_ROWS), 1)
    blocks.append((s, np.exp(np.log(1e-3) + u * (np.log(0.05) - np.log(1e-3))), params, "corner"))
    if cfg == "cfg3_thermal_8":
        _, _, s, th, params = workload.make_batch(cfg, ENDLESS[1], start=ENDLESS[0])
        blocks.append((s, th, params, "endless"))
    return (np.concatenate([b[0] for b in blocks]), np.concatenate([b[1] for b in blocks]),
            np.concatenate([np.stack(b[2], axis=1) for b in blocks]), sum(([b[3]] * len(b[0]) for b in blocks), []))


def classes_of(values, status):
    """[rows] bool x 2: a slot finite with a nonzero word; a slot NaN with INNER_FAIL and no other reason bit"""
    fin = np.isfinite(values) & (status != 0)
    inner = np.isnan(values) & ((status & (ST_INNER | ST_OUTER | ST_CAP | 8)) == ST_INNER)
    return fin.any(axis=1), inner.any(axis=1)


def search(L, threads, max_rows, minutes, first_row, log):
    """{cfg: {"finite_nonzero": [rows], "inner_only": [rows]}} and how far each (config, slot group) was searched"""
    found = {cfg: {"finite_nonzero": [], "inner_only": []} for cfg in CONFIGS}
    looked = {(cfg, g): 0 for cfg in CONFIGS for g in ("faraday", "symphony")}
    deadline = time.time() + 60. * minutes
    for group, mask, share in (("faraday", 0xC0, 0.4), ("symphony", 0x3F, 1.0)):
        stop = time.time() + share * max(deadline - time.time(), 0.)
        for off in range(0, max_rows, SEARCH_BLOCK):
            for cfg in CONFIGS:
                if time.time() >= stop:
                    break
                nb = min(SEARCH_BLOCK, max_rows - off)
                start = first_row[cfg] + off
                kind, _, s, th, params = workload.make_batch(cfg, nb, start=start)
                t0 = time.time()
                v, st, _ = oracle_bind.batch_st(L, kind, s, th, params, mask, threads)
                sel = [k for k in range(8) if mask & (1 << k)]
                fin, inner = classes_of(v[:, sel], st[:, sel])
                for name, hit in (("finite_nonzero", fin), ("inner_only", inner)):
                    have = found[cfg][name]
                    have += [start + int(i) for i in np.flatnonzero(hit) if start + int(i) not in have][:PER_CLASS - len(have)]
                looked[cfg, group] = off + nb
                log("search %-8s %-20s rows %d .. %d: %d finite with a nonzero word, %d NaN with INNER_FAIL alone  (%.1f s)" % (
                    group, cfg, start, start + nb - 1, fin.sum(), inner.sum(), time.time() - t0))
            if time.time() >= stop:
                break
    return found, looked


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


def narrow(work):
    return work.astype(np.uint32) if work.size == 0 or int(work.max()) < 2 ** 32 else work


def histogram(status, slots):
    words, counts = np.unique(status[:, slots], return_counts=True)
    return "  ".join("%d: %d" % (w, c) for w, c in zip(words, counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--search-minutes", type=float, default=20.)
    ap.add_argument("--search-rows", type=int, default=20000)
    ap.add_argument("--n", type=int, default=2048)
    a = ap.parse_args()
    L = oracle_bind.load("det")
    flavour = L.rimo_build_flavour().decode()
    lines = []

    def log(text):
        print(text, flush=True)
        lines.append(text)

    log("tools/make_det_fixtures.py: %s, %d threads, search limited to %d rows per kind and %g minutes" % (
        flavour, a.threads, a.search_rows, a.search_minutes))
    first_row = {}
    main_block = {}
    for cfg in CONFIGS:
        with np.load(os.path.join(GOLDEN, "literal_%s.npz" % cfg)) as z:
            start, n, mask = int(z["start"]), min(int(z["n"]), a.n), int(z["mask"])
            first_row[cfg] = start + int(z["n"])
        main_block[cfg] = (start, n, mask)
    def save(cfg, f):
        path = os.path.join(GOLDEN, "det_%s.npz" % cfg)
        write_npz(path, dict(f, work=narrow(f["work"]), extra_work=narrow(f["extra_work"]), extra_tag=np.array(f["extra_tag"])))
        return os.path.getsize(path)

    # 1. the main blocks and the extra rows that are known beforehand; the files are complete but for what the search adds
    files, seconds = {}, {}
    for cfg in CONFIGS:
        start, n, mask = main_block[cfg]
        es, eth, epar, tags = extra_rows(cfg)
        kind = workload.CONFIGS[cfg][0]
        t0 = time.time()
        ev, est, ew = oracle_bind.batch_st(L, kind, es, eth, [np.ascontiguousarray(epar[:, j]) for j in range(epar.shape[1])],
                                           0xFF, a.threads)
        t_extra = time.time() - t0
        while True:
            _, _, s, th, params = workload.make_batch(cfg, n, start=start)
            t0 = time.time()
            values, status, work = oracle_bind.batch_st(L, kind, s, th, params, mask, a.threads)
            t_main = time.time() - t0
            f = {"flavour": np.array(flavour), "start": np.int64(start), "n": np.int64(n), "mask": np.int64(mask),
                 "values": values, "status": status, "work": work, "extra_s": es, "extra_theta": eth, "extra_params": epar,
                 "extra_tag": tags, "extra_values": ev, "extra_status": est, "extra_work": ew}
            size = save(cfg, f)
            if size <= MAX_BYTES or n // 2 < 1024:
                break
            log("det_%s.npz: %d bytes with n = %d, halving" % (cfg, size, n))
            n //= 2
        files[cfg], seconds[cfg] = f, (t_main, t_extra)
        log("det_%s.npz: main block rows %d .. %d in %.0f s, %d extra rows in %.0f s" % (cfg, start, start + n - 1, t_main, len(es), t_extra))

    # 2. the search for the two classes the census of the bench rows did not show
    t0 = time.time()
    found, looked = search(L, a.threads, a.search_rows, a.search_minutes, first_row, log)
    log("search: %.0f s" % (time.time() - t0))
    for cfg in CONFIGS:
        for group in ("faraday", "symphony"):
            log("searched %-20s %-8s rows %d .. %d" % (cfg, group, first_row[cfg], first_row[cfg] + looked[cfg, group] - 1)
                if looked[cfg, group] else "searched %-20s %-8s no row" % (cfg, group))
        for name in ("finite_nonzero", "inner_only"):
            log("found    %-20s %-14s %s" % (cfg, name, found[cfg][name] or "none"))

    # 3. what it found joins the extra block, all eight slots
    for cfg in CONFIGS:
        f, kind = files[cfg], workload.CONFIGS[cfg][0]
        t0 = time.time()
        for name in ("finite_nonzero", "inner_only"):
            rows = found[cfg][name]
            if rows:
                _, _, s2, th2, p2 = workload.make_rows(cfg, rows)
                v2, st2, w2 = oracle_bind.batch_st(L, kind, s2, th2, p2, 0xFF, a.threads)
                for key, more in (("extra_s", s2), ("extra_theta", th2), ("extra_params", np.stack(p2, axis=1)),
                                  ("extra_values", v2), ("extra_status", st2), ("extra_work", w2)):
                    f[key] = np.concatenate([f[key], more])
                f["extra_tag"] = f["extra_tag"] + [name] * len(rows)
        t_found = time.time() - t0
        size = save(cfg, f)
        assert size <= MAX_BYTES, (cfg, size)
        values, status, work, ev, est, ew = (f[k] for k in ("values", "status", "work", "extra_values", "extra_status", "extra_work"))
        assert (((status & ST_NONFINITE) != 0) == np.isnan(values)).all() and (((est & ST_NONFINITE) != 0) == np.isnan(ev)).all()
        log("")
        log("det_%s.npz: %d bytes; main block %d rows in %.0f s, extra block %d rows in %.0f s + %.0f s" % (
            cfg, size, int(f["n"]), seconds[cfg][0], len(ev), seconds[cfg][1], t_found))
        log("  status word: count")
        log("  main  Symphony slots 0-5   %s" % histogram(status, slice(0, 6)))
        log("  main  Faraday slots 6-7    %s" % histogram(status, slice(6, 8)))
        tags = np.array(f["extra_tag"])
        for tag in sorted(set(tags)):
            log("  extra %-14s Symphony   %s" % (tag, histogram(est[tags == tag], slice(0, 6))))
            log("  extra %-14s Faraday    %s" % (tag, histogram(est[tags == tag], slice(6, 8))))
        log("  samples: main %d Symphony + %d Faraday, extra %d + %d" % (
            work[:, :6].sum(), work[:, 6:].sum(), ew[:, :6].sum(), ew[:, 6:].sum()))
    with open(CENSUS, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
