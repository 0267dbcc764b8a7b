#!/usr/bin/env python3
"""What mu nodes of the caller's choosing cost a 2-D table set per sample: the measurement of
profiles/tabulated_2d_nodes_times.txt.

The same surface on the same nodes -- gamma uniform in ln gamma over [1.01, 1e4], mu uniform over [-1, +1] -- through
rimphony_ctx_set_tables_2d_grid (internal kind 9; with k = 0 given explicitly kind 11) and through
rimphony_ctx_set_tables_2d_nodes (kinds 12 and 13): the same function, so the same samples but for the rounding of t_mu, and
the mu lookup in full (two guide words, the bisection, the cell's own width).  log_n[i][j] = y_i + G_j, y the rolled power law
gamma^-2.5 exp(-30 / gamma - gamma / 500) and G = 0.8 mu - 1.5 mu^2 (the content of profiles/tabulated_2d_pitchy_times.txt), on
512 x 65 nodes (1 MiB of node data).  One more leg, once: the same function on 65 mu nodes graded as fixture set P's are -- 33
uniform below the last of the 128 guide cells and 32 inside it, the last cell 5e-5 wide --, where a sample in that guide cell
bisects over 32 nodes.  Each leg is a fresh process under its own `timeout` with one context and three consecutive batches of
the power-law bench generator's (s, theta), all eight slots; the whole sequence twice, the order of the legs alternating.
Times are rimphony_last_symphony_ms and rimphony_last_faraday_ms, samples rimphony_last_work's.
usage: tab_2d_nodes_times.py [rows]        (a leg that fails ends the run: nothing further is started)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, N_MU = 512, 65
LEGS = ["2-D grid", "2-D nodes", "2-D grid sin^0", "2-D nodes sin^0"]
GRADED = "2-D nodes graded"


def graded_mu():
    last = 1.0 - 2.0 / 128
    import numpy as np
    tail = np.linspace(last, 1.0 - 5e-5, 31)
    return np.concatenate([np.linspace(-1.0, last, 33, endpoint=False), tail, [1.0]])


def child(form, rows):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hashlib
    import time
    import numpy as np
    import tab_bind
    from rimphony_amd import api, workload
    lo, hi = 1.01, 1e4
    g = tab_bind.nodes(lo, hi, N_NODES)
    g[0], g[-1] = lo, hi
    mu = graded_mu() if form == GRADED else np.linspace(-1.0, 1.0, N_MU)
    assert len(mu) == N_MU
    table = tab_bind.log_n_rolled_powerlaw(g, 2.5, 30.0, 500.0)[:, None] + (0.8 * mu - 1.5 * mu * mu)[None, :]
    k = 0.0 if form.endswith("sin^0") else None
    ctx = api.Context(0)
    install = []
    for _ in range(3):
        t0 = time.perf_counter()
        if form.startswith("2-D grid"):
            ctx.set_tables_2d_grid(g, table, k)
        else:
            ctx.set_tables_2d_nodes(g, mu, table, k)
        install.append(1e3 * (time.perf_counter() - t0))
    _, _, s, th, _ = workload.make_batch("cfg2_powerlaw_8", rows, start=0)
    index = np.zeros(rows)
    sym, far, res = [], [], None
    for _ in range(3):
        out = ctx.compute_batch(api.TABULATED, s, th, [index], 0xFF)
        sym.append(ctx.last_symphony_ms())
        far.append(ctx.last_faraday_ms())
        w = ctx.last_work()
        res = {"samples": w["samples"], "passes": w["passes"], "nan": int(np.isnan(out).sum())}
    res.update(sym=sym, far=far, install=install, md5=hashlib.md5(out.tobytes()).hexdigest(), shared=bool(ctx.shared_mode()))
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def leg(form, rows):
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", form, rows],
                       capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode or not line:
        print("leg %s ended with status %d: the run stops here\n%s" % (form, r.returncode, r.stderr[-2000:]), flush=True)
        sys.exit(1)
    return json.loads(line[0][7:])


def main():
    rows = sys.argv[1] if len(sys.argv) > 1 else "4096"
    got = {}
    for seq in (0, 1):
        for form in (LEGS + [GRADED] if seq == 0 else LEGS[::-1]):
            res = leg(form, rows)
            got.setdefault(form, []).append(res)
            print("%-16s %d  Symphony ms %s  Faraday ms %s | samples %d  passes %d  NaN slots %d  install ms %s  md5 %s%s" % (
                form, seq + 1, " ".join("%8.2f" % m for m in res["sym"]), " ".join("%8.2f" % m for m in res["far"]), res["samples"],
                res["passes"], res["nan"], " ".join("%.1f" % m for m in res["install"]), res["md5"][:8],
                "  SHARED MODE" if res["shared"] else ""), flush=True)
    mean = lambda v, key: sum(sum(r[key]) / len(r[key]) for r in v) / len(v)
    for form, v in got.items():
        print("%-16s Symphony %8.2f ms  Faraday %8.2f ms  samples %d  %.2f ps per sample (both kernels)" % (
            form, mean(v, "sym"), mean(v, "far"), v[0]["samples"], 1e9 * (mean(v, "sym") + mean(v, "far")) / v[0]["samples"]))
    for plain, new in (("2-D grid", "2-D nodes"), ("2-D grid sin^0", "2-D nodes sin^0"), ("2-D nodes", GRADED)):
        a, b = got[plain], got[new]
        ratio = lambda key: (mean(b, key) / b[0]["samples"]) / (mean(a, key) / a[0]["samples"])
        print("%s / %s, per sample: Symphony %.3f  Faraday %.3f  (samples %.4f)" % (
            new, plain, ratio("sym"), ratio("far"), b[0]["samples"] / a[0]["samples"]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
