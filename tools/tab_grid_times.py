#!/usr/bin/env python3
"""What the interval search of a table set on given gamma nodes costs: the measurement of profiles/tabulated_grid_times.txt.

The same content in two forms -- the three 64-node tables of tab_bind.edge_tables over [1.01, 1e4] through the sin^k entry
(nodes uniform in ln gamma, internal kind 7) and through rimphony_ctx_set_tables_grid on the very same nodes (kind 8) -- for
(no g, k = 0), (no g, k = 1.5) and (8-node pitch rows, k = 0.3); then the table the form exists for, the T = 0.1 Juettner
shape on 512 nodes uniform in ln(gamma - 1) over [1 + 1e-6, 31].  Each leg is a fresh process under its own `timeout` with
one context and three consecutive batches of the power-law bench generator's (s, theta), the tables in turn, all eight
slots; the whole sequence twice, the order of the legs alternating.  Times are rimphony_last_symphony_ms and
rimphony_last_faraday_ms, samples rimphony_last_work's.
usage: tab_grid_times.py [rows]        (a leg that fails ends the run: nothing further is started)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"no g, k = 0": (None, 0.0), "no g, k = 1.5": (None, 1.5), "8-node rows, k = 0.3": (8, 0.3)}
LEGS = [(case, form) for case in CASES for form in ("sin^k", "grid")] + [("cold Juettner", "grid")]


def child(case, form, rows):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import hashlib
    import numpy as np
    import tab_bind
    import tab_grid_bind as tg
    import tab_pitchy_bind as tpy
    from rimphony_amd import api, workload
    ctx = api.Context(0)
    if case == "cold Juettner":
        g = tg.cold_grid(512)
        ctx.set_tables_grid(g, tab_bind.log_n_juettner(g, tg.COLD_T))
        index = np.zeros(rows)
    else:
        n_mu, k = CASES[case]
        g = tg.grid("uniform")
        t = tg.edge_tables_at(g)
        log_g = None if n_mu is None else tpy.set_b_rows(n_mu)
        if form == "grid":
            ctx.set_tables_grid(g, t, log_g, np.full(3, k))
        else:
            ctx.set_tables(tg.EDGE_LO, tg.EDGE_HI, t, log_g, sin_k=np.full(3, k))
        index = np.tile(np.arange(3, dtype=np.float64), (rows + 2) // 3)[:rows]
    _, _, s, th, _ = workload.make_batch("cfg2_powerlaw_8", rows, start=0)
    sym, far, res = [], [], None
    for _ in range(3):
        out = ctx.compute_batch(api.TABULATED, s, th, [index], 0xFF)
        sym.append(ctx.last_symphony_ms())
        far.append(ctx.last_faraday_ms())
        w = ctx.last_work()
        res = {"samples": w["samples"], "passes": w["passes"], "nan": int(np.isnan(out).sum())}
    res.update(sym=sym, far=far, md5=hashlib.md5(out.tobytes()).hexdigest(), shared=bool(ctx.shared_mode()))
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    rows = sys.argv[1] if len(sys.argv) > 1 else "4096"
    got = {}
    for seq in (0, 1):
        for case, form in (LEGS if seq == 0 else LEGS[::-1]):
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", case, form, rows],
                               capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode or not line:
                print("leg %s / %s %d ended with status %d: the run stops here\n%s" % (case, form, seq + 1, r.returncode, r.stderr[-2000:]), flush=True)
                sys.exit(1)
            res = json.loads(line[0][7:])
            got.setdefault((case, form), []).append(res)
            print("%-21s %-6s %d  Symphony ms %s  Faraday ms %s | samples %d  passes %d  NaN slots %d  md5 %s%s" % (
                case, form, seq + 1, " ".join("%8.2f" % m for m in res["sym"]), " ".join("%8.2f" % m for m in res["far"]), res["samples"],
                res["passes"], res["nan"], res["md5"][:8], "  SHARED MODE" if res["shared"] else ""), flush=True)
    mean = lambda v, key: sum(sum(r[key]) / len(r[key]) for r in v) / len(v)
    for (case, form), v in got.items():
        print("%-21s %-6s Symphony %8.2f ms  Faraday %8.2f ms  samples %d  %.2f ps per sample (both kernels)" % (
            case, form, mean(v, "sym"), mean(v, "far"), v[0]["samples"], 1e9 * (mean(v, "sym") + mean(v, "far")) / v[0]["samples"]))
    for case in CASES:
        a, b = got[case, "sin^k"], got[case, "grid"]
        print("%-21s grid / sin^k: Symphony %.3f  Faraday %.3f  samples %.4f" % (
            case, mean(b, "sym") / mean(a, "sym"), mean(b, "far") / mean(a, "far"), b[0]["samples"] / a[0]["samples"]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main()
