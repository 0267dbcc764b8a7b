#!/usr/bin/env python3
"""What the blend of two tables costs per sample: the measurement of profiles/tabulated_family_times.txt.

A two-table family gamma^-p exp(-gamma / 1e10), p = 2 and 3.5, on 2048 nodes over [1, 1e12], every row at x = 0.5 (internal kinds
14 and, with sin_k = (0, 3), 15), against the plain form (kinds 5 and 7, the parent commit's kernels: profiles/
tabulated_family_unchanged.txt) on ONE table built directly at p = 2.75 (sin_k = 1.5): the same function to rounding, so the same
samples to a few in 1e6, and the blend's extra loads and arithmetic in full.  Each leg is a fresh process under its own `timeout`
with one context, RIMPHONY_TAB_GROUP set to 1 (group kernel) or 0 (one wave per coefficient), and three consecutive batches
of the power-law bench generator's (s, theta), all eight slots; the whole sequence twice, the order of the legs alternating.
Times are rimphony_last_symphony_ms and rimphony_last_faraday_ms, samples rimphony_last_work's (Symphony and Faraday apart).
usage: tab_family_times.py [rows]        (a leg that fails ends the run: nothing further is started)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = [(form, grp) for form in ("plain", "family", "plain sin^k", "family sin^k") for grp in ("group", "solo")]


def child(form, grp, rows):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["RIMPHONY_TAB_GROUP"] = "1" if grp == "group" else "0"
    import hashlib
    import numpy as np
    import tab_bind
    from rimphony_amd import api, workload
    lo, hi, cut = 1.0, 1e12, 1e10
    g = tab_bind.nodes(lo, hi, 2048)
    ctx = api.Context(0)
    if form.startswith("family"):
        ctx.set_tables_family(lo, hi, np.stack([tab_bind.log_n_powerlaw(g, p, cut) for p in (2.0, 3.5)]),
                              [0.0, 3.0] if form.endswith("sin^k") else None)
        index = np.full(rows, 0.5)
    else:
        ctx.set_tables(lo, hi, tab_bind.log_n_powerlaw(g, 2.75, cut), sin_k=1.5 if form.endswith("sin^k") else None)
        index = np.zeros(rows)
    _, _, s, th, _ = workload.make_batch("cfg2_powerlaw_8", rows, start=0)
    sym, far, res = [], [], None
    for _ in range(3):
        out = ctx.compute_batch(api.TABULATED, s, th, [index], 0xFF)
        sym.append(ctx.last_symphony_ms())
        far.append(ctx.last_faraday_ms())
        w = ctx.last_work()
        res = {"samples": w["samples"], "faraday_samples": w["faraday_samples"], "nan": int(np.isnan(out).sum())}
    res.update(sym=sym, far=far, md5=hashlib.md5(out.tobytes()).hexdigest(), shared=bool(ctx.shared_mode()))
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    rows = sys.argv[1] if len(sys.argv) > 1 else "4096"
    got = {}
    for seq in (0, 1):
        for form, grp in (LEGS if seq == 0 else LEGS[::-1]):
            r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", form, grp, rows],
                               capture_output=True, text=True)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode or not line:
                print("leg %s %s %d ended with status %d: the run stops here\n%s" % (form, grp, seq + 1, r.returncode, r.stderr[-2000:]), flush=True)
                sys.exit(1)
            res = json.loads(line[0][7:])
            got.setdefault((form, grp), []).append(res)
            print("%-13s %-5s %d  Symphony ms %s  Faraday ms %s | samples %d + %d  NaN slots %d  md5 %s%s" % (
                form, grp, seq + 1, " ".join("%8.2f" % m for m in res["sym"]), " ".join("%8.2f" % m for m in res["far"]), res["samples"],
                res["faraday_samples"], res["nan"], res["md5"][:8], "  SHARED MODE" if res["shared"] else ""), flush=True)
    mean = lambda v, key: sum(sum(r[key]) / len(r[key]) for r in v) / len(v)
    for (form, grp), v in got.items():
        print("%-13s %-5s Symphony %8.2f ms = %7.2f ps per sample   Faraday %8.2f ms = %7.2f ps per sample" % (
            form, grp, mean(v, "sym"), 1e9 * mean(v, "sym") / v[0]["samples"], mean(v, "far"), 1e9 * mean(v, "far") / v[0]["faraday_samples"]))
    for k in ("", " sin^k"):
        for grp in ("group", "solo"):
            a, b = got[("plain" + k, grp)], got[("family" + k, grp)]
            print("family%s / plain%s, %s: Symphony %.3f  Faraday %.3f  samples %.6f + %.6f" % (
                k, k, grp, mean(b, "sym") / mean(a, "sym"), mean(b, "far") / mean(a, "far"), b[0]["samples"] / a[0]["samples"],
                b[0]["faraday_samples"] / a[0]["faraday_samples"]), flush=True)
    for form in ("family", "family sin^k"):
        assert got[(form, "group")][0]["md5"] == got[(form, "solo")][0]["md5"], "RIMPHONY_TAB_GROUP changed a bit"


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        main()
