#!/usr/bin/env python3
"""What the cubic blend across four surfaces costs per sample against the linear blend of two, and what the per-row normalisation
costs per batch: the measurements of profiles/tabulated_2d_family_cubic_times.txt.

Samples.  A four-table family of tilted power laws ln n = -p u + q u mu + a mu - gamma / 1e10, (p, a, q) = (2.5, 0.8, 0.3),
(2.9, 0.65, 0.22), (3.2, 0.5, 0.15) and (3.5, 0.4, 0.1), on 2048 gamma nodes uniform in ln(gamma - 1) over [1 + 1e-6, 1e12] x 16
mu nodes uniform in xi -- 1 MiB of node data per table --, every row at x = 1.5, installed with blend="cubic" (internal kinds 18
and, with sin_k = (0, 1, 2, 3), 19) and with blend="linear" (kinds 16 and 17, the parent commit's kernels:
profiles/tabulated_2d_family_cubic_unchanged.txt).  The two blends give nearly the same function there -- the content is close to
linear in the index --, so nearly the same samples, and the cubic blend's extra loads and arithmetic in full.  Each leg is a
fresh process under its own `timeout` with one context, RIMPHONY_TAB_GROUP set to 1 (group kernel) or 0 (one wave per
coefficient), and three consecutive batches of the power-law bench generator's (s, theta), all eight slots; the whole sequence
twice, forward and in reverse.  Times are rimphony_last_symphony_ms and rimphony_last_faraday_ms, samples rimphony_last_work's
(Symphony and Faraday apart).

Normalisation.  rimphony_batch_norm of `rows` rows at x = 1.5 of the same kind of family on 128 gamma nodes x n_mu mu nodes, n_mu =
8 and 64, either blend, without and with sin_k: the host's clock around each of three calls (the call ends when the norms are
on the host; 32 KiB of traffic).
usage: tab_2d_family_cubic_times.py [rows]        (a leg that fails ends the run: nothing further is started)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = [(form, grp) for form in ("linear", "cubic", "linear sin^k", "cubic sin^k") for grp in ("group", "solo")]
NORM_NMU = (8, 64)
PAQ = ((2.5, 0.8, 0.3), (2.9, 0.65, 0.22), (3.2, 0.5, 0.15), (3.5, 0.4, 0.1))
SIN_K = [0.0, 1.0, 2.0, 3.0]
X = 1.5


def surfaces(np, n_nodes, n_mu):
    from rimphony_amd import api
    g = 1.0 + np.exp(np.linspace(np.log(1e-6), np.log(1e12 - 1.0), n_nodes))
    g[0], g[-1] = 1.0 + 1e-6, 1e12
    mu = api.mu_nodes_uniform_in_xi(n_mu)
    u = np.log(g)[:, None]
    return g, mu, np.stack([-p * u + q * u * mu[None, :] + a * mu[None, :] - g[:, None] / 1e10 for p, a, q in PAQ])


def child(form, grp, rows):
    sys.path.insert(0, ROOT)
    os.environ["RIMPHONY_TAB_GROUP"] = "1" if grp == "group" else "0"
    import hashlib
    import numpy as np
    from rimphony_amd import api, workload
    g, mu, t = surfaces(np, 2048, 16)
    ctx = api.Context(0)
    ctx.set_tables_2d_family(g, mu, t, SIN_K if form.endswith("sin^k") else None, blend=form.split()[0])
    index = np.full(rows, X)
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


def norm_child(n_mu, with_k, blend, rows):
    sys.path.insert(0, ROOT)
    import time
    import numpy as np
    from rimphony_amd import api
    g, mu, t = surfaces(np, 128, n_mu)
    ctx = api.Context(0)
    ctx.set_tables_2d_family(g, mu, t, SIN_K if with_k else None, blend=blend)
    x = np.full(rows, X)
    ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        nrm = ctx.norm_batch(api.TABULATED, [x])
        ms.append(1e3 * (time.perf_counter() - t0))
    ok = bool(np.isfinite(nrm).all() and (nrm == nrm[0]).all())
    ctx.close()
    print("RESULT " + json.dumps({"ms": ms, "ok": ok, "norm": float(nrm[0])}), flush=True)


def run(args, limit):
    r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode or not line:
        print("leg %s ended with status %d: the run stops here\n%s" % (" ".join(args), r.returncode, r.stderr[-2000:]), flush=True)
        sys.exit(1)
    return json.loads(line[0][7:])


def main():
    rows = sys.argv[1] if len(sys.argv) > 1 else "4096"
    got = {}
    for seq in (0, 1):
        for form, grp in (LEGS if seq == 0 else LEGS[::-1]):
            res = run(["--child", form, grp, rows], 240)
            got.setdefault((form, grp), []).append(res)
            print("%-13s %-5s %d  Symphony ms %s  Faraday ms %s | samples %d + %d  NaN slots %d  md5 %s%s" % (
                form, grp, seq + 1, " ".join("%8.2f" % m for m in res["sym"]), " ".join("%8.2f" % m for m in res["far"]), res["samples"],
                res["faraday_samples"], res["nan"], res["md5"][:8], "  SHARED MODE" if res["shared"] else ""), flush=True)
    mean = lambda v, key: sum(sum(r[key]) / len(r[key]) for r in v) / len(v)
    for (form, grp), v in got.items():
        print("%-13s %-5s Symphony %8.2f ms = %7.2f ps per sample   Faraday %8.2f ms = %7.2f ps per sample" % (
            form, grp, mean(v, "sym"), 1e9 * mean(v, "sym") / v[0]["samples"], mean(v, "far"), 1e9 * mean(v, "far") / v[0]["faraday_samples"]))
    per = lambda v, key, n: mean(v, key) / v[0][n]
    for k in ("", " sin^k"):
        for grp in ("group", "solo"):
            a, b = got[("linear" + k, grp)], got[("cubic" + k, grp)]
            print("cubic%s / linear%s, %s, per sample: Symphony %.3f  Faraday %.3f  (samples %.6f + %.6f)" % (
                k, k, grp, per(b, "sym", "samples") / per(a, "sym", "samples"),
                per(b, "far", "faraday_samples") / per(a, "far", "faraday_samples"), b[0]["samples"] / a[0]["samples"],
                b[0]["faraday_samples"] / a[0]["faraday_samples"]), flush=True)
        a, b = got[("cubic" + k, "group")], got[("cubic" + k, "solo")]
        print("cubic%s, solo / group: Symphony %.3f" % (k, mean(b, "sym") / mean(a, "sym")), flush=True)
    for form in ("cubic", "cubic sin^k"):
        assert got[(form, "group")][0]["md5"] == got[(form, "solo")][0]["md5"], "RIMPHONY_TAB_GROUP changed a bit"
    for n_mu in NORM_NMU:
        for with_k in (0, 1):
            for blend in ("linear", "cubic"):
                res = run(["--norm", str(n_mu), str(with_k), blend, rows], 400)
                print("normalisation of %s rows, 128 x %3d nodes, %-6s %-10s  ms %s%s" % (
                    rows, n_mu, blend, "sin_k" if with_k else "no sin_k", " ".join("%9.2f" % m for m in res["ms"]),
                    "" if res["ok"] else "  NOT FINITE"), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--norm":
        norm_child(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    else:
        main()
