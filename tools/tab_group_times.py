#!/usr/bin/env python3
"""Where the Symphony slots of the tabulated kind are faster: in lock-step on the group kernel (RIMPHONY_TAB_GROUP=1) or
one wave per coefficient (RIMPHONY_SYM_SOLO=1).  The measurement of profiles/tabulated_group_times.txt.

Per form of a table set (isotropic, pitch, 2-D, sin^k) three legs, each a fresh process under its own `timeout` with one
context and four consecutive batches of the power-law bench generator's (s, theta), mask 0x3F; the whole sequence twice,
the order of the legs alternating:
  parent  the parent commit's library (PARENT_LIB; left out if none is given), one wave per coefficient
  solo    this build with RIMPHONY_SYM_SOLO=1 (by the instruction-identity record the same kernel as `parent`: a control)
  group   this build with RIMPHONY_TAB_GROUP=1
usage: tab_group_times.py [PARENT_LIB] [rows]        (a leg that fails ends the run: nothing further is started)
Decision rule printed at the end: a form defaults to the group kernel if its mean time is below the solo leg's by more than
the largest difference between two legs of the same configuration in this run."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("isotropic", "pitch", "2-D", "sin^k")


def child(form, rows):
    sys.path.insert(0, ROOT)
    import numpy as np
    from rimphony_amd import api, workload
    lo, hi = 1.01, 1e4

    def energy(n):          # the rolled power law gamma^-2.5 exp(-30/gamma - gamma/500) at n nodes uniform in ln gamma
        g = np.exp(np.linspace(np.log(lo), np.log(hi), n))
        return -2.5 * np.log(g) - 30.0 / g - g / 500.0

    def pitch(n):           # G = 0.8 mu - 1.5 mu^2 at n nodes uniform in mu
        mu = np.linspace(-1.0, 1.0, n)
        return 0.8 * mu - 1.5 * mu * mu

    ctx = api.Context(0)
    if form == "isotropic":
        ctx.set_tables(lo, hi, energy(2048))
    elif form == "pitch":
        ctx.set_tables(lo, hi, energy(2048), pitch(257))
    elif form == "2-D":
        ctx.set_tables_2d(lo, hi, energy(512)[:, None] + pitch(65)[None, :])
    else:
        ctx.set_tables(lo, hi, energy(2048), sin_k=1.5)
    _, _, s, th, _ = workload.make_batch("cfg2_powerlaw_8", rows, start=0)
    index = np.zeros(rows)
    ms, res = [], None
    for _ in range(4):
        out = ctx.compute_batch(api.TABULATED, s, th, [index], 0x3F)
        ms.append(ctx.last_symphony_ms())
        w = ctx.last_work()
        res = {"samples": w["samples"], "passes": w["passes"], "nan": int(np.isnan(out[:, :6]).sum()),
               "member_passes": ctx.last_tail()["member_passes"]}
    import hashlib
    res.update(ms=ms, md5=hashlib.md5(out.tobytes()).hexdigest(), shared=bool(ctx.shared_mode()))
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    parent = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] else None
    rows = sys.argv[2] if len(sys.argv) > 2 else "4096"
    legs = ([("parent", {"RIMPHONY_HIP_LIB": parent})] if parent else []) + \
        [("solo", {"RIMPHONY_SYM_SOLO": "1"}), ("group", {"RIMPHONY_TAB_GROUP": "1"})]
    got = {}                # (form, leg) -> [result of sequence 1, of sequence 2]
    for seq in (0, 1):
        for form in FORMS:
            for leg, env in (legs if seq == 0 else legs[::-1]):
                base = {k: v for k, v in os.environ.items() if k not in ("RIMPHONY_SYM_SOLO", "RIMPHONY_TAB_GROUP", "RIMPHONY_HIP_LIB")}
                r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", form, rows],
                                   env=dict(base, **env), capture_output=True, text=True)
                line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode or not line:
                    print("leg %s %s %d ended with status %d: the run stops here\n%s" % (form, leg, seq + 1, r.returncode, r.stderr[-2000:]), flush=True)
                    sys.exit(1)
                res = json.loads(line[0][7:])
                got.setdefault((form, leg), []).append(res)
                print("%-9s %-6s %d  Symphony ms %s | samples %d  passes %d  member passes %d  NaN slots %d  md5 %s%s" % (
                    form, leg, seq + 1, " ".join("%8.2f" % m for m in res["ms"]), res["samples"], res["passes"], res["member_passes"],
                    res["nan"], res["md5"][:8], "  SHARED MODE" if res["shared"] else ""), flush=True)
    mean = lambda r: sum(r["ms"]) / len(r["ms"])
    scatter = max(abs(mean(v[0]) - mean(v[1])) for v in got.values())
    print("largest difference between the two legs of one configuration: %.2f ms" % scatter)
    for form in FORMS:
        m = {leg: (mean(got[form, leg][0]) + mean(got[form, leg][1])) / 2 for leg, _ in legs}
        for leg, _ in legs:
            r = got[form, leg][0]
            print("%-9s %-6s mean %8.2f ms (%.2f / %.2f)  %6.2f ps per sample  %6.1f samples per pass" % (
                form, leg, m[leg], mean(got[form, leg][0]), mean(got[form, leg][1]), 1e9 * m[leg] / r["samples"], r["samples"] / r["passes"]))
        same = len({r["md5"] for leg, _ in legs for r in got[form, leg]}) == 1
        print("%-9s group / solo %.3f   tables identical: %s   default: %s" % (
            form, m["group"] / m["solo"], same, "group" if m["solo"] - m["group"] > scatter and same else "solo"), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]))
    else:
        main()
