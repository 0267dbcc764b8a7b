#!/usr/bin/env python3
"""What the ends of the spline cost a 2-D table set installed from device memory: the measurement of
profiles/tabulated_2d_ends_install_times.txt.

The three sets of tools/tab_device_install_times.py (tables x gamma nodes x mu nodes): 64 x 512 x 64 and 8 x 1024 x 1024 on
nodes uniform in ln gamma and in mu, 256 x 256 x 32 on given gamma nodes (uniform in ln(gamma - 1)) and given mu nodes
(uniform in xi), the same ln n in a CUDA tensor.  Per set a fresh process under its own `timeout` with one context: one
warm-up of either choice, then seven rounds of rimphony_ctx_set_tables_2d_device_ends with natural ends on both axes and with
not-a-knot ends on both axes, alternating, a host clock around each call; the entry returns synchronised.  Medians and
spread.  Each choice is also installed once through the host entry, and the sets read back must be equal word for word.
There is no target: the sweeps are a few per cent of an install and the ends add two steps to a line of hundreds.
usage: tab_2d_ends_install_times.py            (a set that fails ends the run: nothing further is started)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"64x512x64": (64, 512, 64, False), "8x1024x1024": (8, 1024, 1024, False), "256x256x32 nodes": (256, 256, 32, True)}
LO, HI = 1.01, 1e4
ROUNDS = 7
CHOICES = ("natural", "not-a-knot")


def child(name):
    sys.path.insert(0, ROOT)
    import time
    import numpy as np
    import torch
    from rimphony_amd import api
    nt, nn, nmu, given = SETS[name]
    gamma = api.grid_nodes_log_gm1(LO, HI, nn) if given else np.exp(np.linspace(np.log(LO), np.log(HI), nn))
    mu = api.mu_nodes_uniform_in_xi(nmu) if given else np.linspace(-1.0, 1.0, nmu)
    u, g, m = np.log(gamma)[None, :, None], gamma[None, :, None], mu[None, None, :]
    p = np.linspace(2.0, 3.5, nt)[:, None, None]
    q = np.linspace(0.0, 0.3, nt)[:, None, None]
    log_n = np.ascontiguousarray(-p * u + q * u * m + 0.5 * m - 30.0 / g - g / 500.0)
    ctx = api.Context(0)
    d = torch.as_tensor(log_n).to("cuda:0").contiguous()
    torch.cuda.synchronize()

    def put(t, ends):
        if given:
            ctx.set_tables_2d_nodes(gamma, mu, t, ends=ends)
        else:
            ctx.set_tables_2d(LO, HI, t, ends=ends)

    def device(ends):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        put(d, ends)
        return 1e3 * (time.perf_counter() - t0)

    same, nan_norms = True, 0
    for ends in CHOICES:
        put(log_n, ends)
        blob_host = ctx.tables_blob()
        device(ends)
        blob_dev = ctx.tables_blob()
        same = same and bool((blob_host.view(np.uint64) == blob_dev.view(np.uint64)).all())
        nan_norms += int(np.isnan(blob_dev[8 + 3:8 + 8 * nt:8]).sum())
    times = {e: [] for e in CHOICES}
    for _ in range(ROUNDS):
        for ends in CHOICES:
            times[ends].append(device(ends))
    res = {"same": same, "nan_norms": nan_norms, "times": times, "set_mib": blob_dev.nbytes / 2 ** 20, "shared": bool(ctx.shared_mode())}
    ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_set(name):
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", name],
                       capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode or not line:
        print("set %s ended with status %d: the run stops here\n%s" % (name, r.returncode, r.stderr[-2000:]), flush=True)
        sys.exit(1)
    return json.loads(line[0][7:])


def main():
    med = lambda v: sorted(v)[len(v) // 2]
    fmt = lambda v: "median %8.2f  min %8.2f  max %8.2f" % (med(v), min(v), max(v))
    failed = []
    for name in SETS:
        r = run_set(name)
        print("%s: set %.0f MiB, device and host sets equal word for word with either choice: %s, NaN normalisations: %d%s" % (
            name, r["set_mib"], r["same"], r["nan_norms"], "  SHARED MODE" if r["shared"] else ""))
        for ends in CHOICES:
            print("  device entry, %-10s ends  ms  %s" % (ends, fmt(r["times"][ends])))
        print("  not-a-knot / natural %.3f" % (med(r["times"]["not-a-knot"]) / med(r["times"]["natural"])), flush=True)
        if not r["same"]:
            failed.append(name)
    if failed:
        print("FAILED: the device and the host sets differ on " + ", ".join(failed))
        sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
