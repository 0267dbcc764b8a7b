#!/usr/bin/env python3
"""What installing a 2-D table set costs from the host and from device memory: the measurement of
profiles/tabulated_device_install_times.txt.

Three sets (tables x gamma nodes x mu nodes): 64 x 512 x 64 and 8 x 1024 x 1024 on nodes uniform in ln gamma and in mu,
256 x 256 x 32 on given gamma nodes (uniform in ln(gamma - 1)) and given mu nodes (uniform in xi).  ln n is a rolled power
law whose index and tilt in mu differ from table to table; it lies in a CUDA tensor, as a simulation would hold it.  Per
set a fresh process under its own `timeout` with one context: one warm-up of either path, then five rounds of
  host    tensor.cpu() (timed by itself: the copy a GPU-resident user must make to use a host entry), then the form's host
          entry -- check, serial spline solve, copy of the set to the device, normalisations on the device --,
  device  rimphony_ctx_set_tables_2d_device on the tensor -- finiteness kernel, front of the set built on the host, the three
          families of sweeps and the same normalisation kernel on the device --,
alternating, a host clock around each call; both entries return synchronised.  Medians and spread; the sets read back must be
equal word for word.  The run fails if the device entry's median is not below the host entry's on any of the sets.
usage: tab_device_install_times.py            (a set that fails ends the run: nothing further is started)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"64x512x64": (64, 512, 64, False), "8x1024x1024": (8, 1024, 1024, False), "256x256x32 nodes": (256, 256, 32, True)}
LO, HI = 1.01, 1e4
ROUNDS = 5


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

    def put(t):
        if given:
            ctx.set_tables_2d_nodes(gamma, mu, t)
        else:
            ctx.set_tables_2d(LO, HI, t)

    def host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = d.cpu().numpy()
        t1 = time.perf_counter()
        put(h)
        return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)

    def device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        put(d)
        return 1e3 * (time.perf_counter() - t0)

    host()
    blob_host = ctx.tables_blob()
    device()
    blob_dev = ctx.tables_blob()
    same = bool((blob_host.view(np.uint64) == blob_dev.view(np.uint64)).all())
    norms = blob_dev[8 + 3:8 + 8 * nt:8]
    copy, hst, dev = [], [], []
    for _ in range(ROUNDS):
        c, h = host()
        copy.append(c)
        hst.append(h)
        dev.append(device())
    res = {"same": same, "nan_norms": int(np.isnan(norms).sum()), "copy": copy, "host": hst, "device": dev,
           "input_mib": log_n.nbytes / 2 ** 20, "set_mib": blob_dev.nbytes / 2 ** 20, "shared": bool(ctx.shared_mode())}
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
        print("%s: input %.0f MiB, set %.0f MiB, sets equal word for word: %s, NaN normalisations: %d%s" % (
            name, r["input_mib"], r["set_mib"], r["same"], r["nan_norms"], "  SHARED MODE" if r["shared"] else ""))
        print("  device-to-host copy  ms  " + fmt(r["copy"]))
        print("  host entry           ms  " + fmt(r["host"]))
        print("  device entry         ms  " + fmt(r["device"]))
        print("  host / device %.2f; (copy + host) / device %.2f" % (
            med(r["host"]) / med(r["device"]), (med(r["copy"]) + med(r["host"])) / med(r["device"])), flush=True)
        if not r["same"] or not med(r["device"]) < med(r["host"]):
            failed.append(name)
    if failed:
        print("FAILED: the device entry is not below the host entry, or the sets differ, on " + ", ".join(failed))
        sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
