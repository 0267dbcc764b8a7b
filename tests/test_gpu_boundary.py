"""GPU tests of the boundary added in round 2: per-coefficient work counters, status histogram, the in-process
multi-device entry, shared / exclusive contexts, stream ordering on one context, the host build of the scalar Bessel
seam against the device batch entry, argument validation, the literal-flavour vectors, and bench.py launching its
own ranks.  Everything goes through the C ABI (rimphony_amd/capi.py)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import faraday_long as fl
import oracle_bind
from rimphony_amd import api, capi, workload

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def test_work_counters_per_coefficient(gpu_ctx, oracle):
    """`work` [n][8] (SURVEY 8b `counters`): integrand samples per coefficient.  Their sum is the launch aggregate of
    rimphony_last_work, unselected slots are 0, and each entry equals the sample count the oracle reports for that
    coefficient (same decision trace -> same work), whichever wave evaluated the requests."""
    kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_8", 96, start=1000000)
    out, st, work = gpu_ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True, want_work=True)
    w = gpu_ctx.last_work()
    assert work[:, :6].sum() == w["samples"]
    assert work[:, 6:].sum() == w["faraday_samples"]
    assert (work > 0).all()
    out2, work2 = gpu_ctx.compute_batch(kind, s, th, params, 0x41, want_work=True)
    assert (work2[:, [1, 2, 3, 4, 5, 7]] == 0).all()
    assert (work2[:, [0, 6]] == work[:, [0, 6]]).all()
    assert same_bits(out2[:, [0, 6]], out[:, [0, 6]]).all()
    for i in (3, 40, 77):
        d, rc = oracle_bind.mkdist(oracle, kind, [p[i] for p in params])
        for slot, (co, stk) in enumerate(api.SLOTS):
            c = oracle_bind.Counters()
            oracle.rimo_compute_dimensionless(d, int(co), int(stk), s[i], th[i], ctypes.byref(c))
            assert c.integrand_evals == work[i, slot], (i, slot)


def test_status_histogram(gpu_ctx):
    import torch
    kind, mask, s, th, params = workload.make_batch("cfg3_thermal_8", 512)
    dev = torch.device("cuda", 0)
    d = [torch.from_numpy(a).to(dev) for a in [s, th] + params]
    out, st = gpu_ctx.compute_batch_device(kind, d[0], d[1], d[2:], 0x3F, want_status=True)
    hist = gpu_ctx.status_histogram(st)
    sth = st.cpu().numpy()
    for slot in range(8):
        for b in range(7):
            assert hist[slot, b] == ((sth[:, slot] >> b) & 1).sum()
        assert hist[slot, 7] == (sth[:, slot] == 0).sum()
    assert hist[6, 6] == 512 and hist[7, 6] == 512          # unselected slots: NOT_COMPUTED


def test_multi_device_entry_and_shared_mode(gpu_ctx):
    """rimphony_batch_compute_multi on a 1-GPU box: n_ctx = 1 is the plain call; n_ctx = 2 and 3 with extra contexts on
    the SAME device exercise the interleaved shard / scatter logic (ragged sizes) -- the table must not depend on
    n_ctx.  A context created while another holds the device runs in shared mode."""
    kind, mask, s, th, params = workload.make_batch("cfg4_pitchypl_8", 37)
    ref, rst = gpu_ctx.compute_batch(kind, s, th, params, 0xC3, want_status=True)
    one, ost, owk = api.compute_batch_multi([gpu_ctx], kind, s, th, params, 0xC3, want_status=True, want_work=True)
    assert same_bits(one, ref).all() and (ost == rst).all()
    c2, c3 = api.Context(0), api.Context(0)
    try:
        assert c2.shared_mode() and c3.shared_mode()
        two, tst, twk = api.compute_batch_multi([gpu_ctx, c2], kind, s, th, params, 0xC3, want_status=True, want_work=True)
        three = api.compute_batch_multi([c3, gpu_ctx, c2], kind, s, th, params, 0xC3)
        assert same_bits(two, ref).all() and (tst == rst).all() and (twk == owk).all()
        assert same_bits(three, ref).all()
        # a shared-mode context alone gives the same bits too (smaller grid, no cooperative tail)
        assert same_bits(c2.compute_batch(kind, s, th, params, 0xC3), ref).all()
    finally:
        c2.close()
        c3.close()


def test_multi_device_entry_with_device_buffers(gpu_ctx):
    """rimphony_batch_compute_multi_device: per-context DEVICE buffers, launches issued from one thread, one
    synchronisation at the end.  On a 1-GPU box the second and third contexts share the device (shared mode); interleaved
    ragged shards of 37 rows must reassemble to the one-call table, status words included."""
    import torch
    dev = torch.device("cuda", 0)
    kind, mask, s, th, params = workload.make_batch("cfg3_thermal_8", 37)
    ref, rst = gpu_ctx.compute_batch(kind, s, th, params, 0xC3, want_status=True)
    c2, c3 = api.Context(0), api.Context(0)
    try:
        dv = ctypes.c_int(-1)
        assert capi.load().rimphony_ctx_device(c2.handle, ctypes.byref(dv)) == 0 and dv.value == 0
        ctxs = [gpu_ctx, c2, c3]
        shards = []
        for r in range(3):
            idx = np.arange(r, 37, 3)
            shards.append((torch.from_numpy(s[idx]).to(dev), torch.from_numpy(th[idx]).to(dev),
                           [torch.from_numpy(p[idx]).to(dev) for p in params]))
        outs, stats = api.compute_batch_multi_device(ctxs, kind, shards, 0xC3, want_status=True)
        got = np.empty((37, 8)); gst = np.empty((37, 8), dtype=np.int32)
        for r in range(3):
            got[r::3] = outs[r].cpu().numpy(); gst[r::3] = stats[r].cpu().numpy()
        assert same_bits(got, ref).all() and (gst == rst).all()
        # an empty shard is skipped, a missing buffer of a non-empty one is an argument error
        outs = api.compute_batch_multi_device([gpu_ctx, c2], kind, [shards[0], (shards[1][0][:0], shards[1][1][:0], [p[:0] for p in shards[1][2]])], 0xC3)
        assert same_bits(outs[0].cpu().numpy(), ref[0::3]).all() and outs[1].shape == (0, 8)
    finally:
        c2.close()
        c3.close()


def test_rccl_gather_of_the_c_abi_in_a_world_of_one(gpu_ctx):
    """north_star's "RCCL gather over xGMI" below Python: rimphony_rccl_* dlopen librccl, make a communicator on the
    context's device and run the grouped send / receive + un-interleave of rimphony_rccl_gather_table -- here in a world of
    one (the root sends to itself: the same RCCL calls as in a world of eight), with and without caller scratch."""
    import torch
    assert api.RcclComm.available(), capi.load().rimphony_last_error()
    dev = torch.device("cuda", 0)
    kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_jI_aI", 67)
    out, _ = gpu_ctx.compute_batch_device(kind, *[torch.from_numpy(x).to(dev) for x in (s, th)],
                                          [torch.from_numpy(p).to(dev) for p in params], mask)
    comm = api.RcclComm(gpu_ctx, 0, 1, api.RcclComm.unique_id())
    try:
        table = comm.gather_table(out, 67)
        torch.cuda.synchronize()
        assert same_bits(table.cpu().numpy(), out.cpu().numpy()).all()
        scratch = torch.empty((67, 8), dtype=torch.float64, device=dev)
        table2 = comm.gather_table(out, 67, scratch=scratch)
        torch.cuda.synchronize()
        assert same_bits(table2.cpu().numpy(), out.cpu().numpy()).all()
    finally:
        comm.close()


def test_heartbeat_is_refused_where_nothing_would_write_it(gpu_ctx):
    """The group kernel (default for the Symphony slots) writes no heartbeat words: asking for a Symphony task's
    heartbeat on such a context is RIMPHONY_ENOTSUP, a Faraday task's (task | 1 << 62) is served."""
    with pytest.raises(capi.RimphonyError) as e:
        gpu_ctx.heartbeat(0)
    assert "code -6" in str(e.value)
    hb = gpu_ctx.heartbeat((1 << 62) | 1)
    assert hb is not None


def test_exclusive_env_refuses_second_context(gpu_ctx):
    os.environ["RIMPHONY_EXCLUSIVE"] = "1"
    try:
        with pytest.raises(capi.RimphonyError) as e:
            api.Context(0)
        assert "code -5" in str(e.value)
    finally:
        del os.environ["RIMPHONY_EXCLUSIVE"]


def test_calls_on_two_streams_of_one_context_are_ordered(gpu_ctx):
    """Two batch calls on different streams share the context's workspace: the library orders them (each call's
    stream waits for the previous call's work), so both tables are the ones sequential calls give."""
    import torch
    dev = torch.device("cuda", 0)
    kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_jI_aI", 3000)
    a = [torch.from_numpy(x[:1500].copy()).to(dev) for x in [s, th] + params]
    b = [torch.from_numpy(x[1500:].copy()).to(dev) for x in [s, th] + params]
    ra, _ = gpu_ctx.compute_batch_device(kind, a[0], a[1], a[2:], mask)
    rb, _ = gpu_ctx.compute_batch_device(kind, b[0], b[1], b[2:], mask)
    torch.cuda.synchronize(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(s1):
        qa, _ = gpu_ctx.compute_batch_device(kind, a[0], a[1], a[2:], mask)
    with torch.cuda.stream(s2):
        qb, _ = gpu_ctx.compute_batch_device(kind, b[0], b[1], b[2:], mask)
    w = gpu_ctx.last_work()          # reads after the second call's work, whatever stream it ran on
    torch.cuda.synchronize(dev)
    assert same_bits(qa.cpu().numpy(), ra.cpu().numpy()).all()
    assert same_bits(qb.cpu().numpy(), rb.cpu().numpy()).all()
    assert w["samples"] > 0


def test_scalar_bessel_seam_matches_device_batch(gpu_ctx):
    """pkgw_bessel_j / pkgw_bessel_dj are the host build of the device functions: same bits as the batched device
    entry on the same arguments (leung-bessel/src/lib.rs:36-42, 56-75)."""
    rng = np.random.default_rng(5)
    n = np.concatenate([np.exp(rng.uniform(np.log(30), np.log(1e13), 4000)), rng.integers(0, 30, 500).astype(float)])
    x = n * rng.uniform(0.3, 1.2, n.size)
    j, dj = gpu_ctx.bessel_batch(n, x)
    lib = capi.load()
    hj = np.array([lib.pkgw_bessel_j(a, b) for a, b in zip(n, x)])
    hdj = np.array([lib.pkgw_bessel_dj(a, b) for a, b in zip(n, x)])
    assert same_bits(hj, j).all() and same_bits(hdj, dj).all()


def test_api_refuses_views_and_wrong_dtypes(gpu_ctx):
    import torch
    dev = torch.device("cuda", 0)
    kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_jI_aI", 8)
    d = [torch.from_numpy(a).to(dev) for a in [s, th] + params]
    table = torch.stack(d, dim=1)                       # [8, 6]: columns are strided views
    with pytest.raises(ValueError):
        gpu_ctx.compute_batch_device(kind, table[:, 0], d[1], d[2:], mask)
    with pytest.raises(TypeError):
        gpu_ctx.compute_batch_device(kind, d[0].float(), d[1], d[2:], mask)
    with pytest.raises(ValueError):
        gpu_ctx.compute_batch_device(kind, d[0], d[1], [d[2], d[3], d[4][:1], d[5]], mask)    # length-1 "broadcast"
    with pytest.raises(ValueError):
        gpu_ctx.compute_batch_device(kind, d[0], d[1].cpu(), d[2:], mask)


# Bounds of the HIP-vs-literal distance per table: 2 x the measured values (bench.py prints the live numbers as `parity`):
# (p99, max, coefficients beyond 1e-6, one-sided NaNs either way).  What is left of a tail on the eight-coefficient tables
# is rho_Q / rho_V of the two anisotropic distributions; `parity.control` shows the same between two
# builds of the literal flavour itself.
LITERAL_BOUNDS = {
    # round 4 (profiles/r4_det_vs_literal.txt; twice the measured values).  Round 3's bounds were (2.9e-8, 1.4e-5, 24, 2),
    # (1.1e-7, 1.8e-5, 24, 12), (6.5e-7, 7.5e-5, 130, 10), (4.2e-7, 5.1e-5, 70, 26): the whole Faraday tail they allowed
    # for was the LITERAL flavour's inaccurate Gamma function (profiles/r4_faraday_tail_attribution.txt).
    "cfg2_powerlaw_jI_aI": (4.3e-10, 4.0e-9, 0, 0),
    "cfg2_powerlaw_8": (1.2e-8, 1.2e-6, 0, 0),
    "cfg3_thermal_8": (1.0e-8, 2.6e-7, 0, 12),
    "cfg4_pitchypl_8": (1.1e-7, 1.5e-5, 8, 10),
    "cfg5_pitchykappa_8": (7.0e-8, 1.5e-6, 2, 20),
}


@pytest.mark.parametrize("cfg", sorted(LITERAL_BOUNDS))
def test_against_literal_flavour_vectors(gpu_ctx, cfg):
    """HIP vs the committed output of the oracle's literal flavour (glibc libm, unfused, GSL summation order) on all five
    tables: the distribution bench.py reports as `parity`.  Since round 4 the power-law and thermal tables hold NO
    coefficient beyond 1e-6 (the class of the literal flavour's own contracted control); a regression of a tail or of the
    one-sided NaN counts fails here.  Symphony slots must agree on the NaN pattern EXACTLY since round 3 (the rule sums are formed
    from QUADPACK's own pair terms: wave_qag.h)."""
    path = os.path.join(ROOT, "tests", "golden", "literal_%s.npz" % cfg)
    z = np.load(path)
    n, start, m = int(z["n"]), int(z["start"]), int(z["mask"])
    kind, _, s, th, params = workload.make_batch(cfg, n, start=start)
    got = gpu_ctx.compute_batch(kind, s, th, params, m)
    r = workload.compare_tables(got, z["out"], m)
    p99, mx, beyond, onesided = LITERAL_BOUNDS[cfg]
    assert r["median"] < 1e-13, r
    assert r["p99"] <= p99 and r["max"] <= mx, r
    assert round((1. - r["within_1e-6"]) * r["both_finite"]) <= beyond, r
    assert r["nan_only_here"] + r["nan_only_there"] <= onesided, r
    sym = workload.compare_tables(got, z["out"], m & 0x3F)
    assert sym["nan_only_here"] == 0 and sym["nan_only_there"] == 0, sym
    assert sym["max"] < 1e-7, sym          # the Symphony coefficients meet north_star's 1e-6 with a decade to spare


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 4` without torchrun: the parent spawns the ranks before touching the GPU.  On this
    1-GPU box the four ranks share cuda:0 (RIMPHONY_BENCH_REHEARSE=1, gloo: one context owns the device, three run in
    shared mode), which exercises the launcher, the interleaved sharding and the gather, not the speed.  (Four ranks, not
    the eight of the scaling run: the box allows six processes on its card, this test runner included; the eight-rank
    launcher / shard / gather path runs on the CPU in tests/test_host_side.py.)"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["RIMPHONY_BENCH_REHEARSE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1", "--warmup", "0",
                        "--points", "67", "--side-rows", "0", "--cpu-sample", "0", "--no-parity"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 4 and line["value"] > 0 and line["roofline"]["frac"] > 0
    assert line["config"]["points_per_step_per_gpu"] == 67


def test_bench_runs_the_rccl_path_in_a_world_of_one():
    """RCCL initialised and the device-tensor gather executed on real hardware (multi-GPU readiness):
    bench.py with RIMPHONY_BENCH_FORCE_DIST=1 calls init_process_group("nccl") and runs sharding.gather_table's
    dist.gather on CUDA tensors without the world-of-one short cut."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["RIMPHONY_BENCH_FORCE_DIST"] = "1"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0",
                        "--points", "256", "--side-rows", "0", "--cpu-sample", "0", "--no-parity"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["value"] > 0
    assert "kernel_ms_min_max_over_ranks" in line["roofline"]      # only present when the collectives ran


def test_bench_side_objects_only_with_full(gpu_ctx):
    """A plain bench run does only what its headline needs: the side legs, `parity` and `cpu_baseline` are printed as
    null.  --full measures them (here on tiny sizes) in the same line."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--points", "64"]
    side = ("two_coeff", "thermal_eight", "pitchypl_eight", "pitchykappa_eight", "corner_theta_lt_0.05", "gamma_min_1",
            "parity", "cpu_baseline")
    with gpu_ctx.released():
        for extra, full in (([], False), (["--full", "--side-rows", "64", "--cpu-sample", "8"], True)):
            r = subprocess.run(cmd + extra, capture_output=True, text=True, env=env, timeout=900)
            assert r.returncode == 0, r.stderr[-3000:]
            line = json.loads(r.stdout.strip().splitlines()[-1])
            assert line["full"] is full and line["value"] > 0 and line["roofline"]["frac"] > 0
            assert [k for k in side if (line[k] is not None) != full] == []


def test_f32_integrand_is_refused_and_slower_where_it_still_runs(gpu_ctx):
    """RIMPHONY_PRECISION_F32_INTEGRAND (BASELINE configs[4]) is not a mode of the product: RIMPHONY_ENOTSUP for every
    distribution (include/rimphony_hip.h says why), as is an unknown precision.  The claim behind the refusal is
    re-measured here through the measurement hook (a context created with RIMPHONY_F32_VARIANT=1; each leg on a context
    that owns the device, one after the other): on the same 8192 power-law rows the variant's kernel time must NOT
    beat the fp64 default's -- if it ever does, this test fails and the refusal has to be reconsidered -- and it carries
    the error envelope recorded in round 2 (bulk ~1e-8, a tail from the noise-driven control flow); the Faraday pair is not
    part of the variant (fp64 bits)."""
    from rimphony_amd import api
    for cfg in ("cfg2_powerlaw_8", "cfg3_thermal_8", "cfg5_pitchykappa_8", "cfg4_pitchypl_8"):
        kind, mask, s, th, params = workload.make_batch(cfg, 8)
        for prec in (api.PRECISION_F32_INTEGRAND, 7):
            with pytest.raises(capi.RimphonyError) as e:
                gpu_ctx.compute_batch(kind, s, th, params, 0x3F, precision=prec)
            assert "code -6" in str(e.value)
        out = gpu_ctx.compute_batch(kind, s, th, params, 0x3F)          # the fp64 path serves the same rows
        assert np.isfinite(out[:, :6]).any()
    # the measurement: each leg on a context that OWNS the device (full grids, cooperative tail), one after the other
    kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_8", 8192, start=1000000)
    with gpu_ctx.released():
        plain = api.Context(0)
        try:
            assert not plain.shared_mode()
            plain.compute_batch(kind, s[:256], th[:256], [p[:256] for p in params], 0x3F)
            f64 = plain.compute_batch(kind, s, th, params, 0x3F)
            t64 = plain.last_symphony_ms()
            a = plain.compute_batch(kind, s[:64], th[:64], [p[:64] for p in params], 0xC0)
        finally:
            plain.close()
        os.environ["RIMPHONY_F32_VARIANT"] = "1"
        try:
            hook = api.Context(0)
        finally:
            del os.environ["RIMPHONY_F32_VARIANT"]
        try:
            assert not hook.shared_mode()
            hook.compute_batch(kind, s[:256], th[:256], [p[:256] for p in params], 0x3F, precision=api.PRECISION_F32_INTEGRAND)
            f32 = hook.compute_batch(kind, s, th, params, 0x3F, precision=api.PRECISION_F32_INTEGRAND)
            t32 = hook.last_symphony_ms()
            b = hook.compute_batch(kind, s[:64], th[:64], [p[:64] for p in params], 0xC0, precision=api.PRECISION_F32_INTEGRAND)
            # the hook does not open the anisotropic kinds
            k3, _, s3, th3, p3 = workload.make_batch("cfg5_pitchykappa_8", 8)
            with pytest.raises(capi.RimphonyError):
                hook.compute_batch(k3, s3, th3, p3, 0x3F, precision=api.PRECISION_F32_INTEGRAND)
        finally:
            hook.close()
    assert t32 >= t64, ("the fp32-integrand variant ran faster than fp64: reconsider the refusal", t32, t64)
    r = workload.compare_tables(f32, f64, 0x3F)
    assert r["bit_identical"] < 0.5                         # it IS a different arithmetic
    assert r["median"] < 1e-6 and r["within_1e-6"] > 0.95 and r["max"] < 5e-2, r
    assert r["nan_only_here"] + r["nan_only_there"] <= 0.01 * r["coefficients"], r
    assert same_bits(a[:, 6:], b[:, 6:]).all()              # the Faraday pair is not part of the variant: fp64 bits


def test_early_help_and_faraday_order_change_no_bit(gpu_ctx):
    """The Faraday launch's scheduling knobs (round 4): its own visiting order (the window 0.9 <= s sin(theta) <= 3 first,
    then ascending; RIMPHONY_FARADAY_ORDER=symphony restores the shared one) and the squad that serves the longest outer
    quadratures from the start of a launch (coop_common.h; RIMPHONY_EARLY_SQUAD = 0 / 64 / 256: off, one title, four
    titles), and the ROUNDS of a long outer quadrature (heyvaerts_wave.h: the children of up to four intervals per batch,
    their rule sums filed ahead of qag.c's picks; RIMPHONY_ROUNDS=0: one interval per batch).  Who evaluates a request, and
    when, never changes its value: the same 12288 power-law and pitchy-kappa rows
    (enough tasks for the squad to be switched on: four per wave of the grid) give the same table and status words, bit
    for bit, under every setting.  Each leg on a context that owns the device."""
    from rimphony_amd import api
    for cfg in ("cfg2_powerlaw_8", "cfg5_pitchykappa_8"):
        kind, _, s, th, params = workload.make_batch(cfg, 12288, start=1131072 if cfg == "cfg2_powerlaw_8" else 0)
        ref = None
        works = []
        for env in ({"RIMPHONY_EARLY_SQUAD": "0", "RIMPHONY_FARADAY_ORDER": "symphony", "RIMPHONY_ROUNDS": "0"}, {"RIMPHONY_EARLY_SQUAD": "0"},
                    {"RIMPHONY_ROUNDS": "0"},
                    {"RIMPHONY_EARLY_SQUAD": "64", "RIMPHONY_EARLY_MIN": "4"}, {"RIMPHONY_EARLY_SQUAD": "256", "RIMPHONY_EARLY_MIN": "4"}, {}):
            with gpu_ctx.released():
                os.environ.update(env)
                try:
                    ctx = api.Context(0)
                finally:
                    for k in env:
                        del os.environ[k]
                try:
                    assert not ctx.shared_mode()
                    out, st = ctx.compute_batch(kind, s, th, params, 0xC0, want_status=True)
                    works.append(ctx.last_work())
                finally:
                    ctx.close()
            if ref is None:
                ref = (out, st)
            else:
                assert same_bits(out[:, 6:], ref[0][:, 6:]).all(), (cfg, env)
                assert (st[:, 6:] == ref[1][:, 6:]).all(), (cfg, env)
        # the launch's sample count is the reference's under every setting (what a round evaluates ahead and nobody asks for
        # comes off it) -- and the rounds did run where they are compiled in: the pitchy-kappa launches evaluated inner
        # integrals that the plain ones (settings 0 and 2: RIMPHONY_ROUNDS=0) did not (the children of intervals that
        # were filed and never picked); the power-law kernel is built without rounds
        assert len({w["faraday_samples"] for w in works}) == 1, (cfg, [w["faraday_samples"] for w in works])
        q = [w["faraday_inner_qags"] for w in works]
        if cfg == "cfg5_pitchykappa_8":
            assert q[0] == q[2] and min(q[1], q[3], q[4]) > q[0], q
        else:
            assert len(set(q)) == 1, q
        # ... and the table all six settings agree on is the ORACLE's where the outer quadratures are longest: the batch holds
        # three rows of the committed fixture of long quadratures (tests/golden/faraday_long_det.npz; lists of 4096 and of
        # 3739 entries), whose rho_Q and rho_V carry the deterministic oracle's bits
        long_rows = fl.load()
        start = 1131072 if cfg == "cfg2_powerlaw_8" else 0
        held = [i for i in range(len(long_rows["row"]))
                if long_rows["config"][i] == cfg and long_rows["cls"][i] == "limit" and start <= long_rows["row"][i] < start + 12288]
        assert len(held) == (1 if cfg == "cfg2_powerlaw_8" else 2), held
        for i in held:
            at = int(long_rows["row"][i]) - start
            assert s[at] == long_rows["s"][i] and th[at] == long_rows["theta"][i]
            assert same_bits(ref[0][at, 6:], long_rows["values"][i, 6:]).all(), (cfg, at, ref[0][at, 6:], long_rows["values"][i, 6:])


def test_kernel_variants_change_no_bit(gpu_ctx):
    """The A/B switches of the library: RIMPHONY_SYM_SOLO=1 (one wave per (point, coefficient), the round-2 Symphony
    kernel) and RIMPHONY_FARADAY_GROUP=1 (rho_Q and rho_V of a point in lock-step, heyvaerts_group.h -- measured slower,
    off by default).  Each in a child process (the variables are read when a context is created; the child's context runs
    in shared mode next to this one): same table and status words, bit for bit, as the default configuration."""
    code = r'''
import sys
sys.path.insert(0, %r)
import numpy as np
from rimphony_amd import api, workload
ctx = api.Context(0)
kind, mask, s, th, params = workload.make_batch("cfg4_pitchypl_8", 96)
out, st = ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True)
np.save(sys.argv[1], out); np.save(sys.argv[2], st)
ctx.close()
''' % ROOT
    import tempfile
    kind, mask, s, th, params = workload.make_batch("cfg4_pitchypl_8", 96)
    ref, ref_st = gpu_ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True)
    for var in ("RIMPHONY_SYM_SOLO", "RIMPHONY_FARADAY_GROUP"):
        with tempfile.TemporaryDirectory() as td:
            fo, fs = os.path.join(td, "o.npy"), os.path.join(td, "s.npy")
            env = dict(os.environ, **{var: "1"})
            r = subprocess.run([sys.executable, "-c", code, fo, fs], capture_output=True, text=True, env=env, timeout=900)
            assert r.returncode == 0, r.stderr[-3000:]
            out, st = np.load(fo), np.load(fs)
        assert same_bits(out, ref).all(), var
        assert (st == ref_st).all(), var


def test_owner_fallback_changes_no_bit(gpu_ctx):
    """The cooperative tail's last resort: an owner whose helpers do not answer in time closes its batch, evaluates all
    of it itself and never publishes again.  With the bound cut to 1 microsecond (RIMPHONY_OWNER_WAIT_US) nearly every
    published batch takes that path, helpers still write late results into abandoned slots -- and the table is the
    same, bit for bit, status for status and work counter for work counter, as the normal run's (run in a child process: the variable is read when
    a context is created, and the child's context runs in shared mode next to this one unless it comes first)."""
    code = r'''
import sys, os
sys.path.insert(0, %r)
import numpy as np
from rimphony_amd import api, workload
ctx = api.Context(0)
kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_8", 192, start=1000000)
out, st, work = ctx.compute_batch(kind, s, th, params, 0xFF, want_status=True, want_work=True)
np.save(sys.argv[1], out); np.save(sys.argv[2], st); np.save(sys.argv[3], work)
print("shared" if ctx.shared_mode() else "exclusive")
''' % ROOT
    import tempfile
    with gpu_ctx.released():        # the children must own the GPU to use the cooperative tail (tests/conftest.py)
        with tempfile.TemporaryDirectory() as d:
            res = {}
            for name, env_extra in (("normal", {}), ("impatient", {"RIMPHONY_OWNER_WAIT_US": "1"})):
                env = dict(os.environ, **env_extra)
                o, s_, w_ = (os.path.join(d, name + x) for x in ("_o.npy", "_s.npy", "_w.npy"))
                r = subprocess.run([sys.executable, "-c", code, o, s_, w_], capture_output=True, text=True, env=env,
                                   timeout=600)
                assert r.returncode == 0, r.stderr[-2000:]
                assert "exclusive" in r.stdout
                res[name] = (np.load(o), np.load(s_), np.load(w_))
            assert same_bits(res["normal"][0], res["impatient"][0]).all()
            assert (res["normal"][1] == res["impatient"][1]).all()
            # work counters count what went into the stored value: an abandoned batch that is evaluated again by its
            # owner is booked once (the owner books a request when it reads the result)
            assert (res["normal"][2] == res["impatient"][2]).all()
