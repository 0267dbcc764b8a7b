"""GPU tests of the Faraday kernels on LONG outer quadratures, against the committed bits of the deterministic CPU oracle
(tests/golden/faraday_long_det.npz, tools/make_faraday_long_fixture.py).  What the kernels do changes with the length of
the outer subinterval list -- 48: rounds (pitchy-kappa); 64: the list leaves LDS; limit / 2 + 2 = 2050: GSL's qpsrt no
longer keeps its list fully sorted, the kernels go on picking by argmax; 4096: the quadrature gives up -- and the fixture's
rows reach every one of those classes.  Every comparison is bit for bit: values with the NaN pattern, the per-coefficient
work column against the oracle's integrand samples, the launch's sample count, and the status words: equal to the
oracle's (the fixture's status column), and by the rule NaN <=> NONFINITE set, finite <=> 0, ended at 4096 => OUTER_FAIL set.

The 'mid' rows (seconds of one CPU core) run with all eight slots in the session's context, whatever its mode; the 'limit'
rows (a quarter of a million inner integrals in one chain) only on a context that owns the device, where the cooperative
tail spreads a batch over the grid: one child process per setting, one after the other, every launch under a time limit
of its own.  A child that fails or is ended at its limit ends the sequence: nothing further is started."""
import contextlib
import faulthandler
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import faraday_long as fl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OUTER_FAIL, ST_NONFINITE, ST_NOT_COMPUTED = 2, 16, 64
MASK = {"mid": 0xFF, "limit": 0xC0}
LAUNCH_LIMIT = {"mid": 120, "limit": 200}          # seconds, per launch (faulthandler ends the process)
CHILD_TIMEOUT = 300                                 # seconds, per child (the parent's subprocess timeout)
# the settings of the exclusive legs (read when a context is created) and the classes each runs: without helpers one wave
# works through a 'limit' row's 255 k inner integrals alone (about 40 s, profiles/r4_launch_tails.txt) -- 'mid' rows only
LEGS = (("default", {}, ("mid", "limit")),
        ("rounds_off", {"RIMPHONY_ROUNDS": "0"}, ("mid", "limit")),
        ("pair", {"RIMPHONY_FARADAY_GROUP": "1"}, ("mid", "limit")),         # rho_Q and rho_V in lock-step, heyvaerts_group.h
        ("no_assist", {"RIMPHONY_NO_ASSIST": "1"}, ("mid",)))
KNOBS = sorted({k for _, env, _ in LEGS for k in env})


@contextlib.contextmanager
def time_limit(seconds):
    """Ends the process (with a traceback of every thread) if the body -- GPU work that may block inside the runtime,
    where no Python exception can reach -- is still running after `seconds`."""
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def launch(ctx, cfg, cls):
    """The fixture's rows of class `cls` of a config in one call: dict of out, st, work and the launch's counters (None when
    the config has no such row)."""
    idx, s, th, params = fl.rows_of(cfg, [cls])
    if not len(idx):
        return None
    with time_limit(LAUNCH_LIMIT[cls]):
        t0 = time.perf_counter()
        out, st, work = ctx.compute_batch(fl.CONFIGS.index(cfg), s, th, params, MASK[cls], want_status=True, want_work=True)
        seconds = time.perf_counter() - t0
        w, tail = ctx.last_work(), ctx.last_tail()
    return {"out": out, "st": st, "work": work.astype(np.uint64), "seconds": seconds,
            "counters": np.array([w["samples"], w["faraday_samples"], w["faraday_inner_qags"], tail["faraday_heaviest_batches"],
                                  tail["faraday_heaviest_row"]], dtype=np.uint64)}


def counters(got):
    return dict(zip(("samples", "faraday_samples", "faraday_inner_qags", "faraday_heaviest_batches", "faraday_heaviest_row"),
                    (int(x) for x in got["counters"])))


def check_launch(cfg, cls, got, where):
    """A launch against the fixture: bits, work columns, sample counts, status words."""
    f = fl.load()
    idx = fl.rows_of(cfg, [cls])[0]
    sel = [k for k in range(8) if MASK[cls] & (1 << k)]
    uns = [k for k in range(8) if k not in sel]
    out, st, work, c = got["out"], got["st"], got["work"], counters(got)
    want, want_work = f["values"][idx], f["integrand_evals"][idx]
    ok = same_bits(out[:, sel], want[:, sel])
    print(where, cfg, cls, "%.2f s" % got["seconds"], c, "| differing (row, slot):",
          [(int(f["row"][idx[i]]), sel[j]) for i, j in np.argwhere(~ok)], "status", st[:, 6:].tolist())
    assert ok.all(), [(int(f["row"][idx[i]]), sel[j], out[i, sel[j]], want[i, sel[j]]) for i, j in np.argwhere(~ok)]
    assert np.isnan(out[:, uns]).all() and (st[:, uns] == (ST_NONFINITE | ST_NOT_COMPUTED)).all() and (work[:, uns] == 0).all()
    assert (work[:, sel] == want_work[:, sel]).all(), (work[:, sel] - want_work[:, sel]).tolist()
    assert c["faraday_samples"] == int(want_work[:, 6:].sum())
    if 0 in sel:
        assert c["samples"] == int(want_work[:, :6].sum())
    nan = np.isnan(out[:, sel])
    assert ((st[:, sel] & ST_NONFINITE) != 0)[nan].all(), st[:, sel].tolist()
    assert (st[:, sel][~nan] == 0).all(), st[:, sel].tolist()
    # the FULL word of every selected slot is the oracle's (the fixture's status column: rimo_compute_dimensionless_st)
    want_st = f["status"][idx][:, sel].astype(np.int64)
    assert (st[:, sel] == want_st).all(), (st[:, sel].tolist(), want_st.tolist())
    at_limit = f["max_outer_size"][idx].astype(np.int64) == fl.LIMIT                    # [rows][2]: the Faraday pair
    assert ((st[:, 6:] & ST_OUTER_FAIL) != 0)[at_limit].all(), st[:, 6:].tolist()
    if cls == "limit":
        assert at_limit.any() and (~at_limit[:, 0]).any()          # one row runs to the limit, one converges before it


@pytest.mark.parametrize("cfg", fl.CONFIGS)
def test_mid_rows_in_the_session_context(gpu_ctx, cfg):
    """The 'mid' rows of a kind, all eight slots, one call in the session's context (shared or exclusive, as it happens to
    be): lists of exactly 48, just past 64, up to 199 entries, long marching loops, and a short control."""
    check_launch(cfg, "mid", launch(gpu_ctx, cfg, "mid"), "session (%s)" % ("shared" if gpu_ctx.shared_mode() else "exclusive"))


def child_main(out_dir, classes):
    """One exclusive leg: a context that owns the device (its settings come with the environment) computes the rows of the
    given classes of every kind, one launch per (kind, class)."""
    from rimphony_amd import api
    t0 = time.perf_counter()
    with time_limit(120):
        ctx = api.Context(0)
    assert not ctx.shared_mode()
    print("exclusive", flush=True)
    times = {}
    for cfg in fl.CONFIGS:
        for cls in classes.split(","):
            got = launch(ctx, cfg, cls)
            if got is not None:
                times[cfg + " " + cls] = round(got.pop("seconds"), 3)
                np.savez(os.path.join(out_dir, "%s_%s.npz" % (cfg, cls)), **got)
    ctx.close()
    times["all"] = round(time.perf_counter() - t0, 3)
    print("times " + json.dumps(times), flush=True)


@pytest.fixture(scope="module")
def legs(gpu_ctx):
    """{leg: {(cfg, cls): launch dict} or an error string}: the exclusive children, one after the other.  After a child that
    did not end well nothing further is started (whatever it was, it is not run again here)."""
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_faraday_long as m; m.child_main(sys.argv[1], sys.argv[2])" % (
        ROOT, os.path.join(ROOT, "tests"))
    base = {k: v for k, v in os.environ.items() if k not in KNOBS}
    res, failed = {}, None
    with gpu_ctx.released():
        for name, env, classes in LEGS:
            if failed:
                res[name] = "not started: the leg '%s' did not end well" % failed
                continue
            with tempfile.TemporaryDirectory() as d:
                t0 = time.perf_counter()
                try:
                    r = subprocess.run([sys.executable, "-c", code, d, ",".join(classes)], capture_output=True, text=True,
                                       env=dict(base, **env), timeout=CHILD_TIMEOUT)
                except subprocess.TimeoutExpired as e:
                    failed, res[name] = name, "ended at the parent's limit of %d s: %s" % (CHILD_TIMEOUT, str(e.stderr)[-2000:])
                    continue
                wall = time.perf_counter() - t0
                if r.returncode != 0 or "exclusive" not in r.stdout:
                    failed, res[name] = name, "exit status %d: %s" % (r.returncode, r.stderr[-3000:])
                    continue
                times = [l[6:] for l in r.stdout.splitlines() if l.startswith("times ")]
                print("leg %s: child wall time %.1f s; launches %s" % (name, wall, times[0] if times else "?"))
                res[name] = {}
                for cfg in fl.CONFIGS:
                    for cls in classes:
                        p = os.path.join(d, "%s_%s.npz" % (cfg, cls))
                        if os.path.exists(p):
                            with np.load(p) as z:
                                res[name][cfg, cls] = dict({k: z[k] for k in z.files}, seconds=json.loads(times[0])[cfg + " " + cls])
    return res


def leg_of(legs, name):
    assert isinstance(legs[name], dict), legs[name]
    return legs[name]


@pytest.mark.parametrize("name", [l[0] for l in LEGS])
def test_exclusive_leg_carries_the_fixture(legs, name):
    """Every launch of a leg -- the default knobs, RIMPHONY_ROUNDS=0, RIMPHONY_FARADAY_GROUP=1 (the lock-step pair kernel,
    whose outer lists live in global memory from the first entry: until this test it had seen lists of up to 31 entries)
    and RIMPHONY_NO_ASSIST=1 -- carries the fixture's bits, work columns, sample counts and status words, through the
    4096-entry rows where the leg runs them."""
    got = leg_of(legs, name)
    classes = dict((l[0], l[2]) for l in LEGS)[name]
    want = {(cfg, cls) for cfg in fl.CONFIGS for cls in classes if len(fl.rows_of(cfg, [cls])[0])}
    assert set(got) == want
    for cfg, cls in sorted(got):
        check_launch(cfg, cls, got[cfg, cls], "leg " + name)


def test_rounds_shorten_the_chain_and_change_nothing_else(legs):
    """Pitchy-kappa, the kind whose kernel has rounds, with and without them (RIMPHONY_ROUNDS=0) on the two 'limit' rows:
    the heaviest task's chain of batches is strictly SHORTER with rounds (a bisection whose children's sums were filed by an
    earlier round is booked without a batch), more inner integrals are evaluated (the children of intervals that were filed
    and never picked), and the launch's sample count is the oracle's either way (what nobody asked for comes off it).  The
    heaviest row without rounds -- where a chain's length is the quadratures' own: one batch per bisection -- is one whose
    list ran to 4096; with rounds the length of a chain depends on which batches went over the board, so the row is
    printed, not asserted."""
    f = fl.load()
    on, off = counters(leg_of(legs, "default")["cfg5_pitchykappa_8", "limit"]), counters(leg_of(legs, "rounds_off")["cfg5_pitchykappa_8", "limit"])
    print("pitchy-kappa 'limit' rows: rounds on", on, "rounds off", off)
    idx = fl.rows_of("cfg5_pitchykappa_8", ["limit"])[0]
    assert on["faraday_heaviest_batches"] < off["faraday_heaviest_batches"]
    assert on["faraday_inner_qags"] > off["faraday_inner_qags"]
    assert on["faraday_samples"] == off["faraday_samples"] == int(f["integrand_evals"][idx, 6:].sum())
    assert f["max_outer_size"][idx[off["faraday_heaviest_row"]]].max() == fl.LIMIT
    assert off["faraday_heaviest_batches"] > fl.LIMIT
    m_on, m_off = counters(leg_of(legs, "default")["cfg5_pitchykappa_8", "mid"]), counters(leg_of(legs, "rounds_off")["cfg5_pitchykappa_8", "mid"])
    print("pitchy-kappa 'mid' rows: rounds on", m_on, "rounds off", m_off)
    assert m_on["faraday_samples"] == m_off["faraday_samples"]


@pytest.mark.parametrize("cfg", [c for c in fl.CONFIGS if c != "cfg5_pitchykappa_8"])
def test_kernels_without_rounds_count_the_same(legs, cfg):
    """The other three kinds' kernels are built without rounds: RIMPHONY_ROUNDS changes none of their counters."""
    a, b = leg_of(legs, "default"), leg_of(legs, "rounds_off")
    keys = [k for k in a if k[0] == cfg]
    assert keys and all(k in b for k in keys)
    for k in keys:
        assert counters(a[k]) == counters(b[k]), k


def test_inner_integrals_are_the_oracles_without_rounds(legs):
    """rimphony_last_work's faraday_inner_qags against the oracle's inner_qag_calls, summed over a launch's rows and the
    Faraday pair, with RIMPHONY_ROUNDS=0.  The two count the same events: the oracle counts every call of its inner QAG
    (rimo_heyvaerts.c inner_qag: the 31 / 62 abscissae of an outer rule application and the four of a derivative probe; an
    outer abscissa whose sigma range is empty returns 0 before it), the kernels count every completed inner quadrature in
    wave_qag_pair (wave_qag.h; hey_eval_pair skips the empty ranges before it), whichever wave ran it -- and without
    rounds nothing is evaluated that qag.c did not ask for."""
    f = fl.load()
    got = leg_of(legs, "rounds_off")
    for cfg, cls in sorted(got):
        idx = fl.rows_of(cfg, [cls])[0]
        c = counters(got[cfg, cls])
        print(cfg, cls, "faraday_inner_qags", c["faraday_inner_qags"], "oracle", int(f["inner_qag_calls"][idx].sum()))
        assert c["faraday_inner_qags"] == int(f["inner_qag_calls"][idx].sum()), (cfg, cls)
