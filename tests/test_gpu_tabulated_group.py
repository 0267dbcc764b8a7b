"""GPU tests of the tabulated distribution's Symphony slots on the group kernel (rimphony_tab_group.hip; RIMPHONY_TAB_GROUP):
the coefficients of a point in lock-step carry the bits, the status words and the per-coefficient sample counts of one wave
per coefficient and of the CPU oracles' committed fixtures, for every form of a table set, for partial groups and through
the cooperative tail; what changes is the number of executed passes.  Every launch runs under a time limit of its own."""
import contextlib
import faulthandler
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import tab2d_bind as t2
import tab_pitch_bind as tp
import tab_pitchy_bind as ty

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TAB = 4
ST_NONFINITE, ST_NOT_COMPUTED = 16, 64
ROWS = 24
FORMS = ("isotropic", "pitch", "2-D", "sin^k")

# Where the Symphony slots of a form run when RIMPHONY_TAB_GROUP is not set: the mirror of RIM_TAB_GROUP_DEFAULT in
# rimphony_amd/csrc/rimphony_hip.hip (True: the group kernel), which profiles/tabulated_group_times.txt decides.
DEFAULT_GROUP = {"isotropic": True, "pitch": True, "2-D": True, "sin^k": True}

# the masks of the partial groups, and whether SymGroupF::shared evaluates both member kinds of a group at once
# (gamma_integrand_f_terms) or a single one (gamma_integrand_f_term)
MASKS = {0x15: "emission only", 0x2A: "absorption only", 0x06: "one of each, in the I/Q group", 0x10: "a single-member V group",
         0x20: "a single-member V group", 0x3F: "everything"}
PARTIAL_FORMS = ("pitch", "2-D")
# (s, theta) rows at which gamma sin xi is rounding noise: theta = pi/2 exactly (cos theta = 6.1e-17) and just beside it
HOSTILE = (np.array([10.0, 10.0]), np.array([math.pi / 2, math.pi / 2 - 1e-12]))


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


def env_context(**env):
    """A context created with the given environment (the knobs are read when a context is created)."""
    from rimphony_amd import api
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def form_case(form):
    """(install(ctx), s, theta, index, values [24][6], work [24][6]) of a form: the committed fixture's rows (the isotropic
    one's first 24) and what the CPU oracle computed for them; install puts the fixture's set into a context."""
    if form == "isotropic":
        f = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))
        glo, ghi, tables = float(f["gamma_lo"]), float(f["gamma_hi"]), f["tables"]
        install = lambda ctx: ctx.set_tables(glo, ghi, tables)
        values, work = f["values"], f["work"]
    elif form == "pitch":
        f = np.load(os.path.join(GOLDEN, "tabulated_pitch_det.npz"))
        glo, ghi, tables, G = float(f["gamma_lo"]), float(f["gamma_hi"]), f["tables"], tp.edge_pitch(int(f["n_mu"][0]))
        install = lambda ctx: ctx.set_tables(glo, ghi, tables, G)
        values, work = f["values"][0], f["work"][0]
    elif form == "2-D":
        f = np.load(os.path.join(GOLDEN, "tabulated_2d_det.npz"))
        n_nodes, n_mu = (int(x) for x in f["geometry"][0])
        glo, ghi, tables = float(f["gamma_lo"]), float(f["gamma_hi"]), t2.edge_tables_2d(n_nodes, n_mu, f["cols_0"])
        install = lambda ctx: ctx.set_tables_2d(glo, ghi, tables)
        values, work = f["values"][0], f["work"][0]
    else:
        f = np.load(os.path.join(GOLDEN, "tabulated_pitchy_det.npz"))
        lo, hi, t, g, k = ty.fixture_set(1)            # set B: the one with pitch rows
        install = lambda ctx: ctx.set_tables(lo, hi, t, g, sin_k=k)
        values, work = f["values"][1], f["work"][1]
    return (install, f["s"][:ROWS].copy(), f["theta"][:ROWS].copy(), f["index"][:ROWS].copy(),
            values[:ROWS, :6].copy(), work[:ROWS, :6].astype(np.uint64))


def run(ctx, case, mask):
    _, s, th, index, _, _ = case
    out, st, work = ctx.compute_batch(TAB, s, th, [index], mask, want_status=True, want_work=True)
    return out, st, work.astype(np.uint64), ctx.last_work()


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """Every launch of tests 1 to 3, once: three contexts -- RIMPHONY_TAB_GROUP=1, RIMPHONY_SYM_SOLO=1, no knob -- next to the
    session's (which is touched first: the three run in shared mode whatever test comes first, so that their pass counts
    compare), each form's rows with mask 0x3F on all three and the partial masks on the group context."""
    res = {}
    with time_limit(600):
        gpu_ctx.shared_mode()
        ctxs = {"group": env_context(RIMPHONY_TAB_GROUP="1"), "solo": env_context(RIMPHONY_SYM_SOLO="1"), "default": env_context()}
        try:
            assert all(c.shared_mode() for c in ctxs.values())
            for form in FORMS:
                case = form_case(form)
                for name, ctx in ctxs.items():
                    case[0](ctx)
                    res[form, name, 0x3F] = run(ctx, case, 0x3F)
                for name in ("group", "solo"):
                    out, st, work = ctxs[name].compute_batch(TAB, HOSTILE[0], HOSTILE[1], [np.zeros(len(HOSTILE[0]))], 0x3F,
                                                             want_status=True, want_work=True)
                    res[form, name, "hostile"] = (out, st, work.astype(np.uint64))
                if form in PARTIAL_FORMS:
                    for mask in MASKS:
                        if mask != 0x3F:
                            res[form, "group", mask] = run(ctxs["group"], case, mask)
        finally:
            for c in ctxs.values():
                c.close()
    return res


@pytest.mark.parametrize("form", FORMS)
def test_group_against_solo(runs, form):
    """The six Symphony slots of the fixture's rows in lock-step and one wave per coefficient: the same values, status words
    and work table, which are the oracle's; the same number of samples; strictly fewer executed passes with the group (an
    executed rule application serves several members) -- on a build without the group kernels of the kind the knob does
    nothing and the two counts are equal."""
    _, _, _, _, want, want_work = form_case(form)
    g, s = runs[form, "group", 0x3F], runs[form, "solo", 0x3F]
    print(form, "samples", g[3]["samples"], "passes: group", g[3]["passes"], "solo", s[3]["passes"])
    assert same_bits(g[0], s[0]).all()
    assert (g[1] == s[1]).all()
    assert (g[2] == s[2]).all()
    for got in (g, s):
        assert same_bits(got[0][:, :6], want).all()
        assert (got[2][:, :6] == want_work).all()
    assert g[3]["samples"] == s[3]["samples"] == int(want_work.sum())
    assert g[3]["passes"] < s[3]["passes"]


@pytest.mark.parametrize("form", FORMS)
def test_noise_above_the_order_is_counted_as_one_wave_per_coefficient_counts_it(runs, form):
    """theta = pi/2 exactly and a rounding beside it, table 0 of every form: the argument of the Bessel pair is rounding noise
    far above the order, where sym_bessel_pair has no value and the reference's complete functions have one.  One wave per
    coefficient evaluates such a request again through the complete functions (test_gpu_tabulated.py::
    test_hostile_s_and_theta holds it to the oracle's 1426 / 2728 samples on the isotropic form); the group path of the kind
    does the same per entry: the same values, status words and sample counts."""
    g, s = runs[form, "group", "hostile"], runs[form, "solo", "hostile"]
    print(form, "work", g[2][:, :6].tolist(), "NaN", np.isnan(g[0][:, :6]).sum(axis=1))
    assert same_bits(g[0], s[0]).all()
    assert (g[1] == s[1]).all()
    assert (g[2] == s[2]).all(), (g[2], s[2])
    assert (g[2][:, :6] > 0).all()


@pytest.mark.parametrize("mask", [m for m in MASKS if m != 0x3F], ids=lambda m: "0x%02X" % m)
@pytest.mark.parametrize("form", PARTIAL_FORMS)
def test_partial_groups(runs, form, mask):
    """A group with some of its members: a selected column carries the bits, the status and the sample counts it has when
    everything is selected, an unselected one is NaN, not computed, and no work."""
    full, part = runs[form, "group", 0x3F], runs[form, "group", mask]
    for col in range(8):
        if mask & (1 << col):
            assert same_bits(part[0][:, col], full[0][:, col]).all(), col
            assert (part[1][:, col] == full[1][:, col]).all(), col
            assert (part[2][:, col] == full[2][:, col]).all(), col
            assert part[2][:, col].sum() > 0
    for got, m in ((full, 0x3F), (part, mask)):
        for col in range(8):
            if not m & (1 << col):
                assert np.isnan(got[0][:, col]).all(), col
                assert (got[1][:, col] == (ST_NONFINITE | ST_NOT_COMPUTED)).all(), col
                assert (got[2][:, col] == 0).all(), col
    assert part[3]["samples"] == int(part[2].sum())


@pytest.mark.parametrize("form", FORMS)
def test_default_routing(runs, form):
    """Without the knob a form runs where DEFAULT_GROUP says: the executed passes are those of the context that was told."""
    told = runs[form, "group" if DEFAULT_GROUP[form] else "solo", 0x3F]
    other = runs[form, "solo" if DEFAULT_GROUP[form] else "group", 0x3F]
    got = runs[form, "default", 0x3F]
    assert got[3]["passes"] == told[3]["passes"] and got[3]["passes"] != other[3]["passes"]
    assert same_bits(got[0], told[0]).all() and (got[1] == told[1]).all() and (got[2] == told[2]).all()


def child_main(out_dir):
    """Test 4's child: owns the device; every form's rows once whole and once row by row on the group kernel."""
    from rimphony_amd import api
    ctx = api.Context(0)
    print("shared" if ctx.shared_mode() else "exclusive", flush=True)
    for k, form in enumerate(FORMS):
        case = form_case(form)
        _, s, th, index, _, _ = case
        with time_limit(240):
            case[0](ctx)
            whole = run(ctx, case, 0x3F)
            rows = [ctx.compute_batch(TAB, s[i:i + 1], th[i:i + 1], [index[i:i + 1]], 0x3F, want_status=True, want_work=True)
                    for i in range(ROWS)]
        np.savez(os.path.join(out_dir, "form%d.npz" % k), whole_out=whole[0], whole_work=whole[2],
                 rows_out=np.concatenate([r[0] for r in rows]), rows_work=np.concatenate([r[2] for r in rows]).astype(np.uint64))
    ctx.close()


def test_cooperative_tail_on_the_group_path(gpu_ctx):
    """Twenty-four rows, and one row, on a grid of thousands of waves: every launch is in its tail from the first cycle, so
    nearly every round is published and evaluated entry by entry by helpers.  One child process that owns the device (the
    tail needs that) computes the rows of every form whole and row by row with RIMPHONY_TAB_GROUP=1: the oracle's bits
    and sample counts both ways."""
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_tabulated_group as m; m.child_main(sys.argv[1])" % (
        ROOT, os.path.join(ROOT, "tests"))
    with gpu_ctx.released():
        with tempfile.TemporaryDirectory() as d:
            r = subprocess.run([sys.executable, "-c", code, d], capture_output=True, text=True,
                               env=dict(os.environ, RIMPHONY_TAB_GROUP="1"), timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            assert "exclusive" in r.stdout
            got = [dict(np.load(os.path.join(d, "form%d.npz" % k))) for k in range(len(FORMS))]
    for form, g in zip(FORMS, got):
        _, _, _, _, want, want_work = form_case(form)
        for how in ("whole", "rows"):
            assert same_bits(g[how + "_out"][:, :6], want).all(), (form, how)
            assert (g[how + "_work"][:, :6] == want_work).all(), (form, how)
