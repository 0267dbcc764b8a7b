"""GPU tests of the ends of the spline of a 2-D table set (rimphony_ctx_set_tables_2d_ends, rimphony_ctx_set_tables_2d_device_ends,
reached through the `ends` keyword of Context.set_tables_2d, set_tables_2d_grid and set_tables_2d_nodes): the host entry
installs the table oracle's set word for word, the device entry the host entry's; a fixture of two sets with not-a-knot ends
is reproduced bit for bit on the group kernel and one wave per coefficient; not-a-knot ends change what is computed; a
refused call leaves the previous set in place.  Every test runs under a time limit of its own."""
import contextlib
import ctypes
import faulthandler
import os
import sys

import numpy as np
import pytest

import tab2d_ends_bind as te

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL = -1
ST_NONFINITE, ST_NORM_FAIL = 16, 32
TAB = 4
NAK, NAT = te.NOT_A_KNOT, te.NATURAL


@contextlib.contextmanager
def time_limit(seconds):
    """Ends the process (with a traceback of every thread) if the body -- GPU work that may block inside the runtime,
    where no Python exception can reach -- is still running after `seconds`."""
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_rows(got, want):
    """coefficients: the same bits, or a NaN on both sides"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def first_difference(name, got, want):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    d = np.flatnonzero(got != want)
    if d.size:
        pytest.fail("%s: %d of %d words differ; first at %d: %r, expected %r" % (
            name, d.size, got.size, d[0], got.view(np.float64)[d[0]], want.view(np.float64)[d[0]]))


def to_device(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0").contiguous()


def install(ctx, form, gamma, mu, log_n, sin_k, ends, lo=te.GLO, hi=te.GHI):
    """through the form's Python entry: log_n a numpy array (the host entry) or a CUDA tensor (the device entry)"""
    if form == "uniform":
        ctx.set_tables_2d(lo, hi, log_n, sin_k, ends=ends)
    elif form == "grid":
        ctx.set_tables_2d_grid(gamma, log_n, sin_k, ends=ends)
    else:
        ctx.set_tables_2d_nodes(gamma, mu, log_n, sin_k, ends=ends)


def a_set(form, shape, prefactor, jitter):
    gamma, mu, g_at, mu_at = te.nodes_of(form, shape[1], shape[2])
    t = te.smooth_tables(shape, g_at, mu_at, seed=shape[1] + shape[2], jitter=jitter)
    return gamma, mu, t, (np.linspace(0.5, 2.5, shape[0]) if prefactor else None)


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


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "tabulated_2d_ends_det.npz"))


def fixture_install(ctx, fix, which, ends=te.FIXTURE_ENDS, device=False):
    """the fixture's set `which` as tab2d_ends_bind.fixture_set builds it, which must be what the fixture stores"""
    gamma, lo, hi, mu, tables, k = te.fixture_set(which)
    first_difference("the tables of set %d" % which, tables, fix["tables_%d" % which])
    if which == 1:
        first_difference("gamma", gamma, fix["gamma_1"])
        first_difference("mu", mu, fix["mu_1"])
    install(ctx, "uniform" if which == 0 else "nodes", gamma, mu, to_device(tables) if device else tables, k, ends, lo, hi)


def rows(ctx, f):
    return ctx.compute_batch(TAB, f["s"].copy(), f["theta"].copy(), [f["index"].copy()], 0xFF, want_status=True, want_work=True)


# ---- 1. the host install is the oracle's set ------------------------------------------------------------------------------
@pytest.mark.parametrize("prefactor", [False, True], ids=["plain", "sin_k"])
@pytest.mark.parametrize("form", te.FORMS)
def test_host_install_is_the_oracle_set_word_for_word(gpu_ctx, form, prefactor):
    """not-a-knot ends on both axes: everything but the normalisation words, which the oracle leaves at 0 and the device
    fills with a positive number"""
    shape = (3, 9, 11)
    gamma, mu, t, k = a_set(form, shape, prefactor, 0.0)
    assert te.set_tables(gamma, mu, t, k, (NAK, NAK), with_norm=False) == 0
    want = te.blob()
    with time_limit(60):
        install(gpu_ctx, form, gamma, mu, t, k, "not-a-knot")
        host = gpu_ctx.tables_blob()
    norm_at = te.norm_at(shape[0])
    print(form, prefactor, "normalisations", host[norm_at])
    assert host.size == want.size
    assert (want[norm_at] == 0.0).all() and np.isfinite(host[norm_at]).all() and (host[norm_at] > 0.0).all()
    assert (te.ends_words(host) == 3).all()
    rest = np.ones(host.size, dtype=bool)
    rest[norm_at] = False
    first_difference("host install against the oracle", host[rest], want[rest])


# ---- 2. the device install is the host install ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", te.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", te.FORMS)
def test_device_install_is_the_host_install_word_for_word(gpu_ctx, form, shape):
    """The same numbers from a CUDA tensor, read back: equal as uint64, normalisations included, with not-a-knot ends on both
    axes and with the mixed choice (natural, not-a-knot).  Every other shape carries a prefactor."""
    gamma, mu, t, k = a_set(form, shape, te.SHAPES.index(shape) % 2 == 1, 0.0)
    d = to_device(t)
    for ends in (("natural", "not-a-knot"), (NAK, NAK)):
        with time_limit(60):
            install(gpu_ctx, form, gamma, mu, t, k, ends)
            host = gpu_ctx.tables_blob()
            install(gpu_ctx, form, gamma, mu, d, k, ends)
            dev = gpu_ctx.tables_blob()
        assert np.isfinite(host[te.norm_at(shape[0])]).all(), host[te.norm_at(shape[0])]
        assert (te.ends_words(host) == (2 if ends[0] == "natural" else 3)).all()
        first_difference("device install against host install, ends %r" % (ends,), dev, host)
    # and the host install was the oracle's: the word-for-word agreement above is not two wrong sets agreeing
    assert te.set_tables(gamma, mu, t, k, (NAK, NAK), with_norm=False) == 0
    rest = np.ones(host.size, dtype=bool)
    rest[te.norm_at(shape[0])] = False
    first_difference("host install against the oracle", host[rest], te.blob()[rest])


def test_natural_ends_through_the_new_entries_install_the_old_sets(gpu_ctx):
    """ends="natural" goes through the two new C entries, ends=None through the form's own: the same set word for word, from
    a numpy array and from a tensor, for the three geometries with and without a prefactor"""
    shape = (3, 9, 11)
    for form in te.FORMS:
        for prefactor in (False, True):
            gamma, mu, t, k = a_set(form, shape, prefactor, 0.0)
            with time_limit(60):
                install(gpu_ctx, form, gamma, mu, t, k, None)
                old = gpu_ctx.tables_blob()
                install(gpu_ctx, form, gamma, mu, t, k, "natural")
                new_host = gpu_ctx.tables_blob()
                install(gpu_ctx, form, gamma, mu, to_device(t), k, "natural")
                new_dev = gpu_ctx.tables_blob()
            first_difference("%s %s: the host entry with natural ends" % (form, prefactor), new_host, old)
            first_difference("%s %s: the device entry with natural ends" % (form, prefactor), new_dev, old)


# ---- 3. the coefficients carry the oracle's bits ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_runs(gpu_ctx, fix):
    """both fixture sets on a context with RIMPHONY_TAB_GROUP=1 (host install) and on one with RIMPHONY_SYM_SOLO=1 (device
    install): the rows, the normalisations and calc_f"""
    res = {}
    with time_limit(600):
        gpu_ctx.shared_mode()
        ctxs = {"group": env_context(RIMPHONY_TAB_GROUP="1"), "solo": env_context(RIMPHONY_SYM_SOLO="1")}
        try:
            for which in (0, 1):
                for name, ctx in ctxs.items():
                    fixture_install(ctx, fix, which, device=name == "solo")
                    res[which, name] = rows(ctx, fix)
                    res[which, name, "norm"] = ctx.norm_batch(TAB, [np.arange(2, dtype=np.float64)])
                    res[which, name, "f"] = [ctx.calc_f_batch(TAB, [float(t)], fix["f_gamma"].copy(), fix["f_mu"].copy()) for t in (0, 1)]
        finally:
            for c in ctxs.values():
                c.close()
    return res


@pytest.mark.parametrize("kernel", ["group", "solo"])
@pytest.mark.parametrize("which", [0, 1], ids=["64x16 uniform", "40x12 nodes sin_k"])
def test_fixture_bits(fixture_runs, fix, which, kernel):
    """tests/golden/tabulated_2d_ends_det.npz: all eight slots of the twelve rows, their status words and sample counts, the
    normalisations and calc_f, in lock-step on the group kernel and one wave per coefficient"""
    out, st, work = fixture_runs[which, kernel]
    want = fix["values"][which]
    assert np.isfinite(want).sum() >= 64
    bad = np.argwhere(~same_rows(out, want))
    assert bad.size == 0, (bad[:8], out[tuple(bad[0])], want[tuple(bad[0])])
    assert (work.astype(np.uint64) == fix["work"][which]).all()
    assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which]).all()
    first_difference("the normalisations", fixture_runs[which, kernel, "norm"], fix["norms"][which])
    for t in (0, 1):
        for i, name in enumerate(("f", "df/dgamma", "df/dmu")):
            first_difference("%s of table %d" % (name, t), fixture_runs[which, kernel, "f"][t][i], fix["f_values"][which][t][i])


# ---- 4. the choice changes what is computed -----------------------------------------------------------------------------------
def test_not_a_knot_ends_change_the_coefficients(gpu_ctx, fix, fixture_runs):
    """set 0 with natural ends: at least one slot of every row differs from the fixture's -- an entry that ignored its
    argument would reproduce it"""
    with time_limit(300):
        fixture_install(gpu_ctx, fix, 0, ends="natural")
        assert (te.ends_words(gpu_ctx.tables_blob()) == 0).all()
        out, st, work = rows(gpu_ctx, fix)
    want = fix["values"][0]
    differ = ~same_rows(out, want) & np.isfinite(out) & np.isfinite(want)
    assert differ.any(axis=1).all(), differ.any(axis=1)


# ---- 5. a refusal keeps the previous set --------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_set_in_place(gpu_ctx, fix):
    """A bad end through both C entries and a non-finite value in the tensor: RIMPHONY_EINVAL each, and the set installed
    before is there to the word.  (No case hands the device entry a host pointer.)"""
    import torch
    gamma, lo, hi, mu, t, k = te.fixture_set(1)
    nt, nn, nmu = t.shape
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)
    t = np.ascontiguousarray(t)
    good = to_device(t)
    nan = good.clone()
    nan.view(-1)[t.size // 3] = float("nan")
    lib, h = gpu_ctx.lib, gpu_ctx.handle

    def host_entry(eg, em):
        return lib.rimphony_ctx_set_tables_2d_ends(h, nt, nn, ptr(gamma), 1.0, 2.0, nmu, ptr(mu), ptr(t), ptr(k), eg, em)

    def device_entry(d, eg, em):
        return lib.rimphony_ctx_set_tables_2d_device_ends(h, nt, nn, ptr(gamma), 1.0, 2.0, nmu, ptr(mu), ctypes.c_void_p(d.data_ptr()),
                                                          ptr(k), eg, em, gpu_ctx._stream())

    with time_limit(120):
        fixture_install(gpu_ctx, fix, 1)
        before = gpu_ctx.tables_blob()
        torch.cuda.synchronize()
        for eg, em in ((-1, 0), (0, 2), (7, 1), (1, 7), (2, 2)):
            assert host_entry(eg, em) == EINVAL, (eg, em)
            first_difference("the set after the host entry with ends %r" % ((eg, em),), gpu_ctx.tables_blob(), before)
            assert device_entry(good, eg, em) == EINVAL, (eg, em)
            first_difference("the set after the device entry with ends %r" % ((eg, em),), gpu_ctx.tables_blob(), before)
        assert device_entry(nan, NAK, NAK) == EINVAL
        first_difference("the set after a NaN in the tensor", gpu_ctx.tables_blob(), before)
        for bad in ("clamped", (0, 1, 1), 3, (True, 0), 1.0):
            with pytest.raises(ValueError):
                gpu_ctx.set_tables_2d_nodes(gamma, mu, t, k, ends=bad)
        first_difference("the set after what Python refuses", gpu_ctx.tables_blob(), before)
        assert device_entry(good, NAK, NAK) == 0 and host_entry(NAK, NAK) == 0     # the same calls, sound
        first_difference("the sound calls", gpu_ctx.tables_blob(), before)
