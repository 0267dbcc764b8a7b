"""GPU tests of a 2-D table set installed from device memory (rimphony_ctx_set_tables_2d_device, reached through
Context.set_tables_2d, set_tables_2d_grid and set_tables_2d_nodes with a CUDA tensor): the set on the device is, word for
word, the set the form's host entry installs from the same numbers -- read back with Context.tables_blob() and compared as
uint64, normalisations included -- and the host-installed set is the form's table oracle's, so a read-back that returned
nonsense could not pass by agreeing with itself.  A fixture set installed from a tensor computes the fixture's recorded
bits; what the entry refuses leaves the previous set in place; a change of form through the entry leaves no state.  Every
test runs under a time limit of its own."""
import contextlib
import ctypes
import faulthandler
import os
import sys

import numpy as np
import pytest

import tab_install_inputs as ti

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL = -1
ST_NONFINITE, ST_NORM_FAIL = 16, 32
TAB = 4
SHAPES = [(1, 8, 8), (3, 9, 11), (5, 70, 13), (1, 300, 8), (1, 8, 1024)]
HDR, T_HDR, T_NORM = 8, 8, 3        # dev_symphony.h: TAB_HDR_DOUBLES, TAB_2D_HDR, TAB_2D_NORM


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


def install(ctx, form, gamma, mu, log_n, sin_k):
    """through the form's Python entry: log_n a numpy array (the host entry) or a CUDA tensor (the device entry)"""
    if form == "uniform":
        ctx.set_tables_2d(ti.GLO, ti.GHI, log_n, sin_k)
    elif form == "grid":
        ctx.set_tables_2d_grid(gamma, log_n, sin_k)
    else:
        ctx.set_tables_2d_nodes(gamma, mu, log_n, sin_k)


def oracle_blob(form, gamma, mu, log_n, sin_k):
    """the set as the form's table oracle lays it out, normalisations 0"""
    if form == "nodes":
        import tab2d_nodes_bind as tn
        assert tn.set_tables(gamma, mu, log_n, sin_k, with_norm=False) == 0
        return tn.blob()
    if sin_k is not None:
        import tab2d_pitchy_bind as tp
        assert tp.set_tables((ti.GLO, ti.GHI) if form == "uniform" else gamma, log_n, sin_k, with_norm=False) == 0
        return tp.blob()
    if form == "uniform":
        import tab2d_bind as t2
        assert t2.set_tables(ti.GLO, ti.GHI, log_n, with_norm=False) == 0
        return t2.blob()
    import tab2d_grid_bind as tq
    assert tq.set_tables(gamma, log_n, with_norm=False) == 0
    return tq.blob()


def raw_device_set(ctx, nt, nn, gamma, glo, ghi, nmu, mu, d_ptr, sin_k=None):
    """the C entry as a C caller reaches it, on the current stream -> its return code"""
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
    return ctx.lib.rimphony_ctx_set_tables_2d_device(ctx.handle, nt, nn, ptr(gamma), glo, ghi, nmu, ptr(mu),
                                                     None if d_ptr is None else ctypes.c_void_p(d_ptr), ptr(sin_k), ctx._stream())


@pytest.fixture(scope="module")
def fix():
    return np.load(os.path.join(GOLDEN, "tabulated_2d_nodes_det.npz"))


def fixture_set(fix, which):
    if which == 0:
        return fix["gamma_p"], fix["mu_p"], fix["tables_p"], None
    return fix["gamma_k"], fix["mu_k"], fix["tables_k"], fix["k_k"]


def rows(ctx, f, n=4):
    return ctx.compute_batch(TAB, f["s"][:n].copy(), f["theta"][:n].copy(), [f["index"][:n].copy()], 0xFF, want_status=True,
                             want_work=True)


# ---- 1. word for word -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("prefactor", [False, True], ids=["plain", "sin_k"])
@pytest.mark.parametrize("form", ["uniform", "grid", "nodes"])
@pytest.mark.parametrize("content", ["jittered", "smooth"])
def test_device_install_is_the_host_install_word_for_word(gpu_ctx, content, form, prefactor, shape):
    """Host install, read back; the same numbers from a CUDA tensor, read back: equal as uint64, normalisation words
    included.  Everything but the normalisation words of the host-installed set equals the form's table oracle's blob.
    The content is a smooth surface with a seeded jitter of 2 % on every value -- on graded nodes, with steps a millionth of
    their neighbours, its spline swings beyond what exp can hold and the normalisation of such a table is a NaN, in both
    installs -- and once more the surface itself, whose normalisations are numbers on every node set: equal numbers say that
    the normalisation kernel ran behind the last sweep."""
    rng = np.random.default_rng(20261020 + 11 * SHAPES.index(shape))
    gamma, mu, g_at, mu_at = ti.nodes_of(form, shape, rng)
    log_n = ti.smooth(shape, g_at, mu_at, rng, jitter=0.02 if content == "jittered" else 0.0)
    sin_k = np.linspace(0.5, 2.5, shape[0]) if prefactor else None
    want = oracle_blob(form, gamma, mu, log_n, sin_k)
    with time_limit(60):
        install(gpu_ctx, form, gamma, mu, log_n, sin_k)
        host = gpu_ctx.tables_blob()
        install(gpu_ctx, form, gamma, mu, to_device(log_n), sin_k)
        dev = gpu_ctx.tables_blob()
    norm_at = HDR + T_HDR * np.arange(shape[0]) + T_NORM
    print(content, form, shape, "normalisations", host[norm_at])
    assert host.size == want.size and dev.size == want.size
    assert (want[norm_at] == 0.0).all() and (host[norm_at] != 0.0).all()        # the device filled them: a number or a NaN
    if content == "smooth":
        assert np.isfinite(host[norm_at]).all() and (host[norm_at] > 0.0).all()
    rest = np.ones(host.size, dtype=bool)
    rest[norm_at] = False
    first_difference("host install against the oracle", host[rest], want[rest])
    first_difference("device install against host install", dev, host)


# ---- 2. a fixture set from a tensor ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["P: plain", "K: k 0.5 2.5"])
def test_fixture_set_from_a_tensor_computes_the_recorded_bits(gpu_ctx, fix, which):
    """tests/golden/tabulated_2d_nodes_det.npz: the coefficients, sample counts and status words of the first four recorded
    rows, from a set that the library only ever saw as a tensor"""
    gamma, mu, t, k = fixture_set(fix, which)
    with time_limit(120):
        gpu_ctx.set_tables_2d_nodes(gamma, mu, to_device(t), k)
        out, st, work = rows(gpu_ctx, fix)
    assert np.isfinite(fix["values"][which][:4]).any()
    assert same_rows(out, fix["values"][which][:4]).all(), (out, fix["values"][which][:4])
    assert (work.astype(np.uint64) == fix["work"][which][:4]).all()
    assert ((st & (ST_NONFINITE | ST_NORM_FAIL)) == fix["status"][which][:4]).all()


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_set_in_place(gpu_ctx, fix):
    """A NaN in the last word of the last table, a +inf in the middle, a null pointer, mu without gamma: RIMPHONY_EINVAL each,
    and after each the set installed before is there to the word and computes its bits.  (No case hands the entry a host
    pointer: the pointer check exists to refuse that, and a test of it would fault the device the day the check breaks.)"""
    import torch
    gamma, mu, t, k = fixture_set(fix, 0)
    nt, nn, nmu = t.shape
    good = to_device(t)
    last_nan, mid_inf = good.clone(), good.clone()
    last_nan.view(-1)[-1] = float("nan")
    mid_inf.view(-1)[t.size // 2] = float("inf")
    uniform_mu = np.linspace(-1.0, 1.0, nmu)
    cases = {
        "NaN in the last word": (gamma, mu, last_nan.data_ptr()),
        "+inf in the middle": (gamma, mu, mid_inf.data_ptr()),
        "null d_log_n": (gamma, mu, None),
        "mu without gamma": (None, uniform_mu, good.data_ptr()),
    }
    with time_limit(120):
        gpu_ctx.set_tables_2d_nodes(gamma, mu, t, k)
        before, first = gpu_ctx.tables_blob(), rows(gpu_ctx, fix, 2)
        torch.cuda.synchronize()
        for name, (g, m, ptr) in cases.items():
            assert raw_device_set(gpu_ctx, nt, nn, g, float(gamma[0]), float(gamma[-1]), nmu, m, ptr) == EINVAL, name
            first_difference("the set after " + name, gpu_ctx.tables_blob(), before)
            again = rows(gpu_ctx, fix, 2)
            first_difference("the rows after " + name, again[0], first[0])
            assert (again[1] == first[1]).all() and (again[2] == first[2]).all(), name
        assert raw_device_set(gpu_ctx, nt, nn, gamma, 1.0, 2.0, nmu, mu, good.data_ptr()) == 0      # the same call, sound
    first_difference("the sound call", gpu_ctx.tables_blob(), before)
    assert same_rows(first[0], fix["values"][0][:2]).all()


def test_python_refuses_without_reaching_the_gpu(gpu_ctx, fix):
    """a float32 tensor, a non-contiguous view, a CPU tensor of the wrong rank, shapes outside the form's limits, rows that do
    not match the nodes: an exception each, and the set installed before stays"""
    import torch
    gamma, mu, t, k = fixture_set(fix, 0)
    good = to_device(t)
    with time_limit(60):
        gpu_ctx.set_tables_2d_nodes(gamma, mu, t, k)
        before = gpu_ctx.tables_blob()
        with pytest.raises(TypeError):
            gpu_ctx.set_tables_2d_nodes(gamma, mu, good.to(torch.float32), k)
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d_nodes(gamma, mu, to_device(np.swapaxes(t, 1, 2).copy()).transpose(1, 2), k)
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d_nodes(gamma, mu, torch.zeros((2, 2, len(gamma), len(mu)), dtype=torch.float64), k)
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d_nodes(gamma, mu, good[0, 0], k)                   # rank 1
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d_nodes(gamma, mu, good[:, :, :8].contiguous(), k)  # rows that do not match the mu nodes
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d_grid(gamma[:16], good)                            # 32 rows for 16 gamma nodes
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d(1.01, 1e4, to_device(np.zeros((1, 8, 7))))        # too few mu nodes
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d(0.5, 1e4, good)                                   # gamma_lo < 1
        with pytest.raises(ValueError):
            gpu_ctx.set_tables_2d_nodes(gamma, mu, good, [0.5, -1.0])               # a negative exponent
        after = gpu_ctx.tables_blob()
    first_difference("the set after the refusals", after, before)


# ---- 4. a change of form --------------------------------------------------------------------------------------------------
def test_a_change_of_form_through_the_device_entry_leaves_no_state(gpu_ctx, fix):
    """2-D on given nodes from a tensor, then the 2-D uniform form from the host: its set and its first four rows are those of
    a fresh context that never saw the device entry, and the fixture's recorded ones."""
    import tab2d_bind as t2
    two = np.load(os.path.join(GOLDEN, "tabulated_2d_det.npz"))
    n_nodes, n_mu = (int(x) for x in two["geometry"][0])
    lo, hi, tables = float(two["gamma_lo"]), float(two["gamma_hi"]), t2.edge_tables_2d(n_nodes, n_mu, two["cols_0"])
    gamma, mu, t, k = fixture_set(fix, 1)
    with time_limit(300):
        gpu_ctx.set_tables_2d_nodes(gamma, mu, to_device(t), k)
        own = rows(gpu_ctx, fix)
        gpu_ctx.set_tables_2d(lo, hi, tables)
        blob, after = gpu_ctx.tables_blob(), rows(gpu_ctx, two)
        gpu_ctx.close_now()                                                         # the next use opens a fresh context
        gpu_ctx.set_tables_2d(lo, hi, tables)
        fresh_blob, fresh = gpu_ctx.tables_blob(), rows(gpu_ctx, two)
    assert np.isfinite(own[0]).any() and np.isfinite(fresh[0]).any()
    first_difference("the set", blob, fresh_blob)
    for i, name in enumerate(("values", "status", "work")):
        assert (np.asarray(after[i]).view(np.uint8) == np.asarray(fresh[i]).view(np.uint8)).all(), name
    assert same_rows(fresh[0], two["values"][0][:4]).all()
