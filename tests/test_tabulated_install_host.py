"""A 2-D table set installed from device memory (rimphony_ctx_set_tables_2d_device), without a GPU: the host build of
tab_install.h -- the text the kernels of rimphony_tab_install.hip run per lane -- looped over the lines as the grid would
visit them (tests/support/tab_install_driver.cpp) against rim_tab_build_2d, rim_tab_build_2d_grid and
rim_tab_build_2d_nodes on the same numbers.  Equality is by bit pattern over the whole set: header, table headers with
sin_k, guides, node words and the four words of every node.  And the geometry-only checks against the full checks.
CPU only.

The shapes: 1 x 8 x 8 is the minimum of both axes; 3 x 9 x 11 and 5 x 70 x 13 are odd sizes that test the table offsets, the
second with more lines than the loop has lanes; 1 x 300 x 8 and 1 x 4096 x 8 are long chains along gamma; 2 x 8 x 1024 is the
mu limit.  Every |ln n| stays below 700: content that overflows makes NaNs whose payload proves nothing."""
import ctypes
import os
import subprocess
from ctypes import POINTER, c_double, c_int, c_longlong, c_size_t

import numpy as np
import pytest

import tab2d_nodes_bind as tn
import tab_bind
import tab_grid_bind as tg
import tab_install_inputs as ti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 8, 8), (3, 9, 11), (5, 70, 13), (1, 300, 8), (2, 8, 1024), (1, 4096, 8)]
LANES = 192                 # three waves: 5 x 70 x 13 has 350 lines along mu, so a lane takes more than one
GLO, GHI = ti.GLO, ti.GHI
_lib = None


def lib():
    global _lib
    if _lib is None:
        from rimphony_amd import _build
        src = os.path.join(ROOT, "tests", "support", "tab_install_driver.cpp")
        so = os.path.join(ROOT, "tests", "support", "tab_install_driver.so")
        deps = [src] + [os.path.join(_build.CSRC, f) for f in os.listdir(_build.CSRC) if f.endswith(".h")]
        if not _build._newer(so, deps):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-mfma", "-msse4.1",
                            "-shared", src, "-o", so], check=True)
        L = ctypes.CDLL(so)
        dp = POINTER(c_double)
        L.tabi_run.restype = c_longlong
        L.tabi_run.argtypes = [c_size_t, c_size_t, dp, c_double, c_double, c_size_t, dp, dp, dp, c_size_t, dp, dp, c_size_t]
        L.tabi_check.restype = c_int
        L.tabi_check.argtypes = [c_size_t, c_size_t, dp, c_double, c_double, c_size_t, dp, c_int, dp, dp, POINTER(c_int),
                                 POINTER(c_int)]
        _lib = L
    return _lib


def _dp(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_double))


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def run(gamma, mu, log_n, sin_k, glo=GLO, ghi=GHI, lanes=LANES):
    nt, nn, nmu = log_n.shape
    gamma, mu, log_n, sin_k = _c(gamma), _c(mu), _c(log_n), _c(sin_k)
    size = lib().tabi_run(nt, nn, _dp(gamma), glo, ghi, nmu, _dp(mu), _dp(log_n), _dp(sin_k), lanes, None, None, 0)
    assert size > 0, size
    host, dev = np.zeros(size), np.zeros(size)
    assert lib().tabi_run(nt, nn, _dp(gamma), glo, ghi, nmu, _dp(mu), _dp(log_n), _dp(sin_k), lanes, _dp(host), _dp(dev), size) == size
    return host, dev


# ---- 1. bit identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smooth", "rough"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", ["uniform", "grid", "nodes"])
def test_lines_reproduce_the_host_build_bit_for_bit(form, shape, kind):
    rng = np.random.default_rng(20261020 + 7 * SHAPES.index(shape) + (1 if kind == "rough" else 0))
    gamma, mu, g_at, mu_at = ti.nodes_of(form, shape, rng)
    log_n = ti.smooth(shape, g_at, mu_at, rng) if kind == "smooth" else ti.rough(shape, rng)
    assert np.isfinite(log_n).all() and np.abs(log_n).max() <= 700.0
    # every other case carries a prefactor, so that both fronts are compared
    sin_k = None if SHAPES.index(shape) % 2 == 0 else np.linspace(0.5, 2.5, shape[0])
    host, dev = run(gamma, mu, log_n, sin_k)
    assert np.isfinite(host).all()
    diff = np.flatnonzero(host.view(np.uint64) != dev.view(np.uint64))
    assert diff.size == 0, (form, shape, kind, diff[:8], host[diff[:8]], dev[diff[:8]])
    nodes = host[-4 * log_n.size:].reshape(shape + (4,))
    assert np.array_equal(nodes[..., 0], log_n)                                     # the right words were compared
    assert np.abs(nodes[..., 1:]).max() > 0.0


def test_the_order_of_the_lines_within_a_family_changes_nothing():
    """One lane, one wave, more lanes than lines: the same bits, because a line reads nothing another line of its family writes"""
    rng = np.random.default_rng(5)
    gamma, mu = ti.graded_gamma(70, rng), ti.graded_mu(13, rng)
    log_n = ti.smooth((5, 70, 13), gamma, mu, rng)
    ref = run(gamma, mu, log_n, None, lanes=1)[1]
    for lanes in (64, 1000):
        assert np.array_equal(run(gamma, mu, log_n, None, lanes=lanes)[1].view(np.uint64), ref.view(np.uint64))


# ---- 2. the geometry-only checks ------------------------------------------------------------------------------------------
def verdicts(gamma, mu, log_n, sin_k, shape, glo=GLO, ghi=GHI, with_mu=False):
    nt, nn, nmu = shape
    gamma, mu, log_n = _c(gamma), _c(mu), _c(log_n)
    if sin_k is not None:
        sin_k = _c(np.broadcast_to(np.asarray(sin_k, dtype=np.float64), (int(nt),)))
    full, geo = c_int(7), c_int(7)
    assert lib().tabi_check(nt, nn, _dp(gamma), glo, ghi, nmu, _dp(mu), int(with_mu), _dp(log_n), _dp(sin_k), ctypes.byref(full),
                            ctypes.byref(geo)) == 0
    return full.value, geo.value


def geometry_agrees(name, gamma, mu, log_n, sin_k, shape=None, with_mu=False, **kw):
    """The case is refused by the full check; the geometry-only check gives the verdict the full check gives once the values
    are out of the question (finite zeros of the stated shape in their place)."""
    shape = log_n.shape if shape is None else shape
    full, geo = verdicts(gamma, mu, log_n, sin_k, shape, with_mu=with_mu, **kw)
    assert full == -1, name
    clean = verdicts(gamma, mu, np.zeros(shape), sin_k, shape, with_mu=with_mu, **kw)
    assert geo == clean[0] == clean[1], (name, geo, clean)
    return geo


def test_geometry_checks_agree_with_the_full_checks_uniform():
    """the refused cases of test_tabulated_2d_host.py and, with a prefactor, of test_tabulated_2d_pitchy_host.py"""
    import tab2d_bind as t2
    good = t2.edge_tables_2d(16, 16)
    lo, hi = t2.EDGE_LO, t2.EDGE_HI
    assert verdicts(None, None, good, None, good.shape, lo, hi) == (0, 0)
    assert verdicts(None, None, np.zeros((1, 1024, 1024)), None, (1, 1024, 1024), lo, hi) == (0, 0)      # the cap itself
    nan_t, inf_t = good.copy(), good.copy()
    nan_t[1, 5, 3], inf_t[2, 0, 15] = np.nan, -np.inf
    k = np.array([0.5, 1.0, 2.5])
    for sin_k in (None, k):
        cases = ((good[:, :, :7], lo, hi, -1), (np.zeros((1, 16, 1025)), lo, hi, -1), (good[:, :7, :], lo, hi, -1),
                 (np.zeros((1, 1025, 1024)), lo, hi, -1), (nan_t, lo, hi, 0), (inf_t, lo, hi, 0),
                 (good, 0.5, hi, -1), (good, 10.0, 10.0, -1), (good, 10.0, 5.0, -1), (good, 1.01, np.inf, -1))
        for i, (log_n, a, b, want) in enumerate(cases):
            sk = None if sin_k is None else sin_k[:log_n.shape[0]]
            assert geometry_agrees(("uniform", i), None, None, log_n, sk, glo=a, ghi=b) == want
    for bad in ([0.5, -0.1, 1.0], [100.5, 1.0, 1.0], [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0]):
        assert geometry_agrees(("uniform k", bad), None, None, good, bad, glo=lo, ghi=hi) == -1
    assert geometry_agrees("null log_n", None, None, None, None, shape=good.shape, glo=lo, ghi=hi) == 0


def test_geometry_checks_agree_with_the_full_checks_grid():
    """the refused cases of test_tabulated_2d_grid_host.py, plain and with a prefactor"""
    import tab2d_grid_bind as tq
    g = tg.grid("jitter")
    t = tq.surfaces_at(g, 16)
    assert verdicts(g, None, t, None, t.shape) == (0, 0)
    for sin_k in (None, 1.5):
        def refused(gamma, log_n, want, shape=None):
            assert geometry_agrees("grid", gamma, None, log_n, sin_k, shape=shape) == want

        refused(g, None, 0, shape=(3, 64, 16))
        for bad in (np.nan, np.inf, -np.inf):
            gb, tb = g.copy(), t.copy()
            gb[3], tb[1, 5, 3] = bad, bad
            refused(gb, t, -1)
            refused(g, tb, 0)
        low, same, swapped, close = g.copy(), g.copy(), g.copy(), g.copy()
        low[0] = np.nextafter(1.0, 0.0)
        same[21] = same[20]
        swapped[[20, 21]] = swapped[[21, 20]]
        close[30] = np.nextafter(close[29], np.inf)
        for gb in (low, same, swapped, close):
            refused(gb, t, -1)
        many, g1025 = tab_bind.nodes(1.01, 1e4, 65537), tab_bind.nodes(1.01, 1e4, 1025)
        refused(g[:7], t[:, :7], -1)
        refused(many, np.zeros((1, 65537, 8)), -1)
        refused(g, t[:, :, :7], -1)
        refused(g[:16], np.zeros((1, 16, 1025)), -1)
        refused(g1025, np.zeros((1, 1025, 1024)), -1)
        assert verdicts(g1025[:1024], None, np.zeros((1, 1024, 1024)), sin_k, (1, 1024, 1024)) == (0, 0)
        assert verdicts(many[:65536], None, np.zeros((1, 65536, 16)), sin_k, (1, 65536, 16)) == (0, 0)


@pytest.mark.parametrize("which", [0, 1])
def test_geometry_checks_agree_with_the_full_checks_nodes(which):
    """every case of tab2d_nodes_bind.refused_cases: only the two that are about the values pass the geometry-only check"""
    gamma, mu, t, k = tn.fixture_set(which)
    assert verdicts(gamma, mu, t, k, t.shape, with_mu=True) == (0, 0)
    passed = []
    for name, (g, m, log_n, sin_k, shape) in tn.refused_cases(gamma, mu, t, k).items():
        if geometry_agrees(name, g, m, log_n, sin_k, shape=shape, with_mu=True) == 0:
            passed.append(name)
    assert sorted(passed) == ["log_n NaN", "null log_n"]
