"""Families of 2-D surfaces on given gamma and mu nodes with a real index per row (rimphony_ctx_set_tables_2d_family) without a
GPU: the entry and its mirrors; a row at an integer index carries the bits of the plain nodes form's oracle; the family at a
fractional index against the plain form installed with ln n blended on the host; two surfaces bilinear in (ln gamma, mu)
against the ANALYTIC tilted power law of tests/support (which shares no code with the tables) at the blended parameters;
continuity and the range of the index; what the host check refuses.  The library's side is the 2-D family oracle
(tests/support/liboracle_tab2dfamily.so): the host build of the device functions and of rim_tab_check_2d_family /
rim_tab_build_2d_family.  CPU only.

The bounds of 3. and 4. come from profiles/tabulated_2d_family_accuracy.txt, which records what tools/tab_2d_family_accuracy.py
measured with the very functions this file calls (tab2d_family_bind.measure_*; every test prints its figures, `pytest -s`):
twice the recorded figure -- the margin covers another libm, nothing else varies."""
import ctypes
import os
import re

import numpy as np
import pytest

import tab2d_ends_bind as te
import tab2d_family_bind as tf
import tab2d_nodes_bind as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "rimphony_ctx_set_tables_2d_family"
MARGIN = 2.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def accuracy():
    return tf.read_accuracy()


# ---- 1. the entry and its mirrors ---------------------------------------------------------------------------------------
def test_entry_in_library_header_and_mirrors():
    from rimphony_amd import _build, api, capi
    _build.build_hip()
    lib = ctypes.CDLL(capi.LIB_PATH)
    fn = getattr(lib, ENTRY)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert fn(None, 0, 0, None, 0, None, None, None, 0, 0) == -1        # a null context is refused before anything is touched
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    assert re.search(r"int rimphony_ctx_set_tables_2d_family\(rimphony_ctx \*ctx, size_t n_tables, size_t n_nodes, const double \*gamma, "
                     r"size_t n_mu,\s+const double \*mu, const double \*log_n, const double \*sin_k, int ends_gamma, int ends_mu\);", hdr)
    assert ENTRY in capi.SYMBOLS
    rs = open(os.path.join(ROOT, "rimphony-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn rimphony_ctx_set_tables_2d_family\(", rs)
    hpp = open(os.path.join(ROOT, "rimphony_amd", "cxx", "rimphony.hpp")).read()
    assert ENTRY in hpp and "class TabulatedFamily2D" in hpp
    gamma, mu = np.exp(np.linspace(0.01, 5.0, 9)), np.linspace(-1.0, 1.0, 8)
    fam = api.TabulatedFamily2D.from_function(lambda g, m, p: g ** -p * np.exp(0.1 * p * m), gamma, mu, [2.0, 3.0, 5.0],
                                              sin_k=[0.0, 1.0, 2.0], ends="not-a-knot")
    assert fam.log_n.shape == (3, 9, 8) and fam.sin_k.tolist() == [0.0, 1.0, 2.0] and fam.ends == (1, 1)
    assert np.allclose(fam.log_n[1], -3.0 * np.log(gamma)[:, None] + 0.3 * mu[None, :], rtol=1e-14, atol=1e-14)
    assert fam.index([2.0, 2.5, 3.0, 4.0, 5.0]).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    assert fam.at(4.0).x == 1.5
    for bad in (1.9, 5.1, np.nan):
        with pytest.raises(ValueError):
            fam.index(bad)
    down = api.TabulatedFamily2D(gamma, mu, np.zeros((3, 9, 8)), param=[10.0, 5.0, 1.0])
    assert down.index([10.0, 7.5, 1.0]).tolist() == [0.0, 0.5, 2.0] and down.ends is None
    with pytest.raises(ValueError):
        api.TabulatedFamily2D(gamma, mu, np.zeros((3, 9, 8)), param=[1.0, 1.0, 2.0])
    with pytest.raises(ValueError):
        api.TabulatedFamily2D(gamma, mu, np.zeros((3, 9, 8)), sin_k=[0.5, 101.0, 1.0])
    with pytest.raises(ValueError):
        api.TabulatedFamily2D(gamma, mu[::-1], np.zeros((3, 9, 8)))
    with pytest.raises(ValueError):
        api.TabulatedFamily2D(gamma, mu, np.zeros((3, 9, 8)), ends="clamped")


# ---- 2. integer rows are the plain nodes form ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A: plain, natural", "B: sin_k, not-a-knot in mu"])
def test_integer_rows_are_the_plain_nodes_form(which):
    """The family oracle at every integer x against the nodes oracle on the same tables, sin_k and ends, as uint64: the
    normalisation, calc_f and both derivatives on 200 gamma x 5 mu, all eight coefficients and the sample counts of the
    fixture's rows at integer x; and the laid-out set, word for word but for the normalisation words."""
    gamma_n, mu_n, t, k, ends = tf.fixture_set(which)
    nt = t.shape[0]
    assert tf.set_tables(gamma_n, mu_n, t, k, ends) == 0
    assert te.set_tables(gamma_n, mu_n, t, k, ends) == 0
    fb, pb = tf.blob(), te.blob()
    at = te.norm_at(nt)
    assert len(fb) == len(pb) and np.isnan(fb[at]).all() and np.isfinite(pb[at]).all()
    assert np.delete(fb, at).tobytes() == np.delete(pb, at).tobytes()
    assert (te.ends_words(fb) == ends[0] + 2 * ends[1]).all() and (fb[-4 * t.size:] != 0).all()
    index = np.arange(nt, dtype=np.float64)
    norm_f, norm_p = tf.batch_norm(index), te.batch_norm(index)
    assert np.isfinite(norm_p).all() and (bits(norm_f) == bits(norm_p)).all()
    gamma = np.repeat(np.exp(np.linspace(np.log(gamma_n[0]), np.log(gamma_n[-1]), 200)), 5)
    mu = np.tile(np.array([-0.9, -0.3, 0.0, 0.45, 0.99]), 200)
    for i in range(nt):
        got = tf.dev_calc_f(float(i), norm_f[i], gamma, mu)
        want = te.dev_calc_f([float(i)], norm_p[i], gamma, mu)
        for name, g, w in zip(("f", "dfdg", "dfdcx"), got, want):
            assert np.isfinite(w).all() and (bits(g) == bits(w)).all(), (name, i)
        assert (got[0] > 0).sum() >= 990 and (got[2] != 0).sum() >= 990
    fix = np.load(os.path.join(ROOT, "tests", "golden", "tabulated_2d_family_det.npz"))
    x = fix["x"][which]
    rows = np.flatnonzero(tf.valid_x(which, x) & (np.floor(x) == x))
    assert len(rows) >= 5 and set(np.abs(x[rows])) == set(index)
    want, ww = te.batch(fix["s"][rows], fix["theta"][rows], np.abs(x[rows]))
    assert np.isfinite(want).mean() > 0.8
    assert same_bits(fix["values"][which][rows], want).all() and (fix["work"][which][rows] == ww).all()
    assert (bits(fix["norm"][which][rows]) == bits(norm_p[np.abs(x[rows]).astype(int)])).all()


def test_fixture_is_the_oracles():
    """The committed rows against the oracle of this tree, the first 8 rows and the bad ones of each set (the GPU test holds all
    24 to the file): values, sample counts, status and normalisations; and the conditions the fixture was made under."""
    fix = np.load(os.path.join(ROOT, "tests", "golden", "tabulated_2d_family_det.npz"))
    for which in (0, 1):
        gamma_n, mu_n, t, k, ends = tf.fixture_set(which)
        assert tf.set_tables(gamma_n, mu_n, t, k, ends) == 0
        x = fix["x"][which]
        assert same_bits(x, tf.fixture_x(which)).all()
        valid = tf.valid_x(which, x)
        rows = np.concatenate([np.arange(8), np.flatnonzero(~valid)])
        v, w = tf.batch(fix["s"][rows], fix["theta"][rows], x[rows])
        assert same_bits(v, fix["values"][which][rows]).all() and (w == fix["work"][which][rows]).all()
        assert same_bits(tf.batch_norm(x), fix["norm"][which]).all()
        finite = np.isfinite(fix["values"][which])
        assert finite.any(axis=0).all() and finite[valid].mean() >= 0.8 and (~valid).sum() == tf.BAD_X
        assert not finite[~valid].any() and (fix["status"][which][~valid] == (16 | 32)).all()
        assert (fix["status"][which][valid] == np.where(finite[valid], 0, 16)).all()


# ---- 3. linearity: the family against the plain form on the blended data ------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_family_is_the_plain_form_on_the_blended_data(accuracy, which):
    """The bicubic is linear in its node words and the tensor-product solve is linear in the data, for natural and for
    not-a-knot ends: the family at a fractional x is the plain form installed with t_a + w (t_b - t_a), to the rounding of the
    blended values.  f, its two derivatives and the eight coefficients; at most twice the recorded figures."""
    worst = tf.measure_linearity(which)
    for name, v in worst.items():
        rec = accuracy["linearity_%s_%s" % ("AB"[which], name)]
        print("linearity", "AB"[which], name, "measured %.3e" % v, "recorded %.3e" % rec)
        assert v <= MARGIN * rec, (name, v, rec)


# ---- 4. exactness: bilinear surfaces against the analytic tilted power law ----------------------------------------------------
@pytest.mark.parametrize("with_k", [False, True], ids=["tilt_oracle", "pitchy_tilt_oracle"])
def test_bilinear_family_against_the_analytic_oracle(accuracy, with_k):
    """Two surfaces ln n = -p u + q u mu + a mu - gamma / cut with different (p, a, q) on 2048 x 8 nodes: ln n is linear in every
    one of them, so the row at x is the closed form at the blended (p, a, q) -- with sin_k at the blended k -- at five interior
    x.  At most twice the recorded figure, and no looser than the plain nodes form's own bound on such a surface: 4 times the
    worst figure of profiles/tabulated_2d_nodes_accuracy.txt (test_tabulated_2d_nodes_host.py: MARGIN, MEASURED_TILT)."""
    name = "exactness_sin_k" if with_k else "exactness_plain"
    got = tf.measure_exactness(with_k)
    plain = [float(m.group(1)) for m in re.finditer(r"^  q = \S+\s+a = \S+\s+k = \S+\s+(\S+)$",
                                                    open(os.path.join(ROOT, "profiles", "tabulated_2d_nodes_accuracy.txt")).read(), re.M)]
    assert len(plain) == 4
    bound = min(MARGIN * accuracy[name], 4.0 * max(plain))
    print(name, "measured %.3e" % got, "recorded %.3e" % accuracy[name], "the plain form's bound %.3e" % (4.0 * max(plain)))
    assert got <= bound, (got, bound)


# ---- 5. continuity and the range of the index --------------------------------------------------------------------------------
def test_continuity_and_range_of_the_index():
    """Set A is ordered in its index where the surfaces' own terms are: the steeper table has the larger normalisation.  The
    values at x = 1 -+ eps against those at 1, bounded as test_tabulated_family_host.py bounds them (1e-9 at eps = 2^-40: the
    family is Lipschitz in x with a constant of a few |ln n|), and at 1 - 2^-52 to a rounding of f; then the range rule."""
    gamma_n, mu_n, t, k, ends = tf.fixture_set(0)
    assert tf.set_tables(gamma_n, mu_n, t, k, ends) == 0
    rng = np.random.default_rng(5)
    gamma = np.exp(rng.uniform(np.log(gamma_n[0]), np.log(gamma_n[-1]), 300))
    mu = rng.uniform(-0.99, 0.99, 300)
    eps = 2.0 ** -40
    xs = np.array([1.0 - eps, 1.0, 1.0 + eps, 1.0 - 2.0 ** -52])
    nrm = tf.batch_norm(xs)
    assert np.isfinite(nrm).all() and abs(nrm[0] / nrm[1] - 1.0) <= 1e-9 and abs(nrm[2] / nrm[1] - 1.0) <= 1e-9
    assert nrm[0] != nrm[1] and nrm[2] != nrm[1]
    fa, fb, fc, fd = (tf.dev_calc_f(x, n, gamma, mu) for x, n in zip(xs, nrm))
    assert (fb[0] > 0).all()
    for i, name in enumerate(("f", "dfdg", "dfdcx")):
        scale = np.abs(fb[i]) + np.abs(fb[0])
        below, above = (np.abs(fa[i] - fb[i]) / scale).max(), (np.abs(fc[i] - fb[i]) / scale).max()
        print("continuity at x = 1:", name, below, above)
        assert below <= 1e-9 and above <= 1e-9
    assert not (bits(fa[0]) == bits(fb[0])).all() and not (bits(fc[0]) == bits(fb[0])).all()
    # one rounding of the index below the table: the weight is 1 - 2^-52, every node word within a rounding of table 1's, and
    # a rounding of a node word is an absolute error of S = ln n of the size of the largest word, hence a relative error of f
    # of that many ulps: 8 (1 + max|ln n|) ulps of slack, the sibling test's allowance with the words' size for |ln f|
    slack = 8.0 * (1.0 + np.abs(t).max()) * np.spacing(fb[0])
    assert (np.abs(fd[0] - fb[0]) <= slack).all()
    # the range, on set A
    last = float(t.shape[0] - 1)
    x = np.array([last, np.nextafter(last, np.inf), -1e-300, np.nan, np.inf, -np.inf, 1e300, -0.0, 0.0])
    nrm = tf.batch_norm(x)
    assert np.isfinite(nrm[0]) and np.isnan(nrm[1:7]).all()
    assert bits(nrm[7:8])[0] == bits(nrm[8:9])[0] and np.isfinite(nrm[7])
    for u, v in zip(tf.dev_calc_f(0.0, nrm[8], gamma, mu), tf.dev_calc_f(-0.0, nrm[7], gamma, mu)):
        assert (bits(u) == bits(v)).all()
    # the line of a row: the weight, the blended k, the distance to the upper table -- none at the last table and for a bad row
    per = t.shape[1] * t.shape[2] * 4
    assert tf.row_line(0.25)[:3] == (0.25, 0.0, per) and tf.row_line(last)[:3] == (0.0, 0.0, 0.0)
    assert tf.row_line(last - 2.0 ** -52)[:3] == (1.0 - 2.0 ** -52, 0.0, per) and tf.row_line(np.nan)[:3] == (0.0, 0.0, per)
    gb, mb, tb, kb, eb = tf.fixture_set(1)
    assert tf.set_tables(gb, mb, tb, kb, eb) == 0
    assert tf.row_line(0.25)[1] == kb[0] + 0.25 * (kb[1] - kb[0]) and tf.row_line(1.0)[1] == kb[1]
    out = tf.batch(np.array([30.0] * 3), np.array([0.9] * 3), np.array([1.0, np.nextafter(1.0, np.inf), np.nan]), 0x03)[0]
    assert np.isfinite(out[0, :2]).all() and np.isnan(out[1:]).all()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_set_in_place():
    """Each limit, non-finite data, mu nodes that do not end at +-1, a bad k and bad ends: what rimphony_ctx_set_tables_2d_nodes
    refuses (tab2d_nodes_bind.refused_cases) and what rimphony_ctx_set_tables_2d_ends refuses of the ends."""
    from rimphony_amd import api
    gamma_n, mu_n, t, k, ends = tf.fixture_set(1)
    assert tf.set_tables(gamma_n, mu_n, t, k, ends) == 0
    before = tf.blob()
    cases = tn.refused_cases(gamma_n, mu_n, t, k)
    assert len(cases) >= 20
    for name, (g, m, tt, kk, shape) in cases.items():
        assert tf.set_tables(g, m, tt, kk, ends, shape) == -1, name
        if g is not None and m is not None and tt is not None:
            with pytest.raises(ValueError):
                api.TabulatedFamily2D(g, m, tt, kk)
    for bad_ends in ((2, 0), (0, -1), (0, 2), (7, 7)):
        assert tf.set_tables(gamma_n, mu_n, t, k, bad_ends) == -1, bad_ends
    assert tf.blob().tobytes() == before.tobytes()
    # n_tables = 0 clears
    assert tf.set_tables(None, None, np.zeros((0, 8, 8)), None) == 0 and len(tf.blob()) == 0
