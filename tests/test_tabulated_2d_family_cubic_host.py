"""Families of 2-D surfaces blended CUBICALLY across their tables (rimphony_ctx_set_tables_2d_family_cubic) without a GPU: the
entry and its mirrors; a row at an integer index carries the bits of the plain nodes form's oracle; the committed fixture; the
family at a fractional index against the plain form installed with ln n blended on the host with weights computed here in
numpy; surfaces whose coefficients are cubic in the knots against the ANALYTIC tilted power law of tests/support (which shares
no code with the tables); the Juettner family next to the linear blend; continuity across every integer index; what the host
check refuses; the laid-out set.  The library's side is the form's oracle (tests/support/liboracle_tab2dfamilycubic.so): the
host build of the device functions and of rim_tab_check_2d_family_cubic / rim_tab_build_2d_family_cubic.  CPU only.

The bounds of 4. and 5. come from profiles/tabulated_2d_family_cubic_accuracy.txt, which records what
tools/tab_2d_family_cubic_accuracy.py measured with the very functions this file calls (tab2d_family_cubic_bind.measure_*; every
test prints its figures, `pytest -s`): twice the recorded figure -- the margin covers another libm, nothing else varies."""
import ctypes
import os
import re

import numpy as np
import pytest

import tab2d_ends_bind as te
import tab2d_family_bind as tf
import tab2d_family_cubic_bind as tc
import tab2d_nodes_bind as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "rimphony_ctx_set_tables_2d_family_cubic"
FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_2d_family_cubic_det.npz")
MARGIN = 2.0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def install(which):
    gamma_n, mu_n, t, k, ends, param = tc.fixture_set(which)
    assert tc.set_tables(gamma_n, mu_n, t, k, ends, param) == 0
    return gamma_n, mu_n, t, k, ends, param


@pytest.fixture(scope="module")
def accuracy():
    return tc.read_accuracy(tc.ACCURACY)


# ---- 1. the entry and its mirrors ---------------------------------------------------------------------------------------
def test_entry_in_library_header_and_mirrors():
    from rimphony_amd import _build, api, capi
    _build.build_hip()
    lib = ctypes.CDLL(capi.LIB_PATH)
    fn = getattr(lib, ENTRY)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    assert fn(None, 0, 0, None, 0, None, None, None, 0, 0, None) == -1  # a null context is refused before anything is touched
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    assert re.search(r"int rimphony_ctx_set_tables_2d_family_cubic\(rimphony_ctx \*ctx, size_t n_tables, size_t n_nodes, "
                     r"const double \*gamma, size_t n_mu,\s+const double \*mu, const double \*log_n, const double \*sin_k, "
                     r"int ends_gamma, int ends_mu,\s+const double \*param\);", hdr)
    assert ENTRY in capi.SYMBOLS
    rs = open(os.path.join(ROOT, "rimphony-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn rimphony_ctx_set_tables_2d_family_cubic\(", rs) and "param: *const c_double," in rs
    hpp = open(os.path.join(ROOT, "rimphony_amd", "cxx", "rimphony.hpp")).read()
    assert ENTRY in hpp and "void set_tables_2d_family_cubic(" in hpp and "bool cubic = false" in hpp
    gamma, mu = np.exp(np.linspace(0.01, 5.0, 9)), np.linspace(-1.0, 1.0, 8)
    fam = api.TabulatedFamily2D.from_function(lambda g, m, p: g ** -p * np.exp(0.1 * p * m), gamma, mu, [2.0, 3.0, 5.0, 6.0],
                                              sin_k=[0.0, 1.0, 2.0, 2.5], ends="not-a-knot", blend="cubic")
    assert fam.blend == "cubic" and fam.log_n.shape == (4, 9, 8) and fam.param.tolist() == [2.0, 3.0, 5.0, 6.0]
    # index() and at() are the linear family's: the row's parameter stays the real index
    assert fam.index([2.0, 2.5, 3.0, 4.0, 5.0, 6.0]).tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0] and fam.at(4.0).x == 1.5
    assert api.TabulatedFamily2D(gamma, mu, np.zeros((3, 9, 8))).blend == "linear"
    with pytest.raises(ValueError):
        api.TabulatedFamily2D(gamma, mu, np.zeros((3, 9, 8)), blend="cubic")            # fewer than four tables
    with pytest.raises(ValueError):
        api.TabulatedFamily2D(gamma, mu, np.zeros((4, 9, 8)), blend="quintic")
    with pytest.raises(ValueError):
        api.TabulatedFamily2D(gamma, mu, np.zeros((4, 9, 8)), param=[1.0, 2.0, 2.0, 3.0], blend="cubic")

    class NoContext:                    # the argument checks come before the library is reached
        lib = handle = None
    for kw in (dict(blend="linear", param=[0.0, 1.0, 2.0, 3.0]), dict(blend="quintic"), dict(blend="cubic", param=[0.0, 1.0, 2.0]),
               dict(blend="cubic", param=[0.0, 1.0, np.nan, 3.0]), dict(blend="cubic", param=[0.0, 2.0, 1.0, 3.0])):
        with pytest.raises(ValueError):
            api.Context.set_tables_2d_family(NoContext(), gamma, mu, np.zeros((4, 9, 8)), **kw)
    with pytest.raises(ValueError):
        api.Context.set_tables_2d_family(NoContext(), gamma, mu, np.zeros((3, 9, 8)), blend="cubic")


# ---- 2. integer rows are the plain nodes form ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A: plain, natural", "B: sin_k, not-a-knot in mu"])
def test_integer_rows_are_the_plain_nodes_form(which):
    """The oracle at every integer x against the nodes oracle on the same tables, sin_k and ends, as uint64: the weights (a 1
    and three zeros), the normalisation, calc_f and both derivatives on 200 gamma x 5 mu, all eight coefficients and the sample
    counts of the fixture's rows at integer x."""
    gamma_n, mu_n, t, k, ends, param = install(which)
    nt = t.shape[0]
    assert te.set_tables(gamma_n, mu_n, t, k, ends) == 0
    index = np.arange(nt, dtype=np.float64)
    for i in range(nt):
        w, kk, stride, L, base, p = tc.row_line(float(i))
        assert base == min(max(i - 1, 0), nt - 4) and sorted(np.abs(L).tolist()) == [0.0, 0.0, 0.0, 1.0] and L[i - base] == 1.0
        assert bits([p])[0] == bits([param[i]])[0] and w == 0.0 and stride == t.shape[1] * t.shape[2] * 4
        assert kk == (0.0 if k is None else k[i])
    norm_f, norm_p = tc.batch_norm(index), te.batch_norm(index)
    assert np.isfinite(norm_p).all() and (bits(norm_f) == bits(norm_p)).all()
    gamma = np.repeat(np.exp(np.linspace(np.log(gamma_n[0]), np.log(gamma_n[-1]), 200)), 5)
    mu = np.tile(np.array([-0.9, -0.3, 0.0, 0.45, 0.99]), 200)
    for i in range(nt):
        got = tc.dev_calc_f(float(i), norm_f[i], gamma, mu)
        want = te.dev_calc_f([float(i)], norm_p[i], gamma, mu)
        for name, g, w in zip(("f", "dfdg", "dfdcx"), got, want):
            assert np.isfinite(w).all() and (bits(g) == bits(w)).all(), (name, i)
        assert (got[0] > 0).sum() >= 990 and (got[2] != 0).sum() >= 990
    fix = np.load(FIXTURE)
    x = fix["x"]
    rows = np.flatnonzero(tc.valid_x(x) & (np.floor(x) == x))
    assert len(rows) >= 8 and set(np.abs(x[rows])) == set(index)
    want, ww = te.batch(fix["s"][rows], fix["theta"][rows], np.abs(x[rows]))
    assert np.isfinite(want).mean() > 0.8
    assert same_bits(fix["values"][which][rows], want).all() and (fix["work"][which][rows] == ww).all()
    assert (bits(fix["norm"][which][rows]) == bits(norm_p[np.abs(x[rows]).astype(int)])).all()
    assert (fix["status"][which][rows] == np.where(np.isfinite(want), 0, 16)).all()


# ---- 3. the committed fixture ---------------------------------------------------------------------------------------------------
def test_fixture_is_the_oracles():
    """The committed rows against the oracle of this tree: the integer rows, one row per table interval and the bad ones of each
    set (the GPU test holds all 24 to the file): values, sample counts, status and normalisations; and the conditions the
    fixture was made under."""
    fix = np.load(FIXTURE)
    x = fix["x"]
    assert same_bits(x, tc.fixture_x()).all()
    valid = tc.valid_x(x)
    assert (~valid).sum() == tc.BAD_X and tuple(x[4:9]) == tc.FRAC_X
    for which in (0, 1):
        install(which)
        rows = np.arange(13)
        v, w = tc.batch(fix["s"][rows], fix["theta"][rows], x[rows])
        assert same_bits(v, fix["values"][which][rows]).all() and (w == fix["work"][which][rows]).all()
        assert same_bits(tc.batch_norm(x), fix["norm"][which]).all()
        finite = np.isfinite(fix["values"][which])
        assert finite.any(axis=0).all() and finite[valid].mean() >= 0.8
        assert not finite[~valid].any() and (fix["status"][which][~valid] == (16 | 32)).all()
        assert (fix["status"][which][valid] == np.where(finite[valid], 0, 16)).all()
        # every stencil position occurs among the valid rows
        assert {tc.row_line(v)[4] for v in x[valid]} == {0, 1, 2}


# ---- 4. independence from the shared text ------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_family_is_the_plain_form_on_the_blended_data(accuracy, which):
    """The bicubic is linear in its node words and the tensor-product solve is linear in the data, for natural and for
    not-a-knot ends: the family at a fractional x is the plain form installed with sum L_i t_{s+i}, the stencil and the weights
    computed here in numpy (tab2d_family_cubic_bind.numpy_weights), to the rounding of the weights and of the blended values.
    First the oracle's weights against numpy's; then f, its two derivatives and the eight coefficients, at most twice the
    recorded figures."""
    gamma_n, mu_n, t, k, ends, param = install(which)
    for x in tc.FRAC_X:
        w, kk, stride, L, base, p = tc.row_line(x)
        s, Ln, pn = tc.numpy_weights(param, len(t), x)
        assert base == s and abs(p - pn) <= 4 * np.spacing(abs(pn)) and abs(L.sum() - 1.0) <= 1e-14
        assert np.abs(L - Ln).max() <= 1e-13 * np.abs(Ln).max()
        if k is not None:
            assert abs(kk - np.dot(Ln, k[s:s + 4])) <= 1e-13 * np.abs(k).max() and 0.0 <= kk <= 100.0
    worst = tc.measure_independence(which)
    for name, v in worst.items():
        rec = accuracy["independence_%s_%s" % ("AB"[which], name)]
        print("independence", "AB"[which], name, "measured %.3e" % v, "recorded %.3e" % rec)
        assert v <= MARGIN * rec, (name, v, rec)


# ---- 5. exactness: coefficients cubic in the knots against the analytic tilted power law ---------------------------------------
@pytest.mark.parametrize("with_k", [False, True], ids=["tilt_oracle", "pitchy_tilt_oracle"])
def test_cubic_family_against_the_analytic_oracle(accuracy, with_k):
    """Five surfaces ln n = -p u + q u mu + a mu - gamma / cut with p, a, q cubic polynomials in unevenly spaced knots on 2048 x
    8 nodes: a 4-point Lagrange cubic reproduces a cubic, so the row at x is the closed form at the polynomials' values -- with
    sin_k at k's polynomial -- at off-knot x in every stencil position.  At most twice the recorded figure."""
    name = "exactness_sin_k" if with_k else "exactness_plain"
    got = tc.measure_exactness(with_k)
    print(name, "measured %.3e" % got, "recorded %.3e" % accuracy[name])
    assert got <= MARGIN * accuracy[name], (got, accuracy[name])
    assert {tc.row_line(x)[4] for x in tc.EX_X} == {0, 1} and len(tc.EX_PARAM) - 4 == 1       # clamped low, interior, clamped high


# ---- 6. the point of the feature -----------------------------------------------------------------------------------------------
def test_cubic_blend_beats_the_linear_blend_on_the_juettner_family(accuracy):
    """The Juettner family of profiles/tabulated_2d_family_accuracy.txt -- the same surface, nodes, ends and rows, the row in
    the middle of every pair -- with the cubic blend on 4 and 8 tables, next to the linear blend computed here through the
    existing form.  Two conditions from an estimate made before any of this was measured (on the 1 / T-dependent part of ln n,
    with numpy: 7.7 times closer on 4 tables, 24 times on 8): at most 1/3 of the linear blend's error on 4 tables, at most 1/8
    on 8.  And the recorded figures, at most twice.

    Measured (CPU oracle): see profiles/tabulated_2d_family_cubic_accuracy.txt."""
    for n, ratio in ((4, 3.0), (8, 8.0)):
        cubic, linear = tc.measure_juettner(n), tf.measure_juettner(n)
        rec = accuracy["juettner_cubic_%d_tables" % n]
        print("juettner", n, "tables: cubic %.3e" % cubic, "linear %.3e" % linear, "ratio %.1f" % (linear / cubic), "recorded %.3e" % rec)
        assert cubic <= linear / ratio, (n, cubic, linear)
        assert cubic <= MARGIN * rec, (n, cubic, rec)


# ---- 7. continuity -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_continuity_across_every_integer_index(which):
    """f, its derivatives, the normalisation and the coefficients at x = t -+ 1e-9 against those at t, for every table t (one
    side at the two ends).  The stencil changes at t = 2 and t = 4 and the weights pass through (0, 1, 0, 0) / (0, 0, 1, 0)
    there, so nothing jumps.  The bound: S = ln n moves by at most step * sum_i |dL_i / dx| * max |ln n| (numpy's weights,
    differenced over the step), which is the relative change of e^S; twice that and 1e-12 for the roundings.  The derivatives
    and the coefficients -- absorption is built from d f / d gamma, the V slots from d f / d mu -- get ten times f's bound,
    relative to |value| + |f| where a derivative passes through zero."""
    gamma_n, mu_n, t, k, ends, param = install(which)
    nt = len(t)
    step = 1e-9
    rng = np.random.default_rng(7 + which)
    gamma = np.exp(rng.uniform(np.log(gamma_n[0]), np.log(gamma_n[-1]), 300))
    mu = rng.uniform(-0.99, 0.99, 300)
    s, th = (v[:4].copy() for v in tc.fixture_rows())
    for i in range(nt):
        sides = [x for x in (i - step, i + step) if 0 <= x <= nt - 1]
        n0 = float(tc.batch_norm(np.array([float(i)]))[0])
        f0 = tc.dev_calc_f(float(i), n0, gamma, mu)
        c0 = tc.batch(s, th, np.full(4, float(i)), 0xFF)[0]
        for x in sides:
            base, L, p = tc.numpy_weights(param, nt, x)
            at = np.zeros(4)
            at[i - base] = 1.0
            moved = np.abs(L - at).sum()                                # = step * sum |dL_i / dx| to first order
            bound = 2.0 * moved * np.abs(t).max() + 1e-12
            assert moved <= 20 * step, (x, moved)                       # the weights themselves are continuous
            n1 = float(tc.batch_norm(np.array([x]))[0])
            f1 = tc.dev_calc_f(x, n1, gamma, mu)
            c1 = tc.batch(s, th, np.full(4, x), 0xFF)[0]
            d_norm = abs(n1 / n0 - 1.0)
            d_f = float(np.abs(f1[0] / f0[0] - 1.0).max())
            d_dg = float((np.abs(f1[1] - f0[1]) / (np.abs(f0[1]) + np.abs(f0[0]))).max())
            d_dm = float((np.abs(f1[2] - f0[2]) / (np.abs(f0[2]) + np.abs(f0[0]))).max())
            both = np.isfinite(c0) & np.isfinite(c1) & (c0 != 0)
            d_c = float(np.abs(c1[both] / c0[both] - 1.0).max())
            print("continuity", "AB"[which], "x", x, "bound %.2e" % bound, "norm %.2e f %.2e dfdg %.2e dfdmu %.2e coefficients %.2e (%d slots)"
                  % (d_norm, d_f, d_dg, d_dm, d_c, both.sum()))
            assert (np.isfinite(c0) == np.isfinite(c1)).all() and both.sum() >= 24
            assert d_norm <= bound and d_f <= bound
            assert d_dg <= 10 * bound and d_dm <= 10 * bound and d_c <= 10 * bound
    # the range rule is the linear family's
    last = float(nt - 1)
    x = np.array([last, np.nextafter(last, np.inf), -1e-300, np.nan, np.inf, -np.inf, 1e300, -0.0, 0.0])
    nrm = tc.batch_norm(x)
    assert np.isfinite(nrm[0]) and np.isnan(nrm[1:7]).all()
    assert bits(nrm[7:8])[0] == bits(nrm[8:9])[0] and np.isfinite(nrm[7])
    # a bad row's line stays inside the set: table 0, the first stencil
    assert tc.row_line(np.nan)[4] == 0 and tc.row_line(-1.0)[4] == 0 and tc.row_line(1e300)[4] == 0


def test_k_overshoot_is_a_nan_row():
    """sin_k = (0, 0, 3, 0, 0, 0) on the knots 0 .. 5: at x = 0.5 the weights are (0.3125, 0.9375, -0.3125, 0.0625), the blended
    k is -0.9375, and the row names no distribution: a NaN normalisation and NaN in every slot.  Its neighbours at the knots,
    and a row whose cubic stays inside [0, 100], are served."""
    gamma, mu, t, k, ends, param = tc.overshoot_set()
    assert tc.set_tables(gamma, mu, t, k, ends, param) == 0
    w, kk, stride, L, base, p = tc.row_line(tc.OVERSHOOT_X)
    assert L.tolist() == [0.3125, 0.9375, -0.3125, 0.0625] and kk == -0.9375 and base == 0 and p == 0.5
    x = np.array([tc.OVERSHOOT_X, 0.0, 1.0, 2.0, 1.5])
    assert tc.row_line(1.5)[1] > 0
    nrm = tc.batch_norm(x)
    assert np.isnan(nrm[0]) and np.isfinite(nrm[1:]).all()
    out = tc.batch(np.full(5, 30.0), np.full(5, 0.9), x, 0x03)[0]
    assert np.isnan(out[0]).all() and np.isfinite(out[1:, :2]).all()
    d, st = tc.mkdist(tc.OVERSHOOT_X)
    assert st != 0


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_set_in_place():
    """Fewer than four tables; knots that are not monotonic, not finite, equal; every refusal of the linear entry (what
    rimphony_ctx_set_tables_2d_nodes refuses, tab2d_nodes_bind.refused_cases, and what rimphony_ctx_set_tables_2d_ends refuses of
    the ends).  A param of the wrong length is the mirrors' to refuse: the C entry reads n_tables words."""
    from rimphony_amd import api
    gamma_n, mu_n, t, k, ends, param = install(1)
    before = tc.blob()
    for n in (1, 2, 3):
        assert tc.set_tables(gamma_n, mu_n, t[:n], k[:n], ends, param[:n]) == -1, n
        assert tc.set_tables(gamma_n, mu_n, t[:n], None, ends, None) == -1, n
        with pytest.raises(ValueError):
            api.TabulatedFamily2D(gamma_n, mu_n, t[:n], blend="cubic")
    bad_params = dict(up_then_down=[0.0, 1.0, 2.0, 1.5, 3.0, 4.0], down_then_up=[5.0, 4.0, 3.0, 3.5, 2.0, 1.0], equal=[0.0, 1.0, 1.0, 2.0, 3.0, 4.0],
                      first_pair_equal=[1.0, 1.0, 2.0, 3.0, 4.0, 5.0], nan=[0.0, 1.0, np.nan, 3.0, 4.0, 5.0], inf=[0.0, 1.0, 2.0, 3.0, 4.0, np.inf],
                      minus_inf=[-np.inf, 1.0, 2.0, 3.0, 4.0, 5.0], nan_first=[np.nan, 1.0, 2.0, 3.0, 4.0, 5.0])
    for name, bad in bad_params.items():
        assert tc.set_tables(gamma_n, mu_n, t, k, ends, np.array(bad)) == -1, name
        with pytest.raises(ValueError):
            api.TabulatedFamily2D(gamma_n, mu_n, t, k, bad, blend="cubic")
    for wrong_length in (param[:5], np.append(param, 2.0)):
        with pytest.raises(ValueError):
            api.TabulatedFamily2D(gamma_n, mu_n, t, k, wrong_length, blend="cubic")
    cases = tn.refused_cases(gamma_n, mu_n, t, k)
    assert len(cases) >= 20
    for name, (g, m, tt, kk, shape) in cases.items():
        assert tc.set_tables(g, m, tt, kk, ends, None, shape) == -1, name
    for bad_ends in ((2, 0), (0, -1), (0, 2), (7, 7)):
        assert tc.set_tables(gamma_n, mu_n, t, k, bad_ends, param) == -1, bad_ends
    assert tc.blob().tobytes() == before.tobytes()
    # n_tables = 0 clears
    assert tc.set_tables(None, None, np.zeros((0, 8, 8)), None) == 0 and len(tc.blob()) == 0


# ---- 9. the laid-out set -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["A", "B"])
def test_blob_is_the_linear_familys_set_and_the_knots(which):
    """tables_blob() minus its trailing knots is the linear family's set on the same data, compared as integers; the knots
    follow, as given -- or 0, 1, 2 .. for a null param."""
    gamma_n, mu_n, t, k, ends, param = install(which)
    nt = len(t)
    cb = tc.blob()
    assert tf.set_tables(gamma_n, mu_n, t, k, ends) == 0
    lb = tf.blob()
    assert len(cb) == len(lb) + nt and (bits(cb[:-nt]) == bits(lb)).all()
    assert (bits(cb[-nt:]) == bits(param)).all()
    assert tc.set_tables(gamma_n, mu_n, t, k, ends, None) == 0
    cb = tc.blob()
    assert (bits(cb[:-nt]) == bits(lb)).all() and cb[-nt:].tolist() == list(range(nt))
