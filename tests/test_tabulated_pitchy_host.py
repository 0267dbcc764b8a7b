"""The sin^k xi prefactor of the tabulated distribution without a GPU: the C entry rimphony_ctx_set_tables_pitchy and its
mirrors, what the host check refuses, sin_k = NULL as the pitch form to the byte, all eight coefficients against the
ANALYTIC pitchy power law of oracle/ (kind 2, which shares no code with the tables) and against an analytic sin^k beam
(tests/support/pitchy_beam_oracle.cpp), P against the closed forms, the limit k = 0 and consistent derivatives.  The
library's side is the sin^k table oracle (tests/support/liboracle_tabpitchy.so): the host build of the device functions
and of rim_tab_check_pitchy / rim_tab_build_pitchy, with P by the oracle's QAG on the device's integrand.  CPU only.

Every bound marked MEASURED is 4 x a figure measured on the host build against the reference named there (every test
prints its figure, `pytest -s`)."""
import ctypes
import os
import re

import mpmath
import numpy as np
import pytest

import oracle_bind
import tab_bind
import tab_pitch_bind as tp
import tab_pitchy_bind as ty

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_det.npz")
GOLD = os.path.join(ROOT, "tests", "golden", "symphony-powerlaw.txt")
mp = mpmath.mp
MARGIN = 4.0
EDGE_LO, EDGE_HI = 1.01, 1e4
ENTRY = "rimphony_ctx_set_tables_pitchy"
PL_P, PL_CUT, PL_LO, PL_HI, PL_NODES = 2.5, 1e10, 1.0, 1e12, 2048      # the table of test_tabulated_power_law_against_kind_0


def ulps(a, b):
    return np.abs(a - b) / np.spacing(np.abs(b))


def check(name, got, measured):
    print(name, "measured", got, "recorded", measured)
    assert measured is not None, "no figure recorded for %s: measured %r" % (name, got)
    assert got <= MARGIN * measured, (name, got, measured)


# ---- 1. the entry, its mirrors and the refusals ------------------------------------------------------------------------
def test_entry_in_library_header_and_mirrors():
    from rimphony_amd import _build, api, capi
    _build.build_hip()
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert hasattr(lib, ENTRY)
    fn = getattr(lib, ENTRY)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                   ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(None, 0, 0, 1.0, 2.0, None, 0, None, None) == -1      # a null context is refused before anything is touched
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    assert re.search(r"int rimphony_ctx_set_tables_pitchy\(rimphony_ctx \*ctx, size_t n_tables, size_t n_nodes, double gamma_lo, "
                     r"double gamma_hi,\s+const double \*log_n, size_t n_mu, const double \*log_g, const double \*sin_k\);", hdr)
    assert "pitchy_pl.rs:56-61" in hdr                              # what d f / d mu gives at |mu| = 1 is said there
    assert ENTRY in capi.SYMBOLS
    rs = open(os.path.join(ROOT, "rimphony-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn rimphony_ctx_set_tables_pitchy\(", rs)
    hpp = open(os.path.join(ROOT, "rimphony_amd", "cxx", "rimphony.hpp")).read()
    assert ENTRY in hpp and re.search(r"TabulatedDistribution\(double gamma_lo, double gamma_hi, std::vector<double> log_n, "
                                      r"std::vector<double> log_g, double sin_k\)", hpp)
    d = api.TabulatedDistribution(1.0, 10.0, np.zeros(8), sin_k=1.5)
    assert d.sin_k.tolist() == [1.5] and d.log_g is None
    d = api.TabulatedDistribution.from_function(lambda g: g ** -2.0, 1.0, 10.0, n_nodes=16, pitch_fn=np.exp, n_mu=9, sin_k=0.5)
    assert d.sin_k.tolist() == [0.5] and d.log_g.shape == (1, 9)
    assert api.TabulatedDistribution(1.0, 10.0, np.zeros(8)).sin_k is None


def test_refusals_without_a_gpu():
    """Each through the library's own host check (rim_tab_check_pitchy, reached as the table oracle applies it) and through
    the Python mirror, which raises before the call."""
    from rimphony_amd import api
    t = tab_bind.edge_tables(EDGE_LO, EDGE_HI, 16)
    g = ty.set_b_rows(8)
    assert ty.set_tables(EDGE_LO, EDGE_HI, t, g, [0.5, 1.0, 100.0]) == 0
    before = ty.blob()
    for bad in (-0.5, -1e-300, np.nan, np.inf, -np.inf, 100.00000000000001, 1e300):
        k = [0.5, bad, 2.0]
        assert ty.set_tables(EDGE_LO, EDGE_HI, t, g, k) == -1, bad
        assert ty.set_tables(EDGE_LO, EDGE_HI, t, None, k) == -1, bad
        with pytest.raises(ValueError):
            api.check_sin_k(k, 3)
        with pytest.raises(ValueError):
            api.TabulatedDistribution(EDGE_LO, EDGE_HI, t[0], sin_k=bad)
    # one of log_g and n_mu without the other
    assert ty.set_tables(EDGE_LO, EDGE_HI, t, g, [0.5, 1.0, 2.0], n_mu=0) == -1
    assert ty.set_tables(EDGE_LO, EDGE_HI, t, None, [0.5, 1.0, 2.0], n_mu=8) == -1
    with pytest.raises(ValueError):
        api.check_pitch_tables(EDGE_LO, EDGE_HI, t, None, n_mu=8)
    with pytest.raises(ValueError):
        api.check_pitch_tables(EDGE_LO, EDGE_HI, t, g, n_mu=0)
    # sin_k of the wrong length: the mirror's check (C cannot see the length of an array)
    for k in ([0.5, 1.0], [0.5, 1.0, 2.0, 3.0], np.zeros((3, 1)), []):
        with pytest.raises(ValueError):
            api.check_sin_k(k, 3)
    assert api.check_sin_k(1.5, 3).tolist() == [1.5, 1.5, 1.5]
    assert api.check_sin_k([0.0, 100.0, -0.0], 3).tolist() == [0.0, 100.0, 0.0]
    # what the pitch form refuses is refused here too
    bad_g = g.copy()
    bad_g[1, 3] = np.nan
    assert ty.set_tables(EDGE_LO, EDGE_HI, t, bad_g, [0.5, 1.0, 2.0]) == -1
    assert ty.set_tables(EDGE_LO, EDGE_HI, t[:, :7], None, [0.5, 1.0, 2.0]) == -1
    assert ty.blob().tobytes() == before.tobytes()                  # the previous set stayed


def test_null_sin_k_is_the_pitch_form_to_the_byte():
    t = tab_bind.edge_tables(EDGE_LO, EDGE_HI, 64)
    for g in (None, ty.set_b_rows(8), ty.set_b_rows(257)):
        assert tp.set_tables(EDGE_LO, EDGE_HI, t, g) == 0
        assert ty.set_tables(EDGE_LO, EDGE_HI, t, g, None) == 0
        assert ty.blob().tobytes() == tp.blob().tobytes() and len(ty.blob()) > 8
    # ... and the layout of the new form: the pitch form's gamma rows, then a 64-byte header per table
    assert ty.set_tables(EDGE_LO, EDGE_HI, t, None, [0.5, 2.0, 0.0]) == 0
    b = ty.blob()
    assert tab_bind.set_tables(EDGE_LO, EDGE_HI, t) == 0
    iso = tab_bind.blob()
    assert len(b) == len(iso) + 3 * 8 and b[:len(iso)].tobytes() == iso.tobytes()
    assert [b[len(iso) + 8 * k] for k in range(3)] == [0.5, 2.0, 0.0]
    assert ty.set_tables(EDGE_LO, EDGE_HI, t, ty.set_b_rows(8), [1.5, 0.3, 3.0]) == 0
    b = ty.blob()
    assert len(b) == len(iso) + 3 * (8 + 16) and b[7] == 8.0


# ---- 2. against the analytic pitchy power law ----------------------------------------------------------------------------
def pl_rows():
    rows = np.load(FIXTURE)["pl_rows"]
    assert len(rows) == 16
    gold = np.loadtxt(GOLD)
    return gold[rows, 0].copy(), gold[rows, 1].copy()


def pl_table():
    return tab_bind.log_n_powerlaw(tab_bind.nodes(PL_LO, PL_HI, PL_NODES), PL_P, PL_CUT)


# max over the 16 rows and 8 slots of |table / analytic - 1|: the 2048-node straight-line table times sin^k xi against
# oracle/liboracle.so's kind 2.  (The isotropic table against kind 0 measured 3.5e-13.)
# Recorded in tab_pitchy_bind.py, because the GPU test of the same comparison uses the same figure.
MEASURED_KIND2 = ty.MEASURED_KIND2


@pytest.mark.parametrize("k", sorted(MEASURED_KIND2))
def test_against_analytic_kind_2(k):
    L = oracle_bind.load()
    s, th = pl_rows()
    n = len(s)
    ref = oracle_bind.batch(L, 2, s, th, [np.full(n, PL_P), np.full(n, k), np.full(n, PL_LO), np.full(n, PL_HI), np.full(n, PL_CUT)],
                            nthreads=16)
    assert ty.set_tables(PL_LO, PL_HI, pl_table(), None, [k]) == 0
    tab = ty.batch(s, th, np.zeros(n), nthreads=16)[0]
    assert np.isfinite(ref).all() and np.isfinite(tab).all() and tab.shape == (16, 8)
    rel = np.abs(tab / ref - 1.0)
    print("k", k, "max rel per slot", rel.max(axis=0))
    check("kind 2, k = %g" % k, rel.max(), MEASURED_KIND2[k])
    assert max(v for v in MEASURED_KIND2.values()) <= 1e-11


# ---- 3. P ---------------------------------------------------------------------------------------------------------------
P_KS = (0.01, 0.1, 0.5, 1.0, 1.7, 2.5, 3.0, 100.0)
# max over the k above of |P_quadrature / P_closed - 1|, a flat row of n_mu nodes; the quadrature is asked for 1e-8
MEASURED_P_FLAT = {8: 2.9e-11, 257: 2.9e-11}


def closed_p(k):
    """Gamma(3/2) Gamma(1 + k/2) / Gamma(3/2 + k/2), 40 digits"""
    k = mp.mpf(k)
    return mp.gamma(mp.mpf(3) / 2) * mp.gamma(1 + k / 2) / mp.gamma(mp.mpf(3) / 2 + k / 2)


def test_closed_form_p_without_g():
    flat = np.zeros((len(P_KS), 8))
    assert ty.set_tables(1.0, 1e3, flat, None, P_KS) == 0
    for i, k in enumerate(P_KS):
        kk, p = ty.table_k_p(i)
        assert kk == k
        err = float(abs(mp.mpf(p) / closed_p(k) - 1))
        print("k", k, "closed form against mpmath", err)
        assert err <= 64 * 2.0 ** -52            # three lgamma of arguments up to 51.5 and one exp: a few ulp of the exponent
    assert ty.p_intervals() == 0
    assert ty.set_tables(1.0, 1e3, flat[:1], None, [0.0]) == 0 and ty.table_k_p(0) == (0.0, 1.0)


@pytest.mark.parametrize("n_mu", sorted(MEASURED_P_FLAT))
def test_p_by_quadrature_on_a_flat_row(n_mu):
    flat = np.zeros((len(P_KS), 8))
    assert ty.set_tables(1.0, 1e3, flat, np.zeros((len(P_KS), n_mu)), P_KS) == 0
    worst = 0.0
    for i, k in enumerate(P_KS):
        p = ty.table_k_p(i)[1]
        assert np.isfinite(p)
        worst = max(worst, float(abs(mp.mpf(p) / closed_p(k) - 1)))
    print("n_mu", n_mu, "subintervals at most", ty.p_intervals())
    assert 0 < ty.p_intervals() <= 100
    check("P flat n_mu %d" % n_mu, worst, MEASURED_P_FLAT[n_mu])
    assert MARGIN * MEASURED_P_FLAT[n_mu] <= 1e-8


MEASURED_P_BEAM = {(1.0, 1.5): 1.8e-11, (-0.7, 0.5): 1.2e-11}


@pytest.mark.parametrize("a,k", sorted(MEASURED_P_BEAM))
def test_p_of_a_straight_line_row(a, k):
    """G = a mu on 8 nodes, which the spline reproduces exactly: P = 1/2 sqrt(pi) Gamma(k/2 + 1) (2/|a|)^((k+1)/2)
    I_((k+1)/2)(|a|)."""
    assert ty.set_tables(1.0, 1e3, np.zeros((1, 8)), tp.log_g_beam(8, a), [k]) == 0
    p = ty.table_k_p(0)[1]
    nu = (mp.mpf(k) + 1) / 2
    want = mp.sqrt(mp.pi) / 2 * mp.gamma(mp.mpf(k) / 2 + 1) * (2 / mp.mpf(abs(a))) ** nu * mp.besseli(nu, abs(a))
    beam_p = ty.beam().pbeamo_pitch_integral(a, k)
    print("a", a, "k", k, "analytic oracle's own P against mpmath", float(abs(mp.mpf(beam_p) / want - 1)))
    assert float(abs(mp.mpf(beam_p) / want - 1)) < 1e-10
    check("P beam a = %g k = %g" % (a, k), float(abs(mp.mpf(p) / want - 1)), MEASURED_P_BEAM[(a, k)])
    assert MARGIN * MEASURED_P_BEAM[(a, k)] <= 1e-8


# ---- 4. against the analytic sin^k beam ----------------------------------------------------------------------------------
# max over the kept rows and 8 slots of |table / analytic - 1|; P's quadrature tolerance, 1e-8, is the floor
MEASURED_BEAM = {(1.0, 1.5): 1.8e-11, (-0.7, 0.5): 1.2e-11}


@pytest.mark.parametrize("a,k", sorted(MEASURED_BEAM))
def test_against_the_analytic_sin_k_beam(a, k):
    """The 2048-node table of gamma^-2.5 exp(-gamma / 1e10) with G = a mu on 8 nodes and sin^k xi, all eight slots, against
    liboracle_pitchy_beam; both signs of a, so that a mirrored mu or a wrong sign of either term of d f / d mu shows."""
    s, th = pl_rows()
    ref = ty.beam_batch(s, th, [PL_P, PL_LO, PL_HI, PL_CUT, a, k], nthreads=16)
    keep = np.isfinite(ref).all(axis=1)
    print("a", a, "k", k, "rows kept", keep.sum(), "of 16")
    assert keep.sum() >= 12
    s, th, ref = s[keep], th[keep], ref[keep]
    assert ty.set_tables(PL_LO, PL_HI, pl_table(), tp.log_g_beam(8, a), [k]) == 0
    tab = ty.batch(s, th, np.zeros(len(s)), nthreads=16)[0]
    assert np.isfinite(tab).all()
    rel = np.abs(tab / ref - 1.0)
    print("max rel per slot", rel.max(axis=0))
    check("beam a = %g k = %g" % (a, k), rel.max(), MEASURED_BEAM[(a, k)])
    assert MARGIN * MEASURED_BEAM[(a, k)] < 1e-8


# ---- 5. k = 0 --------------------------------------------------------------------------------------------------------------
def test_k_zero_is_the_pitch_form():
    """sin^0 = 1: f and d f / d gamma within 4 ulp of the pitch form's (no g, and the rows of set B), d f / d mu +-0 where
    the pitch form's is 0 and its bits elsewhere, the normalisation within 4 ulp without g.  At mu = +-1 the term
    k mu / sin^2 xi is 0 / 0: d f / d mu is NaN there for every k, as the header says."""
    t = tab_bind.edge_tables(EDGE_LO, EDGE_HI, 64)
    rng = np.random.default_rng(5)
    gamma = np.concatenate([np.exp(rng.uniform(np.log(EDGE_LO), np.log(EDGE_HI), 2000)), [EDGE_LO, EDGE_HI, 1.0, 2e4, 3.0, 3.0]])
    mu = np.concatenate([rng.uniform(-1, 1, 2000), [-0.5, 0.5, 0.0, 0.3, -1.0, 1.0]])
    ends = np.abs(mu) == 1.0
    for g in (None, ty.set_b_rows(8)):
        assert tp.set_tables(EDGE_LO, EDGE_HI, t, g) == 0
        ref = [tp.dev_calc_f([float(k)], 1.0, gamma, mu) for k in range(3)]
        ref_norm = tp.batch_norm([0.0, 1.0, 2.0])
        assert ty.set_tables(EDGE_LO, EDGE_HI, t, g, [0.0, 0.0, 0.0]) == 0
        norm = ty.batch_norm([0.0, 1.0, 2.0])
        for k in range(3):
            f, dfdg, dfdcx = ty.dev_calc_f([float(k)], 1.0, gamma, mu)
            live = ref[k][0] != 0
            assert live[:2000].any() and (f[~live] == 0).all() and (dfdg[~live] == 0).all()
            assert ulps(f[live], ref[k][0][live]).max() <= 4 and ulps(dfdg[live], ref[k][1][live]).max() <= 4
            assert np.isnan(dfdcx[ends]).all()
            zero = (ref[k][2] == 0) & ~ends
            assert (dfdcx[zero] == 0).all() and zero.sum() >= (2000 if g is None else 2)
            rest = ~zero & ~ends
            assert ulps(dfdcx[rest], ref[k][2][rest]).max() <= 4 if rest.any() else True
            print("g" if g is not None else "no g", "table", k, "norm in ulp", ulps(norm[k], ref_norm[k]))
            if g is None:
                assert ulps(norm[k], ref_norm[k]) <= 4
            else:
                assert abs(norm[k] / ref_norm[k] - 1) <= 1e-8       # P by the adaptive rule against the fixed one


# ---- 6. derivatives -----------------------------------------------------------------------------------------------------
# Measured with the one-sided difference quotient of step 1e-6 on the three tables of set B: max over the draws of
# |analytic - numeric| / |numeric|, the reference's form, and for d f / d mu also of |analytic - numeric| / (f T) with
# T = |G'| + k mu / (1 - mu^2), the two terms of d ln f / d mu without their cancellation ("dfdcx_scaled").  What is measured
# is the truncation error of the quotient, 1e-6 / 2 x |f'' / f'|, not an error of the derivative.  On every table of set B
# G' - k mu / (1 - mu^2) has a zero inside the range of the draws, where the relative form has a pole (the reference's own
# factor alone has none): the relative form is taken over the draws where the two terms cancel to no less than a tenth,
# |G' - k mu / (1 - mu^2)| >= T / 10; the scaled form covers every draw.  G' comes from the pitch form's oracle, not from
# the code under test.  4 x the figure of d f / d mu is above the reference's own tolerance of 1e-4 (the quotient's truncation
# error at mu near 0.99, where k mu / (1 - mu^2) is steep): there 1e-4, the smaller of the two, is the bound.
MEASURED_FD = dict(dfdg=1.3e-6, dfdcx=3.9e-5, dfdcx_scaled=3.3e-5)
FD_TOL = 1e-4


def test_derivatives_of_set_b():
    """The finite-difference check of pitchy_pl.rs:203-238 (norm 1, step 1e-6, gamma = 1.1 + 1e3 u, cos xi = 0.01 + 0.98 u,
    100 seeded draws per table) on the tables of set B, for both derivatives; the bounds are 4 x the measured figures and
    the reference's own 1e-4, whichever is smaller."""
    EPS = 1e-6
    lo, hi, t, g, k = ty.fixture_set(1)
    assert tp.set_tables(lo, hi, t, g) == 0
    assert ty.set_tables(lo, hi, t, g, k) == 0
    worst = dict(dfdg=0.0, dfdcx=0.0, dfdcx_scaled=0.0)
    for table in range(3):
        rng = np.random.default_rng(60 + table)
        gamma = 1.1 + 1e3 * rng.random(100)
        cx = 0.01 + 0.98 * rng.random(100)
        pf, _, pdfdcx = tp.dev_calc_f([float(table)], 1.0, gamma, cx)
        dG = pdfdcx / pf
        sink = k[table] * cx / (1.0 - cx * cx)
        total, both = dG - sink, np.abs(dG) + sink
        away = np.abs(total) >= 0.1 * both
        f0, dfdg, dfdcx = ty.dev_calc_f([float(table)], 1.0, gamma, cx)
        f1, _, _ = ty.dev_calc_f([float(table)], 1.0, gamma + EPS, cx)
        f2, _, _ = ty.dev_calc_f([float(table)], 1.0, gamma, cx + EPS)
        assert (f0 > 1e-250).all() and (dfdcx != 0).all() and away.sum() >= 80
        assert (np.sign(dfdcx[away]) == np.sign(total[away])).all() and (total > 0).any() and (total < 0).any()
        num_g, num_c = (f1 - f0) / EPS, (f2 - f0) / EPS
        eg, ec = np.abs((dfdg - num_g) / num_g), np.abs((dfdcx - num_c) / num_c)[away]
        es = np.abs(dfdcx - num_c) / (f0 * both)
        print("table", table, "kept", away.sum(), "dfdg", eg.max(), "dfdcx", ec.max(), "scaled", es.max())
        worst["dfdg"] = max(worst["dfdg"], eg.max())
        worst["dfdcx"] = max(worst["dfdcx"], ec.max())
        worst["dfdcx_scaled"] = max(worst["dfdcx_scaled"], es.max())
    for key in worst:
        check(key, worst[key], MEASURED_FD[key])
        assert worst[key] < FD_TOL, (key, worst[key])
