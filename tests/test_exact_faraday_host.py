"""The Faraday pair of the four analytic kinds against the converged Heyvaerts integrals (tests/exact_faraday.py), CPU side: the
reference against its mpmath twin (elements, inner integrals, one whole coefficient pair with the domain stated again), its outer
rule against an adaptive one, the stored fixture against its generator, both oracle flavours against the stored exact values within the stored bounds, and
mutated oracles that must miss them.

The bounds are those of tools/make_exact_faraday_fixture.py: 2 max(|det / exact - 1|, |libm / exact - 1|) + 100 x the relative
error estimate of the exact value, measured on the CPU oracle (profiles/exact_faraday_deviation.txt)."""
import ctypes
import importlib.util
import math
import os
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
from scipy import integrate

import exact_faraday as ef
import exact_symphony as ex
import oracle_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = range(4)
PITCH_COLUMN = {2: 1, 3: 2}


@pytest.fixture(scope="module")
def fix():
    return ef.load_fixture()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.view(np.uint64) == b.view(np.uint64)


def rows_of(fix, kind, cls=None):
    m = fix["row_kind"] == kind
    if cls is not None:
        m &= fix["row_class"] == cls
    return np.flatnonzero(m)


def coefficient_deviation(fix, L, kind):
    """per record of the kind: (record index, |oracle / exact - 1|, oracle value)"""
    rows = rows_of(fix, kind)
    s, theta, params = ef.row_inputs(fix, rows)
    out = oracle_bind.batch(L, kind, s, theta, params, ef.MASK, 8)
    rec = np.flatnonzero(np.isin(fix["rec_row"], rows))
    got = out[np.searchsorted(rows, fix["rec_row"][rec]), 6 + fix["rec_slot"][rec]]
    with np.errstate(all="ignore"):
        return rec, ef.deviation(got, fix["rec_exact"][rec]), got


def inner_values(fix, L, rec):
    out = np.empty(len(rec))
    for j, i in enumerate(rec):
        row = int(fix["in_row"][i])
        d, st = oracle_bind.mkdist(L, int(fix["row_kind"][row]), ef.row_params(fix, row))
        assert st == 0
        out[j] = L.rimo_hey_outer_integrand(ctypes.byref(d), int(fix["in_stokes"][i]), fix["row_s"][row], fix["row_theta"][row],
                                            int(fix["in_qr"][i]), fix["in_u"][i])
    return out


def generator():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location("make_exact_faraday_fixture", os.path.join(ROOT, "tools", "make_exact_faraday_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_is_whole(fix):
    """Every stored value is finite, every row of the generator's list is there with both slots, the error estimates are within
    1e-9 (coefficients) and 1e-8 (inner integrals), the bounds follow the rule, and the rows cover what they are there for: per
    kind five rows of each class, class A with sigma0 in [4, 40], class B with sigma0 < 3, theta > pi / 2, theta near 0.1; a hard
    gamma_max well below the cut-off for the power-law kinds; k from 0.5 to 3 and a visible mu term for the pitch-angle kinds;
    inner integrals on both sides of sigma = 3 and between 3 and the g = 10 root."""
    for k, v in fix.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), k
    gen = generator()
    assert len(gen.ROWS) == len(fix["row_kind"]) == 40 and len(fix["rec_row"]) == 80
    for i, (kind, par, s, theta, cls) in enumerate(gen.ROWS):
        assert (kind, s, theta, cls) == (fix["row_kind"][i], fix["row_s"][i], fix["row_theta"][i], fix["row_class"][i])
        assert par == ef.row_params(fix, i)
        assert sorted(fix["rec_slot"][fix["rec_row"] == i]) == [0, 1]
    assert (fix["rec_err"] <= 1e-9 * np.abs(fix["rec_exact"])).all()
    assert (fix["in_err"] <= 1e-8 * np.abs(fix["in_exact"])).all() and (fix["in_exact"] != 0.).all()
    for pre in ("rec", "in"):
        bound = 2. * np.maximum(fix[pre + "_dev_det"], fix[pre + "_dev_libm"]).astype(np.float64) + 100. * fix[pre + "_err"] / np.abs(fix[pre + "_exact"])
        assert np.allclose(fix[pre + "_bound"], bound, rtol=1e-6, atol=0.)          # the deviations are stored in single precision
    sigma0 = fix["row_s"] * np.sin(fix["row_theta"])
    for kind in KINDS:
        a, b = rows_of(fix, kind, "A"), rows_of(fix, kind, "B")
        assert len(a) == 5 and len(b) == 5
        assert ((sigma0[a] >= 4.) & (sigma0[a] <= 40.)).all()
        assert (sigma0[b] < 3.).sum() >= 2 and (fix["row_theta"][b] > 0.5 * math.pi).any() and (np.abs(fix["row_theta"][b] - 0.1) <= 0.02).any()
        assert ((sigma0[b] < 3.) & (fix["row_theta"][b] > 0.5 * math.pi)).any()
        rec = np.flatnonzero(np.isin(fix["in_row"], np.concatenate([a, b])))
        assert len(rec) == 40
        u = fix["in_u"][rec[fix["in_qr"][rec] == 1]]
        assert (u < 3.).any() and ((u > 3.) & (u < ef.SIGMA_G10)).any() and (u > ef.SIGMA_G10).any()
    for kind, (g_max, g_cut) in ((0, (2, 3)), (2, (3, 4))):
        b = rows_of(fix, kind, "B")
        assert (fix["row_params"][b, g_max] < 0.5 * fix["row_params"][b, g_cut]).any()
    for kind, col in PITCH_COLUMN.items():
        r = rows_of(fix, kind)
        k = fix["row_params"][r, col]
        assert k.min() == 0.5 and k.max() == 3. and (k != np.round(k)).any()
        rec = np.flatnonzero(np.isin(fix["rec_row"], r))
        share = np.abs(1. - fix["rec_nomu"][rec] / fix["rec_exact"][rec])
        assert (share > 20. * fix["rec_bound"][rec]).all(), share.min()


ELEMENTS_MP = [
    # kind, parameters, s, theta, quasi-resonant, fixed, variable
    (1, [1.], 12., 0.2, 1, 2.6, 0.9),             # J/Y form, sigma < 3
    (1, [1.], 12., 0.2, 1, 2.6, 0.1),             # I form at the same sigma
    (3, [4., 2., 0.5, 20.], 6., 2.7, 1, 3.01, -1.567),    # between sigma = 3 and the g = 10 root, upper hemisphere, k = 0.5
    (2, [3., 2.4, 1.05, 1000., 10.], 8., 0.7, 1, 9., 4.),
    (2, [3., 1.3, 1.05, 1000., 10.], 6., 1.0, 0, -7., 11.),
    (3, [5., 1., 2.4, 10.], 25., 0.1, 0, 3.1, 3.99),      # next to x = 0: mu near 1
    (0, [3.5, 1.5, 20., 100.], 10., 2.2, 0, 9., 14.),
]


def dominant_term(stokes, geo, pomega):
    """the largest of the terms whose sum is a quasi-resonant kernel: pi (2 pomega^2 + sigma0^2) / sqrt R / c_l of Q, 2 pi |pomega| / c_l
    of V.  The other terms all but cancel it where g is large."""
    if stokes == ef.STOKES_Q:
        return math.pi * (2. * pomega * pomega + geo.sigma0_sq) / np.sqrt(pomega * pomega + geo.sigma0_sq) / ef.C
    return 2. * math.pi * np.abs(pomega) / ef.C


@pytest.mark.parametrize("kind,par,s,theta,qr,fixed,v", ELEMENTS_MP)
def test_element_against_mpmath(kind, par, s, theta, qr, fixed, v):
    """The integrand in double precision against the 30-digit twin, which forms I_(-nu) - I_nu, x^2, gamma^2 - 1 and 1 - mu^2 by
    their defining subtractions and d mu / d sigma by the quotient rule, with and without the mu term: 1e-12 of the value for a
    non-resonant element, 1e-13 of the dominant term for a quasi-resonant one (a sum that cancels: a few ulp of scipy's Bessel
    functions on each term is all a double-precision evaluation can give)."""
    from mpmath import mp
    dist = ex.make(kind, par)
    geo = ef.Geometry(s, theta)
    for stokes in (ef.STOKES_Q, ef.STOKES_V):
        for mu_term in (True, False):
            got = float(ef.element(dist, stokes, s, theta, qr, fixed, v, mu_term))
            with mp.workdps(30):
                ref = float(ef.element_mp(dist, stokes, s, theta, qr, fixed, v, 30, mu_term))
            tol = 1e-12 * abs(ref)
            if qr:
                x2 = fixed * fixed - v * v - geo.sigma0_sq
                tol = 1e-13 * max(abs(ref), float(dominant_term(stokes, geo, v) * abs(ef.dfdsigma(dist, geo, fixed, v, x2, mu_term))))
            assert ref != 0. and abs(got - ref) <= tol, (stokes, mu_term, got / ref - 1.)


def test_size_of_the_seam_at_g_10():
    """The g = 10 seam itself: the I form and the J/Y form of the quasi-resonant kernels on the curve g = 10, over the sigma that
    reach it (below 3.0197), against the dominant term.  There x is a few per cent of sigma.  As x -> 0 the exact products tend
    to x^2 J' Y' -> sigma / pi and -J Y -> 1 / (pi sigma), whose terms cancel the third one exactly on x = 0: the J/Y form is a
    small remainder (1e-5 of the dominant term for Q).  The I form is the expansion about x = sigma; this far from it its terms
    do not cancel: the Q kernel is of the order of the dominant term itself (0.6 ... 2 times it) and the V kernel is
    pi Y(10) - 1 = -1.7 % of it, against -0.02 ... -0.08 % in the J/Y form.  So the integrand of the reference's algorithm jumps
    by far more than its own size on the J/Y side across the seam for sigma < 3.02; the project reproduces the jump bit for bit
    and the exact integrals carry it.  DESIGN section 2 records the figures printed here."""
    sigma = np.array([0.8, 1.5, 2.2, 2.9, 3.01])
    x = ef._x10(sigma)
    geo = ef.Geometry(2., 0.3)
    pomega = np.sqrt(sigma * sigma - geo.sigma0_sq - x * x)
    for stokes in (ef.STOKES_Q, ef.STOKES_V):
        i_form = ef._qr_kernel(stokes, geo, sigma, pomega, (x * (1. + 1e-9)) ** 2) / dominant_term(stokes, geo, pomega)
        jy_form = ef._qr_kernel(stokes, geo, sigma, pomega, (x * (1. - 1e-9)) ** 2) / dominant_term(stokes, geo, pomega)
        print("g = 10 seam, stokes %d, x / sigma = %r:\n  I form / dominant term = %r\n  J/Y form / dominant term = %r" % (stokes, x / sigma, i_form, jy_form))
        assert (np.abs(jy_form) < 1e-2).all() and (np.abs(i_form) > 10. * np.abs(jy_form)).all()


INNER_MP = [(1, [1.], 12., 0.2, 1, 2.69), (1, [1.], 12., 0.2, 1, 3.0099), (3, [4., 2., 0.5, 20.], 12., 0.2, 1, 2.99),
            (2, [3.5, 3., 1.5, 20., 100.], 10., 2.2, 0, -12.), (0, [3.5, 1.5, 20., 100.], 10., 2.2, 1, 14.)]


@pytest.mark.parametrize("kind,par,s,theta,qr,u", INNER_MP)
def test_inner_integral_against_mpmath(kind, par, s, theta, qr, u):
    """One outer-integrand sample against tanh-sinh quadrature of the twin's integrand at 30 digits: 1e-10, error estimate
    included.  The cases: wholly in the J/Y form with both ends on x = 0, the three pieces between 3 and the g = 10 root,
    x^(k - 2) at k = 0.5, hard gamma limits inside the range, upper hemisphere."""
    dist = ex.make(kind, par)
    for stokes in (ef.STOKES_Q, ef.STOKES_V):
        got, err = ef.inner_integral(dist, stokes, s, theta, qr, [u])
        ref = ef.inner_integral_mp(dist, stokes, s, theta, qr, u, 30)
        assert ref != 0. and abs(got[0] - ref) <= 1e-10 * abs(ref) and err[0] <= 1e-10 * abs(ref), (stokes, got[0] / ref - 1., err[0] / ref)


def test_coefficient_against_mpmath_twin(fix):
    """One whole coefficient pair against the mpmath twin, exact_faraday.coefficients_mp: 20-digit inner integrals of element_mp,
    and a second statement in mpmath of everything the double-precision path takes from its own helpers -- the quasi-resonant
    lower limit, both pomega limits, the g = 10 root, where the non-resonant range is empty, the cut-off lines, the pieces of
    the outer variable and the factor 2 e^2 / (m_e sigma0^2) -- with a plain Gauss-Legendre rule per outer piece.  A cold thermal
    point with sigma0 < 3.  The twin's 768 inner integrals take minutes on one core, so its value is stored by the fixture tool
    (which refuses to write beyond 1e-8) and computed again only by the slow test below; the double-precision value is computed here: 1e-8."""
    kind, par, s, theta = int(fix["mp_kind"]), list(fix["mp_params"]), float(fix["mp_s"]), float(fix["mp_theta"])
    assert s * math.sin(theta) < 3.
    dist = ex.make(kind, par)
    for i, stokes in enumerate((ef.STOKES_Q, ef.STOKES_V)):
        val = sum(ef.parts(dist, stokes, s, theta, 2, 1.5)) * ef.scale(s, theta)
        assert val == fix["mp_exact"][i]
        assert abs(val / fix["mp_value"][i] - 1.) <= 1e-8, (stokes, val / fix["mp_value"][i] - 1.)


@pytest.mark.slow
@pytest.mark.skipif(not os.environ.get("RIMPHONY_SLOW"), reason="set RIMPHONY_SLOW=1 (five minutes on one core)")
def test_stored_mpmath_twin_is_what_the_twin_gives(fix):
    got = ef.coefficients_mp(int(fix["mp_kind"]), list(fix["mp_params"]), float(fix["mp_s"]), float(fix["mp_theta"]), int(fix["mp_digits"]), int(fix["mp_points"]))
    assert (np.abs(got / fix["mp_value"] - 1.) <= 1e-12).all()


def test_twin_states_the_domain_again():
    """The limits that the twin states in mpmath against the double-precision helpers, at sigma on both sides of every seam."""
    from mpmath import mp
    s, theta = 2., 1.1
    geo = ef.Geometry(s, theta)
    for sigma in (1.7826, 1.9, 2.9, 3.01, 3.5, 12.):
        wmax, wq, w10 = (float(z[0]) for z in ef._qr_limits(geo, np.array([sigma])))
        with mp.workdps(20):
            m_max, m_10 = (float(z) for z in ef._qr_limits_mp(s, theta, sigma))
        assert abs(m_max - wmax) <= 1e-12 * wmax and abs(m_10 - w10) <= 1e-9 * wmax, (sigma, m_max, wmax, m_10, w10)
    dist = ex.make(1, [0.15])
    ghi = dist.cap(1.5)
    for qr, cuts in ((0, ef.nr_outer_cuts(dist, geo, ghi)), (1, ef.qr_outer_cuts(dist, geo, ghi))):
        pieces = ef.outer_pieces_mp(dist, s, theta, qr, ghi)
        ends = sorted({e for piece in pieces for e in piece})
        assert all(min(abs(e - c) for c in cuts) <= 1e-9 * max(1., abs(e)) for e in ends), (qr, ends, cuts)
        assert abs(ends[0] - cuts[0]) <= 1e-9
        if qr:          # the twin ends where gamma > ghi everywhere, a cut of the other; beyond it the other's inner range is empty
            assert ef._inner_qr(dist, ef.STOKES_V, geo, [0.5 * (ends[-1] + cuts[-1])], ef.INNER[1], ghi)[0] == 0.
        else:
            assert abs(ends[-1] - cuts[-1]) <= 1e-9 * cuts[-1]


def test_coefficient_against_adaptive_outer_quadrature():
    """The outer rule alone: QUADPACK's adaptive rule in place of the fixed mapped one, over the same inner integrals, cuts and
    limits (those have their second statement in test_coefficient_against_mpmath_twin).  sigma0 < 3, so the J/Y form, the empty
    non-resonant region and all the seams are inside.  1e-9."""
    dist = ex.make(1, [1.])
    s, theta = 2.5, 1.0
    geo, ghi = ef.Geometry(s, theta), dist.cap(1.5)
    assert geo.sigma0 < 3.
    for stokes in (ef.STOKES_Q, ef.STOKES_V):
        val = sum(ef.parts(dist, stokes, s, theta, 2, 1.5))
        total = 0.
        for inner, cuts in ((ef._inner_nr, ef.nr_outer_cuts(dist, geo, ghi)), (ef._inner_qr, ef.qr_outer_cuts(dist, geo, ghi))):
            for a, b in zip(cuts[:-1], cuts[1:]):
                with warnings.catch_warnings():          # (a piece whose integral is below epsabs ends on round-off: the sum is what is held)
                    warnings.simplefilter("ignore", integrate.IntegrationWarning)
                    total += integrate.quad(lambda u: inner(dist, stokes, geo, [u], ef.INNER[1], ghi)[0], a, b, epsabs=1e-11 * abs(val), epsrel=1e-10, limit=200)[0]
        assert abs(total / val - 1.) <= 1e-9, (stokes, total / val - 1.)


def test_fixture_is_what_the_generator_gives(fix):
    """One row and six inner integrals computed again from the stored inputs: 1e-12."""
    for kind in (3,):
        i = rows_of(fix, kind, "A")[1]
        dist = ex.make(kind, ef.row_params(fix, i))
        for r in np.flatnonzero(fix["rec_row"] == i):
            nr, qr = ef.parts(dist, (ef.STOKES_Q, ef.STOKES_V)[fix["rec_slot"][r]], fix["row_s"][i], fix["row_theta"][i], 2, 1.5)
            val = (nr + qr) * ef.scale(fix["row_s"][i], fix["row_theta"][i])
            assert abs(val / fix["rec_exact"][r] - 1.) <= 1e-12 and abs(qr / (nr + qr) - fix["rec_qr_share"][r]) <= 1e-6
    for i in range(0, len(fix["in_u"]), 27):
        row = int(fix["in_row"][i])
        dist = ex.make(int(fix["row_kind"][row]), ef.row_params(fix, row))
        v, e = ef.inner_integral(dist, int(fix["in_stokes"][i]), fix["row_s"][row], fix["row_theta"][row], int(fix["in_qr"][i]), [fix["in_u"][i]])
        assert abs(v[0] / fix["in_exact"][i] - 1.) <= 1e-12


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_coefficients_within_bounds(fix, oracle, oracle_libm, kind):
    """Both flavours on every record of the kind in one batch each; the deterministic one also carries the stored bits."""
    rec, dev, got = coefficient_deviation(fix, oracle, kind)
    assert len(rec) == 20
    assert same_bits(got, fix["rec_det_bits"][rec].view(np.float64)).all()
    assert (dev <= fix["rec_bound"][rec]).all(), (rec[dev > fix["rec_bound"][rec]], dev.max())
    rec, dev, got = coefficient_deviation(fix, oracle_libm, kind)
    assert (dev <= fix["rec_bound"][rec]).all(), (rec[dev > fix["rec_bound"][rec]], dev.max())


def test_oracle_inner_integrals_within_bounds(fix, oracle, oracle_libm):
    rec = np.arange(len(fix["in_u"]))
    assert len(rec) == 160
    for L in (oracle, oracle_libm):
        got = inner_values(fix, L, rec)
        if L is oracle:
            assert same_bits(got, fix["in_det_bits"].view(np.float64)).all()
        dev = ef.deviation(got, fix["in_exact"])
        assert (dev <= fix["in_bound"]).all(), rec[~(dev <= fix["in_bound"])][:5]


def surface_table(fix):
    from rimphony_amd import api
    T, a, lo, hi, n_nodes, n_mu = ex.surface_inputs(fix)
    dist = ex.tilted_juettner(T, a, lo, hi)
    return dist, api.TabulatedDistribution2DGrid.from_function(
        lambda g, mu: g * np.sqrt(g * g - 1.) * dist.f(g, mu, np), api.grid_nodes_log_gm1(lo, hi, n_nodes), n_mu)


def test_tabulated_surface_within_bounds(fix):
    """The non-separable surface of the Symphony fixture, tabulated and run through the table oracle, against the exact integrals
    of the same f(gamma, mu): df/dmu is alive in every sample and comes from the bicubic spline."""
    import tab2d_grid_bind
    dist, table = surface_table(fix)
    assert tab2d_grid_bind.set_tables(table.gamma, table.log_n) == 0
    out, _ = tab2d_grid_bind.batch(fix["surf_s"].copy(), fix["surf_theta"].copy(), np.zeros(len(fix["surf_s"])), ef.MASK)
    assert same_bits(out[:, 6:], fix["surf_oracle_bits"].view(np.float64)).all()
    dev = ef.deviation(out[:, 6:], fix["surf_exact"])
    assert (fix["surf_bound"] <= 1e-5).all() and (fix["surf_err"] <= 1e-9 * np.abs(fix["surf_exact"])).all()
    assert (dev <= fix["surf_bound"]).all(), dev / fix["surf_bound"]


# (what, old text of oracle/rimo_heyvaerts.c, new text, kinds it touches, slots it touches, classes every record of which it must miss)
MUTATIONS = [
    ("the mu term of dfdsigma dropped", "mu_term = dcxi_dsigma * dfdcxi;", "mu_term = 0. * dcxi_dsigma * dfdcxi;", (2, 3), (0, 1), "AB"),
    ("the sign of the mu term of dfdsigma", "mu_term = dcxi_dsigma * dfdcxi;", "mu_term = -dcxi_dsigma * dfdcxi;", (2, 3), (0, 1), "AB"),
    ("t3 of h_qr_element halved", "const double t3 = -RIM_PI * (2. * po_sq", "const double t3 = -0.5 * RIM_PI * (2. * po_sq", (0, 1, 2, 3), (0,), "AB"),
    ("the marching tolerance 1e-5 raised to 1e-1", "const double TOL = 1e-5,", "const double TOL = 1e-1,", (0, 1, 2, 3), (0, 1), "A"),
]


@pytest.mark.parametrize("what,old,new,kinds,slots,classes", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_mutated_oracle_misses_its_records(fix, tmp_path, what, old, new, kinds, slots, classes):
    """Teeth: an oracle compiled from a copy with one slip in the Heyvaerts path misses the bound of every record of the kinds,
    slots and classes the slip touches (the unmutated one passes them all, test_oracle_coefficients_within_bounds).  For the
    marching tolerance that is every class-A record: a loop that stops early is caught where the loops are shortest."""
    shutil.copytree(os.path.join(ROOT, "oracle"), tmp_path / "oracle", ignore=shutil.ignore_patterns("*.so", "_ref"))
    os.makedirs(tmp_path / "rimphony_amd")
    shutil.copytree(os.path.join(ROOT, "rimphony_amd", "csrc"), tmp_path / "rimphony_amd" / "csrc", ignore=shutil.ignore_patterns("*.hip", "*.so", "*.o"))
    src = (tmp_path / "oracle" / "rimo_heyvaerts.c").read_text()
    assert src.count(old) == 1, old
    (tmp_path / "oracle" / "rimo_heyvaerts.c").write_text(src.replace(old, new))
    subprocess.run(["make", "-C", str(tmp_path / "oracle"), "liboracle.so"], check=True, stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(str(tmp_path / "oracle" / "liboracle.so"))
    good = oracle_bind.load("det")
    L.rimo_batch.restype, L.rimo_batch.argtypes = good.rimo_batch.restype, good.rimo_batch.argtypes
    for kind in kinds:
        rec, dev, got = coefficient_deviation(fix, L, kind)
        touched = np.isin(fix["rec_slot"][rec], slots) & np.isin(fix["row_class"][fix["rec_row"][rec]], list(classes))
        assert touched.sum() == 5 * len(classes) * len(slots)
        caught = ~(dev <= fix["rec_bound"][rec])
        assert caught[touched].all(), (what, kind, rec[touched & ~caught], dev[touched & ~caught], fix["rec_bound"][rec][touched & ~caught])
