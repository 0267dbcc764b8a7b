"""The ends of the spline of a 2-D table set, natural or not-a-knot per axis (rimphony_ctx_set_tables_2d_ends,
rimphony_ctx_set_tables_2d_device_ends), without a GPU: the table oracle tests/support/tab2d_ends_oracle.cpp -- the host build
of tab_spline.h and tab_install.h and of the device functions the kernels inline -- on the three geometries (nodes uniform in
ln gamma and mu; jittered gamma nodes; jittered gamma and mu nodes with mu[0] = -1 and mu[-1] = +1 exactly).

The bounds are ten times what tools/tab_2d_ends_accuracy.py measured with this oracle on the CPU
(profiles/tabulated_2d_ends_accuracy.txt, "what the host tests assert"):
  cubics come back            worst deviation 3.8e-15 of max |S| over the six sets      -> 3.8e-14
                              (natural ends on the same sets: 9.5e-2 .. 1.4e-1)
  against scipy.CubicSpline   worst difference 5.0e-15 of a line's max |slope|           -> 5.0e-14
  the normalisation           0 with ends (natural, not-a-knot), 2.2e-16 with not-a-knot on both axes: one unit in the
                              last place of the ratio, which is what the figure is resolved to -> 2.2e-15
                              (natural ends: 6.2e-4)
CPU only."""
import numpy as np
import pytest

import tab2d_ends_bind as te

NAK, NAT = te.NOT_A_KNOT, te.NATURAL
CUBIC_BOUND = 10 * 3.8e-15
SCIPY_BOUND = 10 * 5.0e-15
NORM_BOUND = 10 * 2.2e-16
ALL_ENDS = [(NAT, NAT), (NAK, NAT), (NAT, NAK), (NAK, NAK)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_words(name, got, want):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    d = np.flatnonzero(bits(got) != bits(want))
    assert d.size == 0, (name, d.size, d[:8], got.ravel()[d[:8]], want.ravel()[d[:8]])


def a_set(form, shape, sin_k=False, jitter=0.02):
    """(gamma, mu, log_n, sin_k) of a set of `shape` on the geometry `form`"""
    gamma, mu, g_at, mu_at = te.nodes_of(form, shape[1], shape[2])
    t = te.smooth_tables(shape, g_at, mu_at, seed=shape[1] + shape[2], jitter=jitter)
    return gamma, mu, t, (np.linspace(0.5, 2.5, shape[0]) if sin_k else None)


def built(gamma, mu, t, k, ends):
    assert te.set_tables(gamma, mu, t, k, ends, with_norm=False) == 0
    return te.blob()


# ---- 1. cubics come back --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", te.CUBIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", te.FORMS)
def test_cubics_come_back_with_not_a_knot_ends(form, shape):
    """S = P(u) Q(mu) + R(u) + T(mu), every factor of degree 3: S, S_u and S_mu of the bicubic at 200 points off the nodes,
    half of them in end cells.  With natural ends the same set is at least 1e3 bounds away: the test can tell the two apart."""
    dev = te.cubic_deviation(form, shape, (NAK, NAK))
    natural = te.cubic_deviation(form, shape, (NAT, NAT))
    print(form, shape, "not-a-knot %.3e  natural %.3e" % (dev, natural))
    assert dev <= CUBIC_BOUND
    assert natural >= 1e3 * CUBIC_BOUND


# ---- 2. an independent solver agrees ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", te.SCIPY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scipy_solves_the_same_splines(shape):
    """the S_u, S_mu and S_umu words on jittered nodes against scipy.interpolate.CubicSpline(bc_type="not-a-knot")"""
    diff = te.scipy_difference(shape)
    print(shape, "worst difference %.3e" % diff)
    assert diff <= SCIPY_BOUND


# ---- 3. natural through the new path is the old set -------------------------------------------------------------------------
@pytest.mark.parametrize("prefactor", [False, True], ids=["plain", "sin_k"])
@pytest.mark.parametrize("form", te.FORMS)
def test_natural_ends_build_the_set_of_the_builders_as_they_were(form, prefactor):
    for shape in ((1, 8, 8), (3, 9, 11)):
        gamma, mu, t, k = a_set(form, shape, prefactor)
        same_words((form, shape), built(gamma, mu, t, k, (NAT, NAT)), te.without_ends(gamma, mu, t, k))


# ---- 4. the axes are independent --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", te.FORMS)
def test_each_axis_follows_its_own_choice(form):
    shape = (3, 9, 11)
    gamma, mu, t, k = a_set(form, shape)
    sets = {e: built(gamma, mu, t, k, e) for e in ALL_ENDS}
    nd = {e: te.node_data(b, shape) for e, b in sets.items()}
    for e, b in sets.items():
        assert (te.ends_words(b) == e[0] + 2 * e[1]).all(), (e, te.ends_words(b))
    # the S and S_u words follow the gamma axis alone, the S_mu words the mu axis alone
    same_words("S, S_u of (natural, not-a-knot)", nd[(NAT, NAK)][..., :2], nd[(NAT, NAT)][..., :2])
    same_words("S_mu of (natural, not-a-knot)", nd[(NAT, NAK)][..., 2], nd[(NAK, NAK)][..., 2])
    same_words("S, S_u of (not-a-knot, natural)", nd[(NAK, NAT)][..., :2], nd[(NAK, NAK)][..., :2])
    same_words("S_mu of (not-a-knot, natural)", nd[(NAK, NAT)][..., 2], nd[(NAT, NAT)][..., 2])
    # and the choice is not ignored: along each axis the two kinds of ends give other slopes
    assert (bits(nd[(NAK, NAK)][..., 1]) != bits(nd[(NAT, NAT)][..., 1])).any()
    assert (bits(nd[(NAK, NAK)][..., 2]) != bits(nd[(NAT, NAT)][..., 2])).any()
    assert (bits(nd[(NAK, NAT)][..., 3]) != bits(nd[(NAT, NAT)][..., 3])).any()
    # everything in front of the node data but the word itself is the same in all four
    front = sets[(NAT, NAT)].size - nd[(NAT, NAT)].size
    keep = np.ones(front, dtype=bool)
    keep[te.HDR + te.T_HDR * np.arange(shape[0]) + te.T_ENDS] = False
    for e in ALL_ENDS[1:]:
        same_words(("front", e), sets[e][:front][keep], sets[(NAT, NAT)][:front][keep])


# ---- 5. the line solver is the builder --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", te.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", te.FORMS)
def test_the_line_solver_is_the_builder_word_for_word(form, shape):
    """rim_tab_install_family_line over every line of families 0, 1 and 2, in that order, behind the form's front: the
    builder's set as uint64, with not-a-knot ends on both axes and with the two mixed choices"""
    gamma, mu, t, k = a_set(form, shape, sin_k=te.SHAPES.index(shape) % 2 == 1)
    for e in ((NAK, NAK), (NAT, NAK), (NAK, NAT)):
        want = built(gamma, mu, t, k, e)
        assert np.isfinite(want).all()
        same_words((form, shape, e), te.lines(gamma, mu, t, k, e), want)
    assert np.array_equal(te.node_data(want, shape)[..., 0], t)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def test_a_bad_end_is_refused_and_the_previous_set_stays():
    gamma, mu, t, k = a_set("nodes", (3, 9, 11))
    before = built(gamma, mu, t, k, (NAK, NAK))
    for bad in (-1, 2, 7):
        for e in ((bad, NAT), (NAT, bad), (bad, bad), (bad, NAK)):
            assert te.check(gamma, mu, t, k, e) == -1, e
            assert te.set_tables(gamma, mu, t, k, e, with_norm=False) == -1, e
            same_words(("the set after", e), te.blob(), before)
    for e in ALL_ENDS:
        assert te.check(gamma, mu, t, k, e) == 0


@pytest.mark.parametrize("ends", [(NAT, NAT), (NAK, NAK)], ids=["natural", "not-a-knot"])
def test_what_the_forms_refuse_is_still_refused(ends):
    """the refused cases of the nodes form (tab2d_nodes_bind.refused_cases), a sample of those of the other two, and mu
    without gamma, which is no form"""
    import tab2d_nodes_bind as tn
    for which in (0, 1):
        gamma, mu, t, k = tn.fixture_set(which)
        assert te.check(gamma, mu, t, k, ends) == 0
        for name, (g, m, log_n, sin_k, shape) in tn.refused_cases(gamma, mu, t, k).items():
            if name == "null mu":
                continue        # without mu the call names the form on given gamma nodes, and that form takes it
            assert te.check(g, m, log_n, sin_k, ends, shape=shape) == -1, name
    gamma, mu, t, k = a_set("grid", (3, 9, 11), sin_k=True)
    nan_t, swapped = t.copy(), gamma.copy()
    nan_t[1, 5, 3] = np.nan
    swapped[[3, 4]] = swapped[[4, 3]]
    assert te.check(gamma, None, t, k, ends) == 0 and te.check(None, None, t, k, ends) == 0
    for name, (g, log_n, sin_k, kw) in {
        "grid: log_n NaN": (gamma, nan_t, k, {}), "grid: gamma swapped": (swapped, t, k, {}),
        "grid: 7 mu nodes": (gamma, t[:, :, :7], k, {}), "grid: k negative": (gamma, t, [0.5, -0.1, 1.0], {}),
        "grid: null log_n": (gamma, None, k, {"shape": t.shape}),
        "uniform: log_n NaN": (None, nan_t, k, {}), "uniform: gamma_lo < 1": (None, t, k, {"gamma_lo": 0.5}),
        "uniform: gamma_lo = gamma_hi": (None, t, k, {"gamma_lo": 10.0, "gamma_hi": 10.0}),
        "uniform: 7 gamma nodes": (None, t[:, :7], k, {}), "uniform: k above 100": (None, t, [100.5, 1.0, 1.0], {}),
    }.items():
        assert te.check(g, None, log_n, sin_k, ends, **kw) == -1, name
    assert te.check(None, np.linspace(-1.0, 1.0, 11), t, None, ends) == -1      # mu without gamma


# ---- 7. the normalisation follows -------------------------------------------------------------------------------------------
def test_the_normalisation_of_a_quadratic_in_mu_is_the_closed_form():
    """S = H(u) + 2 mu^2 on 16 mu nodes: N_iso / N = 1/2 int exp(2 mu^2) dmu, from scipy.special.erfi"""
    both, mu_only, natural = te.norm_deviation((NAK, NAK)), te.norm_deviation((NAT, NAK)), te.norm_deviation((NAT, NAT))
    print("not-a-knot on both axes %.3e  along mu only %.3e  natural %.3e" % (both, mu_only, natural))
    assert both <= NORM_BOUND and mu_only <= NORM_BOUND
    assert natural >= 1e3 * NORM_BOUND
