"""The Symphony path of the four analytic kinds against the exact harmonic sum (tests/exact_symphony.py), CPU side: the
reference against its mpmath twin and its own resolution, the stored fixture against its generator, both oracle flavours
against the stored exact values within the stored bounds, and mutated oracles that must miss them.

The bounds are those of tools/make_exact_symphony_fixture.py: 2 max(|det / exact - 1|, |libm / exact - 1|) + 100 x the relative
error estimate of the exact value, measured on the CPU oracle (profiles/exact_symphony_deviation.txt)."""
import ctypes
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact_symphony as ex
import oracle_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = range(4)


@pytest.fixture(scope="module")
def fix():
    return ex.load_fixture()


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
    s, theta, params = ex.row_inputs(fix, rows)
    out = oracle_bind.batch(L, kind, s, theta, params, 0x3F, 8)
    rec = np.flatnonzero(np.isin(fix["rec_row"], rows))
    got = out[np.searchsorted(rows, fix["rec_row"][rec]), fix["rec_slot"][rec]]
    with np.errstate(all="ignore"):
        return rec, ex.deviation(got, fix["rec_exact"][rec]), got


def generator():
    spec = importlib.util.spec_from_file_location("make_exact_symphony_fixture", os.path.join(ROOT, "tools", "make_exact_symphony_fixture.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_fixture_is_whole(fix):
    """Every stored value is finite, every row of the generator's list is there, and the bounds are as tight as the issue
    that introduced the fixture requires: per slot at least three class-A rows within 1e-12 (thermal), 1e-7 (pitchy_kappa),
    1e-5 (power_law, pitchy_pl, V included); 90 % of the single harmonics below 30 of every kind within 1e-6."""
    for k, v in fix.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), k
    gen = generator()
    assert gen.SURFACE == ex.surface_inputs(fix) and gen.SURFACE_POINTS == list(zip(fix["surf_s"], fix["surf_theta"]))
    assert len(gen.ROWS) == len(fix["row_kind"]) and len(gen.HARMONIC_GROUPS) == len(fix["grp_kind"])
    for i, (kind, par, s, theta, cls) in enumerate(gen.ROWS):
        assert (kind, s, theta, cls) == (fix["row_kind"][i], fix["row_s"][i], fix["row_theta"][i], fix["row_class"][i])
        assert par == list(fix["row_params"][i, :len(par)])
    for g, (kind, par, s, theta) in enumerate(gen.HARMONIC_GROUPS):
        assert (kind, par, s, theta) == ex.group_inputs(fix, g)
    assert (fix["rec_err"] <= 1e-11 * np.abs(fix["rec_exact"])).all()
    assert (fix["h_err"] <= 1e-11 * np.abs(fix["h_exact"])).all()
    bound = 2. * np.maximum(fix["rec_dev_det"], fix["rec_dev_libm"]).astype(np.float64) + 100. * fix["rec_err"] / np.abs(fix["rec_exact"])
    assert np.allclose(fix["rec_bound"], bound, rtol=1e-6, atol=0.)          # the deviations are stored in single precision
    for kind, cap in ((0, 1e-5), (1, 1e-12), (2, 1e-5), (3, 1e-7)):
        a = rows_of(fix, kind, "A")
        share = fix["rec_share"][np.isin(fix["rec_row"], a)]
        assert (share < 1e-14).all()
        for slot in range(6):
            b = fix["rec_bound"][np.isin(fix["rec_row"], a) & (fix["rec_slot"] == slot)]
            assert (b <= cap).sum() >= 3, (kind, slot, np.sort(b))
        low = fix["h_bound"][(fix["grp_kind"][fix["h_group"]] == kind) & (fix["h_n"] < 30.)]
        assert (low <= 1e-6).mean() >= 0.9, (kind, (low <= 1e-6).mean())
        # s on both sides of 10, both first harmonics, both hemispheres, k non-integer and above 2
        r = rows_of(fix, kind)
        n_lo = np.floor(fix["row_s"][r] * np.abs(np.sin(fix["row_theta"][r])) + 1.)
        assert (fix["row_s"][r] < 10.).any() and (fix["row_s"][r] > 10.).any() and (n_lo == 1).any() and (n_lo > 1).any()
        assert (np.cos(fix["row_theta"][r]) < 0.).any() and (np.cos(fix["row_theta"][r]) > 0.).any()
    for kind, col in ((2, 1), (3, 2)):
        k = fix["row_params"][rows_of(fix, kind), col]
        assert (k > 2.).any() and (k != np.round(k)).all()


HARMONICS_MP = [(1, [0.3], 2., 0.6, 2.), (3, [4., 1.5, 1.7, 0.3], 2., 0.6, 5.), (2, [3., 1.3, 1.02, 30., 0.3], 2.5, 1.4, 3.),
                (0, [3., 1.5, 12., 30.], 3., 2.2, 31.37)]


@pytest.mark.parametrize("kind,par,s,theta,n", HARMONICS_MP)
def test_harmonic_against_mpmath(kind, par, s, theta, n):
    """G(n) in double precision against tanh-sinh quadrature of the same expression at 25 digits: 1e-11.  The cases: gamma- = 1
    exactly (n = s), non-integer k in both derivative terms, hard gamma limits inside the lobe, a non-integer order."""
    dist = ex.make(kind, par)
    got, err = ex.harmonics_with_error(dist, s, theta, [n])
    ref = ex.harmonic_mp(dist, s, theta, n, digits=25)
    assert (np.abs(got[0] - ref) <= 1e-11 * np.abs(ref)).all(), got[0] / ref - 1.
    assert (err[0] <= 1e-11 * np.abs(ref)).all()


def test_sum_against_mpmath():
    """The whole sum of one cold thermal point against the 25-digit twin over the harmonics that carry it (the double-precision
    sum's count less the forty closing terms below 1e-13 each, which fall off geometrically): 1e-11."""
    dist = ex.make(1, [0.2])
    val, err, count, share = ex.coefficients(dist, 0.8, 1.3)
    ref, _ = ex.coefficients_mp(dist, 0.8, 1.3, digits=25, n_harmonics=count - 40)
    assert (np.abs(val - ref) <= 1e-11 * np.abs(ref)).all(), val / ref - 1.


def test_resolution_doubling(fix):
    """Twice the points per panel move no harmonic by more than 1e-11 of itself, at cold and at
    warm points, integer and non-integer orders."""
    for g in (0, 3, 5, 6):
        kind, par, s, theta = ex.group_inputs(fix, g)
        n = np.unique(fix["h_n"][fix["h_group"] == g])[::3]
        val, err = ex.harmonics_with_error(ex.make(kind, par), s, theta, n, capped=False)
        keep = np.abs(val) > 1e-290
        assert (err[keep] <= 1e-11 * np.abs(val[keep])).all(), (g, (err[keep] / np.abs(val[keep])).max())


def test_fixture_is_what_the_generator_gives(fix):
    """Three cheap rows computed again from the stored inputs: 1e-12."""
    for kind in (1, 2, 3):
        i = rows_of(fix, kind, "A")[0]
        par = fix["row_params"][i, :fix["row_nparams"][i]]
        val, err, count, share = ex.coefficients(ex.make(kind, par), fix["row_s"][i], fix["row_theta"][i])
        assert count == fix["row_harmonics"][i]
        rec = np.flatnonzero(fix["rec_row"] == i)
        assert len(rec) >= 4
        assert (np.abs(val[fix["rec_slot"][rec]] / fix["rec_exact"][rec] - 1.) <= 1e-12).all()


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_coefficients_within_bounds(fix, oracle, oracle_libm, kind):
    """Both flavours on every record of the kind in one batch each; the deterministic one also carries the stored bits."""
    rec, dev, got = coefficient_deviation(fix, oracle, kind)
    assert len(rec) >= 50
    assert same_bits(got, fix["rec_det_bits"][rec].view(np.float64)).all()
    assert (dev <= fix["rec_bound"][rec]).all(), (rec[dev > fix["rec_bound"][rec]], dev.max())
    rec, dev, got = coefficient_deviation(fix, oracle_libm, kind)
    assert (dev <= fix["rec_bound"][rec]).all(), (rec[dev > fix["rec_bound"][rec]], dev.max())


def test_oracle_harmonics_within_bounds(fix, oracle, oracle_libm):
    for L in (oracle, oracle_libm):
        for g in range(len(fix["grp_kind"])):
            kind, par, s, theta = ex.group_inputs(fix, g)
            d, st = oracle_bind.mkdist(L, kind, par)
            assert st == 0
            rec = np.flatnonzero(fix["h_group"] == g)
            assert len(rec) >= 300
            got = np.array([L.rimo_gamma_integral(d, *[int(v) for v in fix["pairs"][fix["h_pair"][i]]], s, theta, fix["h_n"][i])
                            for i in rec])
            if L is oracle:
                assert same_bits(got, fix["h_det_bits"][rec].view(np.float64)).all()
            with np.errstate(all="ignore"):
                dev = ex.deviation(got, fix["h_exact"][rec])
            assert (dev <= fix["h_bound"][rec]).all(), (g, rec[~(dev <= fix["h_bound"][rec])][:5])


def test_tabulated_surface_within_bounds(fix):
    """A non-separable surface, tabulated by TabulatedDistribution2DGrid.from_function on nodes uniform in ln(gamma - 1) and
    run through the table oracle, against the exact sum of the same f(gamma, mu) at two class-A points: the 2-D forms have no
    analytic kind beside them.  The surface's own normalisation and one of the points are computed again here."""
    import tab2d_grid_bind
    from rimphony_amd import api
    T, a, lo, hi, n_nodes, n_mu = ex.surface_inputs(fix)
    dist = ex.tilted_juettner(T, a, lo, hi)
    table = api.TabulatedDistribution2DGrid.from_function(
        lambda g, mu: g * np.sqrt(g * g - 1.) * dist.f(g, mu, np), api.grid_nodes_log_gm1(lo, hi, n_nodes), n_mu)
    assert tab2d_grid_bind.set_tables(table.gamma, table.log_n) == 0
    out, _ = tab2d_grid_bind.batch(fix["surf_s"].copy(), fix["surf_theta"].copy(), np.zeros(len(fix["surf_s"])), 0x3F)
    dev = ex.deviation(out[:, :6], fix["surf_exact"])
    assert (fix["surf_bound"] <= 1e-6).all() and (fix["surf_err"] <= 1e-11 * np.abs(fix["surf_exact"])).all()
    assert (dev <= fix["surf_bound"]).all(), dev / fix["surf_bound"]
    val, err, count, share = ex.coefficients(dist, fix["surf_s"][0], fix["surf_theta"][0])
    assert (share < 1e-14).all() and (np.abs(val / fix["surf_exact"][0] - 1.) <= 1e-12).all()


MUTATIONS = [
    ("the sign of dfdcx_factor", "rimo_symphony.c", "const double dfdcx_factor = (beta * cos_th - cos_xi) / (gamma - 1. / gamma);",
     "const double dfdcx_factor = (cos_xi - beta * cos_th) / (gamma - 1. / gamma);", 1, (2, 3)),
    ("k dropped from dfdcx", "rimo_dist.c", "*dfdcx = -f * k * cos_xi / (sin_xi * sin_xi);", "*dfdcx = -f * cos_xi / (sin_xi * sin_xi);", 2, (2, 3)),
    ("1 / gamma_cutoff dropped from the kappa dfdg", "rimo_dist.c",
     "*dfdg = -f * ((kappa + 1.) / (kappa * width + gamma - 1.) + d->inv_gamma_cutoff);",
     "*dfdg = -f * ((kappa + 1.) / (kappa * width + gamma - 1.));", 1, (3,)),
]


@pytest.mark.parametrize("what,name,old,new,count,kinds", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_a_mutated_oracle_misses_every_cold_row(fix, tmp_path, what, name, old, new, count, kinds):
    """Teeth: an oracle compiled from a copy with one slip in the absorption path misses the bound on every class-A row of the
    kinds the slip touches (the unmutated one passes them, test_oracle_coefficients_within_bounds)."""
    shutil.copytree(os.path.join(ROOT, "oracle"), tmp_path / "oracle", ignore=shutil.ignore_patterns("*.so", "_ref"))
    os.makedirs(tmp_path / "rimphony_amd")
    shutil.copytree(os.path.join(ROOT, "rimphony_amd", "csrc"), tmp_path / "rimphony_amd" / "csrc", ignore=shutil.ignore_patterns("*.hip", "*.so", "*.o"))
    src = (tmp_path / "oracle" / name).read_text()
    assert src.count(old) == count, (name, old)
    (tmp_path / "oracle" / name).write_text(src.replace(old, new))
    subprocess.run(["make", "-C", str(tmp_path / "oracle"), "liboracle.so"], check=True, stdout=subprocess.DEVNULL)
    L = ctypes.CDLL(str(tmp_path / "oracle" / "liboracle.so"))
    good = oracle_bind.load("det")
    L.rimo_batch.restype, L.rimo_batch.argtypes = good.rimo_batch.restype, good.rimo_batch.argtypes
    for kind in kinds:
        rec, dev, got = coefficient_deviation(fix, L, kind)
        missed = ~(dev <= fix["rec_bound"][rec])
        rows = rows_of(fix, kind, "A")
        assert len(rows) >= 4
        for r in rows:
            assert missed[fix["rec_row"][rec] == r].any(), (what, kind, r)
