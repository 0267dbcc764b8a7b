"""The kernels against the converged Heyvaerts integrals (tests/exact_faraday.py, fixture tests/golden/exact_faraday.npz): every
stored record is held to the deterministic oracle's stored bits, as everywhere else in the suite, and to the exact value within
the bound stored with it (measured on the CPU oracle, tools/make_exact_faraday_fixture.py).  Nothing is left out at run time."""
import numpy as np
import pytest

import exact_faraday as ef
import exact_symphony as ex

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return ef.load_fixture()


def hold(name, got, bits, exact, bound, where):
    got = np.ascontiguousarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), (name, where(int(np.flatnonzero(~np.isfinite(got))[0])))
    with np.errstate(all="ignore"):
        dev = ef.deviation(got, exact)
    print("%s: %d records, worst |got / exact - 1| / bound = %.3f" % (name, len(got), np.max(dev / np.maximum(bound, 1e-300))))
    off = np.flatnonzero(got.view(np.uint64) != bits)
    assert not len(off), "%s: %d of %d differ from the oracle's bits; first %r: got %r, oracle %r" % (
        name, len(off), len(got), where(int(off[0])), got[off[0]], bits[off[:1]].view(np.float64)[0])
    out = np.flatnonzero(~(dev <= bound))
    assert not len(out), "%s: %d of %d beyond their bound; first %r: deviation %.3e, bound %.3e" % (
        name, len(out), len(got), where(int(out[0])), dev[out[0]], bound[out[0]])


@pytest.mark.parametrize("kind", range(4))
def test_coefficients(gpu_ctx, fix, kind):
    """All ten rows of the kind, classes A and B, in one compute_batch call with the mask of slots 6 and 7: twenty values, all
    finite, no status bit set."""
    rows = np.flatnonzero(fix["row_kind"] == kind)
    s, theta, params = ef.row_inputs(fix, rows)
    out, status = gpu_ctx.compute_batch(kind, s, theta, params, ef.MASK, want_status=True)
    assert not status[:, 6:].any(), status[:, 6:]
    rec = np.flatnonzero(np.isin(fix["rec_row"], rows))
    assert len(rec) == 20
    got = out[np.searchsorted(rows, fix["rec_row"][rec]), 6 + fix["rec_slot"][rec]]
    hold(ex.KINDS[kind], got, fix["rec_det_bits"][rec], fix["rec_exact"][rec], fix["rec_bound"][rec],
         lambda i: (int(fix["rec_row"][rec[i]]), 6 + int(fix["rec_slot"][rec[i]])))


@pytest.mark.parametrize("kind", range(4))
def test_inner_integrals(gpu_ctx, fix, kind):
    """hey_outer_batch on the stored outer-integrand samples of the kind's two rows: Q and V, non-resonant and quasi-resonant,
    sigma on both sides of 3 and between 3 and the g = 10 root."""
    rec = np.flatnonzero(fix["row_kind"][fix["in_row"]] == kind)
    assert len(rec) == 40
    got = np.empty(len(rec))
    for row in np.unique(fix["in_row"][rec]):
        for stokes in (ef.STOKES_Q, ef.STOKES_V):
            for qr in (0, 1):
                m = (fix["in_row"][rec] == row) & (fix["in_stokes"][rec] == stokes) & (fix["in_qr"][rec] == qr)
                assert m.sum() == 5
                got[m] = gpu_ctx.hey_outer_batch(kind, ef.row_params(fix, row), stokes, float(fix["row_s"][row]), float(fix["row_theta"][row]),
                                                 qr, fix["in_u"][rec[m]].copy())
    hold(ex.KINDS[kind] + " inner integrals", got, fix["in_det_bits"][rec], fix["in_exact"][rec], fix["in_bound"][rec],
         lambda i: (int(fix["in_row"][rec[i]]), int(fix["in_stokes"][rec[i]]), int(fix["in_qr"][rec[i]]), float(fix["in_u"][rec[i]])))


def test_public_path(gpu_ctx, fix):
    """The ten rows of pitchy_kappa through FullSynchrotronCalculator.compute_all_dimensionless."""
    from rimphony_amd import api
    kind = 3
    rows = np.flatnonzero(fix["row_kind"] == kind)
    got, rec = [], []
    for row in rows:
        out = api.FullSynchrotronCalculator(kind, ef.row_params(fix, row), ctx=gpu_ctx).compute_all_dimensionless(
            float(fix["row_s"][row]), float(fix["row_theta"][row]))
        r = np.flatnonzero(fix["rec_row"] == row)
        assert len(r) == 2
        got += list(out[6 + fix["rec_slot"][r]])
        rec += list(r)
    rec = np.array(rec)
    hold(ex.KINDS[kind] + " public", got, fix["rec_det_bits"][rec], fix["rec_exact"][rec], fix["rec_bound"][rec],
         lambda i: (int(fix["rec_row"][rec[i]]), 6 + int(fix["rec_slot"][rec[i]])))


def test_tabulated_surface(gpu_ctx, fix):
    """The tilted_juettner surface through TabulatedDistribution2DGrid.from_function and compute_batch: the table oracle's bits,
    computed here from the same table, and the exact integrals of the same f(gamma, mu) within the stored bounds."""
    import tab2d_grid_bind
    from rimphony_amd import api
    T, a, lo, hi, n_nodes, n_mu = ex.surface_inputs(fix)
    dist = ex.tilted_juettner(T, a, lo, hi)
    table = api.TabulatedDistribution2DGrid.from_function(
        lambda g, mu: g * np.sqrt(g * g - 1.) * dist.f(g, mu, np), api.grid_nodes_log_gm1(lo, hi, n_nodes), n_mu)
    s, theta, index = fix["surf_s"].copy(), fix["surf_theta"].copy(), np.zeros(len(fix["surf_s"]))
    assert tab2d_grid_bind.set_tables(table.gamma, table.log_n) == 0
    ref, _ = tab2d_grid_bind.batch(s, theta, index, ef.MASK)
    gpu_ctx.set_tables_2d_grid(table.gamma, table.log_n)
    out = gpu_ctx.compute_batch(api.TABULATED, s, theta, [index], ef.MASK)
    hold("tabulated surface", out[:, 6:].ravel(), np.ascontiguousarray(ref[:, 6:]).view(np.uint64).ravel(), fix["surf_exact"].ravel(),
         fix["surf_bound"].ravel(), lambda i: (i // 2, 6 + i % 2))
