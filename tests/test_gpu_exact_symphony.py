"""The kernels against the exact harmonic sum (tests/exact_symphony.py, fixture tests/golden/exact_symphony.npz): every stored
record is held to the deterministic oracle's stored bits, as everywhere else in the suite, and to the exact value within the
bound stored with it (measured on the CPU oracle, tools/make_exact_symphony_fixture.py).  Nothing is left out at run time."""
import numpy as np
import pytest

import exact_symphony as ex

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return ex.load_fixture()


def hold(name, got, bits, exact, bound, where):
    got = np.ascontiguousarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), (name, where(int(np.flatnonzero(~np.isfinite(got))[0])))
    with np.errstate(all="ignore"):
        dev = ex.deviation(got, exact)
    print("%s: %d records, worst |got / exact - 1| / bound = %.3f" % (name, len(got), np.max(dev / np.maximum(bound, 1e-300))))
    off = np.flatnonzero(got.view(np.uint64) != bits)
    assert not len(off), "%s: %d of %d differ from the oracle's bits; first %r: got %r, oracle %r" % (
        name, len(off), len(got), where(int(off[0])), got[off[0]], bits[off[:1]].view(np.float64)[0])
    out = np.flatnonzero(~(dev <= bound))
    assert not len(out), "%s: %d of %d beyond their bound; first %r: deviation %.3e, bound %.3e" % (
        name, len(out), len(got), where(int(out[0])), dev[out[0]], bound[out[0]])


@pytest.mark.parametrize("kind", range(4))
def test_coefficients(gpu_ctx, fix, kind):
    """All rows of the kind, classes A and B, in one compute_batch call."""
    rows = np.flatnonzero(fix["row_kind"] == kind)
    s, theta, params = ex.row_inputs(fix, rows)
    out = gpu_ctx.compute_batch(kind, s, theta, params, 0x3F)
    rec = np.flatnonzero(np.isin(fix["rec_row"], rows))
    assert len(rec) >= 50
    got = out[np.searchsorted(rows, fix["rec_row"][rec]), fix["rec_slot"][rec]]
    hold(ex.KINDS[kind], got, fix["rec_det_bits"][rec], fix["rec_exact"][rec], fix["rec_bound"][rec],
         lambda i: (int(fix["rec_row"][rec[i]]), int(fix["rec_slot"][rec[i]])))


@pytest.mark.parametrize("group", range(8))
def test_single_harmonics(gpu_ctx, fix, group):
    """gamma_integral_batch on G(n): integer orders below 30, integer and non-integer ones from 30 to 3000, both V lobes."""
    kind, par, s, theta = ex.group_inputs(fix, group)
    rec = np.flatnonzero(fix["h_group"] == group)
    assert len(rec) >= 300
    got = np.empty(len(rec))
    for p, (coeff, stokes, lobe) in enumerate(fix["pairs"]):
        m = fix["h_pair"][rec] == p
        assert m.any()
        got[m] = gpu_ctx.gamma_integral_batch(kind, par, int(coeff), int(stokes), int(lobe), s, theta, fix["h_n"][rec[m]])
    hold("%s s = %g" % (ex.KINDS[kind], s), got, fix["h_det_bits"][rec], fix["h_exact"][rec], fix["h_bound"][rec],
         lambda i: (tuple(int(v) for v in fix["pairs"][fix["h_pair"][rec[i]]]), float(fix["h_n"][rec[i]])))


@pytest.mark.parametrize("kind", range(4))
def test_public_path(gpu_ctx, fix, kind):
    """The first class-A row of the kind through FullSynchrotronCalculator.compute_all_dimensionless."""
    from rimphony_amd import api
    row = int(np.flatnonzero((fix["row_kind"] == kind) & (fix["row_class"] == "A"))[0])
    par = [float(v) for v in fix["row_params"][row, :fix["row_nparams"][row]]]
    out = api.FullSynchrotronCalculator(kind, par, ctx=gpu_ctx).compute_all_dimensionless(float(fix["row_s"][row]), float(fix["row_theta"][row]))
    rec = np.flatnonzero(fix["rec_row"] == row)
    assert len(rec) == 6
    hold(ex.KINDS[kind] + " public", out[fix["rec_slot"][rec]], fix["rec_det_bits"][rec], fix["rec_exact"][rec], fix["rec_bound"][rec],
         lambda i: (row, int(fix["rec_slot"][rec[i]])))


def test_tabulated_surface(gpu_ctx, fix):
    """The surface of the fixture through TabulatedDistribution2DGrid.from_function and compute_batch: the table oracle's
    bits, computed here from the same table, and the exact sum of the same f(gamma, mu) within the stored bounds."""
    import tab2d_grid_bind
    from rimphony_amd import api
    T, a, lo, hi, n_nodes, n_mu = ex.surface_inputs(fix)
    dist = ex.tilted_juettner(T, a, lo, hi)
    table = api.TabulatedDistribution2DGrid.from_function(
        lambda g, mu: g * np.sqrt(g * g - 1.) * dist.f(g, mu, np), api.grid_nodes_log_gm1(lo, hi, n_nodes), n_mu)
    s, theta, index = fix["surf_s"].copy(), fix["surf_theta"].copy(), np.zeros(len(fix["surf_s"]))
    assert tab2d_grid_bind.set_tables(table.gamma, table.log_n) == 0
    ref, _ = tab2d_grid_bind.batch(s, theta, index, 0x3F)
    gpu_ctx.set_tables_2d_grid(table.gamma, table.log_n)
    out = gpu_ctx.compute_batch(api.TABULATED, s, theta, [index], 0x3F)
    hold("tabulated surface", out[:, :6].ravel(), np.ascontiguousarray(ref[:, :6]).view(np.uint64).ravel(), fix["surf_exact"].ravel(),
         fix["surf_bound"].ravel(), lambda i: (i // 6, i % 6))
