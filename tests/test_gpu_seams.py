"""The eight per-point unit seams (one host-described parameter point, arrays of abscissae) at their boundary: what they
refuse, and the smallest counts -- one item, one item past a 64-thread block, fewer items than any grid has waves.  The
values themselves are held to the oracle by test_gpu_parity.py and the tabulated kind's test files; the inputs here are
theirs.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import oracle_bind
from rimphony_amd import capi
from seam_inputs import harmonic_samples, hey_outer_abscissae, hey_seam_inputs
from test_gpu_parity import HEY_SEAM_POINTS, _kind_params, report_mismatch

pytestmark = pytest.mark.gpu

POWER_LAW = [2.5, 1.0, 1e12, 1e10]

# name -> (the scalars between `params` and `count` as a function of (coeff, stokes), input arrays, output arrays,
#          takes a coefficient, a Stokes parameter the entry accepts)
ENTRIES = {
    "gamma_integrand": (lambda c, k: (c, k, 10., 0.8), 2, 1, True, 0),
    "gamma_integral": (lambda c, k: (c, k, 0, 10., 0.8), 1, 1, True, 0),
    "n_integral": (lambda c, k: (c, k, 0, 10., 0.8), 2, 1, True, 0),
    "deriv_probe": (lambda c, k: (c, k, 0, 10., 0.8), 1, 1, True, 0),
    "gamma_contribution": (lambda c, k: (c, k, 10., 0.8), 1, 1, True, 0),
    "calc_f": (lambda c, k: (float("nan"),), 2, 3, False, None),
    "hey_element": (lambda c, k: (k, 10., 0.8, 0), 2, 1, False, 1),
    "hey_outer": (lambda c, k: (k, 10., 0.8, 0), 1, 1, False, 1),
}


def test_refusals_are_error_codes_and_an_empty_call_is_no_work(gpu_ctx):
    """Every entry refuses a distribution kind out of range, params = NULL, a null array with count = 1, a coefficient or
    Stokes parameter out of range where it takes one (Stokes I for the Heyvaerts entries) and the tabulated kind on a context
    without a table set, with a negative code; count = 0 with valid arguments is RIMPHONY_OK and empty arrays from the Python
    method.  The context computes afterwards."""
    lib = capi.load()
    h = gpu_ctx.handle
    par = (ctypes.c_double * 4)(*POWER_LAW)
    one = (ctypes.c_double * 1)(0.0)
    buf = torch.full((8,), 40.0, dtype=torch.float64, device="cuda:0")      # every array argument: one valid element each
    ptr = [ctypes.c_void_p(buf[i:].data_ptr()) for i in range(8)]
    gpu_ctx.set_tables(1.0, 2.0, None)

    def call(name, kind=0, params=par, coeff=0, stokes=None, count=1, null_array=False):
        scalars, n_in, n_out, _, good_stokes = ENTRIES[name]
        arrays = list(ptr[:n_in + n_out])
        if null_array:
            arrays[0] = None
        return getattr(lib, "rimphony_%s_batch_device" % name)(
            h, kind, params, *scalars(coeff, good_stokes if stokes is None else stokes), count, *arrays, None)

    for name, (_, _, _, takes_coeff, good_stokes) in ENTRIES.items():
        assert call(name, kind=9) < 0, name
        assert call(name, params=None) < 0, name
        assert call(name, null_array=True) < 0, name
        if takes_coeff:
            assert call(name, coeff=2) < 0, name
        if good_stokes is not None:
            assert call(name, stokes=3) < 0, name
        if good_stokes == 1:
            assert call(name, stokes=0) < 0, name
        assert call(name, kind=4, params=one) < 0, name
        assert call(name, count=0) == 0, name
    empty = []
    for got in (gpu_ctx.gamma_integrand_batch(0, POWER_LAW, 0, 0, 10., 0.8, empty, empty),
                gpu_ctx.gamma_integral_batch(0, POWER_LAW, 0, 0, 0, 10., 0.8, empty),
                gpu_ctx.n_integral_batch(0, POWER_LAW, 0, 0, 0, 10., 0.8, empty, empty),
                gpu_ctx.deriv_probe_batch(0, POWER_LAW, 0, 0, 0, 10., 0.8, empty),
                gpu_ctx.gamma_contribution_batch(0, POWER_LAW, 0, 0, 10., 0.8, empty),
                *gpu_ctx.calc_f_batch(0, POWER_LAW, empty, empty),
                gpu_ctx.hey_element_batch(0, POWER_LAW, 1, 10., 0.8, 0, empty, empty),
                gpu_ctx.hey_outer_batch(0, POWER_LAW, 1, 10., 0.8, 0, empty)):
        assert isinstance(got, np.ndarray) and got.shape == (0,) and got.dtype == np.float64
    # the context is still usable afterwards
    got = gpu_ctx.compute_batch(0, [10.0], [0.8], [[2.5], [1.0], [1e12], [1e10]], 0x03)
    assert np.isfinite(got[0, :2]).all()


def _tiled(a, n):
    return np.resize(np.asarray(a, dtype=np.float64), n)


def test_counts_at_the_edges_bit_exact(gpu_ctx, oracle):
    """count = 1 and 65 (one element past a 64-thread block) for the thread-per-item seams, 1 and 3 for the wave-per-item
    seams, power law, with the parameters and abscissae of the seam's test in test_gpu_parity.py: the oracle's bits."""
    hey_kind, hey_par, hey_s, hey_th = HEY_SEAM_POINTS[2]
    assert hey_kind == 0

    def dist(par):
        d, st = oracle_bind.mkdist(oracle, 0, par)
        assert st == 0
        return d

    # -- one thread per item -------------------------------------------------------------------------------------------
    rng = np.random.default_rng(100)
    par = _kind_params(rng, 0)
    s = float(np.exp(rng.uniform(math.log(.1), math.log(1e6))))
    th = float(rng.uniform(0.01, 1.55))
    coeff, stokes = int(rng.integers(0, 2)), int(rng.integers(0, 3))
    n, g = (_tiled(a, 65) for a in harmonic_samples(rng, s, th, 3000))
    d = dist(par)
    ref = np.array([oracle.rimo_gamma_integrand(d, coeff, stokes, s, th, a, b) for a, b in zip(n, g)])
    for count in (1, 65):
        got = gpu_ctx.gamma_integrand_batch(0, par, coeff, stokes, s, th, n[:count], g[:count])
        report_mismatch("gamma_integrand, count %d" % count, got, ref[:count])

    rng = np.random.default_rng(50)
    par = [2.7, 3.0, 1e7, 1e5]
    gamma = _tiled(np.exp(rng.uniform(math.log(1.0001), math.log(2e7), 512)), 65)
    cos_xi = _tiled(rng.uniform(-0.99, 0.99, 512), 65)
    d = dist(par)
    ref = np.empty((3, 65))
    a, b = ctypes.c_double(), ctypes.c_double()
    for i in range(65):
        ref[0, i] = oracle.rimo_calc_f(d, gamma[i], cos_xi[i])
        oracle.rimo_calc_f_derivatives(d, gamma[i], cos_xi[i], ctypes.byref(a), ctypes.byref(b))
        ref[1, i], ref[2, i] = a.value, b.value
    for count in (1, 65):
        got = gpu_ctx.calc_f_batch(0, par, gamma[:count], cos_xi[:count])
        for k, what in enumerate(("calc_f", "dfdg", "dfdcx")):
            report_mismatch("%s, count %d" % (what, count), got[k], ref[k, :count])

    rng = np.random.default_rng(702)
    d = dist(hey_par)
    fixed, v = (_tiled(a, 65) for a in hey_seam_inputs(rng, hey_s, hey_th, 0, 1536))
    ref = np.array([oracle.rimo_hey_element(ctypes.byref(d), 1, hey_s, hey_th, 0, float(p), float(q)) for p, q in zip(fixed, v)])
    for count in (1, 65):
        got = gpu_ctx.hey_element_batch(0, hey_par, 1, hey_s, hey_th, 0, fixed[:count], v[:count])
        report_mismatch("hey_element, count %d" % count, got, ref[:count])

    # -- one wave per item ---------------------------------------------------------------------------------------------
    rng = np.random.default_rng(300)
    par = _kind_params(rng, 0)
    s, th = 3.0, 0.7
    nmin = s * abs(math.sin(th))
    n = np.concatenate([np.floor(nmin + 1) + np.arange(30), nmin + 31 + np.exp(rng.uniform(0, 10, 60))])[:3]
    d = dist(par)
    ref = np.array([oracle.rimo_gamma_integral(d, 0, 0, 0, s, th, x) for x in n])
    for count in (1, 3):
        got = gpu_ctx.gamma_integral_batch(0, par, 0, 0, 0, s, th, n[:count])
        report_mismatch("gamma_integral, count %d" % count, got, ref[:count])

    rng = np.random.default_rng(31)
    par = [2.8, 1.0, 1e12, 1e10]
    s, th = 30., 0.9
    d = dist(par)
    lo = s * math.sin(th) + 31. + rng.uniform(0., 50., 24)
    hi = lo * rng.uniform(1.05, 3., 24)
    ref = np.array([oracle_bind.n_integral(oracle, d, 0, 0, 0, s, th, p, q) for p, q in zip(lo[:3], hi[:3])])
    for count in (1, 3):
        got = gpu_ctx.n_integral_batch(0, par, 0, 0, 0, s, th, lo[:count], hi[:count])
        report_mismatch("n_integral, count %d" % count, got, ref[:count])

    rng = np.random.default_rng(33)
    n0 = np.floor(s * math.sin(th) + 31. + rng.uniform(0., 400., 20))[:3]
    ref = np.array([oracle.rimo_symphony_deriv_probe(ctypes.byref(d), 0, 0, 0, s, th, float(x)) for x in n0])
    for count in (1, 3):
        got = gpu_ctx.deriv_probe_batch(0, par, 0, 0, 0, s, th, n0[:count])
        report_mismatch("deriv_central, count %d" % count, got, ref[:count])

    rng = np.random.default_rng(32)
    s, th = 8., 0.9
    gam = np.exp(rng.uniform(math.log(1.5), math.log(30.), 12))[:3]
    ref = np.array([oracle.rimo_gamma_contribution(ctypes.byref(d), 0, 0, s, th, float(x)) for x in gam])
    for count in (1, 3):
        got = gpu_ctx.gamma_contribution_batch(0, par, 0, 0, s, th, gam[:count])
        report_mismatch("gamma_contribution, count %d" % count, got, ref[:count])

    rng = np.random.default_rng(802)
    d = dist(hey_par)
    u = hey_outer_abscissae(rng, hey_s, hey_th, 0, 40)[:3]
    ref = np.array([oracle.rimo_hey_outer_integrand(ctypes.byref(d), 1, hey_s, hey_th, 0, float(x)) for x in u])
    for count in (1, 3):
        got = gpu_ctx.hey_outer_batch(0, hey_par, 1, hey_s, hey_th, 0, u[:count])
        report_mismatch("hey_outer, count %d" % count, got, ref[:count])
