"""The Symphony groups of the tabulated distribution (symphony_group.h with DIST_TABULATED_ISO and DIST_TABULATED_2D) on the
64-thread wavefront emulator (tests/support/wave_emu.h), against the committed bits and sample counts of the table oracles:
the check of the lock-step path of the kind that needs no GPU.  Slow (barrier-based collectives): only with RIMPHONY_SLOW=1,
as test_wave_emu.py."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import tab2d_bind
import tab_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.skipif(not os.environ.get("RIMPHONY_SLOW"), reason="set RIMPHONY_SLOW=1 (minutes per case)")
DIST_TABULATED_ISO, DIST_TABULATED_2D = 5, 6            # dev_symphony.h


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "support", "wave_emu_tab_driver.cpp")
    so = os.path.join(ROOT, "tests", "support", "wave_emu_tab.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-mfma", "-msse4.1",
                    "-pthread", "-I" + os.path.join(ROOT, "tests", "support"), "-shared", src, "-o", so], check=True)
    E = ctypes.CDLL(so)
    E.emu_symphony_group_tab.restype = ctypes.c_int
    E.emu_symphony_group_tab.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                         ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ulonglong)]
    return E


def cheapest_row(values, work):
    """the fixture row with the fewest Symphony samples among those whose six Symphony slots are all finite"""
    cost = np.where(np.isfinite(values[:, :6]).all(axis=1), work[:, :6].sum(axis=1), np.iinfo(np.int64).max)
    return int(np.argmin(cost))


def _run_group(E, kind, blob, index, norm, slots_list, s, th, want, want_work):
    """The assertions of test_wave_emu.py::_run_group against the oracle's committed row: every member carries its bits, the
    members' samples add up to its counts, member passes >= executed passes."""
    slots = 0
    for i, sl in enumerate(slots_list):
        slots |= sl << (4 * i)
    vals, stats, w = (ctypes.c_double * 4)(), (ctypes.c_int * 4)(), (ctypes.c_ulonglong * 48)()
    par = np.zeros(5)
    par[0] = index
    par[1:2] = np.array([blob.ctypes.data], dtype=np.uint64).view(np.float64)      # (coop_common.h: load_params)
    assert E.emu_symphony_group_tab(kind, slots, len(slots_list), s, th, par.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    norm, vals, stats, w) == 1
    total = 0
    for i, sl in enumerate(slots_list):
        total += int(want_work[sl])
        assert np.float64(vals[i]).view(np.uint64) == np.float64(want[sl]).view(np.uint64), (sl, vals[i], want[sl])
    print("kind", kind, "slots", slots_list, "samples", w[0], "executed passes", w[1], "member passes", w[3])
    assert w[0] == total
    assert w[3] >= w[1]


def test_isotropic_groups_in_emulator(emu):
    f = np.load(os.path.join(GOLDEN, "tabulated_det.npz"))
    assert tab_bind.set_tables(float(f["gamma_lo"]), float(f["gamma_hi"]), f["tables"]) == 0
    blob = tab_bind.blob()
    row = cheapest_row(f["values"][:24], f["work"][:24])
    norm = float(tab_bind.batch_norm([f["index"][row]])[0])
    for group in ([0, 1, 2, 3], [4, 5]):
        _run_group(emu, DIST_TABULATED_ISO, blob, f["index"][row], norm, group, float(f["s"][row]), float(f["theta"][row]),
                   f["values"][row], f["work"][row])


def test_2d_groups_in_emulator(emu):
    f = np.load(os.path.join(GOLDEN, "tabulated_2d_det.npz"))
    n_nodes, n_mu = (int(x) for x in f["geometry"][0])
    t = tab2d_bind.edge_tables_2d(n_nodes, n_mu, f["cols_0"])
    assert tab2d_bind.set_tables(float(f["gamma_lo"]), float(f["gamma_hi"]), t) == 0
    blob = tab2d_bind.blob()
    row = cheapest_row(f["values"][0], f["work"][0])
    norm = float(tab2d_bind.batch_norm([f["index"][row]])[0])
    for group in ([0, 1, 2, 3], [4, 5]):
        _run_group(emu, DIST_TABULATED_2D, blob, f["index"][row], norm, group, float(f["s"][row]), float(f["theta"][row]),
                   f["values"][0][row], f["work"][0][row])


def test_noise_above_the_order_in_emulator(emu):
    """theta = pi/2 exactly (cos theta = 6.1e-17) on table 0 of the 64-node edge set: z is rounding noise far above the
    order, sym_bessel_pair has no value there, and sym_eval_group of the tabulated kinds evaluates the entry again through
    the complete Bessel functions, as sym_eval_pair does.  The oracle's NaNs and its 1426 / 2728 samples per coefficient
    (without the second evaluation: 2046 / 3968)."""
    lo, hi = 1.01, 1e4
    assert tab_bind.set_tables(lo, hi, tab_bind.edge_tables(lo, hi, 64)) == 0
    blob = tab_bind.blob()
    s, th = 10.0, math.pi / 2
    want, want_work = tab_bind.batch(np.array([s]), np.array([th]), np.zeros(1))
    assert (want_work[0, :4] == 1426).all() and (want_work[0, 4:6] == 2728).all()
    norm = float(tab_bind.batch_norm([0.0])[0])
    for group in ([0, 1, 2, 3], [4, 5]):
        _run_group(emu, DIST_TABULATED_ISO, blob, 0.0, norm, group, s, th, want[0], want_work[0])
