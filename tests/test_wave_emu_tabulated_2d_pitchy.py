"""The Symphony groups of the tabulated distribution as 2-D sets with a sin^k xi prefactor (symphony_group.h with
DIST_TABULATED_2D_PITCHY and DIST_TABULATED_2D_GRID_PITCHY) on the 64-thread wavefront emulator (tests/support/wave_emu.h),
against the committed bits and sample counts of the forms' table oracle: the check of the forms' lock-step path that needs no
GPU.  Slow (barrier-based collectives): only with RIMPHONY_SLOW=1, as test_wave_emu_tabulated_2d_grid.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import tab2d_pitchy_bind as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
pytestmark = pytest.mark.skipif(not os.environ.get("RIMPHONY_SLOW"), reason="set RIMPHONY_SLOW=1 (minutes per case)")


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "support", "wave_emu_2d_pitchy_driver.cpp")
    so = os.path.join(ROOT, "tests", "support", "wave_emu_2d_pitchy.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-mfma", "-msse4.1",
                    "-pthread", "-I" + os.path.join(ROOT, "tests", "support"), "-shared", src, "-o", so], check=True)
    E = ctypes.CDLL(so)
    E.emu_symphony_group_2d_pitchy.restype = ctypes.c_int
    E.emu_symphony_group_2d_pitchy.argtypes = [ctypes.c_int, ctypes.c_uint, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                               ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ulonglong)]
    return E


@pytest.mark.parametrize("which", [0, 1], ids=["U: 32 uniform x 8, k 0.5 2.5", "G: 64 log-gm1 x 9, k 1 0"])
def test_2d_pitchy_groups_in_emulator(emu, which):
    """The cheapest fixture row of each set whose six Symphony slots are finite: every member of both groups carries the
    oracle's bits, and the members' samples add up to its counts."""
    f = np.load(os.path.join(GOLDEN, "tabulated_2d_pitchy_det.npz"))
    if which == 0:
        where, t, k = (float(f["range_u"][0]), float(f["range_u"][1])), f["tables_u"], f["k_u"]
    else:
        where, t, k = f["gamma_g"], f["tables_g"], f["k_g"]
    assert tp.set_tables(where, t, k, with_norm=False) == 0 and tp.put_norms(f["norms"][which]) == 0
    blob = tp.blob()
    values, work = f["values"][which], f["work"][which]
    cost = np.where(np.isfinite(values[:, :6]).all(axis=1), work[:, :6].sum(axis=1).astype(np.int64), np.iinfo(np.int64).max)
    row = int(np.argmin(cost))
    norm = float(f["norms"][which][int(f["index"][row])])
    for group in ([0, 1, 2, 3], [4, 5]):
        slots = 0
        for i, sl in enumerate(group):
            slots |= sl << (4 * i)
        vals, stats, w = (ctypes.c_double * 4)(), (ctypes.c_int * 4)(), (ctypes.c_ulonglong * 48)()
        par = np.zeros(5)
        par[0] = f["index"][row]
        par[1:2] = np.array([blob.ctypes.data], dtype=np.uint64).view(np.float64)      # (coop_common.h: load_params)
        assert emu.emu_symphony_group_2d_pitchy(tp.form(), slots, len(group), float(f["s"][row]), float(f["theta"][row]),
                                                par.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), norm, vals, stats, w) == 1
        print("set", "UG"[which], "row", row, "slots", group, "samples", w[0], "executed passes", w[1], "member passes", w[3])
        for i, sl in enumerate(group):
            assert np.float64(vals[i]).view(np.uint64) == np.float64(values[row][sl]).view(np.uint64), (sl, vals[i], values[row][sl])
        assert w[0] == sum(int(work[row][sl]) for sl in group)
        assert w[3] >= w[1]
