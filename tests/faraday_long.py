"""The committed fixture of the long Faraday outer quadratures (tests/golden/faraday_long_det.npz, written by
tools/make_faraday_long_fixture.py) for the host and the GPU tests: loading, the size classes, and the rows of a kind as the
arrays a batch call takes.  Test infrastructure only."""
import os

import numpy as np

import oracle_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "faraday_long_det.npz")
SLOTS = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 1), (2, 2)]        # (coefficient, stokes): rimphony_amd/api.py SLOTS
# the lengths of the outer subinterval list at which the kernels change what they do
ROUND_MIN = 48              # RIM_ROUND_MIN_SIZE, heyvaerts_wave.h: rounds (pitchy-kappa)
CAP_OUTER = 64              # rimphony_internal.h: the list leaves LDS
LIMIT = 4096                # heyvaerts.rs:82-83: the quadrature gives up
HALF = LIMIT // 2 + 2       # qpsrt.c: GSL's order list is no longer fully sorted
CONFIGS = ("cfg2_powerlaw_8", "cfg3_thermal_8", "cfg4_pitchypl_8", "cfg5_pitchykappa_8")
_cache = {}


def load():
    """The fixture as a dict of arrays (read once; nobody writes to them)"""
    if not _cache:
        with np.load(PATH) as f:
            _cache.update({k: f[k] for k in f.files})
        for v in _cache.values():
            v.setflags(write=False)
    return _cache


def index_of(config, row):
    f = load()
    return int(np.flatnonzero((f["config"] == config) & (f["row"] == row))[0])


def rows_of(config, classes):
    """(idx, s, theta, params) of the fixture's rows of a config whose class is in `classes`: idx their places in the fixture"""
    f = load()
    idx = np.flatnonzero((f["config"] == config) & np.isin(f["cls"], classes))
    n = int(f["nparams"][idx[0]]) if len(idx) else 0
    return idx, f["s"][idx].copy(), f["theta"][idx].copy(), [f["params"][idx, j].copy() for j in range(n)]


def recompute(L, i, slot):
    """(value, Counters dict, status word) of slot `slot` of fixture row i by the oracle library L"""
    f = load()
    kind = {c: k for k, c in enumerate(CONFIGS)}[str(f["config"][i])]
    d, st = oracle_bind.mkdist(L, kind, [float(x) for x in f["params"][i, :int(f["nparams"][i])]])
    assert st == 0
    co, stk = SLOTS[slot]
    v, status, c = oracle_bind.compute_st(L, d, co, stk, float(f["s"][i]), float(f["theta"][i]))
    return v, c, status
