"""The committed tables of the deterministic oracle WITH their status words (tests/golden/det_<cfg>.npz, written by
tools/make_det_fixtures.py) for the host and the GPU tests: loading, and the two blocks of a file as the arrays a batch call
takes.  Test infrastructure only."""
import os

import numpy as np

from rimphony_amd import workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ("cfg2_powerlaw_8", "cfg3_thermal_8", "cfg4_pitchypl_8", "cfg5_pitchykappa_8")
# include/rimphony_hip.h:74-80
ST_INNER_FAIL, ST_OUTER_FAIL, ST_CHUNK_CAP, ST_STORE_FULL, ST_NONFINITE, ST_NORM_FAIL, ST_NOT_COMPUTED = 1, 2, 4, 8, 16, 32, 64
_cache = {}


def path(cfg):
    return os.path.join(ROOT, "tests", "golden", "det_%s.npz" % cfg)


def load(cfg):
    """A file as a dict of arrays (read once; nobody writes to them)"""
    if cfg not in _cache:
        with np.load(path(cfg)) as f:
            _cache[cfg] = {k: f[k] for k in f.files}
        for v in _cache[cfg].values():
            v.setflags(write=False)
    return _cache[cfg]


def main_rows(cfg, idx=None):
    """(kind, s, theta, params, mask) of the main block, or of its rows idx"""
    f = load(cfg)
    rows = np.arange(int(f["start"]), int(f["start"]) + int(f["n"]), dtype=np.uint64)
    kind, _, s, th, params = workload.make_rows(cfg, rows if idx is None else rows[idx])
    return kind, s, th, params, int(f["mask"])


def extra_rows(cfg):
    """(kind, s, theta, params, mask) of the extra block"""
    f = load(cfg)
    p = f["extra_params"]
    return workload.CONFIGS[cfg][0], f["extra_s"].copy(), f["extra_theta"].copy(), [p[:, j].copy() for j in range(p.shape[1])], 0xFF


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def status_report(want, got, names):
    """The (wanted word -> got word) count table of two status arrays [rows][8], with the first three (row, slot) of each
    pair; names[i] says which row i is"""
    want, got = np.asarray(want).astype(np.int64), np.asarray(got).astype(np.int64)
    lines = []
    bad = np.argwhere(want != got)
    pairs = sorted({(int(want[i, k]), int(got[i, k])) for i, k in bad})
    for w, g in pairs:
        at = [(names[i], int(k)) for i, k in bad if want[i, k] == w and got[i, k] == g]
        lines.append("wanted %3d -> got %3d: %5d entries, first (row, slot) %s" % (w, g, len(at), at[:3]))
    return "\n".join(lines)
