"""GPU test of the side-by-side booking of the group kernel (symphony_group.h: group_book_turn): a few rows of each
analytic kind and of the isotropic tabulated form, under the masks that make full groups, the I/Q group alone, the V
group alone and a two-member I/Q group, carry the values and the per-coefficient sample counts of the oracle's
per-coefficient runs, and the values, status words and sample counts of one wave per coefficient (RIMPHONY_SYM_SOLO=1).

The rows are indices into the bench tables (workload.make_rows) and into the committed tabulated fixture, chosen with the
oracle's counters so that they contain: gamma-integrals whose list passes the 24 entries of its LDS part (the booking's
fallback), gamma-integrals that end in GSL's round-off status -- at 22 / 23 entries (row 675: side by side) and at 220
(row 772: in the spill region) --, and members of a group that finish a gamma-integral while the others go on.  The test
asserts these properties of the choice from the oracle's own counters.  Every launch runs under a time limit."""
import contextlib
import ctypes
import faulthandler
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_bind
from rimphony_amd import workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAB = 4
CAP_GINNER = 24
GSL_EROUND = 18
MASKS = (0x3F, 0x0F, 0x30, 0x05)
ROWS = {
    "cfg2_powerlaw_8": [169, 202, 70, 152, 111, 26, 110, 8],            # 169: a list of 25 entries
    "cfg3_thermal_8": [675, 772, 485, 1155, 1046, 99, 34, 47],          # 675 .. 1046: round-off; 99: 109 entries; 47: NaN sums
    "cfg4_pitchypl_8": [23, 183, 18, 249, 53, 250, 216, 16],            # 23: 30 entries
    "cfg5_pitchykappa_8": [2, 94, 86, 242, 181, 14, 248, 219],          # 2: 26 entries
}
ROUND_OFF_ROWS = {"cfg3_thermal_8": [675, 772, 485, 1155, 1046]}
TAB_ROWS = [10, 78, 162, 14, 26, 34, 42, 8]                             # of tests/golden/tabulated_det.npz (26, 34: NaN rows)


class Fail(ctypes.Structure):
    _fields_ = [("n", ctypes.c_double), ("a", ctypes.c_double), ("b", ctypes.c_double), ("result", ctypes.c_double),
                ("abserr", ctypes.c_double), ("lobe", ctypes.c_int), ("status", ctypes.c_int), ("size", ctypes.c_int),
                ("level", ctypes.c_int)]


@contextlib.contextmanager
def time_limit(seconds):
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def env_context(**env):
    from rimphony_amd import api
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return api.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def reference(oracle):
    """The oracle's per-coefficient runs of the analytic rows, once: values [n][6], integrand samples [n][6], the longest
    gamma-list [n][6] and whether a gamma-integral of the coefficient ended in the round-off status [n][6]."""
    L = oracle
    L.rimo_set_fail_log.argtypes = [ctypes.POINTER(Fail), ctypes.c_size_t]
    L.rimo_set_fail_log.restype = None
    L.rimo_fail_log_count.restype = ctypes.c_size_t
    jobs = []
    for cfg, rows in ROWS.items():
        kind, _, s, th, params = workload.make_rows(cfg, rows)
        for k in range(len(rows)):
            for slot in range(6):
                jobs.append((cfg, k, slot, kind, s[k], th[k], [p[k] for p in params]))

    def one(job):
        cfg, k, slot, kind, s, th, par = job
        d, _ = oracle_bind.mkdist(L, kind, par)
        log = (Fail * 64)()
        L.rimo_set_fail_log(log, 64)            # (the log belongs to the calling thread)
        c = oracle_bind.Counters()
        v = L.rimo_compute_dimensionless(d, slot & 1, slot >> 1, s, th, ctypes.byref(c))
        n_fail = min(int(L.rimo_fail_log_count()), 64)
        L.rimo_set_fail_log(None, 0)
        round_off = any(log[j].level == 0 and log[j].status == GSL_EROUND for j in range(n_fail))
        return cfg, k, slot, v, c.integrand_evals, c.max_inner_size, round_off

    ref = {cfg: {"values": np.zeros((len(r), 6)), "work": np.zeros((len(r), 6), dtype=np.uint64),
                 "longest": np.zeros((len(r), 6), dtype=int), "round_off": np.zeros((len(r), 6), dtype=bool)}
           for cfg, r in ROWS.items()}
    with ThreadPoolExecutor(16) as ex:
        for cfg, k, slot, v, n, longest, ro in ex.map(one, jobs):
            ref[cfg]["values"][k, slot], ref[cfg]["work"][k, slot] = v, n
            ref[cfg]["longest"][k, slot], ref[cfg]["round_off"][k, slot] = longest, ro
    return ref


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """Every launch of this module, once: a context on the group kernels for the four masks and a context with one wave
    per coefficient for the full mask, next to the session's context (touched first: both run in shared mode)."""
    res = {}
    f = np.load(os.path.join(ROOT, "tests", "golden", "tabulated_det.npz"))
    with time_limit(300):
        gpu_ctx.shared_mode()
        ctxs = {"group": env_context(RIMPHONY_TAB_GROUP="1"), "solo": env_context(RIMPHONY_SYM_SOLO="1")}
        try:
            for ctx in ctxs.values():
                ctx.set_tables(float(f["gamma_lo"]), float(f["gamma_hi"]), f["tables"])
            cases = {cfg: workload.make_rows(cfg, rows) for cfg, rows in ROWS.items()}
            cases["tabulated"] = (TAB, 0, f["s"][TAB_ROWS], f["theta"][TAB_ROWS], [f["index"][TAB_ROWS]])
            for name, (kind, _, s, th, params) in cases.items():
                for mask in MASKS:
                    out, st, work = ctxs["group"].compute_batch(kind, s, th, params, mask, want_status=True, want_work=True)
                    res[name, "group", mask] = (out, st, work.astype(np.uint64))
                out, st, work = ctxs["solo"].compute_batch(kind, s, th, params, 0x3F, want_status=True, want_work=True)
                res[name, "solo", 0x3F] = (out, st, work.astype(np.uint64))
        finally:
            for c in ctxs.values():
                c.close()
    return res


def test_the_rows_contain_what_they_were_chosen_for(reference):
    for cfg, ref in reference.items():
        assert (ref["longest"].max(axis=1) > CAP_GINNER).any(), cfg                 # a list beyond its LDS part
        iq = ref["work"][:, :4]
        assert (iq.min(axis=1) != iq.max(axis=1)).any(), cfg                        # members that needed different numbers of passes
    for cfg, rows in ROUND_OFF_ROWS.items():
        for row in rows:
            k = ROWS[cfg].index(row)
            assert reference[cfg]["round_off"][k].any(), (cfg, row)
    k = ROWS["cfg3_thermal_8"].index(675)           # round-off within the LDS part: booked side by side
    ro = reference["cfg3_thermal_8"]["round_off"][k]
    assert (reference["cfg3_thermal_8"]["longest"][k][ro] <= CAP_GINNER).all()
    k = ROWS["cfg3_thermal_8"].index(772)           # ... and far in the spill region: booked by the fallback
    ro = reference["cfg3_thermal_8"]["round_off"][k]
    assert (reference["cfg3_thermal_8"]["longest"][k][ro] > 64).all()


def _check(got, want_values, want_work, mask):
    out, _, work = got
    sel = [k for k in range(6) if mask & (1 << k)]
    unsel = [k for k in range(8) if not mask & (1 << k)]
    assert same_bits(out[:, sel], want_values[:, sel]).all()
    assert (work[:, sel] == want_work[:, sel]).all()
    assert np.isnan(out[:, unsel]).all()


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("cfg", list(ROWS))
def test_analytic_rows_against_the_oracle(runs, reference, cfg, mask):
    _check(runs[cfg, "group", mask], reference[cfg]["values"], reference[cfg]["work"], mask)


@pytest.mark.parametrize("mask", MASKS)
def test_tabulated_rows_against_the_oracle(runs, mask):
    f = np.load(os.path.join(ROOT, "tests", "golden", "tabulated_det.npz"))
    _check(runs["tabulated", "group", mask], f["values"][TAB_ROWS], f["work"][TAB_ROWS].astype(np.uint64), mask)


@pytest.mark.parametrize("name", list(ROWS) + ["tabulated"])
def test_against_one_wave_per_coefficient(runs, name):
    solo = runs[name, "solo", 0x3F]
    for mask in MASKS:
        sel = [k for k in range(6) if mask & (1 << k)]
        out, st, work = runs[name, "group", mask]
        assert same_bits(out[:, sel], solo[0][:, sel]).all(), hex(mask)
        assert (st[:, sel] == solo[1][:, sel]).all(), hex(mask)
        assert (work[:, sel] == solo[2][:, sel]).all(), hex(mask)
