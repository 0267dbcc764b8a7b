"""GPU test of the members' rule sums of the group kernel (symphony_group.h: group_rule_sums -- the rule's reductions per
served member, one tail for all members of a pass, lanes m / 32 + m filing): eight rows of each analytic kind and of the
isotropic tabulated form, under the masks that make full groups (0x3F), the I/Q group alone (0x0F), the V group alone
(0x30), a two-member I/Q group (0x0A) and a lone member in the group kernel (0x01, 0x10), carry the values and the
per-coefficient sample counts of the oracle's per-coefficient runs, and the values, status words and sample counts of one
wave per coefficient (RIMPHONY_SYM_SOLO=1).

The rows are those of tests/test_gpu_group_book_lanes.py (indices into the bench tables and into the committed tabulated
fixture): they hold gamma-integrals whose lists pass the 24 entries of their LDS part (power law 169, pitchy power law
23, kappa 2), round-off endings (thermal 675, 772) and NaN sums (thermal 47; tabulated 26, 34).  The full-mask launches
must have served several members per pass and filed stash entries (the group kernel's own counters).  Every launch runs
under a time limit."""
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
MASKS = (0x3F, 0x0F, 0x30, 0x0A, 0x01, 0x10)
ROWS = {
    "cfg2_powerlaw_8": [169, 202, 70, 152, 111, 26, 110, 8],
    "cfg3_thermal_8": [675, 772, 485, 1155, 1046, 99, 34, 47],
    "cfg4_pitchypl_8": [23, 183, 18, 249, 53, 250, 216, 16],
    "cfg5_pitchykappa_8": [2, 94, 86, 242, 181, 14, 248, 219],
}
TAB_ROWS = [10, 78, 162, 14, 26, 34, 42, 8]                             # of tests/golden/tabulated_det.npz


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
    """The oracle's per-coefficient runs of the analytic rows, once: values [n][6] and integrand samples [n][6]."""
    L = oracle
    jobs = []
    for cfg, rows in ROWS.items():
        kind, _, s, th, params = workload.make_rows(cfg, rows)
        for k in range(len(rows)):
            for slot in range(6):
                jobs.append((cfg, k, slot, kind, s[k], th[k], [p[k] for p in params]))

    def one(job):
        cfg, k, slot, kind, s, th, par = job
        d, _ = oracle_bind.mkdist(L, kind, par)
        c = oracle_bind.Counters()
        v = L.rimo_compute_dimensionless(d, slot & 1, slot >> 1, s, th, ctypes.byref(c))
        return cfg, k, slot, v, c.integrand_evals

    ref = {cfg: {"values": np.zeros((len(r), 6)), "work": np.zeros((len(r), 6), dtype=np.uint64)} for cfg, r in ROWS.items()}
    with ThreadPoolExecutor(16) as ex:
        for cfg, k, slot, v, n in ex.map(one, jobs):
            ref[cfg]["values"][k, slot], ref[cfg]["work"][k, slot] = v, n
    return ref


@pytest.fixture(scope="module")
def runs(gpu_ctx):
    """Every launch of this module, once: a context on the group kernels for the six masks and a context with one wave
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
                    if mask == 0x3F:
                        res[name, "sharing"] = dict(ctxs["group"].last_tail(), passes=ctxs["group"].last_work()["passes"])
                out, st, work = ctxs["solo"].compute_batch(kind, s, th, params, 0x3F, want_status=True, want_work=True)
                res[name, "solo", 0x3F] = (out, st, work.astype(np.uint64))
        finally:
            for c in ctxs.values():
                c.close()
    return res


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


@pytest.mark.parametrize("name", list(ROWS) + ["tabulated"])
def test_full_groups_served_members_together_and_filed_stash_entries(runs, name):
    sharing = runs[name, "sharing"]
    assert sharing["stash_filed"] > 0
    assert sharing["member_passes"] > sharing["passes"] > 0
