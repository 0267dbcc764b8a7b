"""GPU tests of compute() against the committed tables of the deterministic CPU oracle WITH their status words
(tests/golden/det_<cfg>.npz, tools/make_det_fixtures.py): 2048 rows of each bench table and an extra block of rows off the
tables (distributions cut inside the sampled range, the small-angle corner, an endless marching loop, what a search found).
Every output word of a launch is held to the oracle's: the values bit for bit with the NaN pattern, the per-slot work, the
launch's sample counts and the FULL status word of all eight slots -- the reason bits say why a coefficient is NaN
(status_histogram, tools/nan_map.py), and the oracle sets them from the restated reference's own control flow
(oracle/rimo_symphony.c rimo_compute_dimensionless_st), not from anything the kernels do.  No oracle runs here."""
import contextlib
import faulthandler
import sys

import numpy as np
import pytest

import det_fixtures as df

pytestmark = pytest.mark.gpu
LAUNCH_LIMIT = 240          # seconds (faulthandler ends the process)


@contextlib.contextmanager
def time_limit(seconds):
    """Ends the process (with a traceback of every thread) if the body -- GPU work that may block inside the runtime,
    where no Python exception can reach -- is still running after `seconds`."""
    faulthandler.dump_traceback_later(seconds, exit=True, file=sys.stderr)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def check(ctx, what, rows, want_values, want_status, want_work, names):
    kind, s, th, params, mask = rows
    with time_limit(LAUNCH_LIMIT):
        out, st, work = ctx.compute_batch(kind, s, th, params, mask, want_status=True, want_work=True)
        w = ctx.last_work()
    assert mask == 0xFF
    ok = df.same_bits(out, want_values)
    work = work.astype(np.uint64)
    same_status = st.astype(np.int64) == want_status.astype(np.int64)
    print(what, "%d rows: %d values, %d work words, %d status words differ; samples %d + %d (fixture %d + %d)" % (
        len(s), (~ok).sum(), (work != want_work).sum(), (~same_status).sum(), w["samples"], w["faraday_samples"],
        int(want_work[:, :6].sum(dtype=np.uint64)), int(want_work[:, 6:].sum(dtype=np.uint64))))
    if not same_status.all():
        print(df.status_report(want_status, st, names))
    assert ok.all(), [(names[i], int(k), out[i, k], want_values[i, k]) for i, k in np.argwhere(~ok)[:8]]
    assert (work == want_work).all(), [(names[i], int(k), int(work[i, k]), int(want_work[i, k])) for i, k in np.argwhere(work != want_work)[:8]]
    assert same_status.all(), df.status_report(want_status, st, names)
    assert w["samples"] == int(want_work[:, :6].sum(dtype=np.uint64))
    assert w["faraday_samples"] == int(want_work[:, 6:].sum(dtype=np.uint64))


@pytest.mark.parametrize("cfg", df.CONFIGS)
def test_main_block_carries_every_word(gpu_ctx, cfg):
    """The main block of a table, all eight slots, in one launch (the block of the literal-flavour fixture): values, work,
    sample counts and the full status word of every slot are the oracle's."""
    f = df.load(cfg)
    start = int(f["start"])
    check(gpu_ctx, "main " + cfg, df.main_rows(cfg), f["values"], f["status"], f["work"].astype(np.uint64),
          ["table row %d" % (start + i) for i in range(int(f["n"]))])


@pytest.mark.parametrize("cfg", df.CONFIGS)
def test_extra_block_carries_every_word(gpu_ctx, cfg):
    """The extra block of a kind in one launch, held to the same: the classes the bench rows do not reach (OUTER_FAIL
    alone on a Symphony slot, CHUNK_CAP after 4096 steps and at once, INNER_FAIL + OUTER_FAIL at a rate of a third)."""
    f = df.load(cfg)
    check(gpu_ctx, "extra " + cfg, df.extra_rows(cfg), f["extra_values"], f["extra_status"], f["extra_work"].astype(np.uint64),
          ["extra row %d (%s)" % (i, t) for i, t in enumerate(f["extra_tag"])])
