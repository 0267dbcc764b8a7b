"""The committed tables of the deterministic oracle with their status words (tests/golden/det_<cfg>.npz,
tools/make_det_fixtures.py) against what they were made from, and the oracle's status entry against the entry it extends.
No GPU: the GPU side is tests/test_gpu_det_fixtures.py, which holds the kernels to these files word for word.

The status word is the one output of compute() the reference has no counterpart for, so what the files say is only worth
something if (a) the oracle entry that writes it leaves values and work alone, (b) the files are what that entry computes
today and (c) they hold the failure classes at all.  The floors of (c) are set under the census made when the fixtures were
introduced (profiles/det_fixture_census.txt)."""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import det_fixtures as df
import oracle_bind
from rimphony_amd import workload

SLOTS = [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 1), (2, 2)]        # (coefficient, stokes): rimphony_amd/api.py SLOTS
THREADS = min(16, os.cpu_count() or 1)
SAME_BITS_ROWS, FRESH_PER_CLASS, FRESH_MAIN_ROWS = 64, 8, 64


@pytest.mark.parametrize("cfg", df.CONFIGS)
def test_status_entry_changes_no_bit(oracle, cfg):
    """rimo_compute_dimensionless_st against rimo_compute_dimensionless on 64 rows of a kind, all eight slots: the same
    value bits, the work it reports is Counters.integrand_evals of the plain entry, bit 16 <=> NaN, and (Faraday, I) --
    which no slot asks for -- is NaN with NONFINITE | NOT_COMPUTED."""
    kind, _, s, th, params = workload.make_batch(cfg, SAME_BITS_ROWS, start=int(df.load(cfg)["start"]))
    values, status, work = oracle_bind.batch_st(oracle, kind, s, th, params, 0xFF, THREADS)

    def plain(t):
        i, k = divmod(t, 8)
        d, st = oracle_bind.mkdist(oracle, kind, [float(p[i]) for p in params])
        assert st == 0
        c = oracle_bind.Counters()
        v = oracle.rimo_compute_dimensionless(ctypes.byref(d), SLOTS[k][0], SLOTS[k][1], float(s[i]), float(th[i]), ctypes.byref(c))
        return v, c.integrand_evals

    with ThreadPoolExecutor(THREADS) as pool:
        res = list(pool.map(plain, range(SAME_BITS_ROWS * 8)))
    assert df.same_bits(values.ravel(), [r[0] for r in res]).all()
    assert (work.ravel() == np.array([r[1] for r in res], dtype=np.uint64)).all()
    assert (((status & df.ST_NONFINITE) != 0) == np.isnan(values)).all()
    d, _ = oracle_bind.mkdist(oracle, kind, [float(p[0]) for p in params])
    v, st, c = oracle_bind.compute_st(oracle, d, 2, 0, float(s[0]), float(th[0]))
    assert np.isnan(v) and st == (df.ST_NONFINITE | df.ST_NOT_COMPUTED) and c["integrand_evals"] == 0


def test_unselected_slots_and_failed_norm(oracle):
    """rimo_batch_st outside the selected slots: NaN, NONFINITE | NOT_COMPUTED, no work; with a normalisation that fails
    (a thermal T of NaN): NaN and NONFINITE | NORM_FAIL on the selected slots."""
    kind, _, s, th, params = workload.make_batch("cfg3_thermal_8", 2)
    values, status, work = oracle_bind.batch_st(oracle, kind, s, th, params, 0x41, 2)
    uns = [1, 2, 3, 4, 5, 7]
    assert np.isnan(values[:, uns]).all() and (status[:, uns] == (df.ST_NONFINITE | df.ST_NOT_COMPUTED)).all()
    assert (work[:, uns] == 0).all() and (work[:, [0, 6]] > 0).all()
    d, st = oracle_bind.mkdist(oracle, kind, [float("nan")])
    if st != 0:
        values, status, work = oracle_bind.batch_st(oracle, kind, s, th, [np.full(2, np.nan)], 0x41, 2)
        assert np.isnan(values).all() and (status[:, [0, 6]] == (df.ST_NONFINITE | df.ST_NORM_FAIL)).all()


def _fresh_main_rows(f):
    """Places in the main block: the first 8 rows of every (slot group, status word) present, at most 64 in all"""
    st = f["status"]
    picked = []
    for group in (slice(0, 6), slice(6, 8)):
        for word in np.unique(st[:, group]):
            picked += [int(i) for i in np.flatnonzero((st[:, group] == word).any(axis=1))[:FRESH_PER_CLASS]]
    return np.array(sorted(set(picked))[:FRESH_MAIN_ROWS], dtype=np.int64)


@pytest.mark.parametrize("cfg", df.CONFIGS)
def test_files_are_what_the_oracle_computes(oracle, cfg):
    """Freshness: every row of the extra block, and 8 rows of every status class of the main block (64 rows at the most),
    computed again: values, status words and work exactly.  The block is the literal fixture's, the flavour the library's."""
    f = df.load(cfg)
    assert str(f["flavour"]) == oracle.rimo_build_flavour().decode()
    with np.load(os.path.join(df.ROOT, "tests", "golden", "literal_%s.npz" % cfg)) as lit:
        assert (int(f["start"]), int(f["mask"])) == (int(lit["start"]), int(lit["mask"])) and 1024 <= int(f["n"]) <= int(lit["n"])
    assert os.path.getsize(df.path(cfg)) <= 420 * 1000
    idx = _fresh_main_rows(f)
    kind, s, th, params, mask = df.main_rows(cfg, idx)
    values, status, work = oracle_bind.batch_st(oracle, kind, s, th, params, mask, THREADS)
    assert df.same_bits(values, f["values"][idx]).all()
    assert (status == f["status"][idx]).all(), df.status_report(f["status"][idx], status, idx)
    assert (work == f["work"][idx]).all()
    kind, s, th, params, mask = df.extra_rows(cfg)
    values, status, work = oracle_bind.batch_st(oracle, kind, s, th, params, mask, THREADS)
    assert df.same_bits(values, f["extra_values"]).all()
    assert (status == f["extra_status"]).all(), df.status_report(f["extra_status"], status, np.arange(len(s)))
    assert (work == f["extra_work"]).all()


@pytest.mark.parametrize("cfg", df.CONFIGS)
def test_nan_iff_nonfinite_and_a_clean_majority(cfg):
    """In both blocks of a file: bit 16 <=> NaN, no bit the oracle cannot set (STORE_FULL, NORM_FAIL, NOT_COMPUTED: every
    slot is selected and every norm converges), and word 0 in a majority of the entries."""
    f = df.load(cfg)
    assert f["status"].dtype == np.uint8 and f["extra_status"].dtype == np.uint8
    assert f["values"].shape == f["status"].shape == f["work"].shape == (int(f["n"]), 8)
    assert f["extra_values"].shape == f["extra_status"].shape == f["extra_work"].shape == (len(f["extra_s"]), 8)
    st = np.concatenate([f["status"], f["extra_status"]])
    v = np.concatenate([f["values"], f["extra_values"]])
    assert (((st & df.ST_NONFINITE) != 0) == np.isnan(v)).all()
    assert ((st & (df.ST_STORE_FULL | df.ST_NORM_FAIL | df.ST_NOT_COMPUTED | 128)) == 0).all()
    assert (st == 0).sum() * 2 > st.size


def test_the_failure_classes_are_there():
    """A fixture without the classes proves nothing.  Faraday slots of the four main blocks: OUTER_FAIL alone (18) in at
    least 100 entries, INNER_FAIL + OUTER_FAIL (19) in at least 400, CHUNK_CAP (20) in at least 4.  Symphony slots of the
    thermal main block: 19 in at least 300 entries.  Symphony slots of the extra blocks: 18 in at least 4 entries, 19 in at
    least 200.

    What the files do NOT hold (profiles/det_fixture_census.txt): an entry with INNER_FAIL and without OUTER_FAIL.  The
    search of 6144 further table rows per kind (Faraday slots) and 1536 (Symphony slots) found neither a finite value with
    a nonzero word nor a NaN with INNER_FAIL alone, so a kernel that set OUTER_FAIL wherever it sets INNER_FAIL is not
    told apart from the contract by these files."""
    faraday = np.concatenate([df.load(cfg)["status"][:, 6:].ravel() for cfg in df.CONFIGS])
    assert (faraday == 18).sum() >= 100 and (faraday == 19).sum() >= 400 and (faraday == 20).sum() >= 4, np.unique(faraday, return_counts=True)
    thermal = df.load("cfg3_thermal_8")["status"][:, :6]
    assert (thermal == 19).sum() >= 300, np.unique(thermal, return_counts=True)
    extra = np.concatenate([df.load(cfg)["extra_status"][:, :6].ravel() for cfg in df.CONFIGS])
    assert (extra == 18).sum() >= 4 and (extra == 19).sum() >= 200, np.unique(extra, return_counts=True)
