"""The booking of a turn of the group quadrature (symphony_group.h) on the wavefront emulator: group_book_turn --
group_book_lanes, all members side by side, and its fallback -- against group_book member by member on identical LDS
images.  The member records, the lists and the spill regions must come out byte-identical, the finished and need-pick
masks equal.

A turn books either the members that picked the pass's interval (sums in the hand-over record) or, without a pass, the
members whose pick was on file in their stash: wave_qag_group never has both in one turn, so the mix of the two kinds is
a mix of turns here, each with members at different imax."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP, CAP, STASH, SPILL = 4, 24, 8, 5000
SUCCESS, EFAILED, EMAXITER, EROUND, ESING, ESTORE = 0, 5, 11, 18, 21, 1001
EPSREL, LIMIT = 1e-3, 5000
DBL_EPSILON, DBL_MIN = 2.2204460492503131e-16, 2.2250738585072014e-308


class Member(ctypes.Structure):
    _fields_ = [("area", ctypes.c_double), ("errsum", ctypes.c_double), ("fb", ctypes.c_double * 8),
                ("res", ctypes.c_double * 2), ("qst", ctypes.c_int * 2),
                ("iteration", ctypes.c_int), ("size", ctypes.c_int), ("rt1", ctypes.c_int), ("rt2", ctypes.c_int),
                ("imax", ctypes.c_int), ("samples", ctypes.c_uint),
                ("sk", ctypes.c_int * STASH), ("sf", ctypes.c_int * STASH),
                ("sr1", ctypes.c_double * STASH), ("se1", ctypes.c_double * STASH),
                ("sr2", ctypes.c_double * STASH), ("se2", ctypes.c_double * STASH),
                ("snext", ctypes.c_int), ("hf", ctypes.c_int)]


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "support", "group_book_driver.cpp")
    so = os.path.join(ROOT, "tests", "support", "group_book_emu.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-mfma", "-msse4.1",
                    "-pthread", "-I" + os.path.join(ROOT, "tests", "support"), "-shared", src, "-o", so], check=True)
    E = ctypes.CDLL(so)
    assert E.emu_group_member_size() == ctypes.sizeof(Member) == 456
    assert E.emu_group_list_doubles() == 4 * CAP + CAP // 2
    assert E.emu_group_spill_doubles() == 4 * SPILL + SPILL // 2
    E.emu_group_book_compare.restype = ctypes.c_int
    E.emu_group_book_compare.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint,
                                         ctypes.c_int, ctypes.c_uint, ctypes.c_double, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_uint)]
    return E


class Turn:
    """The LDS image before a booking: four member records, their lists and spill regions."""

    def __init__(self, cur=0, stash=False):
        self.mem = (Member * GROUP)()
        self.lists = np.zeros((GROUP, 4 * CAP + CAP // 2))
        self.spill = np.zeros((GROUP, 4 * SPILL + SPILL // 2))
        self.cur, self.stash, self.set, self.posp = cur, stash, 0, 0
        for m in range(GROUP):
            for k in range(STASH):
                self.mem[m].sk[k] = -1

    def entry(self, m, i, a, b, r, e, stamp):
        if i < CAP:
            self.lists[m, [i, CAP + i, 2 * CAP + i, 3 * CAP + i]] = (a, b, r, e)
            self.lists[m, 4 * CAP:].view(np.int32)[i] = stamp
        else:
            j = i - CAP
            self.spill[m, [j, SPILL + j, 2 * SPILL + j, 3 * SPILL + j]] = (a, b, r, e)
            self.spill[m, 4 * SPILL:].view(np.int32)[j] = stamp

    def member(self, m, size, imax, parent, sums, fl=3, area=1.0, errsum=0.1, iteration=None, rt1=0, rt2=0, pos=0,
               rng=None):
        """Member m with a list of `size` entries whose entry imax is `parent` = (a, b, r, e); sums = the children's
        (result1, abserr1, result2, abserr2), fl their flags."""
        rng = rng or np.random.default_rng(1000 + m)
        M = self.mem[m]
        for i in range(min(size, CAP + 16)):
            a = rng.uniform(1., 10.)
            self.entry(m, i, a, a + rng.uniform(0.01, 1.), rng.normal(), abs(rng.normal()) * 1e-2, i)
        self.entry(m, imax, *parent, 2 * imax)
        M.area, M.errsum = area, errsum
        M.iteration = size if iteration is None else iteration
        M.size, M.rt1, M.rt2, M.imax, M.samples = size, rt1, rt2, imax, 31 + 62 * (size - 1)
        M.res[self.cur], M.qst[self.cur] = -7., -7
        if self.stash:
            for k in range(STASH):          # other entries on file around the pick
                M.sk[k] = (imax + 1 + k) if k != pos else imax
                M.sf[k], M.sr1[k], M.se1[k], M.sr2[k], M.se2[k] = k & 3, 100. + k, 200. + k, 300. + k, 400. + k
            M.sf[pos], M.sr1[pos], M.se1[pos], M.sr2[pos], M.se2[pos] = fl, *sums
            self.posp |= pos << (4 * m)
        else:
            for k in range(4):
                M.fb[4 * self.cur + k] = sums[k]
                M.fb[4 * (1 - self.cur) + k] = 50. + k      # the other integral's first-rule sums: not to be touched
            M.hf = fl
        self.set |= 1 << m
        return self

    def run(self, E, epsrel=EPSREL, limit=LIMIT):
        out = (ctypes.c_uint * 5)()
        before = bytes(self.mem)
        diff = E.emu_group_book_compare(ctypes.byref(self.mem), self.lists.ctypes.data, self.spill.ctypes.data, self.cur,
                                        self.set, int(self.stash), self.posp, epsrel, limit, out)
        assert diff == 0, "records / lists / spill regions differ: mask %d" % diff
        assert (out[0], out[1]) == (out[2], out[3])
        assert out[0] | out[1] == self.set and out[0] & out[1] == 0
        assert bytes(self.mem) != before
        self.finished, self.lanes = out[0], bool(out[4])
        return self


PARENT = (1.0, 2.0, 0.5, 0.05)
GOING_ON = (0.26, 0.04, 0.25, 0.03)          # errsum stays above the tolerance, no round-off mark


@pytest.mark.parametrize("stash", [False, True])
@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("members", [0x1, 0x3, 0x7, 0xF, 0xA, 0x8])
def test_one_to_four_members_at_different_imax(emu, members, cur, stash):
    t = Turn(cur, stash)
    for m in range(GROUP):
        if (members >> m) & 1:
            t.member(m, size=5 + 4 * m, imax=1 + 3 * m, parent=(1. + m, 2. + m, 0.5 * (m + 1), 0.05), sums=GOING_ON, pos=(3 * m + 1) % 8)
    t.run(emu)
    assert t.lanes and t.finished == 0
    for m in range(GROUP):
        if (members >> m) & 1:
            assert t.mem[m].size == 6 + 4 * m and t.mem[m].samples == 31 + 62 * (5 + 4 * m)
            assert t.mem[m].qst[cur] == -7
            if stash:
                assert t.mem[m].sk[(3 * m + 1) % 8] == -1


@pytest.mark.parametrize("stash", [False, True])
def test_one_member_finishes_while_the_others_go_on(emu, stash):
    t = Turn(0, stash)
    t.member(0, 6, 2, PARENT, GOING_ON).member(2, 9, 7, PARENT, GOING_ON, pos=5)
    t.member(1, 7, 3, PARENT, (0.25, 1e-5, 0.25, 1e-5), errsum=0.05 + 1e-4, pos=2)      # errsum 1.2e-4 <= 1e-3 * |area|
    t.run(emu)
    assert t.lanes and t.finished == 0x2
    assert t.mem[1].qst[0] == SUCCESS
    assert t.mem[1].res[0] == np.cumsum(t.lists[1, 2 * CAP:2 * CAP + 8])[-1]           # qag.c's sum over rlist, in order


def test_equal_errors_keep_child_one_in_the_parents_slot(emu):
    for stash in (False, True):
        t = Turn(1, stash).member(0, 6, 2, PARENT, (0.26, 0.04, 0.25, 0.04)).member(3, 8, 0, PARENT, (0.26, 0.03, 0.25, 0.04)).run(emu)
        assert t.lanes
        assert t.lists[0, 2] == 1.0 and t.lists[0, CAP + 2] == 1.5 and t.lists[0, 6] == 1.5        # child 1 kept slot imax
        assert t.lists[3, 0] == 1.5 and t.lists[3, 8] == 1.0                                       # child 2 (larger error) did


def test_nan_sums(emu):
    nan = float("nan")
    for sums in [(nan, 0.04, 0.25, 0.03), (0.26, nan, 0.25, 0.03), (0.26, 0.04, nan, nan), (nan,) * 4]:
        for stash in (False, True):
            t = Turn(0, stash).member(0, 6, 2, PARENT, sums).member(1, 6, 4, PARENT, GOING_ON).run(emu)
            assert t.lanes and t.finished == 0x1
            assert t.mem[0].qst[0] == EFAILED           # a NaN error sum or tolerance is a failure, never a success
    t = Turn(0).member(0, 6, 2, (1.0, 2.0, nan, nan), GOING_ON).member(1, 6, 4, PARENT, GOING_ON, area=nan).run(emu)
    assert t.lanes and t.finished == 0x3


def test_errsum_equal_to_the_tolerance_is_a_success(emu):
    tol = EPSREL * 1024.0
    for stash in (False, True):
        t = Turn(0, stash)
        t.member(0, 6, 2, (1.0, 2.0, 0.0, 0.0), (512., tol / 2, 512., tol / 2), area=0., errsum=0.)
        t.member(1, 6, 2, (1.0, 2.0, 0.0, 0.0), (512., np.nextafter(tol / 2, 1.), 512., np.nextafter(tol / 2, 1.)), area=0., errsum=0.)      # one ulp above
        t.run(emu)
        assert t.lanes and t.finished == 0x1 and t.mem[0].qst[0] == SUCCESS and t.mem[0].errsum == tol


def test_round_off_counters(emu):
    same = (0.25, 0.03, 0.25, 0.03)             # area12 == r_i and error12 >= 0.99 e_i: a mark of rt1; error12 > e_i: of rt2
    for stash in (False, True):
        t = Turn(0, stash)
        t.member(0, 12, 2, PARENT, same, rt1=5)                         # 5 -> 6: round-off
        t.member(1, 12, 3, PARENT, same, rt1=4)                         # 4 -> 5: goes on
        t.member(2, 12, 4, PARENT, same, rt1=5, fl=1)                   # resasc == abserr on one child: no mark
        t.member(3, 12, 5, (1.0, 2.0, 0.5, 5e-4), (0.25, 2.5e-4, 0.25, 2.5e-4), rt1=5, errsum=5e-4)    # a mark, but converged
        t.run(emu)
        assert t.lanes and t.finished == 0x9
        assert [t.mem[m].rt1 for m in range(4)] == [6, 5, 5, 6]
        assert t.mem[0].qst[0] == EROUND and t.mem[3].qst[0] == SUCCESS
        t = Turn(1, stash)
        t.member(0, 12, 2, PARENT, GOING_ON, rt2=19, iteration=10)      # 19 -> 20 at iteration 10: round-off
        t.member(1, 12, 2, PARENT, GOING_ON, rt2=19, iteration=9)       # iteration 9: not counted
        t.member(2, 12, 2, PARENT, GOING_ON, rt2=18, iteration=400)     # 18 -> 19
        t.member(3, 12, 2, PARENT, (0.26, 0.02, 0.25, 0.02), rt2=19, iteration=400)         # error12 < e_i: no mark
        t.run(emu)
        assert t.lanes and t.finished == 0x1 and t.mem[0].qst[1] == EROUND
        assert [t.mem[m].rt2 for m in range(4)] == [20, 19, 19, 19]


def test_last_iteration_and_singular_interval(emu):
    for stash in (False, True):
        t = Turn(0, stash)
        t.member(0, 12, 2, PARENT, GOING_ON, iteration=LIMIT - 1)
        t.member(1, 12, 2, PARENT, GOING_ON, iteration=LIMIT - 2)
        t.member(2, 12, 2, (1e-310, 2e-310, 0.5, 0.05), GOING_ON)      # |a_i|, |b_i| <= tmp: error type 3
        t.member(3, 12, 2, (1e-310, 2e-310, 0.5, 0.05), GOING_ON, rt1=6)                   # ... which overrides type 2
        t.run(emu)
        assert t.lanes and t.finished == 0xD
        assert t.mem[0].qst[0] == EMAXITER and t.mem[2].qst[0] == ESING and t.mem[3].qst[0] == ESING
        t = Turn(0, stash).member(0, 6, 2, PARENT, GOING_ON, iteration=6).run(emu, limit=7)
        assert t.finished == 0x1 and t.mem[0].qst[0] == EMAXITER


def test_lists_at_the_end_of_their_lds_part_take_the_fallback(emu):
    for stash in (False, True):
        t = Turn(0, stash).member(0, CAP - 1, 5, PARENT, (0.26, 0.03, 0.25, 0.04)).member(1, 6, 2, PARENT, GOING_ON).run(emu)
        assert t.lanes and t.mem[0].size == CAP and t.lists[0, CAP - 1] == 1.0      # child 1 in the LDS part's last entry
        t = Turn(0, stash).member(0, CAP, 5, PARENT, (0.26, 0.03, 0.25, 0.04)).member(1, 6, 2, PARENT, GOING_ON).run(emu)
        assert not t.lanes and t.mem[0].size == CAP + 1 and t.spill[0, 0] == 1.0    # ... in the spill region's first
        t = Turn(0, stash).member(1, CAP + 9, CAP + 3, PARENT, GOING_ON).member(2, CAP - 1, CAP - 2, PARENT, GOING_ON).run(emu)
        assert not t.lanes and t.finished == 0
        t = Turn(0, stash).member(0, CAP + SPILL, 5, PARENT, GOING_ON, iteration=40).member(3, 6, 2, PARENT, GOING_ON).run(emu)
        assert not t.lanes and t.finished == 0x1 and t.mem[0].qst[0] == ESTORE and t.mem[0].size == CAP + SPILL


def test_seeded_random_states(emu):
    rng = np.random.default_rng(20240607)
    n_lanes = n_fin = 0
    for case in range(96):
        t = Turn(int(rng.integers(2)), bool(rng.integers(2)))
        members = int(rng.integers(1, 16))
        for m in range(GROUP):
            if not (members >> m) & 1:
                continue
            size = int(rng.integers(1, CAP)) if rng.random() < 0.9 else int(rng.integers(CAP, CAP + 12))
            imax = int(rng.integers(size))
            a = rng.uniform(-3., 3.)
            r_i, e_i = rng.normal(), abs(rng.normal()) * 10. ** rng.integers(-6, 0)
            split = rng.uniform(0.3, 0.7)
            noise = 10. ** rng.integers(-9, -1)
            sums = [r_i * split * (1 + noise * rng.normal()), e_i * rng.uniform(0., 0.8),
                    r_i * (1 - split), e_i * rng.uniform(0., 0.8)]
            if rng.random() < 0.15:
                sums[2] = r_i - sums[0]                 # area12 ~ r_i
            if rng.random() < 0.1:
                sums[3] = sums[1]
            if rng.random() < 0.05:
                sums[int(rng.integers(4))] = float("nan")
            t.member(m, size, imax, (a, a + rng.uniform(1e-3, 2.), r_i, e_i), sums, fl=int(rng.integers(4)) if rng.random() < 0.4 else 3,
                     area=r_i * rng.uniform(0.5, 20.), errsum=e_i * rng.uniform(1., 1.02) if rng.random() < 0.4 else e_i * rng.uniform(1., 30.),
                     iteration=int(rng.integers(max(1, size - 1), size + 14)), rt1=int(rng.integers(0, 7)), rt2=int(rng.integers(12, 21)),
                     pos=int(rng.integers(STASH)), rng=rng)
        t.run(emu)
        n_lanes += t.lanes
        n_fin += t.finished != 0
    assert n_lanes > 48 and n_fin > 8         # the states exercise the side-by-side path, finished members included
