"""The members' part of a pass of the group quadrature (symphony_group.h: group_rule_sums) on the wavefront emulator:
the rule's reductions per served member, ONE tail for all of them (lane m doing member m's child 1, lane 32 + m its
child 2) and lanes m / 32 + m filing -- against the member-by-member form (wave_gk31 per served member, lanes 0 / 32
filing; restated in tests/support/group_rule_tails_driver.cpp) on identical LDS images and identical per-lane sample
vectors.  The member records -- fb, hf, the stash sk / sf / sr1 / se1 / sr2 / se2 / snext, samples -- must come out
byte-identical, and so must the pass's counters.

The pick loop is not covered here: taking the members' picks two at a time (one list per half-wave) was built, measured
slower on the GPU and removed again (profiles/group_rule_tails_ab.txt), so the picks are the code they were."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP, STASH = 4, 8
DBL_EPSILON, DBL_MIN = 2.2204460492503131e-16, 2.2250738585072014e-308
SETS = [0x1, 0x3, 0x7, 0xF, 0xA, 0x8]


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
    src = os.path.join(ROOT, "tests", "support", "group_rule_tails_driver.cpp")
    so = os.path.join(ROOT, "tests", "support", "group_rule_tails_emu.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-mfma", "-msse4.1",
                    "-pthread", "-I" + os.path.join(ROOT, "tests", "support"), "-shared", src, "-o", so], check=True)
    E = ctypes.CDLL(so)
    assert E.emu_group_member_size() == ctypes.sizeof(Member) == 456
    E.emu_group_rule_tails_compare.restype = ctypes.c_int
    E.emu_group_rule_tails_compare.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_uint,
                                               ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p,
                                               ctypes.POINTER(ctypes.c_uint)]
    E.emu_rule_apply.restype = None
    E.emu_rule_apply.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    return E


def smooth(rng, scale=1.0):
    """64 samples of a smooth integrand with some structure: one per lane (lanes 31 and 63 are padding)."""
    x = np.linspace(-1., 1., 64)
    return scale * (rng.uniform(0.5, 2.) + rng.normal() * x + rng.normal() * np.cos(rng.uniform(1., 9.) * x))


class Pass:
    """The LDS image before the members' part of a pass, and the pass's uniform words."""

    def __init__(self, cur, serve, booknow=0, maskA=0, maskB=0, hl=(0.25, 0.25), seed=1):
        rng = np.random.default_rng(seed)
        self.mem = (Member * GROUP)()
        self.cur, self.serve, self.booknow, self.maskA, self.maskB = cur, serve, booknow, maskA, maskB
        self.hl = np.array(hl, dtype=np.float64)
        self.fv = np.stack([smooth(rng) for _ in range(GROUP)])
        self.idx = [3 + 5 * m for m in range(GROUP)]
        self.counts = [0x5 & ~serve, 1000, 20, 4, 7]
        for m in range(GROUP):          # every field holds something recognisable: what a pass must not touch shows
            M = self.mem[m]
            M.area, M.errsum, M.samples, M.snext, M.hf = 10. + m, 20. + m, 31 + 62 * m, (3 + m) % STASH, 2
            M.iteration, M.size, M.rt1, M.rt2, M.imax = 7 + m, 8 + m, 1, 2, 3 + m
            for k in range(8):
                M.fb[k] = 50. + 8 * m + k
            for k in range(STASH):
                M.sk[k], M.sf[k] = -1, k & 3
                M.sr1[k], M.se1[k], M.sr2[k], M.se2[k] = 100. + k, 200. + k, 300. + k, 400. + k

    def stash_keys(self, m, keys):
        for k, key in enumerate(keys):
            self.mem[m].sk[k] = key
        return self

    def run(self, E):
        idxp = sum(self.idx[m] << (16 * m) for m in range(GROUP))
        counts = (ctypes.c_uint * 5)(*self.counts)
        before = bytes(self.mem)
        fv = np.ascontiguousarray(self.fv, dtype=np.float64)
        diff = E.emu_group_rule_tails_compare(ctypes.byref(self.mem), fv.ctypes.data, self.cur, self.serve, self.booknow, idxp,
                                              self.maskA, self.maskB, self.hl.ctypes.data, counts)
        assert diff == 0, "member records / counters differ: mask %d" % diff
        assert bytes(self.mem) != before
        self.after = list(counts)
        return self

    def rule(self, E, m):
        """(result, abserr, resabs, resasc) of member m's child 1 and child 2."""
        out = np.zeros(8)
        fv = np.ascontiguousarray(self.fv[m], dtype=np.float64)
        E.emu_rule_apply(fv.ctypes.data, self.hl.ctypes.data, out.ctypes.data)
        return out[:4], out[4:]


def bits(x):
    return np.float64(x).view(np.uint64)


def assert_filed(p, E):
    """The records hold what the rule gives for every served member, where the pass had to put it."""
    filed = p.serve & ~p.booknow
    for m in range(GROUP):
        M = p.mem[m]
        if not (p.serve >> m) & 1:
            continue
        c1, c2 = p.rule(E, m)
        fl = int(not (c1[3] == c1[1])) | int(not (c2[3] == c2[1])) << 1      # resasc != abserr (true for a NaN)
        if p.cur < 0:
            if (p.maskA >> m) & 1:
                assert [bits(M.fb[k]) for k in range(4)] == [bits(v) for v in c1]
            if (p.maskB >> m) & 1:
                assert [bits(M.fb[4 + k]) for k in range(4)] == [bits(v) for v in c2]
            assert M.samples == 31 * ((p.maskA >> m) & 1) + 31 * ((p.maskB >> m) & 1)
        elif (p.booknow >> m) & 1:
            h = [M.fb[4 * p.cur + k] for k in range(4)]
            assert [bits(v) for v in h] == [bits(v) for v in (c1[0], c1[1], c2[0], c2[1])]
            assert M.hf == fl
        else:
            pos = [k for k in range(STASH) if M.sk[k] == p.idx[m]]
            assert len(pos) == 1
            k = pos[0]
            assert [bits(v) for v in (M.sr1[k], M.se1[k], M.sr2[k], M.se2[k])] == [bits(v) for v in (c1[0], c1[1], c2[0], c2[1])]
            assert M.sf[k] == fl
    if p.cur >= 0:
        assert p.after[0] == p.counts[0] | filed and p.after[4] == p.counts[4] + bin(filed).count("1")
        assert p.after[1:4] == p.counts[1:4]


@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("serve", SETS)
def test_served_sets_all_booked(emu, serve, cur):
    p = Pass(cur, serve, booknow=serve, seed=serve).run(emu)
    assert_filed(p, emu)
    for m in range(GROUP):
        assert list(p.mem[m].sk) == [-1] * STASH            # nothing went to a stash


@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("serve", SETS)
def test_served_sets_booked_and_stash_filed(emu, serve, cur):
    members = [m for m in range(GROUP) if (serve >> m) & 1]
    for booknow in {1 << members[0], 1 << members[-1], serve & 0x5, serve & 0xA}:
        p = Pass(cur, serve, booknow=booknow, seed=16 * serve + booknow)
        p.stash_keys(1, [40, -1, 41, -1, -1, 42, -1, -1])                  # member 1: the first free place is 1
        p.run(emu)
        assert_filed(p, emu)
        if (serve & ~booknow) & 2:
            assert p.mem[1].sk[1] == p.idx[1] and p.mem[1].snext == 4      # a free place: the cursor stays


def test_a_full_stash_replaces_through_the_cursor(emu):
    for serve, booknow in [(0xF, 0x1), (0xA, 0x0), (0x8, 0x0), (0x7, 0x4)]:
        p = Pass(0, serve, booknow=booknow, seed=77 + serve)
        for m in range(GROUP):
            p.stash_keys(m, [60 + k for k in range(STASH)] if m != 2 else [60, 61, 62, -1, 64, 65, 66, 67])
        p.mem[3].snext = STASH - 1                                         # wraps to 0
        p.run(emu)
        assert_filed(p, emu)
        for m in range(GROUP):
            if ((serve & ~booknow) >> m) & 1 and m != 2:
                at = (3 + m) % STASH if m != 3 else STASH - 1
                assert p.mem[m].sk[at] == p.idx[m] and p.mem[m].snext == (at + 1) % STASH
        if (serve & ~booknow) & 4:
            assert p.mem[2].sk[3] == p.idx[2] and p.mem[2].snext == 5      # member 2 had a free place


@pytest.mark.parametrize("maskA,maskB", [(0xF, 0xF), (0xF, 0x0), (0x5, 0xA), (0x3, 0x6), (0x8, 0x0), (0x1, 0x8), (0xB, 0x4)])
def test_first_rule(emu, maskA, maskB):
    p = Pass(-1, maskA | maskB, maskA=maskA, maskB=maskB, hl=(0.7, 0.01), seed=maskA * 16 + maskB).run(emu)
    assert_filed(p, emu)
    nq = bin(maskA).count("1") + bin(maskB).count("1")
    assert p.after == [p.counts[0], p.counts[1] + 31 * nq, p.counts[2] + bin(maskA | maskB).count("1"), p.counts[3] + nq, p.counts[4]]
    for m in range(GROUP):
        if not (maskA >> m) & 1:
            assert [p.mem[m].fb[k] for k in range(4)] == [50. + 8 * m + k for k in range(4)]
        if not (maskB >> m) & 1:
            assert [p.mem[m].fb[4 + k] for k in range(4)] == [54. + 8 * m + k for k in range(4)]


def special_vectors():
    """Sample vectors for the branches of rescale_error, by name.  Lane order: lanes 2k and 2k + 1 hold a symmetric pair
    of nodes, lane 30 the centre."""
    rng = np.random.default_rng(5)
    x = np.linspace(-1., 1., 64)
    odd = np.zeros(64)
    odd[0:30:2], odd[1:30:2] = -np.arange(1., 16.), np.arange(1., 16.)
    odd[32:62:2], odd[33:62:2] = -np.arange(1., 16.), np.arange(1., 16.)
    rough = np.where(np.arange(64) % 4 < 2, 1., -0.5) * (1. + 0.3 * rng.normal(size=64))
    return {
        "zeros": np.zeros(64),                                  # resasc == 0 and err == 0
        "odd": odd,                                             # every pair sums to 0: err == 0, resasc != 0
        "tiny": smooth(rng, 1e-300),                            # resabs below DBL_MIN / (50 eps)
        "smooth": 1. + 0.01 * x * x,                              # scale < 1
        "rough": rough,                                         # scale >= 1: abserr == resasc
    }


def test_the_special_vectors_take_the_branches_they_are_named_for(emu):
    v = special_vectors()
    p = Pass(0, 0xF)
    lim = DBL_MIN / (50 * DBL_EPSILON)
    for m, name in enumerate(["zeros", "odd", "tiny", "smooth"]):
        p.fv[m] = v[name]
    c = [p.rule(emu, m)[0] for m in range(4)]
    assert c[0][3] == 0 and c[0][1] == 0
    assert c[1][0] == 0 and c[1][3] != 0 and c[1][1] == 50 * DBL_EPSILON * c[1][2]      # err == 0: the floor alone
    assert 0 < c[2][2] < lim
    assert 0 < c[3][1] < c[3][3] and c[3][2] > lim
    p.fv[0] = v["rough"]
    r = p.rule(emu, 0)[0]
    assert r[1] == r[3] != 0


@pytest.mark.parametrize("cur", [-1, 0])
def test_special_vectors_in_every_lane_pair(emu, cur):
    v = special_vectors()
    names = list(v)
    for shift in range(len(names)):
        for serve in (0xF, 0x6, 0x8):
            p = Pass(cur, serve, booknow=serve & 0x3, maskA=serve, maskB=serve & 0xC if cur < 0 else 0, seed=shift)
            for m in range(GROUP):
                p.fv[m] = v[names[(m + shift) % len(names)]]
            p.fv[1, 32:] = v[names[(shift + 3) % len(names)]][32:]         # member 1's children differ in kind
            p.run(emu)
            assert_filed(p, emu)


def test_nan_and_infinite_samples(emu):
    nan, inf = float("nan"), float("inf")
    for cur in (-1, 0, 1):
        for serve in (0xF, 0xA, 0x1):
            p = Pass(cur, serve, booknow=serve & 0x9, maskA=serve, maskB=serve & 0x6 if cur < 0 else 0, seed=9)
            p.fv[0, 7] = nan                        # child 1 of member 0
            p.fv[1, 40] = inf                       # child 2 of member 1
            p.fv[2, 3], p.fv[2, 50] = -inf, nan
            p.fv[3, :] = nan
            p.run(emu)
            assert_filed(p, emu)
            if serve & 1 and cur >= 0:
                assert np.isnan(p.mem[0].fb[4 * cur]) and not np.isnan(p.mem[0].fb[4 * cur + 2])
                assert p.mem[0].hf & 1              # NaN != NaN: child 1's flag is set, as in qag.c
            if serve & 2 and cur >= 0:
                k = [k for k in range(STASH) if p.mem[1].sk[k] == p.idx[1]][0]
                assert not np.isfinite(p.mem[1].sr2[k]) and np.isfinite(p.mem[1].sr1[k])


def test_the_padding_lanes_samples_are_never_read(emu):
    for cur, serve in [(-1, 0xF), (0, 0xF), (1, 0x6), (0, 0x8)]:
        recs = []
        for pad in (0., float("nan"), 1e300):
            p = Pass(cur, serve, booknow=serve & 0x5, maskA=serve, maskB=serve if cur < 0 else 0, seed=31)
            p.fv[:, 31], p.fv[:, 63] = pad, pad
            recs.append(bytes(p.run(emu).mem))
        assert recs[0] == recs[1] == recs[2]


def test_seeded_random_passes(emu):
    rng = np.random.default_rng(20240611)
    v = special_vectors()
    names = list(v)
    n_multi = n_filed = n_full = 0
    n_cases = 160
    for case in range(n_cases):
        cur = int(rng.integers(-1, 2))
        serve = int(rng.integers(1, 16)) if rng.random() < 0.8 else 1 << int(rng.integers(4))
        booknow = serve & int(rng.integers(0, 16)) if cur >= 0 else 0
        maskA = serve & int(rng.integers(0, 16)) if cur < 0 else 0
        maskB = serve & ~maskA | (serve & int(rng.integers(0, 16))) if cur < 0 else 0
        if cur < 0 and rng.random() < 0.3:
            maskA, maskB = serve, 0
        p = Pass(cur, serve, booknow=booknow, maskA=maskA, maskB=maskB,
                 hl=(10. ** rng.integers(-8, 3), -10. ** rng.integers(-8, 3) if rng.random() < 0.1 else rng.uniform(0.01, 3.)), seed=case)
        for m in range(GROUP):
            u = rng.random()
            if u < 0.3:
                p.fv[m] = v[names[int(rng.integers(len(names)))]]
            elif u < 0.4:
                p.fv[m, int(rng.integers(64))] = [float("nan"), float("inf"), -float("inf")][int(rng.integers(3))]
            elif u < 0.6:
                p.fv[m] *= 10. ** rng.integers(-320, 300)
            p.idx[m] = int(rng.integers(0, 5000))
            fill = rng.random()
            if fill < 0.4:
                p.stash_keys(m, [5000 + k for k in range(STASH)])
                n_full += 1
            elif fill < 0.8:
                p.stash_keys(m, [5000 + k if rng.random() < 0.6 else -1 for k in range(STASH)])
            p.mem[m].snext = int(rng.integers(STASH))
        p.run(emu)
        assert_filed(p, emu)
        n_multi += bin(serve).count("1") > 1
        n_filed += cur >= 0 and (serve & ~booknow) != 0
    assert 2 * n_multi >= n_cases            # at least half the passes serve more than one member
    assert n_filed > 24 and n_full > 48

