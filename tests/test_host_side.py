"""CPU tests of the host side: the C-ABI library loads and exports every symbol
the header declares, the host build of the scalar device functions matches the
oracle bit for bit, the workload generator is deterministic, and the interleaved
shard / gather logic of the multi-GPU path works (gloo, world_size 2)."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_bind
from rimphony_amd import _build, workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cabi_exports_every_declared_symbol():
    _build.build_hip()
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    names = set(re.findall(r"\b((?:rimphony|pkgw_bessel)_[a-z0-9_]+)\s*\(", hdr))
    names -= {"rimphony_ctx"}
    assert len(names) >= 13
    lib = ctypes.CDLL(os.path.join(ROOT, "rimphony_amd", "librimphony_hip.so"))
    for n in sorted(names):
        assert hasattr(lib, n), "missing export: " + n
    from rimphony_amd import capi
    assert set(capi.SYMBOLS) <= names
    lib.rimphony_dist_nparams.restype = ctypes.c_int
    assert [lib.rimphony_dist_nparams(k) for k in range(4)] == [4, 1, 5, 4]
    assert lib.rimphony_dist_nparams(7) < 0
    lib.rimphony_version.restype = ctypes.c_char_p
    assert b"gfx950" in lib.rimphony_version()


def _c_prototypes(hdr):
    """name -> number of arguments, for every function the header declares"""
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b((?:rimphony|pkgw_bessel)_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else args.count(",") + 1
    return protos


def test_rust_sys_crate_matches_header():
    """rimphony-hip-sys/ (the Rust -sys source, shipped unbuilt -- the image has no Rust toolchain): every
    function of its extern block is declared in include/rimphony_hip.h with the same number of arguments, the constants
    carry the header's values, and the crate has the three files a `links = "rimphony_hip"` crate needs."""
    crate = os.path.join(ROOT, "rimphony-hip-sys")
    for f in ("Cargo.toml", "build.rs", os.path.join("src", "lib.rs")):
        assert os.path.exists(os.path.join(crate, f)), f
    assert 'links = "rimphony_hip"' in open(os.path.join(crate, "Cargo.toml")).read()
    assert "rustc-link-lib=dylib=rimphony_hip" in open(os.path.join(crate, "build.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    protos = _c_prototypes(hdr)
    rs = open(os.path.join(crate, "src", "lib.rs")).read()
    rs = re.sub(r"//[^\n]*", "", rs)
    block = rs[rs.index('extern "C" {'):]
    block = block[:block.index("\n}\n")]
    fns = re.findall(r"pub fn ([a-z0-9_]+)\s*\(([^)]*)\)", block, flags=re.S)
    assert len(fns) >= 20
    for name, args in fns:
        assert name in protos, "not in the header: " + name
        nargs = len([a for a in args.split(",") if a.strip()])
        assert nargs == protos[name], (name, nargs, protos[name])
    for must in ("rimphony_batch_compute", "rimphony_batch_compute_ex", "rimphony_batch_compute_multi",
                 "rimphony_ctx_create", "rimphony_ctx_destroy", "pkgw_bessel_j", "pkgw_bessel_dj"):
        assert must in dict(fns)
    for cname, val in re.findall(r"pub const (RIMPHONY_[A-Z0-9_]+): [a-z_0-9]+ = ([^;]+);", rs):
        m = re.search(r"#define\s+%s\s+(.+?)(?:/\*|\n)" % cname, hdr) or re.search(r"\b%s = (-?\d+)" % cname, hdr)
        assert m, cname
        cval = m.group(1).strip().replace("u", "").strip("()")
        assert eval(cval) == eval(val.strip()), (cname, cval, val)


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from rimphony_amd import api, capi
    with pytest.raises(capi.RimphonyError):
        api.Context(0)
    # the raw C entry point refuses as well
    lib = capi.load()
    h = ctypes.c_void_p()
    assert lib.rimphony_ctx_create(0, ctypes.byref(h)) == -4   # RIMPHONY_ENODEVICE


def test_product_does_not_reference_oracle():
    """The product tree must never include / import / link / load the oracle
    (comments may cite oracle files as documentation)."""
    pat = re.compile(r'#\s*include\s*[<"][^>"]*oracle|import\s+oracle|from\s+oracle|liboracle|oracle_bind|dlopen')
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rimphony_amd")):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".hpp", ".cpp")) and f != "_build.py":
                # _build.build_oracle() compiles the checker for the tests; it does not load it
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                if f == "rimphony_multi.hip":
                    # the one dlopen of the product: librccl for the gather of the table (round 4).  Its candidates are
                    # spelled in one array; the file may not name the oracle at all, not even in a comment.
                    assert "oracle" not in txt.lower()
                    cands = re.search(r'const char \*cands\[4\] = \{([^}]*)\}', txt).group(1)
                    assert all("rccl" in c.lower() for c in re.findall(r'"([^"]*)"', cands)), cands
                    assert txt.count("dlopen(") == 1 and "dlopen(cands[i]" in txt
                    txt = txt.replace("dlopen", "")
                assert not pat.search(txt), f
    # (the header documents that the rimphony_rccl_* entries load librccl at run time: that word is not a reference to the oracle)
    assert not pat.search(open(os.path.join(ROOT, "include", "rimphony_hip.h")).read().replace("dlopen'ed", "loaded"))
    # and the shared library has no dependency on it
    out = subprocess.run(["ldd", os.path.join(ROOT, "rimphony_amd", "librimphony_hip.so")], capture_output=True, text=True).stdout
    assert "oracle" not in out


@pytest.fixture(scope="module")
def devh():
    so = _build.build_test_support()
    D = ctypes.CDLL(so)
    D.devh_bessel_j.restype = ctypes.c_double; D.devh_bessel_j.argtypes = [ctypes.c_double] * 2
    D.devh_bessel_dj.restype = ctypes.c_double; D.devh_bessel_dj.argtypes = [ctypes.c_double] * 2
    D.devh_gamma_integrand.restype = ctypes.c_double
    D.devh_gamma_integrand.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double] * 3 + [ctypes.POINTER(ctypes.c_double)] + [ctypes.c_double] * 3
    return D


def _same(a, b):
    return a == b or (a != a and b != b)


def test_device_bessel_host_build_bit_exact(devh, oracle):
    rng = np.random.default_rng(7)
    for _ in range(20000):
        u = rng.random()
        n = float(rng.integers(0, 31)) if u < 0.2 else float(np.exp(rng.uniform(math.log(30), math.log(1e14))))
        if rng.random() < 0.5 and n >= 1:
            n = float(math.floor(n))
        x = n * (1 - 10 ** rng.uniform(-12, 0)) if rng.random() < 0.9 else n * (1 + 10 ** rng.uniform(-12, -3))
        if rng.random() < 0.08:
            x = n * (1 + 10 ** rng.uniform(-4, 1))     # x > n: Debye / blend / Meissel "second" (bessel.c:358-375)
        if rng.random() < 0.02:
            x = n
        if n < 30 and rng.random() < 0.1:
            x = float(np.exp(rng.uniform(math.log(3e4), math.log(1e9))))       # Hankel branch of the integer orders
        assert _same(oracle.rimo_bessel_j(n, x), devh.devh_bessel_j(n, x)), (n, x)
        assert _same(oracle.rimo_bessel_dj(n, x), devh.devh_bessel_dj(n, x)), (n, x)


def test_device_integrand_host_build_bit_exact(devh, oracle):
    rng = np.random.default_rng(8)
    gen = {0: lambda: [rng.uniform(1.5, 4), float(np.exp(rng.uniform(0, math.log(30)))), 1e12, 1e10],
           1: lambda: [float(np.exp(rng.uniform(math.log(.1), math.log(100))))],
           2: lambda: [rng.uniform(1.5, 4), rng.uniform(0, 3), 1., 1e12, 1e10],
           3: lambda: [rng.uniform(1.5, 4.5), float(np.exp(rng.uniform(1, 3))), rng.uniform(0, 3), 1e10]}
    for i in range(4000):
        kind = i % 4
        par = gen[kind]()
        d, st = oracle_bind.mkdist(oracle, kind, par)
        s = float(np.exp(rng.uniform(math.log(.1), math.log(1e7))))
        th = float(rng.uniform(0.003, 1.57))
        sn, cs = math.sin(th), math.cos(th)
        # the oracle computes sin/cos with detmath; take them from its own gamma_integrand path by
        # passing theta and comparing through the public function
        n = s * abs(sn) + 1 + float(np.exp(rng.uniform(-3, 12)))
        if rng.random() < 0.5:
            n = float(math.floor(n))
        nos = n / s
        root = math.sqrt(max(nos * nos - sn * sn, 0))
        gm, gp = (nos - abs(cs) * root) / sn ** 2, (nos + abs(cs) * root) / sn ** 2
        g = gm + (gp - gm) * rng.random()
        co, stk = int(rng.integers(0, 2)), int(rng.integers(0, 3))
        a = oracle.rimo_gamma_integrand(d, co, stk, s, th, n, g)
        # detmath sincos of theta, as the kernels do
        import test_detmath  # noqa: F401  (keeps the helper build next to this test)
        sv, cv = _detsincos(th)
        pa = (ctypes.c_double * 5)(*(par + [0.] * 5)[:5])
        b = devh.devh_gamma_integrand(kind, co, stk, s, cv, sv, pa, d.norm, n, g)
        assert _same(a, b), (kind, par, s, th, n, g, a, b)


_SC = {}


def _detsincos(x):
    if "lib" not in _SC:
        so = _build.build_test_support()
        L = ctypes.CDLL(so)
        L.devh_sincos.restype = None
        L.devh_sincos.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        _SC["lib"] = L
    s, c = ctypes.c_double(), ctypes.c_double()
    _SC["lib"].devh_sincos(x, ctypes.byref(s), ctypes.byref(c))
    return s.value, c.value


def test_grid_plan_of_the_persistent_launch():
    """rim_plan_grid (launch_plan.h) is the integer arithmetic between "how many tasks" and "grid, squad, stride, classes"
    of a persistent launch.  The expected values are worked out by hand from the launch code it replaced:
    resident = min(occupancy or 4, 4 waves), lowered to (160 KB - 512) / roundup512(LDS) where that is smaller, quartered
    (or 2) in shared mode; grid = min(CUs x resident, 64 x tasks -- tasks alone without the cooperative tail or beyond
    2^40 --), at least 1; squad only with early help, the tail on, tasks >= 4 grid and grid >= 16 squad:
    stride = (grid / squad) | 1, squad = min(squad, (grid - 1) / stride + 1), classes 4 / 2 / 1 from 256 / 128 waves."""
    so = _build.build_test_support()
    L = ctypes.CDLL(so)
    L.devh_plan_grid.restype = None
    L.devh_plan_grid.argtypes = ([ctypes.c_int, ctypes.c_ulonglong, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_ulonglong] +
                                 [ctypes.c_int] * 3 + [ctypes.c_uint, ctypes.c_int, ctypes.POINTER(ctypes.c_longlong)])

    def plan(n_cu=256, ntasks=262144, occ=20, lds=7680, dyn=0, waves=5, shared=0, no_assist=0, squad=0, early=0):
        out = (ctypes.c_longlong * 5)()
        L.devh_plan_grid(n_cu, ntasks, occ, lds, dyn, waves, shared, no_assist, squad, early, out)
        return tuple(out)          # resident_per_cu, grid, early_squad, early_stride, early_classes

    # 7680 bytes = 15 granules: (163840 - 512) // 7680 = 21 such blocks fit a CU, the clamp is idle
    assert plan() == (20, 5120, 0, 1, 1)
    assert plan(squad=64) == (20, 5120, 0, 1, 1)                     # a kernel without the protocol has no squad
    assert plan(squad=64, early=1) == (20, 5120, 64, 81, 1)          # stride (5120 // 64) | 1 = 81, fit 5119 // 81 + 1 = 64
    assert plan(squad=256, early=1) == (20, 5120, 244, 21, 2)        # stride 20 | 1 = 21, fit 5119 // 21 + 1 = 244
    assert plan(squad=128, early=1) == (20, 5120, 125, 41, 1)        # stride 40 | 1 = 41, fit 5119 // 41 + 1 = 125
    # four classes need 256 waves after the fit: 448 CUs x 28 = 12544 = 256 x 49, stride 49, fit 12543 // 49 + 1 = 256
    assert plan(n_cu=448, occ=28, waves=7, lds=0, squad=256, early=1, ntasks=1 << 20) == (28, 12544, 256, 49, 4)
    assert plan(n_cu=512, occ=24, waves=6, lds=0, squad=256, early=1, ntasks=1 << 20) == (24, 12288, 251, 49, 2)   # 12287 // 49 + 1
    # the launches of the bench (131072 rows x 2 tasks on an MI355X: 256 CUs) with what the runtime reported there
    # (profiles/host_refactor_bench_ab.txt): the Symphony groups (occupancy 20, 7648 bytes of LDS, 5 waves) and the
    # Faraday kernel (occupancy 20, 6560 bytes, 5 waves; squad 64 on the power-law table, 256 on the pitchy-kappa one)
    assert plan(occ=20, lds=7648, waves=5) == (20, 5120, 0, 1, 1)
    assert plan(occ=20, lds=6560, waves=5, squad=64, early=1) == (20, 5120, 64, 81, 1)
    assert plan(occ=20, lds=6560, waves=5, squad=256, early=1) == (20, 5120, 244, 21, 2)
    # the LDS clamp: 8192 bytes -> 163328 // 8192 = 19 < 20; one granule less (7680) -> 21, idle.  Static and dynamic
    # LDS add up before the rounding: 7600 + 256 = 7856 -> 8192 as well
    assert plan(lds=8192)[:2] == (19, 4864)
    assert plan(lds=8191)[:2] == (19, 4864) and plan(lds=7681)[:2] == (19, 4864)
    assert plan(lds=7680)[:2] == (20, 5120)
    assert plan(lds=7600, dyn=256)[:2] == (19, 4864)
    assert plan(lds=0)[:2] == (20, 5120)                             # LDS size not known: no clamp
    assert plan(lds=200000)[:2] == (20, 5120)                        # (a block that fits no CU is not this function's to refuse)
    # the occupancy answer capped at 4 waves per SIMD x the launch bounds; a failed query is one wave per SIMD
    assert plan(occ=32, lds=512)[:2] == (20, 5120)
    assert plan(occ=32, lds=512, waves=6)[:2] == (24, 6144)
    assert plan(occ=0)[:2] == (4, 1024) and plan(occ=-1)[:2] == (4, 1024)
    # shared mode: >= 8 is quartered, anything smaller becomes 2; never a squad
    assert plan(shared=1, no_assist=1) == (5, 1280, 0, 1, 1)
    assert plan(shared=1, no_assist=1, occ=8)[:2] == (2, 512)
    assert plan(shared=1, no_assist=1, occ=7)[:2] == (2, 512)
    assert plan(shared=1, no_assist=1, occ=0)[:2] == (2, 512)
    assert plan(shared=1, squad=64, early=1)[2:] == (0, 1, 1)
    # fewer tasks than waves: 64 waves per task (helpers from the start), capped by the device; one per task without the tail
    assert plan(ntasks=10)[:2] == (20, 640)
    assert plan(ntasks=80)[:2] == (20, 5120) and plan(ntasks=79)[:2] == (20, 5056)
    assert plan(ntasks=10, no_assist=1)[:2] == (20, 10)
    assert plan(ntasks=(1 << 40) + 1)[:2] == (20, 5120) and plan(ntasks=1 << 62)[:2] == (20, 5120)
    assert plan(ntasks=0)[:2] == (20, 1) and plan(ntasks=0, no_assist=1)[:2] == (20, 1)
    # the squad's conditions: tasks >= 4 grid, grid >= 16 squad, the tail on
    assert plan(ntasks=4 * 5120, squad=64, early=1)[2:] == (64, 81, 1)
    assert plan(ntasks=4 * 5120 - 1, squad=64, early=1)[2:] == (0, 1, 1)
    assert plan(squad=320, early=1)[2:] == (302, 17, 4)              # 5120 = 16 x 320; stride 16 | 1, fit 5119 // 17 + 1 = 302
    assert plan(squad=321, early=1)[2:] == (0, 1, 1)
    assert plan(squad=64, early=1, no_assist=1)[2:] == (0, 1, 1)
    assert plan(squad=0, early=1)[2:] == (0, 1, 1)


def test_workload_is_deterministic_and_in_range():
    k1, m1, s1, t1, p1 = workload.make_batch("cfg2_powerlaw_jI_aI", 1000)
    k2, m2, s2, t2, p2 = workload.make_batch("cfg2_powerlaw_jI_aI", 500, start=500)
    assert (s1[500:] == s2).all() and (t1[500:] == t2).all() and all((a[500:] == b).all() for a, b in zip(p1, p2))
    assert s1.min() >= 0.1 and s1.max() <= 1e4 and t1.min() >= 0.05 and t1.max() <= 1.52
    assert p1[0].min() >= 1.5 and p1[0].max() <= 4 and p1[1].min() >= 1 and p1[1].max() <= 30
    assert m1 == 0x03 and k1 == 0
    for cfg in workload.CONFIGS:
        kind, mask, s, th, params = workload.make_batch(cfg, 16)
        assert len(params) == [4, 1, 5, 4][kind]
    # splitmix64 reference value: first output for seed 0 is 0xE220A8397B1DCDAF
    with np.errstate(over="ignore"):
        assert int(workload.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF


def test_interleaved_shard_and_gather_gloo_world2(tmp_path):
    """The N>1 path of bench.py / rimphony_amd.sharding on CPU: 2 ranks, gloo, the per-rank
    compute replaced by the oracle (test infrastructure).  The gathered table must equal the
    single-process table bit for bit."""
    script = tmp_path / "w2.py"
    script.write_text(r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, torch, torch.distributed as dist
import oracle_bind
from rimphony_amd import workload, sharding
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
L = oracle_bind.load("det")
kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_jI_aI", 10)   # ragged: 10 rows over 2 ranks... plus 1 more below
kind, mask, s, th, params = workload.make_batch("cfg2_powerlaw_jI_aI", 11)
idx = sharding.shard_indices(11, rank, world)
local = oracle_bind.batch(L, kind, s[idx], th[idx], [p[idx] for p in params], mask, nthreads=2)
table = sharding.gather_table(torch.from_numpy(local), 11, rank, world, dst=0)
if rank == 0:
    ref = oracle_bind.batch(L, kind, s, th, params, mask, nthreads=2)
    t = table.numpy()
    same = (t.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(t) & np.isnan(ref))
    assert same.all()
    print("OK")
dist.destroy_process_group()
''' % (ROOT, ROOT))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", "29533", str(script)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "OK" in r.stdout


def test_interleaved_shard_and_gather_gloo_world8_ragged(tmp_path):
    """The same at the size the scaling run uses: EIGHT ranks started by rimphony_amd.launch.spawn_ranks (what
    `python bench.py --gpus 8` does), gloo, a ragged table (67 rows: ranks 0-2 hold 9 rows, the others 8), the gather
    to rank 0 and the max-over-ranks reduction of bench.py's timing.  Per-rank compute is the oracle on the cheapest
    coefficient pair (test infrastructure); the gathered table must equal the single-process table bit for bit."""
    script = tmp_path / "w8.py"
    script.write_text(r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, torch, torch.distributed as dist
import oracle_bind
from rimphony_amd import workload, sharding
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
assert world == 8
L = oracle_bind.load("det")
n = 67
kind, mask, s, th, params = workload.make_batch("cfg3_thermal_8", n)
mask = 0x03
idx = sharding.shard_indices(n, rank, world)
assert len(idx) == (9 if rank < 3 else 8)
local = oracle_bind.batch(L, kind, s[idx], th[idx], [p[idx] for p in params], mask, nthreads=1)
table = sharding.gather_table(torch.from_numpy(local), n, rank, world, dst=0)
t = torch.tensor([float(rank)], dtype=torch.float64)
dist.all_reduce(t, op=dist.ReduceOp.MAX)
assert t.item() == 7.0
if rank == 0:
    ref = oracle_bind.batch(L, kind, s, th, params, mask, nthreads=4)
    g = table.numpy()
    same = (g.view(np.uint64) == ref.view(np.uint64)) | (np.isnan(g) & np.isnan(ref))
    assert same.all()
    print("OK8")
else:
    assert table is None
dist.destroy_process_group()
''' % (ROOT, ROOT))
    code = ("import sys; sys.path.insert(0, %r); from rimphony_amd import launch; "
            "sys.exit(launch.spawn_ranks(8, [%r], timeout=500))" % (ROOT, str(script)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "OK8" in r.stdout


def test_scalar_bessel_seam_is_host_code_and_matches_oracle(oracle):
    """pkgw_bessel_j / pkgw_bessel_dj (leung-bessel/src/lib.rs:36-42): exported by the product library as HOST code --
    they work here, without a GPU -- and return the oracle's bits, including the x > n side, the integer orders
    below 30 and the error conventions of bessel.c (NaN for non-integer n < 30 and for n >= 1e15 in dj)."""
    from rimphony_amd import capi
    lib = capi.load()
    rng = np.random.default_rng(11)
    n = np.concatenate([np.exp(rng.uniform(math.log(30), math.log(1e12), 6000)), rng.integers(0, 30, 1000).astype(float)])
    x = n * rng.uniform(0.2, 1.3, n.size)
    for a, b in zip(n, x):
        assert _same(lib.pkgw_bessel_j(a, b), oracle.rimo_bessel_j(a, b)), (a, b)
        assert _same(lib.pkgw_bessel_dj(a, b), oracle.rimo_bessel_dj(a, b)), (a, b)
    # leung-bessel/src/lib.rs:83-85 smoke values (n < 30 -> integer-order J_n)
    assert abs(lib.pkgw_bessel_j(1., 1.) - 0.44005058574493355) < 1e-15
    assert math.isnan(lib.pkgw_bessel_j(12.5, 3.))           # bessel.c:327-331
    assert math.isnan(lib.pkgw_bessel_dj(1e15, 5e14))        # bessel.c:382-388
    assert math.isnan(lib.pkgw_bessel_j(-1., 3.))


def test_scalar_bessel_seam_call_rate():
    """The seam replaces a ~100-200 ns C call: it must stay a plain host function."""
    import time
    from rimphony_amd import capi
    lib = capi.load()
    f = lib.pkgw_bessel_j
    t0 = time.perf_counter()
    for i in range(100000):
        f(1000. + i, 900. + i)
    rate = 100000 / (time.perf_counter() - t0)
    assert rate > 2e5, rate          # through ctypes; ~7e6/s from C (tools/ not needed: see DESIGN.md)


def test_spawn_ranks_runs_a_gloo_world_without_torchrun(tmp_path):
    """rimphony_amd.launch.spawn_ranks -- what `python bench.py --gpus N` uses when no launcher set WORLD_SIZE:
    N child processes with the rendezvous variables, rank 0's stdout is the parent's, worst exit code returned."""
    script = tmp_path / "w.py"
    script.write_text(r'''
import os, sys
import torch, torch.distributed as dist
dist.init_process_group("gloo")
rank = dist.get_rank()
t = torch.tensor([float(rank + 1)])
dist.all_reduce(t)
if rank == 0:
    print("SUM", t.item(), os.environ["WORLD_SIZE"], os.environ["MASTER_ADDR"])
dist.destroy_process_group()
sys.exit(int(sys.argv[1]) if rank == 1 else 0)
''')
    code = ("import sys; sys.path.insert(0, %r); from rimphony_amd import launch; "
            "sys.exit(launch.spawn_ranks(2, [%r, sys.argv[1]], timeout=300))" % (ROOT, str(script)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-c", code, "0"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SUM 3.0 2 127.0.0.1" in r.stdout
    r = subprocess.run([sys.executable, "-c", code, "3"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 3


def test_spawn_ranks_ends_the_others_when_a_late_rank_dies(tmp_path):
    """A rank other than 0 dying early must end the run at once (the others would sit in a collective until its own
    timeout), and `timeout` is one deadline for the whole run."""
    import time
    from rimphony_amd import launch
    script = tmp_path / "d.py"
    script.write_text("import os, sys, time\nif os.environ['RANK'] == '1': sys.exit(7)\ntime.sleep(120)\n")
    t0 = time.time()
    assert launch.spawn_ranks(2, [str(script)]) == 7
    assert time.time() - t0 < 20
    script.write_text("import time\ntime.sleep(120)\n")
    t0 = time.time()
    assert launch.spawn_ranks(2, [str(script)], timeout=2) == 124
    assert time.time() - t0 < 20


def test_bench_parent_never_touches_the_gpu():
    """bench.py --gpus N>1 without a launcher must spawn its ranks before anything initialises the GPU: the parent
    path may not import torch (static check of the code in front of the spawn)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    head = src[:src.index("launch.spawn_ranks(")]
    assert "import torch" not in head.split("def main")[1]


def test_bench_refuses_full_only_sizes_without_full():
    """--side-rows and --cpu-sample size what only --full measures: a plain run that is given one refuses it instead of
    ignoring it (before any import of torch)."""
    for opt in ("--side-rows", "--cpu-sample"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), opt, "8"], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr


def test_api_refuses_bad_device_inputs():
    """compute_batch_device takes raw pointers: strided views, wrong dtype, wrong length and host tensors are
    refused before any pointer reaches the C ABI (no GPU needed for these checks)."""
    import torch
    from rimphony_amd import api
    ctx = object.__new__(api.Context)      # no device: only the argument checks run
    ctx.device = 0
    good = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        ctx.compute_batch_device(0, good, good, [good] * 3)              # wrong number of parameter arrays
    with pytest.raises(ValueError):
        ctx.compute_batch_device(9, good, good, [good] * 4)              # unknown kind
    with pytest.raises(ValueError):
        ctx.compute_batch_device(0, good, good, [good] * 4)              # host tensors
    with pytest.raises(TypeError):
        ctx.compute_batch_device(0, np.zeros(4), good, [good] * 4)       # not a tensor


def test_group_kernel_resources_leave_room_for_its_grid(tmp_path):
    """The persistent grid of the group kernel is sized for RIM_GROUP_WAVES waves per SIMD (group_launch.h), every one of
    which must be RESIDENT (a wave that is not is waited for by the cooperative tail up to its 2 s bound: measured as a
    2 x slower launch on a diagnostic build whose LDS went one allocation granule over).  The compiler's own resource report
    of the Symphony group kernels must therefore say: that occupancy, and an LDS block that fits 4 x that many times into a
    CU's 160 KB with one 512-byte granule to spare."""
    hipcc = _build.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "rimphony_amd", "csrc", "rimphony_group.hip")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-c", src, "-o", str(tmp_path / "g.o"),
                                           "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(os.path.join(ROOT, "rimphony_amd", "csrc", "group_launch.h")).read()
    waves = int(re.search(r"#define RIM_GROUP_WAVES (\d+)", text).group(1))
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    seen = 0
    for b in blocks:
        name = b.split()[0]
        if "SymGroupProblem" not in name:
            continue
        seen += 1
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        assert occ >= waves, (name, occ)
        granules = (lds + 511) // 512 * 512
        assert 4 * waves * granules <= 160 * 1024 - 512, (name, lds)
    assert seen == 4


def test_uninterleave_layout_of_the_gather():
    """The block layout rimphony_rccl_gather_table assumes on the root (shards stored rank after rank, ragged): the offset
    expression of its un-interleave kernel (rimphony_multi.hip uninterleave_kernel), restated here, against the cumulative
    shard sizes, for worlds that do and do not divide n -- a world of one (all the GPU test can run) cannot show an indexing
    error."""
    # row i of an n-row table lives on rank i % w at local row i // w; blocks are stored rank after rank
    for n, w in ((67, 8), (64, 8), (5, 8), (9, 2), (1, 1)):
        per = [(n + w - 1 - r) // w for r in range(w)]
        off = np.concatenate([[0], np.cumsum(per)[:-1]])
        for i in range(n):
            r, j = i % w, i // w
            rem = n % w
            p0 = (n + w - 1) // w
            formula = r * p0 if rem == 0 else (r * p0 if r <= rem else rem * p0 + (r - rem) * (p0 - 1))
            assert formula == off[r] and j < per[r]
