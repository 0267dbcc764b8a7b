"""The tabulated distribution (RIMPHONY_TABULATED = 4) without a GPU: the C ABI and its mirrors carry the kind, the host
build of its device functions reproduces a power law from a straight-line table and has consistent derivatives, the
table oracle (tests/support/liboracle_tab.so) agrees with the analytic kinds of the CPU oracle, and the argument checks
refuse what the library refuses.  CPU only."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_bind
import tab_bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "symphony-powerlaw.txt")
FIXTURE = os.path.join(ROOT, "tests", "golden", "tabulated_det.npz")


def test_kind_and_entry_in_library_header_and_mirrors():
    """rimphony_dist_nparams(4) == 1 and (5) < 0 on the cross-compiled library; the header, capi and the Rust crate carry
    RIMPHONY_TABULATED = 4 and rimphony_ctx_set_tables."""
    from rimphony_amd import _build, api, capi
    _build.build_hip()
    lib = ctypes.CDLL(capi.LIB_PATH)
    lib.rimphony_dist_nparams.restype = ctypes.c_int
    assert lib.rimphony_dist_nparams(4) == 1
    assert lib.rimphony_dist_nparams(5) < 0
    assert [lib.rimphony_dist_nparams(k) for k in range(4)] == [4, 1, 5, 4]
    assert hasattr(lib, "rimphony_ctx_set_tables")
    # a null context is refused before anything is touched
    lib.rimphony_ctx_set_tables.restype = ctypes.c_int
    lib.rimphony_ctx_set_tables.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_void_p]
    assert lib.rimphony_ctx_set_tables(None, 0, 0, 1.0, 2.0, None) == -1
    hdr = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    assert re.search(r"\bRIMPHONY_TABULATED = 4\b", hdr)
    assert re.search(r"int rimphony_ctx_set_tables\(rimphony_ctx \*ctx, size_t n_tables, size_t n_nodes, double gamma_lo, "
                     r"double gamma_hi,\s+const double \*log_n\);", hdr)
    assert "rimphony_ctx_set_tables" in capi.SYMBOLS
    assert api.TABULATED == 4 and api.NPARAMS[api.TABULATED] == 1
    rs = open(os.path.join(ROOT, "rimphony-hip-sys", "src", "lib.rs")).read()
    assert re.search(r"pub const RIMPHONY_TABULATED: c_int = 4;", rs)
    assert re.search(r"pub fn rimphony_ctx_set_tables\(", rs)
    hpp = open(os.path.join(ROOT, "rimphony_amd", "cxx", "rimphony.hpp")).read()
    assert "class TabulatedDistribution" in hpp and "rimphony_ctx_set_tables" in hpp


def test_group_unit_keeps_four_way_dispatch(tmp_path):
    """The kind never runs on the analytic kinds' group kernels: their translation unit dispatches over the four analytic
    kinds only, and the kernels of kind 4 have a unit of their own that the build compiles.  That unit, compiled alone for
    gfx950, defines exactly its 24 kernels, by mangled name: the three of a set's installation and 2-D row norms, the two
    persistent kernels for all five forms (K = DIST_TABULATED .. DIST_TABULATED_GRID = 4 .. 8), norm_kernel for the forms
    that have one (a 2-D set's rows load theirs; an isotropic set runs K = 4) and the two unit seams for K = 4, 6, 7, 8."""
    from rimphony_amd import _build
    csrc = os.path.join(ROOT, "rimphony_amd", "csrc")
    group = open(os.path.join(csrc, "rimphony_group.hip")).read()
    assert "rim_with_kind5" not in group and "DIST_TABULATED" not in group
    unit = os.path.join(csrc, "rimphony_tab.hip")
    assert unit in _build.hip_sources()
    hipcc = _build.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", unit, "-o", str(tmp_path / "tab.s")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", open(tmp_path / "tab.s").read(), re.M)
    want = ["_Z23tab2d_table_norm_kernelPdS_", "_Z21tab2d_row_norm_kernel9ParamPtrsmPd", "_Z25tab_pitchy_table_p_kernelPdS_"]
    want += ["_Z11coop_kernelI15SymphonyProblemILi%dELi0EEEv7SymArgs" % k for k in (4, 5, 6, 7, 8)]
    want += ["_Z11coop_kernelI16HeyvaertsProblemILi%dEEEv7SymArgs" % k for k in (4, 5, 6, 7, 8)]
    want += ["_Z11norm_kernelILi%dEEv9ParamPtrsmPdPyS1_" % k for k in (4, 7, 8)]
    want += ["_Z18integrand_kernel_nILi%dEEv9PointArgsPKdmS2_S2_Pd" % k for k in (4, 6, 7, 8)]
    want += ["_Z21gamma_integral_kernelILi%dEEv9PointArgsPKdmS2_PdS3_" % k for k in (4, 6, 7, 8)]
    assert len(want) == 24 and sorted(got) == sorted(want)


def test_straight_line_table_is_the_power_law():
    """Host build of calc_f<4> on a straight-line table of ln n = -p ln gamma against calc_f<0> with gamma_cutoff = inf:
    1e-12 relative.  The spline returns a straight line up to rounding and |H| <= 60, so the exponential carries at most
    about 60 * 2^-52 = 1.3e-14; 1e-12 leaves room for the logarithm."""
    rng = np.random.default_rng(20240)
    for p, nn in ((2.5, 2048), (1.5, 8), (4.0, 300)):
        glo, ghi = 1.0, min(1e12, float(np.exp(60.0 / p)))      # |H| <= 60
        g = tab_bind.nodes(glo, ghi, nn)
        assert tab_bind.set_tables(glo, ghi, tab_bind.log_n_powerlaw(g, p)) == 0
        gamma = np.exp(rng.uniform(np.log(1.0001), np.log(ghi * 0.9999), 4000))
        f4, d4, c4 = tab_bind.dev_calc_f(4, [0.0], 1.0, gamma)
        f0, d0, c0 = tab_bind.dev_calc_f(0, [p, glo, ghi, np.inf], 1.0, gamma)
        rel = np.abs(f4 / f0 - 1.0).max()
        print("p", p, "nodes", nn, "max rel f", rel, "dfdg", np.abs(d4 / d0 - 1.0).max())
        assert rel < 1e-12
        assert (c4 == 0).all()
    # outside the table: f and both derivatives are 0 (the rule of power_law.rs:38,49)
    f, a, b = tab_bind.dev_calc_f(4, [0.0], 1.0, np.array([0.5, ghi * 1.001, 1e300]))
    assert (f == 0).all() and (a == 0).all() and (b == 0).all()


def test_derivatives_on_a_curved_table():
    """The finite-difference check of pitchy_pl.rs:203-238 (step 1e-6, tolerance 1e-4, gamma = 1.1 + 1e3 u, 100 draws) on a
    Juettner-shaped table; d f / d cos xi is 0."""
    EPS, TOL = 1e-6, 1e-4
    rng = np.random.default_rng(4)
    glo, ghi = 1.01, 2e3
    for temperature in (10.0, 300.0):
        g = tab_bind.nodes(glo, ghi, 2048)
        assert tab_bind.set_tables(glo, ghi, tab_bind.log_n_juettner(g, temperature)) == 0
        gamma = 1.1 + 1e3 * rng.random(100)
        cx = 0.01 + 0.98 * rng.random(100)
        f0, dfdg, dfdcx = tab_bind.dev_calc_f(4, [0.0], 1.0, gamma, cx)
        f1, _, _ = tab_bind.dev_calc_f(4, [0.0], 1.0, gamma + EPS, cx)
        keep = f0 > 1e-250          # (at T = 10 the top of the range has underflowed: nothing to difference)
        assert keep.sum() >= 20
        num = (f1 - f0) / EPS
        rel = np.abs((dfdg[keep] - num[keep]) / num[keep])
        print("T", temperature, "draws", int(keep.sum()), "max rel", rel.max())
        assert not np.isnan(rel).any() and rel.max() < TOL
        assert (dfdcx == 0).all()


def _compare(which):
    """The 16 committed rows of the golden file's (s, theta) list: the tabulated oracle against the analytic kind."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_tabulated_fixture as mf
    rows = np.load(FIXTURE)[which + "_rows"]
    assert len(rows) == 16
    gold = np.loadtxt(GOLD)
    tab, ref = mf.comparison(which, gold[rows, 0].copy(), gold[rows, 1].copy(), 8)
    assert np.isfinite(tab).all() and np.isfinite(ref).all()
    rel = np.abs(tab / ref - 1.0)
    print(which, "max rel per slot", rel.max(axis=0))
    return rel.max()


def test_tabulated_power_law_against_kind_0(oracle):
    """liboracle_tab on a 2048-node table of gamma^-2.5 exp(-gamma / 1e10) over [1, 1e12] against liboracle kind 0, all
    eight slots, within the reference's own fixture tolerance of 1 % (tests/symphony.rs:82).  Measured: 3.5e-13."""
    assert _compare("pl") < 0.01


def test_tabulated_juettner_against_kind_1(oracle):
    """The same for a Juettner table (T = 10, 2048 nodes over [1.01, 2000]) against kind 1.  Measured: 4.3e-4, on rho_Q at
    s < 2 -- the electrons below the table's first node; the Symphony slots agree to 4e-7."""
    assert _compare("tj") < 0.01


def test_argument_checks_without_a_gpu():
    from rimphony_amd import api
    one = [np.zeros(3)]
    api.check_param_count(api.TABULATED, one)                   # kind 4 with one array passes the count check
    with pytest.raises(ValueError):
        api.check_param_count(api.TABULATED, one + one)
    with pytest.raises(ValueError):
        api.check_param_count(5, one)                           # kind 5 is refused
    good = np.linspace(0.0, -30.0, 16)
    assert api.check_tables(1.0, 1e3, good).shape == (1, 16)
    bad = good.copy()
    bad[5] = np.nan
    for glo, ghi, t in ((1.0, 1e3, bad), (1.0, 1e3, good[:7]), (10.0, 10.0, good), (10.0, 5.0, good), (0.5, 1e3, good),
                        (1.0, np.inf, good), (1.0, 1e3, np.where(np.arange(16) == 3, -np.inf, good))):
        with pytest.raises(ValueError):
            api.check_tables(glo, ghi, t)
        with pytest.raises(ValueError):
            api.TabulatedDistribution(glo, ghi, t)
        assert tab_bind.set_tables(glo, ghi, t) == -1            # the library's own host check (tab_spline.h)
    d = api.TabulatedDistribution.from_function(lambda g: g ** -2.5 * np.exp(-30.0 / g - g / 500.0), 1.0, 1e4, 64)
    assert d.log_n.shape == (1, 64) and np.isfinite(d.log_n).all()


def test_spline_layout_and_bad_index():
    """The laid-out set: header, then [n_tables][n_nodes][2] = value, slope; a straight line has its slope at every node,
    a row whose index names no table has a NaN normalisation."""
    g = tab_bind.nodes(1.0, 1e6, 32)
    t = np.stack([tab_bind.log_n_powerlaw(g, 2.0), tab_bind.log_n_rolled_powerlaw(g, 2.5, 30.0, 500.0)])
    assert tab_bind.set_tables(1.0, 1e6, t) == 0
    b = tab_bind.blob()
    assert len(b) == 8 + 2 * 32 * 2 and b[0] == 2 and b[1] == 32 and b[2] == 1.0 and b[3] == 1e6
    pairs = b[8:].reshape(2, 32, 2)
    assert (pairs[:, :, 0] == t).all()
    assert np.abs(pairs[0, :, 1] + 2.0).max() < 1e-12
    norms = tab_bind.batch_norm([0.0, 1.0, 2.0, 0.5, -1.0, np.nan])
    assert np.isfinite(norms[:2]).all() and np.isnan(norms[2:]).all()
    # 1 / (4 pi int_1^1e6 g^-2 dg)
    assert abs(norms[0] * 4 * np.pi * (1 - 1e-6) - 1.0) < 1e-7
