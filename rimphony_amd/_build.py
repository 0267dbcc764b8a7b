"""Build helpers: compile the HIP library (gfx950) and, for tests, the CPU oracle.

The product library is librimphony_hip.so, built in-tree with hipcc.  Flags that
matter for correctness (DESIGN.md "Rounding contract"):
  -ffp-contract=off          only the explicit fma() calls fuse, exactly as in the oracle
  -mllvm -disable-machine-licm
      the integrand contains ~300 distinct fp64 literals; gfx9 VOP3 cannot encode
      64-bit literals, and MachineLICM otherwise hoists their materialisation out
      of the quadrature loops into ~200 long-lived VGPRs (256 VGPR + AGPR spills,
      1 wave/SIMD).  With hoisting off the constants are rebuilt by the scalar unit
      next to their use and the Symphony kernel fits 80 VGPRs (6 waves/SIMD).
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rimphony_amd", "csrc")
LIB = os.path.join(ROOT, "rimphony_amd", "librimphony_hip.so")
ORACLE_DIR = os.path.join(ROOT, "oracle")

HIPCC_FLAGS = [
    "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-shared",
    "-ffp-contract=off", "-mllvm", "-disable-machine-licm",
    # host side of the translation units (the pkgw_bessel_j / pkgw_bessel_dj seam is the HOST build of
    # dev_bessel.h): inline fma instead of calls into libm, as the oracle's Makefile does
    "-Xarch_host", "-mfma",
]


def _newer(target, sources):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(s) <= t for s in sources)


def hip_sources():
    srcs = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))]
    srcs.append(os.path.join(ROOT, "include", "rimphony_hip.h"))
    return srcs


def source_id():
    """16 hex digits identifying the kernel sources of this tree (csrc/*.h, *.hip, the C-ABI header): profiles record
    it so that bench.py only quotes a PMC figure for the build it was measured on."""
    import hashlib
    h = hashlib.sha256()
    for path in hip_sources():
        h.update(os.path.basename(path).encode())
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


def find_hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


def build_hip(force=False, verbose=False):
    """Compile librimphony_hip.so for gfx950 (cross-compiles without a GPU)."""
    srcs = hip_sources()
    if not force and _newer(LIB, srcs):
        return LIB
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("hipcc not found: cannot build librimphony_hip.so")
    cmd = [hipcc] + HIPCC_FLAGS + [os.path.join(CSRC, "rimphony_hip.hip"), os.path.join(CSRC, "rimphony_diag.hip"),
                                    os.path.join(CSRC, "rimphony_group.hip"), os.path.join(CSRC, "rimphony_multi.hip"),
                                    os.path.join(CSRC, "rimphony_tab.hip"), os.path.join(CSRC, "rimphony_tab_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_grid_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_grid.hip"), os.path.join(CSRC, "rimphony_tab_2d_grid_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_pitchy.hip"), os.path.join(CSRC, "rimphony_tab_2d_pitchy_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_grid_pitchy.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_grid_pitchy_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_nodes.hip"), os.path.join(CSRC, "rimphony_tab_2d_nodes_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_nodes_pitchy.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_nodes_pitchy_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_family.hip"), os.path.join(CSRC, "rimphony_tab_family_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_family_pitchy.hip"),
                                    os.path.join(CSRC, "rimphony_tab_family_pitchy_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_family.hip"), os.path.join(CSRC, "rimphony_tab_2d_family_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_family_pitchy.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_family_pitchy_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_family_cubic.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_family_cubic_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_family_cubic_pitchy.hip"),
                                    os.path.join(CSRC, "rimphony_tab_2d_family_cubic_pitchy_group.hip"),
                                    os.path.join(CSRC, "rimphony_tab_install.hip"),
                                    "-ldl", "-o", LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True, cwd=ROOT)
    return LIB


def build_oracle(force=False):
    """Compile the CPU oracle (test infrastructure; never loaded by the product)."""
    if force:
        subprocess.run(["make", "-C", ORACLE_DIR, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", ORACLE_DIR, "all"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(ORACLE_DIR, "liboracle.so")


def build_test_support():
    """Host build of the scalar device functions (CPU tests only)."""
    src = os.path.join(ROOT, "tests", "support", "devfn_host.cpp")
    out = os.path.join(ROOT, "tests", "support", "devfn_host.so")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if _newer(out, deps):
        return out
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-math-errno",
                    "-mfma", "-msse4.1", "-shared", src, "-o", out], check=True)
    return out


# the oracle's calculators without its distribution file (oracle/Makefile: SRCS minus rimo_dist.c), and its flags
TAB_ORACLE_C = ["rimo_quad.c", "rimo_bessel.c", "rimo_symphony.c", "rimo_heyvaerts.c", "rimo_highfreq.c"]
ORACLE_CFLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-fno-math-errno", "-mfma", "-msse4.1", "-fopenmp"]


def _build_dist_oracle(src_name, out_name):
    """One distribution file under tests/support linked with the oracle's unchanged calculators."""
    import tempfile
    src = os.path.join(ROOT, "tests", "support", src_name)
    out = os.path.join(ROOT, "tests", "support", out_name)
    csrcs = [os.path.join(ORACLE_DIR, f) for f in TAB_ORACLE_C]
    deps = [src] + csrcs + [os.path.join(ORACLE_DIR, f) for f in ("rimo.h", "rimo_math.h")] + \
        [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if _newer(out, deps):
        return out
    with tempfile.TemporaryDirectory() as tmp:
        objs = []
        for c in csrcs:
            o = os.path.join(tmp, os.path.basename(c)[:-2] + ".o")
            subprocess.run(["gcc"] + ORACLE_CFLAGS + ["-std=gnu11", "-c", c, "-o", o], check=True)
            objs.append(o)
        o = os.path.join(tmp, src_name[:-4] + ".o")
        subprocess.run(["g++"] + ORACLE_CFLAGS + ["-std=c++17", "-c", src, "-o", o], check=True)
        objs.append(o)
        subprocess.run(["g++", "-shared", "-fopenmp", "-Wl,-z,defs"] + objs + ["-o", out, "-lm"], check=True)
    return out


def build_tab_oracle():
    """The CPU oracle of the tabulated distribution (tests only): tests/support/tab_oracle.cpp supplies the three
    distribution symbols the oracle's calculators call, on top of the host build of the device functions."""
    return _build_dist_oracle("tab_oracle.cpp", "liboracle_tab.so")


def build_tab_pitch_oracle():
    """The same for table sets with a pitch-angle factor (tests/support/tab_pitch_oracle.cpp)."""
    return _build_dist_oracle("tab_pitch_oracle.cpp", "liboracle_tabpitch.so")


def build_beam_oracle():
    """The CPU oracle of an analytic power law times an exponential beam in cos xi (tests/support/beam_oracle.cpp): what the
    pitch tables are compared with.  Tests only."""
    return _build_dist_oracle("beam_oracle.cpp", "liboracle_beam.so")


def build_tab2d_oracle():
    """The same for 2-D table sets, ln n(gamma, mu) on a grid (tests/support/tab2d_oracle.cpp)."""
    return _build_dist_oracle("tab2d_oracle.cpp", "liboracle_tab2d.so")


def build_tilt_oracle():
    """The CPU oracle of an analytic non-separable distribution, a power law whose index depends on the pitch angle
    (tests/support/tilt_oracle.cpp): what the 2-D tables are compared with.  Tests only."""
    return _build_dist_oracle("tilt_oracle.cpp", "liboracle_tilt.so")


def build_tab_pitchy_oracle():
    """The same for table sets with a sin^k xi prefactor per table (tests/support/tab_pitchy_oracle.cpp)."""
    return _build_dist_oracle("tab_pitchy_oracle.cpp", "liboracle_tabpitchy.so")


def build_tab_family_oracle():
    """The same for families of energy tables, a real index per row (tests/support/tab_family_oracle.cpp)."""
    return _build_dist_oracle("tab_family_oracle.cpp", "liboracle_tabfamily.so")


def build_tab2d_family_oracle():
    """The same for families of 2-D surfaces on given gamma and mu nodes, a real index per row
    (tests/support/tab2d_family_oracle.cpp)."""
    return _build_dist_oracle("tab2d_family_oracle.cpp", "liboracle_tab2dfamily.so")


def build_tab2d_family_cubic_oracle():
    """The same for families of 2-D surfaces blended cubically across their tables
    (tests/support/tab2d_family_cubic_oracle.cpp)."""
    return _build_dist_oracle("tab2d_family_cubic_oracle.cpp", "liboracle_tab2dfamilycubic.so")


def build_pitchy_beam_oracle():
    """The CPU oracle of an analytic power law times sin^k xi times an exponential beam in cos xi
    (tests/support/pitchy_beam_oracle.cpp): what the tables with a sin^k prefactor are compared with.  Tests only."""
    return _build_dist_oracle("pitchy_beam_oracle.cpp", "liboracle_pitchy_beam.so")


def build_tab_grid_oracle():
    """The same for table sets on given gamma nodes (tests/support/tab_grid_oracle.cpp)."""
    return _build_dist_oracle("tab_grid_oracle.cpp", "liboracle_tabgrid.so")


def build_tab2d_grid_oracle():
    """The same for 2-D table sets on given gamma nodes (tests/support/tab2d_grid_oracle.cpp)."""
    return _build_dist_oracle("tab2d_grid_oracle.cpp", "liboracle_tab2dgrid.so")


def build_tab2d_pitchy_oracle():
    """The same for 2-D table sets with a sin^k xi prefactor per table, on nodes uniform in ln gamma or given
    (tests/support/tab2d_pitchy_oracle.cpp)."""
    return _build_dist_oracle("tab2d_pitchy_oracle.cpp", "liboracle_tab2dpitchy.so")


def build_tab2d_nodes_oracle():
    """The same for 2-D table sets on gamma nodes and mu nodes of the caller's choosing, with or without a sin^k xi
    prefactor (tests/support/tab2d_nodes_oracle.cpp)."""
    return _build_dist_oracle("tab2d_nodes_oracle.cpp", "liboracle_tab2dnodes.so")


def build_tab2d_ends_oracle():
    """The same for 2-D table sets of any of the six forms with a choice of the spline's ends per axis, and the host build
    of the per-line solver of the device install (tests/support/tab2d_ends_oracle.cpp)."""
    return _build_dist_oracle("tab2d_ends_oracle.cpp", "liboracle_tab2dends.so")


def build_pitchy_tilt_oracle():
    """The CPU oracle of the analytic tilted power law times sin^k xi (tests/support/pitchy_tilt_oracle.cpp): what the 2-D
    tables with a sin^k prefactor are compared with.  Tests only."""
    return _build_dist_oracle("pitchy_tilt_oracle.cpp", "liboracle_pitchy_tilt.so")
