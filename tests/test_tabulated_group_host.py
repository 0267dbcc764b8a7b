"""Host-side checks of the tabulated distribution's group kernels (rimphony_tab_group.hip): the compiler's resource report
of the new translation unit, the build recipes and the export, and the knob's text.  No GPU."""
import os
import re
import subprocess

import pytest

from rimphony_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rimphony_amd", "csrc")
UNIT = os.path.join(CSRC, "rimphony_tab_group.hip")


def test_tab_group_kernel_resources_leave_room_for_its_grid(tmp_path):
    """What test_host_side.py::test_group_kernel_resources_leave_room_for_its_grid asks of rimphony_group.hip, of the
    tabulated kind's unit: compiled alone for gfx950 it reports exactly four SymGroupProblem kernels, each resident
    RIM_GROUP_WAVES times per SIMD and with an LDS block that fits 4 x that many times into a CU's 160 KB with one 512-byte
    granule to spare -- the grid is sized for that, and a wave that is not resident is waited for by the cooperative tail."""
    hipcc = _build.find_hipcc()
    if hipcc is None:
        pytest.skip("no hipcc")
    flags = [f for f in _build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    r = subprocess.run([hipcc] + flags + ["--cuda-device-only", "-c", UNIT, "-o", str(tmp_path / "g.o"),
                                           "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(os.path.join(CSRC, "group_launch.h")).read()
    waves = int(re.search(r"#define RIM_GROUP_WAVES (\d+)", text).group(1))
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    names = []
    for b in blocks:
        name = b.split()[0]
        if "SymGroupProblem" not in name:
            continue
        names.append(name)
        occ = int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", b).group(1))
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
        print(name, "occupancy", occ, "LDS", lds, "VGPRs", re.search(r"VGPRs: (\d+)", b).group(1),
              "scratch", re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1))
        assert occ >= waves, (name, occ)
        granules = (lds + 511) // 512 * 512
        assert 4 * waves * granules <= 160 * 1024 - 512, (name, lds)
    # DIST_TABULATED, _ISO, _2D, _PITCHY (dev_symphony.h) and nothing else
    assert sorted(names) == ["_Z12group_kernelI15SymGroupProblemILi%dEEEv9GroupArgs" % k for k in (4, 5, 6, 7)]


def test_build_and_export():
    """The new unit is a source of the library and compiled by the build; tab_launch.h declares its one lookup; the analytic
    kinds' unit still knows nothing of the tabulated kind; and the library's C ABI is the public header's: the feature adds
    no entry point."""
    assert UNIT in _build.hip_sources()
    assert os.path.join(CSRC, "group_kernel.h") in _build.hip_sources()
    seen = []
    real_run, real_newer = subprocess.run, _build._newer
    try:
        _build._newer = lambda *a: False
        subprocess.run = lambda cmd, **kw: seen.append(cmd)
        _build.build_hip(force=True)
    finally:
        subprocess.run, _build._newer = real_run, real_newer
    assert len(seen) == 1 and UNIT in seen[0] and os.path.join(CSRC, "rimphony_group.hip") in seen[0]
    for recipe in ("build_variant.sh", "build_prof.sh"):
        for line in open(os.path.join(ROOT, "tools", recipe)):
            assert ("rimphony_tab.hip" in line) == ("rimphony_tab_group.hip" in line), (recipe, line)
    assert re.search(r"const void \*rim_tab_group_kernel\(int tab_kind\);", open(os.path.join(CSRC, "tab_launch.h")).read())
    # (which instantiations the unit holds is test_tab_group_kernel_resources_leave_room_for_its_grid's exact name set)
    assert "group_kernel<SymGroupProblem<KIND>>" in open(UNIT).read()
    group = open(os.path.join(CSRC, "rimphony_group.hip")).read()
    assert "DIST_TABULATED" not in group and "rim_with_kind5" not in group
    assert "group_kernel<SymGroupProblem<KIND>>" in group and "rim_with_kind(kind" in group
    lib = _build.build_hip()
    r = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    exported = [l.split()[-1] for l in r.stdout.splitlines()]
    assert any("rim_tab_group_kernel" in s for s in exported)          # the lookup is linked in (a C++ symbol)
    c_abi = [s for s in exported if not s.startswith(("_Z", "__hip_"))]
    header = open(os.path.join(ROOT, "include", "rimphony_hip.h")).read()
    declared = set(re.findall(r"\b((?:rimphony|pkgw)_\w+)\s*\(", header))
    assert len(c_abi) >= 40 and sorted(set(c_abi) - declared) == []
    assert not [s for s in c_abi if "group" in s]


def test_knob_text():
    """RIMPHONY_TAB_GROUP is in the knob table and in DESIGN.md's table of environment variables with the same default,
    and the one per-form default table cites the measurements it comes from."""
    src = open(os.path.join(CSRC, "rimphony_hip.hip")).read()
    m = re.search(r'\{ "RIMPHONY_TAB_GROUP", KNOB_INT, &RimKnobs::tab_group, (-?\d+), INT_MIN, 1,', src)
    assert m and int(m.group(1)) == -1
    table = src[src.index("static const RimKnobDef RIM_KNOBS[]"):src.index("static RimKnobs rim_read_knobs()")]
    assert "RIMPHONY_TAB_GROUP" in table
    row = [l for l in open(os.path.join(ROOT, "DESIGN.md")) if l.startswith("| `RIMPHONY_TAB_GROUP` |")]
    assert len(row) == 1
    cells = [c.strip() for c in row[0].split("|")]
    assert cells[3].startswith("-1") and "at most 1" in cells[2]
    # one table for the five forms; the comment above it cites both measurement files
    assert len(re.findall(r"^static const bool RIM_TAB_GROUP_DEFAULT\w*", src, re.M)) == 1
    at = src.index("static const bool RIM_TAB_GROUP_DEFAULT[5]")
    dflt = src[at - 600:at]
    dflt = dflt[dflt.index("// Where the Symphony slots of the tabulated distribution run"):]
    for cited in ("profiles/tabulated_group_times.txt", "profiles/tabulated_grid_times.txt"):
        assert cited in dflt
        assert os.path.exists(os.path.join(ROOT, cited))
