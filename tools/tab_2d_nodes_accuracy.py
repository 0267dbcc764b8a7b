#!/usr/bin/env python3
"""What the 2-D table form on gamma nodes and mu nodes of the caller's choosing measures on the CPU oracle: the figures of
profiles/tabulated_2d_nodes_accuracy.txt, from which tests/test_tabulated_2d_nodes_host.py takes its bounds (MARGIN = 4 times
each).  Runs the test module's own measuring functions.  CPU only; takes a few minutes.

usage: tab_2d_nodes_accuracy.py [out]        (default: profiles/tabulated_2d_nodes_accuracy.txt)"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_tabulated_2d_nodes_host as T  # noqa: E402


def plain_ends_lib(tmp):
    """the oracle with the plain rule on the end cells of nbar, as the test's fixture builds it"""
    from rimphony_amd import _build
    objs = []
    for c in _build.TAB_ORACLE_C:
        o = os.path.join(tmp, c[:-2] + ".o")
        subprocess.run(["gcc"] + _build.ORACLE_CFLAGS + ["-std=gnu11", "-c", os.path.join(_build.ORACLE_DIR, c), "-o", o], check=True)
        objs.append(o)
    o, out = os.path.join(tmp, "tab2d_nodes_oracle.o"), os.path.join(tmp, "liboracle_tab2dnodes_plain.so")
    subprocess.run(["g++"] + _build.ORACLE_CFLAGS + ["-std=c++17", "-DRIM_TAB_2D_PITCHY_PLAIN_ENDS", "-c",
                    os.path.join(ROOT, "tests", "support", "tab2d_nodes_oracle.cpp"), "-o", o], check=True)
    subprocess.run(["g++", "-shared", "-fopenmp", "-Wl,-z,defs"] + objs + [o, "-o", out, "-lm"], check=True)
    return T.tn.Tab2DNodesLib(out)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tabulated_2d_nodes_accuracy.txt")
    lines = ["2-D table form on gamma nodes and mu nodes of the caller's choosing, CPU oracle (tools/tab_2d_nodes_accuracy.py).",
             "The GPU returns the oracle's bits (tests/test_gpu_tabulated_2d_nodes.py), so these figures are the product's.",
             "The host tests bound each comparison by 4 times its figure (MARGIN).", "",
             "the bicubic against an mpmath natural spline, nodes jittered on both axes: |S - ref| in (1 + |S|) 2^-52, S_u and S_mu",
             "in 2^-52 x the steepest chord of the table over its spacing"]
    for shape in T.SHAPES:
        worst, count = T.surface_errors(shape)
        lines.append("  %-8s %4d points  S %.2f  S_u %.2f  S_mu %.2f" % (shape, count, worst["S"], worst["S_u"], worst["S_mu"]))
    lines += ["", "a bilinear surface on 9 jittered gamma nodes x 12 jittered mu nodes or the 9 graded mu nodes of fixture set P, against",
              "the function itself: S_u, S_mu in 2^-52 max|S| / (the narrowest spacing along the axis) -- the rounding of the table's",
              "values over the narrowest cell --, S in that of mu times the widest mu cell"]
    for name in T.BILINEAR_MU:
        worst = T.bilinear_errors(name)
        lines.append("  %-9s S %.3f  S_u %.3f  S_mu %.3f" % (name, worst["S"], worst["S_u"], worst["S_mu"]))
    lines += ["", "against the analytic tilted power law, plain and times sin^k (ln n bilinear in (u, mu), 2048 x 8 jittered mu nodes,",
              "rows finite in the reference): worst |table / reference - 1| over the rows and the eight coefficients"]
    for q, a, k in T.MEASURED_TILT:
        lines.append("  q = %-5g a = %-4g k = %-5s %.2e" % (q, a, k, T.measure_tilt(q, a, k)))
    lines += ["", "on mu nodes -1 + j 2 / 15 against the form on given gamma nodes (with k: its sin^k form), 64 jittered x 16 nodes:",
              "the normalisation, f and d f / d gamma (relative), d f / d mu (relative to f max|S_mu|), the coefficients on 12 rows"]
    for k in T.MEASURED_UNIFORM_MU:
        m = T.measure_uniform_mu(k)
        lines.append("  k = %-5s norm %.2e  f %.2e  dfdg %.2e  dfdcx %.2e  coefficients %.2e" % (
            k, m["norm"], m["f"], m["dfdg"], m["dfdcx"], m["coefficients"]))
    lines += ["", "the ring ln n = H(gamma) + ln(1 + 100 exp(-(mu - mu0)^2 / 2 w^2)), mu0 = cos 0.9, w = 0.004, on %d gamma nodes:" % T.RING_GAMMA_NODES,
              "worst |f / closed - 1| and |d f / d mu - closed| / (f max|S_mu|) over 1000 (gamma, mu), gamma at nodes"]
    pts = {name: T.measure_ring_points(name) for name in ("256 graded", "512 graded", "1024 uniform")}
    for name, m in pts.items():
        lines.append("  %-13s f %.2e  dfdcx %.2e" % (name, m["f"], m["dfdcx"]))
    lines.append("  1024 uniform over 256 graded: f %.0f times, dfdcx %.0f times" % (
        pts["1024 uniform"]["f"] / pts["256 graded"]["f"], pts["1024 uniform"]["dfdcx"] / pts["256 graded"]["dfdcx"]))
    dist, left_out = T.measure_ring_coefficients()
    lines += ["the eight coefficients at theta = 0.9, s = 3, 10, 30 (%d of 24 slots NaN on all three surfaces and left out):" % left_out]
    for pair, v in dist.items():
        lines.append("  %-34s %.2e" % (pair, v))
    lines += ["", "nbar of a flat surface on set P's mu nodes (last cell 5e-5 wide) against Gamma(3/2) Gamma(1 + k/2) / Gamma(3/2 + k/2)"]
    for k in T.END_KS:
        lines.append("  k = %-4g %.2e" % (k, T.end_cell_error(T.tn._tab(), k)))
    with tempfile.TemporaryDirectory() as tmp:
        plain = plain_ends_lib(tmp)
        lines.append("  (what is left at k = 0.5 and 1 is the cell next to the narrow end cell, [0.98, 0.99995]: it keeps the plain rule and")
        lines.append("  the singular derivative at mu = 1 is 5e-5 from its edge, 1/400 of its width)")
        lines.append("  with the plain rule on the end cells: " + "  ".join("k = %g: %.2e" % (k, T.end_cell_error(plain, k)) for k in T.END_KS))
    text = "\n".join(lines) + "\n"
    open(out, "w").write(text)
    print(text)


if __name__ == "__main__":
    main()
