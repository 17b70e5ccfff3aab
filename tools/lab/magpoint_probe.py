"""Lab probe: point values and contour integrals of a 2M-triangle magnetostatic
square (bench.py's configs[2] mesh: 1000 x 1000 cells, synth.magnetostatic).

No solve: the kernels read A whatever it holds, so a smooth A is set
(xfk_mag_set_solution).  HIP-event times (xfk_mag_point_time,
xfk_mag_contour_time: the median of the repeats after a warm-up, launches
alone) of the corner kernel (GetNodalB), the cell grid, 10^6 lattice points
with smoothing off and on, and the three contour batches of
tools/lab/contour_probe.py (one straight segment, one arc of 180 segments, 256
such arcs; 400 samples per segment) for types 1 (H.t) and 3 (stress tensor
force), smoothing on; next to each the time its algorithmic bytes (DESIGN.md's
table) take at 8 TB/s.

usage: python tools/lab/magpoint_probe.py [cells] [repeats]
"""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from xfemm_amd import kernels, synth  # noqa: E402

HBM = 8e12
NPTS = 400
TESTS = 4.0   # triangle tests per point of this grid (xfk_pot_time measures 3.9-4.1 on the same mesh)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    kw = synth.magnetostatic(n)
    ne, nn = len(kw["p"]), len(kw["x"])
    u = [2.54, 0.1, 1., 100., 0.00254, 1.e-04][kw.get("length_units", 0)]
    x, y = np.asarray(kw["x"]) / u, np.asarray(kw["y"]) / u
    P = kernels.Static2DProblem(**kw)
    P.set_solution(1e-3 * np.sin(30 * x / x.max()) * np.cos(20 * y / y.max()))
    xa, xb, ya, yb = x.min(), x.max(), y.min(), y.max()
    W, H = xb - xa, yb - ya
    at = lambda fx, fy: (xa + fx * W, ya + fy * H)
    m = 1000
    gx, gy = np.meshgrid(xa + (np.arange(m) + 0.37) / m * W, ya + (np.arange(m) + 0.61) / m * H)
    t = P.time_points(gx.ravel(), gy.ravel(), repeats)
    v = P.point_values(gx.ravel()[:1000], gy.ravel()[:1000])
    assert (v["elem"] >= 0).all()
    npt = m * m
    print("%d triangles, %d nodes, median of %d" % (ne, nn, repeats))
    # corner kernel: per corner the node's list (about 6 elements: their nodes, B and label) and 16 bytes out
    cb = 3 * ne * (6 * (4 + 12 + 16 + 4) + 16) + 24 * nn
    pb0 = npt * (16 + TESTS * 60 + 12 + 72 + 16 + 4 + 13 * 8)
    pb1 = pb0 + npt * 48
    for name, ms, b in (("corner kernel (GetNodalB)", t["corner"], cb), ("cell grid", t["grid"], 0),
                        ("10^6 points, smoothing off", t["points"], pb0), ("10^6 points, smoothing on", t["points_smooth"], pb1)):
        print("  %-34s %9.4f ms   algorithmic %8.2f MB = %.4f ms at 8 TB/s" % (name, ms, b / 1e6, 1e3 * b / HBM))
    straight = kernels.Contour([at(0.131, 0.217), at(0.829, 0.673)])
    arc = kernels.Contour([at(0.3, 0.45), at(0.7, 0.55)]).bend(180., 1.)
    arcs = [kernels.Contour([at(0.5 - 0.05 - 0.0015 * k, 0.45), at(0.5 + 0.05 + 0.0015 * k, 0.55)]).bend(180., 1.)
            for k in range(256)]
    for name, batch in (("one straight segment", [straight]), ("one arc of 180 segments", [arc]),
                        ("256 arcs of 180 segments", arcs)):
        ns = sum((len(c.points) - 1) * NPTS for c in batch)
        nbytes = ns * (TESTS * 60 + 12 + 72 + 16 + 48) + 24 * ((ns + 255) // 256) + 16 * sum(len(c.points) for c in batch)
        for kind in (1, 3):
            ms = P.time_contours(batch, kind, smooth=True, points=NPTS, repeats=repeats)
            print("  %-26s type %d %9.4f ms   algorithmic %8.2f MB = %.4f ms at 8 TB/s (%d samples)"
                  % (name, kind, ms, nbytes / 1e6, 1e3 * nbytes / HBM, ns))
        missed = P.line_integrals(batch, 1)["missed"]
        assert not missed.any(), missed
    P.close()


if __name__ == "__main__":
    main()
