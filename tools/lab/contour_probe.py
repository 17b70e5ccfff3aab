"""Lab probe: contour integrals of a solved 2M-triangle electrostatic square
(bench.py's configs[2] mesh: 1000 x 1000 cells, the problem of
tools/lab/electro_probe.py), solved once.

HIP-event times (xfk_pot_contour_time: the median of the repeats after a
warm-up, the sample launch and its per-contour sum, no copies) for one straight
segment (400 samples), one arc of 180 segments (72 000 samples) and a batch of
256 such arcs of different radii (18.4 M samples), types 1 (flux of D) and 3
(stress tensor force), smoothing on; next to each the time its algorithmic
bytes (DESIGN.md's table) take at 8 TB/s, and the wall clock of the whole call
(line_integrals: upload of the vertices, launch, read-back of two doubles per
contour).

For comparison the existing point path over the same sample points made on the
host and uploaded: the point kernel alone (xfk_pot_time) and the wall clock of
point_values (upload of the points, launch, read-back of 8 values per point).

usage: python tools/lab/contour_probe.py [cells] [repeats]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from electro_probe import electrostatic_kwargs  # noqa: E402
from xfemm_amd import kernels  # noqa: E402

HBM = 8e12
NPTS = 400


def samples(contour):
    """The sample points of lineIntegral, as the kernel makes them."""
    c = np.asarray(contour.points)
    d = c[1:] - c[:-1]
    ln = np.hypot(d[:, 0], d[:, 1])
    u = (np.arange(NPTS) + 0.5) / NPTS
    pt = c[:-1, None, :] + u[None, :, None] * d[:, None, :]
    n = np.stack([-d[:, 1] / ln, d[:, 0] / ln], axis=1)
    pt = pt + 1e-6 * n[:, None, :]
    return pt.reshape(-1, 2)


def wall(f, repeats):
    f()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        t.append(1e3 * (time.perf_counter() - t0))
    return sorted(t)[len(t) // 2]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    kw, _ = electrostatic_kwargs(n)
    ne, nn = len(kw["p"]), len(kw["x"])
    u = 10.0   # mm -> cm, the problem's length unit
    xa, xb, ya, yb = kw["x"].min() / u, kw["x"].max() / u, kw["y"].min() / u, kw["y"].max() / u
    W, H = xb - xa, yb - ya
    at = lambda fx, fy: (xa + fx * W, ya + fy * H)
    straight = kernels.Contour([at(0.131, 0.217), at(0.829, 0.673)])
    arc = kernels.Contour([at(0.3, 0.45), at(0.7, 0.55)]).bend(180., 1.)
    arcs = [kernels.Contour([at(0.5 - 0.05 - 0.0015 * k, 0.45), at(0.5 + 0.05 + 0.0015 * k, 0.55)]).bend(180., 1.)
            for k in range(256)]
    P = kernels.ElectrostaticProblem(**kw)
    P.solve()
    P.line_integral(straight, 1)   # (the mesh tables, the grid and the corner fields: built once)
    g = P.grid_info()
    print("%d triangles, %d nodes, median of %d; grid %d x %d cells" % (ne, nn, repeats, g["nx"], g["ny"]))
    for name, batch in (("one straight segment", [straight]), ("one arc of 180 segments", [arc]),
                        ("256 arcs of 180 segments", arcs)):
        pts = np.concatenate([samples(c) for c in batch])
        ns = len(pts)
        t = P.time_postproc(pts[:, 0], pts[:, 1], repeats)
        tests = t["tests_per_point"]
        nbytes = ns * (tests * 60 + 48) + 24 * ((ns + 255) // 256) + 16 * sum(len(c) for c in batch)
        print("%s: %d samples, %.2f triangle tests per sample" % (name, ns, tests))
        for kind in (1, 3):
            ms = P.time_contours(batch, kind, smooth=True, points=NPTS, repeats=repeats)
            w = wall(lambda: P.line_integrals(batch, kind, smooth=True, points=NPTS), repeats)
            print("  contour kernel + sums, type %d      %9.4f ms   algorithmic %8.2f MB = %.4f ms at 8 TB/s;"
                  " whole call %.3f ms" % (kind, ms, nbytes / 1e6, 1e3 * nbytes / HBM, w))
        w = wall(lambda: P.point_values(pts[:, 0], pts[:, 1], smooth=True), repeats)
        pbytes = ns * (84 + 48 + tests * 60)
        print("  point kernel, same points uploaded   %9.4f ms   algorithmic %8.2f MB = %.4f ms at 8 TB/s;"
              " whole call %.3f ms" % (t["points_smooth"], pbytes / 1e6, 1e3 * pbytes / HBM, w))
        missed = P.line_integrals(batch, 1)["missed"]
        assert not missed.any(), missed
    P.close()


if __name__ == "__main__":
    main()
