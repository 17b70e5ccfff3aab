"""Lab probe: post-processing of a solved 2M-triangle electrostatic square
(bench.py's configs[2] mesh: 1000 x 1000 cells, the problem of
tools/lab/electro_probe.py), solved once.

HIP-event times (xfk_pot_time: the median of the repeats after a warm-up, the
launches alone, no copies to the host) of the element-field launch, the
corner-field launch, the block-integral launch with its sum, the one-off build
of the cell grid, and the point kernel for lattice x lattice points with
smoothing off and on; the host build of the sorted node lists and the other
mesh tables is wall clock.  Each launch is printed next to the time its
algorithmic bytes (DESIGN.md's table) take at 8 TB/s.  For the point search:
the mean number of triangle tests per point and the size of the oversize list.

The baseline of the point path is the restatement's brute force
(tests/postproc.py, vectorised over the elements) on the CPU for 10^3 points
of the same mesh, scaled to the lattice: an order of magnitude, no more.

usage: python tools/lab/postproc_probe.py [cells] [repeats] [lattice]
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


def brute_force_seconds(kw, u, xs, ys):
    """InTriangleTest of every element for each point, as the restatement's
    Post.containing does it (index-ordered edges, < 0 / > 0)."""
    X, Y = kw["x"] / u, kw["y"] / u
    p = np.asarray(kw["p"], np.int64)
    t0 = time.perf_counter()
    for x, y in zip(xs, ys):
        ok = np.ones(len(p), bool)
        for j in range(3):
            pj, pk = p[:, j], p[:, (j + 1) % 3]
            lo, hi = np.minimum(pj, pk), np.maximum(pj, pk)
            z = (X[hi] - X[lo]) * (y - Y[lo]) - (Y[hi] - Y[lo]) * (x - X[lo])
            ok &= np.where(pk > pj, ~(z < 0), ~(z > 0))
        np.nonzero(ok)
    return (time.perf_counter() - t0) / len(xs)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    lat = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    kw, _ = electrostatic_kwargs(n)
    ne, nn = len(kw["p"]), len(kw["x"])
    u = 10.0   # mm -> cm, the problem's length unit
    xs = np.linspace(kw["x"].min() / u, kw["x"].max() / u, lat).repeat(lat)
    ys = np.tile(np.linspace(kw["y"].min() / u, kw["y"].max() / u, lat), lat)
    P = kernels.ElectrostaticProblem(**kw)
    P.solve()
    t = P.time_postproc(xs, ys, repeats)
    g = P.grid_info()
    P.close()
    npts = len(xs)
    per_test = 12 + 48
    rows = [("element fields", t["element_fields"], ne * (16 + 72 + 32)),
            ("corner fields", t["corner_fields"], 3 * ne * 512),
            ("block integrals (launch + sum)", t["block_integrals"], ne * 96),
            ("cell grid build (count, scan, fill)", t["cell_grid"], 2 * ne * 60 + 2 * g["entries"] * 4 + 3 * g["nx"] * g["ny"] * 4),
            ("points, smoothing off", t["points"], npts * (84 + t["tests_per_point"] * per_test)),
            ("points, smoothing on", t["points_smooth"], npts * (84 + 48 + t["tests_per_point"] * per_test))]
    print("%d triangles, %d nodes, %d points, median of %d" % (ne, nn, npts, repeats))
    print("host build of the sorted node lists and mesh tables (wall clock): %.1f ms" % t["mesh_tables_host"])
    for name, ms, nbytes in rows:
        print("%-40s %9.4f ms   algorithmic %8.1f MB = %.4f ms at 8 TB/s" % (name, ms, nbytes / 1e6, 1e3 * nbytes / HBM))
    print("grid %d x %d cells, %d list entries, %d oversize elements; mean triangle tests per point %.2f"
          % (g["nx"], g["ny"], g["entries"], g["oversize"], t["tests_per_point"]))
    k = np.arange(1000) * 997 % npts
    per = brute_force_seconds(kw, u, xs[k], ys[k])
    print("CPU brute force (numpy, 10^3 points scaled): ~%.0e s for %d points, ~%.0e x the point kernel"
          % (per * npts, npts, per * npts / (1e-3 * t["points"])))


if __name__ == "__main__":
    main()
