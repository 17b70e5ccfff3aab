"""Lab probe: a nonlinear heat-flow problem on the 2M-triangle structured
square (bench.py's configs[2]: 1000 x 1000 cells), the mesh
tools/lab/electro_probe.py solves.  Prints the solved DoF/s and the pass
count: the whole xfk_heatflow call (symbolic phase rebuilt, every pass's
assembly, AMG setup or refresh, PCG, the change norm's read-back) per
wall-clock second, the median of the timed repeats after one warm-up solve.
DoF/s counts the unknowns once, whatever the number of passes.

The problem keeps the magnetostatic one's regions: the outer boundary at 300 K
(BdryFormat 0 edges), a K(T) table where the steel is, heating and cooling
where the coils are, and a prescribed-temperature conductor on the nodes of
the magnet's region (its Dirichlet rows and the flow integral after the solve).

usage: python tools/lab/heat_probe.py [cells] [repeats]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from xfemm_amd import kernels, synth  # noqa: E402


def heatflow_kwargs(n):
    m = synth.magnetostatic(n)
    x, y, p, lbl = m["x"] * 0.01, m["y"] * 0.01, m["p"], m["lbl"]   # cm -> m
    cond = -np.ones(len(x), np.int32)
    cond[np.unique(p[lbl == 4])] = 0
    return dict(x=x, y=y, p=p, lbl=lbl, e=m["e"], conductor=cond,
                blocks=[dict(kx=1.0, ky=1.0),
                        dict(kx=40.0, ky=40.0, T=[300.0, 350.0, 400.0, 500.0], K=[40.0, 36.0, 33.0, 30.0]),
                        dict(kx=1.0, ky=1.0, qv=2e4), dict(kx=1.0, ky=1.0, qv=-2e4), dict(kx=1.0, ky=1.0)],
                labels=[dict(block=k) for k in range(5)], lines=[dict(format=0, Tset=300.0)],
                conductors=[dict(type=1, T=400.0)], depth=1.0, length_units=2, precision=1e-8)


def timed(P, repeats):
    P.solve()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = P.solve(rebuild_symbolic=True)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    kw = heatflow_kwargs(n)
    dof = len(kw["x"])
    P = kernels.HeatFlowProblem(**kw)
    t, r = timed(P, repeats)
    T, q = P.conductors()
    V = P.solution()
    print("heat flow: %d tri, %d DoF, %d passes (last change %.2e), %.2f ms/solve, %.3e DoF/s (cg %d, precond %s, "
          "levels %d, assemble %.3f ms, solve %.3f ms) T %.1f .. %.1f K, conductor flow %.6e W"
          % (len(kw["p"]), dof, r["newton_iters"], r["last_res"], 1e3 * t, dof / t, r["cg_iters"],
             "amg" if r["precond"] == kernels.XFK_PRECOND_AMG else "jacobi", r["amg_levels"], r["ms_assemble"],
             r["ms_solve"], V.min(), V.max(), q[0]), flush=True)
    P.close()


if __name__ == "__main__":
    main()
