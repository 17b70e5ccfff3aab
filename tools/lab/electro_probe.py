"""Lab probe: a 2M-triangle planar electrostatic square next to the
magnetostatic solve of the same structured mesh (bench.py's configs[2]: 1000 x
1000 cells), in one process.  Prints the solved DoF/s of both: the whole
solve (symbolic phase rebuilt, assembly, AMG setup, PCG) per wall-clock
second, the median of the timed repeats after one warm-up solve.

The electrostatic problem keeps the magnetostatic one's regions: the outer
boundary at 0 V (BdryFormat 0 edges), a dielectric where the steel is, +- qv
where the coils are, and a prescribed-voltage conductor on the nodes of the
magnet's region (its Dirichlet rows and the charge integral after the solve).

usage: python tools/lab/electro_probe.py [cells] [repeats]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from xfemm_amd import kernels, synth  # noqa: E402


def electrostatic_kwargs(n):
    m = synth.magnetostatic(n)
    x, y, p, lbl = m["x"] * 10.0, m["y"] * 10.0, m["p"], m["lbl"]   # cm -> mm
    cond = -np.ones(len(x), np.int32)
    cond[np.unique(p[lbl == 4])] = 0
    return dict(x=x, y=y, p=p, lbl=lbl, e=m["e"], conductor=cond,
                blocks=[dict(ex=1.0, ey=1.0), dict(ex=4.0, ey=4.0), dict(ex=1.0, ey=1.0, qv=1e-6),
                        dict(ex=1.0, ey=1.0, qv=-1e-6), dict(ex=1.0, ey=1.0)],
                labels=[dict(block=k) for k in range(5)], lines=[dict(format=0, V=0.0)],
                conductors=[dict(type=1, V=100.0)], depth=1.0, length_units=2, precision=1e-8), m


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
    ekw, mkw = electrostatic_kwargs(n)
    dof = len(ekw["x"])
    for name, P in (("magnetostatic", kernels.Static2DProblem(**mkw)),
                    ("electrostatic", kernels.ElectrostaticProblem(**ekw))):
        t, r = timed(P, repeats)
        extra = ""
        if name == "electrostatic":
            V, q = P.conductors()
            extra = " conductor q %.6e C" % q[0]
        print("%s: %d tri, %d DoF, %.2f ms/solve, %.3e DoF/s (cg %d, precond %s, levels %d, assemble %.3f ms, "
              "solve %.3f ms)%s" % (name, len(ekw["p"]), dof, 1e3 * t, dof / t, r["cg_iters"],
                                    "amg" if r["precond"] == kernels.XFK_PRECOND_AMG else "jacobi", r["amg_levels"],
                                    r["ms_assemble"], r["ms_solve"], extra), flush=True)
        P.close()


if __name__ == "__main__":
    main()
