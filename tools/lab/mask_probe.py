"""Lab probe: the weighted stress tensor force on a dielectric disc in air, on
bench.py's configs[2] mesh (1000 x 1000 cells, 2M triangles), next to the
electrostatic solve of the same problem for scale, in one process.

The outer boundary is at 0 V (BdryFormat 0 edges), a prescribed-voltage
conductor sits on the nodes of a small square left of the disc, the disc
(radius 0.15 L about the centre, er = 4) is the selection.  Prints the
electrostatic solve's times, then of the mask: the first make_mask (which
creates the auxiliary problem and runs its symbolic phase), and the medians of
the timed repeats after that warm-up -- the fixed values with their validity
check ("creation"), the setup (row gather and AMG setup), the PCG, the
integral launch of types 5 and 6 -- and the force and torque.

usage: python tools/lab/mask_probe.py [cells] [repeats]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from xfemm_amd import kernels, synth  # noqa: E402


def disc_kwargs(n):
    m = synth.magnetostatic(n)
    L = 10.0
    x, y, p = m["x"], m["y"], m["p"]
    cx, cy = x[p].mean(axis=1) / L, y[p].mean(axis=1) / L
    lbl = (np.hypot(cx - 0.5, cy - 0.5) < 0.15).astype(np.int32)
    cond = -np.ones(len(x), np.int32)
    u, v = x / L, y / L
    cond[(u > 0.08) & (u < 0.16) & (v > 0.40) & (v < 0.60)] = 0
    return dict(x=x * 10.0, y=y * 10.0, p=p, lbl=lbl, e=m["e"], conductor=cond,   # cm -> mm
                blocks=[dict(ex=1.0, ey=1.0), dict(ex=4.0, ey=4.0)], labels=[dict(block=0), dict(block=1)],
                lines=[dict(format=0, V=0.0)], conductors=[dict(type=1, V=100.0)], depth=1.0, length_units=2,
                precision=1e-8)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    kw = disc_kwargs(n)
    P = kernels.ElectrostaticProblem(**kw)
    P.solve()
    ts, r = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        r = P.solve(rebuild_symbolic=True)
        ts.append(time.perf_counter() - t0)
    print("electrostatic: %d tri, %d DoF, %.2f ms/solve wall (symbolic %.3f, assemble %.3f, amg setup %.3f, "
          "pcg %.3f ms; cg %d, levels %d)" % (len(kw["p"]), len(kw["x"]), 1e3 * np.median(ts), r["ms_symbolic"],
                                               r["ms_assemble"], r["ms_amg_setup"], r["ms_solve"], r["cg_iters"],
                                               r["amg_levels"]), flush=True)
    t0 = time.perf_counter()
    first = P.make_mask([1])
    t_first = 1e3 * (time.perf_counter() - t0)
    print("mask, first call: %.2f ms wall with the read-back of W and msk; %s" % (t_first, first["times"]), flush=True)
    runs = [P.make_mask([1]) for _ in range(repeats)]
    med = {k: float(np.median([q["times"][k] for q in runs])) for k in runs[0]["times"]}
    t_int = P.time_stress(repeats)
    w = P.weighted_stress([1])
    # (the PCG time is xfk_result's ms_solve: the AMG setup runs inside it)
    print("mask, median of %d: creation (fixed values, validity) %.3f ms; setup: assemble %.3f + amg setup %.3f ms; "
          "solve (pcg with that setup) %.3f ms, cg %d; whole make_mask %.3f ms; integrals 5 and 6 %.3f ms"
          % (repeats, med["fixed_values"], med["assemble"], med["amg_setup"], med["solve"], runs[-1]["cg_iters"],
             med["total"], t_int), flush=True)
    print("mask: %d of %d nodes 1; force %s N, torque %.6e N m"
          % (int(runs[-1]["msk"].sum()), len(kw["x"]), w["force"], w["torque"]), flush=True)
    P.close()


if __name__ == "__main__":
    main()
