"""Lab probe: the weighted stress tensor mask and integrals 18-23 of a
magnetostatic problem on the device.

Two problems, each solved first: bench.py's configs[2] mesh (1000 x 1000 cells,
2M triangles, linear mu) with the +J coil selected -- it lies in the air of the
core's window -- and the TorqueBenchmark fixture at 30 degrees with every label
inside its air gap's inner radius selected (the rotor).  make_mask runs twice:
the first call creates the auxiliary problem and its symbolic phase, the second
is the steady cost; mask_info()["times"] are the library's wall-clock and
HIP-event parts (ms), time_stress the HIP-event median of the k_mag_stress
launch with its sum.  Prints one JSON line per problem.

usage: python tools/lab/magmask_probe.py [cells] [repeats]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from xfemm_amd import kernels, synth  # noqa: E402


def probe(name, kw, sel, depth, repeats):
    P = kernels.Static2DProblem(**kw)
    t0 = time.perf_counter()
    r = P.solve()
    out = dict(problem=name, elements=len(kw["p"]), nodes=len(kw["x"]), selected=[int(s) for s in sel],
               solve_wall_ms=1e3 * (time.perf_counter() - t0), solve_cg_iters=r["cg_iters"],
               solve_ms=dict(symbolic=r["ms_symbolic"], assemble=r["ms_assemble"], amg_setup=r["ms_amg_setup"],
                             solve=r["ms_solve"]))
    P.set_depth(depth)
    try:
        t0 = time.perf_counter()
        P.make_mask(sel)
        out["first_make_mask_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        out["first_times"] = P.mask_info()["times"]
        m = P.make_mask(sel)
        out["mask_times"] = m["times"]
        out["mask_cg_iters"] = m["cg_iters"]
        out["mask_ones"] = int(m["msk"].sum())
        out["stress_ms"] = P.time_stress(repeats)
        out["postproc_ms"] = P.time_postproc(repeats)
        w = P.weighted_stress(sel)
        raw = P.block_integrals(sel)["raw"]
        out["weighted_stress"] = dict(force=w["force"].tolist(), torque=w["torque"])
        out["lorentz"] = dict(force=[raw[11].real, raw[12].real], torque=raw[15].real)
    except kernels.XfkError as e:
        out["error"] = str(e)
    P.close()
    print(json.dumps(out), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    probe("configs[2] square, +J coil", synth.magnetostatic(n), [2], 5.0, repeats)
    from oracle import femfile
    from torque import write_case
    from util import kernel_kwargs
    with tempfile.TemporaryDirectory() as d:
        pr, mesh = femfile.load_problem(write_case(d, 30))
    kw = kernel_kwargs(pr, mesh)
    ri = min(a["ri"] for a in kw["ages"])
    u = (2.54, 0.1, 1., 100., 0.00254, 1.e-04)[kw["length_units"]]
    p, lbl = np.asarray(kw["p"]), np.asarray(kw["lbl"])
    rad = np.hypot(np.asarray(kw["x"])[p].mean(axis=1), np.asarray(kw["y"])[p].mean(axis=1)) / u
    sel = [k for k in range(len(kw["labels"])) if np.any(lbl == k) and rad[lbl == k].max() < ri]
    probe("TorqueBenchmark 30 deg, rotor", kw, sel, pr.Depth, repeats)


if __name__ == "__main__":
    main()
