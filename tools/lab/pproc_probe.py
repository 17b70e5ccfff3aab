"""Lab probe: the .res of the configs[2]-sized electrostatic solve of
tools/lab/electro_probe.py (1000 x 1000 cells, 2M triangles) opened by EPProc.
The problem is solved in memory and its solution written as a .res in the
solvers' layout; the probe then prints wall milliseconds for
  read      the host-only reader (EPProc.read)
  create    open() less the read: descriptor, upload, Q marks, solution, label check
  fields    element fields and smoothed corner fields
  bounds    plot bounds (the min / max reduction and its two reads)
each the median of the repeats after one warm-up.

usage: python tools/lab/pproc_probe.py [cells] [repeats]
"""
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
from electro_probe import electrostatic_kwargs  # noqa: E402
from xfemm_amd import kernels, pproc, synth  # noqa: E402


def write_res(path, kw, V, Q, cond):
    u = 10.0   # centimetres -> the solver's mm
    with open(path, "w") as f:
        f.write(synth.potential_text("e", kw))
        f.write("[Solution]\n%d\n" % len(V))
        np.savetxt(f, np.column_stack([kw["x"] / u, kw["y"] / u, V, Q]), fmt=["%.17g", "%.17g", "%.17g", "%d"],
                   delimiter="\t")
        f.write("%d\n" % len(kw["lbl"]))
        np.savetxt(f, np.column_stack([np.asarray(kw["p"]).reshape(-1, 3), kw["lbl"]]), fmt="%d", delimiter="\t")
        f.write("%d\n" % len(cond[0]))
        for a, b in zip(*cond):
            f.write("%.17g\t%.17g\n" % (a, b))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    kw, _ = electrostatic_kwargs(n)
    P = kernels.ElectrostaticProblem(**kw)
    P.solve()
    V, Q, cond = P.solution(), P.qmarks(), P.conductors()
    P.close()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "probe.res")
        write_res(path, kw, V, Q, cond)
        print("%s: %.1f MB, %d nodes, %d triangles" % (os.path.basename(path), os.path.getsize(path) / 1e6, len(V),
                                                      len(kw["lbl"])))
        t = dict(read=[], create=[], fields=[], bounds=[])
        for k in range(repeats + 1):
            F = pproc.EPProc()
            t0 = time.perf_counter()
            assert F.read(path), F.last_error()
            t1 = time.perf_counter()
            assert F.open(path), F.last_error()
            t2 = time.perf_counter()
            Pf = F.problem()
            Pf.element_fields()
            Pf.corner_fields()
            t3 = time.perf_counter()
            Pf.plot_bounds()
            t4 = time.perf_counter()
            F.close()
            if k:
                t["read"].append(t1 - t0)
                t["create"].append((t2 - t1) - (t1 - t0))
                t["fields"].append(t3 - t2)
                t["bounds"].append(t4 - t3)
        print("wall ms (median of %d): " % repeats + ", ".join("%s %.2f" % (k, 1e3 * float(np.median(v)))
                                                                for k, v in t.items()))


if __name__ == "__main__":
    main()
