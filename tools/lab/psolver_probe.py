"""Wall time of the file paths side by side: .fee -> .res (ESolver), .feh ->
.anh (HSolver) and .fem -> .ans (FSolver) on the same four mesh files -- the
configs[2]-sized synthetic square (1000 x 1000 cells, 2M triangles) -- in one
session.  Per solver: the five phases of get_times (LoadMesh, Cuthill, create,
solve, write), the median of --runs runs after a warm-up.  LoadMesh and
Cuthill are shared code: the three columns should agree there.

    python tools/lab/psolver_probe.py [--cells 1000] [--runs 5] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from xfemm_amd import fsolver, psolver, synth  # noqa: E402

PHASES = ("ms_load_mesh", "ms_cuthill", "ms_create", "ms_solve", "ms_write")
MESH_EXT = (".node", ".ele", ".edge", ".pbc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    kw = synth.magnetostatic(args.cells)
    nb, nl = len(kw["blocks"]), len(kw["lines"])
    with tempfile.TemporaryDirectory() as d:
        master = os.path.join(d, "master")
        t0 = time.time()
        synth.write_problem(master, kw)                       # the .fem (its mesh files are replaced below)
        synth.write_potential_mesh(master, kw["x"], kw["y"], kw["p"], kw["lbl"],
                                   edge_marks=synth.side_edge_marks(kw["p"], kw["e"]))
        common = dict(labels=[dict(block=l["block"]) for l in kw["labels"]], length_units=2, depth=1.0,
                      precision=1e-8)
        with open(master + ".fee", "w") as fh:
            fh.write(synth.potential_text("e", dict(common, blocks=[dict(ex=1.0, ey=1.0, qv=1e-6)] * nb,
                                                    lines=[dict(format=0, V=0.0)] * nl)))
        with open(master + ".feh", "w") as fh:
            fh.write(synth.potential_text("h", dict(common, blocks=[dict(kx=1.0, ky=1.0, qv=1e3)] * nb,
                                                    lines=[dict(format=0, Tset=300.0)] * nl)))
        print("mesh files written in %.1f s: %d nodes, %d elements" % (time.time() - t0, len(kw["x"]), len(kw["p"])),
              file=sys.stderr)

        def run(name, make, ext_in, ext_out):
            rows = []
            for k in range(args.runs + 1):
                base = os.path.join(d, "%s%d" % (name, k))
                for ext in MESH_EXT + (ext_in,):
                    os.link(master + ext, base + ext)         # (the solver deletes its mesh files, as the reference does)
                s = make(device=args.device)
                s.PathName = base
                t = time.perf_counter()
                ok = s.LoadProblemFile() and s.runSolver()
                wall = (time.perf_counter() - t) * 1e3
                if not ok:
                    raise SystemExit("%s failed: %s" % (name, s.last_error()))
                row = dict(s.times(), ms_total=wall, cg_iters=s.stats()["cg_iters"],
                           bytes=os.path.getsize(base + ext_out))
                if k:
                    rows.append(row)                          # (run 0: the warm-up)
                os.remove(base + ext_out)
                os.remove(base + ext_in)
                del s
            med = {key: statistics.median(r[key] for r in rows) for key in rows[0]}
            return med

        res = {"cells": args.cells, "nodes": len(kw["x"]), "elements": len(kw["p"]), "runs": args.runs,
               "fsolver": run("f", fsolver.FSolver, ".fem", ".ans"),
               "esolver": run("e", psolver.ESolver, ".fee", ".res"),
               "hsolver": run("h", psolver.HSolver, ".feh", ".anh")}
    print("%-14s %10s %10s %10s" % ("median ms", "fsolver", "esolver", "hsolver"))
    for key in PHASES + ("ms_total",):
        print("%-14s %10.1f %10.1f %10.1f" % (key[3:], res["fsolver"][key], res["esolver"][key], res["hsolver"][key]))
    print("%-14s %10d %10d %10d" % ("cg_iters", res["fsolver"]["cg_iters"], res["esolver"]["cg_iters"],
                                    res["hsolver"]["cg_iters"]))
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
