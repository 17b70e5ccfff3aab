"""Lab probe: post-processing of a magnetostatic square on the device
(bench.py's configs[2] mesh: 1000 x 1000 cells, 2M triangles, linear mu).

No solve: the block integrals read A whatever it holds, so a smooth A is set
(xfk_mag_set_solution).  HIP-event times (xfk_mag_time: the median of the
repeats after a warm-up, the launches alone, no copies to the host) of the
element-B launch and of the block-integral launch with its sum, every label
selected, each next to the time its algorithmic bytes (DESIGN.md's table) take
at 8 TB/s.  Prints one JSON line.

usage: python tools/lab/magpost_probe.py [cells] [repeats]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
from xfemm_amd import kernels, synth  # noqa: E402

HBM = 8e12


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    kw = synth.magnetostatic(n)
    ne, nn = len(kw["p"]), len(kw["x"])
    P = kernels.Static2DProblem(**kw)
    x, y = 0.01 * np.asarray(kw["x"]), 0.01 * np.asarray(kw["y"])
    P.set_solution(1e-3 * np.sin(30 * x) * np.cos(20 * y))
    P.set_depth(5.0)
    ms = P.time_postproc(repeats)
    nl = len(kw["labels"])
    r = P.block_integrals(np.ones(nl, bool))
    P.close()
    # algorithmic bytes: 12 (nodes) + 4 (label) per element, x y A once per node
    # (24 per node; 72 per element when nothing is cached), B written (16), the
    # partials (15 doubles per 256 elements)
    b_elem = ne * (12 + 16) + nn * 24
    b_int = ne * (12 + 4) + nn * 24 + (ne / 256) * 15 * 8 * 2
    b_int_uncached = ne * (12 + 4 + 72) + (ne / 256) * 15 * 8 * 2
    out = dict(cells=n, elements=ne, nodes=nn, repeats=repeats,
               element_b_ms=ms["element_b"], block_integrals_ms=ms["block_integrals"],
               element_b_bytes=b_elem, block_integrals_bytes=b_int,
               block_integrals_bytes_uncached=b_int_uncached,
               element_b_fraction_of_8TBs=b_elem / HBM / (1e-3 * ms["element_b"]),
               block_integrals_fraction_of_8TBs=b_int / HBM / (1e-3 * ms["block_integrals"]),
               block_integrals_fraction_of_8TBs_uncached=b_int_uncached / HBM / (1e-3 * ms["block_integrals"]),
               energy=r["energy"], volume=r["volume"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
