"""Lab probe: post-processing of a time-harmonic square on the device
(synth.harmonic's mesh at 1000 x 1000 cells, 2M triangles, linear blocks).
The sibling of magpost_probe.py; run both in one visit to compare.

No solve: the block integrals read A whatever it holds, so a smooth complex A
is set (xfk_mag_ac_set_solution).  HIP-event times (xfk_mag_ac_time: the median
of the repeats after a warm-up, the launches alone, no copies to the host) of
the complex element-B launch and of the block-integral launch with its sum,
every label selected, each next to the time its algorithmic bytes (DESIGN.md's
table) take at 8 TB/s.  Prints one JSON line.

usage: python tools/lab/magac_probe.py [cells] [repeats]
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
    kw = synth.harmonic(n)
    ne, nn = len(kw["p"]), len(kw["x"])
    P = kernels.Harmonic2DProblem(**kw)
    x, y = 0.01 * np.asarray(kw["x"]), 0.01 * np.asarray(kw["y"])
    P.set_solution_complex(1e-3 * np.sin(30 * x) * np.cos(20 * y) * np.exp(1j * (3 * x - 2 * y)))
    P.set_depth(5.0)
    ms = P.time_postproc_complex(repeats)
    nl = len(kw["labels"])
    r = P.block_integrals_complex(np.ones(nl, bool))
    P.close()
    # algorithmic bytes: 12 (nodes) + 4 (label) per element, x y and the complex
    # A once per node (32 per node), B1 and B2 written (32), the partials (28
    # doubles per 256 elements, written and read)
    b_elem = ne * (12 + 32) + nn * 32
    b_int = ne * (12 + 4) + nn * 32 + (ne / 256) * 28 * 8 * 2
    out = dict(cells=n, elements=ne, nodes=nn, repeats=repeats,
               element_b_ms=ms["element_b"], block_integrals_ms=ms["block_integrals"],
               element_b_bytes=b_elem, block_integrals_bytes=b_int,
               element_b_fraction_of_8TBs=b_elem / HBM / (1e-3 * ms["element_b"]),
               block_integrals_fraction_of_8TBs=b_int / HBM / (1e-3 * ms["block_integrals"]),
               energy=r["energy"].real, total_loss=r["total_loss"].real, volume=r["volume"].real)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
