"""The literal restatement of the reference's post-processors (tests/postproc.py)
reproduces the reference's own recorded output: epproc/test/test.out.check for
the electrostatic fixture, hpproc/test/Temp0.out.check and Temp1.out.check for
the heat-flow ones, every number within half a unit of the last digit %f
prints plus rounding slack (5.1e-7 absolute).

The recorded point (0.01, 0.01) of the heat-flow fixtures is a mesh node
shared by elements of two materials; the reference's stateful search returned
different elements for its "smoothing off" and "smoothing on" lines.  There a
recorded line must equal the restatement at one of the containing elements."""
import os

import numpy as np
import pytest

import electro
import heat
import postproc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 5.1e-7

ES_NAMES = dict(V=0, Dx=1, Dy=2, Ex=3, Ey=4, ex=5, ey=6, nrg=7)
HF_NAMES = dict(T=0, Fx=1, Fy=2, Kx=3, Ky=4, Gx=5, Gy=6)


def load(name):
    """(Post, recorded check, physics) of one fixture (cached: the restatement is built once)."""
    if name not in load.cache:
        if name == "test":
            r = electro.read_res(os.path.join(GOLD, "esolver", "test.res.check"))
            P = postproc.Post(r["kw"], r["V"], "es")
            chk = postproc.read_check(os.path.join(GOLD, "epproc", "test.out.check"))
        else:
            r = heat.read_anh(os.path.join(GOLD, "hpproc", name + ".anh.gz"))
            P = postproc.Post(r["kw"], r["V"], "hf")
            chk = postproc.read_check(os.path.join(GOLD, "hpproc", name + ".out.check"))
        load.cache[name] = (P, chk, r)
    return load.cache[name]


load.cache = {}


def check_integrals(P, chk, out):
    """out: the seven integrals in the device's order against the recorded lines."""
    lines = chk["integrals"]
    want = [lines[0][1][0], lines[1][1][0], lines[2][1][0]] + lines[3][1] + lines[4][1]
    for k, (w, g) in enumerate(zip(want, out)):
        print("integral %d recorded %.6f got %.9g" % (k, w, g))
        assert abs(g - w) <= TOL, (k, w, g)


def check_points(P, chk, values_at):
    """values_at(x, y, smooth) -> {element: 8 values} for the candidates; every
    recorded line equals one candidate (the only one, where there is one)."""
    names = HF_NAMES if P.heat else ES_NAMES
    for smooth in (False, True):
        for x, y, rec in chk["points"][smooth]:
            cands = values_at(x, y, smooth)
            assert cands, (x, y)
            errs = {k: max(abs(v[names[n]] - rec[n]) for n in rec) for k, v in cands.items()}
            best = min(errs, key=errs.get)
            print("point (%g, %g) smooth %d: containing %s, matches element %d (err %.3g)"
                  % (x, y, smooth, sorted(cands), best, errs[best]))
            assert errs[best] <= TOL, (x, y, smooth, errs)


@pytest.mark.parametrize("name", ["test", "Temp0", "Temp1"])
def test_restatement_reproduces_recorded_output(name):
    P, chk, r = load(name)
    assert np.array_equal(P.Q, r["Q"])   # the Q marks of the descriptor are the file's
    out, _ = P.block_integrals([0])
    check_integrals(P, chk, out)

    def values_at(x, y, smooth):
        return {k: P.point_values(x, y, k, smooth) for k in P.containing(x, y)}

    check_points(P, chk, values_at)


def test_fixture_points_single_and_shared():
    """The electrostatic points and (0.005, 0.005) lie in one element each; the
    heat-flow node (0.01, 0.01) in five, of two materials."""
    P, _, _ = load("test")
    assert len(P.containing(0.25, 0.0)) == 1 and len(P.containing(0.1, 0.8)) == 1
    H, _, _ = load("Temp0")
    assert len(H.containing(0.005, 0.005)) == 1
    hits = H.containing(0.01, 0.01)
    assert len(hits) == 5 and len({H.blk[k] for k in hits}) == 2


def test_synthetic_meshes_take_every_branch():
    """The synthetic set of the device tests exercises every case of the
    smoothing: the fit and each of the five punts (the device tests compare
    the device's case per corner with the restatement's)."""
    seen = set()
    for nx, ny, axi, physics in postproc.SYNTH:
        kw, V = postproc.synthetic(nx, ny, axi, physics)
        seen |= set(np.unique(np.array(postproc.Post(kw, V, physics).branch)).tolist())
    assert {0, 1, 2, 3, 4, 5} <= seen, seen
