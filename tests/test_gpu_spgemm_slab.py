"""Dense per-wavefront slabs of the sub-wave SpGEMM (xfk_amg_spgemm.hip: k_spgemm_sort,
k_spgemm_compact_slab) against the padded rows they replace.

Only addresses differ between the two layouts: the products' CSR must come
out entry for entry the same, so everything built from it -- the hierarchy,
the PCG iteration count, the solution -- is bit-identical.  XFK_SPGEMM_SLAB is
read once per process, so every case runs in two fresh child processes (this
file as a script: one with the default, one with XFK_SPGEMM_SLAB=0) and the
two reports are compared for equality; there is no tolerance.

The cases (small meshes, amg_dense=16 so that they coarsen down to a few rows):
level-0 row counts that are no multiple of 16 and coarse levels that are no
multiple of 8, 4 or 2 (the partial last wavefront of every k_spgemm_sort
instance), coarse levels of fewer rows than one wavefront handles (tiny), the empty
P rows of a Dirichlet-heavy problem (bc_showcase), the overflow-and-rebuild
path (XFK_AMG_TEST_SMALL_HINT: rows clamped to the capacity), a nonlinear
problem (the Newton refresh reads A P's pattern) and a 2-rank sharded solve
(galerkin_dist calls the same spgemm<>).  test_capacity_classes_reached checks
that the cases together run all five (G, CAP) instances.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import threading

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = ["square49", "square75", "showcase30", "tiny", "overflow", "nonlinear", "sharded2"]
TINY = [10, 12, 14, 17, 20]   # 121 ... 441 rows: two or three levels, the last of a few rows


# ---------------------------------------------------------------- child side
def _report(P, r):
    A = P.solution()
    return dict(sha=hashlib.sha256(A.tobytes()).hexdigest(), n=int(A.size), cg_iters=int(r["cg_iters"]),
                newton_iters=int(r["newton_iters"]), amg_levels=int(r["amg_levels"]),
                op_complexity=float(r["amg_op_complexity"]).hex(), precond=int(r["precond"]))


def _single(kw, **opt):
    from xfemm_amd import kernels
    P = kernels.Static2DProblem(**kw, precond="amg", **opt)
    out = _report(P, P.solve())
    P.close()
    return out


def _levels(kw, **opt):
    """A fresh setup under XFK_AMG_DEBUG: it prints every level's rows and nnz."""
    os.environ["XFK_AMG_DEBUG"] = "1"
    try:
        _single(kw, **opt)
    finally:
        del os.environ["XFK_AMG_DEBUG"]


def _case(name):
    from xfemm_amd import kernels, synth
    kernels.forget_amg_hints()
    if name == "square49":        # 2500 rows = 16 * 156 + 4
        kw = synth.magnetostatic(49)
        out = [_single(kw, amg_dense=16), _single(kw, amg_dense=16)]   # measured, then hinted capacities
        _levels(kw, amg_dense=16)
    elif name == "square75":      # 5776 rows = 16 * 361; denser coarse levels (the larger capacities)
        kw = synth.magnetostatic(75)
        out = [_single(kw, amg_dense=16), _single(kw, amg_dense=16)]
        _levels(kw, amg_dense=16)
    elif name == "showcase30":    # 961 rows = 16 * 60 + 1, Dirichlet rows: empty P rows
        kw = synth.bc_showcase(30)
        out = [_single(kw, amg_dense=16), _single(kw, amg_dense=16)]
        _levels(kw, amg_dense=16)
    elif name == "tiny":
        out = []
        for n in TINY:
            out.append(_single(synth.magnetostatic(n), amg_dense=16))
            _levels(synth.magnetostatic(n), amg_dense=16)
    elif name == "overflow":
        kw = synth.magnetostatic(49)
        P = kernels.Static2DProblem(**kw, precond="amg", amg_dense=16)
        os.environ["XFK_AMG_TEST_SMALL_HINT"] = "1"
        try:
            out = [_report(P, P.solve())]                               # measured; stores too-small capacities
            out += [_report(P, P.solve(rebuild_symbolic=True)) for _ in range(2)]   # overflow, rebuilt
        finally:
            del os.environ["XFK_AMG_TEST_SMALL_HINT"]
        P.close()
    elif name == "nonlinear":
        out = [_single(synth.magnetostatic(49, nonlinear=True))]
    elif name == "sharded2":
        kw = synth.magnetostatic(49)
        comms = kernels.Comm.local_group(2)
        probs = [kernels.Static2DProblem(**kw, comm=comms[q], precond="amg") for q in range(2)]
        out, err = [None, None], [None, None]

        def work(q):
            try:
                out[q] = _report(probs[q], probs[q].solve())
            except Exception as ex:   # surfaced below
                err[q] = ex

        th = [threading.Thread(target=work, args=(q,)) for q in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for p in probs:
            p.close()
        for c in comms:
            c.close()
        for e in err:
            if e is not None:
                raise e
    else:
        raise ValueError(name)
    kernels.forget_amg_hints()
    return out


def _main():
    sys.path.insert(0, ROOT)
    os.environ["XFK_AMG_HINTS_PRINT"] = "1"
    res = {}
    for name in CASES:
        sys.stderr.write("[case] %s\n" % name)
        sys.stderr.flush()
        res[name] = _case(name)
    print(json.dumps(res))


# --------------------------------------------------------------- parent side
def _child(slab):
    env = dict(os.environ)
    env.pop("XFK_SPGEMM_SLAB", None)
    if not slab:
        env["XFK_SPGEMM_SLAB"] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    levels, caps, name = {}, {}, None
    for ln in r.stderr.splitlines():
        if ln.startswith("[case] "):
            name = ln.split()[1]
            levels[name], caps[name] = [], set()
        elif ln.startswith("[amg hints]"):
            caps[name] |= {int(c) for c in re.findall(r"cap\[\d+\.\d+\]=(\d+)", ln)}
        else:
            m = re.match(r"\[amg\] rank (\d+) level (\d+) n (\d+) nnz (\d+) nc (\d+)", ln)
            if m:
                levels[name].append(tuple(int(g) for g in m.groups()))
    return rep, levels, caps


@pytest.fixture(scope="module")
def runs():
    return _child(True), _child(False)


@pytest.mark.parametrize("name", CASES)
def test_slab_layout_keeps_every_bit(runs, name):
    (rep, levels, caps), (rep0, levels0, caps0) = runs
    print(name, "slab:", rep[name], levels[name], sorted(caps[name]))
    print(name, "padded:", rep0[name], levels0[name], sorted(caps0[name]))
    assert rep[name] == rep0[name]            # solution bits, iterations, levels, operator complexity
    assert levels[name] == levels0[name]      # per level: rows, nnz, coarse rows
    assert caps[name] == caps0[name]
    for one in rep[name]:
        assert one["precond"] == 1 and one["amg_levels"] >= 2   # AMG ran (no fallback), with a hierarchy
    if name == "tiny":
        assert len(levels[name]) >= len(TINY)
    if name in ("square49", "square75", "showcase30"):
        assert rep[name][0] == rep[name][1]   # hinted capacities: the same bits as measured ones
        assert len(levels[name]) >= 2
    if name == "overflow":
        assert rep[name][1] == rep[name][0] and rep[name][2] == rep[name][0]
    if name == "sharded2":
        assert rep[name][0]["sha"] == rep[name][1]["sha"]       # same gathered solution on both ranks


def test_partial_wavefronts_and_tiny_levels(runs):
    """The shapes the cases are there for: level-0 rows no multiple of 16,
    coarse levels no multiple of 8, 4 or 2, one level below 8 rows."""
    (_, levels, _), _ = runs
    n0 = [lv[0][2] for lv in (levels["square49"], levels["showcase30"])]
    assert all(n % 16 for n in n0), n0
    coarse = [t[4] for name in ("square49", "square75", "showcase30", "tiny") for t in levels[name]]
    assert any(n % 2 for n in coarse) and any(n % 4 for n in coarse) and any(n % 8 for n in coarse), coarse
    assert any(0 < n < 8 for n in coarse), coarse


def test_capacity_classes_reached(runs):
    (_, _, caps), _ = runs
    reached = set().union(*caps.values())
    print("capacity classes:", {k: sorted(v) for k, v in caps.items()})
    assert reached >= {16, 32, 64, 128, 256}, reached


if __name__ == "__main__":
    _main()
