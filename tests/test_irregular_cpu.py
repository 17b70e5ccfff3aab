"""The irregular test meshes (tests/irregular.py) on the CPU: the builder's
invariants, the claim that the meshes of tests/test_gpu_irregular.py straddle
every valence / row-length threshold of the device's symbolic phase and
row-gather assembly (the thresholds are read from the sources, so a retuned
constant fails here instead of the coverage silently moving off its edge), and
one property that does not involve the device: a wheel cut in two and glued
again by periodic pairs has the uncut wheel's solution."""
import os
import re

import numpy as np
import pytest

import irregular as ir
from oracle import oracle
from util import ROOT, converged, rel_err, synth_to_oracle

CSRC = os.path.join(ROOT, "xfemm_amd", "csrc")

# what the sweeps of irregular.py were laid out for: (file, regex, value)
CONSTANTS = {
    "sort16": ("xfk_device.hip", r"sort_node_list\(.*?if \(len <= (\d+)\) \{", 16),
    "regs16": ("xfk_device.hip", r"rowcnt\[v\] = ne <= (\d+) \?", 7),
    "kRowRegElems": ("xfk_device.hip", r"constexpr int kRowRegElems = (\d+);", 15),
    "kRowLds": ("xfk_device.hip", r"constexpr int kRowLds = (\d+);", 32),
    "kRowAcc": ("xfk_device.hip", r"constexpr int kRowAcc = (\d+);", 12),
    "kRowBlock": ("xfk_device.hip", r"constexpr int kRowBlock = (\d+);", 128),
    "kN2eWin": ("xfk_device.hip", r"constexpr int kN2eWin = (\d+);", 4096),
    "kPotRowAcc": ("xfk_potential.h", r"constexpr int kPotRowAcc = (\d+);", 12),
    "kMaxColors": ("xfk_api.hip", r"static constexpr int kMaxColors = (\d+);", 128),
}


def constant(name):
    fn, rx, _ = CONSTANTS[name]
    m = re.search(rx, open(os.path.join(CSRC, fn)).read(), re.S)
    assert m, "%s: %r no longer matches %s" % (name, rx, fn)
    return int(m.group(1))


@pytest.fixture(scope="module")
def sweep():
    return {nb: ir.islands(numbering=nb) for nb in ("natural", "hub_last", "permuted", "half")}


@pytest.fixture(scope="module")
def glued():
    """The glued sweep and the oracle's assembled pattern of it."""
    kw = ir.glued_halves()
    pr, mesh, _ = synth_to_oracle(ir.solver_kwargs(kw))
    O, _ = oracle.system(pr, mesh)
    return kw, pr, mesh, O


# ---- the builder -------------------------------------------------------------

@pytest.mark.parametrize("k,rings", [(3, 1), (3, 2), (4, 3), (17, 2), (129, 3)])
def test_wheel_invariants(k, rings):
    kw = ir.wheel(k, rings)
    area = ir.check_mesh(kw["x"], kw["y"], kw["p"])
    n = len(kw["x"])
    assert n == 1 + k * rings and len(kw["p"]) == k * (2 * rings - 1)
    val = ir.valence(kw["p"], n)
    assert val[0] == k and (val[1:] <= 6).all() and (val > 0).all()
    # the rings are regular k-gons of radius j / rings: the area is theirs
    assert abs(area.sum() - 0.5 * k * np.sin(2 * np.pi / k)) <= 1e-12
    # exactly the outermost ring's k edges carry the boundary property
    assert (kw["e"] >= 0).sum() == k
    tagged = np.unique(np.concatenate([kw["p"][:, j][kw["e"][:, j] >= 0] for j in range(3)]
                                      + [kw["p"][:, (j + 1) % 3][kw["e"][:, j] >= 0] for j in range(3)]))
    assert np.array_equal(tagged, np.arange(n - k, n))
    assert len(np.unique(kw["lbl"][np.any(kw["p"] == 0, axis=1)])) >= 2      # two materials at the hub


def test_islands_invariants(sweep):
    nat = sweep["natural"]
    n = len(nat["x"])
    assert (n, len(nat["p"])) == (2664, 4395)          # 27 wheels of 3 rings
    a0 = np.sort(ir.check_mesh(nat["x"], nat["y"], nat["p"]))
    for nb, kw in sweep.items():
        val = ir.valence(kw["p"], len(kw["x"]))
        assert (val > 0).all()
        assert np.array_equal(val[kw["hubs"]], ir.SWEEP), nb
        hub_elems = [kw["lbl"][np.any(kw["p"] == h, axis=1)] for h in kw["hubs"]]
        assert all(len(np.unique(l)) >= 2 for l in hub_elems), nb
        if nb == "half":
            continue
        # a renumbering moves nothing: node for node the same coordinates, the
        # same multiset of triangles with the same labels and edge tags
        assert np.array_equal(kw["x"], nat["x"][kw["orig"]]) and np.array_equal(kw["y"], nat["y"][kw["orig"]])
        assert np.array_equal(np.sort(ir.check_mesh(kw["x"], kw["y"], kw["p"])), a0)

        def canon(q):
            tri = np.concatenate([q["orig"][q["p"]] if "orig" in q else q["p"], q["lbl"][:, None], q["e"]], axis=1)
            r = np.argmin(tri[:, :3], axis=1)            # rotate the smallest vertex first, edges with it
            rot = np.array([[0, 1, 2], [1, 2, 0], [2, 0, 1]])[r]
            tri = np.concatenate([np.take_along_axis(tri[:, :3], rot, 1), tri[:, 3:4],
                                  np.take_along_axis(tri[:, 4:], rot, 1)], axis=1)
            return tri[np.lexsort(tri.T[::-1])]
        assert np.array_equal(canon(kw), canon(nat)), nb
    hl = sweep["hub_last"]
    ends = list(nat["hubs"][1:] - 1) + [n - 1]
    assert np.array_equal(hl["hubs"], ends)
    # the permuted form has work for the per-node sort: some node's elements do not arrive ascending
    assert not np.array_equal(sweep["permuted"]["p"], nat["p"])


def test_axisymmetric_islands_are_off_the_axis():
    kw = ir.islands(ks=(5, 17, 33), rings=2, axisymmetric=True, numbering="permuted")
    assert kw["problem_type"] == 1 and kw["x"].min() >= 0.2 - 1e-12
    assert np.array_equal(ir.valence(kw["p"], len(kw["x"]))[kw["hubs"]], (5, 17, 33))


def test_axisymmetric_sweep_keeps_the_mean_radius_well_conditioned():
    """The reference's logarithmic mean radius is a cancelling sum; what two
    correct f64 evaluations of it may differ by (a log one bit apart, a fused
    multiply-add) is cond x a few 2^-52, relative, on that element's axial
    stiffness.  For the assembled system to be comparable at 1e-12 of max |A|
    the sweep must keep cond <= 1e-12 / (8 x 2^-52) = 5.6e5; 1e5 is asserted,
    a factor 5 in hand.  In one column at r = 1.2 cm, each wheel turned by half
    a sector, it has cond <= 2.9e4; unturned 2e6 (an even wheel's diagonal 4e-5
    off the z direction); on the planar grid's positions (r up to 20 cm) 3e8."""
    kw = ir.islands(numbering="permuted", axisymmetric=True)
    assert kw["x"].min() > 0.19 and kw["x"].max() < 2.21
    assert np.array_equal(ir.valence(kw["p"], len(kw["x"]))[kw["hubs"]], ir.SWEEP)
    cond = ir.log_mean_radius_condition(kw)
    print("log-mean-radius condition: max %.3e over %d elements" % (cond.max(), len(cond)))
    assert len(cond) > 4000 and cond.max() <= 1e5


def test_open_fans_straddle_the_register_row_build():
    """Hubs on a free straight side with 6-8 and 14-17 triangles: both widths
    of the register network and its limit, at nodes whose end neighbours sit
    in one hub triangle only."""
    for nb in ("natural", "permuted"):
        kw = ir.fans(numbering=nb)
        val = ir.valence(kw["p"], len(kw["x"]))
        assert np.array_equal(val[kw["hubs"]], ir.FAN_SWEEP)
        for name in ("regs16", "kRowRegElems", "sort16"):
            c = constant(name)
            assert {c - 1, c, c + 1} <= set(ir.FAN_SWEEP) or name == "sort16" and {c, c + 1} <= set(ir.FAN_SWEEP)
        rows = ir.row_lengths(kw)
        assert np.array_equal(rows[kw["hubs"]], np.array(ir.FAN_SWEEP) + 2)      # k + 1 ring nodes and the hub
        # the fan's two end nodes are in exactly one of the hub's triangles
        for h in kw["hubs"]:
            tri = kw["p"][np.any(kw["p"] == h, axis=1)]
            cnt = np.bincount(tri.reshape(-1))
            assert (cnt[cnt > 0] == 1).sum() == 2


def test_glued_halves_invariants(glued):
    kw = glued[0]
    n = len(kw["x"])
    val = ir.valence(kw["p"], n)
    assert np.array_equal(val[kw["hubs"]], np.repeat(ir.GLUED_SWEEP, 2) // 2)
    pbc = kw["pbc"]
    assert len(pbc) == 5 * len(ir.GLUED_SWEEP) and (pbc[:, 2] == 0).all()
    # a pair joins two copies of one node of the uncut wheel; the hub copies are pairs
    assert np.array_equal(kw["orig"][pbc[:, 0]], kw["orig"][pbc[:, 1]])
    assert set(map(tuple, kw["hubs"].reshape(-1, 2))) <= set(map(tuple, pbc[:, :2]))
    un = ir.islands(ir.GLUED_SWEEP, 3)
    # both halves together are the uncut wheels: the same triangles through `orig`
    t_g = np.sort(np.sort(kw["orig"][kw["p"]], axis=1).view("i8,i8,i8").ravel())
    t_u = np.sort(np.sort(un["p"].astype(np.int64), axis=1).view("i8,i8,i8").ravel())
    assert np.array_equal(t_g, t_u)
    anti = ir.glued_halves(anti=True)
    assert (anti["pbc"][:, 2] == 1).all() and set(np.unique(anti["sign"])) == {-1.0, 1.0}
    assert (anti["lbl"] == 5).any() and not (kw["lbl"] == 5).any()


# ---- the coverage claim ------------------------------------------------------

def test_constants_are_the_ones_the_sweeps_were_laid_out_for():
    """A retuned threshold: re-derive irregular.SWEEP / GLUED_SWEEP /
    HARMONIC_HUBS so that they straddle the new value, then change it here."""
    for name, (_, _, value) in CONSTANTS.items():
        assert constant(name) == value, name


def test_sweep_straddles_every_threshold(sweep):
    for nb, kw in sweep.items():
        n = len(kw["x"])
        val = set(ir.valence(kw["p"], n).tolist())
        rows = ir.row_lengths(kw)
        for name in ("sort16", "regs16", "kRowRegElems", "kMaxColors"):     # governed by incident elements
            c = constant(name)
            assert {c - 1, c, c + 1} <= val, (nb, name)
        for name in ("kRowAcc", "kPotRowAcc"):                              # governed by the row length
            c = constant(name)
            assert {c - 1, c, c + 1} <= set(rows.tolist()), (nb, name)
        assert rows.max() == 130
        # non-periodic rows past the register path have more candidates than the LDS holds: the tmp path
        c = constant("kRowRegElems")
        assert 3 * (c + 1) + 1 > constant("kRowLds")
        blocks = ir.row_blocks(rows, constant("kRowAcc"), constant("kRowBlock"))
        assert any(lg and sh for lg, sh in blocks), nb      # the per-lane store
        assert any(sh and not lg for lg, sh in blocks), nb  # the block-linear store
    win = constant("kN2eWin")
    spans = ir._tile_spans(sweep["half"]["p"])
    assert len(sweep["half"]["x"]) > 8192
    assert {win - 1, win, win + 1} <= set(spans.tolist())
    assert (spans < win // 4).sum() >= 8 and (spans > win + 1).sum() >= 8
    for nb in ("natural", "permuted"):
        assert (ir._tile_spans(sweep[nb]["p"]) < win).all()


def test_harmonic_hubs_use_the_second_mask_word():
    c = constant("kMaxColors")
    assert {63, 64, 65} <= set(ir.HARMONIC_HUBS)           # k_jp_nodes: colours 64.. live in the second word
    assert max(ir.HARMONIC_HUBS) + 9 <= c                  # k - 1 hub colours + at most 9 at the two ring nodes
    assert c + 1 in ir.SWEEP


def test_glued_sweep_crosses_the_lds_candidate_limit(glued):
    """Periodic rows gather 3 ne + nf + 1 candidates, through LDS up to
    kRowLds and through tmp beyond.  nf here is a proxy taken from the
    oracle's assembled pattern, not predicted: the columns its row has beyond
    the element pattern.  The device counts its fill list (RowCands::count),
    which may repeat columns the elements already give, so its figure is this
    one or larger; the hub copies run from 10 to 82 by the proxy (k / 2 = 2 ...
    20 elements), across 32 either way."""
    kw, _, _, O = glued
    n = len(kw["x"])
    rp, _ = ir.element_pattern(kw["p"], n)
    ne = ir.valence(kw["p"], n)
    nf = np.diff(O.indptr) - np.diff(rp)
    # (the hub copies only: their rows have no fixed neighbour, whose zeroed
    # entries the oracle's export leaves out)
    assert (nf[kw["hubs"]] > 0).all()
    c = constant("kRowLds")
    hub_cand = 3 * ne[kw["hubs"]] + nf[kw["hubs"]] + 1
    print("periodic candidate counts at the hub copies:", sorted(set(hub_cand.tolist())))
    assert (hub_cand <= c).any() and (hub_cand > c).any()
    assert np.abs(hub_cand - c).min() <= 2                 # and comes within a step of it
    # and the register path's other condition: periodic rows on both sides of kRowRegElems elements
    r = constant("kRowRegElems")
    assert (ne[kw["hubs"]] <= r).any() and (ne[kw["hubs"]] > r).any()


# ---- a property of the oracle alone ------------------------------------------

@pytest.mark.parametrize("anti", [False, True], ids=["periodic", "antiperiodic"])
def test_glued_halves_solve_to_the_uncut_wheels(anti):
    """The two halves joined by (anti)periodic pairs are the uncut wheels:
    sign * A_uncut[orig].  Both sides are the oracle at Precision 1e-13
    (util.converged), each within 7e-14 of a direct solve of its own system
    (util.converged's measurement); the systems differ by the periodic rows'
    averaging only.  Bound 1e-12 of max |A|: the two stopping errors, 1.4e-13
    together, and a factor 7 for the conditioning of the steel islands.
    Measured: periodic 1.64e-13, antiperiodic 1.64e-13 of max |A| = 2.6e-3."""
    kw = ir.glued_halves(anti=anti)
    pr, mesh, _ = synth_to_oracle(ir.solver_kwargs(kw))
    Ag = converged(pr, mesh)
    pu, mu, _ = synth_to_oracle(ir.solver_kwargs(ir.islands(ir.GLUED_SWEEP, 3)))
    Au = converged(pu, mu)
    err = rel_err(Ag, kw["sign"] * Au[kw["orig"]])
    print("glued vs uncut (%s): %.3e of max |A| = %.3e" % ("anti" if anti else "periodic", err, np.abs(Au).max()))
    assert np.abs(Au).max() > 1e-4
    assert err <= 1e-12
