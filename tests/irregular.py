"""Irregular test meshes for the symbolic phase and the row-gather assembly.

The meshes the rest of the suite solves have 4-8 triangles at a node and rows
of at most 9 entries, so every branch of the device's symbolic phase that is
keyed on a node's valence or a row's length is taken on one side only.  The
builders here make meshes on which both sides are taken: a *wheel* is a hub
node with k incident triangles and concentric rings of k nodes around it
(every annular quad split in two), so the hub's node list has k elements and
its matrix row k + 1 entries while every other node has at most 6 elements.

    wheel(k, rings)                 one wheel, its outer ring fixed at A = 0
    islands(ks, rings, ...)         one wheel per entry of ks, disconnected,
                                    in one mesh; numbering options below
    glued_halves(ks, rings, anti)   every wheel cut along a diameter into two
                                    half-disc islands, the diameter's nodes
                                    duplicated and joined again by periodic or
                                    antiperiodic pairs (the hub's copies too)

Plain numpy, no mesher.  Every mesh is conforming, counter-clockwise and of
positive area: `check_mesh` asserts it, and every builder calls it.

Materials (the blocks of synth.magnetostatic: air, linear or M-19 steel, +J and
-J coils, a magnet) go by annulus and angle so that every hub, and every hub
copy of a cut wheel, touches air and steel.

Numberings (`numbering=`): "natural" (hub first in its island), "hub_last",
"permuted" (seeded random permutations of the nodes and, separately, of the
elements: the arrival order of a node's elements then differs from ascending
order), "half" (a square_mesh island pads the mesh past 8192 nodes, the first
half of nodes and elements stays in order, the rest is permuted, and three
early 256-element tiles get a node span of exactly kN2eWin - 1, kN2eWin and
kN2eWin + 1 by a swap of two node numbers each)."""
from __future__ import annotations

import copy

import numpy as np

from xfemm_amd import synth

SWEEP = tuple(range(3, 21)) + (31, 32, 33, 63, 64, 65, 127, 128, 129)
GLUED_SWEEP = tuple(range(4, 41, 2))
HARMONIC_HUBS = (63, 64, 65, 100, 119)
SPACING = 2.5      # cm between island centres (radius 1 cm)
N2E_TILE = 256     # elements per k_n2e_tile workgroup


def check_mesh(x, y, p, used=True):
    """Positive areas (counter-clockwise), every edge in at most two triangles
    and at most once per direction (conforming, consistently oriented), every
    node used."""
    p = np.asarray(p)
    x, y = np.asarray(x), np.asarray(y)
    a2 = (x[p[:, 1]] - x[p[:, 0]]) * (y[p[:, 2]] - y[p[:, 0]]) - (x[p[:, 2]] - x[p[:, 0]]) * (y[p[:, 1]] - y[p[:, 0]])
    assert (a2 > 0).all(), "a triangle of non-positive area"
    n = len(x)
    a = p.reshape(-1).astype(np.int64)
    b = p[:, [1, 2, 0]].reshape(-1).astype(np.int64)
    assert (a != b).all()
    d, cd = np.unique(a * n + b, return_counts=True)
    assert (cd == 1).all(), "an edge used twice in one direction"
    u, cu = np.unique(np.minimum(a, b) * n + np.maximum(a, b), return_counts=True)
    assert (cu <= 2).all(), "an edge shared by more than two triangles"
    if used:
        assert len(np.unique(p)) == n and p.min() == 0 and p.max() == n - 1, "an unused node"
    return 0.5 * a2


def valence(p, n):
    """Incident elements per node."""
    return np.bincount(np.asarray(p).reshape(-1), minlength=n)


def element_pattern(p, n):
    """The CSR pattern of the element graph: per row the sorted unique union
    of the vertices of its incident elements and the row itself."""
    p = np.asarray(p, np.int64)
    r = np.concatenate([np.repeat(p, 3, axis=1).reshape(-1), np.arange(n)])
    c = np.concatenate([np.tile(p, (1, 3)).reshape(-1), np.arange(n)])
    key = np.unique(r * n + c)
    rows, cols = key // n, key % n
    rowptr = np.zeros(n + 1, np.int64)
    np.add.at(rowptr, rows + 1, 1)
    return np.cumsum(rowptr), cols


def _sector(k, rings, i0, i1, R=1.0):
    """Sectors i0 <= i < i1 of the k-wheel (all of it when i1 - i0 == k): nodes
    (hub first, then ring by ring), triangles (hub fan first, then annulus by
    annulus), per triangle its sector and annulus, the boundary-tagged edges,
    and per node (ring, angular index mod k)."""
    full = i1 - i0 == k
    na = k if full else i1 - i0 + 1

    def nid(j, a):
        return 1 + (j - 1) * na + ((a - i0) % k if full else a - i0)

    xs, ys, who = [0.0], [0.0], [(0, 0)]
    for j in range(1, rings + 1):
        for t in range(na):
            th = 2.0 * np.pi * ((i0 + t) % k) / k
            xs.append(R * j / rings * np.cos(th))
            ys.append(R * j / rings * np.sin(th))
            who.append((j, (i0 + t) % k))
    p, sec, ann, e = [], [], [], []
    for i in range(i0, i1):
        p.append((0, nid(1, i), nid(1, i + 1)))
        sec.append(i % k)
        ann.append(0)
        e.append((-1, 0 if rings == 1 else -1, -1))
    for j in range(1, rings):
        for i in range(i0, i1):
            a0, a1, b0, b1 = nid(j, i), nid(j, i + 1), nid(j + 1, i), nid(j + 1, i + 1)
            p += [(a0, b0, b1), (a0, b1, a1)]
            sec += [i % k, i % k]
            ann += [j, j]
            e += [(-1, 0 if j == rings - 1 else -1, -1), (-1, -1, -1)]
    return (np.array(xs), np.array(ys), np.array(p, np.int32), np.array(sec), np.array(ann),
            np.array(e, np.int32), who)


def _labels(k, rings, sec, ann, flip=False):
    """Block label per triangle by annulus and angle fraction f.  flip: every
    source negated (the coils swapped, the magnet turned: label 5)."""
    f = (sec + 0.5) / k
    lbl = np.zeros(len(sec), np.int32)
    lbl[(ann == 0) & (f >= 0.25) & (f < 0.75)] = 1                  # steel round half the hub
    lbl[(ann == 1) & (f < 0.25)] = 3 if flip else 2                 # coil +J
    lbl[(ann == 1) & (f >= 0.5) & (f < 0.75)] = 2 if flip else 3    # coil -J
    mag_ann = 1 if rings == 2 else 2
    lbl[(ann == mag_ann) & (f >= 0.375) & (f < 0.625)] = 5 if flip else 4    # (astride the cut)
    return lbl


def _problem(x, y, p, lbl, e, nonlinear, pbc=None, precision=1e-8):
    base = synth.magnetostatic(1, nonlinear=nonlinear, precision=precision)
    labels = [dict(lb) for lb in base["labels"]] + [dict(block=4, mag_dir=270.0)]
    return dict(base, x=np.asarray(x, float), y=np.asarray(y, float), p=np.asarray(p, np.int32),
                lbl=np.asarray(lbl, np.int32), e=np.asarray(e, np.int32), labels=labels,
                pbc=None if pbc is None or not len(pbc) else np.asarray(pbc, np.int32))


def wheel(k, rings, nonlinear=False):
    """One k-wheel: kwargs of kernels.Static2DProblem (synth's form), the hub
    node 0, the outermost ring's edges tagged with boundary property 0 (A = 0)."""
    x, y, p, sec, ann, e, _ = _sector(k, rings, 0, k)
    check_mesh(x, y, p)
    kw = _problem(x, y, p, _labels(k, rings, sec, ann), e, nonlinear)
    kw["hubs"] = np.array([0])
    return kw


AXI_R = 1.2        # cm: radius of the hubs of the axisymmetric variant


def _centre(m, axisymmetric=False):
    """Planar: a grid of eight columns.  Axisymmetric: one column along z at
    r = AXI_R, every wheel within 0.2 <= r <= 2.2 cm: the reference's mean
    radius of an element, -q0 q1 q2 / (2 sum_j q_j r_j log r_j), cancels the
    more the further out a small element lies (lost digits ~ (r / q)^2) and
    the closer one of its edges comes to the z direction without lying along
    it (an even wheel's diagonals come within 4e-5 unless the wheel is turned
    by half a sector, as islands() does), and what that costs the f64 sum is the reference's, not the symbolic phase's
    (log_mean_radius_condition, tests/test_irregular_cpu.py)."""
    if axisymmetric:
        return AXI_R, SPACING * m
    return SPACING * (m % 8), SPACING * (m // 8)


def renumber(kw, node_perm=None, elem_order=None):
    """The same mesh with node i renamed node_perm[i] and the elements listed
    in elem_order.  `hubs`, `orig` (node -> node of the mesh first built) and
    the periodic pairs follow."""
    kw = dict(kw)
    n = len(kw["x"])
    if node_perm is not None:
        node_perm = np.asarray(node_perm)
        assert np.array_equal(np.sort(node_perm), np.arange(n))
        inv = np.argsort(node_perm)
        kw["x"], kw["y"] = kw["x"][inv], kw["y"][inv]
        kw["p"] = node_perm[kw["p"]].astype(np.int32)
        kw["hubs"] = node_perm[kw["hubs"]]
        kw["orig"] = kw.get("orig", np.arange(n))[inv]
        if kw.get("sign") is not None:
            kw["sign"] = kw["sign"][inv]
        if kw.get("pbc") is not None:
            pbc = kw["pbc"].copy()
            pbc[:, :2] = node_perm[pbc[:, :2]]
            kw["pbc"] = pbc
    if elem_order is not None:
        elem_order = np.asarray(elem_order)
        kw["p"], kw["lbl"], kw["e"] = kw["p"][elem_order], kw["lbl"][elem_order], kw["e"][elem_order]
    return kw


def _join(parts, nonlinear, axisymmetric, precision=1e-8):
    xs, ys, ps, ls, es, hubs, pbcs, off = [], [], [], [], [], [], [], 0
    for x, y, p, lbl, e, hub, pbc in parts:
        xs.append(x)
        ys.append(y)
        ps.append(p + off)
        ls.append(lbl)
        es.append(e)
        hubs += [h + off for h in hub]
        if len(pbc):
            q = np.asarray(pbc, np.int32).copy()
            q[:, :2] += off
            pbcs.append(q)
        off += len(x)
    kw = _problem(np.concatenate(xs), np.concatenate(ys), np.concatenate(ps), np.concatenate(ls),
                  np.concatenate(es), nonlinear, np.concatenate(pbcs) if pbcs else None, precision)
    kw["hubs"] = np.array(hubs)
    if axisymmetric:
        kw["problem_type"] = 1
    return kw


def _tile_spans(p):
    p = np.asarray(p)
    nt = (len(p) + N2E_TILE - 1) // N2E_TILE
    return np.array([p[t * N2E_TILE:(t + 1) * N2E_TILE].max() - p[t * N2E_TILE:(t + 1) * N2E_TILE].min()
                     for t in range(nt)])


def _half_scramble(kw, seed, win):
    """First half of the nodes and of the elements in order, the rest permuted;
    then tiles 0, 4, 8 are given node spans win - 1, win, win + 1: in each,
    the number of one node that is not the tile's smallest is swapped with the
    number lo + span (a node far outside the narrow tile)."""
    rng = np.random.default_rng(seed)
    n, ne = len(kw["x"]), len(kw["p"])
    perm = np.arange(n)
    perm[n // 2:] = n // 2 + rng.permutation(n - n // 2)
    order = np.arange(ne)
    order[ne // 2:] = ne // 2 + rng.permutation(ne - ne // 2)
    kw = renumber(kw, perm, order)
    for t, span in zip((0, 4, 8), (win - 1, win, win + 1)):     # (tiles four apart share no node)
        tile = kw["p"][t * N2E_TILE:(t + 1) * N2E_TILE]
        lo, hi = int(tile.min()), int(tile.max())
        assert hi - lo < win // 4 and lo + span < n
        swap = np.arange(n)
        swap[hi], swap[lo + span] = lo + span, hi
        kw = renumber(kw, swap)
    return kw


def islands(ks=SWEEP, rings=3, numbering="natural", nonlinear=False, axisymmetric=False, seed=11, win=4096,
            pad_to=11000):
    """One wheel per entry of ks side by side, disconnected, each with its own
    fixed outer ring.  axisymmetric: the same islands shifted to r > 0, in one
    column along z (_centre).
    Returns synth-style kwargs plus `hubs` (node of each hub) and, for the
    renumbered forms, `orig` (node -> node of the natural numbering)."""
    parts = []
    r0 = AXI_R if axisymmetric else 0.0
    for m, k in enumerate(ks):
        x, y, p, sec, ann, e, _ = _sector(k, rings, 0, k)
        cx, cy = _centre(m, axisymmetric)
        if axisymmetric:   # turned by half a sector: no edge within 1e-3 of the z direction (see _centre)
            a = np.pi / k
            x, y = np.cos(a) * x - np.sin(a) * y, np.sin(a) * x + np.cos(a) * y
        parts.append((x + cx, y + cy, p, _labels(k, rings, sec, ann), e, [0], []))
    if numbering == "half":
        n0 = sum(len(q[0]) for q in parts)
        cells = int(np.ceil(np.sqrt(max(pad_to - n0, 4)))) - 1
        sq = synth.magnetostatic(cells, nonlinear=nonlinear)
        # the pad goes first: its banded numbering makes the narrow tiles
        parts.insert(0, (sq["x"] + r0, sq["y"] - 12.0, sq["p"], sq["lbl"], sq["e"], [], []))
    kw = _join(parts, nonlinear, axisymmetric)
    check_mesh(kw["x"], kw["y"], kw["p"])
    n, ne = len(kw["x"]), len(kw["p"])
    if numbering == "natural":
        kw["orig"] = np.arange(n)
    elif numbering == "hub_last":
        # within each island: the hub takes the island's last number
        perm = np.arange(n)
        for h, h1 in zip(kw["hubs"], list(kw["hubs"][1:]) + [n]):
            perm[h + 1:h1] -= 1
            perm[h] = h1 - 1
        kw = renumber(kw, perm)
    elif numbering == "permuted":
        rng = np.random.default_rng(seed)
        kw = renumber(kw, rng.permutation(n), rng.permutation(ne))
    elif numbering == "half":
        assert n > 8192
        kw = _half_scramble(kw, seed, win)
    else:
        raise ValueError(numbering)
    check_mesh(kw["x"], kw["y"], kw["p"])
    return kw


FAN_SWEEP = (6, 7, 8, 14, 15, 16, 17)


def fans(ks=FAN_SWEEP, rings=3, numbering="natural", seed=7):
    """Open fans: the upper half of the 2k-wheel for every k of ks, the hub on
    the straight (free) side with k incident triangles, the arc fixed.  Round
    a closed hub every ring node sits in two hub triangles, so a row build that
    loses one triangle still finds every column; at the two ends of an open
    fan a node sits in one triangle only."""
    parts = []
    for m, k in enumerate(ks):
        x, y, p, sec, ann, e, _ = _sector(2 * k, rings, 0, k)
        cx, cy = _centre(m)
        parts.append((x + cx, y + cy, p, _labels(2 * k, rings, sec, ann), e, [0], []))
    kw = _join(parts, False, False)
    kw["orig"] = np.arange(len(kw["x"]))
    if numbering == "permuted":
        rng = np.random.default_rng(seed)
        kw = renumber(kw, rng.permutation(len(kw["x"])), rng.permutation(len(kw["p"])))
    elif numbering != "natural":
        raise ValueError(numbering)
    check_mesh(kw["x"], kw["y"], kw["p"])
    return kw


def glued_halves(ks=GLUED_SWEEP, rings=3, anti=False, numbering="natural", seed=5):
    """Every k-wheel (k even) cut along the diameter through the angular
    positions 0 and k / 2 into two half-disc islands; the diameter's free
    nodes -- the hub and the inner rings' two nodes -- exist twice and are
    joined by periodic pairs (antiperiodic with anti, the lower half's sources
    then negated, so that its solution is minus the uncut wheel's).  Each hub
    copy is a periodic row with k / 2 incident elements plus fill-in.
    `orig`: node -> node of islands(ks, rings) (natural numbering), `sign`:
    +1, or -1 on the lower halves of the antiperiodic form, so that the
    solution is sign * A_uncut[orig]."""
    if np.isscalar(ks):
        ks = (ks,)
    parts, orig, sign, off_uncut = [], [], [], 0
    for m, k in enumerate(ks):
        assert k % 2 == 0 and k >= 4
        cx, cy = _centre(m)
        up = _sector(k, rings, 0, k // 2)
        lo = _sector(k, rings, k // 2, k)
        ids = [{w: i for i, w in enumerate(h[6])} for h in (up, lo)]
        pbc = [(ids[0][w], len(up[0]) + ids[1][w], 1 if anti else 0)
               for w in up[6] if w in ids[1] and w[0] < rings]
        assert len(pbc) == 1 + 2 * (rings - 1)
        x = np.concatenate([up[0], lo[0]]) + cx
        y = np.concatenate([up[1], lo[1] - 0.125]) + cy          # (the halves pulled apart: two islands)
        p = np.concatenate([up[2], lo[2] + len(up[0])])
        lbl = np.concatenate([_labels(k, rings, up[3], up[4]), _labels(k, rings, lo[3], lo[4], flip=anti)])
        parts.append((x, y, p, lbl, np.concatenate([up[5], lo[5]]), [0, len(up[0])], pbc))
        for h, s in ((up, 1.0), (lo, -1.0 if anti else 1.0)):
            for j, a in h[6]:
                orig.append(off_uncut + (0 if j == 0 else 1 + (j - 1) * k + a))
                sign.append(s)
        off_uncut += 1 + rings * k
    kw = _join(parts, False, False)
    kw["orig"], kw["sign"] = np.array(orig), np.array(sign)
    check_mesh(kw["x"], kw["y"], kw["p"])
    if numbering == "permuted":
        rng = np.random.default_rng(seed)
        kw = renumber(kw, rng.permutation(len(kw["x"])), rng.permutation(len(kw["p"])))
        check_mesh(kw["x"], kw["y"], kw["p"])
    elif numbering != "natural":
        raise ValueError(numbering)
    return kw


def solver_kwargs(kw):
    """The builder's kwargs without its bookkeeping (what synth_to_oracle and
    the problem classes take)."""
    return {k: v for k, v in kw.items() if k not in ("hubs", "orig", "sign")}


def harmonic(ks, rings=2, numbering="permuted", seed=11):
    """The wheels of ks as a time-harmonic planar problem: the material,
    boundary and circuit tables of synth.harmonic (lossy laminated steel, a
    wound coil circuit, a voltage-driven conducting plate) on the islands'
    labels -- label 4, the islands' magnet, is the conducting plate there --
    the outer rings at synth.harmonic's prescribed A with a phase."""
    kw = islands(ks, rings, numbering=numbering, seed=seed)
    h = synth.harmonic(2)
    lbl = kw["lbl"].copy()
    lbl[lbl == 5] = 4
    out = dict(kw, lbl=lbl)
    for key in ("blocks", "labels", "lines", "circuits", "frequency", "precision"):
        out[key] = copy.deepcopy(h[key])
    out["points"], out["marker"] = [], None
    return out


def log_mean_radius_condition(kw):
    """Per element of an axisymmetric mesh that takes the general branch of
    the reference's logarithmic mean radius (no vertex on the axis, no edge
    along z): sum_j |q_j r_j log r_j| / |sum_j q_j r_j log r_j|, the factor by
    which a rounding error of one term grows in the sum."""
    rn = np.asarray(kw["x"])[kw["p"]]
    q = np.stack([rn[:, 2] - rn[:, 1], rn[:, 0] - rn[:, 2], rn[:, 1] - rn[:, 0]], 1)
    gen = (np.abs(q) >= 1e-6).all(axis=1) & (rn >= 1e-6).all(axis=1)
    t = (q * rn * np.log(rn))[gen]
    return np.abs(t).sum(axis=1) / np.abs(t.sum(axis=1))


# ---- coverage bookkeeping (tests/test_irregular_cpu.py) ----------------------

def row_lengths(kw):
    rp, _ = element_pattern(kw["p"], len(kw["x"]))
    return np.diff(rp)


def row_blocks(lengths, acc, block=128):
    """Per block of `block` consecutive rows: (has a row longer than acc, has
    a row of at most acc)."""
    out = []
    for s in range(0, len(lengths), block):
        L = lengths[s:s + block]
        out.append(((L > acc).any(), (L <= acc).any()))
    return out
