"""Address arithmetic of the SpGEMM slab layout (xfk_amg_spgemm.hip: k_spgemm_sort,
k_spgemm_compact_slab), replayed in numpy without a GPU.

A k_spgemm_sort wavefront handles W = 64 / G consecutive rows of at most CAP
entries and writes them back to back from blockIdx.x * W * CAP, each row at the
exclusive prefix of the W row lengths (an inclusive Hillis-Steele scan over
the 64 lanes in steps of G, every lane of a group holding its row's length).
k_spgemm_compact_slab moves slab b as one run of slab_n[b] entries to
crow[b * W].  Shown here for random length vectors -- lengths 0 and CAP and a
row count that is no multiple of W among them: every write stays inside its
slab and the allocation (nrows * CAP), the slab copies tile [0, nnz) exactly
once, and the CSR that comes out is the one of the per-row layout.
"""
import numpy as np
import pytest

# (G, CAP) of the k_spgemm_sort instances (spgemm<>'s launch_sort)
INSTANCES = [(4, 16), (8, 32), (8, 64), (16, 128), (32, 256)]


def wave_prefix(cnt_lane, G):
    """The kernel's scan on one wavefront: cnt_lane[i] is lane i's row length."""
    upto = cnt_lane.copy()
    off = G
    while off < 64:
        t = np.concatenate([upto[:off], upto[:-off]])      # __shfl_up(upto, off, 64)
        upto = np.where(np.arange(64) >= off, upto + t, upto)
        off <<= 1
    return upto


def lengths(rng, nrows, cap, kind):
    if kind == "random":
        c = rng.integers(0, cap + 1, nrows)
    elif kind == "short":            # level-0 rows: a few entries of 16+ slots
        c = rng.integers(0, 6, nrows)
    elif kind == "full":             # every row clamped to CAP (the overflow path)
        c = np.full(nrows, cap)
    elif kind == "empty":
        c = np.zeros(nrows, np.int64)
    else:                            # zeros and CAPs side by side
        c = rng.choice([0, cap], nrows)
    return c.astype(np.int64)


@pytest.mark.parametrize("G,CAP", INSTANCES)
@pytest.mark.parametrize("kind", ["random", "short", "full", "empty", "edges"])
def test_slab_addresses_tile_the_csr(G, CAP, kind):
    W = 64 // G
    rng = np.random.default_rng(1000 * G + CAP + len(kind))
    for nrows in (1, W - 1, W, W + 1, 5 * W + W // 2 + 1, 37 * W - 1, 64 * W):
        if nrows < 1:
            continue
        cnt = lengths(rng, nrows, CAP, kind)
        nslab = (nrows + W - 1) // W
        crow = np.concatenate([[0], np.cumsum(cnt)])
        nnz = int(crow[-1])
        pad = -np.ones(nrows * CAP, np.int64)              # pad_col / pad_val: nrows * CAP slots
        slab_n = np.zeros(nslab, np.int64)
        for b in range(nslab):
            live = np.arange(b * W, (b + 1) * W) < nrows
            c = np.where(live, cnt[np.minimum(np.arange(b * W, (b + 1) * W), nrows - 1)], 0)   # dead rows count 0
            upto = wave_prefix(np.repeat(c, G), G)
            assert np.array_equal(upto[::G], np.cumsum(c))  # every group holds its inclusive prefix
            slab_n[b] = upto[63]
            for g in range(W):
                row = b * W + g
                if row >= nrows:
                    continue
                base = b * W * CAP + upto[g * G] - c[g]
                assert b * W * CAP <= base and base + c[g] <= min((b + 1) * W * CAP, nrows * CAP)
                assert (pad[base:base + c[g]] == -1).all()  # no slot written twice
                pad[base:base + c[g]] = row * CAP + np.arange(c[g])   # tag: (row, rank)
            assert slab_n[b] == crow[min((b + 1) * W, nrows)] - crow[b * W]
        out = -np.ones(nnz, np.int64)
        for b in range(nslab):
            d, n, src = int(crow[b * W]), int(slab_n[b]), b * W * CAP
            assert 0 <= d and d + n <= nnz and n <= W * CAP and src + n <= nrows * CAP
            assert (out[d:d + n] == -1).all()               # the copies do not overlap
            out[d:d + n] = pad[src:src + n]
        ref = np.concatenate([r * CAP + np.arange(cnt[r]) for r in range(nrows)]) if nnz else np.zeros(0, np.int64)
        assert np.array_equal(out, ref)                     # [0, nnz) covered once, rows and ranks in CSR order
