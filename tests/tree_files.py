"""Helpers of the tests of simulation files on refined trees: the expected file image of a tree of the
oracle (oracle/go_tree.c exposes flags and values of every level), and a numpy restatement of what
gfscompare does with two files on different trees.

The image is ftt_cell_write_binary + gfs_cell_write_binary (src/ftt.c:1771-1799, src/domain.c:3176-3207):
pre-order, children n = 0 .. FTT_CELLS - 1 (bit 0 = +x half, bit 1 = -y half, bit 2 = -z half); per cell
`guint flags' = child id | 16 on every leaf, a double -1., one double per variable."""
import struct

import numpy as np

FLAG_LEAF = 16


def child_index(dim, i, j, k, n):
    """array coordinates (1-based, ghost layer at 0) of child n of the cell (i, j, k)"""
    return (2 * (i - 1) + (n & 1) + 1, 2 * (j - 1) + 1 - ((n >> 1) & 1) + 1,
            2 * (k - 1) + 1 - ((n >> 2) & 1) + 1 if dim == 3 else 0)


def preorder(flags, dim):
    """the cells of a tree in file order: (level, array index, child id, is leaf); flags[l] is the
    (n + 2)^dim array of level l (0 absent, 1 leaf, 2 non-leaf)"""
    out = []

    def walk(l, i, j, k, cid):
        idx = (k, j, i) if dim == 3 else (j, i)
        f = flags[l][idx]
        assert f in (1, 2), "no cell at level %d %s" % (l, idx)
        out.append((l, idx, cid, f == 1))
        if f == 2:
            for n in range(1 << dim):
                walk(l + 1, *child_index(dim, i, j, k, n), n)

    walk(0, 1, 1, 1, 0)
    return out


def image(flags, values, dim):
    """values[v][l]: the array of variable v on level l"""
    nv = len(values)
    fmt = "<Id%dd" % nv
    out = bytearray()
    for l, idx, cid, leaf in preorder(flags, dim):
        out += struct.pack(fmt, cid | (FLAG_LEAF if leaf else 0), -1., *[values[v][l][idx] for v in range(nv)])
    return bytes(out)


def image_from_oracle(o, which_list):
    """the cell data a binary simulation file holds for the tree `o' (oracle.Tree) and its variables
    `which_list' (oracle.Tree.U ...), non-leaf cells included"""
    levels = range(o.depth + 1)
    return image([o.flags(l) for l in levels], [[o.values(w, l) for l in levels] for w in which_list], o.dim)


def records(data, nvars):
    """[(flags, solid marker, values)] of an image"""
    rec = 12 + 8 * nvars
    assert len(data) % rec == 0
    return [(struct.unpack_from("<I", data, p)[0], struct.unpack_from("<d", data, p + 4)[0],
             struct.unpack_from("<%dd" % nvars, data, p + 12)) for p in range(0, len(data), rec)]


# ---- gfscompare on two different trees (tools/gfscompare.c:153-214,244-268), restated

def _locate(flags, dim, level, pos):
    """ftt_cell_locate (pos, max_depth = level): the cell of the tree that holds the point, at `level' or the
    leaf above it: (level, index)"""
    l, i, j, k = 0, 1, 1, 1
    while l < level and flags[l][(k, j, i) if dim == 3 else (j, i)] == 2:
        l += 1
        n = 1 << l
        i = min(int((pos[0] + 0.5) * n), n - 1) + 1
        j = min(int((pos[1] + 0.5) * n), n - 1) + 1
        k = min(int((pos[2] + 0.5) * n), n - 1) + 1 if dim == 3 else 0
    return l, ((k, j, i) if dim == 3 else (j, i))


def compare_norms(flags1, v1, flags2, v2, dim, constant=False, weighted=True):
    """The norms gfscompare prints for one variable of FILE1 (flags1, v1[l]) against FILE2
    (difference_tree + inject): every cell of FILE1 is located in FILE2 at its own level; where FILE2 is
    coarser the call returns false and the parent takes over: a cell none of whose children `added' gets
    e = v1 (cell) - v2 (located cell) -- the located cell may be a non-leaf of FILE2: its stored value is
    used -- injected into all its descendants.  Norms over the leaves of FILE1, weights = cell volumes
    (-w: 1); -C subtracts the weighted mean of e first.  Returns (first, second, infty, weight)."""
    err = {}

    def centre(l, idx):
        n = 1 << l
        c = [(-0.5 + (q - 0.5) / n) for q in reversed(idx)]
        return c + [0.] * (3 - len(c))

    def children(l, idx):
        i, j = idx[-1], idx[-2]
        k = idx[0] if dim == 3 else 0
        for n in range(1 << dim):
            ci, cj, ck = child_index(dim, i, j, k, n)
            yield l + 1, ((ck, cj, ci) if dim == 3 else (cj, ci))

    def inject(l, idx):
        if flags1[l][idx] == 2:
            for cl, cidx in children(l, idx):
                err[(cl, cidx)] = err[(l, idx)]
                inject(cl, cidx)

    def difference_tree(l, idx):
        l2, idx2 = _locate(flags2, dim, l, centre(l, idx))
        if l2 != l:
            return False
        added = False
        if flags1[l][idx] == 2:
            for cl, cidx in children(l, idx):
                if difference_tree(cl, cidx):
                    added = True
        if not added:
            err[(l, idx)] = v1[l][idx] - v2[l2][idx2]
            inject(l, idx)
        return True

    assert difference_tree(0, (1, 1, 1) if dim == 3 else (1, 1))
    e, w = [], []
    for l, idx, _, leaf in preorder(flags1, dim):
        if leaf:
            e.append(err[(l, idx)])
            w.append((1. / (1 << l)) ** dim if weighted else 1.)
    e, w = np.array(e), np.array(w)
    if constant:
        e = e - (w * e).sum() / w.sum()
    return (w * abs(e)).sum() / w.sum(), np.sqrt((w * e * e).sum() / w.sum()), abs(e).max(), w.sum()
