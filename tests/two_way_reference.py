"""A plain restatement of the two classes through which particles act on the fluid, GfsParticulateField and
the event of GfsSourceParticulate (modules/particulatecommon.c:1927-2228), for one uniform unit box
(-0.5, 0.5)^dim with L = 1.

Everything is a Python loop over the particles in list order and over the cells in the order of the
reference's traversal, with Python floats (IEEE doubles, one rounding per operation, no contraction): the
sums are the reference's own sequences of additions, so a device result can be compared bit for bit.  The
pruned descent of gfs_domain_cell_traverse_condition is written out as the recursion it is
(src/ftt.c:948-986), not as a stencil.  The line numbers in the comments are those of
modules/particulatecommon.c unless a file is named.

Arrays of cell values are indexed [k][j][i] (3-D) or [j][i] (2-D) like everywhere in tests/, without ghosts.
Cells are named by 0-based integer coordinates ix = (i, j[, k]) counted from the low corner of the box."""
import math

import numpy as np


def cell_centre(l, ix):
    """ftt_cell_pos of cell ix of level l: dyadic numbers, exact"""
    size = 1. / (1 << l)
    return [-0.5 + (i + 0.5) * size for i in ix]


def locate(dim, depth, p):
    """ftt_cell_locate (src/ftt.c:1535-1574) down to the leaves: ix or None.  The comparisons are strict: a
    point on a cell face belongs to the cell on its low side."""
    pos = [0.] * dim
    size = 1. / 2.
    for c in range(dim):
        if p[c] > pos[c] + size or p[c] < pos[c] - size:
            return None
    ix = [0] * dim
    for _ in range(depth):
        size /= 2.
        for c in range(dim):
            up = p[c] > pos[c]
            ix[c] = 2 * ix[c] + (1 if up else 0)
            pos[c] += size if up else -size
    return tuple(ix)


def _index(dim, ix):
    return (ix[1], ix[0]) if dim == 2 else (ix[2], ix[1], ix[0])


def void_fraction(dim, depth, pos, volume):
    """particulate_field_event (:1934-1957): v reset, then v[cell] += volume/ftt_cell_volume (cell) for every
    particle with a cell, in list order"""
    n = 1 << depth
    h = 1. / n
    cellvol = h * h * h if dim == 3 else h * h
    v = np.zeros((n,) * dim)
    for p, vol in zip(pos, volume):
        ix = locate(dim, depth, p)
        if ix is not None:
            v[_index(dim, ix)] += float(vol) / cellvol
    return v


def cond_kernel(dim, l, ix, p, rkernel):
    """cond_kernel (:2126-2156)"""
    pos = cell_centre(l, ix)
    size = (1. / (1 << l)) / 2.
    radeq = size * math.sqrt(2.) if dim == 2 else size * math.sqrt(3.)
    if dim == 2:                                   # ftt_vector_distance, src/ftt.h:53-59
        dist = math.sqrt((pos[0] - p[0]) * (pos[0] - p[0]) + (pos[1] - p[1]) * (pos[1] - p[1]))
    else:
        dist = math.sqrt((pos[0] - p[0]) * (pos[0] - p[0]) + (pos[1] - p[1]) * (pos[1] - p[1]) +
                         (pos[2] - p[2]) * (pos[2] - p[2]))
    if dist - radeq <= rkernel:
        return True
    for c in range(dim):
        if p[c] > pos[c] + size or p[c] < pos[c] - size:
            return False
    return True


def children(dim, ix):
    """the children n = 0 .. FTT_CELLS - 1 of cell ix: child n sits at x:+ for bit 0, y:- for bit 1, z:- for
    bit 2 (coords[], src/ftt.c:301-316)"""
    out = []
    for n in range(1 << dim):
        c = [2 * ix[0] + (n & 1), 2 * ix[1] + (0 if n & 2 else 1)]
        if dim == 3:
            c.append(2 * ix[2] + (0 if n & 4 else 1))
        out.append(tuple(c))
    return out


def descent(dim, depth, p, rkernel):
    """the leaves gfs_domain_cell_traverse_condition (src/domain.c:1550-1574, FTT_PRE_ORDER,
    FTT_TRAVERSE_LEAFS) visits with cond_kernel, in its order: ftt_cell_traverse_condition
    (src/ftt.c:948-986) stops at every cell that fails"""
    out = []

    def traverse(l, ix):
        if not cond_kernel(dim, l, ix, p, rkernel):
            return
        if l == depth:
            out.append(ix)
            return
        for c in children(dim, ix):
            traverse(l + 1, c)

    traverse(0, (0,) * dim)
    return out


def traversal_order(dim, depth):
    """every leaf in the order of the unconditional pre-order traversal"""
    out = []

    def traverse(l, ix):
        if l == depth:
            out.append(ix)
            return
        for c in children(dim, ix):
            traverse(l + 1, c)

    traverse(0, (0,) * dim)
    return out


def flat_filter(dim, depth, p, rkernel, order=None):
    """the leaves that pass cond_kernel themselves, whatever their ancestors do, in traversal order"""
    order = traversal_order(dim, depth) if order is None else order
    return [ix for ix in order if cond_kernel(dim, depth, ix, p, rkernel)]


def normalized_distance(dim, centre, p, volume):
    """distance_normalization (:2089-2099).  As written there, `pos1->z = 0.' comes before the 3-D line
    `pos1->z = (pos1->z - pos2->z)/rb': z is (0. - pos.z)/rb in 3-D, whatever the cell."""
    rb = (3. * volume / (4. * math.pi)) ** (1. / 3.)
    x = (centre[0] - p[0]) / rb
    y = (centre[1] - p[1]) / rb
    z = 0.
    if dim == 3:
        z = (z - p[2]) / rb
    return x, y, z


def spread(dim, depth, pos, volume, force, rkernel, K, t=0., alpha_cell=None):
    """source_particulate_event (:2177-2228) from the stored forces: F reset, then per particle in list
    order kernel_volume over the visited leaves, correction /= volume, diffuse_force over the same leaves.
    K (x, y, z, t) is the kernel function; alpha_cell the array of alpha at the cell centres or None.
    Returns (F, correction): F[c] per component, correction per particle."""
    n = 1 << depth
    h = 1. / n
    cellvol = h * h * h if dim == 3 else h * h
    F = [np.zeros((n,) * dim) for _ in range(dim)]
    corrections = []
    for p, vol, f in zip(pos, volume, force):
        p = [float(a) for a in p]
        vol = float(vol)
        leaves = descent(dim, depth, p, rkernel)
        ksum_volume, correction = 0., 0.
        for ix in leaves:                               # kernel_volume, :2108-2119
            ksum_volume += cellvol
            q = normalized_distance(dim, cell_centre(depth, ix), p, vol)
            correction += K(q[0], q[1], q[2], t) * cellvol
        correction = correction / ksum_volume if leaves else float("nan")      # :2216
        corrections.append(correction)
        if not correction > 1.e-10:                     # diffuse_force, :2158-2175
            continue
        for ix in leaves:
            q = normalized_distance(dim, cell_centre(depth, ix), p, vol)
            k = K(q[0], q[1], q[2], t)
            at = _index(dim, ix)
            liq_rho = 1. / float(alpha_cell[at]) if alpha_cell is not None else 1.
            for c in range(dim):
                F[c][at] -= float(f[c]) / liq_rho / cellvol * k / correction
    return F, np.array(corrections)


def spread_flat(dim, depth, pos, volume, force, rkernel, K, t=0., alpha_cell=None):
    """spread, with the loops over the cells as numpy operations (a box of 32^3 cells and a kernel that reaches all
    of them is out of reach of the loops of spread).  Per particle in list order: the leaves in the order of the
    traversal that pass cond_kernel themselves (flat_filter: the leaves of the pruned descent, see
    test_pruned_descent_visits_the_leaves_of_the_flat_filter), kernel_volume as a strictly sequential accumulation
    over them (np.add.accumulate, never a pairwise np.sum), then the subtraction of diffuse_force in every one of
    them -- one cell at most once per particle, so the additions into a cell keep the list order.  Every operation
    is the elementwise double operation of spread, in its order.  K takes arrays x, y, z."""
    n = 1 << depth
    h = 1. / n
    cellvol = h * h * h if dim == 3 else h * h
    order = np.array(traversal_order(dim, depth))             # [leaf][axis]
    centre = -0.5 + (order + 0.5) * h                         # cell_centre
    at = order[:, 1] * n + order[:, 0] if dim == 2 else (order[:, 2] * n + order[:, 1]) * n + order[:, 0]
    size = h / 2.
    radeq = size * math.sqrt(2.) if dim == 2 else size * math.sqrt(3.)
    F = [np.zeros(n ** dim) for _ in range(dim)]
    liq_rho = 1. / np.asarray(alpha_cell, dtype=float).reshape(-1) if alpha_cell is not None else None
    corrections = []
    for p, vol, f in zip(pos, volume, force):
        p = [float(a) for a in p]
        vol = float(vol)
        d = [centre[:, c] - p[c] for c in range(dim)]         # cond_kernel
        dist = np.sqrt(d[0] * d[0] + d[1] * d[1]) if dim == 2 else np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        inside = np.ones(len(order), dtype=bool)
        for c in range(dim):
            inside &= ~((p[c] > centre[:, c] + size) | (p[c] < centre[:, c] - size))
        leaves = np.flatnonzero((dist - radeq <= rkernel) | inside)
        if len(leaves) == 0:
            corrections.append(float("nan"))
            continue
        rb = (3. * vol / (4. * math.pi)) ** (1. / 3.)         # normalized_distance
        x = (centre[leaves, 0] - p[0]) / rb
        y = (centre[leaves, 1] - p[1]) / rb
        z = np.full(len(leaves), (0. - p[2]) / rb if dim == 3 else 0.)
        k = np.broadcast_to(np.asarray(K(x, y, z, t), dtype=float), x.shape)
        ksum_volume = np.add.accumulate(np.full(len(leaves), cellvol))[-1]
        correction = float(np.add.accumulate(k * cellvol)[-1] / ksum_volume)
        corrections.append(correction)
        if not correction > 1.e-10:
            continue
        cells = at[leaves]
        for c in range(dim):
            fc = float(f[c]) / (liq_rho[cells] if liq_rho is not None else 1.)
            F[c][cells] -= fc / cellvol * k / correction
    return [a.reshape((n,) * dim) for a in F], np.array(corrections)
