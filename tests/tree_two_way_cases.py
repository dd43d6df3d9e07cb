"""The trees, particles, kernels and fields of tests/test_tree_two_way_reference_cpu.py and
tests/test_gpu_tree_two_way.py: everything that needs no device."""
import functools
import math

import numpy as np

import sampler_reference as R
import tree_sampler_cases as TC
import tree_sampler_reference as T
import tree_two_way_reference as TW

P, B = R.SIDE_PERIODIC, R.SIDE_BOUNDARY

# the L-shaped patch of tests/test_gpu_tree_particulates.py: level 2 with three of the four cells in the middle
# refined once; the coarse cell in the notch has refined neighbours on two sides
ELL = (2, lambda x, y: 3 if (abs(x) < 0.25 and abs(y) < 0.25 and not (x > 0. and y > 0.)) else 2, [P]*4)
REFINED = ("square", "graded", "walls2", "cube", "box3", "ell")
ALL = ("uniform2",) + REFINED

# the kernel functions: C text for the device, the same expression for the restatement
POLY = ("(1. - 0.04*(x*x + y*y + z*z))", lambda x, y, z, t: (1. - 0.04*(x*x + y*y + z*z)))
GAUSS = ("exp (-(x*x+y*y+z*z))", lambda x, y, z, t: math.exp(-(x*x + y*y + z*z)))
ONE = ("1", lambda x, y, z, t: 1.)

# a uniform source field that is a GfsSource: dyadic, and large enough that the acceleration sets the time step
G_UNIFORM = (32., -16., 8.)


def spec(name):
    """(dim, refine, sides)"""
    return ELL if name == "ell" else TC.TREES[name][:3]


def refined_set(dim, refine):
    """the cells with children of the tree GfsRefine `refine' gives: a cell is refined while the level wanted at
    its centre is deeper than its own, then wherever a neighbour (faces, edges and corners) is two levels deeper"""
    refined = set()

    def visit(l, q):
        n = 1 << l
        centre = [(q[c] + 0.5)/n - 0.5 for c in range(dim)]
        if refine(*centre) > l:
            refined.add((l, q))
            for o in np.ndindex(*(2,)*dim):
                visit(l + 1, tuple(2*q[c] + o[c] if c < dim else 0 for c in range(3)))
    visit(0, (0, 0, 0))
    while True:
        more = set()
        for l, q in refined:
            if l < 2:
                continue
            n = 1 << l
            for o in np.ndindex(*(3,)*dim):
                nq = tuple(q[c] + o[c] - 1 if c < dim else 0 for c in range(3))
                if all(0 <= nq[c] < n for c in range(dim)):
                    parent = (l - 1, tuple(x//2 for x in nq))
                    if parent not in refined:
                        more.add(parent)
        if not more:
            return refined
        refined |= more


@functools.lru_cache(None)
def host_tree(name):
    """the TreeBox of a named tree, built without the library"""
    dim, refine, _sides = spec(name)
    return T.TreeBox(dim, refined_set(dim, refine))


def levels_of_leaves(box):
    return sorted(set(c.level for c in box.leaves))


def h_fine(box):
    return 1./(1 << max(levels_of_leaves(box)))


def h_coarse(box):
    return 1./(1 << min(levels_of_leaves(box)))


def rkernels(box):
    return (0., 1.5*h_fine(box), 2.5*h_coarse(box))


class Part:
    """what the coupling reads of a GfsParticulate"""
    __slots__ = ("pos", "id", "volume", "force")

    def __init__(self, pos, pid, volume, force):
        self.pos, self.id = [float(x) for x in pos], int(pid)
        self.volume, self.force = float(volume), [float(x) for x in force]


def dyadic_forces(n, dim, seed):
    """multiples of 1/64 in [-2, 2]: every sum and every division by a cell volume is exact"""
    rng = np.random.default_rng(seed)
    f = np.zeros((n, 3))
    f[:, :dim] = rng.integers(-128, 129, (n, dim))/64.
    return f


def spread_particles(box, seed=5, target=90):
    """the particles of the spreading tests, in list order:
    - about `target' of TC.seeds (next to the faces and corners of leaves of every level, a few outside the box), with
      volumes whose rb = pow (3 V/(4 pi), 1./3.) is between 0.06 and 0.3: the polynomial kernel changes sign within
      2.5 h_coarse of most of them;
    - pairs and triples in one leaf (one fine, one coarse), far apart in the list;
    - a particle on a face between two levels, one on a box side, one in a box corner;
    - a particle of volume 1e-12 off the centre of its leaf: |q| > 5 on its whole stencil, the polynomial kernel is
      negative there, correction <= 1e-10 and nothing is deposited.
    Returns pos (n, 3), ids, volume, force (dyadic)."""
    dim = box.dim
    rng = np.random.default_rng(seed)
    pos, _ = TC.seeds(box, 3)
    step = max(1, len(pos)//target)
    pts = [list(p) for p in pos[::step]]
    pts += [list(p) for p in pos[-dim:]]                    # those that start outside the box
    fine = max(box.leaves, key=lambda c: (c.level, c.pos))
    coarse = min(box.leaves, key=lambda c: (c.level, c.pos))
    shared = []
    for c, k in ((fine, 3), (coarse, 2)):
        h = box.cell_size(c)
        for _ in range(k):
            shared.append([c.pos[a] + rng.uniform(-0.4, 0.4)*h if a < dim else 0. for a in range(3)])
    pts = shared[:2] + pts + shared[2:]
    # on a face between two levels: the face of a leaf whose neighbour is coarser
    for c in box.leaves:
        nb = box.neighbor(c, 0)
        if nb is not None and not nb.boundary and nb.level < c.level:
            p = [c.pos[a] if a < dim else 0. for a in range(3)]
            p[0] = c.pos[0] + box.cell_size(c)/2.
            pts.append(p)
            break
    side = [0.]*3
    side[0] = 0.5
    side[1] = 0.1875 + 1./1024.
    pts.append(side)
    pts.append([0.5 - 1./2048. if a < dim else 0. for a in range(3)])
    n_regular = len(pts)
    tiny = [fine.pos[a] + 0.3*box.cell_size(fine) if a < dim else 0. for a in range(3)]
    pts.append(tiny)
    pos = np.array(pts, dtype=np.float64)
    n = len(pos)
    volume = 10.**rng.uniform(-3., -1., n)
    volume[n_regular:] = 1e-12
    return pos, np.arange(1, n + 1, dtype=np.uint32), volume, dyadic_forces(n, dim, seed + 1)


def parts(pos, ids, volume, force):
    return [Part(p, i, v, f) for p, i, v, f in zip(pos.tolist(), ids.tolist(), volume.tolist(), force.tolist())]


def field_array(box, v, level):
    return np.array(v[level], dtype=np.float64)


def leaf_mask(box, level):
    return np.array(box.flags(level)) == T.LEAF


def interior_leaf_mask(box, level):
    """the leaves of the box itself: not the ghost leaves"""
    m = leaf_mask(box, level)
    inner = np.zeros_like(m)
    inner[(slice(1, -1),)*box.dim] = True
    return m & inner


def constant_field(box, g):
    out = []
    for l in range(box.level + 1):
        out.append(np.full(((1 << l) + 2,)*box.dim, float(g)).tolist())
    return out


@functools.lru_cache(None)
def uniform_field_is_exact(name):
    """the premise of the uniform-field test: the restated MAC value of the constant field g is g at every leaf,
    for every component and every g of G_UNIFORM"""
    box = host_tree(name)
    for c in range(box.dim):
        Fc = constant_field(box, G_UNIFORM[c])
        for cell in box.leaves:
            if TW.mac_source_value(box, cell, c, Fc) != G_UNIFORM[c]:
                return False
    return True


def uniform_field_trees():
    return tuple(name for name in REFINED if uniform_field_is_exact(name))


def striped(dim, axis):
    """a band of level 4 in level 3 across the box (2-D; level 3 in level 2 in 3-D) that depends on the coordinate
    `axis' alone: (dim, refine, sides)"""
    lo, hi = (3, 4) if dim == 2 else (2, 3)
    if dim == 2:
        return dim, (lambda x, y: hi if abs((x, y)[axis]) < 0.125 else lo), [P]*4
    return dim, (lambda x, y, z: hi if abs((x, y, z)[axis]) < 0.25 else lo), [P]*6
