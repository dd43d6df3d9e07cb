"""The trees, points, fields and particles of tests/test_gpu_tree_sampler.py: everything that needs no
device, so that it can be built and looked at on a CPU."""
import itertools
import math

import numpy as np

import sampler_reference as R
import tree_sampler_reference as T

P, B = R.SIDE_PERIODIC, R.SIDE_BOUNDARY

# name: (dim, refine (x, y[, z]) -> level, sides, what an event of the tracers must show on this tree)
TREES = {
    "uniform2": (2, lambda x, y: 3, [P]*4, ("wrapped", "left_through_edge")),
    "square": (2, lambda x, y: 3 if (abs(x) < 0.25 and abs(y) < 0.25) else 2, [P]*4,
               ("wrapped", "left_through_edge", "fine_to_coarse", "coarse_to_fine")),
    # two levels in one patch: 16 cells of level 4 inside a ring of level 3 inside level 2
    "graded": (2, lambda x, y: 4 if (abs(x) < 0.13 and abs(y) < 0.13) else 2, [P]*4,
               ("wrapped", "left_through_edge", "fine_to_coarse", "coarse_to_fine")),
    # the patch touches two GfsBoundary sides: inflow on the left, outflow on the right, slip walls
    "walls2": (2, lambda x, y: 4 if (x < -0.25 and y > 0.) else 3, [B]*4,
               ("removed", "fine_to_coarse", "coarse_to_fine")),
    "cube": (3, lambda x, y, z: 3 if (abs(x) < 0.25 and abs(y) < 0.25 and abs(z) < 0.25) else 2, [P]*6,
             ("wrapped", "left_through_edge", "fine_to_coarse", "coarse_to_fine")),
    # slip walls in x and y, periodic in z
    "box3": (3, lambda x, y, z: 3 if (x < -0.25 and y > 0. and abs(z) < 0.26) else 2, [B]*4 + [P]*2,
             ("wrapped", "fine_to_coarse", "coarse_to_fine")),
}


def restatement(dim, flags):
    """the TreeBox of the flags of a gfship.Tree; its own flags, ghost trees included, must be those"""
    box = T.TreeBox.from_flags(dim, flags)
    for l, f in enumerate(flags):
        assert np.array_equal(np.array(box.flags(l), dtype=np.uint8), f), "flags of level %d" % l
    return box


def distinct_values(dim, flags, salt=0):
    """per level an array with ghosts: a distinct value in [0.5, 1.5) for every cell of the tree, ghosts included,
    NaN where the level has no cell (the edge and corner ghosts among them)"""
    out = []
    for l, f in enumerate(flags):
        idx = np.arange(f.size, dtype=np.float64).reshape(f.shape)
        a = np.modf(np.sqrt(3. + 7.*idx + 1015.*(salt + 31*l)))[0] + 0.5
        a[f == T.NONE] = np.nan
        out.append(a)
    return out


def random_values(dim, flags, seed):
    rng = np.random.default_rng(seed)
    out = []
    for f in flags:
        a = rng.uniform(-1., 1., f.shape)
        a[f == T.NONE] = np.nan
        out.append(a)
    return out


def sample_points(box, seed):
    """the half-cell lattice of every leaf (centres, face centres, edges, corners: the strict `>' of the descent
    decides there), points one ulp on either side of every face of every leaf (the changes of level and the box
    sides among them, so +-0.5 and one ulp beyond), the corners of the box, random points"""
    dim = box.dim
    rng = np.random.default_rng(seed)
    pts = set()
    for c in box.leaves:
        h = box.cell_size(c)
        for o in itertools.product((-0.5, 0., 0.5), repeat=dim):
            pts.add(tuple(c.pos[a] + o[a]*h for a in range(dim)) + (0.,)*(3 - dim))
        for a in range(dim):
            for s in (-1., 1.):
                face = c.pos[a] + s*h/2.
                for x in (float(np.nextafter(face, -np.inf)), float(np.nextafter(face, np.inf))):
                    p = [c.pos[b] + rng.uniform(-0.45, 0.45)*h for b in range(dim)] + [0.]*(3 - dim)
                    p[a] = x
                    pts.add(tuple(p))
    for s in itertools.product((-0.5, 0.5), repeat=dim):
        pts.add(tuple(s) + (0.,)*(3 - dim))
        for a in range(dim):
            p = list(s) + [0.]*(3 - dim)
            p[a] = float(np.nextafter(s[a], s[a]*np.inf))
            pts.add(tuple(p))
    out = sorted(pts) + [tuple(rng.uniform(-0.5, 0.5, dim)) + (0.,)*(3 - dim) for _ in range(200)]
    return np.array(out, dtype=np.float64)


def initial_velocity(name, centres):
    """Init {} { U = ... V = ... W = ... } at the cell centres of a level (arrays with ghosts)"""
    dim = TREES[name][0]
    X, Y = centres[0], centres[1]
    Z = centres[2] if dim == 3 else 0.
    if name == "walls2":       # left to right, and a solenoidal eddy that goes up into the patch across y = 0
        Xs = X + 0.5
        return [1. + 0.3*np.cos(2.*math.pi*Y) + 0.45*np.sin(math.pi*Y)*np.sin(2.*math.pi*Xs),
                0.9*np.cos(math.pi*Y)*np.cos(2.*math.pi*Xs)]
    if name == "box3":         # vortices that respect the walls, a stream along z
        Xs, Ys = X + 0.5, Y + 0.5
        return [np.sin(math.pi*Xs)*np.cos(math.pi*Ys), -np.cos(math.pi*Xs)*np.sin(math.pi*Ys),
                0.8 + 0.*Z + 0.1*np.sin(2.*math.pi*X)]
    u = [0.8 + 0.15*np.sin(2.*math.pi*(X + 0.7*Y + 0.4*Z) + k)*np.cos(2.*math.pi*(Y - X) + 0.5*k) for k in range(dim)]
    return u


def inflow_profile(centres):
    return 1. + 0.3*np.cos(2.*math.pi*centres[1])


def seeds(box, seed):
    """particles next to every face and in every corner of every leaf, on the inside, a few per cent of the leaf's
    size away: whatever way the flow goes some cross to a coarser leaf, to a finer one and through a box side within
    a few steps; in the leaves at the corners of the box, at several distances from both sides, so that some have
    their RK2 midpoint inside and their end point outside along two axes; and a few outside from the start"""
    dim = box.dim
    rng = np.random.default_rng(seed)
    pts = []
    for c in box.leaves:
        h = box.cell_size(c)
        for frac in ((0.02, 0.15) if dim == 2 else (0.06,)):
            for a in range(dim):
                for s in (-1., 1.):
                    p = [c.pos[b] + rng.uniform(-0.4, 0.4)*h for b in range(dim)] + [0.]*(3 - dim)
                    p[a] = c.pos[a] + s*(0.5 - frac)*h
                    pts.append(p)
        at_sides = sum(abs(abs(c.pos[a]) + h/2. - 0.5) < 1e-12 for a in range(dim))
        for frac in ((0.03,) if at_sides < dim else (0.03, 0.08, 0.14, 0.2, 0.27, 0.35, 0.45)):
            for s in itertools.product((-1., 1.), repeat=dim):
                pts.append([c.pos[b] + s[b]*(0.5 - frac)*h for b in range(dim)] + [0.]*(3 - dim))
    for a in range(dim):
        p = list(rng.uniform(-0.45, 0.45, dim)) + [0.]*(3 - dim)
        p[a] = 0.50001
        pts.append(p)
    pos = np.array(pts, dtype=np.float64)
    return pos, np.arange(1, len(pos) + 1, dtype=np.uint32)
