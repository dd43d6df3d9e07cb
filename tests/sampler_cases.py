"""The case matrix of the sampler tests, shared by test_sampler_reference_cpu.py (restatement alone,
oracle against restatement) and test_gpu_sampler_reference.py (device against restatement).  The
references are computed once per process (functools caches) and never modified."""
import functools
import itertools
import math

import numpy as np

import sampler_reference as R

P, B, E = R.SIDE_PERIODIC, R.SIDE_BOUNDARY, R.SIDE_EXTERNAL
BC_DIRICHLET, BC_NEUMANN = 1, 2
DIMS_LEVELS = [(dim, level) for dim in (2, 3) for level in (1, 2, 3)]
# mixed1: x periodic, +y closed / -y external, +z external / -z closed
# mixed2: +x closed / -x external, y periodic, +z closed / -z external
SIDES = {"periodic": [P]*6, "closed": [B]*6, "external": [E]*6,
         "mixed1": [P, P, B, E, E, B], "mixed2": [B, E, P, P, B, E]}
SAMPLER_VARIANTS = ("distinct", "nodata", "bc_periodic", "bc_dirichlet", "bc_neumann")
TRACER_FIELDS = ("smooth", "distinct")
NEVENTS = 3


@functools.lru_cache(None)
def box(dim, level):
    return R.Box(dim, level)


def ghost_count(dim, level):
    """per entry of an array with ghosts: the number of its indices lying in a ghost layer"""
    n = 1 << level
    g = np.zeros((n + 2,)*dim, dtype=int)
    for ax in range(dim):
        sl = [slice(None)]*dim
        for i in (0, n + 1):
            sl[ax] = i
            g[tuple(sl)] += 1
    return g


def distinct_field(dim, level, salt=0):
    """a distinct irrational-looking value in [0.5, 1.5) for every interior cell and every face
    ghost; NaN in the edge and corner ghosts, which no cell of the reference corresponds to"""
    n = 1 << level
    shape = (n + 2,)*dim
    idx = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
    a = np.modf(np.sqrt(3. + 7.*idx + 1015.*salt))[0] + 0.5      # 7 k + 3 is never a square
    a[ghost_count(dim, level) >= 2] = np.nan
    return a


@functools.lru_cache(None)
def sample_points(dim, level):
    """points built for every cell: the half-cell lattice (centre, faces, edges and corners of every
    cell: the tie rule of locate; the box sides at exactly +-0.5), the quarter points on the diagonals
    of every cell (x == 0 or y == 0 of the 2-D formula), random interior points, and points one ulp
    outside each box side"""
    n = 1 << level
    h = 1./n
    rng = np.random.default_rng(100*dim + level)
    lat = [-0.5 + k*h/2. for k in range(2*n + 1)]
    pts = [p + (0.,)*(3 - dim) for p in itertools.product(lat, repeat=dim)]
    centres = [-0.5 + (i + 0.5)*h for i in range(n)]
    for c in itertools.product(centres, repeat=dim):
        if dim == 2:
            signs = list(itertools.product((-1., 1.), repeat=2))
        else:       # two of the eight diagonal directions per cell
            signs = [tuple(rng.choice((-1., 1.), 3)) for _ in range(2)]
        for s in signs:
            pts.append(tuple(c[a] + s[a]*h/4. for a in range(dim)) + (0.,)*(3 - dim))
        r = rng.uniform(-0.49, 0.49, dim)
        pts.append(tuple(c[a] + r[a]*h for a in range(dim)) + (0.,)*(3 - dim))
    for a in range(dim):
        for s in (-1., 1.):
            for _ in range(4):
                p = list(rng.uniform(-0.5, 0.5, dim)) + [0.]*(3 - dim)
                p[a] = float(np.nextafter(s*0.5, s*np.inf))
                pts.append(tuple(p))
            p = [s*0.5]*dim + [0.]*(3 - dim)      # past a box corner along one axis only
            p[a] = float(np.nextafter(s*0.5, s*np.inf))
            pts.append(tuple(p))
    out = np.array(pts, dtype=np.float64)
    out.setflags(write=False)
    return out


def _side_slab(dim, level, d, ghost):
    """index of the ghost layer (or of the interior layer next to it) of side d in an [k, j, i] array"""
    n = 1 << level
    sl = [slice(1, n + 1)]*dim
    ax = dim - 1 - d//2
    if ghost:
        sl[ax] = n + 1 if d % 2 == 0 else 0
    else:
        sl[ax] = n if d % 2 == 0 else 1
    return tuple(sl)


@functools.lru_cache(None)
def bc_case(dim, level, kind):
    """(sides, interior values, {side: (bc kind, face values)}, the array with the ghosts the
    reference's boundary cells would hold): periodic: the value of the cell across the box
    (src/boundary.c, GfsBoundaryPeriodic copies the matching cells); Dirichlet: 2*val - neighbour
    (:253-258); Neumann: neighbour + val*size (:336-342).  Edge and corner ghosts: NaN."""
    n = 1 << level
    h = 1./n
    a = distinct_field(dim, level, salt=5)
    vals = {}
    if kind == "periodic":
        sides = [P]*6
        for d in range(2*dim):
            a[_side_slab(dim, level, d, True)] = a[_side_slab(dim, level, d ^ 1, False)]
    else:
        sides = [B]*6
        for d in range(2*dim):
            val = distinct_field(dim, level, salt=10 + d)[_side_slab(dim, level, d, False)] - 1.
            nb = a[_side_slab(dim, level, d, False)]
            if kind == "dirichlet":
                a[_side_slab(dim, level, d, True)] = 2.*val - nb
                vals[d] = (BC_DIRICHLET, np.ascontiguousarray(val))
            else:
                a[_side_slab(dim, level, d, True)] = nb + val*h
                vals[d] = (BC_NEUMANN, np.ascontiguousarray(val))
    interior = a[(slice(1, n + 1),)*dim].copy()
    a.setflags(write=False)
    return sides, interior, vals, a


def face_ghosts_equal(dim, level, a, b):
    return all(np.array_equal(a[_side_slab(dim, level, d, True)], b[_side_slab(dim, level, d, True)])
               for d in range(2*dim))


@functools.lru_cache(None)
def sampler_field(dim, level, variant):
    """the array with ghosts the sampler reads in each variant"""
    n = 1 << level
    if variant == "distinct":
        a = distinct_field(dim, level)
    elif variant == "nodata":
        # GFS_NODATA in one interior cell and in one face ghost (of the +x side)
        a = distinct_field(dim, level)
        a[(1,)*dim] = R.GFS_NODATA
        a[(n,)*(dim - 1) + (n + 1,)] = R.GFS_NODATA
    else:
        a = bc_case(dim, level, variant[3:])[3].copy()
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def reference_sample(dim, level, variant, nodata=False):
    """(values, inside) of the restatement at sample_points.  nodata = False: GFS_NODATA is an
    ordinary number, which is what the library and the oracle do (see gfship_field_interpolate)"""
    b = box(dim, level)
    out, inside = b.sample(b.field(sampler_field(dim, level, variant)), sample_points(dim, level).tolist(),
                           nodata=nodata)
    out, inside = np.array(out), np.array(inside, dtype=bool)
    out.setflags(write=False)
    inside.setflags(write=False)
    return out, inside


# -------------------------------------------------------------------------------------------------
# plain tracers
# -------------------------------------------------------------------------------------------------

def tracer_dt(level):
    return 0.2/(1 << level)


@functools.lru_cache(None)
def tracer_field(dim, level, name):
    """velocity components as arrays with ghosts.  smooth: non-linear, towards the (+,+,+) corner of
    the box; distinct: the distinct-values fill (NaN in the edge and corner ghosts), towards the
    (-,-,-) corner.  Speeds within [0.55, 1.05]."""
    n = 1 << level
    u = []
    if name == "smooth":
        c = -0.5 + (np.arange(n + 2) - 0.5)/n
        X = c.reshape((1,)*(dim - 1) + (n + 2,))
        Y = c.reshape((1,)*(dim - 2) + (n + 2, 1))
        Z = c.reshape((n + 2, 1, 1)) if dim == 3 else 0.
        for k in range(dim):
            u.append(0.8 + 0.15*np.sin(2.*math.pi*(X + 0.7*Y + 0.4*Z) + k)*np.cos(math.pi*(Y - 0.3*X) + 0.5*k)
                     + 0.*(X + Y + Z))
    else:
        for k in range(dim):
            u.append(-(0.3 + 0.5*distinct_field(dim, level, salt=20 + k)))
    for a in u:
        a.setflags(write=False)
    return tuple(u)


@functools.lru_cache(None)
def tracer_particles(dim, level, name):
    """at most 512 particles per list, built for every outcome of an event: paths that stay inside;
    start points so close to a face, an edge or a corner of the box that the RK2 midpoint is already
    outside (the particle does not move); start points from which the midpoint is inside and the end
    point outside through a face, an edge (two coordinates cross) or a corner (three); points on the
    box sides; points outside from the start"""
    n = 1 << level
    s = 1. if name == "smooth" else -1.
    rng = np.random.default_rng(1000*dim + 10*level + (name == "smooth"))
    step = 0.8*tracer_dt(level)          # length of a step along each axis, roughly
    pts = []
    for k in range(1, dim + 1):
        for S in itertools.combinations(range(dim), k):
            for frac in (0.25, 0.75):    # 0.25: the midpoint is outside, 0.75: only the end point
                for _ in range(6):
                    p = list(rng.uniform(-0.45, 0.45, dim)) + [0.]*(3 - dim)
                    for a in S:
                        p[a] = s*(0.5 - frac*step*rng.uniform(0.95, 1.05))
                    pts.append(p)
    for _ in range(60):                  # inside, anywhere
        pts.append(list(rng.uniform(-0.5, 0.5, dim)) + [0.]*(3 - dim))
    for k in range(1, dim + 1):          # on the downstream sides, edges and corner of the box
        for S in itertools.combinations(range(dim), k):
            p = list(rng.uniform(-0.45, 0.45, dim)) + [0.]*(3 - dim)
            for a in S:
                p[a] = s*0.5
            pts.append(p)
    for a in range(dim):                 # outside from the start
        p = list(rng.uniform(-0.45, 0.45, dim)) + [0.]*(3 - dim)
        p[a] = -s*0.50001
        pts.append(p)
    pos = np.array(pts, dtype=np.float64)
    assert len(pos) <= 512
    ids = np.arange(1, len(pos) + 1, dtype=np.uint32)
    pos.setflags(write=False)
    ids.setflags(write=False)
    return pos, ids


@functools.lru_cache(None)
def reference_events(dim, level, sides_name, field_name):
    """the state of the list after each of NEVENTS events, from the restatement: tuples of
    (positions, old positions, ids) as arrays.  Raises IntersectionFailed where the reference is
    undefined."""
    pos, ids = tracer_particles(dim, level, field_name)
    states = R.list_event(box(dim, level), tracer_field(dim, level, field_name), pos.tolist(), ids.tolist(),
                          tracer_dt(level), SIDES[sides_name], nevents=NEVENTS)
    out = []
    for p, po, i in states:
        out.append((np.array(p, dtype=np.float64).reshape(-1, 3), np.array(po, dtype=np.float64).reshape(-1, 3),
                    np.array(i, dtype=np.uint32)))
    return out


def first_event_outcomes(dim, level, field_name):
    """what the first event does to every particle of the list: 'removed' (outside from the start),
    'stuck' (midpoint outside), 'inside', or 'out1' / 'out2' / 'out3' (end point outside along that
    many axes)"""
    b = box(dim, level)
    u = [b.field(a) for a in tracer_field(dim, level, field_name)]
    dt = tracer_dt(level)
    res = []
    for p in tracer_particles(dim, level, field_name)[0].tolist():
        cell = b.locate(p)
        if cell is None:
            res.append("removed")
            continue
        mid = [p[c] + (dt*b.interpolate(cell, p, u[c])/2. if c < dim else 0.) for c in range(3)]
        if b.locate(mid) is None:
            res.append("stuck")
            continue
        q = b.advect_point(u, p, dt)
        nout = sum(abs(q[c]) > 0.5 for c in range(dim))
        res.append("inside" if nout == 0 else "out%d" % nout)
    return res
