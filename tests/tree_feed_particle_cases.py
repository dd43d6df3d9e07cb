"""The inputs of the tests of GfsFeedParticle on refined trees, shared by test_tree_feed_particle_reference_cpu.py
(the premises of the cases, the id rule) and test_gpu_tree_feed_particle.py (the device against the restatement of
tests/feed_particle_reference.py, which runs on a tree_sampler_reference.TreeBox as it stands).  References are
computed once per process (functools caches) and never modified.

The trees are the refined ones of tests/tree_two_way_cases.py and the two uniform trees of level 3.  One run of a
case: a list of NPART particulates (ids 1 .. NPART) with idlast = IDLAST0, then one feed event per entry of COUNTS
on the same list, each with candidates, a velocity of the fluid and a time of its own: a `stage' (u, t).  Without a
device the stages are host_stages below; the GPU test registers the velocities and times its tree goes through
(register_stages) and the restatement runs on those.
"""
import collections
import functools
import itertools

import numpy as np

import feed_particle_cases as FC
import feed_particle_reference as FP
import forces_reference as FR
import sampler_reference as R
import tree_particulate_sources_cases as K
import tree_sampler_cases as TC
import tree_two_way_cases as C

REFINED = C.REFINED
UNIFORM = ("uniform2", "uniform3d")
TREES = REFINED + UNIFORM
NPART = 40
IDLAST0 = FC.IDLAST0
COUNTS = FC.COUNTS                      # 0, 1, 70, 300, 3000: the third makes the arrays grow, the last spans twelve blocks
FUNCTIONS = FC.FUNCTIONS                # constants, the tracer T at the leaf, x y z t, a { block } with a branch
PREMISE = FC.PREMISE                    # the function the placed candidates are built for
State, state_of, feed_of = FC.State, FC.state_of, FC.feed_of
Stage = collections.namedtuple("Stage", "u t")
HOST_SCALE = (1., 0.75, 1.25, 0.5, 1.5)

# the candidates placed by hand in every event of 70 candidates or more
IN_LEVEL = (2, 3, 4)                    # in a leaf of every level of the tree (repeated where it has fewer)
ON_FACE, ON_CORNER = 5, 6               # on a face between a fine and a coarse leaf; on a corner where the level changes
IN_TABLE, IN_UNIFORM = 7, 8             # a leaf whose corner interpolators hold another level; one that sees its own only
ON_SIDE = 9                             # exactly on a side of the box: inside
OUT_X, OUT_LAST = 10, 11                # just outside the +x side and the + side of the last axis: no cell
SHARED, BETWEEN = (20, 22), 21          # two accepted candidates in one leaf and a massless one between them

host_tree, spec, tracer, shapes = K.host_tree, K.spec, K.tracer, K.shapes


def corner_levels(box, cell):
    """the levels of the cells in the interpolators of the corners of a leaf"""
    return set(c.level for d in R.CORNER[box.dim] for c, _w in box.corner_interpolator(cell, d))


def touches_a_side(box, cell):
    h = box.cell_size(cell)
    return any(abs(abs(cell.pos[a]) + h/2. - 0.5) < 1e-12 for a in range(box.dim))


Placed = collections.namedtuple("Placed", "level_leaves face_leaf corner table_leaf uniform_leaf shared_leaf between_leaf")


@functools.lru_cache(None)
def placed(name):
    """the leaves and points the placed candidates are built on"""
    box = host_tree(name)
    dim = box.dim
    leaves = sorted(box.leaves, key=lambda c: (c.level, c.ijk[2], c.ijk[1], c.ijk[0]))
    inner = [c for c in leaves if not touches_a_side(box, c)]
    levels = sorted(set(c.level for c in leaves))
    level_leaves = tuple(next(c for c in leaves if c.level == levels[q % len(levels)]) for q in range(len(IN_LEVEL)))
    face_leaf = corner = None
    for c in leaves:                                        # a leaf whose neighbour along +x is coarser
        nb = box.neighbor(c, 0)
        if nb is not None and not nb.boundary and nb.level < c.level:
            face_leaf = c
            break
    if face_leaf is None:                                   # a uniform tree: a face between two leaves
        face_leaf = inner[len(inner)//2]
    inner = inner or leaves
    h = box.cell_size(face_leaf)
    corner = tuple(face_leaf.pos[a] + h/2. if a < dim else 0. for a in range(3))
    table_leaf = next((c for c in inner if len(corner_levels(box, c)) > 1), None)
    uniform_leaf = next(c for c in inner + leaves if corner_levels(box, c) == {c.level})
    shared_leaf = next(c for c in reversed(inner) if c.pos[0] < 0.1)          # the finest such leaf
    between_leaf = next(c for c in inner if c.pos[0] > 0.1)
    return Placed(level_leaves, face_leaf, corner, table_leaf, uniform_leaf, shared_leaf, between_leaf)


@functools.lru_cache(None)
def candidates(name, e):
    """the positions of the candidates of event e, an (COUNTS[e], 3) array: a quarter of the random ones lies outside
    the box, whatever its sides are"""
    count = COUNTS[e]
    box = host_tree(name)
    dim = box.dim
    rng = np.random.default_rng(8100 + 100*e + sum(map(ord, name)))
    pos = 1.25*(rng.random((count, 3)) - 0.5)

    def inside(cell, frac):
        return [cell.pos[a] + frac*box.cell_size(cell) if a < dim else 0. for a in range(3)]
    if count >= 70:
        P = placed(name)
        for q, c in zip(IN_LEVEL, P.level_leaves):
            pos[q] = inside(c, 0.2)
        c = P.face_leaf
        pos[ON_FACE] = inside(c, 0.125)
        pos[ON_FACE, 0] = c.pos[0] + box.cell_size(c)/2.
        pos[ON_CORNER] = P.corner
        pos[IN_TABLE] = inside(P.table_leaf if P.table_leaf is not None else P.uniform_leaf, -0.3)
        pos[IN_UNIFORM] = inside(P.uniform_leaf, 0.3)
        pos[ON_SIDE] = [0.5, 0.1875 + 1./1024., 0.0625 + 1./512.]
        pos[OUT_X] = [0.5 + 2.**-20, 0.21, -0.13]
        pos[OUT_LAST] = [-0.17, 0.23, 0.11]
        pos[OUT_LAST, dim - 1] = 0.5 + 2.**-20
        for q, o in enumerate(SHARED):
            pos[o] = inside(P.shared_leaf, 0.1 + 0.2*q)
        pos[BETWEEN] = inside(P.between_leaf, -0.1)
    if dim == 2:
        pos[:, 2] = 0.
    pos.setflags(write=False)
    return pos


@functools.lru_cache(None)
def particles(name):
    """the list as created: NPART particulates inside the box"""
    dim = spec(name)[0]
    rng = np.random.default_rng(8000 + sum(map(ord, name)))
    pos = np.zeros((NPART, 3))
    pos[:, :dim] = rng.uniform(-0.45, 0.45, (NPART, dim))
    vel = np.zeros((NPART, 3))
    vel[:, :dim] = 0.8 + rng.uniform(-0.4, 0.4, (NPART, dim))
    volume = 10.**rng.uniform(-5., -4., NPART)
    mass = volume*rng.uniform(0.5, 2., NPART)
    ids = np.arange(1, NPART + 1, dtype=np.uint32)
    for a in (pos, ids, vel, mass, volume):
        a.setflags(write=False)
    return pos, ids, vel, mass, volume


def event_time(e):
    return FC.event_time(e)


@functools.lru_cache(None)
def host_stages(name):
    """a velocity (every level, ghost cells included) and a time per event"""
    box = host_tree(name)
    dim = box.dim
    vname = "cube" if name == "uniform3d" else "square" if name == "ell" else name
    stages = []
    for e in range(len(COUNTS)):
        u = [[np.ascontiguousarray(np.broadcast_to(HOST_SCALE[e]*a, s))
              for a in TC.initial_velocity(vname, K.centres(dim, l))] for l, s in enumerate(shapes(box))]
        stages.append(Stage([[u[l][c] for l in range(box.level + 1)] for c in range(dim)], event_time(e)))
    return tuple(stages)


STAGES = {}


def register_stages(name, where, stages):
    """the stages a device tree went through in the test `where': [(u[c][level] arrays, t)] per event, kept as they
    are.  The steps of a tree are deterministic: a second registration changes nothing"""
    assert where != "host"
    if (name, where) not in STAGES:
        STAGES[name, where] = tuple(Stage(*s) for s in stages)


def stages(name, where):
    return host_stages(name) if where == "host" else STAGES[name, where]


def initial_list(name):
    pos, ids, vel, mass, volume = particles(name)
    return FP.ParticleList([FR.Particulate(pos[q], ids[q], vel[q], mass[q], volume[q]) for q in range(NPART)], IDLAST0)


@functools.lru_cache(None)
def _cached_box(name):
    return FC.CachedBox(host_tree(name))


@functools.lru_cache(None)
def _fields(name, where):
    """the stages as TreeBox.field () lists (the same objects for every function: CachedBox remembers per object)"""
    box = _cached_box(name)
    return tuple([box.field(a) for a in st.u] for st in stages(name, where)), box.field(tracer(name))


def feed_events(name, fname, events, where="host"):
    """the list after each of the feed events `events' (indices into COUNTS) in a row: (the list, its states)"""
    box = _cached_box(name)
    u, T = _fields(name, where)
    st = stages(name, where)
    pl = initial_list(name)
    variables = {"T": T} if "T" in FUNCTIONS[fname][2] else {}
    states = []
    for e in events:
        out = FP.event(box, u[e], pl, feed_of(fname, candidates(name, e), st[e].t), st[e].t, variables)
        states.append(state_of(pl, out))
    return pl, states


@functools.lru_cache(None)
def reference_run(name, fname, where="host"):
    """the state of the list after every event of COUNTS"""
    return tuple(feed_events(name, fname, range(len(COUNTS)), where)[1])


def leaves_around(box, p):
    """the leaves that hold the points next to p on every side of it"""
    eps = 2.**-30
    out = []
    for s in itertools.product((-eps, eps), repeat=box.dim):
        c = box.locate([float(p[a]) + s[a] if a < box.dim else 0. for a in range(3)])
        if c is not None and all(c is not o for o in out):
            out.append(c)
    return out
