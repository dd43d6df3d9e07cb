"""The inputs of the tests of GfsSourceParticulateVol / GfsSourceParticulateMass on refined trees, shared by
test_tree_particulate_sources_reference_cpu.py (the restatement and the premises of the cases) and
test_gpu_tree_particulate_sources.py (the device against the restatement).  References are computed once per
process (functools caches) and never modified.

The trees are those of tests/tree_two_way_cases.py.  One run of a case, on the device and in the restatement alike:
  event 0        on the list as created; the device sorts its storage (gfship_particles_sort) after it;
  event 1        with another velocity, a later time and another dt (a Tree.step on the device);
  sort, the move, sort
                 one gfs_particle_list_event of the list, whose only force is a GfsForceBuoy without gravity: every
                 particle flies pos += vel*dt/2, twice (modules/particulatecommon.c:826-833), with the dt of event 1;
  event 2        on the moved list, again with another velocity, time and dt.
A sort is stable, so the particles of one leaf stay in the order the sort before left them in -- the order of the
leaves they were in then.  The particles FLY sit in leaves of falling index when the list is created and fly into
one leaf: after the second sort they are stored in the reverse of their list order.

The fluid of every event is a `stage' (u, t, dt).  Without a device the stages are HOST_STAGES below; the GPU test
registers the velocities, times and time steps its tree goes through (register_stages) and the restatement runs on
those.  The velocity of the FLY particles needs the dt of the move, which is why `particles' takes it.
"""
import collections
import functools
import math

import numpy as np

import forces_reference as F
import tree_forces_reference as TF
import tree_particulate_sources_reference as PS
import tree_sampler_cases as TC
import tree_sampler_reference as T
import tree_two_way_cases as C

ALL, REFINED = C.ALL, C.REFINED
UNIFORM = {2: 3, 3: 3}          # the levels of the uniform trees that are compared with the box
NEVENTS = 3
MOVE_BEFORE = 2                 # sort, list event, sort come before this source event
SORT_AFTER = (0,)
TARGET = 90
SEED = 4711
# the random numbers of each tree: seeds for which the sums of the shared leaf depend on the order of the additions
# (test_premises_of_the_order_tests asserts that they do)
SEEDS = {"uniform2": 4720, "square": 4711, "graded": 4711, "walls2": 4714, "cube": 4712, "box3": 4714, "ell": 4711,
         "uniform3d": 4711}
RAD_STEP = 0.01                 # the threshold of the function `block'
HOST_T = (0.25, 0.28, 0.32)
HOST_DT = (2.**-7, 0.0061, 0.011)
HOST_SCALE = (1., 0.75, 1.25)

Particles = collections.namedtuple("Particles", "pos ids vel mass volume fine coarse fly on_face on_side outside "
                                   "fine_leaf coarse_leaf fly_leaf")
Stage = collections.namedtuple("Stage", "u t dt")
Event = collections.namedtuple("Event", "ids volume mass deposit rad urel sources leaves")
Run = collections.namedtuple("Run", "events storage moved_pos")


def functions(dim):
    """name -> (C text, the same function for the restatement, the variables it names).  All of them are positive
    and small: the volumes only grow, by less than a millionth of the smallest, so that no radius comes near
    RAD_STEP (test_tree_particulate_sources_reference_cpu.py asserts it)"""
    w = " + Wrelp*Wrelp" if dim == 3 else ""

    def rel2(V):
        s = V["Urelp"]*V["Urelp"] + V["Vrelp"]*V["Vrelp"]
        return s + V["Wrelp"]*V["Wrelp"] if dim == 3 else s

    def block(V):
        a = V["Urelp"]*V["Vrelp"]
        if V["Rad"] > RAD_STEP:
            return 2e-11*a if a > 0. else -1e-12*a
        return 1e-13

    return collections.OrderedDict([
        ("constant", ("2.5e-12", lambda V: 2.5e-12, ())),
        ("tracer", ("1e-11*T*(Urelp*Urelp + Vrelp*Vrelp%s)" % w, lambda V: 1e-11*V["T"]*rel2(V), ("T",))),
        # x, y, z are the centre of the leaf: they tell the levels apart
        ("xyt", ("1e-11*(1. + x) + 1e-12*y*t + 1e-12*z",
                 lambda V: 1e-11*(1. + V["x"]) + 1e-12*V["y"]*V["t"] + 1e-12*V["z"], ())),
        # a branch, and a step of Rad that cannot feel an ulp
        ("block", ("{ double a = Urelp*Vrelp; if (Rad > 0.01) { if (a > 0.) return 2e-11*a; return -1e-12*a; } "
                   "return 1e-13; }", block, ())),
    ])


FUNCTION_NAMES = ("constant", "tracer", "xyt", "block")
ORDER_SENSITIVE = ("tracer", "block")       # their sources differ from particle to particle of one leaf


def host_tree(name):
    if name.startswith("uniform3d"):
        return _uniform(3)
    return C.host_tree(name)


@functools.lru_cache(None)
def _uniform(dim):
    return T.TreeBox.uniform(dim, UNIFORM[dim])


def spec(name):
    if name.startswith("uniform3d"):
        return 3, (lambda x, y, z: UNIFORM[3]), [C.P]*6
    return C.spec(name)


def offsets(box):
    off = [0]
    for l in range(box.level + 1):
        off.append(off[-1] + ((1 << l) + 2)**box.dim)
    return off


def leaf_index(box, cell):
    """the index of a cell in the concatenated dense levels: the order of the sort keys"""
    r = (1 << cell.level) + 2
    i, j, k = cell.ijk
    return offsets(box)[cell.level] + i + r*(j + (r*k if box.dim == 3 else 0))


def centres(dim, level):
    n = 1 << level
    c = -0.5 + (np.arange(n + 2) - 0.5)/n
    if dim == 2:
        return np.meshgrid(c, c, indexing="xy")
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    return x, y, z


def _row_of_leaves(box):
    """a leaf T and three leaves of its level next to each other beyond it along x, of the coarsest level that has
    such a row: (T, [the three, the farthest first])"""
    for cell in sorted(box.leaves, key=lambda c: (c.level, c.ijk[2], c.ijk[1], c.ijk[0])):
        i, j, k = cell.ijk
        row = [box.by_ijk.get((cell.level, (i + m, j, k))) for m in (3, 2, 1)]
        if all(c is not None for c in row):
            return cell, row
    raise AssertionError("no row of four leaves")


@functools.lru_cache(None)
def particles(name, dt_move):
    """the list as created.  About TARGET of TC.seeds, taken as tree_two_way_cases.spread_particles takes them (next
    to the faces and corners of leaves of every level, `dim' of them outside the box), and in between, far apart in
    the list: three particles in one fine leaf and two in one coarse leaf that do not move, the three FLY, one
    particle on a face between two levels and one on a box side"""
    box = host_tree(name)
    dim = box.dim
    rng = np.random.default_rng(SEEDS.get(name, SEED))
    seeds, _ = TC.seeds(box, 3)
    step = max(1, len(seeds)//TARGET)
    regular = [list(p) for p in seeds[::step][:-1]]
    outside = [list(p) for p in seeds[-dim:]]

    def inside(cell, spread):
        h = box.cell_size(cell)
        return [cell.pos[a] + rng.uniform(-spread, spread)*h if a < dim else 0. for a in range(3)]
    target, row = _row_of_leaves(box)
    taken = set(id(c) for c in [target] + row)
    free = [c for c in box.leaves if id(c) not in taken]
    fine_leaf = max(free, key=lambda c: (c.level, c.pos))
    coarse_leaf = min((c for c in free if c is not fine_leaf), key=lambda c: (c.level, c.pos))
    fine = [inside(fine_leaf, 0.4) for _ in range(3)]
    coarse = [inside(coarse_leaf, 0.4) for _ in range(2)]
    fly = [inside(c, 0.25) for c in row]
    land = [inside(target, 0.25) for _ in row]
    face = None
    for c in box.leaves:                                    # the face of a leaf whose neighbour is coarser
        nb = box.neighbor(c, 0)
        if nb is not None and not nb.boundary and nb.level < c.level:
            face = [c.pos[a] if a < dim else 0. for a in range(3)]
            face[0] = c.pos[0] + box.cell_size(c)/2.
            break
    if face is None:                                        # a uniform tree: a face between two leaves
        c = box.leaves[len(box.leaves)//2]
        face = [c.pos[a] if a < dim else 0. for a in range(3)]
        face[0] = c.pos[0] + box.cell_size(c)/2. if c.pos[0] < 0. else c.pos[0] - box.cell_size(c)/2.
    side = [0.]*3
    side[0], side[1] = 0.5, 0.1875 + 1./1024.
    third = len(regular)//3
    entries = []                                            # (position, kind)
    entries += [(fine[0], "fine"), (coarse[0], "coarse"), (fly[0], "fly0")]
    entries += [(p, "regular") for p in regular[:third]]
    entries += [(fine[1], "fine"), (fly[1], "fly1")]
    entries += [(p, "regular") for p in regular[third:2*third]]
    entries += [(coarse[1], "coarse"), (fine[2], "fine"), (fly[2], "fly2")]
    entries += [(p, "regular") for p in regular[2*third:]]
    entries += [(face, "face"), (side, "side")] + [(p, "outside") for p in outside]
    n = len(entries)
    pos = np.array([e[0] for e in entries], dtype=np.float64)
    kinds = [e[1] for e in entries]
    vel = np.zeros((n, 3))
    vel[:, :dim] = rng.uniform(-0.3, 0.3, (n, dim))
    for q, k in enumerate(kinds):
        if k in ("fine", "coarse", "face", "side"):
            vel[q] = 0.
        elif k.startswith("fly"):
            m = int(k[3])
            vel[q] = (np.array(land[m]) - pos[q])/dt_move
    # two groups of volumes: radii near 4e-2 and near 1e-3, RAD_STEP between them
    volume = np.where(np.arange(n) % 2 == 0, 10.**rng.uniform(-4., -3., n), 10.**rng.uniform(-9., -7., n))
    mass = volume*(0.5 + 2.5*rng.random(n))
    ids = np.arange(1, n + 1, dtype=np.uint32)
    for a in (pos, ids, vel, mass, volume):
        a.setflags(write=False)

    def where(k):
        return tuple(q for q, x in enumerate(kinds) if x.startswith(k))
    return Particles(pos, ids, vel, mass, volume, where("fine"), where("coarse"), where("fly"), where("face")[0],
                     where("side")[0], where("outside"), fine_leaf, coarse_leaf, target)


HELD_SALT = {"rad": 1, "urel0": 2, "urel1": 3, "urel2": 4, "deposit": 5}


def shapes(box):
    return [((1 << l) + 2,)*box.dim for l in range(box.level + 1)]


@functools.lru_cache(None)
def held(name, salt):
    """what a variable holds before the first event: a distinct dyadic value per cell of every level (ghost cells
    and the cells a level does not have included), between 1/16 and 1/2 -- times 2^-36 for the deposit, the size of
    the sources: a running sum much larger than its addends rounds each of them on its own and does not depend on
    their order"""
    out = []
    base = 1 << 16
    scale = 2.**-36 if salt == HELD_SALT["deposit"] else 1.
    for l, s in enumerate(shapes(host_tree(name))):
        idx = np.arange(int(np.prod(s)), dtype=np.float64).reshape(s)
        a = scale*(base + 7.*idx + 131.*salt + 1031.*l)/(1 << 20)
        a.setflags(write=False)
        base += 7*int(np.prod(s)) + 2048
        out.append(a)
    return out


@functools.lru_cache(None)
def tracer(name):
    box = host_tree(name)
    flags = [np.array(box.flags(l), dtype=np.uint8) for l in range(box.level + 1)]
    out = [np.nan_to_num(a, nan=0.) for a in TC.distinct_values(box.dim, flags, salt=91)]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(None)
def host_stages(name):
    box = host_tree(name)
    dim = box.dim
    vname = "cube" if name.startswith("uniform3d") else "square" if name == "ell" else name
    stages = []
    for e in range(NEVENTS):
        u = []
        for l, s in enumerate(shapes(box)):
            u.append([np.ascontiguousarray(np.broadcast_to(HOST_SCALE[e]*a, s))
                      for a in TC.initial_velocity(vname, centres(dim, l))])
        stages.append(Stage([[u[l][c] for l in range(box.level + 1)] for c in range(dim)], HOST_T[e], HOST_DT[e]))
    return tuple(stages)


STAGES = {}


def register_stages(name, stages):
    """the stages a device tree went through: [(u[c][level] arrays, t, dt)]*NEVENTS, kept as they are"""
    STAGES[name] = tuple(Stage(*s) for s in stages)


def stages(name, where):
    return host_stages(name) if where == "host" else STAGES[name]


def move(box, sides, stage, plist):
    """gfs_particle_list_event of a list whose only force is a GfsForceBuoy without gravity"""
    sim = F.Sim(box, sides, stage.u, stage.dt, g=(0., 0., 0.), root=F.sqrt_root)
    return TF.list_event(sim, plist, [F.ForceCoeff(F.BUOY)])


def new_fields(name, box, deposit=True, zero_deposit=False):
    def var(key):
        return box.field([np.array(a) for a in held(name, HELD_SALT[key])])
    dep = None
    if deposit:
        dep = box.field([np.zeros(s) for s in shapes(box)]) if zero_deposit else var("deposit")
    return PS.Fields(var("rad"), [var("urel%d" % c) for c in range(box.dim)], dep)


def levels(box, v):
    return [np.array(a, dtype=np.float64) for a in v]


@functools.lru_cache(None)
def reference_run(name, kind, fname, where="host", pow_=math.pow, deposit=True, zero_deposit=False):
    box = host_tree(name)
    dim, _refine, sides = spec(name)
    st = stages(name, where)
    P = particles(name, st[MOVE_BEFORE - 1].dt)
    plist = [F.Particulate(P.pos[q], P.ids[q], P.vel[q], P.mass[q], P.volume[q]) for q in range(len(P.ids))]
    text, fn, names = functions(dim)[fname]
    variables = {"T": box.field(tracer(name))} if "T" in names else {}
    fields = new_fields(name, box, deposit, zero_deposit)
    events, keys = [], []
    moved_pos = None
    for e in range(NEVENTS):
        if e == MOVE_BEFORE:
            keys.append({p.id: box.locate(p.pos) for p in plist})
            plist = move(box, sides, st[e - 1], plist)
            moved_pos = np.array([p.pos for p in plist])
            keys.append({p.id: box.locate(p.pos) for p in plist})
        u = [box.field(a) for a in st[e].u]
        src = PS.event(box, kind, plist, u, st[e].dt, st[e].t, fn, fields, variables, pow_)
        events.append(Event(np.array([p.id for p in plist], dtype=np.uint32),
                            np.array([p.volume for p in plist]), np.array([p.mass for p in plist]),
                            None if fields.deposit is None else levels(box, fields.deposit),
                            levels(box, fields.rad), [levels(box, v) for v in fields.urel], src,
                            [box.locate(p.pos) for p in plist]))
    # the storage order after the sorts: stable sorts by leaf of the slots in their order so far; a particle without
    # a leaf, or off the list, sorts last
    big = 1 << 62
    order = [int(i) for i in P.ids]
    for k in keys:
        order = sorted(order, key=lambda i: big if k.get(i) is None else leaf_index(box, k[i]))
    on_list = set(int(i) for i in events[-1].ids)
    return Run(events, [i for i in order if i in on_list], moved_pos)


def in_leaf(box, event, leaf):
    """the positions in the list of `event' of the particles in `leaf'"""
    return [q for q, c in enumerate(event.leaves) if c is leaf]
