"""The inputs of the tests of GfsSourceParticulateVol / GfsSourceParticulateMass, shared by
test_particulate_sources_reference_cpu.py (the restatement and the premises of the cases) and
test_gpu_particulate_sources.py (the device against the restatement).  References are computed once per
process (functools caches) and never modified.

One run of a case, on the device and in the restatement alike:
  events 0, 1, 2   on the list as created (`static'): a new velocity, a later time and another dt before each;
                   the device sorts its storage (gfship_particles_sort) after event 0;
  the move         one gfs_particle_list_event of the list, whose only force is a GfsForceBuoy without gravity:
                   every particle flies pos += vel*dt/2, twice (modules/particulatecommon.c:826-833); the
                   particle outside the box leaves the list (remove_particles_not_in_domain, :955-969);
  events 3, 4      on the moved list; the device sorts again after event 3.
The second sort is what makes the storage order of a cell differ from its list order: a sort is stable, so the
particles of one cell stay in the order the sort before left them in -- the order of the cells they were in
then.  The particles SHARED sit in cells of falling number when the list is created and fly into one cell.
"""
import collections
import functools
import math

import numpy as np

import forces_cases as FK
import particulate_sources_reference as PS
import sampler_cases as SK
import sampler_reference as R

BOXES = [(2, 3), (2, 4), (3, 3)]
SIDE_NAMES = ("periodic", "closed")
SIDES = {k: SK.SIDES[k] for k in SIDE_NAMES}
NPART = 40
SHARED = (3, 11, 19, 27)        # fly into one cell; interleaved in list order with particles of other cells
SHARED_STATIC = (5, 13, 21)     # share a cell from the start and do not move
ON_FACE, IN_CORNER, OUTSIDE = 7, 9, 15
SENTINEL = -7.5
T0, DT_MOVE = 0.25, 2.**-5
EVENT_DT = (2.**-7, 0.0061, 0.011, 0.0078125, 0.0049)
EVENT_T = (T0, T0 + 0.03, T0 + 0.07, T0 + 0.11, T0 + 0.2)
NEVENTS = 5
MOVE_BEFORE = 3                 # the list event comes before this source event
SORT_AFTER = (0, 3)             # the device sorts its storage after these source events
RAD_STEP = 0.01                 # the threshold of the function `step'
# the random numbers of each case: seeds for which the sums of the shared cell depend on the order of the
# additions in every event after the move (test_premise_of_the_order_tests asserts that they do)
SEEDS = {(2, 3, "periodic"): 9137, (2, 3, "closed"): 9137, (2, 4, "periodic"): 9142, (2, 4, "closed"): 9142,
         (3, 3, "periodic"): 9182, (3, 3, "closed"): 9182}

# name -> (C text, the same function for the restatement, the variables it names)
FUNCTIONS = collections.OrderedDict([
    ("constant", ("2.5e-7", lambda V: 2.5e-7, ())),
    ("tracer", ("1e-3*T*(Urelp*Urelp + Vrelp*Vrelp)",
                lambda V: 1e-3*V["T"]*(V["Urelp"]*V["Urelp"] + V["Vrelp"]*V["Vrelp"]), ("T",))),
    ("xyt", ("1e-6*(1. + x) + 1e-7*y*t + 1e-7*z",
             lambda V: 1e-6*(1. + V["x"]) + 1e-7*V["y"]*V["t"] + 1e-7*V["z"], ())),
    ("block", ("{ double a = Urelp*Vrelp; if (a > 0.) return 2e-6*a; return -1e-7*a; }",
               lambda V: 2e-6*(V["Urelp"]*V["Vrelp"]) if V["Urelp"]*V["Vrelp"] > 0.
               else -1e-7*(V["Urelp"]*V["Vrelp"]), ())),
    # a function of Rad that cannot feel an ulp: every radius of the cases is far from RAD_STEP (asserted)
    ("step", ("Rad > 0.01 ? 1e-5 : 1e-8", lambda V: 1e-5 if V["Rad"] > RAD_STEP else 1e-8, ())),
])
NO_LIBM = ("constant", "tracer", "xyt", "block")


def cell_number(dim, level, cell):
    """the linear number of a leaf (i fastest), the order of the sort keys"""
    n = 1 << level
    i, j, k = cell.ijk
    return (i - 1) + n*((j - 1) + (n*(k - 1) if dim == 3 else 0))


@functools.lru_cache(None)
def particles(dim, level, sides_name):
    """(pos, ids, vel, mass, volume) of the list as created"""
    rng = np.random.default_rng(SEEDS[dim, level, sides_name])
    n = 1 << level
    h = 1./n
    pos = 0.9*(rng.random((NPART, 3)) - 0.5)
    vel = rng.uniform(-1., 1., (NPART, 3))
    mid = n//2

    def centre(i, j, k):
        return np.array([-0.5 + (i - 0.5)*h, -0.5 + (j - 0.5)*h, -0.5 + (k - 0.5)*h])
    # SHARED: cells of falling number along a row, all flying into the cell (2, mid, mid)
    target = centre(2, mid, mid)
    for q, o in enumerate(SHARED):
        pos[o] = centre(n - 1 - q, mid, mid) + (rng.random(3) - 0.5)*0.5*h
        vel[o] = (target + (rng.random(3) - 0.5)*0.5*h - pos[o])/DT_MOVE
    for o in SHARED_STATIC:
        pos[o] = centre(mid + 1, mid + 2, mid - 1) + (rng.random(3) - 0.5)*0.8*h
        vel[o] = 0.
    pos[ON_FACE] = [-0.5 + 3*h, -0.5 + 2.25*h, -0.5 + 1.5*h]      # on the face between cells 3 and 4 along x
    pos[IN_CORNER] = centre(1, 1, 1) + 0.2*h
    vel[ON_FACE] = vel[IN_CORNER] = 0.
    if sides_name == "closed":
        pos[OUTSIDE] = [0.7, 0.1, -0.2]
    # two groups of volumes: radii near 1e-3 and near 4e-2, RAD_STEP between them
    volume = np.where(np.arange(NPART) % 2 == 0, 10.**rng.uniform(-4., -3., NPART), 10.**rng.uniform(-9., -7., NPART))
    mass = volume*(0.5 + 2.5*rng.random(NPART))
    if dim == 2:
        pos[:, 2] = 0.
        vel[:, 2] = 0.
    ids = np.arange(1, NPART + 1, dtype=np.uint32)
    for a in (pos, ids, vel, mass, volume):
        a.setflags(write=False)
    return pos, ids, vel, mass, volume


def velocity(dim, level, e):
    """the velocity of the fluid at source event e: arrays with ghosts"""
    return FK.velocity(dim, level, e)


@functools.lru_cache(None)
def tracer(dim, level):
    a = SK.distinct_field(dim, level, salt=91)
    a.setflags(write=False)
    return a


Event = collections.namedtuple("Event", "volume mass deposit rad urel sources cells")
Run = collections.namedtuple("Run", "events moved_pos moved_vel storage")


def move(box, plist, dt):
    """gfs_particle_list_event of a list whose forces add up to nothing: remove_particles_not_in_domain
    (:955-969), then pos += vel*dt/2, vel += 0.*dt/mass, pos += vel*dt/2 (:826-833); nobody leaves the box"""
    plist = [p for p in plist if box.locate(p.pos) is not None]
    for p in plist:
        for c in range(box.dim):
            p.pos[c] += p.vel[c]*dt/2.
            p.vel[c] += 0.*dt/p.mass
            p.pos[c] += p.vel[c]*dt/2.
        assert box.locate(p.pos) is not None
    return plist


@functools.lru_cache(None)
def reference_run(dim, level, sides_name, kind, fname, pow_=math.pow, deposit=True):
    box = SK.box(dim, level)
    pos, ids, vel, mass, volume = particles(dim, level, sides_name)
    plist = [PS.Particulate(pos[q], vel[q], mass[q], volume[q]) for q in range(NPART)]
    text, fn, names = FUNCTIONS[fname]
    variables = {"T": box.field(tracer(dim, level))} if "T" in names else {}
    fields = PS.Fields(dim, deposit)
    events = []
    nmax = 1 << 62
    keys = []       # the cell numbers at the time of each sort of the device, per creation slot
    for e in range(NEVENTS):
        if e == MOVE_BEFORE:
            plist = move(box, plist, DT_MOVE)
        u = [box.field(a) for a in velocity(dim, level, e)]
        src = PS.event(box, kind, plist, u, EVENT_DT[e], EVENT_T[e], fn, fields, variables, pow_)
        cells = [box.locate(p.pos) for p in plist]
        events.append(Event(np.array([p.volume for p in plist]), np.array([p.mass for p in plist]),
                            None if fields.deposit is None else PS.arrays(box, fields.deposit, 0.),
                            PS.arrays(box, fields.rad, SENTINEL),
                            [PS.arrays(box, d, SENTINEL) for d in fields.urel], src,
                            [None if c is None else cell_number(dim, level, c) for c in cells]))
        if e in SORT_AFTER:
            keys.append(events[-1].cells)
    # the storage order after the two sorts: stable sorts by cell of the slots in their order so far; the
    # particle outside (on the list at the first sort, off it at the second) sorts last
    on_list = on_list_after_move(sides_name)
    assert len(on_list) == len(plist)
    first = dict(zip(range(NPART), keys[0]))
    order = sorted(range(NPART), key=lambda q: nmax if first[q] is None else first[q])
    second = dict(zip(on_list, keys[1]))
    order = sorted(order, key=lambda q: second.get(q, nmax))
    storage = [q for q in order if q in second]
    return Run(events, np.array([p.pos for p in plist]), np.array([p.vel for p in plist]), storage)


def on_list_after_move(sides_name):
    """the creation slots still on the list after the move"""
    return [q for q in range(NPART) if sides_name != "closed" or q != OUTSIDE]
