"""The inputs of the tests of GfsFeedParticle, shared by test_feed_particle_reference_cpu.py (the premises of the
cases) and test_gpu_feed_particle.py (the device against the restatement of feed_particle_reference.py).
References are computed once per process (functools caches) and never modified.

One run of a case: the list of particulate_sources_cases.particles (40 particulates, ids 1 .. 40) with idlast =
IDLAST0, then one feed event per entry of COUNTS on the same list, each with candidates, a velocity of the fluid
and a time of its own.  Every event therefore starts from the idlast the one before left.
"""
import collections
import functools

import numpy as np

import feed_particle_reference as FP
import forces_cases as FK
import forces_reference as FR
import particulate_sources_cases as K
import sampler_cases as SK

BOXES = K.BOXES
SIDE_NAMES = K.SIDE_NAMES
SIDES = K.SIDES
IDLAST0 = 100
COUNTS = (0, 1, 70, 300, 3000)          # 3000: twelve blocks of 256 candidates
T0 = 0.25
# the candidates placed by hand in every event of 70 candidates or more
ON_FACE, IN_CORNER = 5, 9
SHARED, BETWEEN = (20, 22), 21          # two accepted candidates in one cell and a massless one between them
PREMISE = "block"                       # the function the placed candidates are built for

# name -> ((mass, volume) as C text, the same two functions for the restatement, the variables they name)
FUNCTIONS = collections.OrderedDict([
    ("constant", (("2.5e-4", "1e-4"), (lambda V: 2.5e-4, lambda V: 1e-4), ())),
    ("tracer", (("1e-3*(T - 0.9)", "1e-4*T"),
                (lambda V: 1e-3*(V["T"] - 0.9), lambda V: 1e-4*V["T"]), ("T",))),
    ("xyt", (("1e-3*(x + 0.3*y + 0.1*z) + 1e-4*t", "1e-4*(2. + x) + 1e-5*y*t + 1e-5*z"),
             (lambda V: 1e-3*(V["x"] + 0.3*V["y"] + 0.1*V["z"]) + 1e-4*V["t"],
              lambda V: 1e-4*(2. + V["x"]) + 1e-5*V["y"]*V["t"] + 1e-5*V["z"]), ())),
    ("block", (("{ if (x > 0.1) return 0.; return 1e-3*(1. + y); }", "{ double a = 1e-4*(1.5 + x); return a; }"),
               (lambda V: 0. if V["x"] > 0.1 else 1e-3*(1. + V["y"]), lambda V: 1e-4*(1.5 + V["x"])), ())),
])


def event_time(e):
    return T0 + 0.03125*e


def velocity(dim, level, e):
    """the velocity of the fluid at feed event e: arrays with ghosts"""
    return FK.velocity(dim, level, e % 2)


@functools.lru_cache(None)
def candidates(dim, level, e):
    """the positions of the candidates of event e, an (COUNTS[e], 3) array: a quarter of the random ones lies
    outside the box"""
    count = COUNTS[e]
    rng = np.random.default_rng(7000 + 100*e + 10*dim + level)
    n = 1 << level
    h = 1./n
    mid = n//2
    pos = 1.25*(rng.random((count, 3)) - 0.5)

    def centre(i, j, k):
        return np.array([-0.5 + (i - 0.5)*h, -0.5 + (j - 0.5)*h, -0.5 + (k - 0.5)*h])
    if count >= 70:
        pos[ON_FACE] = [-0.5 + 3*h, -0.5 + 2.25*h, -0.5 + 1.5*h]       # on the face between cells 3 and 4 along x
        pos[IN_CORNER] = centre(1, 1, 1) + 0.2*h
        for q, o in enumerate(SHARED):
            pos[o] = centre(2, mid, mid) + (0.1 + 0.2*q)*h
        pos[BETWEEN] = centre(n - 1, mid, mid) - 0.1*h                 # x > 0.1: the block gives no mass there
    if dim == 2:
        pos[:, 2] = 0.
    pos.setflags(write=False)
    return pos


class CachedBox:
    """sampler_reference.Box with locate and interpolate remembered: the functions of a case change, the
    candidates and the velocity do not"""

    def __init__(self, box):
        self._box, self._cells, self._values = box, {}, {}

    def __getattr__(self, name):
        return getattr(self._box, name)

    def locate(self, pos):
        key = tuple(pos)
        if key not in self._cells:
            self._cells[key] = self._box.locate(pos)
        return self._cells[key]

    def interpolate(self, cell, pos, v):
        key = (cell.ijk, tuple(pos), id(v))
        if key not in self._values:
            self._values[key] = self._box.interpolate(cell, pos, v)
        return self._values[key]


@functools.lru_cache(None)
def _shared(dim, level):
    box = CachedBox(SK.box(dim, level))
    u = [[box.field(a) for a in velocity(dim, level, e)] for e in range(2)]
    return box, u, box.field(K.tracer(dim, level))


def initial_list(dim, level, sides_name):
    pos, ids, vel, mass, volume = K.particles(dim, level, sides_name)
    return FP.ParticleList([FR.Particulate(pos[q], ids[q], vel[q], mass[q], volume[q]) for q in range(K.NPART)],
                           IDLAST0)


def feed_of(fname, pos, t):
    """the GfsFeedParticle of a case whose position functions walk through `pos'"""
    it = iter(np.asarray(pos).ravel().tolist())
    fmass, fvolume = FUNCTIONS[fname][1]
    return FP.Feed(nparts=lambda: float(len(pos)), xfeed=lambda: next(it), yfeed=lambda: next(it),
                   zfeed=lambda: next(it), mass=fmass, volume=fvolume)


State = collections.namedtuple("State", "pos ids old vel mass volume force idlast outcomes")


def state_of(pl, outcomes=()):
    p = pl.plist
    return State(np.array([q.pos for q in p]).reshape(-1, 3), np.array([q.id for q in p], dtype=np.uint32),
                 np.array([q.pos_old for q in p]).reshape(-1, 3), np.array([q.vel for q in p]).reshape(-1, 3),
                 np.array([q.mass for q in p]), np.array([q.volume for q in p]),
                 np.array([q.force for q in p]).reshape(-1, 3), pl.idlast, tuple(outcomes))


def feed_events(dim, level, sides_name, fname, events):
    """the list after each of the feed events `events' (indices into COUNTS) in a row: (the list, its states)"""
    box, u, T = _shared(dim, level)
    pl = initial_list(dim, level, sides_name)
    variables = {"T": T} if "T" in FUNCTIONS[fname][2] else {}
    states = []
    for e in events:
        t = event_time(e)
        out = FP.event(box, u[e % 2], pl, feed_of(fname, candidates(dim, level, e), t), t, variables)
        states.append(state_of(pl, out))
    return pl, states


BURST = 70000                           # 274 blocks of candidates: the scan of the block counts takes two rounds


@functools.lru_cache(None)
def burst_candidates(dim):
    pos = 1.25*(np.random.default_rng(7900 + dim).random((BURST, 3)) - 0.5)
    if dim == 2:
        pos[:, 2] = 0.
    pos.setflags(write=False)
    return pos


@functools.lru_cache(None)
def burst_reference(dim, level, sides_name, fname):
    """the state of the list after one event of BURST candidates (velocity and time of event 0)"""
    box, u, T = _shared(dim, level)
    pl = initial_list(dim, level, sides_name)
    variables = {"T": T} if "T" in FUNCTIONS[fname][2] else {}
    t = event_time(0)
    out = FP.event(box, u[0], pl, feed_of(fname, burst_candidates(dim), t), t, variables)
    return state_of(pl, out)


@functools.lru_cache(None)
def reference_run(dim, level, sides_name, fname):
    """the state of the list after every event of COUNTS"""
    return tuple(feed_events(dim, level, sides_name, fname, range(len(COUNTS)))[1])
