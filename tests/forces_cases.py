"""The case matrix of the force tests, shared by test_forces_reference_cpu.py (restatement alone, oracle
against its `pow' variant) and test_gpu_forces_reference.py (device against its `sqrt' variant).  The
references are computed once per process (functools caches) and never modified.

One case = one box, one list of at most 256 particulates, one list of forces and this sequence, the same
for the restatement, the oracle and the device:

    upload U_0; the list; set_forces (Un = U_0 with the ghosts of the default condition)
    upload U_1; event 1
    upload U_2; the forces on the fluid (where the run has them); event 2
    upload U_3; event 3

Every U_k is a distinct-values fill with its own salt per component, uploaded WITH its ghosts: the
gradient of a wall cell reads a ghost no boundary condition would have produced, and Un != U at every
event."""
import collections
import functools
import math

import numpy as np

import forces_reference as F
import sampler_cases as SK
import sampler_reference as R

P, B = R.SIDE_PERIODIC, R.SIDE_BOUNDARY
DIMS_LEVELS = [(2, 2), (2, 3), (3, 2), (3, 3)]
SIDES = {"periodic": [P]*6, "closed": [B]*6, "mixed": [P, P, B, B, B, B]}      # mixed: x periodic, the rest closed
SIDE_NAMES = ("periodic", "closed", "mixed")
NEVENTS = 3
ONFLUID_BEFORE_EVENT = 1          # index of the event the on-fluid evaluation precedes
NU = 1e-2
NU_BRANCHES = 2.**-7      # a power of two: Re = x/nu is exact, so every double near 50 and 1e-8 can be met
GRAVITY = (0.1, -0.5, 0.2)

I_, A_, L_, D_, B_ = F.INERTIAL, F.ADDEDMASS, F.LIFT, F.DRAG, F.BUOY
FORCE_LISTS = collections.OrderedDict([
    ("inertial", [I_]), ("addedmass", [A_]), ("lift", [L_]), ("drag", [D_]), ("buoy", [B_]),
    ("canonical", [I_, A_, L_, D_, B_]),
    ("reverse", [B_, D_, L_, A_, I_]),
    ("buoy-am-buoy", [B_, A_, B_]),
    ("am-am", [A_, A_]),
    ("am-drag", [A_, D_]),                    # no inertial force: Un stays the field of set_forces
    ("inertial-am-drag", [I_, A_, D_]),       # the same fields with an inertial force: Un refreshed
    ("empty", []),
])


def coefficient_functions(dim):
    """force kind -> (C text, the same expression in Python) from + - * /, fabs, sqrt and comparisons.
    Each reads Rep and one of Urelp, Vrelp, Wrelp, Pdia; in 2-D Wrelp does not exist (:198-201)."""
    if dim == 3:
        am = ("0.5 + 0.1*Pdia + 0.01*fabs (Wrelp) + 0.001*Rep",
              lambda rep, u, v, w, d: 0.5 + 0.1*d + 0.01*abs(w) + 0.001*rep)
    else:
        am = ("0.5 + 0.1*Pdia + 0.001*Rep",
              lambda rep, u, v, w, d: 0.5 + 0.1*d + 0.001*rep)
    return {
        A_: am,
        L_: ("0.3 + 0.01*sqrt (Rep) + 0.05*fabs (Urelp)",
             lambda rep, u, v, w, d: 0.3 + 0.01*math.sqrt(rep) + 0.05*abs(u)),
        D_: ("{ double a = 0.4 + 0.01*Rep; if (Vrelp > 0.) a += 0.1*Pdia/(1. + Rep); return a; }",
             lambda rep, u, v, w, d: (0.4 + 0.01*rep) + (0.1*d/(1. + rep) if v > 0. else 0.)),
    }


Case = collections.namedtuple("Case", "id dim level sides forces viscosity coeff dt_factor kind")
# viscosity: "uv" (nu on every component), "pow2" (NU_BRANCHES on every component), "zero", "v-only", "cell"
# (alpha_cell and viscosity_cell fields)
# coeff: coefficient functions on added mass, lift and drag; kind: "fill" or "drag-branches"


def _build_cases():
    cases = []

    def add(tag, dim, level, sides, forces, viscosity="uv", coeff=False, dt_factor=1., kind="fill"):
        cid = "%s-%dd-l%d-%s" % (tag, dim, level, sides)
        cases.append(Case(cid, dim, level, sides, forces, viscosity, coeff, dt_factor, kind))

    for k, (name, forces) in enumerate(FORCE_LISTS.items()):
        for q, (dim, level) in enumerate(DIMS_LEVELS):
            if name in ("canonical", "reverse"):
                for s in SIDE_NAMES:
                    add(name, dim, level, s, name)
            else:       # every list sees every kind of side, every box every list
                add(name, dim, level, SIDE_NAMES[(k + q) % 3], name)
    for q, (dim, level) in enumerate(DIMS_LEVELS):
        add("branches", dim, level, "periodic", "drag", viscosity="pow2", kind="drag-branches")
        add("nu0", dim, level, SIDE_NAMES[(q + 1) % 3], "canonical", viscosity="zero")
        add("nuV", dim, level, SIDE_NAMES[(q + 2) % 3], "canonical", viscosity="v-only")
        add("cell", dim, level, SIDE_NAMES[q % 3], "reverse", viscosity="cell")
        add("dt0", dim, level, "closed", "canonical", dt_factor=0.)
        add("coeff", dim, level, SIDE_NAMES[q % 3], "canonical", coeff=True)
    for dim, level, s in ((2, 3, "closed"), (3, 2, "periodic")):
        add("nu0-coeff", dim, level, s, "canonical", viscosity="zero", coeff=True)
        add("cell-coeff", dim, level, s, "canonical", viscosity="cell", coeff=True)
    return collections.OrderedDict((c.id, c) for c in cases)


CASES = _build_cases()
CASE_IDS = list(CASES)


def dt_of(case):
    return case.dt_factor*0.05/(1 << case.level)


@functools.lru_cache(None)
def velocity(dim, level, k, zero=False):
    """U_k: components as arrays with ghosts in [-1, 1), NaN in the edge and corner ghosts"""
    out = []
    for c in range(dim):
        a = 2.*(SK.distinct_field(dim, level, salt=40 + 3*k + c) - 1.)
        if zero:
            a = np.zeros_like(a)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(None)
def cell_fields(dim, level):
    """(alpha_cell, viscosity_cell): a value of its own in every cell, wall cells included; alpha in
    [0.5, 1.5), the viscosity in [0.005, 0.015)"""
    alpha = SK.distinct_field(dim, level, salt=71).copy()
    mu = 0.01*SK.distinct_field(dim, level, salt=72)
    for a in (alpha, mu):
        a.setflags(write=False)
    return alpha, mu


@functools.lru_cache(None)
def particles(dim, level):
    """(pos, ids, vel, mass, volume): sampler_cases.sample_points thinned to at most 256 -- centres, face,
    edge and corner points of the cells, the box sides at +-0.5, one point one ulp outside per side -- and
    one heavy particle aimed through an edge of the box (in a periodic box it is wrapped along one axis
    only and is on the list, outside, when the forces on the fluid are taken).  vel[:, 2] != 0 in 2-D."""
    rng = np.random.default_rng(7000 + 10*dim + level)
    pts = SK.sample_points(dim, level)
    nout = 2*dim*5
    inside, outside = pts[:-nout], pts[-nout:]
    keep_out = [outside[5*s + (0 if s % 2 else 4)] for s in range(2*dim)]
    on_sides = (np.abs(inside[:, :dim]) == 0.5).sum(axis=1)
    corners = inside[on_sides == dim][[0, -1]]      # two opposite corners of the box
    faces = inside[on_sides == 1]                   # on one side of the box
    others = inside[on_sides == 0]
    total = 120 if dim == 2 else 250
    faces = faces[np.sort(rng.choice(len(faces), 10, replace=False))]
    nsel = total - len(keep_out) - len(corners) - len(faces)
    sel = np.concatenate([others[np.sort(rng.choice(len(others), nsel, replace=False))], faces])
    aimed = np.array([[0.5 - 1e-3, 0.5 - 1e-3, 0.1 if dim == 3 else 0.]])
    pos = np.concatenate([sel, corners, np.array(keep_out), aimed])
    n = len(pos)
    assert n <= 256
    vel = 0.3*rng.standard_normal((n, 3))
    vel[-1] = (1., 1., 0.2)
    volume = 1e-3*(0.5 + rng.random(n))
    mass = volume*(2. + 10.*rng.random(n))
    mass[-1] = volume[-1]*1000.
    order = rng.permutation(n)
    pos, vel, volume, mass = pos[order], vel[order], volume[order], mass[order]
    ids = np.arange(1, n + 1, dtype=np.uint32)
    for a in (pos, ids, vel, mass, volume):
        a.setflags(write=False)
    return pos, ids, vel, mass, volume


RE_50_BELOW, RE_50_ABOVE = math.nextafter(50., 0.), math.nextafter(50., 100.)
RE_TINY_BELOW = math.nextafter(1e-8, 0.)
BRANCH_TARGETS = (("tiny", 1e-10), ("tiny", 3e-9), ("just-below-1e-8", RE_TINY_BELOW), ("at-1e-8", 1e-8),
                  ("middle", 1e-4), ("middle", 0.7), ("middle", 21.), ("just-below-50", RE_50_BELOW),
                  ("at-50", 50.), ("just-above-50", RE_50_ABOVE), ("high", 80.), ("high", 900.))


def _speed_for(re, dia):
    """a speed v with v*dia*1./NU_BRANCHES == re exactly in floating point, or None.  The fluid is at rest
    and of density 1; sqrt (v*v) == v."""
    v = re*NU_BRANCHES/dia
    for _ in range(8):
        v = math.nextafter(v, 0.)
    for _ in range(17):
        if v*dia*1./NU_BRANCHES == re and math.sqrt(v*v) == v:
            return v
        v = math.nextafter(v, math.inf)
    return None


@functools.lru_cache(None)
def branch_particles(dim, level):
    """the drag-branch sub-case: the fluid is at rest, so that Re is set exactly by the particle's velocity:
    8 particles per entry of BRANCH_TARGETS whose first event computes exactly that Re (exact targets),
    the speed along x or y; in 2-D a z velocity that must not enter the norm (:555-556)"""
    rng = np.random.default_rng(7100 + 10*dim + level)
    pos, vel, vol = [], [], []
    for name, re in BRANCH_TARGETS:
        found = tries = 0
        while found < 8:
            tries += 1
            assert tries < 10000, (name, re)
            volume = 1e-3*(0.5 + rng.random())
            dia = 2.*math.pow(3.0*volume/4.0/math.pi, 1./3.)
            v = _speed_for(re, dia)
            if v is None:
                continue
            w = [0., 0., 0.]
            w[found % 2] = v if found % 4 < 2 else -v
            if dim == 2:
                w[2] = float(rng.uniform(0.5, 2.))
            p = list(rng.uniform(-0.45, 0.45, dim)) + [0.]*(3 - dim)
            pos.append(p)
            vel.append(w)
            vol.append(volume)
            found += 1
    pos, vel, volume = np.array(pos), np.array(vel), np.array(vol)
    mass = volume*(0.5 + 2.5*rng.random(len(volume)))
    ids = np.arange(1, len(pos) + 1, dtype=np.uint32)
    assert len(pos) <= 256
    for a in (pos, ids, vel, mass, volume):
        a.setflags(write=False)
    return pos, ids, vel, mass, volume


def case_particles(case):
    return (branch_particles if case.kind == "drag-branches" else particles)(case.dim, case.level)


def case_velocity(case, k):
    return velocity(case.dim, case.level, k, zero=case.kind == "drag-branches")


def force_objects(case):
    """the GfsParticleForce objects of the case's list"""
    fns = coefficient_functions(case.dim) if case.coeff else {}
    return [F.ForceCoeff(kind, fns[kind][1] if kind in fns else None) for kind in FORCE_LISTS[case.forces]]


def coefficient_texts(case):
    """index in the list -> C text"""
    fns = coefficient_functions(case.dim) if case.coeff else {}
    return {q: fns[kind][0] for q, kind in enumerate(FORCE_LISTS[case.forces]) if kind in fns}


def coefficient_callables(case):
    fns = coefficient_functions(case.dim) if case.coeff else {}
    return {q: fns[kind][1] for q, kind in enumerate(FORCE_LISTS[case.forces]) if kind in fns}


State = collections.namedtuple("State", "tag pos old ids vel mass force")
Run = collections.namedtuple("Run", "states inputs branches parts outside_at_onfluid initial_cells")


def _state(tag, plist):
    def arr(rows, shape, dtype=np.float64):
        a = np.array(rows, dtype=dtype).reshape(shape)
        a.setflags(write=False)
        return a
    return State(tag, arr([p.pos for p in plist], (-1, 3)), arr([p.pos_old for p in plist], (-1, 3)),
                 arr([p.id for p in plist], (-1,), np.uint32), arr([p.vel for p in plist], (-1, 3)),
                 arr([p.mass for p in plist], (-1,)), arr([p.force for p in plist], (-1, 3)))


@functools.lru_cache(None)
def reference_run(case_id, root="sqrt", onfluid=True):
    """the restatement on one case.  root: "pow" (the reference's text) or "sqrt" (the device's);
    onfluid: with the evaluation of the forces on the fluid before event ONFLUID_BEFORE_EVENT.

    Run.states: the list after every step, tags "event0", "onfluid", "event1", "event2";
    Run.inputs: what every coefficient function was called with, (kind, Rep, Urelp, Vrelp, Wrelp, Pdia);
    Run.branches: (branch of the drag law, Re) of every drag evaluation of the FIRST event;
    Run.parts: kind -> summed |new_force*volume| over the events;
    Run.outside_at_onfluid: (number of listed particles outside the box when the forces on the fluid are
    taken, the largest |force| any of them held before)."""
    case = CASES[case_id]
    dim, level = case.dim, case.level
    box = SK.box(dim, level)
    sides = SIDES[case.sides]
    alpha = None
    const = lambda cell: NU
    pow2 = lambda cell: NU_BRANCHES
    viscosity = {"uv": (const, const, const), "pow2": (pow2, pow2, pow2), "zero": (None, None, None), "v-only": (None, const, None)}.get(case.viscosity)
    if case.viscosity == "cell":
        af, mf = (box.field(a) for a in cell_fields(dim, level))
        alpha = lambda cell: box.value(cell, af)
        viscosity = (lambda cell: box.value(cell, mf), None, None)
    sim = F.Sim(box, sides, case_velocity(case, 0), dt_of(case), alpha=alpha, viscosity=viscosity, g=GRAVITY,
                root=F.pow_root if root == "pow" else F.sqrt_root)
    pos, ids, vel, mass, volume = case_particles(case)
    plist = [F.Particulate(p, i, v, m, w) for p, i, v, m, w in
             zip(pos.tolist(), ids.tolist(), vel.tolist(), mass.tolist(), volume.tolist())]
    initial_cells = [box.locate(p.pos) for p in plist]
    forces = force_objects(case)
    F.read_forces(sim, forces)
    states, inputs, branches, parts = [], [], [], []
    outside = (0, 0.)
    for k in range(NEVENTS):
        sim.set_velocity(case_velocity(case, k + 1))
        if onfluid and k == ONFLUID_BEFORE_EVENT:
            out = [p for p in plist if box.locate(p.pos) is None]
            outside = (len(out), max([max(abs(x) for x in p.force) for p in out] + [0.]))
            F.forces_on_fluid(sim, plist, forces, inputs)
            states.append(_state("onfluid", plist))
        plist = F.list_event(sim, plist, forces, inputs, branches if k == 0 else None, parts)
        states.append(_state("event%d" % k, plist))
    share = collections.OrderedDict()
    for q, (kind, f) in enumerate(parts):
        share[kind] = share.get(kind, 0.) + sum(abs(x) for x in f)
    return Run(tuple(states), tuple(inputs), tuple(branches), share, outside, tuple(initial_cells))


def wall_class(box, cell):
    """the number of box sides a cell touches"""
    return sum(1 for d in range(box.ndir) if box.neighbor(cell, d).boundary)
