"""Particulates with forces on refined trees (csrc/tree_particles.hip) against the restatement of the reference
on explicit cell trees (tests/tree_forces_reference.py, with the sqrt root of the device's drag law), bit for
bit; a uniform tree's list against the uniform box's; coefficient functions; the refusals that remain."""
import collections
import functools
import math

import numpy as np
import pytest

import gfship
import forces_reference as F
import tree_forces_reference as TF
import tree_sampler_cases as TC
import tree_sampler_reference as T

pytestmark = pytest.mark.gpu
G = gfship.Tree

ORDER_A = (F.INERTIAL, F.ADDEDMASS, F.LIFT, F.DRAG, F.BUOY)
ORDER_B = (F.BUOY, F.DRAG, F.LIFT, F.ADDEDMASS, F.INERTIAL)     # the buoyancy before the added mass changes `mass'
GRAVITY = (0.3, -0.5, 0.2)
NU = 1e-4
# the trees that carry GfsSourceDiffusion {} U nu; the others (one 2-D, one 3-D among them) have no viscosity:
# no drag there, and 0.001 in Rep
VISCOUS = ("square", "walls2", "cube")
CFL = 0.4


# an L-shaped patch: level 2 with three of the four cells in the middle refined once.  The coarse cell in the notch
# has refined neighbours on two sides: the transverse neighbour of a coarse cell with children, which the convex
# patches of TC.TREES do not have
ELL = (2, lambda x, y: 3 if (abs(x) < 0.25 and abs(y) < 0.25 and not (x > 0. and y > 0.)) else 2, [TC.P]*4,
       ("wrapped", "fine_to_coarse", "coarse_to_fine"))


def spec(name):
    return ELL if name == "ell" else TC.TREES[name]


def make_tree(name):
    dim, refine, sides, _ = spec(name)
    g = gfship.Tree(refine, dim=dim, sides=None if all(s == TC.P for s in sides) else sides)
    flags = [g.flags(l) for l in range(g.depth + 1)]
    return g, flags


@functools.lru_cache(None)
def restatement(name):
    g, flags = make_tree(name)
    g.destroy()
    return TC.restatement(spec(name)[0], flags), flags


def velocity_vars(dim):
    return [G.U, G.V, G.W][:dim]


def start_tree(name, nu):
    dim = spec(name)[0]
    g, flags = make_tree(name)
    if name == "walls2":
        prof = [TC.inflow_profile(g.centres(l)) for l in range(g.depth + 1)]
        g.set_bc_u(0, 1, gfship.BC_DIRICHLET, prof)
        g.set_bc_u(0, 0, gfship.BC_NEUMANN)
        g.set_bc(0, gfship.BC_DIRICHLET)
    for l in range(g.depth + 1):
        for var, a in zip(velocity_vars(dim), TC.initial_velocity("square" if name == "ell" else name, g.centres(l))):
            g.upload(var, l, np.ascontiguousarray(np.broadcast_to(a, flags[l].shape)))
    for p in (g.projection_params, g.approx_projection_params):
        p.tolerance = 1e-4
    if nu:
        for c in range(dim):
            g.set_viscosity(c, nu)
    g.set_time(1e30, CFL)
    g.start()
    return g


def particulate_state(dim, n, seed):
    """velocities that differ from the fluid's (which is about 0.8 to 1 along every axis), volumes over two
    decades, density ratios from 0.5 to 2 (fluid_rho = 1)"""
    rng = np.random.default_rng(seed)
    vel = np.zeros((n, 3))
    vel[:, :dim] = 0.8 + rng.uniform(-0.4, 0.4, (n, dim))
    volume = 10.**rng.uniform(-6.5, -4.5, n)
    mass = volume*rng.uniform(0.5, 2., n)
    return vel, mass, volume


def fluid(g, dim):
    return [[g.download(var, l) for l in range(g.depth + 1)] for var in velocity_vars(dim)]


def reference_sim(box, sides, g, dim, nu):
    return F.Sim(box, sides, fluid(g, dim), g.dt, viscosity=((lambda cell: nu) if nu else None, None, None),
                 g=GRAVITY, root=F.sqrt_root)


def reference_list(pos, ids, vel, mass, volume):
    return [F.Particulate(p, i, v, m, w) for p, i, v, m, w in
            zip(pos.tolist(), ids.tolist(), vel.tolist(), mass.tolist(), volume.tolist())]


def assert_previous_velocity(g, sim, flags, dim, what):
    """Un, Vn, Wn on the leaves and the ghost leaves of every level"""
    for c, var in enumerate([G.UPREV, G.VPREV, G.WPREV][:dim]):
        for l in range(g.depth + 1):
            m = flags[l] == T.LEAF
            want = np.array(sim.un[c][l])
            assert not np.isnan(want[m]).any()
            assert np.array_equal(g.download(var, l)[m], want[m]), (what, c, l)


def assert_lists_equal(pl, plist, what):
    p, i = pl.download()
    assert pl.count() == len(plist) == len(i), what
    assert np.array_equal(i, np.array([q.id for q in plist], dtype=np.uint32)), what
    assert np.array_equal(p, np.array([q.pos for q in plist]).reshape(-1, 3)), ("positions", what)
    assert np.array_equal(pl.download_old(), np.array([q.pos_old for q in plist]).reshape(-1, 3)), ("old", what)
    vel, mass, force = pl.particulate_state()
    assert np.array_equal(vel, np.array([q.vel for q in plist]).reshape(-1, 3)), ("velocity", what)
    assert np.array_equal(mass, np.array([q.mass for q in plist])), ("mass", what)
    assert np.array_equal(force, np.array([q.force for q in plist]).reshape(-1, 3)), ("force", what)
    assert not np.isnan(p).any() and not np.isnan(vel).any() and not np.isnan(force).any()


@pytest.mark.parametrize("name", list(TC.TREES))
def test_all_five_forces(name):
    dim, _, sides, must = TC.TREES[name]
    nu = NU if name in VISCOUS else 0.
    order = ORDER_A if list(TC.TREES).index(name) % 2 == 0 else ORDER_B
    other = ORDER_B if order is ORDER_A else ORDER_A
    box, flags = restatement(name)
    box.record = collections.Counter()
    box.gradient_census = census = TF.new_census()
    g = start_tree(name, nu)
    pos, ids = TC.seeds(box, 3)
    vel, mass, volume = particulate_state(dim, len(ids), 17)
    pl = g.particulates(pos, ids, vel, mass, volume)
    pl.set_sort_interval(2)          # a sort between the events: storage order only
    plist = reference_list(pos, ids, vel, mass, volume)
    sim = reference_sim(box, sides, g, dim, nu)
    forces = [F.ForceCoeff(k) for k in order]
    pl.set_forces(list(other), GRAVITY)
    pl.set_forces(list(order), GRAVITY)          # a new list of forces replaces the first
    TF.read_forces(sim, forces)
    assert_previous_velocity(g, sim, flags, dim, "set_forces")
    branch = []
    for k in range(3):
        g.step()
        sim.set_velocity(fluid(g, dim))
        sim.dt = g.dt
        pl.event()
        plist = TF.list_event(sim, plist, forces, branch=branch)
        assert_lists_equal(pl, plist, (name, k))
        assert_previous_velocity(g, sim, flags, dim, ("event", k))
    pl.destroy()
    g.destroy()
    del box.gradient_census
    # what matters happened
    assert box.record["outside_at_start"] >= dim
    for what in must:
        if what in ("wrapped", "removed", "fine_to_coarse", "coarse_to_fine"):
            assert box.record[what] > 0, (what, dict(box.record))
    S, C, K = TF.SAME_LEAF, TF.CHILDREN, TF.COARSER
    assert census[("pair", S, S)] > 0
    assert census["one"] == 0 and census["none"] == 0 and census[TF.TRANSVERSE_ABSENT] == 0
    if name != "uniform2":
        assert census[("pair", S, K)] > 0 and census[("pair", K, S)] > 0, dict(census)
        assert census[("pair", S, C)] > 0 and census[("pair", C, S)] > 0, dict(census)
        assert census[TF.TRANSVERSE_LEAF] > 0
    taken = collections.Counter(b for b, _ in branch)
    if nu:
        assert taken["below-50"] > 0 and taken["from-50"] > 0 and taken["no-viscosity"] == 0, dict(taken)
    else:
        assert taken["no-viscosity"] > 0 and len(taken) == 1, dict(taken)


def test_refined_transverse_neighbour_in_a_notch():
    """the L-shaped patch: the interpolation in a coarse neighbour meets a transverse neighbour with children (the
    mean of its children on the face at 3/4, src/fluid.c:75-88 from :178-186), from the particulate kernel"""
    dim, _, sides, must = ELL
    box, flags = restatement("ell")
    assert sum(c.level == 3 for c in box.leaves) == 12 and sum(c.level == 2 for c in box.leaves) == 13
    box.record = collections.Counter()
    box.gradient_census = census = TF.new_census()
    g = start_tree("ell", NU)
    pos, ids = TC.seeds(box, 3)
    vel, mass, volume = particulate_state(dim, len(ids), 37)
    pl = g.particulates(pos, ids, vel, mass, volume)
    pl.set_sort_interval(2)
    plist = reference_list(pos, ids, vel, mass, volume)
    sim = reference_sim(box, sides, g, dim, NU)
    forces = [F.ForceCoeff(k) for k in ORDER_A]
    pl.set_forces(list(ORDER_A), GRAVITY)
    TF.read_forces(sim, forces)
    assert_previous_velocity(g, sim, flags, dim, "set_forces")
    for k in range(3):
        g.step()
        sim.set_velocity(fluid(g, dim))
        sim.dt = g.dt
        pl.event()
        plist = TF.list_event(sim, plist, forces)
        assert_lists_equal(pl, plist, ("ell", k))
        assert_previous_velocity(g, sim, flags, dim, ("event", k))
    pl.destroy()
    g.destroy()
    del box.gradient_census
    assert census[TF.TRANSVERSE_CHILDREN] > 0 and census[TF.TRANSVERSE_LEAF] > 0, dict(census)
    assert census[TF.TRANSVERSE_ABSENT] == 0 and census["one"] == 0 and census["none"] == 0
    for what in must:
        assert box.record[what] > 0, (what, dict(box.record))


@pytest.mark.parametrize("kind", ORDER_A)
@pytest.mark.parametrize("name", ["square", "cube"])
def test_each_force_alone(name, kind):
    dim, _, sides, _ = TC.TREES[name]
    box, flags = restatement(name)
    g = start_tree(name, NU)
    pos, ids = TC.seeds(box, 3)
    vel, mass, volume = particulate_state(dim, len(ids), 23)
    pl = g.particulates(pos, ids, vel, mass, volume)
    plist = reference_list(pos, ids, vel, mass, volume)
    sim = reference_sim(box, sides, g, dim, NU)
    forces = [F.ForceCoeff(kind)]
    pl.set_forces([kind], GRAVITY)
    TF.read_forces(sim, forces)
    if kind == F.BUOY:       # GfsForceBuoy is no GfsForceCoeff: the tree still has no Un
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            g.download(G.UPREV, 0)
    g.step()
    sim.set_velocity(fluid(g, dim))
    sim.dt = g.dt
    pl.event()
    plist = TF.list_event(sim, plist, forces)
    assert_lists_equal(pl, plist, (name, kind))
    assert np.abs(pl.particulate_state()[2]).max() > 0.
    if kind != F.BUOY:
        assert_previous_velocity(g, sim, flags, dim, "event")
    pl.destroy()
    g.destroy()


@pytest.mark.parametrize("dim,level", [(2, 4), (3, 3)])
def test_uniform_tree_list_equals_uniform_box_list(dim, level):
    """the particulates of a uniform tree against those of the uniform box (pinned on the oracle and on
    tests/forces_reference.py): the same initial velocity, particles and forces, 3 steps.  The viscosity the drag
    reads is given after every step and taken away before the next one, so that the two flows stay the inviscid
    ones that tests/test_gpu_tree_sampler.py compares."""
    refine = (lambda x, y: level) if dim == 2 else (lambda x, y, z: level)
    g = gfship.Tree(refine, dim=dim)
    dom = gfship.Domain(dim, level, side=[gfship.SIDE_PERIODIC]*6)
    sim = gfship.Simulation(dom)
    u0 = TC.initial_velocity("uniform2" if dim == 2 else "cube", g.centres(level))
    n = 1 << level
    for c in range(dim):
        a = np.ascontiguousarray(np.broadcast_to(u0[c], (n + 2,)*dim))
        g.upload(velocity_vars(dim)[c], level, a)
        sim.u[c].upload(a)
    for p in (g.projection_params, g.approx_projection_params, sim.projection_params, sim.approx_projection_params):
        p.tolerance = 1e-4
    g.set_time(1e30, 0.8)
    sim.set_time(1e30)
    sim.advection_params.cfl = 0.8
    rng = np.random.default_rng(dim)
    pos = np.zeros((300, 3))
    pos[:, :dim] = rng.uniform(-0.5, 0.5, (300, dim))
    pos[:40, 0] = 0.5 - rng.uniform(0., 0.01, 40)        # next to the side the flow leaves through
    ids = np.arange(300, dtype=np.uint32)
    vel, mass, volume = particulate_state(dim, 300, 29)
    tl, ul = g.particulates(pos, ids, vel, mass, volume), gfship.ParticleList(sim, pos, ids)
    ul.set_particulate(vel, mass, volume)
    g.start()
    sim.start()
    tl.set_forces(list(ORDER_A), GRAVITY)
    ul.set_forces(list(ORDER_A), GRAVITY)
    for k in range(3):
        g.step()
        sim.step()
        assert g.dt == sim.dt
        g.set_viscosity(0, NU)
        sim.set_viscosity(0, NU)
        tl.event()
        ul.event()
        g.set_viscosity(0, 0.)
        sim.set_viscosity(0, 0.)
        (tp, ti), (up, ui) = tl.download(), ul.download()
        assert np.array_equal(ti, ui) and np.array_equal(tp, up), k
        for a, b in zip(tl.particulate_state(), ul.particulate_state()):
            assert np.array_equal(a, b), k
    assert (np.abs(tp - pos[:len(tp)]) > 0.).any() and np.abs(tl.particulate_state()[2]).max() > 0.
    # the drag acts in this comparison: one event of two lists that hold nothing but a GfsForceDrag, on the fields
    # the two flows have now.  Without a viscosity such a list gets no force at all; with it, the same non-zero one
    td, ud = g.particulates(pos, ids, vel, mass, volume), gfship.ParticleList(sim, pos, ids)
    ud.set_particulate(vel, mass, volume)
    for x in (td, ud):
        x.set_forces([F.DRAG], GRAVITY)
        x.event()
        assert np.abs(x.particulate_state()[2]).max() == 0.
    g.set_viscosity(0, NU)
    sim.set_viscosity(0, NU)
    td.event()
    ud.event()
    g.set_viscosity(0, 0.)
    sim.set_viscosity(0, 0.)
    assert np.array_equal(td.download()[1], ud.download()[1])
    for a, b in zip(td.particulate_state() + td.download()[:1], ud.particulate_state() + ud.download()[:1]):
        assert np.array_equal(a, b)
    drag = td.particulate_state()[2]
    assert (np.abs(drag[:, :dim]).max(axis=1) > 0.).all() and not np.isnan(drag).any()
    td.destroy()
    ud.destroy()
    for x in (tl, ul, sim, dom, g):
        x.destroy()


def _rel_err(a, b):
    scale = max(np.abs(a).max(), 1e-300)
    return np.abs(a - b).max()/scale


@pytest.mark.parametrize("name", ["square", "cube"])
def test_coefficient_functions(name):
    """a GfsFunction on the added-mass, lift and drag coefficients (modules/particulatecommon.c:166-210), compiled
    for the device with hipRTC; the restatement calls the same expressions on the host.  Same survivors in the same
    order; positions, velocities, masses and forces within 1e-12 relative L-infinity: the only operation that is
    not bit-reproducible is pow (Rep, 0.687) of the Schiller-Naumann law, the device's pow against the host's, as
    in tests/test_gpu_particles.py."""
    dim, _, sides, _ = TC.TREES[name]
    box, flags = restatement(name)
    g = start_tree(name, NU)
    pos, ids = TC.seeds(box, 3)
    vel, mass, volume = particulate_state(dim, len(ids), 31)
    pl = g.particulates(pos, ids, vel, mass, volume)
    pl.set_sort_interval(2)
    plist = reference_list(pos, ids, vel, mass, volume)
    sim = reference_sim(box, sides, g, dim, NU)
    coefficients = {
        1: ("0.5 + 0.1*Pdia + 0.01*fabs (Wrelp)",
            lambda rep, u, v, w, d: 0.5 + 0.1*d + 0.01*abs(w)),
        2: ("{ double a = 0.3 + 0.1*Urelp; if (Rep > 1.) a += 0.05*Vrelp; return a; }",
            lambda rep, u, v, w, d: (0.3 + 0.1*u) + (0.05*v if rep > 1. else 0.)),
        3: ("24./Rep*(1. + 0.15*pow (Rep, 0.687))",
            lambda rep, u, v, w, d: 24./rep*(1. + 0.15*math.pow(rep, 0.687))),
    }
    forces = [F.ForceCoeff(k, coefficients[f][1] if f in coefficients else None) for f, k in enumerate(ORDER_A)]
    pl.set_forces(list(ORDER_A), GRAVITY)
    for f, (text, _) in coefficients.items():
        pl.set_force_coefficient(f, text)
    TF.read_forces(sim, forces)
    inputs = []
    for k in range(2):
        g.step()
        sim.set_velocity(fluid(g, dim))
        sim.dt = g.dt
        pl.event()
        plist = TF.list_event(sim, plist, forces, inputs=inputs)
        p, i = pl.download()
        assert np.array_equal(i, np.array([q.id for q in plist], dtype=np.uint32)), k
        gv, gm, gf = pl.particulate_state()
        for got, want, what in ((p, [q.pos for q in plist], "pos"), (gv, [q.vel for q in plist], "vel"),
                                (gm, [q.mass for q in plist], "mass"), (gf, [q.force for q in plist], "force")):
            e = _rel_err(np.array(want).reshape(got.shape), got)
            assert e <= 1e-12, (k, what, e)
    # the functions were really called, with values that are not the defaults
    assert set(a[0] for a in inputs) == {F.ADDEDMASS, F.LIFT, F.DRAG}
    assert any(abs(coefficients[1][1](*a[1:]) - 0.5) > 1e-4 for a in inputs if a[0] == F.ADDEDMASS)
    assert any(abs(coefficients[2][1](*a[1:]) - 0.5) > 1e-2 for a in inputs if a[0] == F.LIFT)
    pl.destroy()
    g.destroy()


def test_refusals_that_remain():
    g, _ = make_tree("square")
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.download(G.UPREV, 0)       # no list has asked for Un yet
    n = 4
    pl = g.particulates(np.zeros((n, 3)), np.arange(n), np.zeros((n, 3)), np.ones(n), np.ones(n))
    dom = gfship.Domain(2, 3, side=[gfship.SIDE_PERIODIC]*6)
    v = dom.variable()
    calls = [lambda: pl.set_particulate(np.zeros((n, 3)), np.ones(n), np.ones(n)),
             lambda: gfship._check(gfship.lib().gfship_particles_set_migrate(pl.ptr, None, None)),
             lambda: gfship._check(gfship.lib().gfship_particles_record_size(pl.ptr)),
             lambda: pl.particulate_field(v),
             lambda: pl.forces_on_fluid(),
             lambda: pl.spread_forces([v, v]),
             lambda: pl.source_particulate_event([v, v]),
             lambda: pl.set_kernel(0.1)]
    for call in calls:
        with pytest.raises(gfship.GfshipError, match="gfship error -5: .*tree"):
            call()
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.download(G.UPREV, 0)
    pl.set_forces([F.BUOY], GRAVITY)
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.download(G.UPREV, 0)       # GfsForceBuoy is no GfsForceCoeff
    pl.set_forces([F.DRAG], GRAVITY)
    assert g.download(G.UPREV, 0).shape == (3, 3) and g.download(G.VPREV, g.depth).shape == (10, 10)
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.download(G.WPREV, 0)       # a quadtree has no Wn
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.upload(G.UPREV, 0, np.zeros((3, 3)))       # Un is the library's to write
    with pytest.raises(gfship.GfshipError, match="gfship error -1: .*does not compile"):
        pl.set_force_coefficient(0, "24./Rep +* nonsense(")
    pl.set_force_coefficient(0, "24./Rep")
    assert pl.count() == n and len(pl.particulate_state()[1]) == n
    pl.destroy()
    g.destroy()
    dom.destroy()
