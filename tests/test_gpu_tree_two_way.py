"""Two-way coupling on refined trees (csrc/tree_particles.hip, csrc/tree.hip) against the restatement of the
reference on explicit cell trees (tests/tree_two_way_reference.py), bit for bit unless said: the void fraction, the
forces on the fluid, the spreading, a uniform tree against the uniform box, the MAC value of the source fields,
uniform source fields against a GfsSource, striped trees, the refusals."""
import functools

import numpy as np
import pytest

import gfship
import forces_reference as F
import tree_forces_reference as TF
import tree_sampler_cases as TC
import tree_sampler_reference as T
import tree_two_way_cases as C
import tree_two_way_reference as TW
import two_way_cases as BC
import two_way_reference as BR

pytestmark = pytest.mark.gpu
G = gfship.Tree

ORDER_A = (F.INERTIAL, F.ADDEDMASS, F.LIFT, F.DRAG, F.BUOY)
ORDER_B = (F.BUOY, F.DRAG, F.LIFT, F.ADDEDMASS, F.INERTIAL)
GRAVITY = (0.3, -0.5, 0.2)
NU = 1e-4
CFL = 0.4
FVARS = [G.FX, G.FY, G.FZ]
UVARS = [G.U, G.V, G.W]


def make_tree(name):
    dim, refine, sides = C.spec(name)
    g = gfship.Tree(refine, dim=dim, sides=None if all(s == C.P for s in sides) else sides)
    return g, [g.flags(l) for l in range(g.depth + 1)]


@functools.lru_cache(None)
def restatement(name):
    g, flags = make_tree(name)
    g.destroy()
    return TC.restatement(C.spec(name)[0], flags), flags


def start_tree(name, nu):
    dim = C.spec(name)[0]
    g, flags = make_tree(name)
    if name == "walls2":
        prof = [TC.inflow_profile(g.centres(l)) for l in range(g.depth + 1)]
        g.set_bc_u(0, 1, gfship.BC_DIRICHLET, prof)
        g.set_bc_u(0, 0, gfship.BC_NEUMANN)
        g.set_bc(0, gfship.BC_DIRICHLET)
    for l in range(g.depth + 1):
        for var, a in zip(UVARS, TC.initial_velocity("square" if name == "ell" else name, g.centres(l))):
            g.upload(var, l, np.ascontiguousarray(np.broadcast_to(a, flags[l].shape)))
    for p in (g.projection_params, g.approx_projection_params):
        p.tolerance = 1e-4
    if nu:
        for c in range(dim):
            g.set_viscosity(c, nu)
    g.set_time(1e30, CFL)
    g.start()
    return g, flags


def fluid(g, dim):
    return [[g.download(var, l) for l in range(g.depth + 1)] for var in UVARS[:dim]]


def levels(g, var):
    return [g.download(var, l) for l in range(g.depth + 1)]


def assert_field_on_leaves(g, var, want, flags, what):
    """the device's variable equals the restatement's field on the leaves of every level, ghost leaves included"""
    for l in range(g.depth + 1):
        m = flags[l] == T.LEAF
        assert np.array_equal(g.download(var, l)[m], np.array(want[l], dtype=np.float64)[m]), (what, l)


def ghost_leaf_mask(flags, l, dim):
    m = flags[l] == T.LEAF
    m[(slice(1, -1),)*dim] = False
    return m


# -------------------------------------------------------------------------------------------------
# void fraction
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.ALL)
def test_void_fraction(name):
    dim = C.spec(name)[0]
    box, flags = restatement(name)
    g, _ = start_tree(name, 0.)
    pos, ids = TC.seeds(box, 3)
    # a particle on a face between two levels (where the tree has two)
    for c in box.leaves:
        nb = box.neighbor(c, 0)
        if nb is not None and not nb.boundary and nb.level < c.level:
            p = np.array([[c.pos[a] if a < dim else 0. for a in range(3)]])
            p[0, 0] = c.pos[0] + box.cell_size(c)/2.
            pos = np.vstack([pos, p])
            ids = np.append(ids, ids.max() + 1).astype(np.uint32)
            break
    n = len(ids)
    rng = np.random.default_rng(11)
    volume = 10.**rng.uniform(-6.5, -3.5, n)
    vel = np.zeros((n, 3))
    vel[:, :dim] = rng.uniform(-1., 1., (n, dim))
    vol_of = dict(zip(ids.tolist(), volume.tolist()))
    pl = g.particulates(pos, ids, vel, 2.*volume, volume)
    assert sum(box.locate(p) is None for p in pos.tolist()) >= dim            # outside the box, on the list
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.download(G.VF, 0)                                                   # before the first call: no such variable

    def check(what):
        p, i = pl.download()
        plist = [C.Part(a, b, vol_of[b], (0., 0., 0.)) for a, b in zip(p.tolist(), i.tolist())]
        want = TW.void_fraction(box, plist)
        g.particulate_field(pl)
        assert_field_on_leaves(g, G.VF, want, flags, (name, what))
        assert max(np.array(want[l]).max() for l in range(g.depth + 1)) > 0.
        for l in range(g.depth + 1):                                          # ghost cells stay 0
            assert not g.download(G.VF, l)[ghost_leaf_mask(flags, l, dim)].any()
        return len(i)

    n0 = check("created")
    pl.sort()
    check("sorted")
    # an event takes the particles outside off the list (and, where there are walls, those that leave through one)
    pl.set_forces([F.BUOY], (0., 0., 0.))
    pl.event()
    n1 = check("after an event")
    assert n1 <= n0 - dim
    pl.sort()
    check("after an event, sorted")
    pl.destroy()
    g.destroy()


# -------------------------------------------------------------------------------------------------
# forces on the fluid
# -------------------------------------------------------------------------------------------------

def particulate_state(dim, n, seed):
    rng = np.random.default_rng(seed)
    vel = np.zeros((n, 3))
    vel[:, :dim] = 0.8 + rng.uniform(-0.4, 0.4, (n, dim))
    volume = 10.**rng.uniform(-6.5, -4.5, n)
    mass = volume*rng.uniform(0.5, 2., n)
    return vel, mass, volume


def reference_sim(box, sides, g, dim, nu):
    return F.Sim(box, sides, fluid(g, dim), g.dt, viscosity=((lambda cell: nu) if nu else None, None, None),
                 g=GRAVITY, root=F.sqrt_root)


def reference_list(pos, ids, vel, mass, volume):
    return [F.Particulate(p, i, v, m, w) for p, i, v, m, w in
            zip(pos.tolist(), ids.tolist(), vel.tolist(), mass.tolist(), volume.tolist())]


def assert_lists_equal(pl, plist, what):
    p, i = pl.download()
    assert pl.count() == len(plist) == len(i), what
    assert np.array_equal(i, np.array([q.id for q in plist], dtype=np.uint32)), what
    assert np.array_equal(p, np.array([q.pos for q in plist]).reshape(-1, 3)), ("positions", what)
    vel, mass, force = pl.particulate_state()
    assert np.array_equal(vel, np.array([q.vel for q in plist]).reshape(-1, 3)), ("velocity", what)
    assert np.array_equal(mass, np.array([q.mass for q in plist])), ("mass", what)
    assert np.array_equal(force, np.array([q.force for q in plist]).reshape(-1, 3)), ("force", what)
    assert not np.isnan(force).any()


@pytest.mark.parametrize("name,nu,order", [("square", NU, ORDER_A), ("graded", 0., ORDER_B), ("walls2", NU, ORDER_B),
                                           ("cube", NU, ORDER_A), ("box3", 0., ORDER_B), ("ell", NU, ORDER_A),
                                           ("square", NU, (F.DRAG,)), ("square", 0., (F.DRAG,))])
def test_forces_on_fluid(name, nu, order):
    dim, _refine, sides = C.spec(name)
    box, flags = restatement(name)
    g, _ = start_tree(name, nu)
    pos, ids = TC.seeds(box, 3)
    vel, mass, volume = particulate_state(dim, len(ids), 17)
    pl = g.particulates(pos, ids, vel, mass, volume)
    plist = reference_list(pos, ids, vel, mass, volume)
    sim = reference_sim(box, sides, g, dim, nu)
    forces = [F.ForceCoeff(k) for k in order]
    pl.set_forces(list(order), GRAVITY)
    TF.read_forces(sim, forces)
    g.step()                                  # Un, Vn, Wn now differ from U, V, W
    sim.set_velocity(fluid(g, dim))
    sim.dt = g.dt
    before = (pl.download(), pl.particulate_state()[0], pl.count())
    prev = [levels(g, v) for v in [G.UPREV, G.VPREV, G.WPREV][:dim]]
    g.forces_on_fluid(pl)
    TW.forces_on_fluid(sim, plist, forces)
    assert_lists_equal(pl, plist, (name, "forces on the fluid"))
    force = pl.particulate_state()[2]
    if nu or len(order) > 1:
        assert np.abs(force).max() > 0.
    else:
        assert not force.any()                # no drag without viscosity
    outside = np.array([box.locate(p) is None for p in pos.tolist()])
    assert outside.sum() >= dim and not force[outside].any()          # without a leaf: the zero force, still listed
    if F.ADDEDMASS in order:
        assert (pl.particulate_state()[1][~outside] > mass[~outside]).all()
        assert np.array_equal(pl.particulate_state()[1][outside], mass[outside])
    # nothing moved, nobody left, Un stays
    after = (pl.download(), pl.particulate_state()[0], pl.count())
    assert np.array_equal(before[0][0], after[0][0]) and np.array_equal(before[0][1], after[0][1])
    assert np.array_equal(before[1], after[1]) and before[2] == after[2] == len(ids)
    for a, var in zip(prev, [G.UPREV, G.VPREV, G.WPREV]):
        for l in range(g.depth + 1):
            assert np.array_equal(a[l], g.download(var, l), equal_nan=True)
    # the next event starts from that state: the added mass persists
    pl.event()
    plist = TF.list_event(sim, plist, forces)
    assert_lists_equal(pl, plist, (name, "event"))
    assert np.array_equal(pl.download_old(), np.array([q.pos_old for q in plist]).reshape(-1, 3))
    pl.destroy()
    g.destroy()


# -------------------------------------------------------------------------------------------------
# spreading
# -------------------------------------------------------------------------------------------------

def spreading_setup(name):
    """the tree after start, a list of C.spread_particles whose stored forces are the device's drag times volume"""
    dim = C.spec(name)[0]
    box, flags = restatement(name)
    g, _ = start_tree(name, NU)
    pos, ids, volume, _force = C.spread_particles(box)
    rng = np.random.default_rng(41)
    vel = np.zeros((len(ids), 3))
    vel[:, :dim] = 0.8 + rng.uniform(-0.4, 0.4, (len(ids), dim))
    pl = g.particulates(pos, ids, vel, 2.*volume, volume)
    pl.set_sort_interval(0)
    pl.set_forces([F.DRAG], (0., 0., 0.))
    g.forces_on_fluid(pl)
    force = pl.particulate_state()[2]
    inside = np.array([box.locate(p) is not None for p in pos.tolist()])
    assert (np.abs(force[inside, :dim]).max(axis=1) > 0.).all()
    return g, flags, box, pl, C.parts(pos, ids, volume, force), force


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("name", C.REFINED)
def test_spreading(name, k):
    dim = C.spec(name)[0]
    g, flags, box, pl, plist, force = spreading_setup(name)
    rkernel = C.rkernels(box)[k]
    want, corr, reached = TW.spread(box, plist, rkernel, C.POLY[1])
    assert sum(c > 1e-10 for c in corr) >= 20 and not corr[-1] > 1e-10      # the last one deposits nothing
    if k > 0:
        assert max(len(set(x.level for x in r)) for r in reached) >= (3 if name == "graded" and k == 2 else 2)
    g.set_kernel(pl, rkernel, C.POLY[0])
    for c in range(dim):                      # the event resets the leaves
        for l in range(g.depth + 1):
            a = np.zeros(flags[l].shape)
            a[(slice(1, -1),)*dim] = 7.
            g.upload(FVARS[c], l, a)
    g.spread_forces(pl)
    first = [levels(g, FVARS[c]) for c in range(dim)]
    for c in range(dim):
        assert_field_on_leaves(g, FVARS[c], want[c], flags, (name, k, c))
        assert max(np.abs(np.array(want[c][l])).max() for l in range(g.depth + 1)) > 0.
        for l in range(g.depth + 1):          # the ghost cells stay 0: no periodic wrap, no boundary condition
            assert not first[c][l][ghost_leaf_mask(flags, l, dim)].any()
    g.spread_forces(pl)
    second = [levels(g, FVARS[c]) for c in range(dim)]
    pl.sort()
    g.spread_forces(pl)
    third = [levels(g, FVARS[c]) for c in range(dim)]
    for c in range(dim):
        for l in range(g.depth + 1):
            assert np.array_equal(first[c][l], second[c][l]) and np.array_equal(first[c][l], third[c][l]), (c, l)
    assert np.array_equal(pl.particulate_state()[2], force)                  # the stored forces are inputs
    pl.destroy()
    g.destroy()


@pytest.mark.parametrize("name", ["square", "cube"])
def test_spreading_with_a_kernel_of_the_device_libm(name):
    """exp of the device's libm against glibc's: both within 1 ulp, K/correction carries two such values, the sums
    of a leaf a few dozen of them: 1e-13 of the largest value of the field, as on the box"""
    dim = C.spec(name)[0]
    g, flags, box, pl, plist, force = spreading_setup(name)
    rkernel = C.rkernels(box)[1]
    g.set_kernel(pl, rkernel, C.GAUSS[0])
    g.spread_forces(pl)
    want, corr, _ = TW.spread(box, plist, rkernel, C.GAUSS[1])
    assert sum(c > 1e-10 for c in corr) >= 20
    for c in range(dim):
        scale = max(np.abs(np.array(want[c][l])).max() for l in range(g.depth + 1))
        assert scale > 0.
        for l in range(g.depth + 1):
            m = flags[l] == T.LEAF
            err = np.abs(g.download(FVARS[c], l)[m] - np.array(want[c][l])[m]).max()/scale if m.any() else 0.
            print("exp kernel %s F[%d] level %d: %.3e of the largest value" % (name, c, l, err))
            assert err <= 1e-13, (c, l)
    pl.destroy()
    g.destroy()


def test_source_particulate_event_and_the_kernels_that_are_refused():
    name = "square"
    dim = 2
    g, flags, box, pl, plist, force = spreading_setup(name)
    r1 = C.rkernels(box)[1]
    # source_particulate_init: rkernel = 0, kernel = 0: nothing is deposited
    g.source_particulate_event(pl)
    assert all(not g.download(FVARS[c], l).any() for c in range(dim) for l in range(g.depth + 1))
    # a constant compiles nothing; the event = the forces (the same again: nothing moved), then the spreading
    g.set_kernel(pl, r1, "0.25")
    g.source_particulate_event(pl)
    assert np.array_equal(pl.particulate_state()[2], force)
    want, _, _ = TW.spread(box, plist, r1, lambda x, y, z, t: 0.25)
    for c in range(dim):
        assert_field_on_leaves(g, FVARS[c], want[c], flags, c)
    with pytest.raises(gfship.GfshipError, match="gfship error -1: .*does not compile"):
        g.set_kernel(pl, r1, "1. +* nonsense(")
    # the slots of this tree at rkernel = 40: min (.., 2^l)^2 per level, 16 + 64: fine.  A quadtree with leaves of
    # the levels 5 to 11: a kernel that covers the box could reach 4^5 + ... + 4^11 leaves, more than the 2^22 slots
    # of a chunk, and is refused; a small one is not
    g.set_kernel(pl, 40., "1.")
    pl.destroy()
    g.destroy()
    big = gfship.Tree(lambda x, y: 11 if (0. < x < 1./32. and 0. < y < 1./32.) else 5, dim=2)
    assert big.depth == 11
    n = 2
    bl = big.particulates(np.zeros((n, 3)), np.arange(n), np.zeros((n, 3)), np.ones(n), np.ones(n))
    with pytest.raises(gfship.GfshipError, match="gfship error -5: .*chunk"):
        big.set_kernel(bl, 0.75, "1.")
    big.set_kernel(bl, 0.01, "1.")
    bl.destroy()
    big.destroy()


# -------------------------------------------------------------------------------------------------
# a uniform tree against the uniform box
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,level", [(2, 4), (3, 3)])
def test_uniform_tree_equals_uniform_box(dim, level):
    refine = (lambda x, y: level) if dim == 2 else (lambda x, y, z: level)
    g = gfship.Tree(refine, dim=dim)
    dom = gfship.Domain(dim, level, side=[gfship.SIDE_PERIODIC]*6)
    sim = gfship.Simulation(dom)
    u0 = TC.initial_velocity("uniform2" if dim == 2 else "cube", g.centres(level))
    n = 1 << level
    h = 1./n
    for c in range(dim):
        a = np.ascontiguousarray(np.broadcast_to(u0[c], (n + 2,)*dim))
        g.upload(UVARS[c], level, a)
        sim.u[c].upload(a)
    for p in (g.projection_params, g.approx_projection_params, sim.projection_params, sim.approx_projection_params):
        p.tolerance = 1e-4
    g.set_time(1e30, 0.8)
    sim.set_time(1e30)
    sim.advection_params.cfl = 0.8
    rng = np.random.default_rng(dim)
    m = 200
    pos = np.zeros((m, 3))
    pos[:, :dim] = rng.uniform(-0.5, 0.5, (m, dim))
    pos[:10, :dim] = pos[10:20, :dim] + 0.01*h          # several per cell
    pos[20, 0] = 0.5000001                              # outside
    ids = np.arange(m, dtype=np.uint32)
    vel, mass, _ = particulate_state(dim, m, 29)
    volume = 10.**rng.uniform(-3., -1., m)
    tl, ul = g.particulates(pos, ids, vel, mass, volume), gfship.ParticleList(sim, pos, ids)
    ul.set_particulate(vel, mass, volume)
    g.start()
    sim.start()
    tl.set_forces(list(ORDER_A), GRAVITY)
    ul.set_forces(list(ORDER_A), GRAVITY)
    g.step()
    sim.step()
    assert g.dt == sim.dt
    g.set_viscosity(0, NU)
    sim.set_viscosity(0, NU)
    g.forces_on_fluid(tl)
    ul.forces_on_fluid()
    g.set_viscosity(0, 0.)
    sim.set_viscosity(0, 0.)
    for a, b in zip(tl.particulate_state(), ul.particulate_state()):
        assert np.array_equal(a, b)
    assert np.abs(tl.particulate_state()[2]).max() > 0.
    v = dom.variable()
    Fb = [dom.variable() for _ in range(dim)]
    g.particulate_field(tl)
    ul.particulate_field(v)
    inner = (slice(1, -1),)*dim
    assert np.array_equal(g.download(G.VF, level)[inner], v.download()[inner]) and v.download().max() > 0.
    for rk in (0., 1.5*h, 2.5*h):
        g.set_kernel(tl, rk, C.POLY[0])
        ul.set_kernel(rk, C.POLY[0])
        g.spread_forces(tl)
        ul.spread_forces(Fb)
        for c in range(dim):
            got, want = g.download(FVARS[c], level), Fb[c].download()
            assert np.array_equal(got[inner], want[inner]) and np.abs(want).max() > 0., (rk, c)
    for x in (tl, ul, sim, dom, g):
        x.destroy()


def test_spreading_in_two_chunks_on_a_uniform_octree():
    """the chunk loop with a second chunk, as in tests/test_gpu_two_way.py: the uniform octree of level 5 and
    rkernel = 16 h.  The record slots of a particle are those of the levels that hold leaves, min (floor (2 (rkernel
    + (h/2) sqrt (3))/h) + 2, 2^level)^3 for the one level of this tree -- the stride of the box -- and 130 particles
    times that many slots do not fit the 2^22 slots of a chunk.  Bit for bit the restatement of the box on the
    forces of the device, which are order-sensitive inputs"""
    level = BC.CHUNKS_DEPTH
    n = 1 << level
    h = 1./n
    rkernel = BC.CHUNKS_RKERNEL_H*h
    pos, ids, vel, mass, volume, _ = BC.spreading_chunks_case()
    stride = min(int(np.floor(2.*(rkernel + h/2.*np.sqrt(3.))/h)) + 2, n)**3
    assert stride == n**3 and len(pos)*stride > 1 << 22 and (1 << 22)//stride == BC.CHUNKS_PER_CHUNK < len(pos)
    g = gfship.Tree(lambda x, y, z: level, dim=3)
    u0 = TC.initial_velocity("cube", g.centres(level))
    for c in range(3):
        g.upload(UVARS[c], level, np.ascontiguousarray(np.broadcast_to(u0[c], (n + 2,)*3)))
    for p in (g.projection_params, g.approx_projection_params):
        p.tolerance = 1e-4
    g.set_time(1e30, 0.8)
    pl = g.particulates(pos, ids, vel, mass, volume)
    pl.set_sort_interval(0)
    try:
        g.start()
        g.set_viscosity(0, NU)
        pl.set_forces([F.DRAG], (0., 0., 0.))
        g.forces_on_fluid(pl)
        force = pl.particulate_state()[2]
        assert (np.abs(force).max(axis=1) > 0.).all()
        want = BC.assert_two_chunks_are_order_sensitive(BR, pos, volume, force)
        g.set_kernel(pl, rkernel, BC.CHUNKS_TEXT)
        g.spread_forces(pl)
        inner = (slice(1, -1),)*3
        for c in range(3):
            assert np.array_equal(g.download(FVARS[c], level)[inner], want[c]), c
    finally:
        pl.destroy()
        g.destroy()


# -------------------------------------------------------------------------------------------------
# the MAC value of the source fields
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.ALL)
def test_mac_source(name):
    dim, _refine, sides = C.spec(name)
    box, flags = restatement(name)
    g, _ = start_tree(name, 0.)
    g.set_source_fields(True)
    census = TW.new_census()
    plain = []
    for c in range(dim):
        vals = TC.distinct_values(dim, flags, salt=c)
        for l in range(g.depth + 1):
            g.upload(FVARS[c], l, np.nan_to_num(vals[l]))
        g.set_source(c, 3.)                   # the constant of a GfsSource is not part of this sum
        g.mac_source(c, G.RES)
        want = TW.mac_source(box, c, box.field(vals), census, sides)
        for l in range(g.depth + 1):
            m = np.zeros(flags[l].shape, dtype=bool)
            m[(slice(1, -1),)*dim] = flags[l][(slice(1, -1),)*dim] == T.LEAF
            assert np.array_equal(g.download(G.RES, l)[m], np.array(want[l])[m]), (name, c, l)
        plain.append(levels(g, G.RES))
    assert census[TW.SAME_LEAF] > 0 and census[TW.NO_NEIGHBOR] == 0
    if name != "uniform2":
        assert census[TW.COARSER] > 0 and census[TW.CHILDREN] > 0, dict(census)
    assert census[TW.GHOST_BOUNDARY if name == "walls2" else TW.GHOST_PERIODIC] > 0
    if name == "box3":
        assert census[TW.GHOST_BOUNDARY] > 0 and census[TW.GHOST_PERIODIC] > 0
    # with a viscosity: 0. + F-term + the source of the diffusion
    if name in ("square", "cube", "walls2"):
        for c in range(dim):
            g.set_viscosity(c, 1e-2)
        for c in range(dim):
            g.set_source_fields(False)
            g.mac_source(c, G.DIV)
            diffusion = levels(g, G.DIV)
            g.set_source_fields(True)
            g.mac_source(c, G.DIV)
            for l in range(g.depth + 1):
                m = np.zeros(flags[l].shape, dtype=bool)
                m[(slice(1, -1),)*dim] = flags[l][(slice(1, -1),)*dim] == T.LEAF
                assert np.array_equal(g.download(G.DIV, l)[m], (0. + plain[c][l][m]) + diffusion[l][m]), (c, l)
                assert not m.any() or np.abs(diffusion[l][m]).max() > 0.
    g.destroy()


# -------------------------------------------------------------------------------------------------
# the time step
# -------------------------------------------------------------------------------------------------

def run_steps(name, nu, fields, nsteps=3):
    dim = C.spec(name)[0]
    g, flags = make_tree(name)
    for l in range(g.depth + 1):
        for var, a in zip(UVARS, TC.initial_velocity("square" if name == "ell" else name, g.centres(l))):
            g.upload(var, l, np.ascontiguousarray(np.broadcast_to(0.05*a, flags[l].shape)))
    for p in (g.projection_params, g.approx_projection_params):
        p.tolerance = 1e-4
    for c in range(dim):
        if nu:
            g.set_viscosity(c, nu)
        if fields:
            for l in range(g.depth + 1):
                g.upload(FVARS[c], l, np.full(flags[l].shape, C.G_UNIFORM[c]))
        else:
            g.set_source(c, C.G_UNIFORM[c])
    if fields:
        g.set_source_fields(True)
    g.set_time(1e30, CFL)
    g.start()
    out = [(g.t, g.dt)]
    for _ in range(nsteps):
        g.step()
        out.append((g.t, g.dt))
    state = [[g.download(var, l)[flags[l] == T.LEAF] for l in range(g.depth + 1)] for var in UVARS[:dim] + [G.P]]
    g.destroy()
    return out, state


@pytest.mark.parametrize("nu", [0., 1e-2])
@pytest.mark.parametrize("name", C.uniform_field_trees())
def test_uniform_source_fields_are_a_gfs_source(name, nu):
    """F_c = g on every cell of every level, ghosts included: U, V(, W), P on the leaves, every dt and t are those
    of gfship_tree_set_source, bit for bit (the premise: tests/test_tree_two_way_reference_cpu.py)"""
    ta, sa = run_steps(name, nu, True)
    tb, sb = run_steps(name, nu, False)
    assert ta == tb and ta[1][1] > 0.
    for va, vb in zip(sa, sb):
        for a, b in zip(va, vb):
            assert np.array_equal(a, b)
    if nu == 0.:
        # the acceleration sets the first time step (gfs_domain_cfl, src/domain.c:2882-2891: 2 length/|g| on the
        # finest leaves against (length/|u|)^2 with |u| <= 0.05): the source fields are read there too
        h = C.h_fine(restatement(name)[0])
        assert ta[0][1] == CFL*np.sqrt(2.*h/max(abs(x) for x in C.G_UNIFORM[:C.spec(name)[0]]))


@pytest.mark.parametrize("dim,axis", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_striped_trees(dim, axis):
    """a band that depends on one coordinate only, fluid at rest, F along an invariant axis with a distinct value
    per row of the other coordinates: after start and one step U_c == dt*F_c on every leaf, the other components and
    P are exactly 0 (the premise, with the oracle: tests/test_tree_two_way_reference_cpu.py)"""
    _dim, refine, _sides = C.striped(dim, axis)
    c = (axis + 1) % dim
    g = gfship.Tree(refine, dim=dim)
    flags = [g.flags(l) for l in range(g.depth + 1)]
    Fc = []
    for l in range(g.depth + 1):
        cs = g.centres(l)
        a = np.zeros(flags[l].shape)
        for b in range(dim):
            if b != c:                        # a function of the other coordinates alone: dyadic, distinct per row
                a = a + np.round(64.*(cs[b] + 0.*cs[0]))/4.*(1 + b) + l
        Fc.append(np.ascontiguousarray(np.broadcast_to(a - 16., flags[l].shape)))
        g.upload(FVARS[c], l, Fc[l])
    g.set_source_fields(True)
    g.set_time(1e30, 0.8)
    g.start()
    dt = g.dt
    g.step()
    assert dt > 0. and g.t == dt
    seen = 0
    for l in range(g.depth + 1):
        m = np.zeros(flags[l].shape, dtype=bool)
        m[(slice(1, -1),)*dim] = flags[l][(slice(1, -1),)*dim] == T.LEAF
        if not m.any():
            continue
        seen += 1
        for a, var in enumerate(UVARS[:dim]):
            want = dt*Fc[l][m] if a == c else np.zeros(int(m.sum()))
            assert np.array_equal(g.download(var, l)[m], want), (l, a)
        assert len(set(Fc[l][m].tolist())) > 1
        assert np.array_equal(g.download(G.P, l)[m], np.zeros(int(m.sum()))), l
    assert seen == 2
    g.destroy()


# -------------------------------------------------------------------------------------------------
# refusals and lifetimes
# -------------------------------------------------------------------------------------------------

def test_refusals_and_lifetimes():
    g, flags = make_tree("square")
    n = 4
    z3, one = np.zeros((n, 3)), np.ones(n)
    tracers = g.particles(z3, np.arange(n))
    dom = gfship.Domain(2, 3, side=[gfship.SIDE_PERIODIC]*6)
    sim = gfship.Simulation(dom)
    boxlist = gfship.ParticleList(sim, z3, np.arange(n))
    boxlist.set_particulate(z3, one, one)
    for pl in (tracers, boxlist):
        for call in (lambda: g.particulate_field(pl), lambda: g.forces_on_fluid(pl), lambda: g.set_kernel(pl, 0.1),
                     lambda: g.spread_forces(pl), lambda: g.source_particulate_event(pl)):
            with pytest.raises(gfship.GfshipError, match="gfship error -5"):
                call()
    for var in (G.VF, G.FX, G.FY):
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            g.download(var, 0)                # they do not exist yet
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.mac_source(0, G.P)
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.mac_source(2, G.RES)
    pl = g.particulates(z3, np.arange(n), z3, one, 1e-3*one)
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        gfship._check(gfship.lib().gfship_tree_particulate_field(pl.ptr, G.FX))
    g.particulate_field(pl)
    assert g.download(G.VF, g.depth).max() > 0.
    with pytest.raises(gfship.GfshipError, match="gfship error -1"):
        g.download(G.FX, 0)                   # the void fraction does not make the forces
    g.set_source_fields(True)
    assert not g.download(G.FX, 0).any() and not g.download(G.FY, g.depth).any()
    for call in (lambda: g.download(G.FZ, 0), lambda: g.upload(G.FZ, 0, np.zeros((3, 3)))):
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            call()                            # a quadtree has no Fz
    # once they exist: the sampler and the snapshot take them like any variable
    a = TC.distinct_values(2, flags, salt=5)
    for l in range(g.depth + 1):
        g.upload(G.FX, l, np.nan_to_num(a[l]))
    out, inside = g.interpolate(G.FX, np.array([[0.3, 0.3, 0.]]))
    assert inside.all() and 0.5 <= out[0] < 1.5
    image = g.snapshot([G.U, G.FX])
    g.upload(G.FX, g.depth, np.zeros(flags[g.depth].shape))
    g.snapshot_read([G.U, G.FX], image)
    m = np.zeros(flags[g.depth].shape, dtype=bool)
    m[1:-1, 1:-1] = flags[g.depth][1:-1, 1:-1] == T.LEAF
    assert np.array_equal(g.download(G.FX, g.depth)[m], a[g.depth][m])
    for x in (pl, tracers, boxlist, sim, dom, g):
        x.destroy()
