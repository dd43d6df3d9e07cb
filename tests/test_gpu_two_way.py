"""Two-way coupling on the device: GfsParticulateField, the forces of the fluid on the particles and the
spreading of GfsSourceParticulate (modules/particulatecommon.c:1927-2228), against the restatement of
tests/two_way_reference.py bit for bit, and the forces against the oracle's particulate event."""
import numpy as np
import pytest

import gfship
import two_way_reference as R
from flow_cases import PERIODIC, oracle_reynolds, oracle_taylor_green
from oracle import oracle as O
from two_way_cases import (BOXES, CHUNKS_DEPTH, CHUNKS_PER_CHUNK, CHUNKS_RKERNEL_H, CHUNKS_TEXT, EXP_TEXT, POLY_TEXT,
                           RKERNEL_H, alpha_cell_case, assert_two_chunks_are_order_sensitive, device_sim, exp_kernel,
                           spreading_chunks_case,
                           poly_kernel, spreading_case, void_fraction_case)

pytestmark = pytest.mark.gpu

# periodic along x and z, walls along y
SIDES = [gfship.SIDE_PERIODIC, gfship.SIDE_PERIODIC, gfship.SIDE_BOUNDARY, gfship.SIDE_BOUNDARY,
         gfship.SIDE_PERIODIC, gfship.SIDE_PERIODIC]
NU = 1e-2


def _interior(a, dim):
    return a[(slice(1, -1),) * dim]


def _rel_err(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _flow_sim(dim, depth, sides=SIDES):
    """a device simulation holding a smooth velocity (ghost cells included), with a viscosity"""
    n = 1 << depth
    gd = gfship.Domain(dim, depth, sides)
    gs = gfship.Simulation(gd)
    x = -0.5 + (np.arange(n + 2) - 0.5) / n
    g = np.meshgrid(*([x] * dim), indexing="ij")
    X, Y = g[-1], g[-2]                              # arrays are indexed [k][j][i]
    Z = g[0] if dim == 3 else np.zeros_like(X)
    tp = 2. * np.pi
    u = [np.sin(tp * X) * np.cos(tp * Y) * (1. + 0.3 * np.cos(tp * Z)),
         -np.cos(tp * X) * np.sin(tp * Y) * (1. + 0.2 * np.sin(tp * Z)),
         0.4 * np.sin(tp * (X + Y + Z))]
    for c in range(dim):
        gs.u[c].upload(u[c])
        gs.set_viscosity(c, NU)
    return gd, gs


# ---- GfsParticulateField ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim,depth", BOXES)
def test_void_fraction_is_the_list_order_sum(dim, depth):
    pos, ids, volume = void_fraction_case(dim, depth)
    want = R.void_fraction(dim, depth, pos, volume)
    gd, gs = _flow_sim(dim, depth, PERIODIC)
    gpl = gfship.ParticleList(gs, pos, ids)
    try:
        gpl.set_sort_interval(0)
        gpl.set_particulate(np.zeros((len(ids), 3)), volume, volume)
        v = gd.variable()
        v.fill(3.)                                   # the event resets the variable
        gpl.particulate_field(v)
        full = v.download()
        got = _interior(full, dim)
        assert np.array_equal(got, want)
        # nothing is written beside the cells of the box
        ghosts = full.copy()
        ghosts[(slice(1, -1),) * dim] = 0.
        assert not ghosts.any()
        # the particle outside is skipped, not taken off the list
        assert gpl.count() == len(ids)
        # wherever the particles are stored
        gpl.sort()
        gpl.particulate_field(v)
        assert np.array_equal(_interior(v.download(), dim), want)
        gpl.particulate_field(v)
        assert np.array_equal(_interior(v.download(), dim), want)
        # same particles, same order after the sort
        p2, i2 = gpl.download()
        assert np.array_equal(i2, ids) and np.array_equal(p2, pos)
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


# ---- the forces of the fluid on the particles ------------------------------------------------------

FORCE_LISTS = {
    "drag": [O.FORCE_DRAG],
    "all-but-buoy": [O.FORCE_INERTIAL, O.FORCE_ADDEDMASS, O.FORCE_LIFT, O.FORCE_DRAG],
    "drag-buoy": [O.FORCE_DRAG, O.FORCE_BUOY],
}


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("name", list(FORCE_LISTS))
def test_forces_on_fluid_against_the_oracle(name, dim):
    """after one event and one time step (so that Un differs from U): the stored force after
    gfship_particles_forces_on_fluid is the oracle's force after an event of the same state with the list
    without buoyancy.  Positions, ids and velocities stay; the mass of a particle inside the box grows by
    fluid_rho*volume*cm per GfsForceAddedMass of the list, as compute_addedmass_force adds it when
    compute_forces_onfluid calls it (modules/particulatecommon.c:391, :757) -- the oracle has no such call,
    its masses get the same addition here -- and the next event is the oracle's"""
    forces = FORCE_LISTS[name]
    without_buoy = [f for f in forces if f != O.FORCE_BUOY]
    gravity = (0., 0.5, 0.)
    osim = oracle_taylor_green(4) if dim == 3 else oracle_reynolds(4)
    for c in range(dim):
        osim.set_viscosity(c, NU)
    rng = np.random.default_rng(17)
    npart = 400
    pos = 0.98 * (rng.random((npart, 3)) - 0.5)
    vel = 0.3 * rng.standard_normal((npart, 3))
    if dim == 2:
        pos[:, 2] = 0.
        vel[:, 2] = 0.
    ids = np.arange(1, npart + 1, dtype=np.uint32)
    vol = 1e-3 * (0.5 + rng.random(npart))
    mass = vol * (0.5 + 2.5 * rng.random(npart))
    gd, gs = device_sim(gfship, osim, PERIODIC)
    if dim == 2:
        gs.set_time(end=2.)
    for c in range(dim):
        gs.set_viscosity(c, NU)
    osim.start()
    gs.start()
    lists = [O.Particles(osim, pos, ids), O.Particles(osim, pos, ids)]
    gpl = gfship.ParticleList(gs, pos, ids)
    try:
        gpl.set_sort_interval(2)
        for pl in lists + [gpl]:
            pl.set_particulate(vel, mass, vol)
            pl.set_forces(forces, gravity)
        for pl in lists + [gpl]:
            pl.event()
        osim.step()
        gs.step()
        before = gpl.download() + gpl.particulate_state()
        gpl.forces_on_fluid()
        after = gpl.download() + gpl.particulate_state()
        for k in (0, 1, 2):      # positions, ids, velocities
            assert np.array_equal(before[k], after[k]), k
        ref, full = lists
        added = forces.count(O.FORCE_ADDEDMASS)

        def with_added_mass(positions, masses, listed_ids):
            inside = np.array([full.locate(p) is not None for p in positions])
            v = vol[np.searchsorted(ids, listed_ids)]
            m = masses.copy()
            for _ in range(added):
                m[inside] += 1. * v[inside] * 0.5
            return m
        want = with_added_mass(before[0], before[3], before[1])
        assert np.array_equal(after[3], want)
        if added:
            assert (after[3] > before[3]).sum() > npart * 8 // 10
        gf = after[4]
        if dim == 2:
            assert not gf[:, 2].any()
        # the oracle: the same state, the list without buoyancy
        ref.set_forces(without_buoy, gravity)
        ref.event()
        oi = ref.state()[1]
        of = ref.particulate_state()[2]
        at = np.searchsorted(after[1], oi)
        assert len(oi) > npart * 9 // 10
        err = _rel_err(gf[at], of)
        print("forces on the fluid, %s %d-D: %.3e relative" % (name, dim, err))
        assert err <= 1e-12
        if O.FORCE_BUOY in forces:
            assert _rel_err(before[4][at], of) > 1e-3        # buoyancy is in the event's force, not here
        # Un, Vn, Wn are what the event left, the masses carry what the evaluation added: the next event is
        # the oracle's on those masses
        op, oi = full.state()
        om = np.ctypeslib.as_array(O.lib().go_particles_mass(full.ptr), shape=(len(oi),))
        om[...] = with_added_mass(op, om, oi)
        full.event()
        gpl.event()
        op, oi = full.state()
        gp, gi = gpl.download()
        assert np.array_equal(oi, gi)
        ov, om, of2 = full.particulate_state()
        gv, gm, gf2 = gpl.particulate_state()
        for a, b, what in ((op, gp, "pos"), (ov, gv, "vel"), (of2, gf2, "force"), (om, gm, "mass")):
            assert _rel_err(b, a) <= 1e-12, what
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


# ---- the spreading ---------------------------------------------------------------------------------

def _spreading_setup(dim, depth, with_alpha=True, case=spreading_case):
    pos, ids, vel, mass, volume, _ = case(dim, depth)
    gd, gs = _flow_sim(dim, depth)
    alpha = None
    if with_alpha:
        alpha = alpha_cell_case(dim, depth)
        a = gd.variable()
        for l in range(depth):
            a.fill(1., l)
        full = np.ones(((1 << depth) + 2,) * dim)
        full[(slice(1, -1),) * dim] = alpha
        a.upload(full)
        gs.set_alpha_cell(a)
    gpl = gfship.ParticleList(gs, pos, ids)
    gpl.set_sort_interval(0)
    gpl.set_particulate(vel, mass, volume)
    gpl.set_forces([O.FORCE_DRAG], (0., 0., 0.))
    gpl.forces_on_fluid()
    force = gpl.particulate_state()[2]
    # the forces the device hands to the spreading: drag times volume, over six decades
    mag = np.abs(force[:, :dim]).max(axis=1)
    assert mag.min() > 0. and (case is not spreading_case or mag.max() / mag.min() > 1e5)
    F = [gd.variable() for _ in range(dim)]
    return gd, gs, gpl, F, (pos, volume, force, alpha)


def _download(F, dim):
    return [_interior(f.download(), dim) for f in F]


@pytest.mark.parametrize("rk", RKERNEL_H)
@pytest.mark.parametrize("dim,depth", BOXES)
def test_spreading_is_the_list_order_sum(dim, depth, rk):
    h = 1. / (1 << depth)
    gd, gs, gpl, F, (pos, volume, force, alpha) = _spreading_setup(dim, depth)
    try:
        want, corr = R.spread(dim, depth, pos, volume, force, rk * h, poly_kernel, alpha_cell=alpha)
        assert (corr > 1.e-10).sum() >= 20 and not corr[40] > 1.e-10
        if rk > 0.:      # the device's forces make an order-sensitive input too
            rev, _ = R.spread(dim, depth, pos[::-1], volume[::-1], force[::-1], rk * h, poly_kernel,
                              alpha_cell=alpha)
            assert any(not np.array_equal(want[c], rev[c]) for c in range(dim))
        gpl.set_kernel(rk * h, POLY_TEXT)
        for f in F:
            f.fill(7.)                               # the event resets the fields
        gpl.spread_forces(F)
        first = _download(F, dim)
        for c in range(dim):
            assert np.array_equal(first[c], want[c]), c
            full = F[c].download()
            full[(slice(1, -1),) * dim] = 0.
            assert not full.any()                    # no cell beside the box is written: no periodic wrap
        # from run to run, and wherever the particles are stored
        gpl.spread_forces(F)
        second = _download(F, dim)
        gpl.sort()
        gpl.spread_forces(F)
        third = _download(F, dim)
        for c in range(dim):
            assert np.array_equal(first[c], second[c]) and np.array_equal(first[c], third[c]), c
        # the stored forces are inputs: unchanged
        assert np.array_equal(gpl.particulate_state()[2], force)
        # the measured call is the same call; its record slots bound the leaves any particle reaches
        ms1, ms2, stride, per_chunk, nbytes = gpl.time_spreading(F)
        fourth = _download(F, dim)
        for c in range(dim):
            assert np.array_equal(first[c], fourth[c]), c
        reach = max(len(R.descent(dim, depth, list(p), rk * h)) for p in pos)
        m = min(int(np.floor(2. * (rk * h + h / 2. * np.sqrt(dim)) / h)) + 2, 1 << depth)
        assert stride == m ** dim and reach <= stride
        assert per_chunk == len(pos) and nbytes == 56 * per_chunk * stride <= 56 << 22
        assert ms1 > 0. and ms2 > 0.
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


@pytest.mark.parametrize("with_alpha", [True, False])
def test_spreading_in_two_chunks(with_alpha):
    """the chunk loop with a second chunk: 32^3 box, rkernel = 16 h, so a particle owns 32^3 record slots and a chunk
    holds 2^22/32^3 = 128 particles; 130 particulates.  The additions into a cell keep the list order across the
    chunks: bit for bit the restatement, whose inputs (the device's forces) are order-sensitive"""
    dim, depth = 3, CHUNKS_DEPTH
    h = 1. / (1 << depth)
    gd, gs, gpl, F, (pos, volume, force, alpha) = _spreading_setup(dim, depth, with_alpha,
                                                                   lambda dim, depth: spreading_chunks_case())
    try:
        want = assert_two_chunks_are_order_sensitive(R, pos, volume, force, alpha)
        gpl.set_kernel(CHUNKS_RKERNEL_H * h, CHUNKS_TEXT)
        for f in F:
            f.fill(7.)
        ms1, ms2, stride, per_chunk, nbytes = gpl.time_spreading(F)
        assert stride == (1 << depth) ** 3 and per_chunk == CHUNKS_PER_CHUNK < len(pos)
        assert nbytes == 56 << 22 and ms1 > 0. and ms2 > 0.
        got = _download(F, dim)
        for c in range(dim):
            assert np.array_equal(got[c], want[c]), c
        gpl.spread_forces(F)                         # the call without the timing is the same call
        again = _download(F, dim)
        for c in range(dim):
            assert np.array_equal(again[c], want[c]), c
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


@pytest.mark.parametrize("dim,depth", BOXES)
def test_source_particulate_event_without_alpha_and_the_default_kernel(dim, depth):
    h = 1. / (1 << depth)
    gd, gs, gpl, F, (pos, volume, force, _) = _spreading_setup(dim, depth, with_alpha=False)
    try:
        # source_particulate_init: rkernel = 0, kernel = 0: nothing is deposited
        for f in F:
            f.fill(7.)
        gpl.source_particulate_event(F)
        assert all(not f.download().any() for f in F)
        # a constant kernel compiles nothing; the event = the forces, then the spreading
        gpl.set_kernel(1.5 * h, "0.25")
        gpl.source_particulate_event(F)
        assert np.array_equal(gpl.particulate_state()[2], force)
        want, _ = R.spread(dim, depth, pos, volume, force, 1.5 * h, lambda x, y, z, t: 0.25)
        got = _download(F, dim)
        for c in range(dim):
            assert np.array_equal(got[c], want[c]), c
        # back to the default
        gpl.set_kernel(0.)
        gpl.source_particulate_event(F)
        assert all(not f.download().any() for f in F)
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


@pytest.mark.parametrize("dim,depth", BOXES)
def test_spreading_with_a_kernel_of_the_device_libm(dim, depth):
    """exp of the device's libm against glibc's: both within 1 ulp, K/correction carries two such values,
    the sums of a cell a few dozen of them: 1e-13 of the largest value of the field"""
    h = 1. / (1 << depth)
    gd, gs, gpl, F, (pos, volume, force, alpha) = _spreading_setup(dim, depth)
    try:
        gpl.set_kernel(1.5 * h, EXP_TEXT)
        gpl.spread_forces(F)
        want, corr = R.spread(dim, depth, pos, volume, force, 1.5 * h, exp_kernel, alpha_cell=alpha)
        assert (corr > 1.e-10).sum() >= 20
        got = _download(F, dim)
        for c in range(dim):
            err = _rel_err(got[c], want[c])
            print("exp kernel %d-D level %d, F[%d]: %.3e relative" % (dim, depth, c, err))
            assert err <= 1e-13, c
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


# ---- refusals --------------------------------------------------------------------------------------

def test_refusals():
    gd, gs = _flow_sim(2, 4)
    pos, ids, vel, mass, volume, _ = spreading_case(2, 4)
    gpl = gfship.ParticleList(gs, pos, ids)
    try:
        v = gd.variable()
        F = [gd.variable(), gd.variable()]
        # tracers have no volume and no forces
        for call in (lambda: gpl.particulate_field(v), gpl.forces_on_fluid, lambda: gpl.set_kernel(0.1, "1."),
                     lambda: gpl.spread_forces(F), lambda: gpl.source_particulate_event(F)):
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*particulates"):
                call()
        gpl.set_particulate(vel, mass, volume)
        with pytest.raises(gfship.GfshipError, match="does not compile"):
            gpl.set_kernel(0.1, "1. +* nonsense(")
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            gpl.set_kernel(-1., "1.")
        with pytest.raises(gfship.GfshipError, match="same field"):
            gpl.spread_forces([F[0], F[0]])
        # what gfship_particles_set_forces refuses: alpha without alpha at the cell centres
        for c in range(2):
            gs.set_viscosity(c, 0.)                  # (a viscosity refuses alpha without alpha_cell by itself)
        A = [gd.variable() for _ in range(2)]
        for a in A:
            for l in range(5):
                a.fill(1., l)
        gs.set_alpha(A)
        for call in (gpl.forces_on_fluid, lambda: gpl.spread_forces(F)):
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*gfship_sim_set_alpha_cell"):
                call()
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


def test_a_box_with_mpi_sides_is_refused():
    sides = [gfship.SIDE_EXTERNAL, gfship.SIDE_EXTERNAL] + [gfship.SIDE_BOUNDARY] * 4
    gd = gfship.Domain(2, 4, sides)
    gs = gfship.Simulation(gd)
    pos, ids, vel, mass, volume, _ = spreading_case(2, 4)
    gpl = gfship.ParticleList(gs, pos, ids)
    try:
        gpl.set_particulate(vel, mass, volume)
        v = gd.variable()
        for call in (lambda: gpl.particulate_field(v), gpl.forces_on_fluid, lambda: gpl.set_kernel(0.1, "1."),
                     lambda: gpl.spread_forces([v, gd.variable()])):
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*GfsBoundaryMpi"):
                call()
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()
