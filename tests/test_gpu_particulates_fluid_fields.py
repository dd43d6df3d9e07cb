"""Particle forces in a fluid whose density and viscosity vary in space: the forces of a list of
GfsParticulate read fluid_rho = 1./alpha and the viscosity of U at the cell that holds the particle
(modules/particulatecommon.c:273-279, 349-359, 439-445, 534-541, 631-632), from gfship_sim_set_alpha_cell
and gfship_sim_set_viscosity_cell.

The oracle's particle code has fluid_rho = 1. and one viscosity, so the path is pinned from two sides:

  (1) against the oracle by an exact scaling.  Every use of fluid_rho is a product or the difference
      mass/volume - fluid_rho, the Reynolds number is norm*dia*fluid_rho/viscosity, and a factor that is a power
      of two is exact: with per-cell factors k in {1, 2, 4}, alpha_cell = 1/k and mu = k*nu0, an event of the
      device equals an event of the oracle (density 1, viscosity nu0) on the masses mass/k -- the same
      Reynolds numbers, velocities and positions, k times the force and the mass;
  (2) for general values, against a restatement of the five forces and of gfs_particulate_event in plain
      Python floats, one particle at a time, in the reference's operand order (:273-336, 349-427, 439-524,
      534-588, 631-653, 828-837), fed with the library's own sampler (Domain.interpolate, pinned on the
      cell-graph restatement of the reference by tests/test_gpu_sampler_reference.py) and the
      downloaded fields.  The build has no contraction, division and
      square root are correctly rounded on both sides: force, vel and mass must be equal bit for bit;
  (3) the refusals.
"""
import math

import numpy as np
import pytest

import gfship
import hook_cases as H
from flow_cases import PERIODIC, oracle_taylor_green, oracle_reynolds
from oracle import oracle as O
from particle_cases import lcg_positions
from test_gpu_timestep import _device_sim

pytestmark = pytest.mark.gpu

ALL_FORCES = [O.FORCE_INERTIAL, O.FORCE_ADDEDMASS, O.FORCE_LIFT, O.FORCE_DRAG, O.FORCE_BUOY]
NU0 = 1e-2


def _rel_err(a, b):
    scale = max(np.abs(a).max(), 1e-300)
    return np.abs(a - b).max() / scale


def _particulate_case(n, dim, seed):
    rng = np.random.default_rng(seed)
    pos, ids = lcg_positions(n, dim=dim)
    vel = 0.3 * rng.standard_normal((n, 3))
    if dim == 2:
        vel[:, 2] = 0.
    vol = 1e-3 * (0.5 + rng.random(n))
    mass = vol * (0.5 + 2.5 * rng.random(n))
    return pos, ids, vel, mass, vol


def _factors(dim, n):
    """k in {1, 2, 4} per leaf cell, ghosts included, indexed [k, j, i] / [j, i]"""
    idx = np.meshgrid(*([np.arange(n + 2)] * dim), indexing="ij")
    s = sum((q + 1) * a for q, a in enumerate(idx))
    return 2. ** (s % 3)


# ---------------------------------------------------------------------------------------------
# (1) exact scaling against the oracle
# ---------------------------------------------------------------------------------------------

COEFFICIENTS = {
    1: ("0.5 + 0.1*Pdia + 0.01*fabs (Wrelp)",
        lambda rep, u, v, w, d: 0.5 + 0.1 * d + 0.01 * abs(w)),
    2: ("{ double a = 0.3 + 0.1*Urelp; if (Rep > 1.) a += 0.05*Vrelp; return a; }",
        lambda rep, u, v, w, d: (0.3 + 0.1 * u) + (0.05 * v if rep > 1. else 0.)),
    3: ("24./Rep*(1. + 0.15*pow (Rep, 0.687))",
        lambda rep, u, v, w, d: 24. / rep * (1. + 0.15 * math.pow(rep, 0.687))),
}


@pytest.mark.parametrize("name", ["taylor-green-3d", "taylor-green-3d-coefficients", "periodic-2d"])
def test_scaled_fields_against_the_oracle(name):
    dim = 2 if name == "periodic-2d" else 3
    level, npart, nsteps = (5, 800, 3) if dim == 2 else (4, 1500, 3)
    osim = oracle_reynolds(level) if dim == 2 else oracle_taylor_green(level)
    for c in range(dim):
        osim.set_viscosity(c, NU0)
    pos, ids, vel, mass, vol = _particulate_case(npart, dim, 31)
    gravity = (0., 0.5, 0.)
    coefficients = COEFFICIENTS if name.endswith("coefficients") else {}
    gd, gs = _device_sim(osim, PERIODIC)
    gpl = None
    try:
        if dim == 2:
            gs.set_time(end=2.)
        for c in range(dim):
            gs.set_viscosity(c, NU0)
        osim.start()
        gs.start()
        # two lists on the oracle: one gets the scaled masses before the last event, the other runs on unscaled
        lists = [O.Particles(osim, pos, ids), O.Particles(osim, pos, ids)]
        gpl = gfship.ParticleList(gs, pos, ids)
        for pl in lists + [gpl]:
            pl.set_particulate(vel, mass, vol)
            pl.set_forces(ALL_FORCES, gravity)
        for f, (text, fn) in coefficients.items():
            for pl in lists:
                pl.set_coefficient(f, fn)
            gpl.set_force_coefficient(f, text)
        opl, unscaled = lists
        for k in range(nsteps):
            for pl in lists + [gpl]:
                pl.event()
            osim.step()
            gs.step()
        op, oi = opl.state()
        gp, gi = gpl.download()
        # (a few particles have left the list on both sides alike: gfs_particle_bc)
        assert np.array_equal(oi, gi) and len(oi) > npart * 9 // 10
        assert _rel_err(op, gp) <= 1e-12
        # the factor of the cell of every particle
        n = 1 << level
        kf = _factors(dim, n)
        # (a particle the last event left outside the box is still on the list: the next event takes it off
        # first, remove_particles_not_in_domain, on both sides; its factor is never used)
        cells = [opl.locate(p) for p in op]
        kp = np.array([1. if c is None else kf[(c[2], c[1], c[0]) if dim == 3 else (c[1], c[0])] for c in cells])
        assert (kp != 1.).sum() > npart // 3 and (kp == 1.).sum() > 0
        factor = dict(zip(oi.tolist(), kp.tolist()))
        # the device gets the two fields, the oracle's list the scaled masses
        alpha_cell, mu = gd.variable(), gd.variable()
        for l in range(level):
            alpha_cell.fill(1., l)
        alpha_cell.upload(1. / kf)
        mu.upload(kf * NU0)
        gs.set_alpha_cell(alpha_cell)
        gs.set_viscosity_cell(mu)
        L = O.lib()
        om = np.ctypeslib.as_array(L.go_particles_mass(opl.ptr), shape=(len(oi),))
        om[:] = om / kp
        for pl in lists + [gpl]:
            pl.event()
        op, oi = opl.state()
        gp, gi = gpl.download()
        assert np.array_equal(oi, gi) and len(oi) > npart * 9 // 10
        kp = np.array([factor[q] for q in oi.tolist()])
        ov, om, of = opl.particulate_state()
        gv, gm, gf = gpl.particulate_state()
        for a, b, what in ((op, gp, "pos"), (ov, gv, "vel"), (of * kp[:, None], gf, "force"), (om * kp, gm, "mass")):
            e = _rel_err(a, b)
            print(name, what, e)
            assert e <= 1e-12, (what, e)
        # the fields are really read: a fluid of density 1 and viscosity nu0 gives other forces
        uf, ui = unscaled.particulate_state()[2], unscaled.state()[1]
        common = np.intersect1d(ui, gi)
        assert len(common) > npart * 9 // 10
        assert _rel_err(uf[np.isin(ui, common)], gf[np.isin(gi, common)]) > 1e-6
    finally:
        if gpl is not None:
            gpl.destroy()
        H.destroy_device(gd, gs)


# ---------------------------------------------------------------------------------------------
# (2) general values against a restatement in plain floats
# ---------------------------------------------------------------------------------------------

def _locate(dim, level, p):
    """gfs_domain_locate on the unit box: the descent of ftt_cell_locate; 1-based (i, j, k)"""
    q, c0, size = [0, 0, 0], [0., 0., 0.], 0.5
    for l in range(level):
        size /= 2.
        for c in range(dim):
            up = p[c] > c0[c]
            q[c] = 2 * q[c] + (1 if up else 0)
            c0[c] += size if up else -size
    return tuple(q[c] + 1 if c < dim else 0 for c in range(3))


def _center_gradient(v, at, ax):
    """gfs_center_gradient, src/fluid.c:434-475, neighbours of the same level"""
    lo, hi = list(at), list(at)
    lo[ax] -= 1
    hi[ax] += 1
    v0, v1, v2 = float(v[at]), float(v[tuple(lo)]), float(v[tuple(hi)])
    return ((v2 - v0) + (v0 - v1)) / 2.


def _restated_event(dim, forces, gravity, dt, size, fvel, fveln, grad, ucell, fluid_rho, viscosity,
                    vel, mass, volume, drag_coefficient):
    """gfs_particulate_event (:768-842) of one particle: (force, vel, mass) after the event.  grad[c][c2] is
    gfs_center_gradient (cell, c2, u[c]), ucell[c] the value of u[c] at the cell.  One list of forces in one
    order, fed by the device's own interpolation; the restatement of every force on the cell graph, with
    positions, wall cells and every order of the list, is tests/forces_reference.py
    (test_gpu_forces_reference.py)."""
    vel = list(vel)
    pf = [0., 0., 0.]
    # compute_inertial_force, :285-302
    dudt = [0., 0., 0.]
    if dt > 0.:
        for c in range(dim):
            dudt[c] = fluid_rho * (fvel[c] - fveln[c]) / dt
        for c in range(dim):
            for c2 in range(dim):
                dudt[c] += fluid_rho * grad[c][c2] * ucell[c2] / size
    rel = [0., 0., 0.]
    for c in range(dim):
        rel[c] = fvel[c] - vel[c]
    for kind in forces:
        force = [0., 0., 0.]
        if kind == O.FORCE_INERTIAL:
            force = list(dudt)
        elif kind == O.FORCE_ADDEDMASS:           # :347-393
            cm = 0.5
            force = [dudt[c] * cm if c < dim else 0. for c in range(3)]
            mass += fluid_rho * volume * cm
        elif kind == O.FORCE_LIFT:                # :447-489, vorticity_vector :146-168
            cl = 0.5
            if dim == 2:
                vz = (grad[1][0] - grad[0][1]) / size
                force[0] = fluid_rho * cl * rel[1] * vz
                force[1] = -fluid_rho * cl * rel[0] * vz
            else:
                vx = (grad[2][1] - grad[1][2]) / size
                vy = (grad[0][2] - grad[2][0]) / size
                vz = (grad[1][0] - grad[0][1]) / size
                force[0] = fluid_rho * cl * (rel[1] * vz - rel[2] * vy)
                force[1] = fluid_rho * cl * (rel[2] * vx - rel[0] * vz)
                force[2] = fluid_rho * cl * (rel[0] * vy - rel[1] * vx)
        elif kind == O.FORCE_DRAG:                # :549-587
            dia = 2. * math.pow(3.0 * volume / 4.0 / math.pi, 1. / 3.)
            if dim == 3:
                norm = math.sqrt(rel[0] * rel[0] + rel[1] * rel[1] + rel[2] * rel[2])
            else:
                norm = math.sqrt(rel[0] * rel[0] + rel[1] * rel[1])
            if viscosity != 0:
                Re = norm * dia * fluid_rho / viscosity
                cd = drag_coefficient(Re)
                for c in range(dim):
                    force[c] += 3. / (4. * dia) * cd * norm * rel[c] * fluid_rho
        elif kind == O.FORCE_BUOY:                # :651-652
            for c in range(dim):
                force[c] += (mass / volume - fluid_rho) * gravity[c]
        for c in range(dim):                      # compute_forces, :738-752
            pf[c] = force[c] * volume + pf[c]
    for c in range(dim):                          # :828-837
        vel[c] += pf[c] * dt / mass
    return pf, vel, mass


@pytest.mark.parametrize("dim,level", [(2, 5), (3, 4)])
def test_general_fields_against_the_restatement(dim, level):
    n = 1 << level
    npart = 150
    gd = gfship.Domain(dim, level)
    gs = gfship.Simulation(gd)
    gpl = None
    try:
        xyz = H._grids(dim, n)
        D, A = [], []
        for c in range(dim):
            xf = xyz[0] + (0.5 / n if c == 0 else 0.)
            yf = xyz[1] + (0.5 / n if c == 1 else 0.)
            d, a = gd.variable(), gd.variable()
            d.upload(0.01 * (1.5 + yf))
            a.upload(1. / (1.5 + xf))
            D.append(d)
            A.append(a)
        ac = gd.variable()
        for l in range(level + 1):
            g = H._grids(dim, 1 << l)
            ac.upload(1. / (1.5 + g[0]) + 0. * g[1], l)
        mu = gd.variable()
        mu.upload(0.01 * (1.5 + xyz[1]) + 0. * xyz[0])
        gs.set_alpha_cell(ac)
        for c in range(dim):
            gs.set_viscosity_faces(c, D)
        gs.set_viscosity_cell(mu)
        gs.set_alpha(A)
        gravity = (0., -0.5, 0.)
        gs.set_source(1, gravity[1])
        x, y = xyz[0], xyz[1]
        init = [(0.25 - x * x) * y, x * (y * y - 0.25)]
        if dim == 3:
            init.append(0.1 * (0.25 - xyz[2] * xyz[2]) * x)
        for c in range(dim):
            u = np.zeros((n + 2,) * dim)
            H.interior(u)[...] = H.interior(init[c])
            gs.u[c].upload(u)
        pos, ids, vel, mass, vol = _particulate_case(npart, dim, 41)
        pos *= 0.8                     # away from the walls
        vel *= 0.2
        gs.set_time(dtmax=0.02)
        gs.start()
        gpl = gfship.ParticleList(gs, pos, ids)
        gpl.set_particulate(vel, mass, vol)
        gpl.set_forces(ALL_FORCES, gravity)
        gpl.set_force_coefficient(3, "0.4 + 1e-3*Rep")
        prev = [gd.variable() for c in range(dim)]
        for k in range(2):
            gpl.event()
            # Un, Vn, Wn of the GfsForceCoeff objects: the velocity at the event, with the default BC (:100-114)
            for c in range(dim):
                prev[c].upload(gs.u[c].download())
                gd.bc(prev[c])
            gs.step()
        p0, i0 = gpl.download()
        v0, m0, _ = gpl.particulate_state()
        assert len(i0) >= npart - 5 and np.array_equal(i0, ids[np.isin(ids, i0)])
        volume = dict(zip(ids.tolist(), vol.tolist()))
        dt = gs.dt
        fvel = [gd.interpolate(gs.u[c], p0)[0] for c in range(dim)]
        fveln = [gd.interpolate(prev[c], p0)[0] for c in range(dim)]
        u = [gs.u[c].download() for c in range(dim)]
        alpha_arr, mu_arr = ac.download(), mu.download()
        gpl.event()
        i1 = gpl.download()[1]
        v1, m1, f1 = gpl.particulate_state()
        assert np.array_equal(i1, ids[np.isin(ids, i1)])
        where = {int(q): r for r, q in enumerate(i1)}
        wf, wv, wm, rows = [], [], [], []
        rhos, mus = set(), set()
        for q in range(len(i0)):
            if int(i0[q]) not in where:
                continue                # left through a wall during this event
            cell = _locate(dim, level, p0[q])
            at = (cell[2], cell[1], cell[0]) if dim == 3 else (cell[1], cell[0])
            grad = [[_center_gradient(u[c], at, dim - 1 - c2) for c2 in range(dim)] for c in range(dim)]
            ucell = [float(u[c][at]) for c in range(dim)]
            fluid_rho = 1. / float(alpha_arr[at])
            viscosity = float(mu_arr[at])
            rhos.add(fluid_rho)
            mus.add(viscosity)
            f, v, m = _restated_event(dim, ALL_FORCES, gravity, dt, 1. / n,
                                      [float(a[q]) for a in fvel], [float(a[q]) for a in fveln], grad, ucell,
                                      fluid_rho, viscosity, [float(a) for a in v0[q]], float(m0[q]),
                                      volume[int(i0[q])],
                                      lambda rep: 0.4 + 1e-3 * rep)
            wf.append(f)
            wv.append(v)
            wm.append(m)
            rows.append(where[int(i0[q])])
        assert len(rows) >= npart - 10 and len(rhos) > 5 and len(mus) > 5
        wf, wv, wm = np.array(wf), np.array(wv), np.array(wm)
        print(dim, "force", _rel_err(wf, f1[rows]), "vel", _rel_err(wv, v1[rows]), "mass", _rel_err(wm, m1[rows]))
        assert np.array_equal(wm, m1[rows])
        assert np.array_equal(wf, f1[rows])
        assert np.array_equal(wv, v1[rows])
    finally:
        if gpl is not None:
            gpl.destroy()
        H.destroy_device(gd, gs)


# ---------------------------------------------------------------------------------------------
# (3) refusals
# ---------------------------------------------------------------------------------------------

def _small():
    dim, level = 2, 4
    n = 1 << level
    gd = gfship.Domain(dim, level)
    gs = gfship.Simulation(gd)
    xyz = H._grids(dim, n)
    D = []
    for c in range(dim):
        d = gd.variable()
        d.upload(0.01 * (1.5 + xyz[1] + (0.5 / n if c == 1 else 0.)))
        D.append(d)
    mu = gd.variable()
    mu.upload(0.01 * (1.5 + xyz[1]) + 0. * xyz[0])
    return gd, gs, D, mu, xyz


def _list(gs, forces=True):
    pl = gfship.ParticleList(gs, np.array([[0.1, 0.2, 0.], [-0.2, 0.1, 0.]]), np.array([1, 2]))
    if forces:
        pl.set_particulate(np.zeros((2, 3)), np.ones(2), np.ones(2))
    return pl


def test_viscosity_fields_need_the_viscosity_at_the_cells():
    gd, gs, D, mu, xyz = _small()
    pl = _list(gs)
    try:
        gs.set_viscosity_faces(0, D)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*gfship_sim_set_viscosity_cell"):
            pl.set_forces([gfship.FORCE_DRAG])
        gs.set_viscosity_faces(0, None)
        pl.set_forces([gfship.FORCE_DRAG])
        gs.set_viscosity_faces(0, D)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*gfship_sim_set_viscosity_cell"):
            pl.event()
        gs.set_viscosity_cell(mu)
        pl.set_forces([gfship.FORCE_DRAG, gfship.FORCE_LIFT])
        pl.event()
        gs.set_viscosity_cell(None)
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            pl.event()
        gs.set_viscosity(0, 0.01)
        pl.set_forces([gfship.FORCE_DRAG])
        pl.event()
        assert pl.count() == 2
    finally:
        pl.destroy()
        H.destroy_device(gd, gs)


def test_alpha_needs_alpha_at_the_cells():
    gd, gs, D, mu, xyz = _small()
    pl = _list(gs)
    try:
        A = []
        for c in range(2):
            a = gd.variable()
            a.upload(1. / (1.5 + xyz[0] + (0.5 / 16 if c == 0 else 0.)))
            A.append(a)
        gs.set_alpha(A)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*gfship_sim_set_alpha_cell"):
            pl.set_forces([gfship.FORCE_BUOY], (0., -1., 0.))
        gs.set_alpha(None)
        pl.set_forces([gfship.FORCE_BUOY], (0., -1., 0.))
        gs.set_alpha(A)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*gfship_sim_set_alpha_cell"):
            pl.event()
        ac = gd.variable()
        for l in range(5):
            g = H._grids(2, 1 << l)
            ac.upload(1. / (1.5 + g[0]) + 0. * g[1], l)
        gs.set_alpha_cell(ac)
        pl.set_forces([gfship.FORCE_BUOY], (0., -1., 0.))
        pl.event()
        assert pl.count() == 2
    finally:
        pl.destroy()
        H.destroy_device(gd, gs)


def test_tracers_run_with_any_of_the_fields():
    gd, gs, D, mu, xyz = _small()
    pl = _list(gs, forces=False)
    try:
        gs.set_viscosity_faces(0, D)
        pl.event()
        A = []
        for c in range(2):
            a = gd.variable()
            a.upload(1. / (1.5 + xyz[0] + (0.5 / 16 if c == 0 else 0.)))
            A.append(a)
        gs.set_viscosity_faces(0, None)
        gs.set_alpha(A)
        pl.event()
        gs.set_viscosity_cell(mu)
        pl.event()
        assert pl.count() == 2
    finally:
        pl.destroy()
        H.destroy_device(gd, gs)
