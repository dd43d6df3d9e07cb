"""The forces on a GfsParticulate and its event, restated from the reference on the explicit cell graph
of tests/sampler_reference.py.

Plain Python floats in the reference's operand order, the reference's file:line at every step.  Written
from modules/particulatecommon.c and src/fluid.c of the reference, not from oracle/go_particles.c,
csrc/particles.hip or the restated event of tests/test_gpu_particulates_fluid_fields.py.  There is no
index arithmetic here: the cell of a particle comes from Box.locate, its neighbours from Box.neighbor,
values from Box.value, the fluid velocity from Box.interpolate.  Every compute_*_force does its own locate
and its own interpolate, as the reference does; the device evaluates them once per particle and shares
them, and that sharing is what the comparison tests.

Named choices, where the reference's text has no defined value:
  RELATIVE_VEL_Z_2D   the z component of a relative velocity in 2-D;
  ONFLUID_FORCE_Z_2D  the z component of the force of compute_forces_onfluid in 2-D.

Test infrastructure only.
"""
import math

import sampler_reference as R

INERTIAL, ADDEDMASS, LIFT, DRAG, BUOY = 1, 2, 3, 4, 5      # the FORCE_* numbers of the library and the oracle


def relative_vel_z_2d(vel_z):
    """In 2-D subs_fttvectors (modules/particulatecommon.c:115-122) writes FTT_DIMENSION components of
    its result, and fluid_vel.z is never written either (:361-365, :447-451): relative_vel.z, which
    enters the norm of the added-mass and lift Reynolds number (:367-369, :457-459), is an uninitialised
    read.  The library and the oracle take the difference with a zero fluid velocity; so does this."""
    return 0. - vel_z


ONFLUID_FORCE_Z_2D = 0.
"""compute_forces_onfluid (:753-765) has no `#if FTT_2D' zeroing: total_force.z is never written in 2-D
and is assigned to p->force.  The library stores the zero source_particulate_event wrote just before
(:2201-2202); so does this."""


def pow_root(x):
    """the reference's text, :580-582"""
    return math.pow(x, 0.5)


sqrt_root = math.sqrt       # the device's


class ForceCoeff:
    """GfsForceCoeff (:166-252): a force of `kind' with an optional GfsFunction `coefficient' (Rep, Urelp,
    Vrelp, Wrelp, Pdia) -> float; GfsForceBuoy is a plain GfsParticleForce and never has one"""
    __slots__ = ("kind", "coefficient")

    def __init__(self, kind, coefficient=None):
        assert kind in (INERTIAL, ADDEDMASS, LIFT, DRAG, BUOY)
        assert coefficient is None or kind in (ADDEDMASS, LIFT, DRAG)
        self.kind, self.coefficient = kind, coefficient


class Particulate(R.Particle):
    """GfsParticulate, modules/particulatecommon.h"""
    __slots__ = ("vel", "mass", "volume", "force")

    def __init__(self, pos, pid, vel, mass, volume):
        R.Particle.__init__(self, pos, pid)
        self.vel = [float(x) for x in vel]
        self.mass, self.volume = float(mass), float(volume)
        self.force = [0., 0., 0.]


class Sim:
    """What the forces read of a GfsSimulation.

    u           the velocity components as Box.field () lists (with ghosts);
    un          Un, Vn, Wn of the GfsForceCoeff objects (:179-185), None until a GfsForceCoeff is read;
    dt          sim->advection_params.dt;
    alpha       None (physical_params.alpha == NULL) or cell -> float;
    viscosity   per velocity component: None (no GfsSourceDiffusion on it) or cell -> float
                (gfs_diffusion_cell (d->D, cell)); the forces look at component 0 only (:278, :358, :444, :540);
    g           per component: the sum of the intensities of the GfsSource objects of it (:635-649);
    root        pow_root or sqrt_root: the square root of the default drag law.
    """

    def __init__(self, box, sides, u, dt, alpha=None, viscosity=(None, None, None), g=(0., 0., 0.),
                 root=pow_root):
        self.box, self.sides, self.dim = box, sides, box.dim
        self.set_velocity(u)
        self.un = None
        self.dt = float(dt)
        self.alpha, self.viscosity, self.g, self.root = alpha, tuple(viscosity), [float(x) for x in g], root

    def set_velocity(self, u):
        self.u = [self.box.field(a) for a in u]

    def fluid_rho(self, cell):
        """sim->physical_params.alpha ? 1./gfs_function_value (alpha, cell) : 1., :273-274 and the like"""
        return 1./self.alpha(cell) if self.alpha is not None else 1.

    def viscosity_of_u(self, cell):
        """viscosity = 0.; d = source_diffusion_viscosity (u[0]); if (d) viscosity = gfs_diffusion_cell (d->D,
        cell), :277-279 and the like"""
        viscosity = 0.
        if self.viscosity[0] is not None:
            viscosity = self.viscosity[0](cell)
        return viscosity


# -------------------------------------------------------------------------------------------------
# src/fluid.c
# -------------------------------------------------------------------------------------------------

def center_gradient(box, cell, c, v, census=None):
    """gfs_center_gradient, src/fluid.c:434-475, on cells of one level: gfs_neighbor_value (:365-378) of a
    leaf neighbour of the same level is its value and leaves x at 1.  census: a dict that counts the branch
    taken ("two", "one", "none" neighbours); box.gradient_census, where a caller has set one, otherwise."""
    if census is None:
        census = getattr(box, "gradient_census", None)
    d = 2*c                                                # :438
    n1 = box.neighbor(cell, R.opposite(d))                 # f1 = gfs_cell_face (cell, opposite), :445
    v0 = box.value(cell, v)                                # :446
    if n1 is not None:                                     # :447
        n2 = box.neighbor(cell, d)                         # :448
        x1 = 1.
        v1 = box.value(n1, v)                              # :451
        if n2 is not None:                                 # :452
            x2 = 1.
            v2 = box.value(n2, v)                          # :456
            if census is not None:
                census["two"] += 1
            return (x1*x1*(v2 - v0) + x2*x2*(v0 - v1))/(x1*x2*(x2 + x1))      # :457
        if census is not None:
            census["one"] += 1
        return (v0 - v1)/x1                                # :461
    n2 = box.neighbor(cell, d)                             # :464
    if n2 is not None:                                     # :466
        x2 = 1.
        if census is not None:
            census["one"] += 1
        return (box.value(n2, v) - v0)/x2                  # :470
    if census is not None:
        census["none"] += 1
    return 0.                                              # :474


# -------------------------------------------------------------------------------------------------
# modules/particulatecommon.c
# -------------------------------------------------------------------------------------------------

def vorticity_vector(box, cell, u):
    """vorticity_vector, :142-164"""
    size = box.cell_size(cell)                             # :150
    if box.dim == 2:
        return [0., 0.,                                    # :152-153
                (center_gradient(box, cell, 0, u[1]) - center_gradient(box, cell, 1, u[0]))/size]      # :154-155
    return [(center_gradient(box, cell, 1, u[2]) - center_gradient(box, cell, 2, u[1]))/size,          # :157-158
            (center_gradient(box, cell, 2, u[0]) - center_gradient(box, cell, 0, u[2]))/size,          # :159-160
            (center_gradient(box, cell, 0, u[1]) - center_gradient(box, cell, 1, u[0]))/size]          # :161-162


def _relative_vel(sim, cell, p):
    """fluid_vel (FTT_DIMENSION interpolations) and subs_fttvectors (&fluid_vel, &particulate->vel),
    :361-365, :447-451, :543-547"""
    box = sim.box
    rel = [0., 0., relative_vel_z_2d(p.vel[2])]
    for c in range(box.dim):
        rel[c] = box.interpolate(cell, p.pos, sim.u[c]) - p.vel[c]
    return rel


def _diameter(p):
    return 2.*math.pow(3.0*p.volume/4.0/math.pi, 1./3.)     # :370, :460, :549


def compute_inertial_force(sim, p, coeff):
    """:255-303"""
    box, dim = sim.box, sim.dim
    force = [0., 0., 0.]                                   # :263-266
    cell = box.locate(p.pos)                               # :268
    if cell is None:
        return force                                       # :269
    size = box.cell_size(cell)                             # :271
    fluid_rho = sim.fluid_rho(cell)                        # :273-274
    u = sim.u
    fluid_vel = [box.interpolate(cell, p.pos, u[c]) for c in range(dim)]          # :281-283
    fluid_veln = [box.interpolate(cell, p.pos, sim.un[c]) for c in range(dim)]    # :285-287
    if sim.dt > 0.:                                        # :290
        for c in range(dim):
            force[c] = fluid_rho*(fluid_vel[c] - fluid_veln[c])/sim.dt            # :292
    else:
        return force                                       # :294
    for c in range(dim):                                   # :297-300
        for c2 in range(dim):
            force[c] += fluid_rho*center_gradient(box, cell, c2, u[c])*box.value(cell, u[c2])/size
    return force


def _coefficient_of_rep(sim, p, coeff, cell, fluid_rho, inputs):
    """the coefficient of the added-mass and lift forces, :353-386 and :456-475"""
    viscosity = sim.viscosity_of_u(cell)                   # :357-359, :443-445
    relative_vel = _relative_vel(sim, cell, p)             # :361-365, :447-451
    norm_relative_vel = math.sqrt(relative_vel[0]*relative_vel[0] +
                                  relative_vel[1]*relative_vel[1] +
                                  relative_vel[2]*relative_vel[2])                # :367-369, :457-459
    dia = _diameter(p)                                     # :370, :460
    if viscosity == 0:                                     # :372-375, :461-464
        viscosity = 0.001
    Re = norm_relative_vel*dia*fluid_rho/viscosity         # :376, :465
    args = (Re, relative_vel[0], relative_vel[1], relative_vel[2], dia)           # :378-384, :467-473
    if inputs is not None:
        inputs.append((coeff.kind,) + args)
    return coeff.coefficient(*args)                        # :385, :474


def compute_addedmass_force(sim, p, coeff, inputs=None):
    """:331-394; adds to p.mass"""
    box, dim = sim.box, sim.dim
    force = [0., 0., 0.]                                   # :339-342
    cell = box.locate(p.pos)                               # :344
    if cell is None:
        return force                                       # :345
    force = compute_inertial_force(sim, p, coeff)          # :347
    fluid_rho = sim.fluid_rho(cell)                        # :349-350
    cm = 0.5                                               # :352
    if coeff.coefficient is not None:                      # :353
        cm = _coefficient_of_rep(sim, p, coeff, cell, fluid_rho, inputs)
    for c in range(dim):
        force[c] *= cm                                     # :388-389
    p.mass += fluid_rho*p.volume*cm                        # :391
    return force


def compute_lift_force(sim, p, coeff, inputs=None):
    """:423-490"""
    box, dim = sim.box, sim.dim
    force = [0., 0., 0.]                                   # :431-434
    cell = box.locate(p.pos)                               # :436
    if cell is None:
        return force                                       # :437
    fluid_rho = sim.fluid_rho(cell)                        # :439-440
    relative_vel = _relative_vel(sim, cell, p)             # :447-451
    vorticity = vorticity_vector(box, cell, sim.u)         # :452-453
    cl = 0.5                                               # :455
    if coeff.coefficient is not None:                      # :456
        cl = _coefficient_of_rep(sim, p, coeff, cell, fluid_rho, inputs)
    if dim == 2:
        force[0] = fluid_rho*cl*relative_vel[1]*vorticity[2]                      # :478
        force[1] = -fluid_rho*cl*relative_vel[0]*vorticity[2]                     # :479
    else:
        force[0] = fluid_rho*cl*(relative_vel[1]*vorticity[2] - relative_vel[2]*vorticity[1])      # :481-482
        force[1] = fluid_rho*cl*(relative_vel[2]*vorticity[0] - relative_vel[0]*vorticity[2])      # :483-484
        force[2] = fluid_rho*cl*(relative_vel[0]*vorticity[1] - relative_vel[1]*vorticity[0])      # :485-486
    return force


DRAG_BRANCHES = ("no-viscosity", "coefficient", "below-1e-8", "below-50", "from-50")


def compute_drag_force(sim, p, coeff, inputs=None, branch=None):
    """:519-588.  branch: a list that receives the name of the branch taken (DRAG_BRANCHES) and Re"""
    box, dim = sim.box, sim.dim
    force = [0., 0., 0.]                                   # :526-529
    cell = box.locate(p.pos)                               # :531
    if cell is None:
        return force                                       # :532
    fluid_rho = sim.fluid_rho(cell)                        # :534-535
    viscosity = sim.viscosity_of_u(cell)                   # :538-541
    relative_vel = _relative_vel(sim, cell, p)             # :543-547
    dia = _diameter(p)                                     # :549
    if dim == 3:
        norm_relative_vel = math.sqrt(relative_vel[0]*relative_vel[0] +
                                      relative_vel[1]*relative_vel[1] +
                                      relative_vel[2]*relative_vel[2])            # :551-553
    else:
        norm_relative_vel = math.sqrt(relative_vel[0]*relative_vel[0] +
                                      relative_vel[1]*relative_vel[1])            # :555-556
    cd = 0.                                                # :559
    if viscosity == 0:                                     # :561-562: before any coefficient is called
        if branch is not None:
            branch.append(("no-viscosity", None))
        return force
    Re = norm_relative_vel*dia*fluid_rho/viscosity         # :564
    if coeff.coefficient is not None:                      # :566-575
        args = (Re, relative_vel[0], relative_vel[1], relative_vel[2], dia)
        if inputs is not None:
            inputs.append((coeff.kind,) + args)
        cd = coeff.coefficient(*args)
        name = "coefficient"
    elif Re < 1e-8:                                        # :577-578
        if branch is not None:
            branch.append(("below-1e-8", Re))
        return force
    elif Re < 50.0:                                        # :579-580
        cd = 16.*(1. + 0.15*sim.root(Re))/Re
        name = "below-50"
    else:                                                  # :581-582
        cd = 48.*(1. - 2.21/sim.root(Re))/Re
        name = "from-50"
    if branch is not None:
        branch.append((name, Re))
    for c in range(dim):                                   # :584-585
        force[c] += 3./(4.*dia)*cd*norm_relative_vel*relative_vel[c]*fluid_rho
    return force


def default_cd(Re, root):
    """cd of the default law, :577-582, for Re >= 1e-8"""
    if Re < 50.0:
        return 16.*(1. + 0.15*root(Re))/Re
    return 48.*(1. - 2.21/root(Re))/Re


def compute_buoyancy_force(sim, p, coeff):
    """:617-655"""
    force = [0., 0., 0.]                                   # :623-626
    cell = sim.box.locate(p.pos)                           # :628
    if cell is None:
        return force                                       # :629
    fluid_rho = sim.fluid_rho(cell)                        # :631-632
    g = sim.g                                              # :635-649
    for c in range(sim.dim):
        force[c] += (p.mass/p.volume - fluid_rho)*g[c]     # :651-652
    return force


def _force_of(sim, p, coeff, inputs=None, branch=None):
    """(event->force) (GFS_PARTICLE (p), event), :740, :757"""
    if coeff.kind == INERTIAL:
        return compute_inertial_force(sim, p, coeff)
    if coeff.kind == ADDEDMASS:
        return compute_addedmass_force(sim, p, coeff, inputs)
    if coeff.kind == LIFT:
        return compute_lift_force(sim, p, coeff, inputs)
    if coeff.kind == DRAG:
        return compute_drag_force(sim, p, coeff, inputs, branch)
    return compute_buoyancy_force(sim, p, coeff)


def compute_forces(sim, coeff, p, inputs=None, branch=None, parts=None):
    """:737-751.  parts: a list that receives (kind, new_force*volume)"""
    new_force = _force_of(sim, p, coeff, inputs, branch)   # :740
    total_force = [0., 0., 0.]
    for c in range(sim.dim):
        total_force[c] = new_force[c]*p.volume + p.force[c]                       # :743-744
    if sim.dim == 2:
        total_force[2] = 0.                                # :746-748
    if parts is not None:
        parts.append((coeff.kind, [new_force[c]*p.volume for c in range(sim.dim)]))
    p.force = total_force                                  # :750


def compute_forces_onfluid(sim, coeff, p, inputs=None):
    """:753-765.  What compute_addedmass_force adds to the mass (:391) is added here as in an event, and
    nothing takes it off again: by the reference's text the mass of a particle grows with every
    evaluation of a GfsSourceParticulate that holds its list."""
    if coeff.kind != BUOY:                                 # :756
        new_force = _force_of(sim, p, coeff, inputs)       # :757
        total_force = [0., 0., ONFLUID_FORCE_Z_2D]
        for c in range(sim.dim):
            total_force[c] = new_force[c]*p.volume + p.force[c]                   # :760-761
        p.force = total_force                              # :763


def forces_on_fluid(sim, plist, forces, inputs=None):
    """the first loop of source_particulate_event, :2199-2206: the list itself is untouched (a particle
    outside the box gets the zero force every compute_*_force returns there and stays on the list)"""
    for p in plist:
        p.force = [0., 0., 0.]                             # :2201-2202
        for coeff in forces:                               # :2203-2204
            compute_forces_onfluid(sim, coeff, p, inputs)


def particulate_event(sim, p, forces, inputs=None, branch=None, parts=None):
    """gfs_particulate_event, :768-842"""
    if not forces:                                         # :776-778: the event of GfsParticle,
        p.pos_old = list(p.pos)                            # src/particle.c:31-44
        p.pos = sim.box.advect_point(sim.u, p.pos, sim.dt)
        return
    pos = list(p.pos)                                      # :804
    p.pos_old = list(pos)                                  # :805
    p.force = [0., 0., 0.]                                 # :815-816, three components
    for coeff in forces:                                   # :818-819
        compute_forces(sim, coeff, p, inputs, branch, parts)
    # :821-826: vliq, the norm of the fluid velocity at the particle, is computed and never read
    for c in range(sim.dim):                               # :828-837
        pos[c] += p.vel[c]*sim.dt/2.                       # :831-832
        p.vel[c] += p.force[c]*sim.dt/p.mass               # :833-834
        pos[c] += p.vel[c]*sim.dt/2.                       # :835-836
    p.pos = pos                                            # :839


def _set_value(cell, v, x):
    i, j, k = cell.ijk
    if len(v) and isinstance(v[0][0], list):
        v[k][j][i] = x
    else:
        v[j][i] = x


def store_previous_vel(box, u, sides):
    """store_domain_previous_vel, :99-113: per component the copy on the leaves (:108-110), then
    gfs_domain_bc of the NEW variable (:111), a scalar with the default condition on every side: on a
    GfsBoundaryPeriodic side the ghost takes the value of the matching cell across the box, on a GfsBoundary
    side `symmetry' of a variable that is no vector component, src/boundary.c:45-57 (:50: the value of the
    neighbour; the default GfsBc of a boundary, :805).  Ghosts that belong to no boundary cell: NaN."""
    un = []
    nan = float("nan")
    for c in range(box.dim):
        v = u[c]
        w = [[nan]*len(row) for row in v] if box.dim == 2 else [[[nan]*len(row) for row in pl] for pl in v]
        for cell in box.leaves:
            _set_value(cell, w, box.value(cell, v))        # copy_cell_gfsvariable, :91-97
        for g in box.ghosts:
            d = g.tree                                     # the side of the box this boundary sits on
            nb = box.neighbor(g, R.opposite(d))            # f->neighbor: boundary->d = opposite (d), src/boundary.c:853
            assert nb is not None and not nb.boundary
            if sides[d] == R.SIDE_PERIODIC:
                # the matching cell: the leaf on the other side of the box, same row
                while True:
                    nx = box.neighbor(nb, R.opposite(d))
                    if nx is None or nx.boundary:
                        break
                    nb = nx
                _set_value(g, w, box.value(nb, w))
            elif sides[d] == R.SIDE_BOUNDARY:
                _set_value(g, w, box.value(nb, w))         # src/boundary.c:50
            else:
                raise NotImplementedError("Un across a GfsBoundaryMpi side needs an exchange")
        un.append(w)
    return un


def read_forces(sim, forces):
    """gfs_force_coeff_read, :168-209: every GfsForceCoeff that is read gets Un, Vn(, Wn) and stores the
    velocity of that moment (:179-185).  GfsForceBuoy is no GfsForceCoeff."""
    for coeff in forces:
        if coeff.kind != BUOY:
            sim.un = store_previous_vel(sim.box, sim.u, sim.sides)


def list_event(sim, plist, forces, inputs=None, branch=None, parts=None):
    """gfs_particle_list_event, :980-1015.  Returns the new list."""
    box = sim.box
    plist = box.remove_particles_not_in_domain(plist)      # :987
    for p in plist:                                        # :989-990: the event of every particle
        particulate_event(sim, p, forces, inputs, branch, parts)
    plist, _sent = box.particle_bc(plist, sim.sides)       # :993
    for coeff in forces:                                   # :1004-1012
        if coeff.kind == INERTIAL:                         # :1007
            sim.un = store_previous_vel(box, sim.u, sim.sides)                    # :1009
    return plist
