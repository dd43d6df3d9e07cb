"""The forces on a GfsParticulate and its event on a REFINED box: forces_reference on the cell trees of
tree_sampler_reference.TreeBox.

Plain Python floats in the reference's operand order, the reference's file:line at every step.  Written from
src/fluid.c and modules/particulatecommon.c of the reference, not from csrc/tree.hpp, csrc/tree_particles.hip or
oracle/.  There is no index arithmetic: the cell of a particle comes from TreeBox.locate, its neighbours from
TreeBox.neighbor, the children of a cell from the cell itself, values from TreeBox.value, the fluid velocity from
TreeBox.interpolate.

What changes with respect to a box of one level is gfs_center_gradient: next to a change of level
gfs_neighbor_value (src/fluid.c:364-396) interpolates in a coarser neighbour (x = 3/2) or takes the mean of the
children of a refined one (x = 3/4).  Everything that reaches it is restated here: the inertial force,
vorticity_vector, the lift and added-mass forces, and the dispatch of compute_forces / gfs_particulate_event /
gfs_particle_list_event, which in forces_reference is bound to the gradient of the uniform box
(forces_reference._force_of).  What does not depend on the gradient is imported: the drag and buoyancy forces,
the coefficient inputs, ForceCoeff, Particulate, Sim.  forces_reference is neither edited nor patched.

Test infrastructure only.
"""
import collections

import sampler_reference as R
import forces_reference as F
from forces_reference import (INERTIAL, ADDEDMASS, LIFT, DRAG, BUOY, ForceCoeff, Particulate, Sim,      # noqa: F401
                              compute_drag_force, compute_buoyancy_force, sqrt_root, pow_root, DRAG_BRANCHES)

# index[d][i] of ftt_cell_children_direction, src/ftt.h:329-341
CHILDREN_DIRECTION = {2: ((1, 3), (0, 2), (0, 1), (2, 3)),
                      3: ((1, 3, 5, 7), (0, 2, 4, 6), (0, 1, 4, 5), (2, 3, 6, 7), (0, 1, 2, 3), (4, 5, 6, 7))}
# perpendicular[d][FTT_CELL_ID], src/fluid.c:265-277
PERPENDICULAR_2D = ((-1, 2, -1, 3),
                    (2, -1, 3, -1),
                    (1, 0, -1, -1),
                    (-1, -1, 1, 0))
PERPENDICULAR_3D = (((-1, -1), (2, 4), (-1, -1), (3, 4), (-1, -1), (2, 5), (-1, -1), (3, 5)),
                    ((2, 4), (-1, -1), (3, 4), (-1, -1), (2, 5), (-1, -1), (3, 5), (-1, -1)),
                    ((4, 1), (4, 0), (-1, -1), (-1, -1), (5, 1), (5, 0), (-1, -1), (-1, -1)),
                    ((-1, -1), (-1, -1), (4, 1), (4, 0), (-1, -1), (-1, -1), (5, 1), (5, 0)),
                    ((1, 2), (0, 2), (1, 3), (0, 3), (-1, -1), (-1, -1), (-1, -1), (-1, -1)),
                    ((-1, -1), (-1, -1), (-1, -1), (-1, -1), (1, 2), (0, 2), (1, 3), (0, 3)))

# the branches of a gfs_neighbor_value, and of every face the interpolation in a coarse neighbour looks through
SAME_LEAF, CHILDREN, COARSER = "same-level-leaf", "children", "coarser"
TRANSVERSE_LEAF, TRANSVERSE_CHILDREN, TRANSVERSE_ABSENT = "transverse-leaf", "transverse-children", "transverse-absent"


def new_census():
    return collections.Counter()


def _count(census, key):
    if census is not None:
        census[key] += 1


# -------------------------------------------------------------------------------------------------
# src/fluid.c
# -------------------------------------------------------------------------------------------------

def average_neighbor_value(box, cell, neighbor, d, v, census=None, transverse=False):
    """average_neighbor_value, src/fluid.c:64-93, of the face (cell, neighbor, d): (value, x); x = None where
    the reference leaves *x as it was.  No solid fractions (w = 1., :82), no GFS_NODATA."""
    assert neighbor.level == cell.level                    # :69
    if neighbor.children is None:                          # :71
        _count(census, TRANSVERSE_LEAF if transverse else SAME_LEAF)
        return box.value(neighbor, v), None                # :72
    av = a = 0.                                            # :75
    od = R.opposite(d)                                     # :76
    for i in CHILDREN_DIRECTION[box.dim][od]:              # :79-80, ftt_cell_children_direction, src/ftt.h:351-353
        ch = neighbor.children[i]
        if not ch.destroyed:                               # :81
            w = 1.                                         # :82
            a += w                                         # :83
            av += w*box.value(ch, v)                       # :84
    if a > 0.:                                             # :86
        _count(census, TRANSVERSE_CHILDREN if transverse else CHILDREN)
        return av/a, 3./4.                                 # :87-88
    _count(census, "children-all-destroyed")
    return box.value(cell, v), None                        # :91


def interpolate_1D1(box, cell, d, x, v, census=None):
    """interpolate_1D1, src/fluid.c:171-191 (FTT_2D): (a, b) of v = a*v(cell) + b"""
    pa, pb = 1., 0.                                        # :176
    neighbor = box.neighbor(cell, d)                       # :179
    if neighbor is not None:                               # :180
        x2 = 1.                                            # :181
        p2, nx = average_neighbor_value(box, cell, neighbor, d, v, census, True)     # :182
        if nx is not None:
            x2 = nx
        a2 = x/x2                                          # :184
        pb += a2*p2                                        # :185
        pa -= a2                                           # :186
    else:
        _count(census, TRANSVERSE_ABSENT)
    return pa, pb


def interpolate_2D1(box, cell, d1, d2, x, y, v, census=None):
    """interpolate_2D1, src/fluid.c:214-245 (FTT_3D)"""
    pa, pb = 1., 0.                                        # :219
    n1 = box.neighbor(cell, d1)                            # :222
    if n1 is not None:                                     # :223
        y1 = 1.                                            # :224
        p1, nx = average_neighbor_value(box, cell, n1, d1, v, census, True)          # :225
        if nx is not None:
            y1 = nx
        a1 = y/y1                                          # :227
        pb += a1*p1                                        # :228
        pa -= a1                                           # :229
    else:
        _count(census, TRANSVERSE_ABSENT)
    n2 = box.neighbor(cell, d2)                            # :233
    if n2 is not None:                                     # :234
        x2 = 1.                                            # :235
        p2, nx = average_neighbor_value(box, cell, n2, d2, v, census, True)          # :236
        if nx is not None:
            x2 = nx
        a2 = x/x2                                          # :238
        pb += a2*p2                                        # :239
        pa -= a2                                           # :240
    else:
        _count(census, TRANSVERSE_ABSENT)
    return pa, pb


def neighbor_value(box, cell, neighbor, d, v, census=None):
    """gfs_neighbor_value, src/fluid.c:364-396, of the face (cell, neighbor, d): (value, x or None, branch)"""
    if neighbor.level == cell.level:                       # :378
        val, x = average_neighbor_value(box, cell, neighbor, d, v, census)           # :380
        return val, x, (SAME_LEAF if neighbor.children is None else CHILDREN)
    assert neighbor.level == cell.level - 1                # neighbor at coarser level, :384
    _count(census, COARSER)
    if box.dim == 2:
        dp = PERPENDICULAR_2D[d][cell.id]                  # :385
        assert dp >= 0                                     # :387
        vca, vcb = interpolate_1D1(box, neighbor, dp, 1./4., v, census)              # :388
    else:
        dp = PERPENDICULAR_3D[d][cell.id]                  # :385
        assert dp[0] >= 0 and dp[1] >= 0                   # :390
        vca, vcb = interpolate_2D1(box, neighbor, dp[0], dp[1], 1./4., 1./4., v, census)      # :391
    return vca*box.value(neighbor, v) + vcb, 3./2., COARSER                          # :393-394


def center_gradient(box, cell, c, v, census=None):
    """gfs_center_gradient, src/fluid.c:434-475.  census: a Counter of the branches taken (box.gradient_census,
    where a caller has set one, otherwise): "two" / "one" / "none" neighbours, the branch of every
    gfs_neighbor_value, ("pair", branch of f1, branch of f2) of a gradient with two neighbours, and the state of
    every transverse neighbour an interpolation in a coarse cell looked at."""
    if census is None:
        census = getattr(box, "gradient_census", None)
    d = 2*c                                                # :438
    n1 = box.neighbor(cell, R.opposite(d))                 # f1, :445
    v0 = box.value(cell, v)                                # :446
    if n1 is not None:                                     # :447
        n2 = box.neighbor(cell, d)                         # f2, :448
        x1 = 1.                                            # :449
        v1, nx, b1 = neighbor_value(box, cell, n1, R.opposite(d), v, census)         # :451
        if nx is not None:
            x1 = nx
        if n2 is not None:                                 # :452
            x2 = 1.                                        # :454
            v2, nx, b2 = neighbor_value(box, cell, n2, d, v, census)                 # :456
            if nx is not None:
                x2 = nx
            _count(census, "two")
            _count(census, ("pair", b1, b2))
            return (x1*x1*(v2 - v0) + x2*x2*(v0 - v1))/(x1*x2*(x2 + x1))             # :457
        _count(census, "one")
        return (v0 - v1)/x1                                # :461
    n2 = box.neighbor(cell, d)                             # :464
    if n2 is not None:                                     # :466
        x2 = 1.                                            # :467
        v2, nx, _b = neighbor_value(box, cell, n2, d, v, census)
        if nx is not None:
            x2 = nx
        _count(census, "one")
        return (v2 - v0)/x2                                # :470
    _count(census, "none")
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
        cm = F._coefficient_of_rep(sim, p, coeff, cell, fluid_rho, inputs)
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
    relative_vel = F._relative_vel(sim, cell, p)           # :447-451
    vorticity = vorticity_vector(box, cell, sim.u)         # :452-453
    cl = 0.5                                               # :455
    if coeff.coefficient is not None:                      # :456
        cl = F._coefficient_of_rep(sim, p, coeff, cell, fluid_rho, inputs)
    if dim == 2:
        force[0] = fluid_rho*cl*relative_vel[1]*vorticity[2]                      # :478
        force[1] = -fluid_rho*cl*relative_vel[0]*vorticity[2]                     # :479
    else:
        force[0] = fluid_rho*cl*(relative_vel[1]*vorticity[2] - relative_vel[2]*vorticity[1])      # :481-482
        force[1] = fluid_rho*cl*(relative_vel[2]*vorticity[0] - relative_vel[0]*vorticity[2])      # :483-484
        force[2] = fluid_rho*cl*(relative_vel[0]*vorticity[1] - relative_vel[1]*vorticity[0])      # :485-486
    return force


def _force_of(sim, p, coeff, inputs=None, branch=None):
    """(event->force) (GFS_PARTICLE (p), event), :740"""
    if coeff.kind == INERTIAL:
        return compute_inertial_force(sim, p, coeff)
    if coeff.kind == ADDEDMASS:
        return compute_addedmass_force(sim, p, coeff, inputs)
    if coeff.kind == LIFT:
        return compute_lift_force(sim, p, coeff, inputs)
    if coeff.kind == DRAG:
        return compute_drag_force(sim, p, coeff, inputs, branch)
    return compute_buoyancy_force(sim, p, coeff)


def compute_forces(sim, coeff, p, inputs=None, branch=None):
    """:737-751"""
    new_force = _force_of(sim, p, coeff, inputs, branch)   # :740
    total_force = [0., 0., 0.]
    for c in range(sim.dim):
        total_force[c] = new_force[c]*p.volume + p.force[c]                       # :743-744
    if sim.dim == 2:
        total_force[2] = 0.                                # :746-748
    p.force = total_force                                  # :750


def particulate_event(sim, p, forces, inputs=None, branch=None):
    """gfs_particulate_event, :768-842"""
    if not forces:                                         # :776-778: the event of GfsParticle,
        p.pos_old = list(p.pos)                            # src/particle.c:31-44
        p.pos = sim.box.advect_point(sim.u, p.pos, sim.dt)
        return
    pos = list(p.pos)                                      # :804
    p.pos_old = list(pos)                                  # :805
    p.force = [0., 0., 0.]                                 # :815-816
    for coeff in forces:                                   # :818-819
        compute_forces(sim, coeff, p, inputs, branch)
    for c in range(sim.dim):                               # :828-837
        pos[c] += p.vel[c]*sim.dt/2.                       # :831-832
        p.vel[c] += p.force[c]*sim.dt/p.mass               # :833-834
        pos[c] += p.vel[c]*sim.dt/2.                       # :835-836
    p.pos = pos                                            # :839


def _set_value(box, cell, v, x):
    i, j, k = cell.ijk
    a = v[cell.level]
    if box.dim == 2:
        a[j][i] = x
    else:
        a[k][j][i] = x


def store_previous_vel(box, u, sides):
    """store_domain_previous_vel, :99-113, on a tree: per component the copy on the leaves of every level
    (FTT_TRAVERSE_LEAFS, -1, :108-110), then gfs_domain_bc (FTT_TRAVERSE_LEAFS, -1) of the NEW variable (:111), a
    scalar with the default condition on every side whatever the conditions of U: on a GfsBoundaryPeriodic side
    the ghost leaf takes the value of the matching cell across the box, on a GfsBoundary side `symmetry' of a
    variable that is no vector component, src/boundary.c:45-57 (:50: the value of the neighbour; the default GfsBc
    of a boundary, :805).  Cells that are neither leaves nor ghost leaves: NaN."""
    nan = float("nan")

    def blank(a):
        return [blank(x) for x in a] if isinstance(a, list) else nan
    un = []
    for c in range(box.dim):
        v = u[c]
        w = [blank(a) for a in v]
        for cell in box.leaves:
            _set_value(box, cell, w, box.value(cell, v))   # copy_cell_gfsvariable, :91-97
        for g in box.ghosts:
            d = g.tree                                     # the side of the box this boundary sits on
            nb = box.neighbor(g, R.opposite(d))            # boundary->d = opposite (d), src/boundary.c:853
            assert nb is not None and not nb.boundary and nb.level == g.level and nb.children is None
            if sides[d] == R.SIDE_PERIODIC:
                # the matching cell: the cell of the level of the ghost on the other side of the box, same row
                # (the two sides of a periodic pair are refined alike)
                while True:
                    nx = box.neighbor(nb, R.opposite(d))
                    if nx is None or nx.boundary:
                        break
                    assert nx.level == g.level
                    nb = nx
                assert nb.children is None
                _set_value(box, g, w, box.value(nb, w))
            elif sides[d] == R.SIDE_BOUNDARY:
                _set_value(box, g, w, box.value(nb, w))    # src/boundary.c:50
            else:
                raise NotImplementedError("Un across a GfsBoundaryMpi side needs an exchange")
        un.append(w)
    return un


def read_forces(sim, forces):
    """gfs_force_coeff_read, :168-209: every GfsForceCoeff that is read gets Un, Vn(, Wn) and stores the velocity
    of that moment (:179-185).  GfsForceBuoy is no GfsForceCoeff."""
    for coeff in forces:
        if coeff.kind != BUOY:
            sim.un = store_previous_vel(sim.box, sim.u, sim.sides)


def list_event(sim, plist, forces, inputs=None, branch=None):
    """gfs_particle_list_event, :980-1015.  Returns the new list.  In box.record (a Counter, where the caller has
    set one): what TreeBox.list_event records of the tracers -- the changes of level of the leaf that holds a
    particle, the particles a periodic side put back and those taken off the list."""
    box = sim.box
    record = getattr(box, "record", None)
    before = {}
    n0 = len(plist)
    plist = box.remove_particles_not_in_domain(plist)      # :987
    if record is not None:
        record["outside_at_start"] += n0 - len(plist)
        for p in plist:
            before[id(p)] = box.locate(p.pos).level
    for p in plist:                                        # :989-990
        particulate_event(sim, p, forces, inputs, branch)
    moved = [(p, sum(abs(p.pos[c]) > 0.5 for c in range(box.dim))) for p in plist]
    plist, _sent = box.particle_bc(plist, sim.sides)       # :993
    assert not _sent
    if record is not None:
        kept = set(id(p) for p in plist)
        for p, nout in moved:
            if nout == 0:
                c = box.locate(p.pos)
                if c is not None and c.level != before[id(p)]:
                    record["fine_to_coarse" if c.level < before[id(p)] else "coarse_to_fine"] += 1
                continue
            if nout >= 2:
                record["left_through_edge"] += 1
            record["wrapped" if id(p) in kept else "removed"] += 1
    for coeff in forces:                                   # :1004-1012
        if coeff.kind == INERTIAL:                         # :1007
            sim.un = store_previous_vel(box, sim.u, sim.sides)                    # :1009
    return plist
