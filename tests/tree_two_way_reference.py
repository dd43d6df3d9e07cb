"""GfsParticulateField and the event of GfsSourceParticulate (modules/particulatecommon.c:1927-2228) on a REFINED
box: two_way_reference on the cell trees of tree_sampler_reference.TreeBox, and the MAC value of the velocity source
(source_particulate_value, :2029-2065) with gfs_face_interpolated_value_generic (src/fluid.c:2186-2253).

Plain Python floats in the reference's operand order, the reference's file:line at every step; written from the
reference's text, not from csrc/.  No index arithmetic: the leaf of a particle comes from TreeBox.locate, the
descent goes through the children a cell holds, the neighbours come from TreeBox.neighbor, the position and the
size of a cell from the cell.  A field is one array with ghosts per level (TreeBox.field); results are written
into such arrays through the cells' own indices.

normalized_distance is two_way_reference's, gfs_neighbor_value and the forces are tree_forces_reference's; neither
file is edited or patched.  The line numbers are those of modules/particulatecommon.c unless a file is named.

Test infrastructure only.
"""
import collections
import math

import sampler_reference as R
import forces_reference as F
import tree_forces_reference as TF
from two_way_reference import normalized_distance

# the branches of a gfs_face_interpolated_value_generic on the positive face of a leaf
SAME_LEAF, COARSER, CHILDREN = "same-level-leaf", "coarser", "children"
GHOST_BOUNDARY, GHOST_PERIODIC, NO_NEIGHBOR = "ghost-boundary", "ghost-periodic", "no-neighbour"


def zeros(box):
    """a field of zeros: one array with ghosts per level, nested lists"""
    out = []
    for l in range(box.level + 1):
        r = (1 << l) + 2
        out.append([[0.]*r for _ in range(r)] if box.dim == 2 else [[[0.]*r for _ in range(r)] for _ in range(r)])
    return out


def get(box, cell, v):
    return box.value(cell, v)


def put(box, cell, v, x):
    i, j, k = cell.ijk
    a = v[cell.level]
    if box.dim == 2:
        a[j][i] = x
    else:
        a[k][j][i] = x


def cell_volume(box, cell):
    """ftt_cell_volume, src/ftt.h:  size*size[*size]"""
    size = box.cell_size(cell)
    return size*size*size if box.dim == 3 else size*size


def void_fraction(box, plist, v=None):
    """particulate_field_event (:1934-1957): v reset on the leaves (:1944-1945), then voidfraction_from_particles
    (:1929-1932) for every particle with a cell (:1949-1950), in list order.  plist: objects with pos, volume"""
    v = zeros(box) if v is None else v
    for cell in box.leaves:
        put(box, cell, v, 0.)
    for p in plist:
        cell = box.locate(p.pos)
        if cell is not None:
            put(box, cell, v, get(box, cell, v) + p.volume/cell_volume(box, cell))
    return v


def cond_kernel(box, cell, p, rkernel):
    """cond_kernel (:2126-2156) of a cell of any level"""
    dim = box.dim
    pos = box.cell_pos(cell)                                       # ftt_cell_pos, :2134
    size = box.cell_size(cell)/2.                                  # :2135
    radeq = size*math.sqrt(2.) if dim == 2 else size*math.sqrt(3.)          # :2137-2141
    if dim == 2:                                                   # ftt_vector_distance, src/ftt.h:53-59
        dist = math.sqrt((pos[0] - p[0])*(pos[0] - p[0]) + (pos[1] - p[1])*(pos[1] - p[1]))
    else:
        dist = math.sqrt((pos[0] - p[0])*(pos[0] - p[0]) + (pos[1] - p[1])*(pos[1] - p[1]) +
                         (pos[2] - p[2])*(pos[2] - p[2]))
    if dist - radeq <= rkernel:                                    # :2143-2144
        return True
    for c in range(dim):                                           # :2146-2153
        if p[c] > pos[c] + size or p[c] < pos[c] - size:
            return False
    return True


def descent(box, p, rkernel):
    """the leaves gfs_domain_cell_traverse_condition (src/domain.c:1550-1574, FTT_PRE_ORDER, FTT_TRAVERSE_LEAFS)
    visits with cond_kernel, in its order: ftt_cell_traverse_condition (src/ftt.c:948-986) returns at a cell that
    fails, visits a leaf, and goes through the children 0 .. FTT_CELLS - 1 of the others"""
    out = []

    def traverse(cell):
        if not cond_kernel(box, cell, p, rkernel):                 # src/ftt.c:957-958
            return
        if cell.children is None:                                  # :960-963 (pre-order), leaves only
            out.append(cell)
            return
        for ch in cell.children:                                   # :965-975
            if not ch.destroyed:
                traverse(ch)

    traverse(box.root)
    return out


def kernel_volume(box, leaves, p, volume, K, t=0.):
    """kernel_volume (:2108-2119) over the visited leaves, then :2216: (volume, correction)"""
    ksum, correction = 0., 0.
    for cell in leaves:
        cellvol = cell_volume(box, cell)
        q = normalized_distance(box.dim, box.cell_pos(cell), p, volume)
        ksum += cellvol                                            # :2116
        correction += K(q[0], q[1], q[2], t)*cellvol               # :2117
    correction = correction/ksum if leaves else float("nan")     # :2216
    return ksum, correction


def diffuse_force(box, leaves, p, volume, force, correction, K, Fv, t=0.):
    """diffuse_force (:2158-2175) over the same leaves; liq_rho = 1. (no alpha)"""
    if not correction > 1.e-10:                                    # :2164
        return
    for cell in leaves:
        cellvol = cell_volume(box, cell)
        q = normalized_distance(box.dim, box.cell_pos(cell), p, volume)
        k = K(q[0], q[1], q[2], t)
        liq_rho = 1.
        for c in range(box.dim):                                   # :2170-2172
            put(box, cell, Fv[c], get(box, cell, Fv[c]) - force[c]/liq_rho/cellvol*k/correction)


def spread(box, plist, rkernel, K, t=0., Fv=None):
    """source_particulate_event (:2177-2228) from the stored forces: F reset on the leaves (:2189-2191), then per
    particle in list order the two traversals (:2208-2222).  plist: objects with pos, volume, force.
    Returns (F, corrections, leaves reached per particle)"""
    Fv = [zeros(box) for _ in range(box.dim)] if Fv is None else Fv
    for c in range(box.dim):
        for cell in box.leaves:
            put(box, cell, Fv[c], 0.)
    corrections, reached = [], []
    for p in plist:
        pos = [float(a) for a in p.pos]
        leaves = descent(box, pos, rkernel)
        _vol, correction = kernel_volume(box, leaves, pos, p.volume, K, t)
        corrections.append(correction)
        reached.append(leaves)
        diffuse_force(box, leaves, pos, p.volume, p.force, correction, K, Fv, t)
    return Fv, corrections, reached


def forces_on_fluid(sim, plist, forces, inputs=None):
    """the first loop of source_particulate_event, :2199-2206, with compute_forces_onfluid (:753-765) and the
    forces of tree_forces_reference: every force but the buoyancy, no move; the list is untouched"""
    for p in plist:
        p.force = [0., 0., 0.]                                     # :2201-2202
        for coeff in forces:                                       # :2203-2204
            if coeff.kind != F.BUOY:                               # :756
                new_force = TF._force_of(sim, p, coeff, inputs)    # :757
                total = [0., 0., F.ONFLUID_FORCE_Z_2D]
                for c in range(sim.dim):
                    total[c] = new_force[c]*p.volume + p.force[c]  # :760-761
                p.force = total                                    # :763


# -------------------------------------------------------------------------------------------------
# src/fluid.c
# -------------------------------------------------------------------------------------------------

def face_interpolated_value(box, cell, neighbor, d, v, census=None):
    """gfs_face_interpolated_value, src/fluid.c:2186-2200, of the face (cell, neighbor, d)"""
    x1 = 1.                                                        # :2189
    if neighbor is not None:                                       # :2193
        v1, nx, _branch = TF.neighbor_value(box, cell, neighbor, d, v, census)      # :2196
        if nx is not None:
            x1 = nx
        return ((x1 - 0.5)*box.value(cell, v) + 0.5*v1)/x1         # :2197
    return box.value(cell, v)                                      # :2200


def face_interpolated_value_generic(box, cell, d, v, census=None, sides=None):
    """gfs_face_interpolated_value_generic, src/fluid.c:2232-2253, of the face d of `cell'.  census: a Counter of the
    branch the face took (sides, the GFSHIP_SIDE_* of the box, tells a ghost of a GfsBoundary from a periodic one)"""
    neighbor = box.neighbor(cell, d)
    if neighbor is None or neighbor.children is None or neighbor.level < cell.level:          # :2237-2238
        if census is not None:
            if neighbor is None:
                census[NO_NEIGHBOR] += 1
            elif neighbor.boundary:
                periodic = sides is not None and sides[neighbor.tree] == R.SIDE_PERIODIC
                census[GHOST_PERIODIC if periodic else GHOST_BOUNDARY] += 1
            else:
                census[COARSER if neighbor.level < cell.level else SAME_LEAF] += 1
        return face_interpolated_value(box, cell, neighbor, d, v)
    # finer neighbour: the mean of the values of its children on the face (:2241-2251)
    if census is not None:
        census[CHILDREN] += 1
    od = R.opposite(d)
    avg, n = 0., 0
    for i in TF.CHILDREN_DIRECTION[box.dim][od]:                   # ftt_cell_children_direction (neighbor, od)
        n += 1
        ch = neighbor.children[i]
        if not ch.destroyed:                                       # :2247
            avg += face_interpolated_value(box, ch, cell, od, v)*1.                 # :2248-2249
    return 0. if avg == 0. else avg/(1.*n)                         # :2251


def mac_source_value(box, cell, c, Fc, census=None, sides=None):
    """source_particulate_value (:2029-2065): F_c on the positive face (right, top, front) of component c"""
    return face_interpolated_value_generic(box, cell, 2*c, Fc, census, sides)


def mac_source(box, c, Fc, census=None, sides=None):
    """the MAC value on every leaf: a field, 0. elsewhere"""
    out = zeros(box)
    for cell in box.leaves:
        put(box, cell, out, mac_source_value(box, cell, c, Fc, census, sides))
    return out


def new_census():
    return collections.Counter()
