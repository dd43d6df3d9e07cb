"""The point sampler and the particle walk of the reference, restated on an explicit cell graph.

Plain Python, floats only.  Written from the reference's source (file:line given at every step), not
from oracle/go_particles.c or csrc/particles.hip: there is no index arithmetic that decides whether
a neighbour exists.  One box of 2^level cells per side is built as the reference holds it in memory:
a cell tree for the box and one flattened cell tree per box side, and every neighbour is found the
way ftt_cell_neighbor finds it.  The only modelling is that graph; field values are read from the
arrays-with-ghosts layout of the tests (index [k][j][i], 0 and n + 1 are the ghost layers).

Test infrastructure only.
"""
import sys

FTT_RIGHT, FTT_LEFT, FTT_TOP, FTT_BOTTOM, FTT_FRONT, FTT_BACK = range(6)    # src/ftt.h:84-93
GFS_NODATA = sys.float_info.max                                             # src/utils.h:80: G_MAXDOUBLE
SIDE_PERIODIC, SIDE_BOUNDARY, SIDE_EXTERNAL = 0, 1, 2                       # GfsBoundaryPeriodic, GfsBoundary,
#                                                                             GfsBoundaryMpi


def opposite(d):
    """FTT_OPPOSITE_DIRECTION, src/ftt.h (ftt_opposite_direction = {1,0,3,2,5,4})"""
    return (1, 0, 3, 2, 5, 4)[d]


# coords[n]: position of child n relative to its parent, src/ftt.c:301-316
COORDS = {2: ((-1., 1., 0.), (1., 1., 0.), (-1., -1., 0.), (1., -1., 0.)),
          3: ((-1., 1., 1.), (1., 1., 1.), (-1., -1., 1.), (1., -1., 1.),
              (-1., 1., -1.), (1., 1., -1.), (-1., -1., -1.), (1., -1., -1.))}
# neighbor_index[d][n], src/ftt.h:495-507: >= 0 a brother of the same oct, < 0 child -n-1 of the
# parent's neighbour
NEIGHBOR_INDEX = {2: ((1, -1, 3, -3), (-2, 0, -4, 2), (-3, -4, 0, 1), (2, 3, -1, -2)),
                  3: ((1, -1, 3, -3, 5, -5, 7, -7), (-2, 0, -4, 2, -6, 4, -8, 6),
                      (-3, -4, 0, 1, -7, -8, 4, 5), (2, 3, -1, -2, 6, 7, -5, -6),
                      (-5, -6, -7, -8, 0, 1, 2, 3), (4, 5, 6, 7, -1, -2, -3, -4))}
# index[d][i] of ftt_cell_flatten, src/ftt.c:1488-1500: the children on side d of their parent
FLATTEN_INDEX = {2: ((1, 3), (0, 2), (0, 1), (2, 3)),
                 3: ((1, 3, 5, 7), (0, 2, 4, 6), (0, 1, 4, 5), (2, 3, 6, 7), (0, 1, 2, 3), (4, 5, 6, 7))}
# corner[i], src/fluid.c:2588-2605
CORNER = {2: ((FTT_LEFT, FTT_BOTTOM), (FTT_RIGHT, FTT_BOTTOM), (FTT_RIGHT, FTT_TOP), (FTT_LEFT, FTT_TOP)),
          3: ((FTT_LEFT, FTT_BOTTOM, FTT_FRONT), (FTT_RIGHT, FTT_BOTTOM, FTT_FRONT),
              (FTT_RIGHT, FTT_TOP, FTT_FRONT), (FTT_LEFT, FTT_TOP, FTT_FRONT),
              (FTT_LEFT, FTT_BOTTOM, FTT_BACK), (FTT_RIGHT, FTT_BOTTOM, FTT_BACK),
              (FTT_RIGHT, FTT_TOP, FTT_BACK), (FTT_LEFT, FTT_TOP, FTT_BACK))}
# path[i][j], src/fluid.c:2938-2954: DIM directions (+-(1 + index into d)), then the index of the cell
# the path leads to
PATH = {2: (((1, 2, 1), (2, 1, 2)),
            ((2, -1, 3), (-1, 2, 0)),
            ((1, -2, 3), (-2, 1, 0)),
            ((-1, -2, 2), (-2, -1, 1))),
        3: (((1, 2, 3, 1), (2, 1, 3, 2), (3, 1, 2, 4)),
            ((2, 3, -1, 3), (3, 2, -1, 5), (-1, 2, 3, 0)),
            ((1, -2, 3, 3), (3, -2, 1, 6), (-2, 3, 1, 0)),
            ((3, -1, -2, 7), (-2, -1, 3, 1), (-1, -2, 3, 2)),
            ((2, 1, -3, 6), (1, 2, -3, 5), (-3, 1, 2, 0)),
            ((2, -1, -3, 7), (-1, 2, -3, 4), (-3, 2, -1, 1)),
            ((1, -2, -3, 7), (-2, 1, -3, 4), (-3, 1, -2, 2)),
            ((-1, -2, -3, 6), (-2, -1, -3, 5), (-3, -1, -2, 3)))}


class IntersectionFailed(Exception):
    """check_intersetion found no face (modules/particulatecommon.c:3146-3147): the reference then
    reads a direction nobody wrote (`FttDirection d' of list_boundary_particles, :3336, is not
    initialised); the input has no defined outcome"""


class Cell:
    """FttCell: `parent' stands for the oct (parent->cell[id] are the brothers, src/ftt.h), a root
    keeps its own neighbours (struct _FttRootCell)"""
    __slots__ = ("parent", "id", "children", "level", "q", "pos", "destroyed", "boundary",
                 "root_neighbors", "ijk", "tree")

    def __init__(self, parent, n, level, q, pos):
        self.parent, self.id, self.level, self.q, self.pos = parent, n, level, q, pos
        self.children = None
        self.destroyed = False          # FTT_FLAG_DESTROYED
        self.boundary = False           # GFS_FLAG_BOUNDARY
        self.root_neighbors = None
        self.ijk = None                 # index into the arrays with ghosts (leaves only)
        self.tree = None                # None: the box; d: the boundary of box side d

    def __repr__(self):
        return "Cell%s%s" % (self.ijk, "" if self.tree is None else "[ghost of side %d]" % self.tree)


class Box:
    """One GfsBox of unit size centred on the origin, refined uniformly to `level', and the boundary
    objects of its 2*dim sides.

    - the box: an FttCell tree, children made by oct_new (src/ftt.c:45-83), positions by coords[]
      (:301-316);
    - every side d holds a GfsBoundary of some class in box->neighbor[d] (periodic:
      src/boundary.c:1526, plain and MPI: gfs_boundary_new :840-853) with boundary->d =
      FTT_OPPOSITE_DIRECTION (d) (:853), the direction from the boundary to the box;
    - boundary_match (:652-685) roots a NEW cell tree per boundary (:657), links its root and the
      box root and nothing else (ftt_cell_set_neighbor_match, :660, src/ftt.c:681-686: the other
      neighbours of the boundary root stay NULL), refines every boundary cell whose box neighbour
      is refined (match, :638-642), flags every cell it visits GFS_FLAG_BOUNDARY (:582; whatever
      the class of the boundary: periodic_match calls boundary_match first, :1307-1309) and
      flattens the tree (:683, src/ftt.c:1476-1515): the half of every oct away from the box is
      destroyed.
    """

    def __init__(self, dim, level):
        assert dim in (2, 3) and level >= 0
        self.dim, self.level, self.n = dim, level, 1 << level
        self.ncells, self.ndir = 1 << dim, 2*dim
        self.root = self._new_root(None, (0., 0., 0.))
        self._refine(self.root)
        self.boundary = []
        for d in range(self.ndir):
            bd = opposite(d)                                   # boundary->d, src/boundary.c:853
            c, sign = d//2, (1. if d % 2 == 0 else -1.)
            pos = [0., 0., 0.]
            pos[c] += sign*1.                                  # rpos[d]*size, src/boundary.c:662-669
            broot = self._new_root(d, tuple(pos))
            broot.root_neighbors[bd] = self.root               # src/ftt.c:681
            self.root.root_neighbors[d] = broot                # src/ftt.c:685
            self._refine(broot)                                # match: src/boundary.c:638-642
            self._flatten(broot, bd)                           # src/boundary.c:683
            self.boundary.append(broot)
        self._inter = {}
        self._index_leaves()

    # -- construction -----------------------------------------------------------------------------
    def _new_root(self, tree, pos):
        r = Cell(None, 0, 0, (0, 0, 0), pos)
        r.root_neighbors = [None]*self.ndir                    # g_malloc0, src/ftt.c:97
        r.tree = tree
        r.boundary = tree is not None
        return r

    def _refine(self, cell):
        if cell.level == self.level:
            return
        size = 1./(1 << (cell.level + 1))/2.                   # half the size of a child
        cell.children = []
        for n in range(self.ncells):
            co = COORDS[self.dim][n]
            q = tuple(2*cell.q[c] + (1 if co[c] > 0. else 0) for c in range(3))
            pos = tuple(cell.pos[c] + co[c]*size for c in range(3))
            ch = Cell(cell, n, cell.level + 1, q, pos)
            ch.tree, ch.boundary = cell.tree, cell.boundary    # src/boundary.c:582
            cell.children.append(ch)
        for ch in cell.children:
            self._refine(ch)

    def _flatten(self, root, d):
        """ftt_cell_flatten, src/ftt.c:1476-1515"""
        if root.children is None:
            return
        od = opposite(d)
        for i in FLATTEN_INDEX[self.dim][od]:
            self._destroy(root.children[i])
        for i in FLATTEN_INDEX[self.dim][d]:
            self._flatten(root.children[i], d)

    def _destroy(self, cell):
        cell.destroyed = True
        if cell.children:
            for ch in cell.children:
                self._destroy(ch)

    def _index_leaves(self):
        self.leaves, self.ghosts = [], []

        def walk(cell):
            if cell.destroyed:
                return
            if cell.children is None:
                ijk = [cell.q[c] + 1 if c < self.dim else 0 for c in range(3)]
                if cell.tree is not None:
                    c = cell.tree//2
                    ijk[c] += self.n if cell.tree % 2 == 0 else -self.n
                cell.ijk = tuple(ijk)
                (self.leaves if cell.tree is None else self.ghosts).append(cell)
            else:
                for ch in cell.children:
                    walk(ch)
        walk(self.root)
        for b in self.boundary:
            walk(b)
        self.by_ijk = {c.ijk: c for c in self.leaves}

    # -- the tree ---------------------------------------------------------------------------------
    def neighbor(self, cell, d):
        """ftt_cell_neighbor of a leaf = ftt_cell_neighbor_not_cached, src/ftt.h:492-530.  The
        neighbour of the parent is asked for again here where the reference reads the copy kept in
        the oct (cell->parent->neighbors.c[d], :522): on a tree that no longer changes the two agree
        (ftt_cell_check, src/ftt.c:110-134)."""
        if cell.parent is None:
            return cell.root_neighbors[d]                      # :515-516
        n = NEIGHBOR_INDEX[self.dim][d][cell.id]
        if n >= 0:
            c = cell.parent.children[n]                        # :519-520
        else:
            c = self.neighbor(cell.parent, d)                  # :522
            if c is not None and c.children is not None:
                c = c.children[-n - 1]                         # :523-524
        if c is None or c.destroyed:                           # :526-527
            return None
        return c

    def cell_pos(self, cell):
        return cell.pos

    def cell_size(self, cell):
        return 1./(1 << cell.level)

    def locate(self, target):
        """ftt_cell_locate (root, target, -1), src/ftt.c:1535-1574"""
        root = self.root
        pos = list(root.pos)
        size = self.cell_size(root)/2.
        for c in range(self.dim):
            if target[c] > pos[c] + size or target[c] < pos[c] - size:     # :1547-1553
                return None
        while True:
            if root.children is None:                                      # :1556-1557
                return root
            if self.dim == 2:                                              # :1559-1560
                n = ((2, 3), (0, 1))[target[1] > pos[1]][target[0] > pos[0]]
            else:                                                          # :1562-1563
                n = (((6, 7), (4, 5)), ((2, 3), (0, 1)))[target[2] > pos[2]][target[1] > pos[1]][target[0] > pos[0]]
            root = root.children[n]
            size /= 2.
            for c in range(self.dim):
                pos[c] += COORDS[self.dim][n][c]*size                      # :1567-1571
            if root.destroyed:                                             # :1572-1573
                return None

    # -- the corner interpolator ------------------------------------------------------------------
    def _corner_neighbor(self, cell, d1):
        """cell_corner_neighbor, src/fluid.c:2813-2846, every cell a leaf of one level: the neighbour
        in direction d1[0] (:2818) or NULL (:2819-2820); `neighbor is at the same level' (:2830-2832)"""
        return self.neighbor(cell, d1[0])

    def _do_path(self, cell, i, n, d):
        """do_path, src/fluid.c:2925-2981, without T-junctions (one level)"""
        dim = self.dim
        for j in range(dim):
            k = PATH[dim][i][j][dim]
            if n[k] is None:
                d1 = [opposite(d[-p - 1]) if p < 0 else d[p - 1] for p in PATH[dim][i][j][:dim]]   # :2965-2967
                n[k] = self._corner_neighbor(cell, d1)                                             # :2968
                if n[k] is not None:
                    self._do_path(n[k], k, n, d)                                                   # :2973-2974

    def corner_cells(self, cell, d):
        """n[] of gfs_cell_corner_interpolator after do_path (src/fluid.c:3032-3035)"""
        n = [None]*self.ncells
        n[0] = cell
        self._do_path(cell, 0, n, d)
        return n

    def corner_interpolator(self, cell, d):
        """gfs_cell_corner_interpolator, src/fluid.c:3015-3069: list of (cell, weight)"""
        key = (id(cell), tuple(d))
        if key in self._inter:
            return self._inter[key]
        n = self.corner_cells(cell, d)
        w = 0.
        boundaries = 0
        ic, iw = [], []
        for i in range(self.ncells):                           # :3045-3054
            if n[i] is not None:
                # distance (), :2983-2992, of a cell without solid: size times the constant
                dist = self.cell_size(n[i])*(0.707106781185 if self.dim == 2 else 0.866025403785)
                a = 1./(dist + 1e-12)                          # :3048
                ic.append(n[i])
                iw.append(a)
                w += a
                if n[i].boundary:                              # :3052-3053
                    boundaries += 1
        if len(ic) == self.dim + 1 and boundaries == self.dim:  # :3057
            w -= iw[0]                                         # :3059
            del ic[0], iw[0]                                   # :3060-3064
        assert w > 0.                                          # :3067
        b = 1./w
        iw = [x*b for x in iw]                                 # interpolator_scale, :2872-2877
        r = list(zip(ic, iw))
        self._inter[key] = r
        return r

    # -- values -----------------------------------------------------------------------------------
    def field(self, a):
        """nested lists of Python floats of an array with ghosts, (n+2)^dim"""
        a = a.tolist() if hasattr(a, "tolist") else a
        assert len(a) == self.n + 2
        return a

    def value(self, cell, v):
        i, j, k = cell.ijk
        return v[j][i] if self.dim == 2 else v[k][j][i]

    def corner_value(self, cell, d, v, nodata=True):
        """gfs_cell_corner_value, src/fluid.c:3081-3101"""
        val = 0.
        for c, w in self.corner_interpolator(cell, d):
            v1 = self.value(c, v)
            if nodata and v1 == GFS_NODATA:                    # :3096-3097
                return self.value(cell, v)
            val += w*v1                                        # :3098
        return val

    def corner_values(self, cell, v, nodata=True):
        """gfs_cell_corner_values, src/fluid.c:2617-2630"""
        f = [self.corner_value(cell, d, v, nodata) for d in CORNER[self.dim]]
        f.append(self.value(cell, v))
        return f

    def interpolate_from_corners(self, cell, p, f):
        """gfs_interpolate_from_corners, src/fluid.c:2640-2683"""
        o = self.cell_pos(cell)
        size = self.cell_size(cell)/2.
        px = (p[0] - o[0])/size
        py = (p[1] - o[1])/size
        if self.dim == 2:
            x, y, v = (px + py)/2., (py - px)/2., f[4]
            if x > 0.:
                v += x*(f[2] - f[4])
            else:
                v -= x*(f[0] - f[4])
            if y > 0.:
                v += y*(f[3] - f[4])
            else:
                v -= y*(f[1] - f[4])
            return v
        pz = (p[2] - o[2])/size
        c = [- f[0] + f[1] + f[2] - f[3] - f[4] + f[5] + f[6] - f[7],
             - f[0] - f[1] + f[2] + f[3] - f[4] - f[5] + f[6] + f[7],
             f[0] + f[1] + f[2] + f[3] - f[4] - f[5] - f[6] - f[7],
             f[0] - f[1] + f[2] - f[3] + f[4] - f[5] + f[6] - f[7],
             - f[0] + f[1] + f[2] - f[3] + f[4] - f[5] - f[6] + f[7],
             - f[0] - f[1] + f[2] + f[3] + f[4] + f[5] - f[6] - f[7],
             f[0] - f[1] + f[2] - f[3] - f[4] + f[5] - f[6] + f[7],
             f[0] + f[1] + f[2] + f[3] + f[4] + f[5] + f[6] + f[7]]
        return (c[0]*px + c[1]*py + c[2]*pz +
                c[3]*px*py + c[4]*px*pz + c[5]*py*pz +
                c[6]*px*py*pz +
                c[7])/8.

    def interpolate(self, cell, p, v, nodata=True):
        """gfs_interpolate, src/fluid.c:2697-2710.  nodata = False: GFS_NODATA is a number like any
        other (neither :2704-2705 nor :3096-3097)"""
        if nodata and self.value(cell, v) == GFS_NODATA:       # :2704-2705
            return GFS_NODATA
        return self.interpolate_from_corners(cell, p, self.corner_values(cell, v, nodata))

    def sample(self, v, points, nodata=True):
        """GfsOutputLocation, src/output.c:1182-1199: (values, inside); 0. where outside"""
        out, inside = [], []
        for p in points:
            cell = self.locate(p)
            inside.append(cell is not None)
            out.append(self.interpolate(cell, p, v, nodata) if cell is not None else 0.)
        return out, inside

    # -- particles --------------------------------------------------------------------------------
    def advect_point(self, u, p, dt):
        """gfs_domain_advect_point, src/domain.c:2764-2788: the new position (p itself where the
        point or its midpoint is outside)"""
        p0, p1 = list(p), list(p)
        cell = self.locate(p0)
        if cell is None:                                       # :2778-2779
            return list(p)
        for c in range(self.dim):
            p1[c] += dt*self.interpolate(cell, p0, u[c])/2.     # :2782
        cell = self.locate(p1)
        if cell is None:                                       # :2784-2785
            return list(p)
        r = list(p)
        for c in range(self.dim):
            r[c] += dt*self.interpolate(cell, p1, u[c])         # :2787
        return r

    def check_intersetion(self, cellpos, p0, p1, size):
        """check_intersetion, modules/particulatecommon.c:3058-3148: the first direction whose face
        of the cell the segment crosses.  The reference leaves *dstore as it was when it finds
        none; here that raises."""
        dim = self.dim
        for d in range(self.ndir):
            normal = float(opposite(d)) - float(d)             # :3068
            c = d//2
            if (p1[c] - p0[c]) != 0 and normal*(p1[c] - p0[c]) > 0:
                t = (cellpos[c] + normal*size*0.5 - p0[c])/(p1[c] - p0[c])
                ok = True
                for a in range(dim):                           # py, pz / px, pz / px, py in this order
                    if a != c:
                        pa = p0[a] + t*(p1[a] - p0[a])
                        ok = ok and (pa - cellpos[a] + size*0.5)*(pa - cellpos[a] - size*0.5) <= 0
                if ok and t*(t - 1) <= 0:
                    return d
        raise IntersectionFailed((cellpos, p0, p1))

    def boundarycell(self, pos_old, pos):
        """boundarycell, modules/particulatecommon.c:3151-3186: (cell, d)"""
        cell = self.locate(pos_old)
        assert cell is not None                                # :3155
        d = self.check_intersetion(self.cell_pos(cell), pos_old, pos, self.cell_size(cell))
        nb = self.neighbor(cell, d)                            # ftt_cell_face, :3163
        if nb is None:
            return cell, d
        while not nb.boundary:                                 # :3168
            cell = nb
            d = self.check_intersetion(self.cell_pos(cell), pos_old, pos, self.cell_size(cell))
            nb = self.neighbor(cell, d)
            if nb is None:
                return cell, d
        return cell, d

    def periodic_bc_particle(self, d, p):
        """periodic_bc_particle, modules/particulatecommon.c:3189-3214, the matching box is the box
        itself: sets pos and pos_old along d/2"""
        box_face, box_face_nbr = list(self.root.pos), list(self.root.pos)
        size = self.cell_size(self.root)
        normal = float(opposite(d)) - float(d)
        box_face[d//2] += normal*size/2.
        box_face_nbr[d//2] -= normal*size/2.
        tolerance = size/1.e8
        distance = (p.pos[d//2] - box_face[d//2])*normal
        p.pos[d//2] = box_face_nbr[d//2] + distance + normal*tolerance
        p.pos_old[d//2] = p.pos[d//2]

    def remove_particles_not_in_domain(self, plist):
        """modules/particulatecommon.c:955-969"""
        return [p for p in plist if self.locate(p.pos) is not None]

    def particle_bc(self, plist, sides):
        """gfs_particle_bc, modules/particulatecommon.c:3375-3395: list_boundary_particles (:3326-3359)
        takes every particle whose position is outside off the list and notes the side it left
        through; box_send_bc / send_particles (:3248-3312) hand it to periodic_bc_particle, which puts
        it back (:3212), only where that side is a GfsBoundaryPeriodic; through a GfsBoundaryMpi it
        is sent away (`sent'), through any other boundary nothing puts it back.

        The order of the list: the reference keeps its particles in a container of the GTS library,
        which is not part of the reference's tree; a particle that is put back is taken to keep its
        place, as the oracle and the device do."""
        keep, sent = [], []
        for p in plist:
            if self.locate(p.pos) is not None:                 # :3333-3334
                keep.append(p)
                continue
            cell, d = self.boundarycell(p.pos_old, p.pos)
            if sides[d] == SIDE_PERIODIC:
                self.periodic_bc_particle(d, p)
                keep.append(p)
            elif sides[d] == SIDE_EXTERNAL:
                sent.append((d, p))
        return keep, sent

    def list_event(self, u, plist, dt, sides):
        """gfs_particle_list_event, modules/particulatecommon.c:980-1015, of plain tracers
        (gfs_particle_event, src/particle.c:31-44: pos_old = pos, then gfs_domain_advect_point).
        u: the velocity components as field () lists.  Returns (the new list, the particles sent
        through GfsBoundaryMpi sides)."""
        plist = self.remove_particles_not_in_domain(plist)     # :987
        for p in plist:
            p.pos_old = list(p.pos)
            p.pos = self.advect_point(u, p.pos, dt)
        return self.particle_bc(plist, sides)                  # :993


class Particle:
    __slots__ = ("pos", "pos_old", "id")

    def __init__(self, pos, pid):
        self.pos = [float(x) for x in pos]
        self.pos_old = list(self.pos)
        self.id = int(pid)


def list_event(box, u, positions, ids, dt, sides, nevents=1):
    """`nevents' events of a list of plain tracers created at `positions': the state after every event
    as (positions, old positions, ids) of the particles on the list, in list order"""
    uf = [box.field(a) for a in u]
    plist = [Particle(p, i) for p, i in zip(positions, ids)]
    states = []
    for _ in range(nevents):
        plist, _sent = box.list_event(uf, plist, dt, sides)
        states.append(([list(p.pos) for p in plist], [list(p.pos_old) for p in plist],
                       [p.id for p in plist]))
    return states
