"""The point sampler and the particle walk of the reference on a REFINED box: sampler_reference.Box
with cells of several levels.

Plain Python, floats only, written from the reference's source (file:line at every step), not from
csrc/tree_particles.hip.  The box is an FttCell tree refined where a set of cells (or the flags of the
library's dense levels) says so; the boundary of every side is a cell tree of its own, refined where
the box cell it touches is refined (match, src/boundary.c:576-650) and flattened.  What changes with
respect to a box of one level is the walk around a corner: cell_corner_neighbor meets coarser and
deeper neighbours, do_path gives up at a T-junction and t_junction_interpolator builds the result from
interpolators of the coarse neighbour (src/fluid.c:2813-2981).  locate, interpolate_from_corners,
advect_point, boundarycell and list_event are those of sampler_reference.Box: they speak of cells.

Field values are read from one array with ghosts per level (index [k][j][i], 0 and n_l + 1 the ghost
layers of level l).

Test infrastructure only.
"""
import collections

from sampler_reference import (Box, Cell, COORDS, CORNER, FLATTEN_INDEX, PATH, opposite, GFS_NODATA,  # noqa: F401
                               SIDE_PERIODIC, SIDE_BOUNDARY, IntersectionFailed, Particle,
                               FTT_RIGHT, FTT_LEFT, FTT_TOP, FTT_BOTTOM, FTT_FRONT, FTT_BACK)

NONE, LEAF, NODE = 0, 1, 2      # the bytes of gfship_tree_flags

# index[d[0]][d[1]] of ftt_cell_child_corner, src/ftt.h:371-376 (FTT_2D)
CHILD_CORNER_2D = ((-1, -1, 1, 3), (-1, -1, 0, 2), (1, 0, -1, -1), (3, 2, -1, -1))
# b[FTT_CELL_ID][d] of ftt_cell_neighbor_is_brother, src/ftt.h:624-631
IS_BROTHER = {2: ((1, 0, 0, 1), (0, 1, 0, 1), (1, 0, 1, 0), (0, 1, 1, 0)),
              3: ((1, 0, 0, 1, 0, 1), (0, 1, 0, 1, 0, 1), (1, 0, 1, 0, 0, 1), (0, 1, 1, 0, 0, 1),
                  (1, 0, 0, 1, 1, 0), (0, 1, 0, 1, 1, 0), (1, 0, 1, 0, 1, 0), (0, 1, 1, 0, 1, 0))}
INTERPOLATOR_MAX = {2: 7, 3: 29}        # g_assert (j < 7) / (j < 29), src/fluid.c:2860-2864

BRANCHES = ("same_level", "coarser", "coarser_t_junction", "deeper", "deeper_child_destroyed",
            "t_junction_2d", "t_junction_3d_d1", "t_junction_3d_d2", "t_junction_3d_four",
            "mixed_level_weights", "domain_corner", "descent_at_top")


def child_corner_index(dim, d):
    """the index of ftt_cell_child_corner (src/ftt.h:366-422): the child whose coords[] (src/ftt.c:301-316)
    point the way of every direction of d; the FTT_2D table is the reference's, literally"""
    for n in range(1 << dim):
        if all(COORDS[dim][n][x // 2] == (1. if x % 2 == 0 else -1.) for x in d[:dim]):
            if dim == 2:
                assert CHILD_CORNER_2D[d[0]][d[1]] == n
            return n
    raise AssertionError("directions %s are not perpendicular" % (d,))


# three entries of the FTT_3D table, src/ftt.h:387-406
assert child_corner_index(3, (FTT_RIGHT, FTT_TOP, FTT_FRONT)) == 1
assert child_corner_index(3, (FTT_LEFT, FTT_BOTTOM, FTT_BACK)) == 6
assert child_corner_index(3, (FTT_BACK, FTT_LEFT, FTT_TOP)) == 4


class TreeBox(Box):
    """One GfsBox of unit size refined to several levels.

    refined: the set of (level, (qx, qy, qz)) of the box cells that have children, q counted from the
    (-x, -y, -z) corner of the box, qz = 0 in 2-D (the root is (0, (0, 0, 0))); every parent of a
    refined cell must be in the set."""

    def __init__(self, dim, refined):
        self._refined = frozenset((int(l), tuple(int(x) for x in q)) for l, q in refined)
        for l, q in self._refined:
            assert l == 0 or (l - 1, tuple(x // 2 for x in q)) in self._refined, "orphan %s" % ((l, q),)
        depth = 1 + max(l for l, q in self._refined) if self._refined else 0
        self.branches = collections.Counter()
        Box.__init__(self, dim, depth)

    @classmethod
    def from_flags(cls, dim, flags):
        """flags[l]: the (n_l + 2)^dim bytes of gfship_tree_flags; the interior cells that are NODE"""
        refined = set()
        for l, f in enumerate(flags):
            n = 1 << l
            f = f.tolist() if hasattr(f, "tolist") else f
            for k in range(1, n + 1) if dim == 3 else (0,):
                for j in range(1, n + 1):
                    for i in range(1, n + 1):
                        if (f[k][j][i] if dim == 3 else f[j][i]) == NODE:
                            refined.add((l, (i - 1, j - 1, k - 1 if dim == 3 else 0)))
        return cls(dim, refined)

    @classmethod
    def uniform(cls, dim, level):
        refined = set()
        for l in range(level):
            n = 1 << l
            for k in range(n if dim == 3 else 1):
                for j in range(n):
                    for i in range(n):
                        refined.add((l, (i, j, k)))
        return cls(dim, refined)

    # -- construction -----------------------------------------------------------------------------
    def _children(self, cell):
        """oct_new, src/ftt.c:45-83; positions by coords[], :301-316"""
        size = 1./(1 << (cell.level + 1))/2.
        cell.children = []
        for n in range(self.ncells):
            co = COORDS[self.dim][n]
            q = tuple(2*cell.q[c] + (1 if co[c] > 0. else 0) if c < self.dim else 0 for c in range(3))
            pos = tuple(cell.pos[c] + co[c]*size for c in range(3))
            ch = Cell(cell, n, cell.level + 1, q, pos)
            ch.tree, ch.boundary = cell.tree, cell.boundary    # src/boundary.c:582
            cell.children.append(ch)

    def _refine(self, cell):
        if cell.tree is None:
            if (cell.level, cell.q) not in self._refined:
                return
            self._children(cell)
            for ch in cell.children:
                self._refine(ch)
            return
        # match, src/boundary.c:576-650, of a cell of the boundary of side cell.tree; boundary->d is the
        # direction from the boundary to the box (:853)
        bd = opposite(cell.tree)
        neighbor = self.neighbor(cell, bd)                                  # :578
        if neighbor is None or neighbor.level < cell.level:                 # :585-592
            self._destroy(cell)
            return
        if neighbor.children is not None:                                   # :638-642
            self._children(cell)
            # ftt_cell_traverse_boundary (boundary->root, boundary->d, ...), :677-679: the children on
            # side boundary->d of their parent; the others go with ftt_cell_flatten (:683)
            for i in FLATTEN_INDEX[self.dim][bd]:
                self._refine(cell.children[i])

    def _index_leaves(self):
        """every cell that is not destroyed gets its index in the array with ghosts of its level"""
        self.leaves, self.ghosts, self.cells = [], [], []

        def walk(cell):
            if cell.destroyed:
                return
            n = 1 << cell.level
            ijk = [cell.q[c] + 1 if c < self.dim else 0 for c in range(3)]
            if cell.tree is not None:
                c = cell.tree//2
                ijk[c] += n if cell.tree % 2 == 0 else -n
            cell.ijk = tuple(ijk)
            self.cells.append(cell)
            if cell.children is None:
                (self.leaves if cell.tree is None else self.ghosts).append(cell)
            else:
                for ch in cell.children:
                    walk(ch)
        walk(self.root)
        for b in self.boundary:
            walk(b)
        self.by_ijk = {(c.level, c.ijk): c for c in self.leaves}

    def flags(self, level):
        """what gfship_tree_flags gives for this tree: nested lists of NONE / LEAF / NODE"""
        r = (1 << level) + 2
        f = [[[NONE]*r for _ in range(r)] for _ in range(r if self.dim == 3 else 1)]
        for c in self.cells:
            if c.level == level:
                i, j, k = c.ijk
                f[k][j][i] = LEAF if c.children is None else NODE
        return f if self.dim == 3 else f[0]

    # -- the corner interpolator ------------------------------------------------------------------
    def is_leaf(self, cell):
        return cell.children is None

    def child_corner(self, cell, d):
        """ftt_cell_child_corner, src/ftt.h:366-422"""
        assert cell.children is not None                                   # :380
        c = cell.children[child_corner_index(self.dim, d)]
        return None if c.destroyed else c                                  # :420-421

    def neighbor_is_brother(self, cell, d):
        """ftt_cell_neighbor_is_brother, src/ftt.h:620-638"""
        if cell.parent is None:
            return False
        return bool(IS_BROTHER[self.dim][cell.id][d])

    def _corner_neighbor(self, cell, d):
        """cell_corner_neighbor, src/fluid.c:2813-2846, max_level = -1: (neighbour, t_junction)"""
        neighbor = self.neighbor(cell, d[0])                               # :2818
        if neighbor is None:
            return None, False                                             # :2819-2820
        level = cell.level
        if neighbor.level < level:                                         # :2823
            # neighbor is at a shallower level
            if self.child_corner(cell.parent, d) is not cell:              # :2825
                self.branches["coarser_t_junction"] += 1
                return neighbor, True                                      # :2826-2827
            self.branches["coarser"] += 1
            return neighbor, False
        if self.is_leaf(neighbor):                                         # :2830
            self.branches["same_level"] += 1
            return neighbor, False                                         # :2832
        # neighbor is at a deeper level
        d1 = [opposite(d[0])] + list(d[1:])                                # :2838-2840
        n = self.child_corner(neighbor, d1)                                # :2841
        if n is None:
            self.branches["deeper_child_destroyed"] += 1
            return neighbor, False
        self.branches["deeper"] += 1
        return n, False                                                    # :2842

    def _merge(self, a, b):
        """interpolator_merge, src/fluid.c:2848-2870; an interpolator is [cells, weights]"""
        for c, w in zip(b[0], b[1]):
            j = 0
            while j < len(a[0]) and c is not a[0][j]:                      # :2855-2856
                j += 1
            if j < len(a[0]):
                a[1][j] += w                                               # :2858
            else:
                assert j < INTERPOLATOR_MAX[self.dim]                      # :2860-2864
                a[0].append(c)                                             # :2865-2867
                a[1].append(w)

    @staticmethod
    def _scale(a, b):
        """interpolator_scale, src/fluid.c:2872-2877"""
        for i in range(len(a[1])):
            a[1][i] *= b

    def _t_junction_interpolator(self, cell, d, n):
        """t_junction_interpolator, src/fluid.c:2879-2923"""
        d1 = [opposite(d[0])] + list(d[1:])                                # :2889, :2891 / :2898
        inter = self._interpolator(n, d1)                                  # :2892 / :2899
        if self.dim == 2:
            d1[1] = opposite(d[1])                                         # :2893
            a = self._interpolator(n, d1)                                  # :2894
            self._merge(inter, a)                                          # :2895
            self._scale(inter, 0.5)                                        # :2896
            self.branches["t_junction_2d"] += 1
            return inter
        if self.neighbor_is_brother(cell, d[1]):                           # :2900
            d1[1] = opposite(d[1])                                         # :2901
            self._merge(inter, self._interpolator(n, d1))                  # :2902-2903
            if self.neighbor_is_brother(cell, d[2]):                       # :2904
                d1[2] = opposite(d[2])                                     # :2905
                self._merge(inter, self._interpolator(n, d1))              # :2906-2907
                d1[1] = d[1]                                               # :2908
                self._merge(inter, self._interpolator(n, d1))              # :2909-2910
                self._scale(inter, 0.25)                                   # :2911
                self.branches["t_junction_3d_four"] += 1
            else:
                self._scale(inter, 0.5)                                    # :2914
                self.branches["t_junction_3d_d1"] += 1
        else:
            d1[2] = opposite(d[2])                                         # :2917
            self._merge(inter, self._interpolator(n, d1))                  # :2918-2919
            self._scale(inter, 0.5)                                        # :2920
            self.branches["t_junction_3d_d2"] += 1
        return inter

    def _do_path(self, cell, i, n, d):
        """do_path, src/fluid.c:2925-2981: None, or the interpolator a T-junction gave"""
        dim = self.dim
        for j in range(dim):
            k = PATH[dim][i][j][dim]                                       # :2958
            if n[k] is None:                                               # :2960
                d1 = [opposite(d[-p - 1]) if p < 0 else d[p - 1] for p in PATH[dim][i][j][:dim]]   # :2965-2967
                n[k], t_junction = self._corner_neighbor(cell, d1)         # :2968
                if t_junction:
                    return self._t_junction_interpolator(cell, d1, n[k])   # :2969-2972
                if n[k] is not None:
                    inter = self._do_path(n[k], k, n, d)                   # :2973-2976
                    if inter is not None:
                        return inter
        return None

    def _interpolator(self, cell, d):
        """gfs_cell_corner_interpolator, src/fluid.c:3015-3069, max_level = -1, centered: a fresh
        [cells, weights]"""
        while not self.is_leaf(cell):                                      # :3028-3031
            n0 = self.child_corner(cell, d)
            if n0 is None:
                break
            self.branches["descent_at_top"] += 1
            cell = n0
        n = [None]*self.ncells                                             # :3032-3034
        n[0] = cell
        inter = self._do_path(cell, 0, n, d)                               # :3035
        if inter is not None:                                              # :3036-3037
            return inter
        w = 0.
        boundaries = 0
        ic, iw = [], []
        sizes = set()
        for i in range(self.ncells):                                       # :3045-3054
            if n[i] is not None:
                # distance (), :2983-2992, centered: the size of the cell n[i] itself times the constant
                dist = self.cell_size(n[i])*(0.707106781185 if self.dim == 2 else 0.866025403785)
                a = 1./(dist + 1e-12)                                      # :3048
                ic.append(n[i])
                iw.append(a)
                w += a
                sizes.add(n[i].level)
                if n[i].boundary:                                          # :3052-3053
                    boundaries += 1
        if len(sizes) > 1:
            self.branches["mixed_level_weights"] += 1
        if len(ic) == self.dim + 1 and boundaries == self.dim:             # :3057
            w -= iw[0]                                                     # :3059
            del ic[0], iw[0]                                               # :3060-3064
            self.branches["domain_corner"] += 1
        assert w > 0.                                                      # :3067
        inter = [ic, iw]
        self._scale(inter, 1./w)                                           # :3068
        return inter

    def corner_interpolator(self, cell, d):
        """list of (cell, weight) of the corner d of `cell', computed once (the tree does not change)"""
        key = (id(cell), tuple(d))
        if key not in self._inter:
            ic, iw = self._interpolator(cell, list(d))
            assert len(ic) <= INTERPOLATOR_MAX[self.dim]                   # GfsInterpolator, src/fluid.h
            self._inter[key] = list(zip(ic, iw))
        return self._inter[key]

    # -- values -----------------------------------------------------------------------------------
    def field(self, levels):
        """one array with ghosts per level -> nested lists of Python floats"""
        levels = [a.tolist() if hasattr(a, "tolist") else a for a in levels]
        assert len(levels) == self.level + 1
        for l, a in enumerate(levels):
            assert len(a) == (1 << l) + 2
        return levels

    def value(self, cell, v):
        i, j, k = cell.ijk
        a = v[cell.level]
        return a[j][i] if self.dim == 2 else a[k][j][i]

    # -- particles: what happened, for the tests --------------------------------------------------
    def list_event(self, u, plist, dt, sides):
        """Box.list_event, and in self.record what it did: the levels of the leaves a particle was in
        before and after, the sides particles were put back through or removed at, and how many
        coordinates of the new position were outside"""
        if not hasattr(self, "record"):
            self.record = collections.Counter()
        before = {}
        for p in plist:
            c = self.locate(p.pos)
            before[id(p)] = None if c is None else c.level
        n0 = len(plist)
        moved = []
        plist = self.remove_particles_not_in_domain(plist)                 # particulatecommon.c:987
        self.record["outside_at_start"] += n0 - len(plist)
        for p in plist:
            p.pos_old = list(p.pos)
            p.pos = self.advect_point(u, p.pos, dt)
            nout = sum(abs(p.pos[c]) > 0.5 for c in range(self.dim))
            moved.append((p, nout))
        keep, sent = self.particle_bc(plist, sides)                        # :993
        kept = set(id(p) for p in keep)
        for p, nout in moved:
            if nout == 0:
                c = self.locate(p.pos)
                if c is not None and before[id(p)] is not None and c.level != before[id(p)]:
                    self.record["fine_to_coarse" if c.level < before[id(p)] else "coarse_to_fine"] += 1
                continue
            if nout >= 2:
                self.record["left_through_edge"] += 1
            self.record["wrapped" if id(p) in kept else "removed"] += 1
        return keep, sent

