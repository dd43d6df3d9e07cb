"""tree_forces_reference alone (no GPU): on a tree without a refined patch it is forces_reference on
sampler_reference.Box, bit for bit; on the smallest refined trees every branch of gfs_center_gradient next to a
change of level (src/fluid.c:64-93,171-245,364-396,434-475) is taken; the gradient of a linear field is its
slope; and one coarse-fine gradient in 2-D and one in 3-D equal what the reference's steps give when they are
worked by hand."""
import functools
import sys

import numpy as np
import pytest

import forces_reference as F
import sampler_cases as SC
import sampler_reference as R
import tree_forces_reference as TF
import tree_sampler_cases as TC
import tree_sampler_reference as T

EPS = sys.float_info.epsilon
ALL_FIVE = (F.INERTIAL, F.ADDEDMASS, F.LIFT, F.DRAG, F.BUOY)


def refined_set(dim, refine):
    """the cells with children of the tree GfsRefine `refine' gives: a cell is refined while the level wanted at
    its centre is deeper than its own, then wherever a neighbour (faces, edges and corners) is two levels deeper"""
    refined = set()

    def visit(l, q):
        n = 1 << l
        centre = [(q[c] + 0.5)/n - 0.5 for c in range(dim)]
        if refine(*centre) > l:
            refined.add((l, q))
            for o in np.ndindex(*(2,)*dim):
                visit(l + 1, tuple(2*q[c] + o[c] if c < dim else 0 for c in range(3)))
    visit(0, (0, 0, 0))
    while True:
        more = set()
        for l, q in refined:
            if l < 2:
                continue
            n = 1 << l
            for o in np.ndindex(*(3,)*dim):
                nq = tuple(q[c] + o[c] - 1 if c < dim else 0 for c in range(3))
                if all(0 <= nq[c] < n for c in range(dim)):
                    parent = (l - 1, tuple(x//2 for x in nq))
                    if parent not in refined:
                        more.add(parent)
        if not more:
            return refined
        refined |= more


@functools.lru_cache(None)
def tree(name):
    if name == "ell":
        # level 2 with three of the four cells in the middle refined once: the coarse cell in the notch of the L
        # has refined neighbours on two sides
        cells = {(1, 1, 0), (2, 1, 0), (1, 2, 0)}
        refined = refined_set(2, lambda x, y: 2) | set((2, c) for c in cells)
        return T.TreeBox(2, refined)
    dim, refine = TC.TREES[name][:2]
    return T.TreeBox(dim, refined_set(dim, refine))


def test_trees_have_the_leaves_of_their_description():
    assert collections_of_levels(tree("square")) == {2: 12, 3: 16}
    assert collections_of_levels(tree("graded")) == {2: 12, 3: 12, 4: 16}
    assert collections_of_levels(tree("cube")) == {2: 56, 3: 64}
    assert collections_of_levels(tree("ell")) == {2: 13, 3: 12}


def collections_of_levels(box):
    out = {}
    for c in box.leaves:
        out[c.level] = out.get(c.level, 0) + 1
    return out


def leaf(box, level, ijk):
    return box.by_ijk[(level, ijk)]


def blank_field(box):
    return [np.full(((1 << l) + 2,)*box.dim, np.nan).tolist() for l in range(box.level + 1)]


def field_of(box, fn):
    """a value fn (cell) in every leaf and ghost leaf, NaN in every other cell"""
    v = blank_field(box)
    for c in box.leaves + box.ghosts:
        TF._set_value(box, c, v, float(fn(c)))
    return v


def distinct(salt):
    return lambda c: 0.5 + np.modf(np.sqrt(3. + 7.*(c.ijk[0] + 37.*c.ijk[1] + 1009.*c.ijk[2]) + 1015.*(salt + 31*c.level)))[0]


# -------------------------------------------------------------------------------------------------
# a tree with no refined patch is the box of forces_reference
# -------------------------------------------------------------------------------------------------

def with_coarse_levels(a, level):
    return [np.full(((1 << l) + 2,)*a.ndim, np.nan) for l in range(level)] + [a]


def particulates(dim, level, sides, cls):
    """96 particulates: 32 of the tracers of sampler_cases (built for every outcome at a box side: most of them
    leave, some start outside) and 64 within 0.3 of the centre, which three events of dt = 0.1 h at these
    velocities do not take to a side: most of the list lasts the three events whatever the sides are"""
    pos, ids = SC.tracer_particles(dim, level, "smooth")
    rng = np.random.default_rng(7)
    pick = rng.permutation(len(ids))[:32]
    pick.sort()
    start = [(pos[q].tolist(), int(ids[q])) for q in pick]
    for k in range(64):
        start.append(([rng.uniform(-0.3, 0.3) if c < dim else 0. for c in range(3)], 100000 + k))
    mean, spread = (0.9, 0.5) if sides == "periodic" else (0.3, 0.3)
    out = []
    for p, i in start:
        vel = [mean + rng.uniform(-spread, spread) if c < dim else 0. for c in range(3)]
        volume = 10.**rng.uniform(-6., -4.5)
        out.append(cls(p, i, vel, volume*rng.uniform(0.5, 2.), volume))
    return out


@pytest.mark.parametrize("kinds", [(k,) for k in ALL_FIVE] + [ALL_FIVE, ALL_FIVE[::-1]])
@pytest.mark.parametrize("dim,level,sides", [(2, 3, "periodic"), (3, 2, "closed")])
def test_uniform_tree_equals_forces_reference(dim, level, sides, kinds):
    t, b = T.TreeBox.uniform(dim, level), SC.box(dim, level)
    sd = SC.SIDES[sides]
    u0 = SC.tracer_field(dim, level, "smooth")
    # (with these diameters, 0.012 to 0.039, the response time of the drag, d^2/(18 nu) >= 0.08, stays above dt:
    # the explicit update of the velocity does not run away)
    nu = 1e-4
    g = (0.3, -9.81, 0.7)
    dt = SC.tracer_dt(level)/2.
    forces = [F.ForceCoeff(k) for k in kinds]
    st = F.Sim(t, sd, [with_coarse_levels(a, level) for a in u0], dt, viscosity=(lambda cell: nu, None, None), g=g)
    sb = F.Sim(b, sd, u0, dt, viscosity=(lambda cell: nu, None, None), g=g)
    pt, pb = particulates(dim, level, sides, F.Particulate), particulates(dim, level, sides, F.Particulate)
    n0 = len(pt)
    inside0 = sum(b.locate(p.pos) is not None for p in pb)
    TF.read_forces(st, forces)
    F.read_forces(sb, forces)
    acted = set()
    for e in range(3):
        if st.un is not None:
            for c in range(dim):
                got, want = np.array(st.un[c][level]), np.array(sb.un[c])
                assert np.array_equal(got, want, equal_nan=True)
        # the fluid of the next step: another velocity, so that U - Un is not zero
        ue = [a*(1. + 0.1*(e + 1)) + 0.01*(e + 1) for a in u0]
        st.set_velocity([with_coarse_levels(a, level) for a in ue])
        sb.set_velocity(ue)
        pt = TF.list_event(st, pt, forces)
        pb = F.list_event(sb, pb, forces)
        assert [p.id for p in pt] == [p.id for p in pb]
        for a, c in zip(pt, pb):
            assert (a.pos, a.pos_old, a.vel, a.mass, a.force) == (c.pos, c.pos_old, c.vel, c.mass, c.force)
        if any(any(p.force) for p in pt):
            acted.add(e)
    # the forces act in every event; most of the list lasts the three events; the particles outside from the start
    # are taken off, and in the closed box some more leave
    assert n0 == 96 and len(pt) > n0//2 and acted == {0, 1, 2}
    assert len(pt) < inside0 if sides == "closed" else len(pt) <= inside0


# -------------------------------------------------------------------------------------------------
# the branches next to a change of level
# -------------------------------------------------------------------------------------------------

def census_of(box):
    census = TF.new_census()
    v = field_of(box, distinct(1))
    for c in box.leaves:
        for comp in range(box.dim):
            g = TF.center_gradient(box, c, comp, v, census)
            assert g == g, "a gradient read a cell that is neither a leaf nor a ghost leaf"
    return census


@pytest.mark.parametrize("name", ["square", "graded", "cube"])
def test_every_branch_is_taken(name):
    box = tree(name)
    census = census_of(box)
    S, C, K = TF.SAME_LEAF, TF.CHILDREN, TF.COARSER
    # both neighbours leaves of the level; a coarser neighbour on either side; a neighbour with children on
    # either side
    for pair in ((S, S), (S, K), (K, S), (S, C), (C, S)):
        assert census[("pair",) + pair] > 0, pair
    # a located leaf is a cell of the box: it has a neighbour on both sides (a ghost at a box side)
    assert census["one"] == 0 and census["none"] == 0
    assert census["two"] == len(box.leaves)*box.dim
    # the transverse neighbours of the coarse cell.  On these trees the patch is convex: the coarse cell beside a
    # fine one lies outside the patch in the direction of the face, and so do its transverse neighbours -- leaves of
    # its level (ghost leaves at a box side).  A refined or an absent one is not reachable here (see `ell' below)
    assert census[TF.TRANSVERSE_LEAF] == census[K]*(box.dim - 1) > 0
    assert census[TF.TRANSVERSE_CHILDREN] == 0 and census[TF.TRANSVERSE_ABSENT] == 0
    assert census["children-all-destroyed"] == 0


def test_a_refined_transverse_neighbour_is_reached_in_a_notch():
    census = census_of(tree("ell"))
    assert census[TF.TRANSVERSE_CHILDREN] > 0 and census[TF.TRANSVERSE_LEAF] > 0
    assert census[TF.TRANSVERSE_ABSENT] == 0 and census["one"] == 0 and census["none"] == 0


# -------------------------------------------------------------------------------------------------
# a check that shares nothing with the reference's text: the gradient of a linear field is its slope
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["square", "graded", "cube", "ell", "walls2", "box3"])
def test_gradient_of_a_linear_field_is_its_slope(name):
    """v = a.x + b with a distinct slope per axis, given at the centre of every leaf and, continued, of every ghost
    leaf (so that no stencil meets a condition of a box side).  The three-point formula with x = 3/2 and x = 3/4
    and the transverse interpolations are exact for a linear field; a wrong x or a wrong entry of `perpendicular'
    is not (it is off by a fraction of the slope).

    The bound, from the number format alone.  The slopes and b are multiples of 1/8 and the cell centres are dyadic,
    so every value is exact, and with u = EPS/2 the unit roundoff:
    - a same-level leaf contributes no error; the mean of the children on a face is exact (dyadic values, a
      division by 2 or 4);
    - the value in a coarser neighbour, pa*v (coarse) + pb: a2 = (1/4)/(3/4) is rounded where a transverse
      neighbour has children (u), then a2*p2 (at most 2 u vmax/3 in all, once per transverse direction), pa (u),
      pa*v (coarse) (2 u vmax), the sum (u vmax): less than 4 u vmax = 2 EPS vmax;
    - that value enters the formula with the weight x1^2/(x1 x2 (x1 + x2)) (or the like with x2): 4/15 beside a
      same-level leaf, 1/3 on each side between two coarser neighbours, 3/7 beside a neighbour with children:
      the two sides together at most 2/3 of 2 EPS vmax;
    - the differences, products, the sum and the quotient of the formula act on numbers of the size of
      slope*size: eight roundings at most, 4 EPS |slope| after the division by size.
    Hence |g/size - slope| <= (4/3) EPS vmax/size + 4 EPS |slope|; the test asks for 2 EPS vmax/size + 8 EPS
    |slope|.  On the level-4 leaves that is some 50 ulp of the slope, all of it cancellation in v (coarse) -
    v (cell) of values a thousand times the difference."""
    box = tree(name)
    a, b = (0.75, -1.25, 2.125), 0.375
    v = field_of(box, lambda c: sum(a[k]*c.pos[k] for k in range(box.dim)) + b)
    for c in box.leaves + box.ghosts:       # the values are exact: the sum in another order gives the same number
        assert box.value(c, v) == b + sum(a[k]*c.pos[k] for k in reversed(range(box.dim)))
    vmax = max(abs(box.value(c, v)) for c in box.leaves + box.ghosts)
    levels = set()
    for c in box.leaves:
        size = box.cell_size(c)
        for comp in range(box.dim):
            g = TF.center_gradient(box, c, comp, v)/size
            assert abs(g - a[comp]) <= 2.*EPS*vmax/size + 8.*EPS*abs(a[comp]), (c, comp, g)
        levels.add(c.level)
    assert len(levels) > 1


# -------------------------------------------------------------------------------------------------
# by hand
# -------------------------------------------------------------------------------------------------

def test_coarse_fine_gradient_2d_by_hand():
    """`square': the leaf of level 3 with index (6, 5) -- q = (5, 4), the last column of the patch, the lower half
    of the coarse row beside it.  Its FTT_CELL_ID is 3 (+x, -y: coords[3] = {1, -1}, src/ftt.c:301-316).  Along x:
    f1.neighbor is the leaf (5, 5) of its level; f2.neighbor is the leaf (4, 3) of level 2, coarser:
    perpendicular[FTT_RIGHT][3] = 3 = FTT_BOTTOM (src/fluid.c:266), interpolate_1D1 (coarse, FTT_BOTTOM, 1/4) looks
    at the leaf (4, 2) of level 2: p = { 1 - 1/4, 1/4*v (4, 2) } (:176-186), x2 = 3/2 (:393)."""
    box = tree("square")
    v = field_of(box, distinct(2))
    cell = leaf(box, 3, (6, 5, 0))
    assert cell.id == 3 and cell.q == (5, 4, 0)
    v0, v1 = box.value(cell, v), box.value(leaf(box, 3, (5, 5, 0)), v)
    coarse, below = leaf(box, 2, (4, 3, 0)), leaf(box, 2, (4, 2, 0))
    assert box.neighbor(cell, R.FTT_RIGHT) is coarse and box.neighbor(coarse, R.FTT_BOTTOM) is below
    a2 = (1./4.)/1.
    pa, pb = 1. - a2, 0. + a2*box.value(below, v)
    v2 = pa*box.value(coarse, v) + pb
    x1, x2 = 1., 3./2.
    want = (x1*x1*(v2 - v0) + x2*x2*(v0 - v1))/(x1*x2*(x2 + x1))
    assert TF.center_gradient(box, cell, 0, v) == want
    # along y both neighbours are leaves of the patch
    up, down = leaf(box, 3, (6, 6, 0)), leaf(box, 3, (6, 4, 0))
    assert TF.center_gradient(box, cell, 1, v) == ((box.value(up, v) - v0) + (v0 - box.value(down, v)))/2.
    # and the coarse leaf sees the mean of the two children on the face, at x = 3/4 (:75-88)
    kids = [leaf(box, 3, (6, 5, 0)), leaf(box, 3, (6, 6, 0))]
    assert [k.id for k in kids] == [3, 1]                   # index[FTT_RIGHT] = {1, 3}, src/ftt.h:330
    av = (0. + 1.*box.value(kids[1], v) + 1.*box.value(kids[0], v))/2.
    ghost = box.neighbor(coarse, R.FTT_RIGHT)              # the coarse leaf is in the last column of the box
    assert ghost.boundary and ghost.level == 2 and ghost.ijk == (5, 3, 0)
    c0, right = box.value(coarse, v), box.value(ghost, v)
    x1, x2 = 3./4., 1.
    assert TF.center_gradient(box, coarse, 0, v) == (x1*x1*(right - c0) + x2*x2*(c0 - av))/(x1*x2*(x2 + x1))


def test_coarse_fine_gradient_3d_by_hand():
    """`cube': the leaf of level 3 with q = (5, 4, 4), FTT_CELL_ID 7 (+x, -y, -z).  Along x the coarse leaf q =
    (3, 2, 2) of level 2: perpendicular[FTT_RIGHT][7] = {3, 5} = FTT_BOTTOM, FTT_BACK (src/fluid.c:272);
    interpolate_2D1 takes d1 = FTT_BOTTOM first (:222-231), then d2 = FTT_BACK (:233-242)."""
    box = tree("cube")
    v = field_of(box, distinct(3))
    cell = leaf(box, 3, (6, 5, 5))
    assert cell.id == 7 and cell.q == (5, 4, 4)
    v0, v1 = box.value(cell, v), box.value(leaf(box, 3, (5, 5, 5)), v)
    coarse = leaf(box, 2, (4, 3, 3))
    below, behind = leaf(box, 2, (4, 2, 3)), leaf(box, 2, (4, 3, 2))
    assert box.neighbor(cell, R.FTT_RIGHT) is coarse
    assert box.neighbor(coarse, R.FTT_BOTTOM) is below and box.neighbor(coarse, R.FTT_BACK) is behind
    pa, pb = 1., 0.
    a1 = (1./4.)/1.
    pb += a1*box.value(below, v)
    pa -= a1
    a2 = (1./4.)/1.
    pb += a2*box.value(behind, v)
    pa -= a2
    v2 = pa*box.value(coarse, v) + pb
    x1, x2 = 1., 3./2.
    assert TF.center_gradient(box, cell, 0, v) == (x1*x1*(v2 - v0) + x2*x2*(v0 - v1))/(x1*x2*(x2 + x1))
