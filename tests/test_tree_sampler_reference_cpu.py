"""tree_sampler_reference.TreeBox alone (no GPU): on a tree without a refined patch it is
sampler_reference.Box, bit for bit; on the smallest refined trees every branch of the reference's walk
around a corner (src/fluid.c:2813-3069) is taken, the weights sum to one, and two T-junction corners
equal what the reference's steps give when they are worked by hand."""
import functools
import sys

import numpy as np
import pytest

import sampler_cases as SC
import sampler_reference as R
import tree_sampler_reference as T

EPS = sys.float_info.epsilon
L, Rt, Bo, To, Fr, Ba = R.FTT_LEFT, R.FTT_RIGHT, R.FTT_BOTTOM, R.FTT_TOP, R.FTT_FRONT, R.FTT_BACK


def patch_refined(dim, base, cells):
    """the refined set of a box uniform to level `base' whose level-`base' cells `cells' have children"""
    refined = set()
    for l in range(base):
        n = 1 << l
        for k in range(n if dim == 3 else 1):
            for j in range(n):
                for i in range(n):
                    refined.add((l, (i, j, k)))
    refined.update((base, c) for c in cells)
    return refined


@functools.lru_cache(None)
def square_patch():
    """2-D, level 2 with the 2 x 2 cells in the middle refined once: 12 + 16 = 28 leaves"""
    return T.TreeBox(2, patch_refined(2, 2, [(i, j, 0) for i in (1, 2) for j in (1, 2)]))


@functools.lru_cache(None)
def cube_patch():
    """3-D, level 2 with the 2 x 2 x 2 cells in the middle refined once: 56 + 64 = 120 leaves"""
    return T.TreeBox(3, patch_refined(3, 2, [(i, j, k) for i in (1, 2) for j in (1, 2) for k in (1, 2)]))


def all_interpolators(box):
    """every corner of every leaf: {(level, ijk, d): [((level, ijk), weight)]}; nothing is skipped"""
    out = {}
    for c in box.leaves:
        for d in R.CORNER[box.dim]:
            out[(c.level, c.ijk, d)] = [((x.level, x.ijk), w) for x, w in box.corner_interpolator(c, d)]
    assert len(out) == len(box.leaves)*(1 << box.dim)
    return out


def leaf(box, level, ijk):
    return box.by_ijk[(level, ijk)]


def with_coarse_levels(a, level):
    """the per-level arrays of a TreeBox from the array of the leaf level (the other levels hold no leaf)"""
    dim = a.ndim
    return [np.full(((1 << l) + 2,)*dim, np.nan) for l in range(level)] + [a]


# -------------------------------------------------------------------------------------------------
# a tree with no refined patch is the box of sampler_reference
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,level", [(2, 0), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2)])
def test_uniform_tree_interpolators_equal_box(dim, level):
    t, b = T.TreeBox.uniform(dim, level), R.Box(dim, level)
    assert [c.ijk for c in t.leaves] == [c.ijk for c in b.leaves]
    assert [(c.ijk, c.tree) for c in t.ghosts] == [(c.ijk, c.tree) for c in b.ghosts]
    for c, cb in zip(t.leaves, b.leaves):
        assert c.pos == cb.pos
        for d in R.CORNER[dim]:
            assert [(x.ijk, x.tree, w) for x, w in t.corner_interpolator(c, d)] == \
                [(x.ijk, x.tree, w) for x, w in b.corner_interpolator(cb, d)]
    for k in ("coarser", "coarser_t_junction", "deeper", "deeper_child_destroyed", "mixed_level_weights",
              "t_junction_2d", "t_junction_3d_d1", "t_junction_3d_d2", "t_junction_3d_four", "descent_at_top"):
        assert t.branches[k] == 0, k


@pytest.mark.parametrize("dim,level", [(2, 1), (2, 3), (3, 2)])
def test_uniform_tree_samples_equal_box(dim, level):
    t = T.TreeBox.uniform(dim, level)
    a = SC.sampler_field(dim, level, "distinct")
    out, inside = t.sample(t.field(with_coarse_levels(a, level)), SC.sample_points(dim, level).tolist(), nodata=False)
    ref_out, ref_inside = SC.reference_sample(dim, level, "distinct")
    assert np.array_equal(np.array(inside, dtype=bool), ref_inside)
    assert np.array_equal(np.array(out), ref_out)


@pytest.mark.parametrize("dim,level,sides", [(2, 2, "periodic"), (2, 3, "closed"), (3, 2, "periodic"), (3, 2, "closed")])
def test_uniform_tree_tracer_events_equal_box(dim, level, sides):
    t = T.TreeBox.uniform(dim, level)
    pos, ids = SC.tracer_particles(dim, level, "smooth")
    u = [t.field(with_coarse_levels(a, level)) for a in SC.tracer_field(dim, level, "smooth")]
    plist = [R.Particle(p, i) for p, i in zip(pos.tolist(), ids.tolist())]
    ref = SC.reference_events(dim, level, sides, "smooth")
    for e in range(SC.NEVENTS):
        plist, sent = t.list_event(u, plist, SC.tracer_dt(level), SC.SIDES[sides])
        assert not sent
        p, po, i = ref[e]
        assert np.array_equal(np.array([q.pos for q in plist]).reshape(-1, 3), p)
        assert np.array_equal(np.array([q.pos_old for q in plist]).reshape(-1, 3), po)
        assert [q.id for q in plist] == i.tolist()
    assert t.record["wrapped" if sides == "periodic" else "removed"] > 0


# -------------------------------------------------------------------------------------------------
# the smallest refined trees
# -------------------------------------------------------------------------------------------------

def test_square_patch_takes_every_branch():
    b = square_patch()
    assert len(b.leaves) == 28
    inter = all_interpolators(b)
    for k in ("same_level", "coarser", "coarser_t_junction", "deeper", "t_junction_2d", "mixed_level_weights",
              "domain_corner"):
        assert b.branches[k] > 0, k
    assert b.branches["deeper_child_destroyed"] == 0      # never reached (the fallback of src/fluid.c:2842)
    assert max(len(v) for v in inter.values()) == 7       # the capacity of a GfsInterpolator in 2-D


def test_cube_patch_takes_every_branch():
    b = cube_patch()
    assert len(b.leaves) == 120
    inter = all_interpolators(b)
    for k in ("same_level", "coarser", "coarser_t_junction", "deeper", "t_junction_3d_d1", "t_junction_3d_d2",
              "t_junction_3d_four", "mixed_level_weights", "domain_corner"):
        assert b.branches[k] > 0, k
    assert b.branches["deeper_child_destroyed"] == 0
    assert b.branches["t_junction_2d"] == 0
    assert max(len(v) for v in inter.values()) == 23      # below the 29 of a GfsInterpolator in 3-D


@pytest.mark.parametrize("tree", [square_patch, cube_patch])
def test_weights_sum_to_one(tree):
    b = tree()
    for key, row in all_interpolators(b).items():
        s = 0.
        for _, w in row:
            assert w > 0.
            s += w
        assert abs(s - 1.) <= 4.*EPS, (key, s)
        assert len(set(c for c, _ in row)) == len(row), key       # interpolator_merge: no cell twice


@pytest.mark.parametrize("tree", [square_patch, cube_patch])
def test_flags_and_ghost_trees(tree):
    """the boundary trees are refined like the box cells they touch (match, src/boundary.c:638-642) and
    keep the half of every oct next to the box (ftt_cell_flatten)"""
    b = tree()
    f2, f3 = np.array(b.flags(2)), np.array(b.flags(3))
    n2, n3 = 4, 8
    assert (f2[(slice(1, n2 + 1),)*b.dim] != T.NONE).all()
    assert int((f2 == T.NODE).sum()) == 1 << b.dim           # the patch touches no side: no ghost has children
    assert int((f3 == T.LEAF).sum()) == 1 << (2*b.dim)
    assert int((f2 == T.LEAF).sum()) == n2**b.dim - (1 << b.dim) + 2*b.dim*n2**(b.dim - 1)
    assert (f3[(0,)*b.dim] == T.NONE) and (f2[(0,)*b.dim] == T.NONE)      # no edge or corner ghosts


def test_locate_at_the_level_boundaries():
    """the strict `>' of the descent (src/ftt.c:1559-1563): a point on a face belongs to the cell below"""
    b = square_patch()
    assert b.locate([-0.25, -0.25, 0.]).ijk == (1, 1, 0) and b.locate([-0.25, -0.25, 0.]).level == 2
    up = float(np.nextafter(-0.25, 1.))
    c = b.locate([up, up, 0.])
    assert (c.level, c.ijk) == (3, (3, 3, 0))
    c = b.locate([0.25, 0.25, 0.])
    assert (c.level, c.ijk) == (3, (6, 6, 0))
    c = b.locate([float(np.nextafter(0.25, 1.)), 0.25, 0.])
    assert (c.level, c.ijk) == (2, (4, 3, 0))
    assert b.locate([0.5, 0.5, 0.]).ijk == (4, 4, 0)
    assert b.locate([float(np.nextafter(0.5, 1.)), 0., 0.]) is None


# -------------------------------------------------------------------------------------------------
# two T-junction corners by hand
# -------------------------------------------------------------------------------------------------

def test_t_junction_2d_by_hand():
    """Level-3 cell (3, 3) is the bottom-left cell of the patch; its corner (right, bottom) is the middle of
    the top face of the level-2 cell (2, 1): a hanging node.

    do_path: n[1] = (4, 3) (right, same level); from there path {2,-1,3}, d1 = (bottom, left): the neighbour
    is the coarser (2, 1) and ftt_cell_child_corner (parent, (bottom, left)) = (3, 3) != (4, 3): T-junction
    (src/fluid.c:2823-2827).  t_junction_interpolator (:2889-2896) with n = the level-2 cell (2, 1):
      A = its corner (top, left): n[] = [(2,1), L3 (3,3) (deeper, :2841), (1,1), (1,2)], weights a2, a3, a2, a2
      B = its corner (top, right): n[] = [(2,1), L3 (4,3), (3,1), L3 (5,3)], weights a2, a3, a2, a3
    each scaled by the reciprocal of its sum (:3068), B merged into A (:2848-2870), then times 0.5."""
    b = square_patch()
    a2 = 1./(0.25*0.707106781185 + 1e-12)
    a3 = 1./(0.125*0.707106781185 + 1e-12)
    sa = 1./(0. + a2 + a3 + a2 + a2)
    sb = 1./(0. + a2 + a3 + a2 + a3)
    expected = [((2, (2, 1, 0)), (a2*sa + a2*sb)*0.5),
                ((3, (3, 3, 0)), a3*sa*0.5),
                ((2, (1, 1, 0)), a2*sa*0.5),
                ((2, (1, 2, 0)), a2*sa*0.5),
                ((3, (4, 3, 0)), a3*sb*0.5),
                ((2, (3, 1, 0)), a2*sb*0.5),
                ((3, (5, 3, 0)), a3*sb*0.5)]
    got = [((x.level, x.ijk), w) for x, w in b.corner_interpolator(leaf(b, 3, (3, 3, 0)), (Rt, Bo))]
    assert got == expected


def test_t_junction_3d_by_hand():
    """Level-3 cell (3, 3, 3) is the corner cell of the cube; its corner (left, bottom, front) lies on the edge
    x = -0.25, y = -0.25 of the cube, half a coarse cell up: a hanging node.

    do_path: path {1,2,3,1}, d1 = (left, bottom, front): the neighbour is the coarser level-2 cell (1, 2, 2) and
    the child of the parent in the corner (left, bottom, front) is (3, 3, 4), not (3, 3, 3): T-junction.
    ftt_cell_neighbor_is_brother ((3,3,3), bottom) is false (id 2: b = {1,0,1,0,0,1}), so :2916-2920: the corners
    (right, bottom, front) and (right, bottom, back) of n = (1, 2, 2), merged, times 0.5.
      A: n[] = [(1,2,2), L3 (3,3,4), (1,1,2), (2,1,2), (1,2,3), L3 (3,3,5), (1,1,3), (2,1,3)]
      B: n[] = [(1,2,2), L3 (3,3,3), (1,1,2), (2,1,2), (1,2,1), (2,2,1), (1,1,1), (2,1,1)]"""
    b = cube_patch()
    a2 = 1./(0.25*0.866025403785 + 1e-12)
    a3 = 1./(0.125*0.866025403785 + 1e-12)
    sa = 1./(0. + a2 + a3 + a2 + a2 + a2 + a3 + a2 + a2)
    sb = 1./(0. + a2 + a3 + a2 + a2 + a2 + a2 + a2 + a2)
    expected = [((2, (1, 2, 2)), (a2*sa + a2*sb)*0.5),
                ((3, (3, 3, 4)), a3*sa*0.5),
                ((2, (1, 1, 2)), (a2*sa + a2*sb)*0.5),
                ((2, (2, 1, 2)), (a2*sa + a2*sb)*0.5),
                ((2, (1, 2, 3)), a2*sa*0.5),
                ((3, (3, 3, 5)), a3*sa*0.5),
                ((2, (1, 1, 3)), a2*sa*0.5),
                ((2, (2, 1, 3)), a2*sa*0.5),
                ((3, (3, 3, 3)), a3*sb*0.5),
                ((2, (1, 2, 1)), a2*sb*0.5),
                ((2, (2, 2, 1)), a2*sb*0.5),
                ((2, (1, 1, 1)), a2*sb*0.5),
                ((2, (2, 1, 1)), a2*sb*0.5)]
    got = [((x.level, x.ijk), w) for x, w in b.corner_interpolator(leaf(b, 3, (3, 3, 3)), (L, Bo, Fr))]
    assert got == expected


def test_interpolation_reproduces_a_constant_and_is_continuous_across_a_level_change():
    """weights that sum to one give back a constant; at a point on the face between a coarse and a fine leaf the
    values interpolated from either side agree to rounding where the face is conforming (the corner values of the
    fine cell at a hanging node are, by t_junction_interpolator, the mean of the coarse cell's corner values)"""
    b = square_patch()
    const = b.field([np.full(((1 << l) + 2,)*2, 3.25) for l in range(4)])
    rng = np.random.default_rng(7)
    for p in rng.uniform(-0.5, 0.5, (64, 2)).tolist():
        c = b.locate(p + [0.])
        assert abs(b.interpolate(c, p + [0.], const, nodata=False) - 3.25) <= 8.*EPS*3.25
    vals = b.field([rng.uniform(0.5, 1.5, ((1 << l) + 2,)*2) for l in range(4)])
    coarse, fine = leaf(b, 2, (1, 2, 0)), leaf(b, 3, (3, 3, 0))
    for y in (-0.25, -0.1875, -0.125):        # the corners of the fine cell on the shared face x = -0.25
        p = [-0.25, y, 0.]
        vc = b.interpolate(coarse, p, vals, nodata=False)
        vf = b.interpolate(fine, p, vals, nodata=False)
        assert abs(vc - vf) <= 16.*EPS, (y, vc, vf)
