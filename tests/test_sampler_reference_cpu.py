"""The restatement of the reference's point sampler and particle walk on an explicit cell graph
(tests/sampler_reference.py): checked on its own, then the oracle (oracle/go_particles.c) against it
by array_equal on the case matrix of tests/sampler_cases.py.  The device is compared with the same
references in test_gpu_sampler_reference.py."""
import collections
import ctypes as C
import math

import numpy as np
import pytest

import sampler_cases as K
import sampler_reference as R
from oracle import oracle as O


def _touching(cell, n, dim):
    return sum(cell.ijk[a] in (1, n) for a in range(dim))


# -------------------------------------------------------------------------------------------------
# the cell graph
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_cell_graph_of_one_box(dim, level):
    """interior cells linked to each other; one tree of ghosts per side, every ghost flagged, linked
    to the interior cell next to it and to the ghosts of its own tree, to nothing across a box edge
    and to nothing away from the box"""
    b = K.box(dim, level)
    n = b.n
    assert len(b.leaves) == n**dim and len(b.ghosts) == 2*dim*n**(dim - 1)
    assert not any(c.boundary for c in b.leaves) and all(c.boundary for c in b.ghosts)
    for c in b.leaves:
        assert c.pos[:dim] == tuple(-0.5 + (c.ijk[a] - 0.5)/n for a in range(dim))
        for d in range(2*dim):
            nb = b.neighbor(c, d)
            want = list(c.ijk)
            want[d//2] += 1 if d % 2 == 0 else -1
            assert nb is not None and nb.ijk == tuple(want)
            assert (nb.tree == d) if not 1 <= want[d//2] <= n else (nb.tree is None)
            assert b.neighbor(nb, R.opposite(d)) is c
    for g in b.ghosts:
        side = g.tree
        for d in range(2*dim):
            nb = b.neighbor(g, d)
            want = list(g.ijk)
            want[d//2] += 1 if d % 2 == 0 else -1
            if d == R.opposite(side):
                assert nb is b.by_ijk[tuple(want)]          # the box
            elif d == side:
                assert nb is None                           # flattened away
            elif 1 <= want[d//2] <= n:
                assert nb.tree == side and nb.ijk == tuple(want)
            else:
                assert nb is None                           # across a box edge


# the cells of each corner interpolator, as they follow from the walk of do_path on that graph
# ("The cell graph of one box and the corner interpolators"), at level 2 (n = 4), for one
# cell of every class and every corner direction of src/fluid.c:2588-2605.  Cells are numbered as
# n[] of the reference: bit 0 the step along d[0] (x), bit 1 along d[1] (y), bit 2 along d[2] (z).
# Per corner: the numbers that are NOT in the interpolator, then whether cell 0 is removed.
FULL = ((), False)
MEMBERSHIP = {
    # 2-D ----------------------------------------------------------------------------------------
    (2, (2, 2, 0)): [FULL, FULL, FULL, FULL],                                 # touches no side
    (2, (4, 2, 0)): [FULL, FULL, FULL, FULL],                                 # +x: ghosts 1, 3 exist
    (2, (4, 4, 0)): [FULL, FULL, ((3,), True), FULL],                         # +x and +y: box corner
    # 3-D ----------------------------------------------------------------------------------------
    (3, (2, 2, 2)): [FULL]*8,
    (3, (4, 2, 2)): [FULL]*8,
    (3, (4, 4, 2)): [FULL, FULL, ((3, 7), False), FULL,                       # box edge +x+y
                     FULL, FULL, ((3, 7), False), FULL],
    (3, (4, 4, 4)): [FULL, ((5, 7), False), ((3, 5, 6, 7), True), ((6, 7), False),   # box corner +x+y+z
                     FULL, FULL, ((3, 7), False), FULL],
}


@pytest.mark.parametrize("dim,ijk", sorted(MEMBERSHIP))
def test_corner_interpolator_membership_by_cell_class(dim, ijk):
    b = K.box(dim, 2)
    cell = b.by_ijk[ijk]
    for ic, d in enumerate(R.CORNER[dim]):
        absent, drop0 = MEMBERSHIP[(dim, ijk)][ic]
        want = []
        for m in range(1 << dim):
            if m in absent or (drop0 and m == 0):
                continue
            c = list(ijk)
            for a in range(dim):
                if m & (1 << a):
                    c[a] += 1 if d[a] % 2 == 0 else -1
            want.append(tuple(c))
        inter = b.corner_interpolator(cell, d)
        assert [c.ijk for c, w in inter] == want, (ijk, ic)
        assert all(w == inter[0][1] for c, w in inter)
        assert abs(sum(w for c, w in inter) - 1.) <= 4*2.**-53


@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_membership_coincides_with_at_most_one_ghost_coordinate(dim, level):
    """the finding recorded in DESIGN.md: on a uniform box the walk reaches exactly the cells of the
    2^dim block with at most one coordinate in the ghost layer, every one of them a boundary cell
    iff it has one -- the index shortcut of the oracle and of the device"""
    b = K.box(dim, level)
    n = b.n
    for cell in b.leaves:
        for d in R.CORNER[dim]:
            got = b.corner_cells(cell, d)
            for m in range(1 << dim):
                c, out = list(cell.ijk), 0
                for a in range(dim):
                    if m & (1 << a):
                        c[a] += 1 if d[a] % 2 == 0 else -1
                        out += not 1 <= c[a] <= n
                if out <= 1:
                    assert got[m].ijk == tuple(c) and got[m].boundary == (out == 1)
                else:
                    assert got[m] is None


# -------------------------------------------------------------------------------------------------
# the restatement on its own
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [2, 3])
def test_linear_field_reproduced_at_interior_points(dim):
    level = 3
    b = K.box(dim, level)
    n = b.n
    c = -0.5 + (np.arange(n + 2) - 0.5)/n
    co = (1.25, 2., -3., 0.5)
    if dim == 2:
        a = co[0] + co[1]*c[None, :] + co[2]*c[:, None]
    else:
        a = co[0] + co[1]*c[None, None, :] + co[2]*c[None, :, None] + co[3]*c[:, None, None]
    v = b.field(a)
    rng = np.random.default_rng(7)
    worst = 0.
    for p in rng.uniform(-0.5, 0.5, (400, dim)).tolist():
        p = p + [0.]*(3 - dim)
        cell = b.locate(p)
        if _touching(cell, n, dim):
            continue                       # cells at a side lose the corner ghosts: not linear there
        exact = co[0] + co[1]*p[0] + co[2]*p[1] + (co[3]*p[2] if dim == 3 else 0.)
        worst = max(worst, abs(b.interpolate(cell, p, v) - exact))
    print("linear field, worst error", worst)
    assert worst <= 1e-15


@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_constant_field_reproduced_in_every_cell_class(dim, level):
    """What depends on the class of a cell (touching 0, 1, 2 or 3 box sides) is the set of cells of
    each corner and hence the weights: they must sum to one, and the coefficients of the polynomial
    must then cancel.  The constant is 1: every product weight*value is exact, so the 2 ulp are those
    of the weights and of the sums alone.  The same bound holds for the corner values of a constant
    with a full mantissa (pi); through the 3-D polynomial (src/fluid.c:2669-2681: seven differences
    of eight corner values each, all multiplied by +-1 at a corner of the cell) such a constant comes
    back within 3 ulp, measured at level 1, 2 ulp at levels 2 and 3: printed, not asserted."""
    b = K.box(dim, level)
    n = b.n
    edge = K.ghost_count(dim, level) >= 2
    one = np.full((n + 2,)*dim, 1.)
    one[edge] = np.nan
    full = np.full((n + 2,)*dim, math.pi)
    full[edge] = np.nan
    v1, vpi = b.field(one), b.field(full)
    classes = collections.Counter()
    worst_pi = 0.
    for p in K.sample_points(dim, level).tolist():
        cell = b.locate(p)
        if cell is None:
            continue
        classes[_touching(cell, n, dim)] += 1
        assert abs(b.interpolate(cell, p, v1) - 1.) <= 2*math.ulp(1.), (cell, p)
        worst_pi = max(worst_pi, abs(b.interpolate(cell, p, vpi) - math.pi)/math.ulp(math.pi))
    for cell in b.leaves:
        for f in b.corner_values(cell, vpi):
            assert abs(f - math.pi) <= 2*math.ulp(math.pi), cell
    print("constant pi through the whole formula: worst %.1f ulp" % worst_pi)
    assert set(classes) == ({dim} if level == 1 else set(range(dim + 1)))


def test_locate_tie_rule_and_box_bounds():
    b = K.box(3, 3)
    h = 1./8
    assert b.locate([0., 0., 0.]).ijk == (4, 4, 4)          # strict '>': a face belongs to the lower cell
    assert b.locate([h, 0., -h]).ijk == (5, 4, 3)
    assert b.locate([0.5, 0.5, 0.5]).ijk == (8, 8, 8)        # the box bounds are inclusive
    assert b.locate([-0.5, -0.5, -0.5]).ijk == (1, 1, 1)
    assert b.locate([math.nextafter(0.5, 1.), 0., 0.]) is None
    assert b.locate([0., math.nextafter(-0.5, -1.), 0.]) is None


@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_nodata_branches_of_the_restatement(dim, level):
    """src/fluid.c:2704-2705: GFS_NODATA in the cell is returned as it is; :3096-3097: a corner that
    sees GFS_NODATA takes the value of the cell"""
    b = K.box(dim, level)
    v = b.field(K.sampler_field(dim, level, "nodata"))
    first = b.by_ijk[(1, 1, 1 if dim == 3 else 0)]
    assert b.interpolate(first, list(first.pos), v) == R.GFS_NODATA
    out, inside = K.reference_sample(dim, level, "nodata", True)
    ordinary, _ = K.reference_sample(dim, level, "distinct")
    assert np.all(np.isfinite(out))
    changed = out != ordinary
    assert 0 < changed.sum() < inside.sum()
    # away from the two cells every value is the one of the field without GFS_NODATA
    assert np.all(np.abs(out[~changed & inside]) < 2.)


def test_check_intersetion_raises_where_the_reference_is_undefined():
    b = K.box(2, 2)
    with pytest.raises(R.IntersectionFailed):
        b.check_intersetion((0.125, 0.125, 0.), [0.1, 0.1, 0.], [0.1, 0.1, 0.], 0.25)


def test_distinct_fill_is_distinct():
    for dim, level in K.DIMS_LEVELS:
        a = K.distinct_field(dim, level)
        vals = a[~np.isnan(a)]
        assert len(np.unique(vals)) == len(vals) == (1 << level)**dim + 2*dim*(1 << level)**(dim - 1)


@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_sample_points_cover_what_they_are_built_for(dim, level):
    pts = K.sample_points(dim, level)
    out, inside = K.reference_sample(dim, level, "distinct")
    n = 1 << level
    assert (~inside).sum() == 2*dim*5
    assert np.all(np.abs(pts[~inside, :dim]).max(axis=1) > 0.5)
    assert not np.isnan(out).any()             # no edge or corner ghost is ever read
    onside = (np.abs(pts[:, :dim]) == 0.5).any(axis=1)
    assert inside[onside & (np.abs(pts[:, :dim]).max(axis=1) <= 0.5)].all() and onside.sum() >= 4*n
    assert len(pts) <= 7000


# -------------------------------------------------------------------------------------------------
# the reference is defined on every case of the GPU tests
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_restatement_raises_on_none_of_the_tracer_cases_and_outcomes_are_covered(dim, level):
    for field in K.TRACER_FIELDS:
        outcomes = collections.Counter(K.first_event_outcomes(dim, level, field))
        for kind in ["inside", "stuck", "removed"] + ["out%d" % k for k in range(1, dim + 1)]:
            assert outcomes[kind] >= 2, (field, kind, outcomes)
        for sides in K.SIDES:
            states = K.reference_events(dim, level, sides, field)      # raises IntersectionFailed if undefined
            assert len(states) == K.NEVENTS
            assert len(states[-1][2]) > 0
    # a path that leaves a periodic box through an edge is wrapped along one axis only and is gone
    # after the next event
    p1, _, i1 = K.reference_events(dim, level, "periodic", "smooth")[0]
    still_out = i1[(np.abs(p1[:, :dim]) > 0.5).any(axis=1)]
    assert len(still_out) >= 2
    assert not np.isin(still_out, K.reference_events(dim, level, "periodic", "smooth")[1][2]).any()


# -------------------------------------------------------------------------------------------------
# the oracle against the restatement
# -------------------------------------------------------------------------------------------------

def _oracle_sample(dom, a, pts):
    L = O.lib()
    pd = C.POINTER(C.c_double)
    L.go_locate.restype, L.go_locate.argtypes = C.c_int, [C.c_void_p, pd, C.POINTER(C.c_int)]
    L.go_interpolate.restype = C.c_double
    L.go_interpolate.argtypes = [C.c_void_p, pd, C.POINTER(C.c_int), pd]
    f = dom.field()
    f.leaf()[...] = a
    v = L.go_field_level(f.ptr, dom.depth)
    out, inside, cells = np.zeros(len(pts)), np.zeros(len(pts), dtype=bool), []
    for q, p in enumerate(pts):
        p = np.ascontiguousarray(p)
        ijk = (C.c_int*3)()
        if L.go_locate(dom.ptr, p.ctypes.data_as(pd), ijk):
            inside[q] = True
            out[q] = L.go_interpolate(dom.ptr, v, ijk, p.ctypes.data_as(pd))
            cells.append(tuple(ijk))
        else:
            cells.append(None)
    return out, inside, cells


@pytest.mark.parametrize("variant", K.SAMPLER_VARIANTS)
@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_oracle_locate_and_interpolate_equal_the_restatement(dim, level, variant):
    pts = K.sample_points(dim, level)
    a = K.sampler_field(dim, level, variant)
    sides = K.bc_case(dim, level, variant[3:])[0] if variant.startswith("bc_") else None
    dom = O.Domain(dim, level, sides)
    if variant.startswith("bc_"):
        # the ghosts are those of the oracle's own boundary conditions
        _, interior, vals, expect = K.bc_case(dim, level, variant[3:])
        f = dom.field()
        f.leaf()[...] = np.nan
        f.interior()[...] = interior
        for d, (kind, val) in vals.items():
            f.set_bc(d, kind, val)
        O.lib().go_bc(f.ptr, f.ptr, level)
        a = f.leaf().copy()
        assert K.face_ghosts_equal(dim, level, a, expect)
    out, inside, cells = _oracle_sample(dom, a, pts)
    ref, ref_inside = K.reference_sample(dim, level, variant)
    b = K.box(dim, level)
    assert np.array_equal(inside, ref_inside)
    assert cells == [c.ijk if c is not None else None for c in map(b.locate, pts.tolist())]
    assert np.array_equal(out, ref, equal_nan=True)
    if variant != "nodata":
        assert not np.isnan(out).any()


@pytest.mark.parametrize("sides", sorted(K.SIDES))
@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_oracle_list_event_equals_the_restatement(dim, level, sides):
    for field in K.TRACER_FIELDS:
        s = O.Sim(dim, level, K.SIDES[sides])
        for c, a in enumerate(K.tracer_field(dim, level, field)):
            s.u[c].leaf()[...] = a
        s.advection_params.dt = K.tracer_dt(level)
        pos, ids = K.tracer_particles(dim, level, field)
        pl = O.Particles(s, pos, ids)
        for k, (rp, rpo, ri) in enumerate(K.reference_events(dim, level, sides, field)):
            pl.event()
            pl.clear_outbox()
            op, oi = pl.state()
            n = len(oi)
            old = np.ctypeslib.as_array(pl.pos_old_ptr(), shape=(max(n, 1), 3))[:n]
            assert np.array_equal(oi, ri), (field, k)
            assert np.array_equal(op, rp), (field, k)
            assert np.array_equal(old, rpo), (field, k)
