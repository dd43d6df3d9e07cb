"""tree_two_way_reference alone (no GPU): on a uniform tree it is two_way_reference on the box, bit for bit; the
fixtures of the GPU tests reach what they are meant to reach; the constant kernel spreads every force exactly; and
the two premises of the time-step tests of tests/test_gpu_tree_two_way.py -- the MAC value of a constant field is
that constant on the trees used there, and a constant GfsSource along the invariant axis of a striped tree gives
U == dt*g exactly in the oracle."""
import numpy as np
import pytest

import sampler_reference as R
import tree_sampler_cases as TC
import tree_sampler_reference as T
import tree_two_way_cases as C
import tree_two_way_reference as TW
import two_way_reference as U


def interior(a, dim):
    return np.array(a)[(slice(1, -1),)*dim]


# -------------------------------------------------------------------------------------------------
# a tree without a refined patch is the box of two_way_reference
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,level", [(2, 4), (3, 3)])
def test_uniform_tree_is_the_uniform_box(dim, level):
    box = T.TreeBox.uniform(dim, level)
    h = 1./(1 << level)
    rng = np.random.default_rng(10 + dim)
    n = 60
    pos = np.zeros((n, 3))
    pos[:, :dim] = rng.uniform(-0.5, 0.5, (n, dim))
    pos[:6, :dim] = pos[6:12, :dim]              # several particles per cell
    pos[12, 0] = 0.5                             # on a side
    pos[13, 0] = 0.5000001                       # outside
    pos[14, :dim] = 0.25                         # on a corner of cells
    volume = 10.**rng.uniform(-3., -1., n)
    force = C.dyadic_forces(n, dim, 3)
    plist = C.parts(pos, np.arange(n), volume, force)
    vf = TW.void_fraction(box, plist)
    want = U.void_fraction(dim, level, pos[:, :dim].tolist(), volume.tolist())
    assert np.array_equal(interior(vf[level], dim), want) and want.max() > 0.
    for rkernel in (0., 1.5*h, 2.5*h):
        Fv, corr, reached = TW.spread(box, plist, rkernel, C.POLY[1])
        wantF, wantc = U.spread(dim, level, pos[:, :dim].tolist(), volume.tolist(), force.tolist(), rkernel, C.POLY[1])
        assert np.array_equal(np.array(corr), wantc, equal_nan=True)
        for c in range(dim):
            assert np.array_equal(interior(Fv[c][level], dim), wantF[c]), (rkernel, c)
            assert np.abs(wantF[c]).max() > 0.
        # the order of the visited leaves is the box's too
        for p, leaves in zip(plist[:10], reached[:10]):
            assert [tuple(x.q[:dim]) for x in leaves] == U.descent(dim, level, p.pos, rkernel)


# -------------------------------------------------------------------------------------------------
# the fixtures
# -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.REFINED)
def test_fixtures_reach_what_they_are_meant_to(name):
    dim, _refine, sides = C.spec(name)
    box = C.host_tree(name)
    pos, ids, volume, force = C.spread_particles(box)
    plist = C.parts(pos, ids, volume, force)
    r0, r1, r2 = C.rkernels(box)
    most = 0
    for rkernel in (r1, r2):
        for p in plist:
            most = max(most, len(set(x.level for x in TW.descent(box, p.pos, rkernel))))
    assert most >= (3 if name == "graded" else 2)
    # a kernel that a side of the box clips: the particle is inside and nearer to the side than rkernel; there is no
    # periodic wrap (cond_kernel takes the distance as it is), so nothing beyond the side is reached
    clipped = [(p, a) for p in plist for a in range(dim)
               if box.locate(p.pos) is not None and 0.5 - abs(p.pos[a]) < r1]
    assert any(sides[2*a + (0 if p.pos[a] > 0. else 1)] == (C.B if name in ("walls2", "box3") else C.P)
               for p, a in clipped)
    if name == "box3":
        assert any(sides[2*a + (0 if p.pos[a] > 0. else 1)] == C.P for p, a in clipped)
    for p, a in clipped[:5]:
        for x in TW.descent(box, p.pos, r1):
            assert not x.boundary and abs(x.pos[a] - p.pos[a]) <= r1 + box.cell_size(x)
    # several particles share a leaf
    homes = [box.locate(p.pos) for p in plist]
    counts = {}
    for c in homes:
        if c is not None:
            counts[id(c)] = counts.get(id(c), 0) + 1
    assert max(counts.values()) >= 3 and sum(c is None for c in homes) >= dim
    # the order of the list is tested: the reversed list gives other sums in at least one leaf
    pv, _ = TC.seeds(box, 3)
    rng = np.random.default_rng(3)
    vols = 10.**rng.uniform(-6.5, -3.5, len(pv))
    vlist = C.parts(pv, np.arange(len(pv)), vols, np.zeros((len(pv), 3)))
    a, b = TW.void_fraction(box, vlist), TW.void_fraction(box, vlist[::-1])
    assert any(not np.array_equal(np.array(a[l]), np.array(b[l])) for l in range(box.level + 1))
    Fa = TW.spread(box, plist, r1, C.POLY[1])[0]
    Fb = TW.spread(box, plist[::-1], r1, C.POLY[1])[0]
    assert any(not np.array_equal(np.array(Fa[c][l]), np.array(Fb[c][l]))
               for c in range(dim) for l in range(box.level + 1))
    # the particle whose kernel is negative on its whole stencil deposits nothing
    _F, corr, reached = TW.spread(box, plist, r0, C.POLY[1])
    assert not corr[-1] > 1e-10 and len(reached[-1]) >= 1
    assert sum(c > 1e-10 for c in corr) > len(corr)//2


@pytest.mark.parametrize("name", C.REFINED)
def test_constant_kernel_spreads_every_force_exactly(name):
    """K = 1: correction is the quotient of two equal sums, 1. exactly, and with dyadic forces F*cellvol is minus
    the sum of the forces of the particles that reach the leaf, exactly"""
    dim = C.spec(name)[0]
    box = C.host_tree(name)
    plist = C.parts(*C.spread_particles(box))
    for rkernel in C.rkernels(box):
        Fv, corr, reached = TW.spread(box, plist, rkernel, C.ONE[1])
        total = {}
        for p, c, leaves in zip(plist, corr, reached):
            if leaves:
                assert c == 1.
            else:
                assert box.locate(p.pos) is None
            for x in leaves:
                t = total.setdefault(id(x), [0.]*dim)
                for a in range(dim):
                    t[a] += p.force[a]
        assert total
        for x in box.leaves:
            for a in range(dim):
                assert TW.get(box, x, Fv[a])*TW.cell_volume(box, x) == -total.get(id(x), [0.]*dim)[a]
        for x in box.ghosts:
            for a in range(dim):
                assert TW.get(box, x, Fv[a]) == 0.


# -------------------------------------------------------------------------------------------------
# the MAC value
# -------------------------------------------------------------------------------------------------

def test_mac_value_takes_every_branch():
    census = TW.new_census()
    for name in C.ALL:
        dim, _refine, sides = C.spec(name)
        box = C.host_tree(name)
        flags = [np.array(box.flags(l), dtype=np.uint8) for l in range(box.level + 1)]
        for c in range(dim):
            Fc = box.field(TC.distinct_values(dim, flags, salt=c))
            got = TW.mac_source(box, c, Fc, census, sides)
            for x in box.leaves:
                assert np.isfinite(TW.get(box, x, got))
    for branch in (TW.SAME_LEAF, TW.COARSER, TW.CHILDREN, TW.GHOST_BOUNDARY, TW.GHOST_PERIODIC):
        assert census[branch] > 0, dict(census)
    assert census[TW.NO_NEIGHBOR] == 0


def test_premise_of_the_uniform_field_test():
    """which trees qualify for `uniform source fields are a GfsSource': those on which the restated MAC value of the
    constant dyadic g is g exactly at every leaf.  On a convex patch the transverse neighbours of a coarse cell are
    leaves at distance 1 and every coefficient is dyadic; in the notch of the L-shaped patch 3/4 enters a
    denominator and exactness is not expected -- with the g of C.G_UNIFORM the roundings happen to cancel there
    too, and this test, not the expectation, decides: the GPU test runs on C.uniform_field_trees ()"""
    ok = C.uniform_field_trees()
    for name in ("square", "walls2", "cube"):
        assert name in ok, ok
    assert set(ok) <= set(C.REFINED)


@pytest.mark.parametrize("dim,axis", [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)])
def test_premise_of_the_striped_test(dim, axis):
    """the oracle on a tree refined in a band that depends on one coordinate only, fluid at rest, a constant GfsSource
    along another axis (along which everything is invariant): after start and one step U_c == dt*g exactly, the
    other components and P are exactly 0"""
    from oracle import oracle as O
    _dim, refine, _sides = C.striped(dim, axis)
    c = (axis + 1) % dim
    g = -16.
    ot = O.Tree(refine, dim=dim)
    assert len(set(l for l in range(ot.depth + 1) if (ot.flags(l) == T.LEAF).any())) == 2
    ot.set_source(c, g)
    ot.set_time(1e30, 0.8)
    ot.start()
    dt = ot.dt                   # the time step of the step to come (gfs_simulation_set_timestep at the end of start)
    ot.step()
    assert dt > 0. and ot.t == dt
    uvw = [O.Tree.U, O.Tree.V, O.Tree.W][:dim]
    for l in range(ot.depth + 1):
        m = np.zeros(ot.flags(l).shape, dtype=bool)
        m[(slice(1, -1),)*dim] = ot.flags(l)[(slice(1, -1),)*dim] == T.LEAF
        if not m.any():
            continue
        for a, var in enumerate(uvw):
            want = dt*g if a == c else 0.
            assert np.array_equal(ot.values(var, l)[m], np.full(int(m.sum()), want)), (l, a)
        assert np.array_equal(ot.values(O.Tree.P, l)[m], np.zeros(int(m.sum()))), l
    ot.destroy()
