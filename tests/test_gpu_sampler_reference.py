"""The device's point sampler (gfship_field_interpolate) and tracer event
(gfship_particle_list_event) against the restatement of the reference on an explicit cell graph
(tests/sampler_reference.py), by array_equal: the library is built with -ffp-contract=off and keeps
the reference's operand order on this path.  2-D and 3-D, levels 1 (every cell at a box corner), 2
(every class of cell) and 3 (a true interior); gfship_domain_create accepts level 1.  The cases
and their references are those of tests/sampler_cases.py, on which test_sampler_reference_cpu.py
shows the restatement to be defined (check_intersetion never fails) and the oracle to agree."""
import numpy as np
import pytest

import gfship
import sampler_cases as K

pytestmark = pytest.mark.gpu


def _same_array(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("variant", ["distinct", "nodata"])
@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_field_interpolate_equals_the_restatement(dim, level, variant):
    """every interior cell and every face ghost holds a value of its own, uploaded with the ghosts;
    the edge and corner ghosts hold NaN and no result is NaN: they are never read.

    nodata: GFS_NODATA (DBL_MAX) in one interior cell and in one face ghost.  Nothing in this library
    produces that value (no solid boundaries, no masked output variables), gfship_field_interpolate
    does not support it (include/gfship.h) and treats it as the number it is: pinned here on the
    restatement without src/fluid.c:2704-2705 and :3096-3097."""
    a = K.sampler_field(dim, level, variant)
    pts = K.sample_points(dim, level)
    gd = gfship.Domain(dim, level, K.SIDES["closed"])
    v = gd.variable()
    v.upload(a)
    assert _same_array(v.download(), a)
    out, inside = gd.interpolate(v, pts)
    ref, ref_inside = K.reference_sample(dim, level, variant)
    assert np.array_equal(inside, ref_inside)
    assert not inside[np.abs(pts[:, :dim]).max(axis=1) > 0.5].any()
    assert np.all(out[~inside] == 0.)
    print("points", len(pts), "inside", inside.sum(), "differing", (out != ref).sum())
    if variant == "distinct":
        assert not np.isnan(out).any()
        assert np.array_equal(out, ref)
    else:
        assert np.array_equal(out, ref, equal_nan=True)
        ordinary, _ = K.reference_sample(dim, level, "distinct")
        assert (out != ordinary).sum() > 0
    gd.destroy()


@pytest.mark.parametrize("kind", ["periodic", "dirichlet", "neumann"])
@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_field_interpolate_with_the_ghosts_of_the_library_bc(dim, level, kind):
    """the ghosts are filled by gfship_bc: they must be the values the reference's boundary cells
    hold (the cell across a periodic box; 2*val - neighbour, src/boundary.c:253-258; neighbour +
    val*size, :336-342), and the sampler must give what the restatement gives on exactly those"""
    sides, interior, vals, expect = K.bc_case(dim, level, kind)
    n = 1 << level
    gd = gfship.Domain(dim, level, sides)
    v = gd.variable()
    a = np.full((n + 2,)*dim, np.nan)
    a[(slice(1, n + 1),)*dim] = interior
    v.upload(a)
    for d, (bc, val) in vals.items():
        v.set_bc(d, bc, val)
    gd.bc(v)
    got = v.download()
    assert np.array_equal(got[(slice(1, n + 1),)*dim], interior)
    assert K.face_ghosts_equal(dim, level, got, expect)
    pts = K.sample_points(dim, level)
    out, inside = gd.interpolate(v, pts)
    ref, ref_inside = K.reference_sample(dim, level, "bc_" + kind)
    assert np.array_equal(inside, ref_inside)
    assert not np.isnan(out).any()
    assert np.array_equal(out, ref)
    gd.destroy()


@pytest.mark.parametrize("sides", sorted(K.SIDES))
@pytest.mark.parametrize("dim,level", K.DIMS_LEVELS)
def test_tracer_list_event_equals_the_restatement(dim, level, sides):
    """K.NEVENTS events of plain tracers in a fixed velocity field (the smooth one, then the
    distinct-values fill), never sorted and sorted by cell at every event: positions, old positions,
    the list of survivors and its order after every event.  A particle that leaves a periodic box
    through an edge is wrapped along one axis only and the next event removes it; through a closed
    or an external side (no migration hook) it leaves the list."""
    gd = gfship.Domain(dim, level, K.SIDES[sides])
    gs = gfship.Simulation(gd)
    for field in K.TRACER_FIELDS:
        u = K.tracer_field(dim, level, field)
        for c in range(dim):
            gs.u[c].upload(u[c])
        gs.advection_params.dt = K.tracer_dt(level)
        pos, ids = K.tracer_particles(dim, level, field)
        reference = K.reference_events(dim, level, sides, field)
        for sort_every in (0, 1):
            gpl = gfship.ParticleList(gs, pos, ids)
            gpl.set_sort_interval(sort_every)
            for k, (rp, rpo, ri) in enumerate(reference):
                gpl.event()
                gp, gi = gpl.download()
                gpo = gpl.download_old()
                what = (field, sort_every, k)
                assert np.array_equal(gi, ri), what
                assert gpl.count() == len(ri), what
                assert np.array_equal(gp, rp), (what, np.abs(gp - rp).max())
                assert np.array_equal(gpo, rpo), (what, np.abs(gpo - rpo).max())
            gpl.destroy()
        for c in range(dim):
            assert _same_array(gs.u[c].download(), u[c])
    gs.destroy()
    gd.destroy()
