"""The point sampler and the Lagrangian tracers on refined trees (csrc/tree_particles.hip) against the
restatement of the reference on explicit cell trees (tests/tree_sampler_reference.py), bit for bit; the
tracers of a uniform tree against those of the uniform box; the refusals of a list on a tree."""
import functools

import numpy as np
import pytest

import gfship
import sampler_reference as R
import tree_sampler_cases as TC

pytestmark = pytest.mark.gpu
G = gfship.Tree


def make_tree(name):
    dim, refine, sides, _ = TC.TREES[name]
    g = gfship.Tree(refine, dim=dim, sides=None if all(s == TC.P for s in sides) else sides)
    flags = [g.flags(l) for l in range(g.depth + 1)]
    return g, flags


@functools.lru_cache(None)
def restatement(name):
    """the TreeBox of a tree of TC.TREES, built once (its interpolators are cached in it) from the flags of
    the library's tree"""
    g, flags = make_tree(name)
    g.destroy()
    return TC.restatement(TC.TREES[name][0], flags), flags


def velocity_vars(dim):
    return [G.U, G.V, G.W][:dim]


@pytest.mark.parametrize("values", ["distinct", "random"])
@pytest.mark.parametrize("name", list(TC.TREES))
def test_interpolate(name, values):
    dim = TC.TREES[name][0]
    box, flags = restatement(name)
    g, gflags = make_tree(name)
    assert all(np.array_equal(a, b) for a, b in zip(flags, gflags))
    vals = TC.distinct_values(dim, flags) if values == "distinct" else TC.random_values(dim, flags, 11)
    for l, a in enumerate(vals):
        g.upload(G.T0, l, a)
    pts = TC.sample_points(box, 5)
    out, inside = g.interpolate(G.T0, pts)
    ref_out, ref_inside = box.sample(box.field(vals), pts.tolist(), nodata=False)
    stats = g.sampler_stats()
    g.destroy()
    assert np.array_equal(inside, np.array(ref_inside, dtype=bool))
    assert not np.isnan(np.array(ref_out)).any()
    assert np.array_equal(out, np.array(ref_out))
    assert inside.any() and not inside.all()
    # corners of leaves, corners in the table: none on a uniform tree, some but not all on a refined one
    assert stats[0] == len(box.leaves)*(1 << dim)
    assert (stats[1] == 0) == (name == "uniform2") and stats[1] < stats[0]
    assert stats[4] <= (7 if dim == 2 else 29)


def start_tree(name):
    dim, refine, sides, _ = TC.TREES[name]
    g, flags = make_tree(name)
    if name == "walls2":
        prof = [TC.inflow_profile(g.centres(l)) for l in range(g.depth + 1)]
        g.set_bc_u(0, 1, gfship.BC_DIRICHLET, prof)
        g.set_bc_u(0, 0, gfship.BC_NEUMANN)
        g.set_bc(0, gfship.BC_DIRICHLET)
    for l in range(g.depth + 1):
        for var, a in zip(velocity_vars(dim), TC.initial_velocity(name, g.centres(l))):
            g.upload(var, l, np.ascontiguousarray(np.broadcast_to(a, flags[l].shape)))
    for p in (g.projection_params, g.approx_projection_params):
        p.tolerance = 1e-4
    g.set_time(1e30, 0.8)
    g.start()
    return g


@pytest.mark.parametrize("name", list(TC.TREES))
def test_tracer_events(name):
    dim, _, sides, must = TC.TREES[name]
    box, flags = restatement(name)
    box.record = type(box.branches)()
    g = start_tree(name)
    pos, ids = TC.seeds(box, 3)
    pl = g.particles(pos, ids)
    pl.set_sort_interval(2)          # a sort between the events: storage order only
    plist = [R.Particle(p, i) for p, i in zip(pos.tolist(), ids.tolist())]
    for k in range(3):
        g.step()
        u = [box.field([g.download(var, l) for l in range(g.depth + 1)]) for var in velocity_vars(dim)]
        pl.event()
        plist, sent = box.list_event(u, plist, g.dt, sides)
        assert not sent
        p, i = pl.download()
        assert pl.count() == len(plist) == len(i)
        assert np.array_equal(i, np.array([q.id for q in plist], dtype=np.uint32))
        assert np.array_equal(p, np.array([q.pos for q in plist]).reshape(-1, 3)), "positions, event %d" % k
        assert np.array_equal(pl.download_old(), np.array([q.pos_old for q in plist]).reshape(-1, 3))
    pl.destroy()
    g.destroy()
    # the seeds outside the box, and what a periodic side put back while it was outside along another axis too
    assert box.record["outside_at_start"] >= dim
    for what in must:
        assert box.record[what] > 0, (what, dict(box.record))


@pytest.mark.parametrize("dim,level", [(2, 4), (3, 3)])
def test_uniform_tree_list_equals_uniform_box_list(dim, level):
    """the list of a uniform tree against the list of the uniform box (pinned on the oracle and on
    tests/sampler_reference.py): the same initial velocity, the same particles, 3 steps"""
    refine = (lambda x, y: level) if dim == 2 else (lambda x, y, z: level)
    g = gfship.Tree(refine, dim=dim)
    dom = gfship.Domain(dim, level, side=[gfship.SIDE_PERIODIC]*6)
    sim = gfship.Simulation(dom)
    u0 = TC.initial_velocity("uniform2" if dim == 2 else "cube", g.centres(level))
    n = 1 << level
    for c in range(dim):
        a = np.ascontiguousarray(np.broadcast_to(u0[c], (n + 2,)*dim))
        g.upload(velocity_vars(dim)[c], level, a)
        sim.u[c].upload(a)
    for p in (g.projection_params, g.approx_projection_params, sim.projection_params, sim.approx_projection_params):
        p.tolerance = 1e-4
    g.set_time(1e30, 0.8)
    sim.set_time(1e30)
    sim.advection_params.cfl = 0.8
    rng = np.random.default_rng(dim)
    pos = np.zeros((300, 3))
    pos[:, :dim] = rng.uniform(-0.5, 0.5, (300, dim))
    pos[:40, 0] = 0.5 - rng.uniform(0., 0.01, 40)        # next to the side the flow leaves through
    ids = np.arange(300, dtype=np.uint32)
    tl, ul = g.particles(pos, ids), gfship.ParticleList(sim, pos, ids)
    g.start()
    sim.start()
    for k in range(3):
        g.step()
        sim.step()
        assert g.dt == sim.dt
        tl.event()
        ul.event()
        (tp, ti), (up, ui) = tl.download(), ul.download()
        assert np.array_equal(ti, ui) and np.array_equal(tp, up), k
        assert np.array_equal(tl.download_old(), ul.download_old())
    assert (np.abs(tp - pos[:len(tp)]) > 0.).any()
    for x in (tl, ul, sim, dom, g):
        x.destroy()


def test_refusals_on_a_tree_list():
    g, _ = make_tree("square")
    pl = g.particles(np.zeros((4, 3)), np.arange(4))
    dom = gfship.Domain(2, 3, side=[gfship.SIDE_PERIODIC]*6)
    v = dom.variable()
    calls = [lambda: pl.set_particulate(np.zeros((4, 3)), np.ones(4), np.ones(4)),
             lambda: pl.set_forces([gfship.FORCE_DRAG]),
             lambda: gfship._check(gfship.lib().gfship_particles_set_migrate(pl.ptr, None, None)),
             lambda: pl.particulate_field(v),
             lambda: pl.forces_on_fluid(),
             lambda: pl.spread_forces([v, v]),
             lambda: pl.source_particulate_event([v, v]),
             lambda: pl.set_kernel(0.1),
             lambda: pl.set_force_coefficient(0, "1."),
             lambda: pl.particulate_state()]
    for call in calls:
        with pytest.raises(gfship.GfshipError, match="gfship error -5: .*tree"):
            call()
    assert pl.count() == 4
    pl.destroy()
    g.destroy()
    dom.destroy()
