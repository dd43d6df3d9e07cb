"""GfsFeedParticle on refined trees on the device (gfship.TreeFeedParticle, Tree.idlast) against the restatement of
tests/feed_particle_reference.py on the runs of tests/tree_feed_particle_cases.py.

Bit for bit (array_equal): positions, ids, the download order, velocities, mass, volume, force, pos_old, the count,
the slots and idlast after every event and after a sort -- no libm call is involved in any of them.  The diameter
and rb of a new particle are values of the device's pow: what is downstream of them (an event with drag, the
spreading of GfsSourceParticulate, a mass source) is compared within the POW_ULPS that
tests/test_gpu_particulate_sources.py measures and justifies for the same expression, by the method of
tests/test_gpu_feed_particle.py: the restatement with the pow of the new particles moved down and up by POW_ULPS,
every device value inside the hull of the results widened by one ulp.  Whatever does not pass through pow stays
bit for bit.

The fluid of the restatement is the device's own: the velocities (ghost cells included) and the times of the tree
at every event are downloaded and registered with the cases."""
import ctypes
import math

import numpy as np
import pytest

import forces_reference as F
import gfship
import particulate_sources_cases as BK
import tree_feed_particle_cases as C
import tree_forces_reference as TF
import tree_particulate_sources_cases as K
import tree_particulate_sources_reference as PS
import tree_two_way_cases as TWC
import tree_two_way_reference as TW
from test_gpu_particulate_sources import POW_ULPS, _shifted_pow, _ulps
from test_gpu_tree_particulate_sources import fluid, levels, start_tree

pytestmark = pytest.mark.gpu

G = gfship.Tree
URELS = [G.URELP, G.VRELP, G.WRELP]
FVARS = [G.FX, G.FY, G.FZ]
DRAG, BUOY = F.DRAG, F.BUOY
NU, GRAVITY = 1e-2, (0., -0.5, 0.)


class Device:
    """a started tree with the tracer T0 of the cases; lists of the particles of the cases with idlast = IDLAST0"""

    def __init__(self, name, nu=0.):
        self.name, self.dim = name, C.spec(name)[0]
        self.g, self.flags = start_tree(name, nu)
        self.owned = []
        self.set_tracer()

    def set_tracer(self):
        for l, a in enumerate(C.tracer(self.name)):      # the steps advect T0: every event reads the same values
            self.g.upload(G.T0, l, a)

    def new_list(self):
        pos, ids, vel, mass, volume = C.particles(self.name)
        pl = self.g.particulates(pos, ids, vel, mass, volume)
        self.owned.append(pl.destroy)
        pl.set_sort_interval(0)
        pl.set_forces([DRAG, BUOY], GRAVITY)
        assert self.g.idlast(pl) == 0                    # gfs_particle_list_init
        self.g.set_idlast(pl, C.IDLAST0)
        return pl

    def feed(self, pl, fname):
        mass, volume = C.FUNCTIONS[fname][0]
        f = gfship.TreeFeedParticle(self.g, pl, mass, volume, {"T": G.T0})
        self.owned.append(f.close)
        return f

    def step(self):
        self.g.step()
        self.set_tracer()

    def stage(self):
        return fluid(self.g, self.dim), self.g.t

    def state(self, pl):
        pos, ids = pl.download()
        vel, mass, force = pl.particulate_state()
        return C.State(pos, ids, pl.download_old(), vel, mass, pl.volumes(), force, self.g.idlast(pl), ())

    def close(self):
        for close in reversed(self.owned):               # the feeds before their lists, the lists before the tree
            close()
        self.g.destroy()


def _assert_state(got, want, what):
    assert len(got.ids) == len(want.ids), what
    for name in ("ids", "pos", "old", "vel", "mass", "volume", "force"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name)
    assert got.idlast == want.idlast, what


def _slots(pl):
    return gfship.lib().gfship_particles_slots(pl.ptr)


# ---- the events, bit for bit ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", C.TREES)
def test_events_equal_the_restatement(name):
    """0, 1, 70, 300 and 3000 candidates in a row on one list per function, a step of the tree between two events:
    the second event starts from the idlast of the first, the third makes the arrays of the list grow (40 slots at
    creation), the last spans twelve blocks"""
    dev = Device(name)
    try:
        lists = {fname: dev.new_list() for fname in C.FUNCTIONS}
        feeds = {fname: dev.feed(lists[fname], fname) for fname in C.FUNCTIONS}
        got = {fname: [] for fname in C.FUNCTIONS}
        stages, slots = [], C.NPART
        for e, count in enumerate(C.COUNTS):
            if e > 0:
                dev.step()
            stages.append(dev.stage())
            slots += count
            for fname, pl in lists.items():
                feeds[fname].event(C.candidates(name, e))
                assert _slots(pl) == slots
                got[fname].append((dev.state(pl), pl.count()))
        assert len(set(s[1] for s in stages)) == len(stages)
        C.register_stages(name, "events", stages)
        for fname, pl in lists.items():
            ref = C.reference_run(name, fname, "events")
            for e, (state, count) in enumerate(got[fname]):
                _assert_state(state, ref[e], (name, fname, e))
                assert count == len(ref[e].ids)
                if dev.dim == 2:
                    assert not state.vel[C.NPART:, 2].any() and not state.pos[:, 2].any()
            assert ref[-1].idlast > C.IDLAST0 + 256 and len(ref[-1].ids) < slots
            # the storage order changes nothing of the list; the dead slots stay slots
            pl.sort()
            _assert_state(dev.state(pl), ref[-1], (name, fname, "sorted"))
            assert _slots(pl) == slots and pl.count() == len(ref[-1].ids)
    finally:
        dev.close()


def test_the_ids_do_not_depend_on_the_run():
    name, fname, e = "cube", "tracer", 4
    runs = []
    for _ in range(2):
        dev = Device(name)
        try:
            pl = dev.new_list()
            dev.feed(pl, fname).event(C.candidates(name, e))
            runs.append(dev.state(pl))
        finally:
            dev.close()
    _assert_state(runs[0], runs[1], "twice")
    assert runs[0].idlast > C.IDLAST0 + 256


def test_idlast_of_any_list_of_a_tree_and_the_defaults():
    name = "square"
    dev = Device(name)
    try:
        g = dev.g
        pl = dev.new_list()
        pos, ids = C.particles(name)[:2]
        tracers = g.particles(pos, ids)
        dev.owned.append(tracers.destroy)
        assert g.idlast(tracers) == 0                     # gfs_particle_list_init
        g.set_idlast(tracers, 17)
        assert g.idlast(tracers) == 17 and g.idlast(pl) == C.IDLAST0
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            g.set_idlast(pl, -1)
        # gfs_feed_particle_init: no mass, nothing is fed, and no id is taken; the candidates are dead slots
        nothing = gfship.TreeFeedParticle(g, pl)
        dev.owned.append(nothing.close)
        nothing.event(C.candidates(name, 2))
        assert pl.count() == C.NPART and g.idlast(pl) == C.IDLAST0 and _slots(pl) == C.NPART + C.COUNTS[2]
        # Rad is no variable of these functions unless the table says so
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile"):
            gfship.TreeFeedParticle(g, pl, "Rad", "1e-4")
        rad = gfship.TreeFeedParticle(g, pl, "1e-3*Rad", "1e-4", {"Rad": G.T0})
        dev.owned.append(rad.close)
        rad.event(np.array([[0.1, 0.2, 0.]]))
        assert pl.count() == C.NPART + 1 and g.idlast(pl) == C.IDLAST0 + 1
        assert pl.download()[1][-1] == C.IDLAST0 + 1
    finally:
        dev.close()


# ---- a uniform tree against the box -----------------------------------------------------------------------

@pytest.mark.parametrize("name,dim", [("uniform2", 2), ("uniform3d", 3)])
def test_uniform_tree_equals_uniform_box(name, dim):
    """the fed list of a uniform tree of level 3 is, bit for bit, the list gfship.FeedParticle gives on the uniform
    box of level 3 with the same velocity, functions and candidates"""
    level = K.UNIFORM[dim]
    dev = Device(name)
    gd = gfship.Domain(dim, level, BK.SIDES["periodic"])
    gs = gfship.Simulation(gd)
    boxed = []
    try:
        Tv = gd.variable()
        Tv.upload(C.tracer(name)[level])
        pos, ids, vel, mass, volume = C.particles(name)
        pairs = {}
        for fname in C.FUNCTIONS:
            pl = dev.new_list()
            gpl = gfship.ParticleList(gs, pos, ids)
            boxed.append(gpl.destroy)
            gpl.set_sort_interval(0)
            gpl.set_particulate(vel, mass, volume)
            gpl.idlast = C.IDLAST0
            bfeed = gfship.FeedParticle(gpl, *C.FUNCTIONS[fname][0], {"T": Tv})
            boxed.append(bfeed.close)
            pairs[fname] = (pl, dev.feed(pl, fname), gpl, bfeed)
        for e in range(len(C.COUNTS)):
            if e > 0:
                dev.step()
            u, t = dev.stage()
            for c in range(dim):
                gs.u[c].upload(u[c][level])
            gs.restart(t, e)
            for fname, (pl, feed, gpl, bfeed) in pairs.items():
                feed.event(C.candidates(name, e))
                bfeed.event(C.candidates(name, e))
                bpos, bids = gpl.download()
                bvel, bmass, bforce = gpl.particulate_state()
                want = C.State(bpos, bids, gpl.download_old(), bvel, bmass, gpl.volumes(), bforce, gpl.idlast, ())
                _assert_state(dev.state(pl), want, (name, fname, e))
                assert pl.count() == gpl.count() and _slots(pl) == _slots(gpl)
        assert dev.g.idlast(pairs["tracer"][0]) > C.IDLAST0 + 256
    finally:
        for close in reversed(boxed):
            close()
        gs.destroy()
        gd.destroy()
        dev.close()


# ---- downstream of a feed: dia, rb and orig of the newcomers, the arrays that follow a grown list ----------

FED_EVENTS = (1, 2)               # 1 and 70 candidates: the list grows from 40 to 111 slots
SPREAD_TEXT = "(1. - 1e-4*(x*x + y*y + z*z))"
SOURCE_FUNCTION = "tracer"        # of tree_particulate_sources_cases: reads T and the relative velocity
RAD_HELD = -3.


def _spread_kernel(x, y, z, t):
    return (1. - 1e-4*(x*x + y*y + z*z))


def _leaf_values(box, arrays):
    """the values of a variable (one array with ghosts per level) at the leaves of the box, in traversal order"""
    f = box.field(arrays)
    return np.array([box.value(c, f) for c in box.leaves])


def _clone(plist):
    out = []
    for p in plist:
        q = F.Particulate(p.pos, p.id, p.vel, p.mass, p.volume)
        q.pos_old, q.force = list(p.pos_old), list(p.force)
        out.append(q)
    return out


def _downstream_reference(name, stage, steps_dia, steps_rb, where="downstream"):
    """the chain of the device test in the restatements, with the pow of the new particles moved by `steps_dia' ulps
    in their diameter and by `steps_rb' ulps in their rb: a dict of its results.  What a leaf sums over its
    particles (the spread forces, the deposit of the mass source) comes per particle (`F_parts', `deposit_parts'),
    in list order, at the leaves of the tree in traversal order"""
    box = C.host_tree(name)
    dim, _refine, sides = C.spec(name)
    u, t, dt = stage
    pl, _ = C.feed_events(name, "tracer", FED_EVENTS, where)
    plist = _clone(pl.plist)
    new_ids = {p.id for p in plist if p.id > C.IDLAST0}
    new_volumes = {p.volume for p in plist if p.id in new_ids}
    assert not new_volumes & {p.volume for p in plist if p.id not in new_ids}
    pow_dia, pow_rb = _shifted_pow(steps_dia), _shifted_pow(steps_rb)
    sim = F.Sim(box, sides, u, dt, viscosity=((lambda cell: NU), None, None), g=GRAVITY, root=F.sqrt_root)
    objs = [F.ForceCoeff(DRAG), F.ForceCoeff(BUOY)]
    TF.read_forces(sim, objs)
    diameter, distance = F._diameter, TW.normalized_distance

    def normalized_distance(dim_, centre, p, volume):
        if volume not in new_volumes:
            return distance(dim_, centre, p, volume)
        rb = pow_rb(3.*volume/(4.*math.pi), 1./3.)        # distance_normalization, :2091
        return ((centre[0] - p[0])/rb, (centre[1] - p[1])/rb, (0. - p[2])/rb if dim_ == 3 else 0.)
    F._diameter = lambda p: 2.*pow_dia(3.0*p.volume/4.0/math.pi, 1./3.) if p.id in new_ids else diameter(p)
    TW.normalized_distance = normalized_distance
    out = {}
    try:
        plist = TF.list_event(sim, plist, objs)
        out["ids"] = np.array([p.id for p in plist], dtype=np.uint32)
        for key in ("pos", "pos_old", "vel", "force"):
            out[key] = np.array([getattr(p, key) for p in plist])
        out["mass"] = np.array([p.mass for p in plist])
        out["void"] = _leaf_values(box, TW.void_fraction(box, plist))
        TW.forces_on_fluid(sim, plist, objs)
        out["onfluid"] = np.array([p.force for p in plist])
        rkernel = 1.5*TWC.h_fine(box)
        parts = []
        for q in range(len(plist)):
            Fv, _corr, _reached = TW.spread(box, plist[q:q + 1], rkernel, _spread_kernel, t)
            parts.append(np.stack([_leaf_values(box, Fv[c]) for c in range(dim)]))
        out["F_parts"] = np.stack(parts)
        rad = [np.full(s, RAD_HELD) for s in C.shapes(box)]
        fields = PS.Fields(box.field(rad), [TW.zeros(box) for _ in range(dim)], TW.zeros(box))
        fn = K.functions(dim)[SOURCE_FUNCTION][1]
        sources = PS.event(box, PS.MASS, plist, sim.u, dt, t, fn, fields, {"T": box.field(C.tracer(name))})
        out["source_mass"] = np.array([p.mass for p in plist])
        index = {id(c): n for n, c in enumerate(box.leaves)}
        dep = np.zeros((len(plist), len(box.leaves)))
        for q, (p, s) in enumerate(zip(plist, sources)):
            if s is not None:          # (a particle without a leaf is skipped)
                dep[q, index[id(box.locate(p.pos))]] = s
        out["deposit_parts"] = dep
        out["rad"] = _leaf_values(box, fields.rad)
    finally:
        F._diameter, TW.normalized_distance = diameter, distance
    return out


@pytest.mark.parametrize("name", C.REFINED)
def test_a_fed_list_behaves_as_one_given_at_creation(name):
    """The bound of what passes through pow is derived, never fitted.  The diameter and the rb of a new particle are
    two values of the device's pow, each within POW_ULPS of glibc's, independently.  A quantity of one particle
    (position, velocity, force, mass) is a function of those two numbers: the device value lies in the hull of the
    restatement over the corners and the centre of [-POW_ULPS, POW_ULPS]^2, widened by one ulp.  A quantity of a
    leaf is a sum over its particles in list order, each term in the hull of that particle's terms (the particles
    are off by different amounts, so the hull of the sums would be no bound); the sum lies between the sums of the
    lower and of the upper ends, widened by the rounding of a sum of n terms, n*eps*sum |term|.  The particles of
    the list as created, the void fraction and the leaves no new particle reaches stay bit for bit."""
    dim = C.spec(name)[0]
    box = C.host_tree(name)
    dev = Device(name, NU)
    try:
        g = dev.g
        stage = (fluid(g, dim), g.t, g.dt)
        C.register_stages(name, "downstream", [stage[:2]]*len(C.COUNTS))
        corners = [(a, b) for a in (-POW_ULPS, 0, POW_ULPS) for b in (-POW_ULPS, 0, POW_ULPS)]
        runs = [_downstream_reference(name, stage, a, b) for a, b in corners]
        exact = runs[corners.index((0, 0))]

        def in_hull(got, key):
            stack = np.stack([r[key] for r in runs])
            lo, hi = np.nextafter(stack.min(axis=0), -np.inf), np.nextafter(stack.max(axis=0), np.inf)
            if got.ndim == 2 and got.shape[1] == 3 and dim == 2:
                got, lo, hi = got[:, :2], lo[:, :2], hi[:, :2]
            assert got.shape == lo.shape, key
            bad = (got < lo) | (got > hi)
            print("%s %s: %d values outside the hull" % (name, key, int(bad.sum())))
            assert not bad.any(), (key, int(bad.sum()))

        def in_hull_of_sums(got, key):
            stack = np.stack([r[key] for r in runs])          # run, particle, ... leaves
            lo, hi = stack.min(axis=0).sum(axis=0), stack.max(axis=0).sum(axis=0)
            slack = stack.shape[1]*np.finfo(float).eps*np.abs(stack).max(axis=0).sum(axis=0)
            assert got.shape == lo.shape, key
            bad = (got < lo - slack) | (got > hi + slack)
            print("%s %s: %d sums outside the bound" % (name, key, int(bad.sum())))
            assert not bad.any(), (key, int(bad.sum()), float(np.abs(got - exact[key].sum(axis=0))[bad].max()))
            # where no new particle contributes the sum is the restatement's, bit for bit
            same = (stack.min(axis=0) == stack.max(axis=0)).all(axis=0)
            serial = np.zeros_like(lo)
            for part in exact[key]:
                serial = serial + part
            assert same.any() and np.array_equal(got[same], serial[same]), key

        pl = dev.new_list()
        feed = dev.feed(pl, "tracer")
        for e in FED_EVENTS:
            feed.event(C.candidates(name, e))
        before = dev.state(pl)
        _assert_state(before, C.feed_events(name, "tracer", FED_EVENTS, "downstream")[1][-1], "fed")
        pl.sort()
        _assert_state(dev.state(pl), before, "sorted")
        old = exact["ids"] <= C.IDLAST0
        # one gfs_particle_list_event with drag and buoyancy: the drag of a new particle reads its diameter
        pl.event()
        got = dev.state(pl)
        assert np.array_equal(got.ids, exact["ids"]) and (got.ids > C.IDLAST0).sum() >= 8
        assert np.array_equal(got.old[:, :dim], exact["pos_old"][:, :dim])      # the event wrote pos_old of the new ones
        for a, key in ((got.pos, "pos"), (got.vel, "vel"), (got.force, "force")):
            in_hull(a, key)
            assert np.array_equal(a[old][:, :dim], exact[key][old][:, :dim]), key      # host-computed diameters
        assert np.array_equal(got.mass, exact["mass"])
        assert np.abs(got.force[~old][:, :dim]).max() > 0.
        # GfsParticulateField: the volumes, and the leaves of the moved particles
        g.particulate_field(pl)
        assert np.array_equal(_leaf_values(box, levels(g, G.VF)), exact["void"]) and exact["void"].max() > 0.
        # GfsSourceParticulate: the forces on the fluid, spread with rb of every particle
        g.set_kernel(pl, 1.5*TWC.h_fine(box), SPREAD_TEXT)
        g.source_particulate_event(pl)
        in_hull(pl.particulate_state()[2], "onfluid")
        spread = np.stack([_leaf_values(box, levels(g, FVARS[c])) for c in range(dim)])
        in_hull_of_sums(spread, "F_parts")
        assert np.abs(spread).max() > 0. and np.abs(exact["F_parts"][~old]).max() > 0.
        # GfsSourceParticulateMass: per creation slot, hence `orig' of the new particles
        src = gfship.TreeParticulateSource(g, pl, gfship.SOURCE_MASS, K.functions(dim)[SOURCE_FUNCTION][0], {"T": G.T0})
        dev.owned.append(src.destroy)
        for l, s in enumerate(C.shapes(box)):
            g.upload(G.RAD, l, np.full(s, RAD_HELD))
            g.upload(G.DMDT, l, np.zeros(s))
        src.set_fields(G.RAD, URELS[:dim], G.DMDT)
        src.event()
        in_hull(pl.particulate_state()[1], "source_mass")
        in_hull_of_sums(_leaf_values(box, levels(g, G.DMDT)), "deposit_parts")
        grad, wrad = _leaf_values(box, levels(g, G.RAD)), exact["rad"]
        written = wrad != RAD_HELD
        assert np.array_equal(grad != RAD_HELD, written) and written.sum() > 10
        assert _ulps(grad[written], wrad[written]).max() <= POW_ULPS
    finally:
        dev.close()


# ---- refusals and lifetimes -------------------------------------------------------------------------------

def _create(pl, mass, volume, names, numbers):
    """gfship_tree_feed_particle_create with a table given as two lists (a dict cannot hold a name twice)"""
    p = ctypes.c_void_p()
    n = len(names)
    r = gfship.lib().gfship_tree_feed_particle_create(
        ctypes.byref(p), pl.ptr, mass.encode(), volume.encode(), n,
        (ctypes.c_char_p*max(n, 1))(*[s.encode() for s in names]), (ctypes.c_int*max(n, 1))(*numbers))
    if r == 0:
        gfship.lib().gfship_feed_particle_destroy(p)
    return r


def test_refusals():
    name = "square"
    dev = Device(name)
    pos, ids, vel, mass, volume = C.particles(name)
    try:
        g = dev.g
        pl = dev.new_list()
        # a list of tracers of a tree, a list of a box
        tracers = g.particles(pos, ids)
        dev.owned.append(tracers.destroy)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*particulates"):
            gfship.TreeFeedParticle(g, tracers, "1e-3", "1e-4")
        gd = gfship.Domain(2, 3, BK.SIDES["periodic"])
        gs = gfship.Simulation(gd)
        bpl = gfship.ParticleList(gs, pos, ids)
        try:
            bpl.set_particulate(vel, mass, volume)
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*tree"):
                gfship.TreeFeedParticle(g, bpl, "1e-3", "1e-4")
            with pytest.raises(gfship.GfshipError, match="gfship error -5"):
                g.idlast(bpl)
            with pytest.raises(gfship.GfshipError, match="gfship error -5"):
                g.set_idlast(bpl, 3)
        finally:
            bpl.destroy()
            gs.destroy()
            gd.destroy()
        # the table: a reserved name, a name twice, no C identifier
        for reserved in ("x", "y", "z", "t"):
            with pytest.raises(gfship.GfshipError, match="gfship error -1"):
                gfship.TreeFeedParticle(g, pl, reserved, "1e-4", {reserved: G.T0})
        assert _create(pl, "1e-3*Q", "1e-4", ["Q", "Q"], [G.T0, G.U]) == -1
        assert _create(pl, "1e-3", "1e-4", ["2Q"], [G.T0]) == -1
        assert _create(pl, "1e-3*Q", "1e-4*R", ["Q", "R"], [G.T0, G.U]) == 0
        # a variable the tree does not have now: one tracer was added, T0, and no T1; nothing has allocated VF; no
        # such number; no W on a quadtree
        for var in (G.T1, G.VF, 99, -1):
            with pytest.raises(gfship.GfshipError, match="gfship error -1.*no variable"):
                gfship.TreeFeedParticle(g, pl, "1e-3*Q", "1e-4", {"Q": var})
        for var in (G.W, G.GZ, G.BCW):
            with pytest.raises(gfship.GfshipError, match="gfship error -1.*no variable"):
                gfship.TreeFeedParticle(g, pl, "1e-3*Q", "1e-4", {"Q": var})
        # a text that does not compile: the error of the box path, the compiler's message in gfship_last_error
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile") as err:
            gfship.TreeFeedParticle(g, pl, "1e-3*Q", "1e-4")
        assert "Q" in str(err.value) and gfship.lib().gfship_last_error()
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile"):
            gfship.TreeFeedParticle(g, pl, "1e-3", "{ return 1e-4 }")
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile"):
            gfship.TreeFeedParticle(g, pl, "1e-3*Urelp", "1e-4")          # no variable of a source here
        # the calls of a box keep refusing a list of a tree
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gfship.FeedParticle(pl, "1e-3", "1e-4")
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            pl.idlast
        # nothing above changed the list; a closed feed is closed once, and the list outlives it
        f = dev.feed(pl, "constant")
        f.event(np.array([[0.1, 0.2, 0.]]))
        f.close()
        f.close()
        assert f.ptr is None and pl.count() == C.NPART + 1 and g.idlast(pl) == C.IDLAST0 + 1
    finally:
        dev.close()
    # on an octree W is a variable like any other
    dev = Device("cube")
    try:
        pl = dev.new_list()
        f = gfship.TreeFeedParticle(dev.g, pl, "1e-3*(2. + Q)", "1e-4", {"Q": G.W})
        dev.owned.append(f.close)
        f.event(np.array([[0.1, 0.2, 0.3]]))
        assert pl.count() == C.NPART + 1
    finally:
        dev.close()
