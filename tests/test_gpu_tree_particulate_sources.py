"""GfsSourceParticulateVol / GfsSourceParticulateMass on refined trees on the device (gfship.TreeParticulateSource)
against the restatement of tests/tree_particulate_sources_reference.py on the runs of
tests/tree_particulate_sources_cases.py.

Bit for bit (array_equal) wherever no libm call is involved: volumes or masses, the deposit and Urelp ... on every
level (the cells nothing writes still hold what was uploaded), the skipped particles -- before and after
gfship_particles_sort and after the second sort that leaves the particles of one leaf stored in the reverse of
their list order (test_tree_particulate_sources_reference_cpu.py asserts that premise on the host's stages).  Rad,
and what a changed volume does to the diameter, are values of the device's pow: compared with glibc's within the
POW_ULPS of tests/test_gpu_particulate_sources.py.

The fluid of the restatement is the device's own: a tree of each name is started and stepped once without a list,
and its velocities, times and time steps are the stages of every run on that tree (the steps of a tree are
deterministic, which every run asserts)."""
import functools
import math

import numpy as np
import pytest

import forces_reference as F
import gfship
import particulate_sources_cases as BK
import tree_forces_reference as TF
import tree_particulate_sources_cases as K
import tree_particulate_sources_reference as PS
import tree_sampler_cases as TC
import tree_sampler_reference as T
from test_gpu_particulate_sources import POW_ULPS

pytestmark = pytest.mark.gpu

G = gfship.Tree
UVARS = [G.U, G.V, G.W]
URELS = [G.URELP, G.VRELP, G.WRELP]
KINDS = {"vol": (gfship.SOURCE_VOLUME, PS.VOLUME, G.VOLSRC), "mass": (gfship.SOURCE_MASS, PS.MASS, G.DMDT)}
CFL = 0.4
NU = 1e-2


def _ulps(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def make_tree(name):
    dim, refine, sides = K.spec(name)
    g = gfship.Tree(refine, dim=dim, sides=None if all(s == TC.P for s in sides) else sides)
    flags = [g.flags(l) for l in range(g.depth + 1)]
    box = K.host_tree(name)
    for l, f in enumerate(flags):      # the tree of the cases is the tree of the device
        assert np.array_equal(np.array(box.flags(l), dtype=np.uint8), f), (name, l)
    return g, flags


def start_tree(name, nu=0.):
    dim = K.spec(name)[0]
    g, flags = make_tree(name)
    if name == "walls2":
        prof = [TC.inflow_profile(g.centres(l)) for l in range(g.depth + 1)]
        g.set_bc_u(0, 1, gfship.BC_DIRICHLET, prof)
        g.set_bc_u(0, 0, gfship.BC_NEUMANN)
        g.set_bc(0, gfship.BC_DIRICHLET)
    vname = "cube" if name == "uniform3d" else "square" if name == "ell" else name
    for l in range(g.depth + 1):
        for var, a in zip(UVARS, TC.initial_velocity(vname, g.centres(l))):
            g.upload(var, l, np.ascontiguousarray(np.broadcast_to(a, flags[l].shape)))
    for p in (g.projection_params, g.approx_projection_params):
        p.tolerance = 1e-4
    if nu:
        for c in range(dim):
            g.set_viscosity(c, nu)
    assert g.add_tracer() == G.T0
    g.set_time(1e30, CFL)
    g.start()
    return g, flags


def fluid(g, dim):
    return [[g.download(var, l) for l in range(g.depth + 1)] for var in UVARS[:dim]]


def levels(g, var):
    return [g.download(var, l) for l in range(g.depth + 1)]


@functools.lru_cache(None)
def device_stages(name):
    """the velocities, times and time steps of a tree of this name at the three events; registered with the cases"""
    dim = K.spec(name)[0]
    g, _ = start_tree(name)
    stages = []
    try:
        for e in range(K.NEVENTS):
            if e > 0:
                g.step()
            stages.append((fluid(g, dim), g.t, g.dt))
    finally:
        g.destroy()
    # three events with different velocities, t and dt
    assert len(set(s[1] for s in stages)) == 3 and len(set(s[2] for s in stages)) == 3
    for a, b in ((0, 1), (1, 2), (0, 2)):
        for c in range(dim):
            assert not np.array_equal(stages[a][0][c][-1], stages[b][0][c][-1], equal_nan=True), (name, a, b, c)
    K.register_stages(name, stages)
    return K.stages(name, "device")


class Device:
    """a started tree with the list of the cases, the tracer and the held values of the five variables"""

    def __init__(self, name, kind, nu=0., forces=(F.BUOY,), zero_deposit=False):
        self.name, self.dim = name, K.spec(name)[0]
        self.st = device_stages(name) if not nu else None
        self.g, self.flags = start_tree(name, nu)
        self.P = K.particles(name, device_stages(name)[K.MOVE_BEFORE - 1].dt)
        P = self.P
        self.gkind, self.pkind, self.dep = KINDS[kind]
        self.pl = self.g.particulates(P.pos, P.ids, P.vel, P.mass, P.volume)
        self.pl.set_sort_interval(0)
        self.pl.set_forces(list(forces), (0., 0., 0.))
        self.sources = []
        self.upload(G.RAD, K.held(name, K.HELD_SALT["rad"]))
        for c in range(self.dim):
            self.upload(URELS[c], K.held(name, K.HELD_SALT["urel%d" % c]))
        shape = K.shapes(K.host_tree(name))
        self.upload(self.dep, [np.zeros(s) for s in shape] if zero_deposit else K.held(name, K.HELD_SALT["deposit"]))
        self.set_tracer()

    def upload(self, var, a):
        for l in range(self.g.depth + 1):
            self.g.upload(var, l, a[l])

    def set_tracer(self):
        self.upload(G.T0, K.tracer(self.name))       # the steps advect T0: every event reads the same values

    def source(self, fname, fields=True, deposit=True):
        text = None if fname is None else K.functions(self.dim)[fname][0]
        src = gfship.TreeParticulateSource(self.g, self.pl, self.gkind, text, {"T": G.T0})
        self.sources.append(src)
        if fields:
            src.set_fields(G.RAD, URELS[:self.dim], self.dep if deposit else None)
        return src

    def advance(self, e):
        """what comes between event e - 1 and event e"""
        if e == K.MOVE_BEFORE:
            self.pl.sort()
            self.pl.event()
            self.pl.sort()
        self.g.step()
        assert (self.g.t, self.g.dt) == (self.st[e].t, self.st[e].dt), (self.name, e)
        for c, u in enumerate(fluid(self.g, self.dim)):
            for l, a in enumerate(u):
                assert np.array_equal(a, self.st[e].u[c][l], equal_nan=True), (self.name, e, c, l)
        self.set_tracer()

    def close(self):
        for s in self.sources:
            s.destroy()
        self.pl.destroy()
        self.g.destroy()


def compare(dev, ev, what, deposit=True):
    g, dim, name = dev.g, dev.dim, dev.name
    pos, ids = dev.pl.download()
    assert np.array_equal(ids, ev.ids), what                  # on or off the list as the restatement says
    assert dev.pl.count() == len(ev.ids), what
    volume, mass = dev.pl.volumes(), dev.pl.particulate_state()[1]
    assert np.array_equal(volume, ev.volume), what
    assert np.array_equal(mass, ev.mass), what
    for q in dev.P.outside:                                   # the skipped particles are unchanged
        at = np.flatnonzero(ids == dev.P.ids[q])
        assert len(at) <= 1
        if len(at):
            assert volume[at[0]] == dev.P.volume[q] and mass[at[0]] == dev.P.mass[q], what
            assert np.array_equal(pos[at[0]], dev.P.pos[q]), what
    if deposit:
        for l, a in enumerate(levels(g, dev.dep)):
            assert np.array_equal(a, ev.deposit[l]), (what, "deposit", l)
    for c in range(dim):
        for l, a in enumerate(levels(g, URELS[c])):
            assert np.array_equal(a, ev.urel[c][l]), (what, "urel", c, l)
    was = K.held(name, K.HELD_SALT["rad"])
    nwritten = 0
    for l, a in enumerate(levels(g, G.RAD)):
        assert np.array_equal(a == was[l], ev.rad[l] == was[l]), (what, "the written cells of Rad", l)
        written = ev.rad[l] != was[l]
        nwritten += int(written.sum())
        if written.any():
            d = _ulps(a[written], ev.rad[l][written])
            print("%s level %d: Rad differs from glibc's by at most %d ulp" % (what, l, d.max()))
            assert d.max() <= POW_ULPS, (what, "Rad", l)
    assert nwritten > 20


# ---- the main comparison -------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", K.ALL)
def test_events_equal_the_restatement(name, kind):
    """every function on every tree for both kinds, after each of the three events.  No function of the cases calls
    libm or feels an ulp of Rad, so the sources, the volumes and the masses are equal bit for bit and Rad differs by
    the pow alone"""
    device_stages(name)
    for fname in K.FUNCTION_NAMES:
        dev = Device(name, kind)
        try:
            ref = K.reference_run(name, dev.pkind, fname, "device")
            src = dev.source(fname)
            for e in range(K.NEVENTS):
                if e > 0:
                    dev.advance(e)
                src.event()
                compare(dev, ref.events[e], (name, kind, fname, e))
                if e in K.SORT_AFTER:
                    dev.pl.sort()
            # the list is what the restatement says after the move; on trees with walls some particles left
            assert len(ref.events[-1].ids) <= len(dev.P.ids)
        finally:
            dev.close()


# ---- fields and NULL function ---------------------------------------------------------------------------

def test_no_fields_no_deposit_and_null_function():
    name = "square"
    dev = Device(name, "vol")
    try:
        ref = K.reference_run(name, PS.VOLUME, "tracer", "device")
        bare = dev.source("tracer", fields=False)
        bare.event()
        assert np.array_equal(dev.pl.volumes(), ref.events[0].volume)
        assert not np.array_equal(dev.pl.volumes(), dev.P.volume)
        for var, key in [(G.RAD, "rad"), (G.URELP, "urel0"), (G.VRELP, "urel1"), (G.VOLSRC, "deposit")]:
            for l, a in enumerate(levels(dev.g, var)):          # every field at -1 writes nothing
                assert np.array_equal(a, K.held(name, K.HELD_SALT[key])[l]), (var, l)
    finally:
        dev.close()
    dev = Device(name, "mass")
    try:
        ref = K.reference_run(name, PS.MASS, "tracer", "device")
        nodep = dev.source(None, deposit=False)                 # NULL: the constant 0
        nodep.event()
        assert np.array_equal(dev.pl.particulate_state()[1], dev.P.mass)
        assert np.array_equal(dev.pl.volumes(), dev.P.volume)
        for l, a in enumerate(levels(dev.g, G.DMDT)):           # the deposit alone is missing: it keeps what it held
            assert np.array_equal(a, K.held(name, K.HELD_SALT["deposit"])[l])
        for c in range(dev.dim):
            for l, a in enumerate(levels(dev.g, URELS[c])):
                assert np.array_equal(a, ref.events[0].urel[c][l])
    finally:
        dev.close()


# ---- downstream of a changed volume ----------------------------------------------------------------------

def _shifted_pow(steps):
    def pow_(x, y):
        r = math.pow(x, y)
        for _ in range(abs(steps)):
            r = math.nextafter(r, math.inf if steps > 0 else -math.inf)
        return r
    return pow_


FORCES = (F.DRAG, F.ADDEDMASS)


def _downstream_device(name, kind, event=True):
    dev = Device(name, kind, nu=NU, forces=FORCES)
    try:
        u, t, dt = fluid(dev.g, dev.dim), dev.g.t, dev.g.dt
        src = dev.source("tracer")
        if event:
            src.event()
        dev.pl.event()
        vel, mass, force = dev.pl.particulate_state()
        pos, ids = dev.pl.download()
        return (u, t, dt), (ids, pos, vel, mass, force, dev.pl.volumes())
    finally:
        dev.close()


def _downstream_reference(name, pkind, stage, steps, event=True):
    box = K.host_tree(name)
    dim, _refine, sides = K.spec(name)
    u, t, dt = stage
    P = K.particles(name, device_stages(name)[K.MOVE_BEFORE - 1].dt)
    plist = [F.Particulate(P.pos[q], P.ids[q], P.vel[q], P.mass[q], P.volume[q]) for q in range(len(P.ids))]
    text, fn, names = K.functions(dim)["tracer"]
    sim = F.Sim(box, sides, u, dt, viscosity=((lambda cell: NU), None, None), g=(0., 0., 0.), root=F.sqrt_root)
    objs = [F.ForceCoeff(k) for k in FORCES]
    TF.read_forces(sim, objs)
    changed = set()
    if event:
        before = [p.volume for p in plist]
        PS.event(box, pkind, plist, [box.field(a) for a in u], dt, t, fn, K.new_fields(name, box),
                 {"T": box.field(K.tracer(name))}, _shifted_pow(steps))
        changed = set(p.id for p, v in zip(plist, before) if pkind == PS.VOLUME and box.locate(p.pos) is not None)
    pow0 = _shifted_pow(steps)
    diameter = F._diameter
    # a volume event recomputes the diameter of every particle with a leaf with the device's pow; the others, and
    # every particle of a list no volume event ran on, keep the diameter of the host
    F._diameter = lambda p: 2.*pow0(3.0*p.volume/4.0/math.pi, 1./3.) if p.id in changed else diameter(p)
    try:
        plist = TF.list_event(sim, plist, objs)
    finally:
        F._diameter = diameter
    return (np.array([p.id for p in plist], dtype=np.uint32), np.array([p.pos for p in plist]),
            np.array([p.vel for p in plist]), np.array([p.mass for p in plist]), np.array([p.force for p in plist]),
            np.array([p.volume for p in plist]))


@pytest.mark.parametrize("name", ["graded", "cube"])
def test_a_mass_event_then_the_list_event_is_exact(name):
    stage, got = _downstream_device(name, "mass")
    want = _downstream_reference(name, PS.MASS, stage, 0)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert np.abs(got[4]).max() > 0.


@pytest.mark.parametrize("name", ["graded", "cube"])
def test_a_volume_event_then_the_list_event_lies_in_the_hull_of_the_bound(name):
    """the rule of the box: the restatement with its radius function (Rad, and the diameter of a changed volume)
    moved down and up by POW_ULPS; every device value lies in the hull of those results and the unmoved one, widened
    by one ulp"""
    stage, got = _downstream_device(name, "vol")
    runs = [_downstream_reference(name, PS.VOLUME, stage, s) for s in (-POW_ULPS, 0, POW_ULPS)]
    assert np.array_equal(got[0], runs[1][0])
    for q in range(1, len(got)):
        stack = np.stack([r[q] for r in runs])
        lo = np.nextafter(stack.min(axis=0), -np.inf)
        hi = np.nextafter(stack.max(axis=0), np.inf)
        assert ((got[q] >= lo) & (got[q] <= hi)).all(), (q, int(((got[q] < lo) | (got[q] > hi)).sum()))
    assert np.abs(got[4]).max() > 0.


@pytest.mark.parametrize("name", ["graded", "cube"])
def test_a_list_with_a_source_but_no_event_is_unchanged(name):
    stage, got = _downstream_device(name, "vol", event=False)
    want = _downstream_reference(name, PS.VOLUME, stage, 0, event=False)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


# ---- a uniform tree against the box -----------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name,dim", [("uniform2", 2), ("uniform3d", 3)])
def test_uniform_tree_equals_uniform_box(name, dim, kind):
    level = K.UNIFORM[dim]
    st = device_stages(name)
    inner = (slice(1, -1),)*dim
    for fname in ("tracer", "xyt"):
        dev = Device(name, kind, zero_deposit=True)
        gd = gfship.Domain(dim, level, BK.SIDES["periodic"])
        gs = gfship.Simulation(gd)
        P = dev.P
        gpl = gfship.ParticleList(gs, P.pos, P.ids)
        bsrc = None
        try:
            gpl.set_sort_interval(0)
            gpl.set_particulate(P.vel, P.mass, P.volume)
            gpl.set_forces([F.BUOY], (0., 0., 0.))
            Tv = gd.variable()
            Tv.upload(K.tracer(name)[level])
            bvars = {}
            for key in ["rad"] + ["urel%d" % c for c in range(dim)]:
                bvars[key] = gd.variable()
                bvars[key].upload(K.held(name, K.HELD_SALT[key])[level])
            bdep = gd.variable()
            bdep.fill(0.)
            bsrc = gfship.ParticulateSource(gpl, dev.gkind, K.functions(dim)[fname][0], {"T": Tv})
            bsrc.set_fields(bvars["rad"], [bvars["urel%d" % c] for c in range(dim)], bdep)
            src = dev.source(fname)
            for e in range(K.NEVENTS):
                if e > 0:
                    if e == K.MOVE_BEFORE:
                        gs.advection_params.dt = st[e - 1].dt
                        gpl.sort()
                        gpl.event()
                        gpl.sort()
                    dev.advance(e)
                for c in range(dim):
                    gs.u[c].upload(st[e].u[c][level])
                gs.restart(st[e].t, e)
                gs.advection_params.dt = st[e].dt
                src.event()
                bsrc.event()
                what = (name, kind, fname, e)
                assert np.array_equal(dev.pl.download()[1], gpl.download()[1]), what
                assert np.array_equal(dev.pl.volumes(), gpl.volumes()), what
                assert np.array_equal(dev.pl.particulate_state()[1], gpl.particulate_state()[1]), what
                for c in range(dim):
                    assert np.array_equal(dev.g.download(URELS[c], level)[inner], bvars["urel%d" % c].download()[inner]), what
                assert np.array_equal(dev.g.download(G.RAD, level)[inner], bvars["rad"].download()[inner]), what
                if e == 0:
                    assert np.array_equal(dev.g.download(dev.dep, level)[inner], bdep.download()[inner]), what
                    assert dev.g.download(dev.dep, level)[inner].max() > 0.
                if e in K.SORT_AFTER:
                    dev.pl.sort()
                    gpl.sort()
        finally:
            if bsrc is not None:
                bsrc.destroy()
            gpl.destroy()
            gs.destroy()
            gd.destroy()
            dev.close()


# ---- refusals and lifetimes -------------------------------------------------------------------------------

def test_refusals():
    name = "square"
    device_stages(name)
    dev = Device(name, "vol")
    P = dev.P
    try:
        g, pl = dev.g, dev.pl
        # a list of a box, and the box's calls on a list and a handle of a tree
        gd = gfship.Domain(2, 3, BK.SIDES["periodic"])
        gs = gfship.Simulation(gd)
        bpl = gfship.ParticleList(gs, P.pos, P.ids)
        try:
            bpl.set_particulate(P.vel, P.mass, P.volume)
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*tree"):
                gfship.TreeParticulateSource(g, bpl, gfship.SOURCE_VOLUME, "1.")
        finally:
            bpl.destroy()
            gs.destroy()
            gd.destroy()
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gfship.ParticulateSource(pl, gfship.SOURCE_VOLUME, "1.")
        tracers = g.particles(P.pos, P.ids)
        try:
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*particulates"):
                gfship.TreeParticulateSource(g, tracers, gfship.SOURCE_MASS, "1.")
        finally:
            tracers.destroy()
        # the table: what the walk writes, the built-in names
        for var in (G.RAD, G.VOLSRC, G.DMDT, G.URELP):
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*writes"):
                gfship.TreeParticulateSource(g, pl, gfship.SOURCE_VOLUME, "2.*Q", {"Q": var})
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            gfship.TreeParticulateSource(g, pl, gfship.SOURCE_MASS, "Rad", {"Rad": G.T0})
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            gfship.TreeParticulateSource(g, pl, gfship.SOURCE_MASS, "Q", {"Q": 99})
        # a variable the tree does not have: the tree has added one tracer, T0, and no T1; no W on a quadtree
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*no variable"):
            gfship.TreeParticulateSource(g, pl, gfship.SOURCE_MASS, "Q", {"Q": G.T1})
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*no variable"):
            gfship.TreeParticulateSource(g, pl, gfship.SOURCE_MASS, "Q", {"Q": G.VF})      # nothing has allocated it
        # a text that does not compile: the compiler's message is in gfship_last_error
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile(.|\n)*Q"):
            gfship.TreeParticulateSource(g, pl, gfship.SOURCE_MASS, "2.*Q")
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile"):
            gfship.TreeParticulateSource(g, pl, gfship.SOURCE_MASS, "2.*Wrelp")      # no Wrelp on a quadtree
        # WRELP on a quadtree
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*WRELP"):
            g.upload(G.WRELP, 0, np.zeros((3, 3)))
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            g.download(G.WRELP, 0)
        vol = dev.source("constant", fields=False)
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*WRELP"):
            vol.set_fields(G.RAD, [G.URELP, G.VRELP, G.WRELP], G.VOLSRC)
        # the deposit of the other kind, a variable in the wrong place
        mass = gfship.TreeParticulateSource(g, pl, gfship.SOURCE_MASS, "1e-12")
        dev.sources.append(mass)
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            mass.set_fields(G.RAD, [G.URELP, G.VRELP], G.VOLSRC)
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            vol.set_fields(G.RAD, [G.URELP, G.VRELP], G.DMDT)
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            vol.set_fields(G.URELP, [G.RAD, G.VRELP], G.VOLSRC)
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            vol.set_fields(G.T0, [], None)
        mass.set_fields(G.RAD, [G.URELP, G.VRELP], G.DMDT)
        # the box's set_fields on a tree handle
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*tree"):
            gfship.ParticulateSource.set_fields(vol, None, (), None)
    finally:
        dev.close()


def test_download_before_anything_allocated_the_variables():
    g, _ = make_tree("square")
    try:
        for var in (G.RAD, G.URELP, G.VRELP, G.VOLSRC, G.DMDT):
            with pytest.raises(gfship.GfshipError, match="gfship error -1"):
                g.download(var, 0)
        g.upload(G.RAD, 1, np.full((4, 4), 0.25))           # an upload is a call that needs it: zeroed elsewhere
        assert np.array_equal(g.download(G.RAD, 1), np.full((4, 4), 0.25))
        assert not g.download(G.RAD, 2).any() and not g.download(G.RAD, 0).any()
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            g.download(G.DMDT, 0)
        out, inside = g.interpolate(G.RAD, np.zeros((1, 3)))
        assert inside.all() and out[0] == 0.
    finally:
        g.destroy()
