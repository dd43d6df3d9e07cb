"""Droplets on refined trees on the device (Tree.tag_droplets, Tree.remove_droplets, gfship.TreeDropletToParticle)
against the literal restatement of tests/tree_droplets_reference.py on the cases of tests/tree_droplets_cases.py.

Bit for bit (array_equal), every case twice: the tags and their number; the list after each of two events in a row
(positions, velocities, mass, volume, ids, order, force, pos_old, count, slots, idlast); c on every level -- the
leaves, the ghost cells by its conditions, the cells with children untouched --; the info; remove_droplets.  On the
uniform trees the tags are those of gfship_tag_droplets on a box with the same field.  No libm call is involved in any
of these: h^dim is a power of two.  The diameter and rb of a new particle are values of the device's pow: the event
with drag and the event of a GfsSourceParticulate that follow are compared by the POW_ULPS rule of DESIGN.md 11.35
(tests/test_gpu_tree_feed_particle.py: the restatement with the pow of the new particles moved by up to POW_ULPS,
every device value inside the hull widened by one ulp, the sums of a leaf between the sums of the ends) and nothing
wider; what does not pass through pow stays bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import droplets_cases as BC
import forces_reference as F
import gfship
import tree_droplets_cases as C
import tree_droplets_reference as TD
import tree_forces_reference as TF
import tree_two_way_cases as TWC
import tree_two_way_reference as TW
from test_gpu_particulate_sources import POW_ULPS, _shifted_pow
from test_gpu_tree_particulate_sources import fluid, levels, start_tree

pytestmark = pytest.mark.gpu

G = gfship.Tree
UVARS = [G.U, G.V, G.W]
FVARS = [G.FX, G.FY, G.FZ]
DRAG = F.DRAG
NU = 1e-2


class Device:
    """a tree at rest in the velocity of the cases, with the tracers T0 (the variable c) and T1"""

    def __init__(self, name):
        self.name = name
        self.dim, refine, self.sides = C.spec(name)
        self.box = C.host_tree(name)
        self.g = gfship.Tree(refine, self.dim, sides=self.sides)
        for l in range(self.g.depth + 1):
            assert np.array_equal(self.g.flags(l), np.array(self.box.flags(l), dtype=np.uint8)), (name, l)
        assert self.g.add_tracer() == G.T0 and self.g.add_tracer() == G.T1
        for c in range(self.dim):
            self.upload(UVARS[c], C.velocity(name)[c])
        self.owned, self.pl = [], None

    def upload(self, var, arrays):
        for l, a in enumerate(arrays):
            self.g.upload(var, l, a)

    def download(self, var):
        return levels(self.g, var)

    def load(self, case):
        """the variables of a case and a fresh list"""
        self.release()
        self.upload(G.T0, case.T)
        self.upload(G.T1, case.S)
        pos, ids, vel, mass, volume = C.particles(self.dim)
        self.pl = self.g.particulates(pos, ids, vel, mass, volume)
        self.pl.set_sort_interval(0)
        self.g.set_idlast(self.pl, C.IDLAST0)
        d = gfship.TreeDropletToParticle(self.g, self.pl, G.T0, case.min, case.reset, 1000., case.function,
                                         {"T": G.T0, "S": G.T1})
        self.owned.append(d.close)
        return d

    def state(self):
        pl = self.pl
        pos, ids = pl.download()
        vel, mass, force = pl.particulate_state()
        return {"ids": ids, "pos": pos, "old": pl.download_old(), "vel": vel, "mass": mass, "volume": pl.volumes(),
                "force": force, "idlast": self.g.idlast(pl)}

    def release(self):
        for close in reversed(self.owned):
            close()
        self.owned = []
        if self.pl is not None:
            self.pl.destroy()
            self.pl = None

    def close(self):
        self.release()
        self.g.destroy()


def _assert_state(got, want, what):
    assert len(got["ids"]) == len(want["ids"]), what
    for name in ("ids", "pos", "old", "vel", "mass", "volume", "force"):
        assert np.array_equal(got[name], want[name]), (what, name)
    assert got["idlast"] == want["idlast"], what


def _leaf_values(box, arrays):
    f = box.field(arrays)
    return np.array([box.value(c, f) for c in box.leaves])


def _expected(box, sides, uploaded, leaves):
    """a variable after an event that ran: what was uploaded on every level, the leaves of the restatement, and the
    ghost leaves by gfs_domain_bc (the periodic image, or the cell the ghost touches: the default GfsBc)"""
    out = [np.array(a) for a in uploaded]
    for cell in box.leaves:
        out[cell.level][C._at(box, cell)] = leaves[cell.level][C._at(box, cell)]
    for gh in box.ghosts:
        n, a = 1 << gh.level, gh.tree//2
        ijk = list(gh.ijk)
        if sides[gh.tree] == C.P:
            ijk[a] = 1 if ijk[a] == n + 1 else n
        else:
            ijk[a] = n if ijk[a] == n + 1 else 1
        src = (ijk[1], ijk[0]) if box.dim == 2 else (ijk[2], ijk[1], ijk[0])
        dst = (gh.ijk[1], gh.ijk[0]) if box.dim == 2 else (gh.ijk[2], gh.ijk[1], gh.ijk[0])
        out[gh.level][dst] = out[gh.level][src]
    return out


def _assert_variable(dev, var, want, what):
    got = dev.download(var)
    for l, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, "level", l)


def _events(dev, case, ref, what):
    """two events in a row on one list, each against the restatement; returns the states"""
    d2p = dev.load(case)
    slots, states = 3, []
    uploaded = case.T
    for e in range(2):
        info, _drops, T, want = ref.events[e]
        got = d2p.event()
        assert got == tuple(info), (what, e)
        ran = info[0] > 0 and -case.min < info[0]
        if ran:
            slots += info[0]          # every droplet of an event that runs takes a slot, dead or alive
        assert gfship.lib().gfship_particles_slots(dev.pl.ptr) == slots, (what, e)
        state = dev.state()
        _assert_state(state, want, (what, e))
        assert dev.pl.count() == len(want["ids"]), (what, e)
        if dev.dim == 2:
            assert not state["vel"][3:, 2].any() and not state["pos"][3:, 2].any()
        if ran:
            uploaded = _expected(dev.box, dev.sides, uploaded, T)
        _assert_variable(dev, G.T0, uploaded, (what, e))
        _assert_variable(dev, G.T1, case.S, (what, e, "S"))
        states.append((state, dev.download(G.T0)))
    return states


@pytest.mark.parametrize("name", C.NAMES)
def test_tags_equal_the_restatement(name):
    dev = Device(name)
    try:
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            dev.g.download(G.TAG, 0)                  # nothing has needed the tags yet
        for cname, case in C.cases(name).items():
            ref = C.reference_run(name, cname)
            dev.upload(G.T0, case.T if case.mask() is None else case.mask())
            for again in range(2):
                n = dev.g.tag_droplets(G.T0)
                assert n == ref.tags.n, (cname, again)
                tags = dev.download(G.TAG)
                assert np.array_equal(_leaf_values(dev.box, tags), ref.leaf_tags.astype(float)), (cname, again)
                # the tag of a cell with children is never written (gfs_cell_reset, :3741, left it 0)
                for cell in TD.interior_cells(dev.box):
                    if not dev.box.is_leaf(cell):
                        assert tags[cell.level][C._at(dev.box, cell)] == 0., cname
    finally:
        dev.close()


@pytest.mark.parametrize("name", C.NAMES)
def test_events_equal_the_restatement(name):
    """every case: two events in a row on one list (the second on the reset variable; the list grows past the three
    slots it was created with), then the whole case again: bit for bit the same"""
    dev = Device(name)
    try:
        for cname, case in C.cases(name).items():
            ref = C.reference_run(name, cname)
            first = _events(dev, case, ref, cname)
            again = _events(dev, case, ref, cname + " again")
            for (s0, t0), (s1, t1) in zip(first, again):
                _assert_state(s0, s1, (cname, "twice"))
                for a, b in zip(t0, t1):
                    assert np.array_equal(a, b), (cname, "twice")
    finally:
        dev.close()


@pytest.mark.parametrize("name", C.NAMES)
def test_remove_droplets_equals_the_restatement(name):
    dev = Device(name)
    try:
        for cname, case in C.cases(name).items():
            if case.function is not None:
                continue
            ref = C.reference_run(name, cname)
            held = [s + 0.5 for s in case.S]
            for again in range(2):
                dev.upload(G.T0, case.T)
                dev.upload(G.T1, held)
                dev.g.remove_droplets(G.T0, G.T1, case.min, -3.)
                ran = ref.remove_info[0] > 0 and -case.min < ref.remove_info[0]
                want = _expected(dev.box, dev.sides, held, ref.removed) if ran else held
                _assert_variable(dev, G.T1, want, (cname, again))
                _assert_variable(dev, G.T0, case.T, (cname, again, "c"))
        # c and v the same variable
        case = C.cases(name)["blobs"]
        v = dev.box.field([np.array(a) for a in case.T])
        info = TD.remove_droplets(dev.box, dev.sides, dev.box.field([np.array(a) for a in case.T]), v, 5, 0.)
        dev.upload(G.T0, case.T)
        dev.g.remove_droplets(G.T0, G.T0, 5, 0.)
        assert info[0] > 0
        _assert_variable(dev, G.T0, _expected(dev.box, dev.sides, case.T, [np.array(a) for a in v]), "in place")
    finally:
        dev.close()


@pytest.mark.parametrize("name", tuple(C.UNIFORM))
def test_uniform_tree_equals_uniform_box(name):
    """on a uniform tree the tags are those of gfship_tag_droplets on the box of that level with the same field"""
    dev = Device(name)
    level = C.UNIFORM[name]
    gd = gfship.Domain(dev.dim, level, dev.sides)
    try:
        Tv, tag = gd.variable(), gd.variable()
        for cname, case in C.cases(name).items():
            mask = case.T if case.mask() is None else case.mask()
            dev.upload(G.T0, mask)
            Tv.upload(mask[level])
            n, nb = dev.g.tag_droplets(G.T0), gd.tag_droplets(Tv, tag)
            assert n == nb, cname
            inner = (slice(1, -1),)*dev.dim
            assert np.array_equal(dev.g.download(G.TAG, level)[inner], tag.download()[inner]), cname
    finally:
        gd.destroy()
        dev.close()


def test_the_situations_on_the_device():
    """the named situations of the issue, with what must come out of each"""
    want = {"pair_coarse_first": 2, "pair_fine_first": 1, "chain": 1, "two_into_one": 2, "periodic_oneway": 1}
    met = set()
    for name in ("graded", "cube"):
        dev = Device(name)
        try:
            for key, n in want.items():
                if key in C.cases(name):
                    dev.upload(G.T0, C.cases(name)[key].T)
                    assert dev.g.tag_droplets(G.T0) == n == C.reference_run(name, key).tags.n, (name, key)
                    met.add(key)
        finally:
            dev.close()
    assert met == set(want)


def test_timing_entry_runs():
    dev = Device("big3")
    try:
        dev.upload(G.T0, C.cases("big3")["random2"].T)
        assert dev.g.time_tag_droplets(G.T0, 3) > 0.
        assert dev.g.tag_droplets(G.T0) == C.reference_run("big3", "random2").tags.n
    finally:
        dev.close()


# ---- downstream: the diameter and rb of the new particles ---------------------------------------------------

SPREAD_TEXT = "(1. - 1e-4*(x*x + y*y + z*z))"
DOWNSTREAM = (("square", "random1"), ("cube", "random1"))


def _spread_kernel(x, y, z, t):
    return (1. - 1e-4*(x*x + y*y + z*z))


def _downstream_reference(name, cname, stage, steps_dia, steps_rb):
    """one event of the case on the device's own fluid, then one gfs_particle_list_event with drag and the event of a
    GfsSourceParticulate, in the restatements, with the pow of the new particles moved by `steps_dia' ulps in their
    diameter and by `steps_rb' ulps in their rb"""
    box = C.host_tree(name)
    dim, _refine, sides = C.spec(name)
    case = C.cases(name)[cname]
    u, t, dt = stage
    pl = C.particle_list(dim)
    uf = [box.field(v) for v in u]
    info, _drops = TD.event(box, sides, pl, box.field([np.array(a) for a in case.T]), uf, case.min, case.reset)
    out = {"info": info, "fed": BC.list_state(pl)}
    plist = pl.plist
    new_ids = {p.id for p in plist if p.id > C.IDLAST0}
    new_volumes = {p.volume for p in plist if p.id in new_ids}
    assert not new_volumes & {p.volume for p in plist if p.id not in new_ids}
    pow_dia, pow_rb = _shifted_pow(steps_dia), _shifted_pow(steps_rb)
    sim = F.Sim(box, sides, u, dt, viscosity=((lambda cell: NU), None, None), root=F.sqrt_root)
    objs = [F.ForceCoeff(DRAG)]
    TF.read_forces(sim, objs)
    diameter, distance = F._diameter, TW.normalized_distance

    def normalized_distance(dim_, centre, p, volume):
        if volume not in new_volumes:
            return distance(dim_, centre, p, volume)
        rb = pow_rb(3.*volume/(4.*math.pi), 1./3.)        # distance_normalization, :2091
        return ((centre[0] - p[0])/rb, (centre[1] - p[1])/rb, (0. - p[2])/rb if dim_ == 3 else 0.)
    F._diameter = lambda p: 2.*pow_dia(3.0*p.volume/4.0/math.pi, 1./3.) if p.id in new_ids else diameter(p)
    TW.normalized_distance = normalized_distance
    try:
        plist = TF.list_event(sim, plist, objs)
        out["ids"] = np.array([p.id for p in plist], dtype=np.uint32)
        for key in ("pos", "pos_old", "vel", "force"):
            out[key] = np.array([getattr(p, key) for p in plist])
        TW.forces_on_fluid(sim, plist, objs)
        out["onfluid"] = np.array([p.force for p in plist])
        rkernel = 1.5*TWC.h_fine(box)
        parts = []
        for q in range(len(plist)):
            Fv, _corr, _reached = TW.spread(box, plist[q:q + 1], rkernel, _spread_kernel, t)
            parts.append(np.stack([_leaf_values(box, Fv[c]) for c in range(dim)]))
        out["F_parts"] = np.stack(parts)
    finally:
        F._diameter, TW.normalized_distance = diameter, distance
    return out


@pytest.mark.parametrize("name,cname", DOWNSTREAM)
def test_a_grown_list_behaves_as_one_given_at_creation(name, cname):
    """the rule of tests/test_gpu_tree_feed_particle.py: a quantity of one particle lies in the hull of the
    restatement over the corners and the centre of [-POW_ULPS, POW_ULPS]^2, widened by one ulp; a quantity of a leaf is
    a sum over its particles in list order and lies between the sums of the ends, widened by the rounding of a sum of
    n terms; the particles of the list as created and the leaves no new particle reaches stay bit for bit"""
    dim = C.spec(name)[0]
    box = C.host_tree(name)
    case = C.cases(name)[cname]
    g, _flags = start_tree(name, NU)
    owned = []
    try:
        assert g.add_tracer() == G.T1
        stage = (fluid(g, dim), g.t, g.dt)
        corners = [(a, b) for a in (-POW_ULPS, 0, POW_ULPS) for b in (-POW_ULPS, 0, POW_ULPS)]
        runs = [_downstream_reference(name, cname, stage, a, b) for a, b in corners]
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
            assert not bad.any(), (key, int(bad.sum()))
            same = (stack.min(axis=0) == stack.max(axis=0)).all(axis=0)
            serial = np.zeros_like(lo)
            for part in exact[key]:
                serial = serial + part
            assert same.any() and np.array_equal(got[same], serial[same]), key

        for l, a in enumerate(case.T):
            g.upload(G.T0, l, a)
        pos, ids, vel, mass, volume = C.particles(dim)
        pl = g.particulates(pos, ids, vel, mass, volume)
        owned.append(pl.destroy)
        pl.set_sort_interval(0)
        pl.set_forces([DRAG])
        g.set_idlast(pl, C.IDLAST0)
        d2p = gfship.TreeDropletToParticle(g, pl, G.T0, case.min, case.reset)
        owned.append(d2p.close)
        assert d2p.event() == tuple(exact["info"]) and exact["info"][2] >= 2

        def state():
            p, i = pl.download()
            v, m, f = pl.particulate_state()
            return {"ids": i, "pos": p, "old": pl.download_old(), "vel": v, "mass": m, "volume": pl.volumes(),
                    "force": f, "idlast": g.idlast(pl)}
        _assert_state(state(), exact["fed"], "converted")
        old = exact["ids"] <= C.IDLAST0
        pl.event()                                            # drag reads the diameter of a new particle
        got = state()
        assert np.array_equal(got["ids"], exact["ids"])
        assert np.array_equal(got["old"][:, :dim], exact["pos_old"][:, :dim])
        for key in ("pos", "vel", "force"):
            in_hull(got[key], key)
            assert np.array_equal(got[key][old][:, :dim], exact[key][old][:, :dim]), key
        assert np.abs(got["force"][~old][:, :dim]).max() > 0.
        g.set_kernel(pl, 1.5*TWC.h_fine(box), SPREAD_TEXT)    # the spreading reads rb of every particle
        g.source_particulate_event(pl)
        in_hull(pl.particulate_state()[2], "onfluid")
        spread = np.stack([_leaf_values(box, levels(g, FVARS[c])) for c in range(dim)])
        in_hull_of_sums(spread, "F_parts")
        assert np.abs(spread).max() > 0. and np.abs(exact["F_parts"][~old]).max() > 0.
    finally:
        for close in reversed(owned):
            close()
        g.destroy()


# ---- refusals and lifetimes -------------------------------------------------------------------------------

def _create(pl, c, function, names, numbers):
    p = ctypes.c_void_p()
    n = len(names)
    r = gfship.lib().gfship_tree_droplet_to_particle_create(
        ctypes.byref(p), pl.ptr, c, 6, 0., 1., None if function is None else function.encode(), n,
        (ctypes.c_char_p*max(n, 1))(*[s.encode() for s in names]), (ctypes.c_int*max(n, 1))(*numbers))
    if r == 0:
        gfship.lib().gfship_droplet_to_particle_destroy(p)
    return r


def test_refusals():
    dev = Device("square")
    pos, ids, vel, mass, volume = C.particles(2)
    try:
        g = dev.g
        d = dev.load(C.cases("square")["blobs"])
        pl = dev.pl
        # a list of tracers of a tree, a list of a box
        tracers = g.particles(pos, ids)
        dev.owned.append(tracers.destroy)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*particulates"):
            gfship.TreeDropletToParticle(g, tracers, G.T0)
        gd = gfship.Domain(2, 3, BC.SIDES["periodic"])
        gs = gfship.Simulation(gd)
        bpl = gfship.ParticleList(gs, pos, ids)
        try:
            bpl.set_particulate(vel, mass, volume)
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*tree"):
                gfship.TreeDropletToParticle(g, bpl, G.T0)
        finally:
            bpl.destroy()
            gs.destroy()
            gd.destroy()
        # the box entry keeps refusing a list of a tree
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gfship.DropletToParticle(pl, type("V", (), {"h": 0})())
        # the table: a reserved name, a name twice, no C identifier
        for reserved in ("x", "y", "z", "t"):
            assert _create(pl, G.T0, reserved, [reserved], [G.T1]) == -1
        assert _create(pl, G.T0, "Q", ["Q", "Q"], [G.T0, G.T1]) == -1
        assert _create(pl, G.T0, "Q", ["2Q"], [G.T1]) == -1
        assert _create(pl, G.T0, "Q - R", ["Q", "R"], [G.T0, G.T1]) == 0
        # a variable the tree does not have now; no W on a quadtree; the tags themselves
        for var in (G.VF, 99, -1, G.W, G.TAG):
            assert _create(pl, var, None, [], []) == -1, var
            assert _create(pl, G.T0, "Q", ["Q"], [var]) == -1, var
            with pytest.raises(gfship.GfshipError, match="gfship error -1.*no variable"):
                g.tag_droplets(var) if var != G.W else g.remove_droplets(G.T0, G.VF, 3)
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*no variable"):
            g.remove_droplets(G.T0, 99, 3)
        # a text that does not compile
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile") as err:
            gfship.TreeDropletToParticle(g, pl, G.T0, function="T - Q", variables={"T": G.T0})
        assert "Q" in str(err.value)
        # nothing above changed the list; a closed object is closed once, and the list outlives it
        ref = C.reference_run("square", "blobs")
        assert d.event() == tuple(ref.events[0][0])
        d.close()
        d.close()
        assert d.ptr is None and pl.count() == len(ref.events[0][3]["ids"])
    finally:
        dev.close()
