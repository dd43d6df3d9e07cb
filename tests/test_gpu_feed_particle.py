"""GfsFeedParticle on the device (gfship.FeedParticle, ParticleList.idlast) against the restatement of
tests/feed_particle_reference.py on the runs of tests/feed_particle_cases.py.

Bit for bit (array_equal): positions, ids, the download order, velocities, mass, volume, force, pos_old, the
count and idlast after every event -- no libm call is involved in any of them.  The diameter and rb of a new
particle are values of the device's pow: what is downstream of them (an event with drag, the spreading of
GfsSourceParticulate, Rad of a mass source) is compared within the POW_ULPS that
tests/test_gpu_particulate_sources.py measures and justifies for the same expression, by the method of that
file: the restatement with the pow of the new particles moved down and up by POW_ULPS, every device value inside
the hull of the three results widened by one ulp.  Whatever does not pass through pow stays bit for bit."""
import math
import os
import subprocess

import numpy as np
import pytest

import feed_particle_cases as C
import feed_particle_reference as FP
import forces_reference as FR
import gfship
import particulate_sources_cases as K
import particulate_sources_reference as PS
import sampler_cases as SK
import two_way_reference as TW
from conftest import ROOT
from test_gpu_particulate_sources import POW_ULPS, _interior, _shifted_pow, _ulps

pytestmark = pytest.mark.gpu

DRAG, BUOY = FR.DRAG, FR.BUOY
VISCOSITY, GRAVITY, DT = 1e-2, (0., -0.5, 0.), 2.**-6


class Device:
    """a simulation with the list of a case (drag and buoyancy, idlast = IDLAST0) and the tracer T"""

    def __init__(self, dim, level, sides_name):
        self.dim, self.level = dim, level
        self.gd = gfship.Domain(dim, level, C.SIDES[sides_name])
        self.gs = gfship.Simulation(self.gd)
        for c in range(dim):
            self.gs.set_viscosity(c, VISCOSITY)
        self.set_event(0)
        pos, ids, vel, mass, volume = K.particles(dim, level, sides_name)
        self.T = self.gd.variable()
        self.T.upload(K.tracer(dim, level))
        self.gpl = gfship.ParticleList(self.gs, pos, ids)
        self.gpl.set_sort_interval(0)
        self.gpl.set_particulate(vel, mass, volume)
        self.gpl.set_forces([DRAG, BUOY], GRAVITY)
        self.gpl.idlast = C.IDLAST0
        self.owned = []

    def feed(self, fname):
        mass, volume = C.FUNCTIONS[fname][0]
        f = gfship.FeedParticle(self.gpl, mass, volume, {"T": self.T})
        self.owned.append(f.close)
        return f

    def set_event(self, e):
        for c, a in enumerate(C.velocity(self.dim, self.level, e)):
            self.gs.u[c].upload(a)
        self.gs.restart(C.event_time(e), e)
        self.gs.advection_params.dt = DT

    def state(self):
        pos, ids = self.gpl.download()
        vel, mass, force = self.gpl.particulate_state()
        return C.State(pos, ids, self.gpl.download_old(), vel, mass, self.gpl.volumes(), force, self.gpl.idlast, ())

    def close(self):
        for close in self.owned:
            close()
        self.gpl.destroy()
        self.gs.destroy()
        self.gd.destroy()


def _assert_state(got, want, what):
    assert len(got.ids) == len(want.ids), what
    for name in ("ids", "pos", "old", "vel", "mass", "volume", "force"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), (what, name)
    assert got.idlast == want.idlast, what


# ---- the events, bit for bit ------------------------------------------------------------------------------

@pytest.mark.parametrize("sides_name", C.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", C.BOXES)
def test_events_equal_the_restatement(dim, level, sides_name):
    """0, 1, 70, 300 and 3000 candidates in a row on one list, for every function: the second event starts from
    the idlast of the first, the third makes the arrays of the list grow (40 slots at creation), the last spans
    twelve blocks"""
    for fname in C.FUNCTIONS:
        ref = C.reference_run(dim, level, sides_name, fname)
        dev = Device(dim, level, sides_name)
        try:
            feed = dev.feed(fname)
            assert dev.gpl.idlast == C.IDLAST0
            slots = K.NPART
            for e, count in enumerate(C.COUNTS):
                dev.set_event(e)
                feed.event(C.candidates(dim, level, e))
                slots += count
                assert gfship.lib().gfship_particles_slots(dev.gpl.ptr) == slots
                got = dev.state()
                _assert_state(got, ref[e], (fname, e))
                assert dev.gpl.count() == len(ref[e].ids)
                if dim == 2:
                    assert not got.vel[K.NPART:, 2].any()
            # the storage order changes nothing of the list
            dev.gpl.sort()
            _assert_state(dev.state(), ref[-1], (fname, "sorted"))
        finally:
            dev.close()


def test_a_burst_whose_block_counts_take_two_rounds_of_the_scan():
    """more than 256 blocks of 256 candidates: feed_scan_kernel carries its sum from one round to the next"""
    dim, level, sides_name, fname = 2, 3, "closed", "block"
    assert C.BURST > 256*256
    want = C.burst_reference(dim, level, sides_name, fname)
    assert want.idlast - C.IDLAST0 > 256*64     # accepted candidates in both rounds
    dev = Device(dim, level, sides_name)
    try:
        feed = dev.feed(fname)
        dev.set_event(0)
        feed.event(C.burst_candidates(dim))
        _assert_state(dev.state(), want, "burst")
        assert dev.gpl.count() == len(want.ids)
    finally:
        dev.close()


def test_the_ids_do_not_depend_on_the_run():
    dim, level, sides_name, fname = 3, 3, "closed", "tracer"
    runs = []
    for _ in range(2):
        dev = Device(dim, level, sides_name)
        try:
            feed = dev.feed(fname)
            dev.set_event(4)
            feed.event(C.candidates(dim, level, 4))
            runs.append(dev.state())
        finally:
            dev.close()
    _assert_state(runs[0], runs[1], "twice")


def test_idlast_of_any_list_of_a_box_and_the_defaults():
    dim, level = 2, 3
    dev = Device(dim, level, "periodic")
    pos, ids = K.particles(dim, level, "periodic")[:2]
    tracers = gfship.ParticleList(dev.gs, pos, ids)
    try:
        assert tracers.idlast == 0                        # gfs_particle_list_init
        tracers.idlast = 17
        assert tracers.idlast == 17 and dev.gpl.idlast == C.IDLAST0
        # gfs_feed_particle_init: no mass, nothing is fed, and no id is taken
        nothing = gfship.FeedParticle(dev.gpl)
        dev.owned.append(nothing.close)
        nothing.event(C.candidates(dim, level, 2))
        assert dev.gpl.count() == K.NPART and dev.gpl.idlast == C.IDLAST0
        # Rad is no variable of these functions unless the table says so
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile"):
            gfship.FeedParticle(dev.gpl, "Rad", "1e-4")
        rad = gfship.FeedParticle(dev.gpl, "1e-3*Rad", "1e-4", {"Rad": dev.T})
        dev.owned.append(rad.close)
        rad.event(np.array([[0.1, 0.2, 0.]]))
        assert dev.gpl.count() == K.NPART + 1 and dev.gpl.idlast == C.IDLAST0 + 1
        assert dev.gpl.download()[1][-1] == C.IDLAST0 + 1
    finally:
        tracers.destroy()
        dev.close()


# ---- downstream of a feed: dia, rb and orig of the newcomers ----------------------------------------------

FED_EVENTS = (1, 2)               # 1 and 70 candidates
SPREAD_TEXT = "(1. - 1e-4*(x*x + y*y + z*z))"
SOURCE_FUNCTION = "tracer"        # of particulate_sources_cases: reads T and the relative velocity


def _spread_kernel(x, y, z, t):
    return (1. - 1e-4*(x*x + y*y + z*z))


def _downstream_reference(dim, level, sides_name, steps_dia, steps_rb):
    """the chain of the device test in the restatements, with the pow of the new particles moved by `steps_dia'
    ulps in their diameter and by `steps_rb' ulps in their rb: a dict of its results.  What a cell sums over its
    particles (the spread forces, the deposit of the mass source) comes per particle (`F_parts',
    `deposit_parts'), in list order"""
    box = SK.box(dim, level)
    pl, _ = C.feed_events(dim, level, sides_name, "tracer", FED_EVENTS)
    plist = pl.plist
    new_ids = {p.id for p in plist if p.id > C.IDLAST0}
    new_volumes = {p.volume for p in plist if p.id in new_ids}
    pow_dia, pow_rb = _shifted_pow(steps_dia), _shifted_pow(steps_rb)
    e = FED_EVENTS[-1]
    u = C.velocity(dim, level, e)
    sim = FR.Sim(box, C.SIDES[sides_name], u, DT, viscosity=(lambda cell: VISCOSITY,)*3, g=GRAVITY, root=FR.sqrt_root)
    objs = [FR.ForceCoeff(DRAG), FR.ForceCoeff(BUOY)]
    FR.read_forces(sim, objs)
    diameter, distance = FR._diameter, TW.normalized_distance

    def normalized_distance(dim_, centre, p, volume):
        if volume not in new_volumes:
            return distance(dim_, centre, p, volume)
        rb = pow_rb(3.*volume/(4.*math.pi), 1./3.)        # distance_normalization, :2091
        return ((centre[0] - p[0])/rb, (centre[1] - p[1])/rb, (0. - p[2])/rb if dim_ == 3 else 0.)
    FR._diameter = lambda p: 2.*pow_dia(3.0*p.volume/4.0/math.pi, 1./3.) if p.id in new_ids else diameter(p)
    TW.normalized_distance = normalized_distance
    out = {}
    try:
        plist = FR.list_event(sim, plist, objs)
        out["ids"] = np.array([p.id for p in plist], dtype=np.uint32)
        for name in ("pos", "pos_old", "vel", "force"):
            out[name] = np.array([getattr(p, name) for p in plist])
        out["mass"] = np.array([p.mass for p in plist])
        volume = np.array([p.volume for p in plist])
        out["void"] = TW.void_fraction(dim, level, out["pos"], volume)
        FR.forces_on_fluid(sim, plist, objs)
        out["onfluid"] = np.array([p.force for p in plist])
        h = 1./(1 << level)
        out["F_parts"] = np.stack([np.stack(TW.spread(dim, level, out["pos"][q:q + 1], volume[q:q + 1],
                                                      out["onfluid"][q:q + 1], 1.5*h, _spread_kernel,
                                                      C.event_time(e))[0]) for q in range(len(plist))])
        fields = PS.Fields(dim)
        fn = K.FUNCTIONS[SOURCE_FUNCTION][1]
        sources = PS.event(box, PS.MASS, plist, sim.u, DT, C.event_time(e), fn, fields,
                           {"T": box.field(K.tracer(dim, level))})
        out["source_mass"] = np.array([p.mass for p in plist])
        parts = np.zeros((len(plist),) + (1 << level,)*dim)
        for q, (p, s) in enumerate(zip(plist, sources)):
            if s is not None:          # (a particle without a cell is skipped)
                parts[q][TW._index(dim, TW.locate(dim, level, p.pos))] = s
        out["deposit_parts"] = parts
        out["rad"] = _interior(PS.arrays(box, fields.rad, K.SENTINEL), dim)
    finally:
        FR._diameter, TW.normalized_distance = diameter, distance
    return out


@pytest.mark.parametrize("sides_name", C.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", C.BOXES)
def test_a_fed_list_behaves_as_one_given_at_creation(dim, level, sides_name):
    """The bound of what passes through pow is derived, never fitted.  The diameter and the rb of a new particle
    are two values of the device's pow, each within POW_ULPS of glibc's, independently.  A quantity of one
    particle (position, velocity, force, mass) is a function of those two numbers: the device value lies in
    the hull of the restatement over the corners and the centre of [-POW_ULPS, POW_ULPS]^2, widened by one ulp.
    A quantity of a cell is a sum over its particles in list order, each term in the hull of that particle's
    terms (the particles are off by different amounts, so the hull of the sums would be no bound); the sum
    lies between the sums of the lower and of the upper ends, widened by the rounding of a sum of n terms,
    n*eps*sum |term|."""
    corners = [(a, b) for a in (-POW_ULPS, 0, POW_ULPS) for b in (-POW_ULPS, 0, POW_ULPS)]
    runs = [_downstream_reference(dim, level, sides_name, a, b) for a, b in corners]
    exact = runs[corners.index((0, 0))]

    def in_hull(g, name):
        stack = np.stack([r[name] for r in runs])
        lo, hi = np.nextafter(stack.min(axis=0), -np.inf), np.nextafter(stack.max(axis=0), np.inf)
        if g.ndim == 2 and g.shape[1] == 3 and dim == 2:
            g, lo, hi = g[:, :2], lo[:, :2], hi[:, :2]
        assert g.shape == lo.shape, name
        assert ((g >= lo) & (g <= hi)).all(), (name, int(((g < lo) | (g > hi)).sum()))

    def in_hull_of_sums(g, name):
        stack = np.stack([r[name] for r in runs])          # run, particle, cells ...
        lo, hi = stack.min(axis=0).sum(axis=0), stack.max(axis=0).sum(axis=0)
        slack = stack.shape[1]*np.finfo(float).eps*np.abs(stack).max(axis=0).sum(axis=0)
        assert g.shape == lo.shape, name
        bad = (g < lo - slack) | (g > hi + slack)
        assert not bad.any(), (name, int(bad.sum()), float(np.abs(g - exact[name].sum(axis=0))[bad].max()))
        # where no new particle contributes the sum is the restatement's, bit for bit
        same = (stack.min(axis=0) == stack.max(axis=0)).all(axis=0)
        serial = np.zeros_like(lo)
        for part in exact[name]:
            serial = serial + part
        assert np.array_equal(g[same], serial[same]), name

    dev = Device(dim, level, sides_name)
    try:
        feed = dev.feed("tracer")
        for e in FED_EVENTS:
            dev.set_event(e)
            feed.event(C.candidates(dim, level, e))
        before = dev.state()
        dev.gpl.sort()
        _assert_state(dev.state(), before, "sorted")
        old = np.arange(len(exact["ids"])) < np.count_nonzero(exact["ids"] <= C.IDLAST0)
        # one gfs_particle_list_event with drag and buoyancy: the drag of a new particle reads its diameter
        dev.gpl.event()
        got = dev.state()
        assert np.array_equal(got.ids, exact["ids"]) and (got.ids > C.IDLAST0).sum() >= 15
        assert np.array_equal(got.old[:, :dim], exact["pos_old"][:, :dim])      # the event wrote pos_old of the new ones
        for g, name in ((got.pos, "pos"), (got.vel, "vel"), (got.force, "force")):
            in_hull(g, name)
            assert np.array_equal(g[old][:, :dim], exact[name][old][:, :dim]), name      # host-computed diameters
        assert np.array_equal(got.mass, exact["mass"])
        assert np.abs(got.force[~old][:, :dim]).max() > 0.
        # GfsParticulateField: the volumes, and the cells of the moved particles
        vf = dev.gd.variable()
        dev.gpl.particulate_field(vf)
        assert np.array_equal(_interior(vf.download(), dim), exact["void"]) and exact["void"].max() > 0.
        # GfsSourceParticulate: the forces on the fluid, spread with rb of every particle
        h = 1./(1 << level)
        F = [dev.gd.variable() for _ in range(dim)]
        dev.gpl.set_kernel(1.5*h, SPREAD_TEXT)
        dev.gpl.source_particulate_event(F)
        in_hull(dev.gpl.particulate_state()[2], "onfluid")
        spread = np.stack([_interior(f.download(), dim) for f in F])
        in_hull_of_sums(spread, "F_parts")
        assert np.abs(spread).max() > 0. and np.abs(exact["F_parts"][~old]).max() > 0.
        # GfsSourceParticulateMass: per creation slot, hence `orig' of the new particles
        src = gfship.ParticulateSource(dev.gpl, gfship.SOURCE_MASS, K.FUNCTIONS[SOURCE_FUNCTION][0], {"T": dev.T})
        dev.owned.append(src.destroy)
        rad, dep = dev.gd.variable(), dev.gd.variable()
        urel = [dev.gd.variable() for _ in range(dim)]
        rad.fill(K.SENTINEL)
        src.set_fields(rad, urel, dep)
        src.event()
        in_hull(dev.gpl.particulate_state()[1], "source_mass")
        in_hull_of_sums(_interior(dep.download(), dim), "deposit_parts")
        grad, wrad = _interior(rad.download(), dim), exact["rad"]
        written = wrad != K.SENTINEL
        assert np.array_equal(grad != K.SENTINEL, written)
        assert _ulps(grad[written], wrad[written]).max() <= POW_ULPS
    finally:
        dev.close()


# ---- refusals ---------------------------------------------------------------------------------------------

def test_refusals():
    dim, level = 2, 3
    dev = Device(dim, level, "periodic")
    pos, ids, vel, mass, volume = K.particles(dim, level, "periodic")
    try:
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile") as err:
            gfship.FeedParticle(dev.gpl, "1e-3*Q", "1e-4")
        assert "Q" in str(err.value) and gfship.lib().gfship_last_error()
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile"):
            gfship.FeedParticle(dev.gpl, "1e-3", "{ return 1e-4 }")
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            gfship.FeedParticle(dev.gpl, "x", "1e-4", {"x": dev.T})
        tracers = gfship.ParticleList(dev.gs, pos, ids)
        try:
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*particulates"):
                gfship.FeedParticle(tracers, "1e-3", "1e-4")
        finally:
            tracers.destroy()
    finally:
        dev.close()
    gt = gfship.Tree(lambda x, y: 2 if (abs(x) > 0.25 or abs(y) > 0.25) else 3)
    gpl = gt.particulates(pos, ids, vel, mass, volume)
    try:
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gfship.FeedParticle(gpl, "1e-3", "1e-4")
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gpl.idlast
    finally:
        gpl.destroy()
        gt.destroy()
    gd = gfship.Domain(2, 3, [gfship.SIDE_EXTERNAL] * 2 + [gfship.SIDE_PERIODIC] * 4)
    gs = gfship.Simulation(gd)
    gpl = gfship.ParticleList(gs, pos, ids)
    try:
        gpl.set_particulate(vel, mass, volume)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*GfsBoundaryMpi"):
            gfship.FeedParticle(gpl, "1e-3", "1e-4")
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


# ---- the front end ----------------------------------------------------------------------------------------

BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin", "gfship2D")
CASE = os.path.join(ROOT, "tests", "cases", "feed.gfs")
CASE_LEVEL, CASE_NSTEPS, CASE_DT, CASE_IDLAST = 3, 3, 0.015625, 40


def _case_restatement():
    """tests/cases/feed.gfs in the restatements: the fluid is at rest and stays there, every step is dtmax long;
    per step the event of the list (drag and buoyancy without gravity), then the five candidates of the feed.
    Returns the text of `--particles'"""
    dim, level = 2, CASE_LEVEL
    n = 1 << level
    box = SK.box(dim, level)
    zero = np.zeros((n + 2,)*dim)
    T = np.zeros((n + 2,)*dim)
    for cell in box.leaves:
        x, y = box.cell_pos(cell)[:2]
        i, j, _ = cell.ijk
        T[j, i] = (x + 0.25*y)
    sim = FR.Sim(box, SK.SIDES["periodic"], (zero, zero), CASE_DT, viscosity=(lambda cell: 1e-2,)*3, root=FR.sqrt_root)
    objs = [FR.ForceCoeff(DRAG), FR.ForceCoeff(BUOY)]
    FR.read_forces(sim, objs)
    pl = FP.ParticleList([FR.Particulate([0.11, 0.23, 0.], 3, [0.5, -0.25, 0.], 2e-3, 1e-3),
                          FR.Particulate([-0.31, 0.07, 0.], 7, [0.1, -0.2, 0.], 1.5e-3, 1e-3)], CASE_IDLAST)
    counter = {"i": 0, "j": 0}

    def xfeed():
        counter["i"] += 1
        return -0.7 + 0.13*((counter["i"] - 1) % 11)

    def yfeed():
        counter["j"] += 1
        return 0.3 - 0.11*((counter["j"] - 1) % 7)
    feed = FP.Feed(nparts=lambda: 5, xfeed=xfeed, yfeed=yfeed,
                   mass=lambda V: 1e-3*V["T"] if V["T"] > 0. else 0., volume=lambda V: (1e-3 + 1e-4*V["x"]))
    outcomes = []
    for step in range(CASE_NSTEPS + 1):          # the events of steps 0 .. NSTEPS - 1, and those after the loop
        pl.plist = FR.list_event(sim, pl.plist, objs)
        outcomes += [w for w, _ in FP.event(box, sim.u, pl, feed, step*CASE_DT, {"T": box.field(T)})]
    assert {"outside", "massless", "added"} == set(outcomes)
    lines = ["GfsParticleList GfsParticulate {"]
    for p in pl.plist:
        lines.append("    GfsParticulate %d %g %g %g %g %g %g %g %g %g %g %g" %
                     (p.id, p.pos[0], p.pos[1], 0., p.mass, p.volume, p.vel[0], p.vel[1], p.vel[2],
                      p.force[0], p.force[1], p.force[2]))
    lines.append("}")
    return "\n".join(lines) + "\n", pl


def test_the_front_end_feeds_the_list_of_the_case(tmp_path):
    want, pl = _case_restatement()
    assert pl.idlast > CASE_IDLAST + 3 and [p.id for p in pl.plist][:3] == [3, 7, CASE_IDLAST + 1]
    out = tmp_path / "particles.txt"
    r = subprocess.run([BIN, "-DLEVEL=%d" % CASE_LEVEL, "-DNSTEPS=%d" % CASE_NSTEPS, CASE, "--particles", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert out.read_text() == want
