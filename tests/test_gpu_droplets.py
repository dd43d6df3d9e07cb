"""Droplets on the device (Domain.tag_droplets, Domain.remove_droplets, gfship.DropletToParticle) against the
restatement of tests/droplets_reference.py on the cases of tests/droplets_cases.py.

Bit for bit (array_equal): the tags and their number, the list after every event (positions, velocities, mass,
volume, ids, order, force, pos_old, count, slots, idlast), the tracer, the info.  No libm call is involved in any of
them: h^dim is a power of two.  The diameter and rb of a new particle are values of the device's pow: the event with
drag that follows is compared within the POW_ULPS that tests/test_gpu_particulate_sources.py measures and justifies
for the same expression: every quantity of a new particle equals, bit for bit, the restatement with that pow moved by
a whole number of ulps, at most POW_ULPS; the particles the list was created with stay bit for bit; the event of a
GfsSourceParticulate after it, whose spreading reads rb, is bounded per cell by the sums over those shifts."""
import copy
import functools
import math

import numpy as np
import pytest

import droplets_cases as C
import droplets_reference as DR
import feed_particle_reference as FP
import forces_reference as FR
import gfship
import sampler_cases as SK
import two_way_reference as TW
from test_gpu_particulate_sources import POW_ULPS, _shifted_pow

pytestmark = pytest.mark.gpu

ALL = [(dim, level, s) for dim, level in C.BOXES for s in C.SIDE_NAMES]
VISCOSITY, DT = 1e-2, 2.**-6
DRAG = FR.DRAG


def _interior(a, dim):
    return a[(slice(1, -1),)*dim]


class Device:
    """a simulation at rest in the velocity of the cases, the tracers T and S, alpha"""

    def __init__(self, dim, level, sides_name):
        self.dim, self.level = dim, level
        self.gd = gfship.Domain(dim, level, C.SIDES[sides_name])
        self.gs = gfship.Simulation(self.gd)
        for c in range(dim):
            self.gs.set_viscosity(c, VISCOSITY)
            self.gs.u[c].upload(C.velocity(dim, level)[c])
        self.gs.restart(0.25, 3)
        self.gs.advection_params.dt = DT
        self.T, self.S, self.alpha, self.tag = (self.gd.variable() for _ in range(4))
        self.gpl, self.owned = None, []

    def load(self, case):
        """the fields of a case and a fresh list"""
        self.release()
        self.T.upload(case.T)
        self.S.upload(case.S)
        if case.alpha is not None:
            self.alpha.upload(case.alpha)
        self.gs.set_alpha_cell(self.alpha if case.alpha is not None else None)
        pos, ids, vel, mass, volume = C.particles(self.dim)
        self.gpl = gfship.ParticleList(self.gs, pos, ids)
        self.gpl.set_sort_interval(0)
        self.gpl.set_particulate(vel, mass, volume)
        self.gpl.set_forces([DRAG])
        self.gpl.idlast = C.IDLAST0
        d = gfship.DropletToParticle(self.gpl, self.T, case.min, case.reset, 1000., case.function,
                                     {"T": self.T, "S": self.S})
        self.owned.append(d.close)
        return d

    def state(self):
        pos, ids = self.gpl.download()
        vel, mass, force = self.gpl.particulate_state()
        return {"ids": ids, "pos": pos, "old": self.gpl.download_old(), "vel": vel, "mass": mass,
                "volume": self.gpl.volumes(), "force": force, "idlast": self.gpl.idlast}

    def release(self):
        for close in self.owned:
            close()
        self.owned = []
        if self.gpl is not None:
            self.gpl.destroy()
            self.gpl = None

    def close(self):
        self.release()
        self.gs.destroy()
        self.gd.destroy()


def _assert_state(got, want, what):
    assert len(got["ids"]) == len(want["ids"]), what
    for name in ("ids", "pos", "old", "vel", "mass", "volume", "force"):
        assert np.array_equal(got[name], want[name]), (what, name)
    assert got["idlast"] == want["idlast"], what


def _assert_field(dev, var, want, what, before=None):
    """the leaves equal the restatement; the ghosts are those of the boundary conditions of the variable, or, where
    nothing happened (before: the field as it was), untouched"""
    got = var.download()
    assert np.array_equal(_interior(got, dev.dim), _interior(want, dev.dim)), what
    if before is not None:
        assert np.array_equal(got, before, equal_nan=True), (what, "untouched")
        return
    dev.gd.bc(var)
    again = var.download()
    faces = SK.ghost_count(dev.dim, dev.level) == 1
    assert np.array_equal(got[faces], again[faces]), (what, "ghosts")


def _events(dev, case, ref, what):
    """two events in a row on one list, each against the restatement; returns the states"""
    d2p = dev.load(case)
    slots, states = 3, []
    for e in range(2):
        info, _, T, want = ref.events[e]
        before = dev.T.download()
        got = d2p.event()
        assert got == tuple(info), (what, e)
        ran = info[0] > 0 and -case.min < info[0]
        if ran:
            slots += info[0]          # every droplet of an event that runs takes a slot, dead or alive
        assert gfship.lib().gfship_particles_slots(dev.gpl.ptr) == slots, (what, e)
        state = dev.state()
        _assert_state(state, want, (what, e))
        assert dev.gpl.count() == len(want["ids"]), (what, e)
        if dev.dim == 2:
            assert not state["vel"][3:, 2].any() and not state["pos"][3:, 2].any()
        _assert_field(dev, dev.T, T, (what, e), None if ran else before)
        states.append((state, dev.T.download()))
    return states


@pytest.mark.parametrize("dim,level,sides_name", ALL)
def test_tags_equal_the_restatement(dim, level, sides_name):
    dev = Device(dim, level, sides_name)
    try:
        for name in C.CASE_NAMES:
            case = C.cases(dim, level, sides_name)[name]
            ref = C.reference_run(dim, level, sides_name, name)
            dev.T.upload(case.T if case.mask() is None else case.mask())
            dev.tag.fill(-7.)
            n = dev.gd.tag_droplets(dev.T, dev.tag)
            assert n == ref.tags.n, name
            assert np.array_equal(_interior(dev.tag.download(), dim), _interior(ref.tag_array, dim)), name
    finally:
        dev.close()


@pytest.mark.parametrize("dim,level,sides_name", ALL)
def test_events_equal_the_restatement(dim, level, sides_name):
    """every case: two events in a row on one list (the second on the reset field; the list grows past the three
    slots it was created with), then the whole case again: bit for bit the same"""
    dev = Device(dim, level, sides_name)
    try:
        for name in C.CASE_NAMES:
            case = C.cases(dim, level, sides_name)[name]
            ref = C.reference_run(dim, level, sides_name, name)
            first = _events(dev, case, ref, name)
            again = _events(dev, case, ref, name + " again")
            for (s0, t0), (s1, t1) in zip(first, again):
                _assert_state(s0, s1, (name, "twice"))
                assert np.array_equal(t0, t1, equal_nan=True), (name, "twice")
    finally:
        dev.close()


@pytest.mark.parametrize("dim,level,sides_name", ALL)
def test_remove_droplets_equals_the_restatement(dim, level, sides_name):
    dev = Device(dim, level, sides_name)
    try:
        for name in C.CASE_NAMES:
            case = C.cases(dim, level, sides_name)[name]
            if case.function is not None:
                continue
            ref = C.reference_run(dim, level, sides_name, name)
            dev.T.upload(case.T)
            dev.S.upload(case.S + 0.5)
            before = dev.S.download()
            dev.gd.remove_droplets(dev.T, dev.S, case.min, -3.)
            ran = ref.remove_info[0] > 0 and -case.min < ref.remove_info[0]
            _assert_field(dev, dev.S, ref.removed, name, None if ran else before)
            assert np.array_equal(dev.T.download(), case.T), name
        # c and v the same field
        case = C.cases(dim, level, sides_name)["sizes"]
        box = SK.box(dim, level)
        want = case.T.copy()
        DR.remove_droplets(box, C.SIDES[sides_name], case.T, want, 5, 0.)
        dev.T.upload(case.T)
        dev.gd.remove_droplets(dev.T, dev.T, 5, 0.)
        _assert_field(dev, dev.T, want, "in place")
    finally:
        dev.close()


# ---- downstream: the diameter and rb of the new particles ---------------------------------------------------

SPREAD_TEXT = "(1. - 1e-4*(x*x + y*y + z*z))"
PARTICLE_CASES = ("join", "join_min-1", "sizes", "threshold", "chain", "function", "alpha")


def _spread_kernel(x, y, z, t):
    return (1. - 1e-4*(x*x + y*y + z*z))


def _makes_particles(dim, level, sides_name, name):
    return any(e[0][2] > 0 for e in C.reference_run(dim, level, sides_name, name).events)


SHIFTS = tuple(range(-POW_ULPS, POW_ULPS + 1))


@functools.lru_cache(None)
def _downstream_reference(dim, level, sides_name, name):
    """the two events of the case, then one gfs_particle_list_event with drag and the event of a
    GfsSourceParticulate, in the restatements, with the pow of the new particles moved by a ulps in their diameter
    and by b ulps in their rb, for every integer a and b in [-POW_ULPS, POW_ULPS].  Returns the ids of the new
    particles, the state after the list event and the forces on the fluid for every a (neither reads rb), and the
    spread forces per particle of the list (`F_parts[a, b]', in list order: what a cell sums over its particles)"""
    case = C.cases(dim, level, sides_name)[name]
    box, sides = SK.box(dim, level), C.SIDES[sides_name]
    pl = C.particle_list(dim)
    T = case.T.copy()
    for _ in range(2):
        mask = None
        if case.function == "S":
            mask = case.S
        elif case.function is not None:
            mask = T - 0.5*case.S
        DR.event(box, sides, pl, T, C.velocity(dim, level), case.min, case.reset, mask, case.alpha)
    new_ids = {p.id for p in pl.plist if p.id > C.IDLAST0}
    new_volumes = {p.volume for p in pl.plist if p.id in new_ids}
    # a new particle must not share its volume with one of the list as created: the volume tells them apart below
    assert new_ids and not new_volumes & set(C.particles(dim)[4].tolist())
    alpha = None if case.alpha is None else (lambda cell: DR._value(box, cell, case.alpha))
    sim = FR.Sim(box, sides, C.velocity(dim, level), DT, alpha=alpha, viscosity=(lambda cell: VISCOSITY,)*3,
                 root=FR.sqrt_root)
    objs = [FR.ForceCoeff(DRAG)]
    FR.read_forces(sim, objs)
    diameter, distance = FR._diameter, TW.normalized_distance
    interior = None if case.alpha is None else _interior(case.alpha, dim)
    h = 1./(1 << level)
    states, parts = {}, {}
    try:
        for a in SHIFTS:
            pow_dia = _shifted_pow(a)
            FR._diameter = lambda p: 2.*pow_dia(3.0*p.volume/4.0/math.pi, 1./3.) if p.id in new_ids else diameter(p)
            run = FP.ParticleList(copy.deepcopy(pl.plist), pl.idlast)
            run.plist = FR.list_event(sim, run.plist, objs)
            out = C.list_state(run)
            FR.forces_on_fluid(sim, run.plist, objs)
            out["onfluid"] = np.array([p.force for p in run.plist]).reshape(-1, 3)
            states[a] = out
            for b in SHIFTS:
                pow_rb = _shifted_pow(b)

                def normalized_distance(dim_, centre, p, volume):
                    if volume not in new_volumes:
                        return distance(dim_, centre, p, volume)
                    rb = pow_rb(3.*volume/(4.*math.pi), 1./3.)        # distance_normalization, :2091
                    return ((centre[0] - p[0])/rb, (centre[1] - p[1])/rb, (0. - p[2])/rb if dim_ == 3 else 0.)
                TW.normalized_distance = normalized_distance
                rows = []
                for q, pid in enumerate(out["ids"]):
                    if pid not in new_ids and (a, b) != (SHIFTS[0], SHIFTS[0]):
                        rows.append(parts[SHIFTS[0], SHIFTS[0]][q])      # no pow of the device in it
                        continue
                    rows.append(np.stack(TW.spread(dim, level, out["pos"][q:q + 1], out["volume"][q:q + 1],
                                                   out["onfluid"][q:q + 1], 1.5*h, _spread_kernel, 0.25, interior)[0]))
                parts[a, b] = np.stack(rows)
    finally:
        FR._diameter, TW.normalized_distance = diameter, distance
    return new_ids, states, parts


@pytest.mark.parametrize("dim,level,sides_name", ALL)
def test_a_grown_list_behaves_as_one_given_at_creation(dim, level, sides_name):
    """Every case whose events make particles -- one with alpha and one with a mask from a function among them --
    then an event with drag (it reads the diameter of a new particle) and the event of a GfsSourceParticulate (its
    spreading reads rb).  The bound is POW_ULPS of tests/test_gpu_particulate_sources.py and nothing else: the
    diameter and the rb of a new particle are two values of the device's pow, each glibc's moved by a whole number
    of ulps, at most POW_ULPS, independently.  Everything else is the reference's arithmetic, so
    - a quantity of one particle that reads its diameter (position, velocity, force, the force on the fluid) equals,
      bit for bit and in all its components at once, the restatement with that pow moved by one of the 2 POW_ULPS + 1
      whole shifts.  (The hull of the restatement at the shifts -POW_ULPS, 0, POW_ULPS widened by one ulp, the form
      this test had first, is no bound: the last bits of such a quantity are not monotone in the shift.  Measured
      on gfx950, case `threshold', 3-D level 4, force on the fluid of particle 41, x: device 0x1.6e045683e0494p-13 =
      the shift -1; the shifts -2, 0, 2 give ...492, ...496, ...494; y: device ...97111, the three shifts ...97108,
      ...9710d, ...9710d.)
    - a quantity of a cell is a sum over its particles in list order, each term one of the (2 POW_ULPS + 1)^2
      restated terms of that particle; the sum lies between the sums of the least and of the greatest of them,
      widened by the rounding of a sum of n terms, n*eps*sum |term|.  Where no new particle contributes it is bit
      for bit."""
    names = [name for name in PARTICLE_CASES if _makes_particles(dim, level, sides_name, name)]
    assert {"join", "sizes", "function", "alpha"} <= set(names)
    dev = Device(dim, level, sides_name)
    try:
        for name in names:
            new_ids, states, parts = _downstream_reference(dim, level, sides_name, name)
            exact = states[0]
            d2p = dev.load(C.cases(dim, level, sides_name)[name])
            d2p.event()
            d2p.event()
            dev.gpl.event()
            got = dev.state()
            assert np.array_equal(got["ids"], exact["ids"]), name
            old = ~np.isin(got["ids"], list(new_ids))
            assert np.array_equal(got["mass"], exact["mass"]) and np.array_equal(got["volume"], exact["volume"])
            # GfsSourceParticulate: the forces on the fluid, spread with rb of every particle
            F = [dev.gd.variable() for _ in range(dim)]
            dev.gpl.set_kernel(1.5/(1 << level), SPREAD_TEXT)
            dev.gpl.source_particulate_event(F)
            got["onfluid"] = dev.gpl.particulate_state()[2]
            spread = np.stack([_interior(f.download(), dim) for f in F])
            for f in F:
                f.free()
            keys = ("pos", "vel", "force", "old", "onfluid")
            for q, pid in enumerate(got["ids"]):
                match = [a for a in SHIFTS
                         if all(np.array_equal(got[k][q, :dim], states[a][k][q, :dim]) for k in keys)]
                print(name, "particle", pid, "equals the restatement at the shifts", match)
                assert match, (name, pid)
                assert not old[q] or len(match) == len(SHIFTS), (name, pid)      # no pow of the device in them
            assert np.abs(got["force"][~old][:, :dim]).max() > 0., name
            stack = np.stack([parts[ab] for ab in sorted(parts)])          # run, particle, component, cells ...
            lo, hi = stack.min(axis=0).sum(axis=0), stack.max(axis=0).sum(axis=0)
            slack = stack.shape[1]*np.finfo(float).eps*np.abs(stack).max(axis=0).sum(axis=0)
            assert spread.shape == lo.shape, name
            bad = (spread < lo - slack) | (spread > hi + slack)
            assert not bad.any(), (name, int(bad.sum()))
            same = (stack.min(axis=0) == stack.max(axis=0)).all(axis=0)
            serial = np.zeros_like(lo)
            for part in parts[0, 0]:
                serial = serial + part
            assert np.array_equal(spread[same], serial[same]), name
            assert np.abs(parts[0, 0][~old]).max() > 0., name
    finally:
        dev.close()


# ---- refusals ----------------------------------------------------------------------------------------------

def test_refusals():
    dim, level = 2, 4
    dev = Device(dim, level, "periodic")
    case = C.cases(dim, level, "periodic")["join"]
    try:
        dev.load(case)
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile") as err:
            gfship.DropletToParticle(dev.gpl, dev.T, 6, 0., 1., "T - 0.5*Q", {"T": dev.T})
        assert "Q" in str(err.value)
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            gfship.DropletToParticle(dev.gpl, dev.T, 6, 0., 1., "x", {"x": dev.T})
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            dev.gd.tag_droplets(dev.T, dev.T)
        pos, ids = C.particles(dim)[:2]
        tracers = gfship.ParticleList(dev.gs, pos, ids)
        try:
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*GfsDropletToParticle.*particulates"):
                gfship.DropletToParticle(tracers, dev.T)
        finally:
            tracers.destroy()
        # a constant function: nothing above the threshold, or the whole box
        nothing = gfship.DropletToParticle(dev.gpl, dev.T, 6, 0., 1., "5e-5")
        dev.owned.append(nothing.close)
        assert nothing.event() == (0, 0, 0, 0)
        assert np.array_equal(dev.T.download(), case.T)
    finally:
        dev.close()
    pos, ids, vel, mass, volume = C.particles(2)
    gt = gfship.Tree(lambda x, y: 2 if (abs(x) > 0.25 or abs(y) > 0.25) else 3)
    gpl = gt.particulates(pos, ids, vel, mass, volume)
    try:
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gfship.DropletToParticle(gpl, dev.T)
    finally:
        gpl.destroy()
        gt.destroy()
    gd = gfship.Domain(2, 3, [gfship.SIDE_EXTERNAL]*2 + [gfship.SIDE_PERIODIC]*4)
    gs = gfship.Simulation(gd)
    gpl = gfship.ParticleList(gs, pos, ids)
    T, tag = gd.variable(), gd.variable()
    try:
        gpl.set_particulate(vel, mass, volume)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*GfsBoundaryMpi"):
            gfship.DropletToParticle(gpl, T)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*GfsBoundaryMpi"):
            gd.tag_droplets(T, tag)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*GfsBoundaryMpi"):
            gd.remove_droplets(T, T, 3, 0.)
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()
