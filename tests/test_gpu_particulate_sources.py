"""GfsSourceParticulateVol / GfsSourceParticulateMass on the device (gfship.ParticulateSource) against the
restatement of tests/particulate_sources_reference.py on the runs of tests/particulate_sources_cases.py.

Bit for bit (array_equal) wherever no libm call is involved: volumes or masses, the deposit, Urelp / Vrelp /
Wrelp with the untouched cells still at the sentinel, the skipped particle outside the box -- before and after
gfship_particles_sort, and after a second sort that leaves the particles of one cell stored in another order
than the list's (test_particulate_sources_reference_cpu.py asserts that premise).  Rad, and what a changed
volume does to the diameter, are values of the device's pow: compared with glibc's within POW_ULPS."""
import math

import numpy as np
import pytest

import forces_reference as FR
import gfship
import particulate_sources_cases as K
import particulate_sources_reference as PS
import sampler_cases as SK
import two_way_reference as TW

pytestmark = pytest.mark.gpu

BUOY = 5
KINDS = {"vol": (gfship.SOURCE_VOLUME, PS.VOLUME), "mass": (gfship.SOURCE_MASS, PS.MASS)}


def _interior(a, dim):
    return a[(slice(1, -1),) * dim]


def _ulps(a, b):
    """the distance of two arrays of positive doubles in units of the last place"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


class Device:
    """a simulation with the list of a case, its tracer and the sentinel-filled variables of a source"""

    def __init__(self, dim, level, sides_name, particles=None, forces=(BUOY,), viscosity=None):
        self.dim, self.level = dim, level
        self.gd = gfship.Domain(dim, level, K.SIDES[sides_name])
        self.gs = gfship.Simulation(self.gd)
        for c in range(dim if viscosity else 0):
            self.gs.set_viscosity(c, viscosity)
        self.set_event(0)       # Un, Vn, Wn of a GfsForceCoeff are the velocity at the time the forces are read
        pos, ids, vel, mass, volume = particles or K.particles(dim, level, sides_name)
        self.T = self.gd.variable()
        self.T.upload(K.tracer(dim, level))
        self.gpl = gfship.ParticleList(self.gs, pos, ids)
        self.gpl.set_sort_interval(0)
        self.gpl.set_particulate(vel, mass, volume)
        self.gpl.set_forces(list(forces), (0., 0., 0.))
        self.sources = []

    def source(self, kind, text, deposit=True, fields=True):
        src = gfship.ParticulateSource(self.gpl, kind, text, {"T": self.T})
        src.rad, src.dep = self.gd.variable(), self.gd.variable() if deposit else None
        src.urel = [self.gd.variable() for _ in range(self.dim)]
        for v in [src.rad] + src.urel + ([src.dep] if deposit else []):
            v.fill(K.SENTINEL)
        if fields:
            src.set_fields(src.rad, src.urel, src.dep)
        self.sources.append(src)
        return src

    def set_event(self, e):
        for c, a in enumerate(K.velocity(self.dim, self.level, e)):
            self.gs.u[c].upload(a)
        self.gs.restart(K.EVENT_T[e], e)
        self.gs.advection_params.dt = K.EVENT_DT[e]

    def close(self):
        for s in self.sources:
            s.destroy()
        self.gpl.destroy()
        self.gs.destroy()
        self.gd.destroy()


def _run(dev, src, ref, pkind, exact_rad):
    """the five events of a case on the device, each compared with the restatement"""
    dim = dev.dim
    for e in range(K.NEVENTS):
        if e == K.MOVE_BEFORE:
            dev.gs.advection_params.dt = K.DT_MOVE
            dev.gpl.event()
            pos, _ = dev.gpl.download()
            assert np.array_equal(pos[:, :dim], ref.moved_pos[:, :dim])
        dev.set_event(e)
        src.event()
        want = ref.events[e]
        vel, mass, _ = dev.gpl.particulate_state()
        volume = dev.gpl.volumes()
        what = (e, pkind)
        assert len(volume) == len(want.volume) == dev.gpl.count(), what
        assert np.array_equal(volume, want.volume), what      # the skipped particle outside keeps its state
        assert np.array_equal(mass, want.mass), what
        assert np.array_equal(_interior(src.dep.download(), dim), _interior(want.deposit, dim)), what
        for c in range(dim):
            assert np.array_equal(_interior(src.urel[c].download(), dim), _interior(want.urel[c], dim)), what
        rad, wrad = _interior(src.rad.download(), dim), _interior(want.rad, dim)
        assert np.array_equal(rad == K.SENTINEL, wrad == K.SENTINEL), what
        written = wrad != K.SENTINEL
        if exact_rad:
            assert np.array_equal(rad, wrad), what
        else:
            assert _ulps(rad[written], wrad[written]).max() <= POW_ULPS, what
        if e in K.SORT_AFTER:
            dev.gpl.sort()


# ---- items 1 and 2: bit for bit with the restatement ---------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("sides_name", K.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", K.BOXES)
def test_events_equal_the_restatement(dim, level, sides_name, kind):
    """functions without a libm call that do not read Rad, and the step of Rad that cannot feel an ulp.  For a
    mass source the volumes never change, so Rad is glibc's value up to the device's pow; for a volume source
    the volumes are exact (source*dt is) and Rad again differs by the pow alone"""
    gkind, pkind = KINDS[kind]
    for fname in K.NO_LIBM + ("step",):
        ref = K.reference_run(dim, level, sides_name, pkind, fname)
        dev = Device(dim, level, sides_name)
        try:
            src = dev.source(gkind, K.FUNCTIONS[fname][0])
            _run(dev, src, ref, (pkind, fname), exact_rad=False)
            # the storage order after the second sort is not the list order, and the list is what it was
            pos, ids = dev.gpl.download()
            assert np.array_equal(ids, np.asarray(K.particles(dim, level, sides_name)[1])[K.on_list_after_move(sides_name)])
        finally:
            dev.close()


def test_no_fields_no_deposit_and_null_function():
    """every field may be -1 (nothing written, nothing sorted), the deposit alone may be missing, and a NULL
    function is the constant 0: the event then writes Rad and Urelp and changes no particle"""
    dim, level, sides_name = 2, 3, "closed"
    pos, ids, vel, mass, volume = K.particles(dim, level, sides_name)
    dev = Device(dim, level, sides_name)
    try:
        bare = dev.source(gfship.SOURCE_VOLUME, K.FUNCTIONS["tracer"][0], fields=False)
        nodep = dev.source(gfship.SOURCE_MASS, None, deposit=False)
        dev.set_event(0)
        bare.event()
        ref = K.reference_run(dim, level, sides_name, PS.VOLUME, "tracer")
        assert np.array_equal(dev.gpl.volumes(), ref.events[0].volume)
        for v in [bare.rad, bare.dep] + bare.urel:
            assert (_interior(v.download(), dim) == K.SENTINEL).all()
        nodep.event()
        assert np.array_equal(dev.gpl.particulate_state()[1], mass)
        for c in range(dim):
            assert np.array_equal(_interior(nodep.urel[c].download(), dim), _interior(ref.events[0].urel[c], dim))
    finally:
        dev.close()


def test_refusals():
    dim, level = 2, 3
    dev = Device(dim, level, "periodic")
    try:
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*deposited"):
            s = gfship.ParticulateSource(dev.gpl, gfship.SOURCE_VOLUME, "2.*T", {"T": dev.T})
            dev.sources.append(s)
            s.set_fields(None, (), dev.T)
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile"):
            gfship.ParticulateSource(dev.gpl, gfship.SOURCE_MASS, "2.*Wrelp")          # no Wrelp in 2-D
        with pytest.raises(gfship.GfshipError, match="gfship error -1.*does not compile"):
            gfship.ParticulateSource(dev.gpl, gfship.SOURCE_MASS, "2.*Q")
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            gfship.ParticulateSource(dev.gpl, gfship.SOURCE_MASS, "Rad", {"Rad": dev.T})
        pos, ids = K.particles(dim, level, "periodic")[:2]
        tracers = gfship.ParticleList(dev.gs, pos, ids)
        try:
            with pytest.raises(gfship.GfshipError, match="gfship error -5.*particulates"):
                gfship.ParticulateSource(tracers, gfship.SOURCE_MASS, "1.")
        finally:
            tracers.destroy()
    finally:
        dev.close()


def test_refused_on_a_tree_and_on_external_sides():
    gt = gfship.Tree(lambda x, y: 2 if (abs(x) > 0.25 or abs(y) > 0.25) else 3)
    pos, ids, vel, mass, volume = K.particles(2, 3, "periodic")
    gpl = gt.particulates(pos, ids, vel, mass, volume)
    try:
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gfship.ParticulateSource(gpl, gfship.SOURCE_VOLUME, "1.")
        assert np.array_equal(gpl.volumes(), volume)      # the volumes of a list of a tree can be read
    finally:
        gpl.destroy()
        gt.destroy()
    gd = gfship.Domain(2, 3, [gfship.SIDE_EXTERNAL] * 2 + [gfship.SIDE_PERIODIC] * 4)
    gs = gfship.Simulation(gd)
    gpl = gfship.ParticleList(gs, pos, ids)
    try:
        gpl.set_particulate(vel, mass, volume)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*GfsBoundaryMpi"):
            gfship.ParticulateSource(gpl, gfship.SOURCE_VOLUME, "1.")
    finally:
        gpl.destroy()
        gs.destroy()
        gd.destroy()


# ---- item 3: the device's pow against glibc's -----------------------------------------------------------

# The double-precision pow of the device library has no bound stated in the headers or documents installed
# with ROCm.  Measured on gfx950 over the volumes of the cases and the sweep below: at most 1 ulp from glibc's
# math.pow (which is itself within 1 ulp of the exact value); one more is allowed because the sweep is a sample.
POW_MEASURED_ULPS = 1
POW_ULPS = POW_MEASURED_ULPS + 1
SWEEP = 1000000


def _device_radii(volumes):
    """pow (3.0*volume/4.0/M_PI, 1./3.) of the device for every volume: a mass source whose function is Rad,
    with dt = 1 on masses of zero -- mass = 0. + Rad*1. is Rad"""
    n = len(volumes)
    rng = np.random.default_rng(5)
    pos = np.zeros((n, 3))
    pos[:, :2] = 0.9 * (rng.random((n, 2)) - 0.5)
    particles = (pos, np.arange(1, n + 1, dtype=np.uint32), np.zeros((n, 3)), np.zeros(n), volumes)
    dev = Device(2, 3, "periodic", particles)
    try:
        src = dev.source(gfship.SOURCE_MASS, "Rad", fields=False)
        dev.set_event(0)
        dev.gs.advection_params.dt = 1.
        src.event()
        return dev.gpl.particulate_state()[1]
    finally:
        dev.close()


def test_the_radius_is_within_the_measured_bound_of_glibc():
    volumes = np.concatenate([10. ** np.linspace(-12., 0., SWEEP)] +
                             [K.particles(d, l, s)[4] for d, l in K.BOXES for s in K.SIDE_NAMES])
    got = _device_radii(volumes)
    want = np.array([PS.radius(v) for v in volumes.tolist()])
    d = _ulps(got, want)
    print("device pow against glibc's over %d volumes: max %d ulp, %d differ" % (len(volumes), d.max(), (d != 0).sum()))
    assert d.max() <= POW_ULPS


# ---- item 4: downstream of a changed volume ------------------------------------------------------------

def _shifted_pow(steps):
    def pow_(x, y):
        r = math.pow(x, y)
        for _ in range(abs(steps)):
            r = math.nextafter(r, math.inf if steps > 0 else -math.inf)
        return r
    return pow_


def _downstream_reference(dim, level, sides_name, pkind, steps, forces):
    """a source event, the list event with `forces', then GfsParticulateField, in the restatement with its radius
    function moved by `steps' ulps: (vel, mass, force, pos) after the list event and the volume fraction"""
    box = SK.box(dim, level)
    pos, ids, vel, mass, volume = K.particles(dim, level, sides_name)
    plist = [FR.Particulate(pos[q], ids[q], vel[q], mass[q], volume[q]) for q in range(K.NPART)]
    text, fn, names = K.FUNCTIONS["tracer"]
    u = [box.field(a) for a in K.velocity(dim, level, 0)]
    PS.event(box, pkind, plist, u, K.EVENT_DT[0], K.EVENT_T[0], fn, PS.Fields(dim), {"T": box.field(K.tracer(dim, level))},
             _shifted_pow(steps))
    sim = FR.Sim(box, K.SIDES[sides_name], K.velocity(dim, level, 0), K.EVENT_DT[0],
                 viscosity=(lambda cell: 1e-2,) * 3, root=FR.sqrt_root)
    pow0 = _shifted_pow(steps)
    diameter = FR._diameter
    FR._diameter = lambda p: 2.*pow0(3.0*p.volume/4.0/math.pi, 1./3.)
    try:
        objs = [FR.ForceCoeff(k) for k in forces]
        FR.read_forces(sim, objs)
        sim.set_velocity(K.velocity(dim, level, 1))
        plist = FR.list_event(sim, plist, objs)
    finally:
        FR._diameter = diameter
    pos = np.array([p.pos for p in plist])
    return (np.array([p.vel for p in plist]), np.array([p.mass for p in plist]), np.array([p.force for p in plist]),
            pos, TW.void_fraction(dim, level, pos, np.array([p.volume for p in plist])))


def _downstream_device(dim, level, sides_name, gkind, forces):
    dev = Device(dim, level, sides_name, forces=forces, viscosity=1e-2)
    try:
        src = dev.source(gkind, K.FUNCTIONS["tracer"][0])
        src.event()
        for c, a in enumerate(K.velocity(dim, level, 1)):
            dev.gs.u[c].upload(a)
        dev.gpl.event()
        vel, mass, force = dev.gpl.particulate_state()
        vf = dev.gd.variable()
        dev.gpl.particulate_field(vf)
        return vel, mass, force, dev.gpl.download()[0], _interior(vf.download(), dim)
    finally:
        dev.close()


@pytest.mark.parametrize("dim,level", [(2, 3), (3, 3)])
def test_a_mass_event_then_the_list_event_is_exact(dim, level):
    forces = (FR.DRAG, FR.ADDEDMASS)
    got = _downstream_device(dim, level, "periodic", gfship.SOURCE_MASS, forces)
    want = _downstream_reference(dim, level, "periodic", PS.MASS, 0, forces)
    for g, w in zip(got[:4], want[:4]):
        assert np.array_equal(g[:, :dim] if g.ndim == 2 else g, w[:, :dim] if w.ndim == 2 else w)
    assert np.array_equal(got[4], want[4]) and got[4].max() > 0.


@pytest.mark.parametrize("dim,level", [(2, 3), (3, 3)])
def test_a_volume_event_then_the_list_event_lies_in_the_hull_of_the_bound(dim, level):
    """the tolerance is derived: the restatement with its radius function (Rad, and the diameter of a changed
    volume) moved down and up by POW_ULPS; every device value lies in the hull of those results and the
    unmoved one, widened by one ulp"""
    forces = (FR.DRAG, FR.ADDEDMASS)
    got = _downstream_device(dim, level, "periodic", gfship.SOURCE_VOLUME, forces)
    runs = [_downstream_reference(dim, level, "periodic", PS.VOLUME, s, forces) for s in (-POW_ULPS, 0, POW_ULPS)]
    for q, g in enumerate(got):
        stack = np.stack([r[q] for r in runs])
        lo = np.nextafter(stack.min(axis=0), -np.inf)
        hi = np.nextafter(stack.max(axis=0), np.inf)
        if q < 4 and g.ndim == 2:
            g, lo, hi = g[:, :dim], lo[:, :dim], hi[:, :dim]
        assert ((g >= lo) & (g <= hi)).all(), (q, int(((g < lo) | (g > hi)).sum()))


# ---- item 5: a list no event has run on ----------------------------------------------------------------

def test_a_list_with_a_source_but_no_event_is_unchanged():
    dim, level = 3, 3
    forces = (FR.DRAG, FR.ADDEDMASS)
    outcomes = []
    for with_source in (False, True):
        dev = Device(dim, level, "periodic", forces=forces, viscosity=1e-2)
        try:
            if with_source:
                dev.source(gfship.SOURCE_VOLUME, K.FUNCTIONS["tracer"][0])
            dev.gpl.event()
            outcomes.append(dev.gpl.particulate_state() + dev.gpl.download() + (dev.gpl.volumes(),))
        finally:
            dev.close()
    for a, b in zip(*outcomes):
        assert np.array_equal(a, b)
    # ... and they are the bits of the restatement with the host's diameter
    box = SK.box(dim, level)
    pos, ids, vel, mass, volume = K.particles(dim, level, "periodic")
    plist = [FR.Particulate(pos[q], ids[q], vel[q], mass[q], volume[q]) for q in range(K.NPART)]
    sim = FR.Sim(box, K.SIDES["periodic"], K.velocity(dim, level, 0), K.EVENT_DT[0],
                 viscosity=(lambda cell: 1e-2,) * 3, root=FR.sqrt_root)
    objs = [FR.ForceCoeff(k) for k in forces]
    FR.read_forces(sim, objs)
    plist = FR.list_event(sim, plist, objs)
    assert np.array_equal(outcomes[0][0], np.array([p.vel for p in plist]))
    assert np.array_equal(outcomes[0][1], np.array([p.mass for p in plist]))
    assert np.array_equal(outcomes[0][2], np.array([p.force for p in plist]))
