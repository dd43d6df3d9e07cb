"""GfsFeedParticle (modules/particulatecommon.c:2375-2647) and add_particulate (:1237-1276), restated on the
explicit cell graph of tests/sampler_reference.py.

Plain Python floats in the reference's order, the reference's file:line at every step.  An event evaluates
nparts once, then per candidate the three position functions in the order x, y, z (functions of the host,
called without a cell: they may have state), gfs_domain_locate, gfs_interpolate of the velocity components, the
volume and the mass functions at the cell, and add_particulate, which drops a mass below 1.e-20 before an id is
taken and otherwise appends an object with id = ++idlast.

The particles are forces_reference.Particulate objects, so that forces_reference, two_way_reference and
particulate_sources_reference run on the list as it stands, old and fed particles together.

Test infrastructure only.
"""
import forces_reference as FR


class ParticleList:
    """GfsParticleList: the objects in list order and idlast (0 from gfs_particle_list_init, or the integer
    that ends the list in the file, :1087-1090)"""

    def __init__(self, plist=(), idlast=0):
        self.plist, self.idlast = list(plist), int(idlast)


class Feed:
    """GfsFeedParticle: nparts, xfeed, yfeed, zfeed are callables without argument; mass and volume are
    callables of the dict V (x, y, z: the centre of the cell; t; the value at the cell of every variable).
    The defaults are those of gfs_feed_particle_init (:2614-2625)."""

    def __init__(self, nparts=lambda: 1., xfeed=lambda: 0., yfeed=lambda: 0., zfeed=lambda: 0.,
                 mass=lambda V: 0., volume=lambda V: 0.):
        self.nparts, self.xfeed, self.yfeed, self.zfeed, self.mass, self.volume = nparts, xfeed, yfeed, zfeed, mass, volume


def particle_id(pl):
    pl.idlast += 1                                          # :1233
    return pl.idlast


def add_particulate(pl, pos, vel, volume, mass):
    """:1237-1276.  Returns the new object, or None"""
    if mass < 1.e-20:                                       # :1244: a NaN is not less
        return None
    p = FR.Particulate(pos, particle_id(pl), vel, mass, volume)      # :1259-1266
    p.pos_old = [0., 0., 0.]                                # a new object; written by the next event (:804-805)
    p.force = [0., 0., 0.]                                  # :1267
    pl.plist.append(p)                                      # :1248-1275: reverse, add at the head, reverse
    return p


def feed_particulate(box, u, pl, feed, t, variables):
    """:2377-2402.  Returns (what happened, the cell): 'outside', 'massless' or 'added'"""
    pos = [float(feed.xfeed()), float(feed.yfeed()), float(feed.zfeed())]      # :2381-2383, in this order
    cell = box.locate(pos)                                  # :2386
    if cell is None:
        return "outside", None                              # :2387
    vel = [0., 0., 0.]
    for c in range(box.dim):                                # :2389-2397; vel.z = 0. in 2-D
        vel[c] = box.interpolate(cell, pos, u[c])
    centre = box.cell_pos(cell)
    V = {"x": centre[0], "y": centre[1], "z": centre[2] if box.dim == 3 else 0., "t": t}
    for name, v in variables.items():
        V[name] = box.value(cell, v)
    volume = float(feed.volume(V))                          # :2398
    mass = float(feed.mass(V))                              # :2399
    p = add_particulate(pl, pos, vel, volume, mass)         # :2400
    return ("massless" if p is None else "added"), cell


def event(box, u, pl, feed, t, variables=None):
    """gfs_feed_particle_event, :2404-2418.  u: the velocity components as Box.field () lists; variables: name ->
    Box.field () list.  Returns the outcome of every candidate, in order"""
    variables = variables or {}
    np_ = int(feed.nparts())                                # :2411, once per event
    return [feed_particulate(box, u, pl, feed, t, variables) for _ in range(np_)]      # :2413-2414
