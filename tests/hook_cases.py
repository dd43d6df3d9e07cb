"""Cases and helpers for the tests of the solver hooks of the C ABI (include/gfship.h, "the pieces,
callable on their own") against their twins of the CPU oracle (oracle/go_timestep.c):

  * Case: one configuration (dimension, level, sides, gradient, viscosity, source, alpha, tracers,
    events); oracle_sim / device_sim build the two simulations with the same settings;
  * random_state / load_state: both simulations are brought to the same state BY UPLOAD (smooth
    fields plus a seeded perturbation in every variable, the MAC velocities included);
  * pieces_step: the loop body of simulation_run (src/simulation.c:479-548) written from the public
    pieces -- the same function drives an oracle.Sim and a gfship.Simulation, whose methods have the
    same names;
  * differences: EVERY variable of the two simulations compared bit for bit.

The oracle part needs no device (tests/test_hooks_recipe_cpu.py); device_sim imports gfship.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O

G_MAXINT = 2147483647
RTOL_SUM = 1e-12       # tree-reduced norm sums of GfsMultilevelParams (tests/test_gpu_poisson.py)

PERIODIC = [O.SIDE_PERIODIC] * 6
BOUNDARY = [O.SIDE_BOUNDARY] * 6
# a box whose x sides are GfsBoundaryMpi sides facing the box itself: the library's own transport on a
# one-rank communicator, as in tests/test_gpu_multibox.py; the results are those of the periodic box,
# which is what the oracle runs
EXTERNAL_X = [O.SIDE_EXTERNAL, O.SIDE_EXTERNAL] + [O.SIDE_PERIODIC] * 4


class Case:
    def __init__(self, dim, level, sides="periodic", gradient=0, visc=0., source=0., alpha=False,
                 tracers=False, event=False):
        self.dim, self.level, self.sides = dim, level, sides
        self.gradient, self.visc, self.source, self.alpha = gradient, visc, source, alpha
        self.tracers, self.event = tracers, event

    @property
    def id(self):
        s = "%dd-l%d-%s-grad%d" % (self.dim, self.level, self.sides, self.gradient)
        for flag, name in ((self.visc, "visc"), (self.source, "source"), (self.alpha, "alpha"),
                           (self.tracers, "tracers"), (self.event, "event")):
            if flag:
                s += "-" + name
        return s

    @property
    def side(self):
        return {"periodic": PERIODIC, "lid": BOUNDARY, "symmetry": BOUNDARY,
                "external": EXTERNAL_X}[self.sides]

    @property
    def oracle_side(self):
        return PERIODIC if self.sides == "external" else self.side

    @property
    def n(self):
        return 1 << self.level

    def event_time(self):
        """an event inside the first time step (velocities of order one: dt is about 0.6/n)"""
        return 0.1 / self.n

    def next_event(self, t, i):
        """what the gfs_event_next loop gives (src/simulation.c:1603-1610) for one event at event_time()"""
        te = self.event_time()
        return te + 1e-9 if t < te else G_MAXINT


# ---------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------

def _grids(dim, n):
    """x, y(, z) of the cell centres, ghosts included, for arrays indexed [k, j, i] / [j, i]"""
    c = (np.arange(n + 2) - 0.5) / n - 0.5
    g = np.meshgrid(*([c] * dim), indexing="ij")
    return [g[dim - 1 - comp] for comp in range(dim)]


def _smooth(xyz, k):
    tp = 2. * np.pi
    a = np.sin(tp * (xyz[0] + 0.07 * k)) * np.cos(tp * (xyz[1] - 0.11 * k))
    if len(xyz) == 3:
        a = a * np.cos(tp * (xyz[2] + 0.05 * k)) + 0.2 * np.sin(tp * (xyz[2] - 0.13 * k))
    return a + 0.1 * np.cos(tp * (xyz[1] + 0.3 * k))


def face_mask(dim, n):
    """the cells of an (n + 2)^dim array that exist in the reference: the leaves and the ghost cells
    across a FACE of the box (the boundary "ghost trees" hold no edge or corner cells)"""
    idx = np.arange(n + 2)
    out = ((idx == 0) | (idx == n + 1)).astype(int)
    cnt = 0
    for ax in range(dim):
        sh = [1] * dim
        sh[ax] = n + 2
        cnt = cnt + out.reshape(sh)
    return cnt <= 1


def interior(a):
    return a[(slice(1, -1),) * a.ndim]


def random_state(case, seed=1):
    """name -> array with ghosts: U, g, gmac, un per component, P, Pmac, tracers T0, T1.  The MAC
    velocity un[c] is stored the way the device does: entry (i, j, k) is the + face of the cell along c,
    entry 0 along c the - face of the first cell."""
    dim, n = case.dim, case.n
    rng = np.random.default_rng(seed)
    xyz = _grids(dim, n)
    shape = (n + 2,) * dim
    st = {}
    k = 0
    for c in range(dim):
        for name, amp, noise in (("U", 1., 0.05), ("g", 0.5, 0.02), ("gmac", 0.5, 0.02)):
            k += 1
            st["%s%d" % (name, c)] = amp * _smooth(xyz, k) + noise * rng.standard_normal(shape)
        k += 1
        face = [q + (0.5 / n if comp == c else 0.) for comp, q in enumerate(xyz)]
        un = _smooth(face, k) + 0.05 * rng.standard_normal(shape)
        ax = dim - 1 - c
        lo, hi = [slice(None)] * dim, [slice(None)] * dim
        lo[ax], hi[ax] = 0, n
        if case.side[2 * c] == O.SIDE_BOUNDARY:      # no flow through a wall
            un[tuple(lo)] = 0.
            un[tuple(hi)] = 0.
        else:                                         # the - face of the first cell is the + face of the last
            un[tuple(lo)] = un[tuple(hi)]
        st["un%d" % c] = un
    for name, amp, noise in (("P", 0.3, 0.02), ("Pmac", 0.3, 0.02), ("T0", 0.5, 0.05), ("T1", 0.5, 0.05)):
        k += 1
        st[name] = amp * _smooth(xyz, k) + noise * rng.standard_normal(shape)
    return st


def alpha_faces(case):
    """a smooth positive alpha = 1/rho at the face centres, in the layout of gfs_poisson_coefficients'
    alpha (the entry of a cell is its + face along c, entry 0 the - face of the first cell)"""
    dim, n = case.dim, case.n
    xyz = _grids(dim, n)
    out = []
    for c in range(dim):
        face = [q + (0.5 / n if comp == c else 0.) for comp, q in enumerate(xyz)]
        rho = 1. + 0.4 * np.sin(2. * np.pi * face[0]) * np.cos(2. * np.pi * face[1])
        if dim == 3:
            rho = rho + 0.2 * np.cos(2. * np.pi * face[2])
        a = 1. / rho
        if case.side[2 * c] != O.SIDE_BOUNDARY:
            ax = dim - 1 - c
            lo, hi = [slice(None)] * dim, [slice(None)] * dim
            lo[ax], hi[ax] = 0, n
            a[tuple(lo)] = a[tuple(hi)]
        out.append(a)
    return out


# ---------------------------------------------------------------------------------------------
# the two simulations
# ---------------------------------------------------------------------------------------------

def _configure(case, sim, BC_DIRICHLET, new_alpha_field):
    """the settings of a case on an oracle.Sim or a gfship.Simulation (same method names)"""
    dim, n = case.dim, case.n
    sim.advection_params.gradient = case.gradient
    for par in (sim.projection_params, sim.approx_projection_params):
        par.tolerance = 1e-6
        par.nitermax = 4       # a handful of cycles: every cycle is compared, none is needed to converge
    if case.sides == "lid":
        # test/lid: Dirichlet walls, the lid (top) moving along x
        for c in range(dim):
            for d in range(2 * dim):
                val = np.full(n ** (dim - 1), 1. if (c == 0 and d == 2) else 0.)
                sim.u[c].set_bc(d, BC_DIRICHLET, val)
    if case.visc:
        for c in range(dim):
            sim.set_viscosity(c, case.visc)
    if case.source:
        sim.set_source(1, case.source)
    sim.hook_tracers = []
    if case.tracers:
        sim.hook_tracers = [sim.add_tracer(gradient=1), sim.add_tracer(gradient=0)]
    if case.alpha:
        sim.hook_alpha = []
        for a in alpha_faces(case):
            sim.hook_alpha.append(new_alpha_field(a))
        sim.set_alpha(sim.hook_alpha)
    if case.event:
        sim.set_next_event(case.next_event)
    return sim


def oracle_sim(case):
    s = O.Sim(case.dim, case.level, case.oracle_side)

    def field(a):
        f = O.Field(s.dom, -1)
        f.leaf()[...] = a
        return f
    return _configure(case, s, O.BC_DIRICHLET, field)


def device_sim(case):
    """(domain, simulation); destroy both with destroy_device"""
    import gfship
    gd = gfship.Domain(case.dim, case.level, case.side)
    gs = gfship.Simulation(gd)
    if case.sides == "external":
        gd.comm_init(gfship.comm_unique_id(), 0, 1, (1, 1, 1))

    def field(a):
        f = gd.variable()
        f.upload(a)
        return f
    _configure(case, gs, gfship.BC_DIRICHLET, field)
    return gd, gs


def destroy_device(gd, gs):
    gs.destroy()
    gd.destroy()


def sim_fields(sim):
    """name -> field object of every variable of a simulation (either kind)"""
    dim = len(sim.u)
    f = {"P": sim.p, "Pmac": sim.pmac}
    for c in range(dim):
        f["U%d" % c], f["g%d" % c], f["gmac%d" % c] = sim.u[c], sim.g[c], sim.gmac[c]
    for k, t in enumerate(sim.hook_tracers):
        f["T%d" % k] = t
    return f


def _oracle_set_un(osim, c, a):
    """cell.f[2c].un = the + face, cell.f[2c + 1].un = the - face = the + face of the cell before"""
    dim = osim.dim
    osim.un(2 * c)[...] = a
    ax = dim - 1 - c
    dst, src = [slice(None)] * dim, [slice(None)] * dim
    dst[ax], src[ax] = slice(1, None), slice(0, -1)
    osim.un(2 * c + 1)[...] = 0.
    osim.un(2 * c + 1)[tuple(dst)] = a[tuple(src)]


def load_state(case, osim, gs, state, un=True, dt=None):
    """upload `state` into both simulations, then the conditions of every variable by the same call on
    both sides (gfs_domain_bc).  un = False leaves the device's MAC velocities alone (asking for their
    handle switches the lazy path of that simulation off).  dt: advection_params.dt of both."""
    L = case.level
    of, gf = sim_fields(osim), sim_fields(gs) if gs is not None else None
    for name, f in of.items():
        f.leaf()[...] = state[name]
        O.lib().go_bc(f.ptr, f.ptr, L)
        if gs is not None:
            gf[name].upload(state[name])
            gs.dom.bc(gf[name])
    if un:
        for c in range(case.dim):
            _oracle_set_un(osim, c, state["un%d" % c])
            if gs is not None:
                gs.mac_velocity(c).upload(state["un%d" % c])
    if dt is not None:
        osim.advection_params.dt = dt
        if gs is not None:
            gs.advection_params.dt = dt


# ---------------------------------------------------------------------------------------------
# the loop body of simulation_run from the pieces
# ---------------------------------------------------------------------------------------------

def pieces_step(sim):
    """src/simulation.c:479-548 (the order of go_sim_step, oracle/go_timestep.c) through the public
    pieces of an oracle.Sim or a gfship.Simulation: the MAC projection on Pmac's field (the reference
    swaps the storage of P and Pmac around it: P's conditions act on Pmac's values, so a case that
    sets a condition on P sets it on Pmac too), g = gmac in the first iteration"""
    dt = sim.dt
    sim.predicted_face_velocities()
    sim.mac_projection(sim.projection_params, dt / 2., sim.pmac, sim.gmac)
    g = sim.g if sim.i > 0 else sim.gmac
    sim.centered_velocity_advection(sim.gmac, g)
    sim.correct_centered_velocities(g, - dt)
    sim.coarse_init()
    sim.approximate_projection(sim.approx_projection_params, dt, sim.p, sim.g)
    sim.advance_time()
    sim.set_timestep()
    for t in sim.hook_tracers:
        sim.tracer_advection(t, sim.dt)


# ---------------------------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------------------------

def oracle_un_plus(osim, c):
    """the oracle's MAC velocities of component c in the device's layout (+ faces, entry 0 the - face
    of the first cell), on the faces that exist: tangential coordinates 1..n, normal 0..n"""
    dim, n = osim.dim, 1 << osim.depth
    sl = [slice(1, n + 1)] * dim
    sl[dim - 1 - c] = slice(0, n + 1)
    return osim.un(2 * c)[tuple(sl)], tuple(sl)


def snapshot(osim):
    """a copy of every variable of an oracle simulation (to compare two oracle runs)"""
    d = {name: [f.level(l).copy() for l in range(osim.depth + 1)] for name, f in sim_fields(osim).items()}
    for c in range(2 * osim.dim):
        d["un[%d]" % c] = osim.un(c).copy()
    d["t"], d["i"], d["dt"] = osim.t, osim.i, osim.dt
    return d


def snapshot_differences(a, b):
    out = []
    for k in a:
        if isinstance(a[k], list):
            if not all(np.array_equal(x, y) for x, y in zip(a[k], b[k])):
                out.append(k)
        elif isinstance(a[k], np.ndarray):
            if not np.array_equal(a[k], b[k]):
                out.append(k)
        elif a[k] != b[k]:
            out.append(k)
    return out


def differences(osim, gs, coarse=False, un=True):
    """names of everything that differs between an oracle and a device simulation, in a fixed order:
    t, i, dt; every variable on the leaves and, separately, on the ghost cells across the faces; the MAC
    velocities; with coarse = True the non-leaf levels of P, Pmac, U, V(, W) and the tracers
    (gfs_cell_coarse_init fills them)"""
    dim, L = osim.dim, osim.depth
    n = 1 << L
    out = []
    if osim.t != gs.t:
        out.append("t (%r, device %r)" % (osim.t, gs.t))
    if osim.i != gs.i:
        out.append("i (%r, device %r)" % (osim.i, gs.i))
    if osim.dt != gs.dt:
        out.append("dt (%r, device %r)" % (osim.dt, gs.dt))
    mask = face_mask(dim, n)
    ghosts = mask.copy()
    ghosts[(slice(1, -1),) * dim] = False
    of, gf = sim_fields(osim), sim_fields(gs)
    for name in of:
        a, b = of[name].leaf(), gf[name].download()
        if not np.array_equal(interior(a), interior(b)):
            out.append(name)
        if not np.array_equal(a[ghosts], b[ghosts]):
            out.append(name + " (ghost cells)")
        if coarse and name[0] in "PUT":
            for l in range(L):
                if not np.array_equal(interior(of[name].level(l)), interior(gf[name].download(l))):
                    out.append("%s (level %d)" % (name, l))
    if un:
        for c in range(dim):
            a, sl = oracle_un_plus(osim, c)
            if not np.array_equal(a, gs.un(c)[sl]):
                out.append("un[%d]" % c)
    return out


def norm_differences(onorm, gnorm, what):
    out = []
    if onorm.infty != gnorm.infty:
        out.append("%s.infty (%r, device %r)" % (what, onorm.infty, gnorm.infty))
    for k in ("first", "second"):
        a, b = getattr(onorm, k), getattr(gnorm, k)
        if abs(a - b) > RTOL_SUM * abs(a):
            out.append("%s.%s (%r, device %r)" % (what, k, a, b))
    return out


def params_differences(opar, gpar, what):
    out = []
    if opar.niter != gpar.niter:
        out.append("%s.niter (%d, device %d)" % (what, opar.niter, gpar.niter))
    out += norm_differences(opar.residual_before, gpar.residual_before, what + ".residual_before")
    out += norm_differences(opar.residual, gpar.residual, what + ".residual")
    return out
