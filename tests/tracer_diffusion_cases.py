"""Cases and helpers for the tests of GfsSourceDiffusion on a GfsVariableTracer
(gfs_tracer_advection_diffusion, src/timestep.c:1028-1055).

Where the expected bits come from (the oracle has no tracer with a MAC source, but it has the arithmetic):

  * zero flow: every flux is 0 times a face value, so rhs = T and the expected result is
    oracle.Sim.variable_diffusion (T, rhs, D, dt, par), i.e. go_variable_diffusion;
  * flow: the oracle's velocity slot 0 has the MAC source.  T goes into u[0] with T's conditions, the MAC
    velocities into un, gmac = 0, g = None, set_viscosity (0, D), T's parameters into diffusion_params (0);
    centered_velocity_advection (gmac, None) then leaves the result in u[0].  variable_sources reads the MAC
    velocities only, and (un*dt/h)*(upw - 0*dt/2) == (un*dt*upw)/h because h is a power of two.  No symmetry
    on the sides normal to x in this recipe: a velocity component changes sign there.

The oracle part needs no device; device_calls imports gfship.
"""
import functools

import numpy as np

import hook_cases as H
from oracle import oracle as O

D_DEFAULT, DT_DEFAULT = 0.05, 0.01


class TCase:
    """dim, level and the sides of T: periodic | dirichlet | neumann | symmetry (all four or six sides),
    dn (Neumann values in x, Dirichlet values elsewhere), mixed (3-D: x periodic, y Dirichlet values,
    front Neumann values, back symmetry)"""

    def __init__(self, dim, level, sides="periodic"):
        self.dim, self.level, self.sides = dim, level, sides

    def __hash__(self):
        return hash((self.dim, self.level, self.sides))

    def __eq__(self, o):
        return (self.dim, self.level, self.sides) == (o.dim, o.level, o.sides)

    @property
    def id(self):
        return "%dd-%d-%s" % (self.dim, 1 << self.level, self.sides)

    @property
    def n(self):
        return 1 << self.level

    @property
    def side(self):
        if self.sides == "periodic":
            return [O.SIDE_PERIODIC] * 6
        if self.sides == "mixed":
            return [O.SIDE_PERIODIC] * 2 + [O.SIDE_BOUNDARY] * 4
        return [O.SIDE_BOUNDARY] * 6

    def conditions(self):
        """{d: (kind, values)} of T, the same for the oracle and the device (the BC_* numbers agree)"""
        rng = np.random.default_rng(7)
        m = self.n ** (self.dim - 1)
        val = {d: 0.3 * rng.standard_normal(m) for d in range(2 * self.dim)}
        if self.sides == "dirichlet":
            return {d: (O.BC_DIRICHLET, val[d]) for d in range(2 * self.dim)}
        if self.sides == "neumann":
            return {d: (O.BC_NEUMANN, val[d]) for d in range(2 * self.dim)}
        if self.sides == "dn":
            return {d: (O.BC_NEUMANN if d < 2 else O.BC_DIRICHLET, val[d]) for d in range(2 * self.dim)}
        if self.sides == "mixed":
            return {2: (O.BC_DIRICHLET, val[2]), 3: (O.BC_DIRICHLET, val[3]), 4: (O.BC_NEUMANN, val[4])}
        return {}

    def hook_case(self):
        """the hook_cases.Case whose random_state gives T and MAC velocities for this box (no flow through a
        wall, the - face of the first cell the + face of the last on a periodic box)"""
        assert self.sides != "mixed"
        return H.Case(self.dim, self.level, "periodic" if self.sides == "periodic" else "lid")


@functools.lru_cache(maxsize=None)
def fields(case, amp=0.3):
    """(T0 with ghosts, [un per component] in the device's layout), read-only"""
    if case.sides == "mixed":
        st = H.random_state(H.Case(case.dim, case.level, "periodic"), seed=3)
        T0, un = st["T0"], None
    else:
        st = H.random_state(case.hook_case(), seed=3)
        T0, un = st["T0"], [amp * st["un%d" % c] for c in range(case.dim)]
        for a in un:
            a.setflags(write=False)
    T0.setflags(write=False)
    return T0, un


def cosine_mode(case):
    """prod_c cos (2 pi x_c) with ghosts, and the eigenvalue of the discrete Laplacian on it"""
    xyz = H._grids(case.dim, case.n)
    T0 = np.ones_like(xyz[0])
    for q in xyz:
        T0 = T0 * np.cos(2. * np.pi * q)
    h = 1. / case.n
    lam = - case.dim * (2. / h ** 2) * (1. - np.cos(2. * np.pi * h))
    return T0, lam


def growth(lam, D, dt, beta):
    """what one call multiplies the mode by"""
    if beta == 1.:
        return 1. / (1. - D * dt * lam)
    assert beta == 0.5
    return (1. + D * dt * lam / 2.) / (1. - D * dt * lam / 2.)


def stats(par):
    return (par.niter, par.residual.infty, par.residual_before.infty)


def _set_conditions(case, f):
    for d, (kind, val) in case.conditions().items():
        f.set_bc(d, kind, val)


# ---------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------

def oracle_zero_flow(case, T0, D, dt, beta, tolerance, ncalls=1):
    """[(interior of T, stats)] after each of ncalls calls of variable_diffusion with rhs = T"""
    s = O.Sim(case.dim, case.level, case.side)
    T, rhs = O.Field(s.dom, -1), O.Field(s.dom, -1)
    _set_conditions(case, T)
    T.leaf()[...] = T0
    O.lib().go_bc(T.ptr, T.ptr, case.level)
    par = s.dom.params()
    par.tolerance, par.beta = tolerance, beta
    out = []
    for _ in range(ncalls):
        rhs.leaf()[...] = T.leaf()
        s.variable_diffusion(T, rhs, D, dt, par)
        out.append((T.interior().copy(), stats(par)))
    return out


def oracle_flow(case, T0, un, D, dt, gradient, beta=1., tolerance=1e-6, ncalls=3):
    """the velocity-slot recipe: [(interior of T, stats)] after each call.  D = 0.: plain advection."""
    assert case.side[0] == O.SIDE_PERIODIC or case.sides in ("dirichlet", "neumann", "dn")
    s = O.Sim(case.dim, case.level, case.side)
    _set_conditions(case, s.u[0])
    s.u[0].leaf()[...] = T0
    O.lib().go_bc(s.u[0].ptr, s.u[0].ptr, case.level)
    for c in range(case.dim):
        H._oracle_set_un(s, c, un[c])
        s.gmac[c].leaf()[...] = 0.
    s.advection_params.gradient = gradient
    s.advection_params.dt = dt
    s.set_viscosity(0, D)
    par = s.diffusion_params(0)
    par.tolerance, par.beta = tolerance, beta
    out = []
    for _ in range(ncalls):
        s.centered_velocity_advection(s.gmac, None)
        out.append((s.u[0].interior().copy(), stats(par) if D else None))
    return out


def oracle_tracer_advection(case, T0, un, dt, gradient, ncalls=3):
    """go_tracer_advection: the tracer without diffusion"""
    s = O.Sim(case.dim, case.level, case.side)
    T = s.add_tracer(gradient=gradient)
    _set_conditions(case, T)
    T.leaf()[...] = T0
    O.lib().go_bc(T.ptr, T.ptr, case.level)
    for c in range(case.dim):
        H._oracle_set_un(s, c, un[c])
    out = []
    for _ in range(ncalls):
        s.tracer_advection(T, dt)
        out.append(T.interior().copy())
    return out


# the expected results, computed once and shared between the tests
@functools.lru_cache(maxsize=None)
def expected_zero_flow(case, beta, D=D_DEFAULT, dt=DT_DEFAULT, tolerance=1e-6, ncalls=1):
    return oracle_zero_flow(case, fields(case)[0], D, dt, beta, tolerance, ncalls)


@functools.lru_cache(maxsize=None)
def expected_flow(case, gradient, beta=1., D=D_DEFAULT, dt=DT_DEFAULT, tolerance=1e-6, ncalls=3):
    T0, un = fields(case)
    return oracle_flow(case, T0, un, D, dt, gradient, beta, tolerance, ncalls)


# ---------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------

def device_calls(case, T0, un, D, dt, gradient=1, beta=1., tolerance=1e-6, ncalls=1, scheme=None, path=1):
    """ncalls calls of gfship_tracer_advection on one tracer: ([(interior of T, stats)], counts).
    un = None: the MAC velocities stay the zeros of a fresh simulation."""
    import gfship
    gd = gfship.Domain(case.dim, case.level, case.side)
    gs = gfship.Simulation(gd)
    try:
        T = gs.add_tracer(gradient=gradient)
        _set_conditions(case, T)
        T.upload(T0)
        gd.bc(T)
        if un is not None:
            for c in range(case.dim):
                gs.mac_velocity(c).upload(un[c])
        gs.set_tracer_diffusion(T, D)
        if scheme is not None:
            gs.set_tracer_scheme(T, scheme)
        gs.tracer_diffusion_path(path)
        par = gs.tracer_diffusion_params(T)
        par.tolerance, par.beta = tolerance, beta
        out = []
        for _ in range(ncalls):
            gs.tracer_advection(T, dt)
            out.append((H.interior(T.download()).copy(), stats(par) if D else None))
        return out, gs.tracer_diffusion_counts()
    finally:
        H.destroy_device(gd, gs)


def mismatches(expected, got):
    """what differs between two lists of (interior of T, stats), call by call"""
    out = []
    for k, ((a, sa), (b, sb)) in enumerate(zip(expected, got)):
        if not np.array_equal(a, b):
            out.append("call %d: T differs in %d cells, by at most %.3e" % (k, np.count_nonzero(a != b), np.abs(a - b).max()))
        if sa != sb:
            out.append("call %d: (niter, residual.infty, residual_before.infty) %r, got %r" % (k, sa, sb))
    assert len(expected) == len(got)
    return out
