"""Set-ups shared by the tests of the GfsMultilevelParams a user can change (nrelax, erelax, minlevel,
omega): tests/test_multigrid_params_oracle_cpu.py pins the oracle's handling of them on a V-cycle composed
from the oracle's primitives, tests/test_gpu_multigrid_params.py pins the device on the oracle.

A set is (nrelax, erelax, minlevel, omega).  Level l of a cycle runs nrelax*erelax^(depth - l) sweeps
(src/poisson.c:1129-1160), the cycle starts on level minlevel from dp = 0.
"""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from poisson_cases import dirichlet_case

RTOL_SUM = 1e-12

# kinds of sides: the GfsBox sides and, per direction, the condition on u
SIDE_KINDS = {
    "periodic": ([O.SIDE_PERIODIC] * 6, [None] * 6),
    # walls alternating Dirichlet / Neumann
    "walls": ([O.SIDE_BOUNDARY] * 6, [O.BC_DIRICHLET, O.BC_NEUMANN] * 3),
    "dirichlet": ([O.SIDE_BOUNDARY] * 6, [O.BC_DIRICHLET] * 6),
    # SIDES["mixed"] of test_gpu_poisson.py
    "mixed": ([O.SIDE_PERIODIC] * 2 + [O.SIDE_BOUNDARY] * 4, [None] * 2 + [O.BC_NEUMANN] * 4),
}

# (dim, level, sides, nrelax, erelax, minlevel, omega, dia): the composed cycle against go_poisson_cycle
COMPOSED_SETS = [
    (2, 4, "walls", 4, 1, 0, 1., False),
    (2, 5, "walls", 3, 2, 1, 0.9, False),
    (2, 5, "periodic", 2, 3, 2, 1., True),
    (2, 4, "walls", 1, 1, 4, 0.9, True),
    (3, 4, "walls", 4, 2, 0, 0.9, False),
    (3, 4, "periodic", 5, 2, 2, 1., True),
    (3, 3, "walls", 2, 3, 3, 1., False),
]

# device cycles, 2-D level 6 and 3-D level 6
SETS_2D = [(4, 2, 0, 1.), (3, 2, 1, 0.9), (2, 3, 2, 0.9), (4, 1, 3, 1.), (1, 1, 6, 0.9)]
SETS_3D = [(4, 2, 0, 1.), (5, 2, 0, 1.), (3, 3, 4, 1.), (4, 1, 5, 1.), (2, 1, 6, 1.), (4, 2, 1, 0.9)]
# one domain, these in turn (omega = 1)
MIXED_ORDER = [(4, 1, 0), (5, 2, 0), (2, 1, 6), (4, 2, 0), (4, 1, 0), (3, 3, 4)]

# (dim, level, minlevel): the Dirichlet problem of poisson_cases.py with nrelax = 1 stalls, the rule
# `residual > before/1.1' of gfs_poisson_solve (src/poisson.c:1258-1262) raises minlevel
STALL_CASES = [(3, 6, 4), (3, 5, 3), (2, 5, 3), (2, 6, 4)]
STALL_NRELAX, STALL_TOLERANCE, STALL_NITERMAX = 1, 1e-9, 12


def sweeps(nrelax, erelax, minlevel, depth):
    """{level: sweeps} of one cycle"""
    return {l: nrelax * erelax ** (depth - l) for l in range(min(minlevel, depth), depth + 1)}


def set_params(par, nrelax, erelax, minlevel, omega=1., depth=None):
    par.nrelax, par.erelax, par.minlevel, par.omega = nrelax, erelax, minlevel, omega
    if depth is not None:
        par.depth = depth
    return par


@functools.lru_cache(maxsize=None)
def cycle_arrays(dim, level, kind, use_dia, seed=0):
    """the inputs of a cycle: u and rhs with ghosts, dia of every level, the values of the conditions"""
    rng = np.random.default_rng(31000 + 100 * dim + 10 * level + seed)
    n = 1 << level
    shape = (n + 2,) * dim
    a = dict(u=rng.standard_normal(shape), rhs=rng.standard_normal(shape))
    a["dia"] = [np.abs(rng.standard_normal(((1 << l) + 2,) * dim)) + 0.5 if use_dia
                else np.zeros(((1 << l) + 2,) * dim) for l in range(level + 1)]
    a["bc"] = [rng.standard_normal(n ** (dim - 1)) for d in range(2 * dim)]
    return a


@functools.lru_cache(maxsize=None)
def alpha_arrays(dim, level, kind):
    """face values of a GfsFunction alpha as _alpha_pair of test_gpu_poisson.py draws them: one array per
    component, the ghost entry in front of the first cell is its - face"""
    rng = np.random.default_rng(77 + 10 * dim + level)
    out = []
    for c in range(dim):
        a = 0.5 + rng.random(((1 << level) + 2,) * dim)
        if SIDE_KINDS[kind][0][2 * c] == O.SIDE_PERIODIC:
            ax = dim - 1 - c
            sl0, sln = [slice(None)] * dim, [slice(None)] * dim
            sl0[ax], sln[ax] = 0, -2
            a[tuple(sl0)] = a[tuple(sln)]
        a.setflags(write=False)
        out.append(a)
    return out


class OracleCycle:
    """u, rhs, dia, res on an oracle domain, u with its conditions applied and res = the residual"""

    def __init__(self, dim, level, kind, use_dia, seed=0, alpha=None):
        L = O.lib()
        side, bc = SIDE_KINDS[kind]
        a = cycle_arrays(dim, level, kind, use_dia, seed)
        self.dim, self.level = dim, level
        self.dom = O.Domain(dim, level, side)
        if alpha is None:
            L.go_poisson_coefficients(self.dom.ptr)
        else:
            self.alpha = []
            for arr in alpha:
                f = self.dom.field()
                f.leaf()[...] = arr
                self.alpha.append(f)
            self.dom.poisson_coefficients_alpha(self.alpha)
        self.u, self.rhs, self.dia, self.res = (self.dom.field() for _ in range(4))
        self.u.leaf()[...] = a["u"]
        self.rhs.leaf()[...] = a["rhs"]
        for l in range(level + 1):
            self.dia.level(l)[...] = a["dia"][l]
        for d in range(2 * dim):
            if bc[d] is not None:
                self.u.set_bc(d, bc[d], a["bc"][d])
        L.go_bc(self.u.ptr, self.u.ptr, level)
        L.go_residual(self.dom.ptr, dim, level, self.u.ptr, self.rhs.ptr, self.dia.ptr, self.res.ptr)
        self.par = self.dom.params()
        self.par.depth = level

    def cycle(self, nrelax, erelax, minlevel, omega=1.):
        set_params(self.par, nrelax, erelax, minlevel, omega)
        O.lib().go_poisson_cycle(self.dom.ptr, C.byref(self.par), self.u.ptr, self.rhs.ptr, self.dia.ptr,
                                 self.res.ptr)
        return self.u.leaf().copy(), self.res.interior().copy()


@functools.lru_cache(maxsize=None)
def oracle_cycles(dim, level, kind, use_dia, sets, seed=0, weighted=False):
    """[(u with ghosts, res interior) after every cycle] of the oracle running the sets (a tuple of
    (nrelax, erelax, minlevel, omega)) in turn on one problem (weighted: with the face weights of
    alpha_arrays): computed once, shared, not to be written to"""
    o = OracleCycle(dim, level, kind, use_dia, seed, alpha_arrays(dim, level, kind) if weighted else None)
    out = [o.cycle(*s) for s in sets]
    for u, r in out:
        u.setflags(write=False)
        r.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------
# gfs_poisson_cycle composed from the primitives of the oracle's ABI (go_residual, go_homogeneous_bc,
# go_relax, go_bc) with the restriction and the prolongation restated in numpy
# ---------------------------------------------------------------------------------------------

def _children(dim):
    """(offset along z, y, x) of child id in the interior of the finer level: bit 0 +x, bit 1 -y, bit 2 -z
    (ftt.h: the children of a cell are numbered from the top-left-front one)"""
    for cid in range(1 << dim):
        ix = cid & 1
        jy = 0 if cid & 2 else 1
        kz = 0 if cid & 4 else 1
        yield cid, ((kz, jy, ix) if dim == 3 else (jy, ix))


def restrict_from_below(fine, coarse, dim, dimension):
    """get_from_below_2D / _3D (src/poisson.c:1044-1068): the children summed in child-id order, halved
    in 3-D"""
    inner = (slice(1, -1),) * dim
    f = fine[inner]
    val = np.zeros_like(coarse[inner])
    for cid, off in _children(dim):
        val = val + f[tuple(slice(o, None, 2) for o in off)]
    coarse[inner] = val if dimension == 2 else val / 2.


def prolongate_from_above(coarse, fine, dim):
    """get_from_above (src/poisson.c:1005-1042): val = p + sum_c rel[c]*(g1 - g2)/2 with the gradients
    g1 = p(+c) - 1.*p, g2 = p(-c) - 1.*p of gfs_face_gradient on the parent's level and rel = -+ 1/4"""
    n = coarse.shape[0] - 2
    inner = (slice(1, -1),) * dim
    p = coarse[inner]
    h = []
    for c in range(dim):
        ax = dim - 1 - c
        hi = [slice(1, -1)] * dim
        lo = [slice(1, -1)] * dim
        hi[ax], lo[ax] = slice(2, n + 2), slice(0, n)
        g1 = coarse[tuple(hi)] - 1. * p
        g2 = coarse[tuple(lo)] - 1. * p
        h.append((g1 - g2) / 2.)
    f = fine[inner]
    for cid, off in _children(dim):
        rel = [(1. if cid & 1 else -1.) / 4., (-1. if cid & 2 else 1.) / 4., (-1. if cid & 4 else 1.) / 4.]
        val = p.copy()
        for c in range(dim):
            val = val + rel[c] * h[c]
        f[tuple(slice(o, None, 2) for o in off)] = val


def composed_cycle(o):
    """one gfs_poisson_cycle (src/poisson.c:1109-1178) on the fields of an OracleCycle with o.par"""
    L = O.lib()
    p, dim, depth = o.par, o.dim, o.par.depth
    dom, u, rhs, dia, res = o.dom, o.u, o.rhs, o.dia, o.res
    dp = dom.field()

    def relax_loop(l, nrelax):
        L.go_homogeneous_bc(dp.ptr, u.ptr, l)
        for _ in range(nrelax - 1):
            L.go_relax(dom.ptr, p.dimension, l, p.omega, dp.ptr, res.ptr, dia.ptr)
            L.go_homogeneous_bc(dp.ptr, u.ptr, l)
        L.go_relax(dom.ptr, p.dimension, l, p.omega, dp.ptr, res.ptr, dia.ptr)

    for l in range(depth - 1, -1, -1):
        restrict_from_below(res.level(l + 1), res.level(l), dim, p.dimension)
    minlevel = p.minlevel
    dp.level(minlevel)[...] = 0.
    for l in range(minlevel, depth + 1):
        if l > minlevel:
            prolongate_from_above(dp.level(l - 1), dp.level(l), dim)
        relax_loop(l, p.nrelax * p.erelax ** (depth - l))
    u.interior()[...] += dp.interior()
    L.go_bc(u.ptr, u.ptr, depth)
    L.go_residual(dom.ptr, p.dimension, depth, u.ptr, rhs.ptr, dia.ptr, res.ptr)


# ---------------------------------------------------------------------------------------------
# the solve of the Dirichlet problem of poisson_cases.py
# ---------------------------------------------------------------------------------------------

class OracleDirichlet:
    def __init__(self, dim, level, kind="dirichlet", seed=None):
        """kind dirichlet: test/poisson's problem; periodic: a random right-hand side of zero mean"""
        L = O.lib()
        self.dim, self.level = dim, level
        self.dom = O.Domain(dim, level, SIDE_KINDS[kind][0])
        self.P, self.div, self.res, self.dia = (self.dom.field() for _ in range(4))
        self.rhs, self.faces = solve_inputs(dim, level, kind)
        self.div.interior()[...] = self.rhs
        if kind == "dirichlet":
            for d, f in enumerate(self.faces):
                self.P.set_bc(d, O.BC_DIRICHLET, f)
        L.go_bc(self.P.ptr, self.P.ptr, level)
        L.go_poisson_coefficients(self.dom.ptr)
        self.par = self.dom.params()

    def solve(self, dt=1.):
        O.lib().go_poisson_solve(self.dom.ptr, C.byref(self.par), self.P.ptr, self.div.ptr, self.res.ptr,
                                 self.dia.ptr, dt)

    def hand_solve(self, dt=1.):
        """the loop of gfs_poisson_solve (src/poisson.c:1225-1269) over go_poisson_cycle: the list of the
        minlevel every cycle ran with"""
        L = O.lib()
        par = self.par
        used = []
        minlevel = par.minlevel
        par.depth = self.level
        par.niter = 0
        L.go_residual(self.dom.ptr, par.dimension, self.level, self.P.ptr, self.div.ptr, self.dia.ptr,
                      self.res.ptr)
        par.residual_before = par.residual = L.go_norm_residual(self.dom.ptr, dt, self.res.ptr)
        before = par.residual.infty
        while par.niter < par.nitermin or (par.residual.infty > par.tolerance and par.niter < par.nitermax):
            used.append(par.minlevel)
            L.go_poisson_cycle(self.dom.ptr, C.byref(par), self.P.ptr, self.div.ptr, self.dia.ptr, self.res.ptr)
            par.residual = L.go_norm_residual(self.dom.ptr, dt, self.res.ptr)
            if par.residual.infty == before:
                break
            if par.residual.infty > before / 1.1 and par.minlevel < par.depth:
                par.minlevel += 1
            before = par.residual.infty
            par.niter += 1
        par.minlevel = minlevel
        return used


@functools.lru_cache(maxsize=None)
def solve_inputs(dim, level, kind):
    if kind == "dirichlet":
        rhs, faces, _ = dirichlet_case(dim, level)
        return rhs, faces
    rng = np.random.default_rng(700 + level)
    rhs = rng.standard_normal(((1 << level),) * dim)
    rhs -= rhs.mean()
    return rhs / (1 << level) ** 2, None


def stall_params(par, minlevel):
    par.nrelax, par.minlevel = STALL_NRELAX, minlevel
    par.tolerance, par.nitermax = STALL_TOLERANCE, STALL_NITERMAX
    return par


@functools.lru_cache(maxsize=None)
def oracle_solve(dim, level, kind, nrelax, erelax, minlevel, tolerance, nitermax):
    """(P interior, res interior, niter, residual.infty, residual_before.infty, residual.first,
    residual.second, minlevel afterwards) of go_poisson_solve: computed once, shared"""
    o = OracleDirichlet(dim, level, kind)
    set_params(o.par, nrelax, erelax, minlevel)
    o.par.tolerance, o.par.nitermax = tolerance, nitermax
    o.solve()
    P, res = o.P.interior().copy(), o.res.interior().copy()
    P.setflags(write=False)
    res.setflags(write=False)
    return (P, res, o.par.niter, o.par.residual.infty, o.par.residual_before.infty, o.par.residual.first,
            o.par.residual.second, o.par.minlevel)
