"""The GfsMultilevelParams a user can change in a .gfs file -- nrelax, erelax, minlevel, omega -- on every
path of the device that takes them, against the CPU oracle (whose handling of them
tests/test_multigrid_params_oracle_cpu.py pins on a cycle composed from primitives): the V-cycle and the
solve of a uniform box with every kernel choice of the pipelined levels, the implicit diffusion, refined
trees, the time step, the .gfs front end and a lattice of boxes.

Fields (interior and face ghosts), niter and the maximum norms are compared with array_equal / ==, summed
norms with the suite's 1e-12.  Level l of a cycle runs nrelax*erelax^(depth - l) sweeps: with SK_MAXF = 8
(csrc/relax_skew.hpp) a 32^3 level with 9, 10 or 40 sweeps leaves the fused relax loop and goes sweep by
sweep in the skewed layout; a minlevel of 4, 5 or 6 takes the coarse end of a 64^3 cycle away from
coarse_cycle_kernel.  kernel_counts() says which branch ran.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gfship
import multigrid_param_cases as M
from oracle import oracle as O
from test_gpu_poisson import _faces_equal, _interior

pytestmark = pytest.mark.gpu
RTOL_SUM = M.RTOL_SUM
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin", "gfship2D")
CASES = os.path.join(ROOT, "tests", "cases")


@pytest.fixture(scope="module", autouse=True)
def _oracle_signatures():
    O._sim_sigs(O.lib())


class DeviceCycle:
    """the problem of M.OracleCycle on the device"""

    def __init__(self, dim, level, kind, use_dia, seed=0, weighted=False):
        side, bc = M.SIDE_KINDS[kind]
        a = M.cycle_arrays(dim, level, kind, use_dia, seed)
        self.dim, self.level = dim, level
        self.gd = gd = gfship.Domain(dim, level, side)
        if weighted:
            self.alpha = []
            for arr in M.alpha_arrays(dim, level, kind):
                v = gd.variable()
                v.upload(arr)
                self.alpha.append(v)
            gd.poisson_coefficients_alpha(self.alpha)
        else:
            gd.poisson_coefficients()
        self.u, self.rhs, self.dia, self.res = (gd.variable() for _ in range(4))
        self.u.upload(a["u"])
        self.rhs.upload(a["rhs"])
        for l in range(level + 1):
            if use_dia:
                self.dia.upload(a["dia"][l], l)
            else:
                self.dia.fill(0., l)
        for d in range(2 * dim):
            if bc[d] is not None:
                self.u.set_bc(d, bc[d], a["bc"][d])
        gd.bc(self.u)
        gd.residual(self.u, self.rhs, self.dia, self.res)
        self.par = gd.params()
        self.par.depth = level

    def cycle(self, nrelax, erelax, minlevel, omega=1.):
        M.set_params(self.par, nrelax, erelax, minlevel, omega)
        self.gd.poisson_cycle(self.par, self.u, self.rhs, self.dia, self.res)

    def same(self, expected, what):
        u, res = expected
        assert _faces_equal(u, self.u.download(), self.dim), what
        assert np.array_equal(res, _interior(self.res.download(), self.dim)), what

    def run(self, sets, expected):
        for k, (s, e) in enumerate(zip(sets, expected)):
            self.cycle(*s)
            self.same(e, (k, s))


# ---------------------------------------------------------------------------------------------
# gfship_poisson_cycle, uniform boxes
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("use_dia", [False, True])
@pytest.mark.parametrize("s", M.SETS_2D)
@pytest.mark.parametrize("kind", ["walls", "periodic"])
def test_cycle_2d_level_6(kind, s, use_dia):
    """coarse_cycle_kernel<2> from a level above the root and with omega, the LDS loop of the leaf level, a
    cycle of the leaf level alone"""
    level = 6
    expected = M.oracle_cycles(2, level, kind, use_dia, (s, s))
    d = DeviceCycle(2, level, kind, use_dia)
    try:
        d.run((s, s), expected)
        kc = d.gd.kernel_counts()
        # coarse_cycle_kernel takes the levels minlevel .. 5 where they are more than one
        coarse = s[2] < level - 1
        assert kc["COARSE_CYCLES"] == (2 if coarse else 0)
        assert kc["COARSE_END_BY_LEVEL"] == (0 if coarse else 2)
    finally:
        d.gd.destroy()


def test_omega_acts_in_2d_and_not_in_3d():
    """the reference's 3-D relax has no omega (src/poisson.c:527): the expected values of the 3-D set with
    omega = 0.9 are those of omega = 1, the 2-D ones are not"""
    a = M.oracle_cycles(3, 6, "periodic", False, ((4, 2, 1, 0.9),) * 2)
    b = M.oracle_cycles(3, 6, "periodic", False, ((4, 2, 1, 1.),) * 2)
    assert np.array_equal(a[1][0], b[1][0])
    a2 = M.oracle_cycles(2, 6, "periodic", False, ((3, 2, 1, 0.9),) * 2)
    b2 = M.oracle_cycles(2, 6, "periodic", False, ((3, 2, 1, 1.),) * 2)
    assert not np.array_equal(a2[1][0], b2[1][0])
    d = DeviceCycle(3, 6, "periodic", False)
    try:
        d.run(((4, 2, 1, 0.9),) * 2, b)
    finally:
        d.gd.destroy()


MODES = {"default": {}, "patch": {"GFSHIP_PATCH_MIN_N": "32"},
         "patch_regs": {"GFSHIP_PATCH_MIN_N": "32", "GFSHIP_PATCH_REGS": "1"}}
PIPELINED = (5, 6)      # the levels of a 64^3 box the pipelined tile kernels run


def _set_mode(monkeypatch, mode):
    """the switches are read when the domain is created"""
    for k in ("GFSHIP_PATCH_MIN_N", "GFSHIP_PATCH_REGS", "GFSHIP_SKEW_LINES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)


def _check_counts_3d(kc, mode, kind, s, cycles):
    """the branches of poisson_cycle (csrc/poisson.hip) a set selects on a 64^3 box"""
    nrelax, erelax, minlevel, _ = s
    L = 6
    # sweeps of level l as the cycle's table has them: levels below minlevel keep those of minlevel
    nrl = {l: nrelax * erelax ** (L - max(l, minlevel)) for l in range(L + 1)}
    fused_loop = lambda l: 2 <= nrl[l] <= 8
    # levels minlevel .. 4 in coarse_cycle_kernel where they are more than one
    coarse = minlevel < 4
    assert kc["COARSE_CYCLES"] == (cycles if coarse else 0)
    assert kc["COARSE_END_BY_LEVEL"] == (0 if coarse else cycles)
    above = [l for l in PIPELINED if l > minlevel]
    patched = mode != "default"
    if patched or kind == "periodic":
        assert kc["PROLONGATION_FUSED"] == cycles * len(above)
    else:
        assert kc["PROLONGATION_FUSED"] == 0
    assert kc["PROLONGATION_DECLINED"] == 0
    assert kc["RESTRICTION_DECLINED"] == 0
    if patched:
        assert kc["RESTRICTION_FUSED"] >= cycles
        # every launch of the loop kernels on a 2 x 2 level: one per fused loop, one per sweep otherwise
        launches = sum(1 if fused_loop(l) else nrl[l] for l in PIPELINED if l >= minlevel)
        assert kc["PATCH_LOOP_HOST_ARMS"] >= cycles * launches
        assert kc["PATCH_LOOP_KERNEL_ARMS"] == 0
    else:
        assert kc["RESTRICTION_FUSED"] == 0
        assert kc["PATCH_LOOP_HOST_ARMS"] == 0 and kc["PATCH_LOOP_KERNEL_ARMS"] == 0
    # the granules of a loop are armed ahead only for a loop the fused kernel runs, on the way down through the
    # levels the restriction visits: never for a count above SK_MAXF, never refused by the switch
    visited = [l + 1 for l in range(L - 1, (4 if coarse else -1), -1) if l + 1 in PIPELINED]
    assert kc["ARM_AHEAD"] <= cycles * sum(1 for l in visited if fused_loop(l))
    assert kc["ARM_AHEAD_DECLINED"] == 0
    if any(not fused_loop(l) for l in PIPELINED if l >= minlevel):
        assert kc["ARM_INLINE"] > 0


@pytest.mark.parametrize("s", M.SETS_3D)
@pytest.mark.parametrize("kind", ["periodic", "dirichlet", "mixed"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_cycle_3d_level_6(mode, kind, s, monkeypatch):
    """64^3, the smallest box with two pipelined levels: the sets of M.SETS_3D under the default kernels and the
    two 2 x 2 kernels on both levels"""
    _set_mode(monkeypatch, mode)
    expected = M.oracle_cycles(3, 6, kind, False, (s, s))
    d = DeviceCycle(3, 6, kind, False)
    try:
        d.run((s, s), expected)
        _check_counts_3d(d.gd.kernel_counts(), mode, kind, s, 2)
    finally:
        d.gd.destroy()


@pytest.mark.parametrize("kind", ["periodic", "mixed"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_cycle_3d_level_6_with_dia(mode, kind, monkeypatch):
    _set_mode(monkeypatch, mode)
    s = (5, 2, 0, 1.)
    expected = M.oracle_cycles(3, 6, kind, True, (s, s))
    d = DeviceCycle(3, 6, kind, True)
    try:
        d.run((s, s), expected)
        _check_counts_3d(d.gd.kernel_counts(), mode, kind, s, 2)
    finally:
        d.gd.destroy()


@pytest.mark.parametrize("s", [(5, 2, 0, 1.), (4, 1, 5, 1.)])
@pytest.mark.parametrize("kind", ["periodic", "dirichlet"])
def test_weighted_cycle_3d_level_6(kind, s):
    """face weights from alpha: 10 sweeps on the pipelined weighted kernel, and a cycle that starts on a pipelined
    level"""
    expected = M.oracle_cycles(3, 6, kind, False, (s, s), weighted=True)
    d = DeviceCycle(3, 6, kind, False, weighted=True)
    try:
        d.run((s, s), expected)
        kc = d.gd.kernel_counts()
        assert kc["WEIGHTED_PIPELINED"] == 2 * 2 and kc["WEIGHTED_HYPERPLANES"] == 0
        assert kc["COARSE_CYCLES"] == 0 and kc["COARSE_END_BY_LEVEL"] == 2
    finally:
        d.gd.destroy()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_sets_in_mixed_order_on_one_domain(mode, monkeypatch):
    """state that outlives a call: granule sets armed for another number of sweeps, residuals left in the layout
    of the 2 x 2 kernels, the trial runs, the flags of the cached dp"""
    _set_mode(monkeypatch, mode)
    sets = tuple(s + (1.,) for s in M.MIXED_ORDER)
    expected = M.oracle_cycles(3, 6, "periodic", False, sets)
    d = DeviceCycle(3, 6, "periodic", False)
    try:
        d.run(sets, expected)
    finally:
        d.gd.destroy()


# ---------------------------------------------------------------------------------------------
# gfship_poisson_solve
# ---------------------------------------------------------------------------------------------

def _device_solve(dim, level, kind, nrelax, erelax, minlevel, tolerance, nitermax):
    n = 1 << level
    rhs, faces = M.solve_inputs(dim, level, kind)
    gd = gfship.Domain(dim, level, M.SIDE_KINDS[kind][0])
    try:
        P, div, res, dia = (gd.variable() for _ in range(4))
        a = np.zeros((n + 2,) * dim)
        a[(slice(1, -1),) * dim] = rhs
        div.upload(a)
        if kind == "dirichlet":
            for d, fv in enumerate(faces):
                P.set_bc(d, gfship.BC_DIRICHLET, fv)
        gd.bc(P)
        gd.poisson_coefficients()
        par = gd.params()
        M.set_params(par, nrelax, erelax, minlevel)
        par.tolerance, par.nitermax = tolerance, nitermax
        gd.poisson_solve(par, P, div, res, dia, 1.)
        return par, _interior(P.download(), dim), _interior(res.download(), dim)
    finally:
        gd.destroy()


def _same_solve(dim, level, kind, *args):
    oP, ores, niter, infty, before, first, second, _ = M.oracle_solve(dim, level, kind, *args)
    par, P, res = _device_solve(dim, level, kind, *args)
    print("niter %d (oracle %d), residual %.17g (oracle %.17g)" % (par.niter, niter, par.residual.infty, infty))
    assert par.niter == niter
    assert par.residual.infty == infty
    assert par.residual_before.infty == before
    assert par.residual.first == pytest.approx(first, rel=RTOL_SUM, abs=0.)
    assert par.residual.second == pytest.approx(second, rel=RTOL_SUM, abs=0.)
    assert np.array_equal(P, oP)
    assert np.array_equal(res, ores)
    assert par.minlevel == args[2]      # back at its input value
    return par


@pytest.mark.parametrize("dim,level,minlevel", M.STALL_CASES[:3])
def test_solve_with_the_stall_rule(dim, level, minlevel):
    """the problems on which test_multigrid_params_oracle_cpu.py shows the rule `residual > before/1.1' of
    gfs_poisson_solve to raise minlevel between the cycles"""
    _same_solve(dim, level, "dirichlet", M.STALL_NRELAX, 1, minlevel, M.STALL_TOLERANCE, M.STALL_NITERMAX)


@pytest.mark.parametrize("kind", ["periodic", "dirichlet"])
def test_solve_to_convergence_with_erelax_and_minlevel(kind):
    par = _same_solve(3, 5, kind, 4, 2, 1, 1e-9, 100)
    assert par.residual.infty <= 1e-9 and par.niter < 100


# ---------------------------------------------------------------------------------------------
# `dimension' that is not the domain's
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,level", [(3, 3), (2, 4)])
def test_a_dimension_that_is_not_the_domains_is_refused(dim, level):
    other = 5 - dim
    d = DeviceCycle(dim, level, "walls", False)
    try:
        u0 = d.u.download()
        def refused():      # GFSHIP_EUNSUPPORTED and its message
            return pytest.raises(gfship.GfshipError,
                                 match=r"gfship error -5: dimension %d on a %d-D domain" % (other, dim))
        with refused():
            d.gd.relax(d.u, d.rhs, d.dia, d=other)
        with refused():
            d.gd.residual(d.u, d.rhs, d.dia, d.res, d=other)
        d.par.dimension = other
        with refused():
            d.gd.poisson_cycle(d.par, d.u, d.rhs, d.dia, d.res)
        d.par.tolerance, d.par.nitermin, d.par.nitermax = 1e-30, 1, 1
        with refused():
            d.gd.poisson_solve(d.par, d.u, d.rhs, d.res, d.dia, 1.)
        assert np.array_equal(u0, d.u.download())
        # and the domain's own still runs
        d.par.dimension = dim
        d.run(((4, 1, 0, 1.),), M.oracle_cycles(dim, level, "walls", False, ((4, 1, 0, 1.),)))
    finally:
        d.gd.destroy()


# ---------------------------------------------------------------------------------------------
# implicit diffusion, uniform boxes
# ---------------------------------------------------------------------------------------------

def _diffusion_pair(dim, level, faces):
    """faces: per-face coefficients and a density (cell update kind 3); else one constant D (kind 1)"""
    from test_gpu_diffusion_faces import DT, Pair
    if faces:
        p = Pair(dim, level, 1.)
        p.coefficients()
    else:
        p = Pair(dim, level, 1., alpha=False, const=1e-2)
        O.lib().go_diffusion_coefficients(p.od.ptr, 1e-2, DT, 1., p.of["rhoc"].ptr)
        p.gd.diffusion_coefficients(1e-2, DT, p.gf["rhoc"], 1.)
    p.rhs()
    p.residual()
    return p


@pytest.mark.parametrize("nrelax", [1, 4])
@pytest.mark.parametrize("faces", [False, True], ids=["constant", "faces"])
def test_diffusion_cycles_3d_level_6(faces, nrelax):
    """gfs_diffusion_cycle runs 10*nrelax sweeps on levelmin: 10 and 40 on the pipelined 32^3 and 64^3 levels,
    beyond the fused loop; then nrelax on every level above"""
    p = _diffusion_pair(3, 6, faces)
    try:
        for levelmin in (0, 3, 5, 6):
            p.cycle(levelmin, nrelax)
            p.same("levelmin %d" % levelmin, ("u", "res"))
        kc = p.gd.kernel_counts()
        assert kc["DIFFUSION_FACES_PIPELINED" if faces else "DIFFUSION_PIPELINED"] > 0
        assert kc["DIFFUSION_FACES_HYPERPLANES"] == 0 and kc["DIFFUSION_HYPERPLANES"] == 0
    finally:
        p.destroy()


@pytest.mark.parametrize("faces", [False, True], ids=["constant", "faces"])
def test_diffusion_cycles_2d_level_6(faces):
    p = _diffusion_pair(2, 6, faces)
    try:
        for levelmin, nrelax in ((4, 4), (6, 4), (4, 1), (6, 1)):
            p.cycle(levelmin, nrelax)
            p.same("levelmin %d nrelax %d" % (levelmin, nrelax), ("u", "res"))
    finally:
        p.destroy()


@pytest.mark.parametrize("faces", [False, True], ids=["constant", "faces"])
def test_diffusion_solve_with_minlevel(faces):
    from test_gpu_diffusion_faces import _oracle_diffusion
    p = _diffusion_pair(3, 5, faces)
    try:
        op, gp = p.od.params(), p.gd.params()
        for par in (op, gp):
            par.tolerance, par.beta, par.minlevel, par.nrelax = 1e-6, 1., 3, 2
        _oracle_diffusion(p, op)
        p.gd.diffusion(gp, p.gf["u"], p.gf["rhs"], p.gf["rhoc"])
        assert gp.niter == op.niter and op.niter >= 1
        assert gp.residual.infty == op.residual.infty
        assert gp.residual_before.infty == op.residual_before.infty
        for name in ("first", "second"):
            assert getattr(gp.residual, name) == pytest.approx(getattr(op.residual, name), rel=RTOL_SUM, abs=0.)
        assert gp.minlevel == 3
        p.same("solve", ("u",))
    finally:
        p.destroy()


# ---------------------------------------------------------------------------------------------
# refined trees
# ---------------------------------------------------------------------------------------------

def _set_projections(trees, erelax, minlevel, nrelax):
    for t in trees:
        for p in (t.projection_params, t.approx_projection_params):
            p.erelax, p.minlevel, p.nrelax = erelax, minlevel, nrelax


def _same_projections(o, g, what, names=("projection_params", "approx_projection_params")):
    for name in names:
        po, pg = getattr(o, name), getattr(g, name)
        assert pg.niter == po.niter, (what, name, pg.niter, po.niter)
        assert pg.residual.infty == po.residual.infty, (what, name)


@pytest.mark.parametrize("erelax,minlevel,nrelax", [(2, 2, 4), (1, 3, 1), (1, 5, 4)])
def test_quadtree_steps(erelax, minlevel, nrelax):
    """the refined patch of test/periodic (levels 4 and 5): (1, 3, 1) needs tens of cycles per projection, (1, 5, 4)
    relaxes the finest level alone"""
    from test_gpu_tree import assert_same_leaves, periodic_pair
    o, g = periodic_pair(4, 1)
    try:
        _set_projections((o, g), erelax, minlevel, nrelax)
        o.start()
        g.start()
        assert g.dt == o.dt
        assert_same_leaves(o, g, "after the initial projection")
        _same_projections(o, g, "start", ("approx_projection_params",))
        for k in range(3):
            o.step()
            g.step()
            assert g.t == o.t and g.dt == o.dt, k
            _same_projections(o, g, "step %d" % k)
            assert_same_leaves(o, g, "step %d" % (k + 1))
        assert o.approx_projection_params.niter >= 1
    finally:
        o.destroy()
        g.destroy()


@pytest.mark.parametrize("switch", [None, "GFSHIP_TREE_NO_FLOW", "GFSHIP_TREE_TEMPLATE_RELAX"])
def test_octree_steps(switch, monkeypatch):
    """a cube with one extra level in an 8^3 octree, both projections with (erelax, minlevel, nrelax) = (2, 1, 4):
    16 and 32 sweeps on the coarse levels, through the dataflow program, the interpreted plan and the kernel that
    walks the tree (a tree looks its switches up when it is created)"""
    import test_gpu_tree as T
    for k in ("GFSHIP_TREE_NO_FLOW", "GFSHIP_TREE_TEMPLATE_RELAX"):
        monkeypatch.delenv(k, raising=False)
    if switch:
        monkeypatch.setenv(switch, "1")
    o, g = T._pair3("cube", 3, 1)
    try:
        _set_projections((o, g), 2, 1, 4)
        OT, G = O.Tree, gfship.Tree
        names = [(G.U, OT.U), (G.V, OT.V), (G.W, OT.W), (G.P, OT.P), (G.PMAC, OT.PMAC)] + \
            [(G.UN0 + d, OT.UN0 + d) for d in range(4)] + [(G.UN4, OT.UN4), (G.UN5, OT.UN5)]
        o.start()
        g.start()
        assert g.dt == o.dt
        _same_projections(o, g, "start", ("approx_projection_params",))
        T._same_leaves(o, g, names, "after the initial projection")
        for k in range(2):
            o.step()
            g.step()
            assert g.t == o.t and g.dt == o.dt
            _same_projections(o, g, "step %d" % k)
            T._same_leaves(o, g, names, "step %d" % (k + 1))
    finally:
        o.destroy()
        g.destroy()


def test_poisson_on_a_quadtree_with_boundaries():
    """test/poisson/circle at level 4 (Neumann sides, two extra levels in the circle), three cycles with
    erelax = 2 and minlevel = 1"""
    from test_gpu_tree import _circle_pair
    level, cycles = 4, 3
    o, g = _circle_pair(level, gfship.BC_NEUMANN)
    try:
        par = o.approx_projection_params
        par.tolerance, par.nitermin, par.nitermax = 1e-30, cycles, cycles
        par.erelax, par.minlevel = 2, 1
        o.poisson_run()
        for l in range(o.depth + 1):
            g.upload(gfship.Tree.DIV, l, o.values(O.Tree.GX, l))
        gp = gfship.MultilevelParams()
        gfship.lib().gfship_multilevel_params_init(gp, 2)
        gp.tolerance, gp.nitermin, gp.nitermax = 1e-30, cycles, cycles
        gp.erelax, gp.minlevel = 2, 1
        g.poisson_solve(gp)
        assert gp.niter == par.niter == cycles
        assert gp.residual.infty == par.residual.infty
        assert gp.residual_before.infty == par.residual_before.infty
        assert gp.minlevel == 1
        for l in range(o.depth + 1):
            leaf = o.flags(l)[1:-1, 1:-1] == 1
            a = g.download(gfship.Tree.P, l)[1:-1, 1:-1][leaf]
            b = o.values(O.Tree.P, l)[1:-1, 1:-1][leaf]
            assert np.array_equal(a, b), "P differs on level %d" % l
    finally:
        o.destroy()
        g.destroy()


def _viscous_steps(o, g, dim, nrelax, minlevel, nsteps):
    import test_gpu_tree as T
    OT, G = O.Tree, gfship.Tree
    names = [(G.U, OT.U), (G.V, OT.V), (G.P, OT.P), (G.PMAC, OT.PMAC)] + ([(G.W, OT.W)] if dim == 3 else [])
    for c in range(dim):
        for p in (o.diffusion_params(c), g.diffusion_params(c)):
            p.nrelax, p.minlevel = nrelax, minlevel
    o.start()
    g.start()
    assert g.dt == o.dt
    for k in range(nsteps):
        o.step()
        g.step()
        assert g.t == o.t and g.dt == o.dt, k
        T._same_leaves(o, g, names, "step %d" % k)
        for c in range(dim):
            pg, po = g.diffusion_params(c), o.diffusion_params(c)
            assert pg.niter == po.niter and pg.residual.infty == po.residual.infty, (k, c)
            assert pg.minlevel == minlevel
        assert max(o.diffusion_params(c).niter for c in range(dim)) >= 1


def test_implicit_viscosity_on_a_quadtree():
    """the lid-driven cavity refined by two levels in a corner, diffusion_params: nrelax = 2, minlevel = 2 (20 sweeps
    on level 2 of every cycle)"""
    from test_gpu_tree import _lid_pair
    level = 4
    o, g = _lid_pair(level, lambda x, y: level + 2 if (x > 0.2 and y > 0.2) else level)
    try:
        _viscous_steps(o, g, 2, 2, 2, 4)
    finally:
        o.destroy()
        g.destroy()


def test_implicit_viscosity_on_an_octree_forty_sweeps_on_a_fine_level():
    """Taylor-Green on the octree of test_gpu_tree_viscous_octree.py (levels 3 to 5): nrelax = 4 and
    minlevel = depth - 1, 40 sweeps on level 4 of every cycle.  A plan of 40 sweeps that the tree refuses would
    make the solve fail here"""
    from test_gpu_tree_viscous_octree import _pair
    o, g = _pair("taylor-green")
    try:
        _viscous_steps(o, g, 3, 4, o.depth - 1, 3)
    finally:
        o.destroy()
        g.destroy()


# ---------------------------------------------------------------------------------------------
# the time step and the front end
# ---------------------------------------------------------------------------------------------

def _sim_steps(osim, nsteps, nrelax, erelax, minlevel):
    from flow_cases import PERIODIC
    from test_gpu_timestep import _assert_same_state, _assert_same_un, _device_sim
    for p in (osim.projection_params, osim.approx_projection_params):
        p.nrelax, p.erelax, p.minlevel = nrelax, erelax, minlevel
    gd, gs = _device_sim(osim, PERIODIC)
    try:
        gs.set_time(end=osim.end)
        osim.start()
        gs.start()
        _assert_same_state(osim, gs, "start")
        for k in range(nsteps):
            osim.step()
            gs.step()
            _assert_same_state(osim, gs, "step %d" % k)
            _assert_same_un(osim, gs, "step %d" % k)
            for name in ("projection_params", "approx_projection_params"):
                po, pg = getattr(osim, name), getattr(gs, name)
                assert pg.niter == po.niter and po.niter >= 1, (k, name)
                assert pg.residual.infty == po.residual.infty, (k, name)
                assert pg.minlevel == minlevel
    finally:
        gs.destroy()
        gd.destroy()


def test_taylor_green_steps_with_erelax_and_minlevel():
    from flow_cases import oracle_taylor_green
    _sim_steps(oracle_taylor_green(5), 2, 3, 2, 1)


def test_reynolds_steps_with_minlevel():
    from flow_cases import oracle_reynolds
    _sim_steps(oracle_reynolds(5), 3, 2, 1, 2)


@pytest.mark.parametrize("nrelax,erelax,minlevel", [(3, 2, 1), (4, 1, 3)])
def test_front_end_reads_the_parameters(nrelax, erelax, minlevel):
    """tests/cases/multigrid_params.gfs through bin/gfship2D: the line `residual.infty:' of OutputProjectionStats
    shows the digits of go_poisson_solve with the same parameters"""
    level, cycles = 6, 3
    defs = dict(LEVEL=level, CYCLE=cycles, NRELAX=nrelax, ERELAX=erelax, MINLEVEL=minlevel)
    cmd = [BIN] + ["-D%s=%s" % kv for kv in defs.items()] + [os.path.join(CASES, "multigrid_params.gfs")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    res = [l.split() for l in r.stdout.splitlines() if l.split()[:1] == ["residual.infty:"]]
    _, _, niter, infty, before, _, _, _ = M.oracle_solve(2, level, "dirichlet", nrelax, erelax, minlevel, 1e-30, cycles)
    assert niter == cycles
    assert res[-1][1:3] == ["%.3e" % before, "%.3e" % infty], (res, before, infty)
    # ... which are not those of the defaults
    _, _, _, infty0, _, _, _, _ = M.oracle_solve(2, level, "dirichlet", 4, 1, 0, 1e-30, cycles)
    assert "%.3e" % infty0 != "%.3e" % infty


# ---------------------------------------------------------------------------------------------
# a lattice of boxes
# ---------------------------------------------------------------------------------------------

LATTICE = dict(nboxes=2, level=4, nsteps=2, params=(3, 2, 1))


def _lattice_state(sim, download):
    out = dict(p=download(sim.p), pmac=download(sim.pmac), dt=sim.dt, t=sim.t,
               niter=(sim.projection_params.niter, sim.approx_projection_params.niter),
               res=(sim.projection_params.residual.infty, sim.approx_projection_params.residual.infty))
    for c, name in enumerate("uvw"):
        out[name] = download(sim.u[c])
    return out


def _lattice_params(sim):
    for p in (sim.projection_params, sim.approx_projection_params):
        p.nrelax, p.erelax, p.minlevel = LATTICE["params"]


@pytest.fixture(scope="module")
def oracle_lattice():
    """two oracle boxes (one thread each, the exchange and reduce hooks over the in-process transport)"""
    import multibox as X
    from gfship import distributed as D
    nboxes, level, nsteps = LATTICE["nboxes"], LATTICE["level"], LATTICE["nsteps"]
    n = 1 << level
    grid = D.BoxGrid(nboxes, 3)

    def worker(rank, fabric):
        sim = O.Sim(3, level, grid.sides(rank))
        sim.dom.set_overlap(0)
        hooks = X.OracleHooks(O.lib(), sim.dom.ptr, 3, X.LocalTransport(grid, rank, fabric))
        for c, a in enumerate(X.lattice_velocity(*X.global_centres(grid, rank, n))):
            sim.u[c].interior()[...] = a
        _lattice_params(sim)
        sim.start()
        for _ in range(nsteps):
            sim.step()
        out = _lattice_state(sim, lambda f: f.interior().copy())
        del hooks
        return out

    return X.run_boxes(nboxes, worker)


@pytest.mark.parametrize("lattice_cycle", [True, False])
def test_lattice_of_two_boxes(lattice_cycle, oracle_lattice, monkeypatch):
    """2 x 1 x 1 boxes of 16^3, overlap = 0: the coarse end of the cycles from level 1 computed for the whole
    lattice after one gather (lattice_cycle_kernel), and with GFSHIP_NO_LATTICE_CYCLE=1 with one exchange per
    sweep and level"""
    import torch
    import multibox as X
    from gfship import distributed as D
    if lattice_cycle:
        monkeypatch.delenv("GFSHIP_NO_LATTICE_CYCLE", raising=False)
    else:
        monkeypatch.setenv("GFSHIP_NO_LATTICE_CYCLE", "1")
    nboxes, level, nsteps = LATTICE["nboxes"], LATTICE["level"], LATTICE["nsteps"]
    n = 1 << level
    grid = D.BoxGrid(nboxes, 3)
    dev = torch.device("cuda", 0)
    i3 = (slice(1, -1),) * 3

    def worker(rank, fabric):
        gd = gfship.Domain(3, level, grid.sides(rank))
        gs = gfship.Simulation(gd)
        hooks = D.DeviceHooks(gd, X.LocalTransport(grid, rank, fabric, dev))
        for c, a in enumerate(X.lattice_velocity(*X.global_centres(grid, rank, n))):
            b = np.zeros((n + 2,) * 3)
            b[i3] = a
            gs.u[c].upload(b)
        _lattice_params(gs)
        gs.start()
        for _ in range(nsteps):
            gs.step()
        gd.synchronize()
        out = _lattice_state(gs, lambda v: v.download()[i3])
        out["cycles"] = gd.path_counts()[0]
        del hooks
        gs.destroy()
        gd.destroy()
        return out

    got = X.run_boxes(nboxes, worker)
    for rank, (d, o) in enumerate(zip(got, oracle_lattice)):
        for name in ("u", "v", "w", "p", "pmac"):
            assert np.array_equal(d[name], o[name]), (rank, name)
        assert d["dt"] == o["dt"] and d["t"] == o["t"], rank
        assert tuple(d["niter"]) == tuple(o["niter"]) and min(o["niter"]) >= 1, rank
        assert d["res"] == o["res"], rank
        if lattice_cycle:
            assert d["cycles"] >= 2 * nsteps
        else:
            assert d["cycles"] == 0
    assert not np.array_equal(got[0]["u"], got[1]["u"])
