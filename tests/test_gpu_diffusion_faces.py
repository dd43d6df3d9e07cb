"""Implicit diffusion with per-face coefficients and a variable density on the device
(gfship_diffusion_coefficients_faces, then gfship_diffusion_rhs / _residual / _cycle and gfship_diffusion
with the six face weights of every cell, RelaxOp kind 3) against the CPU oracle.

The oracle's diffusion pieces (oracle/go_diffusion.c) read whatever face weights are in the domain and
any rhoc field, and go_poisson_coefficients_alpha fills the weights of every level from leaf-face values
with the arithmetic of diffusion_coef and face_coeff_from_below (src/poisson.c:1280-1301, 826-853): it is
given fields holding (beta*dt)*D_face, the product the device forms, and rhoc levels holding 1./alpha.

Everything is compared with array_equal; the tree-reduced norm sums of the solve with the project's 1e-12.

Shapes: the smallest at which each kernel family is the one that runs -- 8^2 and 64^2 the one-workgroup LDS
loop, 128^2 (one case) relax_rows2d_kernel, 16^3 the LDS loop and the coarse end, 32^3 the first level of the
pipelined tile kernel, 128^3 (one case) the level the uniform coefficient sends to the 2 x 2 ring kernels.
"""
import ctypes as C

import numpy as np
import pytest

import gfship
import hook_cases as H
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DT = 0.1
RTOL_SUM = H.RTOL_SUM
SHAPES = [(2, 3), (2, 6), (3, 4), (3, 5)]
# Dirichlet sides in y, a Neumann and a symmetry side in x, the rest periodic
MIXED = [O.SIDE_BOUNDARY] * 4 + [O.SIDE_PERIODIC] * 2
MIXED_BC = [O.BC_NEUMANN, O.BC_SYMMETRY, O.BC_DIRICHLET, O.BC_DIRICHLET, None, None]


@pytest.fixture(scope="module", autouse=True)
def _oracle_signatures():
    O._sim_sigs(O.lib())


def _face_coefficient(dim, n, c, rng, side):
    """D at the + face of every cell along c (the ghost entry in front of the first cell: its - face):
    1e-2 (1 + 0.5 sin (2 pi x) cos (2 pi y)) plus seeded noise of +- 10 %"""
    xyz = H._grids(dim, n)
    face = [q + (0.5 / n if comp == c else 0.) for comp, q in enumerate(xyz)]
    tp = 2. * np.pi
    D = 1e-2 * (1. + 0.5 * np.sin(tp * face[0]) * np.cos(tp * face[1]))
    D = D + 1e-3 * rng.uniform(-1., 1., D.shape)
    if side[2 * c] == O.SIDE_PERIODIC:      # the - face of the first cell is the + face of the last
        ax = dim - 1 - c
        lo, hi = [slice(None)] * dim, [slice(None)] * dim
        lo[ax], hi[ax] = 0, n
        D[tuple(lo)] = D[tuple(hi)]
    return D


class Pair:
    """an oracle and a device domain with the same per-face coefficients, density and fields"""

    def __init__(self, dim, level, beta, side=H.PERIODIC, bc=None, seed=5, alpha=True, const=None):
        self.dim, self.level, self.beta = dim, level, beta
        n = 1 << level
        rng = np.random.default_rng(1000 * dim + 10 * level + seed)
        self.od = O.Domain(dim, level, side)
        self.gd = gfship.Domain(dim, level, side)
        self.of = {k: self.od.field() for k in ("u", "rhs", "rhoc", "res")}
        self.gf = {k: self.gd.variable() for k in ("u", "rhs", "rhoc", "res")}
        xyz = H._grids(dim, n)
        st = {"U%d" % k: H._smooth(xyz, k + 1) + 0.05 * rng.standard_normal((n + 2,) * dim) for k in range(2)}
        if bc is not None:
            for d in range(2 * dim):
                if bc[d] is not None:
                    val = rng.standard_normal(n ** (dim - 1)) if bc[d] != O.BC_SYMMETRY else None
                    self.of["u"].set_bc(d, bc[d], val)
                    self.gf["u"].set_bc(d, bc[d], val)
        for k, name in (("u", "U0"), ("rhs", "U1")):
            self.of[k].leaf()[...] = st[name]
            self.gf[k].upload(st[name])
            O.lib().go_bc(self.of[k].ptr, self.of[k].ptr, level)
            self.gd.bc(self.gf[k])
        # the coefficient at the faces: D on the device, (beta*dt)*D for the oracle
        self.D = [const * np.ones((n + 2,) * dim) if const is not None else
                  _face_coefficient(dim, n, c, rng, side) for c in range(dim)]
        self.gD = [self.gd.variable() for c in range(dim)]
        self.oD = [self.od.field() for c in range(dim)]
        cdt = beta * DT
        for c in range(dim):
            self.gD[c].upload(self.D[c])
            self.oD[c].leaf()[...] = cdt * self.D[c]
        # alpha at the cells of every level, a different seed per level
        self.alpha = None
        if alpha:
            self.alpha = [np.random.default_rng(77 + l + seed).uniform(0.5, 2., ((1 << l) + 2,) * dim)
                          for l in range(level + 1)]
            self.galpha = self.gd.variable()
            for l in range(level + 1):
                self.galpha.upload(self.alpha[l], l)

    def coefficients(self):
        self.od.poisson_coefficients_alpha(self.oD)
        for l in range(self.level + 1):
            self.of["rhoc"].level(l)[...] = 1. / self.alpha[l] if self.alpha else 1.
        self.gd.diffusion_coefficients_faces(self.gD, DT, self.gf["rhoc"],
                                             self.galpha if self.alpha else None, self.beta)

    def rhs(self):
        O.lib().go_diffusion_rhs(self.od.ptr, self.of["u"].ptr, self.of["rhs"].ptr, self.of["rhoc"].ptr, self.beta)
        self.gd.diffusion_rhs(self.gf["u"], self.gf["rhs"], self.gf["rhoc"], self.beta)

    def residual(self):
        of, gf = self.of, self.gf
        O.lib().go_diffusion_residual(self.od.ptr, of["u"].ptr, of["rhs"].ptr, of["rhoc"].ptr, of["res"].ptr)
        self.gd.diffusion_residual(gf["u"], gf["rhs"], gf["rhoc"], gf["res"])

    def cycle(self, levelmin=0, nrelax=4):
        of, gf = self.of, self.gf
        O.lib().go_diffusion_cycle(self.od.ptr, levelmin, self.level, nrelax, of["u"].ptr, of["rhs"].ptr,
                                   of["rhoc"].ptr, of["res"].ptr)
        self.gd.diffusion_cycle(levelmin, nrelax, gf["u"], gf["rhs"], gf["rhoc"], gf["res"])

    def same(self, what, keys=("u", "rhs", "res")):
        for k in keys:
            assert np.array_equal(self.of[k].interior(), H.interior(self.gf[k].download())), (what, k)

    def destroy(self):
        self.gd.destroy()


@pytest.mark.parametrize("dim,level", SHAPES)
@pytest.mark.parametrize("beta", [1., 0.5])
def test_coefficients_rhs_residual_cycle(dim, level, beta):
    """(a) the weights of every level and direction and rhoc of every level, (b) gfship_diffusion_rhs,
    (c) gfship_diffusion_residual, (d) gfship_diffusion_cycle (0, depth, 4) on u and res"""
    p = Pair(dim, level, beta)
    try:
        p.coefficients()
        for l in range(level + 1):
            for d in range(2 * dim):
                assert np.array_equal(H.interior(p.od.weight(d, l)), H.interior(p.gd.poisson_weight(d, l))), (l, d)
            assert np.array_equal(H.interior(1. / p.alpha[l]), H.interior(p.gf["rhoc"].download(l))), ("rhoc", l)
        w = H.interior(p.od.weight(0, level))
        assert w.min() > 0. and w.max() > 1.5 * w.min()
        p.rhs()
        p.same("rhs", ("rhs",))
        p.residual()
        p.same("residual")
        assert np.abs(p.of["res"].interior()).max() > 0.
        p.cycle()
        p.same("cycle")
        if (dim, level) == (3, 5):
            assert p.gd.kernel_counts()["DIFFUSION_FACES_PIPELINED"] > 0
            assert p.gd.kernel_counts()["DIFFUSION_PIPELINED"] == 0
    finally:
        p.destroy()


def test_cycle_at_128_cubed_stays_off_the_ring_kernels():
    """(d) at 128^3, one cycle: the level the uniform coefficient sends to the 2 x 2 ring kernels, which
    know no per-cell weights"""
    p = Pair(3, 7, 1.)
    try:
        p.coefficients()
        p.rhs()
        p.residual()
        p.cycle()
        p.same("cycle")
        kc = p.gd.kernel_counts()
        assert kc["DIFFUSION_FACES_PIPELINED"] > 0
        assert kc["PATCH_LOOP_HOST_ARMS"] == 0 and kc["PATCH_LOOP_KERNEL_ARMS"] == 0
    finally:
        p.destroy()


def test_cycle_by_hyperplanes(monkeypatch):
    """kind 3 follows GFSHIP_WEIGHTED_HYPERPLANES as kind 2 does: the 32^3 level by relax_hyperplane_kernel,
    one launch per hyperplane (the switches are read when the domain is created)"""
    monkeypatch.setenv("GFSHIP_WEIGHTED_HYPERPLANES", "1")
    p = Pair(3, 5, 0.5)
    try:
        p.coefficients()
        p.rhs()
        p.residual()
        p.cycle()
        p.same("cycle")
        kc = p.gd.kernel_counts()
        assert kc["DIFFUSION_FACES_HYPERPLANES"] > 0 and kc["DIFFUSION_FACES_PIPELINED"] == 0
    finally:
        p.destroy()


@pytest.mark.parametrize("rows", [True, False])
def test_cycle_at_128_squared_by_rows_and_by_hyperplanes(monkeypatch, rows):
    """kind 3 in 2-D on a level that does not fit the one-workgroup LDS loop (64^2 and less do): one launch
    per sweep by relax_rows2d_kernel<3>, and with GFSHIP_NO_ROWS2D relax_hyperplane_kernel<2, 3>"""
    if not rows:
        monkeypatch.setenv("GFSHIP_NO_ROWS2D", "1")
    p = Pair(2, 7, 0.5)
    try:
        p.coefficients()
        p.rhs()
        p.residual()
        p.cycle()
        p.same("cycle")
        kc = p.gd.kernel_counts()
        assert kc["ROWS2D" if rows else "HYPERPLANES_2D"] > 0 and kc["HYPERPLANES_2D" if rows else "ROWS2D"] == 0
    finally:
        p.destroy()


def test_uniform_coefficient_after_a_weighted_poisson_call_at_128_cubed():
    """the kernel of a diffusion level is chosen by the coefficients of the diffusion call: a uniform
    coefficient runs on the 2 x 2 ring kernels at 128^3 although the last Poisson call left per-face weights
    on the domain, and gives the oracle's bits"""
    p = Pair(3, 7, 1., alpha=False, const=1e-2)
    try:
        rng = np.random.default_rng(3)
        oa, ga = [], []
        for c in range(3):
            a = 0.5 + rng.random(((1 << 7) + 2,) * 3)
            of, gf = p.od.field(), p.gd.variable()
            of.leaf()[...] = a
            gf.upload(a)
            oa.append(of)
            ga.append(gf)
        p.od.poisson_coefficients_alpha(oa)
        p.gd.poisson_coefficients_alpha(ga)
        O.lib().go_diffusion_coefficients(p.od.ptr, 1e-2, DT, 1., p.of["rhoc"].ptr)
        p.gd.diffusion_coefficients(1e-2, DT, p.gf["rhoc"], 1.)
        p.residual()
        p.cycle()
        p.same("cycle")
        kc = p.gd.kernel_counts()
        assert kc["DIFFUSION_PIPELINED"] > 0 and kc["PATCH_LOOP_HOST_ARMS"] + kc["PATCH_LOOP_KERNEL_ARMS"] > 0
    finally:
        p.destroy()


def _oracle_diffusion(p, par):
    """the loop of gfs_diffusion (src/timestep.c:735-788) as go_variable_diffusion runs it, over the oracle's
    cycle and norm"""
    L = O.lib()
    of = p.of
    minlevel, maxlevel = par.minlevel, p.level
    L.go_diffusion_residual(p.od.ptr, of["u"].ptr, of["rhs"].ptr, of["rhoc"].ptr, of["res"].ptr)
    par.residual = L.go_norm_variable(p.od.ptr, of["res"].ptr)
    par.residual_before = par.residual
    res_max_before = par.residual.infty
    par.niter = 0
    while par.niter < par.nitermin or (par.residual.infty > par.tolerance and par.niter < par.nitermax):
        L.go_diffusion_cycle(p.od.ptr, minlevel, maxlevel, par.nrelax, of["u"].ptr, of["rhs"].ptr,
                             of["rhoc"].ptr, of["res"].ptr)
        par.residual = L.go_norm_variable(p.od.ptr, of["res"].ptr)
        if par.residual.infty == res_max_before:
            break
        if par.residual.infty > res_max_before / 1.1 and minlevel < maxlevel:
            minlevel += 1
        res_max_before = par.residual.infty
        par.niter += 1


@pytest.mark.parametrize("dim,level", SHAPES)
@pytest.mark.parametrize("beta", [1., 0.5])
def test_diffusion_solve(dim, level, beta):
    """(e) gfship_diffusion: same niter, same residual.infty, same u"""
    p = Pair(dim, level, beta)
    try:
        p.coefficients()
        p.rhs()
        op, gp = p.od.params(), p.gd.params()
        for par in (op, gp):
            par.tolerance, par.beta = 1e-6, beta
        _oracle_diffusion(p, op)
        p.gd.diffusion(gp, p.gf["u"], p.gf["rhs"], p.gf["rhoc"])
        assert gp.niter == op.niter and op.niter >= 1
        assert gp.residual.infty == op.residual.infty
        assert gp.residual_before.infty == op.residual_before.infty
        for name in ("first", "second"):
            assert getattr(gp.residual, name) == pytest.approx(getattr(op.residual, name), rel=RTOL_SUM, abs=0.)
        p.same("solve", ("u",))
    finally:
        p.destroy()


@pytest.mark.parametrize("dim,level", [(3, 4), (2, 5), (3, 5)])
def test_cycle_with_dirichlet_neumann_and_symmetry_sides(dim, level):
    """(f) the cycle on a box with Dirichlet sides in y, a Neumann and a symmetry side in x and the rest
    periodic (32^3 as well: the pipelined tile kernel with sides that are not periodic)"""
    p = Pair(dim, level, 1., side=MIXED, bc=MIXED_BC)
    try:
        p.coefficients()
        p.rhs()
        p.residual()
        p.same("residual")
        p.cycle()
        p.same("cycle")
    finally:
        p.destroy()


@pytest.mark.parametrize("dim,level", [(3, 5), (2, 6)])
def test_constant_coefficient_gives_the_bits_of_the_uniform_path(dim, level):
    """(g) device against device: constant D fields and alpha_cell = -1 against gfship_diffusion_coefficients
    followed by a cycle -- both cell updates perform the same operations when every g = w"""
    D = 1e-2
    p = Pair(dim, level, 1., alpha=False, const=D)
    q = Pair(dim, level, 1., alpha=False, const=D)
    try:
        p.gd.diffusion_coefficients_faces(p.gD, DT, p.gf["rhoc"], None, 1.)
        q.gd.diffusion_coefficients(D, DT, q.gf["rhoc"], 1.)
        for g in (p, q):
            g.gd.diffusion_rhs(g.gf["u"], g.gf["rhs"], g.gf["rhoc"], 1.)
            g.gd.diffusion_residual(g.gf["u"], g.gf["rhs"], g.gf["rhoc"], g.gf["res"])
            g.gd.diffusion_cycle(0, 4, g.gf["u"], g.gf["rhs"], g.gf["rhoc"], g.gf["res"])
        for k in ("u", "rhs", "res"):
            assert np.array_equal(H.interior(p.gf[k].download()), H.interior(q.gf[k].download())), k
        for l in range(level + 1):
            assert np.array_equal(H.interior(p.gf["rhoc"].download(l)), H.interior(q.gf["rhoc"].download(l)))
        if dim == 3:
            assert p.gd.kernel_counts()["DIFFUSION_FACES_PIPELINED"] > 0
            assert q.gd.kernel_counts()["DIFFUSION_PIPELINED"] > 0
    finally:
        p.destroy()
        q.destroy()


def _poisson_fields(p, rng):
    """alpha at the faces and the fields of a weighted Poisson cycle on both domains of the pair"""
    dim, level = p.dim, p.level
    shape = ((1 << level) + 2,) * dim
    oa, ga = [], []
    for c in range(dim):
        a = 0.5 + rng.random(shape)
        of, gf = p.od.field(), p.gd.variable()
        of.leaf()[...] = a
        gf.upload(a)
        oa.append(of)
        ga.append(gf)
    f = {}
    for k in ("pu", "prhs", "pdia", "pres"):
        of, gf = p.od.field(), p.gd.variable()
        a = rng.standard_normal(shape)
        of.leaf()[...] = a
        gf.upload(a)
        f[k] = (of, gf)
    for l in range(level + 1):
        f["pdia"][0].level(l)[...] = 0.
        f["pdia"][1].fill(0., l)
    O.lib().go_bc(f["pu"][0].ptr, f["pu"][0].ptr, level)
    p.gd.bc(f["pu"][1])
    return oa, ga, f


def _poisson_cycle(p, f):
    dim, level = p.dim, p.level
    op, gp = p.od.params(), p.gd.params()
    for par in (op, gp):
        par.depth = level
    O.lib().go_residual(p.od.ptr, dim, level, f["pu"][0].ptr, f["prhs"][0].ptr, f["pdia"][0].ptr, f["pres"][0].ptr)
    p.gd.residual(f["pu"][1], f["prhs"][1], f["pdia"][1], f["pres"][1])
    O.lib().go_poisson_cycle(p.od.ptr, C.byref(op), f["pu"][0].ptr, f["prhs"][0].ptr, f["pdia"][0].ptr,
                             f["pres"][0].ptr)
    p.gd.poisson_cycle(gp, f["pu"][1], f["prhs"][1], f["pdia"][1], f["pres"][1])
    for k in ("pu", "pres"):
        assert np.array_equal(f[k][0].interior(), H.interior(f[k][1].download())), k


@pytest.mark.parametrize("first", ["poisson", "diffusion"])
def test_poisson_and_diffusion_coefficients_share_the_weights(first):
    """(h) the two coefficient routines overwrite the same arrays: each solver gets its own weights again
    after the other has run, the skewed copies of the pipelined kernel included (32^3), in either order"""
    p = Pair(3, 5, 1.)
    try:
        oa, ga, f = _poisson_fields(p, np.random.default_rng(31))

        def poisson():
            p.od.poisson_coefficients_alpha(oa)
            p.gd.poisson_coefficients_alpha(ga)
            _poisson_cycle(p, f)

        def diffusion():
            p.coefficients()
            p.residual()
            p.cycle()
            p.same("diffusion cycle")

        if first == "poisson":
            poisson()
        for _ in range(2):
            diffusion()
            poisson()
        kc = p.gd.kernel_counts()
        assert kc["DIFFUSION_FACES_PIPELINED"] > 0 and kc["WEIGHTED_PIPELINED"] > 0
    finally:
        p.destroy()


def test_refusals():
    """(i) a density <= 0 on any level is GFSHIP_EINVAL; a domain with MPI sides GFSHIP_EUNSUPPORTED"""
    p = Pair(3, 4, 1.)
    try:
        a = p.alpha[2].copy()
        a[2, 1, 3] = -0.5
        p.galpha.upload(a, 2)
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            p.gd.diffusion_coefficients_faces(p.gD, DT, p.gf["rhoc"], p.galpha, 1.)
        a[2, 1, 3] = 0.
        p.galpha.upload(a, 2)
        with pytest.raises(gfship.GfshipError, match="gfship error -1"):
            p.gd.diffusion_coefficients_faces(p.gD, DT, p.gf["rhoc"], p.galpha, 1.)
        p.galpha.upload(p.alpha[2], 2)
        p.gd.diffusion_coefficients_faces(p.gD, DT, p.gf["rhoc"], p.galpha, 1.)
    finally:
        p.destroy()
    gd = gfship.Domain(3, 4, H.EXTERNAL_X)
    try:
        D = [gd.variable() for c in range(3)]
        rhoc = gd.variable()
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gd.diffusion_coefficients_faces(D, DT, rhoc, None, 1.)
    finally:
        gd.destroy()
