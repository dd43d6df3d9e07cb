"""The time step with a viscosity given at the faces (gfship_sim_set_viscosity_faces) and a variable
density in the implicit diffusion (gfship_sim_set_alpha + gfship_sim_set_alpha_cell):

  (a) gfship_variable_mac_source against source_diffusion_value (src/source.c:1105-1144) restated in numpy;
  (b) a constant coefficient given as face fields gives the bits of gfship_sim_set_viscosity;
  (c) the wiring inside a step: the implicit diffusion of gfship_centered_velocity_advection against the same
      solve written in the test from the solver's entry points (which tests/test_gpu_diffusion_faces.py pins
      on the oracle), with one coefficient per component, dt and alpha_cell; the MAC source in the predictor
      and in the CFL condition through an exact scaling of alpha_cell and D; and gfship_sim_step against the
      step written from the public pieces (hook_cases.pieces_step);
  (d) the refusals.

2-D 32^2, 3-D 16^3 (general kernels) and 32^3 (where a constant viscosity takes the fused sweeps and the
pipelined diffusion loop), three steps each.
"""
import numpy as np
import pytest

import gfship
import hook_cases as H
from hook_cases import Case

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5), (3, 4), (3, 5)]
NU = 1e-2


def _faces(case, rng=None, const=None):
    """the viscosity at the + face of every cell along c (entry 0: the - face of the first cell)"""
    dim, n = case.dim, case.n
    xyz = H._grids(dim, n)
    out = []
    for c in range(dim):
        if const is not None:
            out.append(np.full((n + 2,) * dim, const))
            continue
        face = [q + (0.5 / n if comp == c else 0.) for comp, q in enumerate(xyz)]
        D = NU * (1. + 0.5 * np.sin(2. * np.pi * face[0]) * np.cos(2. * np.pi * face[1]))
        D = D + 0.1 * NU * rng.uniform(-1., 1., D.shape)
        ax = dim - 1 - c
        lo, hi = [slice(None)] * dim, [slice(None)] * dim
        lo[ax], hi[ax] = 0, n
        D[tuple(lo)] = D[tuple(hi)]
        out.append(D)
    return out


def _alpha_cells(case):
    """alpha = 1/rho at the cell centres of every level (the function of hook_cases.alpha_faces)"""
    out = []
    for l in range(case.level + 1):
        xyz = H._grids(case.dim, 1 << l)
        rho = 1. + 0.4 * np.sin(2. * np.pi * xyz[0]) * np.cos(2. * np.pi * xyz[1])
        if case.dim == 3:
            rho = rho + 0.2 * np.cos(2. * np.pi * xyz[2])
        out.append(1. / rho)
    return out


class Run:
    """a device simulation in an uploaded state"""

    def __init__(self, case, D=None, nu=0., alpha=False, alpha_const=None):
        """D: the face arrays of the viscosity, one list for every component or one list per component;
        alpha: alpha at the faces and at the cells; alpha_const: alpha_cell alone, one value everywhere"""
        self.case = case
        self.gd = gd = gfship.Domain(case.dim, case.level, case.side)
        self.gs = gs = gfship.Simulation(gd)
        gs.hook_tracers = []
        for par in (gs.projection_params, gs.approx_projection_params):
            par.tolerance, par.nitermax = 1e-6, 4
        self.keep = []
        if alpha:
            self.alpha_cell = gd.variable()
            for l, a in enumerate(_alpha_cells(case)):
                self.alpha_cell.upload(a, l)
            gs.set_alpha_cell(self.alpha_cell)
            af = []
            for a in H.alpha_faces(case):
                f = gd.variable()
                f.upload(a)
                af.append(f)
            gs.set_alpha(af)
            self.keep += af
        if alpha_const is not None:
            self.alpha_cell = gd.variable()
            for l in range(case.level + 1):
                self.alpha_cell.fill(alpha_const, l)
            gs.set_alpha_cell(self.alpha_cell)
        if D is not None:
            per_component = isinstance(D[0], (list, tuple))
            self.Dc = []
            for c in range(case.dim):
                if c > 0 and not per_component:
                    self.Dc.append(self.Dc[0])
                    continue
                fields = []
                for a in (D[c] if per_component else D):
                    f = gd.variable()
                    f.upload(a)
                    fields.append(f)
                self.Dc.append(fields)
            self.D = self.Dc[0]
            for c in range(case.dim):
                gs.set_viscosity_faces(c, self.Dc[c])
        elif nu:
            for c in range(case.dim):
                gs.set_viscosity(c, nu)
        st = H.random_state(case, seed=4)
        for name, f in H.sim_fields(gs).items():
            f.upload(st[name])
            gd.bc(f)
        for c in range(case.dim):
            gs.mac_velocity(c).upload(st["un%d" % c])
        self.state = st

    def fields(self):
        out = {name: f.download() for name, f in H.sim_fields(self.gs).items()}
        for c in range(self.case.dim):
            out["un%d" % c] = self.gs.un(c)
        out["t"], out["dt"], out["i"] = self.gs.t, self.gs.dt, self.gs.i
        return out

    def destroy(self):
        H.destroy_device(self.gd, self.gs)


def _same(a, b, dim):
    diff = []
    for k in a:
        if isinstance(a[k], np.ndarray):
            if k.startswith("un"):
                c = int(k[2:])
                sl = [slice(1, -1)] * dim
                sl[dim - 1 - c] = slice(0, -1)
                ok = np.array_equal(a[k][tuple(sl)], b[k][tuple(sl)])
            else:
                ok = np.array_equal(H.interior(a[k]), H.interior(b[k]))
        else:
            ok = a[k] == b[k]
        if not ok:
            diff.append(k)
    return diff


def _shift(a, ax, s):
    """the neighbours at distance s along ax of the interior cells of a"""
    sl = [slice(1, -1)] * a.ndim
    sl[ax] = slice(1 + s, a.shape[ax] - 1 + s)
    return a[tuple(sl)]


def _source_diffusion_value(v, D, alpha, n):
    """source_diffusion_value, src/source.c:1105-1144, in its operation order: d = 0 .. 2 dim - 1"""
    dim = v.ndim
    v0 = H.interior(v)
    ga, gb = 0., 0.
    for c in range(dim):
        ax = dim - 1 - c
        for s in (1, -1):
            Df = _shift(D[c], ax, 0 if s == 1 else -1)      # gfs_source_diffusion_face
            ga = ga + Df * 1.                                # g.a += D*e.a
            gb = gb + Df * _shift(v, ax, s)                  # g.b += D*e.b
    h = 1. / n
    return alpha * (gb - ga * v0) / (h * h)


@pytest.mark.parametrize("dim,level", SHAPES)
@pytest.mark.parametrize("alpha", [False, True])
def test_variable_mac_source(dim, level, alpha):
    """(a)"""
    case = Case(dim, level)
    D = [_faces(case, np.random.default_rng(8 + c)) for c in range(dim)]      # one coefficient per component
    r = Run(case, D=D, alpha=alpha)
    try:
        out = r.gd.variable()
        al = H.interior(_alpha_cells(case)[level]) if alpha else 1.
        for c in range(dim):
            r.gs.variable_mac_source(c, out)
            u = r.gs.u[c].download()
            assert np.array_equal(H.interior(out.download()), _source_diffusion_value(u, D[c], al, case.n)), c
    finally:
        r.destroy()


@pytest.mark.parametrize("dim,level", SHAPES)
def test_constant_faces_give_the_bits_of_the_constant_viscosity(dim, level):
    """(b) three steps with set_viscosity_faces (const) and no alpha against set_viscosity (nu)"""
    case = Case(dim, level)
    a = Run(case, D=_faces(case, const=NU))
    b = Run(case, nu=NU)
    try:
        for r in (a, b):
            r.gs.start()
        assert _same(a.fields(), b.fields(), dim) == []
        for k in range(3):
            a.gs.step()
            b.gs.step()
            assert _same(a.fields(), b.fields(), dim) == [], k
        for c in range(dim):
            pa, pb = a.gs.diffusion_params(c), b.gs.diffusion_params(c)
            assert pa.niter == pb.niter >= 1 and pa.residual.infty == pb.residual.infty
        assert a.gd.kernel_counts()["ADVECT_GENERAL"] > 0
        if (dim, level) == (3, 5):
            assert a.gd.kernel_counts()["DIFFUSION_FACES_PIPELINED"] > 0
            assert b.gd.kernel_counts()["DIFFUSION_PIPELINED"] > 0 and b.gd.kernel_counts()["ADVECT_GENERAL"] == 0
    finally:
        a.destroy()
        b.destroy()


@pytest.mark.parametrize("dim,level", SHAPES)
def test_step_against_the_step_from_the_pieces(dim, level):
    """(c) a viscosity field, alpha and alpha_cell: gfship_sim_step against pieces_step"""
    case = Case(dim, level)
    D = _faces(case, np.random.default_rng(8))
    a = Run(case, D=D, alpha=True)
    b = Run(case, D=D, alpha=True)
    try:
        for r in (a, b):
            r.gs.start()
        assert _same(a.fields(), b.fields(), dim) == []
        for k in range(3):
            a.gs.step()
            H.pieces_step(b.gs)
            assert _same(a.fields(), b.fields(), dim) == [], k
        for c in range(dim):
            pa, pb = a.gs.diffusion_params(c), b.gs.diffusion_params(c)
            assert pa.niter == pb.niter >= 1 and pa.residual.infty == pb.residual.infty
        kc = a.gd.kernel_counts()
        assert kc["ADVECT_GENERAL"] > 0 and kc["PREDICT_GENERAL"] > 0
        if (dim, level) == (3, 5):
            assert kc["DIFFUSION_FACES_PIPELINED"] > 0 and kc["WEIGHTED_PIPELINED"] > 0
        end = a.fields()
        assert np.isfinite(end["U0"]).all() and not np.array_equal(H.interior(end["U0"]), H.interior(a.state["U0"]))
    finally:
        a.destroy()
        b.destroy()


def _zero_flow(r, dt):
    """no MAC velocities and no pressure gradients: the advection part of gfs_centered_velocity_advection_diffusion
    leaves rhs = u (every flux is 0 times a face value), so what the hook does is the implicit diffusion alone"""
    case = r.case
    zero = np.zeros((case.n + 2,) * case.dim)
    for c in range(case.dim):
        r.gs.mac_velocity(c).upload(zero)
        r.gs.g[c].upload(zero)
        r.gs.gmac[c].upload(zero)
    r.gs.advection_params.dt = dt


@pytest.mark.parametrize("dim,level", SHAPES)
def test_diffusion_of_the_step_against_the_solver_entry_points(dim, level):
    """(c), the wiring inside the step: gfship_centered_velocity_advection of a simulation with a viscosity field
    per component, alpha and alpha_cell, on a state without MAC velocities and gradients, against the same
    solve written in the test from the solver's entry points (pinned on the oracle by
    tests/test_gpu_diffusion_faces.py): rhs = u, gfship_diffusion_coefficients_faces with the component's D,
    dt and alpha_cell, gfship_diffusion_rhs, gfship_diffusion on copies.  U, niter and residual.infty."""
    case = Case(dim, level)
    D = [_faces(case, np.random.default_rng(20 + c)) for c in range(dim)]
    r = Run(case, D=D, alpha=True)
    try:
        gd, gs = r.gd, r.gs
        dt = 0.3 / case.n
        _zero_flow(r, dt)
        want, pars = [], []
        for c in range(dim):
            u0 = gs.u[c].download()
            v, rhs, rhoc = gd.variable(c), gd.variable(), gd.variable()
            v.upload(u0)
            rhs.upload(u0)
            par = gd.params()
            par.tolerance = 1e-6               # diffusion_init, src/source.c:966-974
            gd.diffusion_coefficients_faces(r.Dc[c], dt, rhoc, r.alpha_cell, par.beta)
            gd.diffusion_rhs(v, rhs, rhoc, par.beta)
            gd.diffusion(par, v, rhs, rhoc)
            want.append(v.download())
            pars.append(par)
            assert par.niter >= 1 and not np.array_equal(H.interior(want[c]), H.interior(u0))
        gs.centered_velocity_advection(gs.gmac, gs.g)
        for c in range(dim):
            assert np.array_equal(H.interior(gs.u[c].download()), H.interior(want[c])), c
            got = gs.diffusion_params(c)
            assert got.niter == pars[c].niter and got.residual.infty == pars[c].residual.infty, c
            assert got.residual_before.infty == pars[c].residual_before.infty, c
    finally:
        r.destroy()


@pytest.mark.parametrize("dim,level", SHAPES)
def test_alpha_and_the_coefficient_reach_the_predictor_and_the_cfl(dim, level):
    """(c), the MAC source inside the step: scaling by a power of two is exact, so the predictor and the
    acceleration term of the CFL condition of a simulation with the coefficients D_c and alpha_cell = 2 give the
    bits of a simulation with 2 D_c and alpha_cell = 1 -- and not those of D_c with alpha_cell = 1"""
    case = Case(dim, level)
    D = [_faces(case, np.random.default_rng(30 + c)) for c in range(dim)]
    D2 = [[2. * a for a in Dc] for Dc in D]
    runs = [Run(case, D=D, alpha_const=2.), Run(case, D=D2, alpha_const=1.), Run(case, D=D, alpha_const=1.)]
    try:
        un, cfl = [], []
        for r in runs:
            r.gs.advection_params.dt = 0.3 / case.n
            cfl.append(r.gs.cfl())
            r.gs.predicted_face_velocities()
            un.append([r.gs.un(c) for c in range(dim)])
            assert r.gd.kernel_counts()["PREDICT_GENERAL"] > 0
        for c in range(dim):
            sl = [slice(1, -1)] * dim
            sl[dim - 1 - c] = slice(0, -1)
            assert np.array_equal(un[0][c][tuple(sl)], un[1][c][tuple(sl)]), c
            assert not np.array_equal(un[0][c][tuple(sl)], un[2][c][tuple(sl)]), c
        assert cfl[0] == cfl[1]
    finally:
        for r in runs:
            r.destroy()


def test_refusals():
    """(d) set_alpha plus a viscosity without alpha_cell is still refused, in either order, and the message
    names the new call; particle forces plus a viscosity field are refused"""
    case = Case(2, 4)
    r = Run(case)
    try:
        gd, gs = r.gd, r.gs
        af = []
        for a in H.alpha_faces(case):
            f = gd.variable()
            f.upload(a)
            af.append(f)
        D = []
        for a in _faces(case, const=NU):
            f = gd.variable()
            f.upload(a)
            D.append(f)
        gs.set_alpha(af)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*gfship_sim_set_alpha_cell"):
            gs.set_viscosity(0, NU)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*gfship_sim_set_alpha_cell"):
            gs.set_viscosity_faces(0, D)
        gs.set_alpha(None)
        gs.set_viscosity_faces(0, D)
        with pytest.raises(gfship.GfshipError, match="gfship error -5.*gfship_sim_set_alpha_cell"):
            gs.set_alpha(af)
        ac = gd.variable()
        for l, a in enumerate(_alpha_cells(case)):
            ac.upload(a, l)
        gs.set_alpha_cell(ac)
        gs.set_alpha(af)
        gs.set_viscosity(1, NU)
        # particles with forces
        pl = gfship.ParticleList(gs, np.array([[0.1, 0.2, 0.]]), np.array([1]))
        try:
            pl.set_particulate(np.zeros((1, 3)), np.ones(1), np.ones(1))
            with pytest.raises(gfship.GfshipError, match="gfship error -5"):
                pl.set_forces([gfship.FORCE_DRAG])
            gs.set_viscosity_faces(0, None)
            pl.set_forces([gfship.FORCE_DRAG])
            gs.set_viscosity_faces(0, D)
            with pytest.raises(gfship.GfshipError, match="gfship error -5"):
                pl.event()
        finally:
            pl.destroy()
    finally:
        r.destroy()
