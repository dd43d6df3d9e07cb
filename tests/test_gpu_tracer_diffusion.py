"""GfsSourceDiffusion on a GfsVariableTracer (gfs_tracer_advection_diffusion, src/timestep.c:1028-1055) on the
device against the oracle's arithmetic (tracer_diffusion_cases.py says where the expected bits come from; the
recipe itself is checked in test_tracer_diffusion_oracle_cpu.py).  Every comparison is of the interior bits of
T, niter, residual.infty and residual_before.infty."""
import numpy as np
import pytest

import gfship
import hook_cases as H
import tracer_diffusion_cases as TC
from tracer_diffusion_cases import TCase

pytestmark = pytest.mark.gpu

D, DT = TC.D_DEFAULT, TC.DT_DEFAULT
P32, P64 = TCase(3, 5), TCase(3, 6)


def _ids(c):
    return c.id


# 1 ---------------------------------------------------------------------------------------------
ZERO_FLOW = [TCase(2, 4), TCase(2, 4, "dirichlet"), TCase(2, 4, "neumann"), TCase(2, 4, "symmetry"),
             TCase(3, 3, "mixed"), P32]


@pytest.mark.parametrize("case", ZERO_FLOW, ids=_ids)
@pytest.mark.parametrize("beta", [1., 0.5])
def test_zero_flow_is_variable_diffusion(case, beta):
    got, counts = TC.device_calls(case, TC.fields(case)[0], None, D, DT, beta=beta)
    assert TC.mismatches(TC.expected_zero_flow(case, beta), got) == []
    assert got[0][1][0] > 0                         # the solve ran
    if case == P32:
        assert counts[0] == 1 and counts[1] == 0    # the fused pass
    else:
        assert counts == (0, 1)


# 2 ---------------------------------------------------------------------------------------------
FLOW = [(TCase(2, 4), 1, 1., 3), (TCase(2, 4, "dn"), 1, 0.5, 3), (TCase(2, 4, "dirichlet"), 0, 1., 3),
        (TCase(3, 3), 1, 0.5, 3), (P32, 0, 1., 3), (P32, 1, 0.5, 3), (P64, 1, 1., 1)]


@pytest.mark.parametrize("case,gradient,beta,ncalls", FLOW,
                         ids=["%s-grad%d-beta%g" % (c.id, g, b) for c, g, b, _ in FLOW])
def test_flow_is_the_velocity_slot_recipe(case, gradient, beta, ncalls):
    T0, un = TC.fields(case)
    got, counts = TC.device_calls(case, T0, un, D, DT, gradient=gradient, beta=beta, ncalls=ncalls)
    assert TC.mismatches(TC.expected_flow(case, gradient, beta, ncalls=ncalls), got) == []
    fused = case in (P32, P64)
    assert counts == ((ncalls, 0) if fused else (0, ncalls))
    # the flow matters: the zero-flow solve gives other bits
    zero, _ = TC.device_calls(case, T0, None, D, DT, gradient=gradient, beta=beta)
    assert not np.array_equal(zero[0][0], got[0][0])


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gradient,beta", [(0, 0.5), (1, 1.)])
def test_composed_path_equals_fused_path(gradient, beta):
    T0, un = TC.fields(P32)
    fused, cf = TC.device_calls(P32, T0, un, D, DT, gradient=gradient, beta=beta, ncalls=2, path=1)
    composed, cc = TC.device_calls(P32, T0, un, D, DT, gradient=gradient, beta=beta, ncalls=2, path=0)
    assert TC.mismatches(fused, composed) == []
    assert cf == (2, 0) and cc == (0, 2)


def test_limited_gradients_take_the_composed_path():
    # limiters 2 .. 4 do not run on the tiled kernel
    T0, un = TC.fields(P32)
    _, counts = TC.device_calls(P32, T0, un, D, DT, gradient=2)
    assert counts == (0, 1)


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [TCase(2, 4), P32], ids=_ids)
def test_scheme_none_is_the_zero_flow_solve(case):
    T0, un = TC.fields(case)
    got, counts = TC.device_calls(case, T0, un, D, DT, scheme=gfship.SCHEME_NONE)
    assert TC.mismatches(TC.expected_zero_flow(case, 1.), got) == []
    assert counts == (0, 1)


def test_scheme_none_without_diffusion_leaves_the_tracer():
    case = TCase(2, 4)
    T0, un = TC.fields(case)
    got, counts = TC.device_calls(case, T0, un, 0., DT, scheme=gfship.SCHEME_NONE)
    assert np.array_equal(got[0][0], H.interior(T0)) and counts == (0, 0)


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [TCase(2, 5), TCase(3, 4)], ids=_ids)
@pytest.mark.parametrize("beta", [1., 0.5])
def test_cosine_mode_decays_within_n_tolerances(case, beta):
    """I - beta dt D L has an inverse of infinity norm at most 1: N solves deviate from G^N T0 by at most
    N * tolerance"""
    Dm, dt, N, tolerance = 0.05, 0.01, 8, 1e-10
    T0, lam = TC.cosine_mode(case)
    got, _ = TC.device_calls(case, T0, None, Dm, dt, beta=beta, tolerance=tolerance, ncalls=N)
    dev = np.abs(got[-1][0] - TC.growth(lam, Dm, dt, beta) ** N * H.interior(T0)).max()
    print("%s beta %g: deviation %.3e" % (case.id, beta, dev))
    assert dev <= N * tolerance


# 6 ---------------------------------------------------------------------------------------------
def _three_tracer_sim(case, state):
    gd = gfship.Domain(case.dim, case.level, case.side)
    gs = gfship.Simulation(gd)
    for par in (gs.projection_params, gs.approx_projection_params):
        par.tolerance, par.nitermax = 1e-6, 4
    gs.hook_tracers = [gs.add_tracer(gradient=1), gs.add_tracer(gradient=0), gs.add_tracer(gradient=1)]
    for t, (Dt, beta) in zip(gs.hook_tracers, ((0.05, 1.), (0.02, 0.5))):
        gs.set_tracer_diffusion(t, Dt)
        gs.tracer_diffusion_params(t).beta = beta
    for c in range(case.dim):
        gs.u[c].upload(state["U%d" % c])
    for t, a in zip(gs.hook_tracers, (state["T0"], state["T1"], state["T0"] - 0.5 * state["T1"])):
        t.upload(a)
    return gd, gs


@pytest.mark.parametrize("case", [H.Case(2, 4), H.Case(3, 3)], ids=lambda c: c.id)
def test_sim_step_is_the_pieces_with_tracer_diffusion(case):
    state = H.random_state(case)
    ga, a = _three_tracer_sim(case, state)
    gb, b = _three_tracer_sim(case, state)
    try:
        a.start()
        b.start()
        for _ in range(3):
            a.step()
            H.pieces_step(b)
        assert (a.t, a.i, a.dt) == (b.t, b.i, b.dt) and a.i == 3
        fa, fb = H.sim_fields(a), H.sim_fields(b)
        for name in fa:
            assert np.array_equal(H.interior(fa[name].download()), H.interior(fb[name].download())), name
        for ta, tb in zip(a.hook_tracers[:2], b.hook_tracers[:2]):
            assert TC.stats(a.tracer_diffusion_params(ta)) == TC.stats(b.tracer_diffusion_params(tb))
            assert a.tracer_diffusion_params(ta).niter > 0
        # half step of start + three steps, two tracers with a coefficient; the third is only advected
        assert sum(a.tracer_diffusion_counts()) == 8 and sum(b.tracer_diffusion_counts()) == 8
        assert a.tracer_diffusion_params(a.hook_tracers[2]).niter == 0
    finally:
        H.destroy_device(ga, a)
        H.destroy_device(gb, b)


# 7 ---------------------------------------------------------------------------------------------
def test_removing_the_coefficient_restores_plain_advection():
    case = TCase(2, 4)
    T0, un = TC.fields(case)
    expected = TC.oracle_tracer_advection(case, T0, un, DT, 1, ncalls=2)
    gd = gfship.Domain(case.dim, case.level, case.side)
    gs = gfship.Simulation(gd)
    try:
        T = gs.add_tracer()
        T.upload(T0)
        gd.bc(T)
        for c in range(case.dim):
            gs.mac_velocity(c).upload(un[c])
        gs.set_tracer_diffusion(T, D)
        gs.set_tracer_diffusion(T, 0.)
        for k in range(2):
            gs.tracer_advection(T, DT)
            assert np.array_equal(H.interior(T.download()), expected[k])
        assert gs.tracer_diffusion_counts() == (0, 0)
    finally:
        H.destroy_device(gd, gs)


def test_setters_refuse_what_the_header_says():
    gd = gfship.Domain(2, 3, [gfship.SIDE_PERIODIC] * 6)
    gs = gfship.Simulation(gd)
    try:
        T = gs.add_tracer()
        par = gs.tracer_diffusion_params(T)
        assert (par.tolerance, par.beta) == (1e-6, 1.)           # diffusion_init, src/source.c:966-974
        einval = "gfship error -1:"
        with pytest.raises(gfship.GfshipError, match=einval):
            gs.set_tracer_diffusion(T, -1.)
        with pytest.raises(gfship.GfshipError, match=einval):
            gs.set_tracer_diffusion(1, 1.)
        with pytest.raises(gfship.GfshipError, match=einval):
            gs.set_tracer_diffusion(-1, 1.)
        with pytest.raises(gfship.GfshipError, match=einval):
            gs.set_tracer_scheme(T, 2)
        with pytest.raises(gfship.GfshipError, match=einval):
            gs.set_tracer_scheme(1, gfship.SCHEME_NONE)
        with pytest.raises(gfship.GfshipError, match=einval):
            gs.tracer_diffusion_path(2)
        with pytest.raises(gfship.GfshipError):
            gs.tracer_diffusion_params(1)
        # beta outside [0.5, 1]
        gs.set_tracer_diffusion(T, D)
        for beta in (0.4, 1.1):
            par.beta = beta
            with pytest.raises(gfship.GfshipError, match=einval):
                gs.tracer_advection(T, DT)
        # a second tracer leaves the parameters of the first where they are
        par.beta = 0.75
        gs.add_tracer()
        assert gs.tracer_diffusion_params(T).beta == 0.75
    finally:
        H.destroy_device(gd, gs)


def test_a_box_with_mpi_sides_is_unsupported():
    gd = gfship.Domain(3, 3, H.EXTERNAL_X)
    gs = gfship.Simulation(gd)
    try:
        T = gs.add_tracer()
        with pytest.raises(gfship.GfshipError, match="gfship error -5:"):
            gs.set_tracer_diffusion(T, 1.)
        gs.set_tracer_diffusion(T, 0.)
    finally:
        H.destroy_device(gd, gs)
