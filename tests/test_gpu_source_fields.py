"""GfsSourceParticulate in the time step (gfship_sim_set_source_fields): the velocity source read from
fields, as MAC source (modules/particulatecommon.c:2029-2065 through src/source.c:38-59) and as centred
source (:2067-2079 through src/source.c:66-79)."""
import json
import os

import numpy as np
import pytest

import gfship
from conftest import GOLDEN
from flow_cases import PERIODIC
from two_way_cases import PLAIN_RUNS, plain_run_kernel_counts, smooth_velocity

pytestmark = pytest.mark.gpu

CHANNEL = [gfship.SIDE_PERIODIC, gfship.SIDE_PERIODIC, gfship.SIDE_BOUNDARY, gfship.SIDE_BOUNDARY,
           gfship.SIDE_PERIODIC, gfship.SIDE_PERIODIC]
BOXES = [(2, 4, CHANNEL), (3, 3, PERIODIC), (3, 4, CHANNEL)]


def _interior(a, dim):
    return a[(slice(1, -1),) * dim]


def _source_fields(dim, depth):
    """smooth, non-uniform, ghost cells included (the MAC value reads them beyond a side)"""
    u = smooth_velocity(dim, depth)
    return [0.7 * u[(c + 1) % dim] + 0.1 * (c + 1) for c in range(dim)]


def _positive_face_value(F, c, dim):
    """source_particulate_value: ((x1 - 0.5)*v0 + 0.5*v1)/x1 with x1 = 1. towards the positive side of
    component c, on the interior cells (arrays are indexed [k][j][i])"""
    axis = dim - 1 - c
    v0 = _interior(F, dim)
    sl = [slice(1, -1)] * dim
    sl[axis] = slice(2, None)
    v1 = F[tuple(sl)]
    x1 = 1.
    return 0. + ((x1 - 0.5) * v0 + 0.5 * v1) / x1


@pytest.mark.parametrize("dim,depth,sides", BOXES)
def test_mac_source_is_the_positive_face_value_then_the_diffusion(dim, depth, sides):
    gd = gfship.Domain(dim, depth, sides)
    gs = gfship.Simulation(gd)
    try:
        for c, a in enumerate(smooth_velocity(dim, depth)):
            gs.u[c].upload(a)
        Fa = _source_fields(dim, depth)
        F = [gd.variable() for _ in range(dim)]
        for f, a in zip(F, Fa):
            f.upload(a)
        out = gd.variable()
        # without diffusion: the face value alone
        gs.set_source_fields(F)
        for c in range(dim):
            gs.variable_mac_source(c, out)
            assert np.array_equal(_interior(out.download(), dim), _positive_face_value(Fa[c], c, dim)), c
        # with a GfsSourceDiffusion: its own MAC source (the entry as it was), added second
        gs.set_source_fields(None)
        for c in range(dim):
            gs.set_viscosity(c, 1e-2)
        D = []
        for c in range(dim):
            gs.variable_mac_source(c, out)
            D.append(_interior(out.download(), dim).copy())
            assert np.abs(D[c]).max() > 1e-3
        gs.set_source_fields(F)
        for c in range(dim):
            gs.variable_mac_source(c, out)
            assert np.array_equal(_interior(out.download(), dim), _positive_face_value(Fa[c], c, dim) + D[c]), c
        with pytest.raises(gfship.GfshipError, match="source field"):
            gs.variable_mac_source(0, F[0])
    finally:
        gs.destroy()
        gd.destroy()


@pytest.mark.parametrize("dim,depth,sides", BOXES)
def test_centred_source_of_a_fluid_at_rest(dim, depth, sides):
    """u = 0, un = 0, no viscosity, gmac = 0: gfs_centered_velocity_advection leaves u_c = dt*F_c"""
    gd = gfship.Domain(dim, depth, sides)
    gs = gfship.Simulation(gd)
    try:
        Fa = _source_fields(dim, depth)
        F = [gd.variable() for _ in range(dim)]
        for f, a in zip(F, Fa):
            f.upload(a)
        gs.set_source_fields(F)
        gs.advection_params.dt = dt = 0.0123
        gs.centered_velocity_advection(gs.gmac)
        for c in range(dim):
            assert np.array_equal(_interior(gs.u[c].download(), dim), dt * _interior(Fa[c], dim)), c
    finally:
        gs.destroy()
        gd.destroy()


def _three_steps(dim, depth, sides, g, fields, nu=0.):
    gd = gfship.Domain(dim, depth, sides)
    gs = gfship.Simulation(gd)
    try:
        for c, a in enumerate(smooth_velocity(dim, depth)):
            gs.u[c].upload(0.3 * a)
            if nu:
                gs.set_viscosity(c, nu)
        if fields:
            F = [gd.variable() for _ in range(dim)]
            for c in range(dim):
                F[c].upload(np.full(((1 << depth) + 2,) * dim, g[c]))
            gs.set_source_fields(F)
        else:
            for c in range(dim):
                gs.set_source(c, g[c])
        gs.start()
        dts = []
        for _ in range(3):
            gs.step()
            dts.append(gs.dt)
        state = [gs.u[c].download() for c in range(dim)] + [gs.p.download()]
        return state, dts, gs.t, gd.kernel_counts()
    finally:
        gs.destroy()
        gd.destroy()


@pytest.mark.parametrize("nu", [0., 1e-2])
@pytest.mark.parametrize("dim,depth,sides", BOXES)
def test_uniform_source_fields_are_a_gfs_source(dim, depth, sides, nu):
    """F_c = g everywhere: three full steps are those of GfsSource {} U/V/W g (the path pinned on
    test/poiseuille), time steps included; large enough for the acceleration to set the time step.  With a
    constant viscosity the MAC source of the diffusion comes from the array of the per-face kernel instead of
    the expression inside the kernels: the same bits, in the predictor, the advection and the CFL"""
    g = [40., -25., 10.][:dim]
    want, wdt, wt, _ = _three_steps(dim, depth, sides, g, False, nu)
    got, gdt, gt, kc = _three_steps(dim, depth, sides, g, True, nu)
    assert wdt == gdt and wt == gt
    for a, b in zip(want, got):
        assert np.array_equal(_interior(a, dim), _interior(b, dim))
    # the fused periodic kernels are not taken with source fields
    assert kc["ADVECT_GENERAL"] > 0 and kc["PREDICT_GENERAL"] > 0


@pytest.mark.parametrize("name", [r[0] for r in PLAIN_RUNS])
def test_runs_without_source_fields_launch_what_they_launched(name):
    """tests/golden/two_way_kernel_counts.json: gfship_domain_kernel_counts of the same runs recorded with the
    library as it was before source fields existed"""
    recorded = json.load(open(os.path.join(GOLDEN, "two_way_kernel_counts.json")))
    assert plain_run_kernel_counts(gfship, name) == recorded[name]
