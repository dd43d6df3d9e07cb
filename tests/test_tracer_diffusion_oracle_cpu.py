"""The yardstick of tests/test_gpu_tracer_diffusion.py, checked on the oracle alone (no device):

  * the velocity-slot recipe of tracer_diffusion_cases.oracle_flow with D = 0 is go_tracer_advection, bit for
    bit -- so with D != 0 it is variable_sources with the MAC source, then variable_diffusion, on a tracer;
  * N implicit steps of a cosine mode stay within N * tolerance of G^N T0: the operator I - beta dt D L has an
    inverse of infinity norm at most 1, so each solve adds at most its tolerance."""
import numpy as np
import pytest

import tracer_diffusion_cases as TC

RECIPE = [TC.TCase(2, 4, "periodic"), TC.TCase(2, 4, "dirichlet"), TC.TCase(2, 4, "dn"), TC.TCase(3, 3, "periodic")]


@pytest.mark.parametrize("case", RECIPE, ids=lambda c: c.id)
@pytest.mark.parametrize("gradient", [0, 1])
def test_velocity_slot_recipe_without_diffusion_is_the_tracer_advection(case, gradient):
    T0, un = TC.fields(case)
    slot = TC.oracle_flow(case, T0, un, 0., TC.DT_DEFAULT, gradient, ncalls=3)
    tracer = TC.oracle_tracer_advection(case, T0, un, TC.DT_DEFAULT, gradient, ncalls=3)
    for k, ((a, _), b) in enumerate(zip(slot, tracer)):
        assert np.array_equal(a, b), "call %d" % k
    assert not np.array_equal(slot[-1][0], TC.H.interior(T0))      # something was advected


@pytest.mark.parametrize("case", [TC.TCase(2, 5), TC.TCase(3, 4)], ids=lambda c: c.id)
@pytest.mark.parametrize("beta", [1., 0.5])
@pytest.mark.parametrize("tolerance", [1e-6, 1e-10])
def test_cosine_mode_decays_within_n_tolerances_on_the_oracle(case, beta, tolerance):
    D, dt, N = 0.05, 0.01, 8
    T0, lam = TC.cosine_mode(case)
    got = TC.oracle_zero_flow(case, T0, D, dt, beta, tolerance, ncalls=N)[-1][0]
    dev = np.abs(got - TC.growth(lam, D, dt, beta) ** N * TC.H.interior(T0)).max()
    print("%s beta %g tolerance %g: deviation %.3e" % (case.id, beta, tolerance, dev))
    assert dev <= N * tolerance
