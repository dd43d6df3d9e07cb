"""The residual pass after the last cycle of a projection's solve computes the norm alone (the simulation's
res is a temporary nobody reads): a 64^3 periodic Taylor-Green box, the smallest on which the pair kernel
(residual_norm2_kernel) runs, against the oracle for four steps.

nitermin of both parameter sets is 1, 2, 1, 2 from step to step, so the prediction -- the cycle count the
parameter set ended its previous solve with -- is wrong in both directions, and the pass that stores the
residual again before the loop goes on runs by construction; the tally of RESIDUAL_PAIRS says how often.
U, V, W, P, Pmac, g and the rebuilt un are compared with np.array_equal after every step, niter and the
maximum norms with ==, the summed norms with the suite's 1e-12.

The public gfship_poisson_solve keeps storing res: called twice with one parameter set on the same domain
after those steps (the second call would be `predicted' if the entry of the simulation leaked), its res
equals the oracle's."""
import numpy as np
import pytest

import gfship
import multigrid_param_cases as M
from flow_cases import PERIODIC, oracle_taylor_green
from oracle import oracle as O
from test_gpu_timestep import _assert_same_state, _assert_same_un, _device_sim

pytestmark = pytest.mark.gpu
RTOL_SUM = M.RTOL_SUM
LEVEL = 6
NITERMIN = (1, 2, 1, 2)
SETS = ("projection_params", "approx_projection_params")


@pytest.fixture(scope="module", autouse=True)
def _oracle_signatures():
    O._sim_sigs(O.lib())


def _same_params(osim, gs, what):
    for name in SETS:
        a, b = getattr(osim, name), getattr(gs, name)
        assert a.niter == b.niter, (what, name)
        assert a.residual.infty == b.residual.infty, (what, name)
        assert a.residual_before.infty == b.residual_before.infty, (what, name)
        for k in ("first", "second"):
            assert getattr(b.residual, k) == pytest.approx(getattr(a.residual, k), rel=RTOL_SUM), (what, name)
            assert getattr(b.residual_before, k) == \
                pytest.approx(getattr(a.residual_before, k), rel=RTOL_SUM), (what, name)


@pytest.fixture(scope="module")
def stepped():
    """the two simulations after the four steps, and what the steps showed"""
    osim = oracle_taylor_green(LEVEL)
    gd, gs = _device_sim(osim, PERIODIC)
    osim.start()
    gs.start()
    _assert_same_state(osim, gs, "start")
    last = {name: getattr(gs, name).niter for name in SETS}
    counts0 = gd.kernel_counts()
    passes = restored = unstored = 0
    for k, nmin in enumerate(NITERMIN):
        for sim in (osim, gs):
            for name in SETS:
                getattr(sim, name).nitermin = nmin
        osim.step()
        gs.step()
        _assert_same_state(osim, gs, "step %d" % k)
        _assert_same_un(osim, gs, "step %d" % k)
        _same_params(osim, gs, "step %d" % k)
        for name in SETS:
            niter = getattr(gs, name).niter
            assert niter >= nmin
            passes += 1 + niter                     # the initial residual and one per cycle
            if 0 < last[name] <= niter:
                unstored += 1                       # the pass after cycle number last[name]
            if 0 < last[name] < niter:
                restored += 1                       # the loop went on after it
            last[name] = niter
    counts = gd.kernel_counts()
    yield osim, gd, gs, counts["RESIDUAL_PAIRS"] - counts0["RESIDUAL_PAIRS"], passes, restored, unstored
    gs.destroy()
    gd.destroy()


def test_steps_equal_the_oracle_and_the_prediction_misses_both_ways(stepped):
    osim, gd, gs, pairs, passes, restored, unstored = stepped
    print("residual passes %d, of them norm only %d, stored again %d" % (passes, unstored, restored))
    # the loop went on after a norm-only pass at least once per parameter set, and ended on one
    assert restored >= 2 and unstored > restored
    assert pairs == passes + restored
    assert gd.kernel_counts()["RESIDUAL_SCALAR"] == 0


def test_public_solve_still_stores_the_residual(stepped):
    osim, gd, gs, *_ = stepped
    o = M.OracleDirichlet(3, LEVEL, "periodic")
    P, div, res, dia = (gd.variable() for _ in range(4))
    a = np.zeros(((1 << LEVEL) + 2,) * 3)
    a[1:-1, 1:-1, 1:-1] = o.rhs
    div.upload(a)
    gd.bc(P)
    gd.poisson_coefficients()
    par = gd.params()
    for p in (par, o.par):
        p.tolerance, p.nitermin, p.nitermax = 1e-30, 1, 1
    for k in range(2):
        o.solve()
        gd.poisson_solve(par, P, div, res, dia, 1.)
        assert par.niter == o.par.niter == 1
        assert par.residual.infty == o.par.residual.infty
        assert np.array_equal(o.P.interior(), P.download()[1:-1, 1:-1, 1:-1]), k
        assert np.array_equal(o.res.interior(), res.download()[1:-1, 1:-1, 1:-1]), k
