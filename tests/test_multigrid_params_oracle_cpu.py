"""The oracle's handling of nrelax, erelax, minlevel and omega (oracle/go_poisson.c: go_poisson_cycle,
go_poisson_solve), which no golden file of the reference pins on a solid-free input:

  * go_poisson_cycle against a V-cycle composed in Python from the oracle's primitives (residual, relax
    sweep, conditions) with the restriction and prolongation restated in numpy -- bit for bit;
  * go_poisson_solve against a hand loop over go_poisson_cycle with the stall rule of gfs_poisson_solve,
    on problems where the rule does fire: the device tests of tests/test_gpu_multigrid_params.py run the
    same problems and would test nothing if minlevel stayed where it was.
"""
import numpy as np
import pytest

import multigrid_param_cases as M


@pytest.mark.parametrize("dim,level,kind,nrelax,erelax,minlevel,omega,use_dia", M.COMPOSED_SETS)
def test_cycle_composed_from_primitives_equals_go_poisson_cycle(dim, level, kind, nrelax, erelax, minlevel,
                                                                omega, use_dia):
    a = M.OracleCycle(dim, level, kind, use_dia)
    b = M.OracleCycle(dim, level, kind, use_dia)
    M.set_params(b.par, nrelax, erelax, minlevel, omega)
    u0 = a.u.leaf().copy()
    for cyc in range(2):
        ua, ra = a.cycle(nrelax, erelax, minlevel, omega)
        M.composed_cycle(b)
        assert np.array_equal(ua, b.u.leaf()), cyc
        assert np.array_equal(ra, b.res.interior()), cyc
    assert not np.array_equal(ua, u0)


def test_the_sets_change_the_iterates():
    """every parameter bites: each of nrelax, erelax and minlevel changes the result of a cycle; omega changes
    it in 2-D and does not in 3-D (the reference's 3-D relax has no omega, src/poisson.c:527)"""
    def run(dim, level, *s):
        return M.OracleCycle(dim, level, "walls", False).cycle(*s)[0]
    for dim, level in ((2, 4), (3, 3)):
        base = run(dim, level, 4, 1, 0, 1.)
        for other in ((3, 1, 0, 1.), (4, 2, 0, 1.), (4, 1, 2, 1.)):
            assert not np.array_equal(base, run(dim, level, *other)), (dim, other)
    assert not np.array_equal(run(2, 4, 4, 1, 0, 1.), run(2, 4, 4, 1, 0, 0.9))
    assert np.array_equal(run(3, 3, 4, 1, 0, 1.), run(3, 3, 4, 1, 0, 0.9))


@pytest.mark.parametrize("dim,level,minlevel", M.STALL_CASES)
def test_stall_rule_raises_minlevel_and_solve_equals_hand_loop(dim, level, minlevel):
    a = M.OracleDirichlet(dim, level)
    b = M.OracleDirichlet(dim, level)
    M.stall_params(a.par, minlevel)
    M.stall_params(b.par, minlevel)
    a.solve()
    used = b.hand_solve()
    # the rule fired: the cycles did not all run from the same level
    assert used[0] == minlevel and len(set(used)) > 1, used
    assert all(y - x in (0, 1) for x, y in zip(used, used[1:])), used
    assert a.par.minlevel == minlevel and b.par.minlevel == minlevel
    assert a.par.niter == b.par.niter == len(used)
    assert a.par.residual.infty == b.par.residual.infty
    assert a.par.residual_before.infty == b.par.residual_before.infty
    assert np.array_equal(a.P.leaf(), b.P.leaf())
    assert np.array_equal(a.res.interior(), b.res.interior())
    # the shared result the device tests compare with is this solve
    P, res, niter, infty, before, _, _, ml = M.oracle_solve(dim, level, "dirichlet", M.STALL_NRELAX, 1, minlevel,
                                                            M.STALL_TOLERANCE, M.STALL_NITERMAX)
    assert np.array_equal(P, a.P.interior()) and niter == a.par.niter and infty == a.par.residual.infty
    assert ml == minlevel


@pytest.mark.parametrize("dim,level,kind", [(3, 5, "periodic"), (3, 5, "dirichlet"), (2, 5, "dirichlet")])
def test_solve_with_erelax_and_minlevel_converges(dim, level, kind):
    P, res, niter, infty, before, _, _, ml = M.oracle_solve(dim, level, kind, 4, 2, 1, 1e-9, 100)
    assert 1 <= niter < 100 and infty <= 1e-9 < before
    assert ml == 1
