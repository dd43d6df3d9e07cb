"""The first residual of a projection's solve is restricted and copied into the layout of the leaves' relax loop by
the pass that computes it (residual_restrict_pack_kernel, csrc/relax_patch_loop.hip); the natural residual of the
leaves is not stored.  The pass runs where the simulation's res is a temporary (res_unread), on the 2 x 2 levels
of 3-D boxes with the pair arithmetic and a dia known to be zero; it bumps RESTRICTION_FUSED and not
RESIDUAL_PAIRS, which is how these tests see that it ran: per solve one residual pass less is tallied there.

64^3 is the smallest box on which the pair residual runs; GFSHIP_PATCH_MIN_N=32 makes its levels 6 and 5 both
2 x 2 levels (the coarse skewed store runs), GFSHIP_PATCH_MIN_N=64 level 6 alone.  The oracle steps the periodic
Taylor-Green box once (nitermin 1, 2, 1, 2 on both parameter sets, test_gpu_last_residual_unstored.py) for the
cases that compare with it.

The box with boundary sides is the closed box of test_gpu_timestep.py (symmetry conditions on six GfsBoundary
sides, a perturbed cellular flow) at 64^3: flow_cases.py has no 3-D box with boundary sides, and the pass is 3-D
only."""
import numpy as np
import pytest

import gfship
import multigrid_param_cases as M
from flow_cases import PERIODIC, oracle_taylor_green
from oracle import oracle as O
from test_gpu_timestep import _device_sim, _interior

pytestmark = pytest.mark.gpu
RTOL_SUM = M.RTOL_SUM
LEVEL = 6
NITERMIN = (1, 2, 1, 2)
SETS = ("projection_params", "approx_projection_params")
SWITCHES = ("GFSHIP_PATCH_MIN_N", "GFSHIP_PATCH_REGS", "GFSHIP_SKEW_LINES", "GFSHIP_NO_FUSED_RESTRICTION",
            "GFSHIP_RN_SCALAR", "GFSHIP_RN_BLOCKS")
BOX = [O.SIDE_BOUNDARY] * 6


@pytest.fixture(scope="module", autouse=True)
def _oracle_signatures():
    O._sim_sigs(O.lib())


def _un_faces(a, n, c):
    # faces with tangential coordinates in 1..n and normal coordinate in 0..n
    sl = [slice(1, n + 1)] * 3
    sl[2 - c] = slice(0, n + 1)
    return a[tuple(sl)]


def _snapshot(sim, device, full=True):
    """the state after a step: the fields bit for bit, and what the two solves reported"""
    n = 1 << LEVEL if full else 0
    get = (lambda f: _interior(f.download(), 3)) if device else (lambda f: f.interior().copy())
    s = {"dt": sim.dt, "t": sim.t, "P": get(sim.p)}
    for c in range(3):
        s["U%d" % c] = get(sim.u[c])
    if full:
        s["Pmac"] = get(sim.pmac)
        for c in range(3):
            s["g%d" % c] = get(sim.g[c])
            s["un%d" % c] = _un_faces(sim.un(c) if device else sim.un(2 * c), n, c).copy()
    for name in SETS:
        p = getattr(sim, name)
        s[name] = {"exact": (p.niter, p.residual.infty, p.residual_before.infty),
                   "sums": (p.residual.first, p.residual.second, p.residual_before.first,
                            p.residual_before.second)}
    return s


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        if k in SETS:
            assert a[k]["exact"] == b[k]["exact"], (what, k)
            assert b[k]["sums"] == pytest.approx(a[k]["sums"], rel=RTOL_SUM), (what, k)
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def _device_steps(osim, side, env, nitermin, full=True):
    """a device simulation started from the state of the (not yet started) oracle simulation, created under the
    switches of env and stepped once per entry of nitermin (None: as the parameters stand): the snapshots after
    the start and after every step, the tallies of the steps, and the residual passes they should have made"""
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        gd, gs = _device_sim(osim, side)     # the switches are read when the domain is created
    try:
        gs.start()
        snaps = [_snapshot(gs, True, full)]
        last = {name: getattr(gs, name).niter for name in SETS}
        counts0 = gd.kernel_counts()
        passes = restored = solves = cycles = 0
        for nmin in nitermin:
            if nmin is not None:
                for name in SETS:
                    getattr(gs, name).nitermin = nmin
            gs.step()
            snaps.append(_snapshot(gs, True, full))
            for name in SETS:
                niter = getattr(gs, name).niter
                solves += 1
                cycles += niter
                passes += 1 + niter                     # the initial residual and one per cycle
                if 0 < last[name] < niter:
                    restored += 1                       # the loop went on after a norm-only pass
                last[name] = niter
        counts = gd.kernel_counts()
        delta = {k: counts[k] - counts0[k] for k in ("RESIDUAL_PAIRS", "RESIDUAL_SCALAR", "RESTRICTION_FUSED",
                                                     "RESTRICTION_DECLINED")}
        return {"snaps": snaps, "delta": delta, "counts": counts, "passes": passes, "restored": restored,
                "solves": solves, "cycles": cycles}
    finally:
        gs.destroy()
        gd.destroy()


def _assert_fused_tallies(run):
    """one pass per solve went through the fused launch"""
    d = run["delta"]
    print("residual passes %d, stored again %d, solves %d, cycles %d: %r"
          % (run["passes"], run["restored"], run["solves"], run["cycles"], d))
    assert d["RESIDUAL_PAIRS"] == run["passes"] + run["restored"] - run["solves"]
    assert d["RESTRICTION_FUSED"] >= run["cycles"]
    assert run["counts"]["RESIDUAL_SCALAR"] == 0


@pytest.fixture(scope="module")
def oracle_tg():
    """the oracle's periodic Taylor-Green box after the start and after each of the four steps"""
    osim = oracle_taylor_green(LEVEL)
    osim.start()
    snaps = [_snapshot(osim, False)]
    for nmin in NITERMIN:
        for name in SETS:
            getattr(osim, name).nitermin = nmin
        osim.step()
        snaps.append(_snapshot(osim, False))
    return snaps


@pytest.fixture(scope="module")
def both_levels():
    return _device_steps(oracle_taylor_green(LEVEL), PERIODIC, {"GFSHIP_PATCH_MIN_N": "32"}, NITERMIN)


def test_both_levels_patched(oracle_tg, both_levels):
    for k, (o, g) in enumerate(zip(oracle_tg, both_levels["snaps"])):
        _assert_same(o, g, "state %d" % k)
    assert both_levels["solves"] == 8
    _assert_fused_tallies(both_levels)


def test_one_level_patched(oracle_tg):
    """level 5 runs on the one-line kernels: no skewed store of the coarse residual"""
    run = _device_steps(oracle_taylor_green(LEVEL), PERIODIC, {"GFSHIP_PATCH_MIN_N": "64"}, NITERMIN[:2])
    for k, (o, g) in enumerate(zip(oracle_tg[:3], run["snaps"])):
        _assert_same(o, g, "state %d" % k)
    _assert_fused_tallies(run)


def _closed_box():
    osim = O.Sim(3, LEVEL, BOX)
    x, y, z = osim.dom.centres()
    rng = np.random.default_rng(2)
    vel = [np.sin(np.pi * (x + .5)) * np.cos(np.pi * (y + .5)) * np.cos(np.pi * (z + .5)),
           -np.cos(np.pi * (x + .5)) * np.sin(np.pi * (y + .5)) * np.cos(np.pi * (z + .5)),
           0. * x * y * z]
    for c in range(3):
        osim.u[c].interior()[...] = vel[c] + 0.01 * rng.standard_normal(vel[c].shape)
    return osim


def test_boundary_sides():
    """the residual beside every side reads the ghosts the BC has written; the tiles along the sides have the
    partly filled skewed rows"""
    run = _device_steps(_closed_box(), BOX, {"GFSHIP_PATCH_MIN_N": "32"}, (None, None))
    osim = _closed_box()
    osim.start()
    _assert_same(_snapshot(osim, False), run["snaps"][0], "start")
    for k in range(2):
        osim.step()
        _assert_same(_snapshot(osim, False), run["snaps"][k + 1], "step %d" % k)
    _assert_fused_tallies(run)


def test_default_selection_128():
    """128^3 with the default switches takes the fused pass; each of its two off-switches gives the same bits"""
    level = 7
    runs = {}
    osim = oracle_taylor_green(level)      # the initial state alone: the oracle does not step at this size
    for name, env in (("default", {}), ("no_fused_restriction", {"GFSHIP_NO_FUSED_RESTRICTION": "1"}),
                      ("rn_scalar", {"GFSHIP_RN_SCALAR": "1"})):
        runs[name] = _device_steps(osim, PERIODIC, env, (None, None), full=False)
    for name in ("no_fused_restriction", "rn_scalar"):
        for k, (a, b) in enumerate(zip(runs["default"]["snaps"], runs[name]["snaps"])):
            for f in ("U0", "U1", "U2", "P"):
                assert np.array_equal(a[f], b[f]), (name, k, f)
            assert a["t"] == b["t"] and a["dt"] == b["dt"], (name, k)
    _assert_fused_tallies(runs["default"])
    assert runs["default"]["delta"]["RESTRICTION_DECLINED"] == 0
    d = runs["no_fused_restriction"]
    assert d["delta"]["RESTRICTION_DECLINED"] > 0 and d["delta"]["RESTRICTION_FUSED"] == 0
    assert d["delta"]["RESIDUAL_PAIRS"] == d["passes"] + d["restored"]
    d = runs["rn_scalar"]
    assert d["counts"]["RESIDUAL_PAIRS"] == 0 and d["delta"]["RESIDUAL_SCALAR"] >= d["passes"]


def test_workgroup_cap(both_levels):
    """64 workgroups walk the 256 tasks that as many workgroups take one each by default: every task is visited"""
    run = _device_steps(oracle_taylor_green(LEVEL), PERIODIC,
                        {"GFSHIP_PATCH_MIN_N": "32", "GFSHIP_RN_BLOCKS": "64"}, NITERMIN)
    assert run["counts"]["RN_BLOCKS_LIMIT"] == 64 and run["counts"]["RN_BLOCKS_MAX"] == 64
    assert both_levels["counts"]["RN_BLOCKS_MAX"] > 64
    for k, (a, b) in enumerate(zip(both_levels["snaps"], run["snaps"])):
        _assert_same(a, b, "state %d" % k)
    _assert_fused_tallies(run)


def test_public_solve_still_stores_the_residual():
    """gfship_poisson_solve on the patched box: res equals the oracle's, twice with one parameter set"""
    o = M.OracleDirichlet(3, LEVEL, "periodic")
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        mp.setenv("GFSHIP_PATCH_MIN_N", "32")
        gd = gfship.Domain(3, LEVEL, PERIODIC)
    try:
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
            assert par.residual_before.infty == o.par.residual_before.infty
            assert np.array_equal(o.P.interior(), P.download()[1:-1, 1:-1, 1:-1]), k
            assert np.array_equal(o.res.interior(), res.download()[1:-1, 1:-1, 1:-1]), k
        # the initial residual and the one after the cycle, both by the pair kernel, both stored
        assert gd.kernel_counts()["RESIDUAL_PAIRS"] == 4
    finally:
        gd.destroy()
