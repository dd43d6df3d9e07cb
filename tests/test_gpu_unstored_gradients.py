"""The centred pressure gradient g of the approximate projection that ends a step is not stored where its one
reader, the advection of the next step, can form it from P: project_correct_lazy2_kernel
without the stores of g, advect3_sweep2_kernel with the gradient from the pressure, materialize_g for everybody
else.  gfship_sim_gradients_unstored (Simulation.gradients_unstored) counts the projections that left g
unstored; a simulation whose g handles somebody has asked for (gfship.Simulation.g) stores g as before: that is
the "stored run" these tests compare with.

64^3 is the smallest box on which the sweep and the pair kernels run; 128^3 the smallest with two blocks of
planes along z and several tiles across.  The oracle steps the periodic Taylor-Green box at 64^3."""
import numpy as np
import pytest

import gfship
import multigrid_param_cases as M
from flow_cases import PERIODIC, oracle_taylor_green
from oracle import oracle as O
from test_gpu_fused_initial_residual import _closed_box, _un_faces, BOX
from test_gpu_timestep import _device_sim, _interior

pytestmark = pytest.mark.gpu
RTOL_SUM = M.RTOL_SUM
LEVEL = 6
N = 1 << LEVEL
SETS = ("projection_params", "approx_projection_params")
SWITCHES = ("GFSHIP_NO_LAZY_UN", "GFSHIP_NO_FUSED_CORRECTION", "GFSHIP_PC_SCALAR", "GFSHIP_ADVECT_SWEEP1",
            "GFSHIP_NO_ADVECT_SWEEP", "GFSHIP_NO_ADVECT3")
TALLIES = ("ADVECT3_SWEEP2", "PROJECT_PAIRS", "CORRECTION_FUSED")


@pytest.fixture(scope="module", autouse=True)
def _oracle_signatures():
    O._sim_sigs(O.lib())


def _snapshot(sim, device):
    """the state after a step, without a look at g or gmac"""
    get = (lambda f: _interior(f.download(), 3)) if device else (lambda f: f.interior().copy())
    s = {"dt": sim.dt, "t": sim.t, "P": get(sim.p), "Pmac": get(sim.pmac)}
    for c in range(3):
        s["U%d" % c] = get(sim.u[c])
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


def _fields_only(s):
    return {k: v for k, v in s.items() if k not in SETS}


def _make(osim, side=PERIODIC, env=None, handles=False, prepare=None):
    """a device simulation from the state of the oracle simulation, created under the switches of env;
    handles: the g and gmac handles are taken before the first step (the stored run)"""
    with pytest.MonkeyPatch.context() as mp:
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        gd, gs = _device_sim(osim, side)     # the switches are read when the domain is created
    if prepare:
        prepare(gs)
    if handles:
        assert len(gs.g) == 3 and len(gs.gmac) == 3
    return gd, gs


def _gradients(gs):
    """g and gmac, ghost layers included"""
    d = {"g%d" % c: gs.g[c].download() for c in range(3)}
    d.update({"gmac%d" % c: gs.gmac[c].download() for c in range(3)})
    return d


def _uns(gs, n):
    return [_un_faces(gs.un(c), n, c).copy() for c in range(3)]


def _step_tallies(gd, gs, nsteps, snaps, deltas):
    for _ in range(nsteps):
        c0, u0 = gd.kernel_counts(), gs.gradients_unstored()
        gs.step()
        c1 = gd.kernel_counts()
        deltas.append({k: c1[k] - c0[k] for k in TALLIES})
        deltas[-1]["GRADIENTS_UNSTORED"] = gs.gradients_unstored() - u0
        snaps.append(_snapshot(gs, True))


@pytest.fixture(scope="module")
def oracle_run():
    """the oracle's periodic Taylor-Green box after the start and after each of four steps; its g and gmac after
    the third"""
    osim = oracle_taylor_green(LEVEL)
    osim.start()
    snaps = [_snapshot(osim, False)]
    grads = None
    for k in range(4):
        osim.step()
        snaps.append(_snapshot(osim, False))
        if k == 2:
            grads = {"g%d" % c: osim.g[c].interior().copy() for c in range(3)}
            grads.update({"gmac%d" % c: osim.gmac[c].interior().copy() for c in range(3)})
    return {"snaps": snaps, "grads": grads}


@pytest.fixture(scope="module")
def stored_run():
    """the device run that holds the g handles from the start: five steps, g and gmac after the second and the
    third, the MAC velocities after the third"""
    gd, gs = _make(oracle_taylor_green(LEVEL), handles=True)
    try:
        gs.start()
        snaps, deltas, grads = [_snapshot(gs, True)], [], {}
        for k in range(5):
            _step_tallies(gd, gs, 1, snaps, deltas)
            if k in (1, 2):
                grads[k + 1] = _gradients(gs)
            if k == 2:
                un = _uns(gs, N)
        assert gs.gradients_unstored() == 0
        return {"snaps": snaps, "deltas": deltas, "grads": grads, "un": un}
    finally:
        gs.destroy()
        gd.destroy()


@pytest.fixture(scope="module")
def unstored_run():
    """four steps without a look at g or gmac; the whole state after the second for the restart"""
    gd, gs = _make(oracle_taylor_green(LEVEL))
    try:
        gs.start()
        snaps, deltas = [_snapshot(gs, True)], []
        _step_tallies(gd, gs, 2, snaps, deltas)
        state = {"t": gs.t, "i": gs.i, "P": gs.p.download(), "Pmac": gs.pmac.download(),
                 "U": [gs.u[c].download() for c in range(3)]}
        _step_tallies(gd, gs, 2, snaps, deltas)
        assert gs._g is None
        return {"snaps": snaps, "deltas": deltas, "state": state}
    finally:
        gs.destroy()
        gd.destroy()


def test_four_steps_against_the_oracle(oracle_run, stored_run, unstored_run):
    for k, (o, g) in enumerate(zip(oracle_run["snaps"], unstored_run["snaps"])):
        _assert_same(o, g, "state %d" % k)
    d = unstored_run["deltas"]
    print("tallies per step:", d)
    # the approximate projection of every step leaves g unstored (the first step advects with gmac for g and
    # stays as it is; gmac is stored throughout)
    assert [x["GRADIENTS_UNSTORED"] for x in d] == [1, 1, 1, 1]
    for k in ("ADVECT3_SWEEP2", "PROJECT_PAIRS", "CORRECTION_FUSED"):
        assert [x[k] for x in d] == [x[k] for x in stored_run["deltas"][:4]], k
        assert all(x[k] > 0 for x in d), k


def test_materialisation(oracle_run, stored_run):
    gd, gs = _make(oracle_taylor_green(LEVEL))
    try:
        gs.start()
        for _ in range(3):
            gs.step()
        assert gs.gradients_unstored() == 3
        # materialize_un beside materialize_g
        for c, (a, b) in enumerate(zip(stored_run["un"], _uns(gs, N))):
            assert np.array_equal(a, b), "un[%d]" % c
        got = _gradients(gs)
        for k, a in stored_run["grads"][3].items():
            assert np.array_equal(a, got[k]), k                       # ghost layers included
            assert np.array_equal(oracle_run["grads"][k], _interior(got[k], 3)), k
        _assert_same(stored_run["snaps"][3], _snapshot(gs, True), "after the look")
        for k in (4, 5):
            gs.step()
            _assert_same(stored_run["snaps"][k], _snapshot(gs, True), "state %d" % k)
        assert gs.gradients_unstored() == 3          # stored from the look on
    finally:
        gs.destroy()
        gd.destroy()


@pytest.mark.parametrize("write", ["P", "Pmac"])
def test_writes_in_between(stored_run, write):
    """g is stored before anybody overwrites the pressure it is the gradient of"""
    gd, gs = _make(oracle_taylor_green(LEVEL))
    try:
        gs.start()
        for _ in range(2):
            gs.step()
        assert gs.gradients_unstored() == 2
        if write == "P":
            a = gs.p.download()
            gs.p.upload(np.cos(17. * a) + 3.)
        else:
            gs.pmac.fill(0.5)
        got = _gradients(gs)
        for k, a in stored_run["grads"][2].items():
            assert np.array_equal(a, got[k]), k
    finally:
        gs.destroy()
        gd.destroy()


def test_128_unstored_against_stored():
    """two blocks of planes along z, 4 x 8 tiles across: the device against itself"""
    level, n = 7, 128
    osim = oracle_taylor_green(level)      # the initial state alone: the oracle does not step at this size
    runs = {}
    for name in ("unstored", "stored"):
        gd, gs = _make(osim, handles=name == "stored")
        try:
            gs.start()
            snaps = []
            for _ in range(3):
                gs.step()
                snaps.append(_fields_only(_snapshot(gs, True)))
                snaps[-1].update({"un%d" % c: a for c, a in enumerate(_uns(gs, n))})
            runs[name] = {"snaps": snaps, "tally": gs.gradients_unstored(),
                          "grads": _gradients(gs)}
        finally:
            gs.destroy()
            gd.destroy()
    assert runs["unstored"]["tally"] == 3 and runs["stored"]["tally"] == 0
    for k, (a, b) in enumerate(zip(runs["stored"]["snaps"], runs["unstored"]["snaps"])):
        _assert_same(a, b, "step %d" % k)
    for k, a in runs["stored"]["grads"].items():
        assert np.array_equal(a, runs["unstored"]["grads"][k]), k


@pytest.mark.parametrize("switch", SWITCHES)
def test_declined_by_a_switch(oracle_run, switch):
    gd, gs = _make(oracle_taylor_green(LEVEL), env={switch: "1"})
    try:
        gs.start()
        _assert_same(oracle_run["snaps"][0], _snapshot(gs, True), "start")
        for k in range(1, 4):
            gs.step()
            _assert_same(oracle_run["snaps"][k], _snapshot(gs, True), "state %d" % k)
        assert gs.gradients_unstored() == 0
        assert gs._g is None
    finally:
        gs.destroy()
        gd.destroy()


def _tracer(gs):
    x, y, z = np.meshgrid(*((np.arange(N + 2) - 0.5) / N - 0.5,) * 3, indexing="ij")
    gs.add_tracer().upload(np.exp(-40. * (x ** 2 + y ** 2 + z ** 2)))


def _viscosity(gs):
    for c in range(3):
        gs.set_viscosity(c, 1e-2)


@pytest.mark.parametrize("case", ["closed_box", "tracer", "viscosity"])
def test_declined_by_the_case(case):
    """a box with boundary sides, a tracer (it reads the MAC velocities), a viscosity: g is stored, and the run
    equals the one that held the handles from the start"""
    make = _closed_box if case == "closed_box" else lambda: oracle_taylor_green(LEVEL)
    side = BOX if case == "closed_box" else PERIODIC
    prepare = {"closed_box": None, "tracer": _tracer, "viscosity": _viscosity}[case]
    snaps = {}
    for handles in (False, True):
        gd, gs = _make(make(), side=side, handles=handles, prepare=prepare)
        try:
            gs.start()
            snaps[handles] = [_snapshot(gs, True)]
            for _ in range(2):
                gs.step()
                snaps[handles].append(_snapshot(gs, True))
            assert gs.gradients_unstored() == 0
            assert handles or gs._g is None
        finally:
            gs.destroy()
            gd.destroy()
    for k, (a, b) in enumerate(zip(snaps[True], snaps[False])):
        _assert_same(a, b, "state %d" % k)


def test_restart(oracle_run, unstored_run):
    """the state after the second step into a fresh simulation, gfship_sim_restart, start (which rebuilds g from
    P), two more steps: steps three and four of the uninterrupted run"""
    st = unstored_run["state"]
    assert st["i"] == 2
    gd, gs = _make(oracle_taylor_green(LEVEL))
    try:
        gs.p.upload(st["P"])
        gs.pmac.upload(st["Pmac"])
        for c in range(3):
            gs.u[c].upload(st["U"][c])
        gs.restart(st["t"], st["i"])
        gs.start()
        for k in (3, 4):
            gs.step()
            _assert_same(_fields_only(oracle_run["snaps"][k]), _fields_only(_snapshot(gs, True)), "state %d" % k)
            _assert_same(_fields_only(unstored_run["snaps"][k]), _fields_only(_snapshot(gs, True)), "state %d" % k)
        assert gs.gradients_unstored() == 2
        assert gs._g is None
    finally:
        gs.destroy()
        gd.destroy()
