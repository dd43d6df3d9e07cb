"""The recipe of a time step written from the public pieces, on the oracle alone (no device):
N steps of go_sim_step against the same steps through go_predicted_face_velocities,
go_mac_projection (on Pmac's field), go_centered_velocity_advection,
go_correct_centered_velocities, go_coarse_init, go_approximate_projection, "t = tnext, i++",
go_set_timestep and go_tracer_advection in the order of oracle/go_timestep.c (go_sim_step) -- every
variable on every level, the face velocities, t, i and dt identical after every step.

This pins the call sequence tests/test_gpu_hooks.py replays through the C ABI of the device library
(hook_cases.pieces_step drives both): a mismatch there is then the device's, not the sequence's.
go_sim_step itself is pinned on the reference's own files (tests/test_oracle_golden_timestep.py).
"""
import numpy as np
import pytest

import hook_cases as H
from flow_cases import oracle_lid, oracle_reynolds, oracle_taylor_green

NSTEPS = 4


def _reynolds(level, tracer):
    s = oracle_reynolds(level)
    s.hook_tracers = []
    if tracer:
        T = s.add_tracer()
        x, y = s.dom.centres()
        T.interior()[...] = np.exp(-30. * ((x - 0.1) ** 2 + (y + 0.05) ** 2)) + 0. * x * y
        s.hook_tracers = [T]
    return s


def _taylor_green(level, nu):
    s = oracle_taylor_green(level)
    s.hook_tracers = []
    for c in range(3):
        if nu:
            s.set_viscosity(c, nu)
    return s


def _lid(level):
    s = oracle_lid(level)
    s.hook_tracers = []
    return s


def _event(level):
    s = _reynolds(level, False)
    # two events, each inside a time step: the n == 1 branch of gfs_simulation_set_timestep, tnext != t + dt
    times = (0.013, 0.05)

    def next_event(t, i):
        tn = H.G_MAXINT
        for te in times:
            if t < te and te < tn:
                tn = te + 1e-9
        return tn
    s.set_next_event(next_event)
    return s


SETUPS = {
    "reynolds-2d-l5": lambda: _reynolds(5, False),
    "reynolds-2d-l5-tracer": lambda: _reynolds(5, True),
    "reynolds-2d-l5-events": lambda: _event(5),
    "taylor-green-3d-l3": lambda: _taylor_green(3, 0.),
    "taylor-green-3d-l4-viscous": lambda: _taylor_green(4, 1e-2),
    "lid-2d-l5": lambda: _lid(5),
}


@pytest.mark.parametrize("name", sorted(SETUPS))
def test_step_from_the_pieces_equals_go_sim_step(name):
    a, b = SETUPS[name](), SETUPS[name]()
    a.start()
    b.start()
    assert H.snapshot_differences(H.snapshot(a), H.snapshot(b)) == []
    dts = []
    for k in range(NSTEPS):
        a.step()
        H.pieces_step(b)
        assert H.snapshot_differences(H.snapshot(a), H.snapshot(b)) == [], "step %d" % k
        dts.append(a.dt)
    assert a.i == NSTEPS and a.t > 0. and np.abs(a.u[0].interior()).max() > 0.
    if name.endswith("events"):
        # the events did cut steps short: the steps are not all the CFL one
        assert len(set(dts)) > 1 and a.t > 0.05


def test_random_states_of_the_cases_are_consistent():
    """hook_cases.random_state / load_state (what the device tests upload): the oracle's two copies of
    every face velocity agree, walls carry no flow, and a step from such a state runs the same through
    go_sim_step and through the pieces"""
    from oracle import oracle as O
    for case in (H.Case(2, 4, "periodic", tracers=True), H.Case(2, 4, "lid", visc=1e-2),
                 H.Case(3, 3, "symmetry", source=0.7, gradient=1)):
        sims = [H.oracle_sim(case), H.oracle_sim(case)]
        st = H.random_state(case)
        for s in sims:
            H.load_state(case, s, None, st, dt=0.3 / case.n)
        s = sims[0]
        n = case.n
        for c in range(case.dim):
            ax = case.dim - 1 - c
            plus, minus = np.moveaxis(s.un(2 * c), ax, 0), np.moveaxis(s.un(2 * c + 1), ax, 0)
            assert np.array_equal(plus[:-1], minus[1:])
            if case.side[2 * c] == O.SIDE_BOUNDARY:
                assert not plus[0].any() and not plus[n].any()
            else:
                assert np.array_equal(plus[0], plus[n])
        sims[0].step()
        H.pieces_step(sims[1])
        assert H.snapshot_differences(H.snapshot(sims[0]), H.snapshot(sims[1])) == [], case.id


def test_hook_cases_cover_every_axis_and_hook():
    """the case list of tests/test_gpu_hooks.py: every value of every axis of the configurations (dimension
    and level, sides, gradient, viscosity, source, alpha, tracers, events), every hook"""
    from test_gpu_hooks import HOOK_CASES, HOOKS, STEP_CASES
    cases = [c for c, _ in HOOK_CASES]
    assert {(c.dim, c.level) for c in cases} >= {(2, 3), (2, 5), (3, 3), (3, 4), (3, 5), (3, 6)}
    assert {c.sides for c in cases} == {"periodic", "lid", "symmetry", "external"}
    assert {c.gradient for c in cases} == {0, 1, 2}
    for axis in ("visc", "source", "alpha", "tracers", "event"):
        assert {bool(getattr(c, axis)) for c in cases} == {False, True}, axis
    assert {h for _, hooks in HOOK_CASES for h in hooks} == set(HOOKS)
    assert 6 <= len(STEP_CASES) <= 8
