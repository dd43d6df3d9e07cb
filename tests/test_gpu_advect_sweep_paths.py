"""The three implementations of the fused advection of the velocity on a periodic box against each other,
device against device, bit for bit: advect3_sweep2_kernel (the default), the tiled kernels
(GFSHIP_NO_ADVECT_SWEEP) and the first sweep kernel (GFSHIP_ADVECT_SWEEP1).

Sizes: 64^3 is the smallest box the sweeps run on (one chunk along z, and the ring of every workgroup's
column wraps the periodic box); 128^3 has two chunks along z (kb = 64: the seam planes kb and kb + 65 only
feed their neighbours, and the ring waves carry their loads across both of them).

Template arguments <VL, SRC, CORR, MPI> of advect3_sweep2_kernel at its launch site
(launch_advect3_fused) that each case instantiates (VL: van_leer, SRC: source, CORR: fused):
  {centred, van_leer}-{plain, source}-fused     <VL, SRC, 1, 0>
  {centred, van_leer}-{plain, source}-unfused   <VL, SRC, 0, 0>   (GFSHIP_NO_FUSED_CORRECTION: gc given, the
                                                                   correction a kernel of its own)
  test_advection_without_g                      <VL, 0, 0, 0> with gc = nullptr
The MPI flavours (<., ., ., 1>) are the matter of the self-MPI and mock-RCCL tests."""
import numpy as np
import pytest

import gfship
from flow_cases import PERIODIC, oracle_taylor_green

pytestmark = pytest.mark.gpu

PATHS = [
    ("ADVECT3_SWEEP2", {}),
    ("ADVECT3_TILED", {"GFSHIP_NO_ADVECT_SWEEP": "1"}),
    ("ADVECT3_SWEEP1", {"GFSHIP_ADVECT_SWEEP1": "1"}),
]
ADVECT3 = ("ADVECT3_SWEEP2", "ADVECT3_TILED", "ADVECT3_SWEEP1")
SWITCHES = ("GFSHIP_NO_ADVECT_SWEEP", "GFSHIP_ADVECT_SWEEP1", "GFSHIP_NO_FUSED_CORRECTION")

# van Leer gradient x GfsSource on one component x the correction fused or not
CASES = {"%s-%s-%s" % (("centred", "van_leer")[vl], ("plain", "source")[src], ("fused", "unfused")[nf]):
         dict(gradient=vl, source=-0.7 if src else 0., env={"GFSHIP_NO_FUSED_CORRECTION": "1"} if nf else {})
         for vl in (0, 1) for src in (0, 1) for nf in (0, 1)}

_initial = {}


def _initial_velocity(level):
    """the Taylor-Green box with u += 0.35, w -= 0.2 (upwind directions of both signs, faces of zero
    velocity: test_sweep_kernels_64_several_steps_vs_oracle), leaf arrays with ghosts; computed once"""
    if level not in _initial:
        osim = oracle_taylor_green(level)
        osim.u[0].interior()[...] += 0.35
        osim.u[2].interior()[...] -= 0.2
        _initial[level] = [osim.u[c].leaf().copy() for c in range(3)]
    return _initial[level]


def _device_sim(level, gradient, source):
    gd = gfship.Domain(3, level, PERIODIC)
    gs = gfship.Simulation(gd)
    for c, a in enumerate(_initial_velocity(level)):
        gs.u[c].upload(a)
    gs.advection_params.gradient = gradient
    if source:
        gs.set_source(1, source)
    return gd, gs


def _state(gs, level):
    out = [gs.u[c].download() for c in range(3)] + [gs.p.download()]
    out += [gs.un(c) for c in range(3)]
    out += [gs.u[c].download(level - 1) for c in range(3)]      # filled by the sweep (the first coarse level)
    out.append(np.array([gs.t, gs.dt]))
    return out


NAMES = ["U", "V", "W", "P", "un0", "un1", "un2", "U below", "V below", "W below", "[t, dt]"]


def _inside(a):
    return a[1:-1, 1:-1, 1:-1] if a.ndim == 3 else a


def _set_path(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _assert_ran(kc, family, what):
    """the intended kernel of the three ran, and only it"""
    for k in ADVECT3:
        assert (kc[k] > 0) == (k == family), "%s: %s = %d" % (what, k, kc[k])


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("level", [6, 7])
def test_three_steps_same_on_every_path(level, case, monkeypatch):
    """three steps (the first advects with gmac in place of g): U, V, W, P, the three un, the level below the
    leaves of U, V, W and [t, dt] after every step, the tiled kernels and the first sweep kernel against the
    default path with np.array_equal; kernel_counts() says which kernel ran"""
    cfg = CASES[case]
    runs = []
    for family, env in PATHS:
        _set_path(monkeypatch, dict(cfg["env"], **env))
        gd, gs = _device_sim(level, cfg["gradient"], cfg["source"])
        gs.start()
        steps = []
        for _ in range(3):
            gs.step()
            steps.append(_state(gs, level))
        kc = gd.kernel_counts()
        gd.destroy()
        _assert_ran(kc, family, "%s %d" % (case, level))
        assert kc[family] >= 3
        runs.append(steps)
    for (family, _), steps in zip(PATHS[1:], runs[1:]):
        for k, (ref, got) in enumerate(zip(runs[0], steps)):
            for name, a, b in zip(NAMES, ref, got):
                assert np.array_equal(_inside(a), _inside(b)), "%s, step %d: %s" % (family, k, name)


@pytest.mark.parametrize("gradient", [0, 1])
@pytest.mark.parametrize("level", [6, 7])
def test_advection_without_g(level, gradient, monkeypatch):
    """the kernel without gc: gfship_centered_velocity_advection with g = NULL, which the binding reaches
    (Simulation.centered_velocity_advection (gmac, None)), after one step and the predictor and the MAC
    projection of the next; U, V, W of the three paths"""
    runs = []
    for family, env in PATHS:
        _set_path(monkeypatch, env)
        gd, gs = _device_sim(level, gradient, 0.)
        gs.start()
        gs.step()
        before = {k: v for k, v in gd.kernel_counts().items() if k in ADVECT3}
        gs.predicted_face_velocities()
        gs.mac_projection(gs.projection_params, gs.dt / 2., gs.pmac, gs.gmac)
        gs.centered_velocity_advection(gs.gmac, None)
        kc = gd.kernel_counts()
        runs.append([gs.u[c].download() for c in range(3)])
        gd.destroy()
        _assert_ran(kc, family, "without g %d" % level)
        assert kc[family] == before[family] + 1
    for (family, _), got in zip(PATHS[1:], runs[1:]):
        for name, a, b in zip(NAMES, runs[0], got):
            assert np.array_equal(_inside(a), _inside(b)), "%s: %s" % (family, name)
