"""On a 3-D box whose six sides are periodic the kernels that compute the cells along the sides store their
periodic images -- the face ghosts -- themselves, and the launches of the stand-alone BC kernel that followed
them are gone: the pair kernels of the two projections (g, gmac and the corrected U, V, W), the copy out of the
relax loop's layout that adds the correction to u, the prolongation into that layout (patch_prolong_kernel
on the 2 x 2 levels, skew_prolong_pack_kernel on the one-line levels, which replaces prolongate_kernel + BC +
skew_pack_kernel); the ghost planes a relax loop leaves in the natural array are written by the launch that
copies the level out of the layout.  Every other box keeps the stand-alone BC.  Bit for bit against the oracle:
interiors AND face ghosts.

How the new paths are known to have run (no tally family was added for the BC launches: the table of families
ends where tests/test_diffusion_faces_abi_cpu.py pins it): they are selected by the sides of the domain alone,
there is no switch beside them to fall back to, and
  - PROLONGATION_FUSED counts one per level and cycle on the periodic boxes of 32^3 and 64^3, which have no
    2 x 2 level and counted none before, and stays 0 on the Dirichlet and mixed boxes of 64^3;
  - PROJECT_PAIRS / PROJECT_SCALAR tell which projection kernels ran on the 64^3 time steps (GFSHIP_PC_SCALAR=1
    keeps the scalar kernels and with them the stand-alone BC);
  - the face ghosts compared here are written by nobody else on those paths: a producer that left one out would
    leave the previous cycle's or step's value there.
The launch counts per step themselves are in profiles/ (kernel traces of the flagship box before and after)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "gerris-fft-particles_amd"), HERE):
    if _p not in sys.path:      # run as the child of the last test, without the suite's conftest
        sys.path.insert(0, _p)

import switch_cases as S            # noqa: E402
from flow_cases import PERIODIC     # noqa: E402

pytestmark = pytest.mark.gpu


def _differences(ora, got):
    bad = []
    if set(ora) != set(got):
        bad.append("keys differ: %s" % sorted(set(ora) ^ set(got)))
    for k in sorted(set(ora) & set(got)):
        a, b = np.asarray(ora[k]), np.asarray(got[k])
        if k.endswith("~"):       # summed norms: tree-reduced on the device
            if not (float(b) == pytest.approx(float(a), rel=S.RTOL_SUM)):
                bad.append("%s: oracle %r device %r" % (k, float(a), float(b)))
        elif a.shape != b.shape or not np.array_equal(a, b):
            bad.append("%s: differs%s" % (k, "" if a.ndim == 0 or a.shape != b.shape or k.endswith("#") else
                                          " in %d of %d cells" % (int((a != b).sum()), a.size)))
    return bad


# ---------------------------------------------------------------------------------------------
# V-cycles: two cycles, then a solve of three, dia == 0 and dia > 0 (tests/switch_cases.py: _case_vcycle)
# ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _vcycle_oracle(kind, level):
    return S._case_vcycle(kind, level)("oracle", None)


CYCLES = 2 * (2 + 3)      # of both passes (dia == 0, dia > 0) of the case
COARSE_TOP = 4            # the levels up to 16^3 are one launch (coarse_cycle_kernel): no prolongation of their own


@pytest.mark.parametrize("kind,level", [("periodic", 5), ("periodic", 6), ("periodic", 7),
                                        ("dirichlet", 6), ("mixed", 6)])
def test_vcycles_with_face_ghosts_against_the_oracle(kind, level):
    """32^3: the leaf is a one-line level above the coarse end; 64^3: adds the prolongation into the layout of
    32^3; 128^3: a 2 x 2 leaf with one-line levels below.  u (interior and the six face-ghost planes) and res after
    every cycle; the coarser levels of dp show through the next cycle's u; infty exact, first / second to 1e-12"""
    dev = S._Device()
    try:
        got = S._case_vcycle(kind, level)("device", dev)
        counts = S._counts(dev.domains)
    finally:
        for gd in dev.domains:
            gd.destroy()
    print("%s level %d: %s" % (kind, level, {k: v for k, v in counts.items() if v}))
    bad = _differences(_vcycle_oracle(kind, level), got)
    assert not bad, "\n".join(bad)
    if kind == "periodic":
        assert counts["PROLONGATION_FUSED"] == CYCLES * (level - COARSE_TOP) and counts["PROLONGATION_DECLINED"] == 0
    else:
        assert counts["PROLONGATION_FUSED"] == 0 and counts["PROLONGATION_DECLINED"] == 0


# ---------------------------------------------------------------------------------------------
# time steps: periodic Taylor-Green with the mean flow of switch_cases._tg, start + 3 steps
# ---------------------------------------------------------------------------------------------

NSTEPS = 3


def _snapshot(rec, tag, side, sim, full):
    whole = (lambda f: f.leaf()) if side == "oracle" else (lambda f: f.download())
    fields = [("P", sim.p), ("Pmac", sim.pmac)]
    for c in range(3):
        fields += [("U%d" % c, sim.u[c]), ("g%d" % c, sim.g[c]), ("gmac%d" % c, sim.gmac[c])]
    for name, f in fields:
        S._faces(rec, tag + name, whole(f), 3, full)
    rec[tag + "dt"] = float(sim.dt)
    rec[tag + "t"] = float(sim.t)


def _run_steps(side, level, dev=None):
    rec = S._Record()
    osim, _ = S._tg(level, 1, 0., False)
    sim = osim if side == "oracle" else dev.sim(osim, PERIODIC)[1]
    sim.start()
    _snapshot(rec, "start/", side, sim, False)
    for k in range(NSTEPS):
        sim.step()
        _snapshot(rec, "step%d/" % k, side, sim, k == NSTEPS - 1)
    return rec


@functools.lru_cache(maxsize=None)
def _steps_oracle(level):
    return _run_steps("oracle", level)


def _device_steps(level):
    dev = S._Device()
    try:
        rec = _run_steps("device", level, dev)
        counts = S._counts(dev.domains)
    finally:
        for gs in dev.sims:
            gs.destroy()
        for gd in dev.domains:
            gd.destroy()
    return rec, counts


@pytest.mark.parametrize("level", [4, 5, 6])
def test_time_steps_with_face_ghosts_against_the_oracle(level):
    """64^3 is the smallest box the sweep kernels and the pair kernels of the projections accept; 16^3 and 32^3
    take the general Godunov path and the scalar projection kernels, which keep the stand-alone BC"""
    got, counts = _device_steps(level)
    print("level %d: %s" % (level, {k: v for k, v in counts.items() if v}))
    bad = _differences(_steps_oracle(level), got)
    assert not bad, "\n".join(bad)
    if level == 6:
        assert counts["PROJECT_PAIRS"] > 0 and counts["PROJECT_SCALAR"] == 0
        assert counts["PROLONGATION_FUSED"] > 0 and counts["PROLONGATION_DECLINED"] == 0
    else:
        assert counts["PROJECT_PAIRS"] == 0


def test_time_steps_64_with_the_scalar_projection_kernels_in_a_fresh_process(tmp_path):
    """GFSHIP_PC_SCALAR=1 (looked up when the domain is created: a process of its own): the scalar kernels
    write no images, the stand-alone BC follows them, the same bits"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("GFSHIP_") or k in S.KEEP_IN_CHILD}
    env["GFSHIP_PC_SCALAR"] = "1"
    out = str(tmp_path / "steps.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "6", out], env=env, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0, "the child ended with status %d\n%s\n%s" % (p.returncode, p.stdout[-2000:],
                                                                          p.stderr[-4000:])
    counts = json.loads([x for x in p.stdout.splitlines() if x.startswith("COUNTS ")][-1][len("COUNTS "):])
    assert counts["PROJECT_SCALAR"] > 0 and counts["PROJECT_PAIRS"] == 0
    with np.load(out) as z:
        got = {k: z[k] for k in z.files}
    bad = _differences(_steps_oracle(6), got)
    assert not bad, "\n".join(bad)


if __name__ == "__main__":      # the child of the test above: LEVEL OUT.npz
    rec_, counts_ = _device_steps(int(sys.argv[1]))
    np.savez(sys.argv[2], **{k: np.asarray(v) for k, v in rec_.items()})
    print("COUNTS " + json.dumps(counts_))
