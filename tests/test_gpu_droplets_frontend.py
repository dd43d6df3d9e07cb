"""tests/cases/droplets.gfs through the front end (gfship2D) against the restatements: the list written by
`--particles', byte for byte, and the tracers of GfsOutputSimulation { format = text }."""
import os
import subprocess

import numpy as np
import pytest

import droplets_reference as DR
import feed_particle_reference as FP
import forces_reference as FR
import sampler_cases as SK
from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin", "gfship2D")
CASE = os.path.join(ROOT, "tests", "cases", "droplets.gfs")
LEVEL, NSTEPS, DT, IDLAST = 4, 2, 0.015625, 40


def _T(x, y):
    return (0.5 + 0.25*x if abs(x + 0.28125) < 0.07 and abs(y - 0.21875) < 0.1 else
            (0.75 + 0.125*y if abs(x - 0.15625) < 0.2 and abs(y + 0.15625) < 0.2 else
             (0.3 if abs(x - 0.40625) < 0.04 and abs(y - 0.40625) < 0.04 else
              (0.4 if x > 0.45 and abs(y) < 0.07 else 0.))))


def _S(x, y):
    return (0.6 if abs(x + 0.1875) < 0.05 and abs(y + 0.3125) < 0.05 else
            (0.9 if abs(x - 0.28125) < 0.07 and abs(y - 0.28125) < 0.07 else 0.))


def _restatement():
    """the case in the restatements: the fluid is at rest and stays there, the tracers are advected by nothing; per
    step the event of the list (drag), the droplets of T, the droplets of S.  Returns the text of `--particles' and
    the tracers at the end"""
    dim, n = 2, 1 << LEVEL
    box, sides = SK.box(dim, LEVEL), SK.SIDES["periodic"]
    zero = np.zeros((n + 2,)*dim)
    T, S = zero.copy(), zero.copy()
    for cell in box.leaves:
        x, y = box.cell_pos(cell)[:2]
        i, j, _ = cell.ijk
        T[j, i], S[j, i] = _T(x, y), _S(x, y)
    sim = FR.Sim(box, sides, (zero, zero), DT, viscosity=(lambda cell: 1e-2,)*3, root=FR.sqrt_root)
    objs = [FR.ForceCoeff(FR.DRAG)]
    FR.read_forces(sim, objs)
    pl = FP.ParticleList([FR.Particulate([0.11, 0.23, 0.], 3, [0.5, -0.25, 0.], 2e-3, 1e-3),
                          FR.Particulate([-0.31, 0.07, 0.], 7, [0.1, -0.2, 0.], 1.5e-3, 1e-3)], IDLAST)
    infos, removed = [], []
    for step in range(NSTEPS + 1):          # the events of steps 0 .. NSTEPS - 1, and those after the loop
        pl.plist = FR.list_event(sim, pl.plist, objs)
        infos.append(DR.event(box, sides, pl, T, (zero, zero), 12, 0.)[0])
        removed.append(DR.remove_droplets(box, sides, S, S, 5, 0.))
    # four droplets, one particle, 9 + 1 + 2 cells reset; afterwards the large droplet alone
    assert infos[0] == (4, 12, 1, 12) and infos[1] == (1, 12, 0, 0)
    assert removed[0] == (2, 5, 4) and removed[1] == (1, 5, 0)
    lines = ["GfsParticleList GfsParticulate {"]
    for p in pl.plist:
        lines.append("    GfsParticulate %d %g %g %g %g %g %g %g %g %g %g %g" %
                     (p.id, p.pos[0], p.pos[1], 0., p.mass, p.volume, p.vel[0], p.vel[1], p.vel[2],
                      p.force[0], p.force[1], p.force[2]))
    lines.append("}")
    return "\n".join(lines) + "\n", pl, box, T, S


def test_the_front_end_turns_the_droplet_of_the_case_into_a_particle(tmp_path):
    want, pl, box, T, S = _restatement()
    assert [p.id for p in pl.plist] == [3, 7, IDLAST + 1] and pl.idlast == IDLAST + 1
    out = tmp_path / "particles.txt"
    r = subprocess.run([BIN, "-DLEVEL=%d" % LEVEL, "-DNSTEPS=%d" % NSTEPS, CASE, "--particles", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    assert out.read_text() == want
    rows = (tmp_path / "droplets_fields.txt").read_text().splitlines()
    assert rows[0] == "# 1:x 2:y 3:z 4:T 5:S"
    got = {tuple(row.split()[:2]): row.split()[3:] for row in rows[1:]}
    assert len(got) == len(box.leaves)
    for cell in box.leaves:
        x, y = box.cell_pos(cell)[:2]
        i, j, _ = cell.ijk
        assert got[("%g" % x, "%g" % y)] == ["%g" % T[j, i], "%g" % S[j, i]], (x, y)
    assert (T > 0.).sum() == 49 and (S > 0.).sum() == 9

