"""tests/cases/particulates_variable_fluid.gfs (twenty GfsParticulate with the five forces in the box of
variable_viscosity.gfs: GfsSourceViscosity with a function of y, GfsPhysicalParams { alpha } with a function of
x, symmetry walls, gravity from a GfsSource) through gfship2D --particles against the same run driven through
the Python ABI with the fields evaluated in numpy -- the viscosity at the face centres and at the leaf centres,
alpha at the face centres and at the cell centres of every level.  Each expression of the file rounds once per
value, so the compiled functions and numpy give the same bits: the rows of the list, printed with %g like the
front end prints them, must be the same strings."""
import os
import subprocess

import numpy as np
import pytest

import gfship
import hook_cases as H
from conftest import ROOT

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin")
CASES = os.path.join(ROOT, "tests", "cases")
LEVEL, NSTEPS = 5, 3
FORCES = [gfship.FORCE_INERTIAL, gfship.FORCE_ADDEDMASS, gfship.FORCE_LIFT, gfship.FORCE_DRAG, gfship.FORCE_BUOY]


def _particulates_of_the_case():
    rows = []
    for line in open(os.path.join(CASES, "particulates_variable_fluid.gfs")):
        w = line.split()
        if len(w) >= 10 and w[0] == "GfsParticulate" and w[1].isdigit():
            rows.append([float(q) for q in w[1:10]])
    a = np.array(rows)
    return a[:, 0].astype(np.uint32), a[:, 1:4].copy(), a[:, 4].copy(), a[:, 5].copy(), a[:, 6:9].copy()


def _python_run():
    """the run of the case file through the ABI: the rows of its list as the front end prints them"""
    dim, n = 2, 1 << LEVEL
    ids, pos, mass, vol, vel = _particulates_of_the_case()
    assert len(ids) == 20
    gd = gfship.Domain(dim, LEVEL)
    gs = gfship.Simulation(gd)
    pl = None
    try:
        x, y = H._grids(dim, n)
        D, A = [], []
        for c in range(dim):
            xf, yf = x + (0.5 / n if c == 0 else 0.), y + (0.5 / n if c == 1 else 0.)
            d, a = gd.variable(), gd.variable()
            d.upload(0.01 * (1.5 + yf))
            a.upload(1. / (1.5 + xf))
            D.append(d)
            A.append(a)
        ac, mu = gd.variable(), gd.variable()
        for l in range(LEVEL + 1):
            xl, yl = H._grids(dim, 1 << l)
            ac.upload(1. / (1.5 + xl) + 0. * yl, l)
        mu.upload(0.01 * (1.5 + y) + 0. * x)
        gs.set_source(1, -0.5)
        gs.set_alpha_cell(ac)
        for c in range(dim):
            gs.set_viscosity_faces(c, D)
        gs.set_viscosity_cell(mu)
        # the list is read while the fields hold the zeros of a fresh simulation (Un = Vn = 0)
        pl = gfship.ParticleList(gs, pos, ids)
        pl.set_particulate(vel, mass, vol)
        pl.set_forces(FORCES, (0., -0.5, 0.))
        u = np.zeros((n + 2, n + 2))
        v = np.zeros((n + 2, n + 2))
        H.interior(u)[...] = H.interior((0.25 - x * x) * y)
        H.interior(v)[...] = H.interior(x * (y * y - 0.25))
        gs.u[0].upload(u)
        gs.u[1].upload(v)
        gs.set_alpha(A)
        gs.start()
        for _ in range(NSTEPS):
            pl.event()
            gs.step()
        pl.event()
        p, i = pl.download()
        w, m, f = pl.particulate_state()
        volume = dict(zip(ids.tolist(), vol.tolist()))
        rows = []
        for q in range(len(i)):
            vals = [p[q, 0], p[q, 1], p[q, 2], m[q], volume[int(i[q])], w[q, 0], w[q, 1], w[q, 2],
                    f[q, 0], f[q, 1], f[q, 2]]
            rows.append(["GfsParticulate", "%d" % i[q]] + ["%g" % a for a in vals])
        return rows
    finally:
        if pl is not None:
            pl.destroy()
        H.destroy_device(gd, gs)


def test_the_case_equals_the_run_through_the_abi(tmp_path):
    outp = tmp_path / "plist.txt"
    r = subprocess.run([os.path.join(BIN, "gfship2D"), "--particles", str(outp), "-DLEVEL=%d" % LEVEL,
                        "-DNSTEPS=%d" % NSTEPS, os.path.join(CASES, "particulates_variable_fluid.gfs")],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = [l.split() for l in open(outp) if l.strip().startswith("GfsParticulate ")]
    want = _python_run()
    assert len(got) >= 15
    # the forces act: a particle of the list that falls has a force and a mass grown by the added mass
    assert all(float(row[10]) != 0. or float(row[11]) != 0. for row in got)
    assert got == want
