"""tests/cases/evaporation.gfs through the front end on the device: the two GfsOutputScalarSum columns and the
particle file (--particles) against the restatement of the reference (tests/particulate_sources_reference.py for
the two sources, tests/forces_reference.py for the events of the list), driven by the fields of the same run
made through the Python mirror.  The column of the mass source and the masses are exact; what the cube root
touches lies in the hull of the restatement with its radius function moved by the bound of the device's pow."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import forces_reference as FR
import gfship
import particulate_sources_reference as PS
import sampler_cases as SK
from conftest import ROOT
from flow_cases import PERIODIC, reynolds_init
from test_gpu_particulate_sources import POW_ULPS, _shifted_pow

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin", "gfship2D")
CASE = os.path.join(ROOT, "tests", "cases", "evaporation.gfs")
LEVEL, NSTEPS = 4, 2
NU = 1e-2


def _particulates_of_the_case():
    rows = []
    for line in open(CASE):
        w = line.split()
        if len(w) >= 10 and w[0] == "GfsParticulate" and w[1].isdigit():
            rows.append([float(q) for q in w[1:10]])
    a = np.array(rows)
    return a[:, 0].astype(np.uint32), a[:, 1:4].copy(), a[:, 4].copy(), a[:, 5].copy(), a[:, 6:9].copy()


def _fields_of_the_run():
    """the same run through the Python mirror: (U, V, T with ghosts, dt, t) at every visit of the events"""
    n = 1 << LEVEL
    gd = gfship.Domain(2, LEVEL, PERIODIC)
    gs = gfship.Simulation(gd)
    try:
        for c in range(2):
            gs.set_viscosity(c, NU)
        gs.projection_params.tolerance = gs.approx_projection_params.tolerance = 1e-6
        gs.set_time(end=2.)
        T = gs.add_tracer()
        c = -0.5 + (np.arange(1, n + 1) - 0.5) / n
        x, y = c[None, :] + 0. * c[:, None], c[:, None] + 0. * c[None, :]
        u, v = reynolds_init(x, y)
        for var, a in zip(list(gs.u) + [T], (u, v, (1. + 0.5 * x - 0.25 * y * x))):
            full = np.zeros((n + 2, n + 2))
            full[1:-1, 1:-1] = a
            var.upload(full)
        gs.start()
        visits = []
        for k in range(NSTEPS + 1):
            visits.append(([gs.u[0].download(), gs.u[1].download()], T.download(), gs.dt, gs.t))
            if k < NSTEPS:
                gs.step()
        return visits
    finally:
        gs.destroy()
        gd.destroy()


def _restatement(visits, steps):
    """the events of the file in its order, the radius function moved by `steps' ulps: per visit the two sums as
    gfs_output_scalar_sum_event adds them, and the list at the end"""
    box = SK.box(2, LEVEL)
    ids, pos, mass, vol, vel = _particulates_of_the_case()
    plist = [FR.Particulate(pos[q], ids[q], vel[q], mass[q], vol[q]) for q in range(len(ids))]
    pow_ = _shifted_pow(steps)
    diameter = FR._diameter
    FR._diameter = lambda p: 2.*pow_(3.0*p.volume/4.0/math.pi, 1./3.)
    fvol, fmass = PS.Fields(2), PS.Fields(2)
    sums = []
    changed = False
    try:
        for u, T, dt, t in visits:
            sim = FR.Sim(box, PERIODIC, u, dt, viscosity=(lambda cell: NU,)*3, root=FR.sqrt_root)
            if not changed:      # until a volume event has run the diameters are the host's (glibc's pow)
                FR._diameter = diameter
            plist = FR.list_event(sim, plist, [FR.ForceCoeff(FR.DRAG)])
            FR._diameter = lambda p: 2.*pow_(3.0*p.volume/4.0/math.pi, 1./3.)
            changed = True
            uf = [box.field(a) for a in u]
            PS.event(box, PS.VOLUME, plist, uf, dt, t,
                     lambda V: (- 2e-5*V["T"]*(V["Urelp"]*V["Urelp"] + V["Vrelp"]*V["Vrelp"])), fvol,
                     {"T": box.field(T)}, pow_)
            PS.event(box, PS.MASS, plist, uf, dt, t, lambda V: 2e-5, fmass, {}, pow_)
            h = 1./(1 << LEVEL)
            row = []
            for f in (fvol, fmass):
                s = 0.
                for cell in sorted(box.leaves, key=lambda c: (c.ijk[1], c.ijk[0])):     # for_each_cell: j, then i
                    s += h*h*f.deposit[cell.ijk]
                row.append(s)
            sums.append(row)
    finally:
        FR._diameter = diameter
    return sums, plist


def _gfmt(x):
    return float("%g" % x)


def test_the_case_against_the_restatement(tmp_path):
    r = subprocess.run([BIN, "-DLEVEL=%d" % LEVEL, "-DNSTEPS=%d" % NSTEPS, "--particles", "drops.txt", CASE],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = {"Dvol": [], "Dmass": []}
    for line in r.stdout.splitlines():
        m = re.match(r"(Dvol|Dmass) time: (\S+) sum: +(\S+)$", line)
        if m:
            got[m.group(1)].append((float(m.group(2)), m.group(3)))
    assert len(got["Dvol"]) == len(got["Dmass"]) == NSTEPS + 1
    visits = _fields_of_the_run()
    runs = [_restatement(visits, s) for s in (-POW_ULPS, 0, POW_ULPS)]
    for k in range(NSTEPS + 1):
        assert got["Dmass"][k][0] == got["Dvol"][k][0] == _gfmt(visits[k][3])
        # the mass column is exact: the text gfs_output_scalar_sum_event prints
        assert got["Dmass"][k][1] == ("% 15.6e" % runs[1][0][k][1]).strip()
        vals = [float("% 15.6e" % run[0][k][0]) for run in runs]
        assert min(vals) <= float(got["Dvol"][k][1]) <= max(vals) and max(vals) < 0.
    rows = [l.split() for l in (tmp_path / "drops.txt").read_text().splitlines() if l.startswith("    GfsParticulate")]
    assert len(rows) == len(runs[1][1]) == 12
    for q, w in enumerate(rows):
        ps = [run[1][q] for run in runs]
        assert int(w[1]) == ps[1].id
        assert float(w[5]) == _gfmt(ps[1].mass)             # mass: the constant source alone, exact
        want = [[_gfmt(v) for v in p.pos[:2] + [0., 0., p.volume] + p.vel[:2] + [0.] + p.force[:2]] for p in ps]
        have = [float(x) for x in w[2:4] + ["0", "0"] + w[6:9] + ["0"] + w[10:12]]
        for x, col in zip(have, zip(*want)):
            assert min(col) <= x <= max(col), (q, x, col)
    # no drop has gained volume, and most losses show in the six digits of the file
    before = _particulates_of_the_case()[3]
    after = np.array([float(w[6]) for w in rows])
    assert (after <= before).all() and (after < before).sum() >= 6


def test_an_unknown_name_in_the_function_fails_with_the_line(tmp_path):
    """a name that is no device variable of the run and none of Rad, Urelp, Vrelp, x, y, z, t: the compiler of the
    device reports it, and the front end adds the line of the object"""
    text = open(CASE).read().replace("- 2e-5*T*", "- 2e-5*Humidity*")
    bad = tmp_path / "bad.gfs"
    bad.write_text(text)
    r = subprocess.run([BIN, "-DLEVEL=%d" % LEVEL, "-DNSTEPS=1", str(bad)], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=300)
    line = 1 + text[:text.index("  GfsSourceParticulateVol {")].count("\n")
    assert r.returncode != 0
    assert ("gfship: line %d: the function" % line) in r.stderr and "Humidity" in r.stderr, r.stderr
