"""tests/cases/variable_viscosity.gfs (GfsSourceViscosity with a function of y, GfsPhysicalParams { alpha } with
a function of x, a box with symmetry walls) through gfship2D against the same run driven through the Python
ABI with the fields evaluated in numpy: the viscosity at the face centres, alpha at the face centres and at the
cell centres of every level.  Each expression of the file rounds once per value, so the compiled functions
and numpy give the same bits, and the cell data of the two runs must be equal."""
import os
import re
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


def _python_run(path):
    """the run of the case file through the ABI; its cell data written as a simulation file"""
    dim, n = 2, 1 << LEVEL
    gd = gfship.Domain(dim, LEVEL)
    gs = gfship.Simulation(gd)
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
        ac = gd.variable()
        for l in range(LEVEL + 1):
            xl, yl = H._grids(dim, 1 << l)
            ac.upload(1. / (1.5 + xl) + 0. * yl, l)
        gs.set_alpha_cell(ac)
        for c in range(dim):
            gs.set_viscosity_faces(c, D)
        gs.set_alpha(A)
        u = np.zeros((n + 2, n + 2))
        v = np.zeros((n + 2, n + 2))
        H.interior(u)[...] = H.interior((0.25 - x * x) * y)
        H.interior(v)[...] = H.interior(x * (y * y - 0.25))
        gs.u[0].upload(u)
        gs.u[1].upload(v)
        gs.start()
        for _ in range(NSTEPS):
            gs.step()
        names = ["U", "V", "P"]
        data = gd.snapshot_tree([gs.u[0], gs.u[1], gs.p])
        head = ("# Gerris Flow Solver 2D version 1.3.2 (test)\n"
                "1 0 GfsSimulation GfsBox GfsGEdge { version = 120812 variables = %s binary = 1 } {\n"
                "  GfsTime { i = %d t = %.17g }\n}\n"
                "GfsBox { id = 1 pid = -1 size = %d x = 0 y = 0 z = 0 } {\n"
                % (",".join(names), gs.i, gs.t, n * n)).encode()
        with open(path, "wb") as f:
            f.write(head + data + b"}\n")
        return gs.t, gd.kernel_counts()
    finally:
        H.destroy_device(gd, gs)


def test_variable_viscosity_case_equals_the_run_through_the_abi(tmp_path):
    r = subprocess.run([os.path.join(BIN, "gfship2D"), "-DLEVEL=%d" % LEVEL, "-DNSTEPS=%d" % NSTEPS,
                        os.path.join(CASES, "variable_viscosity.gfs")], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    t, kc = _python_run(str(tmp_path / "abi.gfs"))
    assert kc["ADVECT_GENERAL"] > 0
    step = [l for l in r.stdout.splitlines() if l.startswith("step:")][0].split()
    assert int(step[1]) == NSTEPS and float(step[3]) == pytest.approx(t, abs=1e-8)
    end = (tmp_path / "end.gfs").read_bytes()
    m = re.search(rb"GfsTime \{ i = (\d+) t = (\S+)", end)
    assert int(m.group(1)) == NSTEPS and float(m.group(2)) == t
    for var in ("U", "V", "P"):
        c = subprocess.run([os.path.join(BIN, "gfshipcompare2D"), "-v", str(tmp_path / "end.gfs"),
                            str(tmp_path / "abi.gfs"), var], capture_output=True, text=True, timeout=120)
        assert c.returncode == 0, c.stderr
        m = re.search(r"total err first:\s*(\S+) second:\s*(\S+) infty:\s*(\S+)", c.stderr)
        assert float(m.group(3)) == 0., (var, c.stderr)


@pytest.mark.parametrize("line,what", [("  SourceViscosity 0.01*(1. + T)", "diffusion coefficient"),
                                        ("  SourceDiffusion U 0.01*(1. + T)", "diffusion coefficient")])
def test_a_coefficient_that_names_a_tracer_is_refused_with_the_line_number(tmp_path, line, what):
    bad = tmp_path / "bad.gfs"
    bad.write_text("1 0 GfsSimulation GfsBox GfsGEdge {} {\n  Time { iend = 1 }\n  Refine 4\n  VariableTracer T\n"
                   + line + "\n}\nGfsBox {}\n")
    r = subprocess.run([os.path.join(BIN, "gfship2D"), str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "line 5" in r.stderr and what in r.stderr and "`T'" in r.stderr


def test_alpha_that_names_a_tracer_with_a_viscosity_is_refused_with_the_line_number(tmp_path):
    bad = tmp_path / "bad.gfs"
    bad.write_text("1 0 GfsSimulation GfsBox GfsGEdge {} {\n  Time { iend = 1 }\n  Refine 4\n  VariableTracer T\n"
                   "  SourceViscosity 0.01\n  PhysicalParams { alpha = 1./(1. + T) }\n}\nGfsBox {}\n")
    r = subprocess.run([os.path.join(BIN, "gfship2D"), str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "line 6" in r.stderr and "alpha" in r.stderr and "`T'" in r.stderr
