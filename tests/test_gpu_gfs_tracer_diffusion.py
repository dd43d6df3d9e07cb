"""tests/cases/tracer_diffusion.gfs (a GfsAdvection box, VariableTracer T { scheme = none }, SourceDiffusion T 1,
T = 1 on the four sides: the reference's test/diffusion without its Solid) through gfship2D against the same
run driven through the Python ABI; the same file as a GfsSimulation; the refusals of the front end."""
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
CASE = os.path.join(ROOT, "tests", "cases", "tracer_diffusion.gfs")
LEVEL, END, DTMAX = 4, 0.00085, 9e-5


def _python_run(path):
    """the run of the case file through the ABI; T written as a simulation file"""
    n = 1 << LEVEL
    gd = gfship.Domain(2, LEVEL)
    gs = gfship.Simulation(gd)
    try:
        T = gs.add_tracer()
        for d in range(4):
            T.set_bc(d, gfship.BC_DIRICHLET, np.full(n, 1.))
        gs.set_tracer_scheme(T, gfship.SCHEME_NONE)
        gs.set_tracer_diffusion(T, 1.)
        gs.tracer_diffusion_params(T).beta = 1.
        gs.advection_params.cfl = 1.7976931348623157e308     # min_cfl of advection_run without an advected tracer
        gd.bc(T)
        while gs.t < END:
            gs.set_time(END, DTMAX)
            gs.advection_step()
        data = gd.snapshot_tree([T])
        head = ("# Gerris Flow Solver 2D version 1.3.2 (test)\n"
                "1 0 GfsAdvection GfsBox GfsGEdge { version = 120812 variables = T binary = 1 } {\n"
                "  GfsTime { i = %d t = %.17g }\n}\n"
                "GfsBox { id = 1 pid = -1 size = %d x = 0 y = 0 z = 0 } {\n" % (gs.i, gs.t, n * n)).encode()
        with open(path, "wb") as f:
            f.write(head + data + b"}\n")
        return gs.t, gs.i, H.interior(T.download()), gs.tracer_diffusion_counts()
    finally:
        H.destroy_device(gd, gs)


def test_tracer_diffusion_case_equals_the_run_through_the_abi(tmp_path):
    r = subprocess.run([os.path.join(BIN, "gfship2D"), "-DLEVEL=%d" % LEVEL, "-DEND=%r" % END, CASE],
                       cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    t, i, T, counts = _python_run(str(tmp_path / "abi.gfs"))
    assert i == 10 and counts == (0, 10)              # ceil (END/dtmax) steps, all by the composed path (2-D)
    # diffusing in from the walls.  The exact implicit step keeps T between its start (0) and the walls (1); each
    # solve stops at a residual of at most the tolerance and the inverse of the operator has infinity norm at
    # most 1, so i solves leave that range by at most i * tolerance
    slack = i * 1e-6
    assert - slack <= T.min() and T.max() <= 1. + slack and T[0, 0] > T[8, 8] + 0.1
    step = [l for l in r.stdout.splitlines() if l.startswith("step:")][0].split()
    assert int(step[1]) == i and float(step[3]) == pytest.approx(t, abs=1e-8)
    c = subprocess.run([os.path.join(BIN, "gfshipcompare2D"), "-v", str(tmp_path / "end.gfs"),
                        str(tmp_path / "abi.gfs"), "T"], capture_output=True, text=True, timeout=120)
    assert c.returncode == 0, c.stderr
    m = re.search(r"total err first:\s*(\S+) second:\s*(\S+) infty:\s*(\S+)", c.stderr)
    assert float(m.group(3)) == 0., c.stderr
    # OutputDiffusionStats: the block of T (src/output.c:551-556)
    lines = r.stdout.splitlines()
    assert "T diffusion" in lines
    assert "niter:" in lines[lines.index("T diffusion") + 1]


def test_the_same_file_runs_as_a_simulation(tmp_path):
    text = open(CASE).read()
    assert text.count("GfsAdvection") == 1 and text.count("Time { end = END dtmax = 9e-5 }") == 1
    text = text.replace("GfsAdvection", "GfsSimulation").replace(
        "Time { end = END dtmax = 9e-5 }",
        "Time { iend = 3 }\n  Init {} {\n    U = sin(2.*M_PI*x)*cos(2.*M_PI*y)\n    V = -cos(2.*M_PI*x)*sin(2.*M_PI*y)\n  }")
    sim = tmp_path / "sim.gfs"
    sim.write_text(text)
    r = subprocess.run([os.path.join(BIN, "gfship2D"), "-DLEVEL=4", str(sim)], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    step = [l for l in lines if l.startswith("step:")][0].split()
    assert int(step[1]) == 3
    assert "T diffusion" in lines and "U diffusion" not in lines
    # not advected (scheme = none), T = 0 inside at the start and 1 on the walls: it stays between the two
    m = re.search(r"^T time:.* min:\s*(\S+) avg:\s*(\S+) \|\s*(\S+) max:\s*(\S+)", r.stdout, re.M)
    assert m, r.stdout
    slack = 4 * 1e-6 + 0.5e-3       # (the half step of the start and three steps: four solves; %10.3e rounds)
    assert - slack <= float(m.group(1)) < float(m.group(4)) <= 1. + slack


HEAD = "1 0 GfsSimulation GfsBox GfsGEdge {} {\n  Time { iend = 1 }\n  Refine %s\n  VariableTracer T\n"


@pytest.mark.parametrize("refine,body,line,what", [
    ("4", "  SourceDiffusion T 0.01*(1. + x)\n", 5, "must be a constant"),
    ("4", "  SourceDiffusion T U\n", 5, "must be a constant"),
    ("(x > 0 ? 5 : 4)", "  SourceDiffusion T 0.01\n", 5, "refined tree"),
    ("4", "  SourceDiffusion T 0.01\n  SourceDiffusion T 0.02 { beta = 0.5 }\n", 6, "only one diffusion source"),
], ids=["function", "variable", "refined-tree", "second-source"])
def test_front_end_refusals_name_their_line(tmp_path, refine, body, line, what):
    bad = tmp_path / "bad.gfs"
    bad.write_text(HEAD % refine + body + "}\nGfsBox {}\n")
    r = subprocess.run([os.path.join(BIN, "gfship2D"), str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "line %d" % line in r.stderr and what in r.stderr and "`T'" in r.stderr
