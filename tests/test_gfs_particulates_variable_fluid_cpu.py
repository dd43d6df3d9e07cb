"""Simulation files with GfsParticulate forces in a fluid of variable density that the front end refuses before
it touches a device, with the line number: alpha naming a tracer (the density at a particle is alpha at the
centre of its cell, evaluated on the host), and a viscosity function that does not compile."""
import os
import subprocess

from conftest import ROOT

BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin")


def test_alpha_that_names_a_tracer_with_particle_forces_is_refused_with_the_line_number(tmp_path):
    bad = tmp_path / "bad.gfs"
    bad.write_text("1 0 GfsSimulation GfsBox GfsGEdge {} {\n  Time { iend = 1 }\n  Refine 4\n  VariableTracer T\n"
                   "  GModule particulates\n  PhysicalParams { alpha = 1./(1. + T) }\n"
                   "  GfsParticleList { istep = 1 } GfsParticulate {\n    GfsParticulate 1 0.1 0.2 0 2e-3 1e-3 0 0 0\n"
                   "  } {\n    GfsForceBuoy\n  }\n}\nGfsBox {}\n")
    r = subprocess.run([os.path.join(BIN, "gfship2D"), str(bad)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "line 6" in r.stderr and "alpha may depend on x, y, z and t" in r.stderr
    assert "GfsParticulate forces" in r.stderr and "`T'" in r.stderr


def test_a_function_that_does_not_compile_exits_before_the_device(tmp_path):
    bad = tmp_path / "bad.gfs"
    bad.write_text("1 0 GfsSimulation GfsBox GfsGEdge {} {\n  Time { iend = 1 }\n  Refine 4\n"
                   "  GModule particulates\n  SourceViscosity 0.01*(1.5 + +* y)\n"
                   "  GfsParticleList { istep = 1 } GfsParticulate {\n    GfsParticulate 1 0.1 0.2 0 2e-3 1e-3 0 0 0\n"
                   "  } {\n    GfsForceDrag\n  }\n}\nGfsBox {}\n")
    r = subprocess.run([os.path.join(BIN, "gfship2D"), str(bad)], capture_output=True, text=True, timeout=120)
    # the compiler's message carries the line of the file: "simulation file:5:33: error: ..."
    assert r.returncode != 0 and "simulation file:5:" in r.stderr and "error" in r.stderr
