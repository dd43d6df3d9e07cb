"""The C ABI of the implicit diffusion with per-face coefficients and a variable density, without a device:
the four entry points are exported by the library, declared in include/gfship.h (each citing the reference
lines it replaces) and bound by the python package; called with a null domain or simulation they return
GFSHIP_EINVAL; the two kernel counters are the last two of the table."""
import ctypes as C
import os
import re

import gfship
from conftest import ROOT

NEW = ("gfship_diffusion_coefficients_faces", "gfship_sim_set_viscosity_faces", "gfship_sim_set_alpha_cell",
       "gfship_variable_mac_source")
GFSHIP_EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "gfship.h")).read()


def test_the_four_entry_points_are_exported_declared_and_bound():
    L = gfship.lib()
    text = _header()
    for name in NEW:
        assert hasattr(L, name), "libgfship.so does not export %s" % name
        assert name in gfship.SIGNATURES
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % name, text, flags=re.S)
        assert m, "%s is not declared under a comment" % name
        assert re.search(r"src/\w+\.c:\d+", m.group(1)), "%s does not cite the reference" % name
    for method in ("diffusion_coefficients_faces",):
        assert hasattr(gfship.Domain, method)
    for method in ("set_viscosity_faces", "set_alpha_cell", "variable_mac_source"):
        assert hasattr(gfship.Simulation, method)


def test_null_handles_are_invalid_arguments():
    L = gfship.lib()
    D = (C.c_int * 3)(0, 1, 2)
    assert L.gfship_diffusion_coefficients_faces(None, D, 0.1, 0, -1, 1.) == GFSHIP_EINVAL
    assert L.gfship_sim_set_viscosity_faces(None, 0, D) == GFSHIP_EINVAL
    assert L.gfship_sim_set_alpha_cell(None, 0) == GFSHIP_EINVAL
    assert L.gfship_variable_mac_source(None, 0, 0) == GFSHIP_EINVAL
    assert b"null" in L.gfship_last_error()


def test_the_kernel_counters_end_the_table():
    assert gfship.KERNEL_COUNT_NAMES[-2:] == ("DIFFUSION_FACES_PIPELINED", "DIFFUSION_FACES_HYPERPLANES")
    text = _header()
    body = text[text.index("GFSHIP_KC_PREDICT_SWEEP"):text.rindex("GFSHIP_KC_COUNT")]
    assert re.findall(r"GFSHIP_KC_([A-Z0-9_]+)", body)[-2:] == list(gfship.KERNEL_COUNT_NAMES[-2:])


def test_the_header_no_longer_rules_out_alpha_with_a_viscosity():
    assert "Not together with GfsSourceDiffusion" not in _header()
