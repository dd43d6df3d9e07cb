"""The C ABI of the particle forces in a fluid of variable density and viscosity, without a device:
gfship_sim_set_viscosity_cell is exported by the library, declared in include/gfship.h under a comment that
cites the reference, and bound by the python package; with a null simulation it returns GFSHIP_EINVAL; the
header no longer rules out particle forces together with a viscosity given at the faces."""
import os
import re

import gfship
from conftest import ROOT

NAME = "gfship_sim_set_viscosity_cell"
GFSHIP_EINVAL = -1


def _header():
    return open(os.path.join(ROOT, "include", "gfship.h")).read()


def test_the_entry_point_is_exported_declared_and_bound():
    L = gfship.lib()
    assert hasattr(L, NAME), "libgfship.so does not export %s" % NAME
    assert NAME in gfship.SIGNATURES
    assert gfship.SIGNATURES[NAME] == gfship.SIGNATURES["gfship_sim_set_alpha_cell"]
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+%s\s*\(" % NAME, _header(), flags=re.S)
    assert m, "%s is not declared under a comment" % NAME
    assert re.search(r"src/\w+\.c:\d+", m.group(1)), "%s does not cite the reference" % NAME
    assert hasattr(gfship.Simulation, "set_viscosity_cell")


def test_a_null_simulation_is_an_invalid_argument():
    L = gfship.lib()
    assert L.gfship_sim_set_viscosity_cell(None, 0) == GFSHIP_EINVAL
    assert L.gfship_sim_set_viscosity_cell(None, -1) == GFSHIP_EINVAL
    assert b"null" in L.gfship_last_error()


def test_the_header_describes_the_fields_of_the_fluid():
    text = " ".join(_header().split())
    assert "not together with particle forces" not in text
    assert "fluid density 1 (alpha = NULL)" not in text
    block = text[text.index("GfsParticulate with forces"):text.index("GFSHIP_FORCE_INERTIAL = 1")]
    assert "gfship_sim_set_alpha_cell" in block and NAME in block
