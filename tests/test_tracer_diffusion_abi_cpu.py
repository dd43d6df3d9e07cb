"""GfsSourceDiffusion on a tracer: the entry points are declared, exported and bound, and a null handle is an
error (no device needed)."""
import ctypes as C
import os
import re

import pytest

import gfship
from conftest import ROOT

NAMES = ["gfship_sim_set_tracer_diffusion", "gfship_sim_tracer_diffusion_params", "gfship_sim_set_tracer_scheme",
         "gfship_sim_tracer_diffusion_path", "gfship_sim_tracer_diffusion_counts"]
EINVAL = -1


@pytest.mark.parametrize("name", NAMES)
def test_symbol_is_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "gfship.h")).read()
    assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert hasattr(gfship.lib(), name)
    assert name in gfship.SIGNATURES


def test_scheme_constants_follow_the_reference_enum():
    # GfsAdvectionScheme, src/advection.h:32-35
    header = open(os.path.join(ROOT, "include", "gfship.h")).read()
    assert re.search(r"GFSHIP_SCHEME_GODUNOV = 0, GFSHIP_SCHEME_NONE = 1", header)
    assert (gfship.SCHEME_GODUNOV, gfship.SCHEME_NONE) == (0, 1)


def test_null_handles_are_einval():
    L = gfship.lib()
    assert L.gfship_sim_set_tracer_diffusion(None, 0, 1.) == EINVAL
    assert L.gfship_sim_set_tracer_scheme(None, 0, gfship.SCHEME_NONE) == EINVAL
    assert L.gfship_sim_tracer_diffusion_path(None, 1) == EINVAL
    counts = (C.c_ulonglong * 2)()
    assert L.gfship_sim_tracer_diffusion_counts(None, counts) == EINVAL
    assert not L.gfship_sim_tracer_diffusion_params(None, 0)
    for name in ("set_tracer_diffusion", "tracer_diffusion_params", "set_tracer_scheme", "tracer_diffusion_path",
                 "tracer_diffusion_counts"):
        assert callable(getattr(gfship.Simulation, name))
