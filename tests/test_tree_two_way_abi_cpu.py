"""The entry points and variables of the two-way coupling on a tree are declared in include/gfship.h, exported by
the library and bound by the Python mirror (no GPU)."""
import os
import re

import gfship
from conftest import ROOT

ENTRIES = ("gfship_tree_particulate_field", "gfship_tree_particles_forces_on_fluid",
           "gfship_tree_particles_set_kernel", "gfship_tree_particles_spread_forces",
           "gfship_tree_source_particulate_event", "gfship_tree_set_source_fields", "gfship_tree_mac_source")


def header():
    return open(os.path.join(ROOT, "include", "gfship.h")).read()


def test_entries_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    L = gfship.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert name in gfship.SIGNATURES and getattr(L, name).restype is gfship.SIGNATURES[name][0]
    for method in ("particulate_field", "forces_on_fluid", "set_kernel", "spread_forces", "source_particulate_event",
                   "set_source_fields", "mac_source"):
        assert callable(getattr(gfship.Tree, method))


def test_enum_values_are_appended():
    """the GFSHIP_TREE_* numbers of the header, counted: no earlier number moves, the four new ones follow WPREV
    (in an enum of their own that starts at GFSHIP_TREE_WPREV + 1: tests/test_tree_particulates_abi_cpu.py keeps
    UPREV, VPREV, WPREV the last three of the first)"""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    m = re.search(r"enum\s*\{\s*(GFSHIP_TREE_P\s*=\s*0.*?)\}", text, flags=re.S)
    names = [x.strip().split("=")[0].strip() for x in m.group(1).split(",") if x.strip()]
    value = {n: i for i, n in enumerate(names)}
    assert value["GFSHIP_TREE_WPREV"] == 27 == gfship.Tree.WPREV and names[-1] == "GFSHIP_TREE_WPREV"
    m = re.search(r"enum\s*\{\s*GFSHIP_TREE_VF\s*=\s*GFSHIP_TREE_WPREV\s*\+\s*1\s*,(.*?)\}", text, flags=re.S)
    more = ["GFSHIP_TREE_VF"] + [x.strip() for x in m.group(1).split(",") if x.strip()]
    assert more == ["GFSHIP_TREE_VF", "GFSHIP_TREE_FX", "GFSHIP_TREE_FY", "GFSHIP_TREE_FZ"]
    for k, n in enumerate(more):
        value[n] = value["GFSHIP_TREE_WPREV"] + 1 + k
    assert [value["GFSHIP_TREE_" + n] for n in ("VF", "FX", "FY", "FZ")] == [28, 29, 30, 31]
    assert (gfship.Tree.VF, gfship.Tree.FX, gfship.Tree.FY, gfship.Tree.FZ) == (28, 29, 30, 31)
    assert gfship.Tree.RES == value["GFSHIP_TREE_RES"] and gfship.Tree.DIV == value["GFSHIP_TREE_DIV"]
