"""GfsSourceParticulateVol / GfsSourceParticulateMass on refined trees without a device: the two entry points are
declared in include/gfship.h, exported by the library and bound by the Python mirror, and the six variables have
the numbers that follow the two older enums of the tree."""
import os
import re

import gfship
from conftest import ROOT

ENTRIES = ("gfship_tree_particulate_source_create", "gfship_tree_particulate_source_set_fields")
NAMES = ("RAD", "URELP", "VRELP", "WRELP", "VOLSRC", "DMDT")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gfship.h")).read(), flags=re.S)


def test_entries_are_declared_exported_and_bound():
    text = _header()
    L = gfship.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert name in gfship.SIGNATURES and getattr(L, name).restype is gfship.SIGNATURES[name][0]
    # the arguments: the handle of the box's calls, a table of names and GFSHIP_TREE_* numbers
    assert re.search(r"gfship_tree_particulate_source_create\s*\(gfship_particulate_source \*\* src, gfship_particles \* pl, "
                     r"int kind,\s*const char \* function, int nvars, const char \* const \* names,\s*const int \* vars\);",
                     text)
    assert re.search(r"gfship_tree_particulate_source_set_fields\s*\(gfship_particulate_source \* src, int rad, "
                     r"const int urel\[3\],\s*int deposit\);", text)
    assert len(gfship.SIGNATURES["gfship_tree_particulate_source_create"][1]) == 7
    assert len(gfship.SIGNATURES["gfship_tree_particulate_source_set_fields"][1]) == 4


def test_the_six_variables_are_32_to_37_in_a_third_enum():
    text = _header()
    m = re.search(r"enum\s*\{\s*GFSHIP_TREE_RAD\s*=\s*GFSHIP_TREE_FZ\s*\+\s*1\s*,\s*GFSHIP_TREE_URELP\s*,\s*GFSHIP_TREE_VRELP\s*,"
                  r"\s*GFSHIP_TREE_WRELP\s*,\s*GFSHIP_TREE_VOLSRC\s*,\s*GFSHIP_TREE_DMDT\s*\}", text)
    assert m, "the third enum starts at GFSHIP_TREE_FZ + 1"
    # ... and GFSHIP_TREE_FZ is 31: the two enums before it are what they were
    first = re.search(r"enum\s*\{\s*GFSHIP_TREE_P\s*=\s*0\s*,(.*?)\}", text, flags=re.S).group(1)
    assert len([x for x in first.split(",") if x.strip()]) + 1 == 28 and first.split(",")[-1].strip() == "GFSHIP_TREE_WPREV"
    assert re.search(r"enum\s*\{\s*GFSHIP_TREE_VF\s*=\s*GFSHIP_TREE_WPREV\s*\+\s*1\s*,\s*GFSHIP_TREE_FX\s*,\s*GFSHIP_TREE_FY\s*,"
                     r"\s*GFSHIP_TREE_FZ\s*\}", text)
    assert gfship.Tree.FZ == 31
    assert [getattr(gfship.Tree, n) for n in NAMES] == [32, 33, 34, 35, 36, 37]


def test_the_python_mirror_has_the_class():
    cls = gfship.TreeParticulateSource
    for method in ("set_fields", "event", "time_event", "destroy"):
        assert callable(getattr(cls, method))
    assert issubclass(cls, gfship.ParticulateSource)      # event, time_event and destroy are the shared calls
    assert cls.set_fields is not gfship.ParticulateSource.set_fields
