"""Particulates on a tree: the entry point and the variables Un, Vn, Wn are declared, exported and bound, and a
null handle is an error (no device needed)."""
import ctypes as C
import os
import re

import gfship
from conftest import ROOT

NAME = "gfship_particulates_create_tree"
EINVAL = -1


def header():
    return open(os.path.join(ROOT, "include", "gfship.h")).read()


def test_symbol_is_declared_exported_and_bound():
    assert re.search(r"\b%s\s*\(" % NAME, re.sub(r"/\*.*?\*/", "", header(), flags=re.S))
    assert hasattr(gfship.lib(), NAME)
    assert NAME in gfship.SIGNATURES
    assert callable(gfship.Tree.particulates)


def test_previous_velocity_variables_are_appended_to_the_enum():
    """GFSHIP_TREE_UPREV, _VPREV, _WPREV come last: no number of an existing variable moves"""
    m = re.search(r"enum \{ (GFSHIP_TREE_P = 0,.*?)\};", header(), flags=re.S)
    names = [x.strip().split(" ")[0] for x in m.group(1).split(",")]
    assert names[-3:] == ["GFSHIP_TREE_UPREV", "GFSHIP_TREE_VPREV", "GFSHIP_TREE_WPREV"]
    assert names.index("GFSHIP_TREE_BCW") == gfship.Tree.BCW == 24
    assert (gfship.Tree.UPREV, gfship.Tree.VPREV, gfship.Tree.WPREV) == tuple(names.index(n) for n in names[-3:])
    for n in names[:-3]:
        assert getattr(gfship.Tree, n[len("GFSHIP_TREE_"):]) == names.index(n)


def test_null_handles_are_einval():
    L = gfship.lib()
    p = C.c_void_p(1)
    one = (C.c_double * 3)(0., 0., 0.)
    ids = (C.c_uint * 1)(1)
    assert L.gfship_particulates_create_tree(C.byref(p), None, 1, one, ids, one, one, one) == EINVAL
    assert not p.value
    assert L.gfship_particulates_create_tree(None, None, 0, None, None, None, None, None) == EINVAL
    assert L.gfship_tree_download(None, gfship.Tree.UPREV, 0, one) == EINVAL
