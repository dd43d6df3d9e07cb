"""Droplets on refined trees without a device: the entry points are declared in include/gfship.h, exported by the
library and bound by the Python mirror, and the refusals that need no device are made."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import gfship
from conftest import ROOT

ENTRIES = ("gfship_tree_tag_droplets", "gfship_tree_tag_droplets_time", "gfship_tree_remove_droplets",
           "gfship_tree_droplet_to_particle_create", "gfship_tree_host_tag_droplets")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gfship.h")).read(), flags=re.S)


def test_entries_are_declared_exported_and_bound():
    text = _header()
    L = gfship.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert name in gfship.SIGNATURES and getattr(L, name).restype is gfship.SIGNATURES[name][0]
    assert re.search(r"int\s+gfship_tree_tag_droplets\s*\(gfship_tree \* tree, int c_var, unsigned \* n\s*\);", text)
    assert re.search(r"int\s+gfship_tree_tag_droplets_time\s*\(gfship_tree \* tree, int c_var, int reps, double \* ms\s*\);",
                     text)
    assert re.search(r"int\s+gfship_tree_remove_droplets\s*\(gfship_tree \* tree, int c_var, int v_var, int min, "
                     r"double val\s*\);", text)
    assert re.search(r"int\s+gfship_tree_droplet_to_particle_create\s*\(gfship_droplet_to_particle \*\* d, "
                     r"gfship_particles \* pl, int c_var,\s*int min, double reset, double density, "
                     r"const char \* function,\s*int nvars, const char \* const \* names, const int \* vars\s*\);", text)
    # the arguments of the tree's create are those of the box's, with numbers of variables for the handles of fields
    assert len(gfship.SIGNATURES["gfship_tree_droplet_to_particle_create"][1]) == \
        len(gfship.SIGNATURES["gfship_droplet_to_particle_create"][1])


def test_the_tag_variable_follows_the_variables_of_the_sources():
    text = _header()
    assert re.search(r"enum\s*\{\s*GFSHIP_TREE_TAG\s*=\s*GFSHIP_TREE_DMDT\s*\+\s*1\s*\}", text)
    assert gfship.Tree.TAG == gfship.Tree.DMDT + 1 == gfship.TREE_TAG == 38


def test_the_python_mirror():
    assert issubclass(gfship.TreeDropletToParticle, gfship.DropletToParticle)
    assert list(inspect.signature(gfship.TreeDropletToParticle.__init__).parameters) == \
        ["self", "tree", "plist", "c", "min", "reset", "density", "function", "variables"]
    # event and close are inherited: one event call for both kinds of handle
    assert gfship.TreeDropletToParticle.event is gfship.DropletToParticle.event
    assert gfship.TreeDropletToParticle.close is gfship.DropletToParticle.close
    assert list(inspect.signature(gfship.Tree.tag_droplets).parameters) == ["self", "c"]
    assert list(inspect.signature(gfship.Tree.remove_droplets).parameters) == ["self", "c", "v", "min", "val"]
    assert list(inspect.signature(gfship.Tree.time_tag_droplets).parameters) == ["self", "c", "reps"]


def test_refusals_that_need_no_device():
    L = gfship.lib()
    n = ctypes.c_uint(7)
    ms = ctypes.c_double(0.)
    p = ctypes.c_void_p()
    assert L.gfship_tree_tag_droplets(None, gfship.Tree.T0, ctypes.byref(n)) == -1
    assert L.gfship_tree_tag_droplets_time(None, gfship.Tree.T0, 3, ctypes.byref(ms)) == -1
    assert L.gfship_tree_remove_droplets(None, gfship.Tree.T0, gfship.Tree.T0, 3, 0.) == -1
    assert L.gfship_tree_droplet_to_particle_create(None, None, gfship.Tree.T0, 3, 0., 1., None, 0, None, None) == -1
    assert L.gfship_tree_droplet_to_particle_create(ctypes.byref(p), None, gfship.Tree.T0, 3, 0., 1., None, 0, None,
                                                    None) == -1
    assert p.value is None
    assert L.gfship_droplet_to_particle_event(None, None) == -1
    L.gfship_droplet_to_particle_destroy(None)
    # the host planner: a mask of the wrong size
    with pytest.raises(gfship.GfshipError, match="gfship error -1.*cells"):
        gfship.tree_host_tag_droplets(lambda x, y: 2, [np.zeros(3)], 16)
