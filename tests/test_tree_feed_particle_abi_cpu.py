"""GfsFeedParticle on a list of a tree without a device: the entry points are declared in include/gfship.h,
exported by the library and bound by the Python mirror."""
import inspect
import os
import re

import gfship
from conftest import ROOT

ENTRIES = ("gfship_tree_feed_particle_create", "gfship_tree_particles_set_idlast", "gfship_tree_particles_idlast")


def test_entries_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gfship.h")).read(), flags=re.S)
    L = gfship.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert name in gfship.SIGNATURES and getattr(L, name).restype is gfship.SIGNATURES[name][0]
    assert re.search(r"int\s+gfship_tree_feed_particle_create\s*\(gfship_feed_particle \*\* feed, gfship_particles \* pl,\s*"
                     r"const char \* mass, const char \* volume,\s*"
                     r"int nvars, const char \* const \* names, const int \* vars\s*\);", text)
    assert re.search(r"int\s+gfship_tree_particles_set_idlast\s*\(gfship_particles \* pl, int idlast\s*\);", text)
    assert re.search(r"int\s+gfship_tree_particles_idlast\s*\(gfship_particles \* pl\s*\);", text)
    # the arguments of the tree's create are those of the box's, with numbers of variables for the handles of fields
    assert len(gfship.SIGNATURES["gfship_tree_feed_particle_create"][1]) == \
        len(gfship.SIGNATURES["gfship_feed_particle_create"][1])


def test_the_python_mirror():
    assert issubclass(gfship.TreeFeedParticle, gfship.FeedParticle)
    assert list(inspect.signature(gfship.TreeFeedParticle.__init__).parameters) == \
        ["self", "tree", "plist", "mass", "volume", "variables"]
    # event and close are inherited: one event call for both kinds of handle
    assert gfship.TreeFeedParticle.event is gfship.FeedParticle.event
    assert gfship.TreeFeedParticle.close is gfship.FeedParticle.close
    assert callable(gfship.Tree.idlast) and callable(gfship.Tree.set_idlast)
    assert list(inspect.signature(gfship.Tree.set_idlast).parameters) == ["self", "pl", "value"]
    # the property of a list stays the call of a box
    assert isinstance(gfship.ParticleList.idlast, property)
