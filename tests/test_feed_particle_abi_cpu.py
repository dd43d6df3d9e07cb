"""GfsFeedParticle without a device: the entry points are declared in include/gfship.h, exported by the library
and bound by the Python mirror; the front end reads tests/cases/feed.gfs and refuses every malformed variant
with the reference's message and the line it is on (`--check')."""
import os
import re
import subprocess

import pytest

import gfship
from conftest import ROOT

ENTRIES = ("gfship_feed_particle_create", "gfship_feed_particle_event", "gfship_particles_set_idlast",
           "gfship_particles_idlast")
BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin", "gfship2D")
CASE = os.path.join(ROOT, "tests", "cases", "feed.gfs")
LEVEL, NSTEPS = 3, 3


def test_entries_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gfship.h")).read(), flags=re.S)
    L = gfship.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(L, name), name
        assert name in gfship.SIGNATURES and getattr(L, name).restype is gfship.SIGNATURES[name][0]
    assert re.search(r"\bvoid\s+gfship_feed_particle_destroy\s*\(", text)
    assert hasattr(L, "gfship_feed_particle_destroy") and "gfship_feed_particle_destroy" in gfship.SIGNATURES
    assert re.search(r"typedef\s+struct\s+gfship_feed_particle\s+gfship_feed_particle\s*;", text)
    assert re.search(r"int\s+gfship_feed_particle_event\s*\(gfship_feed_particle \* feed, int np, const double \* pos\s*\);",
                     text)
    for method in ("event", "close"):
        assert callable(getattr(gfship.FeedParticle, method))
    assert isinstance(gfship.ParticleList.idlast, property) and gfship.ParticleList.idlast.fset is not None


def _check(text, tmp_path, prog=BIN):
    f = tmp_path / "case.gfs"
    f.write_text(text)
    return subprocess.run([prog, "--check", "-DLEVEL=%d" % LEVEL, "-DNSTEPS=%d" % NSTEPS, str(f)],
                          capture_output=True, text=True, timeout=60)


def test_check_accepts_the_feed_case(tmp_path):
    r = _check(open(CASE).read(), tmp_path)
    assert r.returncode == 0, r.stderr
    ev = [l.split()[1] for l in r.stdout.splitlines() if l.startswith("event ")]
    assert ev == ["ParticleList", "FeedParticle"]      # the events run in the order of the file
    assert re.search(r"event FeedParticle line \d+ start 0 step -1 istep 1 ", r.stdout)
    # every keyword is optional (gfs_feed_particle_init), and so are the event parameters
    text = re.sub(r"GfsFeedParticle \{ istep = 1 \} drops \{.*?\n  \}\n", "GfsFeedParticle drops {\n  }\n",
                  open(CASE).read(), flags=re.S)
    assert "xfeed" not in text
    r = _check(text, tmp_path)
    assert r.returncode == 0, r.stderr


def _line_of(text, needle):
    return 1 + text[:text.index(needle)].count("\n")


FEED = "  GfsFeedParticle {"
TRACERS = "  GfsParticleList *dust { istep = 1 } {\n    GfsParticle 1 0.1 0.2 0\n  }\n"


@pytest.mark.parametrize("old,new,message,where", [
    # the messages of gfs_feed_particle_read (:2435-2575), each on the line of the token it is about
    ("} drops {", "} rain {", "unknown object 'rain'", FEED),
    ("} drops {", "} U {", "object 'U' is not a GfsParticleList", FEED),
    ("GfsFeedParticle { istep = 1 } drops {", "GfsFeedParticle { istep = 1 } {", "expecting a string (object name)", FEED),
    ("GfsFeedParticle { istep = 1 } drops {", "GfsFeedParticle { istep = 1 } drops 5 {", "expecting an opening brace", FEED),
    ("    nparts = 5", "    = 5", "expecting a keyword", "    = 5"),
    ("    zfeed = 0", "    zfeed 0", "expecting '='", "    zfeed 0"),
    ("    zfeed = 0", "    wfeed = 0", "unknown keyword `wfeed'", "    wfeed = 0"),
    # a list of GfsParticle, refused as GfsSourceParticulateVol refuses it
    ("  GfsFeedParticle { istep = 1 } drops", TRACERS + "  GfsFeedParticle { istep = 1 } dust",
     "the list `dust' holds GfsParticle objects: GfsFeedParticle needs GfsParticulate objects", FEED),
])
def test_malformed_variants_are_refused_with_their_line(tmp_path, old, new, message, where):
    text = open(CASE).read()
    assert text.count(old) >= 1
    bad = text.replace(old, new, 1)
    r = _check(bad, tmp_path)
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert r.stderr.startswith("gfship: ") and r.stderr.count("\n") == 1, r.stderr
    assert re.search(r":%d: " % _line_of(bad, where), r.stderr), (_line_of(bad, where), r.stderr)


@pytest.mark.parametrize("keyword", ["nparts", "xfeed", "yfeed", "zfeed"])
def test_a_variable_in_a_function_without_a_cell_is_refused(tmp_path, keyword):
    """nparts and the positions are evaluated with the cell NULL (:2381-2383, :2411): the reference would read
    the variable there"""
    text = open(CASE).read()
    bad, n = re.subn(r"    %s = (.*)\n" % keyword, "    %s = (T > 0.)\n" % keyword, text)
    assert n == 1
    r = _check(bad, tmp_path)
    assert r.returncode != 0
    assert "`%s' of GfsFeedParticle is evaluated without a cell: it cannot read the variable `T'" % keyword in r.stderr, r.stderr
    assert re.search(r":%d: " % _line_of(bad, "    %s = (T > 0.)" % keyword), r.stderr), r.stderr


def test_a_variable_of_the_host_in_the_mass_is_refused(tmp_path):
    """a variable that GfsInit alone makes lives on the host: mass and volume run on the device"""
    text = open(CASE).read()
    bad = text.replace("    T = (x + 0.25*y)\n", "    T = (x + 0.25*y)\n    Host = 1\n").replace("1e-3*T :", "1e-3*Host*T :")
    r = _check(bad, tmp_path)
    assert r.returncode != 0 and "`mass' of GfsFeedParticle reads `Host', which is not kept on the device" in r.stderr, r.stderr
    assert re.search(r":%d: " % _line_of(bad, "    mass = "), r.stderr), r.stderr


def test_refused_on_a_refined_tree(tmp_path):
    text = open(CASE).read().replace("Refine LEVEL", "Refine (x > 0 ? 4 : 3)")
    r = _check(text, tmp_path)
    assert r.returncode != 0
    assert "gfship: line %d: GfsFeedParticle is not supported on a refined tree" % _line_of(text, FEED) in r.stderr, r.stderr


@pytest.mark.parametrize("idlast", ["", " 40", " 0"])
def test_a_particle_list_with_and_without_idlast_parses(tmp_path, idlast):
    text = open(CASE).read()
    assert text.count("  } 40\n") == 1
    r = _check(text.replace("  } 40\n", "  }%s\n" % idlast), tmp_path)
    assert r.returncode == 0, r.stderr
    # ... on a tree of tracers as well
    tree = ("1 2 GfsSimulation GfsBox GfsGEdge {} {\n  Time { iend = 1 }\n  Refine (x > 0 ? 4 : 3)\n"
            "  GModule particulates\n" + TRACERS.replace("  }\n", "  }%s\n" % idlast) + "}\nGfsBox {}\n1 1 right\n1 1 top\n")
    r = _check(tree, tmp_path)
    assert r.returncode == 0, r.stderr
