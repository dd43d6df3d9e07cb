"""tests/cases/tree_tracers.gfs (a GfsParticleList of GfsParticle objects and a GfsOutputLocation on a refined
quadtree) through bin/gfship2D, against the same run driven through the Python mirror of the C ABI, text for text;
and the lists a refined tree does not take, refused with the line number before a tree exists."""
import os
import re
import subprocess

import numpy as np
import pytest

import gfship

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin", "gfship2D")
CASE = os.path.join(ROOT, "tests", "cases", "tree_tracers.gfs")
LEVEL, BOX, NSTEPS = 3, 1, 4


def case_lists():
    """the particles and the points of the case file, read from its text"""
    text = open(CASE).read()
    parts = [[float(x) for x in m.groups()] for m in
             re.finditer(r"^\s+GfsParticle (\d+) (\S+) (\S+) (\S+)\s*$", text, re.M)]
    ids = np.array([p[0] for p in parts], dtype=np.uint32)
    pos = np.array([p[1:] for p in parts])
    pts = np.array(re.search(r"OutputLocation \{[^}]*\} stdout \{([^}]*)\}", text).group(1).split(),
                   dtype=np.float64).reshape(-1, 3)
    return ids, pos, pts


def test_tree_tracers_case_equals_the_abi_run(tmp_path):
    outp = tmp_path / "particles.txt"
    r = subprocess.run([BIN, "--particles", str(outp), "-DLEVEL=%d" % LEVEL, "-DBOX=%d" % BOX,
                        "-DNSTEPS=%d" % NSTEPS, CASE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr

    ids, pos, pts = case_lists()
    assert len(ids) == 9 and len(pts) == 6
    g = gfship.Tree(lambda x, y: LEVEL if (x < -0.25 or x > 0.25 or y < -0.25 or y > 0.25) else LEVEL + BOX)
    for l in range(g.depth + 1):
        x, y = g.centres(l)
        g.upload(g.U, l, (0.8 + 0.4*y*(1. - 4.*x*x)))
        g.upload(g.V, l, (0.7 - 0.5*x*(1. - 4.*y*y)))
    for p in (g.projection_params, g.approx_projection_params):
        p.tolerance = 1e-6
    g.set_time(1.7976931348623157e308, 0.8)
    pl = g.particles(pos, ids)
    rows = ["# 1:t 2:x 3:y 4:z 5:P 6:Pmac 7:U 8:V"]

    def events():
        pl.event()
        cols = [g.interpolate(v, pts) for v in (g.P, g.PMAC, g.U, g.V)]
        for q in range(len(pts)):
            if cols[0][1][q]:
                rows.append(" ".join("%g" % x for x in [g.t] + list(pts[q]) + [c[0][q] for c in cols]))

    g.start()
    events()
    for _ in range(NSTEPS):
        g.step()
        events()
    p, i = pl.download()
    pl.destroy()
    g.destroy()

    got = [l for l in r.stdout.splitlines() if not l.startswith("step:")]
    assert got == rows
    assert len(rows) == 1 + (NSTEPS + 1)*5            # the point at x = 0.7 is outside
    expected = "GfsParticleList GfsParticle {\n" + "".join(
        "    GfsParticle %d %g %g %g\n" % (i[q], p[q][0], p[q][1], p[q][2]) for q in range(len(i))) + "}\n"
    assert open(outp).read() == expected
    assert 9 not in i and len(i) >= 5                  # the particle outside from the start left the list
    assert (p[:, 2] == 0.).all() and (np.abs(p[:, :2]) <= 0.5).all()


BAD_LISTS = {
    "particulate": "GfsParticleList { istep = 1 } GfsParticulate {\n    GfsParticulate 1 0.11 0.23 0 2e-3 1e-3 0 0 0\n  }",
    "force_drag": "GfsParticleList { istep = 1 } GfsParticulate {\n    GfsParticulate 1 0.11 0.23 0 2e-3 1e-3 0 0 0\n  } {\n"
                  "    GfsForceDrag\n  }",
}


@pytest.mark.parametrize("kind", list(BAD_LISTS))
def test_particulates_and_forces_are_refused_on_a_tree(tmp_path, kind):
    text = open(CASE).read()
    a = text.index("  GfsParticleList")
    b = text.index("  OutputLocation")
    bad = text[:a] + "  " + BAD_LISTS[kind] + "\n" + text[b:]
    line = bad[:bad.index("  GfsParticleList {")].count("\n") + 1      # (the comment at the top names the class too)
    path = tmp_path / "bad.gfs"
    path.write_text(bad)
    r = subprocess.run([BIN, "-DLEVEL=3", "-DBOX=1", "-DNSTEPS=1", str(path)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0
    assert "line %d:" % line in r.stderr and "not supported on a refined tree" in r.stderr
    assert r.stdout == ""                              # nothing ran: no tree, no event
