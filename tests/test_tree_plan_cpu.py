"""The planner of refined trees (csrc/tree_plan.hip) is plain host code with no shared state.

Digests: gfship_tree_host_plan_digest hashes (FNV-1a-64, the members of every element, each array preceded by its
length) every array a device tree uploads -- [0] flags, tables and the lists of leaves, non-leaf cells and ghost
leaves, [1] the sweep plans, [2] the loop plans of nrelax sweeps, [3] their flow plans, [4] the face sets.  The
constants below were taken from the commit before the planner was separated from tree.hip, with the same hash
applied to the same arrays at the points where that commit uploaded them: no plan moved by a bit.

Threads: two host checks at the same time return what each returns alone (they used to share a host-only flag that
the first check to finish cleared under the other)."""
import os
import subprocess
import sys
import threading

import pytest

import gfship
from test_tree_host import CASES, MANY_SWEEPS_TREES

DIGESTS = {
    "quadtree, two extra levels in the square":
        (0x847c25656b91a467, 0x71480367f091b694, 0xa764cc3961d1349b, 0x44461139b6c37b00, 0x508405c9f52d452b),
    "quadtree, one extra level, 3 sweeps":
        (0x23176b0ca59cfdc5, 0x6e0b1c20188ee266, 0x3c10695c31477441, 0x611af72a92c4d93a, 0x8c8bd71f7d3f8bc8),
    "uniform quadtree":
        (0x15e1666b278b799b, 0xcd5a2bcd50cc15db, 0x486f01b61835026d, 0x63317df1bb02cf66, 0x1e5f9c41ffbf0519),
    "octree, off-centre ball with two extra levels":
        (0x53c90f313aca68c6, 0x2dee2755a2d2e90f, 0xce6ff36281f2d353, 0x18ac3ccd467c917c, 0x93a63775b4bb8382),
    "octree, cube with one extra level":
        (0xa6a45984df802011, 0xef3b49c876ec77a5, 0x0555a7d229e3c0d8, 0xeae067d12ae3f2d7, 0xd1e9026b9a8b7e9a),
    "quadtree with GfsBoundary sides, circle with two extra levels":
        (0x2de5c8ebf6c00e04, 0xbbc49366a66def12, 0x86d2ef0e8dee4df3, 0x1fe3a1c48c98c88a, 0x778095f083e3584b),
    "octree with GfsBoundary sides":
        (0x5c48e8c29801fd74, 0xd3f35e46e583526f, 0x3d9630dbd9235052, 0xfcaa55e5ea8441f0, 0xd645e6262a8555ce),
}

# (tree of MANY_SWEEPS_TREES, sweeps): the topology, the sweep plans and the face sets are those of the tree
DIGESTS_MANY = {
    ("quadtree 4/6", 8):
        (0x847c25656b91a467, 0x71480367f091b694, 0xa3ceac9d5adccde8, 0xf6547992480bf001, 0x508405c9f52d452b),
    ("quadtree 4/6", 40):
        (0x847c25656b91a467, 0x71480367f091b694, 0x5fc940aa13c30795, 0x2f1fa644085708fc, 0x508405c9f52d452b),
    ("octree 3/4", 8):
        (0xa6a45984df802011, 0xef3b49c876ec77a5, 0x8e4ffef638a55d0d, 0x0c035a8c9c565e5f, 0xd1e9026b9a8b7e9a),
    ("octree 3/4", 40):
        (0xa6a45984df802011, 0xef3b49c876ec77a5, 0x23ed2a53bde75ff9, 0xd46ad116b60cb194, 0xd1e9026b9a8b7e9a),
    ("quadtree with GfsBoundary sides", 8):
        (0x2de5c8ebf6c00e04, 0xbbc49366a66def12, 0xcd5dc8c7baa2e361, 0x5de4d05a950ad062, 0x778095f083e3584b),
    ("quadtree with GfsBoundary sides", 40):
        (0x2de5c8ebf6c00e04, 0xbbc49366a66def12, 0xa60597dac7ad76c7, 0xc2f0aca9bea52e20, 0x778095f083e3584b),
}

# GFSHIP_FLOW_WIDTH -> (quadtree 4/6, octree 3/4), 4 sweeps: only the flow plans depend on the width
DIGESTS_WIDTH = {
    64: ((0x847c25656b91a467, 0x71480367f091b694, 0xa764cc3961d1349b, 0x8a3ac69a51a6f173, 0x508405c9f52d452b),
         (0xa6a45984df802011, 0xef3b49c876ec77a5, 0x0555a7d229e3c0d8, 0x4c1aa66ff287126e, 0xd1e9026b9a8b7e9a)),
    192: ((0x847c25656b91a467, 0x71480367f091b694, 0xa764cc3961d1349b, 0xae41623b79ed9423, 0x508405c9f52d452b),
          (0xa6a45984df802011, 0xef3b49c876ec77a5, 0x0555a7d229e3c0d8, 0xcaace480f9df2f81, 0xd1e9026b9a8b7e9a)),
}


def _digest(kw, nrelax=None):
    k = dict(kw)
    return gfship.tree_host_plan_digest(k["refine"], dim=k.get("dim", 2), sides=k.get("sides"),
                                        nrelax=nrelax or k.get("nrelax", 4))


def _hex(d):
    return tuple("%#018x" % v for v in d)


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_plans_are_those_of_the_commit_before_the_split(name, kw):
    assert _hex(_digest(kw)) == _hex(DIGESTS[name])


@pytest.mark.parametrize("nrelax", [8, 40])
@pytest.mark.parametrize("name,kw", MANY_SWEEPS_TREES, ids=[c[0] for c in MANY_SWEEPS_TREES])
def test_plans_of_many_sweeps_are_those_of_the_commit_before_the_split(name, kw, nrelax):
    assert _hex(_digest(kw, nrelax)) == _hex(DIGESTS_MANY[name, nrelax])


@pytest.mark.parametrize("width", [64, 192])
def test_narrow_flow_plans_are_those_of_the_commit_before_the_split(width):
    """GFSHIP_FLOW_WIDTH is looked up when the plans are made: a child process per width"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import gfship\n"
            "inside = lambda *a: all(-0.25 <= v <= 0.25 for v in a)\n"
            "print(*gfship.tree_host_plan_digest(lambda x, y: 6 if inside(x, y) else 4))\n"
            "print(*gfship.tree_host_plan_digest(lambda x, y, z: 4 if inside(x, y, z) else 3, dim=3))\n")
    env = dict(os.environ)
    env["GFSHIP_FLOW_WIDTH"] = str(width)
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(root, "gerris-fft-particles_amd"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert [_hex(d) for d in got] == [_hex(d) for d in DIGESTS_WIDTH[width]]


def test_two_host_checks_at_the_same_time():
    trees = [dict(MANY_SWEEPS_TREES[0][1]), dict(MANY_SWEEPS_TREES[1][1])]      # quadtree 4/6, octree 3/4
    alone = [gfship.tree_host_check(**kw) for kw in trees]
    for updates, levels_sweeps, levels_loop, differ in alone:
        assert updates > 0 and levels_sweeps > 0 and levels_loop > 0 and differ == 0
    together = [None, None]

    def run(i):
        try:
            together[i] = gfship.tree_host_check(**trees[i])
        except Exception as e:      # reported by the comparison below
            together[i] = e

    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert together == alone
