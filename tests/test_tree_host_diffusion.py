"""Host check of the diffusion relax plans (gfship_tree_host_check_diffusion): for every level of a tree the
relax loop of diffusion_relax (src/poisson.c:1455-1484) runs on the host as the reference's program with the
coefficients of gfs_diffusion_coefficients computed as the reference computes them, through the plan of the
whole loop with the weight classes of the faces, and through its flow plan with the kernel's timing.  The
values must agree bit for bit, the flow plans must be free of hazards and exist on every level."""
import os
import subprocess
import sys

import pytest

import gfship
from test_tree_host import CASES

OCTREES = [c for c in CASES if c[1].get("dim") == 3]
QUADTREES = [c for c in CASES if c[1].get("dim", 2) == 2]
# beta dt nu of a step: (w + w) + w is not 3 w exactly for this w -- the intermediate sums of the coarse sides and
# of face_coeff_from_below round -- and yet the quarters sum back to w (so do four equal children: DESIGN.md 11.11)
W = 1e-3 / 3


def _check(kw, w=W):
    kw = dict(kw)
    dim = kw.pop("dim", 2)
    return gfship.tree_host_check_diffusion(kw["refine"], w, dim=dim, sides=kw.get("sides"),
                                            nrelax=kw.get("nrelax", 4))


def test_the_sums_of_the_coefficients_round_on_the_way():
    from fractions import Fraction
    assert Fraction((W + W) + W) != 3 * Fraction(W)
    q = W / 4
    assert ((0. + q + q) + q) + q == W


def test_four_equal_addends_sum_exactly():
    """what diffusion_weights_exact (csrc/tree_plan.hip) rests on: 0 + x + x + x + x is 4 x for every x"""
    import random
    rnd = random.Random(7)
    for _ in range(100000):
        w = rnd.uniform(0.5, 1.) * 2. ** rnd.randint(-40, 10)
        q = w / 4
        assert ((0. + q + q) + q) + q == w
        assert ((((0. + w) + w) + w) + w) / 4 == w


@pytest.mark.parametrize("name,kw", OCTREES, ids=[c[0] for c in OCTREES])
def test_diffusion_plans_of_an_octree(name, kw):
    updates, levels, not_w, differ, hazards, no_flow = _check(kw)
    assert updates > 0 and levels > 0
    assert differ == 0, "%d values or coefficients differ" % differ
    assert hazards == 0 and no_flow == 0
    assert not_w == 0      # every coefficient the stencils read is exactly w


@pytest.mark.parametrize("width", [64, 192])
def test_diffusion_flow_plans_of_other_widths(width):
    name, kw = OCTREES[0]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GFSHIP_FLOW_WIDTH=str(width))
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "gerris-fft-particles_amd"),
                                         os.path.join(root, "tests"), env.get("PYTHONPATH", "")])
    code = ("import test_tree_host_diffusion as t\n"
            "s = t._check(t.OCTREES[0][1])\n"
            "assert s[3] == 0 and s[4] == 0 and s[5] == 0, s\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.join(root, "tests"))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


@pytest.mark.parametrize("name,kw", QUADTREES, ids=[c[0] for c in QUADTREES])
def test_diffusion_plans_of_a_quadtree_agree_with_the_poisson_plans(name, kw):
    updates, levels, not_w, differ, hazards, no_flow = _check(kw)
    assert differ == 0 and hazards == 0 and not_w == 0
    k = dict(kw)
    dim = k.pop("dim", 2)
    p = gfship.tree_host_check(k["refine"], dim=dim, sides=k.get("sides"), nrelax=k.get("nrelax", 4))
    assert updates == p[0] and levels == p[2]
