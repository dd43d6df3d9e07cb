"""GfsSourceDiffusion on refined octrees: the device against the octree oracle (oracle/go_tree.c), bit for
bit, on every leaf after every step, with the diffusion solvers' iteration counts and residuals.  Every
relax implementation of the tree (the switches of test_gpu_tree.py::test_other_relax_kernels_give_the_same_bits)
gives the same bits, each in a subprocess."""
import os
import subprocess
import sys

import pytest

import gfship
from oracle import oracle as O
from test_gpu_tree import _bc_values, _same_leaves

pytestmark = pytest.mark.gpu

ball = lambda x, y, z: (x - 0.1) ** 2 + (y + 0.05) ** 2 + z * z < 0.04
cube = lambda x, y, z: max(abs(x), abs(y), abs(z)) <= 0.25


def _pair(kind):
    """(oracle tree, device tree) of one case, viscosity set"""
    sides = None
    if kind == "taylor-green":      # periodic, a refined cube and a refined off-centre ball, two extra levels
        refine = lambda x, y, z: 5 if ball(x, y, z) else 4 if cube(x, y, z) else 3
    elif kind == "lid":             # lid-driven cube: six walls, Dirichlet U, V, W, the walls refined
        refine = lambda x, y, z: 4 if max(abs(x), abs(y), abs(z)) > 0.3 else 3
        sides = [gfship.SIDE_BOUNDARY] * 6
    else:                           # channel: periodic in x and z, walls in y refined along the lower wall
        refine = lambda x, y, z: 4 if y < -0.3 else 3
        sides = [gfship.SIDE_PERIODIC, gfship.SIDE_PERIODIC, gfship.SIDE_BOUNDARY, gfship.SIDE_BOUNDARY,
                 gfship.SIDE_PERIODIC, gfship.SIDE_PERIODIC]
    if sides is None:
        o = O.Tree(refine=refine, dim=3)
        g = gfship.Tree(refine, dim=3)
    else:
        o = O.Tree(refine=refine, dim=3, sides=sides)
        g = gfship.Tree(refine, dim=3, sides=sides)
    nu = 2e-3
    for c in range(3):
        if kind == "lid":
            for d in range(6):
                o.set_bc_u(c, d, O.BC_DIRICHLET, 1. if (c == 0 and d == 2) else 0.)
        elif kind == "channel":
            for d in (2, 3):
                o.set_bc_u(c, d, O.BC_DIRICHLET, 0.)
        o.set_viscosity(c, nu)
        g.set_viscosity(c, nu)
        if kind in ("lid", "channel"):
            vals = _bc_values(o, c, None)
            for d in (range(6) if kind == "lid" else (2, 3)):
                g.set_bc_u(c, d, gfship.BC_DIRICHLET, vals)
    if kind == "taylor-green":
        from flow_cases import taylor_green_3d
        for l in range(o.depth + 1):
            x, y, z = o.centres(l)
            for which, arr in zip((O.Tree.U, O.Tree.V, O.Tree.W), taylor_green_3d(x, y, z)):
                o.values(which, l)[...] = arr
        G = gfship.Tree
        for l in range(o.depth + 1):
            for gv, ov in ((G.U, O.Tree.U), (G.V, O.Tree.V), (G.W, O.Tree.W)):
                g.upload(gv, l, o.values(ov, l))
    if kind == "channel":      # test/poiseuille's set-up: beta = 1 (backward Euler)
        o.set_source(0, 1.)
        g.set_source(0, 1.)
        for c in range(3):
            o.diffusion_params(c).beta = 1.
            g.diffusion_params(c).beta = 1.
    o.set_time(300., 0.8)
    g.set_time(300., 0.8)
    return o, g


def run_case(kind, nsteps=5):
    o, g = _pair(kind)
    T, G = O.Tree, gfship.Tree
    names = [(G.U, T.U), (G.V, T.V), (G.W, T.W), (G.P, T.P), (G.PMAC, T.PMAC)]
    o.start()
    g.start()
    assert g.dt == o.dt
    for k in range(nsteps):
        o.step()
        g.step()
        assert g.t == o.t and g.dt == o.dt, k
        _same_leaves(o, g, names, "%s step %d" % (kind, k))
        for c in range(3):
            pg, po = g.diffusion_params(c), o.diffusion_params(c)
            assert pg.niter == po.niter and pg.residual.infty == po.residual.infty, (kind, k, c)
        # the solves ran (a component at rest, W of the channel, needs no iteration)
        assert max(o.diffusion_params(c).niter for c in range(3)) >= 1
    o.destroy()
    g.destroy()


KINDS = ["taylor-green", "lid", "channel"]


@pytest.mark.parametrize("kind", KINDS)
def test_viscous_refined_octree_bit_exact(kind):
    run_case(kind)


SWITCHES = ["GFSHIP_TREE_TEMPLATE_RELAX=1", "GFSHIP_TREE_NO_PIPELINE=1", "GFSHIP_TREE_NO_FLOW=1",
            "GFSHIP_TREE_NO_FLOW=1 GFSHIP_TREE_NO_PREFETCH=1", "GFSHIP_FLOW_WIDTH=128", "GFSHIP_FLOW_WIDTH=64",
            "GFSHIP_TREE_NO_RESIDUAL_TAPE=1"]


@pytest.mark.parametrize("switch", SWITCHES)
def test_viscous_octrees_through_every_relax_kernel(switch):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for kv in switch.split():
        k, v = kv.split("=")
        env[k] = v
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "gerris-fft-particles_amd"),
                                         os.path.join(root, "tests"), env.get("PYTHONPATH", "")])
    code = ("import test_gpu_tree_viscous_octree as t\n"
            "for k in t.KINDS: t.run_case(k, 3)\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600,
                       cwd=os.path.join(root, "tests"))
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
