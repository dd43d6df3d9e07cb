"""Viscous refined octrees beyond the oracle: the refined channel run to its steady state against the analytic
parabola, with the tolerance taken from the same channel on a quadtree refined the same way in x-y; and
tests/cases/refined_cavity_3d.gfs through gfship3D against the octree oracle set up by hand."""
import math
import os
import subprocess

import numpy as np
import pytest

import gfship
from oracle import oracle as O
from test_gpu_tree import _bc_values

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN3 = os.path.join(ROOT, "gerris-fft-particles_amd", "bin", "gfship3D")
CASES = os.path.join(ROOT, "tests", "cases")

NU, G, T_END = 1., 1., 1.5


def _steady_channel_error(dim):
    """the channel periodic in x (and z), Dirichlet U = 0 on the walls y = -1/2, 1/2, GfsSource U G, implicit
    viscosity NU with beta = 1, level 3 with one level more along the lower wall, run to t = T_END (15
    diffusion times 1/(pi^2 NU)): the largest difference of U from G/(2 NU) (1/4 - y^2) on the leaves, and
    the largest |V|, |W|"""
    P, B = gfship.SIDE_PERIODIC, gfship.SIDE_BOUNDARY
    if dim == 2:
        refine = lambda x, y: 4 if y < -0.3 else 3
        sides = [P, P, B, B]
    else:
        refine = lambda x, y, z: 4 if y < -0.3 else 3
        sides = [P, P, B, B, P, P]
    o = O.Tree(refine=refine, dim=dim, sides=sides)
    for d in (2, 3):
        o.set_bc_u(0, d, O.BC_DIRICHLET, 0.)
    vals = _bc_values(o, 0, None)
    o.destroy()
    g = gfship.Tree(refine, dim=dim, sides=sides)
    for d in (2, 3):
        g.set_bc_u(0, d, gfship.BC_DIRICHLET, vals)
    for c in range(dim):
        g.set_viscosity(c, NU)
        g.diffusion_params(c).beta = 1.
    g.set_source(0, G)
    g.set_time(T_END, 0.8)
    g.start()
    k = 0
    while g.t < T_END and k < 5000:
        g.step()
        k += 1
    assert g.t >= T_END, (g.t, k)
    inner = (slice(1, -1),) * dim
    err = other = 0.
    for l in range(g.depth + 1):
        leaf = g.flags(l)[inner] == 1
        if not leaf.any():
            continue
        y = g.centres(l)[1][inner][leaf]
        u = g.download(gfship.Tree.U, l)[inner][leaf]
        err = max(err, float(np.abs(u - G / (2. * NU) * (0.25 - y * y)).max()))
        for c in (gfship.Tree.V,) + ((gfship.Tree.W,) if dim == 3 else ()):
            other = max(other, float(np.abs(g.download(c, l)[inner][leaf]).max()))
    g.destroy()
    return err, other


def test_refined_octree_channel_reaches_the_parabola():
    """The octree channel does not depend on x or z: its discrete steady problem is the quadtree's (the same
    cells in x-y, and the interpolations across the coarse-fine faces in the plane of a face only average values
    that are equal), so its error from the parabola is the quadtree's error up to the solvers' tolerances.  The
    factor 1.05 leaves room for those; the quadtree's error itself must be the small O(h^2) one of the
    coarse-fine stencils (u_max = 1/8)."""
    e2, o2 = _steady_channel_error(2)
    e3, o3 = _steady_channel_error(3)
    print("max error from the parabola: quadtree %.3e, octree %.3e; |V|, |W| %.1e, %.1e" % (e2, e3, o2, o3))
    assert e2 < 0.02 * G / (8. * NU)
    assert e3 <= 1.05 * e2
    assert o3 < 1e-6


def _run3d(case, defs):
    cmd = [BIN3] + ["-D%s=%s" % kv for kv in defs.items()] + [os.path.join(CASES, case)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_refined_cavity_3d_case_matches_the_tree_oracle():
    """tests/cases/refined_cavity_3d.gfs (a lid-driven cube on an octree refined near the walls: BcDirichlet on
    U, V, W on six sides, GfsSourceDiffusion) through gfship3D against the octree oracle after NSTEPS steps: the
    volume-weighted norms OutputScalarNorm prints, to the printed digits, and the time"""
    level, nsteps = 3, 8
    out = _run3d("refined_cavity_3d.gfs", {"LEVEL": level, "NSTEPS": nsteps})
    refine = lambda x, y, z: level + 1 if max(abs(x), abs(y), abs(z)) > 0.25 else level
    s = O.Tree(refine=refine, dim=3, sides=[O.SIDE_BOUNDARY] * 6)
    for c in range(3):
        for d in range(6):
            s.set_bc_u(c, d, O.BC_DIRICHLET, 1. if (c == 0 and d == 2) else 0.)
        s.set_viscosity(c, 1e-3)
    s.set_time(300., 0.8)
    s.start()
    for _ in range(nsteps):
        s.step()
    lines = out.splitlines()
    inner = (slice(1, -1),) * 3
    for name, which in (("U", O.Tree.U), ("V", O.Tree.V), ("W", O.Tree.W), ("P", O.Tree.P)):
        first = second = wsum = 0.
        infty = 0.
        for l in range(s.depth + 1):
            leaf = s.flags(l)[inner] == 1
            if not leaf.any():
                continue
            a = np.abs(s.values(which, l)[inner][leaf])
            w = 1. / (1 << l) ** 3
            first += w * float(a.sum())
            second += w * float((a * a).sum())
            wsum += w * a.size
            infty = max(infty, float(a.max()))
        want = "%s time: %g first: % 10.3e second: % 10.3e infty: % 10.3e" % (
            name, s.t, first / wsum, math.sqrt(second / wsum), infty)
        assert want in lines, (want, [l for l in lines if l.startswith(name + " time")])
    assert "%g" % s.t in out
    s.destroy()
