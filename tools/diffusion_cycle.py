"""Wall time of one V-cycle on one periodic box, same level, same nrelax, three cell updates:
  * gfship_diffusion_cycle with per-face coefficients and a variable density (RelaxOp kind 3),
  * gfship_diffusion_cycle with a constant coefficient (kind 1: the 2 x 2 ring kernels at 128^3 and more),
  * gfship_poisson_cycle with the face weights of a GfsFunction alpha (kind 2),
taken in turn, several rounds, each figure a host clock around `reps' cycles that end in a synchronise:
tools/diffusion_cycle.py [level] [rounds]"""
import os
import sys
import time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "gerris-fft-particles_amd"))
import numpy as np
import gfship
lev = int(sys.argv[1]) if len(sys.argv) > 1 else 7
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
n = 1 << lev
gd = gfship.Domain(3, lev, [gfship.SIDE_PERIODIC] * 6)
u, rhs, rhoc, res, dia, alpha_cell = (gd.variable() for _ in range(6))
rng = np.random.default_rng(0)
rhs.upload(rng.standard_normal((n + 2,) * 3))
for l in range(lev + 1):
    alpha_cell.upload(rng.uniform(0.5, 2., ((1 << l) + 2,) * 3), l)
par = gd.params()
par.depth = lev


def faces(lo, hi):
    out = []
    for c in range(3):
        a = rng.uniform(lo, hi, (n + 2,) * 3)
        sl0, sln = [slice(None)] * 3, [slice(None)] * 3
        sl0[2 - c], sln[2 - c] = 0, -2
        a[tuple(sl0)] = a[tuple(sln)]
        v = gd.variable()
        v.upload(a)
        out.append(v)
    return out


D, alpha = faces(0.5e-2, 1.5e-2), faces(0.5, 1.5)
dt, nrelax = 0.1, 4


def timed(cycle, reps=20):
    cycle()
    gd.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        cycle()
    gd.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def faces_cycle():
    gd.diffusion_coefficients_faces(D, dt, rhoc, alpha_cell, 1.)
    return timed(lambda: gd.diffusion_cycle(0, nrelax, u, rhs, rhoc, res))


def constant_cycle():
    gd.diffusion_coefficients(1e-2, dt, rhoc, 1.)
    return timed(lambda: gd.diffusion_cycle(0, nrelax, u, rhs, rhoc, res))


def weighted_cycle():
    gd.poisson_coefficients_alpha(alpha)
    return timed(lambda: gd.poisson_cycle(par, u, rhs, dia, res))


for r in range(rounds):
    print("level %d round %d  diffusion per face %.3f  diffusion constant %.3f  weighted Poisson %.3f  ms per cycle"
          % (lev, r, faces_cycle(), constant_cycle(), weighted_cycle()), flush=True)
