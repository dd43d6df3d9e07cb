#!/usr/bin/env python3
"""Config D probe: 2M tracers on the 256^3 Taylor-Green box, particle_list_event alone.
   python tools/particles_bench.py [--level 8] [--np 2000000] [--presort] [--repeats 3]
                                   [--particulates [--viscosity NU] [--fluid-fields]]
--particulates: the particles as GfsParticulate objects with the five forces, set up as bench.py --full
sets them up (no viscosity: the drag is inactive); --viscosity NU: a constant viscosity of U, V, W (the
drag acts); --fluid-fields: alpha at the cell centres (1/(1.5 + x)) and the viscosity at the leaf centres
(NU (1.5 + y), NU = 0.01 unless --viscosity gives it), which the forces then read at the cell of every
particle.  One line per repeat."""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "gerris-fft-particles_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import gfship
from bench import taylor_green, with_ghosts
from particle_cases import lcg_positions_fast

ap = argparse.ArgumentParser()
ap.add_argument("--level", type=int, default=8)
ap.add_argument("--np", type=int, default=2000000)
ap.add_argument("--presort", action="store_true")
ap.add_argument("--events", type=int, default=10)
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--particulates", action="store_true")
ap.add_argument("--viscosity", type=float, default=0.)
ap.add_argument("--fluid-fields", action="store_true")
a = ap.parse_args()
if (a.viscosity or a.fluid_fields) and not a.particulates:
    ap.error("--viscosity and --fluid-fields go with --particulates")
n = 1 << a.level
dom = gfship.Domain(3, a.level, [gfship.SIDE_PERIODIC] * 6)
sim = gfship.Simulation(dom)
for c, f in enumerate(taylor_green(n)):
    sim.u[c].upload(with_ghosts(f))
for c in range(3):
    if a.viscosity:
        sim.set_viscosity(c, a.viscosity)
sim.start(); sim.step()
pos, ids = lcg_positions_fast(a.np)
if a.presort:
    ijk = np.floor((pos + 0.5) * n).astype(np.int64)
    key = (ijk[:, 2] * n + ijk[:, 1]) * n + ijk[:, 0]
    o = np.argsort(key, kind="stable")
    pos, ids = pos[o], ids[o]
keep = []
if a.fluid_fields:
    nu = a.viscosity or 0.01
    x = (np.arange(n + 2) - 0.5) / n - 0.5
    alpha_cell, mu = dom.variable(), dom.variable()
    for l in range(a.level):
        alpha_cell.fill(1., l)
    alpha_cell.upload(np.broadcast_to(1. / (1.5 + x)[None, None, :], (n + 2,) * 3))
    mu.upload(np.broadcast_to((nu * (1.5 + x))[None, :, None], (n + 2,) * 3))
    sim.set_alpha_cell(alpha_cell)
    sim.set_viscosity_cell(mu)
    keep = [alpha_cell, mu]
pl = gfship.ParticleList(sim, pos, ids)
what = "tracers"
if a.particulates:
    rng = np.random.default_rng(1)
    vol = 1e-6 * (0.5 + rng.random(a.np))
    pl.set_particulate(np.zeros((a.np, 3)), 2. * vol, vol)
    pl.set_forces([gfship.FORCE_INERTIAL, gfship.FORCE_ADDEDMASS, gfship.FORCE_LIFT,
                   gfship.FORCE_DRAG, gfship.FORCE_BUOY], (0., 1., 0.))
    what = "particulates viscosity %g fluid-fields %s" % (a.viscosity, a.fluid_fields)
pl.event(); dom.synchronize()
for _ in range(a.repeats):
    t0 = time.perf_counter()
    for _ in range(a.events):
        pl.event()
    dom.synchronize()
    dt = (time.perf_counter() - t0) / a.events
    print("np %d level %d presort %s %s: %.3f ms/event, %.1f Mparticle-steps/s, alive %d"
          % (a.np, a.level, a.presort, what, dt * 1e3, a.np / dt / 1e6, pl.count()))
