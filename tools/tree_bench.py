#!/usr/bin/env python3
"""Time steps of the refined-tree path (gfship_tree) on an octree / quadtree with BOX
extra levels inside the central cube / square: leaves, dependency levels of the finest sweep, ms per
step, Mleaf-steps/s.  Not the benchmarked path (that is bench.py); a measurement to quote.
usage: tree_bench.py [dim] [level] [box] [steps] [nu] [--snapshot] [--tracers N] [--particulates N] [--two-way N]
                     [--sources N [--source-function constant|field]] [--droplets]
nu: GfsSourceDiffusion on every velocity component (default 0: inviscid)
--snapshot: also time the file image of the tree (gfship_tree_snapshot_write) for P, Pmac, U, V
(, W): the first call, which builds the offset tables, and the median of 20 more (kernel + copy to the host),
ending in the stream synchronise of the call.  The share of the kernel and of the copy comes from a kernel and
memory-copy trace of the same command.
--tracers N: after the steps, a GfsParticleList of N GfsParticle tracers (the positions of tools/particles_bench.py)
on the tree: one event to warm up (it sorts the list by leaf), then the mean of 10 gfship_particle_list_event, ended
by gfship_particles_count (a stream synchronise); Mparticle-steps/s of the event and the size of the corner tables
of the sampler.
--particulates N: the same for a list of N GfsParticulate with the five forces and their default coefficients (the
particles and forces of tools/particles_bench.py --particulates; the drag acts where nu is given): the event of
tree_particulate_list_event_kernel (the forces of csrc/particulate_forces.hpp) and, after it, the copy of U, V, W
into Un, Vn, Wn.
--two-way N: the two-way coupling of a tree for the list of --particulates N, rkernel = 1.5 h of the
finest leaves, the polynomial kernel: one call to warm up, then the mean of 10 and the least and the largest of them,
each ended by a stream synchronise, of Tree.particulate_field, Tree.forces_on_fluid, Tree.spread_forces and, last (it
moves the particles), of the event of the same list: the yardstick of forces_on_fluid.
--sources N: GfsSourceParticulateVol on a tree for a list of N GfsParticulate with GfsForceDrag, the
storage sorted by leaf, Rad, Urelp ... and the deposit written: a volume source with a constant function and one with
compiled text that reads one variable (--source-function picks one of the two).  Medians of 10 calls after two
uncounted ones, with the least and the largest: the whole event (each call ended by a stream synchronise), the
passes per particle and the sort with the pass per leaf (gfship_particulate_source_time_event: device time between
events on the stream), and last (it moves the particles) the event of the same list.
--droplets: a second line, gfship_tree_tag_droplets_time (a warm-up call, then the milliseconds per call
of 20 between two events on the stream, each call ended by the read of n) of a tracer given on every level: a
few balls, noise (every cell of every level in the mask or not by a hash of its place: many droplets, and gates shut
at random), and the whole tree as one droplet; with the number of droplets, and for context gfship_tag_droplets_time
of the same three on the uniform box whose cell count is nearest to the leaves of the tree."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gerris-fft-particles_amd"))
import gfship

snapshot = "--snapshot" in sys.argv
sys.argv = [a for a in sys.argv if a != "--snapshot"]
ntracers = 0
if "--tracers" in sys.argv:
    k = sys.argv.index("--tracers")
    ntracers = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
nparticulates = 0
if "--particulates" in sys.argv:
    k = sys.argv.index("--particulates")
    nparticulates = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
ntwoway = 0
if "--two-way" in sys.argv:
    k = sys.argv.index("--two-way")
    ntwoway = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
nsources, source_function = 0, "both"
if "--source-function" in sys.argv:
    k = sys.argv.index("--source-function")
    source_function = sys.argv[k + 1]
    assert source_function in ("constant", "field", "both")
    del sys.argv[k:k + 2]
if "--sources" in sys.argv:
    k = sys.argv.index("--sources")
    nsources = int(sys.argv[k + 1])
    del sys.argv[k:k + 2]
droplets = "--droplets" in sys.argv
sys.argv = [a for a in sys.argv if a != "--droplets"]
dim = int(sys.argv[1]) if len(sys.argv) > 1 else 3
level = int(sys.argv[2]) if len(sys.argv) > 2 else 4
box = int(sys.argv[3]) if len(sys.argv) > 3 else 2
steps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
nu = float(sys.argv[5]) if len(sys.argv) > 5 else 0.
inside = lambda *a: all(-0.25 <= v <= 0.25 for v in a)
t0 = time.time()
if dim == 3:
    g = gfship.Tree(lambda x, y, z: level + box if inside(x, y, z) else level, dim=3)
else:
    g = gfship.Tree(lambda x, y: level + box if inside(x, y) else level)
t_build = time.time() - t0
nleaves = 0
for l in range(g.depth + 1):
    f = g.flags(l)
    nleaves += int(np.sum(f[(slice(1, -1),) * dim] == 1))
    c = g.centres(l)
    if dim == 3:
        x, y, z = c
        u = np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) * np.cos(2 * np.pi * z)
        v = -np.cos(2 * np.pi * x) * np.sin(2 * np.pi * y) * np.cos(2 * np.pi * z)
        g.upload(g.W, l, 0. * u)
    else:
        x, y = c
        u = 1. - 2. * np.cos(2 * np.pi * x) * np.sin(2 * np.pi * y)
        v = 1. + 2. * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)
    g.upload(g.U, l, u)
    g.upload(g.V, l, v)
if nu != 0.:
    for c in range(dim):
        g.set_viscosity(c, nu)
cvar = g.add_tracer() if droplets else None      # the tracer whose droplets are tagged: a variable of the run
g.set_time(1e30, 0.8)
g.start()
g.step()
t0 = time.time()
for _ in range(steps):
    g.step()
ms = (time.time() - t0) / steps * 1e3
nc, nl = g.sweep_levels(g.depth)
snap = {}
if snapshot:
    vars_ = [g.P, g.PMAC, g.U, g.V] + ([g.W] if dim == 3 else [])
    t0 = time.time()
    image = g.snapshot(vars_)
    first = (time.time() - t0) * 1e3
    times = []
    for _ in range(20):
        t0 = time.time()
        g.snapshot(vars_)
        times.append((time.time() - t0) * 1e3)
    ncells = len(image) // (12 + 8 * len(vars_))
    snap = {"snapshot_cells": ncells, "snapshot_image_bytes": len(image),
            "snapshot_bytes_moved": len(image) + 8 * len(vars_) * ncells,
            "snapshot_first_ms": round(first, 3), "snapshot_ms": round(sorted(times)[len(times) // 2], 3),
            "snapshot_ms_min_max": [round(min(times), 3), round(max(times), 3)]}
trac = {}
if ntracers:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from particle_cases import lcg_positions_fast
    pos, ids = lcg_positions_fast(ntracers)
    if dim == 2:
        pos[:, 2] = 0.
    pl = g.particles(pos, ids)
    pl.event()
    pl.count()
    events = 10
    t0 = time.perf_counter()
    for _ in range(events):
        pl.event()
    alive = pl.count()
    dt_event = (time.perf_counter() - t0) / events
    st = g.sampler_stats()
    trac = {"tracers": ntracers, "tracers_alive": alive, "ms_per_event": round(dt_event * 1e3, 3),
            "Mparticle_steps_per_s": round(ntracers / dt_event / 1e6, 1),
            "leaf_corners": st[0], "table_corners": st[1], "table_share": round(st[1] / st[0], 4),
            "table_entries": st[2], "table_bytes": st[3], "longest_interpolator": st[4]}
    pl.destroy()
part = {}
if nparticulates:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from particle_cases import lcg_positions_fast
    pos, ids = lcg_positions_fast(nparticulates)
    if dim == 2:
        pos[:, 2] = 0.
    rng = np.random.default_rng(1)
    vol = 1e-6 * (0.5 + rng.random(nparticulates))
    pl = g.particulates(pos, ids, np.zeros((nparticulates, 3)), 2. * vol, vol)
    pl.set_forces([gfship.FORCE_INERTIAL, gfship.FORCE_ADDEDMASS, gfship.FORCE_LIFT, gfship.FORCE_DRAG,
                   gfship.FORCE_BUOY], (0., 1., 0.))
    pl.event()
    pl.count()
    events = 10
    t0 = time.perf_counter()
    for _ in range(events):
        pl.event()
    alive = pl.count()
    dt_event = (time.perf_counter() - t0) / events
    part = {"particulates": nparticulates, "particulates_alive": alive,
            "particulates_ms_per_event": round(dt_event * 1e3, 3),
            "particulates_Mparticle_steps_per_s": round(nparticulates / dt_event / 1e6, 1)}
    pl.destroy()
two = {}
if ntwoway:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from particle_cases import lcg_positions_fast
    pos, ids = lcg_positions_fast(ntwoway)
    if dim == 2:
        pos[:, 2] = 0.
    rng = np.random.default_rng(1)
    vol = 1e-6 * (0.5 + rng.random(ntwoway))
    pl = g.particulates(pos, ids, np.zeros((ntwoway, 3)), 2. * vol, vol)
    pl.set_forces([gfship.FORCE_INERTIAL, gfship.FORCE_ADDEDMASS, gfship.FORCE_LIFT, gfship.FORCE_DRAG,
                   gfship.FORCE_BUOY], (0., 1., 0.))
    g.set_kernel(pl, 1.5 / (1 << g.depth), "(1. - 0.04*(x*x + y*y + z*z))")
    pl.sort()

    def mean_ms(call):
        call()
        pl.count()
        t = []
        for _ in range(10):
            t0 = time.perf_counter()
            call()
            pl.count()
            t.append((time.perf_counter() - t0) * 1e3)
        return {"mean": round(float(np.mean(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}

    two = {"two_way_particulates": ntwoway, "rkernel_h_fine": 1.5}
    for name, call in (("particulate_field_ms", lambda: g.particulate_field(pl)),
                       ("forces_on_fluid_ms", lambda: g.forces_on_fluid(pl)),
                       ("spread_forces_ms", lambda: g.spread_forces(pl)),
                       ("event_ms", pl.event)):
        two[name] = mean_ms(call)
    two["leaves_with_a_deposit"] = int(sum(np.count_nonzero(g.download(g.FX, l)) for l in range(g.depth + 1)))
    pl.destroy()
srcs = {}
if nsources:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from particle_cases import lcg_positions_fast
    pos, ids = lcg_positions_fast(nsources)
    if dim == 2:
        pos[:, 2] = 0.
    rng = np.random.default_rng(1)
    vol = 1e-6 * (0.5 + rng.random(nsources))
    pl = g.particulates(pos, ids, np.zeros((nsources, 3)), 2. * vol, vol)
    pl.set_forces([gfship.FORCE_DRAG], (0., 0., 0.))
    pl.sort()
    w = " + Wrelp*Wrelp" if dim == 3 else ""
    # rates small enough that no volume changes sign over the calls of this run; P stands for any variable of the tree
    texts = {"constant": ("1e-9", None), "field": ("1e-9*T*(Urelp*Urelp + Vrelp*Vrelp%s)" % w, {"T": g.P})}
    urel = [g.URELP, g.VRELP, g.WRELP][:dim]

    def stats(t):
        return {"median": round(float(np.median(t)), 3), "min": round(min(t), 3), "max": round(max(t), 3)}

    def median_ms(call):
        for _ in range(2):
            call()
        pl.count()
        t = []
        for _ in range(10):
            t0 = time.perf_counter()
            call()
            pl.count()
            t.append((time.perf_counter() - t0) * 1e3)
        return stats(t)

    srcs = {"sources_particulates": nsources}
    for name in ("constant", "field"):
        if source_function not in (name, "both"):
            continue
        src = gfship.TreeParticulateSource(g, pl, gfship.SOURCE_VOLUME, texts[name][0], texts[name][1])
        src.set_fields(g.RAD, urel, g.VOLSRC)
        srcs["vol_%s_ms" % name] = median_ms(src.event)
        runs = [src.time_event() for _ in range(10)]
        srcs["vol_%s_per_particle_ms" % name] = stats([r[0] for r in runs])
        srcs["vol_%s_leaves_ms" % name] = stats([r[1] for r in runs])
        src.destroy()
    srcs["leaves_with_a_deposit"] = int(sum(np.count_nonzero(g.download(g.VOLSRC, l)) for l in range(g.depth + 1)))
    srcs["sources_event_ms"] = median_ms(pl.event)
    pl.destroy()
print({"dim": dim, "levels": [level, g.depth], "leaves": nleaves, "finest_sweep_cells": nc,
       "finest_sweep_dependency_levels": nl, "tree_build_s": round(t_build, 2),
       "ms_per_step": round(ms, 2), "Mleaf_steps_per_s": round(nleaves / ms / 1e3, 3),
       "niter": [g.projection_params.niter, g.approx_projection_params.niter],
       **snap, **trac, **part, **two, **srcs,
       **({"nu": nu, "diffusion_niter": [g.diffusion_params(c).niter for c in range(dim)]} if nu != 0. else {})})
if droplets:
    balls = (((0.12, 0.1, 0.05), 0.17), ((-0.27, 0.04, 0.), 0.09), ((0.5, -0.22, 0.1), 0.11), ((-0.3, -0.3, -0.3), 0.1))

    def fields(centres):
        r2 = [sum((centres[a] - c[a])**2 for a in range(dim)) for c, _ in balls]
        blob = np.zeros_like(centres[0])
        for d2, (_, r) in zip(r2, balls):
            blob = np.maximum(blob, (d2 < r*r)*0.75)
        h = np.zeros(centres[0].shape)
        for a in range(dim):
            h = h*7919.13 + np.floor((centres[a] + 0.75)*4096.)
        noise = (np.modf(np.sin(h)*43758.5453)[0] % 1. > 0.5)*0.75
        return {"blobs": blob, "noise": noise, "whole": 0.*blob + 0.75}

    drop = {"leaves": nleaves}
    per_level = [fields(g.centres(l)) for l in range(g.depth + 1)]
    for name in ("blobs", "noise", "whole"):
        for l in range(g.depth + 1):
            g.upload(cvar, l, per_level[l][name])
        n = g.tag_droplets(cvar)
        drop["tree_%s" % name] = {"droplets": n, "ms_per_call": round(g.time_tag_droplets(cvar, 20), 4)}
    blevel = int(round(np.log2(nleaves)/dim))
    gd = gfship.Domain(dim, blevel, [gfship.SIDE_PERIODIC]*6)
    c, tag = gd.variable(), gd.variable()
    nb = 1 << blevel
    cc = -0.5 + (np.arange(nb + 2) - 0.5)/nb
    centres = np.meshgrid(cc, cc, indexing="xy") if dim == 2 else np.meshgrid(cc, cc, cc, indexing="ij")[::-1]
    drop["box_level"], drop["box_cells"] = blevel, nb**dim
    for name, a in fields(centres).items():
        c.upload(np.ascontiguousarray(a))
        n = gd.tag_droplets(c, tag)
        drop["box_%s" % name] = {"droplets": n, "ms_per_call": round(gd.time_tag_droplets(c, tag, 20), 4)}
    gd.destroy()
    print(drop)
g.destroy()
