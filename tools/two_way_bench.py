#!/usr/bin/env python
"""Times the two-way coupling entries on the flagship box: N particulates in the periodic 3-D
Taylor-Green box of 2^level cells per side, rkernel = 1.5 h, the polynomial kernel.

  python tools/two_way_bench.py [--level 8] [--particles 2000000] [--reps 10]

One JSON line: the median of `reps' single calls, each between two synchronisations of the stream, after
two calls that are not counted (the first one allocates the work arrays and compiles the kernel text), for
    particulate_field   gfship_particulate_field
    forces_on_fluid     gfship_particles_forces_on_fluid
    spread_forces       gfship_particles_spread_forces (emit, kernel function, corrections, sort, sums)
    spread_pass1/pass2  gfship_particles_time_spreading: the time of the device in pass 1 (descent, kernel
                        function, corrections) and in pass 2 (sort, sums per cell), from events on the stream
    event               gfship_particle_list_event of the same list with the same forces + buoyancy: the
                        yardstick of forces_on_fluid, measured last (it moves the particles)
and the record slots per particle and per chunk of the spreading."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gerris-fft-particles_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import gfship                                       # noqa: E402
from bench import taylor_green, with_ghosts         # noqa: E402
from particle_cases import lcg_positions_fast       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--particles", type=int, default=2000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--viscosity", type=float, default=1e-3)
    args = ap.parse_args()
    n = 1 << args.level
    h = 1. / n
    dom = gfship.Domain(3, args.level, [gfship.SIDE_PERIODIC] * 6)
    sim = gfship.Simulation(dom)
    for c, a in enumerate(taylor_green(n)):
        sim.u[c].upload(with_ghosts(a))
        sim.set_viscosity(c, args.viscosity)
    sim.start()
    sim.step()
    pos, ids = lcg_positions_fast(args.particles)
    rng = np.random.default_rng(1)
    vol = 1e-6 * (0.5 + rng.random(args.particles))
    pl = gfship.ParticleList(sim, pos, ids)
    pl.set_particulate(np.zeros((args.particles, 3)), 2. * vol, vol)
    forces = [gfship.FORCE_INERTIAL, gfship.FORCE_ADDEDMASS, gfship.FORCE_LIFT, gfship.FORCE_DRAG,
              gfship.FORCE_BUOY]
    pl.set_forces(forces, (0., 1., 0.))
    pl.set_kernel(1.5 * h, "(1. - 0.04*(x*x + y*y + z*z))")
    pl.sort()
    v = dom.variable()
    F = [dom.variable() for _ in range(3)]

    def median_ms(call):
        for _ in range(2):
            call()
        dom.synchronize()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            dom.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(t)), float(min(t)), float(max(t))

    out = {"level": args.level, "particles": args.particles, "reps": args.reps, "rkernel_h": 1.5}
    for name, call in (("particulate_field", lambda: pl.particulate_field(v)),
                       ("forces_on_fluid", pl.forces_on_fluid),
                       ("spread_forces", lambda: pl.spread_forces(F))):
        med, lo, hi = median_ms(call)
        out[name + "_ms"] = {"median": med, "min": lo, "max": hi}
    # the two passes of the spreading and its record buffer, as the library reports them
    runs = [pl.time_spreading(F) for _ in range(args.reps)]
    for k, name in enumerate(("spread_pass1_ms", "spread_pass2_ms")):
        t = [r[k] for r in runs]
        out[name] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
    _, _, stride, per_chunk, nbytes = runs[0]
    out["record_slots_per_particle"] = stride
    out["particles_per_chunk"] = per_chunk
    out["chunks"] = -(-args.particles // per_chunk)
    out["work_array_bytes"] = nbytes
    med, lo, hi = median_ms(pl.event)
    out["event_ms"] = {"median": med, "min": lo, "max": hi}
    Fx = F[0].download()[1:-1, 1:-1, 1:-1]
    out["cells_with_a_deposit"] = int(np.count_nonzero(Fx))
    print(json.dumps(out))
    pl.destroy()


if __name__ == "__main__":
    main()
