#!/usr/bin/env python
"""Times GfsSourceParticulateVol on the flagship box: N particulates with drag in the periodic 3-D
Taylor-Green box of 2^level cells per side, the storage sorted by cell.

  python tools/particulate_sources_bench.py [--level 8] [--particles 2000000] [--reps 10]

One JSON line: the median of `reps' single calls, each between two synchronisations of the stream, after
two calls that are not counted (the first one allocates the work arrays), for
    vol_constant          the event of a volume source with a constant function, all five variables written
    vol_field             the same with a function that reads one field and the relative velocity (hipRTC)
    vol_field_no_fields   the same with no variable written: nothing is sorted
    *_per_particle/_cells gfship_particulate_source_time_event: the time of the device in the passes per
                          particle (locate, interpolation, function, update) and in the sort with the pass per
                          cell, from events on the stream
    event                 gfship_particle_list_event of the same list (GfsForceDrag), the yardstick, measured
                          last (it moves the particles)."""
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
    pl.set_forces([gfship.FORCE_DRAG], (0., 0., 0.))
    pl.sort()
    T = dom.variable()
    T.fill(1.)
    variables = [dom.variable() for _ in range(5)]
    # rates small enough that no volume changes sign over the calls of this run
    sources = {"vol_constant": gfship.ParticulateSource(pl, gfship.SOURCE_VOLUME, "1e-9"),
               "vol_field": gfship.ParticulateSource(pl, gfship.SOURCE_VOLUME,
                                                     "1e-9*T*(Urelp*Urelp + Vrelp*Vrelp + Wrelp*Wrelp)", {"T": T}),
               "vol_field_no_fields": gfship.ParticulateSource(pl, gfship.SOURCE_VOLUME,
                                                               "1e-9*T*(Urelp*Urelp + Vrelp*Vrelp + Wrelp*Wrelp)",
                                                               {"T": T})}
    for name in ("vol_constant", "vol_field"):
        sources[name].set_fields(variables[0], variables[1:4], variables[4])

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
        return {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}

    out = {"level": args.level, "particles": args.particles, "reps": args.reps}
    for name, src in sources.items():
        out[name + "_ms"] = median_ms(src.event)
        runs = [src.time_event() for _ in range(args.reps)]
        for k, part in enumerate(("_per_particle_ms", "_cells_ms")):
            t = [r[k] for r in runs]
            out[name + part] = {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
    out["cells_with_a_deposit"] = int(np.count_nonzero(variables[4].download()[1:-1, 1:-1, 1:-1]))
    out["event_ms"] = median_ms(pl.event)
    print(json.dumps(out))
    for src in sources.values():
        src.destroy()
    pl.destroy()


if __name__ == "__main__":
    main()
