"""Wall time of gfship_tracer_advection on one periodic box: a tracer without a GfsSourceDiffusion, with one
on the fused path (leaf copy + advection + diffusion_rhs in one pass), with one on the composed path (the three
passes) -- taken in turn, several rounds, each figure a host clock around `reps' calls that end in a synchronise,
after one warm-up call.  The implicit solve is the same work on both paths (same right-hand side, bit for bit),
so the difference of the two is the gain of the fused pass:
tools/tracer_diffusion.py [level] [rounds]"""
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
gs = gfship.Simulation(gd)
T = gs.add_tracer()
c = (np.arange(n + 2) - 0.5) / n - 0.5
z, y, x = np.meshgrid(c, c, c, indexing="ij")
tp = 2. * np.pi
T0 = np.sin(tp * x) * np.cos(tp * y) * np.cos(tp * z)
# a divergence-free MAC field of amplitude 0.3 (+ faces; entry 0 along c is the image of entry n)
h = 0.5 / n
gs.mac_velocity(0).upload(0.3 * np.sin(tp * (x + h)) * np.cos(tp * y) * np.cos(tp * z))
gs.mac_velocity(1).upload(-0.3 * np.cos(tp * x) * np.sin(tp * (y + h)) * np.cos(tp * z))
gs.mac_velocity(2).upload(np.zeros_like(x))
D, dt = 0.05, 0.2 / n


def timed(Dv, path, reps=20):
    T.upload(T0)
    gd.bc(T)
    gs.set_tracer_diffusion(T, Dv)
    gs.tracer_diffusion_path(path)
    gs.tracer_advection(T, dt)
    gd.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        gs.tracer_advection(T, dt)
    gd.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, gs.tracer_diffusion_params(T).niter


rows = []
for r in range(rounds):
    plain, fused, composed = timed(0., 1), timed(D, 1), timed(D, 0)
    rows.append((plain[0], fused[0], composed[0]))
    print("level %d round %d  no diffusion %.3f  fused %.3f  composed %.3f  ms per call (niter of the last solve %d, %d)"
          % (lev, r, plain[0], fused[0], composed[0], fused[1], composed[1]), flush=True)
a = np.array(rows)
print("median               no diffusion %.3f  fused %.3f  composed %.3f  composed - fused %.3f ms"
      % (np.median(a[:, 0]), np.median(a[:, 1]), np.median(a[:, 2]), np.median(a[:, 2] - a[:, 1])))
print("spread (max - min)   no diffusion %.3f  fused %.3f  composed %.3f ms"
      % tuple(a.max(axis=0) - a.min(axis=0)))
print("counts (fused, composed): %r" % (gs.tracer_diffusion_counts(),))
