"""Worker of tests/test_gpu_mock_rccl.py: runs in a process of its own with GFSHIP_RCCL_LIBRARY naming
tests/mock_rccl/librccl_mock.so (libgfship opens its RCCL once per process).  N ranks of the library's
OWN transport (csrc/transport.hip: comm_exchange kind 0 and 1 + e, comm_exchange_begin / _end,
comm_exchange_raw, comm_reduce, comm_allgather, comm_migrate) as N threads on one GPU, every box
holding its part of a field with one period over the lattice, against oracle boxes of the same
lattice, bit for bit.  Prints one JSON line.

  python tests/mock_rccl_worker.py flow NBOXES LEVEL NSTEPS OVERLAP [nofast]
  python tests/mock_rccl_worker.py flow --lattice BXxBYxBZ --level L --nsteps N [--overlap 1] [--gradient 0|1]
         [--source U|V|W:value] [--visc nu] [--switch GFSHIP_NAME ...]
  python tests/mock_rccl_worker.py particles
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "mock_rccl", "librccl_mock.so")
os.environ["GFSHIP_RCCL_LIBRARY"] = MOCK
for p in (ROOT, os.path.join(ROOT, "gerris-fft-particles_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402

import gfship  # noqa: E402
from gfship import distributed as D  # noqa: E402
import multibox as M  # noqa: E402


def mock_counters():
    L = C.CDLL(MOCK)      # the copy libgfship opened (same path: same handle)
    for f in ("mock_rccl_mismatches", "mock_rccl_messages", "mock_rccl_timeouts"):
        getattr(L, f).restype = C.c_ulonglong
    return dict(mismatches=int(L.mock_rccl_mismatches()), messages=int(L.mock_rccl_messages()),
                timeouts=int(L.mock_rccl_timeouts()))


KERNEL_FAMILIES = ("PREDICT_SWEEP_MPI", "PREDICT_TILED_MPI", "PREDICT_GENERAL", "ADVECT3_SWEEP2_MPI",
                   "ADVECT3_TILED_MPI", "ADVECT_GENERAL", "CORRECTION_FUSED", "CORRECTION_DECLINED",
                   "DIVERGENCE_FUSED")


def differing(d, o):
    """names of what differs between two states of tests/test_multibox_cpu.py::lattice_flow_state"""
    bad = [name for name in ("u", "v", "w", "p", "pmac") if not np.array_equal(d[name], o[name])]
    for key, tag in (("g", "g%d"), ("un", "un%d"), ("coarse", "coarse%d")):
        bad += [tag % c for c in range(3) if not np.array_equal(d[key][c], o[key][c])]
    bad += [name for name in ("dt", "t", "res") if d[name] != o[name]]
    if tuple(d["niter"]) != tuple(o["niter"]):
        bad.append("niter")
    return bad


def flow(grid, level, nsteps, overlap, gradient=None, source=None, visc=0., switches=()):
    """device boxes of the lattice `grid` over the library's transport against oracle boxes of the same
    lattice: everything lattice_flow_state holds, after the start-up (step 0) and after every step"""
    import time
    from test_multibox_cpu import lattice_flow_state, run_lattice_flow_threads
    for name in switches:
        assert name.startswith("GFSHIP_"), name
        os.environ[name] = "1"          # a domain looks its switches up when it is created
    n = 1 << level
    nboxes = grid.n
    t0 = time.time()
    ora = run_lattice_flow_threads(nboxes, level, nsteps, overlap, grid=grid, gradient=gradient,
                                   source=source, visc=visc, per_step=True)
    t1 = time.time()
    uid = gfship.comm_unique_id()
    bad = []
    i3 = (slice(1, -1),) * 3

    def worker(rank, fabric):
        gd = gfship.Domain(3, level, grid.sides(rank))
        if overlap:
            gd.set_overlap(overlap)
        gd.comm_init(uid, rank, nboxes, grid.b)
        assert gd.comm_size() == nboxes
        gs = gfship.Simulation(gd)
        X, Y, Z = M.global_centres(grid, rank, n)
        for c, a in enumerate(M.lattice_velocity(X, Y, Z)):
            b = np.zeros((n + 2,) * 3)
            b[1:-1, 1:-1, 1:-1] = a
            gs.u[c].upload(b)
        if gradient is not None:
            gs.advection_params.gradient = gradient
        if source is not None:
            gs.set_source(*source)
        if visc:
            for c in range(3):
                gs.set_viscosity(c, visc)

        def check(step):
            gd.synchronize()
            st = lattice_flow_state(gs, n, level, gs.un, lambda f: f.download()[i3],
                                    lambda f: f.download(level - 1)[i3])
            bad.extend((rank, step, name) for name in differing(st, ora[rank][step]))
            return st

        gs.start()
        st = check(0)
        for k in range(nsteps):
            gs.step()
            st = check(k + 1)
        kc = gd.kernel_counts()
        out = dict(u=st["u"], kernels={f: kc[f] for f in KERNEL_FAMILIES}, counts=gd.path_counts(),
                   stats=gd.comm_stats())
        fabric.barrier.wait()       # nobody destroys buffers a neighbour may still read
        gs.destroy()
        gd.destroy()
        return out

    dev = M.run_boxes(nboxes, worker)
    t2 = time.time()
    differ = all(not np.array_equal(dev[a]["u"], dev[b]["u"]) for a in range(nboxes) for b in range(a))
    return dict(bad=sorted(bad), differ=bool(differ), kernels=[d["kernels"] for d in dev],
                lattice_cycles=[int(d["counts"][0]) for d in dev],
                fused_mpi=[int(d["counts"][1]) for d in dev],
                sent=[int(d["stats"][0]) for d in dev],
                seconds=dict(oracle=round(t1 - t0, 2), device=round(t2 - t1, 2)), **mock_counters())


def flow_arguments(argv):
    """flow NBOXES LEVEL NSTEPS OVERLAP [nofast], or flow --lattice BXxBYxBZ --level L --nsteps N with
    --overlap, --gradient, --source U|V|W:value, --visc nu and --switch GFSHIP_NAME (repeatable)"""
    if argv and not argv[0].startswith("--"):
        nofast = len(argv) > 4 and argv[4] == "nofast"
        return dict(grid=D.BoxGrid(int(argv[0]), 3), level=int(argv[1]), nsteps=int(argv[2]),
                    overlap=int(argv[3]),
                    switches=("GFSHIP_NO_LATTICE_CYCLE", "GFSHIP_NO_FUSED_MPI") if nofast else ())
    import argparse
    ap = argparse.ArgumentParser(prog="mock_rccl_worker.py flow")
    ap.add_argument("--lattice", required=True)
    ap.add_argument("--level", type=int, required=True)
    ap.add_argument("--nsteps", type=int, required=True)
    ap.add_argument("--overlap", type=int, default=0)
    ap.add_argument("--gradient", type=int, default=None)
    ap.add_argument("--source", default=None)
    ap.add_argument("--visc", type=float, default=0.)
    ap.add_argument("--switch", action="append", default=[])
    a = ap.parse_args(argv)
    source = None
    if a.source:
        comp, value = a.source.split(":")
        source = ("UVW".index(comp), float(value))
    return dict(grid=M.ShapedGrid([int(x) for x in a.lattice.split("x")]), level=a.level, nsteps=a.nsteps,
                overlap=a.overlap, gradient=a.gradient, source=source, visc=a.visc, switches=tuple(a.switch))


def particles():
    """tracers crossing the sides of 2 x 2 x 2 boxes: comm_migrate with real peers (counts, then the
    records; sides without leavers included) against oracle boxes of the same lattice that hand their
    packets over through the in-process transport (send_particles / rcv_particles,
    modules/particulatecommon.c:3218-3312)"""
    from oracle import oracle as O
    from particle_cases import lcg_positions
    nboxes, level, nev = 8, 4, 6
    n = 1 << level
    grid = D.BoxGrid(nboxes, 3)
    uid = gfship.comm_unique_id()
    L = O.lib()

    def seeds(rank):
        pos, ids = lcg_positions(300, seed=17 + rank)
        return pos, (ids + 1000 * rank).astype(np.uint32)

    def velocity(rank):
        X, Y, Z = M.global_centres(grid, rank, n)
        u, v, w = M.lattice_velocity(X, Y, Z)
        return [2. * u + 0.8, 2. * v - 0.6, 2. * w + 0.7]       # through-flow across every side

    def oworker(rank, fabric):
        sim = O.Sim(3, level, grid.sides(rank))
        tr = M.LocalTransport(grid, rank, fabric)
        hooks = M.OracleHooks(L, sim.dom.ptr, 3, tr)
        for c, a in enumerate(velocity(rank)):
            sim.u[c].interior()[...] = a
        opl = O.Particles(sim, *seeds(rank))
        sim.start()
        moved = 0
        for _ in range(nev):
            opl.event()
            out = {d: opl.outbox(d) for d in grid.external_sides()}
            moved += sum(len(a) for a in out.values())
            opl.clear_outbox()
            for d, a in sorted(tr.exchange_records(out).items()):
                opl.append(a)
            sim.step()
        st = opl.state()
        del hooks
        return st + (moved,)

    def dworker(rank, fabric):
        gd = gfship.Domain(3, level, grid.sides(rank))
        gd.comm_init(uid, rank, nboxes, grid.b)
        gs = gfship.Simulation(gd)
        for c, a in enumerate(velocity(rank)):
            b = np.zeros((n + 2,) * 3)
            b[1:-1, 1:-1, 1:-1] = a
            gs.u[c].upload(b)
        pl = gfship.ParticleList(gs, *seeds(rank))
        pl.set_sort_interval(2)
        gs.start()
        for _ in range(nev):
            pl.event()
            gs.step()
        gd.synchronize()
        p, i = pl.download()
        fabric.barrier.wait()
        pl.destroy()
        gs.destroy()
        gd.destroy()
        return p, i

    dev = M.run_boxes(nboxes, dworker)
    ora = M.run_boxes(nboxes, oworker)
    bad, moved, foreign = [], 0, 0
    for rank, ((dp, di), (op, oi, mv)) in enumerate(zip(dev, ora)):
        a, b = np.argsort(di, kind="stable"), np.argsort(oi, kind="stable")
        if not (len(di) == len(oi) and np.array_equal(di[a], oi[b]) and np.array_equal(dp[a], op[b])):
            bad.append(rank)
        moved += int(mv)
        foreign += int(np.sum(np.asarray(oi) // 1000 != rank))
    return dict(bad=bad, moved=moved, foreign=foreign, **mock_counters())


if __name__ == "__main__":
    if sys.argv[1] == "flow":
        out = flow(**flow_arguments(sys.argv[2:]))
    else:
        out = particles()
    print("MOCKRCCL " + json.dumps(out))
