"""N > 1 ranks of the library's OWN RCCL transport (csrc/transport.hip) on the one GPU of the test box:
the ranks are threads of one process and the RCCL the library opens is the in-process stand-in of
tests/mock_rccl (GFSHIP_RCCL_LIBRARY), which keeps NCCL's matching rule -- the k-th send from A to B
meets the k-th receive from A on B, counts must agree -- and reports mismatches and waits that can
never be served.  With a self-communicator (tests/test_gpu_multibox.py) every peer is rank 0; here the
peers are distinct: a wrong peer[], a wrong rank_of, a left / right mix-up or a posting-order mismatch
between two peers gives wrong bits, a count mismatch or a time-out.  Device boxes against oracle boxes
of the same lattice, bit for bit.  (One process per case: the library opens its RCCL once.)
The real multi-GPU run is tests/test_gpu_two_ranks.py (skipped with fewer than two devices)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "mock_rccl_worker.py")] +
                       [str(a) for a in args], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("MOCKRCCL ")][-1]
    return json.loads(line[len("MOCKRCCL "):])


@pytest.mark.parametrize("nboxes,level,overlap,fast", [(2, 5, 0, True), (4, 4, 0, True), (8, 4, 0, True),
                                                       (8, 4, 0, False), (2, 4, 1, True), (8, 4, 1, True)])
def test_lattice_flow_over_the_library_transport_with_distinct_peers(nboxes, level, overlap, fast):
    out = _run("flow", nboxes, level, 2, overlap, "fast" if fast else "nofast")
    assert out["bad"] == [], out
    assert out["differ"]                       # the boxes hold different parts of the field
    assert out["mismatches"] == 0 and out["timeouts"] == 0
    assert out["messages"] > 100 and min(out["sent"]) > 50
    if fast and not overlap:
        # the coarse end of every V-cycle after one all-gather, the tiled Godunov kernels with one
        # message of face states per side
        assert min(out["lattice_cycles"]) >= 4
        if level >= 5:       # the tiles of the Godunov kernels are 32 cells long
            assert min(out["fused_mpi"]) >= 4
    else:
        assert max(out["lattice_cycles"]) == 0


# ---------------------------------------------------------------------------------------------
# The Godunov sweeps along z with MPI sides (advect3_sweep2_kernel<.., MPI>, predict_un_sweep_kernel<.., MPI>)
# need boxes of 64^3 at least.  On a box that is its own neighbour (tests/test_gpu_multibox.py, the
# selfmpi64 switch case) whatever the neighbour sends equals the periodic image of the box's own data,
# so reading the wrong one of the two gives the same bits.  Here every box holds its part of
# M.lattice_velocity (one period over the lattice, both signs along every axis): its own wrap is
# wrong data.  DESIGN.md 11.26 has the table of what each case launches and which mutations it catches.
# ---------------------------------------------------------------------------------------------

_MPI_FAMILIES = ("PREDICT_SWEEP_MPI", "PREDICT_TILED_MPI", "PREDICT_GENERAL",
                 "ADVECT3_SWEEP2_MPI", "ADVECT3_TILED_MPI", "ADVECT_GENERAL")


def _paths(*on):
    """the Godunov families that must have run once per step at least; the others of the six: never"""
    return dict(on=on, off=tuple(f for f in _MPI_FAMILIES if f not in on))


_SWEEP = _paths("PREDICT_SWEEP_MPI", "ADVECT3_SWEEP2_MPI")
_FUSED = dict(on=("CORRECTION_FUSED", "DIVERGENCE_FUSED"), off=("CORRECTION_DECLINED",))
_UNFUSED = dict(on=("CORRECTION_DECLINED", "DIVERGENCE_FUSED"), off=("CORRECTION_FUSED",))


def _case(name, lattice, level, nsteps, paths, more, *args):
    ev = dict(on=paths["on"] + more["on"], off=paths["off"] + more["off"])
    return pytest.param(lattice, level, nsteps, ev, args, id=name)


def _flavours():
    """every <VL, SRC, CORR, 1> of advect3_sweep2_kernel and, with it, <VL, VS, 1, 1> of the predictor"""
    out = []
    for gradient, gname in ((0, "centred"), (1, "vanleer")):
        for source in (None, "V:-0.8"):
            for unfused in (False, True):
                args = ["--gradient", gradient]
                if source:
                    args += ["--source", source]
                if unfused:
                    args += ["--switch", "GFSHIP_NO_FUSED_CORRECTION"]
                name = "2x2x2-%s%s%s" % (gname, "-source" if source else "", "-unfused" if unfused else "")
                out.append(_case(name, "2x2x2", 6, 2, _SWEEP, _UNFUSED if unfused else _FUSED, *args))
    return out


_NONE = dict(on=(), off=())
SWEEP_CASES = [
    # one axis each: the x ring columns, the y ring rows, the planes 0 and n + 1; then the ring corners
    _case("2x1x1", "2x1x1", 6, 2, _SWEEP, _FUSED),
    _case("1x2x1", "1x2x1", 6, 2, _SWEEP, _FUSED),
    _case("1x1x2", "1x1x2", 6, 2, _SWEEP, _FUSED),
    _case("2x2x1", "2x2x1", 6, 2, _SWEEP, _FUSED),
] + _flavours() + [
    # the predictor with the viscous MAC source, then the components one by one and the diffusion solves
    _case("2x2x2-viscous", "2x2x2", 6, 2, _paths("PREDICT_SWEEP_MPI", "ADVECT_GENERAL"),
          dict(on=("DIVERGENCE_FUSED",), off=("CORRECTION_FUSED", "CORRECTION_DECLINED")), "--visc", 2e-3),
    _case("2x2x2-divergence-apart", "2x2x2", 6, 2, _SWEEP,
          dict(on=("CORRECTION_FUSED",), off=("CORRECTION_DECLINED", "DIVERGENCE_FUSED")),
          "--switch", "GFSHIP_NO_FUSED_DIVERGENCE"),
    _case("2x2x2-tiled", "2x2x2", 6, 2, _paths("PREDICT_TILED_MPI", "ADVECT3_TILED_MPI"),
          dict(on=("CORRECTION_FUSED",), off=("CORRECTION_DECLINED",)), "--switch", "GFSHIP_NO_MPI_SWEEP"),
    _case("2x2x2-general", "2x2x2", 6, 2, _paths("PREDICT_GENERAL", "ADVECT_GENERAL"),
          dict(on=(), off=("CORRECTION_FUSED", "CORRECTION_DECLINED", "DIVERGENCE_FUSED")),
          "--switch", "GFSHIP_NO_FUSED_MPI", "--switch", "GFSHIP_NO_LATTICE_CYCLE"),
    _case("2x2x2-overlap", "2x2x2", 6, 2, _SWEEP, _FUSED, "--overlap", 1),
    # 128^3: two chunks along z, the second with kb = 64 (the received states are indexed by the plane
    # of the box, not of the chunk)
    _case("128-2x2x2", "2x2x2", 7, 1, _SWEEP, _FUSED),
    _case("128-2x2x2-centred-source-unfused", "2x2x2", 7, 1, _SWEEP, _UNFUSED,
          "--gradient", 0, "--source", "V:-0.8", "--switch", "GFSHIP_NO_FUSED_CORRECTION"),
]


@pytest.mark.parametrize("lattice,level,nsteps,evidence,args", SWEEP_CASES)
def test_godunov_sweeps_with_mpi_sides_on_lattices_of_distinct_boxes(lattice, level, nsteps, evidence, args):
    out = _run("flow", "--lattice", lattice, "--level", level, "--nsteps", nsteps, *args)
    print("seconds", out["seconds"], "kernels of rank 0", out["kernels"][0])
    # (rank, step, name): U V W P Pmac g un, the level below the leaves of U V W, dt t niter residual;
    # step 0 is the start-up
    assert out["bad"] == [], out["bad"][:40]
    assert out["mismatches"] == 0 and out["timeouts"] == 0
    assert out["differ"]                       # no two boxes hold the same part of the field
    nboxes = 1
    for b in lattice.split("x"):
        nboxes *= int(b)
    assert len(out["kernels"]) == nboxes
    for rank, kc in enumerate(out["kernels"]):
        for f in evidence["on"]:
            assert kc[f] >= nsteps, (rank, f, kc)
        for f in evidence["off"]:
            assert kc[f] == 0, (rank, f, kc)      # a case that fell back to another path fails here
    if "GFSHIP_NO_LATTICE_CYCLE" in args:
        assert max(out["lattice_cycles"]) == 0


def test_particle_migration_over_the_library_transport_with_distinct_peers():
    out = _run("particles")
    assert out["bad"] == [], out
    assert out["moved"] > 100 and out["foreign"] > 50
    assert out["mismatches"] == 0 and out["timeouts"] == 0
