"""Every path of coarse_cycle_kernel<3> (csrc/poisson_kernels.hip) against the oracle: one or two
gfs_poisson_cycle of a 32^3 box, whose coarse end is the levels 0 .. 4 in one launch -- the top level 16^3
has four waves per sweep slot --, and one of a 64^3 box.  Seeded random right-hand side and initial guess.

  sides     six periodic (the all-periodic ghost refresh); six boundaries with the condition the pressure
            has there (the default of a scalar, homogeneous Neumann); periodic in x only: the last two go
            through the generic refresh
  nrelax    1 with erelax 1 (no sweep follows a sweep: nothing is refreshed), 2, 4, 5
  erelax    2: up to 160 sweeps on the coarsest level, the sweep slots wrap many times
  minlevel  0, 1, 3
  dia       non-zero on the coarse levels: the general cell path
  threads   GFSHIP_COARSE_THREADS = 256 and 512, each in a fresh process (the switch is read when the domain
            is created): with 256 threads nconc*nface > nt at 16^3, the strided path runs

np.array_equal on the solution with its face ghosts, on the new residual and on every level of the residual
the coarse end wrote (minlevel .. depth - 1, interior).  The oracle half of a case is computed once and
shared between the in-process test and the children."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "gerris-fft-particles_amd")]

import gfship  # noqa: E402
import multigrid_param_cases as M  # noqa: E402
from oracle import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

# the condition of the pressure on a GfsBoundary: nothing set, the default of a scalar
M.SIDE_KINDS.setdefault("boundary", ([O.SIDE_BOUNDARY] * 6, [None] * 6))

# (level, sides, dia, (nrelax, erelax, minlevel), cycles)
CASES = [
    (5, "periodic", False, (1, 1, 0), 1),
    (5, "periodic", False, (2, 1, 0), 1),
    (5, "periodic", False, (4, 1, 0), 2),     # the sets of the flagship step
    (5, "periodic", False, (5, 1, 1), 1),
    (5, "periodic", False, (1, 2, 0), 1),
    (5, "periodic", False, (2, 2, 1), 1),
    (5, "periodic", False, (4, 2, 3), 1),
    (5, "periodic", False, (5, 2, 0), 2),
    (5, "boundary", False, (1, 1, 0), 1),
    (5, "boundary", False, (4, 1, 0), 2),
    (5, "boundary", False, (5, 2, 1), 1),
    (5, "boundary", False, (2, 2, 3), 1),
    (5, "mixed", False, (4, 1, 0), 2),
    (5, "mixed", False, (1, 2, 0), 1),
    (5, "mixed", False, (5, 2, 3), 1),
    (5, "mixed", False, (2, 1, 1), 1),
    (5, "periodic", True, (5, 2, 0), 1),
    (5, "mixed", True, (4, 1, 1), 1),
    (6, "periodic", False, (4, 1, 0), 1),
]
# the cases a child with another thread count runs
CHILD_CASES = [c for c in CASES if c[0] == 5 and c[3] in ((4, 1, 0), (5, 2, 0), (5, 2, 1), (1, 2, 0), (4, 1, 1))]
THREADS = (256, 512)


def _id(case):
    level, kind, dia, s, cycles = case
    return "%d-%s%s-%d-%d-%d-x%d" % (1 << level, kind, "-dia" if dia else "", s[0], s[1], s[2], cycles)


@functools.lru_cache(maxsize=None)
def oracle_case(case):
    """[(u with ghosts, res interior, {level: res interior of the level})] after every cycle"""
    level, kind, dia, (nrelax, erelax, minlevel), cycles = case
    o = M.OracleCycle(3, level, kind, dia)
    out = []
    for _ in range(cycles):
        u, res = o.cycle(nrelax, erelax, minlevel)
        coarse = {l: o.res.level(l)[1:-1, 1:-1, 1:-1].copy() for l in range(minlevel, level)}
        out.append((u, res, coarse))
    return out


def _face_ghosts_equal(a, b):
    """interior and the six face ghost layers (edges and corners hold nothing the reference defines)"""
    inner = slice(1, -1)
    ok = np.array_equal(a[inner, inner, inner], b[inner, inner, inner])
    for ax in range(3):
        for side in (0, -1):
            sl = [inner] * 3
            sl[ax] = side
            ok = ok and np.array_equal(a[tuple(sl)], b[tuple(sl)])
    return ok


def device_case(case, threads):
    """the differences of the device from the oracle, one line each; the kernel tallies are checked too"""
    level, kind, dia, (nrelax, erelax, minlevel), cycles = case
    side, bc = M.SIDE_KINDS[kind]
    a = M.cycle_arrays(3, level, kind, dia)
    expected = oracle_case(case)
    gd = gfship.Domain(3, level, side)
    bad = []
    try:
        gd.poisson_coefficients()
        u, rhs, dv, res = (gd.variable() for _ in range(4))
        u.upload(a["u"])
        rhs.upload(a["rhs"])
        for l in range(level + 1):
            if dia:
                dv.upload(a["dia"][l], l)
            else:
                dv.fill(0., l)
        for d in range(6):
            if bc[d] is not None:
                u.set_bc(d, bc[d], a["bc"][d])
        gd.bc(u)
        gd.residual(u, rhs, dv, res)
        par = gd.params()
        par.depth = level
        M.set_params(par, nrelax, erelax, minlevel)
        for k in range(cycles):
            gd.poisson_cycle(par, u, rhs, dv, res)
            eu, eres, ecoarse = expected[k]
            if not _face_ghosts_equal(eu, u.download()):
                bad.append("cycle %d: the solution differs" % k)
            if not np.array_equal(eres, res.download()[1:-1, 1:-1, 1:-1]):
                bad.append("cycle %d: the new residual differs" % k)
            for l, e in ecoarse.items():
                got = res.download(l)[1:-1, 1:-1, 1:-1]
                if not np.array_equal(e, got):
                    bad.append("cycle %d: the residual of level %d differs in %d cells"
                               % (k, l, int((e != got).sum())))
        kc = gd.kernel_counts()
        if kc["COARSE_CYCLES"] != cycles or kc["COARSE_END_BY_LEVEL"] != 0:
            bad.append("COARSE_CYCLES %d, COARSE_END_BY_LEVEL %d"
                       % (kc["COARSE_CYCLES"], kc["COARSE_END_BY_LEVEL"]))
        if kc["COARSE_THREADS"] != threads:
            bad.append("COARSE_THREADS %d, expected %d" % (kc["COARSE_THREADS"], threads))
    finally:
        gd.destroy()
    return bad


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_coarse_cycle_equals_the_oracle(case, monkeypatch):
    monkeypatch.delenv("GFSHIP_COARSE_THREADS", raising=False)
    bad = device_case(case, 1024)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("threads", THREADS)
def test_coarse_cycle_with_fewer_threads(threads):
    """a fresh process per thread count, one at a time"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("GFSHIP_") or k == "GFSHIP_LIB"}
    env["GFSHIP_COARSE_THREADS"] = str(threads)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(threads)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "exit status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    line = [x for x in r.stdout.splitlines() if x.startswith("COARSEWORKER ")][-1]
    bad = json.loads(line[len("COARSEWORKER "):])
    assert bad == {_id(c): [] for c in CHILD_CASES}, json.dumps(bad, indent=1)


if __name__ == "__main__":
    print("COARSEWORKER " + json.dumps({_id(c): device_case(c, int(sys.argv[1])) for c in CHILD_CASES}))
