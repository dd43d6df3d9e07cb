"""Domains of several GfsBoxes on the CPU (no GPU): the oracle with GfsBoundaryMpi sides, several
boxes per process (one thread per box, tests/multibox.py) and one box per process over gloo.

Every box holds ITS part of a field defined on the whole lattice (nothing is a copy or a mirror
image of anything else), and the checks use the lattice geometry only:
  * after a BC application every ghost layer equals the layer of the GLOBAL array next to it;
  * a converged multi-box Poisson solve satisfies the discrete equations of the WHOLE periodic
    grid (a wrong peer, a swapped side or a transposed face would solve another problem);
  * the reference's two cell orders of a parallel relax loop (domain parameter overlap = 0 and the
    default overlap = 1: cells along MPI sides first, src/domain.c:1093-1125) give different
    iterates of the same solution;
  * two processes over gloo (the transport bench.py's rehearsal uses) reproduce the threads bit
    for bit.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "gerris-fft-particles_amd"))
from gfship import distributed as D   # noqa: E402
import multibox as M                  # noqa: E402
from oracle import oracle as O        # noqa: E402


def _global_random(grid, n, seed):
    rng = np.random.default_rng(seed)
    b = grid.b
    return rng.standard_normal((b[2] * n, b[1] * n, b[0] * n))


def _part(grid, rank, G, n):
    cx, cy, cz = grid.coords(rank)
    return G[cz * n:(cz + 1) * n, cy * n:(cy + 1) * n, cx * n:(cx + 1) * n]


SHAPES = [(1, 1, 2), (1, 2, 1), (1, 2, 2), (2, 1, 2)]     # lattices that doubling along x first never gives


def _shape_id(b):
    return "%dx%dx%d" % tuple(b)


@pytest.mark.parametrize("nboxes", [2, 4, 8] + [pytest.param(b, id=_shape_id(b)) for b in SHAPES])
def test_ghost_layers_come_from_the_geometric_neighbour(nboxes):
    level = 3
    n = 1 << level
    if isinstance(nboxes, tuple):
        grid = M.ShapedGrid(nboxes)
        nboxes = grid.n
        G = _global_random(grid, n, 7 + 100 * grid.b[0] + 10 * grid.b[1] + grid.b[2])
    else:
        grid = D.BoxGrid(nboxes, 3)
        G = _global_random(grid, n, 7 + nboxes)
    L = O.lib()

    def worker(rank, fabric):
        dom = O.Domain(3, level, grid.sides(rank))
        hooks = M.OracleHooks(L, dom.ptr, 3, M.LocalTransport(grid, rank, fabric))
        f = dom.field()
        f.interior()[...] = _part(grid, rank, G, n)
        L.go_bc(f.ptr, f.ptr, level)
        a = f.leaf().copy()
        del hooks
        return a

    out = M.run_boxes(nboxes, worker)
    b = grid.b
    for rank in range(nboxes):
        cx, cy, cz = grid.coords(rank)
        a = out[rank]
        # the box with its ghost layers, cut out of the periodic global array
        kk = np.arange(cz * n - 1, (cz + 1) * n + 1) % (b[2] * n)
        jj = np.arange(cy * n - 1, (cy + 1) * n + 1) % (b[1] * n)
        ii = np.arange(cx * n - 1, (cx + 1) * n + 1) % (b[0] * n)
        want = G[np.ix_(kk, jj, ii)]
        for ax in range(3):
            for s in (0, -1):
                sl = [slice(1, -1)] * 3
                sl[ax] = s
                assert np.array_equal(a[tuple(sl)], want[tuple(sl)]), (rank, ax, s)


@pytest.mark.parametrize("b", SHAPES + [(2, 2, 2)], ids=_shape_id)
def test_shaped_grid_neighbours_follow_the_rank_formula_of_the_transport(b):
    """rank r sits at (r % bx, (r / bx) % by, r / (bx by)) (struct Comm, csrc/transport.hip); the box
    across side d is one step along axis d / 2, + for even d, on the periodic lattice"""
    bx, by, bz = b
    grid = M.ShapedGrid(b)
    assert grid.n == bx * by * bz and grid.b == tuple(b)
    assert grid.external_sides() == [d for d in range(6) if b[d // 2] > 1]
    for r in range(grid.n):
        c = [r % bx, (r // bx) % by, r // (bx * by)]
        assert grid.coords(r) == tuple(c) and grid.rank_of(c) == r
        assert grid.sides(r) == [D.SIDE_EXTERNAL if b[d // 2] > 1 else D.SIDE_PERIODIC for d in range(6)]
        for d in range(6):
            cc = list(c)
            cc[d // 2] += -1 if d & 1 else 1
            cc = [(x % m + m) % m for x, m in zip(cc, b)]
            assert grid.neighbour(r, d) == cc[0] + bx * (cc[1] + by * cc[2]), (r, d)
            assert grid.neighbour(grid.neighbour(r, d), d ^ 1) == r


def test_shaped_grid_refuses_what_is_no_lattice():
    for b in ((2, 2), (0, 1, 1), (2, 1, 1, 1)):
        with pytest.raises(ValueError):
            M.ShapedGrid(b)
    with pytest.raises(ValueError):
        M.ShapedGrid((2, 1, 2), dim=2)


def _solve_boxes(nboxes, level, overlap, cycles, tolerance=1e-30):
    n = 1 << level
    grid = D.BoxGrid(nboxes, 3)
    G = _global_random(grid, n, 99)
    G -= G.mean()
    L = O.lib()

    def worker(rank, fabric):
        dom = O.Domain(3, level, grid.sides(rank))
        dom.set_overlap(overlap)
        hooks = M.OracleHooks(L, dom.ptr, 3, M.LocalTransport(grid, rank, fabric))
        P, rhs, res, dia = (dom.field() for _ in range(4))
        rhs.interior()[...] = _part(grid, rank, G, n)
        L.go_bc(P.ptr, P.ptr, level)
        L.go_poisson_coefficients(dom.ptr)
        par = dom.params()
        par.tolerance, par.nitermin, par.nitermax = tolerance, cycles, cycles
        L.go_poisson_solve(dom.ptr, C.byref(par), P.ptr, rhs.ptr, res.ptr, dia.ptr, 1.)
        out = (P.interior().copy(), par.residual.infty, par.niter)
        del hooks
        return out

    out = M.run_boxes(nboxes, worker)
    return grid, G, out


@pytest.mark.parametrize("nboxes,overlap", [(2, 0), (8, 0), (8, 1)])
def test_converged_multibox_solve_satisfies_the_global_equations(nboxes, overlap):
    level = 3
    n = 1 << level
    grid, G, out = _solve_boxes(nboxes, level, overlap, 60)
    # every box sees the same all-reduced norm
    assert len({o[1] for o in out}) == 1
    P = M.assemble(grid, [o[0] for o in out], n)
    lap = sum(np.roll(P, s, ax) for ax in range(3) for s in (1, -1)) - 6. * P
    assert np.abs(G - lap).max() < 1e-9 * np.abs(G).max()
    # MPI_Allreduce (max) of the residual agrees with the global residual (scaled by h^2)
    assert out[0][1] == pytest.approx(np.abs(G - lap).max() * n * n, rel=1e-6, abs=1e-9)


def test_overlap_order_changes_the_iterates_not_the_solution():
    grid, G, a = _solve_boxes(8, 3, 0, 2)
    _, _, b = _solve_boxes(8, 3, 1, 2)
    Pa, Pb = M.assemble(grid, [o[0] for o in a], 8), M.assemble(grid, [o[0] for o in b], 8)
    assert not np.array_equal(Pa, Pb)           # different cell order: different iterates
    assert np.abs(Pa - Pb).max() < 0.1 * np.abs(Pa).max()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("overlap", [0, 1])
def test_two_ranks_over_gloo_equal_two_threads_on_the_lattice_field(tmp_path, overlap):
    """non-identical boxes: a flow with one period over the 2 x 1 x 1 lattice, two time steps"""
    level, nsteps = 3, 2
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(29581 + overlap),
           os.path.join(ROOT, "tests", "dist_worker.py"), str(tmp_path), str(level), str(nsteps),
           "lattice", str(overlap)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ref = run_lattice_flow_threads(2, level, nsteps, overlap)
    for rank in range(2):
        d = np.load(os.path.join(str(tmp_path), "rank%d.npz" % rank))
        for name in ("u", "v", "w", "p"):
            assert np.array_equal(d[name], ref[rank][name]), (rank, name)
        assert float(d["dt"]) == ref[rank]["dt"] and float(d["t"]) == ref[rank]["t"]
    # the two boxes really differ
    assert not np.array_equal(ref[0]["u"], ref[1]["u"])


def lattice_flow_state(sim, n, depth, un, interior, coarse):
    """what the lattice tests compare of one box, oracle or device alike: un (c) the MAC velocities of
    component c with ghosts, interior (f) / coarse (f) the leaf cells / level depth - 1 of a field"""
    st = dict(u=interior(sim.u[0]), v=interior(sim.u[1]), w=interior(sim.u[2]), p=interior(sim.p),
              dt=sim.dt, t=sim.t, g=[interior(sim.g[c]) for c in range(3)], pmac=interior(sim.pmac),
              niter=(sim.projection_params.niter, sim.approx_projection_params.niter),
              res=sim.approx_projection_params.residual.infty)
    # the faces with tangential coordinates in 1..n and normal coordinate in 0..n (_assert_same_un of
    # tests/test_gpu_timestep.py): face 0 along an MPI side is the one shared with the neighbour box
    st["un"] = []
    for c in range(3):
        sl = [slice(1, n + 1)] * 3
        sl[2 - c] = slice(0, n + 1)
        st["un"].append(np.array(un(c)[tuple(sl)]))
    st["coarse"] = [coarse(sim.u[c]) for c in range(3)]
    return st


def run_lattice_flow_threads(nboxes, level, nsteps, overlap, tolerance=None, grid=None, gradient=None,
                             source=None, visc=0., per_step=False):
    """the oracle on a lattice of boxes, one thread per box: state of every box after nsteps.
    grid: the lattice (default: nboxes doubled along x, y, z in turn); gradient: of the velocity
    advection (0 centred, 1 van Leer); source = (component, value): GfsSource; visc: SourceDiffusion on
    U, V, W; per_step: the list of states after the start-up and after every step instead"""
    n = 1 << level
    if grid is None:
        grid = D.BoxGrid(nboxes, 3)
    assert grid.n == nboxes
    L = O.lib()

    def worker(rank, fabric):
        sim = O.Sim(3, level, grid.sides(rank))
        sim.dom.set_overlap(overlap)
        hooks = M.OracleHooks(L, sim.dom.ptr, 3, M.LocalTransport(grid, rank, fabric))
        X, Y, Z = M.global_centres(grid, rank, n)
        for c, a in enumerate(M.lattice_velocity(X, Y, Z)):
            sim.u[c].interior()[...] = a
        if tolerance is not None:
            sim.projection_params.tolerance = tolerance
            sim.approx_projection_params.tolerance = tolerance
        if gradient is not None:
            sim.advection_params.gradient = gradient
        if source is not None:
            sim.set_source(*source)
        if visc:
            for c in range(3):
                sim.set_viscosity(c, visc)

        def state():
            return lattice_flow_state(sim, n, level, lambda c: sim.un(2 * c), lambda f: f.interior().copy(),
                                      lambda f: f.interior(level - 1).copy())

        sim.start()
        states = [state()] if per_step else []
        for _ in range(nsteps):
            sim.step()
            if per_step:
                states.append(state())
        out = states if per_step else state()
        del hooks
        return out

    return M.run_boxes(nboxes, worker)


def test_lattice_flow_threads_options():
    """per_step ends on the state the plain call returns; gradient, source and viscosity reach the
    oracle (each changes the flow); a lattice split along z alone runs and differs from the one along x"""
    level, nsteps = 3, 2
    n = 1 << level
    plain = run_lattice_flow_threads(2, level, nsteps, 0)
    steps = run_lattice_flow_threads(2, level, nsteps, 0, per_step=True)
    assert [len(s) for s in steps] == [nsteps + 1] * 2
    for rank in range(2):
        a, b = plain[rank], steps[rank][-1]
        assert set(a) == set(b) >= {"u", "v", "w", "p", "pmac", "g", "dt", "t", "niter", "res", "un", "coarse"}
        for name in ("u", "v", "w", "p", "pmac"):
            assert np.array_equal(a[name], b[name]) and a[name].shape == (n,) * 3
        for c in range(3):
            assert np.array_equal(a["un"][c], b["un"][c]) and np.array_equal(a["coarse"][c], b["coarse"][c])
            assert a["coarse"][c].shape == (n // 2,) * 3
            sh = [n] * 3
            sh[2 - c] = n + 1
            assert a["un"][c].shape == tuple(sh)
        assert a["t"] == b["t"] and steps[rank][0]["t"] == 0. and steps[rank][1]["t"] < b["t"]
        # the MAC velocity of the face shared by the two boxes: both hold it (x: + face of box 0 is
        # face 0 of box 1 and the other way round, the lattice being periodic)
        assert np.array_equal(plain[rank]["un"][0][:, :, n], plain[rank ^ 1]["un"][0][:, :, 0])
    for kw in (dict(gradient=1), dict(source=(1, -0.8)), dict(visc=2e-3)):
        other = run_lattice_flow_threads(2, level, nsteps, 0, **kw)
        assert not np.array_equal(other[0]["v"], plain[0]["v"]), kw
    z = run_lattice_flow_threads(2, level, nsteps, 0, grid=M.ShapedGrid((1, 1, 2)))
    assert not np.array_equal(z[0]["u"], plain[0]["u"])
    assert np.array_equal(z[0]["un"][2][n], z[1]["un"][2][0])


def test_multibox_flow_approaches_the_single_box_flow_of_the_whole_grid():
    """2 x 2 x 2 boxes of 8^3 against ONE periodic box of 16^3 holding the same global field: the
    partition changes the iterates of the multigrid (lagged ghosts, no level above the boxes), not
    the equations: with tight projection tolerances the velocities agree to solver accuracy"""
    level, nsteps = 3, 2
    n = 1 << level
    grid = D.BoxGrid(8, 3)
    parts = run_lattice_flow_threads(8, level, nsteps, 0, tolerance=1e-9)
    one = O.Sim(3, level + 1, [O.SIDE_PERIODIC] * 6)
    c = (np.arange(2 * n) + 0.5) / (2 * n)
    X, Y, Z = c[None, None, :], c[None, :, None], c[:, None, None]
    # the single box is the unit cube, the lattice boxes are unit cubes too (twice the physical
    # size of its cells): the same cell values with h halved means velocities scale by 1/2 to
    # keep u dt / h, i.e. the same discrete problem
    for cc, a in enumerate(M.lattice_velocity(X, Y, Z)):
        one.u[cc].interior()[...] = a / 2.
    one.projection_params.tolerance = 1e-9
    one.approx_projection_params.tolerance = 1e-9
    one.start()
    for _ in range(nsteps):
        one.step()
    assert parts[0]["dt"] == pytest.approx(one.dt, rel=1e-7)
    for name, f in (("u", one.u[0]), ("v", one.u[1]), ("w", one.u[2])):
        Gm = M.assemble(grid, [p[name] for p in parts], n)
        assert np.abs(Gm / 2. - f.interior()).max() < 1e-7, name
