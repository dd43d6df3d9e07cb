"""Registry of the GFSHIP_* environment switches and the cases that pin them on the oracle
(tests/test_gpu_switches.py, tests/switch_worker.py, tests/test_switch_registry_cpu.py).

Every switch is looked up when a Domain or a Tree is created (csrc/switches.hpp).  Each setting
still runs in a process of its own (switch_worker.py), so that a fault under one switch cannot take
the others with it, and the parent compares what it wrote with the oracle.  A case is one function
that drives either side the same way -- run_case (name, "oracle") on the CPU, run_case (name,
"device") in the worker -- and returns a flat {key: array or scalar}:
the state after the last step in full, the state after every earlier step as SHA-256 digests of
the same arrays (so the files stay small and every step is still compared bit for bit).

A switch names the cases it runs on and the *evidence* it must leave in the tallies of
gfship_domain_kernel_counts, summed over the domains of a case:
  on      families that must be > 0 under the switch and == 0 in the control run of the case,
  off     families for which the converse holds,
  values  families that hold a value: {family: (under the switch, in the control run)}.
Importable without a GPU."""
import ctypes as C
import hashlib

import numpy as np

from flow_cases import PERIODIC, oracle_lid, oracle_reynolds, oracle_taylor_green
from oracle import oracle as O

BOX = [O.SIDE_BOUNDARY] * 6
RTOL_SUM = 1e-12          # tests/test_gpu_fullsize.py: summed norms are tree-reduced on the device


# ---------------------------------------------------------------------------------------------
# what a run leaves behind
# ---------------------------------------------------------------------------------------------

def _digest(a):
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8).copy()


class _Record(dict):
    """{key: value}; arrays of the snapshots before the last are kept as digests (key + "#")"""

    def put(self, key, a, full):
        if np.ndim(a) == 0:
            self[key] = a
        elif full:
            self[key] = np.array(a, copy=True)
        else:
            self[key + "#"] = _digest(a)


def _inner(a, dim):
    return a[(slice(1, -1),) * dim]


def _un_faces(a, dim, n, c):
    """the faces normal to component c the reference owns (tests/test_gpu_timestep.py:_assert_same_un)"""
    sl = [slice(1, n + 1)] * dim
    sl[dim - 1 - c] = slice(0, n + 1)
    return a[tuple(sl)]


def _params(rec, tag, name, p):
    rec[tag + name + ".niter"] = int(p.niter)
    rec[tag + name + ".residual.infty"] = float(p.residual.infty)
    rec[tag + name + ".residual_before.infty"] = float(p.residual_before.infty)
    rec[tag + name + ".residual.first~"] = float(p.residual.first)      # "~": compared with RTOL_SUM
    rec[tag + name + ".residual.second~"] = float(p.residual.second)


def _flow_snapshot(rec, tag, side, sim, full, stepped=True, tracers=(), un=True, diffusion=False, coarse=False):
    """side "oracle": sim is an oracle.Sim; "device": a gfship.Simulation"""
    dim, depth = sim.dom.dim, sim.dom.depth
    n = 1 << depth
    if side == "oracle":
        leaf = lambda f: f.interior()                                   # noqa: E731
        below = lambda f: _inner(f.level(depth - 1), dim)           # noqa: E731
        face = lambda c: sim.un(2 * c)                                  # noqa: E731
    else:
        leaf = lambda f: _inner(f.download(), dim)                      # noqa: E731
        below = lambda f: _inner(f.download(depth - 1), dim)        # noqa: E731
        face = lambda c: sim.un(c)                                      # noqa: E731
    for c in range(dim):
        rec.put("%sU%d" % (tag, c), leaf(sim.u[c]), full)
        rec.put("%sg%d" % (tag, c), leaf(sim.g[c]), full)
        if un:
            rec.put("%sun%d" % (tag, c), _un_faces(face(c), dim, n, c), full)
        if coarse:       # gfs_cell_coarse_init inside the step (filled by the fused correction)
            rec.put("%sU%d.level%d" % (tag, c, depth - 1), below(sim.u[c]), full)
        if diffusion and stepped:      # no diffusion solve and no MAC projection before the first step
            _params(rec, tag, "diffusion%d" % c, sim.diffusion_params(c))
    rec.put(tag + "P", leaf(sim.p), full)
    rec.put(tag + "Pmac", leaf(sim.pmac), full)
    for k, t in enumerate(tracers):
        rec.put("%sT%d" % (tag, k), leaf(t), full)
    rec[tag + "dt"] = float(sim.dt)
    rec[tag + "t"] = float(sim.t)
    if stepped:
        _params(rec, tag, "projection", sim.projection_params)
    _params(rec, tag, "approx_projection", sim.approx_projection_params)


def _run_flow(rec, prefix, side, sim, nsteps, **what):
    sim.start()
    _flow_snapshot(rec, prefix + "start/", side, sim, False, stepped=False, **what)
    for k in range(nsteps):
        sim.step()
        _flow_snapshot(rec, "%sstep%d/" % (prefix, k), side, sim, k == nsteps - 1, **what)
    rec[prefix + "cfl"] = float(sim.cfl())
    nm = sim.divergence_norm()
    rec[prefix + "divergence.infty"] = float(nm.infty)
    rec[prefix + "divergence.second~"] = float(nm.second)


def _ghosted(a, dim):
    b = np.zeros(tuple(s + 2 for s in a.shape))
    b[(slice(1, -1),) * dim] = a
    return b


def _counts(domains):
    """tallies of gfship_domain_kernel_counts summed over the domains of a case (values: the largest)"""
    import gfship
    out = {}
    for gd in domains:
        for k, v in gd.kernel_counts().items():
            out[k] = max(out.get(k, 0), v) if k in gfship.KERNEL_COUNT_VALUES else out.get(k, 0) + v
    return out


class _Device:
    """the device side of a case: domains stay alive until the tallies have been read"""

    def __init__(self):
        self.domains, self.sims = [], []
        self.extra = {}

    def sim(self, osim, side):
        from test_gpu_timestep import _device_sim
        gd, gs = _device_sim(osim, side)
        self.domains.append(gd)
        self.sims.append(gs)
        return gd, gs

    def lid(self, osim, level, nu):
        from test_gpu_timestep import _device_lid
        gd, gs = _device_lid(osim, level, nu)
        self.domains.append(gd)
        self.sims.append(gs)
        return gd, gs


# ---------------------------------------------------------------------------------------------
# the flow cases
# ---------------------------------------------------------------------------------------------

def _tg(level, gradient, source, tracer):
    """Taylor-Green with a mean flow that gives upwind directions of both signs and faces of zero
    velocity (test_sweep_kernels_64_several_steps_vs_oracle)"""
    osim = oracle_taylor_green(level)
    osim.u[0].interior()[...] += 0.35
    osim.u[2].interior()[...] -= 0.2
    osim.advection_params.gradient = gradient
    T0 = None
    if tracer:
        x, y, z = osim.dom.centres()
        # a step profile: the van Leer limiter is active on both flanks, in every direction
        T0 = ((np.abs(x + 0.1) < 0.27) & (np.abs(y - 0.05) < 0.31) & (np.abs(z) < 0.22)) * 1. + \
            0.25 * np.sin(2. * np.pi * (x + 2. * y - z))
    return osim, T0


def _case_tg(level, gradient, source, tracer, nsteps):
    def run(side, dev):
        rec = _Record()
        osim, T0 = _tg(level, gradient, source, tracer)
        if side == "oracle":
            sim, tracers = osim, []
            if source:
                osim.set_source(1, source)
            if tracer:
                ot = osim.add_tracer()
                ot.interior()[...] = T0
                tracers = [ot]
        else:
            gd, sim = dev.sim(osim, PERIODIC)
            tracers = []
            if source:
                sim.set_source(1, source)
            if tracer:
                gt = sim.add_tracer()
                gt.upload(_ghosted(T0, 3))
                tracers = [gt]
        _run_flow(rec, "", side, sim, nsteps, tracers=tracers, coarse=True)
        return rec
    return run


def _viscous_box(level, nu):
    osim = O.Sim(3, level, BOX)
    n = 1 << level
    for c in range(3):
        for d in range(6):
            osim.u[c].set_bc(d, O.BC_DIRICHLET, np.full(n * n, 1. if (c == 0 and d == 2) else 0.))
        osim.set_viscosity(c, nu)
    return osim


def _case_visc64(side, dev):
    """the Dirichlet lid box of test_viscous_box_3d_steps_bit_exact and a viscous periodic
    Taylor-Green box, 64^3: the diffusion relax loops, advect_tiled_kernel with the viscous source"""
    rec = _Record()
    level, nu, nsteps = 6, 1e-2, 2
    osim = _viscous_box(level, nu)
    sim = osim if side == "oracle" else dev.lid(osim, level, nu)[1]
    _run_flow(rec, "lid/", side, sim, nsteps, un=False, diffusion=True)
    osim, _ = _tg(level, 1, 0., False)
    if side == "oracle":
        sim = osim
    else:
        sim = dev.sim(osim, PERIODIC)[1]
    for c in range(3):
        sim.set_viscosity(c, nu)
    _run_flow(rec, "periodic/", side, sim, nsteps, diffusion=True)
    return rec


class _NoDomain:
    """stands in for the device domain where only the oracle half of _alpha_faces is wanted"""

    class _V:
        def upload(self, a):
            pass

    def variable(self):
        return self._V()


def _case_alpha64(side, dev):
    """variable density (test_variable_density_steps_bit_exact): 3-D periodic 64^3 and closed box 32^3"""
    from flow_cases import taylor_green_3d
    from test_gpu_timestep import _alpha_faces
    rec = _Record()
    for kind, level in (("periodic", 6), ("box", 5)):
        sides = PERIODIC if kind == "periodic" else BOX
        osim = O.Sim(3, level, sides)
        x, y, z = osim.dom.centres()
        rng = np.random.default_rng(5)
        if kind == "periodic":
            vel = taylor_green_3d(x, y, z)
        else:
            vel = [np.sin(np.pi * (x + .5)) * np.cos(np.pi * (y + .5)) * np.cos(np.pi * (z + .5)),
                   -np.cos(np.pi * (x + .5)) * np.sin(np.pi * (y + .5)) * np.cos(np.pi * (z + .5)),
                   0. * x * y * z]
        for c in range(3):
            osim.u[c].interior()[...] = vel[c] + 0.01 * rng.standard_normal(np.shape(vel[c]))
        if side == "oracle":
            oa, _ = _alpha_faces(osim, _NoDomain(), kind)
            sim = osim
            sim.set_alpha(oa)
        else:
            gd, sim = dev.sim(osim, sides)
            _, ga = _alpha_faces(osim, gd, kind)
            sim.set_alpha(ga)
        _run_flow(rec, kind + "/", side, sim, 2)
    return rec


def _case_rows2d(side, dev):
    """2-D: Reynolds periodic 128^2 and the viscous lid 256^2 with Dirichlet walls, 3 steps each"""
    rec = _Record()
    osim = oracle_reynolds(7)
    if side == "oracle":
        sim = osim
    else:
        sim = dev.sim(osim, PERIODIC)[1]
        sim.set_time(end=2.)
    _run_flow(rec, "reynolds/", side, sim, 3)
    osim = oracle_lid(8, 1e-3)
    if side == "oracle":
        sim = osim
    else:
        sim = dev.lid(osim, 8, 1e-3)[1]
        sim.set_time(end=300.)
    _run_flow(rec, "lid/", side, sim, 3, diffusion=True)
    return rec


def _case_selfmpi64(side, dev):
    """test_rccl_transport_on_one_rank_reproduces_the_periodic_box at level 6: the sides of `axes' are
    GfsBoundaryMpi sides whose peer is the box itself; the oracle is the periodic single box"""
    import gfship
    rec = _Record()
    stats = {}
    for axes in ("xyz", "y"):
        osim = oracle_taylor_green(6)
        osim.u[0].interior()[...] += 0.3
        osim.u[1].interior()[...] -= 0.2
        if side == "oracle":
            sim = osim
        else:
            sides = [gfship.SIDE_EXTERNAL if "xyz"[d // 2] in axes else gfship.SIDE_PERIODIC
                     for d in range(6)]
            gd, sim = dev.sim(osim, sides)
            gd.comm_init(gfship.comm_unique_id(), 0, 1, (1, 1, 1))
        sim.set_source(1, -0.8)
        _run_flow(rec, axes + "/", side, sim, 2, un=False)
        if side == "device":
            cycles, fused = gd.path_counts()
            msgs, nbytes = gd.comm_stats()
            stats[axes] = dict(lattice_cycles=cycles, fused_mpi=fused, messages=msgs, bytes=nbytes)
    if side == "device":
        dev.extra["selfmpi"] = stats
    return rec


# ---------------------------------------------------------------------------------------------
# the multigrid cases: V-cycles and a solve on random fields, 128^3
# ---------------------------------------------------------------------------------------------

VCYCLE_SIDES = {
    "periodic": (PERIODIC, O.BC_SYMMETRY),
    "dirichlet": (BOX, O.BC_DIRICHLET),
    "mixed": ([O.SIDE_PERIODIC, O.SIDE_PERIODIC] + [O.SIDE_BOUNDARY] * 4, O.BC_NEUMANN),
}


def _faces(rec, key, a, dim, full):
    """interior and the face ghosts (edge and corner ghosts are not part of the reference's data)"""
    rec.put(key, _inner(a, dim), full)
    for ax in range(dim):
        for s in (0, -1):
            sl = [slice(1, -1)] * dim
            sl[ax] = s
            rec.put("%s.ghost%d%s" % (key, ax, "lo" if s == 0 else "hi"), a[tuple(sl)], full)


def _case_vcycle(kind, level=7):
    """two V-cycles, then a solve of three cycles, on random fields with random BC values, with
    dia == 0 and with a non-zero dia (test_fused_relax_loop_non_periodic_sides_bit_exact)"""
    def run(side, dev):
        import gfship
        rec = _Record()
        dim = 3
        sides, bck = VCYCLE_SIDES[kind]
        n = 1 << level
        for with_dia in (False, True):
            tag = "dia/" if with_dia else "nodia/"
            rng = np.random.default_rng(7000 + 10 * level + with_dia)
            shape = (n + 2,) * dim
            arrays = {nm: rng.standard_normal(shape) for nm in ("u", "rhs", "res")}
            dia = [np.abs(rng.standard_normal((((1 << l) + 2),) * dim)) * (0.3 if with_dia else 0.)
                   for l in range(level + 1)]
            vals = [rng.standard_normal(n * n) for _ in range(2 * dim)]
            if side == "oracle":
                L = O.lib()
                od = O.Domain(dim, level, sides)
                L.go_poisson_coefficients(od.ptr)
                f = {nm: od.field() for nm in arrays}
                f["dia"] = od.field()
                for nm, a in arrays.items():
                    f[nm].leaf()[...] = a
                for l in range(level + 1):
                    f["dia"].level(l)[...] = dia[l]
                if kind != "periodic":
                    for d in range(2 * dim):
                        f["u"].set_bc(d, bck, vals[d])
                L.go_bc(f["u"].ptr, f["u"].ptr, level)
                L.go_residual(od.ptr, dim, level, f["u"].ptr, f["rhs"].ptr, f["dia"].ptr, f["res"].ptr)
                par = od.params()
                par.depth = level
                get = lambda nm: f[nm].leaf()                                       # noqa: E731
                cycle = lambda: L.go_poisson_cycle(od.ptr, C.byref(par), f["u"].ptr, f["rhs"].ptr,   # noqa: E731
                                                   f["dia"].ptr, f["res"].ptr)
                solve = lambda p: L.go_poisson_solve(od.ptr, C.byref(p), f["u"].ptr, f["rhs"].ptr,   # noqa: E731
                                                     f["res"].ptr, f["dia"].ptr, 1.)
                newpar = od.params
            else:
                gd = gfship.Domain(dim, level, sides)
                dev.domains.append(gd)
                gd.poisson_coefficients()
                f = {nm: gd.variable() for nm in arrays}
                f["dia"] = gd.variable()
                for nm, a in arrays.items():
                    f[nm].upload(a)
                for l in range(level + 1):
                    if with_dia:
                        f["dia"].upload(dia[l], l)
                    else:
                        f["dia"].fill(0., l)
                if kind != "periodic":
                    for d in range(2 * dim):
                        f["u"].set_bc(d, bck, vals[d])
                gd.bc(f["u"])
                gd.residual(f["u"], f["rhs"], f["dia"], f["res"])
                par = gd.params()
                par.depth = level
                get = lambda nm: f[nm].download()                                   # noqa: E731
                cycle = lambda: gd.poisson_cycle(par, f["u"], f["rhs"], f["dia"], f["res"])   # noqa: E731
                solve = lambda p: gd.poisson_solve(p, f["u"], f["rhs"], f["res"], f["dia"], 1.)   # noqa: E731
                newpar = gd.params
            for k in range(2):
                cycle()
                _faces(rec, "%scycle%d/u" % (tag, k), get("u"), dim, False)
                rec.put("%scycle%d/res" % (tag, k), _inner(get("res"), dim), False)
            p = newpar()
            p.tolerance, p.nitermin, p.nitermax = 1e-30, 3, 3
            solve(p)
            _faces(rec, tag + "solve/u", get("u"), dim, True)
            rec.put(tag + "solve/res", _inner(get("res"), dim), True)
            _params(rec, tag + "solve/", "params", p)
        return rec
    return run


CASES = {
    # name: (function (side, device) -> record, cells of the largest level, time limit of the device half [s])
    "tg64_vl_src": (_case_tg(6, 1, -0.7, False, 3), 64 ** 3),
    "tg64_centred": (_case_tg(6, 0, 0., False, 3), 64 ** 3),
    "tg64_tracer": (_case_tg(6, 1, -0.7, True, 3), 64 ** 3),
    "tg128": (_case_tg(7, 1, 0., False, 2), 128 ** 3),
    "visc64": (_case_visc64, 64 ** 3),
    "alpha64": (_case_alpha64, 64 ** 3),
    "vcycle128_periodic": (_case_vcycle("periodic"), 128 ** 3),
    "vcycle128_dirichlet": (_case_vcycle("dirichlet"), 128 ** 3),
    "vcycle128_mixed": (_case_vcycle("mixed"), 128 ** 3),
    "rows2d": (_case_rows2d, 256 ** 2),
    "selfmpi64": (_case_selfmpi64, 64 ** 3),
}
# the oracle half of these runs in the suite without a GPU as well (the others on the GPU box only)
CPU_CASES = [c for c, (_, cells) in CASES.items() if cells <= 64 ** 3]


def run_case(name, side):
    """-> (record, tallies, extra); tallies and extra are {} on the oracle side"""
    fn = CASES[name][0]
    if side == "oracle":
        return fn("oracle", None), {}, {}
    dev = _Device()
    rec = fn("device", dev)
    counts = _counts(dev.domains)
    for gs in dev.sims:
        gs.destroy()
    for gd in dev.domains:
        gd.destroy()
    return rec, counts, dev.extra


# ---------------------------------------------------------------------------------------------
# the switches
# ---------------------------------------------------------------------------------------------

def E(on=(), off=(), values=None):
    return dict(on=tuple(on), off=tuple(off), values=dict(values or {}))


TG64 = ("tg64_vl_src", "tg64_centred", "tg64_tracer")
VC128 = ("vcycle128_periodic", "vcycle128_dirichlet", "vcycle128_mixed")


def _sw(env, evidence, cases, **per_case):
    """cases: names that use `evidence'; per_case: name = evidence of its own"""
    m = {c: evidence for c in cases}
    m.update(per_case)
    return dict(env={"GFSHIP_" + k: v for k, v in env.items()}, cases=m)


_TILED = E(on=("PREDICT_TILED", "ADVECT3_TILED"), off=("PREDICT_SWEEP", "ADVECT3_SWEEP2"))
_TILED_MPI = E(on=("PREDICT_TILED_MPI", "ADVECT3_TILED_MPI"), off=("PREDICT_SWEEP_MPI", "ADVECT3_SWEEP2_MPI"))
_PC = E(on=("PROJECT_SCALAR",), off=("PROJECT_PAIRS",))
_RN = E(on=("RESIDUAL_SCALAR",), off=("RESIDUAL_PAIRS",))

SWITCHES = {
    "default": _sw({}, E(), list(CASES)),
    # --- Godunov kernels
    "NO_ADVECT_SWEEP": _sw({"NO_ADVECT_SWEEP": "1"}, _TILED, TG64 + ("tg128",),
                           # viscous: the components are advected one by one on either path
                           visc64=E(on=("PREDICT_TILED",), off=("PREDICT_SWEEP",)),
                           selfmpi64=_TILED_MPI),
    "ADVECT_SWEEP1": _sw({"ADVECT_SWEEP1": "1"}, E(on=("ADVECT3_SWEEP1",), off=("ADVECT3_SWEEP2",)), TG64),
    "NO_ADVECT3": _sw({"NO_ADVECT3": "1"},
                      E(on=("ADVECT1_TILED_VELOCITY",), off=("ADVECT3_SWEEP2", "CORRECTION_FUSED")), TG64),
    "NO_FUSED_CORRECTION": _sw({"NO_FUSED_CORRECTION": "1"},
                               E(on=("CORRECTION_DECLINED",), off=("CORRECTION_FUSED",)), TG64),
    "NO_FUSED_DIVERGENCE": _sw({"NO_FUSED_DIVERGENCE": "1"},
                               E(on=("DIVERGENCE_DECLINED", "DIVERGENCE_SEPARATE"), off=("DIVERGENCE_FUSED",)),
                               TG64),
    "NO_ADVECT_SWEEP+NO_FUSED_CORRECTION": _sw(
        {"NO_ADVECT_SWEEP": "1", "NO_FUSED_CORRECTION": "1"},
        E(on=("PREDICT_TILED", "ADVECT3_TILED", "CORRECTION_DECLINED"),
          off=("PREDICT_SWEEP", "ADVECT3_SWEEP2", "CORRECTION_FUSED")), ("tg64_vl_src",)),
    "NO_ADVECT_SWEEP+NO_ADVECT3": _sw(
        {"NO_ADVECT_SWEEP": "1", "NO_ADVECT3": "1"},
        E(on=("PREDICT_TILED", "ADVECT1_TILED_VELOCITY"), off=("PREDICT_SWEEP", "ADVECT3_SWEEP2")),
        ("tg64_vl_src",)),
    # --- two cells per thread against one
    "PC_SCALAR": _sw({"PC_SCALAR": "1"}, _PC, ("tg64_vl_src", "tg128"),
                     # no projection in a V-cycle: nothing to select, the bits are still compared
                     **{c: E() for c in VC128}),
    "RN_SCALAR": _sw({"RN_SCALAR": "1"}, _RN, ("tg64_vl_src", "tg128") + VC128),
    "RN_BLOCKS=64": _sw({"RN_BLOCKS": "64"}, E(values={"RN_BLOCKS_LIMIT": (64, 4096), "RN_BLOCKS_MAX": (64, 4096)}),
                        ("tg128",) + VC128,
                        tg64_vl_src=E(values={"RN_BLOCKS_LIMIT": (64, 4096), "RN_BLOCKS_MAX": (64, 512)})),
    # the limit is read, but with two cells per thread 128^3 needs 4096 workgroups: the grid only
    # changes from 256^3 on ...
    "RN_BLOCKS=8192": _sw({"RN_BLOCKS": "8192"},
                          E(values={"RN_BLOCKS_LIMIT": (8192, 4096), "RN_BLOCKS_MAX": (4096, 4096)}),
                          ("tg128",) + VC128,
                          tg64_vl_src=E(values={"RN_BLOCKS_LIMIT": (8192, 4096), "RN_BLOCKS_MAX": (512, 512)})),
    # ... so the larger grid is reached with the one-cell kernel (one workgroup per row, 128^2 rows)
    "RN_SCALAR+RN_BLOCKS=8192": _sw({"RN_SCALAR": "1", "RN_BLOCKS": "8192"},
                                    E(on=("RESIDUAL_SCALAR",), off=("RESIDUAL_PAIRS",),
                                      values={"RN_BLOCKS_LIMIT": (8192, 4096), "RN_BLOCKS_MAX": (8192, 4096)}),
                                    VC128),
    # --- the multigrid cycle
    "NO_FUSED_PROLONGATION": _sw({"NO_FUSED_PROLONGATION": "1"},
                                 E(on=("PROLONGATION_DECLINED",),
                                   off=("PROLONGATION_FUSED", "PROLONG_PACK_NEW", "RESTRICTION_FUSED")),
                                 VC128 + ("tg128",)),
    "NO_FUSED_RESTRICTION": _sw({"NO_FUSED_RESTRICTION": "1"},
                                E(on=("RESTRICTION_DECLINED",), off=("RESTRICTION_FUSED",)), VC128 + ("tg128",)),
    "OLD_PROLONG_PACK": _sw({"OLD_PROLONG_PACK": "1"},
                            E(on=("PROLONG_PACK_OLD",), off=("PROLONG_PACK_NEW",)), VC128 + ("tg128",)),
    "NO_ARM_AHEAD": _sw({"NO_ARM_AHEAD": "1"},
                        E(on=("ARM_AHEAD_DECLINED",), off=("ARM_AHEAD",)), VC128 + ("tg128",)),
    "KERNEL_ARMING": _sw({"KERNEL_ARMING": "1"},
                         E(on=("PATCH_LOOP_KERNEL_ARMS",), off=("PATCH_LOOP_HOST_ARMS",)), VC128 + ("tg128",)),
    "XCD_SCOPE+NEAR_MODE=0": _sw({"XCD_SCOPE": "1", "XCD_NEAR_MODE": "0"},
                                 E(on=("XCD_SCOPE_ON",), off=("XCD_SCOPE_OFF",), values={"XCD_NEAR_MODE": (1, 0)}),
                                 VC128 + ("tg128",)),
    "XCD_SCOPE+NEAR_MODE=1": _sw({"XCD_SCOPE": "1", "XCD_NEAR_MODE": "1"},
                                 E(on=("XCD_SCOPE_ON",), off=("XCD_SCOPE_OFF",), values={"XCD_NEAR_MODE": (2, 0)}),
                                 VC128 + ("tg128",)),
    "XCD_SCOPE+NEAR_MODE=2": _sw({"XCD_SCOPE": "1", "XCD_NEAR_MODE": "2"},
                                 E(on=("XCD_SCOPE_ON",), off=("XCD_SCOPE_OFF",), values={"XCD_NEAR_MODE": (3, 0)}),
                                 VC128 + ("tg128",)),
    "XCD_PLACE": _sw({"XCD_PLACE": "1"}, E(on=("XCD_PLACE_ON",), off=("XCD_PLACE_OFF",)), VC128 + ("tg128",)),
    "COARSE_THREADS=256": _sw({"COARSE_THREADS": "256"}, E(values={"COARSE_THREADS": (256, 1024)}),
                              VC128 + ("tg128",)),
    # --- sweeps by hyperplanes
    "DIFFUSION_HYPERPLANES": _sw({"DIFFUSION_HYPERPLANES": "1"},
                                 E(on=("DIFFUSION_HYPERPLANES",), off=("DIFFUSION_PIPELINED",)), ("visc64",)),
    "WEIGHTED_HYPERPLANES": _sw({"WEIGHTED_HYPERPLANES": "1"},
                                E(on=("WEIGHTED_HYPERPLANES",), off=("WEIGHTED_PIPELINED",)), ("alpha64",)),
    "NO_ROWS2D": _sw({"NO_ROWS2D": "1"}, E(on=("HYPERPLANES_2D",), off=("ROWS2D",)), ("rows2d",)),
    # --- a box with GfsBoundaryMpi sides
    "NO_MPI_SWEEP": _sw({"NO_MPI_SWEEP": "1"}, _TILED_MPI, ("selfmpi64",)),
    "NO_FUSED_MPI": _sw({"NO_FUSED_MPI": "1"},
                        E(on=("PREDICT_GENERAL", "ADVECT_GENERAL"), off=("PREDICT_SWEEP_MPI", "ADVECT3_SWEEP2_MPI")),
                        ("selfmpi64",)),
    "NO_LATTICE_CYCLE": _sw({"NO_LATTICE_CYCLE": "1"}, E(on=("COARSE_END_BY_LEVEL",)), ("selfmpi64",)),
}

# the variables of the registry
REGISTRY_NAMES = sorted({k for s in SWITCHES.values() for k in s["env"]})

# read by the sources, but not pinned here: name -> why
NOT_KERNEL_SELECTING = {
    "GFSHIP_SKEW_STATS": "prints per-tile timings of the relax loops to stderr; selects nothing",
    "GFSHIP_TREE_DEBUG": "prints the plans of the refined-tree solver to stderr; selects nothing",
    "GFSHIP_RCCL_LIBRARY": "names the RCCL shared object to open (tests/test_gpu_mock_rccl.py uses it)",
    "GFSHIP_CC": "the C compiler the front end runs on GfsFunction expressions (host side)",
    "GFSHIP_FAULT_DROP_HANDOFF": "fault injection for the relax loop's hang detector (tests/test_gpu_poisson.py); selects no kernel",
    "GFSHIP_DIST_BACKEND": "transport of bench.py's multi-rank run (RCCL or host-staged gloo); host side",
    "GFSHIP_LIB": "path of the libgfship.so the python package loads",
    "GFSHIP_NO_TORCH": "keeps the python package from importing torch before the library is loaded",
}
# of these, the loader's own settings stay in the environment of a worker (it must load the library
# the parent tests); every other GFSHIP_* variable the caller's shell may hold is stripped
KEEP_IN_CHILD = ("GFSHIP_LIB", "GFSHIP_NO_TORCH")
# kernel-selecting, pinned elsewhere: name -> file
PINNED_ELSEWHERE = {
    "GFSHIP_SKEW_OLD": "tests/test_gpu_poisson.py",
    "GFSHIP_SKEW_LINES": "tests/test_gpu_poisson.py",
    "GFSHIP_WAVE_LOOP": "tests/test_gpu_poisson.py",
    "GFSHIP_PATCH_REGS": "tests/test_gpu_poisson.py",
    "GFSHIP_PATCH_MIN_N": "tests/test_gpu_poisson.py",
    "GFSHIP_NO_LAZY_UN": "tests/test_gpu_timestep.py",
    "GFSHIP_FLOW_WIDTH": "tests/test_gpu_tree.py",
    "GFSHIP_TREE_NO_RESIDUAL_TAPE": "tests/test_gpu_tree.py",
    "GFSHIP_TREE_TEMPLATE_RELAX": "tests/test_gpu_tree.py",
    "GFSHIP_TREE_NO_PIPELINE": "tests/test_gpu_tree.py",
    "GFSHIP_TREE_NO_FLOW": "tests/test_gpu_tree.py",
    "GFSHIP_TREE_NO_PREFETCH": "tests/test_gpu_tree.py",
}

def child_timeout(switch):
    """time limit of the worker of a switch [s]: start-up plus a generous allowance per case (uploads
    and downloads of 128^3 fields dominate; the hyperplane variants launch ~200 kernels per sweep)"""
    return 120 + 60 * len(SWITCHES[switch]["cases"])
