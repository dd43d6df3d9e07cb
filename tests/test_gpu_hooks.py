"""The solver hooks of the C ABI (include/gfship.h: "the pieces, callable on their own"), one by one and
in mixed order, against their twins of the CPU oracle -- bit for bit, in EVERY variable.

gfship_sim_step does not run the public pieces: it runs internal variants with fused kernels and state
that a simulation carries between calls (MAC velocities left unstored, leaf storage swapped with
scratch arrays, maxima kept for the CFL condition).  What a Gerris maintainer binds
 are the pieces; these tests call them:

  1. test_hook_*: both sides brought to the same state by upload, ONE hook on each side, then every
     variable compared (leaves, ghost cells across the faces, the MAC velocities, dt, t, i, the
     statistics of the projections, and the non-leaf levels where the hook fills them);
  2. test_steps_*: four steps three ways -- gfship_sim_step, the loop body of simulation_run written
     from the pieces through the ABI (hook_cases.pieces_step; the sequence itself is pinned on the
     oracle alone by tests/test_hooks_recipe_cpu.py), go_sim_step -- and the two device styles
     alternating step by step;
  3. test_after_lazy_steps_* and below: the state between calls.  The expected result always comes
     from the oracle doing the same calls in the same order (it has no hidden state).

Entry points of the time-step section of the header and where they are called here (through the
wrappers of gfship.Simulation): gfship_predicted_face_velocities, gfship_mac_projection,
gfship_approximate_projection, gfship_centered_velocity_advection,
gfship_correct_centered_velocities, gfship_tracer_advection, gfship_domain_cfl, gfship_set_timestep,
gfship_coarse_init, gfship_sim_advance_time (HOOKS / pieces_step); gfship_diffusion_residual,
gfship_diffusion_cycle (test_diffusion_pieces); gfship_field_device_ptr, gfship_field_fill
(test_writes_between_steps, test_device_ptr_*); gfship_sim_set_next_event (the "event" cases).

Comparison is np.array_equal throughout; the one tolerance is RTOL_SUM = 1e-12 for the tree-reduced
norm sums of the GfsMultilevelParams statistics (max norms exact), as in tests/test_gpu_poisson.py.
"""
import ctypes as C

import numpy as np
import pytest

import gfship
import hook_cases as H
from hook_cases import Case
from oracle import oracle as O

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# 1. each hook on its own
# ---------------------------------------------------------------------------------------------

def _tracers(sim, dt):
    for t in sim.hook_tracers:
        sim.tracer_advection(t, dt)


# name -> the call, on an oracle.Sim or a gfship.Simulation; the value returned is compared too
HOOKS = {
    "predicted_face_velocities": lambda s: s.predicted_face_velocities(),
    # as simulation_run calls it: on Pmac's field, time step dt/2, gradient into gmac
    "mac_projection": lambda s: s.mac_projection(s.projection_params, s.dt / 2., s.pmac, s.gmac),
    "approximate_projection": lambda s: s.approximate_projection(s.approx_projection_params, s.dt, s.p, s.g),
    "centered_velocity_advection": lambda s: s.centered_velocity_advection(s.gmac, s.g),
    # the first iteration of the loop: g = gmac
    "centered_velocity_advection_gmac": lambda s: s.centered_velocity_advection(s.gmac, s.gmac),
    "correct_centered_velocities": lambda s: s.correct_centered_velocities(s.g, - s.dt),
    "tracer_advection_dt": lambda s: _tracers(s, s.dt),
    "tracer_advection_halfdt": lambda s: _tracers(s, s.dt / 2.),
    "domain_cfl": lambda s: s.cfl(),
    "set_timestep": lambda s: s.set_timestep(),
    "coarse_init": lambda s: s.coarse_init(),
}

STEP_HOOKS = ["predicted_face_velocities", "mac_projection", "approximate_projection",
              "centered_velocity_advection", "correct_centered_velocities", "domain_cfl", "set_timestep",
              "coarse_init"]
KERNEL_HOOKS = ["predicted_face_velocities", "mac_projection", "centered_velocity_advection"]
TRACER_HOOKS = ["tracer_advection_dt", "tracer_advection_halfdt", "coarse_init"]

# (case, hooks): every value of every axis (dimension and level, sides, gradient, viscosity, source,
# alpha, tracers, events) meets every hook it can change; levels 3 and 4 in 3-D take the general
# kernels (n % 32 != 0), 5 and 6 the fused Godunov / sweep kernels where the box is periodic
HOOK_CASES = [
    (Case(2, 3), STEP_HOOKS + ["centered_velocity_advection_gmac"]),
    (Case(2, 5), STEP_HOOKS + ["centered_velocity_advection_gmac"]),
    (Case(2, 5, gradient=1), KERNEL_HOOKS),
    (Case(2, 5, gradient=2), KERNEL_HOOKS),
    (Case(2, 5, "lid"), STEP_HOOKS),
    (Case(2, 5, "lid", visc=1e-2), STEP_HOOKS),
    (Case(2, 5, "symmetry"), STEP_HOOKS),
    (Case(2, 5, "symmetry", source=0.7), KERNEL_HOOKS + ["domain_cfl", "set_timestep"]),
    (Case(2, 5, alpha=True), ["mac_projection", "approximate_projection", "set_timestep"]),
    (Case(2, 5, tracers=True), TRACER_HOOKS + ["set_timestep"]),
    (Case(2, 5, "symmetry", gradient=2, tracers=True), TRACER_HOOKS),
    (Case(2, 5, event=True), ["set_timestep"]),
    (Case(2, 5, gradient=1, visc=1e-2, source=0.7), KERNEL_HOOKS + ["domain_cfl", "set_timestep"]),
    (Case(3, 3), STEP_HOOKS + ["centered_velocity_advection_gmac"]),
    (Case(3, 4), STEP_HOOKS),
    (Case(3, 4, gradient=1), KERNEL_HOOKS),
    (Case(3, 4, gradient=2), KERNEL_HOOKS),
    (Case(3, 4, visc=1e-2), KERNEL_HOOKS + ["domain_cfl", "set_timestep"]),
    (Case(3, 4, source=0.7), KERNEL_HOOKS + ["domain_cfl", "set_timestep"]),
    (Case(3, 4, alpha=True), ["mac_projection", "approximate_projection", "set_timestep"]),
    (Case(3, 4, tracers=True), TRACER_HOOKS),
    (Case(3, 4, "lid"), STEP_HOOKS),
    (Case(3, 4, "symmetry"), STEP_HOOKS),
    (Case(3, 4, "symmetry", alpha=True), ["mac_projection", "approximate_projection"]),
    (Case(3, 5, "external"), KERNEL_HOOKS + ["approximate_projection", "correct_centered_velocities"]),
    (Case(3, 5, "external", tracers=True), ["tracer_advection_dt"]),
    (Case(3, 5), STEP_HOOKS + ["centered_velocity_advection_gmac"]),
    (Case(3, 5, gradient=1), KERNEL_HOOKS),
    (Case(3, 5, gradient=2), KERNEL_HOOKS),
    (Case(3, 5, visc=1e-2), KERNEL_HOOKS + ["domain_cfl", "set_timestep"]),
    (Case(3, 5, source=0.7), KERNEL_HOOKS + ["domain_cfl", "set_timestep"]),
    (Case(3, 5, alpha=True), ["mac_projection", "approximate_projection"]),
    (Case(3, 5, tracers=True), TRACER_HOOKS),
    (Case(3, 5, gradient=2, tracers=True), ["tracer_advection_dt"]),
    (Case(3, 5, event=True), ["set_timestep"]),
    (Case(3, 5, "symmetry"), KERNEL_HOOKS + ["approximate_projection"]),
    (Case(3, 6), KERNEL_HOOKS),
    (Case(3, 6, gradient=1, tracers=True), ["tracer_advection_dt", "centered_velocity_advection"]),
]

HOOK_PARAMS = [pytest.param(case, hook, id="%s-%s" % (case.id, hook)) for case, hooks in HOOK_CASES
               for hook in hooks]


def _pair(case, seed=1, un=True, dt=True):
    """an oracle and a device simulation of a case in the same uploaded state"""
    osim = H.oracle_sim(case)
    gd, gs = H.device_sim(case)
    H.load_state(case, osim, gs, H.random_state(case, seed), un=un, dt=0.3 / case.n if dt else None)
    return osim, gd, gs


def _all_differences(osim, gs, coarse=False, un=True):
    d = H.differences(osim, gs, coarse=coarse, un=un)
    d += H.params_differences(osim.projection_params, gs.projection_params, "projection_params")
    d += H.params_differences(osim.approx_projection_params, gs.approx_projection_params,
                              "approx_projection_params")
    for c in range(osim.dim):
        d += H.params_differences(osim.diffusion_params(c), gs.diffusion_params(c),
                                  "diffusion_params[%d]" % c)
    return d


@pytest.mark.parametrize("case,hook", HOOK_PARAMS)
def test_hook(case, hook):
    """one public piece on a state given by upload: everything the simulation holds afterwards is the
    oracle's, the variables the hook has no business with included"""
    osim, gd, gs = _pair(case)
    try:
        assert _all_differences(osim, gs) == [], "the uploaded states differ"
        ro = HOOKS[hook](osim)
        rg = HOOKS[hook](gs)
        assert ro == rg, "value returned by %s" % hook
        assert _all_differences(osim, gs, coarse=(hook == "coarse_init")) == []
        if hook == "set_timestep" and case.event:
            # the event cut the step: the n == 1 branch, tnext is the event's (t = 0)
            assert osim.dt == case.event_time() + 1e-9 and osim.dt < 0.3 / case.n
            osim.advance_time()
            gs.advance_time()
            assert osim.t == gs.t == case.event_time() + 1e-9 and gs.i == 1
    finally:
        H.destroy_device(gd, gs)


def test_alpha_with_viscosity_is_refused():
    """GfsSourceDiffusion together with GfsPhysicalParams { alpha }: GFSHIP_EUNSUPPORTED, either order,
    and the simulation keeps what it had"""
    case = Case(2, 4, alpha=True)
    gd, gs = H.device_sim(case)
    try:
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gs.set_viscosity(0, 1e-2)
        gs.set_alpha(None)
        gs.set_viscosity(0, 1e-2)
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gs.set_alpha(gs.hook_alpha)
    finally:
        H.destroy_device(gd, gs)


@pytest.mark.parametrize("dim,level", [(2, 5), (3, 4), (3, 5)])
@pytest.mark.parametrize("beta", [0.5, 1.])
def test_diffusion_pieces(dim, level, beta):
    """gfship_diffusion_residual and gfship_diffusion_cycle on their own (gfs_diffusion_residual,
    gfs_diffusion_cycle, src/poisson.c:1587-1690): the residual, one cycle, the residual after it"""
    L = O.lib()
    case = Case(dim, level)
    n = case.n
    st = H.random_state(case, seed=3)
    od = O.Domain(dim, level, H.PERIODIC)
    gd = gfship.Domain(dim, level, H.PERIODIC)
    try:
        of = {k: od.field() for k in ("u", "rhs", "rhoc", "res")}
        gf = {k: gd.variable() for k in ("u", "rhs", "rhoc", "res")}
        for k, name in (("u", "U0"), ("rhs", "U1")):
            of[k].leaf()[...] = st[name]
            gf[k].upload(st[name])
            L.go_bc(of[k].ptr, of[k].ptr, level)
            gd.bc(gf[k])
        D, dt = 1e-2, 0.3 / n
        L.go_diffusion_coefficients(od.ptr, D, dt, beta, of["rhoc"].ptr)
        gd.diffusion_coefficients(D, dt, gf["rhoc"], beta)
        L.go_diffusion_rhs(od.ptr, of["u"].ptr, of["rhs"].ptr, of["rhoc"].ptr, beta)
        gd.diffusion_rhs(gf["u"], gf["rhs"], gf["rhoc"], beta)
        assert np.array_equal(of["rhs"].interior(), H.interior(gf["rhs"].download())), "rhs"

        def same(what):
            for k in ("u", "rhs", "res"):
                assert np.array_equal(of[k].interior(), H.interior(gf[k].download())), (what, k)
            for l in range(level + 1):
                assert np.array_equal(of["rhoc"].interior(l), H.interior(gf["rhoc"].download(l))), (what, "rhoc", l)

        L.go_diffusion_residual(od.ptr, of["u"].ptr, of["rhs"].ptr, of["rhoc"].ptr, of["res"].ptr)
        gd.diffusion_residual(gf["u"], gf["rhs"], gf["rhoc"], gf["res"])
        same("residual")
        assert np.abs(of["res"].interior()).max() > 0.
        L.go_diffusion_cycle(od.ptr, 0, level, 4, of["u"].ptr, of["rhs"].ptr, of["rhoc"].ptr, of["res"].ptr)
        gd.diffusion_cycle(0, 4, gf["u"], gf["rhs"], gf["rhoc"], gf["res"])
        same("cycle")
        L.go_diffusion_residual(od.ptr, of["u"].ptr, of["rhs"].ptr, of["rhoc"].ptr, of["res"].ptr)
        gd.diffusion_residual(gf["u"], gf["rhs"], gf["rhoc"], gf["res"])
        same("residual after the cycle")
    finally:
        gd.destroy()


# ---------------------------------------------------------------------------------------------
# 2. a step written from the pieces
# ---------------------------------------------------------------------------------------------

STEP_CASES = [Case(2, 5), Case(2, 5, gradient=1, tracers=True), Case(2, 5, "lid", visc=1e-2),
              Case(2, 5, event=True), Case(3, 4, "symmetry", source=0.7), Case(3, 4, alpha=True),
              Case(3, 5), Case(3, 5, tracers=True)]
NSTEPS = 4


def _started(case, ndevice):
    """an oracle simulation and ndevice device simulations (each on its own domain) of a case, started
    from the same velocities and tracers (everything else zero); the handle of the MAC velocities is
    NOT taken, so the device keeps its lazy path"""
    st = H.random_state(case, seed=2)
    for k in st:
        if k[0] not in "UT":
            st[k] = np.zeros_like(st[k])
    osim = H.oracle_sim(case)
    H.load_state(case, osim, None, st, un=False)
    dev = []
    for _ in range(ndevice):
        gd, gs = H.device_sim(case)
        H.load_state(case, osim, gs, st, un=False)
        dev.append((gd, gs))
    osim.start()
    for gd, gs in dev:
        gs.start()
    return osim, dev


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in STEP_CASES])
def test_steps_three_ways(case):
    """gfship_sim_step, the pieces through the ABI in simulation_run's order, go_sim_step: identical
    after every step in every variable, the non-leaf levels, un, t, i, dt"""
    osim, dev = _started(case, 2)
    try:
        (_, fused), (_, pieces) = dev
        assert _all_differences(osim, fused, coarse=True) == [], "start"
        assert _all_differences(osim, pieces, coarse=True) == [], "start"
        for k in range(NSTEPS):
            osim.step()
            fused.step()
            H.pieces_step(pieces)
            assert _all_differences(osim, fused, coarse=True) == [], "gfship_sim_step, step %d" % k
            assert _all_differences(osim, pieces, coarse=True) == [], "the pieces, step %d" % k
        assert osim.i == NSTEPS
    finally:
        for gd, gs in dev:
            H.destroy_device(gd, gs)


@pytest.mark.parametrize("first", ["fused_first", "pieces_first"])
@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in STEP_CASES])
def test_steps_alternating_styles(case, first):
    """gfship_sim_step and the pieces alternating step by step on ONE simulation: what a fused step
    leaves behind (MAC velocities not stored, swapped storage, the divergence and the CFL maxima kept for
    the next call) must not leak into the pieces, nor the other way round.  Nothing is asked of the
    device between the steps but downloads of the variables; the MAC velocities are compared at the end."""
    osim, dev = _started(case, 1)
    try:
        gs = dev[0][1]
        for k in range(NSTEPS):
            osim.step()
            if (k % 2 == 0) == (first == "fused_first"):
                gs.step()
            else:
                H.pieces_step(gs)
            assert _all_differences(osim, gs, coarse=True, un=False) == [], "step %d" % k
        assert _all_differences(osim, gs, coarse=True) == [], "after the last step"
    finally:
        H.destroy_device(*dev[0])


# ---------------------------------------------------------------------------------------------
# 3. the state between calls
# ---------------------------------------------------------------------------------------------

LAZY = Case(3, 5)      # periodic, no tracers, no viscosity, no source: gfship_sim_step leaves un unstored


def _hip():
    import multibox as M
    return M._hip()


def _ptr_copy(gd, var, host, to_device, level=None):
    """copy between a host array with ghosts and the storage gfship_field_device_ptr returns, with the
    pitch and offset it returns"""
    level = gd.depth if level is None else level
    px, xo = C.c_int(), C.c_int()
    ptr = gfship.lib().gfship_field_device_ptr(gd.ptr, var.h, level, C.byref(px), C.byref(xo))
    assert ptr
    gd.synchronize()
    rows = (1 << level) + 2
    assert host.flags.c_contiguous and host.shape == (rows,) * gd.dim and px.value >= rows
    dev = C.c_void_p(ptr + 8 * xo.value)
    hst = C.c_void_p(host.ctypes.data)
    width, height = C.c_size_t(8 * rows), C.c_size_t(rows ** (gd.dim - 1))
    dpitch, hpitch = C.c_size_t(8 * px.value), C.c_size_t(8 * rows)
    if to_device:
        rc = _hip().hipMemcpy2D(dev, dpitch, hst, hpitch, width, height, 1)
    else:
        rc = _hip().hipMemcpy2D(hst, hpitch, dev, dpitch, width, height, 2)
    assert rc == 0
    return ptr


def test_lazy_path_is_taken_and_gives_the_bits_of_the_stored_one(monkeypatch):
    """the configuration of the tests below does take the lazy path of gfship_sim_step: the lazy
    projection swaps the storage of U, V, W once more than the advection, so the leaves of U are back at
    the address they had before the step, and are not under GFSHIP_NO_LAZY_UN=1; both give the
    oracle's bits"""
    def run():
        osim, dev = _started(LAZY, 1)
        gd, gs = dev[0]
        try:
            before = gfship.lib().gfship_field_device_ptr(gd.ptr, gs.u[0].h, gd.depth, None, None)
            for _ in range(2):
                osim.step()
                gs.step()
            after = gfship.lib().gfship_field_device_ptr(gd.ptr, gs.u[0].h, gd.depth, None, None)
            assert _all_differences(osim, gs, coarse=True) == []
            osim.step()
            gs.step()
            third = gfship.lib().gfship_field_device_ptr(gd.ptr, gs.u[0].h, gd.depth, None, None)
            return before, after, third
        finally:
            H.destroy_device(gd, gs)
    before, after, third = run()
    assert before == after == third
    monkeypatch.setenv("GFSHIP_NO_LAZY_UN", "1")
    before, after, third = run()
    assert before == after and third != after


PIECES_AFTER = ["predicted_face_velocities", "mac_projection", "approximate_projection",
                "centered_velocity_advection", "correct_centered_velocities", "domain_cfl", "set_timestep",
                "coarse_init", "pieces_step", "download_un"]


@pytest.mark.parametrize("piece", PIECES_AFTER)
@pytest.mark.parametrize("k", [1, 2])
def test_after_lazy_steps_each_piece(k, piece):
    """k gfship_sim_step on the 3-D periodic box at 32^3 without tracers (the MAC velocities of the last
    projection are not stored), then a public piece as the very next call"""
    osim, dev = _started(LAZY, 1)
    gd, gs = dev[0]
    try:
        for _ in range(k):
            osim.step()
            gs.step()
        if piece == "pieces_step":
            H.pieces_step(osim)
            H.pieces_step(gs)
        elif piece != "download_un":
            assert HOOKS[piece](osim) == HOOKS[piece](gs)
        assert _all_differences(osim, gs, coarse=True) == []
        # ... and the simulation goes on like the oracle's
        osim.step()
        gs.step()
        assert _all_differences(osim, gs, coarse=True) == [], "the step after"
    finally:
        H.destroy_device(gd, gs)


def _write(kind, case, osim, gd, gs):
    """the same write into a variable of both simulations, between two calls"""
    st = H.random_state(case, seed=7)
    if kind == "fill_P":
        osim.p.leaf()[...] = 0.25
        gs.p.fill(0.25)
    elif kind == "upload_P":
        osim.p.leaf()[...] = st["P"]
        gs.p.upload(st["P"])
    elif kind == "upload_Pmac":
        # its non-leaf values are those gfs_cell_coarse_init computed in the last step, not those of the
        # new leaves (the device computes them when somebody asks)
        osim.pmac.leaf()[...] = st["Pmac"]
        gs.pmac.upload(st["Pmac"])
    elif kind == "upload_U":
        osim.u[0].leaf()[...] = st["U0"]
        gs.u[0].upload(st["U0"])
    elif kind == "device_ptr_P":
        osim.p.leaf()[...] = st["P"]
        _ptr_copy(gd, gs.p, np.ascontiguousarray(st["P"]), True)
    elif kind == "device_ptr_U":
        osim.u[0].leaf()[...] = st["U0"]
        _ptr_copy(gd, gs.u[0], np.ascontiguousarray(st["U0"]), True)
    elif kind == "bc_P":
        # gfs_domain_bc of P after its ghost cells were overwritten
        osim.p.leaf()[...] = st["P"]
        gs.p.upload(st["P"])
        O.lib().go_bc(osim.p.ptr, osim.p.ptr, case.level)
        gd.bc(gs.p)
    else:
        raise ValueError(kind)
    # whoever writes a variable applies its conditions (gfs_domain_bc after an Init or an event): the
    # ghost cells of both sides are those of the new values
    of, gf = {"P": (osim.p, gs.p), "c": (osim.pmac, gs.pmac), "U": (osim.u[0], gs.u[0])}[kind[-1]]
    O.lib().go_bc(of.ptr, of.ptr, case.level)
    gd.bc(gf)


WRITES = ["fill_P", "upload_P", "upload_Pmac", "upload_U", "device_ptr_P", "device_ptr_U", "bc_P"]


@pytest.mark.parametrize("then", ["download_un", "mac_projection", "centered_velocity_advection", "step"])
@pytest.mark.parametrize("kind", WRITES)
def test_writes_between_steps(kind, then):
    """two lazy steps, then the caller rewrites a variable: the MAC velocities are those of the state
    BEFORE the write (the reference stores them in the cells; so does the oracle), whoever reads them
    next -- gfship_sim_download_un, a projection, the advection -- and the next step is the one of the
    oracle that received the same write"""
    osim, dev = _started(LAZY, 1)
    gd, gs = dev[0]
    try:
        for _ in range(2):
            osim.step()
            gs.step()
        _write(kind, LAZY, osim, gd, gs)
        if then == "step":
            osim.step()
            gs.step()
        elif then != "download_un":
            HOOKS[then](osim)
            HOOKS[then](gs)
        assert _all_differences(osim, gs, coarse=True) == []
        osim.step()
        gs.step()
        assert _all_differences(osim, gs, coarse=True) == [], "the step after"
    finally:
        H.destroy_device(gd, gs)


def test_un_handle_after_lazy_steps():
    """gfship_sim_variable (GFSHIP_VAR_UN) asked for after lazy steps: the handle's contents are the
    oracle's MAC velocities, and later steps stay identical (the lazy path is off from then on)"""
    osim, dev = _started(LAZY, 1)
    gd, gs = dev[0]
    try:
        for _ in range(2):
            osim.step()
            gs.step()
        for c in range(3):
            a, sl = H.oracle_un_plus(osim, c)
            assert np.array_equal(a, gs.mac_velocity(c).download()[sl]), "un[%d]" % c
        assert _all_differences(osim, gs, coarse=True, un=False) == []
        before = gfship.lib().gfship_field_device_ptr(gd.ptr, gs.u[0].h, gd.depth, None, None)
        for k in range(2):
            osim.step()
            gs.step()
            assert _all_differences(osim, gs, coarse=True, un=False) == [], k
            for c in range(3):
                a, sl = H.oracle_un_plus(osim, c)
                assert np.array_equal(a, gs.mac_velocity(c).download()[sl]), "un[%d]" % c
        # one swap per step now (the advection's): the lazy path is off
        osim.step()
        gs.step()
        assert gfship.lib().gfship_field_device_ptr(gd.ptr, gs.u[0].h, gd.depth, None, None) != before
    finally:
        H.destroy_device(gd, gs)


@pytest.mark.parametrize("change", ["add_tracer", "viscosity", "source", "alpha_on_off", "dtmax", "gradient"])
def test_settings_changed_between_steps(change):
    """a tracer added after two steps, gfship_sim_set_viscosity, _set_source, _set_alpha (NULL ->
    fields -> NULL), gfship_sim_set_time (dtmax), the gradient of the advection changed between steps:
    the next time steps and the next steps are the oracle's"""
    case = LAZY
    osim, dev = _started(case, 1)
    gd, gs = dev[0]
    try:
        for _ in range(2):
            osim.step()
            gs.step()
        sims = (osim, gs)
        if change == "add_tracer":
            st = H.random_state(case, seed=9)
            ot, gt = osim.add_tracer(gradient=1), gs.add_tracer(gradient=1)
            osim.hook_tracers.append(ot)
            gs.hook_tracers.append(gt)
            ot.leaf()[...] = st["T0"]
            gt.upload(st["T0"])
            O.lib().go_bc(ot.ptr, ot.ptr, case.level)
            gd.bc(gt)
        elif change == "viscosity":
            for s in sims:
                for c in range(3):
                    s.set_viscosity(c, 1e-2)
        elif change == "source":
            for s in sims:
                s.set_source(2, -0.9)
        elif change == "dtmax":
            for s in sims:
                s.set_time(dtmax=0.2 * osim.dt)
        elif change == "gradient":
            for s in sims:
                s.advection_params.gradient = 2
        elif change == "alpha_on_off":
            a = H.alpha_faces(case)
            oa, ga = [], []
            for c in range(3):
                f, v = O.Field(osim.dom, -1), gd.variable()
                f.leaf()[...] = a[c]
                v.upload(a[c])
                oa.append(f)
                ga.append(v)
            osim.set_alpha(oa)
            gs.set_alpha(ga)
        for k in range(2):
            osim.step()
            gs.step()
            assert _all_differences(osim, gs, coarse=True) == [], "step %d after the change" % k
        if change == "dtmax":
            assert osim.dt == gs.dt and osim.dt <= 0.2 * 0.1
        if change == "alpha_on_off":
            osim.set_alpha(None)
            gs.set_alpha(None)
            for k in range(2):
                osim.step()
                gs.step()
                assert _all_differences(osim, gs, coarse=True) == [], "step %d, alpha = NULL again" % k
    finally:
        H.destroy_device(gd, gs)


def test_second_simulation_on_a_domain_is_refused():
    """one gfship_sim per gfship_domain (include/gfship.h): a second gfship_sim_create fails with
    GFSHIP_EUNSUPPORTED and leaves the first stepping bit for bit; after gfship_sim_destroy the domain
    takes a new simulation"""
    osim, dev = _started(LAZY, 1)
    gd, gs = dev[0]
    try:
        osim.step()
        gs.step()
        with pytest.raises(gfship.GfshipError, match="gfship error -5"):
            gfship.Simulation(gd)
        for k in range(2):
            osim.step()
            gs.step()
            assert _all_differences(osim, gs, coarse=True, un=(k == 1)) == [], k
        gs.destroy()
        again = gfship.Simulation(gd)
        again.destroy()
    finally:
        H.destroy_device(gd, gs)


@pytest.mark.parametrize("case", [pytest.param(c, id=c.id) for c in (LAZY, Case(2, 5, tracers=True))])
def test_device_ptr_addresses_the_storage_of_download_and_upload(case):
    """what include/gfship.h promises of gfship_field_device_ptr: a pointer taken after a call addresses,
    with the pitch and offset returned, the storage gfship_field_download reads and _upload writes, on
    every level, and stays good until the next call that advances the simulation -- after which it is
    asked for again (the storage of U, V, W and the tracers is swapped with scratch arrays)"""
    osim, dev = _started(case, 1)
    gd, gs = dev[0]
    try:
        fields = H.sim_fields(gs)
        for k in range(3):
            osim.step()
            gs.step()
            for name, f in fields.items():
                for level in ((gd.depth, gd.depth - 1) if name[0] in "PUT" else (gd.depth,)):
                    got = np.empty(f._shape(level))
                    _ptr_copy(gd, f, got, False, level)
                    assert np.array_equal(got, f.download(level)), (k, name, level)
        # stable between two advancing calls: an upload lands where the pointer points, and a write
        # through the pointer is what download and the next step see
        st = H.random_state(case, seed=11)
        u = gs.u[0]
        p0 = _ptr_copy(gd, u, np.empty(u._shape(gd.depth)), False)
        u.upload(st["U0"])
        got = np.empty(u._shape(gd.depth))
        assert _ptr_copy(gd, u, got, False) == p0
        assert np.array_equal(got, st["U0"])
        _ptr_copy(gd, u, np.ascontiguousarray(st["U1"]), True)
        assert np.array_equal(u.download(), st["U1"])
        osim.u[0].leaf()[...] = st["U1"]
        O.lib().go_bc(osim.u[0].ptr, osim.u[0].ptr, case.level)
        gd.bc(u)
        osim.step()
        gs.step()
        assert _all_differences(osim, gs, coarse=True) == []
    finally:
        H.destroy_device(gd, gs)
