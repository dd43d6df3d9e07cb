"""The device's particulate forces (gfship_particle_list_event, gfship_particles_forces_on_fluid, read
back through gfship_particles_download* and particulate_state) against the restatement of the reference
(tests/forces_reference.py, its `sqrt' variant) on the case matrix of tests/forces_cases.py, by
array_equal on every array: positions, old positions, survivors and their order, vel, mass and force after
every event and after the evaluation of the forces on the fluid.  No tolerance anywhere: the library is
built with -ffp-contract=off, also for the compiled coefficient functions, and keeps the reference's
operand order; the square root of the default drag law is its one deliberate departure.
test_forces_reference_cpu.py shows on the same matrix that the restatement is defined, that its conditions
hold and that the oracle agrees with the `pow' variant."""
import numpy as np
import pytest

import forces_cases as K
import gfship

pytestmark = pytest.mark.gpu


def _upload_velocity(gs, case, k):
    for c, a in enumerate(K.case_velocity(case, k)):
        gs.u[c].upload(a)


def _state(gpl, tag):
    pos, ids = gpl.download()
    vel, mass, force = gpl.particulate_state()
    return K.State(tag, pos, gpl.download_old(), ids, vel, mass, force)


def _compare(got, ref, what):
    assert np.array_equal(got.ids, ref.ids), (what, ref.tag)
    for a in ("pos", "old", "vel", "mass", "force"):
        x, y = getattr(got, a), getattr(ref, a)
        assert np.array_equal(x, y), (what, ref.tag, a, int((x != y).sum()), float(np.nanmax(np.abs(x - y))))


def _device_states(case, sort_every):
    dim, level = case.dim, case.level
    n = 1 << level
    gd = gfship.Domain(dim, level, K.SIDES[case.sides])
    gs = gfship.Simulation(gd)
    gpl = None
    states = []
    try:
        if case.viscosity in ("uv", "pow2"):
            for c in range(dim):
                gs.set_viscosity(c, K.NU if case.viscosity == "uv" else K.NU_BRANCHES)
        elif case.viscosity == "v-only":
            gs.set_viscosity(1, K.NU)
        elif case.viscosity == "cell":
            alpha, mu = K.cell_fields(dim, level)
            va, vm = gd.variable(), gd.variable()
            for l in range(level):
                va.fill(1., l)
            va.upload(alpha)
            vm.upload(mu)
            gs.set_alpha_cell(va)
            gs.set_viscosity_cell(vm)
        gs.advection_params.dt = K.dt_of(case)
        _upload_velocity(gs, case, 0)
        pos, ids, vel, mass, volume = K.case_particles(case)
        gpl = gfship.ParticleList(gs, pos, ids)
        gpl.set_sort_interval(sort_every)
        gpl.set_particulate(vel, mass, volume)
        gpl.set_forces(K.FORCE_LISTS[case.forces], K.GRAVITY)
        for q, text in K.coefficient_texts(case).items():
            gpl.set_force_coefficient(q, text)
        for k in range(K.NEVENTS):
            _upload_velocity(gs, case, k + 1)
            if k == K.ONFLUID_BEFORE_EVENT:
                gpl.forces_on_fluid()
                states.append(_state(gpl, "onfluid"))
            gpl.event()
            states.append(_state(gpl, "event%d" % k))
            assert gpl.count() == len(states[-1].ids)
        for c, a in enumerate(K.case_velocity(case, K.NEVENTS)):
            assert np.array_equal(gs.u[c].download(), a, equal_nan=True)
    finally:
        if gpl is not None:
            gpl.destroy()
        gs.destroy()
        gd.destroy()
    return states


@pytest.mark.parametrize("cid", K.CASE_IDS)
def test_device_equals_the_sqrt_variant(cid):
    case = K.CASES[cid]
    ref = K.reference_run(cid, root="sqrt", onfluid=True)
    for sort_every in (0, 1):
        got = _device_states(case, sort_every)
        assert [s.tag for s in got] == [s.tag for s in ref.states]
        for g, r in zip(got, ref.states):
            _compare(g, r, (cid, sort_every))


def test_the_variants_were_dispatched():
    """cases with and without coefficient functions and cell fields give different results on the same
    particles, fields and list of forces: the coefficient kernels and the <RHO, MU> instantiations ran
    (gfship_domain_kernel_counts does not count the particle kernels)"""
    plain = _device_states(K.CASES["canonical-3d-l2-periodic"], 0)[-1]
    coeff = _device_states(K.CASES["coeff-3d-l2-mixed"]._replace(sides="periodic"), 0)[-1]
    cell = _device_states(K.CASES["cell-coeff-3d-l2-periodic"]._replace(coeff=False), 0)[-1]
    cell_coeff = _device_states(K.CASES["cell-coeff-3d-l2-periodic"], 0)[-1]
    pairs = [(plain, coeff), (plain, cell), (cell, cell_coeff), (coeff, cell_coeff)]
    for a, b in pairs:
        common = np.intersect1d(a.ids, b.ids)
        assert len(common) > 200
        fa, fb = a.force[np.isin(a.ids, common)], b.force[np.isin(b.ids, common)]
        assert (fa != fb).any(axis=1).mean() > 0.9
