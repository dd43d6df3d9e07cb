"""Properties of the restatement of GfsParticulateField and GfsSourceParticulate (tests/two_way_reference.py)
and of the inputs the GPU tests run it on, and the C ABI of the feature without a device."""
import ctypes as C

import numpy as np
import pytest

import gfship
import two_way_reference as R
from conftest import has_gpu
from two_way_cases import (BOXES, RKERNEL_H, alpha_cell_case, assert_two_chunks_are_order_sensitive, poly_kernel,
                           spreading_case, spreading_chunks_case, void_fraction_case)


@pytest.mark.parametrize("dim,depth", [(2, 3), (3, 2)])
def test_pruned_descent_visits_the_leaves_of_the_flat_filter(dim, depth):
    """cond_kernel is monotone along a branch: every leaf that passes has ancestors that pass (the ball
    around a cell of radius (size/2) sqrt (dim) contains its children's, and a cell that holds the particle
    lies in a parent that holds it), so pruning loses nothing.  Brute force on 8^2 and 4^3, 50 random
    particles each, some of them outside the box."""
    rng = np.random.default_rng(5)
    h = 1. / (1 << depth)
    order = R.traversal_order(dim, depth)
    assert len(order) == (1 << depth) ** dim and len(set(order)) == len(order)
    for q in range(50):
        p = list(1.3 * (rng.random(3) - 0.5))
        if dim == 2:
            p[2] = 0.
        for rk in (0., 0.3 * h, 1.5 * h, 2.5 * h):
            assert R.descent(dim, depth, p, rk) == R.flat_filter(dim, depth, p, rk, order), (q, rk)
        own = R.locate(dim, depth, p)
        if own is not None:
            assert own in R.descent(dim, depth, p, 0.)


def test_locate_puts_a_point_on_a_face_into_the_low_cell():
    h = 1. / 16
    assert R.locate(2, 4, [-0.5 + 3 * h, 0.01, 0.]) == (2, 8)
    assert R.locate(2, 4, [-0.5 + 3 * h + 1e-15, 0.01, 0.]) == (3, 8)
    assert R.locate(3, 3, [0.7, 0., 0.]) is None
    assert R.locate(3, 3, [0.5, 0.5, 0.5]) == (7, 7, 7)


@pytest.mark.parametrize("dim,depth", BOXES)
def test_void_fraction_sums_to_the_volume_of_the_located_particles(dim, depth):
    pos, ids, volume = void_fraction_case(dim, depth)
    v = R.void_fraction(dim, depth, pos, volume)
    h = 1. / (1 << depth)
    cellvol = h ** dim
    located = np.array([R.locate(dim, depth, p) is not None for p in pos])
    assert (~located).sum() >= 1
    total = volume[located].sum()
    assert abs((v * cellvol).sum() - total) <= 1e-12 * np.abs(volume[located]).sum()
    # the inputs are what the issue asks for: shared cells, a particle on a face, one outside
    cells = [R.locate(dim, depth, p) for p in pos]
    counts = {}
    for c in cells:
        counts[c] = counts.get(c, 0) + 1
    assert sum(1 for c in cells if c is not None and counts[c] > 1) >= 20
    assert cells[40] is not None and cells[41] is not None and cells[41][0] == cells[40][0] + 1
    assert cells[42] is None


@pytest.mark.parametrize("dim,depth", BOXES)
def test_void_fraction_inputs_are_order_sensitive(dim, depth):
    pos, ids, volume = void_fraction_case(dim, depth)
    a = R.void_fraction(dim, depth, pos, volume)
    b = R.void_fraction(dim, depth, pos[::-1], volume[::-1])
    assert not np.array_equal(a, b)
    assert np.allclose(a, b, rtol=1e-12, atol=0.)


@pytest.mark.parametrize("rk", RKERNEL_H)
@pytest.mark.parametrize("dim,depth", BOXES)
def test_spreading_conserves_the_force_and_is_order_sensitive(dim, depth, rk):
    pos, ids, vel, mass, volume, force = spreading_case(dim, depth)
    h = 1. / (1 << depth)
    cellvol = h ** dim
    alpha = alpha_cell_case(dim, depth)
    F, corr = R.spread(dim, depth, pos, volume, force, rk * h, poly_kernel, alpha_cell=alpha)
    deposits = corr > 1.e-10
    # both kinds of particle are there: some deposit, at least one has a kernel that vanishes or is negative
    assert deposits.sum() >= 20 and (~deposits).sum() >= 1
    # What the reference's normalisation conserves.  correction = sum (K cellvol)/sum (cellvol) is the MEAN of
    # K over the N leaves a particle reaches (:2112-2118, :2216), so sum over them of K/correction is N, not 1:
    # sum F_c liq_rho cellvol = - sum over the depositing particles of N force_c.  (It is - sum force_c only
    # where every particle reaches one leaf.)  To 1e-12 of the sum of magnitudes, the project's bound for sums.
    liq_rho = 1. / alpha
    nleaves = np.array([len(R.descent(dim, depth, list(p), rk * h)) for p in pos])
    assert nleaves[deposits].max() > 1
    for c in range(dim):
        lhs = (F[c] * liq_rho * cellvol).sum()
        rhs = -(nleaves[deposits] * force[deposits, c]).sum()
        scale = np.abs(nleaves[deposits] * force[deposits, c]).sum()
        assert abs(lhs - rhs) <= 1e-12 * scale, (c, lhs, rhs)
    # the clipping: a particle next to x = +0.5 reaches no cell across the side
    reach = R.descent(dim, depth, list(pos[14]), rk * h)
    assert all(0 <= ix[0] < (1 << depth) for ix in reach)
    if rk > 0.:
        inner = R.descent(dim, depth, list(pos[0]), rk * h)
        assert len(reach) < len(inner)
        # at least ten particles deposit into one cell
        hits = np.zeros((1 << depth,) * dim, dtype=int)
        for q in np.flatnonzero(deposits):
            for ix in R.descent(dim, depth, list(pos[q]), rk * h):
                hits[(ix[1], ix[0]) if dim == 2 else (ix[2], ix[1], ix[0])] += 1
        assert hits.max() >= 10
    Fr, _ = R.spread(dim, depth, pos[::-1], volume[::-1], force[::-1], rk * h, poly_kernel, alpha_cell=alpha)
    if rk > 0.:      # with rkernel = 0 a cell mostly gets one particle: nothing to reorder
        assert any(not np.array_equal(F[c], Fr[c]) for c in range(dim))
    for c in range(dim):
        assert np.allclose(F[c], Fr[c], rtol=1e-9, atol=1e-9 * np.abs(F[c]).max())


def test_spreading_defaults_deposit_nothing():
    pos, ids, vel, mass, volume, force = spreading_case(2, 4)
    F, corr = R.spread(2, 4, pos, volume, force, 0., lambda x, y, z, t: 0.)
    assert all(not f.any() for f in F) and not (corr > 1.e-10).any()


@pytest.mark.parametrize("rk", RKERNEL_H)
@pytest.mark.parametrize("dim,depth", BOXES)
def test_spread_flat_is_spread(dim, depth, rk):
    """the restatement vectorised over the cells, bit for bit on every small case of this file, either list order,
    with and without alpha"""
    pos, ids, vel, mass, volume, force = spreading_case(dim, depth)
    h = 1. / (1 << depth)
    for alpha in (alpha_cell_case(dim, depth), None):
        for s in (slice(None), slice(None, None, -1)):
            F, corr = R.spread(dim, depth, pos[s], volume[s], force[s], rk * h, poly_kernel, alpha_cell=alpha)
            G, gcorr = R.spread_flat(dim, depth, pos[s], volume[s], force[s], rk * h, poly_kernel, alpha_cell=alpha)
            assert np.array_equal(corr, gcorr, equal_nan=True)
            for c in range(dim):
                assert np.array_equal(F[c], G[c]), c
    assert any(f.any() for f in F)


def test_spread_flat_of_the_defaults_deposits_nothing():
    pos, ids, vel, mass, volume, force = spreading_case(2, 4)
    F, corr = R.spread_flat(2, 4, pos, volume, force, 0., lambda x, y, z, t: 0.)
    assert all(not f.any() for f in F) and not (corr > 1.e-10).any()


def test_the_two_chunk_case_is_order_sensitive_on_the_restatement():
    """the inputs of the multi-chunk GPU tests (with the stand-in forces), with and without alpha"""
    pos, ids, vel, mass, volume, force = spreading_chunks_case()
    for alpha in (alpha_cell_case(3, 5), None):
        want = assert_two_chunks_are_order_sensitive(R, pos, volume, force, alpha)
        assert all(f.all() for f in want)       # rkernel = 16 h: every particle reaches most of the box


NEW_SYMBOLS = ["gfship_particulate_field", "gfship_particles_forces_on_fluid", "gfship_particles_set_kernel",
               "gfship_source_particulate_event", "gfship_particles_spread_forces",
               "gfship_sim_set_source_fields", "gfship_particles_time_spreading"]


def test_new_symbols_are_exported_and_bound():
    L = gfship.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in gfship.SIGNATURES, name
    for method in ("particulate_field", "forces_on_fluid", "set_kernel", "spread_forces",
                   "source_particulate_event"):
        assert callable(getattr(gfship.ParticleList, method))


def test_new_entries_refuse_a_null_list():
    L = gfship.lib()
    F = (C.c_int * 3)(0, 1, 2)
    for call in (lambda: L.gfship_particulate_field(None, 0),
                 lambda: L.gfship_particles_forces_on_fluid(None),
                 lambda: L.gfship_particles_set_kernel(None, 0.1, b"1."),
                 lambda: L.gfship_source_particulate_event(None, F),
                 lambda: L.gfship_particles_spread_forces(None, F)):
        assert call() == -1                       # GFSHIP_EINVAL
        assert b"null particle list" in L.gfship_last_error()
    assert L.gfship_sim_set_source_fields(None, F) == -1
    assert b"null simulation" in L.gfship_last_error()
    assert callable(gfship.Simulation.set_source_fields)


@pytest.mark.skipif(has_gpu(), reason="checks the no-device error path")
def test_no_device_is_an_error_for_the_coupling_too():
    with pytest.raises(gfship.GfshipError, match="no HIP device"):
        gd = gfship.Domain(2, 4)
        gs = gfship.Simulation(gd)
        gfship.ParticleList(gs, np.zeros((1, 3)), np.ones(1, dtype=np.uint32)).particulate_field(gd.variable())
