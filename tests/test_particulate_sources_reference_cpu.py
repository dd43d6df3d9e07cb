"""The restatement of GfsSourceParticulateVol / ...Mass (tests/particulate_sources_reference.py) by hand, and the
premises of the runs the device is compared on (tests/particulate_sources_cases.py): no GPU."""
import math

import numpy as np
import pytest

import particulate_sources_cases as K
import particulate_sources_reference as PS
import sampler_cases as SK


def _zero_velocity(box):
    return [box.field(np.zeros((box.n + 2,)*box.dim)) for _ in range(box.dim)]


def test_two_particles_in_one_cell_and_in_two_cells():
    box = SK.box(2, 2)
    h = 0.25
    a = PS.Particulate([-0.5 + 0.3*h, -0.5 + 0.4*h, 0.], [0.5, -1., 0.], 2., 1e-3)
    b = PS.Particulate([-0.5 + 0.7*h, -0.5 + 0.6*h, 0.], [0.25, 2., 0.], 3., 8e-3)
    f = PS.Fields(2)
    src = PS.event(box, PS.VOLUME, [a, b], _zero_velocity(box), 0.5, 0., lambda V: 1e-3*(4.*V["Urelp"] + V["Rad"]), f)
    ra, rb = math.pow(3.0*1e-3/4.0/math.pi, 1./3.), math.pow(3.0*8e-3/4.0/math.pi, 1./3.)
    # each particle sees its own radius and relative velocity (0. - vel), whoever shares the cell
    assert src == [1e-3*(4.*(0. - 0.5) + ra), 1e-3*(4.*(0. - 0.25) + rb)]
    assert (a.volume, b.volume) == (1e-3 + src[0]*0.5, 8e-3 + src[1]*0.5)
    assert (a.mass, b.mass) == (2., 3.)
    # the cell keeps the values of the last particle and the sum of both sources from 0
    assert f.rad == {(1, 1, 0): rb} and f.urel[0] == {(1, 1, 0): -0.25} and f.urel[1] == {(1, 1, 0): -2.}
    assert f.deposit[(1, 1, 0)] == 0. + src[0] + src[1]
    assert sum(1 for v in f.deposit.values() if v != 0.) == 1 and len(f.deposit) == 16
    # two cells: b one cell to the right; a mass source leaves the volumes alone, the deposit is reset first
    b.pos[0] += h
    va, vb = a.volume, b.volume
    src = PS.event(box, PS.MASS, [a, b], _zero_velocity(box), 0.25, 0., lambda V: V["x"] + 2.*V["y"], f)
    assert src == [-0.375 + 2.*-0.375, -0.125 + 2.*-0.375]
    assert (a.mass, b.mass) == (2. + src[0]*0.25, 3. + src[1]*0.25) and (a.volume, b.volume) == (va, vb)
    assert f.deposit[(1, 1, 0)] == src[0] and f.deposit[(2, 1, 0)] == src[1]
    assert f.rad == {(1, 1, 0): PS.radius(va), (2, 1, 0): PS.radius(vb)}
    # a particle without a cell is skipped
    c = PS.Particulate([0.7, 0., 0.], [0., 0., 0.], 1., 1e-3)
    assert PS.event(box, PS.MASS, [c], _zero_velocity(box), 0.25, 0., lambda V: 1., f) == [None]
    assert (c.mass, c.volume) == (1., 1e-3) and not any(f.deposit.values())


@pytest.mark.parametrize("sides_name", K.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", K.BOXES)
def test_a_constant_source(dim, level, sides_name):
    """every volume becomes v + s*dt exactly and the deposit of a cell is the sequential sum"""
    s = K.FUNCTIONS["constant"][1](None)
    run = K.reference_run(dim, level, sides_name, PS.VOLUME, "constant")
    volume = np.array(K.particles(dim, level, sides_name)[4])
    ev = run.events[0]
    inside = np.array([c is not None for c in ev.cells])
    assert np.array_equal(ev.volume[inside], volume[inside] + s*K.EVENT_DT[0])
    assert np.array_equal(ev.volume[~inside], volume[~inside]) and (~inside).sum() == (sides_name == "closed")
    want = np.zeros(1 << (dim*level))
    for c in ev.cells:
        if c is not None:
            want[c] = want[c] + s
    got = ev.deposit[(slice(1, -1),)*dim].ravel()
    assert np.array_equal(got, want)
    assert want.max() >= 3*s and (want == 0.).sum() > len(want)//3      # a shared cell, and cells that hold none


@pytest.mark.parametrize("sides_name", K.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", K.BOXES)
def test_the_case_holds_what_the_device_tests_rely_on(dim, level, sides_name):
    box = SK.box(dim, level)
    pos = K.particles(dim, level, sides_name)[0]
    run = K.reference_run(dim, level, sides_name, PS.VOLUME, "tracer")
    first, moved = run.events[0].cells, run.events[K.MOVE_BEFORE].cells
    # as created: three in one cell, interleaved in list order with particles of other cells
    assert len({first[o] for o in K.SHARED_STATIC}) == 1
    assert all(first[o + 1] != first[o] for o in K.SHARED_STATIC)
    # one on a cell face (the coordinate is the face's, exactly), one in a corner cell, one outside (walls)
    n = 1 << level
    assert (pos[K.ON_FACE][0] + 0.5)*n == 3. and first[K.ON_FACE] % n == 2
    assert first[K.IN_CORNER] == 0
    assert (first[K.OUTSIDE] is None) == (sides_name == "closed")
    assert len(moved) == K.NPART - (sides_name == "closed")
    # after the move the particles SHARED sit in one cell, interleaved in list order with others
    on_list = K.on_list_after_move(sides_name)
    cell_of = dict(zip(on_list, moved))
    assert len({cell_of[o] for o in K.SHARED}) == 1
    assert all(cell_of[o + 1] != cell_of[o] for o in K.SHARED)


@pytest.mark.parametrize("fname", ["tracer", "block"])
@pytest.mark.parametrize("sides_name", K.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", K.BOXES)
def test_premise_of_the_order_tests(dim, level, sides_name, fname):
    """in the events after the move the deposit of the shared cell in list order differs in its bits from the
    same sum in reverse order and from the sum in the storage order the second sort leaves, and the last
    particle of that cell in list order is not the last one stored: a device that sums, or picks the last
    particle, in another order than the list's cannot pass"""
    run = K.reference_run(dim, level, sides_name, PS.VOLUME, fname)
    on_list = K.on_list_after_move(sides_name)
    for e in range(K.MOVE_BEFORE, K.NEVENTS):
        ev = run.events[e]
        cell_of = dict(zip(on_list, ev.cells))
        src_of = dict(zip(on_list, ev.sources))
        shared = cell_of[K.SHARED[0]]
        in_list_order = [o for o in on_list if cell_of[o] == shared]
        in_storage_order = [o for o in run.storage if cell_of[o] == shared]
        assert sorted(in_storage_order) == in_list_order and len(in_list_order) >= 4

        def total(order):
            s = 0.
            for o in order:
                s += src_of[o]
            return s
        got = ev.deposit[(slice(1, -1),)*dim].ravel()[shared]
        assert got == total(in_list_order)
        assert total(in_list_order) != total(reversed(in_list_order))
        assert total(in_list_order) != total(in_storage_order)
        assert in_list_order[-1] != in_storage_order[-1]


@pytest.mark.parametrize("kind", [PS.VOLUME, PS.MASS])
@pytest.mark.parametrize("sides_name", K.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", K.BOXES)
def test_premise_of_the_step_function(dim, level, sides_name, kind):
    """every radius the function `step' sees is far from its threshold: a factor of 2 at least, where the
    device's pow and glibc's differ by ulps"""
    run = K.reference_run(dim, level, sides_name, kind, "step")
    volume = np.array(K.particles(dim, level, sides_name)[4])
    seen = [PS.radius(v) for v in volume] + [PS.radius(v) for ev in run.events for v in ev.volume]
    assert all(r > 2.*K.RAD_STEP or r < K.RAD_STEP/2. for r in seen)
    assert any(r > K.RAD_STEP for r in seen) and any(r < K.RAD_STEP for r in seen)
    both = {s for ev in run.events for s in ev.sources if s is not None}
    assert both == {1e-5, 1e-8}


@pytest.mark.parametrize("kind", [PS.VOLUME, PS.MASS])
@pytest.mark.parametrize("fname", list(K.FUNCTIONS))
@pytest.mark.parametrize("sides_name", K.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", K.BOXES)
def test_every_run_is_defined(dim, level, sides_name, fname, kind):
    """volumes and masses stay positive, and every particle with a cell gets a source that is not zero"""
    run = K.reference_run(dim, level, sides_name, kind, fname)
    for ev in run.events:
        assert (ev.volume > 0.).all() and (ev.mass > 0.).all()
        assert all((s is None) == (c is None) and s != 0. for s, c in zip(ev.sources, ev.cells))


def test_the_radius_function_is_a_parameter():
    up = lambda x, y: math.nextafter(math.pow(x, y), math.inf)
    a = K.reference_run(2, 3, "periodic", PS.MASS, "step")
    b = K.reference_run(2, 3, "periodic", PS.MASS, "step", up)
    assert np.array_equal(a.events[0].mass, b.events[0].mass)
    ra, rb = a.events[0].rad, b.events[0].rad
    w = ra != K.SENTINEL
    assert w.any() and np.array_equal(np.nextafter(ra[w], np.inf), rb[w])
