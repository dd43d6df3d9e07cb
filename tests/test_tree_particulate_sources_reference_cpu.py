"""The restatement of GfsSourceParticulateVol / GfsSourceParticulateMass on refined trees
(tests/tree_particulate_sources_reference.py) and the premises of the cases of
tests/tree_particulate_sources_cases.py, without a device: what the GPU test compares the device with must show
what it is meant to show."""
import math

import numpy as np
import pytest

import forces_reference as F
import particulate_sources_reference as BOX
import sampler_cases as SK
import tree_particulate_sources_cases as K
import tree_particulate_sources_reference as PS
import tree_sampler_reference as T

KINDS = {"vol": PS.VOLUME, "mass": PS.MASS}


def _sum(start, values):
    s = start
    for v in values:
        s += v
    return s


def _cell_value(box, levels, cell):
    i, j, k = cell.ijk
    a = levels[cell.level]
    return float(a[j, i] if box.dim == 2 else a[k, j, i])


@pytest.mark.parametrize("name", K.ALL)
def test_the_fixture_has_what_the_tests_need(name):
    box = K.host_tree(name)
    P = K.particles(name, K.HOST_DT[1])
    assert 80 <= len(P.ids) <= 140
    leaves = [box.locate(p) for p in P.pos.tolist()]
    # the skipped particles have no leaf; everybody else has one
    assert len(P.outside) == box.dim and all(leaves[q] is None for q in P.outside)
    assert all(c is not None for q, c in enumerate(leaves) if q not in P.outside)
    # three particles in one fine leaf, two in one coarse leaf, far apart in the list
    assert len(P.fine) == 3 and all(leaves[q] is P.fine_leaf for q in P.fine)
    assert len(P.coarse) == 2 and all(leaves[q] is P.coarse_leaf for q in P.coarse)
    assert min(np.diff(P.fine)) > 20 and np.diff(P.coarse)[0] > 40
    levels = sorted(set(c.level for c in leaves if c is not None))
    if name in K.REFINED:
        assert P.fine_leaf.level > P.coarse_leaf.level
        assert len(levels) >= (3 if name == "graded" else 2)
        face = leaves[P.on_face]
        assert any(nb is not None and nb.level != face.level for nb in (box.neighbor(face, d) for d in range(2*box.dim)))
    assert P.pos[P.on_side][0] == 0.5 and leaves[P.on_side] is not None
    # FLY: leaves of falling index in list order, one leaf after the move
    fly = [K.leaf_index(box, leaves[q]) for q in P.fly]
    assert list(P.fly) == sorted(P.fly) and fly == sorted(fly, reverse=True) and len(set(fly)) == 3
    # no radius near the step of the function `block', and far fewer than an ulp-sized change can cross it
    rad = np.array([PS.radius(v) for v in P.volume.tolist()])
    assert ((rad < K.RAD_STEP/2.) | (rad > 2.*K.RAD_STEP)).all() and (rad > K.RAD_STEP).any() and (rad < K.RAD_STEP).any()
    # the held values are distinct and dyadic
    for key, salt in K.HELD_SALT.items():
        allv = np.concatenate([a.ravel() for a in K.held(name, salt)])
        scaled = allv*2.**(56 if key == "deposit" else 20)
        assert len(np.unique(allv)) == len(allv) and np.array_equal(scaled, np.round(scaled))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", K.ALL)
def test_premises_of_the_order_tests(name, kind):
    box = K.host_tree(name)
    P = K.particles(name, K.HOST_DT[1])
    for fname in K.ORDER_SENSITIVE:
        run = K.reference_run(name, KINDS[kind], fname)
        first, last = run.events[1], run.events[2]
        # after the move the FLY particles share their leaf, and the second sort stored them in reverse
        ids = [int(P.ids[q]) for q in P.fly]
        where = [list(last.ids).index(i) for i in ids]
        assert all(last.leaves[q] is P.fly_leaf for q in where)
        members = K.in_leaf(box, last, P.fly_leaf)
        listed = [int(last.ids[q]) for q in members]
        stored = [i for i in run.storage if i in set(listed)]
        assert [i for i in stored if i in ids] == ids[::-1]
        assert listed[-1] != stored[-1]          # the last particle of the list in that leaf is not the last one stored
        src = dict(zip(listed, [last.sources[q] for q in members]))
        start = _cell_value(box, first.deposit, P.fly_leaf)      # what the leaf held before the event
        in_list_order = _sum(start, [src[i] for i in listed])
        assert in_list_order == _cell_value(box, last.deposit, P.fly_leaf)
        assert in_list_order != _sum(start, [src[i] for i in listed[::-1]]), (name, kind, fname)
        assert in_list_order != _sum(start, [src[i] for i in stored]), (name, kind, fname)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", K.ALL)
def test_what_the_events_leave_in_the_cells(name, kind):
    box = K.host_tree(name)
    pkind = KINDS[kind]
    run = K.reference_run(name, pkind, "tracer")
    uploaded = K.held(name, K.HELD_SALT["deposit"])
    for e, ev in enumerate(run.events):
        with_particle = set(id(c) for c in ev.leaves if c is not None)
        touched = set()
        for prev in run.events[:e + 1]:
            touched |= set(id(c) for c in prev.leaves if c is not None)
        for cell in box.cells:
            got, was = _cell_value(box, ev.deposit, cell), _cell_value(box, uploaded, cell)
            if pkind == PS.VOLUME and cell.tree is None and cell.level <= 1:
                assert got == 0. or id(cell) in with_particle       # levels 0 and 1 hold 0 (none of them is a leaf here)
                continue
            if id(cell) not in touched:
                # cells with children at level >= 2, leaves without a particle, ghost cells: what was uploaded
                assert got == was, (name, kind, e, cell.level, cell.ijk)
            elif id(cell) in with_particle:
                assert got != was
        # the cells a level does not have keep what was uploaded too
        flags = [np.array(box.flags(l)) for l in range(box.level + 1)]
        for l, f in enumerate(flags):
            assert np.array_equal(ev.deposit[l][f == T.NONE], uploaded[l][f == T.NONE])
    if name in K.REFINED:
        assert all(c.level >= 2 for c in box.leaves)
    # after two events a leaf's deposit differs from the deposit of the second event alone
    P = K.particles(name, K.HOST_DT[1])
    leaf = P.fine_leaf
    members = K.in_leaf(box, run.events[1], leaf)
    alone = _sum(0., [run.events[1].sources[q] for q in members])
    both = _cell_value(box, run.events[1].deposit, leaf)
    if pkind == PS.VOLUME and leaf.level <= 1:
        assert both == alone
    else:
        assert both != alone and both != _cell_value(box, uploaded, leaf) + alone
        assert both == _sum(_cell_value(box, run.events[0].deposit, leaf), [run.events[1].sources[q] for q in members])
    # Rad, Urelp ... of a leaf are those of its last particle in list order
    last = run.events[2]
    for leaf in (P.fine_leaf, P.coarse_leaf, P.fly_leaf):
        q = K.in_leaf(box, last, leaf)[-1]
        pos = [float(x) for x in run.moved_pos[q]]
        u = [box.field(a) for a in K.host_stages(name)[2].u]
        vel = K.particles(name, K.HOST_DT[1]).vel[int(last.ids[q]) - 1]
        for c in range(box.dim):
            assert _cell_value(box, last.urel[c], leaf) == box.interpolate(leaf, pos, u[c]) - float(vel[c])


@pytest.mark.parametrize("name", K.ALL)
def test_a_mass_source_changes_nothing_but_leaves_with_particles(name):
    box = K.host_tree(name)
    run = K.reference_run(name, PS.MASS, "xyt")
    uploaded = K.held(name, K.HELD_SALT["deposit"])
    touched = set()
    for ev in run.events:
        touched |= set((c.level, c.ijk) for c in ev.leaves if c is not None)
    changed = set()
    for l in range(box.level + 1):
        for idx in np.argwhere(run.events[-1].deposit[l] != uploaded[l]):
            ijk = tuple(int(x) for x in idx[::-1]) + ((0,) if box.dim == 2 else ())
            changed.add((l, ijk))
    assert changed == touched


def _box_velocity(box, stage, level):
    return [box.field(stage.u[c][level]) for c in range(box.dim)]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name,dim", [("uniform2", 2), ("uniform3d", 3)])
def test_uniform_tree_equals_the_restatement_on_the_box(name, dim, kind):
    """with a zero deposit uploaded the first event is that of tests/particulate_sources_reference.py on the box in
    every array (afterwards the box resets its deposit and the tree does not); volumes, masses, Rad and Urelp ...
    agree for all three events"""
    level = K.UNIFORM[dim]
    tbox = K.host_tree(name)
    assert tbox.level == level and all(c.level == level for c in tbox.leaves)
    box = SK.box(dim, level)
    pkind = KINDS[kind]
    st = K.host_stages(name)
    P = K.particles(name, st[1].dt)
    for fname in K.FUNCTION_NAMES:
        run = K.reference_run(name, pkind, fname, zero_deposit=True)
        text, fn, names = K.functions(dim)[fname]
        plist = [F.Particulate(P.pos[q], P.ids[q], P.vel[q], P.mass[q], P.volume[q]) for q in range(len(P.ids))]
        variables = {"T": box.field(K.tracer(name)[level])} if "T" in names else {}
        fields = BOX.Fields(dim)
        inner = (slice(1, -1),)*dim
        for e in range(K.NEVENTS):
            if e == K.MOVE_BEFORE:
                sim = F.Sim(box, SK.SIDES["periodic"], st[e - 1].u and [st[e - 1].u[c][level] for c in range(dim)],
                            st[e - 1].dt, g=(0., 0., 0.), root=F.sqrt_root)
                plist = F.list_event(sim, plist, [F.ForceCoeff(F.BUOY)])
            BOX.event(box, pkind, plist, _box_velocity(box, st[e], level), st[e].dt, st[e].t, fn, fields, variables)
            ev = run.events[e]
            assert np.array_equal(ev.ids, np.array([p.id for p in plist], dtype=np.uint32))
            assert np.array_equal(ev.volume, np.array([p.volume for p in plist]))
            assert np.array_equal(ev.mass, np.array([p.mass for p in plist]))
            for got, want in [(ev.rad, fields.rad)] + list(zip(ev.urel, fields.urel)):
                w = BOX.arrays(box, want, math.nan)
                written = ~np.isnan(w)
                assert written[inner].sum() > 20 and np.array_equal(got[level][written], w[written])
            if e == 0:
                assert np.array_equal(ev.deposit[level][inner], BOX.arrays(box, fields.deposit, 0.)[inner])
