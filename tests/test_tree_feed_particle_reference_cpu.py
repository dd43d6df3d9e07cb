"""The premises of the cases of GfsFeedParticle on refined trees (tests/tree_feed_particle_cases.py) and the id rule
of the restatement (tests/feed_particle_reference.py) on a tree: what the device is compared with in
test_gpu_tree_feed_particle.py really holds the situations a wrong implementation would get wrong."""
import numpy as np
import pytest

import tree_feed_particle_cases as C
import tree_sampler_reference as T
from sampler_reference import SIDE_BOUNDARY, SIDE_PERIODIC


def test_the_restatement_runs_on_a_tree_box_as_it_stands():
    box = C.host_tree("graded")
    assert isinstance(box, T.TreeBox)
    for method in ("locate", "interpolate", "cell_pos", "value"):
        assert callable(getattr(box, method))
    assert sorted(set(c.level for c in box.leaves)) == [2, 3, 4]


@pytest.mark.parametrize("name", C.TREES)
def test_premises_of_the_candidates(name):
    """with the function the placed candidates are built for"""
    box = C.host_tree(name)
    dim, _refine, sides = C.spec(name)
    refined = name in C.REFINED
    levels = sorted(set(c.level for c in box.leaves))
    assert len(levels) >= (2 if refined else 1)
    run = C.reference_run(name, C.PREMISE)
    for e, count in enumerate(C.COUNTS):
        out = run[e].outcomes
        pos = C.candidates(name, e)
        assert len(out) == count == len(pos)
        if count < 70:
            continue
        what = [w for w, _ in out]
        cells = [c for _, c in out]
        # the random candidates outside the box have no cell, whatever the side they are beyond
        assert what.count("outside") > count//8
        assert all((np.abs(pos[q, :dim]) > 0.5).any() == (what[q] == "outside") for q in range(count))
        # a leaf of every level
        assert sorted(set(cells[q].level for q in C.IN_LEVEL)) == levels
        # on a face between a fine and a coarse leaf: the tie rule of ftt_cell_locate takes the leaf below the face
        P = C.placed(name)
        assert cells[C.ON_FACE] is P.face_leaf and pos[C.ON_FACE, 0] == P.face_leaf.pos[0] + box.cell_size(P.face_leaf)/2.
        around = C.leaves_around(box, pos[C.ON_FACE])
        assert len(around) >= 2 and (len(set(c.level for c in around)) == 2) == refined
        # on a corner where the level changes
        assert cells[C.ON_CORNER] is not None
        around = C.leaves_around(box, pos[C.ON_CORNER])
        assert len(around) >= 3 and (len(set(c.level for c in around)) >= 2) == refined
        # a leaf whose corner interpolators hold cells of another level, and one whose corners see its own level only
        if refined:
            assert cells[C.IN_TABLE] is P.table_leaf and len(C.corner_levels(box, P.table_leaf)) > 1
        assert cells[C.IN_UNIFORM] is P.uniform_leaf and C.corner_levels(box, P.uniform_leaf) == {P.uniform_leaf.level}
        # exactly on a side of the box: inside
        assert pos[C.ON_SIDE, 0] == 0.5 and cells[C.ON_SIDE] is not None
        # just outside a side: no cell, periodic or not (gfs_domain_locate does not wrap)
        assert what[C.OUT_X] == what[C.OUT_LAST] == "outside"
        assert (np.abs(pos[C.OUT_X, :dim]) > 0.5).tolist() == [True] + [False]*(dim - 1)
        assert (np.abs(pos[C.OUT_LAST, :dim]) > 0.5).tolist() == [False]*(dim - 1) + [True]
        # two accepted candidates in one leaf, and a massless one with a leaf between them
        a, b = C.SHARED
        assert what[a] == what[b] == "added" and cells[a] is cells[b]
        assert a < C.BETWEEN < b and what[C.BETWEEN] == "massless" and cells[C.BETWEEN] is not None
        # accepted and refused candidates on both sides of candidate 64 and of candidate 256
        for edge in (64, 256):
            if count > edge + 32:
                for part in (what[edge - 32:edge], what[edge:edge + 32]):
                    assert "added" in part and ("outside" in part or "massless" in part)
        # the random candidates reach leaves of every level
        assert sorted(set(c.level for c in cells[32:] if c is not None)) == levels


def test_both_kinds_of_side_are_left():
    """the candidate beyond +x and the one beyond the + side of the last axis leave through a GfsBoundary side on
    some trees and through a periodic side on others"""
    kinds = set()
    for name in C.TREES:
        dim, _refine, sides = C.spec(name)
        kinds.add(sides[0])
        kinds.add(sides[2*(dim - 1)])
    assert kinds == {SIDE_BOUNDARY, SIDE_PERIODIC}


@pytest.mark.parametrize("fname", list(C.FUNCTIONS))
@pytest.mark.parametrize("name", C.TREES)
def test_ids_count_the_accepted_candidates_only(name, fname):
    dim = C.spec(name)[0]
    states = C.reference_run(name, fname)
    idlast, length = C.IDLAST0, C.NPART
    first = np.asarray(C.particles(name)[1])
    for e, st in enumerate(states):
        added = [q for q, (w, _) in enumerate(st.outcomes) if w == "added"]
        assert st.idlast == idlast + len(added) and len(st.ids) == length + len(added)
        # the list as created comes first, then the accepted candidates in candidate order, ids without gaps
        assert np.array_equal(st.ids[:C.NPART], first)
        assert np.array_equal(st.ids[length:], np.arange(idlast + 1, idlast + len(added) + 1))
        assert np.array_equal(st.pos[length:], C.candidates(name, e)[added])
        assert (st.old[length:] == 0.).all() and (st.force[length:] == 0.).all()
        assert not (st.mass[length:] < 1.e-20).any()
        if dim == 2:
            assert (st.vel[length:, 2] == 0.).all()
        idlast, length = st.idlast, len(st.ids)
    assert idlast > C.IDLAST0 + 256     # more than a block of candidates is accepted
    what = [w for w, _ in states[-1].outcomes]
    assert "outside" in what            # a refused candidate takes no id: an id per candidate would show
    if fname != "constant":
        assert "massless" in what[:what.index("added") + 200]


@pytest.mark.parametrize("name", C.REFINED)
def test_the_centre_of_the_leaf_tells_the_levels_apart(name):
    """x, y, z of the functions are ftt_cell_pos of the leaf, at its level: the masses of `xyt' of two candidates in
    leaves of different levels differ from what the centre of a cell of one level would give"""
    box = C.host_tree(name)
    run = C.reference_run(name, "xyt")
    e = 2
    depth = box.level
    pos = C.candidates(name, e)
    coarse = [q for q, (w, c) in enumerate(run[e].outcomes) if c is not None and c.level < depth]
    assert coarse
    q = coarse[0]
    centre = box.cell_pos(run[e].outcomes[q][1])
    h = 1./(1 << depth)
    fine_centre = [-0.5 + (np.floor((pos[q, a] + 0.5)/h) + 0.5)*h for a in range(box.dim)]
    assert list(centre[:box.dim]) != fine_centre
