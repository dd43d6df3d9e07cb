"""The premises of the cases of GfsFeedParticle (tests/feed_particle_cases.py) and the id rule of the restatement
(tests/feed_particle_reference.py): what the device is compared with in test_gpu_feed_particle.py really holds
the situations a wrong implementation would get wrong."""
import math

import numpy as np
import pytest

import feed_particle_cases as C
import feed_particle_reference as FP
import particulate_sources_cases as K
import sampler_cases as SK


def _outcomes(dim, level, sides_name, fname, e):
    return C.reference_run(dim, level, sides_name, fname)[e].outcomes


@pytest.mark.parametrize("dim,level", C.BOXES)
def test_premises_of_the_candidates(dim, level):
    """on a closed box, with the function the placed candidates are built for"""
    n = 1 << level
    h = 1./n
    box = SK.box(dim, level)
    for e, count in enumerate(C.COUNTS):
        out = _outcomes(dim, level, "closed", C.PREMISE, e)
        assert len(out) == count == len(C.candidates(dim, level, e))
        if count < 70:
            continue
        what = [w for w, _ in out]
        pos = C.candidates(dim, level, e)
        # at least one candidate outside the box
        assert "outside" in what and all((np.abs(pos[q, :dim]) > 0.5).any() for q in range(count) if what[q] == "outside")
        # one exactly on a cell face, one in a corner cell (ghost corners enter its interpolation)
        assert (pos[C.ON_FACE, 0] + 0.5)/h == 3. and what[C.ON_FACE] != "outside"
        assert out[C.ON_FACE][1].ijk[0] == 3        # the tie rule of ftt_cell_locate: the cell below the face
        corner = out[C.IN_CORNER][1].ijk
        assert corner[:dim] == (1,)*dim and what[C.IN_CORNER] == "added"
        # two accepted candidates in one cell, and a massless one with a cell between them
        a, b = C.SHARED
        assert what[a] == what[b] == "added" and out[a][1] is out[b][1]
        assert a < C.BETWEEN < b and what[C.BETWEEN] == "massless" and out[C.BETWEEN][1] is not None
        # accepted and refused candidates on both sides of index 64 and of index 256
        for edge in (64, 256):
            if count > edge + 32:
                for part in (what[edge - 32:edge], what[edge:edge + 32]):
                    assert "added" in part and ("outside" in part or "massless" in part)
    assert box.locate([0.7, 0.1, 0.]) is None


@pytest.mark.parametrize("fname", list(C.FUNCTIONS))
@pytest.mark.parametrize("sides_name", C.SIDE_NAMES)
@pytest.mark.parametrize("dim,level", C.BOXES)
def test_ids_count_the_accepted_candidates_only(dim, level, sides_name, fname):
    states = C.reference_run(dim, level, sides_name, fname)
    idlast, length = C.IDLAST0, K.NPART
    first = np.asarray(K.particles(dim, level, sides_name)[1])
    for e, st in enumerate(states):
        added = [q for q, (w, _) in enumerate(st.outcomes) if w == "added"]
        assert st.idlast == idlast + len(added) and len(st.ids) == length + len(added)
        # the list as created comes first, then the accepted candidates in candidate order, ids without gaps
        assert np.array_equal(st.ids[:K.NPART], first)
        assert np.array_equal(st.ids[length:], np.arange(idlast + 1, idlast + len(added) + 1))
        assert np.array_equal(st.pos[length:], C.candidates(dim, level, e)[added])
        assert (st.old[length:] == 0.).all() and (st.force[length:] == 0.).all()
        assert not (st.mass[length:] < 1.e-20).any()
        if dim == 2:
            assert (st.vel[length:, 2] == 0.).all()
        idlast, length = st.idlast, len(st.ids)
    assert idlast > C.IDLAST0 + 256     # the burst accepts more than a block of candidates
    if fname != "constant":
        # a wrong id rule (an id per candidate, or per candidate with a cell) would show
        what = [w for w, _ in states[-1].outcomes]
        assert "massless" in what[:what.index("added") + 200] and "outside" in what


def test_add_particulate_follows_c_on_a_nan_and_on_the_threshold():
    pl = FP.ParticleList(idlast=7)
    assert FP.add_particulate(pl, [0.]*3, [0.]*3, 1e-3, 0.) is None and pl.idlast == 7
    assert FP.add_particulate(pl, [0.]*3, [0.]*3, 1e-3, 9.9e-21) is None and pl.idlast == 7
    assert FP.add_particulate(pl, [0.]*3, [0.]*3, 1e-3, 1e-20).id == 8
    assert FP.add_particulate(pl, [0.]*3, [0.]*3, 1e-3, math.nan).id == 9 and pl.idlast == 9
    assert [p.id for p in pl.plist] == [8, 9]


def test_position_functions_are_called_in_the_order_x_y_z_per_candidate():
    calls = []
    box = SK.box(2, 3)
    u = [box.field(a) for a in C.velocity(2, 3, 0)]
    feed = FP.Feed(nparts=lambda: calls.append("n") or 2.9, xfeed=lambda: calls.append("x") or 0.1,
                   yfeed=lambda: calls.append("y") or 0.2, zfeed=lambda: calls.append("z") or 0.,
                   mass=lambda V: 1., volume=lambda V: 1.)
    pl = FP.ParticleList()
    FP.event(box, u, pl, feed, 0.)
    assert calls == ["n", "x", "y", "z", "x", "y", "z"]      # (guint) 2.9 is 2; nparts once
    assert [p.id for p in pl.plist] == [1, 2]
    # the defaults of gfs_feed_particle_init feed nothing: one candidate at the origin without a mass
    assert FP.event(box, u, pl, FP.Feed(), 0.)[0][0] == "massless" and pl.idlast == 2
