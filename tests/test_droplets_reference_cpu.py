"""The restatement of tests/droplets_reference.py alone, on the cases of tests/droplets_cases.py: the premises the
device tests rest on.  No GPU.

The device labels by a union-find whose roots are smallest traversal indices.  That is right only
if the literal algorithm -- fifo fill in traversal order, `touch' table, chain reduction, renumbering -- gives every
region the tag 1 + its rank by smallest traversal index under face connectivity with periodic sides: asserted here
on every case, against a computation that shares nothing with the restatement but the fields."""
import numpy as np
import pytest

import droplets_cases as C
import droplets_reference as DR
import sampler_cases as SK

ALL = [(dim, level, s) for dim, level in C.BOXES for s in C.SIDE_NAMES]


def morton(dim, level, q):
    """the traversal index of the cell q (from the low corner): bit 0 of a level from x, bit 1 from n - 1 - y, bit 2
    from n - 1 - z"""
    n = 1 << level
    o = [q[0]] + [n - 1 - v for v in q[1:dim]]
    m = 0
    for b in range(level):
        for a in range(dim):
            m |= ((o[a] >> b) & 1) << (dim*b + a)
    return m


def rank_tags(dim, level, sides, mask):
    """1 + the rank of every region by its smallest traversal index: union-find on the interior array"""
    n = 1 << level
    inside = mask[(slice(1, -1),)*dim] > DR.THRESHOLD
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    cells = [tuple(reversed(idx)) for idx in np.ndindex(*(n,)*dim) if inside[idx]]
    for q in cells:
        parent[q] = q
    for q in cells:
        for a in range(dim):
            nb = list(q)
            nb[a] += 1
            if nb[a] == n:
                if sides[2*a] != C.P:
                    continue
                nb[a] = 0
            nb = tuple(nb)
            if nb in parent:
                ra, rb = find(q), find(nb)
                if ra != rb:
                    parent[ra] = rb
    smallest = {}
    for q in cells:
        r = find(q)
        smallest[r] = min(smallest.get(r, 1 << 62), morton(dim, level, q))
    order = {r: k + 1 for k, r in enumerate(sorted(smallest, key=smallest.get))}
    out = np.zeros_like(mask)
    for q in cells:
        out[tuple(v + 1 for v in reversed(q))] = order[find(q)]
    return out, len(order)


@pytest.mark.parametrize("dim,level", C.BOXES)
def test_the_traversal_index_is_the_morton_key(dim, level):
    box = SK.box(dim, level)
    assert [morton(dim, level, cell.q) for cell in box.leaves] == list(range(len(box.leaves)))


@pytest.mark.parametrize("dim,level,sides_name", ALL)
def test_literal_tags_are_ranks_by_smallest_traversal_index(dim, level, sides_name):
    for name in C.CASE_NAMES:
        case = C.cases(dim, level, sides_name)[name]
        ref = C.reference_run(dim, level, sides_name, name)
        mask = case.T if case.mask() is None else case.mask()
        want, n = rank_tags(dim, level, C.SIDES[sides_name], mask)
        assert ref.tags.n == n, name
        assert np.array_equal(ref.tag_array, want), name


def _droplet_of(ref, box, dim, q):
    return ref.tags.v[id(box.by_ijk[tuple(v + 1 for v in (tuple(q) + (C.ZC,))[:dim]) + (0,)*(3 - dim)])]


@pytest.mark.parametrize("dim,level,sides_name", ALL)
def test_the_named_situations_occur(dim, level, sides_name):
    box, n = SK.box(dim, level), 1 << level
    run = lambda name: C.reference_run(dim, level, sides_name, name)
    tag = lambda ref, q: _droplet_of(ref, box, dim, q)
    # join: two blobs joined through a periodic side only; the last-leaf droplets; on a side; one cell
    ref = run("join")
    info, drops = ref.events[0][:2]
    assert info[0] == 7 and ref.tags.ntag == 8      # the fill alone sees the two halves of P1 apart
    g = C._join_cells(n)
    assert tag(ref, g["P1"][0]) == tag(ref, g["P1"][2]) > 0
    first = ref.tags.first
    cellof = lambda q: box.by_ijk[tuple(v + 1 for v in (tuple(q) + (C.ZC,))[:dim]) + (0,)*(3 - dim)]
    assert first[id(cellof(g["P1"][0]))] != first[id(cellof(g["P1"][2]))]
    d = lambda key: drops[tag(ref, g[key][0]) - 1]
    assert (d("F1").boundary, d("F1").size, d("F1").outcome) == (1, 2, "boundary")
    assert (d("F2").boundary, d("F2").size, d("F2").outcome) == (0, 2, "converted")
    assert (d("G").boundary, d("G").size, d("G").outcome) == (1, 0, "boundary")
    assert (d("H").boundary, d("H").size, d("H").outcome) == (0, 1, "size<=1")
    assert d("P1").outcome == "boundary" and d("P1").size == 2
    for key in ("G", "H", "P1", "F1", "F2", "C1", "C2"):      # all smaller than min = 6: reset
        for q in g[key]:
            i, j, k = cellof(q).ijk
            assert (ref.events[0][2][j, i] if dim == 2 else ref.events[0][2][k, j, i]) == 0.
    # min < 0
    sizes = sorted((dr.size for dr in drops), reverse=True)
    assert run("join_min-1").events[0][0][1] == sizes[0] and run("join_min-2").events[0][0][1] == sizes[1]
    assert run("join_min-7").events[0][0] == (7, 0, 0, 0)
    assert np.array_equal(run("join_min-7").events[0][2], C.cases(dim, level, sides_name)["join"].T)
    # sizes: exactly min and min - 1 counted cells; two regions that touch at a corner stay two
    ref = run("sizes")
    info, drops = ref.events[0][:2]
    g = C._sizes_cells()
    d = lambda key: drops[tag(ref, g[key][0]) - 1]
    assert (d("M").size, d("M").outcome) == (5, "size>=min") and (d("Mm").size, d("Mm").outcome) == (4, "converted")
    assert tag(ref, g["D1"][0]) != tag(ref, g["D2"][0]) and info[0] == 5
    # threshold
    ref = run("threshold")
    assert tag(ref, (2, 2)) == 0 and tag(ref, (1, 2)) != tag(ref, (3, 2)) and min(tag(ref, (1, 2)), tag(ref, (3, 2))) > 0
    assert tag(ref, (1, 4)) == tag(ref, (2, 4)) == tag(ref, (3, 4)) > 0 and tag(ref, (5, 5)) == 0
    # chain: three blobs through two periodic joins, a chain of the touch table longer than 1
    ref = run("chain")
    g = C._chain_cells(n)
    assert tag(ref, g["A"][0]) == tag(ref, g["B"][0]) == tag(ref, g["C"][0]) > 0 and ref.tags.n == 2
    assert len({first[id(cellof(g[k][0]))] for k in "ABC" for first in [ref.tags.first]}) == 3
    raw = ref.tags.touch_raw
    assert any(raw[i] > 0 and raw[raw[i]] > 0 for i in range(len(raw)))
    # spiral: one droplet, one cell wide, in every tile
    ref = run("spiral")
    assert ref.tags.n == 1
    inside = C.cases(dim, level, sides_name)["spiral"].T[(slice(1, -1),)*dim] > 0.
    plane = inside if dim == 2 else inside[1]
    nb = sum(np.roll(plane, s, a) for s in (-1, 1) for a in (0, 1))
    assert (nb[plane] <= 2).all() and plane.sum() > n*n//3
    tile = 16 if dim == 2 else 8
    for idx in np.ndindex(*(max(n//tile, 1),)*dim):
        sl = tuple(slice(t*tile, (t + 1)*tile) for t in idx)
        assert inside[sl].any()
    assert run("spiral_small").events[0][1][0].outcome in ("size>=min", "boundary")
    # no droplet; the box as one droplet
    assert run("empty").tags.n == 0 and run("empty").events[0][0] == (0, 0, 0, 0)
    ref = run("full_large_min")
    assert ref.tags.n == 1 and ref.events[0][0][3] == n**dim and not ref.events[0][2][(slice(1, -1),)*dim].any()
    assert run("full").events[0][0] == (1, 0, 0, 0)
    # the function makes the mask, T the volume
    ref = run("function")
    info, drops = ref.events[0][:2]
    g = C._join_cells(n)
    assert tag(ref, g["C1"][0]) == 0 and tag(ref, (5, 1)) > 0
    assert drops[tag(ref, (5, 1)) - 1].outcome == "mass" and drops[tag(ref, (5, 1)) - 1].volume == 0.
    assert run("function_variable").events[0][0][:3] == (1, 6, 0)
    # alpha, and the droplet without mass between two that convert
    ref = run("alpha")
    assert [dr.outcome for dr in ref.events[0][1]] == ["converted", "mass", "converted"]
    ids = ref.events[0][3]["ids"]
    assert list(ids[-2:]) == [C.IDLAST0 + 1, C.IDLAST0 + 2]


@pytest.mark.parametrize("dim,level,sides_name", ALL)
def test_every_set_converts_and_refuses_for_every_reason(dim, level, sides_name):
    outcomes = []
    for name in C.CASE_NAMES:
        outcomes += [dr.outcome for dr in C.reference_run(dim, level, sides_name, name).events[0][1]]
    assert outcomes.count("converted") >= 2
    for reason in ("boundary", "size<=1", "size>=min", "mass"):
        assert reason in outcomes, reason
    assert "outside" not in outcomes


@pytest.mark.parametrize("dim,level,sides_name", ALL)
def test_sums_depend_on_the_order_and_the_second_event_sees_the_reset(dim, level, sides_name):
    ref = C.reference_run(dim, level, sides_name, "sizes")
    drops = ref.events[0][1]
    case = C.cases(dim, level, sides_name)["sizes"]
    # the sums round on the way: for some droplet, the volume in traversal order is not the sum in the opposite
    # order (were every addition exact, the order would not matter)
    reordered = 0
    for key, cells in C._sizes_cells().items():
        full = [tuple(q) + (C.ZC,)*(dim - 2) for q in cells]
        full.sort(key=lambda q: morton(dim, level, q))
        terms = [2.**(-dim*level)*float(case.T[C._at(dim, q)]) for q in full]
        forward = backward = 0.
        for t in terms:
            forward += t
        for t in reversed(terms):
            backward += t
        assert forward in [dr.volume for dr in drops], key
        reordered += forward != backward
    assert reordered
    # the second event works on the reset field: the droplets of the first that were reset are gone
    first, second = ref.events[0][0], ref.events[1][0]
    assert second[0] < first[0] and second[0] == 1      # M alone is left (reset = -0.25 is outside the mask)
    assert (ref.events[0][2][(slice(1, -1),)*dim] == -0.25).sum() == first[3]
