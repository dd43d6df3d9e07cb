"""The literal restatement of gfs_domain_tag_droplets on refined trees (tests/tree_droplets_reference.py) against
its closed form, against plain undirected components, and against the host planner of the library
(gfship_tree_host_tag_droplets: plan_droplets and the order of the device's steps, run on the host).

What is pinned here:
- every situation the issue names occurs in the cases, with the outcome it must have;
- closed form == literal, on every case and on random masks and gates per tree;
- the host planner == literal, on the same;
- undirected components differ from the literal in the named cases: a union-find alone is wrong on a tree.
"""
import collections

import numpy as np
import pytest

import gfship
import tree_droplets_cases as C
import tree_droplets_reference as TD


def _field(box, arrays):
    return box.field([np.array(a) for a in arrays])


def _three(name, arrays):
    box = C.host_tree(name)
    dim, refine, sides = C.spec(name)
    f = _field(box, arrays)
    seen = collections.Counter()
    lit = TD.tag_droplets(box, sides, f, seen)
    return box, lit, TD.closed_form(box, sides, f), TD.undirected(box, sides, f), seen


def _host(name, arrays):
    box = C.host_tree(name)
    dim, refine, sides = C.spec(name)
    return gfship.tree_host_tag_droplets(refine, arrays, len(box.leaves), dim, sides)


@pytest.mark.parametrize("name", C.NAMES)
def test_closed_form_and_host_planner_equal_the_literal_fill_on_every_case(name):
    for cname, case in C.cases(name).items():
        mask = case.T if case.mask() is None else case.mask()
        box, lit, cf, _un, _seen = _three(name, mask)
        want = TD.leaf_tags(box, lit)
        assert TD.leaf_tags(box, cf) == want and cf.n == lit.n, cname
        tags, n, _counts = _host(name, mask)
        assert list(tags) == want and n == lit.n, cname


@pytest.mark.parametrize("name", C.NAMES)
def test_closed_form_and_host_planner_equal_the_literal_fill_on_random_masks_and_gates(name):
    box = C.host_tree(name)
    cells = TD.interior_cells(box)
    rng = np.random.default_rng(77 + len(box.leaves))
    differ = 0
    for trial in range(12):
        p, g = rng.uniform(0.2, 0.9), rng.uniform(0., 1.)
        a = C.zeros(box)
        for c in cells:
            inside = rng.random() < (p if box.is_leaf(c) else g)
            a[c.level][C._at(box, c)] = C.tval(c) if inside else (C.BELOW if rng.random() < 0.5 else 0.)
        box, lit, cf, un, _seen = _three(name, a)
        want = TD.leaf_tags(box, lit)
        assert TD.leaf_tags(box, cf) == want and cf.n == lit.n, trial
        tags, n, _counts = _host(name, a)
        assert list(tags) == want and n == lit.n, trial
        differ += TD.leaf_tags(box, un) != want
    if name in C.UNIFORM:                                # no change of level: the fill is undirected
        assert differ == 0
    else:
        assert differ > 0


def test_the_situations_occur_with_their_outcomes():
    met = collections.Counter()
    branches = collections.Counter()
    for name in C.NAMES:
        box = C.host_tree(name)
        index = {id(c): n for n, c in enumerate(box.leaves)}
        sit = C.situations(name)
        for cname, case in C.cases(name).items():
            mask = case.T if case.mask() is None else case.mask()
            _box, lit, _cf, un, seen = _three(name, mask)
            branches.update(seen)
            same = TD.leaf_tags(box, un) == TD.leaf_tags(box, lit)
            if cname == "pair_coarse_first":             # the gate shut, the coarse leaf first: two droplets
                f, k = sit[cname]
                assert index[id(k)] < index[id(f)] and lit.n == 2 and un.n == 1 and not same
                met[cname] += 1
            elif cname == "pair_fine_first":             # the fine leaf first: one
                f, k = sit[cname]
                assert index[id(f)] < index[id(k)] and lit.n == 1 and seen["gate_shut"] == 1
                met[cname] += 1
            elif cname == "chain":                       # level 4 -> 3 -> 2, two one-way contacts in a row
                f, k, j = sit[cname]
                assert (f.level, k.level, j.level) == (4, 3, 2) and name == "graded"
                assert lit.n == 1 and seen["leaf_coarser"] == 2 and seen["gate_shut"] == 2
                met[cname] += 1
            elif cname == "two_into_one":                # two seeds reach one coarse leaf: it goes with the first
                f, g, k = sit[cname]
                assert lit.n == 2 and lit.v[id(k)] == lit.v[id(f)] == 1 and lit.v[id(g)] == 2 and un.n == 1
                met[cname] += 1
            elif cname == "periodic_oneway":             # A ~ C periodic, B -> C one-way: one droplet, literally
                a, b, c = sit[cname]
                assert index[id(a)] < index[id(b)] < index[id(c)]
                assert lit.ntag == 2 and lit.first[id(a)] == 1 and lit.first[id(b)] == lit.first[id(c)] == 2
                assert lit.n == 1
                # the periodic contact merged into the symmetric graph BEFORE the directed step gives two: {A, C}
                # has the label of A, smaller than that of B, and B stays alone
                wrong = TD.closed_form(box, C.spec(name)[2], _field(box, mask), periodic_first=True)
                assert wrong.n == 2 and wrong.v[id(a)] == wrong.v[id(c)] == 1 and wrong.v[id(b)] == 2
                met[cname] += 1
            ref = C.reference_run(name, cname)
            for e, (info, drops, _T, _state) in enumerate(ref.events):
                for dr in drops:
                    if dr.outcome == "converted" and len(dr.levels) == 2:
                        met["two_sizes"] += 1            # a droplet whose leaves have two sizes
                    if dr.outcome == "converted" and dr.cell.level not in dr.levels:
                        met["centre_in_another_level"] += 1
                    if dr.outcome == "converted" and not box.value(dr.cell, _field(box, mask)) > TD.THRESHOLD:
                        met["centre_outside_the_mask"] += 1
                    if dr.outcome == "boundary" and name in ("walls2", "box3"):
                        met["last_leaf_on_a_boundary"] += 1
                if case.min < 0 and info[0] > 0 and -case.min < info[0]:
                    met["min<0"] += 1
            if case.function == "T - 0.5*S" and name in C.REFINED:
                # the values of the function on the cells with children shut gates the variable's would open
                _b, lit_T, _c, _u, seen_T = _three(name, case.T)
                if seen["gate_shut"] > 0 and seen_T["gate_shut"] == 0 and seen_T["gate_open"] > 0:
                    met["function_shuts_a_gate"] += 1
    for key in ("pair_coarse_first", "pair_fine_first", "chain", "two_into_one", "periodic_oneway", "two_sizes",
                "centre_in_another_level", "centre_outside_the_mask", "last_leaf_on_a_boundary", "min<0",
                "function_shuts_a_gate"):
        assert met[key] > 0, key
    for key in ("leaf_same", "leaf_coarser", "leaf_finer", "gate_open", "gate_shut"):
        assert branches[key] > 0, key


def test_a_union_find_alone_is_wrong_in_the_named_cases():
    differ = []
    for name in C.REFINED:
        for cname in ("pair_coarse_first", "two_into_one", "full_shut"):
            if cname in C.cases(name):
                box, lit, _cf, un, _seen = _three(name, C.cases(name)[cname].T)
                if TD.leaf_tags(box, un) != TD.leaf_tags(box, lit):
                    differ.append((name, cname))
                    assert un.n < lit.n
    assert ("square", "pair_coarse_first") in differ and ("cube", "two_into_one") in differ
    assert ("big3", "full_shut") in differ


def test_the_sums_of_the_cases_depend_on_their_order():
    """the premise of the bit-for-bit comparisons: a droplet's volume changes when its leaves are added backwards"""
    changed = 0
    for name in ("graded", "big2", "big3"):
        box = C.host_tree(name)
        case = C.cases(name)["random1"]
        f = _field(box, case.T)
        tags = C.reference_run(name, "random1").tags
        for i in range(1, tags.n + 1):
            terms = [pow(box.cell_size(c), box.dim)*box.value(c, f) for c in box.leaves if tags.v[id(c)] == i]
            fwd = bwd = 0.
            for t in terms:
                fwd += t
            for t in reversed(terms):
                bwd += t
            changed += fwd != bwd
    assert changed > 0


def test_the_plan_counts_of_the_host_planner():
    """the contacts of the plan are those of the restatement's graph: every pair of leaves in face contact once, the
    fine-coarse ones with a gate, the periodic pairs once"""
    for name in C.NAMES:
        box = C.host_tree(name)
        full = C.cases(name)["full"].T
        _tags, _n, (ncon, ngated, nper) = _host(name, full)
        edges, _oneway = TD.contacts(box, _field(box, full))
        pairs = set((min(a, b), max(a, b)) for a, b in edges)
        assert ncon == len(pairs), name
        assert ngated == len(C.fine_coarse_contacts(box)), name
        assert nper == len(TD.periodic_contacts(box, C.spec(name)[2], _field(box, full))), name
