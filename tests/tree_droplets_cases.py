"""The cases of the droplet tests on refined trees, shared by test_tree_droplets_reference_cpu.py (the restatement
alone, and the host planner) and test_gpu_tree_droplets.py (device against restatement).  References are computed
once per process and never modified.

Trees: those of tree_sampler_cases.TREES, a uniform octree, and two whose leaves span several workgroups of the
labelling (256 consecutive leaves): `big2' (level 6 in level 4) and `big3' (level 4 in level 3, 960 leaves).

A variable is given per level, cells with children included: a case sets the gates of the fill -- the value of the
mask on the cell N with children that a coarse leaf sees beside it -- directly.  A value in the mask is (2^52 + m) *
2^-(53 + s) with an odd m < 2^52 and s in 0 .. 4 from the level and the cell numbers, as in droplets_cases.py: 53
significant bits and five exponents, so that a sum of a few rounds and depends on the order of its terms.
"""
import functools

import numpy as np

import droplets_cases as BC
import feed_particle_reference as FP
import forces_reference as FR
import sampler_reference as R
import tree_droplets_reference as TD
import tree_sampler_cases as TC
import tree_sampler_reference as T
import tree_two_way_cases as TWC

P, B = R.SIDE_PERIODIC, R.SIDE_BOUNDARY
IDLAST0 = BC.IDLAST0
EXACT, ABOVE, BELOW = BC.EXACT, BC.ABOVE, BC.BELOW
OPEN, SHUT = 0.75, 0.

TREES = dict((k, v[:3]) for k, v in TC.TREES.items())
TREES["uniform3"] = (3, lambda x, y, z: 3, [P]*6)
TREES["big2"] = (2, lambda x, y: 6 if (abs(x) < 0.13 and abs(y) < 0.13) else 4, [P]*4)
TREES["big3"] = (3, lambda x, y, z: 4 if (abs(x) < 0.25 and abs(y) < 0.25 and abs(z) < 0.25) else 3, [P]*6)
NAMES = tuple(TREES)
UNIFORM = {"uniform2": 3, "uniform3": 3}
REFINED = tuple(n for n in NAMES if n not in UNIFORM)

BLOBS = (((0.12, 0.1, 0.05), 0.17), ((-0.27, 0.04, 0.), 0.09), ((0.5, -0.22, 0.1), 0.11), ((-0.38, -0.38, -0.3), 0.07),
         ((-0.05, -0.31, 0.2), 0.08))


def spec(name):
    return TREES[name]


@functools.lru_cache(None)
def host_tree(name):
    dim, refine, _sides = spec(name)
    return T.TreeBox(dim, TWC.refined_set(dim, refine))


def shapes(box):
    return [((1 << l) + 2,)*box.dim for l in range(box.level + 1)]


def tval(cell):
    x, y, z = cell.q
    l = cell.level
    m = ((131*x + 71*y + 31*z + 977*l + 7)*0x9E3779B97F4A7C15) % (1 << 52) | 1
    return float((1 << 52) + m)*2.**-(53 + (x + 2*y + 3*z + l) % 5)


def uval(cell, c):
    x, y, z = cell.q
    l = cell.level
    m = ((17*x + 29*y + 37*z + 3*c + 11*l + 1)*0xC2B2AE3D27D4EB4F) % (1 << 52) | 1
    return (-1. if (x + y + z + c + l) % 3 == 0 else 1.)*float((1 << 52) + m)*2.**-(54 + (3*x + y + 2*z + c + l) % 4)


def _at(box, cell):
    i, j, k = cell.ijk
    return (j, i) if box.dim == 2 else (k, j, i)


def zeros(box):
    return [np.zeros(s) for s in shapes(box)]


def variable(box, leaves, gates=OPEN, values=None):
    """per level an array with ghosts: tval on the leaves given, `gates' (a number, or a function of the cell) on every
    cell with children that has one of them below it, 0 elsewhere; values: cell -> a value instead"""
    a = zeros(box)
    inside = set(id(c) for c in leaves)
    for c in leaves:
        a[c.level][_at(box, c)] = tval(c)
        p = c.parent
        while p is not None and id(p) not in inside:
            inside.add(id(p))
            a[p.level][_at(box, p)] = gates(p) if callable(gates) else gates
            p = p.parent
    for c, v in (values or {}).items():
        a[c.level][_at(box, c)] = v
    return a


@functools.lru_cache(None)
def velocity(name):
    box = host_tree(name)
    out = []
    for c in range(box.dim):
        a = zeros(box)
        for cell in TD.interior_cells(box):
            a[cell.level][_at(box, cell)] = uval(cell, c)
        for lev in a:
            lev.setflags(write=False)
        out.append(a)
    return tuple(out)


class Case:
    """one event: the tracer T, the second tracer S, the function text (or None), min, reset"""

    def __init__(self, name, box, T, min_, S=None, function=None, reset=0.):
        self.name, self.T, self.min, self.reset, self.function = name, T, min_, reset, function
        self.S = S if S is not None else zeros(box)
        for a in self.T + self.S:
            a.setflags(write=False)

    def mask(self, T=None):
        """the values of the function at every cell of every level (None: the variable T itself)"""
        T = self.T if T is None else T
        if self.function is None:
            return None
        if self.function == "S":
            return self.S
        assert self.function == "T - 0.5*S"
        return [t - 0.5*s for t, s in zip(T, self.S)]


def _in_blobs(box, cell):
    return any(sum((cell.pos[a] - c[a])**2 for a in range(box.dim)) < r*r for c, r in BLOBS)


def fine_coarse_contacts(box):
    """(f, k, N): a fine leaf, the coarser leaf beside it, the parent of f"""
    out = []
    for f in box.leaves:
        for d in range(box.ndir):
            k = box.neighbor(f, d)
            if k is not None and not k.boundary and box.is_leaf(k) and k.level < f.level:
                out.append((f, k, f.parent))
    return out


def _adjacent(box, a, b):
    return any(box.neighbor(a, d) is b for d in range(box.ndir)) or any(box.neighbor(b, d) is a for d in range(box.ndir))


def situations(name):
    """the crafted masks this tree offers: name -> (leaves, what must come out)"""
    box = host_tree(name)
    sides = spec(name)[2]
    index = {id(c): n for n, c in enumerate(box.leaves)}
    fc = fine_coarse_contacts(box)
    out = {}
    for f, k, _N in fc:                                      # the gate shut: the coarse leaf first, the fine leaf first
        key = "pair_coarse_first" if index[id(k)] < index[id(f)] else "pair_fine_first"
        out.setdefault(key, [f, k])
    for f, k, _N in fc:                                      # a chain of two one-way contacts
        for g, j, _M in fc:
            if g is k and "chain" not in out and index[id(f)] < index[id(k)] < index[id(j)]:
                out["chain"] = [f, k, j]
    for f, k, _N in fc:                                      # two one-way contacts into one coarse leaf
        for g, j, _M in fc:
            if j is k and g is not f and not _adjacent(box, f, g) and "two_into_one" not in out and \
               index[id(f)] < index[id(g)] < index[id(k)]:
                out["two_into_one"] = [f, g, k]
    for f, k, _N in fc:                                      # A ~ C through a periodic side, B -> C one-way
        for d in range(box.ndir):
            if sides[d] == P and TD.on_side(box, k, d) and "periodic_oneway" not in out:
                a = TD.periodic_image(box, k, d)
                if a is not k and index[id(a)] < index[id(f)] < index[id(k)] and not _adjacent(box, a, f):
                    out["periodic_oneway"] = [a, f, k]
    return out


def _ring(box):
    """the leaves one level above the deepest that touch a deepest leaf, by a face or across a corner: a closed ring
    around an inner patch, or nothing"""
    deep = max(c.level for c in box.leaves)
    h = 1./(1 << deep)
    fine = [c for c in box.leaves if c.level == deep]
    lo = [min(c.pos[a] for c in fine) - h/2. for a in range(box.dim)]
    hi = [max(c.pos[a] for c in fine) + h/2. for a in range(box.dim)]
    ring = [c for c in box.leaves if c.level == deep - 1 and
            all(lo[a] - 2.5*h < c.pos[a] < hi[a] + 2.5*h for a in range(box.dim))]
    if not ring or any(TD.touches_a_side(box, c) for c in ring):
        return []
    return ring


@functools.lru_cache(None)
def cases(name):
    box = host_tree(name)
    out = {}

    def add(case):
        out[case.name] = case

    blobs = [c for c in box.leaves if _in_blobs(box, c)]
    add(Case("blobs", box, variable(box, blobs), 12))
    add(Case("blobs_shut", box, variable(box, blobs, SHUT), 12, reset=-0.25))
    for m in (-1, -2):
        add(Case("blobs_min%d" % m, box, variable(box, blobs), m))
    add(Case("full", box, variable(box, box.leaves), -1))
    add(Case("full_shut", box, variable(box, box.leaves, SHUT), 1 << 30))
    add(Case("empty", box, variable(box, [], values={box.leaves[1]: BELOW, box.leaves[2]: EXACT}), 6))
    # exactly 1e-4 stays out, the next double above is in: on leaves and on gates
    thr = {c: (EXACT if n % 3 == 0 else ABOVE) for n, c in enumerate(blobs) if n % 5 < 2}
    add(Case("threshold", box, variable(box, blobs, lambda p: EXACT if (p.q[0] + p.q[1]) % 2 else ABOVE, thr), 12))
    for seed, p in ((1, 0.35), (2, 0.6)):
        rng = np.random.default_rng(1000*seed + len(box.leaves))
        leaves = [c for c in box.leaves if rng.random() < p]
        gates = {id(c): (OPEN if rng.random() < 0.5 else SHUT) for c in TD.interior_cells(box)}
        add(Case("random%d" % seed, box, variable(box, leaves, lambda c: gates[id(c)]), 6, reset=2.**-20))
    for key, leaves in situations(name).items():
        add(Case(key, box, variable(box, leaves, SHUT), 6))
    ring = _ring(box)
    if ring:
        add(Case("ring", box, variable(box, ring), 1 << 20))
    # the mask from a function: S = 2 T on the cells with children makes T - 0.5*S shut every gate the variable opens,
    # and takes every seventh leaf of the blobs out; where T = 0 and S = -1 the mask has leaves whose volume is 0
    T = variable(box, blobs)
    S = zeros(box)
    for c in TD.interior_cells(box):
        if not box.is_leaf(c):
            S[c.level][_at(box, c)] = 2.*T[c.level][_at(box, c)]
    for n, c in enumerate(blobs):
        if n % 7 == 3:
            S[c.level][_at(box, c)] = 2.*T[c.level][_at(box, c)]
    extra = [c for c in box.leaves if not _in_blobs(box, c)][5:8]
    for c in extra:
        S[c.level][_at(box, c)] = -1.
    add(Case("function", box, variable(box, blobs), 12, S=S, function="T - 0.5*S"))
    S2 = variable(box, blobs[::2] + extra, SHUT)
    add(Case("function_variable", box, variable(box, blobs), 12, S=[0.75*(a > 0.) for a in S2], function="S"))
    return out


def case_names(name):
    return tuple(cases(name))


def particles(dim):
    return BC.particles(dim)


def particle_list(dim):
    return BC.particle_list(dim)


class Result:
    """what a case leaves: the tags, per event of two in a row the info, the droplets, the tracer and the list, and
    gfs_domain_remove_droplets"""


def _copy(levels):
    return [np.array(a) for a in levels]


def _lists(box, levels):
    return box.field([np.array(a) for a in levels])


def _arrays(levels):
    return [np.array(a) for a in levels]


@functools.lru_cache(None)
def reference_run(name, cname):
    box = host_tree(name)
    dim, _refine, sides = spec(name)
    case = cases(name)[cname]
    out = Result()
    mask0 = case.T if case.mask() is None else case.mask()
    out.tags = TD.tag_droplets(box, sides, _lists(box, mask0))
    out.leaf_tags = np.array(TD.leaf_tags(box, out.tags), dtype=np.uint32)
    pl = particle_list(dim)
    T = _lists(box, case.T)
    u = [_lists(box, v) for v in velocity(name)]
    out.events = []
    for _ in range(2):
        mask = case.mask(_arrays(T))
        info, drops = TD.event(box, sides, pl, T, u, case.min, case.reset, None if mask is None else _lists(box, mask))
        out.events.append((info, drops, _arrays(T), BC.list_state(pl)))
    v = _lists(box, [s + 0.5 for s in case.S])
    out.remove_info = TD.remove_droplets(box, sides, _lists(box, case.T), v, case.min, -3.)
    out.removed = _arrays(v)
    return out
