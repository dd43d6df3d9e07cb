"""The cases of the droplet tests, shared by test_droplets_reference_cpu.py (the restatement alone) and
test_gpu_droplets.py (device against restatement).  References are computed once per process and never modified.

Boxes: the tile of the labelling is 16 x 16 cells in 2-D and 8 x 8 x 8 in 3-D, so level 4 (2-D)
and level 3 (3-D) are one tile, level 5 and level 4 two tiles per direction.

Fields are integer patterns scaled by powers of two: a value in the mask is (2^52 + m)*2^-(53 + s) with an odd
integer m < 2^52 and s in 0 .. 4 from the cell numbers: 53 significant bits and five different exponents, so that a
sum of a few of them rounds in its last bits and depends on the order of its terms.

The shapes are given in cell numbers q = (x, y[, z]) from the low corner, 0 .. n - 1 per direction (q = 0 and
q = n - 1 touch a side); they live in the 8 x 8 corner of the (x, y) plane and, in 3-D, in the plane z = 3, unless
they say otherwise.
"""
import functools

import numpy as np

import droplets_reference as DR
import feed_particle_reference as FP
import forces_reference as FR
import sampler_cases as SK
import sampler_reference as R

P, B = R.SIDE_PERIODIC, R.SIDE_BOUNDARY
SIDES = {"periodic": [P]*6, "xclosed": [B, B, P, P, P, P]}
SIDE_NAMES = tuple(SIDES)
BOXES = [(2, 4), (2, 5), (3, 3), (3, 4)]
ZC = 3
IDLAST0 = 40
EXACT, ABOVE = 1e-4, float(np.nextafter(1e-4, 1.))
BELOW = 2.**-14            # a positive value outside the mask


def tval(q):
    x, y, z = (tuple(q) + (0,))[:3]
    m = ((131*x + 71*y + 31*z + 7)*0x9E3779B97F4A7C15) % (1 << 52) | 1
    return float((1 << 52) + m)*2.**-(53 + (x + 2*y + 3*z) % 5)


def uval(q, c):
    x, y, z = (tuple(q) + (0,))[:3]
    m = ((17*x + 29*y + 37*z + 3*c + 1)*0xC2B2AE3D27D4EB4F) % (1 << 52) | 1
    return (-1. if (x + y + z + c) % 3 == 0 else 1.)*float((1 << 52) + m)*2.**-(54 + (3*x + y + 2*z + c) % 4)


def _at(dim, q):
    """index into an array with ghosts"""
    q = tuple(q)
    if dim == 3 and len(q) == 2:
        q = q + (ZC,)
    return tuple(v + 1 for v in reversed(q[:dim]))


def _zeros(dim, level):
    return np.zeros(((1 << level) + 2,)*dim)


def field(dim, level, cells, values=None):
    """an array with T = tval on `cells' (values: q -> a value instead)"""
    a = _zeros(dim, level)
    for q in cells:
        a[_at(dim, q)] = tval(q if dim == 2 or len(q) == 3 else tuple(q) + (ZC,))
    for q, v in (values or {}).items():
        a[_at(dim, q)] = v
    return a


@functools.lru_cache(None)
def velocity(dim, level):
    n = 1 << level
    out = []
    for c in range(dim):
        a = _zeros(dim, level)
        for idx in np.ndindex(*(n,)*dim):
            q = tuple(reversed(idx))
            a[tuple(v + 1 for v in idx)] = uval(q, c)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


def spiral(n):
    """a one-cell-wide square spiral of the n x n plane, from the corner (0, 0) inwards, one cell between its arms;
    the row and the column n - 1 stay empty, so that the arms do not meet through a periodic side"""
    cells, x, y, dx, dy = [(0, 0)], 0, 0, 1, 0
    lo, hi = [0, 0], [n - 2, n - 2]
    taken = {(0, 0)}
    turns = 0
    while turns < 2:
        nx, ny = x + dx, y + dy
        ahead = (nx + dx, ny + dy)
        if not (lo[0] <= nx <= hi[0] and lo[1] <= ny <= hi[1]) or ahead in taken or (nx, ny) in taken:
            dx, dy = -dy, dx
            turns += 1
            continue
        # no touching an earlier arm sideways
        side = [(nx - dy, ny + dx), (nx + dy, ny - dx)]
        if any(s in taken and s != (x, y) for s in side):
            dx, dy = -dy, dx
            turns += 1
            continue
        x, y = nx, ny
        cells.append((x, y))
        taken.add((x, y))
        turns = 0
    return cells


class Case:
    """one event: the tracer T, the second tracer S and alpha (or None), the function text (or None) and its mask,
    min, reset"""

    def __init__(self, name, dim, level, T, min_, S=None, alpha=None, function=None, reset=0.):
        self.name, self.dim, self.level, self.T, self.min, self.reset = name, dim, level, T, min_, reset
        self.S = S if S is not None else _zeros(dim, level)
        self.alpha, self.function = alpha, function
        for a in (self.T, self.S, self.alpha):
            if a is not None:
                a.setflags(write=False)

    def mask(self):
        if self.function is None:
            return None
        if self.function == "S":
            return self.S
        assert self.function == "T - 0.5*S"
        return self.T - 0.5*self.S


def _join_cells(n):
    return {"P1": [(3, n - 1), (3, n - 2), (3, 0), (3, 1)],            # one droplet through the periodic y side
            "F1": [(1, 2), (1, 1), (1, 0)],                            # its last leaf (1, 0) touches a side
            "F2": [(5, n - 1), (5, n - 2), (5, n - 3)],                # its first leaf touches a side, its last not
            "G": [(0, 3), (0, 4)],                                     # entirely on the x side: size 0
            "H": [(6, 3)],                                             # one cell
            "C1": [(3, 4), (4, 4)],                                    # converts
            "C2": [(1, 5), (1, 6)] + ([(2, 6)] if n > 8 else [])}


def _sizes_cells():
    return {"M": [(1, 1), (2, 1), (3, 1), (4, 1), (5, 1)],             # exactly min = 5 counted cells
            "Mm": [(1, 3), (2, 3), (3, 3), (4, 3)],                    # min - 1
            "D1": [(6, 3), (6, 4)], "D2": [(5, 5), (5, 6)],            # touch at a corner only
            "E": [(1, 5), (2, 5)]}


def _chain_cells(n):
    a, b = 2, 5
    return {"A": [(a, n - 1), (a, n - 2)],
            "B": [(a, 0), (a, 1), (a, 2)] + [(x, 2) for x in range(a + 1, b + 1)] + [(b, y) for y in range(3, n)],
            "C": [(b, 0)]}


def _flat(groups):
    return [q for g in groups.values() for q in g]


@functools.lru_cache(None)
def cases(dim, level, sides_name):
    """the cases of one box and one set of sides, by name"""
    n = 1 << level
    out = {}

    def add(case):
        out[case.name] = case

    join = _flat(_join_cells(n))
    T = field(dim, level, join)
    add(Case("join", dim, level, T, 6))
    # min < 0: the largest, the second largest size, and -n: nothing happens
    ndrops = 7
    for m in (-1, -2, -ndrops):
        add(Case("join_min%d" % m, dim, level, T, m))
    add(Case("sizes", dim, level, field(dim, level, _flat(_sizes_cells())), 5, reset=-0.25))
    # a cell at exactly 1e-4 between two cells of the mask stays out; the next double above joins its two
    thr = {(1, 2): tval((1, 2)), (2, 2): EXACT, (3, 2): tval((3, 2)),
           (1, 4): tval((1, 4)), (2, 4): ABOVE, (3, 4): tval((3, 4)), (5, 5): BELOW, (5, 2): tval((5, 2)),
           (6, 2): tval((6, 2))}
    add(Case("threshold", dim, level, field(dim, level, [], thr), 6))
    add(Case("chain", dim, level, field(dim, level, _flat(_chain_cells(n)) + [(3, 4), (3, 5)]), 40))
    # the spiral: in 3-D in every other plane, joined at its outer and at its inner end in turn
    sp = spiral(n)
    if dim == 2:
        cells = sp
    else:
        cells = []
        for z in range(1, n - 1, 2):
            cells += [q + (z,) for q in sp]
            if z + 2 < n - 1:
                cells.append((sp[-1] if (z//2) % 2 == 0 else sp[0]) + (z + 1,))
    add(Case("spiral", dim, level, field(dim, level, cells), -1))
    add(Case("spiral_small", dim, level, field(dim, level, cells), 10))
    add(Case("empty", dim, level, field(dim, level, [], {(2, 2): BELOW, (3, 2): EXACT}), 6))
    full = _zeros(dim, level)
    for idx in np.ndindex(*(n,)*dim):
        full[tuple(v + 1 for v in idx)] = tval(tuple(reversed(idx)))
    add(Case("full", dim, level, full, -1))
    add(Case("full_large_min", dim, level, full.copy(), 1 << 30))
    # the mask from a function: S = 2 T takes C1 out of the mask; where T = 0 and S = -1 the mask has a droplet
    # whose volume, taken from T, is 0: no mass
    S = _zeros(dim, level)
    for q in _join_cells(n)["C1"]:
        S[_at(dim, q)] = 2.*T[_at(dim, q)]
    for q in [(5, 1), (6, 1)]:
        S[_at(dim, q)] = -1.
    add(Case("function", dim, level, T.copy(), 6, S=S, function="T - 0.5*S"))
    add(Case("function_variable", dim, level, T.copy(), 6, S=np.where(S < 0., 0.75, 0.), function="S"))
    # alpha: three droplets that convert, in tag order; alpha = 2^80 at the second makes its mass fall under 1e-20
    three = {"a": [(1, 5), (2, 5)], "b": [(4, 5), (5, 5)], "c": [(1, 2), (2, 2), (2, 1)]}
    alpha = _zeros(dim, level) + 1.
    for idx in np.ndindex(*(n,)*dim):
        q = tuple(reversed(idx))
        alpha[tuple(v + 1 for v in idx)] = 0.5 + ((5*q[0] + 3*q[1] + (q[2] if dim == 3 else 0)) % 13)/16.
    for q in three["b"]:
        alpha[_at(dim, q)] = 2.**80
    add(Case("alpha", dim, level, field(dim, level, _flat(three)), 6, alpha=alpha))
    return out


CASE_NAMES = ("join", "join_min-1", "join_min-2", "join_min-7", "sizes", "threshold", "chain", "spiral",
              "spiral_small", "empty", "full", "full_large_min", "function", "function_variable", "alpha")


def particles(dim):
    """the list before the first event: three particulates"""
    z = 0.05 if dim == 3 else 0.
    pos = np.array([[0.11, 0.23, z], [-0.31, 0.07, -z], [0.02, -0.4, z]])
    ids = np.array([3, 7, 12], dtype=np.uint32)
    vel = np.array([[0.5, -0.25, 2.*z], [0.1, -0.2, -z], [-0.125, 0.0625, 0.]])
    mass = np.array([2e-3, 1.5e-3, 1e-3])
    volume = np.array([1e-3, 1e-3, 5e-4])
    return pos, ids, vel, mass, volume


def particle_list(dim):
    pos, ids, vel, mass, volume = particles(dim)
    return FP.ParticleList([FR.Particulate(list(map(float, pos[q])), int(ids[q]), list(map(float, vel[q])),
                                           float(mass[q]), float(volume[q])) for q in range(len(ids))], IDLAST0)


class Result:
    """what two events of a case in a row leave: per event the info, the droplets, the tracer, and a copy of the list"""


@functools.lru_cache(None)
def reference_run(dim, level, sides_name, name):
    case = cases(dim, level, sides_name)[name]
    box, sides = SK.box(dim, level), SIDES[sides_name]
    pl = particle_list(dim)
    T = case.T.copy()
    out = Result()
    out.tags = DR.tag_droplets(box, sides, case.T if case.mask() is None else case.mask())
    out.tag_array = DR.tag_array(box, out.tags, case.T)
    out.events = []
    for _ in range(2):
        mask = None
        if case.function == "S":
            mask = case.S
        elif case.function is not None:
            mask = T - 0.5*case.S
        info, drops = DR.event(box, sides, pl, T, velocity(dim, level), case.min, case.reset, mask, case.alpha)
        out.events.append((info, drops, T.copy(), list_state(pl)))
    # gfs_domain_remove_droplets on a fresh copy: v is a second field
    v = case.S.copy() + 0.5
    out.remove_info = DR.remove_droplets(box, sides, case.T, v, case.min, -3.)
    out.removed = v
    return out


def list_state(pl):
    """the arrays the device downloads, in list order"""
    ps = pl.plist
    return {"ids": np.array([p.id for p in ps], dtype=np.uint32), "pos": np.array([p.pos for p in ps]).reshape(-1, 3),
            "old": np.array([p.pos_old for p in ps]).reshape(-1, 3), "vel": np.array([p.vel for p in ps]).reshape(-1, 3),
            "mass": np.array([p.mass for p in ps]), "volume": np.array([p.volume for p in ps]),
            "force": np.array([p.force for p in ps]).reshape(-1, 3), "idlast": pl.idlast}
