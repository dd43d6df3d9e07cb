"""gfs_domain_tag_droplets (src/domain.c:3564-3796), gfs_domain_remove_droplets (:3798-3880) and GfsDropletToParticle
(modules/particulatecommon.c:1163-1404), restated on the explicit cell graph of tests/sampler_reference.py.

Plain Python floats in the reference's order, the reference's file:line at every step.  The tagging is literal: the
fifo fill in traversal order, the `touch' table of the periodic sides, the reduction of its chains and the
renumbering.  One deliberate deviation, the library's: the fill does not step into the boundary
cells of a side (the reference's tag_cell_fraction would, :3575-3581, and reads there what the boundary condition
of c left and what the temporary tag variable happened to hold).

Fields are numpy arrays with ghosts, (n+2)^dim, indexed [k][j][i] as everywhere in these tests.

Test infrastructure only.
"""
import collections

import feed_particle_reference as FP
import sampler_reference as R

THRESHOLD = 1e-4                                            # src/domain.c:3564


def _value(box, cell, a):
    i, j, k = cell.ijk
    return float(a[j, i]) if box.dim == 2 else float(a[k, j, i])


def _set(box, cell, a, x):
    i, j, k = cell.ijk
    if box.dim == 2:
        a[j, i] = x
    else:
        a[k, j, i] = x


def touching_regions(tag1, tag2, touch):
    """:3620-3641"""
    if tag2 < tag1:
        tag1, tag2 = tag2, tag1
    elif tag2 == tag1:
        return
    ntag = touch[tag2]
    if ntag == tag1:
        return
    if ntag == 0:
        touch[tag2] = tag1
    else:
        if tag1 < ntag:
            touch[tag2] = tag1
        touching_regions(tag1, ntag, touch)


class Tags:
    """the result of tag_droplets: v[id (leaf)] = the final tag, n = the number of droplets; first[id (leaf)] = the
    tag of the fill alone, ntag its count, touch_raw the `touch' table before its chains are reduced"""


def tag_droplets(box, sides, c):
    """gfs_domain_tag_droplets, :3727-3796, on one box (no MPI: unify_tag_range does nothing)"""
    v = {id(cell): 0 for cell in box.leaves}                # gfs_cell_reset, :3741-3742
    tag = 0
    for cell in box.leaves:                                 # :3743-3744, FTT_PRE_ORDER over the leaves
        # tag_new_fraction_region, :3604-3615
        if v[id(cell)] == 0 and _value(box, cell, c) > THRESHOLD:
            tag += 1
            v[id(cell)] = tag
            fifo = collections.deque([cell])
            while fifo:
                cur = fifo.popleft()
                # tag_cell_fraction, :3566-3596: every neighbour is a leaf
                for d in range(box.ndir):
                    nb = box.neighbor(cur, d)
                    if nb is None or nb.boundary:           # the deviation: no step into a boundary cell
                        continue
                    if v[id(nb)] == 0 and _value(box, nb, c) > THRESHOLD:
                        v[id(nb)] = tag
                        fifo.append(nb)
    out = Tags()
    out.first, out.ntag = dict(v), tag
    # gfs_domain_bc (tag), :3748: the ghost of a periodic side holds the tag of the cell across the box
    touch = [0]*(tag + 1)                                   # :3749
    for d in range(box.ndir):                               # match_box_bc, :3700-3706
        if sides[d] != R.SIDE_PERIODIC:
            continue
        a = d//2
        for cell in box.leaves:                             # ftt_cell_traverse_boundary (root, d): leaves on side d
            if cell.q[a] != (box.n - 1 if d % 2 == 0 else 0):
                continue
            t = v[id(cell)]                                 # match_periodic_bc, :3689-3698
            if t > 0:
                ghost = box.neighbor(cell, d)
                assert ghost is not None and ghost.boundary
                ijk = list(ghost.ijk)
                ijk[a] = 1 if ijk[a] == box.n + 1 else box.n
                ntag = v[id(box.by_ijk[tuple(ijk)])]
                if ntag > 0:
                    touching_regions(t, ntag, touch)
    out.touch_raw = list(touch)
    # :3764-3776
    touching, maxtag = False, 0
    for i in range(1, tag + 1):
        t = touch[i]
        while t > 0:
            touch[i] = t
            t = touch[t]
            touching = True
        if touch[i] == 0 and i > maxtag:
            maxtag = i
    if touching:                                            # :3779-3792
        ntag = 0
        tags = [0]*(maxtag + 1)
        for i in range(1, maxtag + 1):
            if touch[i] == 0:
                touch[i] = i
                ntag += 1
                tags[i] = ntag
        maxtag = ntag
        for cell in box.leaves:                             # fix_touching, :3708-3711
            v[id(cell)] = tags[touch[v[id(cell)]]]
    out.v, out.n = v, maxtag
    return out


def tag_array(box, tags, like):
    """the tags as an array with ghosts (zeros there)"""
    a = like*0.
    for cell in box.leaves:
        _set(box, cell, a, float(tags.v[id(cell)]))
    return a


def _select_min(sizes, n, min_):
    """convert_droplets, :1311-1321; src/domain.c:3863-3872"""
    if min_ >= 0:
        return min_
    tmp = sorted(sizes, reverse=True)                       # qsort (greater)
    assert -1 - min_ < n
    return tmp[-1 - min_]


def remove_droplets(box, sides, c, v, min_, val):
    """gfs_domain_remove_droplets, :3836-3880.  v is modified in place; returns (n, the min used, cells reset)"""
    tags = tag_droplets(box, sides, c)
    n = tags.n
    if not (n > 0 and -min_ < n):                           # :3851
        return n, 0, 0
    sizes = [0]*n
    for cell in box.leaves:                                 # compute_droplet_size, :3805-3810
        i = tags.v[id(cell)]
        if i > 0:
            sizes[i - 1] += 1
    pmin = _select_min(sizes, n, min_)
    reset = 0
    for cell in box.leaves:                                 # reset_small_fraction, :3812-3817
        i = tags.v[id(cell)]
        if i > 0 and sizes[i - 1] < pmin:
            _set(box, cell, v, val)
            reset += 1
    return n, pmin, reset


class Droplet:
    def __init__(self):
        self.pos, self.vel, self.volume, self.boundary, self.size = [0., 0., 0.], [0., 0., 0.], 0., 0, 0
        self.outcome = None


def droplet_properties(box, tags, c, u):
    """convert_droplets up to :1300: compute_droplet_properties (:1194-1229) over the leaves in traversal order"""
    drops = [Droplet() for _ in range(tags.n)]
    for cell in box.leaves:
        i = tags.v[id(cell)]
        if i <= 0:
            continue
        dr = drops[i - 1]
        hit = False
        for d in range(box.ndir):                           # :1201-1209
            nb = box.neighbor(cell, d)
            if nb is not None and nb.boundary:
                dr.boundary = 1
                hit = True
                break
            dr.boundary = 0
        if hit:
            continue
        h = box.cell_size(cell)
        pos = box.cell_pos(cell)
        dr.size += 1                                        # :1220
        vol = pow(h, box.dim)                               # :1221
        dr.volume += vol*_value(box, cell, c)               # :1222
        for a in range(box.dim):                            # :1224-1227
            dr.pos[a] += pos[a]
            dr.vel[a] += _value(box, cell, u[a])
    return drops


def event(box, sides, pl, c, u, min_, resetval, mask=None, alpha=None):
    """gfs_droplet_to_particle_event, :1362-1404, and convert_droplets, :1278-1348.  c (the variable, modified in
    place), u and mask (the values of the function at every cell, or None: c) are arrays with ghosts; alpha: None or
    an array; pl a feed_particle_reference.ParticleList.  Returns ((n, the min used, particles made, cells reset),
    the droplets with their outcome)"""
    tags = tag_droplets(box, sides, c if mask is None else mask)      # :1379 / :1393
    n = tags.n
    if not (n > 0 and -min_ < n):                           # :1381
        return (n, 0, 0, 0), []
    drops = droplet_properties(box, tags, c, u)             # p.c = d->c, :1382
    sizes = [d.size for d in drops]
    pmin = _select_min(sizes, n, min_)
    made = 0
    for dr in drops:                                        # :1323-1340
        if dr.boundary:
            dr.outcome = "boundary"
            continue
        if not (dr.size < pmin and dr.size > 1):
            dr.outcome = "size<=1" if dr.size <= 1 else "size>=min"
            continue
        pos = [dr.pos[a]/dr.size if a < box.dim else 0. for a in range(3)]      # pos.z, vel.z: 0 in 2-D
        vel = [dr.vel[a]/dr.size if a < box.dim else 0. for a in range(3)]
        cell = box.locate(pos)                              # :1331
        if cell is None:
            dr.outcome = "outside"
            continue
        volume = dr.volume
        mass = 1./_value(box, cell, alpha) if alpha is not None else 1.      # :1334-1335
        mass *= volume                                      # :1336
        p = FP.add_particulate(pl, pos, vel, volume, mass)  # :1337
        dr.outcome = "mass" if p is None else "converted"
        made += p is not None
    reset = 0
    for cell in box.leaves:                                 # reset_small_fraction, :1187-1192
        i = tags.v[id(cell)]
        if i > 0 and sizes[i - 1] < pmin:
            _set(box, cell, c, resetval)
            reset += 1
    return (n, pmin, made, reset), drops
