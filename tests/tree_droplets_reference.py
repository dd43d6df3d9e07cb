"""gfs_domain_tag_droplets (src/domain.c:3564-3796), gfs_domain_remove_droplets (:3798-3880) and GfsDropletToParticle
(modules/particulatecommon.c:1163-1404) on a REFINED box, restated on tree_sampler_reference.TreeBox.

Plain Python floats in the reference's order, the reference's file:line at every step.  The tagging is literal: the
fifo fill over the leaves in FTT_PRE_ORDER with both branches of tag_cell_fraction -- the neighbour is a leaf; the
neighbour is a cell with children, tested ITSELF with the value c holds on it before its children on the face are
looked at --, the `touch' table of the periodic sides, the reduction of its chains and the renumbering.  One
deliberate deviation, the library's: the fill does not step into the boundary cells of a side.

closed_form () is the second statement of the same tags: the smallest traversal index over the leaves from which a
leaf can be reached by a directed path inside the mask, then the periodic sides.  undirected () is what a union-find
over all the contacts alone would give; it is wrong wherever a gate is shut.

A variable is one nested list per level (TreeBox.field), index [k][j][i], ghosts included.

Test infrastructure only.
"""
import collections

import droplets_reference as DR
import feed_particle_reference as FP
from sampler_reference import FLATTEN_INDEX, SIDE_PERIODIC, opposite

THRESHOLD = DR.THRESHOLD                                    # src/domain.c:3564


def _set(box, cell, a, x):
    i, j, k = cell.ijk
    if box.dim == 2:
        a[cell.level][j][i] = x
    else:
        a[cell.level][k][j][i] = x


def children_direction(box, cell, d):
    """ftt_cell_children_direction, src/ftt.h:321-355: index[d][i] is the table of ftt_cell_flatten"""
    assert cell.children is not None                        # :345
    return [None if cell.children[i].destroyed else cell.children[i] for i in FLATTEN_INDEX[box.dim][d]]


def interior_cells(box):
    """the cells of the box itself, of every level: FTT_TRAVERSE_ALL"""
    return [c for c in box.cells if c.tree is None]


def on_side(box, cell, d):
    """the cell touches side d of the box: ftt_cell_traverse_boundary (root, d) visits it"""
    a = d//2
    return cell.q[a] == ((1 << cell.level) - 1 if d % 2 == 0 else 0)


def tag_cell_fraction(box, fifo, cell, c, v, tag, seen):
    """:3566-3596.  seen: a Counter of the branches taken"""
    assert box.is_leaf(cell)                                # :3574
    for d in range(box.ndir):                               # ftt_cell_neighbors, src/ftt.h:432-480
        nb = box.neighbor(cell, d)
        if nb is None or nb.boundary:                       # the deviation: no step into a boundary cell
            continue
        if v[id(nb)] == 0 and box.value(nb, c) > THRESHOLD:             # :3577, on the neighbour ITSELF
            if box.is_leaf(nb):                             # :3578-3581
                v[id(nb)] = tag
                fifo.append(nb)
                seen["leaf_coarser" if nb.level < cell.level else "leaf_same"] += 1
            else:                                           # :3582-3594
                od = opposite(d)
                seen["gate_open"] += 1
                for child in children_direction(box, nb, od):
                    if child is not None and v[id(child)] == 0 and box.value(child, c) > THRESHOLD:
                        assert box.is_leaf(child)           # 2:1 grading
                        v[id(child)] = tag
                        fifo.append(child)
                        seen["leaf_finer"] += 1
        elif not box.is_leaf(nb):
            assert v[id(nb)] == 0                           # nobody writes the tag of a cell with children
            if any(ch is not None and box.value(ch, c) > THRESHOLD for ch in children_direction(box, nb, opposite(d))):
                seen["gate_shut"] += 1


def fill(box, c, seen=None):
    """:3741-3744: (v, ntag), v[id (cell)] of every interior cell of every level"""
    seen = collections.Counter() if seen is None else seen
    v = {id(cell): 0 for cell in interior_cells(box)}       # gfs_cell_reset over FTT_TRAVERSE_ALL, :3741-3742
    tag = 0
    for cell in box.leaves:                                 # :3743-3744, FTT_PRE_ORDER over the leaves
        # tag_new_fraction_region, :3604-3615
        if v[id(cell)] == 0 and box.value(cell, c) > THRESHOLD:
            tag += 1
            v[id(cell)] = tag
            fifo = collections.deque([cell])
            while fifo:
                tag_cell_fraction(box, fifo, fifo.popleft(), c, v, tag, seen)
    return v, tag


def periodic_image(box, cell, d):
    """the leaf the ghost cell beyond the periodic side d copies (gfs_domain_bc of the tag, :3748)"""
    ghost = box.neighbor(cell, d)
    assert ghost is not None and ghost.boundary and ghost.level == cell.level and ghost.children is None
    n, a = 1 << cell.level, d//2
    ijk = list(cell.ijk)
    ijk[a] = 1 if cell.ijk[a] == n else n
    return box.by_ijk[(cell.level, tuple(ijk))]


def tag_droplets(box, sides, c, seen=None):
    """gfs_domain_tag_droplets, :3727-3796, on one box (no MPI: unify_tag_range does nothing)"""
    v, tag = fill(box, c, seen)
    out = DR.Tags()
    out.first, out.ntag = dict(v), tag
    touch = [0]*(tag + 1)                                   # :3749
    for d in range(box.ndir):                               # match_box_bc, :3700-3706
        if sides[d] != SIDE_PERIODIC:
            continue
        for cell in box.leaves:                             # ftt_cell_traverse_boundary (root, d), leaves
            if not on_side(box, cell, d):
                continue
            t = v[id(cell)]                                 # match_periodic_bc, :3689-3698
            if t > 0:
                ntag = v[id(periodic_image(box, cell, d))]
                if ntag > 0:
                    DR.touching_regions(t, ntag, touch)
    out.touch_raw = list(touch)
    touching, maxtag = False, 0                             # :3764-3776
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


def contacts(box, c):
    """the directed graph of the fill among the leaves of the mask: (edges u -> v as pairs of traversal indices, the
    one-way contacts (f, k) among them whose reverse is missing)"""
    index = {id(cell): n for n, cell in enumerate(box.leaves)}
    inside = [box.value(cell, c) > THRESHOLD for cell in box.leaves]
    edges = set()
    for n, cell in enumerate(box.leaves):
        if not inside[n]:
            continue
        for d in range(box.ndir):
            nb = box.neighbor(cell, d)
            if nb is None or nb.boundary:
                continue
            if box.is_leaf(nb):
                if inside[index[id(nb)]]:
                    edges.add((n, index[id(nb)]))
            elif box.value(nb, c) > THRESHOLD:
                for child in children_direction(box, nb, opposite(d)):
                    if child is not None and inside[index[id(child)]]:
                        edges.add((n, index[id(child)]))
    oneway = sorted((u, w) for u, w in edges if (w, u) not in edges)
    return edges, oneway


def periodic_contacts(box, sides, c):
    index = {id(cell): n for n, cell in enumerate(box.leaves)}
    out = set()
    for d in range(box.ndir):
        if sides[d] != SIDE_PERIODIC:
            continue
        for n, cell in enumerate(box.leaves):
            if on_side(box, cell, d) and box.value(cell, c) > THRESHOLD:
                m = index[id(periodic_image(box, cell, d))]
                if box.value(box.leaves[m], c) > THRESHOLD:
                    out.add((min(n, m), max(n, m)))
    return out


def _components(n, labels, pairs):
    """the undirected join of the labels (a label per traversal index, None outside) through `pairs' of traversal
    indices: the smallest label of each class"""
    parent = {l: l for l in set(labels) if l is not None}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x
    for a, b in pairs:
        ra, rb = find(labels[a]), find(labels[b])
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return [None if l is None else find(l) for l in labels]


def _ranked(box, labels):
    roots = sorted(set(l for l in labels if l is not None))
    rank = {l: q + 1 for q, l in enumerate(roots)}
    out = DR.Tags()
    out.v = {id(cell): 0 if labels[n] is None else rank[labels[n]] for n, cell in enumerate(box.leaves)}
    out.n = len(roots)
    return out


def closed_form(box, sides, c, periodic_first=False):
    """L (x) = the smallest traversal index of a leaf from which x is reached by a directed path
    inside the mask; fill tag = 1 + rank of L (x); then the periodic sides join fill regions, undirected, and the
    final tag is 1 + rank by the smallest L.  periodic_first: the WRONG order, for the tests -- the periodic contacts
    as symmetric edges of the graph of the fill, and no join afterwards"""
    edges, _ = contacts(box, c)
    if periodic_first:
        edges = set(edges)
        for u, w in periodic_contacts(box, sides, c):
            edges.update(((u, w), (w, u)))
        sides = [None]*len(sides)
    n = len(box.leaves)
    L = [q if box.value(cell, c) > THRESHOLD else None for q, cell in enumerate(box.leaves)]
    changed = True
    while changed:
        changed = False
        for u, w in edges:
            if L[u] < L[w]:
                L[w] = L[u]
                changed = True
    out = _ranked(box, _components(n, L, periodic_contacts(box, sides, c)))
    out.fill = L
    return out


def undirected(box, sides, c):
    """plain connected components of all the contacts, gates ignored: what a union-find alone gives"""
    index = {id(cell): n for n, cell in enumerate(box.leaves)}
    inside = [box.value(cell, c) > THRESHOLD for cell in box.leaves]
    pairs = set(periodic_contacts(box, sides, c))
    for n, cell in enumerate(box.leaves):
        for d in range(box.ndir):
            nb = box.neighbor(cell, d)
            if inside[n] and nb is not None and not nb.boundary and box.is_leaf(nb) and inside[index[id(nb)]]:
                pairs.add((n, index[id(nb)]))
    labels = [q if inside[q] else None for q in range(len(box.leaves))]
    return _ranked(box, _components(len(box.leaves), labels, pairs))


def leaf_tags(box, tags):
    """the tags of the leaves in traversal order"""
    return [tags.v[id(cell)] for cell in box.leaves]


def touches_a_side(box, cell):
    """:1201-1209: a neighbour is a boundary cell"""
    for d in range(box.ndir):
        nb = box.neighbor(cell, d)
        if nb is not None and nb.boundary:
            return True
    return False


def remove_droplets(box, sides, c, v, min_, val):
    """gfs_domain_remove_droplets, :3836-3880.  v is modified in place, on the leaves; returns (n, the min used, cells
    reset)"""
    tags = tag_droplets(box, sides, c)
    n = tags.n
    if not (n > 0 and -min_ < n):                           # :3851
        return n, 0, 0
    sizes = [0]*n
    for cell in box.leaves:                                 # compute_droplet_size, :3805-3810: leaves of any level
        i = tags.v[id(cell)]
        if i > 0:
            sizes[i - 1] += 1
    pmin = DR._select_min(sizes, n, min_)
    reset = 0
    for cell in box.leaves:                                 # reset_small_fraction, :3812-3817
        i = tags.v[id(cell)]
        if i > 0 and sizes[i - 1] < pmin:
            _set(box, cell, v, val)
            reset += 1
    return n, pmin, reset


def droplet_properties(box, tags, c, u):
    """convert_droplets up to :1300: compute_droplet_properties (:1194-1229) over the leaves in traversal order"""
    drops = [DR.Droplet() for _ in range(tags.n)]
    for dr in drops:
        dr.levels = set()
    for cell in box.leaves:
        i = tags.v[id(cell)]
        if i <= 0:
            continue
        dr = drops[i - 1]
        if touches_a_side(box, cell):                       # :1201-1209
            dr.boundary = 1
            continue
        dr.boundary = 0
        h = box.cell_size(cell)                             # :1214: the size of the leaf
        pos = box.cell_pos(cell)
        dr.size += 1                                        # :1220: whatever its level
        vol = pow(h, box.dim)                               # :1221
        dr.volume += vol*box.value(cell, c)                 # :1222
        dr.levels.add(cell.level)
        for a in range(box.dim):                            # :1224-1227
            dr.pos[a] += pos[a]
            dr.vel[a] += box.value(cell, u[a])
    return drops


def event(box, sides, pl, c, u, min_, resetval, mask=None):
    """gfs_droplet_to_particle_event, :1362-1404, and convert_droplets, :1278-1348.  c (the variable, modified in
    place on its leaves), u and mask (the values of the function at every cell of every level, compute_v :1357-1390,
    or None: c) are variables; pl a feed_particle_reference.ParticleList.  Returns ((n, the min used, particles made,
    cells reset), the droplets with their outcome)"""
    tags = tag_droplets(box, sides, c if mask is None else mask)      # :1379 / :1393
    n = tags.n
    if not (n > 0 and -min_ < n):                           # :1381
        return (n, 0, 0, 0), []
    drops = droplet_properties(box, tags, c, u)             # p.c = d->c, :1382
    sizes = [d.size for d in drops]
    pmin = DR._select_min(sizes, n, min_)
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
        cell = box.locate(pos)                              # :1331: gfs_domain_locate (pos, -1), the leaf
        if cell is None:
            dr.outcome = "outside"
            continue
        dr.cell = cell
        volume = dr.volume
        mass = 1.                                           # :1334-1335: a tree has no alpha
        mass *= volume                                      # :1336
        p = FP.add_particulate(pl, pos, vel, volume, mass)  # :1337
        dr.outcome = "mass" if p is None else "converted"
        made += p is not None
    reset = 0
    for cell in box.leaves:                                 # reset_small_fraction, :1187-1192: leaves only
        i = tags.v[id(cell)]
        if i > 0 and sizes[i - 1] < pmin:
            _set(box, cell, c, resetval)
            reset += 1
    return (n, pmin, made, reset), drops
