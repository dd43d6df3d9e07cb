"""GfsSourceParticulateVol and GfsSourceParticulateMass (modules/particulatecommon.c:2734-3047) on a REFINED box:
the restatement of tests/particulate_sources_reference.py on the cell tree of tests/tree_sampler_reference.py.

Plain Python floats in the reference's operand order, the reference's file:line at every step.  locate and the
corner interpolators are TreeBox's.  Two things differ from the restatement on a box of one level:

- the reset.  Both events pass max_depth = 1 to gfs_domain_cell_traverse (:2844, :3004), and ftt_cell_traverse
  stops below that level (src/ftt.c:696, :745): a volume source zeroes the cells of levels 0 and 1
  (FTT_TRAVERSE_ALL), a mass source the LEAVES of level <= 1 (FTT_TRAVERSE_LEAFS) -- none on a tree whose leaves
  are deeper.  Every other cell keeps what it held and deposit[cell] += source (:2830, :2989) adds onto it, event
  after event.  `traverse' below is that traversal, written as the reference's recursion;
- the cell of a particle is the leaf gfs_domain_locate (pos, -1) finds, whatever its level: x, y, z of the function
  are ftt_cell_pos of that leaf, and every other variable is read there.

A variable is one array with ghosts per level as nested lists ([k][j][i], TreeBox.field); the event writes into
them.  The source is a Python callable source(V) of a dict V, as in particulate_sources_reference.py; the radius
function is a parameter (math.pow, glibc's, by default).

A particle for which gfs_domain_locate finds no cell makes the reference dereference NULL (:2812, :2970); it is
skipped here, as the library documents.

Test infrastructure only.
"""
import math

VOLUME, MASS = 0, 1


def radius(volume, pow_=math.pow):
    return pow_(3.0*volume/4.0/math.pi, 1./3.)              # :2812, :2970


def set_value(box, cell, v, x):
    """GFS_VALUE (cell, v) = x"""
    i, j, k = cell.ijk
    a = v[cell.level]
    if box.dim == 2:
        a[j][i] = x
    else:
        a[k][j][i] = x


class Fields:
    """the variables of the object as TreeBox.field () lists, written in place: rad, urel[dim], and the optional
    deposit (volsource, :2797-2803; dmdtvariable, :2954-2960)"""

    def __init__(self, rad, urel, deposit=None):
        self.rad, self.urel, self.deposit = rad, list(urel), deposit


def traverse(cell, max_depth, leafs, func):
    """ftt_cell_traverse (root, FTT_PRE_ORDER, FTT_TRAVERSE_ALL | FTT_TRAVERSE_LEAFS, max_depth, func):
    cell_traverse_pre_order_all (src/ftt.c:689-715) and cell_traverse_leafs (:740-761)"""
    if max_depth >= 0 and cell.level > max_depth:           # :696, :745
        return
    if not leafs or cell.children is None:                  # :700; :748-749
        func(cell)
    if cell.children is not None:                           # :704-713, :750-759
        for ch in cell.children:
            if not ch.destroyed:
                traverse(ch, max_depth, leafs, func)


def reset(box, kind, deposit):
    """gfs_domain_cell_traverse (domain, FTT_PRE_ORDER, FTT_TRAVERSE_ALL, 1, gfs_cell_reset, volsource), :2844-2845;
    (..., FTT_TRAVERSE_LEAFS, 1, gfs_cell_reset, dmdtvariable), :3004-3005.  The traversal of a domain is that of
    the root cell of its boxes: the cell trees of the boundaries are not visited."""
    traverse(box.root, 1, kind == MASS, lambda cell: set_value(box, cell, deposit, 0.))


def event(box, kind, plist, u, dt, t, source, fields, variables=None, pow_=math.pow):
    """source_particulatevol_event (:2834-2852) / source_particulatemass_event (:2993-3012) on the list `plist' of
    objects with pos, vel, mass, volume, in list order.  u: the velocity components as TreeBox.field () lists;
    variables: name -> TreeBox.field () list.  Returns the sources in list order (None for a skipped particle)."""
    variables = variables or {}
    dim = box.dim
    if fields.deposit is not None:
        reset(box, kind, fields.deposit)
    out = []
    for p in plist:                                         # gts_container_foreach, :2847, :3007
        cell = box.locate(p.pos)                            # :2811, :2969: the leaf, whatever its level
        if cell is None:
            out.append(None)
            continue
        rad = radius(p.volume, pow_)                        # :2812, :2970
        set_value(box, cell, fields.rad, rad)
        rel = []
        for c in range(dim):                                # :2817-2824, :2975-2982
            rel.append(box.interpolate(cell, p.pos, u[c]) - p.vel[c])
            set_value(box, cell, fields.urel[c], rel[c])
        pos = box.cell_pos(cell)                            # ftt_cell_pos: of the level of the leaf
        V = {"Rad": rad, "Urelp": rel[0], "Vrelp": rel[1],
             "x": pos[0], "y": pos[1], "z": pos[2] if dim == 3 else 0., "t": t}
        if dim == 3:
            V["Wrelp"] = rel[2]
        for name, v in variables.items():
            V[name] = box.value(cell, v)
        s = float(source(V))                                # gfs_function_value (spv->source, cell), :2826, :2984
        if kind == VOLUME:
            p.volume += s*dt                                # :2828
        else:
            p.mass += s*dt                                  # :2986
        if fields.deposit is not None:
            set_value(box, cell, fields.deposit, box.value(cell, fields.deposit) + s)      # :2830, :2989
        out.append(s)
    return out
