"""GfsSourceParticulateVol and GfsSourceParticulateMass (modules/particulatecommon.c:2734-3047), restated on
the explicit cell graph of tests/sampler_reference.py.

Plain Python floats in the reference's operand order, the reference's file:line at every step.  The list is
walked literally as update_vol (:2806-2832) and update_mass (:2964-2991) walk it: every particle writes Rad,
Urelp, Vrelp(, Wrelp) into its cell, the function is evaluated at that cell right after, the volume or the
mass takes source*dt and the deposit variable of the cell takes the source.  Fields are dicts from the ijk of a
leaf (Box.by_ijk) to a float; `arrays' turns them into the arrays with ghosts of the tests.

The source is a Python callable source(V) of a dict V: Rad, Urelp, Vrelp, Wrelp (3-D) as the cell holds them at
that moment, x, y, z (the centre of the cell), t, and the value at the cell of every field of `variables'.
The radius is a parameter (math.pow, glibc's, by default): the device evaluates the same expression with its
own pow.

One choice where the reference has no defined outcome: a particle for which gfs_domain_locate finds no cell
makes the reference dereference NULL (:2812, :2970); it is skipped here, as the library documents.

Test infrastructure only.
"""
import math

VOLUME, MASS = 0, 1


def radius(volume, pow_=math.pow):
    return pow_(3.0*volume/4.0/math.pi, 1./3.)              # :2812, :2970


class Particulate:
    __slots__ = ("pos", "vel", "mass", "volume")

    def __init__(self, pos, vel, mass, volume):
        self.pos = [float(x) for x in pos]
        self.vel = [float(x) for x in vel]
        self.mass, self.volume = float(mass), float(volume)


class Fields:
    """the variables of the object: rad, urel[dim] and the optional deposit, as dicts ijk -> float; a cell that
    is not in a dict has never been written (the tests pre-fill the device fields with a sentinel)"""

    def __init__(self, dim, deposit=True):
        self.rad, self.urel = {}, [{} for _ in range(dim)]
        self.deposit = {} if deposit else None


def event(box, kind, plist, u, dt, t, source, fields, variables=None, pow_=math.pow):
    """source_particulatevol_event (:2834-2852) / source_particulatemass_event (:2993-3012) on the list
    `plist' of Particulate objects, in list order.  u: the velocity components as Box.field () lists;
    variables: name -> Box.field () list.  Returns the sources in list order (None for a skipped particle)."""
    variables = variables or {}
    dim = box.dim
    if fields.deposit is not None:
        # gfs_cell_reset of volsource (:2843-2845) / dmdtvariable (:3003-3005) on the leaves
        for cell in box.leaves:
            fields.deposit[cell.ijk] = 0.
    out = []
    for p in plist:                                         # gts_container_foreach, :2847, :3007
        cell = box.locate(p.pos)                            # :2811, :2969
        if cell is None:
            out.append(None)
            continue
        fields.rad[cell.ijk] = radius(p.volume, pow_)       # :2812, :2970
        for c in range(dim):                                # :2817-2824, :2975-2982
            fields.urel[c][cell.ijk] = box.interpolate(cell, p.pos, u[c]) - p.vel[c]
        pos = box.cell_pos(cell)
        V = {"Rad": fields.rad[cell.ijk], "Urelp": fields.urel[0][cell.ijk], "Vrelp": fields.urel[1][cell.ijk],
             "x": pos[0], "y": pos[1], "z": pos[2] if dim == 3 else 0., "t": t}
        if dim == 3:
            V["Wrelp"] = fields.urel[2][cell.ijk]
        for name, v in variables.items():
            V[name] = box.value(cell, v)
        s = float(source(V))                                # gfs_function_value (spv->source, cell), :2826, :2984
        if kind == VOLUME:
            p.volume += s*dt                                # :2828
        else:
            p.mass += s*dt                                  # :2986
        if fields.deposit is not None:
            fields.deposit[cell.ijk] += s                   # :2830, :2989
        out.append(s)
    return out


def arrays(box, d, fill):
    """a dict ijk -> float as the array with ghosts of the tests ([k][j][i]), `fill' where nothing was written"""
    import numpy as np
    a = np.full((box.n + 2,)*box.dim, float(fill))
    for (i, j, k), v in d.items():
        if box.dim == 2:
            a[j, i] = v
        else:
            a[k, j, i] = v
    return a
