"""The file image of a refined tree (gfship_tree_snapshot_*) and the restart from it (gfship_tree_restart),
through the C ABI against the tree oracle: the image must be, byte for byte, what ftt_cell_write_binary +
gfs_cell_write_binary give for the oracle's tree -- record offsets, flags, the values of the leaves and
the values the non-leaf cells hold since the gfs_cell_coarse_init in the middle of the step (they are not
the restriction of the leaves of the same file)."""
import struct

import numpy as np
import pytest

import gfship
from oracle import oracle as O
from test_gpu_tree import _bc_values, _refine3, periodic_refine
from tree_files import image_from_oracle

pytestmark = pytest.mark.gpu

T, G = O.Tree, gfship.Tree


class Case:
    """a tree of the oracle and the recipe of the same tree on the device"""

    def __init__(self, kind, level, box, nu=0., tracer=False):
        self.kind, self.nu, self.tracer = kind, nu, tracer
        self.dim = 3 if kind in ("cube", "blob") else 2
        self.sides = [gfship.SIDE_BOUNDARY] * 4 if kind == "cavity" else None
        if kind == "periodic":
            self.refine = periodic_refine(level, box)
        elif kind == "cavity":          # the refined lid-driven cavity: finer along the walls
            self.refine = lambda x, y: level + box if (abs(x) > 0.25 or abs(y) > 0.25) else level
        else:
            self.refine = _refine3(kind, level, box)
        self.o = O.Tree(refine=self.refine, dim=self.dim, sides=self.sides)
        self.ot = None
        self._configure_oracle()
        self.ovars = [T.P, T.PMAC, T.U, T.V] + ([T.W] if self.dim == 3 else []) + ([self.ot] if tracer else [])
        self.gvars = [G.P, G.PMAC, G.U, G.V] + ([G.W] if self.dim == 3 else []) + ([G.T0] if tracer else [])
        self.init = [[self.o.values(w, l).copy() for l in range(self.o.depth + 1)] for w in self.ovars]

    def _configure_oracle(self):
        o, dim = self.o, self.dim
        if self.kind == "cavity":
            for c in range(2):
                for d in range(4):
                    o.set_bc_u(c, d, O.BC_DIRICHLET, 1. if (c == 0 and d == 2) else 0.)
        for c in range(dim):
            if self.nu:
                o.set_viscosity(c, self.nu)
        if self.tracer:
            self.ot = o.add_tracer(1)
        for l in range(o.depth + 1):
            c = o.centres(l)
            if self.kind != "cavity":
                zf = np.cos(2. * np.pi * c[2]) if dim == 3 else 1.
                o.values(T.U, l)[...] = (1. - 2. * np.cos(2. * np.pi * c[0]) * np.sin(2. * np.pi * c[1])) * zf
                o.values(T.V, l)[...] = (1. + 2. * np.sin(2. * np.pi * c[0]) * np.cos(2. * np.pi * c[1])) * zf
                if dim == 3:
                    o.values(T.W, l)[...] = 0.5 * np.sin(2. * np.pi * (c[0] + c[1])) * np.sin(2. * np.pi * c[2]) + 0.1
            if self.tracer:
                o.values(self.ot, l)[...] = np.exp(-30. * sum((q - 0.2) ** 2 for q in c))
        for p in (o.projection_params, o.approx_projection_params):
            p.tolerance = 1e-4
        o.set_time(300. if self.kind == "cavity" else 1e30, 0.75)

    def device(self, upload=True):
        """a fresh device tree with the parameters of the oracle's; upload: and its initial values"""
        o = self.o
        g = gfship.Tree(self.refine, dim=self.dim, sides=self.sides)
        assert g.depth == o.depth
        for l in range(o.depth + 1):
            assert np.array_equal(g.flags(l), o.flags(l))
        if self.kind == "cavity":
            for c in range(2):
                vals = _bc_values(o, c, None)
                for d in range(4):
                    g.set_bc_u(c, d, gfship.BC_DIRICHLET, vals)
        for c in range(self.dim):
            if self.nu:
                g.set_viscosity(c, self.nu)
        if self.tracer:
            assert g.add_tracer(1) == G.T0
        if upload:
            for v, gv in enumerate(self.gvars):
                for l in range(o.depth + 1):
                    g.upload(gv, l, self.init[v][l])
        for p in (g.projection_params, g.approx_projection_params):
            p.tolerance = 1e-4
        g.set_time(300. if self.kind == "cavity" else 1e30, 0.75)
        return g

    def interior_cells(self, l):
        return self.o.flags(l)[(slice(1, -1),) * self.dim] != 0


CASES = {"periodic-4-1": ("periodic", 4, 1), "periodic-4-2": ("periodic", 4, 2), "periodic-5-2": ("periodic", 5, 2),
         "cavity": ("cavity", 4, 1, 1e-3), "cube-3-1": ("cube", 3, 1), "blob-3-2": ("blob", 3, 2),
         "tracer": ("periodic", 4, 2, 0., True)}


def _first_difference(a, b, nvars):
    rec = 12 + 8 * nvars
    if len(a) != len(b):
        return "%d bytes, expected %d" % (len(a), len(b))
    for q in range(0, len(a), rec):
        if a[q:q + rec] != b[q:q + rec]:
            return "record %d of %d: %s, expected %s" % (q // rec, len(a) // rec, struct.unpack_from(
                "<Id%dd" % nvars, a, q), struct.unpack_from("<Id%dd" % nvars, b, q))
    return None


@pytest.mark.parametrize("name", sorted(CASES))
def test_image_is_the_oracle_tree_byte_for_byte(name):
    case = Case(*CASES[name])
    o, g = case.o, case.device()
    nv = len(case.gvars)
    o.start()
    g.start()

    def check(what):
        got, want = g.snapshot(case.gvars), image_from_oracle(o, case.ovars)
        ncells = sum(int(case.interior_cells(l).sum()) for l in range(o.depth + 1))
        assert len(want) == ncells * (12 + 8 * nv)
        assert got == want, "%s, %s: %s" % (name, what, _first_difference(got, want, nv))
        return got

    check("after start()")
    o.step()
    g.step()
    check("after 1 step")
    for _ in range(2):
        o.step()
        g.step()
    data = check("after 3 steps")

    # and back: into a fresh tree of the same refinement, every cell of every level
    inner = (slice(1, -1),) * case.dim
    h = case.device(upload=False)
    h.snapshot_read(case.gvars, data)
    for l in range(o.depth + 1):
        cells = case.interior_cells(l)
        for gv, ov in zip(case.gvars, case.ovars):
            assert np.array_equal(h.download(gv, l)[inner][cells], o.values(ov, l)[inner][cells]), (name, gv, l)
    assert h.snapshot(case.gvars) == data
    o.destroy()
    g.destroy()
    h.destroy()


def test_bad_images_are_refused():
    case = Case("periodic", 4, 1)
    g = case.device()
    vars_ = case.gvars
    rec = 12 + 8 * len(vars_)
    data = g.snapshot(vars_)
    assert len(data) == 597 * rec          # 1 + 4 + 16 + 64 + 256 + 256 cells
    with pytest.raises(gfship.GfshipError, match="bytes, not"):
        g.snapshot_read(vars_, data[:-rec])
    with pytest.raises(gfship.GfshipError, match="bytes, not"):
        g.snapshot_read(vars_, data + bytes(rec))
    with pytest.raises(gfship.GfshipError, match="bytes, not"):
        g.snapshot_read(vars_[:-1], data)
    # an image of another tree with the same number of cells: the refined patch one coarse cell to the right
    other = gfship.Tree(lambda x, y: 5 if (-0.1875 < x < 0.3125 and abs(y) <= 0.25) else 4)
    image_other = other.snapshot(vars_)
    assert len(image_other) == len(data) and image_other != data
    with pytest.raises(gfship.GfshipError, match="the tree of the file is not the tree of this simulation"):
        g.snapshot_read(vars_, image_other)
    other.destroy()
    # a flipped leaf bit
    bad = bytearray(data)
    bad[5 * rec] ^= 16
    with pytest.raises(gfship.GfshipError, match="the tree of the file is not the tree of this simulation"):
        g.snapshot_read(vars_, bytes(bad))
    # a child id that is not the cell's
    bad = bytearray(data)
    bad[rec] ^= 1
    with pytest.raises(gfship.GfshipError, match="make sure the file has 2 spatial dimensions"):
        g.snapshot_read(vars_, bytes(bad))
    # a solid fraction
    bad = bytearray(data)
    bad[7 * rec + 4:7 * rec + 12] = struct.pack("<d", 0.5)
    with pytest.raises(gfship.GfshipError, match="solid fractions"):
        g.snapshot_read(vars_, bytes(bad))
    # unknown variables
    with pytest.raises(gfship.GfshipError, match="no tracer"):
        g.snapshot([G.P, G.T0])
    with pytest.raises(gfship.GfshipError, match="variable"):
        g.snapshot([G.P, 99])
    # the tree is as usable as before
    g.snapshot_read(vars_, data)
    assert g.snapshot(vars_) == data
    g.destroy()


@pytest.mark.parametrize("kind,level,box,nu,tracer", [("periodic", 4, 2, 0., False), ("periodic", 4, 2, 1e-2, True),
                                                      ("cube", 3, 1, 0., True), ("cube", 3, 1, 1e-2, False)])
def test_restart_continues_bit_for_bit(kind, level, box, nu, tracer):
    """n steps, the file image, a new tree from it with restart (t, i), m more steps: the leaves, t, dt and the
    iterations of the projections are those of n + m uninterrupted steps, which are the oracle's"""
    n, m = 3, 3
    case = Case(kind, level, box, nu, tracer)
    o, a = case.o, case.device()
    o.start()
    a.start()
    for _ in range(n):
        o.step()
        a.step()
    data, t, i = a.snapshot(case.gvars), a.t, a.i
    assert i == n
    b = case.device(upload=False)
    b.snapshot_read(case.gvars, data)
    b.restart(t, i)
    b.start()
    assert (b.t, b.i, b.dt) == (a.t, a.i, a.dt)
    for _ in range(m):
        o.step()
        a.step()
        b.step()
    inner = (slice(1, -1),) * case.dim
    for x, what in ((a, "uninterrupted"), (b, "restarted")):
        assert (x.t, x.dt, x.i) == (o.t, o.dt, n + m), what
        for xp, op in ((x.projection_params, o.projection_params),
                       (x.approx_projection_params, o.approx_projection_params)):
            assert xp.niter == op.niter, what
        for l in range(o.depth + 1):
            leaf = o.flags(l)[inner] == 1
            for gv, ov in zip(case.gvars, case.ovars):
                assert np.array_equal(x.download(gv, l)[inner][leaf], o.values(ov, l)[inner][leaf]), (what, gv, l)
    o.destroy()
    a.destroy()
    b.destroy()
