"""Simulation files of refined trees, on the CPU: the helper that writes the expected file image of an oracle
tree (tests/tree_files.py) is pinned on the oracle's walk of the uniform tree, which tests/test_oracle_snapshot.py
pins on the reference's format; and the comparison tool (gfshipcompare2D/3D) on two different trees, against a
numpy restatement of difference_tree + inject (tools/gfscompare.c:153-214)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O
from tree_files import compare_norms, image, image_from_oracle, preorder

BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin")


@pytest.mark.parametrize("dim,level", [(2, 3), (3, 2)])
def test_image_helper_matches_the_uniform_walk(dim, level):
    rng = np.random.default_rng(11)
    tree = O.Tree(refine=(lambda x, y: level) if dim == 2 else (lambda x, y, z: level), dim=dim)
    assert tree.depth == level
    dom = O.Domain(dim, level, [O.SIDE_PERIODIC] * 6)
    which = [O.Tree.U, O.Tree.P]
    fields = [dom.field() for _ in which]
    for w, f in zip(which, fields):
        for l in range(level + 1):
            a = rng.standard_normal(f.level(l).shape)     # every level: the non-leaf cells are no restriction
            f.level(l)[...] = a
            tree.values(w, l)[...] = a
    want = dom.snapshot_tree(fields)
    got = image_from_oracle(tree, which)
    cells = sum((1 << dim) ** l for l in range(level + 1))
    assert len(want) == cells * 28 == {2: 2380, 3: 2044}[dim]
    assert got == want
    tree.destroy()


def test_image_helper_counts_the_cells_of_a_refined_tree():
    tree = O.Tree(periodic=(4, 2))
    cells = preorder([tree.flags(l) for l in range(tree.depth + 1)], 2)
    assert len(cells) == 1765 == sum(int((tree.flags(l)[1:-1, 1:-1] != 0).sum()) for l in range(tree.depth + 1))
    assert sum(1 for c in cells if c[3]) == 1324
    tree.destroy()


# ---- the comparison tool on two different trees

def _tree(spec):
    kind = spec[0]
    if kind == "periodic":
        return O.Tree(periodic=spec[1:])
    if kind == "uniform":
        return O.Tree(refine=lambda x, y: spec[1])
    if kind == "uniform3":
        return O.Tree(refine=lambda x, y, z: spec[1], dim=3)
    assert kind == "cube"
    level, box = spec[1:]
    inside = lambda *q: all(abs(x) <= 0.25 for x in q)
    return O.Tree(refine=lambda x, y, z: level + box if inside(x, y, z) else level, dim=3)


def _random_tree(spec, rng):
    """flags, and two variables with random values on every cell of every level"""
    tree = _tree(spec)
    flags = [tree.flags(l).copy() for l in range(tree.depth + 1)]
    values = [[rng.standard_normal(f.shape) for f in flags] for _ in range(2)]
    dim = tree.dim
    tree.destroy()
    return flags, values, dim


def _write(path, flags, values, names, dim, binary, t=0.5, i=7):
    data = image(flags, values, dim)
    nleaf = sum(1 for c in preorder(flags, dim) if c[3])
    head = ("# Gerris Flow Solver %dD version 1.3.2 (test)\n"
            "1 %d GfsSimulation GfsBox GfsGEdge { version = 120812 variables = %s %s} {\n"
            "  GfsTime { i = %d t = %.17g }\n}\n"
            "GfsBox { id = 1 pid = -1 size = %d x = 0 y = 0 z = 0 } {\n"
            % (dim, dim, ",".join(names), "binary = 1 " if binary else "", i, t, nleaf)).encode()
    if not binary:
        rec = 12 + 8 * len(values)
        lines = []
        for o in range(0, len(data), rec):
            flag = int.from_bytes(data[o:o + 4], "little")
            vals = np.frombuffer(data[o + 12:o + rec], dtype="<f8")
            lines.append("%u -1 " % flag + " ".join("%.17g" % v for v in vals))
        data = ("\n".join(lines) + "\n").encode()
    tail = b"}\n" + "".join("1 1 %s\n" % d for d in ("right", "top", "front")[:dim]).encode()
    with open(path, "wb") as f:
        f.write(head + data + tail)


def _compare(dim, *args):
    return subprocess.run([os.path.join(BIN, "gfshipcompare%dD" % dim)] + list(args),
                          capture_output=True, text=True, timeout=120)


def _norms(r):
    m = re.search(r"total err first:\s*(\S+) second:\s*(\S+) infty:\s*(\S+) w: (\S+)", r.stderr)
    assert m, r.stderr
    return [float(x) for x in m.groups()]


PAIRS = [(("periodic", 4, 1), ("uniform", 4)), (("uniform", 5), ("periodic", 4, 1)),
         (("periodic", 4, 2), ("periodic", 4, 1)), (("cube", 2, 1), ("uniform3", 3))]


@pytest.mark.parametrize("binary", [True, False])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%s-vs-%s" % ("_".join(map(str, p[0])), "_".join(map(str, p[1]))))
def test_compare_tool_on_different_trees(tmp_path, pair, binary):
    rng = np.random.default_rng(5)
    A, B = _random_tree(pair[0], rng), _random_tree(pair[1], rng)
    dim = A[2]
    pa, pb = str(tmp_path / "a.gfs"), str(tmp_path / "b.gfs")
    _write(pa, A[0], A[1], ["P", "U"], dim, binary)
    _write(pb, B[0], [B[1][1], B[1][0]], ["U", "P"], dim, binary)        # another column order
    for (f1, T1), (f2, T2) in (((pa, A), (pb, B)), ((pb, B), (pa, A))):       # both argument orders
        for v, name in enumerate(["P", "U"]):
            for constant in (False, True):
                r = _compare(dim, *(["-v"] + (["-C"] if constant else []) + [f1, f2, name]))
                assert r.returncode == 0, r.stderr
                want = compare_norms(T1[0], T1[1][v], T2[0], T2[1][v], dim, constant=constant)
                assert _norms(r) == pytest.approx(list(want), rel=2e-3), (f1, f2, name, constant)
    # not weighted
    r = _compare(dim, "-v", "-w", pa, pb, "P")
    assert _norms(r) == pytest.approx(list(compare_norms(A[0], A[1][0], B[0], B[1][0], dim, weighted=False)), rel=2e-3)
    # a refined file against itself: exactly zero
    r = _compare(dim, "-v", pa, pa, "U")
    assert r.returncode == 0 and _norms(r)[:3] == [0., 0., 0.]
    # a file of the other dimension is refused
    r = _compare(5 - dim, "-v", pa, pb, "P")
    assert r.returncode == 1, r.stderr


def test_the_stored_value_of_a_non_leaf_cell_is_what_is_compared(tmp_path):
    """FILE1 coarse, FILE2 fine: the error of a coarse leaf is taken against the record of the non-leaf cell
    of FILE2 at that place, whatever its children hold"""
    rng = np.random.default_rng(8)
    A, B = _random_tree(("uniform", 3), rng), _random_tree(("uniform", 4), rng)
    pa, pb = str(tmp_path / "a.gfs"), str(tmp_path / "b.gfs")
    _write(pa, A[0], A[1], ["P", "U"], 2, True)
    _write(pb, B[0], B[1], ["P", "U"], 2, True)
    e = (A[1][0][3] - B[1][0][3])[1:-1, 1:-1]          # level 3 of both, the non-leaf cells of B
    assert _norms(_compare(2, "-v", pa, pb, "P")) == pytest.approx(
        [np.abs(e).mean(), np.sqrt((e * e).mean()), np.abs(e).max(), 1.], rel=2e-3)
    restricted = B[1][0][4][1:-1, 1:-1].reshape(8, 2, 8, 2).mean(axis=(1, 3))
    assert np.abs(restricted - B[1][0][3][1:-1, 1:-1]).max() > 0.1     # and they are no restriction


def test_truncated_refined_file_is_an_error(tmp_path):
    rng = np.random.default_rng(2)
    A = _random_tree(("periodic", 4, 1), rng)
    pa = str(tmp_path / "a.gfs")
    _write(pa, A[0], A[1], ["P", "U"], 2, True)
    raw = open(pa, "rb").read()
    cut = raw.index(b"} {\n", raw.index(b"GfsBox {")) + 4 + 28 * 300
    open(str(tmp_path / "t.gfs"), "wb").write(raw[:cut] + b"}\n1 1 right\n1 1 top\n")
    r = _compare(2, "-v", str(tmp_path / "t.gfs"), pa, "P")
    assert r.returncode == 1 and "not a valid simulation file" in r.stderr
