"""GfsOutputSimulation and the restart from its file on refined trees, through the front end (gfship2D / gfship3D):
a run writes the simulation in the middle and at the end, a second run starts from the file of the middle.  The
bytes of the cell data are pinned against the oracle at the ABI (tests/test_gpu_tree_snapshot.py); here the tree of
the file, the GfsBox line, the text formats and the restart are."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import oracle as O
from tree_files import preorder

pytestmark = pytest.mark.gpu

BIN = os.path.join(ROOT, "gerris-fft-particles_amd", "bin")
CASES = os.path.join(ROOT, "tests", "cases")


def _oracle_tree(name):
    if name == "refined_tracer.gfs":
        return O.Tree(periodic=(4, 2))
    refine = lambda x, y, z: 4 if max(abs(x), abs(y), abs(z)) > 0.25 else 3
    return O.Tree(refine=refine, dim=3, sides=[O.SIDE_BOUNDARY] * 6)


def _cell_data(raw):
    """(variables, image) of a simulation file with a binary tree"""
    names = re.search(rb"variables = (\S+)", raw).group(1).decode().split(",")
    b = raw.index(b"} {\n", raw.index(b"\nGfsBox {")) + 4
    return names, raw[b:]


def _compare(dim, *args):
    return subprocess.run([os.path.join(BIN, "gfshipcompare%dD" % dim)] + list(args),
                          capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("binary", [1, 0])
@pytest.mark.parametrize("name,dim,defs,names", [
    ("refined_tracer.gfs", 2, ["-DLEVEL=4", "-DBOX=2", "-DNSTEPS=8"], ["U", "V", "P", "T"]),
    ("refined_cavity_3d.gfs", 3, ["-DLEVEL=3", "-DNSTEPS=8"], ["U", "V", "W", "P"])])
def test_front_end_writes_and_restarts_a_refined_tree(tmp_path, name, dim, defs, names, binary):
    exe = os.path.join(BIN, "gfship%dD" % dim)
    case = open(os.path.join(CASES, name)).read()
    extra = ("  OutputSimulation { istart = 4 istep = 100 } mid.gfs { binary = %d }\n"
             "  OutputSimulation { start = end } end.gfs { binary = 1 }\n"
             "  OutputSimulation { start = end } end.txt { format = text }\n" % binary)
    if "OutputScalarNorm { start = end } stdout { v = U }" not in case:
        extra += "".join("  OutputScalarNorm { start = end } stdout { v = %s }\n" % v for v in names if v != "T")
    k = case.rindex("}", 0, case.rindex("GfsBox"))
    (tmp_path / "run.gfs").write_text(case[:k] + extra + case[k:])
    r = subprocess.run([exe] + defs + ["run.gfs"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    stdout = r.stdout
    mid, end = tmp_path / "mid.gfs", tmp_path / "end.gfs"
    assert b"GfsTime { i = 4 " in mid.read_bytes() and b"GfsTime { i = 8 " in end.read_bytes()
    assert b"Refine" not in mid.read_bytes()              # the tree follows
    (tmp_path / "first").mkdir()
    first = tmp_path / "first" / "end.gfs"
    os.rename(str(end), str(first))

    # ---- the file of the end: the tree is the oracle's, leaf for leaf
    o = _oracle_tree(name)
    cells = preorder([o.flags(l) for l in range(o.depth + 1)], dim)
    nleaves = sum(1 for c in cells if c[3])
    raw = first.read_bytes()
    variables, data = _cell_data(raw)
    rec = 12 + 8 * len(variables)
    assert data[len(cells) * rec:].startswith(b"}\n"), "the cell data is not %d records" % len(cells)
    flags = [struct.unpack_from("<I", data, q * rec)[0] for q in range(len(cells))]
    assert flags == [cid | (16 if leaf else 0) for _, _, cid, leaf in cells]
    assert all(struct.unpack_from("<d", data, q * rec + 4)[0] == -1. for q in range(len(cells)))
    assert int(re.search(rb"GfsBox \{ id = 1 pid = -1 size = (\d+) ", raw).group(1)) == nleaves
    # the norms the run printed at the end are those of the leaves of the file
    t = float(re.search(rb"GfsTime \{ i = 8 t = (\S+)", raw).group(1))
    lines = stdout.splitlines()
    for v in names:
        col = variables.index(v)
        a = np.array([struct.unpack_from("<d", data, q * rec + 12 + 8 * col)[0] for q, c in enumerate(cells) if c[3]])
        w = np.array([(1. / (1 << c[0])) ** dim for c in cells if c[3]])
        want = "%s time: %g first: % 10.3e second: % 10.3e infty: % 10.3e" % (
            v, t, (w * abs(a)).sum() / w.sum(), math.sqrt((w * a * a).sum() / w.sum()), abs(a).max())
        assert want in lines, (want, [l for l in lines if l.startswith(v + " time")])
    # format = text: one line per leaf, in traversal order, with the centre of the leaf
    text = [l for l in (tmp_path / "end.txt").read_text().splitlines() if not l.startswith("#")]
    assert len(text) == nleaves
    centres = [o.centres(l) for l in range(o.depth + 1)]
    got = np.array([[float(x) for x in l.split()[:3]] for l in text])
    want = np.array([[float("%g" % centres[l][c][idx]) for c in range(dim)] + [0.] * (3 - dim)
                     for l, idx, _, leaf in cells if leaf])
    assert np.array_equal(got, want)
    o.destroy()

    # ---- the second run, from the file of the middle
    r = subprocess.run([exe, "mid.gfs"], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    a, b = first.read_bytes(), end.read_bytes()
    for v in names:
        c = _compare(dim, "-v", str(first), str(end), v)
        assert c.returncode == 0, c.stderr
        err = float(re.search(r"total err first:\s*(\S+) second:\s*(\S+) infty:\s*(\S+)", c.stderr).group(3))
        print("%s binary = %d: %s infty %g" % (name, binary, v, err))
        if binary:
            assert err == 0., v
        else:
            assert 0. < err < 1e-4, v
    if binary:
        assert re.search(rb"GfsTime \{[^}]*\}", a).group(0) == re.search(rb"GfsTime \{[^}]*\}", b).group(0)
