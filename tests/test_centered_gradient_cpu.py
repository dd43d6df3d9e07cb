"""The one definition of the centred pressure gradient (csrc/centered_gradient.hpp), without a GPU.

The header is plain C++ for the host compiler (its GFSHIP_HOST_DEVICE is empty there), so a small program that
calls centered_gradient on one triple of pressures per record is built with -ffp-contract=off, the setting of
the library.  Its results on a few thousand random triples, with n = 64 and 256, equal the same expression in
numpy float64 bit for bit: v = 0; v += (pc - pm)*n; v += (pn - pc)*n; g = v/2 -- every operation of it is one
IEEE double operation in the order written, and the factors 1. and the division by 1. change no bit."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gerris-fft-particles_amd", "csrc")

PROGRAM = r"""
#include "centered_gradient.hpp"
#include <cstdio>
#include <cstdlib>
// record: pm pc pn
int main (int argc, char ** argv)
{
  const double rn = atof (argv[1]);
  FILE * in = fopen (argv[2], "rb"), * out = fopen (argv[3], "wb");
  if (!in || !out) return 1;
  double r[3];
  while (fread (r, sizeof (double), 3, in) == 3) {
    const double v = centered_gradient (r[0], r[1], r[2], rn);
    fwrite (&v, sizeof (double), 1, out);
  }
  return fclose (out) != 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("centered_gradient")
    src, exe = str(tmp / "centered_gradient.cpp"), str(tmp / "centered_gradient")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
                    "-I", CSRC, src, "-o", exe], check=True, capture_output=True, text=True, timeout=120)

    def run(n, records):
        fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
        np.ascontiguousarray(records, dtype=np.float64).tofile(fin)
        subprocess.run([exe, str(n), fin, fout], check=True, timeout=60)
        return np.fromfile(fout, dtype=np.float64)
    return run


@pytest.mark.parametrize("n", [64, 256])
def test_centered_gradient_is_the_expression_in_float64(program, n):
    rng = np.random.default_rng(n)
    # pressures of a smooth field (neighbours close to each other, the differences cancel digits) and unrelated ones
    base = rng.standard_normal((4096, 1))
    t = np.concatenate([base + 1e-3 * rng.standard_normal((4096, 3)), rng.standard_normal((4096, 3)),
                        np.zeros((1, 3)), np.array([[1., 1., 1.], [0., 1., 0.], [-1., 0., 1.]])])
    pm, pc, pn = (t[:, k].astype(np.float64) for k in range(3))
    rn = np.float64(n)
    v = np.zeros_like(pc)
    v = v + (pc - pm) * rn
    v = v + (pn - pc) * rn
    want = v / 2.
    got = program(n, t)
    assert got.shape == want.shape
    assert np.all(got == want)
    assert np.count_nonzero(want) > 8000
