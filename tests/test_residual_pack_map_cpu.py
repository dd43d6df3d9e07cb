"""The task-to-cell map of residual_restrict_pack_kernel (csrc/residual_pack_map.hpp), without a GPU.

The header is plain C++ once __host__ and __device__ are defined away, so a small program walks the tasks of a
level with the host compiler, as the kernel's workgroups do, and counts: every cell (I, j, k) of the level is
owned by exactly one task (the norm counts it once), every coarse cell is written by exactly one, every cell a
task copies into the skewed layout or restricts is one it has computed, and everything stays inside the task's
buffer of 32 lines of ROWS + 8 cells.  n = 64 and 128, with 64 rows per block as the kernel has them."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "gerris-fft-particles_amd", "csrc")

PROGRAM = r"""
#include "residual_pack_map.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace gfship;
#define ROWS 64
#define W (ROWS + 8)
#define CHECK(x) do { if (!(x)) { printf ("line %d: %s\n", __LINE__, #x); return 1; } } while (0)
int main (int argc, char ** argv)
{
  const int n = atoi (argv[1]), ntj = n/16, ntiles = ntj*ntj, nrb = (n + 15 + ROWS - 1)/ROWS;
  const int ntasks = residual_restrict_ntasks (nrb, ntiles);
  std::vector<int> owned ((size_t) n*n*n, 0), coarse ((size_t) n*n*n/8, 0), task (ntiles*8*nrb, 0);
  for (int t = 0; t < ntasks; t++) {
    const ResidualRestrictTask T = residual_restrict_task (t, nrb);
    if (T.tile >= ntiles) continue;
    CHECK (T.tile >= 0 && T.PB >= 0 && T.PB < 8 && T.rb >= 0 && T.rb < nrb);
    task[(T.tile*8 + T.PB)*nrb + T.rb]++;
    const int P = T.tile % ntj, Q = T.tile / ntj, r0 = T.rb*ROWS, PB = T.PB;
    const int I0 = residual_restrict_origin (r0, PB);
    bool buf[32][W] = {};
    for (int e = 0; e < 32*(ROWS/2 + 1); e++) {
      const ResidualRestrictPair p = residual_restrict_pair<ROWS> (e, r0, PB);
      if (!residual_restrict_pair_needed<ROWS> (p, n)) continue;
      const int j = n - (16*P + p.a), k = n - (16*Q + 2*PB + p.db);
      CHECK (p.line >= 0 && p.line < 32 && j >= 1 && j <= n && k >= 1 && k <= n);
      CHECK (p.I % 2 == 0 && p.I + 1 < n && p.I - I0 >= 0 && p.I - I0 + 1 < W);
      buf[p.line][p.I - I0] = buf[p.line][p.I - I0 + 1] = true;
      for (int q = 0; q < 2; q++)
	if (residual_restrict_owns<ROWS> (p, q))
	  owned[(size_t) (p.I + q) + (size_t) n*((j - 1) + (size_t) n*(k - 1))]++;
    }
    // the copy into the skewed layout, as patch_restrict_pack_kernel walks the rows
    for (int e = 0; e < ROWS*32; e++) {
      const int row = e / 32, col = e % 32, PA = col >> 2, p = col & 3;
      const int a = 2*PA + (p & 1), db = p >> 1, I = r0 + row - PA - PB;
      if (I >= 0 && I < n) CHECK (buf[a + 16*db][I - I0]);
    }
    for (int e = 0; e < 8*(ROWS/2); e++) {
      const ResidualRestrictCoarse c = residual_restrict_coarse<ROWS> (e, r0, PB);
      if (c.I < 0 || c.I >= n) continue;
      CHECK (c.I % 2 == 0 && c.PA >= 0 && c.PA < 8);
      for (int id = 0; id < 8; id++)
	CHECK (buf[2*c.PA + ((id >> 1) & 1) + 16*(id >> 2)][c.I - I0 + (id & 1)]);
      const int m = c.I >> 1, pj = (n - 16*P - 2*c.PA) >> 1, pk = (n - 16*Q - 2*PB) >> 1;
      CHECK (pj >= 1 && pj <= n/2 && pk >= 1 && pk <= n/2);
      coarse[(size_t) m + (size_t) (n/2)*((pj - 1) + (size_t) (n/2)*(pk - 1))]++;
    }
  }
  for (int c : task) CHECK (c == 1);
  for (int c : owned) CHECK (c == 1);
  for (int c : coarse) CHECK (c == 1);
  printf ("ok %d tasks\n", ntasks);
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("residual_pack_map")
    src, exe = str(tmp / "map.cpp"), str(tmp / "map")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Werror", "-D__host__=",
                    "-D__device__=", "-I", CSRC, src, "-o", exe], check=True, capture_output=True, text=True,
                   timeout=120)
    return exe


@pytest.mark.parametrize("n,ntasks", [(64, 256), (128, 1536)])
def test_every_cell_and_every_coarse_cell_has_one_owner(program, n, ntasks):
    r = subprocess.run([program, str(n)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok %d tasks" % ntasks
