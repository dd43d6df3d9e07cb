// residual_pack_map.hpp -- who computes what in residual_restrict_pack_kernel (relax_patch_loop.hip): the tasks
// of a level, the pairs of cells a task computes, the cells and the coarse cells it owns.
//
// A level of n^3 cells is (n/16)^2 tiles of 16 x 16 lines; line (a, b) of tile (P, Q) is j = n - (16 P + a),
// k = n - (16 Q + b), and its cell I (x index I + 1) sits in the skewed row rho = I + (a >> 1) + (b >> 1) of the
// tile (the layout of the 2 x 2 kernels).  A task is (tile, PB, block rb of ROWS skewed rows): the 16 x 2 lines
// with b >> 1 == PB, and of each of them the cells whose row is in r0 .. r0 + ROWS - 1, r0 = rb*ROWS, that is
// I = lo .. lo + ROWS - 1 with lo = r0 - (a >> 1) - PB.  Those cells the task owns: each cell of the level
// belongs to one row of one tile, hence to one task.  The task also restricts: it owns the coarse cells whose
// first child along x (I even) it owns, and so needs the cell lo + ROWS where lo + ROWS - 1 is even.  The cells
// are computed as aligned pairs (I, I + 1), I even: ROWS/2 pairs of a line where lo is even, ROWS/2 + 1 where
// it is odd (the first cell of the first pair is then not needed, and computed all the same).
//
// Plain C++: a host compiler reads it with __host__ and __device__ defined away
// (tests/test_residual_pack_map_cpu.py).
#pragma once

namespace gfship {

struct ResidualRestrictTask { int tile, PB, rb; };

// tasks of a level of ntiles tiles and nrb blocks of rows, those of residual_restrict_task that name no tile included
__host__ __device__ inline int residual_restrict_ntasks (int nrb, int ntiles)
{
  return 64*((nrb*ntiles + 7)/8);
}

// the tasks in the order the workgroups take them: the eight PB of a (tile, block of rows) are eight workgroups
// apart, so that they run at the same time on one XCD (the workgroups are dealt round-robin over the 8 XCDs),
// whose L2 then serves the k-planes of u that neighbouring PB share.  tile >= ntiles: nothing to do
__host__ __device__ inline ResidualRestrictTask residual_restrict_task (int t, int nrb)
{
  ResidualRestrictTask T;
  const int idx = (t & 7) + 8*(t >> 6);
  T.PB = (t >> 3) & 7;
  T.rb = idx % nrb;
  T.tile = idx / nrb;
  return T;
}

// item e = 0 .. 32*(ROWS/2 + 1) - 1 of a task: the pair (I, I + 1) of line (a, 2 PB + db)
struct ResidualRestrictPair { int line, a, db, lo, I; };

template <int ROWS>
__host__ __device__ inline ResidualRestrictPair residual_restrict_pair (int e, int r0, int PB)
{
  ResidualRestrictPair p;
  const int pi = e % (ROWS/2 + 1);
  p.line = e / (ROWS/2 + 1);
  p.a = p.line & 15; p.db = p.line >> 4;
  p.lo = r0 - (p.a >> 1) - PB;
  p.I = (p.lo & ~1) + 2*pi;
  return p;
}

// the pair is in the box and the task needs it
template <int ROWS>
__host__ __device__ inline bool residual_restrict_pair_needed (const ResidualRestrictPair & p, int n)
{
  return p.I >= 0 && p.I < n && p.I < p.lo + ROWS;
}

// the task owns cell I + q of the pair, q = 0, 1
template <int ROWS>
__host__ __device__ inline bool residual_restrict_owns (const ResidualRestrictPair & p, int q)
{
  return p.I + q >= p.lo && p.I + q < p.lo + ROWS;
}

// the even cell at or below the first cell of any line of the task: the origin of its buffer, whose lines hold
// ROWS + 8 cells
__host__ __device__ inline int residual_restrict_origin (int r0, int PB)
{
  return (r0 - 7 - PB) & ~1;
}

// item e = 0 .. 8*(ROWS/2) - 1 of a task: the coarse cell of the lines 2 PA, 2 PA + 1 (both db) whose first
// child along x is cell I of the task's rows (in the box where 0 <= I < n): 32 consecutive items are 32
// consecutive coarse cells of one coarse line
struct ResidualRestrictCoarse { int PA, I; };

template <int ROWS>
__host__ __device__ inline ResidualRestrictCoarse residual_restrict_coarse (int e, int r0, int PB)
{
  ResidualRestrictCoarse c;
  c.PA = e / (ROWS/2);
  const int mi = e % (ROWS/2);
  const int par = (c.PA + PB + r0) & 1;            /* rows of the block whose I = r0 + row - PA - PB is even */
  c.I = r0 + 2*mi + par - c.PA - PB;
  return c;
}

} // namespace gfship
