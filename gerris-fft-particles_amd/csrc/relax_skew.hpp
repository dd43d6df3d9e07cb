// relax_skew.hpp -- definitions shared by the pipelined exact-order sweep kernels
#pragma once
#include "gfship_internal.hpp"

namespace gfship {

#define SK_T   16            /* tile edge (lines) */
#define SK_NL  (SK_T*SK_T)   /* lines = threads per tile */
#define SK_PAD (2*SK_T - 2)  /* extra rows of a tile: max skew */
#ifndef SK_D
#define SK_D   6             /* prefetch distance (steps) of the own streams: 16 was 12 % slower at */
                             /* 256^3 (round 2, tools/lab/knobs.sh: 4, 6, 8, 12, 16 tried): what is */
                             /* in flight in a CU is what a hand-off poll of that CU queues behind  */
#endif
#ifndef SK_DH
#define SK_DH  3             /* prefetch distance of the halo streams (divides SK_D): the lag */
                             /* between neighbouring tiles grows with it                     */
#endif
/* rows of padding in front of and behind every tile, so that prefetch addresses never need
   clamping: 15 rows in front (first lines of the next tile are read at row t - 15), 2*SK_D behind
   (rows up to T + SK_D, T rounded up to SK_D) */
#define SK_FP  48
/* rows of a tile's hand-off / snapshot granule array: n + 30 used, the streams read ahead by up
   to SK_D (rounding of T) + SK_DH + 1 rows */
#define SK_HROWS(n_) ((n_) + 2*SK_T + 36)   /* 36 = 16 + 4 + 16: the largest read-ahead of any of the kernels */

typedef unsigned long long u64;
#define SK_SENTINEL 0xFFFFFFFFFFFFFFFFull

struct SkewArgs {
  Layout L;
  int ntj;                 // tiles per side
  int RT;                  // rows per tile
  double * us;             // skewed u
  const double * rs;       // skewed rhs
  const double * ds;       // skewed dia (or nullptr)
  double * un;             // natural u (ghost layer + mirrored side cells)
  u64 * hbJ;               // [tile][n + SK_T - 1][SK_T] new values of line a = 15
  u64 * hbK;               // [tile][n + SK_T - 1][SK_T] new values of line b = 15
  const unsigned short * order; // ticket -> tile (anti-diagonal major)
  unsigned * ticket;       // ticket counter (zeroed before the launch)
  unsigned * err;          // set to 1 when a bounded spin gives up
  const u64 * dummy;       // 8 readable bytes for the streams a lane does not need
  u64 * stats;             // optional per-tile { start, end, spins, slow entries } (debug)
};

#define SK_MAXF 8    /* sweeps per launch */
#ifndef SK_POLL_SLEEP
#define SK_POLL_SLEEP 0   /* s_sleep argument between two polls of a hand-off granule */
#endif
#ifndef SK_EXP
#define SK_EXP 0    /* timing experiments: 1 plain halo prefetch loads, 2 plain granule stores */
#endif
#define SK_HLOAD(p_) ((SK_EXP & 1) ? *(p_) : load_sc1 (p_))
#ifndef SK_KO
#define SK_KO 0      /* timing experiments only: knock out parts of the step (wrong results) */
#endif


struct SkewLoopArgs {
  Layout L;
  int ntj, RT, nsweeps;
  // homogeneous BC of the sides d = 0..5 (right, left, top, bottom, front, back) between the sweeps
  // of a fused loop: sgn[d] = 0 periodic; otherwise ghost = sgn[d] * adjacent interior value (-1
  // Dirichlet and the normal component at a symmetry side, +1 Neumann and symmetry otherwise)
  double sgn[6];
  int mirror;              // single sweep with the BC kernel around it: cells next to the box sides
                           // are also written to the natural array (any kind of side)
  double * us;             // skewed u (in place)
  const double * rs;       // skewed rhs
  const double * ds;       // skewed dia (or nullptr)
  double * un;             // natural u: ghosts of sweep 0 are read, ghosts of the last BC written
  u64 * hb;                // per sweep: [J hand-off | K hand-off | J snapshot | K snapshot]
  long hb_sweep;           // granules per sweep
  long hb_words;           // granules of one hand-off array (ntiles*hstride)
  const unsigned short * order;
  unsigned * ticket, * err;
  const u64 * dummy;
  u64 * stats;             // optional [tile][sweep]{start, end} (debug, GFSHIP_SKEW_STATS)
  // XCD-aware placement (all tiles resident): the tiles are split into 8 blocks, one per XCD, and
  // a workgroup claims a tile of the block of the XCD it runs on (any other block once its own is
  // exhausted): most hand-offs then stay inside one L2
  const unsigned short * xorder;   // [8][per_xcd] tiles of each block, anti-diagonal order
  unsigned * xticket;              // [8] ticket counters (zeroed before the launch)
  int per_xcd;                     // 0: placement by the single ticket counter
  // arming of the other granule set (relax_patch_loop.hip): arm_pairs 16-byte pairs from `arm',
  // shared between the tiles by arm_cum[tile] .. arm_cum[tile + 1] of arm_cum[ntiles]
  u64 * arm;
  unsigned long long arm_pairs;
  const unsigned * arm_cum;
  // XCD of the workgroup that claimed each tile (armed all ones with the granules; relax_patch_loop.hip)
  unsigned * tile_xcd;
  int fault_tile;          // test of the error path (GFSHIP_FAULT_DROP_HANDOFF=tile): that tile publishes nothing in sweep 0
  int near_mode;           // stores towards a consumer on the same XCD: 0 agent scope like the others, 1 plain, 2 workgroup scope
  // cell update: the RelaxOp kind (cell_update.hpp); dia is rhoc for kinds 1 and 3, ws[d] are skewed copies
  // of the face weights of kinds 2 and 3, streamed beside u / rhs / dia
  int op;
  double w, h2;
  const double * ws[6];
};

typedef __attribute__((address_space(1))) u64 gu64;

__device__ __forceinline__ u64 load_sc1 (const u64 * p)
{
  return __hip_atomic_load ((gu64 *) p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void store_sc1 (u64 * p, u64 v)
{
  __hip_atomic_store ((gu64 *) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// get_from_above of fine cell (i, j, k): prolongate_kernel's expression (poisson_kernels.hip)
__device__ __forceinline__ double patch_prolong (const Layout & Lc, const double * __restrict__ vc,
						 int i, int j, int k)
{
  const int pi = (i + 1)/2, pj = (j + 1)/2, pk = (k + 1)/2;
  const long p = Lc.idx (pi, pj, pk);
  const double pv = vc[p];
  double h[3];
  const long off[3] = { 1, Lc.sy, Lc.sz };
#pragma unroll
  for (int cc = 0; cc < 3; cc++) {
    double g1 = vc[p + off[cc]] - 1.*pv;
    double g2 = vc[p - off[cc]] - 1.*pv;
    h[cc] = (g1 - g2)/2.;
  }
  const double rel[3] = { ((i & 1) ? -1. : 1.)/4., ((j & 1) ? -1. : 1.)/4., ((k & 1) ? -1. : 1.)/4. };
  double val = pv;
#pragma unroll
  for (int cc = 0; cc < 3; cc++)
    val += rel[cc]*h[cc];
  return val;
}

// The y and z ghost planes of the natural array that the last BC application of a fused loop left = periodic
// images (or, at a non-periodic side, +- the adjacent line) of the side cells after sweep nsweeps - 2, taken
// from that sweep's granules; what of SkewLoopArgs that takes.  On the levels of the one-line kernels:
//   hand-off J of tile (ntj-1,Q): line a = 15 (j = 1)  -> ghost j = n + 1     row I + b
//   snapshot J of tile (0,Q):     line a = 0  (j = n)  -> ghost j = 0         row I + b + 15
//   hand-off K of tile (P,ntj-1): line b = 15 (k = 1)  -> ghost k = n + 1     row I + a
//   snapshot K of tile (P,0):     line b = 0  (k = n)  -> ghost k = 0         row I + a + 15
// on those of the 2 x 2 kernels (patch) the rows are I + (l >> 1) and I + (l >> 1) + 7.
struct LoopGhosts {
  Layout L;
  int ntj = 0, nsweeps = 0;
  double sgn[6] = {};
  const u64 * hb = nullptr;
  long hb_sweep = 0, hb_words = 0;
  double * un = nullptr;
  bool patch = false;
  bool active = false;     // host side: the loop has left them to the copy out of its layout (skew_unpack)
};

inline __host__ __device__ LoopGhosts loop_ghosts_of (const SkewLoopArgs & A, bool patch)
{
  LoopGhosts G;
  G.L = A.L; G.ntj = A.ntj; G.nsweeps = A.nsweeps;
  for (int d = 0; d < 6; d++) G.sgn[d] = A.sgn[d];
  G.hb = A.hb; G.hb_sweep = A.hb_sweep; G.hb_words = A.hb_words;
  G.un = A.un;
  G.patch = patch;
  G.active = true;
  return G;
}

// ghost cell of plane 0 .. 3 (j = n + 1, j = 0, k = n + 1, k = 0) at x index I + 1, tangential index c (0 .. n-1)
__device__ __forceinline__ void loop_ghost_cell (const LoopGhosts & A, int I, int c, int plane)
{
  const int n = A.L.n, ntj = A.ntj;
  const long hstride = (long) SK_HROWS (n)*SK_T;
  const int sw = A.nsweeps - 2;
  const u64 * hbJ = A.hb + sw*A.hb_sweep, * hbK = hbJ + A.hb_words;
  const u64 * snJ = hbK + A.hb_words, * snK = snJ + A.hb_words;
  const int T_ = c / SK_T, l = c % SK_T;                  // tile and line of the tangential index
  const int lr = A.patch ? l >> 1 : l, back = A.patch ? 7 : SK_T - 1;
  // periodic: the line next to the opposite side; otherwise sgn * the line next to the same side
  const long lastJ = (long) ((ntj - 1) + ntj*T_)*hstride, firstJ = (long) (0 + ntj*T_)*hstride;
  const long lastK = (long) (T_ + ntj*(ntj - 1))*hstride, firstK = (long) (T_ + ntj*0)*hstride;
  const long rowHb = (long) (I + lr)*SK_T + l, rowSn = (long) (I + lr + back)*SK_T + l;
  u64 bits;
  long dst;
  double sg;
  switch (plane) {
  case 0: sg = A.sgn[2]; bits = sg == 0. ? hbJ[lastJ + rowHb] : snJ[firstJ + rowSn];     // ghost j = n + 1
    dst = A.L.idx (I + 1, n + 1, n - c); break;
  case 1: sg = A.sgn[3]; bits = sg == 0. ? snJ[firstJ + rowSn] : hbJ[lastJ + rowHb];     // ghost j = 0
    dst = A.L.idx (I + 1, 0, n - c); break;
  case 2: sg = A.sgn[4]; bits = sg == 0. ? hbK[lastK + rowHb] : snK[firstK + rowSn];     // ghost k = n + 1
    dst = A.L.idx (I + 1, n - c, n + 1); break;
  default: sg = A.sgn[5]; bits = sg == 0. ? snK[firstK + rowSn] : hbK[lastK + rowHb];    // ghost k = 0
    dst = A.L.idx (I + 1, n - c, 0);
  }
  const double v = __longlong_as_double ((long long) bits);
  A.un[dst] = sg == 0. ? v : sg*v;
}

// The same from the grid of the copy out of the layout, whose cells are the interior ones: the blocks behind
// its `first_z' planes of blocks take the 4 n^2 ghost cells, one per thread (256 threads per block)
__device__ __forceinline__ void loop_ghost_blocks (const LoopGhosts & A, int first_z)
{
  const long g = blockIdx.x + (long) gridDim.x*(blockIdx.y + (long) gridDim.y*(blockIdx.z - first_z));
  const long t = g*blockDim.x + threadIdx.x;
  const int n = A.L.n;
  if (t >= 4l*n*n) return;
  loop_ghost_cell (A, (int) (t % n), (int) ((t / n) % n), (int) (t / ((long) n*n)));
}

// planes of blocks that takes in a grid of gx x gy blocks of 256 threads
inline int loop_ghost_planes (const LoopGhosts & A, int gx, int gy)
{
  const long cells = 4l*A.L.n*A.L.n, per_plane = 256l*gx*gy;
  return A.active ? (int) ((cells + per_plane - 1)/per_plane) : 0;
}

// ghosts != nullptr: the ghost planes of a loop of nrelax >= 2 sweeps are left to the caller (*ghosts)
int patch_loop_launch (gfship_domain * dom, const SkewLoopArgs & A, int ntiles, bool has_dia,
		       unsigned nrelax, float * ms, LoopGhosts * ghosts = nullptr);

} // namespace gfship
