// droplets.hip -- connected regions of a field on a uniform box: gfs_domain_tag_droplets (src/domain.c:3564-3796),
// gfs_domain_remove_droplets (:3798-3880) and GfsDropletToParticle (modules/particulatecommon.c:1163-1527).
//
// The reference tags by a flood fill in traversal order, one region after the other, then joins the regions that
// meet through a periodic side (the `touch' table) and renumbers.  The result (proved on a
// literal restatement by tests/test_droplets_reference_cpu.py): the tag of a region is 1 + its rank, among the
// regions under face connectivity with periodic sides, by the smallest traversal index of its cells.  Here:
//   1. labels.  A label is the traversal index of a cell (32 bits): the key of morton_key, poisson_kernels.hip, bit
//      0 of every level from I = i - 1, bit 1 from J = n - j, bit 2 from K = n - k, so that a run of 2^(dim*b)
//      indices is an aligned cube of side 2^b.  All the work arrays are indexed by the traversal index.  A union-
//      find in which the smaller index wins, so that the root of a region IS its smallest traversal index:
//      a. drop_tile_kernel: one workgroup per tile (16 x 16 cells in 2-D, 8 x 8 x 8 in 3-D, or the whole box where
//         it is smaller) resolves the labels of its tile in LDS with atomicMin and stores root labels;
//      b. drop_border_kernel: one thread per cell of the low face of every tile, and of the box where the side is
//         periodic, merges with the cell across the face by atomicMin on the parent array;
//      c. drop_flatten_kernel: every cell takes its root; a root raises its flag.
//      Integer atomicMin only: the roots do not depend on the order.  No kernel waits for another workgroup, and
//      nothing is relaunched until convergence: three launches.
//   2. tags.  An exclusive scan (hipCUB) of the flags gives the rank of every root, tag = 1 + rank[root], and n =
//      the total: the first of the two words an event reads back.
//   3. sizes by integer atomicAdd, the last leaf of a droplet in traversal order by integer atomicMax; the boundary
//      flag of compute_droplet_properties (:1194-1229) is that of the last leaf.
//   4. min < 0: a descending radix sort of the sizes, and the second word read back.
//   5. the fp64 sums of the droplets that convert, in traversal order: the counted leaves of those droplets write
//      keys (droplet << 32 | traversal index) into the segment of their droplet (offsets: a scan of the sizes),
//      a radix sort orders them, and one thread per droplet adds its segment in order.  No floating-point atomic.
//   6. the droplets are the candidates of launch_feed_ids (feed_particle.hip), in tag order: n slots after those
//      in use, cell = PSOURCE_NO_CELL for a droplet that does not convert.
//   7. the reset of the variable on the leaves, then its ghosts by its boundary conditions.
#include "particle_events.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace gfship {

constexpr unsigned DROP_NONE = 0xFFFFFFFFu;
constexpr int DROP_BLOCK = 256;
constexpr double DROP_THRESHOLD = 1e-4;        /* src/domain.c:3564 */
constexpr int DROP_TILE_BITS_2D = 4, DROP_TILE_BITS_3D = 3;

struct DropGeom {
  Layout L;
  int depth, n, tb;      // levels, cells per side, log2 of the side of a tile
  unsigned N;            // cells
  int per[3];            // both sides of the direction are periodic
};

// the work arrays of the labelling, kept by the domain between calls
struct DropWork {
  unsigned * parent = nullptr, * rank = nullptr, * tagi = nullptr;      // per cell, by traversal index
  size_t ncap = 0;
  // per droplet
  unsigned * sizes = nullptr, * last = nullptr, * segsize = nullptr, * seg = nullptr, * cursor = nullptr,
    * sorted = nullptr, * cell = nullptr, * block = nullptr;
  size_t dcap = 0;
  unsigned long long * key = nullptr, * key2 = nullptr;                 // per counted leaf of a droplet that converts
  size_t kcap = 0;
  void * tmp = nullptr;                                                 // of hipCUB
  size_t tmp_bytes = 0;
  unsigned * counters = nullptr;     // n, the size that min < 0 selects, particles made, cells reset
};

template <int DIM>
__host__ __device__ __forceinline__ unsigned drop_encode (int bits, int I, int J, int K)
{
  unsigned t = 0;
  for (int b = 0; b < bits; b++) {
    t |= (unsigned) ((I >> b) & 1) << (DIM*b);
    t |= (unsigned) ((J >> b) & 1) << (DIM*b + 1);
    if (DIM == 3) t |= (unsigned) ((K >> b) & 1) << (DIM*b + 2);
  }
  return t;
}

template <int DIM>
__host__ __device__ __forceinline__ void drop_decode (int bits, unsigned t, int x[3])
{
  x[0] = x[1] = x[2] = 0;
  for (int b = 0; b < bits; b++) {
    x[0] |= (int) ((t >> (DIM*b)) & 1u) << b;
    x[1] |= (int) ((t >> (DIM*b + 1)) & 1u) << b;
    if (DIM == 3) x[2] |= (int) ((t >> (DIM*b + 2)) & 1u) << b;
  }
}

// the place in a field of the cell with oriented coordinates x
template <int DIM>
__device__ __forceinline__ long drop_index (const DropGeom & G, const int x[3])
{
  return G.L.idx (x[0] + 1, G.n - x[1], DIM == 3 ? G.n - x[2] : 0);
}

// a face neighbour of the cell is a boundary cell: every side of the box is a boundary, a periodic one included
// (a GfsBoundaryPeriodic cell carries GFS_FLAG_BOUNDARY, src/boundary.c:576-582)
template <int DIM>
__device__ __forceinline__ bool drop_on_side (const DropGeom & G, const int x[3])
{
  bool side = false;
#pragma unroll
  for (int a = 0; a < DIM; a++)
    side = side || x[a] == 0 || x[a] == G.n - 1;
  return side;
}

// the root of x in p (LDS or global): parents only decrease, and a parent read late is still an ancestor.  The loads
// are relaxed agent-scope atomic loads through a generic pointer (flat atomics, on LDS too): they bypass the L1 of
// the CU on the global array, and the compiler may not keep a parent in a register while other threads lower it
__device__ __forceinline__ unsigned drop_find (unsigned * p, unsigned x)
{
  unsigned q;
  while ((q = __hip_atomic_load (&p[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x)
    x = q;
  return x;
}

// join the regions of a and b: the larger root takes the smaller as its parent.  Lock-free: a thread whose
// atomicMin finds the root already moved goes on with where it moved to
__device__ __forceinline__ void drop_union (unsigned * p, unsigned a, unsigned b)
{
  for (;;) {
    a = drop_find (p, a);
    b = drop_find (p, b);
    if (a == b) return;
    if (a < b) { const unsigned s = a; a = b; b = s; }
    const unsigned old = atomicMin (&p[a], b);
    if (old == a) return;
    a = old;
  }
}

// 1a. the labels of one tile, in LDS.  c: the variable (a field), or fv: the values of the function by traversal index
template <int DIM>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_tile_kernel (DropGeom G, const double * __restrict__ c, const double * __restrict__ fv,
		  unsigned * __restrict__ parent)
{
  constexpr int MAXTC = DIM == 3 ? 1 << (3*DROP_TILE_BITS_3D) : 1 << (2*DROP_TILE_BITS_2D);
  __shared__ unsigned lab[MAXTC];
  const int TC = 1 << (DIM*G.tb);
  const unsigned base = blockIdx.x*(unsigned) TC;
  for (int l = threadIdx.x; l < TC; l += DROP_BLOCK) {
    const unsigned t = base + (unsigned) l;
    double v;
    if (fv) v = fv[t];
    else {
      int x[3];
      drop_decode<DIM> (G.depth, t, x);
      v = c[drop_index<DIM> (G, x)];
    }
    lab[l] = v > DROP_THRESHOLD ? (unsigned) l : DROP_NONE;
  }
  __syncthreads ();
  /* a cell outside the mask stays DROP_NONE, a cell inside never becomes it: these reads need no care */
  for (int l = threadIdx.x; l < TC; l += DROP_BLOCK)
    if (lab[l] != DROP_NONE) {
      int x[3];
      drop_decode<DIM> (G.tb, (unsigned) l, x);
#pragma unroll
      for (int a = 0; a < DIM; a++)
	if (x[a] > 0) {
	  int y[3] = { x[0], x[1], x[2] };
	  y[a]--;
	  const unsigned m = drop_encode<DIM> (G.tb, y[0], y[1], y[2]);
	  if (m < (unsigned) TC && lab[m] != DROP_NONE)
	    drop_union (lab, (unsigned) l, m);
	}
    }
  __syncthreads ();
  for (int l = threadIdx.x; l < TC; l += DROP_BLOCK)
    if (lab[l] == DROP_NONE) parent[base + (unsigned) l] = DROP_NONE;
    else {      /* nothing writes lab after the barrier: plain loads */
      unsigned x = (unsigned) l;
      while (lab[x] != x) x = lab[x];
      parent[base + (unsigned) l] = base + x;
    }
}

// 1b. one thread per cell of the low face of a tile in each direction: join with the cell across the face, through
// the side of the box where the direction is periodic
template <int DIM>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_border_kernel (DropGeom G, unsigned long long count, unsigned * __restrict__ parent)
{
  const unsigned long long q = (unsigned long long) blockIdx.x*DROP_BLOCK + threadIdx.x;
  if (q >= count) return;
  const unsigned n = (unsigned) G.n, ns = n >> G.tb;
  const unsigned long long plane = DIM == 3 ? (unsigned long long) n*n : n, slab = ns*plane;
  const int a = (int) (q/slab);
  const unsigned long long r = q % slab;
  const int X = (int) (r/plane) << G.tb;
  const unsigned w = (unsigned) (r % plane);
  int Xn = X - 1;
  if (X == 0) {
    if (!G.per[a]) return;
    Xn = G.n - 1;
  }
  const int u = (int) (w % n), v = (int) (w/n);
  int x[3], y[3];
  x[a] = X; y[a] = Xn;
  x[(a + 1) % DIM] = y[(a + 1) % DIM] = u;
  if (DIM == 3) x[(a + 2) % DIM] = y[(a + 2) % DIM] = v;
  else x[2] = y[2] = 0;
  const unsigned t1 = drop_encode<DIM> (G.depth, x[0], x[1], x[2]), t2 = drop_encode<DIM> (G.depth, y[0], y[1], y[2]);
  if (t1 >= G.N || t2 >= G.N) return;
  if (parent[t1] == DROP_NONE || parent[t2] == DROP_NONE) return;
  drop_union (parent, t1, t2);
}

// 1c. every cell takes its root; flag = the cell is a root
__global__ void __launch_bounds__(DROP_BLOCK)
drop_flatten_kernel (unsigned N, unsigned * __restrict__ parent, unsigned * __restrict__ flag)
{
  const unsigned t = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (t >= N) return;
  unsigned p = parent[t];
  if (p != DROP_NONE) {
    p = drop_find (parent, t);
    /* a root keeps itself; any other cell moves to an ancestor: the finds of others stay right */
    __hip_atomic_store (&parent[t], p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  flag[t] = p == t ? 1u : 0u;
}

__global__ void drop_count_kernel (unsigned N, const unsigned * __restrict__ rank, const unsigned * __restrict__ flag,
				   unsigned * __restrict__ counters)
{
  counters[0] = rank[N - 1] + flag[N - 1];
  counters[1] = counters[2] = counters[3] = 0u;
}

// 2 and 3. tag = 1 + the rank of the root (0 outside), into tagi and, as a double, into the field tagf; the size of
// every droplet -- all its leaves (compute_droplet_size, src/domain.c:3805-3810), or those that touch no side
// (compute_droplet_properties) -- and its last leaf
template <int DIM>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_tag_kernel (DropGeom G, const unsigned * __restrict__ parent, const unsigned * __restrict__ rank,
		 unsigned * __restrict__ tagi, double * __restrict__ tagf, unsigned * __restrict__ sizes,
		 unsigned * __restrict__ last, int all)
{
  const unsigned t = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  const bool valid = t < G.N;
  unsigned tag = 0u;
  bool counted = false;
  if (valid) {
    const unsigned p = parent[t];
    tag = p == DROP_NONE ? 0u : 1u + rank[p];
    tagi[t] = tag;
    int x[3];
    drop_decode<DIM> (G.depth, t, x);
    if (tagf) tagf[drop_index<DIM> (G, x)] = (double) tag;
    counted = tag && (all || !drop_on_side<DIM> (G, x));
  }
  if (!sizes) return;
  /* the lanes of a wave that share a tag add once (a wave is 64 consecutive traversal indices: mostly one droplet),
     so that a large droplet is not one atomic per cell on one address; the sums are integers: any grouping gives
     the same result */
  const int lane = threadIdx.x & 63;
  bool pending = tag != 0u;
  unsigned long long todo = __ballot (pending);
  while (todo) {
    const int lead = __ffsll ((long long) todo) - 1;
    const unsigned ltag = (unsigned) __shfl ((int) tag, lead, 64);
    const bool mine = pending && tag == ltag;
    const unsigned long long m = __ballot (mine), mc = __ballot (mine && counted);
    if (lane == lead) {
      if (mc) atomicAdd (&sizes[ltag - 1], (unsigned) __popcll (mc));
      atomicMax (&last[ltag - 1], t - (unsigned) lane + (unsigned) (63 - __clzll ((long long) m)));
    }
    pending = pending && !mine;
    todo &= ~m;
  }
}

// convert_droplets, :1323-1325: which droplets convert, and the length of their segment of keys
template <int DIM>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_candidate_kernel (DropGeom G, unsigned n, unsigned min, const unsigned * __restrict__ sizes,
		       const unsigned * __restrict__ last, unsigned * __restrict__ segsize,
		       unsigned * __restrict__ cursor)
{
  const unsigned i = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (i >= n) return;
  int x[3];
  drop_decode<DIM> (G.depth, last[i], x);
  const unsigned s = sizes[i];
  segsize[i] = !drop_on_side<DIM> (G, x) && s < min && s > 1u ? s : 0u;
  cursor[i] = 0u;
}

// 5. the keys of the counted leaves of the droplets that convert, anywhere in the segment of their droplet: the sort
// puts them in traversal order
template <int DIM>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_keys_kernel (DropGeom G, const unsigned * __restrict__ tagi, const unsigned * __restrict__ segsize,
		  const unsigned * __restrict__ seg, unsigned * __restrict__ cursor, unsigned long long cap,
		  unsigned long long * __restrict__ key)
{
  const unsigned t = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (t >= G.N) return;
  const unsigned tag = tagi[t];
  if (!tag || !segsize[tag - 1]) return;
  int x[3];
  drop_decode<DIM> (G.depth, t, x);
  if (drop_on_side<DIM> (G, x)) return;
  const unsigned long long slot = (unsigned long long) seg[tag - 1] + atomicAdd (&cursor[tag - 1], 1u);
  if (slot < cap) key[slot] = (unsigned long long) (tag - 1) << 32 | t;
}

struct DropConvertArgs {
  DropGeom G;
  unsigned n;
  int base;
  const unsigned * sizes, * segsize, * seg;
  const unsigned long long * key;
  const double * c, * u[3], * alpha;
  double * pos[3], * old[3], * vel[3], * force[3], * mass, * volume;
  unsigned * orig, * cell;
};

// 5 and 6. compute_droplet_properties (:1214-1228) over the leaves of a droplet in traversal order, then
// convert_droplets (:1326-1338) up to add_particulate: one droplet per thread, one slot of the list per droplet
template <int DIM>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_convert_kernel (DropConvertArgs A)
{
  const unsigned i = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (i >= A.n) return;
  const int s = A.base + (int) i;
  double pos[3] = { 0., 0., 0. }, vel[3] = { 0., 0., 0. }, volume = 0., mass = 0.;
  unsigned cell = PSOURCE_NO_CELL;
  const unsigned size = A.segsize[i];
  if (size) {
    const double h = 1./(double) A.G.n, vol = DIM == 3 ? h*h*h : h*h;      /* pow (h, FTT_DIMENSION): powers of two */
    const unsigned long long * key = A.key + A.seg[i];
    for (unsigned q = 0; q < size; q++) {
      int x[3];
      drop_decode<DIM> (A.G.depth, (unsigned) key[q], x);
      const long idx = drop_index<DIM> (A.G, x);
      const int ix[3] = { x[0], A.G.n - 1 - x[1], A.G.n - 1 - x[2] };
      volume += vol*A.c[idx];
#pragma unroll
      for (int a = 0; a < DIM; a++) {
	pos[a] += -0.5 + (ix[a] + 0.5)*h;      /* ftt_cell_pos: dyadic, exact */
	vel[a] += A.u[a][idx];
      }
    }
#pragma unroll
    for (int a = 0; a < DIM; a++) {
      pos[a] = pos[a]/(double) A.sizes[i];
      vel[a] = vel[a]/(double) A.sizes[i];
    }
    int c[3];
    if (locate<DIM> (A.G.depth, pos, c)) {
      const unsigned n = (unsigned) A.G.n;
      cell = (unsigned) (c[0] - 1) + n*((unsigned) (c[1] - 1) + (DIM == 3 ? n*(unsigned) (c[2] - 1) : 0u));
      mass = A.alpha ? 1./A.alpha[A.G.L.idx (c[0], c[1], c[2])] : 1.;
      mass *= volume;
    }
    else
      volume = 0.;
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
    A.pos[a][s] = pos[a];
    A.old[a][s] = 0.;
    A.force[a][s] = 0.;
    A.vel[a][s] = vel[a];
  }
  A.orig[s] = (unsigned) s;
  A.mass[s] = mass;
  A.volume[s] = volume;
  A.cell[i] = cell;
}

// the particles the ordered passes of feed_particle.hip made of the n slots
__global__ void __launch_bounds__(DROP_BLOCK)
drop_made_kernel (unsigned n, const unsigned char * __restrict__ alive, unsigned * __restrict__ counters)
{
  const unsigned i = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (i < n && alive[i]) atomicAdd (&counters[2], 1u);
}

// 7. reset_small_fraction (:1187-1192, src/domain.c:3812-3817): v = val on the leaves of every droplet smaller than min
template <int DIM>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_reset_kernel (DropGeom G, const unsigned * __restrict__ tagi, const unsigned * __restrict__ sizes,
		   unsigned min, double val, double * __restrict__ v, unsigned * __restrict__ counters)
{
  const unsigned t = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (t >= G.N) return;
  const unsigned tag = tagi[t];
  if (!tag || !(sizes[tag - 1] < min)) return;
  int x[3];
  drop_decode<DIM> (G.depth, t, x);
  v[drop_index<DIM> (G, x)] = val;
  atomicAdd (&counters[3], 1u);
}

// the linear number (rtc_launch_cell) of the cell of every traversal index
template <int DIM>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_cells_kernel (DropGeom G, unsigned * __restrict__ cell)
{
  const unsigned t = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (t >= G.N) return;
  int x[3];
  drop_decode<DIM> (G.depth, t, x);
  const unsigned n = (unsigned) G.n;
  cell[t] = (unsigned) x[0] + n*((unsigned) (G.n - 1 - x[1]) + (DIM == 3 ? n*(unsigned) (G.n - 1 - x[2]) : 0u));
}

static DropGeom drop_geom (const gfship_domain * dom)
{
  DropGeom G;
  G.L = dom->lay[dom->depth];
  G.depth = dom->depth;
  G.n = 1 << dom->depth;
  G.tb = std::min (dom->depth, dom->dim == 3 ? DROP_TILE_BITS_3D : DROP_TILE_BITS_2D);
  G.N = 1u << (dom->dim*dom->depth);
  for (int a = 0; a < 3; a++)
    G.per[a] = a < dom->dim && dom->side[2*a] == GFSHIP_SIDE_PERIODIC && dom->side[2*a + 1] == GFSHIP_SIDE_PERIODIC;
  return G;
}

static inline unsigned drop_grid (unsigned long long n) { return (unsigned) ((n + DROP_BLOCK - 1)/DROP_BLOCK); }

template <class T> static int drop_grow (T ** p, size_t count)
{
  if (*p) (void) hipFree (*p);
  *p = nullptr;
  GFSHIP_HIP (hipMalloc ((void **) p, count*sizeof (T)));
  return GFSHIP_OK;
}

static int drop_work (gfship_domain * dom, DropWork ** out)
{
  if (!dom->droplets) {
    DropWork * W = new DropWork;
    hipError_t e = hipMalloc ((void **) &W->counters, 4*sizeof (unsigned));
    if (e != hipSuccess) {
      delete W;
      GFSHIP_HIP (e);
    }
    dom->droplets = W;
  }
  *out = (DropWork *) dom->droplets;
  return GFSHIP_OK;
}

static int drop_reserve_cells (gfship_domain * dom, DropWork * W, size_t N)
{
  if (W->ncap >= N) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (dom->stream));
  W->ncap = 0;
  int r;
  if ((r = drop_grow (&W->parent, N)) || (r = drop_grow (&W->rank, N)) || (r = drop_grow (&W->tagi, N))) return r;
  W->ncap = N;
  return GFSHIP_OK;
}

static int drop_reserve_droplets (gfship_domain * dom, DropWork * W, size_t n)
{
  if (W->dcap >= n) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (dom->stream));
  W->dcap = 0;
  int r;
  unsigned ** a[] = { &W->sizes, &W->last, &W->segsize, &W->seg, &W->cursor, &W->sorted, &W->cell };
  for (unsigned ** p : a)
    if ((r = drop_grow (p, n))) return r;
  if ((r = drop_grow (&W->block, (n + 255)/256))) return r;
  W->dcap = n;
  return GFSHIP_OK;
}

static int drop_reserve_keys (gfship_domain * dom, DropWork * W, size_t n)
{
  if (W->kcap >= n) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (dom->stream));
  W->kcap = 0;
  int r;
  if ((r = drop_grow (&W->key, n)) || (r = drop_grow (&W->key2, n))) return r;
  W->kcap = n;
  return GFSHIP_OK;
}

static int drop_reserve_tmp (gfship_domain * dom, DropWork * W, size_t bytes)
{
  if (W->tmp_bytes >= bytes) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (dom->stream));
  if (W->tmp) (void) hipFree (W->tmp);
  W->tmp = nullptr;
  W->tmp_bytes = 0;
  GFSHIP_HIP (hipMalloc (&W->tmp, bytes));
  W->tmp_bytes = bytes;
  return GFSHIP_OK;
}

void droplets_free (gfship_domain * dom)
{
  DropWork * W = (DropWork *) dom->droplets;
  if (!W) return;
  void * a[] = { W->parent, W->rank, W->tagi, W->sizes, W->last, W->segsize, W->seg, W->cursor, W->sorted, W->cell,
		 W->block, W->key, W->key2, W->tmp, W->counters };
  for (void * p : a)
    if (p) (void) hipFree (p);
  delete W;
  dom->droplets = nullptr;
}

static int drop_scan (gfship_domain * dom, DropWork * W, const unsigned * in, unsigned * out, size_t count)
{
  size_t need = 0;
  int r;
  GFSHIP_HIP (hipcub::DeviceScan::ExclusiveSum (nullptr, need, in, out, count, dom->stream));
  if ((r = drop_reserve_tmp (dom, W, need))) return r;
  size_t bytes = W->tmp_bytes;
  GFSHIP_HIP (hipcub::DeviceScan::ExclusiveSum (W->tmp, bytes, in, out, count, dom->stream));
  return GFSHIP_OK;
}

// what the labelling refuses
static int drop_check (gfship_domain * dom, const char * what)
{
  GFSHIP_CHECK (dom != nullptr, GFSHIP_EINVAL, "null domain");
  GFSHIP_CHECK (!dom->has_external, GFSHIP_EUNSUPPORTED,
		"%s on a box with GfsBoundaryMpi sides is not supported: the tags of the boxes are not numbered "
		"together (unify_tag_range, src/domain.c:3662-3687)", what);
  GFSHIP_CHECK (dom->dim*dom->depth < 32, GFSHIP_EUNSUPPORTED,
		"%s: the %d-D box of level %d has 2^32 cells or more", what, dom->dim, dom->depth);
  return GFSHIP_OK;
}

// steps 1 and 2 up to the number of droplets: the roots in parent, their ranks in rank; *n is read back
static int drop_labels (gfship_domain * dom, DropWork * W, const DropGeom & G, const double * c, const double * fv,
			unsigned * n)
{
  int r;
  if ((r = drop_reserve_cells (dom, W, G.N))) return r;
  const unsigned ns = (unsigned) G.n >> G.tb;
  const unsigned long long plane = dom->dim == 3 ? (unsigned long long) G.n*G.n : (unsigned long long) G.n;
  const unsigned long long border = (unsigned long long) dom->dim*ns*plane;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (drop_tile_kernel<DIM>, dim3 (G.N >> (DIM*G.tb)), dim3 (DROP_BLOCK), 0, dom->stream, G, c, fv,
			W->parent);
    hipLaunchKernelGGL (drop_border_kernel<DIM>, dim3 (drop_grid (border)), dim3 (DROP_BLOCK), 0, dom->stream, G,
			border, W->parent);
  }, dom->dim == 3);
  hipLaunchKernelGGL (drop_flatten_kernel, dim3 (drop_grid (G.N)), dim3 (DROP_BLOCK), 0, dom->stream, G.N, W->parent,
		      W->tagi);
  GFSHIP_HIP (hipGetLastError ());
  if ((r = drop_scan (dom, W, W->tagi, W->rank, G.N))) return r;
  hipLaunchKernelGGL (drop_count_kernel, dim3 (1), dim3 (1), 0, dom->stream, G.N, W->rank, W->tagi, W->counters);
  GFSHIP_HIP (hipGetLastError ());
  GFSHIP_HIP (hipMemcpyAsync (n, W->counters, sizeof (unsigned), hipMemcpyDeviceToHost, dom->stream));
  GFSHIP_HIP (hipStreamSynchronize (dom->stream));
  return GFSHIP_OK;
}

// steps 2 and 3: the tags (into tagf too where given) and, with sizes, the size and the last leaf of the n droplets
static int drop_tags (gfship_domain * dom, DropWork * W, const DropGeom & G, double * tagf, unsigned n, bool sizes,
		      bool all)
{
  int r;
  if (sizes) {
    if ((r = drop_reserve_droplets (dom, W, n))) return r;
    GFSHIP_HIP (hipMemsetAsync (W->sizes, 0, n*sizeof (unsigned), dom->stream));
    GFSHIP_HIP (hipMemsetAsync (W->last, 0, n*sizeof (unsigned), dom->stream));
  }
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (drop_tag_kernel<DIM>, dim3 (drop_grid (G.N)), dim3 (DROP_BLOCK), 0, dom->stream, G, W->parent,
			W->rank, W->tagi, tagf, sizes ? W->sizes : nullptr, W->last, all ? 1 : 0);
  }, dom->dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

// step 4 (convert_droplets, :1311-1321; src/domain.c:3863-3872): min itself, or the (-1 - min)-th largest size
static int drop_min (gfship_domain * dom, DropWork * W, unsigned n, int min, unsigned * out)
{
  if (min >= 0) {
    *out = (unsigned) min;
    return GFSHIP_OK;
  }
  size_t need = 0;
  int r;
  GFSHIP_HIP (hipcub::DeviceRadixSort::SortKeysDescending (nullptr, need, W->sizes, W->sorted, n, 0, 32, dom->stream));
  if ((r = drop_reserve_tmp (dom, W, need))) return r;
  size_t bytes = W->tmp_bytes;
  GFSHIP_HIP (hipcub::DeviceRadixSort::SortKeysDescending (W->tmp, bytes, W->sizes, W->sorted, n, 0, 32, dom->stream));
  GFSHIP_HIP (hipMemcpyAsync (out, W->sorted + (size_t) (-1 - min), sizeof (unsigned), hipMemcpyDeviceToHost,
			      dom->stream));
  GFSHIP_HIP (hipStreamSynchronize (dom->stream));
  return GFSHIP_OK;
}

// step 7, on the leaves of the field and then on its ghosts
static int drop_reset (gfship_domain * dom, DropWork * W, const DropGeom & G, Field * V, unsigned min, double val)
{
  int r;
  if ((r = coarse_flush (dom, V, dom->depth, true))) return r;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (drop_reset_kernel<DIM>, dim3 (drop_grid (G.N)), dim3 (DROP_BLOCK), 0, dom->stream, G, W->tagi,
			W->sizes, min, val, V->lev[dom->depth], W->counters);
  }, dom->dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  V->zero[dom->depth] = false;
  return launch_bc (dom, V, V, dom->depth, 0);
}

} // namespace gfship

using namespace gfship;

// a GfsDropletToParticle on a list of particulates of a box
struct gfship_droplet_to_particle {
  gfship_particles * pl = nullptr;
  gfship_field c = -1;
  int min = 0;
  double reset = 0., density = 0.;
  // the mask: the variable c, the variable the function names, or the values of the function by traversal index
  gfship_field mask = -1;
  gfship::RtcKernel * fn = nullptr;
  bool constant = false;
  double value = 0.;
  std::vector<gfship_field> read;
  double * fv = nullptr;
  unsigned * cells = nullptr;
};

extern "C" {

int gfship_tag_droplets (gfship_domain * dom, gfship_field c, gfship_field tag, unsigned * n)
{
  int r = drop_check (dom, "gfs_domain_tag_droplets");
  if (r) return r;
  GFSHIP_CHECK (n != nullptr, GFSHIP_EINVAL, "null output pointer");
  Field * C = get_field (dom, c), * T = get_field (dom, tag);
  GFSHIP_CHECK (C && T && C != T, GFSHIP_EINVAL, "c and tag are two fields of the domain");
  GFSHIP_HIP (hipSetDevice (dom->device));
  if ((r = before_write (dom))) return r;
  if ((r = coarse_flush (dom, T, dom->depth, true))) return r;
  DropWork * W;
  if ((r = drop_work (dom, &W))) return r;
  const DropGeom G = drop_geom (dom);
  if ((r = drop_labels (dom, W, G, C->lev[dom->depth], nullptr, n))) return r;
  if ((r = drop_tags (dom, W, G, T->lev[dom->depth], *n, false, false))) return r;
  T->zero[dom->depth] = false;
  return GFSHIP_OK;
}

int gfship_tag_droplets_time (gfship_domain * dom, gfship_field c, gfship_field tag, int reps, double * ms)
{
  GFSHIP_CHECK (dom && reps > 0 && ms, GFSHIP_EINVAL, "invalid argument");
  unsigned n;
  int r = gfship_tag_droplets (dom, c, tag, &n);      /* warm-up: the work arrays exist afterwards */
  if (r) return r;
  GFSHIP_HIP (hipEventRecord (dom->ev0, dom->stream));
  for (int q = 0; q < reps; q++)
    if ((r = gfship_tag_droplets (dom, c, tag, &n))) return r;
  GFSHIP_HIP (hipEventRecord (dom->ev1, dom->stream));
  GFSHIP_HIP (hipEventSynchronize (dom->ev1));
  float t = 0.f;
  GFSHIP_HIP (hipEventElapsedTime (&t, dom->ev0, dom->ev1));
  *ms = (double) t/reps;
  return GFSHIP_OK;
}

int gfship_remove_droplets (gfship_domain * dom, gfship_field c, gfship_field v, int min, double val)
{
  int r = drop_check (dom, "gfs_domain_remove_droplets");
  if (r) return r;
  Field * C = get_field (dom, c), * V = get_field (dom, v);
  GFSHIP_CHECK (C && V, GFSHIP_EINVAL, "c and v are fields of the domain");
  GFSHIP_HIP (hipSetDevice (dom->device));
  if ((r = before_write (dom))) return r;
  DropWork * W;
  if ((r = drop_work (dom, &W))) return r;
  const DropGeom G = drop_geom (dom);
  unsigned n = 0, umin = 0;
  if ((r = drop_labels (dom, W, G, C->lev[dom->depth], nullptr, &n))) return r;
  if (!(n > 0 && -(long) min < (long) n)) return GFSHIP_OK;      /* src/domain.c:3851 */
  if ((r = drop_tags (dom, W, G, nullptr, n, true, true))) return r;
  if ((r = drop_min (dom, W, n, min, &umin))) return r;
  return drop_reset (dom, W, G, V, umin, val);
}

int gfship_droplet_to_particle_create (gfship_droplet_to_particle ** out, gfship_particles * pl, gfship_field c,
					int min, double reset, double density, const char * function, int nvars,
					const char * const * names, const gfship_field * fields)
{
  GFSHIP_CHECK (out != nullptr, GFSHIP_EINVAL, "null output pointer");
  *out = nullptr;
  int r = feed_check (pl, "GfsDropletToParticle");
  if (r) return r;
  if ((r = feed_names_check (nvars, names, fields, "field"))) return r;
  gfship_domain * dom = pl->dom;
  GFSHIP_CHECK (get_field (dom, c) != nullptr, GFSHIP_EINVAL, "c is not a field of the domain");
  for (int q = 0; q < nvars; q++)
    GFSHIP_CHECK (get_field (dom, fields[q]) != nullptr, GFSHIP_EINVAL, "`%s' of the table is not a field of the domain", names[q]);
  GFSHIP_HIP (hipSetDevice (dom->device));
  gfship_droplet_to_particle * d = new gfship_droplet_to_particle;
  d->pl = pl; d->c = d->mask = c; d->min = min; d->reset = reset; d->density = density;
  if (function) {
    std::string text (function);
    const size_t b = text.find_first_not_of (" \t\r\n"), e = text.find_last_not_of (" \t\r\n");
    text = b == std::string::npos ? std::string () : text.substr (b, e - b + 1);
    bool variable = false;
    for (int q = 0; q < nvars && !variable; q++)
      if (text == names[q]) {      /* gfs_function_get_variable: the function is that variable */
	d->mask = fields[q];
	variable = true;
      }
    if (!variable) {
      const DropGeom G = drop_geom (dom);
      d->mask = -1;
      if (text_constant (function, &d->value)) d->constant = true;
      else {
	const std::vector<const char *> named = named_variables (function, nvars, names, fields, d->read);
	if ((r = rtc_compile_cell (dom, function, (int) named.size (), named.data (), &d->fn))) {
	  gfship_droplet_to_particle_destroy (d);
	  return r;
	}
      }
      hipError_t e1 = hipMalloc ((void **) &d->fv, (size_t) G.N*sizeof (double));
      hipError_t e2 = e1 == hipSuccess ? hipMalloc ((void **) &d->cells, (size_t) G.N*sizeof (unsigned)) : e1;
      if (e2 != hipSuccess) {
	gfship_droplet_to_particle_destroy (d);
	GFSHIP_HIP (e2);
      }
      with_bools ([&] (auto D3) {
	constexpr int DIM = decltype (D3)::value ? 3 : 2;
	hipLaunchKernelGGL (drop_cells_kernel<DIM>, dim3 (drop_grid (G.N)), dim3 (DROP_BLOCK), 0, dom->stream, G,
			    d->cells);
      }, dom->dim == 3);
      hipError_t e3 = hipGetLastError ();
      if (e3 != hipSuccess) {
	gfship_droplet_to_particle_destroy (d);
	GFSHIP_HIP (e3);
      }
    }
  }
  *out = d;
  return GFSHIP_OK;
}

int gfship_droplet_to_particle_event (gfship_droplet_to_particle * d, gfship_droplet_info * info)
{
  GFSHIP_CHECK (d != nullptr, GFSHIP_EINVAL, "null GfsDropletToParticle");
  if (info) info->n = info->min = info->converted = info->reset = 0u;
  gfship_particles * pl = d->pl;
  int r = feed_check (pl, "GfsDropletToParticle");
  if (r) return r;
  gfship_domain * dom = pl->dom;
  const gfship_sim_view sv = gfship_sim_view_get (pl->sim);
  GFSHIP_CHECK (!sv.has_alpha || sv.alpha_cell >= 0, GFSHIP_EUNSUPPORTED,
		"GfsDropletToParticle together with GfsPhysicalParams { alpha } needs alpha at the cell centres "
		"(mass = volume/alpha): call gfship_sim_set_alpha_cell first");
  GFSHIP_HIP (hipSetDevice (dom->device));
  if ((r = before_write (dom))) return r;
  Field * C = get_field (dom, d->c);
  if (!C) return GFSHIP_EINVAL;
  DropWork * W;
  if ((r = drop_work (dom, &W))) return r;
  const DropGeom G = drop_geom (dom);
  const Layout & L = dom->lay[dom->depth];
  /* the mask (gfs_droplet_to_particle_event, :1368-1393) */
  const double * mask = nullptr;
  if (d->mask >= 0) {
    Field * M = get_field (dom, d->mask);
    if (!M) return GFSHIP_EINVAL;
    mask = M->lev[dom->depth];
  }
  else if (d->constant) {
    if ((r = launch_fill (dom->stream, (long) G.N, d->value, d->fv))) return r;
  }
  else {
    std::vector<const double *> read;
    for (gfship_field v : d->read) {
      Field * F = get_field (dom, v);
      if (!F) return GFSHIP_EINVAL;
      read.push_back (F->lev[dom->depth]);
    }
    if ((r = rtc_launch_cell (d->fn, dom->stream, (int) G.N, L, d->cells, gfship_sim_time (pl->sim),
			      (int) read.size (), read.data (), d->fv)))
      return r;
  }
  unsigned n = 0, umin = 0;
  if ((r = drop_labels (dom, W, G, mask, mask ? nullptr : d->fv, &n))) return r;
  if (info) info->n = n;
  if (!(n > 0 && -(long) d->min < (long) n)) return GFSHIP_OK;      /* :1381 */
  GFSHIP_CHECK ((long) pl->n + (long) n <= 0x7fffffffL, GFSHIP_ENOMEM, "the list would hold 2^31 slots or more");
  if ((r = drop_tags (dom, W, G, nullptr, n, true, false))) return r;
  if ((r = drop_min (dom, W, n, d->min, &umin))) return r;
  if (info) info->min = umin;
  /* the segments of keys of the droplets that convert: at most min - 1 leaves each */
  unsigned long long cap = umin > 2u ? std::min ((unsigned long long) G.N, (unsigned long long) n*(umin - 1u)) : 0ull;
  if ((r = drop_reserve_keys (dom, W, (size_t) cap))) return r;
  if ((r = particles_reserve (pl, pl->n + (int) n))) return r;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (drop_candidate_kernel<DIM>, dim3 (drop_grid (n)), dim3 (DROP_BLOCK), 0, dom->stream, G, n, umin,
			W->sizes, W->last, W->segsize, W->cursor);
  }, dom->dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  if ((r = drop_scan (dom, W, W->segsize, W->seg, n))) return r;
  const unsigned long long * sorted = W->key;
  if (cap) {
    GFSHIP_HIP (hipMemsetAsync (W->key, 0xFF, (size_t) cap*sizeof (unsigned long long), dom->stream));
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      hipLaunchKernelGGL (drop_keys_kernel<DIM>, dim3 (drop_grid (G.N)), dim3 (DROP_BLOCK), 0, dom->stream, G, W->tagi,
			  W->segsize, W->seg, W->cursor, cap, W->key);
    }, dom->dim == 3);
    GFSHIP_HIP (hipGetLastError ());
    int bits = 33;
    while (bits < 64 && (1ull << (bits - 32)) <= (unsigned long long) n) bits++;
    size_t need = 0;
    GFSHIP_HIP (hipcub::DeviceRadixSort::SortKeys (nullptr, need, W->key, W->key2, cap, 0, bits, dom->stream));
    if ((r = drop_reserve_tmp (dom, W, need))) return r;
    size_t bytes = W->tmp_bytes;
    GFSHIP_HIP (hipcub::DeviceRadixSort::SortKeys (W->tmp, bytes, W->key, W->key2, cap, 0, bits, dom->stream));
    sorted = W->key2;
  }
  DropConvertArgs A;
  A.G = G; A.n = n; A.base = pl->n;
  A.sizes = W->sizes; A.segsize = W->segsize; A.seg = W->seg; A.key = sorted;
  A.c = C->lev[dom->depth];
  A.alpha = sv.alpha_cell >= 0 ? dom->fields[sv.alpha_cell].lev[dom->depth] : nullptr;
  for (int a = 0; a < 3; a++) {
    A.u[a] = a < dom->dim ? dom->fields[sv.u[a]].lev[dom->depth] : nullptr;
    A.pos[a] = pl->pos[a]; A.old[a] = pl->old[a]; A.vel[a] = pl->vel[a]; A.force[a] = pl->force[a];
  }
  A.mass = pl->mass; A.volume = pl->volume; A.orig = pl->orig; A.cell = W->cell;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (drop_convert_kernel<DIM>, dim3 (drop_grid (n)), dim3 (DROP_BLOCK), 0, dom->stream, A);
  }, dom->dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  const int base = pl->n;
  if ((r = launch_feed_ids (pl, base, (int) n, W->cell, W->block))) return r;
  pl->n += (int) n;
  if (info) {
    hipLaunchKernelGGL (drop_made_kernel, dim3 (drop_grid (n)), dim3 (DROP_BLOCK), 0, dom->stream, n, pl->alive + base,
			W->counters);
    GFSHIP_HIP (hipGetLastError ());
  }
  if ((r = drop_reset (dom, W, G, C, umin, d->reset))) return r;
  if (info) {
    unsigned h[4];
    GFSHIP_HIP (hipMemcpyAsync (h, W->counters, sizeof h, hipMemcpyDeviceToHost, dom->stream));
    GFSHIP_HIP (hipStreamSynchronize (dom->stream));
    info->converted = h[2];
    info->reset = h[3];
  }
  return GFSHIP_OK;
}

void gfship_droplet_to_particle_destroy (gfship_droplet_to_particle * d)
{
  if (!d) return;
  (void) hipStreamSynchronize (d->pl->stream);
  if (d->fv) (void) hipFree (d->fv);
  if (d->cells) (void) hipFree (d->cells);
  rtc_free (d->fn);
  delete d;
}

} // extern "C"
