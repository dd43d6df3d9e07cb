// droplets.hpp -- what the droplets of a uniform box (droplets.hip) and of a refined tree (tree_droplets.hip) share:
// the union-find in which the smaller label wins, and everything that follows the labels -- steps 2 to 7 of the
// header of droplets.hip: the rank scan, the sizes and the last leaf, min, the keys, their sort and the ordered fp64
// sums, the conversion into slots of the list, the reset.
//
// A label is the position of a leaf in traversal order (32 bits); the work arrays are indexed by it.  What the two
// meshes do differently is behind a geometry G (BoxDrops<DIM>, droplets.hip; TreeDrops<DIM>, tree_droplets.hip), a
// kernel argument with, for the leaf of traversal position t,
//   N: the number of leaves;                      index (t): its place in the arrays of a variable;
//   on_side (t): it touches a side of the box;    volume (t): pow (h, FTT_DIMENSION);
//   pos (t, x): ftt_cell_pos;                     locate (pos, &cell, &idx): gfs_domain_locate (pos, -1), the cell for
//                                                 launch_feed_ids and its place in the arrays;
// and a host mesh M with dim, stream, N and geom<DIM> ().
#pragma once
#include "particles.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <vector>

namespace gfship {

constexpr unsigned DROP_NONE = 0xFFFFFFFFu;
constexpr int DROP_BLOCK = 256;
constexpr double DROP_THRESHOLD = 1e-4;        /* src/domain.c:3564 */

// the work arrays of the labelling, kept by the domain or by the tree between calls
struct DropWork {
  unsigned * parent = nullptr, * rank = nullptr, * tagi = nullptr;      // per leaf, by traversal position
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

// 1c. every leaf takes its root; flag = the leaf is a root
static __global__ void __launch_bounds__(DROP_BLOCK)
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

static __global__ void drop_count_kernel (unsigned N, const unsigned * __restrict__ rank,
					  const unsigned * __restrict__ flag, unsigned * __restrict__ counters)
{
  counters[0] = rank[N - 1] + flag[N - 1];
  counters[1] = counters[2] = counters[3] = 0u;
}

// 2 and 3. tag = 1 + the rank of the root (0 outside), into tagi and, as a double, into the variable tagf; the size of
// every droplet -- all its leaves (compute_droplet_size, src/domain.c:3805-3810), or those that touch no side
// (compute_droplet_properties) -- and its last leaf
template <class G>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_tag_kernel (G geom, const unsigned * __restrict__ parent, const unsigned * __restrict__ rank,
		 unsigned * __restrict__ tagi, double * __restrict__ tagf, unsigned * __restrict__ sizes,
		 unsigned * __restrict__ last, int all)
{
  const unsigned t = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  const bool valid = t < geom.N;
  unsigned tag = 0u;
  bool counted = false;
  if (valid) {
    const unsigned p = parent[t];
    tag = p == DROP_NONE ? 0u : 1u + rank[p];
    tagi[t] = tag;
    if (tagf) tagf[geom.index (t)] = (double) tag;
    counted = tag && (all || !geom.on_side (t));
  }
  if (!sizes) return;
  /* the lanes of a wave that share a tag add once (a wave is 64 consecutive traversal positions: mostly one droplet),
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
template <class G>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_candidate_kernel (G geom, unsigned n, unsigned min, const unsigned * __restrict__ sizes,
		       const unsigned * __restrict__ last, unsigned * __restrict__ segsize,
		       unsigned * __restrict__ cursor)
{
  const unsigned i = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (i >= n) return;
  const unsigned s = sizes[i];
  segsize[i] = !geom.on_side (last[i]) && s < min && s > 1u ? s : 0u;
  cursor[i] = 0u;
}

// 5. the keys of the counted leaves of the droplets that convert, anywhere in the segment of their droplet: the sort
// puts them in traversal order
template <class G>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_keys_kernel (G geom, const unsigned * __restrict__ tagi, const unsigned * __restrict__ segsize,
		  const unsigned * __restrict__ seg, unsigned * __restrict__ cursor, unsigned long long cap,
		  unsigned long long * __restrict__ key)
{
  const unsigned t = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (t >= geom.N) return;
  const unsigned tag = tagi[t];
  if (!tag || !segsize[tag - 1]) return;
  if (geom.on_side (t)) return;
  const unsigned long long slot = (unsigned long long) seg[tag - 1] + atomicAdd (&cursor[tag - 1], 1u);
  if (slot < cap) key[slot] = (unsigned long long) (tag - 1) << 32 | t;
}

template <class G>
struct DropConvertArgs {
  G geom;
  unsigned n;
  int base;
  const unsigned * sizes, * segsize, * seg;
  const unsigned long long * key;
  const double * c, * u[3], * alpha;      // alpha: nullptr on a tree and without GfsPhysicalParams { alpha }
  double * pos[3], * old[3], * vel[3], * force[3], * mass, * volume;
  unsigned * orig, * cell;
};

// 5 and 6. compute_droplet_properties (:1214-1228) over the leaves of a droplet in traversal order, then
// convert_droplets (:1326-1338) up to add_particulate: one droplet per thread, one slot of the list per droplet
template <int DIM, class G>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_convert_kernel (DropConvertArgs<G> A)
{
  const unsigned i = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (i >= A.n) return;
  const int s = A.base + (int) i;
  double pos[3] = { 0., 0., 0. }, vel[3] = { 0., 0., 0. }, volume = 0., mass = 0.;
  unsigned cell = PSOURCE_NO_CELL;
  const unsigned size = A.segsize[i];
  if (size) {
    const unsigned long long * key = A.key + A.seg[i];
    for (unsigned q = 0; q < size; q++) {
      const unsigned t = (unsigned) key[q];
      const long idx = A.geom.index (t);
      double x[3];
      A.geom.pos (t, x);
      volume += A.geom.volume (t)*A.c[idx];
#pragma unroll
      for (int a = 0; a < DIM; a++) {
	pos[a] += x[a];
	vel[a] += A.u[a][idx];
      }
    }
#pragma unroll
    for (int a = 0; a < DIM; a++) {
      pos[a] = pos[a]/(double) A.sizes[i];
      vel[a] = vel[a]/(double) A.sizes[i];
    }
    long at;
    if (A.geom.locate (pos, cell, at)) {
      mass = A.alpha ? 1./A.alpha[at] : 1.;
      mass *= volume;
    }
    else {
      cell = PSOURCE_NO_CELL;
      volume = 0.;
    }
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
static __global__ void __launch_bounds__(DROP_BLOCK)
drop_made_kernel (unsigned n, const unsigned char * __restrict__ alive, unsigned * __restrict__ counters)
{
  const unsigned i = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (i < n && alive[i]) atomicAdd (&counters[2], 1u);
}

// 7. reset_small_fraction (:1187-1192, src/domain.c:3812-3817): v = val on the leaves of every droplet smaller than min
template <class G>
__global__ void __launch_bounds__(DROP_BLOCK)
drop_reset_kernel (G geom, const unsigned * __restrict__ tagi, const unsigned * __restrict__ sizes,
		   unsigned min, double val, double * __restrict__ v, unsigned * __restrict__ counters)
{
  const unsigned t = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (t >= geom.N) return;
  const unsigned tag = tagi[t];
  if (!tag || !(sizes[tag - 1] < min)) return;
  v[geom.index (t)] = val;
  atomicAdd (&counters[3], 1u);
}

static inline unsigned drop_grid (unsigned long long n) { return (unsigned) ((n + DROP_BLOCK - 1)/DROP_BLOCK); }

template <class T> static int drop_grow (T ** p, size_t count)
{
  if (*p) (void) hipFree (*p);
  *p = nullptr;
  GFSHIP_HIP (hipMalloc ((void **) p, count*sizeof (T)));
  return GFSHIP_OK;
}

static inline int drop_work_new (DropWork ** out)
{
  DropWork * W = new DropWork;
  hipError_t e = hipMalloc ((void **) &W->counters, 4*sizeof (unsigned));
  if (e != hipSuccess) {
    delete W;
    GFSHIP_HIP (e);
  }
  *out = W;
  return GFSHIP_OK;
}

static inline void drop_work_free (DropWork * W)
{
  if (!W) return;
  void * a[] = { W->parent, W->rank, W->tagi, W->sizes, W->last, W->segsize, W->seg, W->cursor, W->sorted, W->cell,
		 W->block, W->key, W->key2, W->tmp, W->counters };
  for (void * p : a)
    if (p) (void) hipFree (p);
  delete W;
}

static inline int drop_reserve_cells (hipStream_t stream, DropWork * W, size_t N)
{
  if (W->ncap >= N) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (stream));
  W->ncap = 0;
  int r;
  if ((r = drop_grow (&W->parent, N)) || (r = drop_grow (&W->rank, N)) || (r = drop_grow (&W->tagi, N))) return r;
  W->ncap = N;
  return GFSHIP_OK;
}

static inline int drop_reserve_droplets (hipStream_t stream, DropWork * W, size_t n)
{
  if (W->dcap >= n) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (stream));
  W->dcap = 0;
  int r;
  unsigned ** a[] = { &W->sizes, &W->last, &W->segsize, &W->seg, &W->cursor, &W->sorted, &W->cell };
  for (unsigned ** p : a)
    if ((r = drop_grow (p, n))) return r;
  if ((r = drop_grow (&W->block, (n + 255)/256))) return r;
  W->dcap = n;
  return GFSHIP_OK;
}

static inline int drop_reserve_keys (hipStream_t stream, DropWork * W, size_t n)
{
  if (W->kcap >= n) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (stream));
  W->kcap = 0;
  int r;
  if ((r = drop_grow (&W->key, n)) || (r = drop_grow (&W->key2, n))) return r;
  W->kcap = n;
  return GFSHIP_OK;
}

static inline int drop_reserve_tmp (hipStream_t stream, DropWork * W, size_t bytes)
{
  if (W->tmp_bytes >= bytes) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (stream));
  if (W->tmp) (void) hipFree (W->tmp);
  W->tmp = nullptr;
  W->tmp_bytes = 0;
  GFSHIP_HIP (hipMalloc (&W->tmp, bytes));
  W->tmp_bytes = bytes;
  return GFSHIP_OK;
}

static inline int drop_scan (hipStream_t stream, DropWork * W, const unsigned * in, unsigned * out, size_t count)
{
  size_t need = 0;
  int r;
  GFSHIP_HIP (hipcub::DeviceScan::ExclusiveSum (nullptr, need, in, out, count, stream));
  if ((r = drop_reserve_tmp (stream, W, need))) return r;
  size_t bytes = W->tmp_bytes;
  GFSHIP_HIP (hipcub::DeviceScan::ExclusiveSum (W->tmp, bytes, in, out, count, stream));
  return GFSHIP_OK;
}

// the end of step 1 and step 2 up to the number of droplets, once the forest is in parent: the roots in parent,
// their ranks in rank; *n is read back
static inline int drop_ranks (hipStream_t stream, DropWork * W, unsigned N, unsigned * n)
{
  int r;
  hipLaunchKernelGGL (drop_flatten_kernel, dim3 (drop_grid (N)), dim3 (DROP_BLOCK), 0, stream, N, W->parent, W->tagi);
  GFSHIP_HIP (hipGetLastError ());
  if ((r = drop_scan (stream, W, W->tagi, W->rank, N))) return r;
  hipLaunchKernelGGL (drop_count_kernel, dim3 (1), dim3 (1), 0, stream, N, W->rank, W->tagi, W->counters);
  GFSHIP_HIP (hipGetLastError ());
  GFSHIP_HIP (hipMemcpyAsync (n, W->counters, sizeof (unsigned), hipMemcpyDeviceToHost, stream));
  GFSHIP_HIP (hipStreamSynchronize (stream));
  return GFSHIP_OK;
}

// steps 2 and 3: the tags (into tagf too where given) and, with sizes, the size and the last leaf of the n droplets
template <class Mesh>
int drop_tags (const Mesh & M, DropWork * W, double * tagf, unsigned n, bool sizes, bool all)
{
  int r;
  if (sizes) {
    if ((r = drop_reserve_droplets (M.stream, W, n))) return r;
    GFSHIP_HIP (hipMemsetAsync (W->sizes, 0, n*sizeof (unsigned), M.stream));
    GFSHIP_HIP (hipMemsetAsync (W->last, 0, n*sizeof (unsigned), M.stream));
  }
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    auto G = M.template geom<DIM> ();
    hipLaunchKernelGGL (drop_tag_kernel<decltype (G)>, dim3 (drop_grid (M.N)), dim3 (DROP_BLOCK), 0, M.stream, G,
			W->parent, W->rank, W->tagi, tagf, sizes ? W->sizes : nullptr, W->last, all ? 1 : 0);
  }, M.dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

// step 4 (convert_droplets, :1311-1321; src/domain.c:3863-3872): min itself, or the (-1 - min)-th largest size
static inline int drop_min (hipStream_t stream, DropWork * W, unsigned n, int min, unsigned * out)
{
  if (min >= 0) {
    *out = (unsigned) min;
    return GFSHIP_OK;
  }
  size_t need = 0;
  int r;
  GFSHIP_HIP (hipcub::DeviceRadixSort::SortKeysDescending (nullptr, need, W->sizes, W->sorted, n, 0, 32, stream));
  if ((r = drop_reserve_tmp (stream, W, need))) return r;
  size_t bytes = W->tmp_bytes;
  GFSHIP_HIP (hipcub::DeviceRadixSort::SortKeysDescending (W->tmp, bytes, W->sizes, W->sorted, n, 0, 32, stream));
  GFSHIP_HIP (hipMemcpyAsync (out, W->sorted + (size_t) (-1 - min), sizeof (unsigned), hipMemcpyDeviceToHost, stream));
  GFSHIP_HIP (hipStreamSynchronize (stream));
  return GFSHIP_OK;
}

// step 7 on the leaves of the array v of a variable; its ghosts are the caller's
template <class Mesh>
int drop_reset_leaves (const Mesh & M, DropWork * W, double * v, unsigned min, double val)
{
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    auto G = M.template geom<DIM> ();
    hipLaunchKernelGGL (drop_reset_kernel<decltype (G)>, dim3 (drop_grid (M.N)), dim3 (DROP_BLOCK), 0, M.stream, G,
			W->tagi, W->sizes, min, val, v, W->counters);
  }, M.dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

// steps 5 and 6 (convert_droplets, :1323-1340) for the n droplets whose sizes and last leaves drop_tags has left: the
// n slots after those of the list in use, in tag order.  c, u, alpha: the arrays of the variables; made: count the
// particles into counters[2]
template <class Mesh>
int drop_convert (const Mesh & M, DropWork * W, gfship_particles * pl, unsigned n, unsigned umin, const double * c,
		  const double * const u[3], const double * alpha, bool made)
{
  int r;
  /* the segments of keys of the droplets that convert: at most min - 1 leaves each */
  unsigned long long cap = umin > 2u ? std::min ((unsigned long long) M.N, (unsigned long long) n*(umin - 1u)) : 0ull;
  if ((r = drop_reserve_keys (M.stream, W, (size_t) cap))) return r;
  if ((r = particles_reserve (pl, pl->n + (int) n))) return r;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    auto G = M.template geom<DIM> ();
    hipLaunchKernelGGL (drop_candidate_kernel<decltype (G)>, dim3 (drop_grid (n)), dim3 (DROP_BLOCK), 0, M.stream, G,
			n, umin, W->sizes, W->last, W->segsize, W->cursor);
  }, M.dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  if ((r = drop_scan (M.stream, W, W->segsize, W->seg, n))) return r;
  const unsigned long long * sorted = W->key;
  if (cap) {
    GFSHIP_HIP (hipMemsetAsync (W->key, 0xFF, (size_t) cap*sizeof (unsigned long long), M.stream));
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      auto G = M.template geom<DIM> ();
      hipLaunchKernelGGL (drop_keys_kernel<decltype (G)>, dim3 (drop_grid (M.N)), dim3 (DROP_BLOCK), 0, M.stream, G,
			  W->tagi, W->segsize, W->seg, W->cursor, cap, W->key);
    }, M.dim == 3);
    GFSHIP_HIP (hipGetLastError ());
    int bits = 33;
    while (bits < 64 && (1ull << (bits - 32)) <= (unsigned long long) n) bits++;
    size_t need = 0;
    GFSHIP_HIP (hipcub::DeviceRadixSort::SortKeys (nullptr, need, W->key, W->key2, cap, 0, bits, M.stream));
    if ((r = drop_reserve_tmp (M.stream, W, need))) return r;
    size_t bytes = W->tmp_bytes;
    GFSHIP_HIP (hipcub::DeviceRadixSort::SortKeys (W->tmp, bytes, W->key, W->key2, cap, 0, bits, M.stream));
    sorted = W->key2;
  }
  const int base = pl->n;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    auto G = M.template geom<DIM> ();
    DropConvertArgs<decltype (G)> A;
    A.geom = G; A.n = n; A.base = base;
    A.sizes = W->sizes; A.segsize = W->segsize; A.seg = W->seg; A.key = sorted;
    A.c = c; A.alpha = alpha;
    for (int a = 0; a < 3; a++) {
      A.u[a] = u[a];
      A.pos[a] = pl->pos[a]; A.old[a] = pl->old[a]; A.vel[a] = pl->vel[a]; A.force[a] = pl->force[a];
    }
    A.mass = pl->mass; A.volume = pl->volume; A.orig = pl->orig; A.cell = W->cell;
    hipLaunchKernelGGL ((drop_convert_kernel<DIM, decltype (G)>), dim3 (drop_grid (n)), dim3 (DROP_BLOCK), 0, M.stream,
			A);
  }, M.dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  if ((r = launch_feed_ids (pl, base, (int) n, W->cell, W->block))) return r;
  pl->n += (int) n;
  if (made) {
    hipLaunchKernelGGL (drop_made_kernel, dim3 (drop_grid (n)), dim3 (DROP_BLOCK), 0, M.stream, n, pl->alive + base,
			W->counters);
    GFSHIP_HIP (hipGetLastError ());
  }
  return GFSHIP_OK;
}

// particles made and cells reset, once the stream has been waited for
static inline int drop_info (hipStream_t stream, DropWork * W, gfship_droplet_info * info)
{
  unsigned h[4];
  GFSHIP_HIP (hipMemcpyAsync (h, W->counters, sizeof h, hipMemcpyDeviceToHost, stream));
  GFSHIP_HIP (hipStreamSynchronize (stream));
  info->converted = h[2];
  info->reset = h[3];
  return GFSHIP_OK;
}

// a GfsDropletToParticle on a list of a tree (tree_droplets.hip): the event and what its destruction frees there
int tree_droplet_event (gfship_droplet_to_particle * d, gfship_droplet_info * info);

} // namespace gfship

// a GfsDropletToParticle on a list of particulates of a box, or of a tree (pl->tree: the variables are GFSHIP_TREE_*
// numbers, the arrays hold every cell of every level)
struct gfship_droplet_to_particle {
  gfship_particles * pl = nullptr;
  int c = -1;
  int min = 0;
  double reset = 0., density = 0.;
  // the mask: the variable c, the variable the function names, or the values of the function by traversal index (a
  // box) or at every cell of every level (a tree)
  int mask = -1;
  gfship::RtcKernel * fn = nullptr;
  bool constant = false;
  double value = 0.;
  std::vector<gfship_field> read;
  double * fv = nullptr;
  unsigned * cells = nullptr;
};
