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
// Steps 1c to 7 and the union-find itself are in droplets.hpp, templated on a geometry: the refined trees
// (tree_droplets.hip) label differently and share the rest.
#include "particle_events.hpp"
#include "droplets.hpp"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace gfship {

constexpr int DROP_TILE_BITS_2D = 4, DROP_TILE_BITS_3D = 3;

struct DropGeom {
  Layout L;
  int depth, n, tb;      // levels, cells per side, log2 of the side of a tile
  unsigned N;            // cells
  int per[3];            // both sides of the direction are periodic
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

// the leaves of the box as the geometry of droplets.hpp
template <int DIM>
struct BoxDrops {
  DropGeom G;
  unsigned N;
  __device__ __forceinline__ long index (unsigned t) const {
    int x[3];
    drop_decode<DIM> (G.depth, t, x);
    return drop_index<DIM> (G, x);
  }
  __device__ __forceinline__ bool on_side (unsigned t) const {
    int x[3];
    drop_decode<DIM> (G.depth, t, x);
    return drop_on_side<DIM> (G, x);
  }
  __device__ __forceinline__ double volume (unsigned) const {
    const double h = 1./(double) G.n;
    return DIM == 3 ? h*h*h : h*h;      /* pow (h, FTT_DIMENSION): powers of two */
  }
  __device__ __forceinline__ void pos (unsigned t, double p[3]) const {
    int x[3];
    drop_decode<DIM> (G.depth, t, x);
    const int ix[3] = { x[0], G.n - 1 - x[1], G.n - 1 - x[2] };
    const double h = 1./(double) G.n;
    p[2] = 0.;
#pragma unroll
    for (int a = 0; a < DIM; a++)
      p[a] = -0.5 + (ix[a] + 0.5)*h;      /* ftt_cell_pos: dyadic, exact */
  }
  __device__ __forceinline__ bool locate (const double p[3], unsigned & cell, long & at) const {
    int c[3];
    if (!gfship::locate<DIM> (G.depth, p, c)) return false;
    const unsigned n = (unsigned) G.n;
    cell = (unsigned) (c[0] - 1) + n*((unsigned) (c[1] - 1) + (DIM == 3 ? n*(unsigned) (c[2] - 1) : 0u));
    at = G.L.idx (c[0], c[1], c[2]);
    return true;
  }
};

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

// the box as the host mesh of droplets.hpp
struct BoxDropMesh {
  DropGeom G;
  int dim;
  hipStream_t stream;
  unsigned N;
  explicit BoxDropMesh (const gfship_domain * dom) : G (drop_geom (dom)), dim (dom->dim), stream (dom->stream), N (G.N) {}
  template <int DIM> BoxDrops<DIM> geom () const { return BoxDrops<DIM> { G, G.N }; }
};

static int drop_work (gfship_domain * dom, DropWork ** out)
{
  if (!dom->droplets) {
    DropWork * W;
    int r = drop_work_new (&W);
    if (r) return r;
    dom->droplets = W;
  }
  *out = (DropWork *) dom->droplets;
  return GFSHIP_OK;
}

void droplets_free (gfship_domain * dom)
{
  drop_work_free ((DropWork *) dom->droplets);
  dom->droplets = nullptr;
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
  if ((r = drop_reserve_cells (dom->stream, W, G.N))) return r;
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
  GFSHIP_HIP (hipGetLastError ());
  return drop_ranks (dom->stream, W, G.N, n);
}

// step 7, on the leaves of the field and then on its ghosts
static int drop_reset (gfship_domain * dom, DropWork * W, const BoxDropMesh & M, Field * V, unsigned min, double val)
{
  int r;
  if ((r = coarse_flush (dom, V, dom->depth, true))) return r;
  if ((r = drop_reset_leaves (M, W, V->lev[dom->depth], min, val))) return r;
  V->zero[dom->depth] = false;
  return launch_bc (dom, V, V, dom->depth, 0);
}

} // namespace gfship

using namespace gfship;

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
  const BoxDropMesh M (dom);
  if ((r = drop_labels (dom, W, M.G, C->lev[dom->depth], nullptr, n))) return r;
  if ((r = drop_tags (M, W, T->lev[dom->depth], *n, false, false))) return r;
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
  const BoxDropMesh M (dom);
  unsigned n = 0, umin = 0;
  if ((r = drop_labels (dom, W, M.G, C->lev[dom->depth], nullptr, &n))) return r;
  if (!(n > 0 && -(long) min < (long) n)) return GFSHIP_OK;      /* src/domain.c:3851 */
  if ((r = drop_tags (M, W, nullptr, n, true, true))) return r;
  if ((r = drop_min (dom->stream, W, n, min, &umin))) return r;
  return drop_reset (dom, W, M, V, umin, val);
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
  if (pl && pl->tree) return tree_droplet_event (d, info);      /* a handle of gfship_tree_droplet_to_particle_create */
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
  const BoxDropMesh M (dom);
  const DropGeom & G = M.G;
  const Layout & L = dom->lay[dom->depth];
  /* the mask (gfs_droplet_to_particle_event, :1368-1393) */
  const double * mask = nullptr;
  if (d->mask >= 0) {
    Field * F = get_field (dom, d->mask);
    if (!F) return GFSHIP_EINVAL;
    mask = F->lev[dom->depth];
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
  if ((r = drop_tags (M, W, nullptr, n, true, false))) return r;
  if ((r = drop_min (dom->stream, W, n, d->min, &umin))) return r;
  if (info) info->min = umin;
  const double * u[3];
  for (int a = 0; a < 3; a++)
    u[a] = a < dom->dim ? dom->fields[sv.u[a]].lev[dom->depth] : nullptr;
  const double * alpha = sv.alpha_cell >= 0 ? dom->fields[sv.alpha_cell].lev[dom->depth] : nullptr;
  if ((r = drop_convert (M, W, pl, n, umin, C->lev[dom->depth], u, alpha, info != nullptr))) return r;
  if ((r = drop_reset (dom, W, M, C, umin, d->reset))) return r;
  return info ? drop_info (dom->stream, W, info) : GFSHIP_OK;
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
