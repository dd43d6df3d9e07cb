// coupling.hip -- the particles act on the fluid: GfsParticulateField and the event of
// GfsSourceParticulate (modules/particulatecommon.c:1927-2228) on a uniform box.
//
// Both are sums over the particles, cell by cell, in the order of the reference's particle list
// (the order of gfship_particles_download: the creation slot `orig'), and a sum of doubles depends
// on that order.  Neither may depend on where a particle is stored or on how threads are scheduled,
// so nothing here adds with atomics: every contribution becomes a record with the 64-bit key
// (cell << 32 | creation slot), the records are radix-sorted by that key, and one thread per run of
// equal cells adds its records serially -- in list order, the reference's own sequence of
// additions.
//
//   void fraction (particulate_field_event, :1934-1957): one record per located particle.
//   spreading (source_particulate_event, :2208-2222), per chunk of particles in list order:
//     1. one thread per particle walks the reference's pruned pre-order descent (cond_kernel,
//        :2126-2156, through ftt_cell_traverse_condition, src/ftt.c:948-986) with an explicit
//        stack and writes, for every leaf it reaches and in that order, the key and the normalised
//        distance q of distance_normalization (:2089-2099);
//     2. the kernel function K (q) of every record (a constant, or the GfsFunction compiled by
//        rtc.hip);
//     3. one thread per particle adds volume and correction over its records in traversal order
//        (kernel_volume, :2108-2119) and divides (:2216);
//     4. sort by key, then the per-cell sums of diffuse_force (:2158-2175) in list order.
//   Chunks follow the list order, so the additions into one cell keep that order across chunks.
//   A particle owns `stride' record slots -- an upper bound of the leaves cond_kernel can pass, see
//   kernel_stride -- and a chunk holds at most RECORD_CAP slots: the work arrays take 56 bytes per
//   slot, 224 MiB at the most, whatever the number of particles.
// The sums of steps 3 and 4 and of the void fraction are the kernels of cell_sums.hpp on BoxCells; the lists of a
// tree (tree_particles.hip) launch the same kernels on TreeCells.  The host side of both events (the chunk loop, the
// sorts, the timing of `info') is particle_events.hpp, instantiated here on BoxMesh; this file keeps the checks of
// the entries of a box, the key and emit kernels with their launches and stride (BoxMesh::) and the work arrays.
#include "particle_events.hpp"
#include <cmath>
#include <cstdlib>

namespace gfship {

constexpr size_t RECORD_CAP = COUPLING_RECORD_CAP;
constexpr int DESCENT_MAXDEPTH = 15;

// record slots per particle.  A leaf passes cond_kernel if |centre - pos| - (h/2) sqrt (dim) <= rkernel or if
// it holds the particle; either way |centre[c] - pos[c]| <= rho = rkernel + (h/2) sqrt (dim) along every axis
// (the second case: <= h/2 < rho).  Centres are h apart, so at most floor (2 rho/h) + 1 of them lie in an
// interval of length 2 rho; one more for the rounding of the comparison, and never more than the box has.
// (a 64-bit count: the callers refuse a kernel whose slots do not fit into one chunk, see stride_check)
unsigned long long BoxMesh::kernel_stride (double rkernel) const
{
  const int n = L.n;
  const double h = 1./n;
  const double rho = rkernel + h/2.*sqrt ((double) dom->dim);
  double m = floor (2.*rho/h) + 2.;
  if (!(m < n)) m = n;
  const unsigned long long s = (unsigned long long) m;
  return dom->dim == 3 ? s*s*s : s*s;
}

// a particle's slots must fit into one chunk: that is what bounds the work arrays at 56 B x RECORD_CAP
int BoxMesh::stride_check (double rkernel) const
{
  const unsigned long long stride = kernel_stride (rkernel);
  GFSHIP_CHECK (stride <= RECORD_CAP, GFSHIP_EUNSUPPORTED,
		"GfsSourceParticulate: a kernel of rkernel = %g may reach %llu leaves of this box, more than "
		"the %llu records of a chunk", rkernel, stride, (unsigned long long) RECORD_CAP);
  return GFSHIP_OK;
}

// gfs_domain_cell_traverse_condition (src/domain.c:1550-1574), FTT_PRE_ORDER, FTT_TRAVERSE_LEAFS: the
// children n = 0 .. FTT_CELLS - 1 of a cell that passes, child n at x:+ (bit 0), y:- (bit 1), z:- (bit 2)
// (src/ftt.c:301-316), the order of every traversal of this library; visit (ix) for the leaves
template <int DIM, class Visit>
__device__ __forceinline__ void kernel_descent (int depth, const double p[3], double rkernel, Visit visit)
{
  int ix[3] = { 0, 0, 0 };
  if (!cond_kernel<DIM> (0, ix, p, rkernel))
    return;
  if (depth == 0) {
    visit (ix);
    return;
  }
  unsigned char next[DESCENT_MAXDEPTH + 1];     // next child to try, per level
  int l = 0;
  next[0] = 0;
  while (l >= 0) {
    if (next[l] == (1 << DIM)) {
      l--;
#pragma unroll
      for (int c = 0; c < DIM; c++) ix[c] >>= 1;
      continue;
    }
    const int n = next[l]++;
    int cx[3] = { 2*ix[0] + (n & 1), 2*ix[1] + ((n & 2) ? 0 : 1), DIM == 3 ? 2*ix[2] + ((n & 4) ? 0 : 1) : 0 };
    if (!cond_kernel<DIM> (l + 1, cx, p, rkernel))
      continue;
    if (l + 1 == depth)
      visit (cx);
    else {
      l++;
#pragma unroll
      for (int c = 0; c < DIM; c++) ix[c] = cx[c];
      next[l] = 0;
    }
  }
}

__global__ void __launch_bounds__(256)
where_kernel (int n, const unsigned * __restrict__ orig, unsigned * __restrict__ where)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q < n) where[orig[q]] = (unsigned) q;
}

// key of the cell that holds each particle, (cell << 32 | creation slot); pad (cell = number of cells) for
// the particles that are off the list or have no cell (:1949-1950)
// (tree_field_keys_kernel, tree_particles.hip, is this kernel on the leaves of a tree)
template <int DIM>
__global__ void __launch_bounds__(256)
field_keys_kernel (int nside, int depth, int n, const double * __restrict__ x, const double * __restrict__ y,
		   const double * __restrict__ z, const unsigned char * __restrict__ alive,
		   const unsigned * __restrict__ orig, unsigned long long pad, unsigned long long * __restrict__ key)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= n) return;
  unsigned long long k = pad;
  if (alive[q] == 1) {
    double p[3] = { x[q], y[q], DIM == 3 ? z[q] : 0. };
    int c[3];
    if (locate<DIM> (depth, p, c))
      k = (unsigned long long) (c[0] - 1) + (unsigned long long) nside*((c[1] - 1) +
				(DIM == 3 ? (unsigned long long) nside*(c[2] - 1) : 0ull));
  }
  key[q] = k << 32 | orig[q];
}

struct SpreadArgs {
  Layout L;
  int depth, o0, nchunk, stride;
  double rkernel;
  const unsigned * where;
  const unsigned char * alive;
  const double * pos[3];
  const double * rb;
  unsigned long long pad;       // key of an unused slot: cell = number of cells
  unsigned long long * key;
  double * q[3];
  int * cnt, * flag;
};

// step 1: the leaves the kernel of each particle of the chunk reaches, in traversal order
template <int DIM>
__global__ void __launch_bounds__(256)
spread_emit_kernel (SpreadArgs A)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= A.nchunk) return;
  const unsigned o = (unsigned) (A.o0 + t);
  const unsigned s = A.where[o];
  const size_t base = (size_t) t*A.stride;
  int cnt = 0;
  if (A.alive[s] == 1) {
    const double p[3] = { A.pos[0][s], A.pos[1][s], DIM == 3 ? A.pos[2][s] : 0. };
    const double rb = A.rb[o];
    const double cellsize = 1./A.L.n;
    const unsigned n = (unsigned) A.L.n;
    kernel_descent<DIM> (A.depth, p, A.rkernel, [&] (const int ix[3]) {
      if (cnt < A.stride) {
	const unsigned long long cell = (unsigned) ix[0] + (unsigned long long) n*
	  ((unsigned) ix[1] + (DIM == 3 ? (unsigned long long) n*(unsigned) ix[2] : 0ull));
	A.key[base + cnt] = cell << 32 | o;
	// distance_normalization (:2089-2099).  In 3-D the line `pos1->z = 0.' comes before
	// `pos1->z = (pos1->z - pos2->z)/rb': z is (0. - pos.z)/rb, whatever the cell
	A.q[0][base + cnt] = (-0.5 + (ix[0] + 0.5)*cellsize - p[0])/rb;
	A.q[1][base + cnt] = (-0.5 + (ix[1] + 0.5)*cellsize - p[1])/rb;
	A.q[2][base + cnt] = DIM == 3 ? (0. - p[2])/rb : 0.;
      }
      cnt++;
    });
  }
  if (cnt > A.stride) {      /* cannot happen (kernel_stride); reported, never written */
    *A.flag = 1;
    cnt = A.stride;
  }
  A.cnt[t] = cnt;
  for (int j = cnt; j < A.stride; j++)
    A.key[base + j] = A.pad << 32 | 0xFFFFFFFFull;
}

// a constant GfsFunction: of the kernel of a GfsSourceParticulate, of a GfsSourceParticulateVol / ...Mass
__global__ void __launch_bounds__(256)
fill_kernel (long n, double value, double * __restrict__ out)
{
  long r = (long) blockIdx.x*blockDim.x + threadIdx.x;
  if (r < n) out[r] = value;
}

// source_particulate_value (:2029-2065): gfs_face_interpolated_value_generic of F on the positive face of
// the component (right, top, front) -- ((x1 - 0.5)*v0 + 0.5*v1)/x1 with x1 = 1. between cells of one level
// (src/fluid.c:2186-2200); beyond a side v1 is what the ghost cell of F holds, and the reference's event
// applies no boundary condition to F: the caller's, like every field's.  First term of
// gfs_variable_mac_source (see mac_source_array, simulation.hip), the source of the diffusion second.
template <bool ADD>
__global__ void __launch_bounds__(256)
mac_source_fields_kernel (Layout L, long off, const double * __restrict__ F, double * __restrict__ out)
{
  const long q = (long) blockIdx.x*blockDim.x + threadIdx.x;
  const long n = L.n;
  if (q >= (L.dim == 3 ? n*n*n : n*n)) return;
  const int i = (int) (q % n) + 1, j = (int) ((q/n) % n) + 1, k = L.dim == 3 ? (int) (q/(n*n)) + 1 : 0;
  const long c = L.idx (i, j, k);
  const double x1 = 1.;
  double sum = 0.;
  sum += ((x1 - 0.5)*F[c] + 0.5*F[c + off])/x1;
  if (ADD) sum += out[c];
  out[c] = sum;
}

// add_sources (src/source.c:66-79): the centred value of the source fields (source_particulate_centered_value,
// :2067-2079), then the intensity of a GfsSource
__global__ void __launch_bounds__(256)
centered_source_fields_kernel (Layout L, double * __restrict__ v, const double * __restrict__ F, double gsrc,
			       double dt)
{
  const long q = (long) blockIdx.x*blockDim.x + threadIdx.x;
  const long n = L.n;
  if (q >= (L.dim == 3 ? n*n*n : n*n)) return;
  const int i = (int) (q % n) + 1, j = (int) ((q/n) % n) + 1, k = L.dim == 3 ? (int) (q/(n*n)) + 1 : 0;
  const long c = L.idx (i, j, k);
  double sum = 0;
  sum += F[c];
  if (gsrc != 0.) sum += gsrc;
  v[c] += dt*sum;
}

int launch_mac_source_fields (gfship_domain * dom, int c, const double * F, bool add_out, double * out)
{
  const Layout & L = dom->lay[dom->depth];
  const long off = c == 0 ? 1 : c == 1 ? L.sy : L.sz;
  const long nc = ncells (L);
  const dim3 grid ((unsigned) ((nc + 255)/256)), block (256);
  if (add_out)
    hipLaunchKernelGGL (mac_source_fields_kernel<true>, grid, block, 0, dom->stream, L, off, F, out);
  else
    hipLaunchKernelGGL (mac_source_fields_kernel<false>, grid, block, 0, dom->stream, L, off, F, out);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

int launch_centered_source_fields (gfship_domain * dom, double * v, const double * F, double gsrc, double dt)
{
  const Layout & L = dom->lay[dom->depth];
  const long nc = ncells (L);
  hipLaunchKernelGGL (centered_source_fields_kernel, dim3 ((unsigned) ((nc + 255)/256)), dim3 (256), 0,
		      dom->stream, L, v, F, gsrc, dt);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

void coupling_free (gfship_particles * pl)
{
  void * a[] = { pl->where, pl->ckey, pl->ckey2, pl->cq[0], pl->cq[1], pl->cq[2], pl->cval, pl->cval2,
		 pl->ccorr, pl->ccnt, pl->cflag };
  for (void * p : a)
    if (p) (void) hipFree (p);
  rtc_free (pl->kernel_fn);
  pl->kernel_fn = nullptr;
}

// the work arrays.  The void fraction needs the two key arrays alone (spreading = false: 16 B per particle);
// the spreading also q, K, the per-particle arrays of a chunk and the slot map of the list
int coupling_reserve (gfship_particles * pl, size_t nrec, size_t npart, bool spreading)
{
  auto fresh = [] (void ** a, size_t bytes) -> hipError_t {
    if (*a) (void) hipFree (*a);
    *a = nullptr;
    return hipMalloc (a, bytes);
  };
  if (nrec > pl->ckey_cap) {
    GFSHIP_HIP (hipStreamSynchronize (pl->stream));
    pl->ckey_cap = 0;
    GFSHIP_HIP (fresh ((void **) &pl->ckey, nrec*sizeof (unsigned long long)));
    GFSHIP_HIP (fresh ((void **) &pl->ckey2, nrec*sizeof (unsigned long long)));
    pl->ckey_cap = nrec;
  }
  if (!spreading)
    return GFSHIP_OK;
  if (pl->where_cap < pl->cap) {
    GFSHIP_HIP (fresh ((void **) &pl->where, (size_t) pl->cap*sizeof (unsigned)));
    pl->where_cap = pl->cap;
  }
  if (nrec > pl->crec_cap) {
    GFSHIP_HIP (hipStreamSynchronize (pl->stream));
    pl->crec_cap = 0;
    for (int c = 0; c < 3; c++)
      GFSHIP_HIP (fresh ((void **) &pl->cq[c], nrec*sizeof (double)));
    GFSHIP_HIP (fresh ((void **) &pl->cval, nrec*sizeof (double)));
    GFSHIP_HIP (fresh ((void **) &pl->cval2, nrec*sizeof (double)));
    pl->crec_cap = nrec;
  }
  if (npart > pl->cpart_cap) {
    GFSHIP_HIP (hipStreamSynchronize (pl->stream));
    pl->cpart_cap = 0;
    GFSHIP_HIP (fresh ((void **) &pl->ccorr, npart*sizeof (double)));
    GFSHIP_HIP (fresh ((void **) &pl->ccnt, npart*sizeof (int)));
    pl->cpart_cap = npart;
  }
  if (!pl->cflag)
    GFSHIP_HIP (hipMalloc ((void **) &pl->cflag, sizeof (int)));
  return GFSHIP_OK;
}

int coupling_sort_reserve (gfship_particles * pl, size_t need)
{
  if (need > pl->sort_tmp_bytes) {
    GFSHIP_HIP (hipStreamSynchronize (pl->stream));
    if (pl->sort_tmp) GFSHIP_HIP (hipFree (pl->sort_tmp));
    pl->sort_tmp = nullptr;
    pl->sort_tmp_bytes = 0;
    GFSHIP_HIP (hipMalloc (&pl->sort_tmp, need));
    pl->sort_tmp_bytes = need;
  }
  return GFSHIP_OK;
}

// bits of the keys: 32 of the creation slot, then those of the cell numbers 0 .. ncell (ncell = pad), which
// coupling_check keeps below 2^32
int coupling_key_bits (unsigned long long ncell)
{
  int b = 0;
  while (b < 32 && (ncell >> b)) b++;
  return 32 + b;
}

// what both classes refuse
static int coupling_check (gfship_particles * pl, const char * what)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_LIST (pl, what);
  GFSHIP_CHECK (pl->particulate, GFSHIP_EUNSUPPORTED,
		"%s needs a list of particulates (gfship_particles_set_particulate)", what);
  GFSHIP_CHECK (!pl->dom->has_external, GFSHIP_EUNSUPPORTED,
		"%s on a box with GfsBoundaryMpi sides is not supported: the particles next to such a side "
		"would have to reach into the neighbouring box", what);
  GFSHIP_CHECK (pl->dom->depth <= DESCENT_MAXDEPTH, GFSHIP_EUNSUPPORTED, "%s: more than %d levels", what,
		DESCENT_MAXDEPTH);
  /* the keys hold the cell number and the pad (= the number of cells) in 32 bits */
  GFSHIP_CHECK (pl->dom->dim*pl->dom->depth < 32, GFSHIP_EUNSUPPORTED,
		"%s: the %d-D box of level %d has 2^32 cells or more", what, pl->dom->dim, pl->dom->depth);
  return GFSHIP_OK;
}

int launch_where (gfship_particles * pl)
{
  const int block = 256;
  hipLaunchKernelGGL (where_kernel, dim3 ((pl->n + block - 1)/block), dim3 (block), 0, pl->stream, pl->n, pl->orig,
		      pl->where);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

int BoxMesh::field_keys (unsigned long long * key) const
{
  const int block = 256, grid = (pl->n + block - 1)/block;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (field_keys_kernel<DIM>, dim3 (grid), dim3 (block), 0, stream, L.n, dom->depth, pl->n,
			pl->pos[0], pl->pos[1], pl->pos[2], pl->alive, pl->orig, ncell, key);
  }, dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

int BoxMesh::spread_emit (int o0, int nchunk, int stride) const
{
  SpreadArgs A;
  A.L = L; A.depth = dom->depth; A.o0 = o0; A.nchunk = nchunk; A.stride = stride; A.rkernel = pl->rkernel;
  A.where = pl->where; A.alive = pl->alive; A.rb = pl->rb;
  for (int c = 0; c < 3; c++) { A.pos[c] = pl->pos[c]; A.q[c] = pl->cq[c]; }
  A.pad = ncell; A.key = pl->ckey; A.cnt = pl->ccnt; A.flag = pl->cflag;
  const int block = 256;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (spread_emit_kernel<DIM>, dim3 ((nchunk + block - 1)/block), dim3 (block), 0, stream, A);
  }, dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

int launch_fill (hipStream_t stream, long n, double value, double * out)
{
  const int block = 256;
  hipLaunchKernelGGL (fill_kernel, dim3 ((unsigned) ((n + block - 1)/block)), dim3 (block), 0, stream, n, value, out);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

} // namespace gfship

using namespace gfship;

extern "C" {

int gfship_particulate_field (gfship_particles * pl, gfship_field v)
{
  int r = coupling_check (pl, "GfsParticulateField");
  if (r) return r;
  gfship_domain * dom = pl->dom;
  Field * V = get_field (dom, v);
  GFSHIP_CHECK (V != nullptr, GFSHIP_EINVAL, "v is not a field of the domain");
  if ((r = before_write (dom))) return r;
  const BoxMesh M (pl);
  /* gfs_cell_reset on the leaves (:1944-1945) */
  if ((r = M.reset_leaves (V))) return r;
  return particulate_field_body (M, pl, V->lev[dom->depth]);
}

int gfship_particles_set_kernel (gfship_particles * pl, double rkernel, const char * function)
{
  int r = coupling_check (pl, "GfsSourceParticulate");
  if (r) return r;
  return set_kernel_body (BoxMesh (pl), pl, rkernel, function);
}

} // extern "C"

static int spread_forces (gfship_particles * pl, const gfship_field F[3], double * info)
{
  int r = coupling_check (pl, "GfsSourceParticulate");
  if (r) return r;
  GFSHIP_CHECK (F != nullptr, GFSHIP_EINVAL, "null argument");
  gfship_domain * dom = pl->dom;
  if ((r = particulate_fluid_check (gfship_sim_view_get (pl->sim)))) return r;
  double * Fa[3] = { nullptr, nullptr, nullptr };
  for (int c = 0; c < dom->dim; c++) {
    Field * Fc = get_field (dom, F[c]);
    GFSHIP_CHECK (Fc != nullptr, GFSHIP_EINVAL, "F[%d] is not a field of the domain", c);
    for (int c2 = 0; c2 < c; c2++)
      GFSHIP_CHECK (F[c2] != F[c], GFSHIP_EINVAL, "F[%d] and F[%d] are the same field", c2, c);
    Fa[c] = Fc->lev[dom->depth];
  }
  if ((r = before_write (dom))) return r;
  const BoxMesh M (pl);
  /* gfs_cell_reset on the leaves (:2189-2191) */
  for (int c = 0; c < dom->dim; c++)
    if ((r = M.reset_leaves (get_field (dom, F[c])))) return r;
  return spread_forces_body (M, pl, Fa, info);
}

extern "C" {

int gfship_particles_spread_forces (gfship_particles * pl, const gfship_field F[3])
{
  return spread_forces (pl, F, nullptr);
}

int gfship_particles_time_spreading (gfship_particles * pl, const gfship_field F[3], double info[5])
{
  GFSHIP_CHECK (info != nullptr, GFSHIP_EINVAL, "null argument");
  return spread_forces (pl, F, info);
}

int gfship_source_particulate_event (gfship_particles * pl, const gfship_field F[3])
{
  int r = gfship_particles_forces_on_fluid (pl);
  if (r) return r;
  return gfship_particles_spread_forces (pl, F);
}

} // extern "C"
