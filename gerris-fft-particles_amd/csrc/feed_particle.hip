// feed_particle.hip -- particles join a list during a run: GfsFeedParticle (modules/particulatecommon.c:2375-2647)
// on a list of particulates of a uniform box or of a refined tree, and idlast of a GfsParticleList.
//
// The event of the reference (gfs_feed_particle_event, :2404-2418) calls feed_particulate (:2377-2402) once per
// candidate: the position from three functions without a cell, gfs_domain_locate (no cell: the candidate is
// dropped), the velocity of the fluid interpolated there, the mass and the volume from two functions at the cell,
// then add_particulate (:1237-1276): nothing below a mass of 1.e-20, else a new object at the END of the list
// with id = ++idlast.  The positions are the host's business (functions with state, evaluated in order); what
// follows is independent per candidate except for the id, which counts the accepted candidates before it.  Here:
//   1. one thread per candidate: locate, interpolate, and the slot of a new object (feed_gather_kernel,
//      particles.hip, and tree_feed_gather_kernel, tree_particles.hip: the locate and the interpolate of the event
//      kernels of a box and of a tree; on a tree the cell is the leaf, whatever its level);
//   2. the two functions of every candidate with a cell: a constant, or the kernel hipRTC compiled around the
//      text (rtc.hip: at the cell of a box, or at the leaf of a tree), written straight into the mass and the
//      volume of the new slots;
//   3. the ids, an ordered prefix count of the accept flags in three passes: per block of 256 candidates the
//      number accepted (ballot and popcount per wave, the waves added in LDS), one block scans those counts and
//      moves idlast, then every candidate takes idlast + 1 + (accepted before it) and its flag; an accepted one
//      also gets its diameter (:552) and rb (:2091).  No atomic counter: the ids do not depend on the scheduling
//      nor on the shape of the launch.  launch_feed_ids is these three passes, for a box and for a tree alike.
// The passes are issued by feed_event_body (particle_events.hpp), once for the lists of a box (here, on BoxMesh) and of
// a tree (tree_feed_event, tree_particles.hip); the two create entries share feed_create below.
// Slots: the np candidates take the np slots after those in use, in candidate order; a refused candidate is a
// dead slot (alive = 0), which every reader of the list already skips.  The download order (creation slots) is
// therefore the reference's list order.  idlast lives on the device; only its getter reads it back.
//
// pow: the diameter and rb of a new particle are values of the device's pow in the reference's expressions, as
// after a volume event (particulate_sources.hip); everything else is the reference's arithmetic.
#include "particle_events.hpp"
#include "tree_particles.hpp"
#include <cstdlib>
#include <vector>

namespace gfship {

constexpr int FEED_BLOCK = 256, FEED_WAVES = FEED_BLOCK/64;

// add_particulate, :1244: `if (mass < 1.e-20) return;' -- a NaN passes, as in C
__device__ __forceinline__ bool feed_accept (int i, int np, const unsigned * __restrict__ cell,
					     const double * __restrict__ mass)
{
  return i < np && cell[i] != PSOURCE_NO_CELL && !(mass[i] < 1.e-20);
}

// pass 1 of the ids: accepted candidates per block
__global__ void __launch_bounds__(FEED_BLOCK)
feed_count_kernel (int np, const unsigned * __restrict__ cell, const double * __restrict__ mass,
		   unsigned * __restrict__ block)
{
  __shared__ unsigned wave[FEED_WAVES];
  const int i = blockIdx.x*FEED_BLOCK + threadIdx.x;
  const unsigned long long m = __ballot (feed_accept (i, np, cell, mass));
  if ((threadIdx.x & 63) == 0) wave[threadIdx.x >> 6] = (unsigned) __popcll (m);
  __syncthreads ();
  if (threadIdx.x == 0) {
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < FEED_WAVES; w++) s += wave[w];
    block[blockIdx.x] = s;
  }
}

// pass 2: one block turns the counts into the id before the first accepted candidate of every block (idlast +
// the accepted candidates of the blocks before it), FEED_BLOCK counts at a time, and moves idlast
__global__ void __launch_bounds__(FEED_BLOCK)
feed_scan_kernel (int nblocks, unsigned * __restrict__ block, unsigned * __restrict__ idlast)
{
  __shared__ unsigned wave[FEED_WAVES];
  __shared__ unsigned carry;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = *idlast;
  __syncthreads ();
  for (int b0 = 0; b0 < nblocks; b0 += FEED_BLOCK) {
    const int b = b0 + threadIdx.x;
    const unsigned v = b < nblocks ? block[b] : 0u;
    unsigned s = v;      /* inclusive scan of the wave */
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned up = __shfl_up (s, d, 64);
      if (lane >= d) s += up;
    }
    if (lane == 63) wave[w] = s;
    __syncthreads ();
    unsigned before = carry;
#pragma unroll
    for (int q = 0; q < FEED_WAVES; q++)
      if (q < w) before += wave[q];
    if (b < nblocks) block[b] = before + s - v;
    __syncthreads ();
    if (threadIdx.x == FEED_BLOCK - 1) carry = before + s;
    __syncthreads ();
  }
  if (threadIdx.x == 0) *idlast = carry;
}

// pass 3: id and flag of every candidate; diameter and rb of an accepted one (compute_drag_force, :552,
// distance_normalization, :2091), zeros for a refused one (its functions may not have been evaluated)
__global__ void __launch_bounds__(FEED_BLOCK)
feed_scatter_kernel (int np, const unsigned * __restrict__ cell, const unsigned * __restrict__ block,
		     double * __restrict__ mass, double * __restrict__ volume, double * __restrict__ dia,
		     double * __restrict__ rb, unsigned * __restrict__ id, unsigned char * __restrict__ alive)
{
  __shared__ unsigned wave[FEED_WAVES];
  const int i = blockIdx.x*FEED_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool ok = feed_accept (i, np, cell, mass);
  const unsigned long long m = __ballot (ok);
  if (lane == 0) wave[w] = (unsigned) __popcll (m);
  __syncthreads ();
  if (i >= np) return;
  unsigned before = block[blockIdx.x];
#pragma unroll
  for (int q = 0; q < FEED_WAVES; q++)
    if (q < w) before += wave[q];
  before += (unsigned) __popcll (m & ((1ull << lane) - 1ull));
  alive[i] = ok ? 1 : 0;
  if (ok) {
    const double v = volume[i];
    id[i] = before + 1u;
    dia[i] = 2.*pow (3.0*v/4.0/M_PI, 1./3.);
    rb[i] = pow (3.*v/(4.*M_PI), 1./3.);
  }
  else {
    id[i] = 0u;
    mass[i] = volume[i] = dia[i] = rb[i] = 0.;
  }
}

int launch_feed_ids (gfship_particles * pl, int base, int np, const unsigned * cell, unsigned * block)
{
  const int grid = (np + FEED_BLOCK - 1)/FEED_BLOCK;
  double * mass = pl->mass + base, * volume = pl->volume + base;
  hipLaunchKernelGGL (feed_count_kernel, dim3 (grid), dim3 (FEED_BLOCK), 0, pl->stream, np, cell, mass, block);
  hipLaunchKernelGGL (feed_scan_kernel, dim3 (1), dim3 (FEED_BLOCK), 0, pl->stream, grid, block, pl->d_idlast);
  hipLaunchKernelGGL (feed_scatter_kernel, dim3 (grid), dim3 (FEED_BLOCK), 0, pl->stream, np, cell, block,
		      mass, volume, pl->dia + base, pl->rb + base, pl->id + base, pl->alive + base);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

// what gfship_feed_particle_create and the event refuse: the refusals of a GfsSourceParticulateVol
// (source_check, particulate_sources.hip)
int feed_check (gfship_particles * pl, const char * what)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_LIST (pl, what);
  GFSHIP_CHECK (pl->particulate, GFSHIP_EUNSUPPORTED,
		"%s needs a list of particulates (gfship_particles_set_particulate): it sets the mass, the volume "
		"and the velocity of what it adds", what);
  GFSHIP_CHECK (!pl->dom->has_external, GFSHIP_EUNSUPPORTED,
		"%s on a box with GfsBoundaryMpi sides is not supported: the ids of the boxes are not numbered "
		"together (mpi_particle_numbering)", what);
  GFSHIP_CHECK (pl->dom->dim*pl->dom->depth < 32, GFSHIP_EUNSUPPORTED,
		"%s: the %d-D box of level %d has 2^32 cells or more", what, pl->dom->dim, pl->dom->depth);
  return GFSHIP_OK;
}

int feed_reserve (gfship_feed_particle * f, int np)
{
  if (f->cap >= np) return GFSHIP_OK;
  gfship_particles * pl = f->pl;
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  void ** a[] = { (void **) &f->cand, (void **) &f->cell, (void **) &f->block };
  f->cap = 0;
  for (void ** p : a) {
    if (*p) (void) hipFree (*p);
    *p = nullptr;
  }
  const size_t m = (size_t) np;
  GFSHIP_HIP (hipMalloc ((void **) &f->cand, 3*m*sizeof (double)));
  GFSHIP_HIP (hipMalloc ((void **) &f->cell, m*sizeof (unsigned)));
  GFSHIP_HIP (hipMalloc ((void **) &f->block, (m + FEED_BLOCK - 1)/FEED_BLOCK*sizeof (unsigned)));
  f->cap = np;
  return GFSHIP_OK;
}

// gfs_feed_particle_read (:2435-2575) once the entry has made its checks and those of its table of variables: each
// of the two functions is a constant, or compile (text, nf, names, &kernel) around the names of the table it uses
template <class Compile>
static int feed_create (gfship_feed_particle ** out, gfship_particles * pl, const char * mass, const char * volume,
			int nvars, const char * const * names, const int * vars, Compile compile)
{
  gfship_feed_particle * f = new gfship_feed_particle;
  f->pl = pl;
  const char * text[2] = { mass, volume };
  for (int w = 0; w < 2; w++) {
    if (!text[w] || text_constant (text[w], &f->value[w])) continue;
    const std::vector<const char *> named = named_variables (text[w], nvars, names, vars, f->read[w]);
    const int r = compile (text[w], (int) named.size (), named.data (), &f->fn[w]);
    if (r) {
      gfship_feed_particle_destroy (f);
      return r;
    }
  }
  *out = f;
  return GFSHIP_OK;
}

} // namespace gfship

using namespace gfship;

extern "C" {

int gfship_feed_particle_create (gfship_feed_particle ** out, gfship_particles * pl, const char * mass,
				 const char * volume, int nvars, const char * const * names,
				 const gfship_field * fields)
{
  GFSHIP_CHECK (out != nullptr, GFSHIP_EINVAL, "null output pointer");
  *out = nullptr;
  int r = feed_check (pl);
  if (r) return r;
  if ((r = feed_names_check (nvars, names, fields, "field"))) return r;
  gfship_domain * dom = pl->dom;
  for (int q = 0; q < nvars; q++)
    if (!get_field (dom, fields[q])) return GFSHIP_EINVAL;
  return feed_create (out, pl, mass, volume, nvars, names, fields,
		      [&] (const char * text, int nf, const char * const * named, RtcKernel ** k) -> int {
			return rtc_compile_cell (dom, text, nf, named, k);
		      });
}

int gfship_feed_particle_event (gfship_feed_particle * f, int np, const double * pos)
{
  GFSHIP_CHECK (f != nullptr, GFSHIP_EINVAL, "null GfsFeedParticle");
  GFSHIP_CHECK (np >= 0 && (np == 0 || pos), GFSHIP_EINVAL, "invalid argument");
  gfship_particles * pl = f->pl;
  if (pl && pl->tree) return tree_feed_event (f, np, pos);      /* a handle of gfship_tree_feed_particle_create */
  int r = feed_check (pl);
  if (r) return r;
  if (np == 0) return GFSHIP_OK;
  return feed_event_body (BoxMesh (pl), f, np, pos);
}

void gfship_feed_particle_destroy (gfship_feed_particle * f)
{
  if (!f) return;
  (void) hipStreamSynchronize (f->pl->stream);
  void * a[] = { f->cand, f->cell, f->block };
  for (void * p : a)
    if (p) (void) hipFree (p);
  rtc_free (f->fn[0]);
  rtc_free (f->fn[1]);
  delete f;
}

// idlast of a list, of a box or of a tree, on its stream
static int set_idlast (gfship_particles * pl, int idlast)
{
  GFSHIP_CHECK (idlast >= 0, GFSHIP_EINVAL, "idlast is a guint");
  const unsigned v = (unsigned) idlast;
  GFSHIP_HIP (hipMemcpyAsync (pl->d_idlast, &v, sizeof (unsigned), hipMemcpyHostToDevice, pl->stream));
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  return GFSHIP_OK;
}

static int get_idlast (gfship_particles * pl)
{
  unsigned v = 0;
  GFSHIP_HIP (hipMemcpyAsync (&v, pl->d_idlast, sizeof (unsigned), hipMemcpyDeviceToHost, pl->stream));
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  return (int) v;
}

int gfship_particles_set_idlast (gfship_particles * pl, int idlast)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_LIST (pl, "gfship_particles_set_idlast");
  return set_idlast (pl, idlast);
}

int gfship_particles_idlast (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_LIST (pl, "gfship_particles_idlast");
  return get_idlast (pl);
}

// gfs_feed_particle_read (:2435-2575) on a list made by gfship_particulates_create_tree: the table names variables
// of the tree, read at the leaf, and the texts are compiled for the device of the tree
int gfship_tree_feed_particle_create (gfship_feed_particle ** out, gfship_particles * pl, const char * mass,
				      const char * volume, int nvars, const char * const * names, const int * vars)
{
  GFSHIP_CHECK (out != nullptr, GFSHIP_EINVAL, "null output pointer");
  *out = nullptr;
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_tree_feed_particle_create");
  int r = feed_names_check (nvars, names, vars, "variable of the tree");
  if (r) return r;
  for (int q = 0; q < nvars; q++)
    GFSHIP_CHECK (tree_feed_variable (pl, vars[q]), GFSHIP_EINVAL,
		  "`%s': the tree has no variable %d", names[q], vars[q]);
  const int device = tree_device (pl->tree);
  GFSHIP_HIP (hipSetDevice (device));
  return feed_create (out, pl, mass, volume, nvars, names, vars,
		      [&] (const char * text, int nf, const char * const * named, RtcKernel ** k) -> int {
			return rtc_compile_tree_cell (device, pl->dim, text, nf, named, k);
		      });
}

int gfship_tree_particles_set_idlast (gfship_particles * pl, int idlast)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_CHECK (pl->tree != nullptr, GFSHIP_EUNSUPPORTED,
		"gfship_tree_particles_set_idlast: a list of a box (gfship_particles_set_idlast)");
  GFSHIP_HIP (hipSetDevice (tree_device (pl->tree)));
  return set_idlast (pl, idlast);
}

int gfship_tree_particles_idlast (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_CHECK (pl->tree != nullptr, GFSHIP_EUNSUPPORTED,
		"gfship_tree_particles_idlast: a list of a box (gfship_particles_idlast)");
  GFSHIP_HIP (hipSetDevice (tree_device (pl->tree)));
  return get_idlast (pl);
}

} // extern "C"
