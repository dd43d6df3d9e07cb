// particulate_sources.hip -- the particles themselves change: GfsSourceParticulateVol and
// GfsSourceParticulateMass (modules/particulatecommon.c:2734-3047) on a uniform box.
//
// The event of the reference resets the deposit variable and walks the list in its order (update_vol,
// :2806-2832; update_mass, :2964-2991): locate the cell, write Rad and Urelp, Vrelp(, Wrelp) of the particle
// into it, evaluate the GfsFunction at the cell, volume (mass) += source*dt, deposit[cell] += source.  The
// function is evaluated right after the particle wrote its own four values, so what it sees depends on the
// particle alone and on fields nobody writes during the walk: the work per particle is independent.  What
// does depend on the order is what a cell is left with: the sum of the sources of its particles, added from 0
// in list order, and the four values of its LAST particle in list order.  Here:
//   1. one thread per particle: locate, radius, relative velocity (particulate_source_gather_kernel,
//      particles.hip: the locate and the interpolate of the event kernels), stored per creation slot;
//   2. the function of every particle: a constant, or the kernel hipRTC compiled around its text (rtc.hip);
//   3. one thread per creation slot: volume or mass += source*dt, for a volume also the diameter (:552) and rb
//      (:2091) of the particle, and the key (cell << 32 | creation slot);
//   4. where a field is to be written: radix sort of the keys (the arrays and the key bits of coupling.hip),
//      then one thread per run of equal cells adds the sources serially and copies the values of the last
//      record (particulate_source_cell_kernel, cell_sums.hpp, shared with the lists of a tree).  No atomics: the
//      result does not depend on where a particle is stored nor on the scheduling.
// The event has no chunks: one record of 8 bytes per particle (the spreading needs chunks because one particle
// owns many records).
// The passes are issued by source_event_body (particle_events.hpp), for a box here and for a tree in
// tree_particles.hip; an entry finds and resets the variables it writes, each mesh by its own rule.
//
// pow: Rad, and the diameter and rb of a particle whose volume an event has changed, are values of the
// device's pow (the reference's expression, glibc's pow there); everything else is the reference's arithmetic,
// operation by operation.  A list no volume event has run on keeps the diameter and rb computed on the host
// (particulate_alloc).
#include "particle_events.hpp"
#include "tree_particles.hpp"
#include <cmath>
#include <cstdlib>
#include <vector>

namespace gfship {

// step 3: :2828 / :2986, then the diameter of compute_drag_force (:552) and rb of distance_normalization (:2091)
template <bool VOLUME>
__global__ void __launch_bounds__(256)
particulate_source_update_kernel (int n, const unsigned * __restrict__ cell, const double * __restrict__ src,
				  double dt, double * __restrict__ state, double * __restrict__ dia,
				  double * __restrict__ rb, unsigned long long pad, unsigned long long * __restrict__ key)
{
  int o = blockIdx.x*blockDim.x + threadIdx.x;
  if (o >= n) return;
  const unsigned c = cell[o];
  if (c == PSOURCE_NO_CELL) {      /* not on the list, or no cell: nothing changes */
    if (key) key[o] = pad << 32 | (unsigned) o;
    return;
  }
  const double s = state[o] + src[o]*dt;
  state[o] = s;
  if constexpr (VOLUME) {
    dia[o] = 2.*pow (3.0*s/4.0/M_PI, 1./3.);
    rb[o] = pow (3.*s/(4.*M_PI), 1./3.);
  }
  if (key) key[o] = (unsigned long long) c << 32 | (unsigned) o;
}

// what gfship_particulate_source_create and the event refuse: coupling_check of coupling.hip, word for word
static int source_check (gfship_particles * pl, const char * what)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_LIST (pl, what);
  GFSHIP_CHECK (pl->particulate, GFSHIP_EUNSUPPORTED,
		"%s needs a list of particulates (gfship_particles_set_particulate)", what);
  GFSHIP_CHECK (!pl->dom->has_external, GFSHIP_EUNSUPPORTED,
		"%s on a box with GfsBoundaryMpi sides is not supported: particles would arrive and leave "
		"between the events of the list", what);
  /* the keys hold the cell number and the pad (= the number of cells) in 32 bits */
  GFSHIP_CHECK (pl->dom->dim*pl->dom->depth < 32, GFSHIP_EUNSUPPORTED,
		"%s: the %d-D box of level %d has 2^32 cells or more", what, pl->dom->dim, pl->dom->depth);
  return GFSHIP_OK;
}

static const char * kind_name (int kind)
{
  return kind == GFSHIP_PARTICULATE_SOURCE_VOLUME ? "GfsSourceParticulateVol" : "GfsSourceParticulateMass";
}

int particulate_source_reserve (gfship_particulate_source * s)
{
  gfship_particles * pl = s->pl;
  if (s->cap >= pl->n) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  void ** a[] = { (void **) &s->cell, (void **) &s->prad, (void **) &s->purel[0], (void **) &s->purel[1],
		  (void **) &s->purel[2], (void **) &s->src };
  s->cap = 0;
  for (void ** p : a) {
    if (*p) (void) hipFree (*p);
    *p = nullptr;
    GFSHIP_HIP (hipMalloc (p, (size_t) pl->cap*(p == (void **) &s->cell ? sizeof (unsigned) : sizeof (double))));
  }
  s->cap = pl->cap;
  return GFSHIP_OK;
}

int launch_particulate_source_update (gfship_particulate_source * s, hipStream_t stream, double dt,
				      unsigned long long pad, unsigned long long * key)
{
  gfship_particles * pl = s->pl;
  const int n = pl->n, block = 256, grid = (n + block - 1)/block;
  if (s->kind == GFSHIP_PARTICULATE_SOURCE_VOLUME)
    hipLaunchKernelGGL (particulate_source_update_kernel<true>, dim3 (grid), dim3 (block), 0, stream, n,
			s->cell, s->src, dt, pl->volume, pl->dia, pl->rb, pad, key);
  else
    hipLaunchKernelGGL (particulate_source_update_kernel<false>, dim3 (grid), dim3 (block), 0, stream, n,
			s->cell, s->src, dt, pl->mass, nullptr, nullptr, pad, key);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

static int source_event (gfship_particulate_source * s, double * info)
{
  GFSHIP_CHECK (s != nullptr, GFSHIP_EINVAL, "null particulate source");
  gfship_particles * pl = s->pl;
  if (pl->tree)      /* the handle knows what made it */
    return tree_particulate_source_event (s, info);
  const char * what = kind_name (s->kind);
  int r = source_check (pl, what);
  if (r) return r;
  gfship_domain * dom = pl->dom;
  const bool volume = s->kind == GFSHIP_PARTICULATE_SOURCE_VOLUME;
  const BoxMesh M (pl);
  Field * D = nullptr, * R = nullptr, * U[3] = { nullptr, nullptr, nullptr };
  if (s->deposit >= 0 && !(D = get_field (dom, s->deposit))) return GFSHIP_EINVAL;
  if (s->rad >= 0 && !(R = get_field (dom, s->rad))) return GFSHIP_EINVAL;
  for (int c = 0; c < dom->dim; c++)
    if (s->urel[c] >= 0 && !(U[c] = get_field (dom, s->urel[c]))) return GFSHIP_EINVAL;
  std::vector<const double *> read;
  if ((r = M.arrays (s->read, read))) return r;
  const bool fields = D || R || U[0] || U[1] || U[2];
  if (fields && (r = before_write (dom))) return r;
  if (D) {
    /* gfs_cell_reset of the deposit: on every cell for a volume (FTT_TRAVERSE_ALL, :2844), on the leaves for a
       mass (:3004) */
    for (int l = volume ? 0 : dom->depth; l <= dom->depth; l++) {
      GFSHIP_HIP (hipMemsetAsync (D->lev[l], 0, dom->lay[l].total*sizeof (double), dom->stream));
      D->zero[l] = l < dom->depth;
    }
  }
  if (R) R->zero[dom->depth] = false;
  double * Ua[3] = { nullptr, nullptr, nullptr };
  for (int c = 0; c < dom->dim; c++)
    if (U[c]) {
      U[c]->zero[dom->depth] = false;
      Ua[c] = U[c]->lev[dom->depth];
    }
  return source_event_body (M, s, D ? D->lev[dom->depth] : nullptr, R ? R->lev[dom->depth] : nullptr, Ua, read, info);
}

// gfs_source_particulatevol_read / ...mass_read once the entry has made its checks: the table of variables (kind:
// what a name of the table stands for; extra: the caller's check of variable q), then the function -- a constant,
// or compile (text, nf, names, &kernel) around the names of the table the text uses
template <class Extra, class Compile>
static int source_create (gfship_particulate_source ** out, gfship_particles * pl, int kind, const char * function,
			  int nvars, const char * const * names, const int * vars, const char * var_kind, Extra extra,
			  Compile compile)
{
  int r = names_table_check (nvars, names, vars, { "Rad", "Urelp", "Vrelp", "Wrelp", "x", "y", "z", "t" }, var_kind,
			     extra);
  if (r) return r;
  RtcKernel * k = nullptr;
  double value = 0.;
  std::vector<gfship_field> read;
  /* a constant (gfs_function_read: a number is kept as f->val) needs no compilation */
  if (function && !text_constant (function, &value)) {
    const std::vector<const char *> named = named_variables (function, nvars, names, vars, read);
    if ((r = compile (function, (int) named.size (), named.data (), &k))) return r;
  }
  gfship_particulate_source * s = new gfship_particulate_source;
  s->pl = pl; s->kind = kind; s->fn = k; s->value = value; s->read = read;
  *out = s;
  return GFSHIP_OK;
}

} // namespace gfship

using namespace gfship;

extern "C" {

int gfship_particulate_source_create (gfship_particulate_source ** out, gfship_particles * pl, int kind,
				      const char * function, int nvars, const char * const * names,
				      const gfship_field * fields)
{
  GFSHIP_CHECK (out != nullptr, GFSHIP_EINVAL, "null output pointer");
  *out = nullptr;
  GFSHIP_CHECK (kind == GFSHIP_PARTICULATE_SOURCE_VOLUME || kind == GFSHIP_PARTICULATE_SOURCE_MASS, GFSHIP_EINVAL,
		"kind must be GFSHIP_PARTICULATE_SOURCE_VOLUME or GFSHIP_PARTICULATE_SOURCE_MASS");
  int r = source_check (pl, kind_name (kind));
  if (r) return r;
  gfship_domain * dom = pl->dom;
  return source_create (out, pl, kind, function, nvars, names, fields, "field",
			[&] (int q) -> int { return get_field (dom, fields[q]) ? GFSHIP_OK : GFSHIP_EINVAL; },
			[&] (const char * text, int nf, const char * const * named, RtcKernel ** k) -> int {
			  return rtc_compile_source (dom, text, nf, named, k);
			});
}

int gfship_tree_particulate_source_create (gfship_particulate_source ** out, gfship_particles * pl, int kind,
					   const char * function, int nvars, const char * const * names,
					   const int * vars)
{
  GFSHIP_CHECK (out != nullptr, GFSHIP_EINVAL, "null output pointer");
  *out = nullptr;
  GFSHIP_CHECK (kind == GFSHIP_PARTICULATE_SOURCE_VOLUME || kind == GFSHIP_PARTICULATE_SOURCE_MASS, GFSHIP_EINVAL,
		"kind must be GFSHIP_PARTICULATE_SOURCE_VOLUME or GFSHIP_PARTICULATE_SOURCE_MASS");
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_tree_particulate_source_create");
  auto written = [&] (int q) -> int {
    GFSHIP_CHECK (!(vars[q] >= GFSHIP_TREE_RAD && vars[q] <= GFSHIP_TREE_DMDT), GFSHIP_EUNSUPPORTED,
		  "%s: `%s' names a variable the walk of the list writes (Rad, Urelp, Vrelp, Wrelp or a deposit)",
		  kind_name (kind), names[q]);
    GFSHIP_CHECK (tree_has_variable (pl->tree, vars[q]), GFSHIP_EINVAL,
		  "`%s': the tree has no variable %d", names[q], vars[q]);
    return GFSHIP_OK;
  };
  return source_create (out, pl, kind, function, nvars, names, vars, "variable of the tree", written,
			[&] (const char * text, int nf, const char * const * named, RtcKernel ** k) -> int {
			  const int device = tree_device (pl->tree);
			  GFSHIP_HIP (hipSetDevice (device));
			  return rtc_compile_tree_source (device, pl->dim, text, nf, named, k);
			});
}

int gfship_tree_particulate_source_set_fields (gfship_particulate_source * s, int rad, const int urel[3], int deposit)
{
  GFSHIP_CHECK (s != nullptr, GFSHIP_EINVAL, "null particulate source");
  GFSHIP_CHECK (s->pl->tree != nullptr, GFSHIP_EUNSUPPORTED,
		"gfship_tree_particulate_source_set_fields: the source of a list of a box "
		"(gfship_particulate_source_set_fields)");
  const int dim = s->pl->dim;
  const int w[5] = { rad, urel ? urel[0] : -1, urel ? urel[1] : -1, urel ? urel[2] : -1, deposit };
  const int designated[5] = { GFSHIP_TREE_RAD, GFSHIP_TREE_URELP, GFSHIP_TREE_VRELP, GFSHIP_TREE_WRELP,
			      s->kind == GFSHIP_PARTICULATE_SOURCE_VOLUME ? GFSHIP_TREE_VOLSRC : GFSHIP_TREE_DMDT };
  static const char * name[5] = { "rad", "urel[0]", "urel[1]", "urel[2]", "deposit" };
  for (int q = 0; q < 5; q++)
    GFSHIP_CHECK (w[q] < 0 || w[q] == designated[q], GFSHIP_EINVAL,
		  "%s: %s is variable %d of a tree, or -1", kind_name (s->kind), name[q], designated[q]);
  GFSHIP_CHECK (dim == 3 || w[3] < 0, GFSHIP_EINVAL, "a quadtree has no GFSHIP_TREE_WRELP");
  /* an argument is allocated here, zeroed: the event finds it */
  for (int q = 0; q < 5; q++)
    if (w[q] >= 0) {
      int r = tree_source_variable (s->pl->tree, w[q], nullptr);
      if (r) return r;
    }
  s->rad = w[0] < 0 ? -1 : w[0];
  for (int c = 0; c < 3; c++) s->urel[c] = w[1 + c] < 0 ? -1 : w[1 + c];
  s->deposit = w[4] < 0 ? -1 : w[4];
  return GFSHIP_OK;
}

int gfship_particulate_source_set_fields (gfship_particulate_source * s, gfship_field rad,
					  const gfship_field urel[3], gfship_field deposit)
{
  GFSHIP_CHECK (s != nullptr, GFSHIP_EINVAL, "null particulate source");
  GFSHIP_CHECK (s->pl->tree == nullptr, GFSHIP_EUNSUPPORTED,
		"gfship_particulate_source_set_fields: the source of a list of a tree takes the variables of the tree "
		"(gfship_tree_particulate_source_set_fields)");
  gfship_domain * dom = s->pl->dom;
  gfship_field w[5] = { rad, urel ? urel[0] : -1, urel ? urel[1] : -1, urel && dom->dim == 3 ? urel[2] : -1,
			deposit };
  for (int q = 0; q < 5; q++) {
    if (w[q] < 0) { w[q] = -1; continue; }
    if (!get_field (dom, w[q])) return GFSHIP_EINVAL;
    for (int p = 0; p < q; p++)
      GFSHIP_CHECK (w[p] != w[q], GFSHIP_EINVAL, "one field is given for two of Rad, Urelp, Vrelp, Wrelp and the deposit");
    for (gfship_field f : s->read) {
      /* the function would read a running sum that depends on the walk (:2830) */
      GFSHIP_CHECK (!(q == 4 && f == w[q]), GFSHIP_EUNSUPPORTED,
		    "%s: the function names the variable its sources are deposited into", kind_name (s->kind));
      GFSHIP_CHECK (f != w[q], GFSHIP_EINVAL,
		    "%s: the function reads a field under a name of its own that is also written as Rad, Urelp, "
		    "Vrelp or Wrelp", kind_name (s->kind));
    }
  }
  s->rad = w[0]; s->urel[0] = w[1]; s->urel[1] = w[2]; s->urel[2] = w[3]; s->deposit = w[4];
  return GFSHIP_OK;
}

int gfship_particulate_source_event (gfship_particulate_source * s)
{
  return source_event (s, nullptr);
}

int gfship_particulate_source_time_event (gfship_particulate_source * s, double info[2])
{
  GFSHIP_CHECK (info != nullptr, GFSHIP_EINVAL, "null argument");
  return source_event (s, info);
}

void gfship_particulate_source_destroy (gfship_particulate_source * s)
{
  if (!s) return;
  (void) hipStreamSynchronize (s->pl->stream);
  void * a[] = { s->cell, s->prad, s->purel[0], s->purel[1], s->purel[2], s->src };
  for (void * p : a)
    if (p) (void) hipFree (p);
  rtc_free (s->fn);
  delete s;
}

} // extern "C"
