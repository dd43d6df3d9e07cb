// particle_events.hpp -- the host side of the events of a list of particulates, written once for the lists of a
// uniform box and of a refined tree: the void fraction and the spreading of coupling.hip, the event of
// particulate_sources.hip, the event of feed_particle.hip, and what their objects do with the text of a function.
//
// A body is a template over `the mesh the list lives on': BoxMesh (below) or TreeMesh (tree_particles.hip, next to
// the tables of the sampler its kernels read).  Both offer, under the same names,
//   dim, stream, t, dt, ncell (the pad of the keys), cells<DIM> () (BoxCells / TreeCells of cell_sums.hpp), TREE;
//   kernel_stride, stride_check: the record slots of a particle for an rkernel, and the refusal;
//   field_keys, spread_emit, source_gather, feed_gather: the launches that keep one kernel body per mesh;
//   compile_spatial, launch_source, launch_cell: the compiled functions (rtc.hip);
//   arrays: the device arrays of the variables a function reads.
// The ABI entries stay apart: each does its own checks, finds and resets its variables, then calls the body, which is
// instantiated in the object that holds its kernels (BoxCells: coupling.hip, particulate_sources.hip; TreeCells:
// tree_particles.hip).
#pragma once
#include "particles.hpp"
#include "cell_sums.hpp"
#include "function_text.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <vector>

namespace gfship {

// the table of variables of an object that takes the text of a function (function_text.hpp), with the messages.
// extra (q): what the caller asks of variable q besides, in the order of the table (0, or the code it has reported)
template <class Extra>
int names_table_check (int nvars, const char * const * names, const void * vars,
		       std::initializer_list<const char *> builtin, const char * kind, Extra extra)
{
  const TableFault f = table_fault (nvars, names, vars, builtin.begin (), (int) builtin.size ());
  GFSHIP_CHECK (f.rule != TABLE_INVALID, GFSHIP_EINVAL, "invalid table of variables");
  for (int q = 0, r; q < f.q; q++)
    if ((r = extra (q))) return r;
  GFSHIP_CHECK (f.rule != TABLE_NO_C_NAME, GFSHIP_EINVAL, "variable %d of the table has no C name", f.q);
  GFSHIP_CHECK (f.rule != TABLE_BUILTIN, GFSHIP_EINVAL,
		"`%s' is a variable of the function itself: it cannot name a %s", f.name, kind);
  GFSHIP_CHECK (f.rule != TABLE_TWICE, GFSHIP_EINVAL, "`%s' is in the table twice", f.name);
  return GFSHIP_OK;
}

// the table of a GfsFeedParticle (and of a GfsDropletToParticle): a function of the cell sees x, y, z, t
inline int feed_names_check (int nvars, const char * const * names, const void * vars, const char * kind)
{
  return names_table_check (nvars, names, vars, { "x", "y", "z", "t" }, kind, [] (int) { return GFSHIP_OK; });
}

// the names of the table the text uses, in the order of the table: the arguments of the compiled function; their
// variables go to `read'
inline std::vector<const char *> named_variables (const char * text, int nvars, const char * const * names,
						  const int * vars, std::vector<gfship_field> & read)
{
  std::vector<const char *> named;
  for (int q = 0; q < nvars; q++)
    if (names_identifier (text, names[q])) {
      named.push_back (names[q]);
      read.push_back (vars[q]);
    }
  return named;
}

// radix sort of the n keys ckey -> ckey2 of a list of the mesh M (its stream, the bits of its cell numbers), or of
// the pairs (ckey, cval) -> (ckey2, cval2): the size query, the temporary storage of the list, the sort.
// (templates: the kernels of the sort belong to the objects that instantiate a body, and to no other)
template <class Sort>
int coupling_sort (gfship_particles * pl, Sort sort)
{
  size_t need = 0;
  GFSHIP_HIP (sort (nullptr, need));
  int r = coupling_sort_reserve (pl, need);
  if (r) return r;
  size_t tmp_bytes = pl->sort_tmp_bytes;
  GFSHIP_HIP (sort (pl->sort_tmp, tmp_bytes));
  return GFSHIP_OK;
}
template <class Mesh>
int coupling_sort_keys (const Mesh & M, gfship_particles * pl, int n)
{
  const int bits = coupling_key_bits (M.ncell);
  return coupling_sort (pl, [&] (void * tmp, size_t & bytes) {
    return hipcub::DeviceRadixSort::SortKeys (tmp, bytes, pl->ckey, pl->ckey2, n, 0, bits, M.stream);
  });
}
template <class Mesh>
int coupling_sort_pairs (const Mesh & M, gfship_particles * pl, long nrec)
{
  const int bits = coupling_key_bits (M.ncell);
  return coupling_sort (pl, [&] (void * tmp, size_t & bytes) {
    return hipcub::DeviceRadixSort::SortPairs (tmp, bytes, pl->ckey, pl->ckey2, pl->cval, pl->cval2, nrec, 0, bits,
					       M.stream);
  });
}

// the timing an entry with an `info' argument reports: events recorded on the stream, the milliseconds between two
// of them once the stream has been waited for.  Off (info == nullptr): nothing is created or recorded
struct StreamTimer {
  hipStream_t stream;
  bool on;
  std::vector<hipEvent_t> ev;
  StreamTimer (hipStream_t s, bool on_) : stream (s), on (on_) {}
  StreamTimer (const StreamTimer &) = delete;
  ~StreamTimer () { for (hipEvent_t e : ev) (void) hipEventDestroy (e); }
  hipError_t mark () {
    if (!on) return hipSuccess;
    hipEvent_t e;
    hipError_t err = hipEventCreate (&e);
    if (err != hipSuccess) return err;
    ev.push_back (e);
    return hipEventRecord (e, stream);
  }
  double ms (size_t q) const {      // from mark q to mark q + 1
    float a = 0.f;
    (void) hipEventElapsedTime (&a, ev[q], ev[q + 1]);
    return a;
  }
};

// the leaves of a uniform box as the mesh of a list
struct BoxMesh {
  static constexpr bool TREE = false;
  gfship_particles * pl;
  gfship_domain * dom;
  gfship_sim_view v;
  const Layout & L;
  int dim;
  hipStream_t stream;
  double t, dt;
  unsigned long long ncell;
  explicit BoxMesh (gfship_particles * p) :
    pl (p), dom (p->dom), v (gfship_sim_view_get (p->sim)), L (dom->lay[dom->depth]), dim (dom->dim),
    stream (dom->stream), t (gfship_sim_time (p->sim)), dt (v.dt), ncell ((unsigned long long) ncells (L)) {}
  template <int DIM> BoxCells<DIM> cells () const { return BoxCells<DIM> { L }; }
  const double * alpha () const { return v.alpha_cell >= 0 ? dom->fields[v.alpha_cell].lev[dom->depth] : nullptr; }
  // gfs_cell_reset on the leaves of a field
  int reset_leaves (Field * F) const {
    GFSHIP_HIP (hipMemsetAsync (F->lev[dom->depth], 0, L.total*sizeof (double), stream));
    F->zero[dom->depth] = false;
    return GFSHIP_OK;
  }
  int arrays (const std::vector<gfship_field> & vars, std::vector<const double *> & out, bool = false) const {
    for (gfship_field f : vars) {
      Field * F = get_field (dom, f);
      if (!F) return GFSHIP_EINVAL;
      out.push_back (F->lev[dom->depth]);
    }
    return GFSHIP_OK;
  }
  int compile_spatial (const char * text, RtcKernel ** k) const { return rtc_compile_spatial (dom, text, k); }
  int launch_source (const gfship_particulate_source * s, const std::vector<const double *> & read) const {
    return rtc_launch_source (s->fn, stream, pl->n, L, s->cell, s->prad, s->purel, t, (int) read.size (), read.data (),
			      s->src);
  }
  int launch_cell (RtcKernel * k, int np, const unsigned * cell, const std::vector<const double *> & read,
		   double * out) const {
    return rtc_launch_cell (k, stream, np, L, cell, t, (int) read.size (), read.data (), out);
  }
  // coupling.hip
  unsigned long long kernel_stride (double rkernel) const;
  int stride_check (double rkernel) const;
  int field_keys (unsigned long long * key) const;
  int spread_emit (int o0, int nchunk, int stride) const;
  // particles.hip, with the locate and the interpolate of the event kernels.  The first pass of a source: per
  // creation slot the cell of the particle (PSOURCE_NO_CELL off the list or without one), Rad and fluid velocity - vel
  int source_gather (gfship_particulate_source * s) const;
  // feed_particulate (:2377-2396) up to the two functions for np candidates (3 doubles each, device): slot base + i
  // gets the position, pos_old = 0, force = 0, orig = its number and the velocity of the fluid; cell[i] as above
  int feed_gather (int base, int np, const double * cand, unsigned * cell) const;
};

// GfsParticulateField (particulate_field_event, modules/particulatecommon.c:1934-1957) into the leaves `a', which
// the caller has reset: one record per located particle, sorted, summed per cell in list order
template <class Mesh>
int particulate_field_body (const Mesh & M, gfship_particles * pl, double * a)
{
  int r;
  if (pl->n == 0) return GFSHIP_OK;
  if ((r = coupling_reserve (pl, (size_t) pl->n, 0, false))) return r;
  if ((r = M.field_keys (pl->ckey))) return r;
  if ((r = coupling_sort_keys (M, pl, pl->n))) return r;
  const int block = 256, grid = (pl->n + block - 1)/block;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    auto C = M.template cells<DIM> ();
    hipLaunchKernelGGL ((field_sum_kernel<DIM, decltype (C)>), dim3 (grid), dim3 (block), 0,
			M.stream, C, pl->n, pl->ckey2, M.ncell, pl->volume, a);
  }, M.dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

// rkernel and kernel of a GfsSourceParticulate (source_particulate_read, :2271-2289)
template <class Mesh>
int set_kernel_body (const Mesh & M, gfship_particles * pl, double rkernel, const char * function)
{
  GFSHIP_CHECK (rkernel >= 0. && std::isfinite (rkernel), GFSHIP_EINVAL, "rkernel must be a length >= 0");
  int r = M.stride_check (rkernel);
  if (r) return r;
  RtcKernel * k = nullptr;
  double value = 0.;
  if (function && !text_constant (function, &value) && (r = M.compile_spatial (function, &k))) return r;
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  rtc_free (pl->kernel_fn);
  pl->kernel_fn = k;
  pl->kernel_value = value;
  pl->rkernel = rkernel;
  return GFSHIP_OK;
}

// source_particulate_event from the stored forces (:2208-2222) into the leaves Fa[0 .. dim - 1], which the caller
// has reset; the passes are those of the header of coupling.hip.
// info != nullptr: the milliseconds of pass 1 (emit, kernel function, corrections) and of pass 2 (sort, sums)
// summed over the chunks from events on the stream, the record slots per particle, the particles per chunk
// and the bytes of the work arrays
template <class Mesh>
int spread_forces_body (const Mesh & M, gfship_particles * pl, double * const Fa[3], double * info)
{
  int r;
  if (info) for (int q = 0; q < 5; q++) info[q] = 0.;
  if (pl->n == 0) return GFSHIP_OK;
  if ((r = M.stride_check (pl->rkernel))) return r;
  const int stride = (int) M.kernel_stride (pl->rkernel);
  const int per_chunk = (int) std::min ((size_t) pl->n, COUPLING_RECORD_CAP/(size_t) stride);
  if ((r = coupling_reserve (pl, (size_t) per_chunk*stride, (size_t) per_chunk, true))) return r;
  StreamTimer T (M.stream, info != nullptr);
  const int block = 256;
  if ((r = launch_where (pl))) return r;
  GFSHIP_HIP (hipMemsetAsync (pl->cflag, 0, sizeof (int), M.stream));
  const double * alpha = M.alpha ();
  for (int o0 = 0; o0 < pl->n; o0 += per_chunk) {
    const int nchunk = std::min (per_chunk, pl->n - o0);
    const long nrec = (long) nchunk*stride;
    const int pgrid = (nchunk + block - 1)/block;
    const unsigned rgrid = (unsigned) ((nrec + block - 1)/block);
    GFSHIP_HIP (T.mark ());
    if ((r = M.spread_emit (o0, nchunk, stride))) return r;
    if (pl->kernel_fn) {
      if ((r = rtc_launch_spatial (pl->kernel_fn, M.stream, nrec, stride, pl->ccnt, pl->cq[0], pl->cq[1], pl->cq[2],
				   M.t, pl->cval)))
	return r;
    }
    else if ((r = launch_fill (M.stream, nrec, pl->kernel_value, pl->cval)))
      return r;
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      auto C = M.template cells<DIM> ();
      hipLaunchKernelGGL ((spread_correction_kernel<DIM, decltype (C)>), dim3 (pgrid),
			  dim3 (block), 0, M.stream, C, nchunk, stride, pl->ccnt, pl->ckey, pl->cval, pl->ccorr);
    }, M.dim == 3);
    GFSHIP_HIP (hipGetLastError ());
    GFSHIP_HIP (T.mark ());
    if ((r = coupling_sort_pairs (M, pl, nrec))) return r;
    with_bools ([&] (auto D3, auto RHO) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      constexpr bool R = !Mesh::TREE && decltype (RHO)::value;      /* a tree has no alpha */
      auto C = M.template cells<DIM> ();
      hipLaunchKernelGGL ((spread_sum_kernel<DIM, R, decltype (C)>), dim3 (rgrid), dim3 (block),
			  0, M.stream, C, nrec, pl->ckey2, M.ncell, pl->cval2, o0, pl->ccorr, pl->force[0], pl->force[1],
			  pl->force[2], alpha, Fa[0], Fa[1], Fa[2]);
    }, M.dim == 3, alpha != nullptr);
    GFSHIP_HIP (hipGetLastError ());
    GFSHIP_HIP (T.mark ());
  }
  int flag = 0;
  GFSHIP_HIP (hipMemcpyAsync (&flag, pl->cflag, sizeof (int), hipMemcpyDeviceToHost, M.stream));
  GFSHIP_HIP (hipStreamSynchronize (M.stream));
  if (info) {
    for (size_t q = 0; q + 2 < T.ev.size (); q += 3) {
      info[0] += T.ms (q);
      info[1] += T.ms (q + 1);
    }
    info[2] = stride;
    info[3] = per_chunk;
    info[4] = 56.*(double) per_chunk*stride;
  }
  GFSHIP_CHECK (flag == 0, GFSHIP_EHIP, "GfsSourceParticulate: a kernel reaches more than %d leaves", stride);
  return GFSHIP_OK;
}

// source_particulatevol_event (:2834-2852) / source_particulatemass_event (:2993-3012) once the caller has found
// and reset the variables it writes (leaves D, R, U[0 .. dim - 1], nullptr: not written) and the arrays `read' of
// the variables the function names: the passes of the header of particulate_sources.hip.
// info != nullptr: the milliseconds of the per-particle passes (steps 1 to 3) and of the sort with the pass per
// cell (step 4), from events on the stream
template <class Mesh>
int source_event_body (const Mesh & M, gfship_particulate_source * s, double * D, double * R, double * const U[3],
		       const std::vector<const double *> & read, double * info)
{
  gfship_particles * pl = s->pl;
  int r;
  if (info) info[0] = info[1] = 0.;
  if (pl->n == 0) return GFSHIP_OK;
  if ((r = particulate_source_reserve (s))) return r;
  StreamTimer T (M.stream, info != nullptr);
  GFSHIP_HIP (T.mark ());
  if ((r = M.source_gather (s))) return r;
  const int n = pl->n, block = 256, grid = (n + block - 1)/block;
  if (s->fn) {
    if ((r = M.launch_source (s, read))) return r;
  }
  else if ((r = launch_fill (M.stream, n, s->value, s->src)))
    return r;
  const bool fields = D || R || U[0] || U[1] || U[2];
  if (fields && (r = coupling_reserve (pl, (size_t) n, 0, false))) return r;
  if ((r = launch_particulate_source_update (s, M.stream, M.dt, M.ncell, fields ? pl->ckey : nullptr))) return r;
  GFSHIP_HIP (T.mark ());
  if (fields) {
    if ((r = coupling_sort_keys (M, pl, n))) return r;
    SourceCellArgs A;
    A.n = n; A.key = pl->ckey2; A.ncell = M.ncell;
    A.src = s->src; A.prad = s->prad;
    A.deposit = D; A.rad = R;
    for (int c = 0; c < 3; c++) {
      A.purel[c] = s->purel[c];
      A.urel[c] = U[c];
    }
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      auto C = M.template cells<DIM> ();
      hipLaunchKernelGGL ((particulate_source_cell_kernel<DIM, Mesh::TREE, decltype (C)>),
			  dim3 (grid), dim3 (block), 0, M.stream, C, A);
    }, M.dim == 3);
    GFSHIP_HIP (hipGetLastError ());
  }
  if (info) {
    GFSHIP_HIP (T.mark ());
    GFSHIP_HIP (hipStreamSynchronize (M.stream));
    info[0] = T.ms (0);
    info[1] = T.ms (1);
  }
  return GFSHIP_OK;
}

// gfs_feed_particle_event (:2404-2418) for np > 0 candidates, once the caller has made its checks: the passes of
// the header of feed_particle.hip
template <class Mesh>
int feed_event_body (const Mesh & M, gfship_feed_particle * f, int np, const double * pos)
{
  gfship_particles * pl = f->pl;
  GFSHIP_CHECK ((long) pl->n + np <= 0x7fffffffL, GFSHIP_ENOMEM, "the list would hold 2^31 slots or more");
  int r;
  std::vector<const double *> read[2];
  for (int w = 0; w < 2; w++)
    if ((r = M.arrays (f->read[w], read[w], true))) return r;
  if ((r = feed_reserve (f, np))) return r;
  if ((r = particles_reserve (pl, pl->n + np))) return r;
  /* the candidates come from pageable memory: the copy is staged before the call returns */
  GFSHIP_HIP (hipMemcpyAsync (f->cand, pos, 3*(size_t) np*sizeof (double), hipMemcpyHostToDevice, M.stream));
  const int base = pl->n;
  if ((r = M.feed_gather (base, np, f->cand, f->cell))) return r;
  double * out[2] = { pl->mass + base, pl->volume + base };
  for (int w = 0; w < 2; w++) {
    if (f->fn[w])
      r = M.launch_cell (f->fn[w], np, f->cell, read[w], out[w]);
    else
      r = launch_fill (M.stream, np, f->value[w], out[w]);
    if (r) return r;
  }
  if ((r = launch_feed_ids (pl, base, np, f->cell, f->block))) return r;
  pl->n += np;
  return GFSHIP_OK;
}

} // namespace gfship
