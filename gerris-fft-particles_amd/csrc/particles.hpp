// particles.hpp -- the particle list, the objects of its events and the cell search shared by particles.hip,
// coupling.hip, particulate_sources.hip, feed_particle.hip, droplets.hip and tree_particles.hip.  The host side of the
// events that run on a box and on a tree alike is particle_events.hpp; the checks of a function's text and of a table
// of variables are function_text.hpp.
#pragma once
#include "gfship_internal.hpp"
#include <functional>
#include <string>
#include <vector>

namespace gfship {
struct RtcKernel;
int  rtc_compile_coefficient (gfship_domain * dom, const char * text, RtcKernel ** out);
int  rtc_compile_coefficient_on (int device, const char * text, RtcKernel ** out);   // a list of a tree
int  rtc_launch_coefficient (RtcKernel * k, hipStream_t stream, int n, const unsigned char * alive,
			     const double * rep, const double * const rel[3], const double * pdia,
			     double t, double * out);
void rtc_free (RtcKernel * k);
// the kernel function of a GfsSourceParticulate: a GfsFunction (spatial) of x, y, z, t, evaluated for the
// first cnt[r/stride] records of every block of `stride' records
int  rtc_compile_spatial (gfship_domain * dom, const char * text, RtcKernel ** out);
int  rtc_compile_spatial_on (int device, const char * text, RtcKernel ** out);       // a list of a tree
int  rtc_launch_spatial (RtcKernel * k, hipStream_t stream, long nrec, int stride, const int * cnt,
			 const double * x, const double * y, const double * z, double t, double * out);
// the function of a GfsSourceParticulateVol / ...Mass: a GfsFunction of Rad, Urelp, Vrelp(, Wrelp: dim == 3), of
// x, y, z (the centre of the particle's cell), t and of the nf variables `names', evaluated for every creation
// slot o < n whose cell[o] is a cell of the box (its linear number; PSOURCE_NO_CELL: none)
constexpr unsigned PSOURCE_NO_CELL = 0xFFFFFFFFu;
int  rtc_compile_source (gfship_domain * dom, const char * text, int nf, const char * const * names,
			 RtcKernel ** out);
int  rtc_launch_source (RtcKernel * k, hipStream_t stream, int n, const Layout & L, const unsigned * cell,
			const double * rad, const double * const urel[3], double t, int nf,
			const double * const * fields, double * out);
// the mass and the volume of a GfsFeedParticle (feed_particle.hip): a GfsFunction of x, y, z (the centre of the
// candidate's cell), t and of the nf variables `names', evaluated for every candidate o < n with a cell
int  rtc_compile_cell (gfship_domain * dom, const char * text, int nf, const char * const * names, RtcKernel ** out);
int  rtc_launch_cell (RtcKernel * k, hipStream_t stream, int n, const Layout & L, const unsigned * cell, double t,
		      int nf, const double * const * fields, double * out);
// the same function on a list of a tree: cell[o] is the index of the leaf in the concatenated levels (Topo::gi);
// the kernel finds the level of the leaf from the level offsets off[0 .. depth + 1] and its integer coordinates
// from its index in the dense level, x, y, z = ftt_cell_pos of the leaf, and reads the variables (arrays of all
// levels) at the leaf
int  rtc_compile_tree_source (int device, int dim, const char * text, int nf, const char * const * names,
			      RtcKernel ** out);
int  rtc_launch_tree_source (RtcKernel * k, hipStream_t stream, int n, int dim, int depth, const int * off,
			     const unsigned * cell, const double * rad, const double * const urel[3], double t,
			     int nf, const double * const * fields, double * out);
// the mass and the volume of a GfsFeedParticle on a list of a tree: the function of rtc_compile_cell with the leaf
// of rtc_compile_tree_source as the cell (the same text and options; no Rad, Urelp ...), for every candidate o < n
// with a leaf
int  rtc_compile_tree_cell (int device, int dim, const char * text, int nf, const char * const * names,
			    RtcKernel ** out);
int  rtc_launch_tree_cell (RtcKernel * k, hipStream_t stream, int n, int depth, const int * off,
			   const unsigned * cell, double t, int nf, const double * const * fields, double * out);
}

// a GfsSourceParticulateVol / ...Mass (particulate_sources.hip) on a list of a box, or of a tree (pl->tree: the
// variables are GFSHIP_TREE_* numbers and the event is tree_particulate_source_event, tree_particles.hip)
struct gfship_particulate_source {
  gfship_particles * pl = nullptr;
  int kind = GFSHIP_PARTICULATE_SOURCE_VOLUME;
  gfship::RtcKernel * fn = nullptr;      // nullptr: the constant `value'
  double value = 0.;
  std::vector<gfship_field> read;        // the fields the function names, in the order of its arguments
  gfship_field rad = -1, urel[3] = { -1, -1, -1 }, deposit = -1;
  // per creation slot: the cell, Rad, Urelp ..., the source
  unsigned * cell = nullptr;
  double * prad = nullptr, * purel[3] = {}, * src = nullptr;
  int cap = 0;
};

// a GfsFeedParticle (feed_particle.hip) on a list of particulates of a box, or of a tree (pl->tree: the variables
// are GFSHIP_TREE_* numbers and the cell is the leaf): its two functions of the cell (0: mass, 1: volume) and the
// work arrays of an event
struct gfship_feed_particle {
  gfship_particles * pl = nullptr;
  gfship::RtcKernel * fn[2] = {};        // nullptr: the constant `value'
  double value[2] = {};
  std::vector<gfship_field> read[2];     // the fields each function names, in the order of its arguments
  double * cand = nullptr;               // 3 doubles per candidate
  // per candidate: the linear number of its cell (a box), the index of its leaf in the concatenated levels (a
  // tree), or PSOURCE_NO_CELL
  unsigned * cell = nullptr;
  unsigned * block = nullptr;            // per block of candidates: accepted, then the id before its first
  int cap = 0;
};

struct gfship_particles {
  gfship_sim * sim = nullptr;
  gfship_domain * dom = nullptr;
  gfship_tree * tree = nullptr;       // a list of GfsParticle or GfsParticulate on a refined tree (tree_particles.hip): sim, dom = nullptr
  hipStream_t stream = nullptr;       // the stream of dom or of tree
  int dim = 0;
  int n = 0;                   // slots in use (alive or not)
  int cap = 0;                 // slots allocated
  double * pos[3] = {}, * old[3] = {};
  unsigned * id = nullptr;
  unsigned char * alive = nullptr;
  unsigned * d_count = nullptr;
  unsigned * d_idlast = nullptr;      // idlast of the GfsParticleList (particle_id, :1231-1234), 0 at creation: every list
  // sort by cell
  unsigned * orig = nullptr;          // creation slot of the particle stored in each slot
  double * pos2[3] = {}, * old2[3] = {};   // gather targets (swapped with pos/old after a sort)
  unsigned * id2 = nullptr, * orig2 = nullptr;
  unsigned char * alive2 = nullptr;
  unsigned * key = nullptr, * key2 = nullptr, * slot = nullptr, * slot2 = nullptr;
  void * sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  int sort_every = 16, events_since_sort = -1;   // -1: never sorted yet
  // migration through GfsBoundaryMpi sides
  gfship_particle_migrate_fn migrate = nullptr; void * migrate_ctx = nullptr;
  double * outbox = nullptr;          // device, 6 x out_cap records of 7 doubles
  unsigned * out_count = nullptr;     // device, 6 counters
  int out_cap = 0;
  // GfsParticulate (modules/particulatecommon.h:35-48), indexed by the creation slot (`orig`):
  // velocity, force, mass, volume, diameter; the list's forces in application order
  bool particulate = false;
  int np0 = 0;                        // particles at creation
  double * vel[3] = {}, * force[3] = {}, * mass = nullptr, * volume = nullptr, * dia = nullptr;
  int nforces = 0, forces[8] = {};
  double gravity[3] = {};
  gfship_field uold[3] = { -1, -1, -1 };   // Un, Vn, Wn of GfsForceCoeff
  // GfsFunction coefficients of the GfsForceCoeff objects, compiled for the device (rtc.hip): the
  // variables Rep, Urelp, Vrelp, Wrelp, Pdia of every particle (slot order), and the values
  gfship::RtcKernel * coef_fn[8] = {};
  double * coef[8] = {}, * cin[6] = {};
  int coef_cap = 0;
  // two-way coupling (coupling.hip): rb of distance_normalization per creation slot, the kernel of the
  // GfsSourceParticulate (its radius; a constant or a compiled GfsFunction) and the work arrays of the
  // void fraction and of the spreading
  double * rb = nullptr;
  double rkernel = 0., kernel_value = 0.;
  gfship::RtcKernel * kernel_fn = nullptr;
  unsigned * where = nullptr;         // slot of each creation slot
  int where_cap = 0;
  unsigned long long * ckey = nullptr, * ckey2 = nullptr;   // (cell, creation slot) keys
  double * cq[3] = {}, * cval = nullptr, * cval2 = nullptr; // per record: q of the cell, K (q)
  double * ccorr = nullptr;           // per particle of the chunk: correction
  int * ccnt = nullptr;               // per particle of the chunk: leaves its kernel reaches
  int * cflag = nullptr;
  size_t ckey_cap = 0, crec_cap = 0, cpart_cap = 0;
};

extern "C" {
struct gfship_sim_view {
  gfship_domain * dom; const gfship_field * u; double dt; double visc; int visc_faces;
  int has_alpha;                    /* gfship_sim_set_alpha */
  gfship_field alpha_cell, mu;      /* gfship_sim_set_alpha_cell, gfship_sim_set_viscosity_cell; -1: not set */
};
gfship_sim_view gfship_sim_view_get (gfship_sim * s);   /* simulation.hip */
}

namespace gfship {
// the refusals of every entry that evaluates the forces of a list (particles.hip)
int particulate_fluid_check (const gfship_sim_view & v);
// what the event kernels of a box and of a tree share of their arguments (particulate_forces.hpp): the state of
// the particulates and the forces of the list with the default coefficients; then, where a force has a GfsFunction
// coefficient, cin and coef of the list (allocated for its capacity), the caller's coefficient-input kernel
// through launch_inputs, one rtc_launch_coefficient per function at time t, and A.coef[] (particles.hip)
struct ParticleForceArgs;
void particulate_force_args (const gfship_particles * pl, ParticleForceArgs & A);
int particulate_coefficients (gfship_particles * pl, ParticleForceArgs & A, hipStream_t stream, double t,
			      const std::function<void ()> & launch_inputs);
void coupling_free (gfship_particles * pl);   // coupling.hip
// the work arrays of the void fraction and of the spreading (coupling.hip), shared with the lists of a tree
// (tree_particles.hip): nrec record slots, npart particles of a chunk, on the stream of the list; a chunk holds
// at most COUPLING_RECORD_CAP slots
constexpr size_t COUPLING_RECORD_CAP = (size_t) 1 << 22;
int coupling_reserve (gfship_particles * pl, size_t nrec, size_t npart, bool spreading);
int coupling_sort_reserve (gfship_particles * pl, size_t need);
int coupling_key_bits (unsigned long long ncell);
// where[creation slot] = slot for the n slots of the list, and out[0 .. n - 1] = value (a constant GfsFunction), on
// the stream of the list / the stream given (coupling.hip)
int launch_where (gfship_particles * pl);
int launch_fill (hipStream_t stream, long n, double value, double * out);
// the per-particle arrays of a new list of np tracers (particles.hip); pl->stream is set by the caller
int particles_alloc (gfship_particles * pl, int np, const double * pos, const unsigned * id);
// grow the per-particle arrays to at least `need' slots, contents kept (particles.hip)
int particles_reserve (gfship_particles * pl, int need);
// the ids of the np candidates that took the slots from `base' on (feed_particle.hip), after their mass and volume
// are written: the accepted candidates per block, the scan that moves idlast, then id, flag, diameter and rb of
// every slot; `block' holds one count per 256 candidates.  On the stream of the list, for a box and for a tree
int launch_feed_ids (gfship_particles * pl, int base, int np, const unsigned * cell, unsigned * block);
// what an object that adds particulates to a list of a box refuses (feed_particle.hip): a list of a tree, a list of
// tracers, GfsBoundaryMpi sides, 2^32 cells or more; the work arrays of an event of np candidates
int feed_check (gfship_particles * pl, const char * what = "GfsFeedParticle");
int feed_reserve (gfship_feed_particle * f, int np);
// a GfsFeedParticle on a list of a tree (tree_particles.hip): does the tree have the variable `var' for a function to
// read at a leaf; the event of np candidates (feed_event_body, particle_events.hpp, on the stream of the tree)
bool tree_feed_variable (gfship_particles * pl, int var);
int tree_feed_event (gfship_feed_particle * f, int np, const double * pos);
// a list on a tree (tree_particles.hip): the event of its tracers, the keys of gfship_particles_sort and their bits
int tree_particle_list_event (gfship_particles * pl);
int tree_particle_keys (gfship_particles * pl, int * bits);
// the state of GfsParticulate of a list (velocity, mass, volume, diameter, rb; force = 0): what
// gfship_particles_set_particulate does after its checks (particles.hip)
int particulate_alloc (gfship_particles * pl, const double * vel, const double * mass, const double * volume);
// a list of particulates on a tree (gfship_particulates_create_tree, tree_particles.hip): its event with forces
int tree_particulate_list_event (gfship_particles * pl);
// the passes of particulate_sources.hip that are no kernel of a mesh: the per-slot arrays of the object and step 3
// (volume or mass += source*dt, diameter and rb, the key cell << 32 | slot); the constant function is launch_fill
int particulate_source_reserve (gfship_particulate_source * s);
int launch_particulate_source_update (gfship_particulate_source * s, hipStream_t stream, double dt,
				      unsigned long long pad, unsigned long long * key);
// the event of a source on a list of a tree (tree_particles.hip); info as in source_event_body
int tree_particulate_source_event (gfship_particulate_source * s, double * info);
}

// the coupling calls of a tree (gfship_tree_particulate_field ...): lists made by gfship_particulates_create_tree
#define GFSHIP_TREE_PARTICULATES_ONLY(pl, what) GFSHIP_CHECK ((pl)->tree && (pl)->particulate, GFSHIP_EUNSUPPORTED, \
    "%s needs a list of particulates of a tree (gfship_particulates_create_tree)", what)

// the calls of a box: migration exists on uniform boxes only, and the coupling, the sources and the feed of a list
// of a tree have entries of their own (gfship_tree_particulate_field ..., gfship_tree_particulate_source_create,
// gfship_tree_feed_particle_create).  A list of a tree is born as tracers (gfship_particles_create_tree) or as
// particulates (gfship_particulates_create_tree)
#define GFSHIP_NO_TREE_LIST(pl, what) GFSHIP_CHECK (!(pl)->tree, GFSHIP_EUNSUPPORTED, \
    "%s: a particle list on a refined tree holds GfsParticle tracers only (no particulates, forces, " \
    "coupling or migration)", what)
// forces and the particulate state: not on a list of tracers of a tree
#define GFSHIP_NO_TREE_TRACER_LIST(pl, what) GFSHIP_CHECK (!((pl)->tree && !(pl)->particulate), GFSHIP_EUNSUPPORTED, \
    "%s: a particle list on a refined tree holds GfsParticle tracers only (no particulates, forces, " \
    "coupling or migration)", what)

namespace gfship {

// ftt_cell_locate on the unit box centred on the origin, leaf level
template <int DIM>
__device__ __forceinline__ bool locate (int depth, const double target[3], int ijk[3])
{
  double pos[3] = { 0., 0., 0. };
  double size = 1./2.;
#pragma unroll
  for (int c = 0; c < DIM; c++)
    if (target[c] > pos[c] + size || target[c] < pos[c] - size)
      return false;
  int q[3] = { 0, 0, 0 };
  for (int l = 0; l < depth; l++) {
    size /= 2.;
#pragma unroll
    for (int c = 0; c < DIM; c++) {
      bool up = target[c] > pos[c];
      q[c] = 2*q[c] + (up ? 1 : 0);
      pos[c] += (up ? 1. : -1.)*size;
    }
  }
  ijk[0] = q[0] + 1; ijk[1] = q[1] + 1; ijk[2] = DIM == 3 ? q[2] + 1 : 0;
  return true;
}

// cond_kernel (:2126-2156) of cell ix[] of level l (0-based indices from the low corner of the box)
template <int DIM>
__device__ __forceinline__ bool cond_kernel (int l, const int ix[3], const double p[3], double rkernel)
{
  const double cellsize = 1./(double) (1 << l);
  double pos[3] = { 0., 0., 0. };
#pragma unroll
  for (int c = 0; c < DIM; c++)
    pos[c] = -0.5 + (ix[c] + 0.5)*cellsize;      /* ftt_cell_pos: dyadic, exact */
  const double size = cellsize/2.;
  const double radeq = DIM == 2 ? size*sqrt (2.) : size*sqrt (3.);
  const double dist = DIM == 2 ?
    sqrt ((pos[0] - p[0])*(pos[0] - p[0]) + (pos[1] - p[1])*(pos[1] - p[1])) :
    sqrt ((pos[0] - p[0])*(pos[0] - p[0]) + (pos[1] - p[1])*(pos[1] - p[1]) +
	  (pos[2] - p[2])*(pos[2] - p[2]));
  if (dist - radeq <= rkernel)
    return true;
#pragma unroll
  for (int c = 0; c < DIM; c++)
    if (p[c] > pos[c] + size || p[c] < pos[c] - size)
      return false;
  return true;
}

// check_intersetion, modules/particulatecommon.c:3058-3146
template <int DIM>
__device__ bool check_intersection (const double cellpos[3], const double p0[3], const double p1[3],
				    int * dstore, double size)
{
  for (int d = 0; d < 2*DIM; d++) {
    double normal = (double) (d ^ 1) - (double) d;
    int c = d/2;
    if ((p1[c] - p0[c]) != 0 && normal*(p1[c] - p0[c]) > 0) {
      double t = (cellpos[c] + normal*size*0.5 - p0[c])/(p1[c] - p0[c]);
      bool inside = true;
      for (int a = 0; a < DIM; a++)
	if (a != c) {
	  double pa = p0[a] + t*(p1[a] - p0[a]);
	  if (!((pa - cellpos[a] + size*0.5)*(pa - cellpos[a] - size*0.5) <= 0))
	    inside = false;
	}
      if (inside && t*(t - 1) <= 0) {
	*dstore = d;
	return true;
      }
    }
  }
  return false;
}

} // namespace gfship
