/* gfship.h -- C ABI of libgfship: the MI355X (gfx950) projection / advection / particle path
 * of Gerris behind the reference's own solver-plugin boundary.
 *
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference tree).  Plain C types only: opaque domain handle, integer field handles, host
 * pointers and sizes.  All functions returning int return 0 on success and a negative
 * GFSHIP_E* code on failure; gfship_last_error() then holds a message (the reference's hooks
 * return void and report through g_warning / g_log).
 *
 * The library is device-only: there is no CPU fallback.  gfship_domain_create() fails with
 * GFSHIP_ENODEVICE when no HIP device is present.
 *
 * Host-side array convention (upload/download): level l of a field is (n+2)^dim doubles,
 * n = 2^l, x fastest, one ghost layer per side; cell (i,j,k), 1 <= i,j,k <= n, is at
 * i + (n+2)*(j + (n+2)*k).  j grows with y, k with z.  The box is the unit cube/square
 * centred on the origin (GfsBox of size 1, boundary.h:319-327).
 */
#ifndef GFSHIP_H
#define GFSHIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFSHIP_VERSION   1
#define GFSHIP_MAXLEVEL  12

enum { GFSHIP_OK = 0, GFSHIP_EINVAL = -1, GFSHIP_ENODEVICE = -2, GFSHIP_ENOMEM = -3,
       GFSHIP_EHIP = -4, GFSHIP_EUNSUPPORTED = -5 };

/* what is behind each side of the box: box->neighbor[d] (src/boundary.h:319-327) */
enum { GFSHIP_SIDE_PERIODIC = 0,   /* GfsBoundaryPeriodic self edge, src/boundary.c:1704-1760 */
       GFSHIP_SIDE_BOUNDARY = 1,   /* GfsBoundary + per-variable GfsBc (default symmetry)    */
       GFSHIP_SIDE_EXTERNAL = 2 }; /* GfsBoundaryMpi, src/mpi_boundary.c:78-246              */

/* GfsBc kinds on a GFSHIP_SIDE_BOUNDARY side: src/boundary.c:45-74 (symmetry, the default),
   :253-279 (GfsBcDirichlet), :336-360 (GfsBcNeumann) */
enum { GFSHIP_BC_SYMMETRY = 0, GFSHIP_BC_DIRICHLET = 1, GFSHIP_BC_NEUMANN = 2 };

/* smoother of gfship_relax / gfship_poisson_cycle:
   EXACT  reproduces the reference's in-place sweep (src/poisson.c:507-557, tree pre-order of
          src/ftt.c:837-852) bit for bit on the device;
   REDBLACK is a two-colour Gauss-Seidel of the same operator: same fixed point, different
          iterates (not a reference algorithm; opt-in);
   EXACT_HYPERPLANE is EXACT with one launch per hyperplane instead of the pipelined
          tile sweep (same bits; kept as an independent implementation to test against);
   EXACT_PER_SWEEP is EXACT with one launch per sweep of a relax loop even where the sweeps of
          the loop can be pipelined in a single launch, and with the advection step through the
          face-value arrays even where it can be fused (same bits; the general paths, kept
          selectable to test the fused ones against them). */
enum { GFSHIP_RELAX_EXACT = 0, GFSHIP_RELAX_REDBLACK = 1, GFSHIP_RELAX_EXACT_HYPERPLANE = 2,
       GFSHIP_RELAX_EXACT_PER_SWEEP = 3 };

typedef struct gfship_domain gfship_domain;   /* GfsDomain + its per-level SoA device arrays */
typedef int gfship_field;                     /* GfsVariable handle (>= 0) */

typedef struct {           /* GfsNorm, src/fluid.h; filled as src/fluid.c:2107-2171 */
  double bias, first, second, infty, w;
} gfship_norm;

typedef struct {           /* GfsMultilevelParams, src/poisson.h:39-52, field for field */
  double tolerance;
  unsigned nrelax, erelax;
  unsigned minlevel;
  unsigned nitermax, nitermin;
  unsigned dimension;
  unsigned niter;
  unsigned depth;
  int weighted, function;
  double beta, omega;
  gfship_norm residual_before, residual;
} gfship_multilevel_params;

const char * gfship_last_error (void);
int          gfship_version (void);
int          gfship_device_count (void);

/* ---- domain and variables -------------------------------------------------------------- */

/* One uniform GfsBox refined to `depth` (Refine depth): replaces the FttCell/FttOct tree of
   src/ftt.h:134-159 and the per-cell GfsStateVector of src/fluid.h:39-52 by per-level SoA
   device arrays.  side[d], d = 0..2*dim-1 in the order of src/ftt.h:78-89. */
int  gfship_domain_create (gfship_domain ** dom, int dim, int depth, const int side[6],
			   int device);
void gfship_domain_destroy (gfship_domain * dom);
int  gfship_domain_set_relax_mode (gfship_domain * dom, int mode);
int  gfship_domain_synchronize (gfship_domain * dom);
/* raw HIP stream (hipStream_t) all work of this domain is enqueued on */
void * gfship_domain_stream (gfship_domain * dom);

/* gfs_domain_add_variable / gfs_temporary_variable (src/domain.c:3271-3385);
   component = 0..2 for a vector component (gfs_variable_set_vector), -1 for scalars */
gfship_field gfship_field_alloc (gfship_domain * dom, int component);
int  gfship_field_free (gfship_domain * dom, gfship_field f);
/* GfsBc of variable f on side d (src/boundary.c:1853-2014 box reader); val = n^(dim-1)
   leaf-level face-centre values (first tangential axis fastest) or NULL for 0 */
int  gfship_field_set_bc (gfship_domain * dom, gfship_field f, int d, int type,
			  const double * val);
int  gfship_field_upload (gfship_domain * dom, gfship_field f, int level, const double * host);
int  gfship_field_download (gfship_domain * dom, gfship_field f, int level, double * host);
int  gfship_field_fill (gfship_domain * dom, gfship_field f, int level, double value);
/* device pointer and layout of level `level`: cell (i,j,k) is at
   ptr[xo + i + px*(j + (n+2)*k)], the storage gfship_field_upload / _download of that level move
   at the time of the call.  Work enqueued on gfship_domain_stream is ordered with the library's.
   The pointer stays valid until the next call that advances a simulation of the domain
   (gfship_sim_start, gfship_sim_step, gfship_sim_advection_step, or any of the pieces
   gfship_predicted_face_velocities ... gfship_coarse_init): the library computes U, V, W and the
   tracers out of place and swaps the storage of a variable with a scratch array, so a pointer taken
   before such a call may address scratch after it -- ask again after every such call.  Between two of
   them the pointer is stable, and uploads, fills and downloads go to the same storage.  The call
   counts as a write of the field (a simulation brings the state it keeps unstored up to date first). */
void * gfship_field_device_ptr (gfship_domain * dom, gfship_field f, int level,
				int * px, int * xo);

/* gfs_domain_copy_bc (src/domain.c:846-867) / gfs_domain_homogeneous_bc (:945-965) */
int  gfship_bc (gfship_domain * dom, gfship_field v, gfship_field v1, int level);
int  gfship_homogeneous_bc (gfship_domain * dom, gfship_field ov, gfship_field v, int level);

/* ---- Poisson multigrid (the GfsPoissonSolverFunc boundary, src/poisson.h:32-38) -------- */

void gfship_multilevel_params_init (gfship_multilevel_params * par, int dim);
						/* gfs_multilevel_params_init, src/poisson.c:70-89 */
/* gfs_poisson_coefficients (src/poisson.c:856-901) with alpha = NULL */
int  gfship_poisson_coefficients (gfship_domain * dom);
/* gfs_poisson_coefficients (src/poisson.c:856-901) with a GfsFunction alpha (the inverse of the
   density: the equation is div (alpha grad p) = ...): alpha[c] holds gfs_function_face_value (alpha,
   face) of the leaf faces normal to c in the layout of a variable (the entry of a cell is its + face
   along c, the ghost entry in front of the first cell its - face).  Sets f[d].v of every cell of
   every level (poisson_coeff :769-797, face_coeff_from_below :826-853 with its one-neighbour rule);
   relax, residual, cycle and solve then use them (exact sweep order; 3-D levels of 32^3 and more on the
   pipelined tile kernel with the six weight rows streamed beside u / rhs / dia, 2-D levels in one
   launch per sweep).  alpha = NULL: gfship_poisson_coefficients.  The projections of a gfship_sim take
   the alpha of gfship_sim_set_alpha.  gfship_poisson_weights: the variable holding f[d].v,
   d = 0 .. 2 dim - 1. */
int  gfship_poisson_coefficients_alpha (gfship_domain * dom, const gfship_field alpha[3]);
int  gfship_poisson_weights (gfship_domain * dom, int d, gfship_field * w);
/* gfs_relax, src/poisson.c:604-632: one in-place sweep of level `level`.  d (and the `dimension' of the
   parameters of gfship_poisson_cycle / _solve) must be the dimension of the domain: GFSHIP_EUNSUPPORTED
   otherwise (the reference's d = 2 on a 3-D domain, relax2D over four neighbours, is not implemented) */
int  gfship_relax (gfship_domain * dom, unsigned d, int level, double omega,
		   gfship_field u, gfship_field rhs, gfship_field dia);
/* gfs_residual, src/poisson.c:721-747 */
int  gfship_residual (gfship_domain * dom, unsigned d, int level,
		      gfship_field u, gfship_field rhs, gfship_field dia, gfship_field res);
/* gfs_domain_norm_residual, src/domain.c:2239-2288 */
int  gfship_norm_residual (gfship_domain * dom, double dt, gfship_field res, gfship_norm * out);
/* gfs_domain_norm_variable on leaves, src/domain.c:2197-2232 */
int  gfship_norm_variable (gfship_domain * dom, gfship_field v, gfship_norm * out);
/* Two properties of the pipelined sweeps behind gfship_relax / _cycle / _solve on 3-D levels of 32^3
   cells and more, stated here because a caller can run into them:
   - their tiles hand lines over through 8-byte words in which the value itself is the flag: a word
     of all ones (0xFFFFFFFFFFFFFFFF, a NaN with that particular payload, which no arithmetic of the
     solver produces) means "not there yet".  A field that holds exactly that bit pattern in a cell
     along a tile border makes the hand-off wait run into its bound: the call returns GFSHIP_EHIP with
     the level in gfship_last_error().  Ordinary NaNs and infinities pass through like any value;
   - the loop of a periodic level in one launch needs all its tiles (256 workgroups at 256^3) resident
     on the device at the same time.  The library checks the occupancy and makes one trial run per
     level; if another process or stream holds compute units later on, the bounded waits time out,
     that solve fails with GFSHIP_EHIP (the field may then hold partially updated values) and the
     domain falls back to one launch per sweep for the rest of its life -- results of later calls
     are unaffected (same arithmetic, same order). */
/* gfs_poisson_cycle, src/poisson.c:1109-1178 */
int  gfship_poisson_cycle (gfship_domain * dom, gfship_multilevel_params * p,
			   gfship_field u, gfship_field rhs, gfship_field dia, gfship_field res);
/* gfs_poisson_solve, src/poisson.c:1225-1269: the function installed in
   GfsMultilevelParams.poisson_solve (called at src/timestep.c:423, src/simulation.c:2267) */
int  gfship_poisson_solve (gfship_domain * dom, gfship_multilevel_params * par,
			   gfship_field lhs, gfship_field rhs, gfship_field res,
			   gfship_field dia, double dt);

/* ---- implicit diffusion (GfsSourceDiffusion, no solids) -------------------------------------- */

/* gfs_diffusion_coefficients, src/poisson.c:1357-1390: face weights lambda2*beta*dt*D on every
   level (one scalar per level on a uniform box) and rhoc = 1. on every cell */
int  gfship_diffusion_coefficients (gfship_domain * dom, double D, double dt, gfship_field rhoc,
				    double beta);
/* gfs_diffusion_coefficients, src/poisson.c:1357-1399, with a coefficient that varies in space and a
   variable density (diffusion_coef :1280-1301, diffusion_mixed_coeff :1303-1333, face_coeff_from_below
   :826-853): D[c] holds gfs_source_diffusion_face (src/source.c:933-939) of the leaf faces normal to c
   in the layout of gfship_poisson_coefficients_alpha (the entry of a cell is its + face, the ghost
   entry in front of the first cell its - face).  Sets f[d].v = lambda2*(beta*dt)*D_face on the leaves
   (assignment) and every coarser level from below, on the device, into the variables
   gfship_poisson_weights returns: as in the reference the Poisson and the diffusion coefficients share
   f[d].v, so whoever solves a Poisson problem afterwards calls gfship_poisson_coefficients[_alpha]
   again.  alpha_cell: a variable the caller has filled with gfs_function_value (alpha, cell) on EVERY
   level (FTT_TRAVERSE_ALL, :1384-1386), rhoc = 1./alpha_cell on every level; alpha_cell = -1:
   rhoc = 1.  GFSHIP_EINVAL if a density is <= 0 (the reference's "density is negative", :1323-1330):
   rhoc and the coefficients are then undefined until the next successful call.
   gfship_diffusion_rhs, _residual, _cycle and gfship_diffusion then run with the six weights of every
   cell (diffusion_rhs :1401-1430, diffusion_relax :1471-1498, diffusion_residual :1534-1569) until
   gfship_diffusion_coefficients is called again.  Uniform boxes without MPI sides
   (GFSHIP_EUNSUPPORTED otherwise). */
int  gfship_diffusion_coefficients_faces (gfship_domain * dom, const gfship_field D[3], double dt,
					  gfship_field rhoc, gfship_field alpha_cell, double beta);
/* gfs_diffusion_rhs, src/poisson.c:1447-1453 (diffusion_rhs :1392-1436) */
int  gfship_diffusion_rhs (gfship_domain * dom, gfship_field v, gfship_field rhs,
			   gfship_field rhoc, double beta);
/* gfs_diffusion_residual, src/poisson.c:1587-1612 (diffusion_residual :1534-1569) */
int  gfship_diffusion_residual (gfship_domain * dom, gfship_field u, gfship_field rhs,
				gfship_field rhoc, gfship_field res);
/* gfs_diffusion_cycle, src/poisson.c:1633-1690 */
int  gfship_diffusion_cycle (gfship_domain * dom, unsigned levelmin, unsigned depth,
			     unsigned nrelax, gfship_field u, gfship_field rhs, gfship_field rhoc,
			     gfship_field res);
/* gfs_diffusion, src/timestep.c:735-788: the function installed in
   GfsAdvectionParams.diffusion_solve (called at src/timestep.c:944) */
int  gfship_diffusion (gfship_domain * dom, gfship_multilevel_params * par, gfship_field v,
		       gfship_field rhs, gfship_field rhoc);

/* ---- projection + advection time step (src/timestep.c, src/advection.c, src/simulation.c) -- */

typedef struct gfship_sim gfship_sim;   /* GfsSimulation on one box, src/simulation.h:56-82 */

typedef struct {           /* the fields of GfsAdvectionParams used here, src/advection.h:50-69 */
  double cfl, dt;
  int gradient;            /* 0 gfs_center_gradient (src/fluid.c:434-475),
			      1 gfs_center_van_leer_gradient (:522-561), 2 gfs_center_minmod_gradient,
			      3 gfs_center_superbee_gradient, 4 gfs_center_sweby_gradient (:563-690) */
  int gc;
} gfship_advection_params;

enum { GFSHIP_VAR_P = 0, GFSHIP_VAR_PMAC = 1, GFSHIP_VAR_U = 2, GFSHIP_VAR_G = 3,
       GFSHIP_VAR_GMAC = 4, GFSHIP_VAR_TRACER = 5,
       GFSHIP_VAR_UN = 6 /* MAC velocity of the + face of every cell along c (ghost cell 0: the - face of
			    the first cell), GFS_STATE (cell)->f[2c].un */ };

/* gfs_simulation_new + simulation_init (src/simulation.c:910-1015): allocates P, Pmac, U, V(, W),
   the gradient vectors g[], gmac[] of simulation_run (:432-456) and the face state.  One simulation
   per domain, as one GfsSimulation is its GfsDomain: a second gfship_sim_create on a domain that has
   one fails with GFSHIP_EUNSUPPORTED (and leaves the first untouched); after gfship_sim_destroy the
   domain takes a new one.
   State between calls: a gfship_sim_step may leave the MAC velocities of its approximate projection
   unstored; every entry point that reads them (the pieces below, gfship_sim_download_un,
   gfship_sim_variable (GFSHIP_VAR_UN)) or that lets the caller write a field of the domain
   (gfship_field_upload, _fill, _device_ptr, gfship_bc, the snapshot reader, the solvers called on
   their own) stores them first, from the fields as the step left them.  So the pieces and
   gfship_sim_step can be mixed in any order, and the fields can be rewritten between two calls.
   Likewise the centred gradient g of that projection where its only reader is the advection of the
   next gfship_sim_step, which forms it from P: it is stored before the caller can write a field, and
   for good once gfship_sim_variable (GFSHIP_VAR_G) has given out its handles. */
int  gfship_sim_create (gfship_sim ** sim, gfship_domain * dom);
void gfship_sim_destroy (gfship_sim * sim);
gfship_field gfship_sim_variable (gfship_sim * sim, int which, int c);
gfship_multilevel_params * gfship_sim_projection_params (gfship_sim * sim);
gfship_multilevel_params * gfship_sim_approx_projection_params (gfship_sim * sim);
gfship_advection_params *  gfship_sim_advection_params (gfship_sim * sim);
int      gfship_sim_set_time (gfship_sim * sim, double end, double dtmax); /* GfsTime */
/* gfs_simulation_set_timestep shortens the step so that it lands on the next event
   (src/simulation.c:1603-1610: for every GfsEvent, `if (t < next && next < tnext) tnext = next +
   1e-9` with next = gfs_event_next, starting from G_MAXINT).  The events belong to the host:
   the hook returns that tnext for the simulation time t and iteration i it is given. */
typedef double (* gfship_next_event_fn) (void * ctx, double t, unsigned i);
int      gfship_sim_set_next_event (gfship_sim * sim, gfship_next_event_fn fn, void * ctx);
double   gfship_sim_time (gfship_sim * sim);
unsigned gfship_sim_iter (gfship_sim * sim);
int      gfship_sim_add_tracer (gfship_sim * sim);       /* GfsVariableTracer, src/variable.c:427-431 */
/* GfsVariableTracer { gradient = gfs_center_gradient | gfs_center_van_leer_gradient (default) |
   gfs_center_minmod_gradient | gfs_center_superbee_gradient | gfs_center_sweby_gradient }: 0 .. 4
   (src/fluid.c:434-690); the same numbers in gfship_advection_params.gradient */
int      gfship_sim_set_tracer_gradient (gfship_sim * sim, int tracer, int gradient);
/* GfsVariableTracer { scheme = godunov | none } (GfsAdvectionScheme, src/advection.h:32-35).  With none the
   Godunov block of variable_sources (src/timestep.c:878-899) is skipped: the tracer is not advected, only
   its sources act.  Such a tracer does not enter min_cfl (src/simulation.c:1547-1550). */
enum { GFSHIP_SCHEME_GODUNOV = 0, GFSHIP_SCHEME_NONE = 1 };
int      gfship_sim_set_tracer_scheme (gfship_sim * sim, int tracer, int scheme);
/* GfsSourceDiffusion T D (src/source.c:933-1160) on a tracer: constant coefficient D (0. removes it).
   gfship_tracer_advection then follows the diffusion branch of gfs_tracer_advection_diffusion
   (src/timestep.c:1039-1048): rhs = a copy of T on the leaves, variable_sources (T -> rhs) with
   source_diffusion_value (src/source.c:1105-1144, no alpha factor: :1141-1143 is for velocity components) as
   the MAC source of the face values, then variable_diffusion (:923-949) with alpha = NULL, i.e.
   gfship_diffusion_coefficients (D, dt, rhoc, beta), gfship_diffusion_rhs and gfship_diffusion on T with its
   own conditions and its own parameters.  The CFL condition is untouched (the acceleration term of
   gfs_domain_cfl reads the sources of U, V, W only, src/domain.c:2893-2901).  D < 0 or a bad index:
   GFSHIP_EINVAL; a box with GFSHIP_SIDE_EXTERNAL sides: GFSHIP_EUNSUPPORTED. */
int      gfship_sim_set_tracer_diffusion (gfship_sim * sim, int tracer, double D);
/* the GfsMultilevelParams of that solve (tolerance 1e-6, beta 1: diffusion_init, src/source.c:966-974); the
   address holds for the life of the simulation; NULL for a bad index */
gfship_multilevel_params * gfship_sim_tracer_diffusion_params (gfship_sim * sim, int tracer);
/* How gfship_tracer_advection starts the solve of a tracer with a GfsSourceDiffusion.  fused = 1 (the
   default): where a tracer runs on the tiled Godunov kernel (3-D, six periodic sides, n a multiple of 32,
   gradient 0 or 1, scheme godunov) one pass over T writes rhs = T + fluxes + (1 - beta)/beta*f/(h*h) (the leaf
   copy, variable_sources and diffusion_rhs, src/timestep.c:1043-1045 and src/poisson.c:1392-1451); fused = 0:
   the three passes everywhere.  Same bits either way.  counts[0], counts[1]: the solves started by the fused
   and by the composed path since the simulation was created. */
int      gfship_sim_tracer_diffusion_path (gfship_sim * sim, int fused);
int      gfship_sim_tracer_diffusion_counts (gfship_sim * sim, unsigned long long counts[2]);
/* How many projections of gfship_sim_step have left their centred gradient unstored so far (see
   gfship_sim_create: for tests, the stored and the unstored path give the same bits). */
int      gfship_sim_gradients_unstored (gfship_sim * sim, unsigned long long * count);
/* GfsSourceDiffusion {} U|V|W nu (src/source.c:933-1160): constant implicit viscosity of
   velocity component c (0. removes it), and the GfsMultilevelParams of its solver
   (tolerance 1e-6, beta 1: diffusion_init, src/source.c:966-974) */
int      gfship_sim_set_viscosity (gfship_sim * sim, int c, double nu);
/* GfsSourceDiffusion {} U|V|W f(x,y,z,t) / GfsSourceViscosity f: D[q] holds gfs_source_diffusion_face
   (diffusion_face, src/source.c:933-939) of the leaf faces normal to q, in the layout of
   gfship_diffusion_coefficients_faces, kept by handle like alpha (the caller may rewrite the fields
   between steps); NULL removes it.  variable_diffusion (src/timestep.c:923-949) then runs
   gfship_diffusion_coefficients_faces, and the step takes the general advection path (face-value arrays
   + flux kernel) with the MAC source of gfship_variable_mac_source.  A component has one
   GfsSourceDiffusion: this call replaces a constant set by gfship_sim_set_viscosity, and
   gfship_sim_set_viscosity with nu != 0 replaces the fields.  Not on boxes with MPI sides
   (GFSHIP_EUNSUPPORTED). */
int      gfship_sim_set_viscosity_faces (gfship_sim * sim, int c, const gfship_field D[3]);
/* gfs_function_value (alpha, cell) of GfsPhysicalParams { alpha } on the cells of EVERY level, by
   handle (-1 removes it): the density of the implicit diffusion, rhoc = 1./alpha (diffusion_mixed_coeff,
   src/poisson.c:1321-1332, FTT_TRAVERSE_ALL), and the factor of its MAC source
   (source_diffusion_value, src/source.c:1141-1143).  With it gfship_sim_set_alpha and a viscosity go
   together. */
int      gfship_sim_set_alpha_cell (gfship_sim * sim, gfship_field alpha_cell);
/* the `mu' of the GfsDiffusion of U (update_mu / gfs_diffusion_cell, src/source.c:906-946): the
   GfsFunction of the GfsSourceDiffusion / GfsSourceViscosity of U at the centres of the leaf cells, by
   handle like alpha_cell (the caller may rewrite the field between events; -1 removes it).  Only the
   interior cells of the leaf level are read.  It is the viscosity the forces of a list of
   GfsParticulate take at the cell of each particle; nothing else reads it. */
int      gfship_sim_set_viscosity_cell (gfship_sim * sim, gfship_field mu);
/* gfs_variable_mac_source (src/source.c:38-59) of velocity component c for its GfsSourceDiffusion:
   source_diffusion_value (src/source.c:1105-1144) of every leaf cell,
   alpha(cell)*(sum_d D_f*e.b - (sum_d D_f)*v0)/(h*h), into the leaves of out */
int      gfship_variable_mac_source (gfship_sim * sim, int c, gfship_field out);
/* GfsPhysicalParams { alpha = ... } (src/simulation.c:1306-1440): the inverse of the density as
   gfs_function_face_value (alpha, face) on the leaf faces, alpha[c] in the layout of
   gfship_poisson_coefficients_alpha (kept by handle: the caller may rewrite the fields between steps
   when alpha depends on time or on a tracer).  Both projections then run gfs_poisson_coefficients
   with it (src/timestep.c:376), the multigrid with the face weights, and gfs_correct_normal_velocities
   / gfs_update_gradients with gfs_face_weighted_gradient's weights (:118-144,306-322).  NULL: alpha =
   NULL again.  Together with GfsSourceDiffusion once gfship_sim_set_alpha_cell has given alpha at the
   cell centres (the density of the diffusion equation); GFSHIP_EUNSUPPORTED before that. */
int      gfship_sim_set_alpha (gfship_sim * sim, const gfship_field alpha[3]);
/* GfsSource {} U|V|W g (src/source.c:362-500) with a constant intensity g on velocity component c
   (0. removes it): a body force per unit mass -- the MAC source of gfs_cell_advected_face_values
   (src/advection.c:88, gfs_variable_mac_source), the centred source added at the end of
   variable_sources (gfs_domain_variable_centered_sources, src/source.c:62-108), the acceleration
   time scale of gfs_domain_cfl (src/domain.c:2893-2901), and the gravity GfsForceBuoy reads
   (modules/particulatecommon.c:632-647).  Pinned by test/poiseuille (error.ref). */
int      gfship_sim_set_source (gfship_sim * sim, int c, double intensity);
gfship_multilevel_params * gfship_sim_diffusion_params (gfship_sim * sim, int c);
/* simulation_run before its loop (src/simulation.c:458-476): BCs, first time step, initial
   approximate projection */
int  gfship_sim_start (gfship_sim * sim);
/* GfsTime { i = .. t = .. } of a simulation file that is a snapshot of a running simulation
   (gfs_time_read, src/simulation.c:1687-1725): call it before gfship_sim_start, which then takes
   simulation_run's `time.i > 0' branch (no initial projection; gfs_update_gradients,
   src/simulation.c:474-475) */
int  gfship_sim_restart (gfship_sim * sim, double t, unsigned i);
/* one iteration of the simulation_run loop body (src/simulation.c:479-548) */
int  gfship_sim_step (gfship_sim * sim);
/* loop body of advection_run (GfsAdvection, src/simulation.c:2078-2111) with given MAC velocities
   (GfsVariableStreamFunction, src/variable.c:931-1086: upload them through GFSHIP_VAR_UN and the
   centred ones through GFSHIP_VAR_U): coarse values, time step, tracers */
int  gfship_sim_advection_step (gfship_sim * sim);
/* the pieces, callable on their own: */
int  gfship_predicted_face_velocities (gfship_sim * sim);      /* src/timestep.c:681-717 */
int  gfship_mac_projection (gfship_sim * sim, gfship_multilevel_params * par, double dt,
			    gfship_field p, const gfship_field g[3]);        /* :460-484 */
int  gfship_approximate_projection (gfship_sim * sim, gfship_multilevel_params * par, double dt,
				    gfship_field p, const gfship_field g[3]); /* :560-596 */
int  gfship_centered_velocity_advection (gfship_sim * sim, const gfship_field gmac[3],
					 const gfship_field g[3]);           /* :976-1016 */
/* gfs_correct_centered_velocities (src/timestep.c:498-530): U -= g dt on the leaves, then the
   conditions of U, V(, W) -- the statement between the advection and gfs_cell_coarse_init in the
   loop body of simulation_run (src/simulation.c:517-521, there with g or gmac and - dt) */
int  gfship_correct_centered_velocities (gfship_sim * sim, const gfship_field g[3], double dt);
/* gfs_tracer_advection_diffusion: with a coefficient set by gfship_sim_set_tracer_diffusion the branch of
   :1039-1048, otherwise variable_sources in place and the conditions of t */
int  gfship_tracer_advection (gfship_sim * sim, gfship_field t, double dt);  /* :1028-1055 */
int  gfship_domain_cfl (gfship_sim * sim, double * cfl);       /* src/domain.c:2824-2923 */
int  gfship_set_timestep (gfship_sim * sim);                   /* src/simulation.c:1569-1633 */
int  gfship_coarse_init (gfship_sim * sim);                    /* src/adaptive.c:43-58 */
/* `sim->time.t = sim->tnext; sim->time.i++' of the loop body (src/simulation.c:538-539), tnext being
   the one the last gfship_set_timestep chose (it is not t + dt where an event cut the step) */
int  gfship_sim_advance_time (gfship_sim * sim);
/* OutputScalarNorm { v = Divergence }: gfs_divergence (src/fluid.c:2357-2376) + norm */
int  gfship_divergence_norm (gfship_sim * sim, gfship_norm * out);
/* MAC normal velocity on the faces orthogonal to component c, as a host array in the cell
   convention: entry (i,j,k) is the face on the + side of cell (i,j,k) (0 <= i <= n along c) */
int  gfship_sim_download_un (gfship_sim * sim, int c, double * host);

/* GfsOutputLocation's sampling (src/output.c:1182-1199): gfs_domain_locate + gfs_interpolate
   (src/fluid.c:2983-3101) of variable v at np points (pos = 3*np doubles); inside[q] = 0 where
   the point is outside the domain (out[q] is then 0).
   GFS_NODATA (DBL_MAX) is not supported: nothing in this library produces it (no solid boundaries, no
   masked variables), so neither `return GFS_NODATA' of gfs_interpolate (:2704-2705) nor the fall-back
   to the cell's value in gfs_cell_corner_value (:3096-3097) exists here; a field that holds DBL_MAX is
   sampled as the number it is (tests/test_gpu_sampler_reference.py pins that).  The same holds for the
   particle events, which share the sampler. */
int  gfship_field_interpolate (gfship_domain * dom, gfship_field v, int np, const double * pos,
			       double * out, unsigned char * inside);

/* ---- snapshots: the cell data of a binary simulation file (GfsOutputSimulation { binary = 1 }) ---- */

/* What gfs_box_write / gfs_box_read put between the braces of the GfsBox when the domain parameter
   `binary = 1' is set (src/boundary.c:1819-1851,1853-2014): ftt_cell_write_binary
   (src/ftt.c:1771-1799) -- the tree in pre-order, children 0..7 in the order of src/ftt.c:301-316, per
   cell `guint flags' = child id | FTT_FLAG_LEAF on the deepest level -- with gfs_cell_write_binary
   (src/domain.c:3176-3207) as the per-cell function: a double -1. (no solid fractions), then one
   double per variable of `variables = ...'.  Every level of every variable is written / read (the
   non-leaf values are whatever gfs_cell_coarse_init left); ghost cells are not part of the file
   (apply the BCs after reading, as gfs_simulation_init does).
     gfship_snapshot_tree_bytes: size of that byte image for nvars variables;
     gfship_snapshot_tree_write: builds it on the device and copies it into host_buf;
     gfship_snapshot_tree_read: takes it apart into the variables; fails if the child ids, the leaf
       flags (the tree must be the uniform tree of this domain) or the -1. markers do not match
       (cell_read_binary src/ftt.c:1915-1945, gfs_cell_read_binary src/domain.c:3219-3270). */
size_t gfship_snapshot_tree_bytes (gfship_domain * dom, int nvars);
int  gfship_snapshot_tree_write (gfship_domain * dom, int nvars, const gfship_field * vars,
				 void * host_buf, size_t bytes);
int  gfship_snapshot_tree_read (gfship_domain * dom, int nvars, const gfship_field * vars,
				const void * host_buf, size_t bytes);

/* ---- energy spectra (modules/fft.c) ------------------------------------------------------------ */

/* GfsOutputEnergySpectra (modules/fft.c:1340-1474) of the whole box at the finest level: for each of
   the ncomp variables (U, V[, W]) the real-to-complex DFT of (u - <u>)/ntot (fill_cartesian_matrix,
   :966-1001), |F|^2 summed into Ek[knx^2 + kny^2 + kz^2] with the weights of :1409-1448.  Ek has
   gfship_energy_spectra_bins() entries; the reference prints "deltak*sqrt(i) Ek[i]" for i >= 1 and
   "# Total energy = Etot" (write_energy_spectra, :1340-1348).  The DFT is rocFFT's through hipFFT
   (FFTW in the reference): same definition, not the same rounding. */
int  gfship_energy_spectra_bins (gfship_domain * dom);
int  gfship_energy_spectra (gfship_domain * dom, int ncomp, const gfship_field * comps, double * Ek,
			    double * Etot, double * deltak);

/* GfsOutputSpectra (modules/fft.c:1101-1160) of the whole 3-D domain at the finest level: the r2c DFT
   (FFTW's sign and normalisation: none) of (v - <v>)/ntot, with <v> the volume average over the
   cells of all levels (substract_average, :897-908).  out receives N*N*(N/2 + 1) complex numbers
   (re, im), index (ix*N + iy)*(N/2 + 1) + iz, N = gfship_output_spectra_side(); *kstep = 2 pi/(x1 - x0)
   (init_kmax, :1031-1045): write_spectra prints "kx ky kz re*L im*L" with k = kstep times the
   signed index.  On a box of a lattice (communicator or gather hook) every rank receives the
   transform of the whole lattice -- the reference redistributes slabs for FFTW-MPI (:467-669) --
   and gfship_energy_spectra likewise bins the whole domain.
   gfship_output_spectra_plane: the same event with a flat box (realdim == 2, :1131-1141,
   fill_interpolated_cartesian_matrix :822-883): the cells the points of the plane normal to `normal' (0 x,
   1 y, 2 z) at coordinate pos (-0.5 <= pos < 0.5) lie in, minus their mean, over their number.  order_array
   (:795-820) sorts the directions by descending size, so the flat one comes LAST and is the one that is
   "halved" (1/2 + 1 = 1): the transform is the FULL 2-D DFT.  out receives N*N complex numbers (2*N*N
   doubles: twice what the half-spectrum layout of earlier versions took -- size the buffer accordingly),
   index ia*N + ib, ia / ib the first / second in-plane coordinate in coordinate order; write_spectra prints
   k = kstep times the signed index (q < N/2 + 1 ? q : q - N) along both and 0 along the normal; one box.
   GfsOutputSpectraInterface samples the position of a VOF interface (out of scope with VOF): not provided. */
int  gfship_output_spectra_side (gfship_domain * dom);
int  gfship_output_spectra (gfship_domain * dom, gfship_field v, double * out, double * kstep);
int  gfship_output_spectra_plane (gfship_domain * dom, gfship_field v, int normal, double pos, double * out,
				  double * kstep);

/* GfsVariableTurbulentViscosity (modules/turbulence.c:953-1105): out = (Cs h)^2 |S| on the leaf cells
   from the centred differences of u (gfs_cm_gradient); model 1 = Smagorinsky (what the reference's
   files get: model_type is never read), model 0 = the sigma model of :980-1048 (libm calls: not
   bit-identical across C libraries). */
int  gfship_turbulent_viscosity (gfship_domain * dom, const gfship_field u[3], double Cs, int model,
				 gfship_field out);

/* GfsInitSpectra (modules/turbulence.c:270-901), 3-D: fills the variables v[0..2] with a synthetic
   solenoidal velocity field whose shell energies follow Pope's model spectrum (ReL != 0:
   alpha epsilon^(2/3) k^(-5/3) fL feta with c1, c2, c3) or k^2 (ReL = 0) below kmax, rescaled to the
   total energy E, on a periodic cube of side L centred on (x0, y0, z0) with 2^level points per side,
   interpolated at the cell centres.  The phases follow the reference: srand (seed) before every
   rand(), i.e. one value for all modes.  Field names in the struct = keywords of the .gfs object. */
typedef struct {
  double x0, y0, z0, L, E;
  double alpha, epsilon, c1, c2, c3, ReL, kmax, seed;
  int level;
} gfship_init_spectra_params;
int  gfship_init_spectra (gfship_domain * dom, const gfship_init_spectra_params * par,
			  const gfship_field v[3]);

/* ---- Lagrangian tracers (src/particle.c, modules/particulatecommon.c) ------------------------ */

typedef struct gfship_particles gfship_particles;   /* GfsParticleList of GfsParticle */

/* GfsParticleList read (modules/particulatecommon.c:1022-1093): np particles, pos = 3*np doubles
   (x y z per particle, z ignored in 2-D), id = np unsigned (src/particle.c:46-99 text format) */
int  gfship_particles_create (gfship_particles ** pl, gfship_sim * sim, int np,
			      const double * pos, const unsigned * id);
void gfship_particles_destroy (gfship_particles * pl);
/* gfs_particle_list_event (modules/particulatecommon.c:980-1015) without forces: drop particles
   outside the domain, RK2-advect each with the simulation's current velocity and dt
   (gfs_particle_event src/particle.c:31-44 -> gfs_domain_advect_point src/domain.c:2764-2788),
   then gfs_particle_bc (:3375-3395, periodic wrap :3189-3214) */
int  gfship_particle_list_event (gfship_particles * pl);
/* storage order only (no reference counterpart; arithmetic and download order unchanged): sort
   the slots by containing cell now / every `every` events (default 16, 0 = never) */
int  gfship_particles_sort (gfship_particles * pl);
int  gfship_particles_set_sort_interval (gfship_particles * pl, int every);
/* particles crossing a GFSHIP_SIDE_EXTERNAL side go to the box across it (send_particles /
   rcv_particles, modules/particulatecommon.c:3218-3312).  On a domain with the library's communicator
   (gfship_domain_comm_init) the packets travel by ncclSend / ncclRecv, counts first, then the records,
   and no hook is needed; without communicator and without hook the particles are dropped like at any
   non-periodic side.  A hook, when set, takes precedence.  It is called once per event by every box: nsend[d] records leave
   through side d (send[d]: gfship_particles_record_size doubles each -- position, old position, id,
   for particulates also velocity, mass, volume, force -- already in the
   coordinates of the receiving box, sorted by id); it returns in nrecv[d] / recv[d] the records
   that arrive through side d (host memory owned by the hook until its next call); they join the
   list in side order */
typedef int (* gfship_particle_migrate_fn) (void * ctx, const int nsend[6],
					    const double * const send[6], int nrecv[6],
					    const double * recv[6]);
int  gfship_particles_set_migrate (gfship_particles * pl, gfship_particle_migrate_fn fn, void * ctx);
/* doubles per record of the migration packets: 7, or 15 for particulates (+ velocity, mass, volume,
   force) */
int  gfship_particles_record_size (gfship_particles * pl);
/* slots in use (alive or not): upper bound of the count, size of the download buffers */
int  gfship_particles_slots (gfship_particles * pl);
int  gfship_particles_count (gfship_particles * pl);
/* positions and ids of the particles still on the list, in list order; returns their number */
int  gfship_particles_download (gfship_particles * pl, double * pos, unsigned * id);
/* pos_old (GfsParticle, src/particle.h) of the same particles in the same order; returns their number */
int  gfship_particles_download_old (gfship_particles * pl, double * old);

/* GfsParticulate with forces (modules/particulatecommon.h:35-61, particulatecommon.c:91-842): the
   particles of the list get a velocity (3*np), a mass and a volume (np each), and the list a set of
   GfsParticleForce objects applied in the given order.  gfship_particle_list_event then runs
   gfs_particulate_event (:768-842): forces per unit volume from the fields at the start of the
   step -- GfsForceInertial Du/Dt (:285-336, with the velocity of the previous step kept in Un, Vn,
   Wn), GfsForceAddedMass (:363-427, cm = 0.5, adds rho*volume*cm to the mass at every event like the
   reference), GfsForceLift (:455-524, cl = 0.5), GfsForceDrag (:527-588, default law
   cd = 16 (1 + 0.15 Re^0.5)/Re below Re = 50, 48 (1 - 2.21/Re^0.5)/Re above; no force without
   viscosity), GfsForceBuoy (:619-653, gravity = the sum of the GfsSource intensities on U, V, W) --
   then pos += vel*dt/2, vel += force*dt/mass, pos += vel*dt/2 and gfs_particle_bc.  The density and
   the viscosity of the fluid are those of the cell that holds the particle (fluid_rho = 1./alpha and
   gfs_diffusion_cell of the GfsSourceDiffusion of U, :273-279): 1./alpha_cell wherever
   gfship_sim_set_alpha_cell is set (1. otherwise), the field of gfship_sim_set_viscosity_cell where it
   is set and the constant gfship_sim_set_viscosity of U otherwise.  A cell without viscosity gives no
   drag, and 0.001 in the Rep of the coefficient functions.  GFSHIP_EUNSUPPORTED from
   gfship_particles_set_forces and gfship_particle_list_event while U has gfship_sim_set_viscosity_faces
   and no gfship_sim_set_viscosity_cell, or the simulation gfship_sim_set_alpha and no
   gfship_sim_set_alpha_cell.  Particulates migrate between boxes like
   tracers, with 15-double records.
   gfship_particles_set_force_coefficient: the GfsFunction a GfsForceAddedMass / GfsForceLift /
   GfsForceDrag object of the list may carry (gfs_force_coeff_read, :166-210) -- C text as in the
   simulation file, an expression or a { block } with a return, of the variables Rep, Urelp, Vrelp,
   Wrelp, Pdia (set per particle as in :364-384,462-485,545-573) and t.  gerris compiles it with the
   host compiler; here it is compiled for the GPU of the domain with hipRTC and evaluated for all
   particles by a kernel of its own before the event kernel (same C arithmetic, the device's libm).
   `force' is the index into the list given to gfship_particles_set_forces.  A text that does not
   compile: GFSHIP_EINVAL with the compiler's messages in gfship_last_error(). */
enum { GFSHIP_FORCE_INERTIAL = 1, GFSHIP_FORCE_ADDEDMASS = 2, GFSHIP_FORCE_LIFT = 3,
       GFSHIP_FORCE_DRAG = 4, GFSHIP_FORCE_BUOY = 5 };
int  gfship_particles_set_particulate (gfship_particles * pl, const double * vel, const double * mass,
				       const double * volume);
int  gfship_particles_set_forces (gfship_particles * pl, int nforces, const int * kinds,
				  const double gravity[3]);
int  gfship_particles_set_force_coefficient (gfship_particles * pl, int force, const char * function);
/* velocity (3 per particle), mass and force of the particles still on the list, in list order (any
   pointer may be NULL); returns their number */
int  gfship_particles_download_particulate (gfship_particles * pl, double * vel, double * mass,
					    double * force);

/* Two-way coupling: the particles act on the fluid (modules/particulatecommon.c:1927-2228).  Uniform
   boxes without GfsBoundaryMpi sides, lists of particulates; GFSHIP_EUNSUPPORTED otherwise, and where
   gfship_particles_set_forces refuses.  Every result is the reference's sum in the order of its particle
   list (the order of gfship_particles_download), bit for bit, whatever the storage order of the particles
   (gfship_particles_sort) and from run to run: contributions are sorted by (cell, list position) and
   added serially per cell, never with atomics.
   gfship_particulate_field: GfsParticulateField (particulate_field_event, :1934-1957).  v is reset on the
   leaves, then v[cell] += volume/ftt_cell_volume (cell) for every particle that gfs_domain_locate finds a
   cell for (L = 1).
   gfship_particles_forces_on_fluid: for every particle force = 0, then force[c] = new_force[c]*volume +
   force[c] over the forces of the list in order except GfsForceBuoy (compute_forces_onfluid, :753-765, in
   source_particulate_event, :2199-2206).  The stored force changes (read it with
   gfship_particles_download_particulate), and the mass of a particle inside the box grows by what every
   GfsForceAddedMass of the list adds (compute_addedmass_force, :391, is called here as in an event and
   nothing takes the addition back).  No particle moves or leaves; Un, Vn, Wn stay.
   gfship_particles_set_kernel: rkernel and kernel of GfsSourceParticulate (source_particulate_read,
   :2271-2289): rkernel is an absolute length (cond_kernel, :2143; the `influencerad' of :2210 is never
   used); function is a GfsFunction (spatial) of x, y, z, t -- C text, an expression or a { block },
   compiled for the device with hipRTC like the force coefficients (GFSHIP_EINVAL with the compiler's
   messages where it does not compile); a number is a constant and compiles nothing; NULL is the constant 0
   of source_particulate_init (:2342-2350), which deposits nothing.
   gfship_particles_spread_forces: F[c] (c < dim) are reset on the leaves, then for every particle in list
   order the two pruned traversals of :2208-2222: a leaf is reached if it and its ancestors pass cond_kernel
   (:2126-2156: |centre - pos| - (size/2) sqrt (dim) <= rkernel, or the particle inside the cell; no
   periodic wrap), correction = sum K (q) cellvol / sum cellvol in traversal order with q =
   distance_normalization (:2089-2099: (centre - pos)/rb for x and y, rb = pow (3 volume/(4 pi), 1./3.); z is
   0 in 2-D and (0. - pos.z)/rb in 3-D, as written there), and where correction > 1.e-10
   F[c][cell] -= force[c]/liq_rho/cellvol*K (q)/correction with liq_rho = 1./alpha_cell where
   gfship_sim_set_alpha_cell is set and 1. otherwise (diffuse_force, :2158-2175).
   gfship_source_particulate_event: source_particulate_event (:2177-2228), the two calls above in turn. */
int  gfship_particulate_field (gfship_particles * pl, gfship_field v);
int  gfship_particles_forces_on_fluid (gfship_particles * pl);
int  gfship_particles_set_kernel (gfship_particles * pl, double rkernel, const char * function);
int  gfship_source_particulate_event (gfship_particles * pl, const gfship_field F[3]);
int  gfship_particles_spread_forces (gfship_particles * pl, const gfship_field F[3]);
/* gfship_particles_spread_forces, measured (no reference counterpart): info[0], info[1] = the milliseconds
   the device spent in pass 1 (the descent of every particle, the kernel function, volume and correction:
   kernel_volume, :2108-2119) and in pass 2 (the sort of the records and the sums per cell: diffuse_force,
   :2158-2175), summed over the chunks from events on the domain's stream; info[2] = the record slots of a
   particle, info[3] = the particles of a chunk, info[4] = the bytes of the record arrays (56 per slot, at
   most 2^22 slots).  A kernel whose slots per particle exceed a chunk is refused (GFSHIP_EUNSUPPORTED, by
   gfship_particles_set_kernel already), and so is a box of 2^32 cells or more. */
int  gfship_particles_time_spreading (gfship_particles * pl, const gfship_field F[3], double info[5]);
/* GfsSourceParticulate in the time step: U, V, W (c < dim) get the velocity source whose centred value is
   F[c] of the cell (source_particulate_centered_value, :2067-2079) and whose MAC value is F[c] interpolated
   on the positive face of component c, gfs_face_interpolated_value_generic (source_particulate_value,
   :2029-2065; beyond a side of the box it reads the ghost cells of F as the caller left them: the
   reference's event applies no boundary condition to them).  The MAC value enters gfs_variable_mac_source
   (src/source.c:38-59) -- the face values of the advection (src/advection.c:82,124), hence the predicted
   face velocities, and the acceleration scale of gfs_domain_cfl (src/domain.c:2882-2883) -- and the centred
   value add_sources (src/source.c:66-79).  v->sources is visited last-read first (gts_container_add puts a
   source at the head; a GfsSourceParticulate stands below its particle list, after the other sources of a
   usual file): sum = 0. + F-term + GfsSourceDiffusion + GfsSource.  The fields are read at every use: the
   event may rewrite them between steps.  With source fields the time step takes the general advection path
   (face-value arrays), not the fused periodic one; gfship_variable_mac_source then gives the sum without the
   constant of gfship_sim_set_source.  NULL removes the source.  GFSHIP_EUNSUPPORTED on a box with
   GfsBoundaryMpi sides. */
int  gfship_sim_set_source_fields (gfship_sim * sim, const gfship_field F[3]);

/* The particles themselves change: GfsSourceParticulateVol (modules/particulatecommon.c:2734-2887) and
   GfsSourceParticulateMass (:2889-3047), objects on a list of particulates of a uniform box.
   GFSHIP_EUNSUPPORTED on a list of a tree, on a list of tracers, on a box with GFSHIP_SIDE_EXTERNAL sides and
   on a box of 2^32 cells or more (what the two-way coupling refuses).
   gfship_particulate_source_create (source_particulatevol_read, :2752-2804; ..mass_read, :2908-2962): kind is
   the class; function is its GfsFunction -- C text as in the simulation file, an expression or a { block }
   with a return -- compiled for the device of the domain with hipRTC exactly as the force coefficients are
   (-ffp-contract=off, the device's libm; GFSHIP_EINVAL with the compiler's messages in gfship_last_error ()
   where it does not compile).  A number is a constant and compiles nothing; NULL is the constant 0 of
   source_particulatevol_init / ..mass_init (:2861-2864, :3021-3024).  The function may name Rad, Urelp, Vrelp,
   Wrelp (3-D only), x, y, z, t, and the nvars variables of the table (names[q], fields[q]); a name of the
   table that is one of those eight, or no C identifier, is GFSHIP_EINVAL.  Destroy the object before its list.
   gfship_particulate_source_set_fields: the variables Rad, Urelp, Vrelp, Wrelp (gfs_domain_get_or_add_variable,
   :2785-2793) and the optional volsource / dmdtvariable (:2797-2803, :2954-2960); each may be -1: nothing is
   written there (urel[2] is ignored in 2-D; with all five at -1 the event sorts nothing).  A function that
   names the deposit variable would read a running sum that depends on the walk: GFSHIP_EUNSUPPORTED.
   gfship_particulate_source_event (source_particulatevol_event, :2834-2852; ..mass_event, :2993-3012), on the
   stream of the list: the deposit is reset (on every level for a volume, FTT_TRAVERSE_ALL :2844; on the leaves
   for a mass, :3004), then for every particle in list order (update_vol, :2806-2832; update_mass, :2964-2991)
   cell = gfs_domain_locate (pos); Rad[cell] = pow (3.0*volume/4.0/M_PI, 1./3.); Urelp ...[cell] =
   gfs_interpolate (cell, pos, U ...) - vel; source = the function at the cell; volume (mass) += source*dt with
   the dt of gfship_particle_list_event; deposit[cell] += source.  The function sees the particle's own Rad and
   relative velocity however many particles share the cell, the cell's value of every variable of the table,
   the centre of the cell for x, y, z and gfship_sim_time for t.  After the event Rad, Urelp ... of a cell hold
   the values of its last particle in list order (cells without a particle keep what they held: nothing resets
   these four), and the deposit of a cell is the left-to-right sum of its sources in list order from 0, bit for
   bit, whatever the storage order (gfship_particles_sort) and from run to run: records sorted by (cell, list
   position), added serially, no atomics.  A particle for which gfs_domain_locate finds no cell makes the
   reference dereference NULL; here it is skipped: nothing is written for it and nothing of it changes.
   After a volume event the diameter (compute_drag_force, :552) and rb (distance_normalization, :2091) of every
   particle with a cell are recomputed from the new volume.  pow: Rad, and the diameter and rb of a particle
   whose volume an event has changed, are values of the device's pow in the reference's expression (glibc's
   and the device's need not round alike); everything else is the reference's arithmetic.  A list no volume
   event has run on keeps its host-computed diameter and rb: its events give the bits they gave before.
   gfship_particulate_source_time_event: the event, measured (no reference counterpart): info[0], info[1] = the
   milliseconds the device spent in the passes per particle (locate and interpolation, the function, the
   update) and in the sort with the pass per cell.
   gfship_particles_download_volume: the volume of the particles still on the list, in list order; returns
   their number (lists of particulates, of a box or of a tree). */
typedef struct gfship_particulate_source gfship_particulate_source;
enum { GFSHIP_PARTICULATE_SOURCE_VOLUME = 0, GFSHIP_PARTICULATE_SOURCE_MASS = 1 };
int  gfship_particulate_source_create (gfship_particulate_source ** src, gfship_particles * pl, int kind,
				       const char * function, int nvars, const char * const * names,
				       const gfship_field * fields);
int  gfship_particulate_source_set_fields (gfship_particulate_source * src, gfship_field rad,
					   const gfship_field urel[3], gfship_field deposit);
int  gfship_particulate_source_event (gfship_particulate_source * src);
int  gfship_particulate_source_time_event (gfship_particulate_source * src, double info[2]);
void gfship_particulate_source_destroy (gfship_particulate_source * src);
int  gfship_particles_download_volume (gfship_particles * pl, double * volume);

/* Particles join a list during a run: GfsFeedParticle (modules/particulatecommon.c:2375-2647), an object on a
   list of particulates of a uniform box.  GFSHIP_EUNSUPPORTED on a list of a tree (its object is made by
   gfship_tree_feed_particle_create, below, and its idlast has calls of its own), on a list of tracers (the
   reference would write the members of a GfsParticulate into GfsParticle objects), on a box with
   GFSHIP_SIDE_EXTERNAL sides (mpi_particle_numbering, :51-87, is not written) and on a box of 2^32 cells or more.
   gfship_feed_particle_create (gfs_feed_particle_read, :2435-2575): mass and volume are the GfsFunction texts of
   the keywords of the same names -- C text as in the simulation file, an expression or a { block } with a return
   -- compiled for the device of the domain with hipRTC exactly as the function of a GfsSourceParticulateVol is
   (-ffp-contract=off, the device's libm; GFSHIP_EINVAL with the compiler's messages in gfship_last_error () where
   one does not compile).  A number is a constant and compiles nothing; NULL is the constant 0 of
   gfs_feed_particle_init (:2614-2625), and an object without mass feeds nothing.  The texts may name x, y, z, t
   and the nvars variables of the table (names[q], fields[q]); a name of the table that is one of those four, or
   no C identifier, is GFSHIP_EINVAL.  Rad, Urelp ... are not variables of these functions: they are what the
   table says, or unknown to the compiler.  Destroy the object before its list.
   gfship_feed_particle_event (gfs_feed_particle_event, :2404-2418, from the position on), on the stream of the
   list: for each of the np candidates pos (x y z each, host memory; all three are kept in 2-D as well) in the
   order given, feed_particulate (:2377-2402): cell = gfs_domain_locate (pos) -- a candidate without a cell is
   dropped -- vel[c] = gfs_interpolate (cell, pos, U ...) for c < dim with the velocity of the simulation as it
   is now (vel.z = 0. in 2-D; the velx, vely, velz of the object are never evaluated, :2388-2392), mass and volume
   = the two functions at the cell (its centre for x, y, z, gfship_sim_time for t, the cell's value of every
   variable of the table), then add_particulate (:1237-1276): a candidate with mass < 1.e-20 is dropped before it
   takes an id (a NaN is not less: it joins), any other joins the END of the list with id = ++idlast, force = 0
   and pos_old = 0 until its first gfship_particle_list_event, and the forces of the list.  The new particles
   follow every particle of the list in the order of gfship_particles_download, in candidate order; their ids are
   idlast + 1 + the number of accepted candidates before them, an ordered count (never an atomic counter): the
   same from run to run.  Candidates and results stay on the device; a dropped candidate leaves a dead slot
   (gfship_particles_slots counts it, gfship_particles_count does not).  The diameter (:552) and rb (:2091) of a
   new particle are values of the device's pow, as after a volume event.  np = 0 does nothing.
   gfship_particles_set_idlast, gfship_particles_idlast: idlast of a GfsParticleList (particle_id, :1231-1234; 0
   from gfs_particle_list_init, or the integer that ends the list in the file, :1087-1090), on any list of a box.
   Nothing makes the new ids differ from those the list was created with unless idlast says so, as in the
   reference.  The getter waits for the stream of the list. */
typedef struct gfship_feed_particle gfship_feed_particle;
int  gfship_feed_particle_create (gfship_feed_particle ** feed, gfship_particles * pl,
				  const char * mass, const char * volume,
				  int nvars, const char * const * names, const gfship_field * fields);
int  gfship_feed_particle_event (gfship_feed_particle * feed, int np, const double * pos /* 3*np, host */);
void gfship_feed_particle_destroy (gfship_feed_particle * feed);
int  gfship_particles_set_idlast (gfship_particles * pl, int idlast);
int  gfship_particles_idlast (gfship_particles * pl);

/* Droplets: the connected regions of the leaves where a variable exceeds THRESHOLD = 1e-4 (src/domain.c:3564),
   across faces and through periodic sides, on a uniform box.  GFSHIP_EUNSUPPORTED on a box with
   GFSHIP_SIDE_EXTERNAL sides (unify_tag_range, src/domain.c:3662-3687, is not written) and on a box of 2^32 cells or
   more (a label is a 32-bit traversal index).  All on the stream of the domain.
   gfship_tag_droplets (gfs_domain_tag_droplets, src/domain.c:3727-3796): the leaves of `tag' receive, as doubles,
   the strictly positive index of their droplet, 0 outside; *n = the number of droplets.  The tag of a droplet is
   1 + its rank by the smallest traversal index (FTT_PRE_ORDER over the leaves) of its cells, which is what the
   flood fill, the `touch' table and the renumbering of the reference give.  The ghost cells of `tag' are left as
   they are, and the ghost cells of c are not read: the reference's fill may run along the ghost cells of a side,
   which with periodic or homogeneous Neumann ghosts joins nothing the interior does not.  c and
   tag are two fields.  Host reads: n.
   gfship_tag_droplets_time: a warm-up call, then `reps' calls between two events; *ms = milliseconds per call.
   gfship_remove_droplets (gfs_domain_remove_droplets, src/domain.c:3836-3880): the droplets of c, their sizes
   counting all their leaves (compute_droplet_size, :3805-3810); min >= 0 is the bound itself, min < 0 the
   (-1 - min)-th largest size; nothing happens unless n > 0 && -min < n (:3851); v = val on the leaves of every
   droplet with size < min (unsigned, :3812-3817), then the ghost cells of v by its boundary conditions.  c and v may
   be the same field.  Host reads: n, and the size that a negative min selects.
   GfsDropletToParticle (modules/particulatecommon.c:1163-1527), an object on a list of particulates of a uniform
   box; the refusals are those of gfship_feed_particle_create.  gfship_droplet_to_particle_create
   (gfs_droplet_to_particle_read, :1407-1467): c is the variable, min, reset and density the keywords (density is
   kept and never used, as in the reference); function is the optional GfsFunction that makes the mask instead of c
   -- NULL, a number (a constant), the name of a variable of the table (gfs_function_get_variable: that variable), or
   C text of x, y, z, t and of the names of the table, compiled with hipRTC as the functions of a GfsFeedParticle are
   (GFSHIP_EINVAL with the compiler's messages in gfship_last_error () where it does not compile) and evaluated at
   every leaf at the start of an event.  Destroy the object before its list.
   gfship_droplet_to_particle_event (gfs_droplet_to_particle_event, :1362-1404, convert_droplets, :1278-1348): the
   droplets of the mask; per droplet, over its leaves in traversal order that touch no side of the box (every side
   is a boundary, a periodic one included), sizes++, volume += h^dim*c, pos += the centre, vel += U
   (compute_droplet_properties, :1194-1229: fp64 sums in that order, bit for bit), and boundary = whether its LAST
   leaf touches a side; min as above; in tag order a droplet with boundary == 0 and 1 < sizes < min becomes a
   candidate at pos/sizes with velocity vel/sizes, cell = gfs_domain_locate (pos), volume, mass = (alpha ?
   1./alpha (cell) : 1.)*volume with alpha at the cell centres (gfship_sim_set_alpha_cell; GFSHIP_EUNSUPPORTED
   where the simulation has an alpha and no such field), pos.z = vel.z = 0 in 2-D; add_particulate (:1237-1276) as
   for gfship_feed_particle_event: the n droplets take the n slots after those in use, in tag order, and one that
   does not convert or whose mass is below 1.e-20 leaves a dead slot and takes no id.  Then c = reset on the leaves
   of every droplet with sizes < min (reset_small_fraction, :1187-1192: those on a side, of size 0 or 1, or refused
   for their mass included), and the ghost cells of c by its boundary conditions.  info may be NULL; otherwise it
   receives the number of droplets, the min used, the particles made and the cells reset (0, 0, 0 where the event
   does nothing).  Host reads: n, and the size that a negative min selects; with info, one more at the end. */
typedef struct gfship_droplet_to_particle gfship_droplet_to_particle;
typedef struct { unsigned n, min, converted, reset; } gfship_droplet_info;
int  gfship_tag_droplets (gfship_domain * dom, gfship_field c, gfship_field tag, unsigned * n);
int  gfship_tag_droplets_time (gfship_domain * dom, gfship_field c, gfship_field tag, int reps, double * ms);
int  gfship_remove_droplets (gfship_domain * dom, gfship_field c, gfship_field v, int min, double val);
int  gfship_droplet_to_particle_create (gfship_droplet_to_particle ** d, gfship_particles * pl, gfship_field c,
					int min, double reset, double density, const char * function,
					int nvars, const char * const * names, const gfship_field * fields);
int  gfship_droplet_to_particle_event (gfship_droplet_to_particle * d, gfship_droplet_info * info);
void gfship_droplet_to_particle_destroy (gfship_droplet_to_particle * d);

/* ---- one box per GPU: GfsBoundaryMpi sides (src/mpi_boundary.c:78-246) ----------------------- */

/* Either the in-library RCCL transport below (gfship_domain_comm_init: what bench.py uses), or two
   hooks of the caller for every GFSHIP_SIDE_EXTERNAL side (the tests implement them in-process and
   over gloo).  Semantics are the reference's parallel run with the
   domain parameter `overlap = 0` (src/domain.c:225,1104,1183): plain traversal order, ghost cells
   of MPI sides refreshed by every BC application, i.e. lagged by one sweep exactly like the
   periodic and MPI boundaries of the reference (send src/mpi_boundary.c:89-130, receive
   :132-222).
   exchange: fill the ghost layer of the level array `dev_ptr` (layout px, xo as in
     gfship_field_device_ptr) on external sides from the neighbour boxes' interior layer;
     kind = 0: a cell-centred variable, every external side (gfs_domain_copy_bc);
     kind = 1 + e: the face-value array fv[e] of gfs_domain_face_bc: only side e^1 is needed.
     Work must be ordered after everything already enqueued on gfship_domain_stream().
   reduce: MPI_Allreduce of vals[0..n-1] over all boxes, op = 0 sum, 1 max, 2 min
     (norms src/domain.c:2135-2166, CFL :2921). */
/* The domain parameter `overlap' of a parallel run (src/domain.c:225,682; "overlap = 0" in the
   graph parameters of the simulation file).  0 (the default here): every sweep of a relax loop in
   plain traversal order, BC application after it.  1 (the reference's default): the first
   nrelax - 1 sweeps of a relax loop in the order of gfs_traverse_and_homogeneous_bc
   (src/domain.c:1093-1125) -- the cells along the GfsBoundaryMpi sides first, side by side in
   traversal order, then the rest -- with the halo layers travelling beside the bulk of the sweep
   when the library's own communicator is used; the last sweep in plain order (src/poisson.c:1080-
   1086).  The two orders give different iterates of the same solution: a multi-box run must be
   compared with a reference run of the same setting.  No effect on a box without MPI sides. */
int  gfship_domain_set_overlap (gfship_domain * dom, int overlap);
typedef int (* gfship_exchange_fn) (void * ctx, void * dev_ptr, int level, int kind);
typedef int (* gfship_reduce_fn) (void * ctx, double * vals, int n, int op);
int  gfship_domain_set_exchange (gfship_domain * dom, gfship_exchange_fn fn, void * ctx);
int  gfship_domain_set_reduce (gfship_domain * dom, gfship_reduce_fn fn, void * ctx);
/* Optional third hook, together with the place of the box on the periodic lattice of boxes (rank r
   at (r % bx, (r / bx) % by, r / (bx by)), as for gfship_domain_comm_init below):
   gather: MPI_Allgather of `bytes' bytes of device memory per box: dev_recv + r*bytes receives what
     box r passed as dev_send; ordered after everything enqueued on gfship_domain_stream(), complete
     (or enqueued on that stream) on return.
   With it -- or with the library's own communicator -- the coarse end of a multigrid cycle (the
   levels of at most 16^3 cells per box: restrictions, relax loops with the BC application between
   their sweeps, prolongations; src/poisson.c:1131-1168) needs ONE collective instead of one halo
   exchange per sweep and level: every rank gathers the residuals of all boxes on the finest of
   those levels and runs the sweeps of every box of the lattice itself, handing the layers between
   the boxes over in device memory exactly where the reference's BC application would -- the same
   arithmetic in the same order on every rank, hence the same bits as one exchange per sweep.
   GFSHIP_NO_LATTICE_CYCLE=1 in the environment keeps one exchange per sweep. */
typedef int (* gfship_gather_fn) (void * ctx, const void * dev_send, void * dev_recv, size_t bytes);
int  gfship_domain_set_gather (gfship_domain * dom, gfship_gather_fn fn, void * ctx, int rank,
			       int nboxes, const int lattice[3]);
/* Which of the multi-box fast paths have run on this domain (for tests and benchmarks: both are
   bit-identical to the paths they replace): coarse ends of V-cycles computed for the whole lattice
   after one gather; launches of the tiled Godunov kernels with the face states beyond the MPI sides
   exchanged in one message per side (library communicator only, GFSHIP_NO_FUSED_MPI=1 disables). */
int  gfship_domain_path_counts (gfship_domain * dom, unsigned long long * lattice_cycles,
				unsigned long long * fused_mpi_launches);
/* Which branch of every switchable dispatch has run on this domain (for tests: the variants behind the
   GFSHIP_* environment switches are bit-identical, and a test that sets one needs proof that the other
   branch really ran).  Plain host-side tallies made where the kernel is chosen; nothing on the device
   knows of them.  counts[k] receives family k for k < min (n, GFSHIP_KC_COUNT).  Unless said
   otherwise a family counts launches (or sweeps / loops, where one decision covers several launches);
   the "declined" families count the times a switch alone kept a fused pass from being used. */
enum {
  GFSHIP_KC_PREDICT_SWEEP = 0,       /* predict_un_sweep_kernel, periodic box */
  GFSHIP_KC_PREDICT_SWEEP_MPI,       /* ... with the states beyond the MPI sides from the buffers */
  GFSHIP_KC_PREDICT_TILED,           /* predict_un_tiled_kernel, periodic box */
  GFSHIP_KC_PREDICT_TILED_MPI,       /* ... on a box with MPI sides */
  GFSHIP_KC_PREDICT_GENERAL,         /* face-value arrays + predict_un_kernel per component */
  GFSHIP_KC_ADVECT3_SWEEP2,          /* advect3_sweep2_kernel, periodic box */
  GFSHIP_KC_ADVECT3_SWEEP2_MPI,
  GFSHIP_KC_ADVECT3_SWEEP1,          /* advect3_sweep_kernel (GFSHIP_ADVECT_SWEEP1) */
  GFSHIP_KC_ADVECT3_TILED,           /* advect3_tiled_kernel, periodic box */
  GFSHIP_KC_ADVECT3_TILED_MPI,
  GFSHIP_KC_ADVECT1_TILED_VELOCITY,  /* advect_tiled_kernel on one velocity component */
  GFSHIP_KC_ADVECT1_TILED_TRACER,    /* advect_tiled_kernel on a tracer */
  GFSHIP_KC_ADVECT_GENERAL,          /* face-value arrays + flux kernel, one variable */
  GFSHIP_KC_CORRECTION_FUSED,        /* centred correction + coarse fill inside the advection pass */
  GFSHIP_KC_CORRECTION_DECLINED,     /* GFSHIP_NO_FUSED_CORRECTION alone kept it separate */
  GFSHIP_KC_DIVERGENCE_FUSED,        /* MAC divergence left behind by the predictor sweep */
  GFSHIP_KC_DIVERGENCE_DECLINED,     /* GFSHIP_NO_FUSED_DIVERGENCE alone kept it separate */
  GFSHIP_KC_DIVERGENCE_SEPARATE,     /* divergence kernel of the MAC projection */
  GFSHIP_KC_PROJECT_PAIRS,           /* projection update / face interpolation, two cells per thread */
  GFSHIP_KC_PROJECT_SCALAR,          /* the same launches by the one-cell kernels (GFSHIP_PC_SCALAR) */
  GFSHIP_KC_RESIDUAL_PAIRS,          /* residual (+ norm), two cells per thread */
  GFSHIP_KC_RESIDUAL_SCALAR,         /* the same launches by the one-cell kernels (GFSHIP_RN_SCALAR) */
  GFSHIP_KC_RN_BLOCKS_LIMIT,         /* value: the limit on workgroups of residual + norm last applied */
  GFSHIP_KC_RN_BLOCKS_MAX,           /* value: the largest grid residual + norm was launched with */
  GFSHIP_KC_ROWS2D,                  /* 2-D sweeps by relax_rows2d_kernel */
  GFSHIP_KC_HYPERPLANES_2D,          /* 2-D sweeps, one launch per hyperplane */
  GFSHIP_KC_DIFFUSION_PIPELINED,     /* diffusion relax loops on the pipelined tile kernels */
  GFSHIP_KC_DIFFUSION_HYPERPLANES,   /* the same loops, one launch per hyperplane */
  GFSHIP_KC_WEIGHTED_PIPELINED,      /* weighted sweeps / loops on the pipelined tile kernel */
  GFSHIP_KC_WEIGHTED_HYPERPLANES,    /* the same sweeps, one launch per hyperplane */
  GFSHIP_KC_PROLONGATION_FUSED,      /* prolongation while the level is packed */
  GFSHIP_KC_PROLONGATION_DECLINED,   /* GFSHIP_NO_FUSED_PROLONGATION alone: prolongate_kernel, then the copy */
  GFSHIP_KC_RESTRICTION_FUSED,       /* restriction while the residual is packed */
  GFSHIP_KC_RESTRICTION_DECLINED,    /* GFSHIP_NO_FUSED_RESTRICTION alone: restrict_kernel, then the copy */
  GFSHIP_KC_PROLONG_PACK_NEW,        /* patch_prolong_kernel */
  GFSHIP_KC_PROLONG_PACK_OLD,        /* prolongation inside patch_pack_kernel (GFSHIP_OLD_PROLONG_PACK) */
  GFSHIP_KC_ARM_AHEAD,               /* granule sets armed on the side stream */
  GFSHIP_KC_ARM_AHEAD_DECLINED,      /* GFSHIP_NO_ARM_AHEAD alone left the set to the loop */
  GFSHIP_KC_ARM_INLINE,              /* granule sets armed on the main stream, before the loop */
  GFSHIP_KC_PATCH_LOOP_KERNEL_ARMS,  /* 2 x 2 loops that arm the other set (GFSHIP_KERNEL_ARMING) */
  GFSHIP_KC_PATCH_LOOP_HOST_ARMS,    /* 2 x 2 loops that do not */
  GFSHIP_KC_XCD_SCOPE_ON,            /* 2 x 2 loops with XCD blocks (GFSHIP_XCD_SCOPE) */
  GFSHIP_KC_XCD_SCOPE_OFF,           /* 2 x 2 loops without */
  GFSHIP_KC_XCD_NEAR_MODE,           /* value: 1 + the GFSHIP_XCD_NEAR_MODE last used, 0 = never */
  GFSHIP_KC_XCD_PLACE_ON,            /* one-line loops of >= 8 tiles placed by XCD (GFSHIP_XCD_PLACE) */
  GFSHIP_KC_XCD_PLACE_OFF,           /* one-line loops of >= 8 tiles in ticket order */
  GFSHIP_KC_COARSE_CYCLES,           /* coarse ends of V-cycles in one launch */
  GFSHIP_KC_COARSE_THREADS,          /* value: threads of the last such launch */
  GFSHIP_KC_COARSE_END_BY_LEVEL,     /* V-cycles whose coarse end ran level by level */
  GFSHIP_KC_DIFFUSION_FACES_PIPELINED,   /* per-face diffusion relax loops on the pipelined tile kernel */
  GFSHIP_KC_DIFFUSION_FACES_HYPERPLANES, /* the same loops, one launch per hyperplane */
  GFSHIP_KC_COUNT
};
int  gfship_domain_kernel_counts (gfship_domain * dom, unsigned long long * counts, int n);
/* The same boundary served inside the library over RCCL (xGMI on one node), no hooks: the domain
   is one GfsBox of a periodic lattice of lattice[0] x lattice[1] x lattice[2] boxes, one box per
   rank / GPU, rank r at (r % bx, (r / bx) % by, r / (bx by)) (gfs_domain_split, src/domain.c:2576-2599,
   one box per PE).  Every BC application becomes: pack kernel -> ncclSend / ncclRecv of the packed
   layers in one group (MPI_Isend / MPI_Recv of sndbuf / rcvbuf, src/mpi_boundary.c:89-222) -> unpack
   kernel, on the domain's stream; norms and the CFL minimum are reduced over the boxes
   (src/domain.c:2135-2166,2921) in one collective each.  Sides facing another box must be
   GFSHIP_SIDE_EXTERNAL; a communicator takes precedence over the hooks above.
     gfship_comm_available: opens RCCL (dlopen) without creating anything: GFSHIP_OK when
       gfship_domain_comm_init can be entered on this rank -- a launcher agrees on that over its own
       channel BEFORE the collective ncclCommInitRank, so that no rank waits in it alone;
     gfship_comm_unique_id: ncclGetUniqueId (GFSHIP_UNIQUE_ID_BYTES bytes): called by one rank, the
       bytes are then given to every rank (through the launcher's own channel: a file, a TCP store);
     gfship_domain_comm_init: ncclCommInitRank on the domain's device, collective over the ranks;
     gfship_domain_comm_size: ncclCommCount (0 without a communicator);
     gfship_domain_comm_stats: messages and bytes sent so far (domain->mpi_messages, mpi_size). */
#define GFSHIP_UNIQUE_ID_BYTES 128
int  gfship_comm_available (void);
int  gfship_comm_unique_id (void * id);
int  gfship_domain_comm_init (gfship_domain * dom, const void * unique_id, int rank, int nranks,
			      const int lattice[3]);
int  gfship_domain_comm_size (gfship_domain * dom);
int  gfship_domain_comm_stats (gfship_domain * dom, unsigned long long * messages,
			       unsigned long long * bytes);
int  gfship_domain_comm_destroy (gfship_domain * dom);

/* pack the interior layer adjacent to `side` of a level array into n^(dim-1) contiguous doubles
   (first tangential axis fastest) / unpack such a buffer into the ghost layer of `side`
   (the sndbuf / rcvbuf of src/boundary.c:1240-1258,1333-1347); device pointers, asynchronous on
   the domain's stream */
int  gfship_halo_pack (gfship_domain * dom, const void * dev_ptr, int level, int side, void * dev_buf);
int  gfship_halo_unpack (gfship_domain * dom, void * dev_ptr, int level, int side, const void * dev_buf);
/* the same for several sides with one kernel launch each way: sides[q] -> dev_bufs[q] */
int  gfship_halo_pack_sides (gfship_domain * dom, const void * dev_ptr, int level, int nsides,
			     const int * sides, void * const * dev_bufs);
int  gfship_halo_unpack_sides (gfship_domain * dom, void * dev_ptr, int level, int nsides,
			       const int * sides, void * const * dev_bufs);

/* ---- statically refined quadtree / octree (coarse-fine stencils) ---------------------------- */

/* A GfsSimulation on one periodic GfsBox whose tree is refined by a GfsRefine function instead of
   `Refine <int>' (the case of test/periodic/periodic.gfs with BOX = 1, 2; quadtree for dim = 2, octree
   for dim = 3): replaces the tree of FttCell / FttOct records (src/ftt.h:134-159) by one dense
   (n + 2)^dim array per level -- n = 2^l, one ghost layer, index i + (n + 2) (j + (n + 2) k) with
   1 <= i, j, k <= n inside, j growing with y and k with z (no k in 2-D) -- and a flag per
   cell: 0 no such cell, 1 leaf, 2 refined.  `refine' is the GfsFunction of the GfsRefine object:
   a cell whose level is below refine (x, y, z) at its centre is refined (refine_maxlevel,
   src/refine.c:35-38), with the constraints of the reference: neighbours differ by one level at most
   (oct_new, src/ftt.c:45-83) and the corner rule of ftt_refine_corner (src/ftt.c:2013-2074,
   src/simulation.c:1226-1231).  The algorithms are those of gfship_sim with the fine / coarse
   branches of src/fluid.c:64-93,178-197,283-309,364-396,778-893, src/advection.c:132-180,267-343,
   398-435,513-587, src/timestep.c:118-144 (in 3-D their FTT_3D forms: interpolate_2D1, src/fluid.c:214-245,
   src/advection.c:183-249): Euler equations, centred gradients, alpha = NULL, all sides periodic,
   refinement equal across each periodic pair (else GFSHIP_EUNSUPPORTED).  Results are those of the
   reference's traversal orders: the sweeps of gfs_relax run in tree order, the face loops accumulate
   in face-traversal order.  The host checks (gfship_tree_host_check ...) touch no device and no shared
   state: they may run on any thread at any time; everything else follows the threading rule of the rest
   of the ABI: one thread per tree. */
typedef struct gfship_tree gfship_tree;
typedef double (* gfship_refine_fn) (double x, double y, double z, void * ctx);
enum { GFSHIP_TREE_P = 0, GFSHIP_TREE_PMAC, GFSHIP_TREE_U, GFSHIP_TREE_V, GFSHIP_TREE_GX, GFSHIP_TREE_GY,
       GFSHIP_TREE_GMACX, GFSHIP_TREE_GMACY, GFSHIP_TREE_UN0, GFSHIP_TREE_UN1, GFSHIP_TREE_UN2,
       GFSHIP_TREE_UN3, GFSHIP_TREE_W, GFSHIP_TREE_GZ, GFSHIP_TREE_GMACZ, GFSHIP_TREE_UN4,
       GFSHIP_TREE_UN5, GFSHIP_TREE_DIV, GFSHIP_TREE_BCVAL, GFSHIP_TREE_RES,
       GFSHIP_TREE_T0, GFSHIP_TREE_T1, GFSHIP_TREE_BCU, GFSHIP_TREE_BCV, GFSHIP_TREE_BCW,
       GFSHIP_TREE_UPREV, GFSHIP_TREE_VPREV, GFSHIP_TREE_WPREV };
/* the numbers go on: the variables of the two-way coupling on a tree (28 .. 31, see gfship_tree_particulate_field) */
enum { GFSHIP_TREE_VF = GFSHIP_TREE_WPREV + 1, GFSHIP_TREE_FX, GFSHIP_TREE_FY, GFSHIP_TREE_FZ };
/* ... and on: the variables of GfsSourceParticulateVol / ...Mass on a tree (32 .. 37, see
   gfship_tree_particulate_source_create) */
enum { GFSHIP_TREE_RAD = GFSHIP_TREE_FZ + 1, GFSHIP_TREE_URELP, GFSHIP_TREE_VRELP, GFSHIP_TREE_WRELP,
       GFSHIP_TREE_VOLSRC, GFSHIP_TREE_DMDT };
				    /* variables of a tree: P, Pmac, U, V, g, gmac, f[d].un; then the 3-D ones;
				       DIV: the result of gfship_tree_divergence / the right-hand side of
				       gfship_tree_poisson_solve; BCVAL: the values of the conditions of P, one per
				       ghost cell (at the face centres); RES: the residual of the last solve;
				       T0, T1: the tracers of gfship_tree_add_tracer; BCU, BCV, BCW: the values of the
				       conditions of U, V, W, one per ghost cell (at the face centres);
				       UPREV, VPREV, WPREV: Un, Vn, Wn of the GfsForceCoeff objects
				       (modules/particulatecommon.c:179-185), which exist once a list of
				       particulates of the tree has a force that reads a coefficient:
				       gfship_tree_download returns GFSHIP_EINVAL before (they are the library's to
				       write: gfship_tree_upload does not take them) */
int  gfship_tree_create (gfship_tree ** tree, int dim, gfship_refine_fn refine, void * ctx, int device);
/* the same with GfsBoundary sides (side[d] = GFSHIP_SIDE_PERIODIC or GFSHIP_SIDE_BOUNDARY; the ghost
   cells of a boundary are refined like the cells they touch, gfs_domain_match): such a tree carries
   the Poisson problem of a GfsPoisson simulation (poisson_run, src/simulation.c:2213-2285; the case
   of test/poisson/circle/circle.gfs) -- gfship_tree_set_bc gives the condition of P on a side
   (GFSHIP_BC_SYMMETRY by default, _DIRICHLET, _NEUMANN: src/boundary.c:45-62,253-279,336-347), its
   values are uploaded as the variable GFSHIP_TREE_BCVAL, the right-hand side as GFSHIP_TREE_DIV, and
   gfship_tree_poisson_solve is gfs_poisson_solve (src/poisson.c:1225-1269) with dia = 0: the
   homogeneous conditions between the sweeps, the conditions themselves after each correction.
   gfship_tree_start / _step run on such a tree with the default conditions (GfsBc symmetry: slip
   walls -- the normal velocity component and its face values odd, everything else even,
   src/boundary.c:45-74); with a Dirichlet or Neumann condition set: GFSHIP_EUNSUPPORTED. */
int  gfship_tree_create_sides (gfship_tree ** tree, int dim, gfship_refine_fn refine, void * ctx,
			       const int * side, int device);
int  gfship_tree_set_bc (gfship_tree * tree, int d, int kind);
int  gfship_tree_poisson_solve (gfship_tree * tree, gfship_multilevel_params * par, double dt);
void gfship_tree_destroy (gfship_tree * tree);
int  gfship_tree_depth (const gfship_tree * tree);                   /* gfs_domain_depth */
int  gfship_tree_dim (const gfship_tree * tree);
int  gfship_tree_flags (const gfship_tree * tree, int level, unsigned char * out /* (n + 2)^dim */);
int  gfship_tree_upload (gfship_tree * tree, int var, int level, const double * in /* (n + 2)^dim */);
int  gfship_tree_download (gfship_tree * tree, int var, int level, double * out);
gfship_multilevel_params * gfship_tree_projection_params (gfship_tree * tree, int approx);
int  gfship_tree_set_time (gfship_tree * tree, double end, double cfl);  /* GfsTime end, AdvectionParams cfl */
int  gfship_tree_set_next_event (gfship_tree * tree, gfship_next_event_fn fn, void * ctx); /* as gfship_sim_set_next_event */
double   gfship_tree_time (const gfship_tree * tree);
double   gfship_tree_dt (const gfship_tree * tree);
unsigned gfship_tree_iter (const gfship_tree * tree);
/* simulation_run up to its loop (src/simulation.c:458-476) and one iteration of the loop (:479-548) */
/* GfsVariableTracer [{ gradient = }] on a tree (src/variable.c:427-431): advected with the MAC
   velocities at the end of every step and by half a step at the start (gfs_advance_tracers,
   src/simulation.c:405-430,476,548; gfs_tracer_advection_diffusion src/timestep.c:1028-1055 with
   gfs_face_advection_flux src/advection.c:356-381 -- flux/FTT_CELLS towards a coarse neighbour -- and the
   gradient 0 gfs_center_gradient / 1 gfs_center_van_leer_gradient (default) through gfs_neighbor_value,
   src/fluid.c:364-396,522-561), restricted by gfs_cell_coarse_init; default (symmetry) condition on
   GfsBoundary sides.  Returns GFSHIP_TREE_T0 / _T1 (two tracers at most), to be called before
   gfship_tree_start. */
int  gfship_tree_add_tracer (gfship_tree * tree, int gradient);
/* GfsBcDirichlet / GfsBcNeumann U|V|W on a GfsBoundary side of a tree (src/boundary.c:253-279,336-360 with
   their face_* forms for the Godunov face values; GFSHIP_BC_SYMMETRY: the default GfsBc), the values per
   ghost cell in GFSHIP_TREE_BCU + c; the conditions of P of gfship_tree_set_bc apply in the time step too
   (an outflow: BcDirichlet P 0 + BcNeumann U 0).
   GfsSourceDiffusion {} U|V|W nu on a tree: the implicit solve of gfs_diffusion (src/timestep.c:735-788,
   923-949, src/poisson.c:1271-1690: coefficients with their fine-coarse forms, gfs_diffusion_rhs,
   diffusion_relax in tree order with the homogeneous conditions of the component, gfs_diffusion_cycle with
   10 nrelax sweeps on the first level), the explicit term as MAC source of the face values and in the
   CFL condition.  Quadtrees and octrees: the coefficients of the coarse side of a fine-coarse face
   (0 + w/4 + w/4 + w/4 + w/4 in 3-D) and of face_coeff_from_below are exactly w = beta dt nu on the trees
   this library builds; set_viscosity checks that of the tree once (GFSHIP_EUNSUPPORTED if a face read by
   the stencils had another coefficient).  With Dirichlet walls this is the lid-driven cavity of test/lid
   (a cube in 3-D) on a refined tree. */
int  gfship_tree_set_bc_u (gfship_tree * tree, int c, int d, int kind);
int  gfship_tree_set_viscosity (gfship_tree * tree, int c, double nu);
/* GfsSource {} U|V|W g with a constant intensity on a tree (as gfship_sim_set_source: MAC source of the face
   values, centred source of the update, acceleration scale of the CFL condition) */
int  gfship_tree_set_source (gfship_tree * tree, int c, double g);
gfship_multilevel_params * gfship_tree_diffusion_params (gfship_tree * tree, int c);
int  gfship_tree_start (gfship_tree * tree);
int  gfship_tree_step (gfship_tree * tree);
/* The cell data of a simulation file of a refined tree: what gfs_box_write puts between the braces of a GfsBox
   with `binary = 1' -- ftt_cell_write_binary (src/ftt.c:1771-1799: pre-order, children 0 .. FTT_CELLS - 1, per
   cell `guint flags' = child id | FTT_FLAG_LEAF on every leaf) and gfs_cell_write_binary (src/domain.c:3176-3207:
   a double -1., then one double per variable).  vars: GFSHIP_TREE_* (tracers included), in file order.  The
   records of the non-leaf cells hold what those cells hold: the result of the last gfs_cell_coarse_init.
     gfship_tree_snapshot_bytes: the size of the image (0 on error); builds and caches the offset tables;
     gfship_tree_snapshot_write: builds the image on the device and copies it into host_buf;
     gfship_tree_snapshot_read: cell_read_binary + gfs_cell_read_binary (src/ftt.c:1913-1975, src/domain.c:3227-3250)
       into a tree of the same refinement; `bytes' must be gfship_tree_snapshot_bytes; fails if a child id
       (GFSHIP_EINVAL), a leaf bit or a solid fraction (GFSHIP_EUNSUPPORTED) is not that of this tree;
     gfship_tree_restart: GfsTime { t = i = } of the file; with i > 0 gfship_tree_start takes the branch
       time.i > 0 of simulation_run (src/simulation.c:456-476): conditions, gfs_cell_coarse_init, the time step
       and gfs_update_gradients (src/timestep.c:305-322) -- no projection, no half step of the tracers. */
size_t gfship_tree_snapshot_bytes (const gfship_tree * tree, int nvars);
int  gfship_tree_snapshot_write (gfship_tree * tree, int nvars, const int * vars, void * host_buf, size_t bytes);
int  gfship_tree_snapshot_read (gfship_tree * tree, int nvars, const int * vars, const void * host_buf, size_t bytes);
int  gfship_tree_restart (gfship_tree * tree, double t, unsigned i);
/* the derived variable `Divergence' (gfs_divergence, src/fluid.c:2357-2376, with
   gfs_face_interpolated_value_generic :2200-2221) of the leaves into GFSHIP_TREE_DIV */
int  gfship_tree_divergence (gfship_tree * tree);
/* host-side self-check of the plans of a tree, needs no device (CPU tests): for every level the relax
   loop of nrelax sweeps is run on the host (a) as the reference's program -- ghost copies, the cells in
   tree order through the stencil code that walks the tree --, (b) through the compiled stencils by
   dependency level, each level backwards, (c) through the plan of the whole loop, each level
   backwards; stats[0] = cell updates, [1] = dependency levels sweep after sweep, [2] = levels of the
   loop plans, [3] = number of values that differ between (a), (b), (c): 0 for valid plans */
int  gfship_tree_host_check (int dim, gfship_refine_fn refine, void * ctx, const int * side,
			     unsigned nrelax, long long stats[4]);
/* the same for the diffusion relax (diffusion_relax, src/poisson.c:1471-1498) with the coefficients of
   gfs_diffusion_coefficients for the face weight w > 0 (the homogeneous conditions of U): for every level
   (a) the reference's program with the coefficients computed in the reference's order for this w, (b) the
   plan of the whole loop, (c) its flow plan with the kernel's timing, both with w on every face as the
   device runs them.  stats[0] = cell updates, [1] = levels of the loop plans, [2] = faces whose coefficient
   is not w (negative: - that number - 1 when the tree would be refused), [3] = values that differ: 0 for
   valid plans, [4] = hazards of the flow plans, [5] = levels without a flow plan */
int  gfship_tree_host_check_diffusion (int dim, gfship_refine_fn refine, void * ctx, const int * side,
				       unsigned nrelax, double w, long long stats[6]);
/* lab: FNV-1a-64 digests of every array a device tree of these arguments uploads (the members of each element, no
   padding; each array preceded by its length as 64 bits), with the GFSHIP_* switches of the moment: out[0] the
   flags, the tables and the lists of leaves, non-leaf cells and ghost leaves; [1] the sweep plans of all levels;
   [2] their loop plans for nrelax sweeps with the homogeneous conditions of P; [3] the flow plans of those (an
   absent one hashed as such); [4] the face sets.  Needs no device */
int  gfship_tree_host_plan_digest (int dim, gfship_refine_fn refine, void * ctx, const int * side,
				   unsigned nrelax, unsigned long long out[5]);
/* diagnostics: the cells of the sweep of gfs_relax on `level' (the cells of the level and the
   coarser leaves) and the number of dependency levels its tree order leaves on the device */
int  gfship_tree_sweep_levels (const gfship_tree * tree, int level, int * ncells, int * nlevels);

/* ---- point sampling and Lagrangian tracers on a tree ------------------------------------------ */

/* GfsOutputLocation on a tree (src/output.c:1182-1199): ftt_cell_locate (src/ftt.c:1535-1574: inclusive box
   bounds, a strict `>' in the descent) down to the leaf that holds the point, then gfs_interpolate
   (src/fluid.c:2697-2710): the corner values of gfs_cell_corner_value (:3081-3101) through
   gfs_cell_corner_interpolator (:3015-3069) with the coarser and deeper neighbours of cell_corner_neighbor
   (:2813-2846) and the T-junctions of t_junction_interpolator (:2879-2923), then gfs_interpolate_from_corners
   (:2640-2683) with the position and the size of the leaf.  The contract of gfship_field_interpolate: pos = 3*np
   doubles, out = 0 and inside = 0 for a point outside the box, no GFS_NODATA branches.  var: any GFSHIP_TREE_*.
   The interpolators of the corners that touch a change of level are walked once on the host, in the reference's
   order of operations, when the first sampler call or the first list of the tree needs them; the device sums
   weight * value in that order.
   Ghost cells: the sampler reads the ghost cells of the leaves of every level and writes nothing.  gfship_tree_start
   and gfship_tree_step leave them current for P, U, V, W and the tracers (the last gfs_domain_bc of the step);
   gfship_tree_upload leaves what the caller uploaded, ghost layer included: the caller of a sampler after an
   upload gives the ghost values it wants read. */
int  gfship_tree_interpolate (gfship_tree * tree, int var, int np, const double * pos,
			      double * out, unsigned char * inside);
/* the size of those tables: stats[0] = corners of leaves (leaves * 2^dim), [1] = corners that read the table
   (the others take the arithmetic of the uniform box), [2] = (cell, weight) entries, [3] = bytes on the device,
   [4] = the longest interpolator (at most 7 in 2-D, 29 in 3-D: GfsInterpolator, src/fluid.h) */
int  gfship_tree_sampler_stats (gfship_tree * tree, long long stats[5]);
/* a GfsParticleList of GfsParticle on a tree (modules/particulatecommon.c:1022-1093).  On such a list
   gfship_particle_list_event is gfs_particle_list_event (:980-1015): remove_particles_not_in_domain (:955-969),
   gfs_particle_event (src/particle.c:31-44) with the RK2 of gfs_domain_advect_point (src/domain.c:2764-2788) on
   the tree's U, V(, W) and gfship_tree_dt, then gfs_particle_bc (:3375-3395): boundarycell (:3151-3186) marches
   over the ftt_cell_face neighbours, whatever their level, to the side the particle left through; a periodic
   side puts it back (periodic_bc_particle, :3189-3214), a GfsBoundary side takes it off the list.  The velocity
   is read as gfship_tree_interpolate reads it (call the event after gfship_tree_start / _step).
   gfship_particles_count, _slots, _download, _download_old, _sort, _set_sort_interval and _destroy work on such a
   list (destroy it before its tree); everything of particulates, forces, coupling and migration returns
   GFSHIP_EUNSUPPORTED on a list made by this call. */
int  gfship_particles_create_tree (gfship_particles ** pl, gfship_tree * tree, int np,
				   const double * pos, const unsigned * id);
/* a GfsParticleList of GfsParticulate on a tree: gfship_particles_create_tree, then what
   gfship_particles_set_particulate does (vel = 3*np doubles, mass and volume np doubles; the diameter of
   compute_drag_force, modules/particulatecommon.c:549, and rb of distance_normalization, :2091, from the host's
   pow; force = 0).  On such a list gfship_particles_set_forces (gfs_force_coeff_read, :166-210),
   gfship_particles_set_force_coefficient, gfship_particles_download_particulate and gfship_particle_list_event
   work as on the uniform box: gfs_particle_list_event (:980-1015) with gfs_particulate_event (:768-842) and the
   compute_*_force functions (:255-655) in the reference's order, gfs_particle_bc as for the tracers of a tree.
   The data of the fluid are those of the tree: fluid_rho = 1. (a tree has no alpha); the viscosity is the
   constant of gfship_tree_set_viscosity (tree, 0, nu) (0: no drag, 0.001 in Rep); dt = gfship_tree_dt; the t of
   a coefficient function = gfship_tree_time; gravity = the argument of gfship_particles_set_forces.
   gfs_center_gradient (src/fluid.c:434-475) of Du/Dt (:297-300) and of vorticity_vector (:142-164) is taken at
   the leaf that holds the particle: next to a change of level through gfs_neighbor_value (:364-396) -- a coarser
   neighbour at x = 3/2 with interpolate_1D1 / interpolate_2D1 (:171-245) in the coarse cell, a neighbour with
   children at x = 3/4 with the mean of the children on the face (:64-93).
   Un, Vn, Wn (store_domain_previous_vel, :99-113) are the variables GFSHIP_TREE_UPREV, _VPREV, _WPREV of the
   tree: the copy of U, V, W on the leaves of every level, then the default GfsBc of a scalar on the ghost leaves
   (the value of the cell a ghost of a GfsBoundary side touches, the periodic image elsewhere).  Stored by
   gfship_particles_set_forces when any force but GfsForceBuoy is listed and after every event of a list with a
   GfsForceInertial.
   gfship_particles_set_particulate, the coupling calls, gfship_particles_set_kernel, _set_migrate and
   _record_size keep returning GFSHIP_EUNSUPPORTED on every list of a tree (the coupling of a tree has calls of its
   own: gfship_tree_particulate_field ... below). */
int  gfship_particulates_create_tree (gfship_particles ** pl, gfship_tree * tree, int np,
				      const double * pos, const unsigned * id,
				      const double * vel, const double * mass, const double * volume);

/* ---- two-way coupling on a tree (modules/particulatecommon.c:1927-2228) ------------------------ */

/* GfsParticulateField and GfsSourceParticulate on a refined quadtree / octree, on a list made by
   gfship_particulates_create_tree (GFSHIP_EUNSUPPORTED on a list of tracers and on a list of a box; the calls of the
   uniform box, gfship_particulate_field ..., keep refusing a list of a tree).  One GfsParticulateField and one
   GfsSourceParticulate per tree: their variables are GFSHIP_TREE_VF and GFSHIP_TREE_FX, _FY, _FZ (<list>_Fx ...,
   :2300-2312; no _FZ on a quadtree), allocated zeroed -- every level, ghost cells included -- by the first call
   that needs them, gfship_tree_upload among them; before that gfship_tree_download returns GFSHIP_EINVAL, after it
   download, gfship_tree_interpolate and the snapshot calls take them like any variable.  As on the box every sum is
   the reference's in list order, bit for bit, whatever the storage order (gfship_particles_sort): the contributions
   are records keyed (leaf << 32 | list position), leaf = the index of the leaf in the concatenated levels,
   radix-sorted and added serially per leaf, never with atomics.
   gfship_tree_particulate_field: particulate_field_event (:1934-1957).  var = GFSHIP_TREE_VF, reset on the interior
   leaves of every level, then v[leaf] += volume/ftt_cell_volume (leaf) for every particle on the list that
   ftt_cell_locate finds a leaf for, cellvol = h*h[*h], h = 1/(1 << level of the leaf).
   gfship_tree_particles_forces_on_fluid: compute_forces_onfluid (:753-765, :2199-2206); the contract of
   gfship_particles_forces_on_fluid with the fluid data of gfship_particulates_create_tree (the gradients at a
   change of level included).
   gfship_tree_particles_set_kernel: as gfship_particles_set_kernel; the function is compiled for the tree's device.
   A kernel whose record slots exceed a chunk (2^22) is refused, GFSHIP_EUNSUPPORTED.  The slots of a particle:
   the sum, over the levels l that hold interior leaves, of min (floor (2 rho_l/h_l) + 2, 2^l)^dim with h_l = 2^-l,
   rho_l = rkernel + (h_l/2) sqrt (dim): the stride of the box on a uniform tree.
   gfship_tree_particles_spread_forces: :2208-2222 into GFSHIP_TREE_FX ...: reset on the interior leaves of every level
   (ghost cells keep what they hold: 0 unless uploaded), then per particle in list order the two pruned traversals
   of ftt_cell_traverse_condition (src/ftt.c:948-986) over the tree itself: the root passes cond_kernel (:2126-2156,
   with the centre and the half size of the cell at hand, whatever its level) or nothing is visited; a cell that
   passes is visited if it is a leaf, and sends the descent into its children 0 .. FTT_CELLS - 1 otherwise.
   correction = sum K (q) cellvol (leaf)/sum cellvol (leaf) in traversal order, and where correction > 1.e-10
   F_c[leaf] -= force_c/liq_rho/cellvol (leaf)*K (q)/correction with liq_rho = 1. (a tree has no alpha).
   gfship_tree_source_particulate_event: source_particulate_event (:2177-2228), the two calls above in turn. */
int  gfship_tree_particulate_field (gfship_particles * pl, int var);
int  gfship_tree_particles_forces_on_fluid (gfship_particles * pl);
int  gfship_tree_particles_set_kernel (gfship_particles * pl, double rkernel, const char * function);
int  gfship_tree_particles_spread_forces (gfship_particles * pl);
int  gfship_tree_source_particulate_event (gfship_particles * pl);
/* GfsSourceParticulate in the time step of a tree (as gfship_sim_set_source_fields).  on != 0: U, V(, W) take the
   velocity source of GFSHIP_TREE_FX ... (allocated here if need be): the centred value is F_c of the leaf
   (source_particulate_centered_value, :2067-2079), the MAC value gfs_face_interpolated_value_generic
   (src/fluid.c:2232-2253) of F_c on the positive face of component c (source_particulate_value, :2029-2065) -- the
   neighbour a leaf of the same level, a coarser leaf (gfs_neighbor_value, :364-396), a cell with children (the mean
   of the children's face values) or a ghost cell, whose F is read as it is: neither the reference's event nor this
   library applies a boundary condition to these variables.  First term of every sum, 0. + F-term +
   GfsSourceDiffusion + GfsSource (v->sources is visited last-read first), in the face values of the advection, the
   centred update and the acceleration scale of gfs_domain_cfl.  Read at every use; 0 removes it.  Before or after
   gfship_tree_start.
   gfship_tree_mac_source: the sum gfs_variable_mac_source (src/source.c:38-59) gives on the leaves for component c,
   without the constant of gfship_tree_set_source (the counterpart of gfship_variable_mac_source), into var_out =
   GFSHIP_TREE_RES or GFSHIP_TREE_DIV (GFSHIP_EINVAL otherwise). */
int  gfship_tree_set_source_fields (gfship_tree * tree, int on);
int  gfship_tree_mac_source (gfship_tree * tree, int c, int var_out);

/* ---- the particles themselves change, on a tree (modules/particulatecommon.c:2734-3047) -------- */

/* GfsSourceParticulateVol and GfsSourceParticulateMass on a refined quadtree / octree, on a list made by
   gfship_particulates_create_tree (GFSHIP_EUNSUPPORTED on a list of tracers and on a list of a box;
   gfship_particulate_source_create keeps refusing a list of a tree and gfship_particulate_source_set_fields a
   handle made here).  The variables of the two classes are GFSHIP_TREE_RAD, _URELP, _VRELP, _WRELP (Rad, Urelp ...,
   :2785-2793; no _WRELP on a quadtree: GFSHIP_EINVAL), GFSHIP_TREE_VOLSRC (volsource, :2797-2803) and GFSHIP_TREE_DMDT
   (dmdtvariable, :2954-2960), allocated zeroed -- every level, ghost cells included -- by the first call that needs
   them, gfship_tree_upload among them; before that gfship_tree_download returns GFSHIP_EINVAL, after it download,
   gfship_tree_interpolate and the snapshot calls take them like any variable.
   gfship_tree_particulate_source_create: kind, function and NULL as for gfship_particulate_source_create; the
   function is compiled for the device of the tree (-ffp-contract=off).  vars[q] is the GFSHIP_TREE_* variable the
   name names[q] reads at the leaf.  A name that is one of Rad, Urelp, Vrelp, Wrelp, x, y, z, t or no C identifier, and
   a variable the tree does not have, are GFSHIP_EINVAL; an entry that is _RAD, _URELP, _VRELP, _WRELP, _VOLSRC or
   _DMDT is GFSHIP_EUNSUPPORTED: it would read what the walk is writing.
   gfship_tree_particulate_source_set_fields: each argument is its designated variable or -1 (not written): rad =
   GFSHIP_TREE_RAD, urel[c] = GFSHIP_TREE_URELP + c (urel[2] is -1 on a quadtree), deposit = GFSHIP_TREE_VOLSRC
   for a volume source and GFSHIP_TREE_DMDT for a mass source; anything else is GFSHIP_EINVAL.  With all five at -1
   the event sorts nothing.
   gfship_particulate_source_event, _time_event and _destroy work on such a handle (it knows what made it); the dt
   is gfship_tree_dt, t is gfship_tree_time.  Per event, on the stream of the tree:
   the reset of the deposit, which the reference does NOT do on the whole tree: both events pass max_depth = 1 to
   gfs_domain_cell_traverse (:2844, :3004) and ftt_cell_traverse stops below level 1 (src/ftt.c:696, :745).  For a
   volume the interior cells of levels 0 and 1 are zeroed (FTT_TRAVERSE_ALL), for a mass the interior LEAVES of levels
   0 and 1 (FTT_TRAVERSE_LEAFS: none on a tree whose leaves are all deeper).  Every other cell keeps what it held and
   deposit[cell] += source (:2830, :2989) adds onto it, event after event.  (The box path resets every level / every
   leaf: a known deviation)
   Then for every particle in list order (update_vol, :2806-2832; update_mass, :2964-2991): cell = gfs_domain_locate
   (pos, -1), the leaf whatever its level; Rad[cell] = pow (3.0*volume/4.0/M_PI, 1./3.); Urelp ...[cell] =
   gfs_interpolate (cell, pos, U ...) - vel with the corner interpolators of gfship_tree_interpolate; source = the
   function at the cell -- the particle's own Rad and Urelp ..., x, y, z = ftt_cell_pos of the leaf (dyadic, of its
   level), t, any other name = its variable at the leaf; volume (mass) += source*dt; deposit[cell] += source.  A
   leaf is left with the value it held plus the sources of its particles added left to right in list order, bit for
   bit, whatever the storage order (gfship_particles_sort), and with Rad, Urelp ... of its last particle in list
   order: records keyed (leaf << 32 | list position), leaf = the index of the leaf in the concatenated levels,
   radix-sorted and added serially per leaf, never with atomics.  Leaves without a particle, cells with children and
   ghost cells keep what they held (but levels 0 and 1 of a volume's deposit).  A particle without a leaf -- off the
   list, or outside a GfsBoundary side -- is skipped as on the box (the reference would dereference NULL).  pow: as on
   the box.  Destroy the source before its list, and the list before its tree. */
int  gfship_tree_particulate_source_create (gfship_particulate_source ** src, gfship_particles * pl, int kind,
					    const char * function, int nvars, const char * const * names,
					    const int * vars);
int  gfship_tree_particulate_source_set_fields (gfship_particulate_source * src, int rad, const int urel[3],
						int deposit);

/* GfsFeedParticle (modules/particulatecommon.c:2375-2647) on a refined quadtree / octree, on a list made by
   gfship_particulates_create_tree (GFSHIP_EUNSUPPORTED on a list of tracers of a tree and on a list of a box;
   gfship_feed_particle_create, gfship_particles_set_idlast and gfship_particles_idlast keep refusing a list of a
   tree).
   gfship_tree_feed_particle_create (gfs_feed_particle_read, :2435-2575): mass, volume and NULL as for
   gfship_feed_particle_create -- a number, C text (an expression or a { block } with a return) or NULL, the constant
   0 -- compiled for the device of the tree with the text and the options of the function of
   gfship_tree_particulate_source_create (-ffp-contract=off, the device's libm), without Rad, Urelp ...: those are what
   the table says, or unknown to the compiler.  vars[q] is the GFSHIP_TREE_* variable the name names[q] reads at the
   leaf.  A name that is x, y, z or t, a name given twice or a name that is no C identifier, and a variable the tree
   does not have now (GFSHIP_TREE_W on a quadtree, a tracer that was not added, a variable no call has allocated
   yet), are GFSHIP_EINVAL; a text that does not compile is GFSHIP_EINVAL with the compiler's messages in
   gfship_last_error (), as on the box.
   gfship_feed_particle_event and gfship_feed_particle_destroy work on such a handle (it knows what made it).  Per
   event, on the stream of the tree, for each of the np candidates in the order given, feed_particulate (:2377-2402):
   cell = gfs_domain_locate (pos, -1), the leaf whatever its level.  The position is not wrapped: a candidate outside a
   periodic side has no cell, exactly like one outside a GfsBoundary side, and is dropped; one exactly on a side of
   the box (a coordinate of 0.5 or -0.5) is inside (ftt_cell_locate tests with >).  vel[c] = gfs_interpolate (cell,
   pos, U ...) for c < dim (vel.z = 0. in 2-D) as gfship_tree_interpolate reads it, ghost cells included, the bits of
   Urelp + vel of a source: call the event after gfship_tree_start / _step, or after an upload that gives the ghosts.
   mass and volume = the two functions at the leaf: x, y, z = ftt_cell_pos of the leaf (dyadic, of its level), t =
   gfship_tree_time, any other name = its variable at the leaf.  Then add_particulate (:1237-1276) as on the box: a
   candidate with mass < 1.e-20 is dropped before it takes an id (a NaN is not less: it joins), any other joins the END
   of the list with id = ++idlast, force = 0 and pos_old = 0, in candidate order; the ids are an ordered count
   (never an atomic counter), the same from run to run.  The np candidates take the np slots after those in use; a
   dropped candidate leaves a dead slot (gfship_particles_slots counts it, gfship_particles_count does not, the
   next gfship_particles_sort moves it behind the live ones).  All three coordinates of a candidate are kept on a
   quadtree as well; gfship_particles_download returns z = 0 there.  The arrays of the list, of its forces, of its
   coupling and of its sources follow a list that has grown; nothing waits for the device but such a growth.  A list
   that would hold 2^31 slots or more is GFSHIP_ENOMEM.  The diameter (:552) and rb (:2091) of a new particle are
   values of the device's pow, as on the box.  np = 0 does nothing.
   gfship_tree_particles_set_idlast (idlast >= 0, else GFSHIP_EINVAL), gfship_tree_particles_idlast: idlast of the
   GfsParticleList (particle_id, :1231-1234; 0 from gfs_particle_list_init) of any list of a tree, tracers included;
   GFSHIP_EUNSUPPORTED on a list of a box.  The getter waits for the stream of the tree.
   Destroy the feed before its list, and the list before its tree. */
int  gfship_tree_feed_particle_create (gfship_feed_particle ** feed, gfship_particles * pl,
				       const char * mass, const char * volume,
				       int nvars, const char * const * names, const int * vars);
int  gfship_tree_particles_set_idlast (gfship_particles * pl, int idlast);
int  gfship_tree_particles_idlast (gfship_particles * pl);

/* ---- droplets on a tree (src/domain.c:3564-3880, modules/particulatecommon.c:1163-1527) -------- */

/* gfs_domain_tag_droplets, gfs_domain_remove_droplets and GfsDropletToParticle on a refined quadtree / octree
   (DESIGN.md 11.41).  c_var, v_var and the variables of a table are GFSHIP_TREE_* variables the tree has now
   (GFSHIP_EINVAL otherwise).  The tags go to GFSHIP_TREE_TAG, a variable of the library (gfship_tree_upload does not
   take it) allocated zeroed -- every level, ghost cells included -- by the first call that needs it; before that
   gfship_tree_download returns GFSHIP_EINVAL.
   gfship_tree_tag_droplets (gfs_domain_tag_droplets, src/domain.c:3727-3796, with tag_new_fraction_region and
   tag_cell_fraction, :3566-3615): the leaves of GFSHIP_TREE_TAG receive, as doubles, the index of their droplet, 0
   outside; every other cell keeps what it held; *n = the number of droplets.  On a tree the fill is directed: from a
   fine leaf it always steps into the coarser leaf beside it (:3578-3581), from the coarse leaf k it steps into the
   fine leaves only if c > 1e-4 on the cell N of the level of k that holds them (:3577: the test is made on N, with the
   value c holds on that cell with children -- what gfship_tree_upload gave that level, or what the step's
   coarse init left).  The tag of a leaf is 1 + the rank, among the seeds, of the smallest traversal index (FTT_PRE_ORDER
   over the leaves) of a leaf from which a directed path inside the mask reaches it; then the periodic sides join
   the regions of the fill (match_periodic_bc, touching_regions, :3620-3711) and the final tag is 1 + the rank by the
   smallest such label.  As on the box the fill does not step into the ghost cells of a side; on a tree the
   reference's route through the ghost cells of a periodic side may also pass a gate, through the image of N, where
   the interior gate is shut.  Integer atomics only: the same tags from run to run.
   gfship_tree_tag_droplets_time: a warm-up call, then `reps' calls between two events; *ms = milliseconds per call.
   gfship_tree_remove_droplets (gfs_domain_remove_droplets, :3836-3880): sizes count the leaves of a droplet whatever
   their level (compute_droplet_size, :3805-3810), min as for gfship_remove_droplets, v_var = val on the LEAVES of every
   droplet with size < min (:3812-3817; the cells with children keep their values), then the ghost cells of v_var
   as those of a tracer: the periodic image, and on a GfsBoundary side the default GfsBc of a scalar.  The conditions
   a variable has of its own on such a side (those of gfship_tree_set_bc for P, of gfship_tree_set_bc_u for U, V, W)
   are NOT applied: for such a v_var the caller restores its ghost cells.  The same holds for c_var in the event of a
   GfsDropletToParticle.
   gfship_tree_droplet_to_particle_create (gfs_droplet_to_particle_read, modules/particulatecommon.c:1407-1467) on a
   list made by gfship_particulates_create_tree (GFSHIP_EUNSUPPORTED on a list of tracers of a tree and on a list of
   a box; gfship_droplet_to_particle_create keeps refusing a list of a tree): c_var, min, reset, density and function
   as for gfship_droplet_to_particle_create; the function is compiled as those of gfship_tree_feed_particle_create
   and the refusals of the table are the same.  A function that is the name of a variable of the table is that
   variable; any other is evaluated at EVERY cell of every level, cells with children included (compute_v, :1357-1390,
   FTT_TRAVERSE_ALL: x, y, z = ftt_cell_pos of that cell, a name = its variable at that cell), and the gates read those
   values.
   gfship_droplet_to_particle_event and _destroy work on such a handle (it knows what made it).  Per event, on the
   stream of the tree (compute_droplet_properties, :1194-1229; convert_droplets, :1278-1348): over the leaves of a
   droplet in traversal order that touch no side, sizes++ whatever the level, volume += pow (h, dim)*c with h the size of
   the leaf, pos += ftt_cell_pos, vel += U ...; boundary = whether its last leaf touches a side; the position and
   velocity are the sums over sizes, cell = gfs_domain_locate (pos, -1), the leaf whatever its level (a droplet whose
   centre lies outside the box is skipped); a tree has no alpha: mass = 1.*volume; then add_particulate and the slots
   as for gfship_droplet_to_particle_event.  c_var = reset on the leaves of every droplet with sizes < min, then its
   ghost cells.  The host reads n, the size a negative min selects, and with info one more word.
   Destroy the object before its list, and the list before its tree. */
enum { GFSHIP_TREE_TAG = GFSHIP_TREE_DMDT + 1 };
int  gfship_tree_tag_droplets (gfship_tree * tree, int c_var, unsigned * n);
int  gfship_tree_tag_droplets_time (gfship_tree * tree, int c_var, int reps, double * ms);
int  gfship_tree_remove_droplets (gfship_tree * tree, int c_var, int v_var, int min, double val);
int  gfship_tree_droplet_to_particle_create (gfship_droplet_to_particle ** d, gfship_particles * pl, int c_var,
					     int min, double reset, double density, const char * function,
					     int nvars, const char * const * names, const int * vars);
/* A test aid, not the device path: the droplet plan of a tree (the same plan_droplets the device uploads) and the
   closed form of the fill on the host, without a device, in the order of the steps of tree_droplets.hip (symmetric
   contacts, one-way contacts, periodic pairs), so that the CPU suite pins the plan on the literal fill.  c holds
   ncell values, every cell of the levels 0, 1 ... one after the other ((2^l + 2)^dim each); tags receives one tag per
   interior leaf in traversal order, *n the number of droplets; counts: the contacts between leaves, those with a gate,
   the periodic pairs */
int  gfship_tree_host_tag_droplets (int dim, gfship_refine_fn refine, void * ctx, const int * side, long long ncell,
				    const double * c, long long nleaves, unsigned * tags, unsigned * n,
				    long long counts[3]);

/* ---- instrumentation -------------------------------------------------------------------- */

/* time (HIP events on the domain's stream) of `reps` back-to-back sweeps of gfship_relax on
   `level`, in milliseconds per sweep; used by bench.py for the roofline entry */
int  gfship_time_relax (gfship_domain * dom, unsigned d, int level, gfship_field u,
			gfship_field rhs, gfship_field dia, int reps, double * ms_per_sweep);

/* the same for a whole relax loop of `nrelax` sweeps with the homogeneous BC between them
   (src/poisson.c:1070-1089): milliseconds per loop of the sweep kernel(s) alone (pack / unpack of
   the level and the re-arming memsets are outside the timed region); *fused is set to 1 when the
   sweeps ran pipelined in one launch */
int  gfship_time_relax_loop (gfship_domain * dom, int level, gfship_field u, gfship_field rhs,
			     gfship_field dia, unsigned nrelax, int reps, double * ms_per_loop,
			     int * fused);

/* the same, and in *ms_inclusive the time of everything such a loop costs inside a V-cycle: BC
   kernel, copy into the skewed layout, arming of the hand-off granules, the sweeps, the ghost planes
   of the last BC application, copy back (HIP events on the domain's stream around all of it) */
int  gfship_time_relax_loop_inclusive (gfship_domain * dom, int level, gfship_field u, gfship_field rhs,
				       gfship_field dia, unsigned nrelax, int reps,
				       double * ms_per_loop, int * fused, double * ms_inclusive);

#ifdef __cplusplus
}
#endif
#endif /* GFSHIP_H */
