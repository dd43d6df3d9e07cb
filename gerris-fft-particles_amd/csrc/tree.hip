// tree.hip -- the reference's time step on a statically refined quadtree (2-D) or octree (3-D) in
// one periodic box (the coarse-fine stencils; the case of test/periodic/periodic.gfs
// with BOX = 1, 2 and its 3-D analogues).
//
// How the tree algorithms of the reference map onto the device:
//  * cell loops whose result does not depend on the order (src/ftt.c:689-926 traversals of leaves,
//    of the non-leaf cells of a level ...) are one thread per entry of a list built once on the host;
//  * face loops that scatter into both cells of a face (ftt_face_traverse, src/ftt.c:2152-2215:
//    MAC velocities, pressure correction, fluxes) are split into a kernel that computes one number
//    per face and a kernel in which every cell gathers the numbers of its faces IN THE ORDER the
//    reference's traversal visits them -- the same floating-point sums, no atomics;
//  * the Gauss-Seidel sweep of gfs_relax visits the cells of a level and the coarser leaves in tree
//    order (src/poisson.c:604-632): the planner (tree_plan.hip, plain host code) derives, from the very
//    stencil code the kernels run (tree.hpp with a recording reader), which cells each cell reads, and groups
//    the cells of the sweep into dependency levels; one workgroup then runs a whole relax loop (nrelax sweeps with
//    the periodic copies between them, src/poisson.c:1070-1089), level after level, barrier between
//    -- by default as a dataflow program of fixed-format micro-operations (tree_flow.hpp, t_relax_flow),
//    else from the tapes of the compiled stencils (t_relax_nodes_pf, t_relax_tape) or by the code that
//    walks the tree (t_relax_loop).
// The 2-D refined cases are small (10^4 - 10^5 cells): this path is about the reference's results on
// a tree, not about bandwidth; the uniform 3-D path of the other files is the one that is benchmarked.
//
// Restated here: src/poisson.c:998-1269 (cycle, solve), src/timestep.c:36-187,356-444,498-530,560-596,
// 644-717,872-921,976-1016, src/advection.c:27-99,132-180,267-343,398-435,513-587,
// src/fluid.c:1843-1864,2310-2324, src/domain.c:2239-2288,2824-2923, src/simulation.c:432-557,
// 1569-1633.  The tree itself, its lists and every plan are made by tree_plan.hip (tree_plan.hpp has the types):
// this file uploads them (one `upload' per type) and runs them.
#include "gfship_internal.hpp"
#include "cell_loop.hpp"
#include "tree_plan.hpp"
#include "tree_tape.hpp"
#include "tree_particles.hpp"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>

using namespace gfship;
using namespace gfship::tree;

namespace {

enum { V_P, V_PMAC, V_U /* 3 */, V_G = V_U + 3 /* 3 */, V_GM = V_G + 3 /* 3 */, V_UN = V_GM + 3 /* 6 */,
       V_FV = V_UN + 6 /* 6 */, V_DIV = V_FV + 6, V_RES, V_DP, V_BCVAL, V_T /* 2: GfsVariableTracer */,
       V_BCU = V_T + 2 /* 3: the values of the conditions of U, V, W per ghost cell */,
       V_DRHS = V_BCU + 3 /* right-hand side of the implicit diffusion */, V_NVAR };
#define TREE_MAXTRACERS 2

// the variables of the C ABI (GFSHIP_TREE_*) -> storage
const int abi_var[] = { V_P, V_PMAC, V_U, V_U + 1, V_G, V_G + 1, V_GM, V_GM + 1, V_UN, V_UN + 1, V_UN + 2,
			V_UN + 3, V_U + 2, V_G + 2, V_GM + 2, V_UN + 4, V_UN + 5, V_DIV, V_BCVAL, V_RES,
			V_T, V_T + 1, V_BCU, V_BCU + 1, V_BCU + 2 };
const int abi_nvar = sizeof (abi_var)/sizeof (abi_var[0]);

struct P3 { double * p[3]; };       // the components of a vector
struct P6 { double * p[6]; };       // a number per direction

// The plans of tree_plan.hpp on the device: pointers and sizes, plus only the host data that is read again later

struct FaceSet {            // FacePlan
  int nfaces = 0;
  FaceRec * faces = nullptr;
  int * inc_off = nullptr, * inc = nullptr;
  double * fval = nullptr;            // one number per face
};

struct FlowPlan {           // FlowProgram, and the working copies of the loop
  int nlev = 0, nct = 0, npos = 0, width = FLOW_WIDTH;
  FlowRec * rec = nullptr;
  int * lev_off = nullptr, * gidx = nullptr;
  double * ct = nullptr;
  double * up = nullptr, * rp = nullptr;   // the values and the right-hand side in the order of the plan
};

struct Sweep {              // SweepPlan
  int ncells = 0, nlev = 0, nghosts = 0, nchunks = 0;
  Cell * cells = nullptr;
  int * lev_off = nullptr, * ti = nullptr, * tv = nullptr, * cell_off = nullptr, * chunk = nullptr;
  Ghost * ghosts = nullptr;
  double * td = nullptr;
  bool taped = false;
  SweepPlan h;              // what plan_loop reads for another nrelax (cells, lev_off and chunk are dropped once uploaded)
  struct Loop {             // LoopPlan: nothing of it is needed on the host once it is uploaded
    unsigned nrelax = 0;
    int nnodes = 0, nlev = 0, nchunks = 0;
    int * ti = nullptr, * tv = nullptr, * node_off = nullptr, * node_g = nullptr, * chunk = nullptr;
    double * td = nullptr;
    int * desc = nullptr, * rec = nullptr;
    double sg[6] = { 0., 0., 0., 0., 0., 0. };
    FlowPlan * flow = nullptr;        // nullptr: not expressible, or not uploaded
  } loop;
  // the loops of the diffusion solves (10 nrelax sweeps on the first level, the conditions of U, V, W)
  Loop dloop[6];
  int dloop_next = 0;
};

struct DevReader {
  const double * p;
  __device__ inline double operator() (const Topo & T, Cell c) const { return p[T.gi (c)]; }
};

} // namespace

// the tree on the host (H, ncell, hflag, the tables, hleaves, side, has_boundary: TreePlan, whose lists of non-leaf
// cells and of ghost leaves are dropped once uploaded) and what the device holds of it
struct gfship_tree : TreePlan {
  int device = 0;
  gfship::Switches sw;                            // the GFSHIP_* environment switches, read by gfship_tree_create
  hipStream_t stream = nullptr;
  Topo D;
  unsigned char * dflag = nullptr;
  int * d_nbtab = nullptr, * d_child0 = nullptr;
  unsigned char * d_cmask = nullptr, * d_idtab = nullptr;
  double * var[V_NVAR] = {};
  int nleaves = 0;
  Cell * leaves = nullptr;                        // device: interior leaves in traversal order
  int nnonleaf[GFSHIP_MAXLEVEL + 1] = {};
  Cell * nonleaf[GFSHIP_MAXLEVEL + 1] = {};       // device: interior non-leaf cells of a level
  Ghost * ghost_leaves = nullptr; int nghost_leaves = 0;
  Sweep sweep[GFSHIP_MAXLEVEL + 1];
  FaceSet fs[4];                                  // 0: FTT_XYZ, 1 + c: the faces normal to c
  double * d_red = nullptr;                       // reductions: [0] max bits / min bits, [1..3] sums
  double * h_red = nullptr;                       // pinned
  gfship_multilevel_params projection_params, approx_projection_params;
  double cfl = 0.8, dt = 0., t = 0., end = DBL_MAX, tnext = 0.;
  unsigned iter = 0;
  gfship_next_event_fn next_event = nullptr; void * next_event_ctx = nullptr;
  int bc_p[6] = { 0, 0, 0, 0, 0, 0 };             // condition of P on a GfsBoundary side (GFSHIP_BC_*)
  bool tape_attr_set = false;                     // dynamic-LDS limit of t_relax_tape raised on this device
  int ntracers = 0, tracer_gradient[TREE_MAXTRACERS] = { 1, 1 };   // GfsVariableTracer: 0 centred, 1 van Leer
  // conditions of U, V, W on GfsBoundary sides (GFSHIP_BC_SYMMETRY: the default GfsBc) with their values in
  // V_BCU + c; GfsSourceDiffusion {} U|V|W nu with its GfsMultilevelParams
  int bc_u[3][6] = {};
  double visc[3] = { 0., 0., 0. };
  gfship_multilevel_params diffusion_params[3];
  double src[3] = { 0., 0., 0. };   // GfsSource {} U|V|W g: constant intensities
  int diffusion_exact = -1;         // octrees: every diffusion coefficient the stencils read is w (-1: not checked yet)
  // the file image of the tree (gfship_tree_snapshot_*), built on first use: every interior cell (the leaves, then
  // the non-leaf cells level by level) and, per cell of the dense levels, the index of its record in the pre-order
  // of ftt_cell_write
  Cell * snap_cells = nullptr; int snap_ncells = 0;
  unsigned long long * snap_off = nullptr;
  unsigned long long snap_records = 0;
  bool restarted = false;           // gfship_tree_restart with i > 0: gfship_tree_start takes the branch time.i > 0
  // the corner interpolators of the point sampler and of the tracers (tree_particles.hip), built on first use
  void * sampler = nullptr;
  void (* sampler_free) (void *) = nullptr;
  // Un, Vn, Wn of the GfsForceCoeff objects (GFSHIP_TREE_UPREV ...): allocated when the first list of particulates
  // with such a force asks for them (tree_previous_vel)
  double * uprev[3] = {};
  // the variable of a GfsParticulateField and <list>_Fx, _Fy, _Fz of a GfsSourceParticulate (GFSHIP_TREE_VF, _FX ...):
  // allocated zeroed by the first call that needs them (tree_coupling_variable)
  double * cvar[4] = {};
  // Rad, Urelp, Vrelp, Wrelp and the deposits of GfsSourceParticulateVol / ...Mass (GFSHIP_TREE_RAD ... _DMDT), in the
  // same way (tree_source_variable)
  double * svar[6] = {};
  bool src_fields = false;          // gfship_tree_set_source_fields: U, V, W take the velocity source of _FX ...
  // gfs_domain_tag_droplets (tree_droplets.hip): the plan of the contacts of the leaves, made on first use; what that
  // file keeps on the device of it, with its work arrays; the tags (GFSHIP_TREE_TAG), allocated zeroed on first use
  std::optional<DropletPlan> droplet_plan;
  void * droplets = nullptr;
  void (* droplets_free) (void *) = nullptr;
  double * tagvar = nullptr;
};

namespace {

// ---- kernels --------------------------------------------------------------------------------

__global__ void t_copy_ghosts (const Ghost * gh, int n, double * v)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t < n) v[gh[t].g] = v[gh[t].img];
}

// symmetry (the default GfsBc, src/boundary.c:45-62) of a vector component / periodic copy: ghost = s * cell
__global__ void t_copy_ghosts_signed (const Ghost * gh, int n, double * v, Sgn6 sg)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t < n) v[gh[t].g] = sg.s[gh[t].side]*v[gh[t].img];
}

// the conditions of P on GfsBoundary sides (src/boundary.c:45-62,253-279,336-347): symmetry (scalar),
// Dirichlet 2 val - nb, Neumann nb + val h; periodic sides: the copy
__global__ void t_bc_values (const Ghost * gh, int n, double * v, const double * bcval, Sgn6 kind, int comp = -1)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Ghost G = gh[t];
  const double nb = v[G.img];
  const int k = (int) kind.s[G.side];     /* -1 periodic, else GFSHIP_BC_* */
  double x = nb;
  if (k == GFSHIP_BC_SYMMETRY && comp == G.side/2)    /* the normal component of a vector, src/boundary.c:45-51 */
    x = - nb;
  else if (k == GFSHIP_BC_DIRICHLET)
    x = 2.*bcval[G.g] - nb;
  else if (k == GFSHIP_BC_NEUMANN)
    x = nb + bcval[G.g]*(1./(1 << G.l));
  v[G.g] = x;
}

// gfs_domain_face_bc on periodic sides (src/boundary.c:1251-1258,1343-1347): the leaf ghost beyond
// side sd takes f[OPP (sd)].v of its image
// wall: 0 periodic, 1 + GFSHIP_BC_* of the variable on a GfsBoundary side (face_dirichlet src/boundary.c:270-275,
// face_neumann :349-355 with the values of the condition per ghost cell)
__global__ void t_face_bc (const Ghost * gh, int n, P6 fv, Sgn6 wall, int comp, const double * v = nullptr,
			   const double * bcval = nullptr)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Ghost G = gh[t];
  double * a = fv.p[G.side ^ 1];
  if (wall.s[G.side] == 0.) {       /* periodic side */
    a[G.g] = a[G.img];
    return;
  }
  const int kind = (int) wall.s[G.side] - 1;
  if (kind == GFSHIP_BC_DIRICHLET) {
    a[G.g] = fv.p[G.side][G.img] = bcval[G.g];
    return;
  }
  if (kind == GFSHIP_BC_NEUMANN) {
    a[G.g] = v[G.img] + bcval[G.g]*(1./(1 << G.l))/2.;
    return;
  }
  // face_symmetry, src/boundary.c:64-74 (img: the cell the ghost touches)
  double * own = fv.p[G.side];
  if (comp == G.side/2)
    a[G.g] = own[G.img] = 0.;
  else
    a[G.g] = own[G.img];
}

// gfs_get_from_below_intensive (src/fluid.c:1843-1864, mode 0) / get_from_below_2D
// (src/poisson.c:1057-1068, mode 1) on the non-leaf cells of one level
__global__ void t_from_below (Topo T, const Cell * cells, int n, double * v, int mode)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell c = cells[t];
  double val = 0., sa = 0.;
  for (int k = 0; k < T.nc (); k++) {
    const Cell ch = T.child (c, k);
    if (exists (ch)) {
      if (mode == 0) {
	val += v[T.gi (ch)]*1.;
	sa += 1.;
      }
      else
	val += v[T.gi (ch)];
    }
  }
  // get_from_below_2D: the sum; get_from_below_3D: the sum/2 (src/poisson.c:1044-1068)
  v[T.gi (c)] = mode == 0 ? val/sa : T.dim == 2 ? val : val/2.;
}

// get_from_above, src/poisson.c:1005-1042
__global__ void t_from_above (Topo T, const Cell * cells, int n, double * v)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell parent = cells[t];
  DevReader R = { v };
  const double vp = v[T.gi (parent)];
  double h[3];
  for (int c = 0; c < T.dim; c++) {
    Face f;
    f.cell = parent;
    f.d = 2*c;
    f.neighbor = T.neighbor (parent, f.d);
    Grad2 g = face_gradient (T, f, R, parent.l);
    const double g1 = g.b - g.a*vp;
    f.d = 2*c + 1;
    f.neighbor = T.neighbor (parent, f.d);
    g = face_gradient (T, f, R, parent.l);
    const double g2 = g.b - g.a*vp;
    h[c] = (g1 - g2)/2.;
  }
  for (int k = 0; k < T.nc (); k++) {
    const Cell ch = T.child (parent, k);
    if (exists (ch)) {
      const double px = (k & 1) ? 0.25 : -0.25, py = (k & 2) ? -0.25 : 0.25,
	pz = (k & 4) ? -0.25 : 0.25;                 /* ftt_cell_relative_pos */
      double x = vp;
      x += px*h[0];
      x += py*h[1];
      if (T.dim == 3)
	x += pz*h[2];
      v[T.gi (ch)] = x;
    }
  }
}

// relax_loop, src/poisson.c:1070-1089, of one level: one workgroup, the cells of a sweep by
// dependency level
__global__ void __launch_bounds__(1024)
t_relax_loop (Topo T, const Cell * cells, const int * lev_off, int nlev, const Ghost * gh, int ngh,
	      double * u, const double * rhs, unsigned nrelax, double omega, int max_level, Sgn6 sg,
	      int op = 0, double w = 1.)
{
  DevReader R = { u };
  for (int t = threadIdx.x; t < ngh; t += blockDim.x)
    u[gh[t].g] = sg.s[gh[t].side]*u[gh[t].img];
  __syncthreads ();
  for (unsigned s = 0; s < nrelax; s++) {
    for (int L = 0; L < nlev; L++) {
      const int a = lev_off[L], b = lev_off[L + 1];
      for (int t = a + threadIdx.x; t < b; t += blockDim.x) {
	const Cell c = cells[t];
	const int g = T.gi (c);
	u[g] = op == 0 ? relax_cell (T, c, R, rhs[g], omega, max_level) :
	  diffusion_relax_cell (T, c, R, rhs[g], WConst { w }, max_level);
      }
      __syncthreads ();
    }
    if (s + 1 < nrelax) {
      for (int t = threadIdx.x; t < ngh; t += blockDim.x)
	u[gh[t].g] = sg.s[gh[t].side]*u[gh[t].img];
      __syncthreads ();
    }
  }
}

struct TapeCursorG {         // the same with the values read through the stream of cells (global memory)
  const int * ti; const double * td; const int * tvi; const double * u;
  __device__ inline double val () { return u[*tvi++]; }
};

#include "tree_flow.hpp"

// relax_loop (src/poisson.c:1070-1089) of one level from the compiled stencils: one workgroup; per
// chunk of a dependency level: stage the streams and gather the values (all threads), barrier,
// one thread per cell evaluates from LDS and stores the new value, barrier
__global__ void __launch_bounds__(1024)
t_relax_tape (Topo T, const Cell * cells, const int * cell_off, int ncells, const int * chunk, int nchunks,
	      const int * ti_g, const double * td_g, const int * tv_g,
	      const Ghost * gh, int ngh, double * u, const double * rhs, unsigned nrelax, double omega, Sgn6 sg)
{
  extern __shared__ double lds[];
  const int nd = T.nd (), dim = T.dim, ncd = T.ncd ();
  for (int t = threadIdx.x; t < ngh; t += blockDim.x)
    u[gh[t].g] = sg.s[gh[t].side]*u[gh[t].img];
  __syncthreads ();
  for (unsigned s = 0; s < nrelax; s++) {
    for (int k = 0; k < nchunks; k++) {
      const int c0 = chunk[k], c1 = chunk[k + 1];
      const int i0 = cell_off[3*c0], i1 = cell_off[3*c1];
      const int d0 = cell_off[3*c0 + 1], d1 = cell_off[3*c1 + 1];
      const int v0 = cell_off[3*c0 + 2], v1 = cell_off[3*c1 + 2];
      // LDS: values, then constants, then codes
      double * lv = lds, * ld = lds + (v1 - v0);
      int * li = (int *) (ld + (d1 - d0));
      for (int t = threadIdx.x; t < v1 - v0; t += blockDim.x)
	lv[t] = u[tv_g[v0 + t]];
      for (int t = threadIdx.x; t < d1 - d0; t += blockDim.x)
	ld[t] = td_g[d0 + t];
      for (int t = threadIdx.x; t < i1 - i0; t += blockDim.x)
	li[t] = ti_g[i0 + t];
      __syncthreads ();
      for (int c = c0 + threadIdx.x; c < c1; c += blockDim.x) {
	TapeCursor cur = { li + (cell_off[3*c] - i0), ld + (cell_off[3*c + 1] - d0), lv + (cell_off[3*c + 2] - v0) };
	const double self = *cur.tv++;
	double ga, gb;
	tape_cell (cur, nd, dim, ncd, ga, gb);
	const int g = T.gi (cells[c]);
	double x = 0.;
	if (ga != 0.)
	  x = dim == 2 ? (1. - omega)*self + omega*(gb - rhs[g])/ga : (gb - rhs[g])/ga;
	u[g] = x;
      }
      __syncthreads ();
    }
    if (s + 1 < nrelax) {
      for (int t = threadIdx.x; t < ngh; t += blockDim.x)
	u[gh[t].g] = sg.s[gh[t].side]*u[gh[t].img];
      __syncthreads ();
    }
  }
}

// the same for the plan of a whole relax loop (loop_plan): the nodes -- (cell, sweep) and the copies
// of the ghost cells between the sweeps -- by dependency level; the streams are laid out in node order
__global__ void __launch_bounds__(1024)
t_relax_nodes (Topo T, const int * node_g, const int * node_off, const int * chunk, int nchunks,
	       const int * ti_g, const double * td_g, const int * tv_g, double * u, const double * rhs,
	       double omega, int op = 0, double w = 1.)
{
  extern __shared__ double lds[];
  const int nd = T.nd (), dim = T.dim, ncd = T.ncd ();
  for (int k = 0; k < nchunks; k++) {
    const int c0 = chunk[k], c1 = chunk[k + 1];
    const int i0 = node_off[3*c0], i1 = node_off[3*c1];
    const int d0 = node_off[3*c0 + 1], d1 = node_off[3*c1 + 1];
    const int v0 = node_off[3*c0 + 2], v1 = node_off[3*c1 + 2];
    double * lv = lds, * ld = lds + (v1 - v0);
    int * li = (int *) (ld + (d1 - d0));
    for (int t = threadIdx.x; t < v1 - v0; t += blockDim.x)
      lv[t] = u[tv_g[v0 + t]];
    for (int t = threadIdx.x; t < d1 - d0; t += blockDim.x)
      ld[t] = td_g[d0 + t];
    for (int t = threadIdx.x; t < i1 - i0; t += blockDim.x)
      li[t] = ti_g[i0 + t];
    __syncthreads ();
    for (int c = c0 + threadIdx.x; c < c1; c += blockDim.x) {
      TapeCursor cur = { li + (node_off[3*c] - i0), ld + (node_off[3*c + 1] - d0), lv + (node_off[3*c + 2] - v0) };
      const int g = node_g[c];
      if (*cur.ti == K_GHOST)       /* homogeneous condition / periodic copy: ghost = s * cell */
	u[g] = (*cur.td)*(*cur.tv);
      else if (op == 0) {
	const double self = *cur.tv++;
	double ga, gb;
	tape_cell (cur, nd, dim, ncd, ga, gb);
	double x = 0.;
	if (ga != 0.)
	  x = dim == 2 ? (1. - omega)*self + omega*(gb - rhs[g])/ga : (gb - rhs[g])/ga;
	u[g] = x;
      }
      else {      /* diffusion_relax, src/poisson.c:1471-1498 (rhoc = 1): diffusion_relax_cell of tree.hpp */
	cur.tv++;
	double ga, gb;
	tape_cell (cur, nd, dim, ncd, ga, gb, w);
	int l = 0;
	while (g >= T.off[l + 1]) l++;
	const double h = 1./(1 << l);
	const double a = 1.*h*h;
	ga = 1. + ga/a;
	u[g] = (gb/a + rhs[g])/ga;
      }
    }
    __syncthreads ();
  }
}

// t_relax_nodes with everything that does not depend on the values loaded a chunk ahead.  A step of
// t_relax_nodes is a chain of seven dependent global round trips (chunk bounds, node offsets, gather index,
// value, node cell, right-hand side, store acknowledgement: 2.9 us); here the descriptor of the next chunk is
// loaded while this one is staged, the node record and the gather indices of the next chunk while this one is
// evaluated, its right-hand side behind the stores: what is left on the chain is the gather of the values,
// the evaluation from LDS and the acknowledgement of the stores.
#define PF_R 8      /* gather indices a thread keeps for the next chunk (chunks with more: loaded in place) */
struct I8 { int v[8]; };

__global__ void __launch_bounds__(1024)
t_relax_nodes_pf (Topo T, const int * rec_g, const int * desc_g, int nchunks,
		  const int * ti_g, const double * td_g, const int * tv_g, double * u, const double * rhs,
		  double omega, int op, double w, const int * node_g, const int * node_off)
{
  extern __shared__ double lds[];
  const int nd = T.nd (), dim = T.dim, ncd = T.ncd ();
  const int tid = threadIdx.x;
  typedef int int4v __attribute__((ext_vector_type(4)));
  I8 D = *(const I8 *) desc_g;
  int4v rec = { 0, 0, 0, 0 };
  double rhs_r = 0.;
  int idx[PF_R];
  if (D.v[0] + tid < D.v[1]) {
    rec = *(const int4v *) (rec_g + 4*(size_t) (D.v[0] + tid));
    rhs_r = rhs[rec.w];
  }
#pragma unroll
  for (int r = 0; r < PF_R; r++) {
    const int t = tid + r*1024;
    idx[r] = t < D.v[7] - D.v[6] ? tv_g[D.v[6] + t] : 0;
  }
  for (int k = 0; k < nchunks; k++) {
    const int c0 = D.v[0], c1 = D.v[1], i0 = D.v[2], i1 = D.v[3], d0 = D.v[4], d1 = D.v[5], v0 = D.v[6], v1 = D.v[7];
    double * lv = lds, * ld = lds + (v1 - v0);
    int * li = (int *) (ld + (d1 - d0));
    // ---- stage: the values (indices already here), the constants, the codes
#pragma unroll
    for (int r = 0; r < PF_R; r++) {
      const int t = tid + r*1024;
      if (t < v1 - v0) lv[t] = u[idx[r]];
    }
    for (int t = tid + PF_R*1024; t < v1 - v0; t += 1024)
      lv[t] = u[tv_g[v0 + t]];
    for (int t = tid; t < d1 - d0; t += 1024)
      ld[t] = td_g[d0 + t];
    for (int t = tid; t < i1 - i0; t += 1024)
      li[t] = ti_g[i0 + t];
    const I8 Dn = *(const I8 *) (desc_g + 8*(size_t) (k + 1));      /* zeros behind the last chunk */
    __syncthreads ();
    // ---- the loads for the next chunk that do not depend on this one's results
    int4v recn = { 0, 0, 0, 0 };
    int idxn[PF_R];
    const bool nextnode = Dn.v[0] + tid < Dn.v[1];
    if (nextnode)
      recn = *(const int4v *) (rec_g + 4*(size_t) (Dn.v[0] + tid));
#pragma unroll
    for (int r = 0; r < PF_R; r++) {
      const int t = tid + r*1024;
      idxn[r] = t < Dn.v[7] - Dn.v[6] ? tv_g[Dn.v[6] + t] : 0;
    }
    // ---- evaluate
    for (int c = c0 + tid; c < c1; c += 1024) {
      int io, dof, vo, g;
      double rh;
      if (c == c0 + tid) { io = rec.x; dof = rec.y; vo = rec.z; g = rec.w; rh = rhs_r; }
      else { io = node_off[3*c]; dof = node_off[3*c + 1]; vo = node_off[3*c + 2]; g = node_g[c]; rh = rhs[g]; }
      TapeCursor cur = { li + (io - i0), ld + (dof - d0), lv + (vo - v0) };
      if (*cur.ti == K_GHOST)       /* homogeneous condition / periodic copy: ghost = s * cell */
	u[g] = (*cur.td)*(*cur.tv);
      else if (op == 0) {
	const double self = *cur.tv++;
	double ga, gb;
	tape_cell (cur, nd, dim, ncd, ga, gb);
	double x = 0.;
	if (ga != 0.)
	  x = dim == 2 ? (1. - omega)*self + omega*(gb - rh)/ga : (gb - rh)/ga;
	u[g] = x;
      }
      else {      /* diffusion_relax, src/poisson.c:1471-1498 (rhoc = 1) */
	cur.tv++;
	double ga, gb;
	tape_cell (cur, nd, dim, ncd, ga, gb, w);
	int l = 0;
	while (g >= T.off[l + 1]) l++;
	const double h = 1./(1 << l);
	const double a = 1.*h*h;
	ga = 1. + ga/a;
	u[g] = (gb/a + rh)/ga;
      }
    }
    double rhs_n = 0.;
    if (nextnode)
      rhs_n = rhs[recn.w];
    __syncthreads ();
    D = Dn; rec = recn; rhs_r = rhs_n;
#pragma unroll
    for (int r = 0; r < PF_R; r++) idx[r] = idxn[r];
  }
}

__device__ inline void atomic_max_pos (double * addr, double v)   /* v >= 0 */
{
  atomicMax ((unsigned long long *) addr, (unsigned long long) __double_as_longlong (v));
}
__device__ inline void atomic_min_pos (double * addr, double v)
{
  atomicMin ((unsigned long long *) addr, (unsigned long long) __double_as_longlong (v));
}

// the sum / maximum / minimum of a wavefront in lane 0 (every lane of the wavefront calls these): one atomic
// per wavefront and number instead of one per cell -- 40 000 atomics on four addresses were the time of
// t_residual (80 us)
// (wave_sum and wave_min: cell_loop.hpp; its wave_max is fmax, which drops a NaN)
__device__ inline double wave_max_nan (double v)
{
  for (int o = 32; o > 0; o >>= 1) {      /* a NaN wins, as it does in atomic_max_pos (its bits are the largest) */
    const double b = __shfl_down (v, o);
    v = (v > b || v != v) ? v : b;
  }
  return v;
}
// gfs_residual on the leaves + add_norm_residual (src/domain.c:2239-2246): the maximum is exact, the
// sums are accumulated in no particular order (reported, never branched on)
__global__ void t_residual (Topo T, const Cell * cells, int n, const double * u, const double * rhs,
			    double * res, double * red)
{
  // (eight lanes per leaf, one per face, with the sums in direction order by lane 0: 74 -> 244 us -- the lanes of a
  // wavefront then walk eight different ways through the tree)
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  double r = 0., val = 0.;
  if (t < n) {
    const Cell c = cells[t];
    DevReader R = { u };
    const int g = T.gi (c);
    r = residual_cell (T, c, R, rhs[g]);
    res[g] = r;
    const double size = T.size (c);
    val = r/(1.*size*size);
  }
  const double m = wave_max_nan (fabs (val)), s1 = wave_sum (r), s2 = wave_sum (fabs (val)), s3 = wave_sum (val*val);
  if ((threadIdx.x & 63) == 0) {
    atomic_max_pos (&red[0], m);
    atomicAdd (&red[1], s1);
    atomicAdd (&red[2], s2);
    atomicAdd (&red[3], s3);
  }
}

// the same from the compiled stencils of the finest sweep (its cells are the leaves): the streams of a cell say
// which values to read -- two dependent loads each instead of the chain of loads through the tree (tree.hpp)
// that made t_residual run at the latency of its longest thread
__global__ void t_residual_tape (Topo T, const Cell * cells, const int * cell_off, int n, const int * ti_g,
				 const double * td_g, const int * tv_g, const double * u, const double * rhs,
				 double * res, double * red)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  double r = 0., val = 0.;
  if (t < n) {
    TapeCursorG cur = { ti_g + cell_off[3*t], td_g + cell_off[3*t + 1], tv_g + cell_off[3*t + 2], u };
    const double self = cur.val ();
    double ga, gb;
    tape_cell (cur, T.nd (), T.dim, T.ncd (), ga, gb);
    const int g = T.gi (cells[t]);
    r = rhs[g] - (gb - self*ga);
    res[g] = r;
    const double size = T.size (cells[t]);
    val = r/(1.*size*size);
  }
  const double m = wave_max_nan (fabs (val)), s1 = wave_sum (r), s2 = wave_sum (fabs (val)), s3 = wave_sum (val*val);
  if ((threadIdx.x & 63) == 0) {
    atomic_max_pos (&red[0], m);
    atomicAdd (&red[1], s1);
    atomicAdd (&red[2], s2);
    atomicAdd (&red[3], s3);
  }
}

__global__ void t_correct (Topo T, const Cell * cells, int n, double * u, const double * dp)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int g = T.gi (cells[t]);
  u[g] += dp[g];
}

// gfs_face_interpolated_normal_velocity, src/advection.c:549-573: the value of the face
// gfs_diffusion_rhs, src/poisson.c:1392-1451 (rhoc = 1, the face weight w of a quadtree)
__global__ void t_diffusion_rhs (Topo T, const Cell * cells, int n, const double * v, double * rhs, double w, double pbeta)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell c = cells[t];
  DevReader R = { v };
  rhs[T.gi (c)] += diffusion_rhs_cell (T, c, R, WConst { w }, pbeta);
}

// gfs_diffusion_residual (src/poisson.c:1534-1569) on the leaves + gfs_domain_norm_variable
// (src/domain.c:2197-2232: weights = cell volumes): the maximum is exact, the sums in no particular order
__global__ void t_diffusion_residual (Topo T, const Cell * cells, int n, const double * u, const double * rhs,
				      double * res, double w, double * red)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  double r = 0., vol = 0.;
  if (t < n) {
    const Cell c = cells[t];
    DevReader R = { u };
    const int g = T.gi (c);
    r = diffusion_residual_cell (T, c, R, rhs[g], WConst { w });
    res[g] = r;
    const double size = T.size (c);
    vol = T.dim == 3 ? size*size*size : size*size;
  }
  const double m = wave_max_nan (fabs (r)), s1 = wave_sum (vol*r), s2 = wave_sum (vol*fabs (r)), s3 = wave_sum (vol*r*r),
    s4 = wave_sum (vol);
  if ((threadIdx.x & 63) == 0) {
    atomic_max_pos (&red[0], m);
    atomicAdd (&red[1], s1);
    atomicAdd (&red[2], s2);
    atomicAdd (&red[3], s3);
    atomicAdd (&red[4], s4);
  }
}

__global__ void t_copy_leaves (Topo T, const Cell * cells, int n, const double * src, double * dst)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int g = T.gi (cells[t]);
  dst[g] = src[g];
}

__global__ void t_face_interp (Topo T, const FaceRec * faces, int n, P3 u, double * fval)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Face f = { faces[t].cell, faces[t].neighbor, faces[t].d };
  DevReader R = { u.p[f.d/2] };
  fval[t] = face_interpolated_value (T, f, R);
}

// the normal velocities of a leaf from the faces that touch it, in the order of the traversal:
// f[d].un of the cell of a face is set; that of its neighbour is set (same level) or gets half of
// the value (coarser neighbour, FTT_CELLS_DIRECTION = 2), after gfs_face_reset_normal_velocity
__global__ void t_gather_un (Topo T, const Cell * cells, int n, const FaceRec * faces, const int * inc_off,
			     const int * inc, const double * fval, P6 un, int dmask)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  double acc[6] = { 0., 0., 0., 0., 0., 0. };
  for (int k = inc_off[t]; k < inc_off[t + 1]; k++) {
    const int fi = inc[k] >> 1, role = inc[k] & 1;
    const FaceRec & f = faces[fi];
    const double u = fval[fi];
    if (role == 0)
      acc[f.d] = u;
    else if (f.neighbor.l == f.cell.l)
      acc[f.d ^ 1] = u;
    else
      acc[f.d ^ 1] += u*1./(1.*T.ncd ());
  }
  const int g = T.gi (cells[t]);
  for (int d = 0; d < T.nd (); d++)
    if (dmask & (1 << d))
      un.p[d][g] = acc[d];
}

// correct_normal_velocity, src/timestep.c:118-144: dp of the face
__global__ void t_face_correct (Topo T, const FaceRec * faces, int n, const double * p, double * fval)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Face f = { faces[t].cell, faces[t].neighbor, faces[t].d };
  DevReader R = { p };
  const Grad2 g = face_gradient (T, f, R, -1);
  double dp = (g.b - g.a*p[T.gi (f.cell)])/T.size (f.cell);
  if (f.d & 1)
    dp = - dp;
  dp /= 1.;
  fval[t] = dp;
}

__global__ void t_gather_correct (Topo T, const Cell * cells, int n, const FaceRec * faces,
				  const int * inc_off, const int * inc, const double * fval,
				  P6 un, P3 gv, double dt)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int g = T.gi (cells[t]);
  double gacc[3];
  for (int c = 0; c < 3; c++)
    gacc[c] = gv.p[c] ? gv.p[c][g] : 0.;
  for (int k = inc_off[t]; k < inc_off[t + 1]; k++) {
    const int fi = inc[k] >> 1, role = inc[k] & 1;
    const FaceRec & f = faces[fi];
    double dp = fval[fi];
    if (role == 0) {
      un.p[f.d][g] -= dp*dt;
      gacc[f.d/2] += dp*1.;
    }
    else {
      if (f.neighbor.l < f.cell.l)
	dp *= 1./(1.*T.nc ()/2);
      un.p[f.d ^ 1][g] -= dp*dt;
      gacc[f.d/2] += dp*1.;
    }
  }
  for (int c = 0; c < 3; c++)
    if (gv.p[c])
      gv.p[c][g] = gacc[c];
}

// gfs_normal_divergence + scale_divergence, src/fluid.c:2310-2324, src/timestep.c:181-187
__global__ void t_divergence (Topo T, const Cell * cells, int n, P6 un, double * div, double dt)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell c = cells[t];
  const int g = T.gi (c);
  double d = 0.;
  for (int e = 0; e < T.nd (); e++)
    d += ((e & 1) ? -1. : 1.)*un.p[e][g]*1.;
  d = d*T.size (c);
  div[g] = d/dt;
}

__global__ void t_scale (Topo T, const Cell * cells, int n, P3 a, double s, int mode, P3 g)
{
  // mode 0: a[c] /= 2 (scale_cell_gradients, src/timestep.c:60-90: both neighbours exist);
  // mode 1: a[c] -= g[c]*s (correct, src/timestep.c:486-496)
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int gi = T.gi (cells[t]);
  for (int c = 0; c < T.dim; c++) {
    if (mode == 0)
      a.p[c][gi] /= 2.;
    else
      a.p[c][gi] -= g.p[c][gi]*s;
  }
}

struct AdvArgs {
  const double * v, * u[3], * un[6];
  double * fv[6];
  double dt;
  int use_centered;
  int gradient;            // 0 gfs_center_gradient, 1 gfs_center_van_leer_gradient
  double visc;             // GfsSourceDiffusion on the variable: its explicit term is the MAC source (0: none)
  double gsrc;             // the intensity of a GfsSource on the variable (0: none)
  const double * fsrc;     // F_c of a GfsSourceParticulate on the velocity component fcomp (nullptr: none)
  int fcomp;
};

// source_particulate_value (modules/particulatecommon.c:2029-2065): gfs_face_interpolated_value_generic of F_c on
// the positive face of component c of the leaf -- a leaf of the same level, a coarser leaf (gfs_neighbor_value with
// interpolate_1D1 / interpolate_2D1), a cell with children (the mean of the children's face values) or a ghost,
// whose F is read as it is: no boundary condition is applied to these variables.  v->sources is visited last-read
// first: this is the first term of the sum of gfs_variable_mac_source
__device__ inline double mac_source_fields (const Topo & T, Cell cell, int c, const double * F)
{
  DevReader R = { F };
  const Face f = { cell, T.neighbor (cell, 2*c), 2*c };
  return face_interpolated_value_generic (T, f, R);
}

// transverse_term, src/advection.c:27-47
__device__ inline double transverse_term (const Topo & T, const AdvArgs & A, Cell cell, int g, double v0,
					  DevReader & R, double msize, int ct)
{
  const double vtan = A.use_centered ? A.u[ct][g] : (A.un[2*ct][g] + A.un[2*ct + 1][g])/2.;
  Face f;
  f.d = vtan > 0. ? 2*ct + 1 : 2*ct;
  f.cell = cell;
  f.neighbor = T.neighbor (cell, f.d);
  const Grad2 gf = face_gradient (T, f, R, -1);
  double gt = gf.b - gf.a*v0;
  if (vtan > 0.) gt = - gt;
  return A.dt*vtan*gt/(2.*msize);
}

// gfs_cell_advected_face_values, src/advection.c:58-99 (centred gradient, no sources)
// one thread per leaf and direction: the three directions of a leaf are independent, and each is a chain of
// dependent loads through the tree (a leaf per thread left less than one wavefront per compute unit on the
// trees of the benches: the kernel ran at the latency of the longest chain)
__global__ void t_face_values (Topo T, const Cell * cells, int n, AdvArgs A)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n*T.dim) return;
  const Cell cell = cells[t/T.dim];
  const int g = T.gi (cell);
  DevReader R = { A.v };
  const double size = T.size (cell);
  const double v0 = A.v[g];
  {
    const int c = t % T.dim;
    const double msize = size;
    const double unorm = A.use_centered ? A.dt*A.u[c][g]/msize :
      A.dt*(A.un[2*c][g] + A.un[2*c + 1][g])/(2.*msize);
    const double gr = A.gradient ? van_leer_gradient (T, cell, c, R) : center_gradient (T, cell, c, R);
    const double m1 = (1. - unorm)/2., m2 = (- 1. - unorm)/2.;
    const double vl = v0 + (m1 < 0.5 ? m1 : 0.5)*gr;
    const double vr = v0 + (m2 > -0.5 ? m2 : -0.5)*gr;
    double msrc = 0.;        /* gfs_variable_mac_source, src/source.c:38-59 */
    if (A.visc != 0. || A.gsrc != 0. || A.fsrc) {
      double sum = 0.;
      if (A.fsrc)
	sum += mac_source_fields (T, cell, A.fcomp, A.fsrc);
      if (A.visc != 0.)
	sum += source_diffusion_value (T, cell, R, A.visc);
      if (A.gsrc != 0.)
	sum += A.gsrc;
      msrc = sum;
    }
    const double src = A.dt*msrc/2.;
    double dv;
    if (T.dim == 2)
      dv = transverse_term (T, A, cell, g, v0, R, msize, (c + 1) % 2);
    else {
      // orthogonal[c] = { {Y, Z}, {X, Z}, {X, Y} }
      const int o0 = c == 0 ? 1 : 0, o1 = c == 2 ? 1 : 2;
      dv =  transverse_term (T, A, cell, g, v0, R, msize, o0);
      dv += transverse_term (T, A, cell, g, v0, R, msize, o1);
    }
    A.fv[2*c][g]     = vl + src - dv;
    A.fv[2*c + 1][g] = vr + src - dv;
  }
}

struct UpwindArgs { const double * u[3], * un[6], * fv[6]; };

// interpolate_1D1 of src/advection.c:132-180 (the assigned values of s2: see oracle/go_tree.c)
__device__ inline double adv_interpolate_1D1 (const Topo & T, const UpwindArgs & A, Cell cell, int dright,
					      int dup, double x)
{
  const int dleft = dright ^ 1;
  Cell nb = T.neighbor (cell, dup);
  if (exists (nb) && T.interior (nb)) {
    double s2 = T.leaf (nb) ? 1. : 0.5;
    const double s1 = 1.;
    const double v1 = A.fv[dleft][T.gi (cell)];
    double v2;
    if (T.leaf (nb))
      v2 = A.fv[dleft][T.gi (nb)];
    else {
      // ftt_cell_child_corner: the child of nb in the corner (dleft, opposite of dup)
      nb = T.child_corner (nb, dleft, dup ^ 1, -1);
      if (exists (nb))
	v2 = A.fv[dleft][T.gi (nb)];
      else
	s2 = v2 = 0.;
    }
    return s2 > 0. ? (v2*(s1 - 1. + 2.*x) + v1*(s2 + 1. - 2.*x))/(s1 + s2) : v1;
  }
  return A.fv[dleft][T.gi (cell)];
}

// interpolate_2D1 of src/advection.c:183-249 (3-D)
__device__ inline double adv_interpolate_2D1 (const Topo & T, const UpwindArgs & A, Cell cell, int dright,
					      int d1, int d2, double x, double y)
{
  double x1 = 0., y1 = 1.;
  double x2 = 1., y2 = 0.;
  double v1, v2;
  const int dleft = dright ^ 1;
  const double v0 = A.fv[dleft][T.gi (cell)];
  Cell n1 = T.neighbor (cell, d1);
  if (exists (n1) && T.interior (n1)) {
    if (!T.leaf (n1)) {
      n1 = T.child_corner (n1, dright ^ 1, d1 ^ 1, d2);
      if (exists (n1)) {
	v1 = A.fv[dleft][T.gi (n1)];
	x1 = 1./4.;
	y1 = 3./4.;
      }
      else
	v1 = v0;
    }
    else
      v1 = A.fv[dleft][T.gi (n1)];
  }
  else
    v1 = v0;
  Cell n2 = T.neighbor (cell, d2);
  if (exists (n2) && T.interior (n2)) {
    if (!T.leaf (n2)) {
      n2 = T.child_corner (n2, dright ^ 1, d2 ^ 1, d1);
      if (exists (n2)) {
	v2 = A.fv[dleft][T.gi (n2)];
	x2 = 3./4.;
	y2 = 1./4.;
      }
      else
	v2 = v0;
    }
    else
      v2 = A.fv[dleft][T.gi (n2)];
  }
  else
    v2 = v0;
  return ((v1 - v0)*(x*y2 - x2*y) + (v2 - v0)*(x1*y - x*y1))/(x1*y2 - x2*y1) + v0;
}

// gfs_face_upwinded_value, src/advection.c:267-343
__device__ inline double face_upwinded_value (const Topo & T, const UpwindArgs & A, const Face & face,
					      int centered)
{
  double un;
  if (centered) {
    DevReader R = { A.u[face.d/2] };
    un = face_interpolated_value (T, face, R);
  }
  else
    un = A.un[face.d][T.gi (face.cell)];
  if (face.d & 1)
    un = - un;
  const double fc = A.fv[face.d][T.gi (face.cell)];
  if (!fine_coarse (face)) {
    const double fn = A.fv[face.d ^ 1][T.gi (face.neighbor)];
    return un > 0. ? fc : un < 0. ? fn : (fc + fn)/2.;
  }
  if (un > 0.)
    return fc;
  const int id = T.id (face.cell);
  const double vcoarse = T.dim == 2 ?
    adv_interpolate_1D1 (T, A, face.neighbor, face.d, perpendicular (face.d, id), 1./4.) :
    adv_interpolate_2D1 (T, A, face.neighbor, face.d, perpendicular3 (face.d, id, 0),
			 perpendicular3 (face.d, id, 1), 1./4., 1./4.);
  if (un == 0.)
    return (fc + vcoarse)/2.;
  return vcoarse;
}

// gfs_face_advected_normal_velocity, src/advection.c:513-539: the value of the face
__global__ void t_face_advected_un (Topo T, const FaceRec * faces, int n, UpwindArgs A, double * fval)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Face f = { faces[t].cell, faces[t].neighbor, faces[t].d };
  fval[t] = face_upwinded_value (T, A, f, 1);
}

// gfs_face_velocity_advection_flux, src/advection.c:398-435: the flux of the face
// gm == nullptr: gfs_face_advection_flux, src/advection.c:356-381 (a tracer)
__global__ void t_face_flux (Topo T, const FaceRec * faces, int n, UpwindArgs A, const double * gm,
			     double dt, double * fval)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Face f = { faces[t].cell, faces[t].neighbor, faces[t].d };
  DevReader G = { gm };
  double flux;
  if (gm) {
    flux = 1.*A.un[f.d][T.gi (f.cell)]*dt/T.size (f.cell);
    flux *= face_upwinded_value (T, A, f, 0) - face_interpolated_value (T, f, G)*dt/2.;
  }
  else
    flux = 1.*A.un[f.d][T.gi (f.cell)]*dt*face_upwinded_value (T, A, f, 0)/T.size (f.cell);
  if (f.d & 1)
    flux = - flux;
  fval[t] = flux;
}

// the flux sums of a leaf in traversal order, gfs_advection_update (src/advection.c:784-819) and
// add_pressure_gradient (src/timestep.c:809-812)
__global__ void t_gather_flux (Topo T, const Cell * cells, int n, const FaceRec * faces,
			       const int * inc_off, const int * inc, const double * fval,
			       double * v, const double * g, double dt, double gsrc = 0.,
			       const double * fsrc = nullptr)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  double f = 0.;
  for (int k = inc_off[t]; k < inc_off[t + 1]; k++) {
    const int fi = inc[k] >> 1, role = inc[k] & 1;
    const FaceRec & F = faces[fi];
    const double flux = fval[fi];
    if (role == 0)
      f -= flux;
    else if (F.neighbor.l == F.cell.l)
      f += flux;
    else
      f += flux/T.nc ();
  }
  const int gi = T.gi (cells[t]);
  double x = v[gi];
  x += f/1.;
  if (g)
    x -= g[gi]*dt;
  if (gsrc != 0. || fsrc) {     /* gfs_domain_variable_centered_sources, src/source.c:62-108 */
    double sum = 0;
    if (fsrc)             /* source_particulate_centered_value, modules/particulatecommon.c:2067-2079 */
      sum += fsrc[gi];
    if (gsrc != 0.)       /* a GfsSource */
      sum += gsrc;
    x += dt*sum;
  }
  v[gi] = x;
}

// gfs_divergence, src/fluid.c:2357-2376: the derived variable `Divergence' of the leaves
__global__ void t_divergence_centered (Topo T, const Cell * cells, int n, P3 u, double * div)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell cell = cells[t];
  double d = 0.;
  Face f;
  f.cell = cell;
  for (f.d = 0; f.d < T.nd (); f.d++) {
    f.neighbor = T.neighbor (cell, f.d);
    if (exists (f.neighbor)) {
      DevReader R = { u.p[f.d/2] };
      d += 1.*((f.d & 1) ? -1. : 1.)*face_interpolated_value_generic (T, f, R);
    }
  }
  div[T.gi (cell)] = d/(1.*T.size (cell));
}

// gfs_domain_cfl, src/domain.c:2824-2923: the minimum of (length/|u|)^2 over faces and cells
__global__ void t_cfl_faces (Topo T, const FaceRec * faces, int n, P6 un, double * red)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  double best = DBL_MAX;
  if (t < n) {
    const double u = un.p[faces[t].d][T.gi (faces[t].cell)];
    if (u != 0.) {
      const double cflu = T.size (faces[t].cell)/fabs (u);
      best = cflu*cflu;
    }
  }
  best = wave_min (best);
  if ((threadIdx.x & 63) == 0 && best != DBL_MAX)
    atomic_min_pos (red, best);
}

struct D3 { double d[3]; };
__global__ void t_cfl_cells (Topo T, const Cell * cells, int n, P3 u, double * red, D3 visc, D3 src, P3 fsrc)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  double best = DBL_MAX;
  const bool in = t < n;
  if (!in) t = 0;
  const int g = T.gi (cells[t]);
  const double length = T.size (cells[t]);
  for (int c = 0; c < T.dim; c++) {
    const double fm = 1.;
    if (in && u.p[c][g] != 0.) {
      const double cflu = length/fabs (fm*u.p[c][g]);
      best = fmin (best, cflu*cflu);
    }
    if (visc.d[c] != 0. || src.d[c] != 0. || fsrc.p[c]) {      /* p->v[c]->sources: the acceleration scale, src/domain.c:2882-2891 */
      DevReader R = { u.p[c] };
      double gs = 0.;
      if (fsrc.p[c])
	gs += mac_source_fields (T, cells[t], c, fsrc.p[c]);
      if (visc.d[c] != 0.)
	gs += source_diffusion_value (T, cells[t], R, visc.d[c]);
      if (src.d[c] != 0.)
	gs += src.d[c];
      if (in && gs != 0.) {
	const double cflg = 2.*length/fabs (fm*gs);
	best = fmin (best, cflg);
      }
    }
  }
  best = wave_min (best);
  if ((threadIdx.x & 63) == 0 && best != DBL_MAX)
    atomic_min_pos (red, best);
}

// gfs_variable_mac_source (src/source.c:38-59) of velocity component c on the leaves, without the constant of a
// GfsSource (gfship_tree_mac_source): 0. + the F-term + the source of the diffusion
__global__ void t_mac_source (Topo T, const Cell * cells, int n, int c, const double * u, const double * fsrc,
			      double visc, double * out)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell cell = cells[t];
  DevReader R = { u };
  double sum = 0.;
  if (fsrc)
    sum += mac_source_fields (T, cell, c, fsrc);
  if (visc != 0.)
    sum += source_diffusion_value (T, cell, R, visc);
  out[T.gi (cell)] = sum;
}

inline int blocks (int n) { return (n + 255)/256; }

// ---- host: the plans of tree_plan.hpp onto the device -------------------------------------------

template <class X> int to_device (const std::vector<X> & h, X ** d)
{
  *d = nullptr;       /* stays nullptr for an empty array: never dereferenced */
  if (h.empty ()) return 0;
  GFSHIP_HIP (hipMalloc ((void **) d, h.size ()*sizeof (X)));
  GFSHIP_HIP (hipMemcpy (*d, h.data (), h.size ()*sizeof (X), hipMemcpyHostToDevice));
  return 0;
}

template <class X> void release (std::vector<X> & v) { std::vector<X> ().swap (v); }

// the plan S->h; keeps of it what plan_loop reads
int upload (Sweep * S)
{
  const SweepPlan & h = S->h;
  S->ncells = (int) h.cells.size ();
  S->nlev = h.nlev;
  S->nghosts = (int) h.ghosts.size ();
  S->nchunks = (int) h.chunk.size () - 1;
  int e;
  if ((e = to_device (h.cells, &S->cells)) || (e = to_device (h.lev_off, &S->lev_off)) ||
      (e = to_device (h.ghosts, &S->ghosts)) ||
      (e = to_device (h.ti, &S->ti)) || (e = to_device (h.td, &S->td)) || (e = to_device (h.tv, &S->tv)) ||
      (e = to_device (h.cell_off, &S->cell_off)) || (e = to_device (h.chunk, &S->chunk)))
    return e;
  S->taped = true;
  release (S->h.cells); release (S->h.lev_off); release (S->h.chunk);
  return 0;
}

void flow_free (FlowPlan & F)
{
  (void) hipFree (F.rec); (void) hipFree (F.lev_off); (void) hipFree (F.ct);
  (void) hipFree (F.gidx); (void) hipFree (F.up); (void) hipFree (F.rp);
  F = FlowPlan ();
}

// false: no memory for it (the caller keeps the tape kernels)
bool upload (const FlowProgram & h, FlowPlan * F)
{
  F->nlev = h.nlev; F->nct = h.nct; F->npos = h.npos; F->width = h.width;
  if (to_device (h.rec, &F->rec) || to_device (h.lev_off, &F->lev_off) || to_device (h.ct, &F->ct) ||
      to_device (h.gidx, &F->gidx) ||
      hipMalloc ((void **) &F->up, h.gidx.size ()*sizeof (double)) != hipSuccess ||
      hipMalloc ((void **) &F->rp, h.gidx.size ()*sizeof (double)) != hipSuccess) {
    flow_free (*F);
    return false;
  }
  return true;
}

void loop_free (Sweep::Loop & P)
{
  (void) hipFree (P.ti); (void) hipFree (P.tv); (void) hipFree (P.td);
  (void) hipFree (P.node_off); (void) hipFree (P.node_g); (void) hipFree (P.chunk);
  (void) hipFree (P.desc); (void) hipFree (P.rec);
  if (P.flow) { flow_free (*P.flow); delete P.flow; }
  P = Sweep::Loop ();
}

int upload (const LoopPlan & h, Sweep::Loop * P)
{
  for (int d = 0; d < 6; d++) P->sg[d] = h.sg[d];
  P->nchunks = h.nchunks ();
  P->nnodes = h.nnodes ();
  P->nlev = h.nlev;
  int e;
  if ((e = to_device (h.ti, &P->ti)) || (e = to_device (h.td, &P->td)) || (e = to_device (h.tv, &P->tv)) ||
      (e = to_device (h.node_off, &P->node_off)) || (e = to_device (h.node_g, &P->node_g)) ||
      (e = to_device (h.chunk, &P->chunk)) || (e = to_device (h.desc, &P->desc)) || (e = to_device (h.rec, &P->rec)))
    return e;
  P->nrelax = h.nrelax;
  if (h.flow) {
    P->flow = new FlowPlan;
    if (!upload (*h.flow, P->flow)) {
      delete P->flow;
      P->flow = nullptr;
    }
  }
  return 0;
}

int upload (const FacePlan & h, FaceSet * F)
{
  F->nfaces = (int) h.faces.size ();
  int e;
  if ((e = to_device (h.faces, &F->faces)) || (e = to_device (h.inc_off, &F->inc_off)) ||
      (e = to_device (h.inc, &F->inc)))
    return e;
  GFSHIP_HIP (hipMalloc ((void **) &F->fval, std::max<size_t> (1, h.faces.size ())*sizeof (double)));
  return 0;
}

Sgn6 homogeneous_signs (const gfship_tree * tr) { return tree::homogeneous_signs (tr->side, tr->bc_p); }

// the relax loop of nrelax sweeps of level m with the conditions `signs' (those of P by default), planned and
// uploaded into `out' (S->loop by default)
int loop_plan (gfship_tree * tr, int m, unsigned nrelax, Sweep * S, Sweep::Loop * out = nullptr,
	       const Sgn6 * signs = nullptr)
{
  Sweep::Loop & P = out ? *out : S->loop;
  loop_free (P);
  LoopPlan h;
  int e = plan_loop (*tr, S->h, m, nrelax, signs ? *signs : homogeneous_signs (tr), tr->sw.flow_width,
		     tr->sw.tree_debug, h);
  return e ? e : upload (h, &P);
}

#define KCHECK() GFSHIP_HIP (hipGetLastError ())

// ---- host: the algorithms ----------------------------------------------------------------------

// gfs_domain_bc of P on the leaves of a tree with GfsBoundary sides
int bc_solution (gfship_tree * tr, double * v)
{
  if (!tr->nghost_leaves) return 0;
  Sgn6 kind;
  for (int d = 0; d < 6; d++)
    kind.s[d] = tr->side[d] == GFSHIP_SIDE_PERIODIC ? -1. : (double) tr->bc_p[d];
  t_bc_values<<<blocks (tr->nghost_leaves), 256, 0, tr->stream>>> (tr->ghost_leaves, tr->nghost_leaves, v,
      tr->var[V_BCVAL], kind);
  GFSHIP_HIP (hipGetLastError ());
  return 0;
}

int bc_leaves (gfship_tree * tr, double * v, int comp = -1)
{
  if (tr->has_boundary && comp >= 0) {      /* a vector component: symmetry on the GfsBoundary sides */
    Sgn6 sg;
    for (int d = 0; d < 6; d++)
      sg.s[d] = tr->side[d] != GFSHIP_SIDE_PERIODIC && comp == d/2 ? -1. : 1.;
    if (tr->nghost_leaves)
      t_copy_ghosts_signed<<<blocks (tr->nghost_leaves), 256, 0, tr->stream>>> (tr->ghost_leaves, tr->nghost_leaves, v, sg);
    GFSHIP_HIP (hipGetLastError ());
    return 0;
  }
  if (tr->has_boundary)      /* P and the other scalars: the conditions of P */
    return bc_solution (tr, v);
  if (tr->nghost_leaves)
    t_copy_ghosts<<<blocks (tr->nghost_leaves), 256, 0, tr->stream>>> (tr->ghost_leaves, tr->nghost_leaves, v);
  KCHECK ();
  return 0;
}

// gfs_domain_bc of velocity component c: the conditions of gfship_tree_set_bc_u (symmetry by default)
int bc_velocity (gfship_tree * tr, int c)
{
  bool plain = true;
  for (int d = 0; d < 6; d++)
    if (tr->side[d] != GFSHIP_SIDE_PERIODIC && tr->bc_u[c][d] != GFSHIP_BC_SYMMETRY) plain = false;
  if (plain || !tr->nghost_leaves)
    return bc_leaves (tr, tr->var[V_U + c], c);
  Sgn6 kind;
  for (int d = 0; d < 6; d++)
    kind.s[d] = tr->side[d] == GFSHIP_SIDE_PERIODIC ? -1. : (double) tr->bc_u[c][d];
  t_bc_values<<<blocks (tr->nghost_leaves), 256, 0, tr->stream>>> (tr->ghost_leaves, tr->nghost_leaves, tr->var[V_U + c],
      tr->var[V_BCU + c], kind, c);
  KCHECK ();
  return 0;
}

// the homogeneous conditions of velocity component c (gfs_domain_homogeneous_bc in the relax loops of its
// diffusion solve): ghost = s * cell
Sgn6 homogeneous_signs_u (const gfship_tree * tr, int c) { return tree::homogeneous_signs_u (tr->side, tr->bc_u[c], c); }

// post-order traversal of the non-leaf cells: deepest level first
// the same for several variables in one launch per level (gfs_cell_coarse_init restricts five to seven variables:
// thirty to forty launches of a few microseconds each per step otherwise)
struct PN { double * p[8]; };
__global__ void t_from_below_n (Topo T, const Cell * cells, int n, PN V, int nv)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n*nv) return;
  const Cell c = cells[t/nv];
  double * v = V.p[t % nv];
  double val = 0., sa = 0.;
  for (int k = 0; k < T.nc (); k++) {
    const Cell ch = T.child (c, k);
    if (exists (ch)) {
      val += v[T.gi (ch)]*1.;
      sa += 1.;
    }
  }
  v[T.gi (c)] = val/sa;
}

int from_below_n (gfship_tree * tr, const PN & V, int nv)
{
  for (int l = tr->H.depth - 1; l >= 0; l--)
    if (tr->nnonleaf[l]) {
      t_from_below_n<<<blocks (tr->nnonleaf[l]*nv), 256, 0, tr->stream>>> (tr->D, tr->nonleaf[l], tr->nnonleaf[l], V, nv);
      KCHECK ();
    }
  return 0;
}

int from_below (gfship_tree * tr, double * v, int mode)
{
  for (int l = tr->H.depth - 1; l >= 0; l--)
    if (tr->nnonleaf[l]) {
      t_from_below<<<blocks (tr->nnonleaf[l]), 256, 0, tr->stream>>> (tr->D, tr->nonleaf[l], tr->nnonleaf[l], v, mode);
      KCHECK ();
    }
  return 0;
}

int residual_norm (gfship_tree * tr, const double * u, const double * rhs, double * res, double dt,
		   gfship_norm * out)
{
  GFSHIP_HIP (hipMemsetAsync (tr->d_red, 0, 4*sizeof (double), tr->stream));
  {
    const Sweep & S = tr->sweep[tr->H.depth];
    if (tr->sw.tree_residual_tape && S.taped && S.ncells == tr->nleaves)
      t_residual_tape<<<blocks (S.ncells), 256, 0, tr->stream>>> (tr->D, S.cells, S.cell_off, S.ncells, S.ti, S.td, S.tv,
								   u, rhs, res, tr->d_red);
    else
      t_residual<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, u, rhs, res, tr->d_red);
  }
  KCHECK ();
  GFSHIP_HIP (hipMemcpyAsync (tr->h_red, tr->d_red, 4*sizeof (double), hipMemcpyDeviceToHost, tr->stream));
  GFSHIP_HIP (hipStreamSynchronize (tr->stream));
  // gfs_norm_update + the scaling of gfs_domain_norm_residual, src/domain.c:2264-2288
  const double w = tr->nleaves;
  dt *= dt;
  out->bias = tr->h_red[1]*dt;
  out->first = tr->h_red[2]/w*dt;
  out->second = sqrt (tr->h_red[3]/w)*dt;
  out->infty = tr->h_red[0]*dt;
  out->w = w;
  return 0;
}

// op 0: the Poisson relax on V_DP with the conditions of P; op 1: diffusion_relax with the face weight w and
// the homogeneous conditions sg of the variable being diffused
int relax_loop (gfship_tree * tr, int m, unsigned nrelax, double omega, int op = 0, double w = 1.,
		const Sgn6 * sgp = nullptr)
{
  Sweep & S = tr->sweep[m];
  const bool use_template = tr->sw.tree_template_relax;
  if (!tr->tape_attr_set) {       /* more than 64 KB of dynamic LDS needs the attribute */
    GFSHIP_HIP (hipFuncSetAttribute ((const void *) t_relax_tape, hipFuncAttributeMaxDynamicSharedMemorySize,
				     TAPE_LDS_BYTES));
    tr->tape_attr_set = true;
  }
  const Sgn6 sg = sgp ? *sgp : homogeneous_signs (tr);
  if (S.taped && !use_template && (tr->sw.tree_pipeline || op == 1)) {
    Sweep::Loop * P = &S.loop;
    if (op == 1) {
      /* the plan with these conditions and this number of sweeps, kept from an earlier solve */
      P = nullptr;
      for (Sweep::Loop & Q : S.dloop)
	if (Q.nrelax == nrelax && Q.nnodes > 0 && !memcmp (Q.sg, sg.s, sizeof (Q.sg))) P = &Q;
      if (!P) {
	P = &S.dloop[S.dloop_next];
	S.dloop_next = (S.dloop_next + 1) % 6;
	int e = loop_plan (tr, m, nrelax, &S, P, &sg);
	if (e) return e;
      }
    }
    else if (S.loop.nrelax != nrelax || memcmp (S.loop.sg, sg.s, sizeof (S.loop.sg))) {
      int e = loop_plan (tr, m, nrelax, &S);
      if (e) return e;
    }
    if (P->flow && tr->sw.tree_flow) {
      const FlowPlan & F = *P->flow;
      t_flow_pack<<<blocks (F.npos), 256, 0, tr->stream>>> (F.gidx, F.npos, tr->var[V_DP], tr->var[V_RES], F.up, F.rp);
      if (tr->H.dim == 3)
	t_relax_flow<3><<<1, F.width + 64, 0, tr->stream>>> (F.rec, F.lev_off, F.nlev, F.ct, F.nct, F.up, F.rp, F.npos, omega, op, w);
      else
	t_relax_flow<2><<<1, F.width + 64, 0, tr->stream>>> (F.rec, F.lev_off, F.nlev, F.ct, F.nct, F.up, F.rp, F.npos, omega, op, w);
      t_flow_unpack<<<blocks (F.npos), 256, 0, tr->stream>>> (F.gidx, F.npos, F.up, tr->var[V_DP]);
      KCHECK ();
      return 0;
    }
    if (!tr->sw.tree_prefetch) {
      GFSHIP_HIP (hipFuncSetAttribute ((const void *) t_relax_nodes, hipFuncAttributeMaxDynamicSharedMemorySize,
				       TAPE_LDS_BYTES));
      t_relax_nodes<<<1, 1024, TAPE_LDS_BYTES, tr->stream>>> (tr->D, P->node_g, P->node_off, P->chunk,
	  P->nchunks, P->ti, P->td, P->tv, tr->var[V_DP], tr->var[V_RES], omega, op, w);
    }
    else {
      GFSHIP_HIP (hipFuncSetAttribute ((const void *) t_relax_nodes_pf, hipFuncAttributeMaxDynamicSharedMemorySize,
				       TAPE_LDS_BYTES));
      t_relax_nodes_pf<<<1, 1024, TAPE_LDS_BYTES, tr->stream>>> (tr->D, P->rec, P->desc, P->nchunks, P->ti, P->td, P->tv,
	  tr->var[V_DP], tr->var[V_RES], omega, op, w, P->node_g, P->node_off);
    }
  }
  else if (S.taped && !use_template)
    t_relax_tape<<<1, 1024, TAPE_LDS_BYTES, tr->stream>>> (tr->D, S.cells, S.cell_off, S.ncells, S.chunk, S.nchunks,
	S.ti, S.td, S.tv, S.ghosts, S.nghosts, tr->var[V_DP], tr->var[V_RES], nrelax, omega, sg);
  else
    t_relax_loop<<<1, 1024, 0, tr->stream>>> (tr->D, S.cells, S.lev_off, S.nlev, S.ghosts, S.nghosts,
					       tr->var[V_DP], tr->var[V_RES], nrelax, omega, m, sg, op, w);
  KCHECK ();
  return 0;
}

// gfs_poisson_cycle, src/poisson.c:1105-1178 (dia = 0)
int poisson_cycle (gfship_tree * tr, gfship_multilevel_params * p, double * u, const double * rhs)
{
  int e;
  const unsigned minlevel = p->minlevel;
  if ((e = from_below (tr, tr->var[V_RES], 1))) return e;
  unsigned nrelax = p->nrelax;
  for (unsigned l = minlevel; l < p->depth; l++)
    nrelax *= p->erelax;
  // dp: the cells of the first level are reset, every other cell is written before it is read
  GFSHIP_HIP (hipMemsetAsync (tr->var[V_DP], 0, tr->ncell*sizeof (double), tr->stream));
  if ((e = relax_loop (tr, minlevel, nrelax, p->omega))) return e;
  nrelax /= p->erelax;
  for (unsigned m = minlevel + 1; m <= p->depth; m++, nrelax /= p->erelax) {
    if (tr->nnonleaf[m - 1]) {
      t_from_above<<<blocks (tr->nnonleaf[m - 1]), 256, 0, tr->stream>>> (tr->D, tr->nonleaf[m - 1], tr->nnonleaf[m - 1], tr->var[V_DP]);
      KCHECK ();
    }
    if ((e = relax_loop (tr, m, nrelax, p->omega))) return e;
  }
  t_correct<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, u, tr->var[V_DP]);
  KCHECK ();
  return bc_leaves (tr, u);
}

// gfs_poisson_solve, src/poisson.c:1225-1269
int poisson_solve (gfship_tree * tr, gfship_multilevel_params * par, double * lhs, const double * rhs, double dt)
{
  int e;
  const unsigned minlevel = par->minlevel;
  par->depth = tr->H.depth;
  par->niter = 0;
  if ((e = residual_norm (tr, lhs, rhs, tr->var[V_RES], dt, &par->residual))) return e;
  par->residual_before = par->residual;
  double res_max_before = par->residual.infty;
  while (par->niter < par->nitermin ||
	 (par->residual.infty > par->tolerance && par->niter < par->nitermax)) {
    if ((e = poisson_cycle (tr, par, lhs, rhs))) return e;
    if ((e = residual_norm (tr, lhs, rhs, tr->var[V_RES], dt, &par->residual))) return e;
    if (par->residual.infty == res_max_before)
      break;
    if (par->residual.infty > res_max_before/1.1 && par->minlevel < par->depth)
      par->minlevel++;
    res_max_before = par->residual.infty;
    par->niter++;
  }
  par->minlevel = minlevel;
  return 0;
}

P3 p3 (gfship_tree * tr, int first)
{
  P3 a;
  for (int c = 0; c < 3; c++) a.p[c] = tr->var[first + c];
  return a;
}

P6 p6 (gfship_tree * tr, int first)
{
  P6 a;
  for (int d = 0; d < 6; d++) a.p[d] = tr->var[first + d];
  return a;
}

int gather_un (gfship_tree * tr, int kind, int dmask)
{
  FaceSet & F = tr->fs[kind];
  t_gather_un<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, F.faces, F.inc_off, F.inc, F.fval,
      p6 (tr, V_UN), dmask);
  KCHECK ();
  return 0;
}

int correct_normal_velocities (gfship_tree * tr, const double * p, int gvar, double dt);

// mac_projection, src/timestep.c:356-444
int mac_projection (gfship_tree * tr, gfship_multilevel_params * par, double dt, double * p, int gvar)
{
  int e;
  const int dim = tr->H.dim;
  for (int c = 0; c < dim; c++)   /* gfs_reset_gradients on the leaves (the other cells are never read) */
    GFSHIP_HIP (hipMemsetAsync (tr->var[gvar + c], 0, tr->ncell*sizeof (double), tr->stream));
  t_divergence<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, p6 (tr, V_UN), tr->var[V_DIV], dt);
  KCHECK ();
  if ((e = poisson_solve (tr, par, p, tr->var[V_DIV], dt))) return e;
  return correct_normal_velocities (tr, p, gvar, dt);
}

// gfs_correct_normal_velocities + gfs_scale_gradients + the conditions of g: the end of mac_projection, and with
// dt = 0 (the face velocities stay as they are) gfs_update_gradients, src/timestep.c:305-322
int correct_normal_velocities (gfship_tree * tr, const double * p, int gvar, double dt)
{
  int e;
  const int dim = tr->H.dim;
  // gfs_correct_normal_velocities, src/timestep.c:163-179: FTT_XY (the x faces, then the y faces) in
  // 2-D, FTT_XYZ (one traversal) in 3-D
  for (int k = 0; k < (dim == 2 ? 2 : 1); k++) {
    FaceSet & F = tr->fs[dim == 2 ? 1 + k : 0];
    P3 gv = { { nullptr, nullptr, nullptr } };
    if (dim == 2) gv.p[k] = tr->var[gvar + k];
    else gv = p3 (tr, gvar);
    t_face_correct<<<blocks (F.nfaces), 256, 0, tr->stream>>> (tr->D, F.faces, F.nfaces, p, F.fval);
    KCHECK ();
    t_gather_correct<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, F.faces, F.inc_off, F.inc, F.fval,
	p6 (tr, V_UN), gv, dt);
    KCHECK ();
  }
  // gfs_scale_gradients, src/timestep.c:92-107
  t_scale<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, p3 (tr, gvar), 0., 0, p3 (tr, gvar));
  KCHECK ();
  for (int c = 0; c < dim; c++)
    if ((e = bc_leaves (tr, tr->var[gvar + c], c))) return e;
  return 0;
}

int correct_centered (gfship_tree * tr, int gvar, double dt)   /* src/timestep.c:498-530 */
{
  int e;
  t_scale<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, p3 (tr, V_U), dt, 1, p3 (tr, gvar));
  KCHECK ();
  for (int c = 0; c < tr->H.dim; c++)
    if ((e = bc_velocity (tr, c))) return e;
  return 0;
}

int approximate_projection (gfship_tree * tr, gfship_multilevel_params * par, double dt)
{ /* src/timestep.c:560-596 */
  int e;
  FaceSet & F = tr->fs[0];
  t_face_interp<<<blocks (F.nfaces), 256, 0, tr->stream>>> (tr->D, F.faces, F.nfaces, p3 (tr, V_U), F.fval);
  KCHECK ();
  if ((e = gather_un (tr, 0, 63))) return e;
  if ((e = mac_projection (tr, par, dt, tr->var[V_P], V_G))) return e;
  return correct_centered (tr, V_G, dt);
}

UpwindArgs upwind_args (gfship_tree * tr)
{
  UpwindArgs A;
  for (int c = 0; c < 3; c++) A.u[c] = tr->var[V_U + c];
  for (int d = 0; d < 6; d++) { A.un[d] = tr->var[V_UN + d]; A.fv[d] = tr->var[V_FV + d]; }
  return A;
}

int face_values_set (gfship_tree * tr, const double * v, double dt, int use_centered, int comp, int gradient = 0)
{ /* src/timestep.c:644-654 */
  AdvArgs A;
  A.v = v; A.dt = dt; A.use_centered = use_centered; A.gradient = gradient;
  A.visc = A.gsrc = 0.;
  A.fsrc = nullptr; A.fcomp = 0;
  for (int c = 0; c < 3; c++)
    if (v == tr->var[V_U + c]) {
      A.visc = tr->visc[c]; A.gsrc = tr->src[c];
      if (tr->src_fields && c < tr->H.dim) { A.fsrc = tr->cvar[1 + c]; A.fcomp = c; }
    }
  for (int c = 0; c < 3; c++) A.u[c] = tr->var[V_U + c];
  for (int d = 0; d < 6; d++) { A.un[d] = tr->var[V_UN + d]; A.fv[d] = tr->var[V_FV + d]; }
  t_face_values<<<blocks (tr->nleaves*tr->H.dim), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, A);
  KCHECK ();
  if (tr->nghost_leaves)
  {
    Sgn6 wall;
    int ucomp = -1;
    for (int c = 0; c < 3; c++) if (v == tr->var[V_U + c]) ucomp = c;
    for (int d = 0; d < 6; d++)
      wall.s[d] = tr->side[d] != GFSHIP_SIDE_PERIODIC ? 1. + (ucomp >= 0 ? tr->bc_u[ucomp][d] : GFSHIP_BC_SYMMETRY) : 0.;
    t_face_bc<<<blocks (tr->nghost_leaves), 256, 0, tr->stream>>> (tr->ghost_leaves, tr->nghost_leaves, p6 (tr, V_FV), wall, comp,
	v, ucomp >= 0 ? tr->var[V_BCU + ucomp] : nullptr);
  }
  KCHECK ();
  return 0;
}

// gfs_diffusion_residual + the norm of gfs_diffusion (src/timestep.c:756-760)
int diffusion_residual_norm (gfship_tree * tr, const double * u, const double * rhs, double w, gfship_norm * out)
{
  GFSHIP_HIP (hipMemsetAsync (tr->d_red, 0, 5*sizeof (double), tr->stream));
  t_diffusion_residual<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, u, rhs,
      tr->var[V_RES], w, tr->d_red);
  KCHECK ();
  GFSHIP_HIP (hipMemcpyAsync (tr->h_red, tr->d_red, 5*sizeof (double), hipMemcpyDeviceToHost, tr->stream));
  GFSHIP_HIP (hipStreamSynchronize (tr->stream));
  const double ws = tr->h_red[4];
  out->w = ws;
  out->infty = ws > 0. ? tr->h_red[0] : 0.;
  out->bias = ws > 0. ? tr->h_red[1]/ws : 0.;
  out->first = ws > 0. ? tr->h_red[2]/ws : 0.;
  out->second = ws > 0. ? sqrt (tr->h_red[3]/ws) : 0.;
  return 0;
}

// gfs_diffusion_cycle, src/poisson.c:1633-1690: the residual restricted by gfs_get_from_below_intensive,
// 10 nrelax sweeps on the first level, the homogeneous conditions of the variable in the loops
int diffusion_cycle (gfship_tree * tr, unsigned levelmin, unsigned depth, unsigned nrelax, int c, double w)
{
  int e;
  const Sgn6 sg = homogeneous_signs_u (tr, c);
  double * u = tr->var[V_U + c];
  if ((e = from_below (tr, tr->var[V_RES], 0))) return e;
  GFSHIP_HIP (hipMemsetAsync (tr->var[V_DP], 0, tr->ncell*sizeof (double), tr->stream));
  if ((e = relax_loop (tr, levelmin, 10*nrelax, 1., 1, w, &sg))) return e;
  for (unsigned m = levelmin + 1; m <= depth; m++) {
    if (tr->nnonleaf[m - 1]) {
      t_from_above<<<blocks (tr->nnonleaf[m - 1]), 256, 0, tr->stream>>> (tr->D, tr->nonleaf[m - 1], tr->nnonleaf[m - 1], tr->var[V_DP]);
      KCHECK ();
    }
    if ((e = relax_loop (tr, m, nrelax, 1., 1, w, &sg))) return e;
  }
  t_correct<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, u, tr->var[V_DP]);
  KCHECK ();
  return bc_velocity (tr, c);
}

// variable_diffusion (src/timestep.c:923-949) + gfs_diffusion (:735-788) of velocity component c; the
// right-hand side is V_DRHS.  Every face carries the weight beta dt D (face_gradient_w, WConst; octrees:
// diffusion_weights_exact)
int variable_diffusion (gfship_tree * tr, int c)
{
  int e;
  gfship_multilevel_params * par = &tr->diffusion_params[c];
  const double w = 1.*(par->beta*tr->dt)*tr->visc[c]*1./1.;      /* diffusion_coef, src/poisson.c:1280-1285 */
  double * v = tr->var[V_U + c], * rhs = tr->var[V_DRHS];
  t_diffusion_rhs<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, v, rhs, w,
      (1. - par->beta)/par->beta);
  KCHECK ();
  unsigned minlevel = par->minlevel;
  const unsigned maxlevel = tr->H.depth;
  if ((e = diffusion_residual_norm (tr, v, rhs, w, &par->residual))) return e;
  par->residual_before = par->residual;
  double res_max_before = par->residual.infty;
  par->niter = 0;
  while (par->niter < par->nitermin ||
	 (par->residual.infty > par->tolerance && par->niter < par->nitermax)) {
    if ((e = diffusion_cycle (tr, minlevel, maxlevel, par->nrelax, c, w))) return e;
    if ((e = diffusion_residual_norm (tr, v, rhs, w, &par->residual))) return e;
    if (par->residual.infty == res_max_before)
      break;
    if (par->residual.infty > res_max_before/1.1 && minlevel < maxlevel)
      minlevel++;
    res_max_before = par->residual.infty;
    par->niter++;
  }
  return 0;
}

int predicted_face_velocities (gfship_tree * tr)   /* src/timestep.c:681-717 */
{
  int e;
  for (int c = 0; c < tr->H.dim; c++) {
    if ((e = face_values_set (tr, tr->var[V_U + c], tr->dt, 1, c))) return e;
    FaceSet & F = tr->fs[1 + c];
    t_face_advected_un<<<blocks (F.nfaces), 256, 0, tr->stream>>> (tr->D, F.faces, F.nfaces, upwind_args (tr), F.fval);
    KCHECK ();
    if ((e = gather_un (tr, 1 + c, 3 << (2*c)))) return e;
  }
  return 0;
}

// gfs_centered_velocity_advection_diffusion, src/timestep.c:976-1016, with variable_sources :872-921
int centered_velocity_advection (gfship_tree * tr, int gmac, int g)
{
  int e;
  FaceSet & F = tr->fs[0];
  for (int c = 0; c < tr->H.dim; c++) {
    if ((e = face_values_set (tr, tr->var[V_U + c], tr->dt, 0, c))) return e;
    t_face_flux<<<blocks (F.nfaces), 256, 0, tr->stream>>> (tr->D, F.faces, F.nfaces, upwind_args (tr), tr->var[gmac + c], tr->dt, F.fval);
    KCHECK ();
    double * sv = tr->var[V_U + c];
    if (tr->visc[c] != 0.) {
      /* source_diffusion (v[c]): rhs = copy of v, the sources into rhs, then the implicit solve
	 (src/timestep.c:996-1007) */
      sv = tr->var[V_DRHS];
      t_copy_leaves<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, tr->var[V_U + c], sv);
      KCHECK ();
    }
    t_gather_flux<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, F.faces, F.inc_off, F.inc, F.fval,
	sv, tr->var[g + c], tr->dt, tr->src[c], tr->src_fields ? tr->cvar[1 + c] : nullptr);
    KCHECK ();
    if (tr->visc[c] != 0. && (e = variable_diffusion (tr, c))) return e;
  }
  for (int c = 0; c < tr->H.dim; c++)
    if ((e = bc_velocity (tr, c))) return e;
  return 0;
}

// a scalar with the default GfsBc on the GfsBoundary sides (symmetry, src/boundary.c:45-62: the ghost
// takes the value of the cell it touches), the periodic image elsewhere
int bc_scalar (gfship_tree * tr, double * v)
{
  if (!tr->nghost_leaves) return 0;
  Sgn6 sg;
  for (int d = 0; d < 6; d++) sg.s[d] = 1.;
  t_copy_ghosts_signed<<<blocks (tr->nghost_leaves), 256, 0, tr->stream>>> (tr->ghost_leaves, tr->nghost_leaves, v, sg);
  KCHECK ();
  return 0;
}

// gfs_tracer_advection_diffusion (src/timestep.c:1028-1055, no diffusion) with variable_sources
// :872-921: the face values with the gradient of the GfsVariableTracer, gfs_face_advection_flux, the
// update, gfs_domain_bc
int tracer_advection (gfship_tree * tr, int k, double dt)
{
  int e;
  FaceSet & F = tr->fs[0];
  double * v = tr->var[V_T + k];
  if ((e = face_values_set (tr, v, dt, 0, -1, tr->tracer_gradient[k]))) return e;
  t_face_flux<<<blocks (F.nfaces), 256, 0, tr->stream>>> (tr->D, F.faces, F.nfaces, upwind_args (tr), nullptr, dt, F.fval);
  KCHECK ();
  t_gather_flux<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, F.faces, F.inc_off, F.inc, F.fval,
      v, nullptr, dt);
  KCHECK ();
  return bc_scalar (tr, v);
}

int advance_tracers (gfship_tree * tr, double dt)   /* src/simulation.c:405-430 */
{
  int e;
  for (int k = 0; k < tr->ntracers; k++)
    if ((e = tracer_advection (tr, k, dt))) return e;
  return 0;
}

int domain_cfl (gfship_tree * tr, double * cfl)   /* src/domain.c:2899-2923 */
{
  const double big = DBL_MAX;
  GFSHIP_HIP (hipMemcpyAsync (tr->d_red, &big, sizeof (double), hipMemcpyHostToDevice, tr->stream));
  FaceSet & F = tr->fs[0];
  t_cfl_faces<<<blocks (F.nfaces), 256, 0, tr->stream>>> (tr->D, F.faces, F.nfaces, p6 (tr, V_UN), tr->d_red);
  KCHECK ();
  D3 visc = { { tr->visc[0], tr->visc[1], tr->visc[2] } }, srcs = { { tr->src[0], tr->src[1], tr->src[2] } };
  P3 fsrc = { { nullptr, nullptr, nullptr } };
  for (int c = 0; c < tr->H.dim && tr->src_fields; c++) fsrc.p[c] = tr->cvar[1 + c];
  t_cfl_cells<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, p3 (tr, V_U), tr->d_red, visc, srcs, fsrc);
  KCHECK ();
  GFSHIP_HIP (hipMemcpyAsync (tr->h_red, tr->d_red, sizeof (double), hipMemcpyDeviceToHost, tr->stream));
  GFSHIP_HIP (hipStreamSynchronize (tr->stream));
  *cfl = sqrt (tr->h_red[0]);
  return 0;
}

int set_timestep (gfship_tree * tr)   /* src/simulation.c:1569-1633; the only event time is `end' */
{
  int e;
  double c;
  if ((e = domain_cfl (tr, &c))) return e;
  const double t = tr->t;
  tr->dt = tr->cfl*c;
  double tnext = 2147483647;
  if (tr->next_event)          /* the gfs_event_next loop, src/simulation.c:1603-1610 */
    tnext = tr->next_event (tr->next_event_ctx, t, tr->iter);
  if (tr->end < tnext)
    tnext = tr->end;
  const double n = ceil ((tnext - t)/tr->dt);
  if (n > 0. && n < 2147483647) {
    tr->dt = (tnext - t)/n;
    if (n == 1.)
      tr->tnext = tnext;
    else
      tr->tnext = t + tr->dt;
  }
  else
    tr->tnext = t + tr->dt;
  if (tr->dt < 1e-9)
    tr->dt = 1e-9;
  return 0;
}

int coarse_init (gfship_tree * tr)   /* src/adaptive.c:43-58 */
{
  const int vars[] = { V_P, V_PMAC, V_U, V_U + 1, V_U + 2 };
  PN V;
  int nv = 0;
  for (int k = 0; k < 2 + tr->H.dim; k++) V.p[nv++] = tr->var[vars[k]];
  for (int k = 0; k < tr->ntracers && nv < 8; k++) V.p[nv++] = tr->var[V_T + k];
  return from_below_n (tr, V, nv);
}


// ---- the file image of the tree ------------------------------------------------------------------
// ftt_cell_write_binary (src/ftt.c:1771-1799) walks the tree in pre-order, children n = 0 .. FTT_CELLS - 1, and
// writes per cell `guint flags' = child id | FTT_FLAG_LEAF on every leaf, then gfs_cell_write_binary
// (src/domain.c:3176-3207): a double -1. (no solid fractions) and one double per variable.  On a refined tree the
// position of a record is not a closed form of the coordinates: the sizes of the subtrees are summed bottom-up, the
// offsets handed down top-down, one launch per level each, once per tree.

#define TSNAP_FLAG_LEAF 16u          /* FTT_FLAG_LEAF = 1 << 4, src/ftt.h:115 */
#define TSNAP_MAXVARS 16

struct SnapVars { double * v[TSNAP_MAXVARS]; int nvars; };

__global__ void t_snap_sub_leaves (Topo T, const Cell * cells, int n, unsigned long long * sub)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  sub[T.gi (cells[t])] = 1;
}

__global__ void t_snap_sub (Topo T, const Cell * cells, int n, unsigned long long * sub)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell c = cells[t];
  unsigned long long s = 1;
  for (int k = 0; k < T.nc (); k++) {
    const Cell ch = T.child (c, k);
    if (exists (ch))
      s += sub[T.gi (ch)];
  }
  sub[T.gi (c)] = s;
}

__global__ void t_snap_off (Topo T, const Cell * cells, int n, const unsigned long long * sub, unsigned long long * off)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell c = cells[t];
  unsigned long long o = off[T.gi (c)] + 1;
  for (int k = 0; k < T.nc (); k++) {
    const Cell ch = T.child (c, k);
    if (exists (ch)) {
      off[T.gi (ch)] = o;
      o += sub[T.gi (ch)];
    }
  }
}

// records are multiples of 4 bytes: 4-byte accesses
__device__ __forceinline__ void tsnap_put_u32 (unsigned char * p, unsigned v) { *(unsigned *) p = v; }
__device__ __forceinline__ unsigned tsnap_get_u32 (const unsigned char * p) { return *(const unsigned *) p; }
__device__ __forceinline__ void tsnap_put_f64 (unsigned char * p, double v)
{
  const unsigned long long b = (unsigned long long) __double_as_longlong (v);
  tsnap_put_u32 (p, (unsigned) b);
  tsnap_put_u32 (p + 4, (unsigned) (b >> 32));
}
__device__ __forceinline__ double tsnap_get_f64 (const unsigned char * p)
{
  const unsigned long long b = (unsigned long long) tsnap_get_u32 (p) | ((unsigned long long) tsnap_get_u32 (p + 4) << 32);
  return __longlong_as_double ((long long) b);
}

// one thread per cell of the tree
template <bool READ>
__global__ void __launch_bounds__(256)
t_snapshot (Topo T, const Cell * cells, int n, const unsigned long long * off, SnapVars V, unsigned char * image,
	    unsigned long long * err)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const Cell c = cells[t];
  const int g = T.gi (c);
  const unsigned rec = 12u + 8u*V.nvars;
  unsigned char * p = image + off[g]*rec;
  const unsigned id = c.l == 0 ? 0u : (unsigned) T.id (c);       /* the root has no FTT_FLAG_ID */
  const bool leaf = T.flag[g] == LEAF;
  if (READ) {
    // cell_read_binary (src/ftt.c:1915-1945): the child id must match; the tree of the file must be this
    // tree; no solid fractions (gfs_cell_read_binary, src/domain.c:3227-3236)
    // a sequential reader stops at the first record it cannot take: *err keeps the least 4*record + kind of
    // error (0: child id, 1: leaf bit, 2: solid fraction)
    const unsigned f = tsnap_get_u32 (p);
    if ((f & 7u) != id) atomicMin (err, 4ull*off[g]);
    else if (((f & TSNAP_FLAG_LEAF) != 0) != leaf) atomicMin (err, 4ull*off[g] + 1);
    else if (tsnap_get_f64 (p + 4) != -1.) atomicMin (err, 4ull*off[g] + 2);
    for (int v = 0; v < V.nvars; v++)
      V.v[v][g] = tsnap_get_f64 (p + 12 + 8*v);
  }
  else {
    tsnap_put_u32 (p, id | (leaf ? TSNAP_FLAG_LEAF : 0u));
    tsnap_put_f64 (p + 4, -1.);
    for (int v = 0; v < V.nvars; v++)
      tsnap_put_f64 (p + 12 + 8*v, V.v[v][g]);
  }
}

void snapshot_tables_free (gfship_tree * tr)
{
  (void) hipFree (tr->snap_cells); tr->snap_cells = nullptr;
  (void) hipFree (tr->snap_off); tr->snap_off = nullptr;
  tr->snap_ncells = 0;
  tr->snap_records = 0;
}

int snapshot_tables (gfship_tree * tr)
{
  if (tr->snap_off) return 0;
  GFSHIP_HIP (hipSetDevice (tr->device));
  const Topo & T = tr->H;
  int ncells = tr->nleaves;
  for (int l = 0; l < T.depth; l++) ncells += tr->nnonleaf[l];
  unsigned long long * sub = nullptr;
  auto fail = [&] (hipError_t e, const char * what) {
    (void) hipFree (sub);
    snapshot_tables_free (tr);
    return hip_fail (e, what, __FILE__, __LINE__);
  };
#define SNAPHIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail (e_, #call); } while (0)
  SNAPHIP (hipMalloc ((void **) &tr->snap_cells, (size_t) ncells*sizeof (Cell)));
  SNAPHIP (hipMalloc ((void **) &tr->snap_off, (size_t) tr->ncell*sizeof (unsigned long long)));
  SNAPHIP (hipMalloc ((void **) &sub, (size_t) tr->ncell*sizeof (unsigned long long)));
  SNAPHIP (hipMemsetAsync (sub, 0, (size_t) tr->ncell*sizeof (unsigned long long), tr->stream));
  SNAPHIP (hipMemsetAsync (tr->snap_off, 0, (size_t) tr->ncell*sizeof (unsigned long long), tr->stream));
  int at = 0;
  SNAPHIP (hipMemcpyAsync (tr->snap_cells, tr->leaves, (size_t) tr->nleaves*sizeof (Cell), hipMemcpyDeviceToDevice, tr->stream));
  at += tr->nleaves;
  for (int l = 0; l < T.depth; l++)
    if (tr->nnonleaf[l]) {
      SNAPHIP (hipMemcpyAsync (tr->snap_cells + at, tr->nonleaf[l], (size_t) tr->nnonleaf[l]*sizeof (Cell),
			       hipMemcpyDeviceToDevice, tr->stream));
      at += tr->nnonleaf[l];
    }
  t_snap_sub_leaves<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, sub);
  SNAPHIP (hipGetLastError ());
  for (int l = T.depth - 1; l >= 0; l--)
    if (tr->nnonleaf[l]) {
      t_snap_sub<<<blocks (tr->nnonleaf[l]), 256, 0, tr->stream>>> (tr->D, tr->nonleaf[l], tr->nnonleaf[l], sub);
      SNAPHIP (hipGetLastError ());
    }
  for (int l = 0; l < T.depth; l++)
    if (tr->nnonleaf[l]) {
      t_snap_off<<<blocks (tr->nnonleaf[l]), 256, 0, tr->stream>>> (tr->D, tr->nonleaf[l], tr->nnonleaf[l], sub, tr->snap_off);
      SNAPHIP (hipGetLastError ());
    }
  unsigned long long records = 0;
  const Cell root = root_cell (T);
  SNAPHIP (hipMemcpyAsync (&records, sub + T.gi (root), sizeof (records), hipMemcpyDeviceToHost, tr->stream));
  SNAPHIP (hipStreamSynchronize (tr->stream));
#undef SNAPHIP
  (void) hipFree (sub);
  if (records != (unsigned long long) ncells) {      /* every interior cell is in exactly one list */
    snapshot_tables_free (tr);
    set_error ("gfship_tree_snapshot: %llu records for %d cells", records, ncells);
    return GFSHIP_EINVAL;
  }
  tr->snap_ncells = ncells;
  tr->snap_records = records;
  return 0;
}

int snapshot_vars (gfship_tree * tr, int nvars, const int * vars, SnapVars * V)
{
  GFSHIP_CHECK (tr && (vars || nvars == 0), GFSHIP_EINVAL, "gfship_tree_snapshot: null argument");
  GFSHIP_CHECK (nvars >= 0 && nvars <= TSNAP_MAXVARS, GFSHIP_EINVAL, "at most %d variables", TSNAP_MAXVARS);
  V->nvars = nvars;
  for (int v = 0; v < nvars; v++) {
    if (vars[v] >= GFSHIP_TREE_VF && vars[v] <= GFSHIP_TREE_FZ && tr->cvar[vars[v] - GFSHIP_TREE_VF]) {
      V->v[v] = tr->cvar[vars[v] - GFSHIP_TREE_VF];
      continue;
    }
    if (vars[v] >= GFSHIP_TREE_RAD && vars[v] <= GFSHIP_TREE_DMDT && tr->svar[vars[v] - GFSHIP_TREE_RAD]) {
      V->v[v] = tr->svar[vars[v] - GFSHIP_TREE_RAD];
      continue;
    }
    GFSHIP_CHECK (vars[v] >= 0 && vars[v] < abi_nvar, GFSHIP_EINVAL, "gfship_tree_snapshot: variable %d", vars[v]);
    GFSHIP_CHECK (vars[v] < GFSHIP_TREE_T0 || vars[v] > GFSHIP_TREE_T1 || vars[v] - GFSHIP_TREE_T0 < tr->ntracers,
		  GFSHIP_EINVAL, "gfship_tree_snapshot: the tree has no tracer T%d", vars[v] - GFSHIP_TREE_T0);
    V->v[v] = tr->var[abi_var[vars[v]]];
  }
  return 0;
}

void tree_free (gfship_tree * tr)
{
  if (!tr) return;
  if (tr->sampler && tr->sampler_free) tr->sampler_free (tr->sampler);
  if (tr->droplets && tr->droplets_free) tr->droplets_free (tr->droplets);
  (void) hipFree (tr->tagvar);
  snapshot_tables_free (tr);
  (void) hipFree (tr->dflag);
  (void) hipFree (tr->d_nbtab); (void) hipFree (tr->d_child0); (void) hipFree (tr->d_cmask); (void) hipFree (tr->d_idtab);
  for (double * p : tr->var) (void) hipFree (p);
  for (double * p : tr->uprev) (void) hipFree (p);
  for (double * p : tr->cvar) (void) hipFree (p);
  for (double * p : tr->svar) (void) hipFree (p);
  (void) hipFree (tr->leaves);
  (void) hipFree (tr->ghost_leaves);
  for (int l = 0; l <= GFSHIP_MAXLEVEL; l++) {
    (void) hipFree (tr->nonleaf[l]);
    (void) hipFree (tr->sweep[l].cells); (void) hipFree (tr->sweep[l].lev_off); (void) hipFree (tr->sweep[l].ghosts);
    (void) hipFree (tr->sweep[l].ti); (void) hipFree (tr->sweep[l].td); (void) hipFree (tr->sweep[l].tv);
    (void) hipFree (tr->sweep[l].cell_off); (void) hipFree (tr->sweep[l].chunk);
    loop_free (tr->sweep[l].loop);
    for (Sweep::Loop & P : tr->sweep[l].dloop) loop_free (P);
  }
  for (FaceSet & F : tr->fs) { (void) hipFree (F.faces); (void) hipFree (F.inc_off); (void) hipFree (F.inc); (void) hipFree (F.fval); }
  (void) hipFree (tr->d_red);
  if (tr->h_red) (void) hipHostFree (tr->h_red);
  if (tr->stream) (void) hipStreamDestroy (tr->stream);
  delete tr;
}

} // namespace

// ---- what tree_particles.hip sees of a tree --------------------------------------------------------

void gfship::tree_view (gfship_tree * tr, gfship::TreeView * v)
{
  v->H = tr->H; v->D = tr->D;
  v->stream = tr->stream;
  v->device = tr->device; v->ncell = tr->ncell; v->nleaves = tr->nleaves;
  v->hleaves = tr->hleaves.data ();
  v->dleaves = tr->leaves;
  v->side = tr->side;
  v->dt = tr->dt;
  v->t = tr->t;
  v->viscosity = tr->visc[0];
  for (int c = 0; c < 3; c++) v->uprev[c] = tr->uprev[c];
  v->sampler = &tr->sampler;
  v->sampler_free = &tr->sampler_free;
}

double * gfship::tree_variable (gfship_tree * tr, int var)
{
  if (var >= GFSHIP_TREE_UPREV && var <= GFSHIP_TREE_WPREV)
    return tr->uprev[var - GFSHIP_TREE_UPREV];
  if (var >= GFSHIP_TREE_VF && var <= GFSHIP_TREE_FZ)
    return tr->cvar[var - GFSHIP_TREE_VF];
  if (var >= GFSHIP_TREE_RAD && var <= GFSHIP_TREE_DMDT)
    return tr->svar[var - GFSHIP_TREE_RAD];
  if (var == GFSHIP_TREE_TAG)
    return tr->tagvar;
  return var >= 0 && var < abi_nvar ? tr->var[abi_var[var]] : nullptr;
}

int gfship::tree_device (gfship_tree * tr) { return tr->device; }

// a variable that the first call that needs it allocates zeroed, every level and ghost cells included
static int lazy_variable (gfship_tree * tr, double *& a, double ** out)
{
  if (!a) {
    GFSHIP_HIP (hipSetDevice (tr->device));
    GFSHIP_HIP (hipMalloc ((void **) &a, tr->ncell*sizeof (double)));
    GFSHIP_HIP (hipMemsetAsync (a, 0, tr->ncell*sizeof (double), tr->stream));
  }
  if (out) *out = a;
  return GFSHIP_OK;
}

int gfship::tree_coupling_variable (gfship_tree * tr, int var, double ** out)
{
  GFSHIP_CHECK (var >= GFSHIP_TREE_VF && var <= GFSHIP_TREE_FZ, GFSHIP_EINVAL,
		"%d is not GFSHIP_TREE_VF, _FX, _FY or _FZ", var);
  GFSHIP_CHECK (var != GFSHIP_TREE_FZ || tr->H.dim == 3, GFSHIP_EINVAL, "a quadtree has no GFSHIP_TREE_FZ");
  return lazy_variable (tr, tr->cvar[var - GFSHIP_TREE_VF], out);
}

int gfship::tree_source_variable (gfship_tree * tr, int var, double ** out)
{
  GFSHIP_CHECK (var >= GFSHIP_TREE_RAD && var <= GFSHIP_TREE_DMDT, GFSHIP_EINVAL,
		"%d is not GFSHIP_TREE_RAD, _URELP, _VRELP, _WRELP, _VOLSRC or _DMDT", var);
  GFSHIP_CHECK (var != GFSHIP_TREE_WRELP || tr->H.dim == 3, GFSHIP_EINVAL, "a quadtree has no GFSHIP_TREE_WRELP");
  return lazy_variable (tr, tr->svar[var - GFSHIP_TREE_RAD], out);
}

int gfship::tree_tag_variable (gfship_tree * tr, double ** out)
{
  return lazy_variable (tr, tr->tagvar, out);
}

int gfship::tree_droplet_plan (gfship_tree * tr, TreeDropletSlot * slot)
{
  if (!tr->droplet_plan) {
    DropletPlan P;
    int e = plan_droplets (*tr, P);
    if (e) return e;
    tr->droplet_plan = std::move (P);
  }
  slot->plan = &*tr->droplet_plan;
  slot->state = &tr->droplets;
  slot->state_free = &tr->droplets_free;
  return GFSHIP_OK;
}

int gfship::tree_bc_scalar (gfship_tree * tr, double * v) { return bc_scalar (tr, v); }

bool gfship::tree_has_variable (gfship_tree * tr, int var)
{
  if (var >= GFSHIP_TREE_T0 && var <= GFSHIP_TREE_T1 && var - GFSHIP_TREE_T0 >= tr->ntracers)
    return false;      /* as snapshot_vars: the arrays exist, the tracer does not */
  return tree_variable (tr, var) != nullptr;
}

// store_domain_previous_vel, modules/particulatecommon.c:99-113: the copy of U, V, W on the leaves (:108-110), then
// gfs_domain_bc of the new variable (:111), a scalar with the default GfsBc whatever the conditions of U
int gfship::tree_previous_vel (gfship_tree * tr)
{
  GFSHIP_HIP (hipSetDevice (tr->device));
  for (int c = 0; c < tr->H.dim; c++) {
    if (!tr->uprev[c]) {
      GFSHIP_HIP (hipMalloc ((void **) &tr->uprev[c], tr->ncell*sizeof (double)));
      GFSHIP_HIP (hipMemsetAsync (tr->uprev[c], 0, tr->ncell*sizeof (double), tr->stream));
    }
    t_copy_leaves<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, tr->var[V_U + c], tr->uprev[c]);
    GFSHIP_HIP (hipGetLastError ());
    int e = bc_scalar (tr, tr->uprev[c]);
    if (e) return e;
  }
  return GFSHIP_OK;
}

// ---- C ABI -------------------------------------------------------------------------------------

extern "C" {

int gfship_tree_create (gfship_tree ** out, int dim, gfship_refine_fn refine, void * ctx, int device)
{
  return gfship_tree_create_sides (out, dim, refine, ctx, nullptr, device);
}

// the tree (tr is a TreePlan), the sweep plans tr->sweep[].h and the face plans onto the device
static int tree_upload (gfship_tree * tr, const FacePlan * faces)
{
  hipError_t he = hipStreamCreate (&tr->stream);
  if (he != hipSuccess) return hip_fail (he, "hipStreamCreate", __FILE__, __LINE__);
  GFSHIP_HIP (hipMalloc ((void **) &tr->dflag, tr->ncell));
  GFSHIP_HIP (hipMemcpy (tr->dflag, tr->hflag.data (), tr->ncell, hipMemcpyHostToDevice));
  int e;
  if ((e = to_device (tr->h_nbtab, &tr->d_nbtab)) || (e = to_device (tr->h_child0, &tr->d_child0)) ||
      (e = to_device (tr->h_cmask, &tr->d_cmask)) || (e = to_device (tr->h_idtab, &tr->d_idtab)))
    return e;
  tr->D = tr->H;
  tr->D.flag = tr->dflag;
  tr->D.nbtab = tr->d_nbtab;
  tr->D.child0 = tr->d_child0;
  tr->D.cmask = tr->d_cmask;
  tr->D.idtab = tr->d_idtab;
  for (int v = 0; v < V_NVAR; v++) {
    GFSHIP_HIP (hipMalloc ((void **) &tr->var[v], tr->ncell*sizeof (double)));
    GFSHIP_HIP (hipMemset (tr->var[v], 0, tr->ncell*sizeof (double)));
  }
  GFSHIP_HIP (hipMalloc ((void **) &tr->d_red, 8*sizeof (double)));
  GFSHIP_HIP (hipHostMalloc ((void **) &tr->h_red, 8*sizeof (double), 0));
  tr->nleaves = (int) tr->hleaves.size ();
  if ((e = to_device (tr->hleaves, &tr->leaves))) return e;
  for (int l = 0; l < tr->H.depth; l++) {
    tr->nnonleaf[l] = (int) tr->hnonleaf[l].size ();
    if ((e = to_device (tr->hnonleaf[l], &tr->nonleaf[l]))) return e;
  }
  tr->nghost_leaves = (int) tr->hghost_leaves.size ();
  if ((e = to_device (tr->hghost_leaves, &tr->ghost_leaves))) return e;
  release (tr->hnonleaf); release (tr->hghost_leaves);
  for (int m = 0; m <= tr->H.depth; m++)
    if ((e = upload (&tr->sweep[m]))) return e;
  for (int k = 0; k < 1 + tr->H.dim; k++)
    if ((e = upload (faces[k], &tr->fs[k]))) return e;
  return 0;
}

// no exception crosses the C ABI: a tree too large for the host comes back as an error
int gfship_tree_create_sides (gfship_tree ** out, int dim, gfship_refine_fn refine, void * ctx,
			      const int * side, int device)
try {
  GFSHIP_CHECK (out && refine, GFSHIP_EINVAL, "gfship_tree_create: null argument");
  GFSHIP_CHECK (dim == 2 || dim == 3, GFSHIP_EINVAL, "gfship_tree_create: dim = %d", dim);
  // 1. the device
  int ndev = 0;
  if (hipGetDeviceCount (&ndev) != hipSuccess || ndev == 0) {
    set_error ("gfship_tree_create: no HIP device");
    return GFSHIP_ENODEVICE;
  }
  GFSHIP_CHECK (device >= 0 && device < ndev, GFSHIP_EINVAL, "gfship_tree_create: device %d of %d", device, ndev);
  GFSHIP_HIP (hipSetDevice (device));
  // 2. the plans (tree_plan.hip): nothing to free on failure but the plans themselves
  TreePlans h;
  int e = plan_tree_create (dim, refine, ctx, side, h);
  if (e) return e;
  // 3. the device tree: the plans are moved in, uploaded, and what nothing reads again is dropped
  gfship_tree * tr = new gfship_tree;
  static_cast<TreePlan &> (*tr) = std::move (h.T);
  tr->device = device;
  tr->sw = h.sw;
  for (int m = 0; m <= tr->H.depth; m++)
    tr->sweep[m].h = std::move (h.sweep[m]);
  if ((e = tree_upload (tr, h.faces))) {
    tree_free (tr);
    return e;
  }
  // 4. the defaults of the parameters
  for (int d = 0; d < 2*dim; d++)
    tr->bc_p[d] = GFSHIP_BC_SYMMETRY;
  gfship_multilevel_params_init (&tr->projection_params, dim);
  gfship_multilevel_params_init (&tr->approx_projection_params, dim);
  for (int c = 0; c < 3; c++) {     /* diffusion_init, src/source.c:966-974 */
    gfship_multilevel_params_init (&tr->diffusion_params[c], dim);
    tr->diffusion_params[c].tolerance = 1e-6;
  }
  *out = tr;
  return GFSHIP_OK;
}
catch (const std::bad_alloc &) {
  set_error ("gfship_tree_create: out of host memory while the tree was built");
  return GFSHIP_EUNSUPPORTED;
}

void gfship_tree_destroy (gfship_tree * tr) { tree_free (tr); }

int gfship_tree_depth (const gfship_tree * tr) { return tr ? tr->H.depth : -1; }
int gfship_tree_dim (const gfship_tree * tr) { return tr ? tr->H.dim : -1; }

int gfship_tree_flags (const gfship_tree * tr, int level, unsigned char * out)
{
  GFSHIP_CHECK (tr && out && level >= 0 && level <= tr->H.depth, GFSHIP_EINVAL, "gfship_tree_flags: bad argument");
  memcpy (out, tr->hflag.data () + tr->H.off[level], (size_t) tr->H.lsize (level));
  return GFSHIP_OK;
}

int gfship_tree_upload (gfship_tree * tr, int var, int level, const double * in)
{
  GFSHIP_CHECK (tr && in && level >= 0 && level <= tr->H.depth, GFSHIP_EINVAL, "gfship_tree_upload: bad argument");
  double * a = nullptr;
  if (var >= GFSHIP_TREE_VF && var <= GFSHIP_TREE_FZ) {      /* an upload is a call that needs them */
    int r = tree_coupling_variable (tr, var, &a);
    if (r) return r;
  }
  else if (var >= GFSHIP_TREE_RAD && var <= GFSHIP_TREE_DMDT) {
    int r = tree_source_variable (tr, var, &a);
    if (r) return r;
  }
  else {
    GFSHIP_CHECK (var >= 0 && var < abi_nvar, GFSHIP_EINVAL, "gfship_tree_upload: bad argument");
    a = tr->var[abi_var[var]];
  }
  GFSHIP_HIP (hipMemcpyAsync (a + tr->H.off[level], in, (size_t) tr->H.lsize (level)*sizeof (double),
			      hipMemcpyHostToDevice, tr->stream));
  GFSHIP_HIP (hipStreamSynchronize (tr->stream));
  return GFSHIP_OK;
}

int gfship_tree_download (gfship_tree * tr, int var, int level, double * out)
{
  GFSHIP_CHECK (tr && out && tree_variable (tr, var) && level >= 0 && level <= tr->H.depth, GFSHIP_EINVAL,
		"gfship_tree_download: bad argument");
  GFSHIP_HIP (hipMemcpyAsync (out, tree_variable (tr, var) + tr->H.off[level], (size_t) tr->H.lsize (level)*sizeof (double),
			      hipMemcpyDeviceToHost, tr->stream));
  GFSHIP_HIP (hipStreamSynchronize (tr->stream));
  return GFSHIP_OK;
}

gfship_multilevel_params * gfship_tree_projection_params (gfship_tree * tr, int approx)
{
  return approx ? &tr->approx_projection_params : &tr->projection_params;
}

int gfship_tree_set_bc (gfship_tree * tr, int d, int kind)
{
  GFSHIP_CHECK (tr && d >= 0 && d < 2*tr->H.dim && tr->side[d] == GFSHIP_SIDE_BOUNDARY &&
		(kind == GFSHIP_BC_SYMMETRY || kind == GFSHIP_BC_DIRICHLET || kind == GFSHIP_BC_NEUMANN),
		GFSHIP_EINVAL, "gfship_tree_set_bc: bad argument");
  tr->bc_p[d] = kind;
  for (int l = 0; l <= GFSHIP_MAXLEVEL; l++)     /* the signs of the homogeneous conditions are in the plans */
    loop_free (tr->sweep[l].loop);
  return GFSHIP_OK;
}

/* gfs_poisson_solve (src/poisson.c:1225-1269) on the tree: P (GFSHIP_TREE_P) holds the guess, the
   right-hand side is in GFSHIP_TREE_DIV, dia = 0, alpha = NULL; the residual is left in GFSHIP_TREE_RES */
int gfship_tree_poisson_solve (gfship_tree * tr, gfship_multilevel_params * par, double dt)
{
  GFSHIP_CHECK (tr && par, GFSHIP_EINVAL, "gfship_tree_poisson_solve: null argument");
  GFSHIP_HIP (hipSetDevice (tr->device));
  int e;
  if ((e = bc_leaves (tr, tr->var[V_P]))) return e;
  return poisson_solve (tr, par, tr->var[V_P], tr->var[V_DIV], dt);
}

int gfship_tree_set_time (gfship_tree * tr, double end, double cfl)
{
  GFSHIP_CHECK (tr && cfl > 0., GFSHIP_EINVAL, "gfship_tree_set_time: bad argument");
  tr->end = end;
  tr->cfl = cfl;
  return GFSHIP_OK;
}

int gfship_tree_set_next_event (gfship_tree * tr, gfship_next_event_fn fn, void * ctx)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_set_next_event: null tree");
  tr->next_event = fn;
  tr->next_event_ctx = ctx;
  return GFSHIP_OK;
}

double gfship_tree_time (const gfship_tree * tr) { return tr->t; }
double gfship_tree_dt (const gfship_tree * tr) { return tr->dt; }
unsigned gfship_tree_iter (const gfship_tree * tr) { return tr->iter; }

/* gfs_divergence of (U, V, W) on the leaves into the variable GFSHIP_TREE_DIV (the scratch `div' of
   the projections: valid until the next step) */
int gfship_tree_divergence (gfship_tree * tr)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_divergence: null tree");
  GFSHIP_HIP (hipSetDevice (tr->device));
  GFSHIP_HIP (hipMemsetAsync (tr->var[V_DIV], 0, tr->ncell*sizeof (double), tr->stream));
  t_divergence_centered<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, p3 (tr, V_U), tr->var[V_DIV]);
  KCHECK ();
  return GFSHIP_OK;
}

/* the cells of the sweep of level `level' and the number of dependency levels they form */
int gfship_tree_sweep_levels (const gfship_tree * tr, int level, int * ncells, int * nlevels)
{
  GFSHIP_CHECK (tr && level >= 0 && level <= tr->H.depth, GFSHIP_EINVAL, "gfship_tree_sweep_levels: bad argument");
  if (ncells) *ncells = tr->sweep[level].ncells;
  if (nlevels) *nlevels = tr->sweep[level].nlev;
  return GFSHIP_OK;
}

int gfship_tree_set_bc_u (gfship_tree * tr, int c, int d, int kind)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_set_bc_u: null tree");
  GFSHIP_CHECK (c >= 0 && c < tr->H.dim && d >= 0 && d < 2*tr->H.dim, GFSHIP_EINVAL, "component %d / side %d out of range", c, d);
  GFSHIP_CHECK (kind == GFSHIP_BC_SYMMETRY || kind == GFSHIP_BC_DIRICHLET || kind == GFSHIP_BC_NEUMANN, GFSHIP_EINVAL,
		"kind of condition %d", kind);
  GFSHIP_CHECK (tr->side[d] != GFSHIP_SIDE_PERIODIC || kind == GFSHIP_BC_SYMMETRY, GFSHIP_EINVAL, "side %d is periodic", d);
  tr->bc_u[c][d] = kind;
  return GFSHIP_OK;
}

int gfship_tree_set_viscosity (gfship_tree * tr, int c, double nu)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_set_viscosity: null tree");
  GFSHIP_CHECK (c >= 0 && c < tr->H.dim, GFSHIP_EINVAL, "component %d out of range", c);
  GFSHIP_CHECK (nu >= 0., GFSHIP_EINVAL, "the diffusion coefficient must be positive");
  /* the coefficients of gfs_diffusion_coefficients (src/poisson.c:1280-1303,826-853) are w on every face the
     stencils read, quadtrees and octrees alike (diffusion_weights_exact): checked once per octree */
  if (nu != 0. && tr->H.dim == 3 && tr->diffusion_exact < 0) {
    try { tr->diffusion_exact = diffusion_weights_exact (tr->H) ? 1 : 0; }
    catch (const std::bad_alloc &) { set_error ("gfship_tree_set_viscosity: out of host memory"); return GFSHIP_EUNSUPPORTED; }
  }
  GFSHIP_CHECK (nu == 0. || tr->H.dim == 2 || tr->diffusion_exact == 1, GFSHIP_EUNSUPPORTED,
		"GfsSourceDiffusion on this octree: a diffusion coefficient is not the same number on every face");
  tr->visc[c] = nu;
  return GFSHIP_OK;
}

int gfship_tree_set_source_fields (gfship_tree * tr, int on)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_set_source_fields: null tree");
  if (on)
    for (int c = 0; c < tr->H.dim; c++) {
      int r = tree_coupling_variable (tr, GFSHIP_TREE_FX + c, nullptr);
      if (r) return r;
    }
  tr->src_fields = on != 0;
  return GFSHIP_OK;
}

int gfship_tree_mac_source (gfship_tree * tr, int c, int var_out)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_mac_source: null tree");
  GFSHIP_CHECK (c >= 0 && c < tr->H.dim, GFSHIP_EINVAL, "component %d out of range", c);
  GFSHIP_CHECK (var_out == GFSHIP_TREE_RES || var_out == GFSHIP_TREE_DIV, GFSHIP_EINVAL,
		"gfship_tree_mac_source writes into GFSHIP_TREE_RES or GFSHIP_TREE_DIV");
  GFSHIP_HIP (hipSetDevice (tr->device));
  t_mac_source<<<blocks (tr->nleaves), 256, 0, tr->stream>>> (tr->D, tr->leaves, tr->nleaves, c, tr->var[V_U + c],
      tr->src_fields ? tr->cvar[1 + c] : nullptr, tr->visc[c], tr->var[abi_var[var_out]]);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

int gfship_tree_set_source (gfship_tree * tr, int c, double g)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_set_source: null tree");
  GFSHIP_CHECK (c >= 0 && c < tr->H.dim, GFSHIP_EINVAL, "component %d out of range", c);
  tr->src[c] = g;
  return GFSHIP_OK;
}

gfship_multilevel_params * gfship_tree_diffusion_params (gfship_tree * tr, int c)
{ return (tr && c >= 0 && c < 3) ? &tr->diffusion_params[c] : nullptr; }

int gfship_tree_add_tracer (gfship_tree * tr, int gradient)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_add_tracer: null tree");
  GFSHIP_CHECK (gradient == 0 || gradient == 1, GFSHIP_EINVAL, "gradient: 0 centred, 1 van Leer");
  GFSHIP_CHECK (tr->ntracers < TREE_MAXTRACERS, GFSHIP_EUNSUPPORTED, "a tree carries %d tracers at most", TREE_MAXTRACERS);
  tr->tracer_gradient[tr->ntracers] = gradient;
  return GFSHIP_TREE_T0 + tr->ntracers++;
}

/* simulation_run up to the loop, src/simulation.c:458-476 */
int gfship_tree_start (gfship_tree * tr)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_start: null tree");
  GFSHIP_HIP (hipSetDevice (tr->device));
  int e;
  const int vars[] = { V_P, V_PMAC, V_U, V_U + 1, V_U + 2 };
  for (int k = 0; k < 2 + tr->H.dim; k++)
    if ((e = k >= 2 ? bc_velocity (tr, k - 2) : bc_leaves (tr, tr->var[vars[k]], -1))) return e;
  for (int k = 0; k < tr->ntracers; k++)
    if ((e = bc_scalar (tr, tr->var[V_T + k]))) return e;
  if ((e = coarse_init (tr))) return e;
  if ((e = set_timestep (tr))) return e;
  if (tr->restarted) {
    /* time.i > 0, src/simulation.c:475-476: no projection, no half step of the tracers; gfs_update_gradients
       (src/timestep.c:305-322) rebuilds g from P, which the first iteration reads */
    for (int c = 0; c < tr->H.dim; c++)
      GFSHIP_HIP (hipMemsetAsync (tr->var[V_G + c], 0, tr->ncell*sizeof (double), tr->stream));
    return correct_normal_velocities (tr, tr->var[V_P], V_G, 0.);
  }
  if ((e = approximate_projection (tr, &tr->approx_projection_params, tr->dt))) return e;
  if ((e = set_timestep (tr))) return e;
  return advance_tracers (tr, tr->dt/2.);
}

/* a simulation read from a file with GfsTime { i = ... t = ... }: the state comes from gfship_tree_snapshot_read,
   gfship_tree_start then takes the branch time.i > 0 of simulation_run (src/simulation.c:456-476) */
int gfship_tree_restart (gfship_tree * tr, double t, unsigned i)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_restart: null tree");
  tr->t = tr->tnext = t;
  tr->iter = i;
  tr->restarted = i > 0;
  return GFSHIP_OK;
}

/* ftt_cell_write_binary + gfs_cell_write_binary (src/ftt.c:1771-1799, src/domain.c:3176-3207): the bytes between
   the braces of a GfsBox with `binary = 1', for the variables `vars' (GFSHIP_TREE_*) in that order */
size_t gfship_tree_snapshot_bytes (const gfship_tree * ctr, int nvars)
{
  gfship_tree * tr = const_cast<gfship_tree *> (ctr);      /* the tables are a cache */
  if (!tr || nvars < 0 || snapshot_tables (tr)) return 0;
  return (size_t) (tr->snap_records*(12ull + 8ull*(unsigned long long) nvars));
}

int gfship_tree_snapshot_write (gfship_tree * tr, int nvars, const int * vars, void * host_buf, size_t bytes)
{
  SnapVars V;
  int e;
  if ((e = snapshot_vars (tr, nvars, vars, &V))) return e;
  GFSHIP_HIP (hipSetDevice (tr->device));
  if ((e = snapshot_tables (tr))) return e;
  const size_t need = gfship_tree_snapshot_bytes (tr, nvars);
  GFSHIP_CHECK (host_buf && bytes >= need, GFSHIP_EINVAL, "the buffer must hold %zu bytes", need);
  unsigned char * image = nullptr;
  GFSHIP_HIP (hipMalloc ((void **) &image, need));
  t_snapshot<false><<<blocks (tr->snap_ncells), 256, 0, tr->stream>>> (tr->D, tr->snap_cells, tr->snap_ncells, tr->snap_off,
      V, image, (unsigned long long *) nullptr);
  hipError_t he = hipGetLastError ();
  if (he == hipSuccess)
    he = hipMemcpyAsync (host_buf, image, need, hipMemcpyDeviceToHost, tr->stream);
  if (he == hipSuccess)
    he = hipStreamSynchronize (tr->stream);
  (void) hipFree (image);
  GFSHIP_HIP (he);
  return GFSHIP_OK;
}

/* cell_read_binary + gfs_cell_read_binary (src/ftt.c:1913-1975, src/domain.c:3227-3250) into a tree that already
   has the refinement of the file: every record is checked against it */
int gfship_tree_snapshot_read (gfship_tree * tr, int nvars, const int * vars, const void * host_buf, size_t bytes)
{
  SnapVars V;
  int e;
  if ((e = snapshot_vars (tr, nvars, vars, &V))) return e;
  GFSHIP_HIP (hipSetDevice (tr->device));
  if ((e = snapshot_tables (tr))) return e;
  const size_t need = gfship_tree_snapshot_bytes (tr, nvars);
  GFSHIP_CHECK (host_buf != nullptr, GFSHIP_EINVAL, "null buffer");
  GFSHIP_CHECK (bytes == need, GFSHIP_EINVAL,
		"the cell data of this tree (%llu cells) with %d variables is %zu bytes, not %zu",
		tr->snap_records, nvars, need, bytes);
  unsigned char * image = nullptr;
  GFSHIP_HIP (hipMalloc ((void **) &image, need + 16));
  unsigned long long * err = (unsigned long long *) (image + ((need + 7) & ~(size_t) 7));
  unsigned long long herr = ~0ull;
  hipError_t he = hipMemsetAsync (err, 0xff, sizeof (herr), tr->stream);
  if (he == hipSuccess)
    he = hipMemcpyAsync (image, host_buf, need, hipMemcpyHostToDevice, tr->stream);
  if (he == hipSuccess) {
    t_snapshot<true><<<blocks (tr->snap_ncells), 256, 0, tr->stream>>> (tr->D, tr->snap_cells, tr->snap_ncells, tr->snap_off,
	V, image, err);
    he = hipGetLastError ();
  }
  if (he == hipSuccess)
    he = hipMemcpyAsync (&herr, err, sizeof (herr), hipMemcpyDeviceToHost, tr->stream);
  if (he == hipSuccess)
    he = hipStreamSynchronize (tr->stream);
  (void) hipFree (image);
  GFSHIP_HIP (he);
  const int kind = herr == ~0ull ? -1 : (int) (herr & 3);
  GFSHIP_CHECK (kind != 0, GFSHIP_EINVAL,
		"FTT_CELL_ID (cell) != (flags & FTT_FLAG_ID): make sure the file has %d spatial dimensions", tr->H.dim);
  GFSHIP_CHECK (kind != 1, GFSHIP_EUNSUPPORTED, "the tree of the file is not the tree of this simulation");
  GFSHIP_CHECK (kind != 2, GFSHIP_EUNSUPPORTED, "the file has solid fractions (mixed cells)");
  return GFSHIP_OK;
}

/* one iteration of the loop, src/simulation.c:479-548 */
int gfship_tree_step (gfship_tree * tr)
{
  GFSHIP_CHECK (tr, GFSHIP_EINVAL, "gfship_tree_step: null tree");

  GFSHIP_HIP (hipSetDevice (tr->device));
  int e;
  if ((e = predicted_face_velocities (tr))) return e;
  /* gfs_variables_swap (p, pmac) around the MAC projection */
  if ((e = mac_projection (tr, &tr->projection_params, tr->dt/2., tr->var[V_PMAC], V_GM))) return e;
  const int g = tr->iter > 0 ? V_G : V_GM;
  if ((e = centered_velocity_advection (tr, V_GM, g))) return e;
  if ((e = correct_centered (tr, g, - tr->dt))) return e;
  if ((e = coarse_init (tr))) return e;
  if ((e = approximate_projection (tr, &tr->approx_projection_params, tr->dt))) return e;
  tr->t = tr->tnext;
  tr->iter++;
  if ((e = set_timestep (tr))) return e;
  return advance_tracers (tr, tr->dt);
}

} // extern "C"
