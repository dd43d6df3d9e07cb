// tree_droplets.hip -- gfs_domain_tag_droplets (src/domain.c:3727-3796), gfs_domain_remove_droplets (:3798-3880) and
// GfsDropletToParticle (modules/particulatecommon.c:1163-1527) on a refined quadtree / octree.
//
// On a tree the fill of the reference is directed.  From a leaf, tag_cell_fraction (:3566-3596) tests `tag == 0 && c >
// THRESHOLD' on the neighbour ftt_cell_neighbors gives: a leaf of its level or coarser is tagged; a cell N of its
// level with children is tested ITSELF, with the value c holds on that cell, and only then are its children on the
// face looked at.  So a fine leaf f always reaches the coarser leaf k beside it, and k reaches f only where c (N) >
// THRESHOLD for the parent N of f.  The fill label of a leaf (proved in 11.41, pinned by
// tests/test_tree_droplets_reference_cpu.py on a literal restatement) is the smallest traversal position of a leaf
// from which a directed path inside the mask reaches it; the periodic sides then join fill regions undirected.
// A label is the position of a leaf in traversal order.  With the contacts of the host planner (plan_droplets):
//   1. tdrop_block_kernel: workgroups of 256 consecutive positions (spatially compact in traversal order) take the
//      mask of their leaves and unite in LDS the contacts that are symmetric -- two leaves of a level, or a gate that
//      is open -- and lie inside the block;
//   2. tdrop_cross_kernel: the same for the contacts that leave the block, by atomicMin on the global parents.
//      In both, a contact whose gate is shut unites nothing and appends a one-way record (f, k) to a list through an
//      integer counter; nothing depends on the order of the list;
//   3. tdrop_oneway_kernel: ONE workgroup, which leaves at once where the list is empty: L[root (k)] = min (L[root
//      (k)], L[root (f)]) over the records, block barriers between the rounds, until nothing changes (labels only
//      decrease); then parent[root] = L[root].  L[root] is a seed (L = itself), so the forest stays a forest;
//   4. tdrop_periodic_kernel: the periodic pairs, united on that forest;
// then droplets.hpp: flatten, flags, scan, tag = 1 + rank, and everything an event does with the tags.  Integer
// atomics only; no kernel waits for another workgroup.  The host reads n, the size a negative min selects and, with
// info, one more word; never the number of records.
#include "particle_events.hpp"
#include "droplets.hpp"
#include "tree_particles.hpp"
#include "tree_plan.hpp"
#include <string>
#include <vector>

namespace gfship {

namespace {

using tree::Topo;
using tree::Cell;
using tree::DropContact;

// the interior leaves of the tree as the geometry of droplets.hpp
template <int DIM>
struct TreeDrops {
  Topo T;
  const Cell * leaves;
  const unsigned char * side;
  unsigned N;
  __device__ __forceinline__ long index (unsigned t) const { return T.gi (leaves[t]); }
  __device__ __forceinline__ bool on_side (unsigned t) const { return side[t] != 0; }
  __device__ __forceinline__ double volume (unsigned t) const {
    const double h = 1./(double) (1 << leaves[t].l);
    return DIM == 3 ? h*h*h : h*h;      /* pow (h, FTT_DIMENSION): powers of two */
  }
  __device__ __forceinline__ void pos (unsigned t, double p[3]) const {
    const Cell c = leaves[t];
    const int r = (1 << c.l) + 2;
    const int x[3] = { c.q % r, (c.q/r) % r, DIM == 3 ? c.q/(r*r) : 0 };
    const double h = 1./(double) (1 << c.l);
    p[2] = 0.;
#pragma unroll
    for (int a = 0; a < DIM; a++)
      p[a] = -0.5 + (x[a] - 0.5)*h;      /* ftt_cell_pos: dyadic, exact */
  }
  __device__ __forceinline__ bool locate (const double p[3], unsigned & cell, long & at) const {
    Leaf c;
    if (!tree_locate<DIM> (*this, p, c)) return false;
    cell = (unsigned) c.g;
    at = c.g;
    return true;
  }
};

// what the labelling keeps on the device of a tree: the plan, the work arrays of droplets.hpp and its own
struct TreeDropState {
  DropWork * W = nullptr;
  int * con_off = nullptr;
  DropContact * con = nullptr;
  unsigned * periodic = nullptr, * cells = nullptr;
  unsigned char * on_side = nullptr;
  unsigned nper = 0, ngated = 0;
  unsigned * L = nullptr;       // per leaf: the fill label of the component it is the root of
  unsigned * rec = nullptr;     // the one-way records (f, k) of a call, at most ngated
  unsigned * nrec = nullptr;
};

struct TreeLabelArgs {
  Topo T;
  const Cell * leaves;
  unsigned N, cap;
  const double * c;             // the mask, every cell of every level
  const int * con_off;
  const DropContact * con;
  unsigned * parent, * L, * rec, * nrec;
};

// a contact whose gate is shut: from the fine end the fill reaches the coarse one, not the other way
__device__ __forceinline__ void tdrop_record (const TreeLabelArgs & A, unsigned p, unsigned q, int gate)
{
  const unsigned slot = atomicAdd (A.nrec, 1u);
  if (slot < A.cap) {
    A.rec[2*slot] = (gate & 1) ? p : q;
    A.rec[2*slot + 1] = (gate & 1) ? q : p;
  }
}

// 1. the mask of 256 consecutive leaves and their symmetric contacts inside the block, in LDS
__global__ void __launch_bounds__(DROP_BLOCK)
tdrop_block_kernel (TreeLabelArgs A)
{
  __shared__ unsigned lab[DROP_BLOCK];
  const unsigned l = threadIdx.x, base = blockIdx.x*(unsigned) DROP_BLOCK, t = base + l;
  const bool in = t < A.N && A.c[A.T.gi (A.leaves[t])] > DROP_THRESHOLD;
  lab[l] = in ? l : DROP_NONE;
  __syncthreads ();
  /* a leaf outside the mask stays DROP_NONE, a leaf inside never becomes it: these reads need no care */
  if (in)
    for (int o = A.con_off[t]; o < A.con_off[t + 1]; o++) {
      const DropContact C = A.con[o];
      if (C.other < base || lab[C.other - base] == DROP_NONE) continue;
      if (C.gate < 0 || A.c[C.gate >> 1] > DROP_THRESHOLD) drop_union (lab, l, C.other - base);
      else tdrop_record (A, t, C.other, C.gate);
    }
  __syncthreads ();
  if (t < A.N) {
    unsigned x = l;
    if (in)      /* nothing writes lab after the barrier: plain loads */
      while (lab[x] != x) x = lab[x];
    A.parent[t] = in ? base + x : DROP_NONE;
    A.L[t] = t;
  }
}

// 2. the contacts with a leaf of an earlier block
__global__ void __launch_bounds__(DROP_BLOCK)
tdrop_cross_kernel (TreeLabelArgs A)
{
  const unsigned base = blockIdx.x*(unsigned) DROP_BLOCK, t = base + threadIdx.x;
  if (t >= A.N || A.parent[t] == DROP_NONE) return;
  for (int o = A.con_off[t]; o < A.con_off[t + 1]; o++) {
    const DropContact C = A.con[o];
    if (C.other >= base || A.parent[C.other] == DROP_NONE) continue;
    if (C.gate < 0 || A.c[C.gate >> 1] > DROP_THRESHOLD) drop_union (A.parent, t, C.other);
    else tdrop_record (A, t, C.other, C.gate);
  }
}

__device__ __forceinline__ unsigned tdrop_load (const unsigned * p)
{
  return __hip_atomic_load (p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 3. the one-way contacts: one workgroup
__global__ void __launch_bounds__(DROP_BLOCK)
tdrop_oneway_kernel (unsigned cap, const unsigned * __restrict__ nrec, unsigned * rec, unsigned * parent, unsigned * L)
{
  __shared__ int changed;
  unsigned m = *nrec;
  if (m == 0) return;
  if (m > cap) m = cap;      /* cannot happen: a contact with a gate gives one record at most */
  for (unsigned o = threadIdx.x; o < 2*m; o += DROP_BLOCK)
    rec[o] = drop_find (parent, rec[o]);      /* the forest of the unions is final: the roots */
  __syncthreads ();
  for (;;) {
    if (threadIdx.x == 0) changed = 0;
    __syncthreads ();
    for (unsigned o = threadIdx.x; o < m; o += DROP_BLOCK) {
      const unsigned f = rec[2*o], k = rec[2*o + 1], lf = tdrop_load (&L[f]);
      if (lf < tdrop_load (&L[k])) {
	atomicMin (&L[k], lf);
	changed = 1;
      }
    }
    __syncthreads ();
    const int again = changed;
    __syncthreads ();
    if (!again) break;
  }
  /* the root of a component that a seed reaches takes the seed as its parent: L of a seed is the seed itself */
  for (unsigned o = threadIdx.x; o < m; o += DROP_BLOCK) {
    const unsigned k = rec[2*o + 1];
    parent[k] = tdrop_load (&L[k]);
  }
}

// 4. the leaves that meet through a periodic side
__global__ void __launch_bounds__(DROP_BLOCK)
tdrop_periodic_kernel (unsigned npairs, const unsigned * __restrict__ pair, unsigned * parent)
{
  const unsigned o = blockIdx.x*(unsigned) DROP_BLOCK + threadIdx.x;
  if (o >= npairs) return;
  const unsigned p = pair[2*o], q = pair[2*o + 1];
  if (tdrop_load (&parent[p]) == DROP_NONE || tdrop_load (&parent[q]) == DROP_NONE) return;
  drop_union (parent, p, q);
}

void tree_drop_state_free (void * p)
{
  TreeDropState * S = (TreeDropState *) p;
  if (!S) return;
  drop_work_free (S->W);
  void * a[] = { S->con_off, S->con, S->periodic, S->cells, S->on_side, S->L, S->rec, S->nrec };
  for (void * q : a)
    if (q) (void) hipFree (q);
  delete S;
}

template <class T> int tdrop_upload (const std::vector<T> & h, T ** d)
{
  const size_t n = std::max<size_t> (h.size (), 1);      /* no empty allocation */
  GFSHIP_HIP (hipMalloc ((void **) d, n*sizeof (T)));
  if (!h.empty ())
    GFSHIP_HIP (hipMemcpy (*d, h.data (), h.size ()*sizeof (T), hipMemcpyHostToDevice));
  return GFSHIP_OK;
}

// the tree as the host mesh of droplets.hpp
struct TreeDropMesh {
  gfship_tree * tr = nullptr;
  TreeView V;
  TreeDropState * S = nullptr;
  int dim = 0;
  hipStream_t stream = nullptr;
  unsigned N = 0;
  template <int DIM> TreeDrops<DIM> geom () const { return TreeDrops<DIM> { V.D, V.dleaves, S->on_side, N }; }

  // the plan and the work arrays of the labelling on the device: all of them, or nothing (a later call tries again)
  int upload_plan (const tree::DropletPlan & P, TreeDropState ** out) const {
    TreeDropState * built = new TreeDropState;
    built->nper = (unsigned) (P.periodic.size ()/2);
    built->ngated = P.ngated;
    auto alloc = [] (unsigned ** d, size_t n) -> int {
      GFSHIP_HIP (hipMalloc ((void **) d, n*sizeof (unsigned)));
      return GFSHIP_OK;
    };
    int r;
    if ((r = drop_work_new (&built->W)) || (r = tdrop_upload (P.con_off, &built->con_off)) ||
	(r = tdrop_upload (P.con, &built->con)) || (r = tdrop_upload (P.periodic, &built->periodic)) ||
	(r = tdrop_upload (P.cells, &built->cells)) || (r = tdrop_upload (P.on_side, &built->on_side)) ||
	(r = alloc (&built->L, std::max (N, 1u))) || (r = alloc (&built->rec, 2*(size_t) std::max (P.ngated, 1u))) ||
	(r = alloc (&built->nrec, 1))) {
      tree_drop_state_free (built);
      return r;
    }
    *out = built;
    return GFSHIP_OK;
  }

  // the view of the tree and, on first use, its droplet plan on its device
  int init (gfship_tree * tree) {
    tr = tree;
    tree_view (tr, &V);
    GFSHIP_HIP (hipSetDevice (V.device));
    dim = V.H.dim; stream = V.stream; N = (unsigned) V.nleaves;
    TreeDropletSlot slot;
    int r = tree_droplet_plan (tr, &slot);
    if (r) return r;
    if (!*slot.state) {
      TreeDropState * built = nullptr;
      if ((r = upload_plan (*slot.plan, &built))) return r;      /* nothing is kept of a plan that did not get there */
      *slot.state = built;
      *slot.state_free = tree_drop_state_free;
    }
    S = (TreeDropState *) *slot.state;
    return GFSHIP_OK;
  }

  // steps 1 to 4 and the ranks: the mask is c (every cell of every level); *n is read back
  int labels (const double * c, unsigned * n) const {
    int r;
    if ((r = drop_reserve_cells (stream, S->W, N))) return r;
    TreeLabelArgs A;
    A.T = V.D; A.leaves = V.dleaves; A.N = N; A.cap = S->ngated; A.c = c;
    A.con_off = S->con_off; A.con = S->con;
    A.parent = S->W->parent; A.L = S->L; A.rec = S->rec; A.nrec = S->nrec;
    GFSHIP_HIP (hipMemsetAsync (S->nrec, 0, sizeof (unsigned), stream));
    hipLaunchKernelGGL (tdrop_block_kernel, dim3 (drop_grid (N)), dim3 (DROP_BLOCK), 0, stream, A);
    hipLaunchKernelGGL (tdrop_cross_kernel, dim3 (drop_grid (N)), dim3 (DROP_BLOCK), 0, stream, A);
    hipLaunchKernelGGL (tdrop_oneway_kernel, dim3 (1), dim3 (DROP_BLOCK), 0, stream, S->ngated, S->nrec, S->rec,
			S->W->parent, S->L);
    if (S->nper)
      hipLaunchKernelGGL (tdrop_periodic_kernel, dim3 (drop_grid (S->nper)), dim3 (DROP_BLOCK), 0, stream, S->nper,
			  S->periodic, S->W->parent);
    GFSHIP_HIP (hipGetLastError ());
    return drop_ranks (stream, S->W, N, n);
  }

  // step 7 on the leaves of v, then gfs_domain_bc (v)
  int reset (double * v, unsigned min, double val) const {
    int r = drop_reset_leaves (*this, S->W, v, min, val);
    if (r) return r;
    return tree_bc_scalar (tr, v);
  }
};

// a variable of the tree a mask may be: one the tree has now, and not the tags themselves
int tdrop_variable (gfship_tree * tr, int var, const char * what, double ** out)
{
  *out = var != GFSHIP_TREE_TAG && tree_has_variable (tr, var) ? tree_variable (tr, var) : nullptr;
  GFSHIP_CHECK (*out != nullptr, GFSHIP_EINVAL, "%s: the tree has no variable %d", what, var);
  return GFSHIP_OK;
}

} // namespace

// gfs_droplet_to_particle_event (modules/particulatecommon.c:1362-1404) on a list of a tree
int tree_droplet_event (gfship_droplet_to_particle * d, gfship_droplet_info * info)
{
  gfship_particles * pl = d->pl;
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_droplet_to_particle_event");
  TreeDropMesh M;
  int r = M.init (pl->tree);
  if (r) return r;
  double * c = nullptr, * mask = nullptr;
  if ((r = tdrop_variable (pl->tree, d->c, "GfsDropletToParticle", &c))) return r;
  /* the mask (:1368-1393); a function that is no variable at every cell of every level (compute_v, :1357-1390) */
  if (d->mask >= 0) {
    if ((r = tdrop_variable (pl->tree, d->mask, "GfsDropletToParticle", &mask))) return r;
  }
  else if (d->constant) {
    if ((r = launch_fill (M.stream, (long) M.V.ncell, d->value, d->fv))) return r;
    mask = d->fv;
  }
  else {
    std::vector<const double *> read;
    for (int var : d->read) {
      double * a = nullptr;
      if ((r = tdrop_variable (pl->tree, var, "GfsDropletToParticle", &a))) return r;
      read.push_back (a);
    }
    if ((r = rtc_launch_tree_cell (d->fn, M.stream, M.V.ncell, M.V.H.depth, M.V.H.off, M.S->cells, M.V.t,
				   (int) read.size (), read.data (), d->fv)))
      return r;
    mask = d->fv;
  }
  unsigned n = 0, umin = 0;
  if ((r = M.labels (mask, &n))) return r;
  if (info) info->n = n;
  if (!(n > 0 && -(long) d->min < (long) n)) return GFSHIP_OK;      /* :1381 */
  GFSHIP_CHECK ((long) pl->n + (long) n <= 0x7fffffffL, GFSHIP_ENOMEM, "the list would hold 2^31 slots or more");
  DropWork * W = M.S->W;
  if ((r = drop_tags (M, W, nullptr, n, true, false))) return r;
  if ((r = drop_min (M.stream, W, n, d->min, &umin))) return r;
  if (info) info->min = umin;
  const int uvar[3] = { GFSHIP_TREE_U, GFSHIP_TREE_V, GFSHIP_TREE_W };
  const double * u[3];
  for (int a = 0; a < 3; a++)
    u[a] = a < M.dim ? tree_variable (pl->tree, uvar[a]) : nullptr;
  /* a tree has no alpha: mass = 1.*volume (:1334-1336) */
  if ((r = drop_convert (M, W, pl, n, umin, c, u, nullptr, info != nullptr))) return r;
  if ((r = M.reset (c, umin, d->reset))) return r;
  return info ? drop_info (M.stream, W, info) : GFSHIP_OK;
}

} // namespace gfship

using namespace gfship;

extern "C" {

int gfship_tree_tag_droplets (gfship_tree * tr, int c_var, unsigned * n)
{
  GFSHIP_CHECK (tr && n, GFSHIP_EINVAL, "gfship_tree_tag_droplets: null argument");
  double * c = nullptr, * tag = nullptr;
  int r = tdrop_variable (tr, c_var, "gfs_domain_tag_droplets", &c);
  if (r) return r;
  TreeDropMesh M;
  if ((r = M.init (tr))) return r;
  if ((r = tree_tag_variable (tr, &tag))) return r;
  if ((r = M.labels (c, n))) return r;
  return drop_tags (M, M.S->W, tag, *n, false, false);
}

int gfship_tree_tag_droplets_time (gfship_tree * tr, int c_var, int reps, double * ms)
{
  GFSHIP_CHECK (tr && reps > 0 && ms, GFSHIP_EINVAL, "invalid argument");
  unsigned n;
  int r = gfship_tree_tag_droplets (tr, c_var, &n);      /* warm-up: the plan and the work arrays exist afterwards */
  if (r) return r;
  TreeView V;
  tree_view (tr, &V);
  hipEvent_t ev[2] = { nullptr, nullptr };
  hipError_t e = hipEventCreate (&ev[0]);
  if (e == hipSuccess) e = hipEventCreate (&ev[1]);
  if (e == hipSuccess) e = hipEventRecord (ev[0], V.stream);
  for (int q = 0; q < reps && e == hipSuccess && !r; q++)
    r = gfship_tree_tag_droplets (tr, c_var, &n);
  if (e == hipSuccess && !r) e = hipEventRecord (ev[1], V.stream);
  if (e == hipSuccess && !r) e = hipEventSynchronize (ev[1]);
  float t = 0.f;
  if (e == hipSuccess && !r) e = hipEventElapsedTime (&t, ev[0], ev[1]);
  for (hipEvent_t x : ev)
    if (x) (void) hipEventDestroy (x);
  if (r) return r;
  GFSHIP_HIP (e);
  *ms = (double) t/reps;
  return GFSHIP_OK;
}

int gfship_tree_remove_droplets (gfship_tree * tr, int c_var, int v_var, int min, double val)
{
  GFSHIP_CHECK (tr != nullptr, GFSHIP_EINVAL, "gfship_tree_remove_droplets: null tree");
  double * c = nullptr, * v = nullptr;
  int r;
  if ((r = tdrop_variable (tr, c_var, "gfs_domain_remove_droplets", &c))) return r;
  if ((r = tdrop_variable (tr, v_var, "gfs_domain_remove_droplets", &v))) return r;
  TreeDropMesh M;
  if ((r = M.init (tr))) return r;
  unsigned n = 0, umin = 0;
  if ((r = M.labels (c, &n))) return r;
  if (!(n > 0 && -(long) min < (long) n)) return GFSHIP_OK;      /* src/domain.c:3851 */
  if ((r = drop_tags (M, M.S->W, nullptr, n, true, true))) return r;
  if ((r = drop_min (M.stream, M.S->W, n, min, &umin))) return r;
  return M.reset (v, umin, val);
}

int gfship_tree_droplet_to_particle_create (gfship_droplet_to_particle ** out, gfship_particles * pl, int c_var,
					    int min, double reset, double density, const char * function, int nvars,
					    const char * const * names, const int * vars)
{
  GFSHIP_CHECK (out != nullptr, GFSHIP_EINVAL, "null output pointer");
  *out = nullptr;
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_tree_droplet_to_particle_create");
  int r = feed_names_check (nvars, names, vars, "variable of the tree");
  if (r) return r;
  GFSHIP_CHECK (c_var != GFSHIP_TREE_TAG && tree_feed_variable (pl, c_var), GFSHIP_EINVAL,
		"c: the tree has no variable %d", c_var);
  for (int q = 0; q < nvars; q++)
    GFSHIP_CHECK (vars[q] != GFSHIP_TREE_TAG && tree_feed_variable (pl, vars[q]), GFSHIP_EINVAL,
		  "`%s': the tree has no variable %d", names[q], vars[q]);
  TreeDropMesh M;
  if ((r = M.init (pl->tree))) return r;
  gfship_droplet_to_particle * d = new gfship_droplet_to_particle;
  d->pl = pl; d->c = d->mask = c_var; d->min = min; d->reset = reset; d->density = density;
  if (function) {
    std::string text (function);
    const size_t b = text.find_first_not_of (" \t\r\n"), e = text.find_last_not_of (" \t\r\n");
    text = b == std::string::npos ? std::string () : text.substr (b, e - b + 1);
    bool variable = false;
    for (int q = 0; q < nvars && !variable; q++)
      if (text == names[q]) {      /* gfs_function_get_variable: the function is that variable */
	d->mask = vars[q];
	variable = true;
      }
    if (!variable) {
      d->mask = -1;
      if (text_constant (function, &d->value)) d->constant = true;
      else {
	const std::vector<const char *> named = named_variables (function, nvars, names, vars, d->read);
	if ((r = rtc_compile_tree_cell (M.V.device, pl->dim, function, (int) named.size (), named.data (), &d->fn))) {
	  gfship_droplet_to_particle_destroy (d);
	  return r;
	}
      }
      /* the values of the function at every cell of the concatenated levels; 0 where the tree has no interior cell */
      hipError_t e1 = hipMalloc ((void **) &d->fv, (size_t) M.V.ncell*sizeof (double));
      if (e1 == hipSuccess) e1 = hipMemsetAsync (d->fv, 0, (size_t) M.V.ncell*sizeof (double), M.stream);
      if (e1 != hipSuccess) {
	gfship_droplet_to_particle_destroy (d);
	GFSHIP_HIP (e1);
      }
    }
  }
  *out = d;
  return GFSHIP_OK;
}

} // extern "C"
