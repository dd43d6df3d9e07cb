// tree_particles.hpp -- what the point sampler and the tracers (tree_particles.hip) see of a gfship_tree
// (tree.hip keeps the struct to itself).
#pragma once
#include "tree.hpp"

namespace gfship {

namespace tree { struct DropletPlan; }

// a leaf found by a descent: g = Topo::gi; i, j, k: the indices in the dense level (with ghosts)
struct Leaf { int l, q, g, i, j, k; };

// ftt_cell_locate (root, target, -1), src/ftt.c:1535-1574, on the unit box centred on the origin, over the tables of
// the tree on the device: S.T is the Topo of the device
template <int DIM, class Tables>
__device__ __forceinline__ bool tree_locate (const Tables & S, const double target[3], Leaf & c)
{
  double pos[3] = { 0., 0., 0. };
  double size = 1./2.;
#pragma unroll
  for (int a = 0; a < DIM; a++)
    if (target[a] > pos[a] + size || target[a] < pos[a] - size)
      return false;
  int l = 0, i = 1, j = 1, k = DIM == 3 ? 1 : 0;
  int q = 1 + 3*(1 + (DIM == 3 ? 3 : 0));
  int g = S.T.off[0] + q;
  while (l < S.T.depth && S.T.cmask[g] != 0) {
    const bool ux = target[0] > pos[0], uy = target[1] > pos[1], uz = DIM == 3 && target[2] > pos[2];
    const int rr = (2 << l) + 2;
    q = S.T.child0[g] + (ux ? 1 : 0) - (uy ? 0 : rr) - (DIM == 3 && !uz ? rr*rr : 0);
    i = 2*i - 1 + (ux ? 1 : 0);
    j = 2*j - (uy ? 0 : 1);
    if (DIM == 3) k = 2*k - (uz ? 0 : 1);
    size /= 2.;
    pos[0] += (ux ? 1. : -1.)*size;
    pos[1] += (uy ? 1. : -1.)*size;
    if (DIM == 3) pos[2] += (uz ? 1. : -1.)*size;
    l++;
    g = S.T.off[l] + q;
  }
  c.l = l; c.q = q; c.g = g; c.i = i; c.j = j; c.k = k;
  return true;
}

struct TreeView {
  tree::Topo H, D;                  // the tables of the tree on the host and on the device
  hipStream_t stream;
  int device, ncell, nleaves;
  const tree::Cell * hleaves;       // host: interior leaves in traversal order
  const tree::Cell * dleaves;       // device: the same
  const int * side;                 // GFSHIP_SIDE_* of the 2*dim sides
  double dt, t;
  double viscosity;                 // of U (gfship_tree_set_viscosity (tree, 0, nu)); 0.: no GfsSourceDiffusion
  double * uprev[3];                // GFSHIP_TREE_UPREV ...; nullptr until tree_previous_vel has run
  // the tables of the sampler, built on first use and freed with the tree
  void ** sampler;
  void (** sampler_free) (void *);
};

void tree_view (gfship_tree * tr, TreeView * v);
// the device array (all levels) of the variable GFSHIP_TREE_* `var'; nullptr: no such variable
double * tree_variable (gfship_tree * tr, int var);
// store_domain_previous_vel on the tree: GFSHIP_TREE_UPREV ... = U, V, W of this moment (allocates them the first time)
int tree_previous_vel (gfship_tree * tr);
int tree_device (gfship_tree * tr);
// the device array of GFSHIP_TREE_VF, _FX, _FY, _FZ, allocated zeroed (every level, ghost cells included) by the
// first call that needs it; GFSHIP_EINVAL for another variable and for _FZ on a quadtree
int tree_coupling_variable (gfship_tree * tr, int var, double ** out);
// the same for GFSHIP_TREE_RAD, _URELP, _VRELP, _WRELP, _VOLSRC, _DMDT; GFSHIP_EINVAL for another variable and for
// _WRELP on a quadtree
int tree_source_variable (gfship_tree * tr, int var, double ** out);
// does the tree have the variable `var' now?  tree_variable () != nullptr, and for GFSHIP_TREE_T0, _T1 a tracer of
// gfship_tree_add_tracer behind it
bool tree_has_variable (gfship_tree * tr, int var);
// the device array of GFSHIP_TREE_TAG, allocated zeroed by the first call that needs it
int tree_tag_variable (gfship_tree * tr, double ** out);
// the droplet plan of the tree (tree_plan.hpp), made by the first call, and the place where tree_droplets.hip keeps
// its device copy and its work arrays; the tree frees them with itself
struct TreeDropletSlot {
  const tree::DropletPlan * plan;
  void ** state;
  void (** state_free) (void *);
};
int tree_droplet_plan (gfship_tree * tr, TreeDropletSlot * slot);
// gfs_domain_bc of a scalar with the default GfsBc: the ghost leaves of v (all levels) from the cells they touch or
// their periodic images
int tree_bc_scalar (gfship_tree * tr, double * v);

}
