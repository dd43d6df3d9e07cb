// tree_particles.hpp -- what the point sampler and the tracers (tree_particles.hip) see of a gfship_tree
// (tree.hip keeps the struct to itself).
#pragma once
#include "tree.hpp"

namespace gfship {

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

}
