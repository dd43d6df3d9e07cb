// tree_plan.hpp -- the plans of a refined tree: everything the host works out once about a static tree, as plain
// structs of std::vector.  The planner (tree_plan.hip) is host C++ that never touches a device; tree.hip uploads a
// plan (one function per type) and runs it; the host checks (gfship_tree_host_check ...) run it on the host.
#pragma once
#include "tree.hpp"
#include "tree_flow_ops.hpp"
#include "switches.hpp"
#include <optional>
#include <vector>

namespace gfship { namespace tree {

struct FaceRec { Cell cell, neighbor; int d; };
struct Ghost { int g, img, side, l; };   // img: the periodic image, or the cell the ghost touches (GfsBoundary)
struct Sgn6 { double s[6]; };            // homogeneous condition of each side: ghost = s * cell

// the tree on the host.  H reads the vectors below: a TreePlan is moved, never copied
struct TreePlan {
  Topo H;
  int ncell = 0;
  std::vector<unsigned char> hflag, h_cmask, h_idtab;
  std::vector<int> h_nbtab, h_child0;
  std::vector<Cell> hleaves;                      // interior leaves in traversal order
  std::vector<std::vector<Cell>> hnonleaf;        // interior non-leaf cells of each level below the deepest
  std::vector<Ghost> hghost_leaves;
  int side[6] = { 0, 0, 0, 0, 0, 0 };             // GFSHIP_SIDE_PERIODIC / GFSHIP_SIDE_BOUNDARY
  bool has_boundary = false;
  TreePlan () = default;
  TreePlan (TreePlan &&) = default;
  TreePlan & operator= (TreePlan &&) = default;
};

// the sweep of gfs_relax on level m (T_LEVEL_LEAFS) in dependency levels, with its compiled stencils: per cell,
// in the order of `cells', a stream of codes / counts (ti), of constant coefficients (td) and of the cells whose
// values it reads (tv); the cells of a dependency level in chunks that fit the LDS
struct SweepPlan {
  int nlev = 0;
  std::vector<Cell> cells;             // sorted by level (stable: traversal order inside)
  std::vector<int> lev_off;            // nlev + 1
  std::vector<Ghost> ghosts;           // ghost cells of the selection
  std::vector<int> ti, tv;
  std::vector<double> td;
  std::vector<int> cell_off;           // 3*(ncells + 1): start of each cell in ti / td / tv
  std::vector<int> chunk;              // first cell of each chunk + end marker
  std::vector<int> g;                  // the index of each cell in the concatenated arrays
};

// the relax loop as a dataflow program of micro-operations (tree_flow.hpp).  The loop works on copies of the
// values and of the right-hand side in the ORDER OF THE PLAN (the cells in the order their operations first
// appear): the cells of a level, and their neighbours on the next, are then next to each other in memory -- in
// the tree's own arrays (one dense array per level) the cells of a dependency level lie on a skew hyperplane
// and every 8-byte value costs a 128-byte line from the L2
struct FlowProgram {
  int nlev = 0, nops = 0, nct = 0, npos = 0;
  int width = FLOW_WIDTH;              // operations per level at most = threads of the launch
  std::vector<FlowRec> rec;            // + the records the kernel loads ahead of the last level and on idle lanes
  std::vector<int> lev_off;
  std::vector<double> ct;              // never empty
  std::vector<int> gidx;               // the cell at each place, + spare places the idle lanes load
};

// a whole relax loop (nrelax sweeps + the copies of the ghosts between them) as ONE list of nodes in dependency
// levels: sweep s + 1 of a cell starts as soon as what it reads is final
struct LoopPlan {
  unsigned nrelax = 0;
  int nlev = 0;
  std::vector<int> ti, tv, node_off, node_g, node_level, chunk;
  std::vector<double> td;
  // the same plan for t_relax_nodes_pf: per chunk { c0, c1, i0, i1, d0, d1, v0, v1 }, per node { start in ti, td,
  // tv, cell } -- one load each, issued a chunk ahead
  std::vector<int> desc, rec;
  double sg[6] = { 0., 0., 0., 0., 0., 0. };   // the homogeneous conditions compiled into the copies of the ghosts
  std::optional<FlowProgram> flow;             // the same loop for t_relax_flow (none: not expressible)
  int nnodes () const { return (int) node_g.size (); }
  int nchunks () const { return (int) chunk.size () - 1; }
};

struct FacePlan {           // the faces of one ftt_face_traverse, in its order
  std::vector<FaceRec> faces;
  std::vector<int> inc_off;            // per leaf (position in the leaf list) + 1
  std::vector<int> inc;                // face << 1 | role (0: the cell of the face, 1: its neighbour)
};

// everything gfship_tree_create plans before it touches the device, with the GFSHIP_* switches of the moment
struct TreePlans {
  Switches sw;
  TreePlan T;
  std::vector<SweepPlan> sweep;        // of every level
  FacePlan faces[4];                   // 0: FTT_XYZ, 1 + c: the faces normal to c
};

// gfs_domain_tag_droplets (src/domain.c:3727-3796) on a static tree, DESIGN.md 11.41: the face contacts of the interior
// leaves.  A label is the position of a leaf in hleaves.  con_off[p] .. con_off[p + 1]: the contacts of leaf p with
// leaves of lower position.  gate < 0: two leaves of one level.  Otherwise a fine leaf f beside a coarser leaf k, and
// gate = (index in the concatenated levels of the cell N beside k that holds f, the one whose value of c decides
// whether the fill steps from k into f, tag_cell_fraction :3577) << 1 | (leaf p is the fine end)
struct DropContact { unsigned other; int gate; };
struct DropletPlan {
  std::vector<int> con_off;            // nleaves + 1
  std::vector<DropContact> con;
  std::vector<unsigned> periodic;      // pairs (p, q < p) of leaves of one level that meet through a periodic side
  std::vector<unsigned char> on_side;  // per leaf: it touches a side of the box, periodic or not
  std::vector<unsigned> cells;         // per cell of the concatenated levels: itself if it is an interior cell of the
                                       // tree (a leaf or not: compute_v runs over FTT_TRAVERSE_ALL), else 0xFFFFFFFF
  unsigned ngated = 0;                 // contacts with a gate: the one-way records of a call are at most as many
};
int plan_droplets (const TreePlan & T, DropletPlan & out);
// the closed form of the fill on the host: tag[p] of every leaf (0 outside the mask) from the values c of every cell
// of the concatenated levels; returns the number of droplets
unsigned droplet_tags_host (const TreePlan & T, const DropletPlan & P, const double * c, std::vector<unsigned> & tag);

// gfs_refine_refine + gfs_simulation_refine with the corner rule, gfs_domain_match, the tables of Topo, the lists of
// cells, the sweeps and the face sets; side: nullptr = all periodic.  Returns GFSHIP_OK or the error of
// gfship_tree_create; no exception leaves it
int plan_tree_create (int dim, gfship_refine_fn refine, void * ctx, const int * side, TreePlans & out);
// flow_width, debug: Switches::flow_width (0: chosen by dimension), Switches::tree_debug
int plan_loop (const TreePlan & T, const SweepPlan & S, int m, unsigned nrelax, const Sgn6 & sg, int flow_width,
	       bool debug, LoopPlan & out);

// the device runs the diffusion stencils of a tree with the same weight w on every face (WConst): true when every
// coefficient that diffusion_relax / _residual / _rhs read on this tree, on any level of the multigrid cycle, is w
// for every w (a coefficient of another form would make the device differ from the reference: refused)
bool diffusion_weights_exact (const Topo & T);

inline Cell root_cell (const Topo & T) { return T.make (0, 1, 1, 1); }

// the homogeneous form of the conditions (gfs_domain_homogeneous_bc): ghost = s * cell; of P ...
inline Sgn6 homogeneous_signs (const int * side, const int * bc_p)
{
  Sgn6 sg;
  for (int d = 0; d < 6; d++)
    sg.s[d] = side[d] != GFSHIP_SIDE_PERIODIC && bc_p[d] == GFSHIP_BC_DIRICHLET ? -1. : 1.;
  return sg;
}
// ... and of velocity component c (in the relax loops of its diffusion solve)
inline Sgn6 homogeneous_signs_u (const int * side, const int * bc_u, int c)
{
  Sgn6 sg;
  for (int d = 0; d < 6; d++) {
    sg.s[d] = 1.;
    if (side[d] != GFSHIP_SIDE_PERIODIC) {
      const int k = bc_u[d];
      sg.s[d] = k == GFSHIP_BC_DIRICHLET ? -1. : k == GFSHIP_BC_NEUMANN ? 1. : (c == d/2 ? -1. : 1.);
    }
  }
  return sg;
}

} } // namespace gfship::tree
