// switches.hpp -- the GFSHIP_* environment switches of libgfship, in one table.
// Every switch is looked up when a domain (gfship_domain_create) or a tree (gfship_tree_create) is
// created and kept in its `sw' member: nothing is read once per process, nothing per call.
// Plain C++ (no HIP): a host compiler builds it alone (tests/test_switches_table_cpu.py).
#pragma once

#include <algorithm>
#include <cstdlib>

namespace gfship {

struct Switches {
  // --- Godunov kernels (timestep_kernels.hip, simulation.hip)
  bool advect_sweep = true;        // the sweeps along z; off: the tiled kernels
  bool mpi_sweep = true;           // ... on boxes with MPI sides
  bool advect_sweep1 = false;      // advect3_sweep_kernel instead of advect3_sweep2_kernel
  bool advect3 = true;             // the three velocity components at once; off: one launch per component
  bool fused_mpi = true;           // tiled kernels on boxes with MPI sides; off: face-value arrays
  bool fused_divergence = true;    // the divergence of the MAC projection left by the predictor's sweep
  bool fused_correction = true;    // gfs_correct_centered_velocities in the pass of the advection
  bool lazy_un = true;             // the MAC velocities of the approximate projection stay unstored
  bool project_pairs = true;       // projection updates with two cells per thread; off: one
  // --- the multigrid cycle (poisson.hip, poisson_kernels.hip, relax_*.hip)
  bool residual_pairs = true;      // residual (and its norm) with two cells per thread; off: one
  int rn_blocks = 0;               // workgroups of the residual norm (64..8192, anything else: 4096)
  int coarse_threads = 1024;       // threads of coarse_cycle_kernel (a multiple of 64 up to 1024)
  bool rows2d = true;              // 2-D sweeps by rows; off: one launch per hyperplane
  bool diffusion_pipelined = true; // diffusion relax loops on the pipelined tile kernels; off: hyperplanes
  bool weighted_pipelined = true;  // the same for the sweeps with face weights
  bool lattice_cycle = true;       // the coarse end of a lattice of boxes replicated on every rank; off (also
                                   // after a barrier of that kernel timed out): one exchange per sweep and level
  bool fused_restriction = true;   // off: restrict_kernel, then the copy of the rhs
  bool fused_prolongation = true;  // off: prolongate_kernel, then the copy
  bool old_prolong_pack = false;   // the prolongation by the transposing copy instead of patch_prolong_kernel
  bool arm_ahead = true;           // hand-off granules armed on the side stream; off: in line, before the loop
  bool kernel_arming = false;      // the loop kernels arm the other granule set (measured: no gain)
  bool xcd_scope = false;          // XCD blocks of tiles + narrower-scope stores towards same-XCD consumers (measured: no gain)
  int xcd_near_mode = 2;           // ... 2: workgroup-scope stores, 1: plain stores, 0: as without
  bool xcd_place = false;          // XCD-aware tile placement in the loop kernel (experiment)
  bool wave_loop = false;          // fused relax loops by the experimental one-wave-per-tile kernel
  bool skew_old = false;           // single sweeps by the older four-wave kernel
  bool skew_lines = false;         // one line per thread on every level
  int patch_min_n = 128;           // 2 x 2 lines per lane from this n on: on 64^3 and 32^3 (16 and 4 tiles) one line per thread is a few us faster
  bool patch_regs = false;         // the 2 x 2 variant that streams through registers
  bool skew_stats = false;         // debug: per-tile timings of the relax loops on stderr
  // --- refined trees (tree.hip)
  bool tree_residual_tape = true;  // off: the residual by the code that walks the tree
  bool tree_template_relax = false;// the stencil code walks the tree in every sweep
  bool tree_pipeline = true;       // off: sweep after sweep (t_relax_tape)
  bool tree_flow = true;           // off: the tape kernels (t_relax_nodes_pf)
  bool tree_prefetch = true;       // off: t_relax_nodes (every load in place)
  int flow_width = 0;              // lab: operations per level of a flow plan (a multiple of 64); 0: chosen by dimension
  bool tree_debug = false;         // debug: the plans of the tree solver on stderr

  // 2 x 2 lines per lane (relax_patch_loop.hip) on the levels where it wins
  bool patch () const { return !skew_lines && !skew_old; }
};

inline bool env_set (const char * name) { return getenv (name) != nullptr; }     // any value, "0" included
inline bool env_is_1 (const char * name) { const char * e = getenv (name); return e && e[0] == '1'; }
inline int env_int (const char * name, int unset) { const char * e = getenv (name); return e ? atoi (e) : unset; }

// The table: one line per variable.  Three more are read elsewhere: GFSHIP_FAULT_DROP_HANDOFF
// (relax_skew_loop.hip), GFSHIP_RCCL_LIBRARY (transport.hip) and GFSHIP_CC (host/gfs_function.hpp).
inline Switches read_switches ()
{
  Switches s;
  s.advect_sweep = !env_set ("GFSHIP_NO_ADVECT_SWEEP");
  s.mpi_sweep = !env_set ("GFSHIP_NO_MPI_SWEEP");
  s.advect_sweep1 = env_set ("GFSHIP_ADVECT_SWEEP1");
  s.advect3 = !env_set ("GFSHIP_NO_ADVECT3");
  s.fused_mpi = !env_set ("GFSHIP_NO_FUSED_MPI");
  s.fused_divergence = !env_set ("GFSHIP_NO_FUSED_DIVERGENCE");
  s.fused_correction = !env_set ("GFSHIP_NO_FUSED_CORRECTION");
  s.lazy_un = !env_set ("GFSHIP_NO_LAZY_UN");
  s.project_pairs = !env_set ("GFSHIP_PC_SCALAR");
  s.residual_pairs = !env_set ("GFSHIP_RN_SCALAR");
  s.rn_blocks = env_int ("GFSHIP_RN_BLOCKS", 0);
  s.coarse_threads = env_int ("GFSHIP_COARSE_THREADS", 1024);
  s.rows2d = !env_set ("GFSHIP_NO_ROWS2D");
  s.diffusion_pipelined = !env_set ("GFSHIP_DIFFUSION_HYPERPLANES");
  s.weighted_pipelined = !env_set ("GFSHIP_WEIGHTED_HYPERPLANES");
  s.lattice_cycle = !env_set ("GFSHIP_NO_LATTICE_CYCLE");
  s.fused_restriction = !env_set ("GFSHIP_NO_FUSED_RESTRICTION");
  s.fused_prolongation = !env_set ("GFSHIP_NO_FUSED_PROLONGATION");
  s.old_prolong_pack = env_set ("GFSHIP_OLD_PROLONG_PACK");
  s.arm_ahead = !env_set ("GFSHIP_NO_ARM_AHEAD");
  s.kernel_arming = env_set ("GFSHIP_KERNEL_ARMING");
  s.xcd_scope = env_set ("GFSHIP_XCD_SCOPE");
  s.xcd_near_mode = env_int ("GFSHIP_XCD_NEAR_MODE", 2);
  s.xcd_place = env_is_1 ("GFSHIP_XCD_PLACE");
  s.wave_loop = env_is_1 ("GFSHIP_WAVE_LOOP");
  s.skew_old = env_set ("GFSHIP_SKEW_OLD");
  s.skew_lines = env_set ("GFSHIP_SKEW_LINES");
  s.patch_min_n = env_int ("GFSHIP_PATCH_MIN_N", 128);
  s.patch_regs = env_set ("GFSHIP_PATCH_REGS");
  s.skew_stats = env_set ("GFSHIP_SKEW_STATS");
  s.tree_residual_tape = !env_int ("GFSHIP_TREE_NO_RESIDUAL_TAPE", 0);
  s.tree_template_relax = env_int ("GFSHIP_TREE_TEMPLATE_RELAX", 0);
  s.tree_pipeline = !env_int ("GFSHIP_TREE_NO_PIPELINE", 0);
  s.tree_flow = !env_int ("GFSHIP_TREE_NO_FLOW", 0);
  s.tree_prefetch = !env_int ("GFSHIP_TREE_NO_PREFETCH", 0);
  s.flow_width = env_set ("GFSHIP_FLOW_WIDTH") ? std::max (64, env_int ("GFSHIP_FLOW_WIDTH", 0)/64*64) : 0;
  s.tree_debug = env_set ("GFSHIP_TREE_DEBUG");
  return s;
}

} // namespace gfship
