// tree_tape.hpp -- the compiled stencils of a sweep: the evaluation of the streams that the planner writes
// (tape_cell_gen, tree_plan.hip), shared by the kernels of tree.hip and by the host checks.
//
// relax_cell / face_gradient (tree.hpp) walk the tree for every cell of every sweep: a chain of
// dependent loads (neighbour table, flags, children, values) that one thread pays in full, and the
// slowest cell of a dependency level -- a coarse leaf with fine neighbours reads ~40 values through
// two levels of interpolation -- sets the time of the level.  The tree does not change: the host
// walks it once per cell and writes down what the walk found: which values are
// read, with which constant coefficients, combined in which order.  The sweep kernel stages the
// streams of a chunk of cells in LDS together with the gathered values (one independent load per
// thread), then evaluates them from LDS: same operations in the same order as the template code.
#pragma once
#include <hip/hip_runtime.h>

namespace gfship { namespace tree {

enum { K_NONE = 0, K_SAME = 1, K_FC = 2, K_DEEP = 3, K_GHOST = 4 };

#define TAPE_LDS_BYTES (120*1024)    /* the streams and values of a chunk of cells (lds_chunks, tree_plan.hip) */

struct TapeCursor {          // the streams of a cell, the values gathered beforehand (LDS / host)
  const int * ti; const double * td; const double * tv;
  __host__ __device__ inline double val () { return *tv++; }
};

// p.b of interpolate_1D1 / interpolate_2D1 from the streams: sum of a_j * P_j, P_j a value or the
// average of the children of a refined neighbour (average_neighbor_value)
template <class CUR>
__host__ __device__ inline double tape_interpolation (CUR & c)
{
  const int nt = *c.ti++;
  double pb = 0.;
  for (int t = 0; t < nt; t++) {
    const double a = *c.td++;
    const int cnt = *c.ti++;
    double P;
    if (cnt == 0)
      P = c.val ();
    else {
      double av = 0., n = 0.;
      for (int k = 0; k < cnt; k++) {
	n += 1.;
	av += 1.*(c.val ());
      }
      P = av/n;
    }
    pb += a*P;
  }
  return pb;
}

// the sums g.a, g.b of relax / residual_set over the faces of a cell (src/poisson.c:507-557,634-678)
// w: the weight every face carries (1. for the Poisson problem with alpha = NULL; the diffusion
// coefficient of a quadtree, face_gradient_w of tree.hpp) -- the products by 1. leave the bits alone
template <class CUR>
__host__ __device__ inline void tape_cell (CUR & c, int nd, int dim, int ncd, double & ga, double & gb,
					   double w = 1.)
{
  ga = 0.; gb = 0.;
  for (int d = 0; d < nd; d++) {
    const int kind = *c.ti++;
    if (kind == K_NONE)
      continue;
    double na, nb;
    if (kind == K_SAME) {
      na = w;
      nb = w*(c.val ());
    }
    else if (kind == K_FC) {      /* gradient_fine_coarse towards a coarser neighbour */
      const double cb = *c.td++;
      const double uN = c.val ();
      const double pb = tape_interpolation (c);
      const double gc = 2.*pb/3.;
      na = w*(2./3.);
      nb = w*(cb*uN + gc);
    }
    else {                        /* the fine cells behind a face of a coarser leaf */
      const int nch = *c.ti++;
      na = 0.; nb = 0.;
      for (int i = 0; i < nch; i++) {
	const double gbi = *c.td++;
	const double uch = c.val ();
	const double pb = tape_interpolation (c);
	const double gc = 2.*pb/3.;
	na += w*gbi;
	nb += w*((2./3.)*uch - gc);
      }
      if (dim > 2) {
	na /= ncd/2.;
	nb /= ncd/2.;
      }
    }
    ga += na;
    gb += nb;
  }
}

} } // namespace gfship::tree
