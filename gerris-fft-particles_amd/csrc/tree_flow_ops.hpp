// tree_flow_ops.hpp -- the micro-operations of a flow plan (tree_flow.hpp has the account and the kernels,
// tree_plan.hip the planner): the record format and the arithmetic of one operation, shared by the kernel
// t_relax_flow and by the emulator of the host checks (flow_emulate).  Everything here is plain
// __host__ __device__ code.
#pragma once
#include <hip/hip_runtime.h>

namespace gfship { namespace tree {

enum { F_CELL = 0, F_FC = 1, F_CHILD = 2, F_SUM = 3, F_GHOST = 4, F_NOP = 5 };
enum { FK_NONE = 0, FK_SAME = 1, FK_PAIR = 2 };
#define FLOW_WIDTH  512             /* most operations per level = threads of the workgroup; a plan may use fewer */
#define FLOW_PD     1               /* old values are loaded FLOW_PD levels ahead, records FLOW_PD + 2 */
#define FLOW_NBUF   (FLOW_PD + 2)   /* a result stays in the LDS for FLOW_PD + 1 levels: its store is issued a level late */
#define FLOW_NIN    10
#define FLOW_NCONST 128
// an input of a record: < 0: the result of an operation of one of the last FLOW_PD levels, bits 4-14 = its
// slot (level % FLOW_NBUF)*FLOW_WIDTH + operation (i.e. bits 0-14 = its byte address in the LDS);
// >= 0: a cell, as the byte offset 8 g of its value in global memory.  out_g: the same offset, or -1
#define FLOW_IS_LDS(ref)  ((ref) < 0)
#define FLOW_LDS_REF(slot) ((int) (0x80000000u | ((unsigned) (slot) << 4)))
#define FLOW_LDS_ADDR(ref) ((ref) & 0x7ff0)
#define FLOW_NONE   FLOW_LDS_REF (FLOW_LDS_SLOTS - 1)      /* no input: a slot no operation writes */
#define FLOW_LDS_SLOTS 2048         /* 32 KB: any masked address stays inside */
#define FLOW_MAXLEV  5900            /* levels of a plan (their first operations sit in the LDS) */

struct __attribute__((aligned(16))) FlowRec { unsigned w0; int out_g; int in[FLOW_NIN]; };
// w0: bits 0-2 the kind
//   CELL   3-14 the kind of each face (FK_*), 15-19 the level of the cell, 20: reads its own value
//          in[0] the cell itself, in[1 + d] the neighbour (FK_SAME) or the pair of the face (FK_PAIR)
//   FC / CHILD  3-4 terms of the interpolation, 5-7 / 8-10 cells averaged in term 0 / 1 (0: one
//          value), 11-17 / 18-24 / 25-31 the constants cb (gbi), a0, a1 in the table
//          in[0] the coarse neighbour (the child), in[1 + TS t + k] value k of term t
//   SUM    3-5 children;  in[i] the pair of child i
//   GHOST  11-17 the constant (the sign of the homogeneous condition);  in[0] the image
// The operations of a level are sorted by kind (CELL | FC, CHILD | SUM, GHOST), each kind starting at a multiple of
// 64 when the plan is 256 wide at least (the schedule keeps the room): a wavefront runs one branch of flow_eval

template <int DIM> struct FlowShape {
  static constexpr int TS = DIM == 3 ? 4 : 2;            /* values of one interpolation term */
  static constexpr int NIN = DIM == 3 ? 9 : 5;           /* inputs a record of this dimension uses */
};

struct __attribute__((aligned(16))) FlowPair { double x, y; };

// one micro-operation, arithmetic only.  x[j]: the input j (a value from global memory or the result of an
// operation of the previous level), y[j]: the second number of the pair when input j is a pair; rh: the
// right-hand side of a CELL; ct: the constants
template <int DIM>
__host__ __device__ inline FlowPair flow_eval (unsigned w0, const double * x, const double * y, double rh,
					       const double * ct, double omega, int op, double w)
{
  constexpr int TS = FlowShape<DIM>::TS;
  const int kind = w0 & 7;
  FlowPair o = { 0., 0. };
  if (kind == F_CELL) {
    double ga = 0., gb = 0.;
#pragma unroll
    for (int d = 0; d < 2*DIM; d++) {
      const int fk = (w0 >> (3 + 2*d)) & 3;
      if (fk == FK_SAME) {
	const double na = w, nb = w*x[1 + d];
	ga += na; gb += nb;
      }
      else if (fk == FK_PAIR) {
	ga += y[1 + d]; gb += x[1 + d];
      }
    }
    if (op == 0) {
      double r = 0.;
      if (ga != 0.) {
	const double t = gb - rh;
	const double q = ga == 4. ? t*0.25 : t/ga;      /* t/4 and t*0.25 are the same number */
	if (DIM == 2)
	  r = (1. - omega)*x[0] + omega*q;
	else
	  r = q;
      }
      o.x = r;
    }
    else {      /* diffusion_relax, src/poisson.c:1471-1498 (rhoc = 1) */
      const int l = (w0 >> 15) & 31;
      const double h = 1./(1 << l);
      const double a = 1.*h*h;
      ga = 1. + ga/a;
      o.x = (gb/a + rh)/ga;
    }
  }
  else if (kind == F_FC || kind == F_CHILD) {
    const int nt = (w0 >> 3) & 3;
    double pb = 0.;
#pragma unroll
    for (int t = 0; t < DIM - 1; t++)
      if (t < nt) {
	const double a = ct[(w0 >> (18 + 7*t)) & 127];
	const int cnt = (w0 >> (5 + 3*t)) & 7;
	double P;
	if (cnt == 0)
	  P = x[1 + TS*t];
	else {
	  double av = 0., n = 0.;
#pragma unroll
	  for (int k = 0; k < TS; k++)
	    if (k < cnt) {
	      n += 1.;
	      av += 1.*x[1 + TS*t + k];
	    }
	  /* av/n; n = 1, 2, 4: the product by 1/n is the same number, without the division */
	  P = n == 4. ? av*0.25 : n == 2. ? av*0.5 : n == 1. ? av : av/n;
	}
	pb += a*P;
      }
    const double gc = 2.*pb/3.;
    const double c0 = ct[(w0 >> 11) & 127];
    if (kind == F_FC) {
      o.y = w*(2./3.);
      o.x = w*(c0*x[0] + gc);
    }
    else {
      o.y = w*c0;
      o.x = w*((2./3.)*x[0] - gc);
    }
  }
  else if (kind == F_SUM) {
    const int nch = (w0 >> 3) & 7;
    double na = 0., nb = 0.;
#pragma unroll
    for (int i = 0; i < (DIM == 3 ? 4 : 2); i++)
      if (i < nch) {
	na += y[i];
	nb += x[i];
      }
    if (DIM > 2) {
      na /= 4/2.;
      nb /= 4/2.;
    }
    o.x = nb; o.y = na;
  }
  else if (kind == F_GHOST)
    o.x = ct[(w0 >> 11) & 127]*x[0];
  return o;
}

// The same operations without a branch, for a wavefront whose lanes all run the same kind (the operations of
// a level are sorted by kind): what a lane does not have is added as + 0. -- the sums start from + 0. and a
// sum that starts from + 0. is never - 0., so x + 0. = x bit for bit -- and selected afterwards.  The branches
// of flow_eval cost more than its arithmetic (46 exec-mask branches per operation).  Divisions: one per
// operation (t/ga; 2 pb/3); av/n is a product for n = 1, 2, 4 and a division, behind a branch the whole
// wavefront takes together, when a lane has n = 3.
template <int DIM, int KIND, class ANY>
__host__ __device__ inline FlowPair flow_eval_uniform (unsigned w0, const double * x, const double * y, double rh,
						       const double * ct, double omega, int op, double w, const ANY & any)
{
  constexpr int TS = FlowShape<DIM>::TS;
  FlowPair o = { 0., 0. };
  if (KIND == F_CELL) {
    double ga = 0., gb = 0.;
#pragma unroll
    for (int d = 0; d < 2*DIM; d++) {
      const int fk = (w0 >> (3 + 2*d)) & 3;
      const double na = fk == FK_SAME ? w : fk == FK_PAIR ? y[1 + d] : 0.;
      const double nb = fk == FK_SAME ? w*x[1 + d] : fk == FK_PAIR ? x[1 + d] : 0.;
      ga += na; gb += nb;
    }
    if (op == 0) {
      const double q = (gb - rh)/ga;
      const double r = DIM == 2 ? (1. - omega)*x[0] + omega*q : q;
      o.x = ga != 0. ? r : 0.;
    }
    else {
      const int l = (w0 >> 15) & 31;
      const double h = 1./(1 << l);
      const double a = 1.*h*h;
      ga = 1. + ga/a;
      o.x = (gb/a + rh)/ga;
    }
  }
  else if (KIND == F_FC) {      /* FC and CHILD */
    const int nt = (w0 >> 3) & 3;
    double pb = 0.;
#pragma unroll
    for (int t = 0; t < DIM - 1; t++) {
      const double a = ct[(w0 >> (18 + 7*t)) & 127];
      const int cnt = (w0 >> (5 + 3*t)) & 7;
      double av = 0.;
#pragma unroll
      for (int k = 0; k < TS; k++)
	av += k < cnt ? 1.*x[1 + TS*t + k] : 0.;
      double P = cnt == 4 ? av*0.25 : cnt == 2 ? av*0.5 : av;      /* av/n, n = 4, 2, 1 */
      if (any (t < nt && cnt == 3)) {
	const double n3 = 3.;
	P = cnt == 3 ? av/n3 : P;
      }
      P = cnt == 0 ? x[1 + TS*t] : P;
      pb += t < nt ? a*P : 0.;
    }
    const double gc = 2.*pb/3.;
    const double c0 = ct[(w0 >> 11) & 127];
    const bool fc = (w0 & 7) == F_FC;
    o.y = fc ? w*(2./3.) : w*c0;
    o.x = fc ? w*(c0*x[0] + gc) : w*((2./3.)*x[0] - gc);
  }
  else if (KIND == F_SUM) {
    const int nch = (w0 >> 3) & 7;
    double na = 0., nb = 0.;
#pragma unroll
    for (int i = 0; i < (DIM == 3 ? 4 : 2); i++) {
      na += i < nch ? y[i] : 0.;
      nb += i < nch ? x[i] : 0.;
    }
    if (DIM > 2) {
      na /= 4/2.;
      nb /= 4/2.;
    }
    o.x = nb; o.y = na;
  }
  else if (KIND == F_GHOST)
    o.x = ct[(w0 >> 11) & 127]*x[0];
  return o;
}

// the kind all the operations of a wavefront share (NOPs apart), or -1
__host__ __device__ inline int flow_class (int kind) { return kind == F_CHILD ? F_FC : kind; }

} } // namespace gfship::tree
