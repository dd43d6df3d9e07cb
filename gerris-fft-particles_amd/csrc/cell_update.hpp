// cell_update.hpp -- the same-level cell update and residual of the multigrid solver on uniform boxes,
// once, for the four operator kinds of RelaxOp::kind:
//
//   kind | update                                            | weight source     | reference
//   -----+---------------------------------------------------+-------------------+---------------------------------
//     0  | relax / relax2D                                   | UnitW             | src/poisson.c:507-557, with
//     2  | relax / relax2D, the six f[d].v of each cell      | CellW or ArrayW   | face_weighted_gradient's same-
//        |                                                   |                   | level branch src/fluid.c:858-864
//     1  | diffusion_relax, one weight w per level, h2 = h*h | UniformW { w }    | src/poisson.c:1471-1498, with
//     3  | diffusion_relax, the six f[d].v of each cell, h2  | CellW or ArrayW   | gfs_face_cm_weighted_gradient's
//        |                                                   |                   | same-level branch src/fluid.c:1361-1366
//
// Both branches give g.a = w, g.b = w*u_nb for the face d = 0 .. 2 DIM - 1 = right, left, top, bottom,
// front, back, and the cell sums a += g.a, b += g.b in that order: from dia for relax (then
// u = (b - rhs)/a, over-relaxed by omega in 2-D, 0. where a == 0.), from 0. for diffusion_relax (then, with
// a = dia*h*h and dia the rhoc of the cell, u = (g.b/a + rhs)/(1. + g.a/a)).  The residuals are
// residual_set / residual_set2D (src/poisson.c:634-678) and diffusion_residual (:1534-1569), the flux sum
// is diffusion_rhs (:1392-1451).
//
// Nothing here knows a kernel's layout: a kernel passes sources for what it holds (global memory, LDS,
// registers, a ring) and stores the result where it wants.  Every expression keeps the reference's operand
// order (the library is built with -ffp-contract=off): kinds 0 and 1 are the same source as kinds 2 and 3
// with a weight the compiler knows, a += 1.; b += 1.*u still, and the results agree with the CPU algorithm
// bit for bit.  The order in which the statements READ is part of the contract with the kernels too: the
// compiler's schedule follows it, and the sweep kernels of the measured path are held to the bytes they had
// (DESIGN.md 11.18).  Hence sources that are read at the face, in face order, instead of twelve values passed
// up front; hence also the few kernels that keep a body of their own, each with a comment that names the
// function here it mirrors.
//
// Plain C++ apart from divide_by_6's device body: a host compiler reads it with __device__ and
// __forceinline__ defined away (tests/test_cell_update_cpu.py).
#pragma once

namespace gfship {

struct W6 { const double * p[6]; };   // the six face weights f[d].v of a level (arrays of the level's layout)

// Sources: a kernel describes where the six face weights g = w (d) and the six neighbour values u (d) of a
// cell are, and face_sums reads them when it comes to the face d, in the reference's order.  Weights: 1., the
// weight of the level, six values the caller holds, or the entries of the level's arrays at the index of the
// cell.  Neighbours: six values the caller holds (registers, a ring, LDS), or an array around the index c.
struct UnitW    { __device__ __forceinline__ double operator() (int) const { return 1.; } };
struct UniformW { double w; __device__ __forceinline__ double operator() (int) const { return w; } };
struct CellW    { double g[6]; __device__ __forceinline__ double operator() (int d) const { return g[d]; } };
struct ArrayW   { const W6 * wf; long c; __device__ __forceinline__ double operator() (int d) const { return wf->p[d][c]; } };

struct CellU    { double u[6]; __device__ __forceinline__ double operator() (int d) const { return u[d]; } };
struct ArrayU {
  const double * u; long c, sy, sz;
  __device__ __forceinline__ double operator() (int d) const {
    return d == 0 ? u[c + 1] : d == 1 ? u[c - 1] : d == 2 ? u[c + sy] : d == 3 ? u[c - sy] : d == 4 ? u[c + sz] : u[c - sz];
  }
};

// the weights of kind KIND: w is the weight of the level, cell the source of the kinds with weights per cell
template <int KIND, class C>
__device__ __forceinline__ auto kind_weights (double w, const C & cell)
{
  if constexpr (KIND >= 2)
    return cell;
  else if constexpr (KIND == 1)
    return UniformW { w };
  else
    return UnitW {};
}

// a = a0 + sum g_d, b = sum g_d*u_d over d = 0 .. 2 DIM - 1
struct FaceSums { double a, b; };

template <int DIM, class W, class U>
__device__ __forceinline__ FaceSums face_sums (const W & w, const U & u, double a0)
{
  double a = a0, b = 0.;
  { const double g = w (0); a += g; b += g*u (0); }
  { const double g = w (1); a += g; b += g*u (1); }
  { const double g = w (2); a += g; b += g*u (2); }
  { const double g = w (3); a += g; b += g*u (3); }
  if (DIM == 3) {
    { const double g = w (4); a += g; b += g*u (4); }
    { const double g = w (5); a += g; b += g*u (5); }
  }
  return { a, b };
}

// f = sum (g.b - g.a*val) of diffusion_rhs
template <int DIM, class W, class U>
__device__ __forceinline__ double flux_sum (const W & w, const U & u, double val)
{
  double f = 0.;
  { const double g = w (0); f += g*u (0) - g*val; }
  { const double g = w (1); f += g*u (1) - g*val; }
  { const double g = w (2); f += g*u (2) - g*val; }
  { const double g = w (3); f += g*u (3) - g*val; }
  if (DIM == 3) {
    { const double g = w (4); f += g*u (4) - g*val; }
    { const double g = w (5); f += g*u (5) - g*val; }
  }
  return f;
}

// (*cur, the value the cell holds, is read by the over-relaxation of relax2D only)
__device__ __forceinline__ double relax_close (double a, double b, double rhs, const double * cur,
					       unsigned dimension, double omega)
{
  if (dimension == 2)
    return a != 0. ? (1. - omega)*(*cur) + omega*(b - rhs)/a : 0.;
  return a != 0. ? (b - rhs)/a : 0.;
}

__device__ __forceinline__ double diffusion_close (double ga, double gb, double rhs, double dia, double h2)
{
  const double a = dia*h2;
  ga = 1. + ga/a;
  return (gb/a + rhs)/ga;
}

// the same operations written as one statement: the compiler emits the two quotients in the order of the
// source, and the kernels that were written this way (rows-2D, the LDS loop and the skewed sweep, kind 3) keep
// their bytes only with it
__device__ __forceinline__ double diffusion_close_1 (double ga, double gb, double rhs, double dia, double h2)
{
  const double a = dia*h2;
  return (gb/a + rhs)/(1. + ga/a);
}

__device__ __forceinline__ double residual_close (double a, double b, double rhs, double u)
{
  return rhs - (b - u*a);
}

__device__ __forceinline__ double diffusion_residual_close (double ga, double gb, double rhs, double dia,
							    double h2, double u)
{
  const double a = dia*h2;
  ga = 1. + ga/a;
  gb = rhs + gb/a;
  return gb - ga*u;
}

// (bb - rhs)/aa of relax (src/poisson.c:527) when dia == 0: aa = 0. + 1. + ... + 1. = 6. exactly,
// and the correctly rounded quotient x/6 is obtained without the 14-instruction IEEE division
// sequence: q = x*r, rem = fma (-q, 6, x) (exact), q' = fma (rem, r, q) with r = RN (1/6)
// (Markstein's correction step).  x/6 = (x/2)/3 is never closer than 1/6 ulp to a rounding
// boundary while q + rem*r differs from x/6 by less than 2^-52 ulp, so q' = RN (x/6) whenever
// nothing underflows: for x = +0 the sequence gives +0 (x is never -0 here: it is a difference
// whose minuend is a sum started from +0.), large x does not overflow (q <= x/6, the product in
// the fma is exact), infinities and NaNs give NaN where the division gives inf/NaN (the solve has
// diverged either way); only for 0 < |x| < 2^-1000, where q or the remainder may be subnormal,
// the true division is used.  The guard is one exponent extraction and one integer compare, off
// the dependent chain (tools/lab/step_lab.hip: the earlier two-sided floating-point range test
// cost more than the division it replaced).  Checked against x/6. on 1.5e9 operands.
__device__ __forceinline__ double divide_by_6 (double x)
{
#ifdef __HIP_DEVICE_COMPILE__
  const double r = 0x1.5555555555555p-3;
  const double q = x*r;
  const double rem = __builtin_fma (- q, 6., x);
  double q2 = __builtin_fma (rem, r, q);
  // frexp exponent: 0 for zeros, infinities and NaNs; below -999 only for tiny non-zero x
  const bool tiny = __builtin_amdgcn_frexp_exp (x) < -999;
  if (__builtin_expect (__builtin_amdgcn_ballot_w64 (tiny) != 0, 0))
    q2 = x/6.;
  return q2;
#else
  return x/6.;
#endif
}

// the update of one cell: its weights and neighbours, right-hand side, dia (rhoc for kinds 1 and 3) and, for the
// over-relaxation of relax2D, where its current value is
template <int DIM, int KIND, class W, class U>
__device__ __forceinline__ double cell_update (const W & w, const U & u, double rhs, double dia, const double * cur,
					       unsigned dimension, double omega, double h2)
{
  const FaceSums s = face_sums<DIM> (w, u, (KIND & 1) ? 0. : dia);
  return (KIND & 1) ? diffusion_close (s.a, s.b, rhs, dia, h2) : relax_close (s.a, s.b, rhs, cur, dimension, omega);
}

// kind 0 in 3-D (dimension == 3) without dia: a = 6. exactly, see divide_by_6
template <class U>
__device__ __forceinline__ double cell_update_six (const U & u, double rhs)
{
  return divide_by_6 (face_sums<3> (UnitW {}, u, 0.).b - rhs);
}

} // namespace gfship
