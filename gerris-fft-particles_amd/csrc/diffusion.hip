// diffusion.hip -- implicit diffusion (GfsSourceDiffusion / viscosity): kernels and host control
// behind gfs_diffusion_coefficients, gfs_diffusion_rhs, gfs_diffusion_residual,
// gfs_diffusion_cycle (src/poisson.c:1271-1690) and gfs_diffusion (src/timestep.c:735-788), without
// solid boundaries.
//
// With a constant diffusion coefficient and a constant density (gfship_diffusion_coefficients) every
// leaf face carries the same weight w = lambda2*beta*dt*D (diffusion_coef, src/poisson.c:1280-1303)
// and every cell the same rhoc = 1. (diffusion_mixed_coef :1305-1348), so a level is described by one
// scalar instead of 2*dim arrays; the coarse weights are computed on the host with
// face_coeff_from_below's arithmetic (:826-853), one scalar per level: RelaxOp kind 1 of cell_update.hpp.
//
// With a coefficient given at the leaf faces and a density given at the cells of every level
// (gfship_diffusion_coefficients_faces) the weights are the arrays f[d].v the weighted Poisson solver
// uses (dom->wf), computed on the device: kind 3.  The domain remembers which of the two was set last
// (diff_kind).  The in-place sweeps are the exact-order kernels of poisson_kernels.hip with that kind.
#include "gfship_internal.hpp"
#include "cell_loop.hpp"
#include <cmath>
#include <cstdlib>

using namespace gfship;

namespace gfship {

// gfs_diffusion_rhs / diffusion_rhs, src/poisson.c:1392-1451:
//   f = sum_d (g.b - g.a*v) with g.a = w, g.b = w*v_nb ; rhs += (1 - beta)/beta*f/(h*h*rhoc)
template <int DIM>
__global__ void __launch_bounds__(256)
diffusion_rhs_kernel (Layout L, double w, double pbeta, const double * __restrict__ v,
		      const double * __restrict__ rhoc, double * __restrict__ rhs)
{
  CELL_LOOP_PROLOGUE (L);
  const double h = 1./L.n;
  const double f = flux_sum<DIM> (UniformW { w }, ArrayU { v, c, L.sy, L.sz }, v[c]);
  rhs[c] += pbeta*f/(h*h*rhoc[c]);
}

// diffusion_residual, src/poisson.c:1534-1569
template <int DIM>
__global__ void __launch_bounds__(256)
diffusion_residual_kernel (Layout L, double w, const double * __restrict__ u,
			   const double * __restrict__ rhs, const double * __restrict__ rhoc,
			   double * __restrict__ res)
{
  CELL_LOOP_PROLOGUE (L);
  const double h = 1./L.n;
  const double a = rhoc[c];
  const FaceSums s = face_sums<DIM> (UniformW { w }, ArrayU { u, c, L.sy, L.sz }, 0.);
  res[c] = diffusion_residual_close (s.a, s.b, rhs[c], a, h*h, u[c]);
}

// gfs_get_from_below_intensive, src/fluid.c:1843-1864 (unit cell fractions): children in
// child-id order (bit0 -> +x, bit1 -> -y, bit2 -> -z), val/sa
template <int DIM>
__global__ void __launch_bounds__(256)
restrict_intensive_kernel (Layout Lc, Layout Lf, double * __restrict__ vc,
			   const double * __restrict__ vf)
{
  CELL_LOOP_PROLOGUE (Lc);
  double val = 0., sa = 0.;
#pragma unroll
  for (int id = 0; id < (1 << DIM); id++) {
    int ci = 2*i - 1 + (id & 1);
    int cj = 2*j - 1 + ((id & 2) ? 0 : 1);
    int ck = DIM == 3 ? 2*k - 1 + ((id & 4) ? 0 : 1) : 0;
    double a = 1.;
    val += vf[Lf.idx (ci, cj, ck)]*a;
    sa += a;
  }
  vc[c] = val/sa;
}

// the same two with the six face weights of the cell: flux_sum, and face_sums with diffusion_residual_close,
// of ArrayW { &wf, c }, as written before the shared header (through it three of the four kernels come out an
// instruction longer or shorter)

template <int DIM>
__global__ void __launch_bounds__(256)
diffusion_rhs_faces_kernel (Layout L, W6 wf, double pbeta, const double * __restrict__ v,
			    const double * __restrict__ rhoc, double * __restrict__ rhs)
{
  CELL_LOOP_PROLOGUE (L);
  const double h = 1./L.n;
  const long off[3] = { 1, L.sy, L.sz };
  const double val = v[c];
  double f = 0.;
#pragma unroll
  for (int cc = 0; cc < DIM; cc++) {
    { const double g = wf.p[2*cc][c]; f += g*v[c + off[cc]] - g*val; }
    { const double g = wf.p[2*cc + 1][c]; f += g*v[c - off[cc]] - g*val; }
  }
  rhs[c] += pbeta*f/(h*h*rhoc[c]);
}

template <int DIM>
__global__ void __launch_bounds__(256)
diffusion_residual_faces_kernel (Layout L, W6 wf, const double * __restrict__ u,
				 const double * __restrict__ rhs, const double * __restrict__ rhoc,
				 double * __restrict__ res)
{
  CELL_LOOP_PROLOGUE (L);
  const double h = 1./L.n;
  const long off[3] = { 1, L.sy, L.sz };
  double a = rhoc[c];
  double ga = 0., gb = 0.;
#pragma unroll
  for (int cc = 0; cc < DIM; cc++) {
    { const double g = wf.p[2*cc][c]; ga += g; gb += g*u[c + off[cc]]; }
    { const double g = wf.p[2*cc + 1][c]; ga += g; gb += g*u[c - off[cc]]; }
  }
  a *= h*h;
  ga = 1. + ga/a;
  gb = rhs[c] + gb/a;
  res[c] = gb - ga*u[c];
}

// diffusion_mixed_coeff, src/poisson.c:1321-1332, on the cells of one level: rho = 1./alpha (the cell
// fraction is 1.); *bad is set where the reference stops with "density is negative", and for an alpha
// that is zero or not a number
template <int DIM>
__global__ void __launch_bounds__(256)
diffusion_rhoc_kernel (Layout L, const double * __restrict__ alpha, double * __restrict__ rhoc,
		       unsigned * __restrict__ bad)
{
  CELL_LOOP_PROLOGUE (L);
  const double al = alpha[c];
  const double rho = 1./al;
  if (!(al > 0.) || !(rho > 0.))
    *bad = 1u;
  rhoc[c] = rho*1.;
}

static W6 level_weights (gfship_domain * dom, int level)
{
  W6 w;
  for (int d = 0; d < 6; d++)
    w.p[d] = d < 2*dom->dim ? dom->fields[dom->wf[d]].lev[level] : nullptr;
  return w;
}

static RelaxOp level_op (gfship_domain * dom, int level)
{
  RelaxOp op;
  if (dom->diff_kind == 3) {
    op = weighted_op (dom, level);      /* the six arrays of the level */
    op.kind = 3;
  }
  else {
    op.kind = 1;
    op.w = dom->diff_w[level];
  }
  double h = 1./dom->lay[level].n;
  op.h2 = h*h;
  return op;
}

// the 2 x 2 ring kernels know the uniform weight only: whether a level may run on them is decided by
// the coefficients of THIS call, whatever the last Poisson call left in dom->weighted
struct PatchCall {
  gfship_domain * dom;
  PatchCall (gfship_domain * d, int kind) : dom (d) { dom->patch_call = kind == 1; }
  ~PatchCall () { dom->patch_call = -1; }
};

// relax_loop, src/poisson.c:1070-1089, with diffusion_relax as the cell update
static int relax_loop (gfship_domain * dom, Field * dp, Field * u, int level, Field * res,
		       Field * dia, unsigned nrelax)
{
  int r;
  RelaxOp op = level_op (dom, level);
  PatchCall scope (dom, op.kind);
  const bool faces = op.kind == 3;
  dp->zero[level] = false;
  bool done = false;
  if ((r = launch_relax_loop_small (dom, dom->dim, level, 1., dp, u, res->lev[level],
				    dia->lev[level], nrelax, &done, &op)))
    return r;
  if (done)
    return GFSHIP_OK;
  /* 3-D levels of 32^3 and more: the pipelined tile kernels with the diffusion cell update (rhoc
     travels as their dia stream); the whole loop in one launch on boxes without MPI sides */
  const bool pipelined = faces ? dom->sw.weighted_pipelined : dom->sw.diffusion_pipelined;
  const bool pipelined_applies = dom->dim == 3 && dom->relax_mode == GFSHIP_RELAX_EXACT && !dom->force_hyperplane &&
    skew_supported (dom, level) && !(dom->has_external && dom->overlap && nrelax > 1);
  if (pipelined_applies && faces)
    dom->kc[pipelined ? GFSHIP_KC_DIFFUSION_FACES_PIPELINED : GFSHIP_KC_DIFFUSION_FACES_HYPERPLANES]++;
  else if (pipelined_applies)
    dom->kc[pipelined ? GFSHIP_KC_DIFFUSION_PIPELINED : GFSHIP_KC_DIFFUSION_HYPERPLANES]++;
  if (pipelined && pipelined_applies)
    return launch_relax_loop_skew (dom, level, dp, u, res->lev[level], dia->lev[level], false, nrelax,
				   true, nullptr, nullptr, &op);
  if ((r = launch_bc (dom, u, dp, level, 1))) return r;
  for (unsigned n = 0; n < nrelax - 1; n++) {
    if ((r = launch_relax_exact (dom, dom->dim, level, 1., dp->lev[level], res->lev[level],
				 dia->lev[level], &op)))
      return r;
    if ((r = launch_bc (dom, u, dp, level, 1))) return r;
  }
  return launch_relax_exact (dom, dom->dim, level, 1., dp->lev[level], res->lev[level],
			     dia->lev[level], &op);
}

static int residual (gfship_domain * dom, Field * U, Field * R, Field * C, Field * S)
{
  const int L = dom->depth;
  dim3 grid, block;
  cell_grid (dom->lay[L], &grid, &block);
  S->zero[L] = false;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    if (dom->diff_kind == 3)
      hipLaunchKernelGGL (diffusion_residual_faces_kernel<DIM>, grid, block, 0, dom->stream, dom->lay[L],
			  level_weights (dom, L), U->lev[L], R->lev[L], C->lev[L], S->lev[L]);
    else
      hipLaunchKernelGGL (diffusion_residual_kernel<DIM>, grid, block, 0, dom->stream, dom->lay[L],
			  dom->diff_w[L], U->lev[L], R->lev[L], C->lev[L], S->lev[L]);
  }, dom->dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

} // namespace gfship

extern "C" {

int gfship_diffusion_coefficients (gfship_domain * dom, double D, double dt, gfship_field rhoc,
				   double beta)
{
  GFSHIP_CHECK (dom != nullptr, GFSHIP_EINVAL, "null domain");
  GFSHIP_CHECK (beta >= 0.5 && beta <= 1., GFSHIP_EINVAL, "beta must be in [0.5,1]");
  Field * C = get_field (dom, rhoc);
  if (!C) return GFSHIP_EINVAL;
  const int L = dom->depth;
  /* diffusion_coef: v = lambda2[c]*dt*D*fraction/alpha with dt <- beta*dt */
  double cdt = beta*dt;
  dom->diff_w[L] = 1.*cdt*D*1./1.;
  /* face_coeff_from_below: mean over the FTT_CELLS/2 children on the face, in child order */
  for (int l = L - 1; l >= 0; l--) {
    double w = dom->diff_w[l + 1], sw = 0.;
    int nd = dom->dim == 3 ? 4 : 2;
    for (int m = 0; m < nd; m++)
      sw += w;
    dom->diff_w[l] = sw/nd;
  }
  /* diffusion_mixed_coef: rhoc = 1. on every cell of every level */
  for (int l = 0; l <= L; l++) {
    int r = gfship_field_fill (dom, rhoc, l, 1.*1.);
    if (r) return r;
  }
  dom->diff_ready = true;
  dom->diff_kind = 1;
  return GFSHIP_OK;
}

int gfship_diffusion_coefficients_faces (gfship_domain * dom, const gfship_field D[3], double dt,
					 gfship_field rhoc, gfship_field alpha_cell, double beta)
{
  GFSHIP_CHECK (dom != nullptr, GFSHIP_EINVAL, "null domain");
  GFSHIP_CHECK (D != nullptr, GFSHIP_EINVAL, "null diffusion coefficient");
  GFSHIP_CHECK (beta >= 0.5 && beta <= 1., GFSHIP_EINVAL, "beta must be in [0.5,1]");
  GFSHIP_CHECK (!dom->has_external, GFSHIP_EUNSUPPORTED,
		"per-face diffusion coefficients on a box with MPI sides are not supported");
  Field * C = get_field (dom, rhoc);
  if (!C) return GFSHIP_EINVAL;
  Field * A = nullptr;
  if (alpha_cell != -1 && !(A = get_field (dom, alpha_cell))) return GFSHIP_EINVAL;
  double * d[3] = { nullptr, nullptr, nullptr };
  for (int c = 0; c < dom->dim; c++) {
    Field * F = get_field (dom, D[c]);
    if (!F) return GFSHIP_EINVAL;
    d[c] = F->lev[dom->depth];
  }
  int r;
  if ((r = before_write (dom))) return r;
  const int L = dom->depth;
  /* diffusion_mixed_coeff on every cell of every level (FTT_TRAVERSE_ALL) */
  if (A) {
    unsigned * bad = (unsigned *) (dom->d_scratch + dom->scratch_doubles - 1), hbad = 0;
    GFSHIP_HIP (hipMemsetAsync (bad, 0, sizeof (unsigned), dom->stream));
    for (int l = 0; l <= L; l++) {
      dim3 grid, block;
      cell_grid (dom->lay[l], &grid, &block);
      C->zero[l] = false;
      with_bools ([&] (auto D3) {
	hipLaunchKernelGGL (diffusion_rhoc_kernel<decltype (D3)::value ? 3 : 2>, grid, block, 0, dom->stream,
			    dom->lay[l], A->lev[l], C->lev[l], bad);
      }, dom->dim == 3);
      GFSHIP_HIP (hipGetLastError ());
    }
    GFSHIP_HIP (hipMemcpyAsync (&hbad, bad, sizeof (unsigned), hipMemcpyDeviceToHost, dom->stream));
    GFSHIP_HIP (hipStreamSynchronize (dom->stream));
    if (hbad)
      dom->diff_ready = false;      /* rhoc has been overwritten: no solve before the next successful call */
    GFSHIP_CHECK (!hbad, GFSHIP_EINVAL, "density is negative or zero: check the definition of alpha");
  }
  else
    for (int l = 0; l <= L; l++)
      if ((r = gfship_field_fill (dom, rhoc, l, 1.*1.))) return r;
  /* diffusion_coef with dt <- beta*dt, then face_coeff_from_below: into f[d].v, which the Poisson
     solver shares (the skewed copies of either are stale from here) */
  if ((r = alloc_weights (dom))) return r;
  if ((r = launch_diffusion_weights (dom, d, beta*dt))) return r;
  dom->weights_stamp++;
  dom->diff_ready = true;
  dom->diff_kind = 3;
  return GFSHIP_OK;
}

int gfship_diffusion_rhs (gfship_domain * dom, gfship_field v, gfship_field rhs,
			  gfship_field rhoc, double beta)
{
  Field * V = get_field (dom, v), * R = get_field (dom, rhs), * C = get_field (dom, rhoc);
  if (!V || !R || !C) return GFSHIP_EINVAL;
  GFSHIP_CHECK (dom->diff_ready, GFSHIP_EINVAL, "call gfship_diffusion_coefficients first");
  { int r = before_write (dom); if (r) return r; }
  const int L = dom->depth;
  dim3 grid, block;
  cell_grid (dom->lay[L], &grid, &block);
  R->zero[L] = false;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    if (dom->diff_kind == 3)
      hipLaunchKernelGGL (diffusion_rhs_faces_kernel<DIM>, grid, block, 0, dom->stream, dom->lay[L],
			  level_weights (dom, L), (1. - beta)/beta, V->lev[L], C->lev[L], R->lev[L]);
    else
      hipLaunchKernelGGL (diffusion_rhs_kernel<DIM>, grid, block, 0, dom->stream, dom->lay[L],
			  dom->diff_w[L], (1. - beta)/beta, V->lev[L], C->lev[L], R->lev[L]);
  }, dom->dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

int gfship_diffusion_residual (gfship_domain * dom, gfship_field u, gfship_field rhs,
			       gfship_field rhoc, gfship_field res)
{
  Field * U = get_field (dom, u), * R = get_field (dom, rhs), * C = get_field (dom, rhoc),
    * S = get_field (dom, res);
  if (!U || !R || !C || !S) return GFSHIP_EINVAL;
  GFSHIP_CHECK (dom->diff_ready, GFSHIP_EINVAL, "call gfship_diffusion_coefficients first");
  { int r = before_write (dom); if (r) return r; }
  return residual (dom, U, R, C, S);
}

int gfship_diffusion_cycle (gfship_domain * dom, unsigned levelmin, unsigned depth,
			    unsigned nrelax, gfship_field u, gfship_field rhs, gfship_field rhoc,
			    gfship_field res)
{
  GFSHIP_CHECK (dom != nullptr, GFSHIP_EINVAL, "null domain");
  GFSHIP_CHECK (dom->diff_ready, GFSHIP_EINVAL, "call gfship_diffusion_coefficients first");
  GFSHIP_CHECK (nrelax > 0, GFSHIP_EINVAL, "nrelax must be non zero");
  { int r = before_write (dom); if (r) return r; }
  GFSHIP_CHECK (depth == (unsigned) dom->depth && levelmin <= depth, GFSHIP_EINVAL,
		"levels %u..%u do not match the domain depth %d", levelmin, depth, dom->depth);
  if (dom->dp_cache < 0)
    dom->dp_cache = gfship_field_alloc (dom, -1);
  if (dom->dp_cache < 0) return dom->dp_cache;
  Field * U = get_field (dom, u), * R = get_field (dom, rhs), * C = get_field (dom, rhoc),
    * S = get_field (dom, res), * DP = get_field (dom, dom->dp_cache);
  if (!U || !R || !C || !S) return GFSHIP_EINVAL;
  const int L = dom->depth;
  int r;
#define TRY(x) do { if ((r = (x)) != GFSHIP_OK) return r; } while (0)
  /* compute residual on non-leafs cells */
  for (int l = L - 1; l >= 0; l--) {
    dim3 grid, block;
    cell_grid (dom->lay[l], &grid, &block);
    S->zero[l] = false;
    with_bools ([&] (auto D3) {
      hipLaunchKernelGGL (restrict_intensive_kernel<decltype (D3)::value ? 3 : 2>, grid, block, 0, dom->stream,
			  dom->lay[l], dom->lay[l + 1], S->lev[l], S->lev[l + 1]);
    }, dom->dim == 3);
    GFSHIP_HIP (hipGetLastError ());
  }
  /* relax top level */
  for (int l = 0; l <= L; l++)
    DP->zero[l] = false;
  TRY (launch_fill (dom, levelmin, DP->lev[levelmin], 0.));
  TRY (relax_loop (dom, DP, U, levelmin, S, C, 10*nrelax));
  /* relax from top to bottom */
  for (unsigned l = levelmin + 1; l <= depth; l++) {
    /* get initial guess from coarser grid */
    TRY (launch_prolongate (dom, l - 1, DP->lev[l - 1], DP->lev[l]));
    TRY (relax_loop (dom, DP, U, l, S, C, nrelax));
  }
  /* correct on leaf cells */
  U->zero[L] = false;
  TRY (launch_correct (dom, L, U->lev[L], DP->lev[L]));
  TRY (launch_bc (dom, U, U, L, 0));
  /* compute new residual on leaf cells */
  TRY (residual (dom, U, R, C, S));
#undef TRY
  return GFSHIP_OK;
}

int gfship_diffusion (gfship_domain * dom, gfship_multilevel_params * par, gfship_field v,
		      gfship_field rhs, gfship_field rhoc)
{
  GFSHIP_CHECK (dom && par, GFSHIP_EINVAL, "null argument");
  int r;
  if ((r = before_write (dom))) return r;
  /* res = gfs_temporary_variable (domain): kept between calls like the cycle's dp */
  if (dom->res_cache < 0)
    dom->res_cache = gfship_field_alloc (dom, -1);
  if (dom->res_cache < 0) return dom->res_cache;
  gfship_field res = dom->res_cache;
  unsigned minlevel = par->minlevel, maxlevel = dom->depth;
  if (minlevel > maxlevel) minlevel = maxlevel;
  if ((r = gfship_diffusion_residual (dom, v, rhs, rhoc, res))) return r;
  if ((r = gfship_norm_variable (dom, res, &par->residual))) return r;
  par->residual_before = par->residual;
  double res_max_before = par->residual.infty;
  par->niter = 0;
  while (par->niter < par->nitermin ||
	 (par->residual.infty > par->tolerance && par->niter < par->nitermax)) {
    if ((r = gfship_diffusion_cycle (dom, minlevel, maxlevel, par->nrelax, v, rhs, rhoc, res)))
      return r;
    if ((r = gfship_norm_variable (dom, res, &par->residual))) return r;
    if (par->residual.infty == res_max_before) /* convergence has stopped!! */
      break;
    if (par->residual.infty > res_max_before/1.1 && minlevel < maxlevel)
      minlevel++;
    res_max_before = par->residual.infty;
    par->niter++;
  }
  return GFSHIP_OK;
}

} // extern "C"
