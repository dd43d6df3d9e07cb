// cell_loop.hpp -- device-side pieces shared by the cell-parallel kernels: one thread per interior
// cell (x fastest), and the reductions of a wavefront and of a workgroup
#pragma once
#include "gfship_internal.hpp"

namespace gfship {

#define CELL_LOOP_PROLOGUE(L)						\
  int i = blockIdx.x*blockDim.x + threadIdx.x + 1;			\
  int j = blockIdx.y + 1;						\
  int k = (L).dim == 3 ? blockIdx.z + 1 : 0;				\
  if (i > (L).n) return;						\
  long c = (L).idx (i, j, k)

static inline void cell_grid (const Layout & L, dim3 * grid, dim3 * block)
{
  int b = L.n >= 256 ? 256 : L.n >= 128 ? 128 : 64;
  *block = dim3 (b);
  *grid = dim3 ((L.n + b - 1)/b, L.n, L.dim == 3 ? L.n : 1);
}

// the sum / maximum / minimum of a wavefront in lane 0 (every lane of the wavefront calls these)
__device__ __forceinline__ double wave_sum (double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v += __shfl_down (v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max (double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v = fmax (v, __shfl_down (v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_min (double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    v = fmin (v, __shfl_down (v, o, 64));
  return v;
}

// the end of a norm kernel: what the threads of a workgroup hold of the four sums s0, s1, s2, s4 and of the
// maximum s3 (gfs_norm_add, src/fluid.c:2139-2154), reduced into the slot-th group of five of `partial' by
// thread 0 -- wavefronts (at most 4) first, then their results in order
__device__ __forceinline__ void block_norm_sums (double s0, double s1, double s2, double s3, double s4,
						 double * __restrict__ partial, size_t slot)
{
  __shared__ double sh[5][4];
  s0 = wave_sum (s0); s1 = wave_sum (s1); s2 = wave_sum (s2); s3 = wave_max (s3); s4 = wave_sum (s4);
  int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { sh[0][w] = s0; sh[1][w] = s1; sh[2][w] = s2; sh[3][w] = s3; sh[4][w] = s4; }
  __syncthreads ();
  if (threadIdx.x == 0) {
    int nw = blockDim.x >> 6;
    double r0 = 0., r1 = 0., r2 = 0., r3 = 0., r4 = 0.;
    for (int q = 0; q < nw; q++) {
      r0 += sh[0][q]; r1 += sh[1][q]; r2 += sh[2][q]; r3 = fmax (r3, sh[3][q]); r4 += sh[4][q];
    }
    double * p = partial + 5*slot;
    p[0] = r0; p[1] = r1; p[2] = r2; p[3] = r3; p[4] = r4;
  }
}

} // namespace gfship
