// barrier_lab.hip -- micro-benchmark of ONE workgroup alone on the device, as coarse_cycle_kernel runs: time per
// iteration of a workgroup barrier, of the chain LDS read -> six additions, divide_by_6 -> LDS write of one
// wave, and of both together, by the number of waves of the workgroup and of those with work
//   hipcc -O3 --offload-arch=gfx950 -ffp-contract=off tools/lab/barrier_lab.hip -o tools/lab/barrier_lab
#include <hip/hip_runtime.h>
#include <cstdio>

__device__ __forceinline__ double div6 (double x)
{
  const double r = 0x1.5555555555555p-3;
  const double q = x*r;
  const double rem = __builtin_fma (- q, 6., x);
  return __builtin_fma (rem, r, q);
}

// V bit 0: body (first wave(s) `active` threads), bit 1: barrier, bit 2: second dependent LDS round trip
template <int V>
__global__ void __launch_bounds__(1024) lab (int iters, int active, double * out, long long * ticks)
{
  __shared__ double s[4096];
  const int tid = threadIdx.x;
  for (int q = tid; q < 4096; q += blockDim.x) s[q] = 1e-3*q;
  __syncthreads ();
  double acc = 0.;
  int i = 400 + (tid & 255);
  long long t0 = wall_clock64 ();
  for (int q = 0; q < iters; q++) {
    if ((V & 1) && tid < active) {
      double b = 0.;
      b += s[i + 1];
      if (V & 4) { int k = 400 + ((int) b & 1); b += s[k]; } else b += s[i - 1];
      b += s[i + 18]; b += s[i - 18]; b += s[i + 324]; b += s[i - 324];
      const double v = div6 (b - 0.5);
      s[i] = v;
      acc += v;
    }
    if (V & 2) __syncthreads ();
    else __builtin_amdgcn_fence (__ATOMIC_SEQ_CST, "workgroup");
  }
  long long t1 = wall_clock64 ();
  if (tid == 0) ticks[0] = t1 - t0;
  out[tid] = acc;
}

template <int V> static void run (const char * what, int nt, int active)
{
  double * out; long long * ticks, h;
  hipMalloc (&out, 1024*sizeof (double)); hipMalloc (&ticks, sizeof (long long));
  const int iters = 2000;
  for (int rep = 0; rep < 3; rep++) {
    hipLaunchKernelGGL (lab<V>, dim3 (1), dim3 (nt), 0, 0, iters, active, out, ticks);
    if (hipDeviceSynchronize () != hipSuccess) { printf ("launch failed\n"); exit (1); }
  }
  hipMemcpy (&h, ticks, sizeof h, hipMemcpyDeviceToHost);
  printf ("%-34s nt %4d active %4d: %.3f us per iteration\n", what, nt, active, (double) h/100./iters);
  hipFree (out); hipFree (ticks);
}

int main ()
{
  const int nts[4] = { 64, 256, 768, 1024 };
  for (int k = 0; k < 4; k++) run<2> ("barrier only", nts[k], 0);
  run<1> ("body, no barrier", 64, 64);
  run<5> ("body + 2nd round trip, no barrier", 64, 64);
  for (int k = 0; k < 4; k++) run<3> ("body + barrier, one wave active", nts[k], 64);
  run<3> ("body + barrier, all active", 256, 256);
  run<3> ("body + barrier, 768 active", 1024, 768);
  run<7> ("body + 2nd trip + barrier", 1024, 768);
  return 0;
}
