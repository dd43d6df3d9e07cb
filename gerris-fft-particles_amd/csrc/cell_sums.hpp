// cell_sums.hpp -- the serial sums per cell of the two-way coupling (coupling.hip) and of
// GfsSourceParticulateVol / ...Mass (particulate_sources.hip), once, for the cells of a uniform box
// and the leaves of a refined tree (tree_particles.hip).
//
// The records (cell << 32 | creation slot) arrive sorted by cell, the records of one cell in list order; the thread
// of the first record of a cell adds what the reference adds, serially and in that order (no atomics).  What `cell'
// means is the map's business:
//   BoxCells<DIM>    the linear number of a leaf cell of the box; index = its place in the Layout, one cellvol;
//   TreeCells<DIM>   the index of a leaf in the concatenated levels (Topo::gi): index = itself, the cellvol of its level.
#pragma once
#include "gfship_internal.hpp"
#include "tree.hpp"

namespace gfship {

// leaf index of the Layout of linear cell number `cell'
template <int DIM>
__device__ __forceinline__ long cell_index (const Layout & L, unsigned long long cell)
{
  const unsigned n = (unsigned) L.n;
  const int i = (int) (cell % n) + 1, j = (int) ((cell/n) % n) + 1;
  const int k = DIM == 3 ? (int) (cell/((unsigned long long) n*n)) + 1 : 0;
  return L.idx (i, j, k);
}

// the level of cell g of the concatenated levels
__device__ __forceinline__ int level_of (const tree::Topo & T, unsigned g)
{
  int l = 0;
  while (l < T.depth && (int) g >= T.off[l + 1]) l++;
  return l;
}

template <int DIM>
__device__ __forceinline__ double level_cellvol (int l)      /* ftt_cell_volume */
{
  const double h = 1./(double) (1 << l);
  return DIM == 3 ? h*h*h : h*h;
}

template <int DIM>
struct BoxCells {
  Layout L;
  __device__ __forceinline__ long index (unsigned long long cell) const { return cell_index<DIM> (L, cell); }
  __device__ __forceinline__ double cellvol (unsigned long long) const {      /* ftt_cell_volume, no solid */
    const double h = 1./L.n;
    return DIM == 3 ? h*h*h : h*h;
  }
};

template <int DIM>
struct TreeCells {
  tree::Topo T;
  __device__ __forceinline__ long index (unsigned long long cell) const { return (long) cell; }
  __device__ __forceinline__ double cellvol (unsigned long long cell) const {
    return level_cellvol<DIM> (level_of (T, (unsigned) cell));
  }
};

// voidfraction_from_particles (:1929-1932) for the particles of one cell, in list order
template <int DIM, class Cells>
__global__ void __launch_bounds__(256)
field_sum_kernel (Cells C, int n, const unsigned long long * __restrict__ key, unsigned long long ncell,
		  const double * __restrict__ volume, double * __restrict__ v)
{
  int r = blockIdx.x*blockDim.x + threadIdx.x;
  if (r >= n) return;
  const unsigned long long cell = key[r] >> 32;
  if (cell >= ncell) return;
  if (r > 0 && key[r - 1] >> 32 == cell) return;      /* not the first of its cell */
  const double cellvol = C.cellvol (cell);
  const long idx = C.index (cell);
  double s = v[idx];
  for (int m = r; m < n && key[m] >> 32 == cell; m++)
    s += volume[(unsigned) (key[m] & 0xFFFFFFFFull)]/cellvol;
  v[idx] = s;
}

// step 3 of the spreading: kernel_volume (:2108-2119) over the leaves of each particle in traversal order, then :2216
template <int DIM, class Cells>
__global__ void __launch_bounds__(256)
spread_correction_kernel (Cells C, int nchunk, int stride, const int * __restrict__ cnt,
			  const unsigned long long * __restrict__ key, const double * __restrict__ K,
			  double * __restrict__ corr)
{
  int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= nchunk) return;
  double volume = 0., correction = 0.;
  const size_t base = (size_t) t*stride;
  for (int j = 0; j < cnt[t]; j++) {
    const double cellvol = C.cellvol (key[base + j] >> 32);
    volume += cellvol;
    correction += K[base + j]*cellvol;
  }
  correction /= volume;      /* no leaf: 0./0., which is not > 1.e-10 -- and there is nothing to add to */
  corr[t] = correction;
}

// step 4 of the spreading: diffuse_force (:2158-2175) for the records of one cell, in list order; RHO:
// liq_rho = 1./alpha_cell[idx] (:2167-2168), otherwise 1. (no alpha; a tree has none)
template <int DIM, bool RHO, class Cells>
__global__ void __launch_bounds__(256)
spread_sum_kernel (Cells C, long nrec, const unsigned long long * __restrict__ key, unsigned long long ncell,
		   const double * __restrict__ K, int o0, const double * __restrict__ corr,
		   const double * __restrict__ fx, const double * __restrict__ fy, const double * __restrict__ fz,
		   const double * __restrict__ alpha_cell,
		   double * __restrict__ Fx, double * __restrict__ Fy, double * __restrict__ Fz)
{
  long r = (long) blockIdx.x*blockDim.x + threadIdx.x;
  if (r >= nrec) return;
  const unsigned long long cell = key[r] >> 32;
  if (cell >= ncell) return;
  if (r > 0 && key[r - 1] >> 32 == cell) return;
  const double cellvol = C.cellvol (cell);
  const long idx = C.index (cell);
  double liq_rho = 1.;
  if constexpr (RHO) liq_rho = 1./alpha_cell[idx];
  double F[3] = { Fx[idx], Fy[idx], DIM == 3 ? Fz[idx] : 0. };
  for (long m = r; m < nrec && key[m] >> 32 == cell; m++) {
    const unsigned o = (unsigned) (key[m] & 0xFFFFFFFFull);
    const double correction = corr[o - (unsigned) o0];
    if (correction > 1.e-10) {
      const double k = K[m];
      F[0] -= fx[o]/liq_rho/cellvol*k/correction;
      F[1] -= fy[o]/liq_rho/cellvol*k/correction;
      if (DIM == 3) F[2] -= fz[o]/liq_rho/cellvol*k/correction;
    }
  }
  Fx[idx] = F[0];
  Fy[idx] = F[1];
  if (DIM == 3) Fz[idx] = F[2];
}

struct SourceCellArgs {
  int n;
  const unsigned long long * key;
  unsigned long long ncell;
  const double * src, * prad, * purel[3];
  double * deposit, * rad, * urel[3];      // nullptr: not written
};

// the last step of a GfsSourceParticulateVol / ...Mass: the records of one cell in list order: deposit += source
// (:2830, :2989), Rad, Urelp ... of the last one (:2812-2824: every particle overwrites what the one before left).
// HELD: the sum starts from what the cell holds (a tree: nothing has reset its leaves below level 1); otherwise
// from the 0. of the reset
template <int DIM, bool HELD, class Cells>
__global__ void __launch_bounds__(256)
particulate_source_cell_kernel (Cells C, SourceCellArgs A)
{
  int r = blockIdx.x*blockDim.x + threadIdx.x;
  if (r >= A.n) return;
  const unsigned long long cell = A.key[r] >> 32;
  if (cell >= A.ncell) return;
  if (r > 0 && A.key[r - 1] >> 32 == cell) return;      /* not the first of its cell */
  const long idx = C.index (cell);
  double s = 0.;
  if (HELD && A.deposit) s = A.deposit[idx];
  int m = r;
  for (; m < A.n && A.key[m] >> 32 == cell; m++)
    s += A.src[(unsigned) (A.key[m] & 0xFFFFFFFFull)];
  const unsigned last = (unsigned) (A.key[m - 1] & 0xFFFFFFFFull);
  if (A.deposit) A.deposit[idx] = s;
  if (A.rad) A.rad[idx] = A.prad[last];
#pragma unroll
  for (int c = 0; c < DIM; c++)
    if (A.urel[c]) A.urel[c][idx] = A.purel[c][last];
}

} // namespace gfship
