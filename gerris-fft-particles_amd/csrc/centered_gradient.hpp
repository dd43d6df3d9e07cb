// The centred pressure gradient of a cell along one direction, the one definition every kernel that
// forms it shares (and the host, which tests compile on their own): gfs_correct_normal_velocities
// accumulates the face differences dp = (w*p[nb] - w*p[cell])/h; dp /= face_fraction of the - and the
// + face with unit weights (src/timestep.c:118-144), gfs_scale_gradients halves the sum
// (src/timestep.c:60-87).  h = 1/n is a power of two: /h is written as an exact scaling by rn = n.
// pm, pc, pn: the pressure in the cell before, the cell itself and the cell after along the direction.
#ifndef GFSHIP_CENTERED_GRADIENT_HPP
#define GFSHIP_CENTERED_GRADIENT_HPP

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GFSHIP_HOST_DEVICE __host__ __device__
#else
#define GFSHIP_HOST_DEVICE
#endif

GFSHIP_HOST_DEVICE inline double centered_gradient (double pm, double pc, double pn, double rn)
{
  double dpm = (1.*pc - 1.*pm)*rn;
  dpm /= 1.;
  double dpp = (1.*pn - 1.*pc)*rn;
  dpp /= 1.;
  double v = 0.;
  v += dpm*1.;
  v += dpp*1.;
  return v/2.;
}

#endif
