// particles.hip -- Lagrangian tracers on the device: GfsParticle in a GfsParticleList
// (src/particle.c:31-44, modules/particulatecommon.c:955-1015,3058-3395).
//
// One thread per particle, SoA storage (x, y, z, old position, id, alive).  Each step:
//   remove_particles_not_in_domain -> gfs_particle_event (RK2 midpoint through
//   gfs_domain_advect_point, src/domain.c:2764-2788) -> gfs_particle_bc (ray march to the exit
//   face, periodic wrap).
// locate = ftt_cell_locate's descent with its strict '>' comparisons (src/ftt.c:1535-1574);
// interpolate = gfs_interpolate: corner values are inverse-distance weighted means of the cells
// sharing the corner (src/fluid.c:2983-3101), then the reference's 8-corner polynomial
// (:2640-2683).  All in the reference's operand order: cell indices and positions are
// bit-identical to the CPU algorithm.  The reference has no test for this path.  It is pinned on a
// restatement of the reference on an explicit cell graph (tests/sampler_reference.py: the box tree
// and the flattened boundary tree of every side, neighbours found as ftt_cell_neighbor finds them):
// sample_kernel and particle_list_event_kernel against it in tests/test_gpu_sampler_reference.py,
// the oracle against it in tests/test_sampler_reference_cpu.py, all by array_equal.  On a uniform
// box the walk of do_path reaches exactly the cells of the 2^DIM block that have at most one
// coordinate in the ghost layer: `out <= 1' below is that statement.
//
// Sort by cell: the gather of a particle reads the 27 cells around it for three components and
// two RK stages, so particles of one wavefront should sit in neighbouring cells.  Every
// `sort_every` events the slots are reordered by the linear index of the containing leaf cell
// (stable LSD radix sort of (cell, slot) pairs, rocPRIM through hipCUB), which changes where a
// particle is stored, never its arithmetic: `orig` remembers the slot a particle was created in
// and gfship_particles_download returns the survivors in that order (the reference's list
// order).  Tracers move less than one cell per step (CFL < 1), so the order stays good between
// sorts.
#include "particle_events.hpp"
#include "particulate_forces.hpp"
#include "tree_particles.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <numeric>


namespace gfship {

struct PartArgs {
  Layout L;
  int side[6];
  int n;
  double * pos[3];
  double * old[3];
  unsigned char * alive;
  const double * u[3];
  double dt;
  unsigned * count;
  int migrate;                 // particles leaving through an external side are kept for the hook
};

// gfs_interpolate (src/fluid.c:2697-2710) of one variable at p inside cell (i,j,k)
template <int DIM>
__device__ double interpolate (const Layout & L, const double * __restrict__ v, const int cell[3],
			       const double p_[3])
{
  const int n = L.n;
  const double h = 1./n;
  constexpr int NC = 4*(DIM - 1);
  // the 3^DIM neighbourhood (edge/corner ghosts are allocated, never used)
  double nb[DIM == 3 ? 27 : 9];
  bool outm[3], outp[3];    // is cell - 1 / cell + 1 a ghost along each axis?
#pragma unroll
  for (int a = 0; a < DIM; a++) {
    outm[a] = cell[a] - 1 < 1;
    outp[a] = cell[a] + 1 > n;
  }
  const long base = L.idx (cell[0], cell[1], cell[2]);
#pragma unroll
  for (int dz = (DIM == 3 ? -1 : 0); dz <= (DIM == 3 ? 1 : 0); dz++)
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
      for (int dx = -1; dx <= 1; dx++)
	nb[(dx + 1) + 3*(dy + 1) + 9*(DIM == 3 ? dz + 1 : 0)] = v[base + dx + dy*L.sy + dz*L.sz];

  const double a_ = 1./(h*(DIM == 2 ? 0.707106781185 : 0.866025403785) + 1e-12);
  // corner directions, src/fluid.c:2588-2605
  const int c2[4][3] = { {-1,-1,0}, {1,-1,0}, {1,1,0}, {-1,1,0} };
  const int c3[8][3] = { {-1,-1,1}, {1,-1,1}, {1,1,1}, {-1,1,1},
			 {-1,-1,-1}, {1,-1,-1}, {1,1,-1}, {-1,1,-1} };
  double f[NC + 1];
#pragma unroll
  for (int ic = 0; ic < NC; ic++) {
    int sg[3];
#pragma unroll
    for (int a = 0; a < 3; a++) sg[a] = DIM == 2 ? c2[ic][a] : c3[ic][a];
    // gfs_cell_corner_interpolator (src/fluid.c:2983-3068): cells n[m], m = 0..2^DIM-1, offset by
    // (m&1) along x, (m&2) along y, (m&4) along z towards the corner
    double wsum = 0., w0 = 0.;
    int cnt = 0, boundaries = 0;
    bool ex[1 << DIM];
#pragma unroll
    for (int m = 0; m < (1 << DIM); m++) {
      int out = 0;
#pragma unroll
      for (int a = 0; a < DIM; a++)
	if (m & (1 << a))
	  out += (sg[a] < 0 ? outm[a] : outp[a]) ? 1 : 0;
      ex[m] = out <= 1;
      if (ex[m]) {
	if (cnt == 0) w0 = a_;
	cnt++;
	wsum += a_;
	if (out > 0) boundaries++;
      }
    }
    bool skip0 = (cnt == DIM + 1 && boundaries == DIM);   // domain corner: drop the central cell
    if (skip0)
      wsum -= w0;
    const double scale = 1./wsum;
    double r = 0.;
#pragma unroll
    for (int m = 0; m < (1 << DIM); m++) {
      int ox = (m & 1) ? sg[0] : 0, oy = (m & 2) ? sg[1] : 0, oz = (DIM == 3 && (m & 4)) ? sg[2] : 0;
      double val = nb[(ox + 1) + 3*(oy + 1) + 9*(DIM == 3 ? oz + 1 : 0)];
      if (ex[m] && !(skip0 && m == 0)) {
	double wm = a_*scale;
	r += wm*val;
      }
    }
    f[ic] = r;
  }
  f[NC] = nb[1 + 3 + (DIM == 3 ? 9 : 0)];

  // gfs_interpolate_from_corners, src/fluid.c:2640-2683
  double o[3] = { -0.5 + (cell[0] - 0.5)*h, -0.5 + (cell[1] - 0.5)*h,
		  DIM == 3 ? -0.5 + (cell[2] - 0.5)*h : 0. };
  const double size = h/2.;
  double p[3];
  p[0] = (p_[0] - o[0])/size;
  p[1] = (p_[1] - o[1])/size;
  if (DIM == 2) {
    double x = (p[0] + p[1])/2., y = (p[1] - p[0])/2., val = f[4];
    if (x > 0.)
      val += x*(f[2] - f[4]);
    else
      val -= x*(f[0] - f[4]);
    if (y > 0.)
      val += y*(f[3] - f[4]);
    else
      val -= y*(f[1] - f[4]);
    return val;
  }
  p[2] = (p_[2] - o[2])/size;
  double c[8];
  c[0] = - f[0] + f[1] + f[2] - f[3] - f[4] + f[5] + f[6] - f[7];
  c[1] = - f[0] - f[1] + f[2] + f[3] - f[4] - f[5] + f[6] + f[7];
  c[2] =   f[0] + f[1] + f[2] + f[3] - f[4] - f[5] - f[6] - f[7];
  c[3] =   f[0] - f[1] + f[2] - f[3] + f[4] - f[5] + f[6] - f[7];
  c[4] = - f[0] + f[1] + f[2] - f[3] + f[4] - f[5] - f[6] + f[7];
  c[5] = - f[0] - f[1] + f[2] + f[3] + f[4] + f[5] - f[6] - f[7];
  c[6] =   f[0] - f[1] + f[2] - f[3] - f[4] + f[5] - f[6] + f[7];
  c[7] =   f[0] + f[1] + f[2] + f[3] + f[4] + f[5] + f[6] + f[7];
  return (c[0]*p[0] + c[1]*p[1] + c[2]*p[2] +
	  c[3]*p[0]*p[1] + c[4]*p[0]*p[2] + c[5]*p[1]*p[2] +
	  c[6]*p[0]*p[1]*p[2] +
	  c[7])/8.;
}

// gfs_particle_bc, modules/particulatecommon.c:3326-3395: a particle that left the box is taken
// off the list (or marked for the box across a GfsBoundaryMpi side) unless a periodic side puts it
// back; stores the position
template <int DIM>
__device__ void particle_bc_and_store (const PartArgs & A, int q, int depth, const int cell[3],
				       double p[3], double po[3])
{
  const int n = A.L.n;
  const double h = 1./n;
  int cn[3];
  bool keep = true;
  int mig = 0;
  if (!locate<DIM> (depth, p, cn)) {
    // boundarycell (:3149-3186): march from the cell of pos_old to the box side
    int d = 0;
    int cc[3] = { cell[0], cell[1], cell[2] };
    for (int guard = 0; guard < 4*n; guard++) {
      double cellpos[3] = { -0.5 + (cc[0] - 0.5)*h, -0.5 + (cc[1] - 0.5)*h,
			    DIM == 3 ? -0.5 + (cc[2] - 0.5)*h : 0. };
      check_intersection<DIM> (cellpos, po, p, &d, h);
      int c = d/2, next = cc[c] + ((d & 1) ? -1 : 1);
      if (next < 1 || next > n)
	break;
      cc[c] = next;
    }
    if (A.side[d] == GFSHIP_SIDE_EXTERNAL && A.migrate)
      mig = 2 + d;                  /* GfsBoundaryMpi: sent to the box across the side */
    else if (A.side[d] != GFSHIP_SIDE_PERIODIC)
      keep = false;                 /* taken off the list, nothing puts it back */
    else {
      // periodic_bc_particle (:3189-3214), box of size 1 matching itself
      double size = 1.;
      double normal = (double) (d ^ 1) - (double) d;
      double box_face = 0., box_face_nbr = 0.;
      box_face += normal*size/2.;
      box_face_nbr -= normal*size/2.;
      double tolerance = size/1.e8;
      double distance = (p[d/2] - box_face)*normal;
      p[d/2] = box_face_nbr + distance + normal*tolerance;
      po[d/2] = p[d/2];
    }
  }
#pragma unroll
  for (int c = 0; c < DIM; c++) {
    A.pos[c][q] = p[c];
    A.old[c][q] = po[c];
  }
  if (!keep)
    A.alive[q] = 0;
  else if (mig)
    A.alive[q] = (unsigned char) mig;
}

template <int DIM>
__global__ void __launch_bounds__(256)
particle_list_event_kernel (PartArgs A, int depth)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= A.n) return;
  if (A.alive[q] != 1) return;
  double p[3] = { A.pos[0][q], A.pos[1][q], DIM == 3 ? A.pos[2][q] : 0. };
  int cell[3];
  // remove_particles_not_in_domain, modules/particulatecommon.c:955-969
  if (!locate<DIM> (depth, p, cell)) {
    A.alive[q] = 0;
    return;
  }
  // gfs_particle_event (src/particle.c:31-44): pos_old = pos; gfs_domain_advect_point
  double po[3] = { p[0], p[1], p[2] };
  {
    double p1[3] = { p[0], p[1], p[2] };
#pragma unroll
    for (int c = 0; c < DIM; c++)
      p1[c] += A.dt*interpolate<DIM> (A.L, A.u[c], cell, po)/2.;
    int cell1[3];
    if (locate<DIM> (depth, p1, cell1)) {
#pragma unroll
      for (int c = 0; c < DIM; c++)
	p[c] += A.dt*interpolate<DIM> (A.L, A.u[c], cell1, p1);
    }
  }
  particle_bc_and_store<DIM> (A, q, depth, cell, p, po);
}

// ---------------------------------------------------------------------------------------------
// GfsParticulate with forces (modules/particulatecommon.c:91-842): uniform box.  The forces, the integration
// step and the coefficient inputs are those of particulate_forces.hpp (shared with tree_particles.hip); the
// kernels here locate the particle, gather what the forces read of the fluid, store and apply gfs_particle_bc.
// The density and the viscosity of the fluid are those of the
// cell that holds the particle (:273-279, 349-359, 439-445, 534-541, 631-632): the kernels are
// instantiated on RHO (fluid_rho = 1./alpha_cell[idx]; false: alpha = NULL, fluid_rho = 1.) and on MU
// (viscosity = mu_cell[idx], gfs_diffusion_cell; false: the constant of the launch).  <false, false>
// takes ParticulateArgs itself: the kernel arguments of a build without the two fields.
// ---------------------------------------------------------------------------------------------
// the arguments of <false, false>: the list's box, then the state and the forces of its particulates, in the layout
// the kernels have always had
struct BoxListArgs { PartArgs P; };
struct ParticulateArgs : BoxListArgs, ParticleForceArgs {};

// the arguments of an instantiation that reads a field of the fluid at the particle's cell
struct ParticulateFieldArgs : ParticulateArgs {
  const double * alpha_cell, * mu_cell;      // leaf level, layout of P.u; nullptr where not read
};
template <bool RHO, bool MU>
using ParticulateArgsOf = std::conditional_t<RHO || MU, ParticulateFieldArgs, ParticulateArgs>;

// fluid_rho (1./gfs_function_value (alpha, cell), :273-274) and the viscosity (gfs_diffusion_cell
// (d->D, cell), :277-279) of cell idx
template <bool RHO, class Args>
__device__ __forceinline__ double cell_fluid_rho (const Args & A, long idx)
{
  if constexpr (RHO) return 1./A.alpha_cell[idx];
  else return 1.;
}

// (MU = false: 0., never read -- the constant of the launch is read where it is used, as in a build
// without the fields)
template <bool MU, class Args>
__device__ __forceinline__ double cell_viscosity (const Args & A, long idx)
{
  if constexpr (MU) return A.mu_cell[idx];
  else return 0.;
}

// gfs_center_gradient, src/fluid.c:434-475, both neighbours at the same level (x1 = x2 = 1.)
__device__ __forceinline__ double center_gradient (const double * __restrict__ v, long idx, long off)
{
  const double v0 = v[idx], v1 = v[idx - off], v2 = v[idx + off];
  return ((v2 - v0) + (v0 - v1))/2.;
}

// the sources of particulate_forces.hpp on a box: gfs_center_gradient (cell, c2, u[c]) and u[c2] at cell idx,
// gfs_interpolate of component c of U (or Un) at p
struct BoxGradient {
  const PartArgs & P; long idx; const long * off;
  __device__ __forceinline__ double operator() (int c, int c2) const { return center_gradient (P.u[c], idx, off[c2]); }
};
struct BoxCellU {
  const PartArgs & P; long idx;
  __device__ __forceinline__ double operator() (int c2) const { return P.u[c2][idx]; }
};
template <int DIM>
struct BoxInterpolated {
  const Layout & L; const double * const * u; const int * cell; const double * p;
  __device__ __forceinline__ double operator() (int c) const { return interpolate<DIM> (L, u[c], cell, p); }
};

// compute_inertial_force at cell idx: a function of its own, which takes the three interpolations of Un with it
// when it is inlined
template <int DIM, bool RHO, class Args>
__device__ void box_inertial_force (const Args & A, const int cell[3], const double p[3], long idx,
				    const double fvel[3], double force[3])
{
  const Layout & L = A.P.L;
  const long off[3] = { 1, (long) L.sy, (long) L.sz };
  inertial_force<DIM> (cell_fluid_rho<RHO> (A, idx), A.P.dt, 1./L.n, fvel, BoxInterpolated<DIM> { L, A.uold, cell, p },
		       BoxGradient { A.P, idx, off }, BoxCellU { A.P, idx }, force);
}

// the viscosity of the fluid at the particle: that of its cell, or the constant of the launch read at its use
template <bool MU, class Args>
__device__ __forceinline__ auto viscosity_source (const Args & A, double mu)
{
  if constexpr (MU) return ValueOf { mu };
  else return ListViscosity { A };
}

// the variables a GfsFunction of a GfsForceCoeff sees: coefficient_inputs (particulate_forces.hpp) at the
// particle's cell
template <int DIM, bool RHO, bool MU>
__global__ void __launch_bounds__(256)
particulate_coeff_inputs_kernel (ParticulateArgsOf<RHO, MU> A, int depth)
{
  const PartArgs & P = A.P;
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= P.n) return;
  if (P.alive[q] != 1) return;
  const Layout & L = P.L;
  double p[3] = { P.pos[0][q], P.pos[1][q], DIM == 3 ? P.pos[2][q] : 0. };
  int cell[3];
  if (!locate<DIM> (depth, p, cell)) return;
  const unsigned o = A.orig[q];
  const long idx = RHO || MU ? L.idx (cell[0], cell[1], DIM == 3 ? cell[2] : 0) : 0;
  const double fluid_rho = cell_fluid_rho<RHO> (A, idx);
  const double mu = cell_viscosity<MU> (A, idx);
  double fvel[3] = { 0., 0., 0. };
#pragma unroll
  for (int c = 0; c < DIM; c++)
    fvel[c] = interpolate<DIM> (L, P.u[c], cell, p);
  coefficient_inputs<DIM> (A, q, o, fvel, fluid_rho, viscosity_source<MU> (A, mu));
}

// gfs_particulate_event (:768-842) in a gfs_particle_list_event (:980-1015)
// ONFLUID: the forces of the fluid on the particle that a GfsSourceParticulate gives back to the fluid
// (compute_forces_onfluid, :753-765, in source_particulate_event, :2199-2206): force = 0, then every force
// of the list but GfsForceBuoy, force[c] = new_force[c]*volume + force[c]; `force' is written, and `mass':
// compute_addedmass_force adds to particulate->mass here as in an event (:391) and nothing takes it back.
// The particle does not move and stays on the list; a particle without a cell gets the zero force every
// compute_*_force returns there and keeps its mass
// (tree_particulate_list_event_kernel, tree_particles.hip, is this kernel on the leaves of a tree)
template <int DIM, bool RHO, bool MU, bool ONFLUID = false>
__global__ void __launch_bounds__(256)
particulate_list_event_kernel (ParticulateArgsOf<RHO, MU> A, int depth)
{
  const PartArgs & P = A.P;
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= P.n) return;
  if (P.alive[q] != 1) return;
  const Layout & L = P.L;
  double p[3] = { P.pos[0][q], P.pos[1][q], DIM == 3 ? P.pos[2][q] : 0. };
  int cell[3];
  // remove_particles_not_in_domain, :955-969
  if (!locate<DIM> (depth, p, cell)) {
    if constexpr (ONFLUID) {
      const unsigned o = A.orig[q];
#pragma unroll
      for (int c = 0; c < 3; c++)
	A.force[c][o] = 0.;
    }
    else
      P.alive[q] = 0;
    return;
  }
  const unsigned o = A.orig[q];
  const long idx = L.idx (cell[0], cell[1], DIM == 3 ? cell[2] : 0);
  const long off[3] = { 1, (long) L.sy, (long) L.sz };
  const double size = 1./L.n;
  // the two fields of the fluid at the particle's cell: loads that depend on idx alone, issued here with
  // the first gathers of the interpolation, not behind its chain
  const double fluid_rho = cell_fluid_rho<RHO> (A, idx);
  const double mu = cell_viscosity<MU> (A, idx);
  const double dt = P.dt;
  double po[3] = { p[0], p[1], p[2] };
  double vel[3] = { A.vel[0][o], A.vel[1][o], A.vel[2][o] };
  double mass = A.mass[o];
  const double volume = A.volume[o];
  double pf[3] = { 0., 0., 0. };
  ForceNeeds need;
  force_needs<ONFLUID> (A, need);
  const BoxGradient grad = { P, idx, off };
  double fvel[3] = { 0., 0., 0. }, dudt[3] = { 0., 0., 0. };
  if (need.fvel) {
#pragma unroll
    for (int c = 0; c < DIM; c++)
      fvel[c] = interpolate<DIM> (L, P.u[c], cell, p);
  }
  if (need.dudt)
    box_inertial_force<DIM, RHO> (A, cell, p, idx, fvel, dudt);
  particulate_forces<DIM, ONFLUID> (A, q, o, fluid_rho, viscosity_source<MU> (A, mu), size, grad, fvel, dudt, vel,
				    volume, mass, pf);
  if constexpr (ONFLUID) {
#pragma unroll
    for (int c = 0; c < 3; c++)
      A.force[c][o] = pf[c];
    A.mass[o] = mass;
    return;
  }
  particulate_advance<DIM> (p, vel, pf, dt, mass);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    A.vel[c][o] = vel[c];
    A.force[c][o] = pf[c];
  }
  A.mass[o] = mass;
  particle_bc_and_store<DIM> (P, q, depth, cell, p, po);
}

// the instantiations without fields come first, in the order of a build without the two fields
template __global__ void particulate_coeff_inputs_kernel<3, false, false> (ParticulateArgs, int);
template __global__ void particulate_coeff_inputs_kernel<2, false, false> (ParticulateArgs, int);
template __global__ void particulate_list_event_kernel<3, false, false> (ParticulateArgs, int);
template __global__ void particulate_list_event_kernel<2, false, false> (ParticulateArgs, int);


// mpi_send_particle (modules/particulatecommon.c:3218-3222): the particles marked 2 + d go into the
// packet of side d (7 doubles: position and old position in the coordinates of the receiving
// box -- the same point of space, one box size less along the normal -- and the id) and leave
// the list
struct OutboxArgs {
  int n, out_cap, rs;          // rs doubles per record: 7, or 15 for particulates
  const double * pos[3], * old[3];
  const unsigned * id;
  unsigned char * alive;
  double * outbox;
  unsigned * out_count;
  const unsigned * orig;       // particulates: state indexed by the creation slot
  const double * vel[3], * force[3], * mass, * volume;
};

__global__ void __launch_bounds__(256)
particle_outbox_kernel (OutboxArgs A)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= A.n) return;
  int code = A.alive[q];
  if (code < 2) return;
  int d = code - 2;
  A.alive[q] = 0;
  unsigned k = atomicAdd (A.out_count + d, 1u);
  if (k >= (unsigned) A.out_cap) return;      /* the host sees the count and reports the overflow */
  double * r = A.outbox + (size_t) A.rs*((size_t) d*A.out_cap + k);
  double normal = (double) (d ^ 1) - (double) d;
#pragma unroll
  for (int c = 0; c < 3; c++) { r[c] = A.pos[c][q]; r[3 + c] = A.old[c][q]; }
  r[d/2] -= normal*1.;
  r[3 + d/2] -= normal*1.;
  r[6] = (double) A.id[q];
  if (A.rs > 7) {
    const unsigned o = A.orig[q];
#pragma unroll
    for (int c = 0; c < 3; c++) { r[7 + c] = A.vel[c][o]; r[12 + c] = A.force[c][o]; }
    r[10] = A.mass[o];
    r[11] = A.volume[o];
  }
}

// key = linear index of the containing leaf cell, dead or outside particles last
// (tree_particle_keys_kernel, tree_particles.hip, is this kernel on the leaves of a tree)
template <int DIM>
__global__ void __launch_bounds__(256)
particle_keys_kernel (Layout L, int depth, int n, const double * __restrict__ x,
		      const double * __restrict__ y, const double * __restrict__ z,
		      const unsigned char * __restrict__ alive, unsigned * __restrict__ key,
		      unsigned * __restrict__ slot)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= n) return;
  unsigned k = 0xFFFFFFFFu;
  if (alive[q] == 1) {
    double p[3] = { x[q], y[q], DIM == 3 ? z[q] : 0. };
    int c[3];
    if (locate<DIM> (depth, p, c))
      k = (unsigned) (c[0] - 1) + (unsigned) L.n*((unsigned) (c[1] - 1) +
						 (DIM == 3 ? (unsigned) L.n*(unsigned) (c[2] - 1) : 0u));
  }
  key[q] = k;
  slot[q] = q;
}

struct GatherArgs {
  int n;
  const unsigned * slot;
  const double * pos[3], * old[3];
  const unsigned * id, * orig;
  const unsigned char * alive;
  double * pos2[3], * old2[3];
  unsigned * id2, * orig2;
  unsigned char * alive2;
};

__global__ void __launch_bounds__(256)
particle_gather_kernel (GatherArgs G)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= G.n) return;
  unsigned s = G.slot[q];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    G.pos2[c][q] = G.pos[c][s];
    G.old2[c][q] = G.old[c][s];
  }
  G.id2[q] = G.id[s];
  G.orig2[q] = G.orig[s];
  G.alive2[q] = G.alive[s];
}

// GfsOutputLocation (src/output.c:1182-1199): gfs_domain_locate then gfs_interpolate of one
// variable at arbitrary points
template <int DIM>
__global__ void __launch_bounds__(256)
sample_kernel (Layout L, int depth, int np, const double * __restrict__ pos,
	       const double * __restrict__ v, double * __restrict__ out,
	       unsigned char * __restrict__ inside)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= np) return;
  double p[3] = { pos[3*(size_t) q], pos[3*(size_t) q + 1], DIM == 3 ? pos[3*(size_t) q + 2] : 0. };
  int cell[3];
  if (!locate<DIM> (depth, p, cell)) {
    inside[q] = 0;
    out[q] = 0.;
    return;
  }
  inside[q] = 1;
  out[q] = interpolate<DIM> (L, v, cell, p);
}

__global__ void __launch_bounds__(256)
count_alive_kernel (const unsigned char * alive, int n, unsigned * count)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  unsigned long long m = __ballot (q < n && alive[q] == 1);
  if ((threadIdx.x & 63) == 0 && m)
    atomicAdd (count, (unsigned) __popcll (m));
}

// update_vol / update_mass (modules/particulatecommon.c:2806-2824, 2964-2982) up to the call of the function:
// gfs_domain_locate, the radius, gfs_interpolate of the velocity and the relative velocity of one particle,
// stored at its creation slot (what the function and the ordered pass of particulate_sources.hip read)
struct SourceGatherArgs {
  Layout L;
  int depth, n;
  const double * pos[3];
  const unsigned char * alive;
  const unsigned * orig;
  const double * u[3], * vel[3], * volume;
  unsigned * cell;
  double * rad, * urel[3];
};

// (tree_particulate_source_gather_kernel, tree_particles.hip, is this kernel on the leaves of a tree)
template <int DIM>
__global__ void __launch_bounds__(256)
particulate_source_gather_kernel (SourceGatherArgs A)
{
  int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= A.n) return;
  const unsigned o = A.orig[q];
  double p[3] = { A.pos[0][q], A.pos[1][q], DIM == 3 ? A.pos[2][q] : 0. };
  int c[3];
  if (A.alive[q] != 1 || !locate<DIM> (A.depth, p, c)) {
    A.cell[o] = PSOURCE_NO_CELL;
    return;
  }
  const unsigned n = (unsigned) A.L.n;
  A.cell[o] = (unsigned) (c[0] - 1) + n*((unsigned) (c[1] - 1) + (DIM == 3 ? n*(unsigned) (c[2] - 1) : 0u));
  A.rad[o] = pow (3.0*A.volume[o]/4.0/M_PI, 1./3.);      /* :2812, the device's pow */
#pragma unroll
  for (int a = 0; a < DIM; a++)
    A.urel[a][o] = interpolate<DIM> (A.L, A.u[a], c, p) - A.vel[a][o];
}

// feed_particulate (modules/particulatecommon.c:2377-2393) for one candidate per thread: gfs_domain_locate, then
// vel[c] = gfs_interpolate (cell, pos, u[c]) (vel.z = 0. in 2-D); the slot is that of a new object (pos_old = 0,
// force = 0) whose fate the ordered passes of feed_particle.hip decide
struct FeedGatherArgs {
  Layout L;
  int depth, np, base;
  const double * cand;
  const double * u[3];
  double * pos[3], * old[3], * vel[3], * force[3];
  unsigned * orig, * cell;
};

template <int DIM>
__global__ void __launch_bounds__(256)
feed_gather_kernel (FeedGatherArgs A)
{
  int i = blockIdx.x*blockDim.x + threadIdx.x;
  if (i >= A.np) return;
  const int s = A.base + i;
  const double p[3] = { A.cand[3*(size_t) i], A.cand[3*(size_t) i + 1], A.cand[3*(size_t) i + 2] };
#pragma unroll
  for (int c = 0; c < 3; c++) {
    A.pos[c][s] = p[c];
    A.old[c][s] = 0.;
    A.force[c][s] = 0.;
  }
  A.orig[s] = (unsigned) s;
  int c[3];
  double vel[3] = { 0., 0., 0. };
  unsigned cell = PSOURCE_NO_CELL;
  if (locate<DIM> (A.depth, p, c)) {
    const unsigned n = (unsigned) A.L.n;
    cell = (unsigned) (c[0] - 1) + n*((unsigned) (c[1] - 1) + (DIM == 3 ? n*(unsigned) (c[2] - 1) : 0u));
#pragma unroll
    for (int a = 0; a < DIM; a++)
      vel[a] = interpolate<DIM> (A.L, A.u[a], c, p);
  }
  A.cell[i] = cell;
#pragma unroll
  for (int a = 0; a < 3; a++)
    A.vel[a][s] = vel[a];
}

} // namespace gfship

using namespace gfship;

extern "C" {

int gfship_particles_create (gfship_particles ** out, gfship_sim * sim, int np,
			     const double * pos, const unsigned * id)
{
  GFSHIP_CHECK (out && sim && (np == 0 || (pos && id)) && np >= 0, GFSHIP_EINVAL, "invalid argument");
  *out = nullptr;
  gfship_particles * pl = new gfship_particles;
  pl->sim = sim;
  pl->dom = gfship_sim_view_get (sim).dom;
  pl->stream = pl->dom->stream;
  pl->dim = pl->dom->dim;
  int r = gfship::particles_alloc (pl, np, pos, id);
  if (r) return r;
  *out = pl;
  return GFSHIP_OK;
}

} // extern "C"

int gfship::particles_alloc (gfship_particles * pl, int np, const double * pos, const unsigned * id)
{
  pl->n = np;
  pl->np0 = np;
  pl->cap = std::max (np, 1);
  size_t m = pl->cap;
  std::vector<double> tmp (m);
  for (int c = 0; c < 3; c++) {
    GFSHIP_HIP (hipMalloc ((void **) &pl->pos[c], m*sizeof (double)));
    GFSHIP_HIP (hipMalloc ((void **) &pl->old[c], m*sizeof (double)));
    for (int q = 0; q < np; q++) tmp[q] = pos[3*(size_t) q + c];
    GFSHIP_HIP (hipMemcpy (pl->pos[c], tmp.data (), m*sizeof (double), hipMemcpyHostToDevice));
    GFSHIP_HIP (hipMemcpy (pl->old[c], tmp.data (), m*sizeof (double), hipMemcpyHostToDevice));
  }
  GFSHIP_HIP (hipMalloc ((void **) &pl->id, m*sizeof (unsigned)));
  if (np) GFSHIP_HIP (hipMemcpy (pl->id, id, np*sizeof (unsigned), hipMemcpyHostToDevice));
  GFSHIP_HIP (hipMalloc ((void **) &pl->alive, m));
  GFSHIP_HIP (hipMemset (pl->alive, 1, m));
  GFSHIP_HIP (hipMalloc ((void **) &pl->d_count, sizeof (unsigned)));
  GFSHIP_HIP (hipMalloc ((void **) &pl->d_idlast, sizeof (unsigned)));
  GFSHIP_HIP (hipMemset (pl->d_idlast, 0, sizeof (unsigned)));      /* gfs_particle_list_init */
  for (int c = 0; c < 3; c++) {
    GFSHIP_HIP (hipMalloc ((void **) &pl->pos2[c], m*sizeof (double)));
    GFSHIP_HIP (hipMalloc ((void **) &pl->old2[c], m*sizeof (double)));
  }
  unsigned ** ua[] = { &pl->orig, &pl->orig2, &pl->id2, &pl->key, &pl->key2, &pl->slot, &pl->slot2 };
  for (unsigned ** a : ua)
    GFSHIP_HIP (hipMalloc ((void **) a, m*sizeof (unsigned)));
  GFSHIP_HIP (hipMalloc ((void **) &pl->alive2, m));
  {
    std::vector<unsigned> iota (m);
    std::iota (iota.begin (), iota.end (), 0u);
    GFSHIP_HIP (hipMemcpy (pl->orig, iota.data (), m*sizeof (unsigned), hipMemcpyHostToDevice));
  }
  return GFSHIP_OK;
}

extern "C" {

void gfship_particles_destroy (gfship_particles * pl)
{
  if (!pl) return;
  (void) hipStreamSynchronize (pl->stream);
  for (int c = 0; c < 3; c++) {
    if (pl->pos[c]) (void) hipFree (pl->pos[c]);
    if (pl->old[c]) (void) hipFree (pl->old[c]);
  }
  if (pl->id) (void) hipFree (pl->id);
  if (pl->alive) (void) hipFree (pl->alive);
  if (pl->d_count) (void) hipFree (pl->d_count);
  if (pl->d_idlast) (void) hipFree (pl->d_idlast);
  for (int c = 0; c < 3; c++) {
    if (pl->pos2[c]) (void) hipFree (pl->pos2[c]);
    if (pl->old2[c]) (void) hipFree (pl->old2[c]);
  }
  void * extra[] = { pl->orig, pl->orig2, pl->id2, pl->key, pl->key2, pl->slot, pl->slot2,
		     pl->alive2, pl->sort_tmp, pl->outbox, pl->out_count };
  for (void * a : extra)
    if (a) (void) hipFree (a);
  for (int c = 0; c < 3; c++) {
    if (pl->vel[c]) (void) hipFree (pl->vel[c]);
    if (pl->force[c]) (void) hipFree (pl->force[c]);
    if (pl->uold[c] >= 0 && pl->dom) gfship_field_free (pl->dom, pl->uold[c]);
  }
  if (pl->mass) (void) hipFree (pl->mass);
  if (pl->volume) (void) hipFree (pl->volume);
  if (pl->dia) (void) hipFree (pl->dia);
  if (pl->rb) (void) hipFree (pl->rb);
  gfship::coupling_free (pl);
  for (int f = 0; f < 8; f++) {
    if (pl->coef[f]) (void) hipFree (pl->coef[f]);
    gfship::rtc_free (pl->coef_fn[f]);
  }
  for (int q = 0; q < 6; q++)
    if (pl->cin[q]) (void) hipFree (pl->cin[q]);
  delete pl;
}

int gfship_field_interpolate (gfship_domain * dom, gfship_field v, int np, const double * pos,
			      double * out, unsigned char * inside)
{
  GFSHIP_CHECK (dom && pos && out && inside && np >= 0, GFSHIP_EINVAL, "invalid argument");
  Field * V = get_field (dom, v);
  if (!V) return GFSHIP_EINVAL;
  if (np == 0) return GFSHIP_OK;
  double * dpos = nullptr, * dout = nullptr;
  unsigned char * din = nullptr;
  GFSHIP_HIP (hipMalloc ((void **) &dpos, 3*(size_t) np*sizeof (double)));
  GFSHIP_HIP (hipMalloc ((void **) &dout, (size_t) np*sizeof (double)));
  GFSHIP_HIP (hipMalloc ((void **) &din, (size_t) np));
  int r = GFSHIP_OK;
  hipError_t e = hipMemcpyAsync (dpos, pos, 3*(size_t) np*sizeof (double), hipMemcpyHostToDevice,
				 dom->stream);
  if (e == hipSuccess) {
    int block = 256, grid = (np + block - 1)/block;
    const Layout & L = dom->lay[dom->depth];
    if (dom->dim == 3)
      hipLaunchKernelGGL (sample_kernel<3>, dim3 (grid), dim3 (block), 0, dom->stream, L, dom->depth,
			  np, dpos, V->lev[dom->depth], dout, din);
    else
      hipLaunchKernelGGL (sample_kernel<2>, dim3 (grid), dim3 (block), 0, dom->stream, L, dom->depth,
			  np, dpos, V->lev[dom->depth], dout, din);
    e = hipGetLastError ();
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync (out, dout, (size_t) np*sizeof (double), hipMemcpyDeviceToHost, dom->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync (inside, din, (size_t) np, hipMemcpyDeviceToHost, dom->stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize (dom->stream);
  if (e != hipSuccess)
    r = hip_fail (e, "gfship_field_interpolate", __FILE__, __LINE__);
  (void) hipFree (dpos); (void) hipFree (dout); (void) hipFree (din);
  return r;
}

int gfship_particles_set_sort_interval (gfship_particles * pl, int every)
{
  GFSHIP_CHECK (pl != nullptr && every >= 0, GFSHIP_EINVAL, "invalid argument");
  pl->sort_every = every;
  return GFSHIP_OK;
}

int gfship_particles_sort (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  if (pl->n == 0) return GFSHIP_OK;
  gfship_domain * dom = pl->dom;
  hipStream_t stream = pl->stream;
  int block = 256, grid = (pl->n + block - 1)/block;
  int bits;
  if (pl->tree) {      /* key = the leaf in the concatenated levels of the tree */
    int r = gfship::tree_particle_keys (pl, &bits);
    if (r) return r;
  }
  else {
    const Layout & L = dom->lay[dom->depth];
    if (dom->dim == 3)
      hipLaunchKernelGGL (particle_keys_kernel<3>, dim3 (grid), dim3 (block), 0, dom->stream, L,
			  dom->depth, pl->n, pl->pos[0], pl->pos[1], pl->pos[2], pl->alive, pl->key,
			  pl->slot);
    else
      hipLaunchKernelGGL (particle_keys_kernel<2>, dim3 (grid), dim3 (block), 0, dom->stream, L,
			  dom->depth, pl->n, pl->pos[0], pl->pos[1], pl->pos[2], pl->alive, pl->key,
			  pl->slot);
    GFSHIP_HIP (hipGetLastError ());
    /* the key needs dim*depth bits (+1 so that the all-ones key of the dead sorts last) */
    bits = dom->dim*dom->depth + 1;
  }
  size_t need = 0;
  GFSHIP_HIP (hipcub::DeviceRadixSort::SortPairs (nullptr, need, pl->key, pl->key2, pl->slot,
						  pl->slot2, pl->n, 0, 32, stream));
  if (need > pl->sort_tmp_bytes) {
    if (pl->sort_tmp) GFSHIP_HIP (hipFree (pl->sort_tmp));
    pl->sort_tmp = nullptr;
    GFSHIP_HIP (hipMalloc (&pl->sort_tmp, need));
    pl->sort_tmp_bytes = need;
  }
  if (bits > 32) bits = 32;
  size_t tmp_bytes = pl->sort_tmp_bytes;
  GFSHIP_HIP (hipcub::DeviceRadixSort::SortPairs (pl->sort_tmp, tmp_bytes, pl->key, pl->key2,
						  pl->slot, pl->slot2, pl->n, 0, bits, stream));
  GatherArgs G;
  G.n = pl->n;
  G.slot = pl->slot2;
  for (int c = 0; c < 3; c++) {
    G.pos[c] = pl->pos[c]; G.old[c] = pl->old[c];
    G.pos2[c] = pl->pos2[c]; G.old2[c] = pl->old2[c];
  }
  G.id = pl->id; G.orig = pl->orig; G.alive = pl->alive;
  G.id2 = pl->id2; G.orig2 = pl->orig2; G.alive2 = pl->alive2;
  hipLaunchKernelGGL (particle_gather_kernel, dim3 (grid), dim3 (block), 0, stream, G);
  GFSHIP_HIP (hipGetLastError ());
  for (int c = 0; c < 3; c++) {
    std::swap (pl->pos[c], pl->pos2[c]);
    std::swap (pl->old[c], pl->old2[c]);
  }
  std::swap (pl->id, pl->id2);
  std::swap (pl->orig, pl->orig2);
  std::swap (pl->alive, pl->alive2);
  pl->events_since_sort = 0;
  return GFSHIP_OK;
}

} // extern "C"

// grow the per-particle arrays to at least `need` slots (contents of the live arrays kept)
int gfship::particles_reserve (gfship_particles * pl, int need)
{
  if (need <= pl->cap) return GFSHIP_OK;
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));      /* of the box or of the tree */
  size_t m = std::max (need, 2*pl->cap), old = pl->cap;
  auto grow = [&] (void ** a, size_t elem, bool keep) -> hipError_t {
    void * nw = nullptr;
    hipError_t e = hipMalloc (&nw, m*elem);
    if (e != hipSuccess) return e;
    if (keep && *a) e = hipMemcpy (nw, *a, old*elem, hipMemcpyDeviceToDevice);
    if (*a) (void) hipFree (*a);
    *a = nw;
    return e;
  };
  for (int c = 0; c < 3; c++) {
    GFSHIP_HIP (grow ((void **) &pl->pos[c], sizeof (double), true));
    GFSHIP_HIP (grow ((void **) &pl->old[c], sizeof (double), true));
    GFSHIP_HIP (grow ((void **) &pl->pos2[c], sizeof (double), false));
    GFSHIP_HIP (grow ((void **) &pl->old2[c], sizeof (double), false));
  }
  GFSHIP_HIP (grow ((void **) &pl->id, sizeof (unsigned), true));
  GFSHIP_HIP (grow ((void **) &pl->orig, sizeof (unsigned), true));
  GFSHIP_HIP (grow ((void **) &pl->alive, 1, true));
  unsigned ** scratch[] = { &pl->orig2, &pl->id2, &pl->key, &pl->key2, &pl->slot, &pl->slot2 };
  for (unsigned ** a : scratch)
    GFSHIP_HIP (grow ((void **) a, sizeof (unsigned), false));
  GFSHIP_HIP (grow ((void **) &pl->alive2, 1, false));
  if (pl->particulate) {
    for (int c = 0; c < 3; c++) {
      GFSHIP_HIP (grow ((void **) &pl->vel[c], sizeof (double), true));
      GFSHIP_HIP (grow ((void **) &pl->force[c], sizeof (double), true));
    }
    GFSHIP_HIP (grow ((void **) &pl->mass, sizeof (double), true));
    GFSHIP_HIP (grow ((void **) &pl->volume, sizeof (double), true));
    GFSHIP_HIP (grow ((void **) &pl->dia, sizeof (double), true));
    /* rb of the particles on the list is kept; a GfsFeedParticle writes it for its newcomers, a GfsBoundaryMpi
       side does not (every reader of rb refuses a box with such sides, coupling.hip) */
    GFSHIP_HIP (grow ((void **) &pl->rb, sizeof (double), true));
  }
  pl->cap = (int) m;
  return GFSHIP_OK;
}

extern "C" {

// send_particles / rcv_particles through the GfsBoundaryMpi sides
// (modules/particulatecommon.c:3247-3312): packets per side out, the neighbours' packets in
static int particles_migrate (gfship_particles * pl)
{
  gfship_domain * dom = pl->dom;
  const int rs = pl->particulate ? 15 : 7;
  const int want = std::max (4096, pl->n/4);
  if (pl->out_cap < want) {
    if (pl->outbox) GFSHIP_HIP (hipFree (pl->outbox));
    pl->outbox = nullptr;
    GFSHIP_HIP (hipMalloc ((void **) &pl->outbox, 6*(size_t) want*15*sizeof (double)));
    pl->out_cap = want;
  }
  if (!pl->out_count)
    GFSHIP_HIP (hipMalloc ((void **) &pl->out_count, 6*sizeof (unsigned)));
  GFSHIP_HIP (hipMemsetAsync (pl->out_count, 0, 6*sizeof (unsigned), dom->stream));
  OutboxArgs O;
  O.n = pl->n; O.out_cap = pl->out_cap; O.rs = rs;
  O.orig = pl->orig; O.mass = pl->mass; O.volume = pl->volume;
  for (int c = 0; c < 3; c++) { O.vel[c] = pl->vel[c]; O.force[c] = pl->force[c]; }
  for (int c = 0; c < 3; c++) { O.pos[c] = pl->pos[c]; O.old[c] = pl->old[c]; }
  O.id = pl->id; O.alive = pl->alive; O.outbox = pl->outbox; O.out_count = pl->out_count;
  if (pl->n > 0) {
    hipLaunchKernelGGL (particle_outbox_kernel, dim3 ((pl->n + 255)/256), dim3 (256), 0, dom->stream, O);
    GFSHIP_HIP (hipGetLastError ());
  }
  unsigned cnt[6];
  GFSHIP_HIP (hipMemcpyAsync (cnt, pl->out_count, sizeof (cnt), hipMemcpyDeviceToHost, dom->stream));
  GFSHIP_HIP (hipStreamSynchronize (dom->stream));
  std::vector<double> send[6];
  int nsend[6], nrecv[6] = { 0, 0, 0, 0, 0, 0 };
  const double * sp[6], * rp[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
  for (int d = 0; d < 6; d++) {
    GFSHIP_CHECK (cnt[d] <= (unsigned) pl->out_cap, GFSHIP_ENOMEM,
		  "%u particles leave through side %d in one step: more than the %d the packet holds",
		  cnt[d], d, pl->out_cap);
    nsend[d] = (int) cnt[d];
    send[d].resize ((size_t) rs*cnt[d]);
    if (cnt[d])
      GFSHIP_HIP (hipMemcpy (send[d].data (), pl->outbox + (size_t) rs*d*pl->out_cap,
			     (size_t) rs*cnt[d]*sizeof (double), hipMemcpyDeviceToHost));
    /* the device fills the packet in no particular order: sort it by id */
    std::vector<size_t> o (cnt[d]);
    std::iota (o.begin (), o.end (), (size_t) 0);
    std::sort (o.begin (), o.end (), [&] (size_t a, size_t b) { return send[d][rs*a + 6] < send[d][rs*b + 6]; });
    std::vector<double> sorted (send[d].size ());
    for (size_t q = 0; q < o.size (); q++)
      memcpy (&sorted[rs*q], &send[d][rs*o[q]], rs*sizeof (double));
    send[d].swap (sorted);
    sp[d] = send[d].data ();
  }
  int r;
  std::vector<double> inbox[6];
  if (pl->migrate) {
    r = pl->migrate (pl->migrate_ctx, nsend, sp, nrecv, rp);
    GFSHIP_CHECK (r == 0, GFSHIP_EHIP, "the particle migration hook failed (%d)", r);
  }
  else {
    /* the library's communicator */
    if ((r = comm_migrate (dom, rs, nsend, sp, nrecv, inbox))) return r;
    for (int d = 0; d < 6; d++) rp[d] = inbox[d].data ();
  }
  int total = 0;
  for (int d = 0; d < 6; d++) total += nrecv[d];
  if (total == 0) return GFSHIP_OK;
  if ((r = particles_reserve (pl, pl->n + total))) return r;
  std::vector<double> col (total);
  std::vector<unsigned> ids (total), orig (total);
  std::vector<unsigned char> one (total, 1);
  for (int c = 0; c < 6; c++) {
    size_t k = 0;
    for (int d = 0; d < 6; d++)             /* box_rcv_bc: side by side, in packet order */
      for (int q = 0; q < nrecv[d]; q++)
	col[k++] = rp[d][(size_t) rs*q + c];
    GFSHIP_HIP (hipMemcpy ((c < 3 ? pl->pos[c] : pl->old[c - 3]) + pl->n, col.data (),
			   total*sizeof (double), hipMemcpyHostToDevice));
  }
  size_t k = 0;
  for (int d = 0; d < 6; d++)
    for (int q = 0; q < nrecv[d]; q++, k++) {
      ids[k] = (unsigned) rp[d][(size_t) rs*q + 6];
      orig[k] = (unsigned) (pl->n + k);
    }
  GFSHIP_HIP (hipMemcpy (pl->id + pl->n, ids.data (), total*sizeof (unsigned), hipMemcpyHostToDevice));
  GFSHIP_HIP (hipMemcpy (pl->orig + pl->n, orig.data (), total*sizeof (unsigned), hipMemcpyHostToDevice));
  GFSHIP_HIP (hipMemcpy (pl->alive + pl->n, one.data (), total, hipMemcpyHostToDevice));
  if (pl->particulate) {
    /* the state of the newcomers lives at their creation slots pl->n .. pl->n + total - 1 */
    for (int c = 0; c < 9; c++) {      /* record columns 7 .. 14: vel, mass, volume, force; then dia */
      size_t kk = 0;
      for (int d = 0; d < 6; d++)
	for (int q = 0; q < nrecv[d]; q++) {
	  const double * r = rp[d] + (size_t) rs*q;
	  col[kk++] = c < 8 ? r[7 + c] : 2.*pow (3.0*r[11]/4.0/M_PI, 1./3.);
	}
      double * dst = c < 3 ? pl->vel[c] : c == 3 ? pl->mass : c == 4 ? pl->volume :
	c < 8 ? pl->force[c - 5] : pl->dia;
      GFSHIP_HIP (hipMemcpy (dst + pl->n, col.data (), total*sizeof (double), hipMemcpyHostToDevice));
    }
  }
  pl->n += total;
  return GFSHIP_OK;
}

int gfship_particles_set_migrate (gfship_particles * pl, gfship_particle_migrate_fn fn, void * ctx)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_LIST (pl, "gfship_particles_set_migrate");
  pl->migrate = fn;
  pl->migrate_ctx = ctx;
  return GFSHIP_OK;
}

int gfship_particles_record_size (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_LIST (pl, "gfship_particles_record_size");
  return pl->particulate ? 15 : 7;
}

int gfship_particles_slots (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  return pl->n;
}

// store_domain_previous_vel, modules/particulatecommon.c:100-114: copy on the leaves, then the BC
// of the new variable (a scalar with the default BC)
static int store_previous_vel (gfship_particles * pl)
{
  gfship_domain * dom = pl->dom;
  gfship_sim_view v = gfship_sim_view_get (pl->sim);
  const Layout & L = dom->lay[dom->depth];
  for (int c = 0; c < dom->dim; c++) {
    GFSHIP_HIP (hipMemcpyAsync (dom->fields[pl->uold[c]].lev[dom->depth],
				dom->fields[v.u[c]].lev[dom->depth], L.total*sizeof (double),
				hipMemcpyDeviceToDevice, dom->stream));
    int r = gfship_bc (dom, pl->uold[c], pl->uold[c], dom->depth);
    if (r) return r;
  }
  return GFSHIP_OK;
}

// the fields of the fluid the forces of a list read (fluid_rho and viscosity of compute_*_force): alpha
// at the cell centres whenever the simulation has it, the viscosity of U at the leaf centres where U
// has one -- which it must where the viscosity of U is given on the faces
} // extern "C"

int gfship::particulate_fluid_check (const gfship_sim_view & v)
{
  GFSHIP_CHECK (!v.visc_faces || v.mu >= 0, GFSHIP_EUNSUPPORTED,
		"particle forces together with a viscosity that varies in space need the viscosity at the "
		"centres of the leaf cells (gfs_diffusion_cell): call gfship_sim_set_viscosity_cell first");
  GFSHIP_CHECK (!v.has_alpha || v.alpha_cell >= 0, GFSHIP_EUNSUPPORTED,
		"particle forces together with GfsPhysicalParams { alpha } need alpha at the cell centres "
		"(fluid_rho = 1./alpha): call gfship_sim_set_alpha_cell first");
  return GFSHIP_OK;
}

// the state of the particulates of a list and its forces, with the default coefficients
void gfship::particulate_force_args (const gfship_particles * pl, ParticleForceArgs & A)
{
  A.orig = pl->orig;
  for (int c = 0; c < 3; c++) {
    A.vel[c] = pl->vel[c];
    A.force[c] = pl->force[c];
    A.gravity[c] = pl->gravity[c];
  }
  A.mass = pl->mass; A.volume = pl->volume; A.dia = pl->dia;
  A.nforces = pl->nforces;
  for (int f = 0; f < 8; f++) {
    A.forces[f] = pl->forces[f];
    A.coef[f] = nullptr;
  }
  for (int q = 0; q < 6; q++) A.cin[q] = nullptr;
}

// the GfsFunction coefficients of the forces of a list: the inputs of every particle (launch_inputs: the
// coefficient-input kernel of the caller, which reads A), then one compiled kernel per function
int gfship::particulate_coefficients (gfship_particles * pl, ParticleForceArgs & A, hipStream_t stream, double t,
				      const std::function<void ()> & launch_inputs)
{
  bool any = false;
  for (int f = 0; f < pl->nforces; f++)
    if (pl->coef_fn[f]) any = true;
  if (!any)
    return GFSHIP_OK;
  if (pl->coef_cap < pl->cap) {
    for (int q = 0; q < 6; q++) {
      if (pl->cin[q]) GFSHIP_HIP (hipFree (pl->cin[q]));
      pl->cin[q] = nullptr;
      GFSHIP_HIP (hipMalloc ((void **) &pl->cin[q], (size_t) pl->cap*sizeof (double)));
    }
    for (int f = 0; f < 8; f++) {
      if (pl->coef[f]) GFSHIP_HIP (hipFree (pl->coef[f]));
      pl->coef[f] = nullptr;
    }
    pl->coef_cap = pl->cap;
  }
  for (int q = 0; q < 6; q++) A.cin[q] = pl->cin[q];
  launch_inputs ();
  GFSHIP_HIP (hipGetLastError ());
  const double * rel[3] = { pl->cin[1], pl->cin[2], pl->cin[3] };
  for (int f = 0; f < pl->nforces; f++)
    if (pl->coef_fn[f]) {
      if (!pl->coef[f])
	GFSHIP_HIP (hipMalloc ((void **) &pl->coef[f], (size_t) pl->coef_cap*sizeof (double)));
      const double * rep = pl->dim == 2 && pl->forces[f] == GFSHIP_FORCE_DRAG ? pl->cin[5] : pl->cin[0];
      int r = rtc_launch_coefficient (pl->coef_fn[f], stream, pl->n, pl->alive, rep, rel, pl->cin[4], t, pl->coef[f]);
      if (r) return r;
      A.coef[f] = pl->coef[f];
    }
  return GFSHIP_OK;
}

extern "C" {

// onfluid: the forces on the fluid alone (particulate_list_event_kernel <ONFLUID>): `force' changes, and `mass'
// where the list holds a GfsForceAddedMass
static int particulate_event (gfship_particles * pl, const PartArgs & P, const gfship_sim_view & v,
			      bool onfluid = false)
{
  gfship_domain * dom = pl->dom;
  ParticulateFieldArgs A;
  const bool rho = v.alpha_cell >= 0, mu = v.mu >= 0;
  A.alpha_cell = rho ? dom->fields[v.alpha_cell].lev[dom->depth] : nullptr;
  A.mu_cell = mu ? dom->fields[v.mu].lev[dom->depth] : nullptr;
  A.P = P;
  particulate_force_args (pl, A);
  for (int c = 0; c < 3; c++)
    A.uold[c] = c < dom->dim && pl->uold[c] >= 0 ? dom->fields[pl->uold[c]].lev[dom->depth] : nullptr;
  A.viscosity = v.visc;
  int block = 256, grid = (pl->n + block - 1)/block;
  int r = particulate_coefficients (pl, A, dom->stream, gfship_sim_time (pl->sim), [&] {
    with_bools ([&] (auto D3, auto RHO, auto MU) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      constexpr bool R = decltype (RHO)::value, M = decltype (MU)::value;
      hipLaunchKernelGGL ((particulate_coeff_inputs_kernel<DIM, R, M>), dim3 (grid), dim3 (block), 0, dom->stream,
			  static_cast<const ParticulateArgsOf<R, M> &> (A), dom->depth);
    }, dom->dim == 3, rho, mu);
  });
  if (r) return r;
  if (onfluid) {
    with_bools ([&] (auto D3, auto RHO, auto MU) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      constexpr bool R = decltype (RHO)::value, M = decltype (MU)::value;
      hipLaunchKernelGGL ((particulate_list_event_kernel<DIM, R, M, true>), dim3 (grid), dim3 (block), 0,
			  dom->stream, static_cast<const ParticulateArgsOf<R, M> &> (A), dom->depth);
    }, dom->dim == 3, rho, mu);
    GFSHIP_HIP (hipGetLastError ());
    return GFSHIP_OK;
  }
  with_bools ([&] (auto D3, auto RHO, auto MU) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    constexpr bool R = decltype (RHO)::value, M = decltype (MU)::value;
    hipLaunchKernelGGL ((particulate_list_event_kernel<DIM, R, M>), dim3 (grid), dim3 (block), 0, dom->stream,
			static_cast<const ParticulateArgsOf<R, M> &> (A), dom->depth);
  }, dom->dim == 3, rho, mu);
  GFSHIP_HIP (hipGetLastError ());
  // the velocity of this step for the inertial force of the next one (:1003-1012: only for
  // GfsForceInertial objects)
  for (int f = 0; f < pl->nforces; f++)
    if (pl->forces[f] == GFSHIP_FORCE_INERTIAL)
      return store_previous_vel (pl);
  return GFSHIP_OK;
}

int gfship_particles_set_particulate (gfship_particles * pl, const double * vel, const double * mass,
				      const double * volume)
{
  GFSHIP_CHECK (pl && vel && mass && volume, GFSHIP_EINVAL, "null argument");
  GFSHIP_NO_TREE_LIST (pl, "gfship_particles_set_particulate");
  GFSHIP_CHECK (!pl->particulate, GFSHIP_EINVAL, "the list already holds particulates");
  GFSHIP_CHECK (pl->n == pl->np0, GFSHIP_EINVAL, "set the particulate state before the first migration");
  return gfship::particulate_alloc (pl, vel, mass, volume);
}

} // extern "C"

int gfship::particulate_alloc (gfship_particles * pl, const double * vel, const double * mass, const double * volume)
{
  size_t m = (size_t) pl->cap, np = (size_t) pl->n;
  std::vector<double> tmp (m, 0.);
  for (int c = 0; c < 3; c++) {
    GFSHIP_HIP (hipMalloc ((void **) &pl->vel[c], m*sizeof (double)));
    GFSHIP_HIP (hipMalloc ((void **) &pl->force[c], m*sizeof (double)));
    for (size_t q = 0; q < np; q++) tmp[q] = vel[3*q + c];
    GFSHIP_HIP (hipMemcpy (pl->vel[c], tmp.data (), m*sizeof (double), hipMemcpyHostToDevice));
    GFSHIP_HIP (hipMemset (pl->force[c], 0, m*sizeof (double)));
  }
  GFSHIP_HIP (hipMalloc ((void **) &pl->mass, m*sizeof (double)));
  GFSHIP_HIP (hipMalloc ((void **) &pl->volume, m*sizeof (double)));
  GFSHIP_HIP (hipMalloc ((void **) &pl->dia, m*sizeof (double)));
  if (np) {
    GFSHIP_HIP (hipMemcpy (pl->mass, mass, np*sizeof (double), hipMemcpyHostToDevice));
    GFSHIP_HIP (hipMemcpy (pl->volume, volume, np*sizeof (double), hipMemcpyHostToDevice));
    /* diameter of the sphere of that volume, on the host with the reference's expression
       (compute_drag_force, :552) */
    for (size_t q = 0; q < np; q++)
      tmp[q] = 2.*pow (3.0*volume[q]/4.0/M_PI, 1./3.);
    GFSHIP_HIP (hipMemcpy (pl->dia, tmp.data (), np*sizeof (double), hipMemcpyHostToDevice));
  }
  /* rb of distance_normalization (:2091), the host's pow like the diameter */
  GFSHIP_HIP (hipMalloc ((void **) &pl->rb, m*sizeof (double)));
  if (np) {
    for (size_t q = 0; q < np; q++)
      tmp[q] = pow (3.*volume[q]/(4.*M_PI), 1./3.);
    GFSHIP_HIP (hipMemcpy (pl->rb, tmp.data (), np*sizeof (double), hipMemcpyHostToDevice));
  }
  pl->particulate = true;
  return GFSHIP_OK;
}

extern "C" {

int gfship_particles_set_forces (gfship_particles * pl, int nforces, const int * kinds,
				 const double gravity[3])
{
  GFSHIP_CHECK (pl && (nforces == 0 || kinds), GFSHIP_EINVAL, "null argument");
  GFSHIP_NO_TREE_TRACER_LIST (pl, "gfship_particles_set_forces");
  GFSHIP_CHECK (pl->particulate, GFSHIP_EINVAL, "forces act on particulates (gfship_particles_set_particulate)");
  GFSHIP_CHECK (nforces >= 0 && nforces <= 8, GFSHIP_EINVAL, "at most 8 forces");
  if (nforces > 0 && !pl->tree) {
    int r = particulate_fluid_check (gfship_sim_view_get (pl->sim));
    if (r) return r;
  }
  bool coeff = false;
  for (int f = 0; f < nforces; f++)
    GFSHIP_CHECK (kinds[f] >= GFSHIP_FORCE_INERTIAL && kinds[f] <= GFSHIP_FORCE_BUOY, GFSHIP_EINVAL,
		  "unknown force");
  /* a new list of forces: the compiled GfsFunction of a slot belonged to the force that sat there
     (gfship_particles_set_force_coefficient comes after this call) */
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  for (int f = 0; f < 8; f++) {
    gfship::rtc_free (pl->coef_fn[f]);
    pl->coef_fn[f] = nullptr;
    if (pl->coef[f]) (void) hipFree (pl->coef[f]);
    pl->coef[f] = nullptr;
  }
  for (int f = 0; f < nforces; f++) {
    pl->forces[f] = kinds[f];
    if (kinds[f] != GFSHIP_FORCE_BUOY) coeff = true;
  }
  pl->nforces = nforces;
  for (int c = 0; c < 3; c++) pl->gravity[c] = gravity ? gravity[c] : 0.;
  /* every GfsForceCoeff creates Un, Vn, Wn and stores the velocity when it is read (:181-187) */
  if (pl->tree)      /* Un, Vn, Wn are variables of the tree (GFSHIP_TREE_UPREV ...) */
    return coeff ? gfship::tree_previous_vel (pl->tree) : GFSHIP_OK;
  if (coeff && pl->uold[0] < 0) {
    for (int c = 0; c < pl->dom->dim; c++) {
      pl->uold[c] = gfship_field_alloc (pl->dom, -1);
      GFSHIP_CHECK (pl->uold[c] >= 0, GFSHIP_ENOMEM, "no field for the previous velocity");
    }
    return store_previous_vel (pl);
  }
  return GFSHIP_OK;
}

int gfship_particles_set_force_coefficient (gfship_particles * pl, int force, const char * function)
{
  GFSHIP_CHECK (pl && function, GFSHIP_EINVAL, "null argument");
  GFSHIP_NO_TREE_TRACER_LIST (pl, "gfship_particles_set_force_coefficient");
  GFSHIP_CHECK (force >= 0 && force < pl->nforces, GFSHIP_EINVAL,
		"force %d: the list has %d forces (gfship_particles_set_forces)", force, pl->nforces);
  GFSHIP_CHECK (pl->forces[force] == GFSHIP_FORCE_ADDEDMASS || pl->forces[force] == GFSHIP_FORCE_LIFT ||
		pl->forces[force] == GFSHIP_FORCE_DRAG, GFSHIP_EINVAL,
		"only GfsForceAddedMass, GfsForceLift and GfsForceDrag read a coefficient");
  gfship::RtcKernel * k = nullptr;
  int r = pl->tree ? gfship::rtc_compile_coefficient_on (gfship::tree_device (pl->tree), function, &k) :
    gfship::rtc_compile_coefficient (pl->dom, function, &k);
  if (r) return r;
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  gfship::rtc_free (pl->coef_fn[force]);
  pl->coef_fn[force] = k;
  return GFSHIP_OK;
}

int gfship_particles_download_particulate (gfship_particles * pl, double * vel, double * mass,
					   double * force)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_TRACER_LIST (pl, "gfship_particles_download_particulate");
  GFSHIP_CHECK (pl->particulate, GFSHIP_EINVAL, "not a list of particulates");
  if (pl->n == 0) return 0;
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  size_t m = pl->n, m0 = pl->n;      /* creation slots = slots in use */
  std::vector<unsigned> orig (m), where (m);
  std::vector<unsigned char> al (m);
  std::vector<double> v[3], f[3], ms (m0);
  GFSHIP_HIP (hipMemcpy (orig.data (), pl->orig, m*sizeof (unsigned), hipMemcpyDeviceToHost));
  GFSHIP_HIP (hipMemcpy (al.data (), pl->alive, m, hipMemcpyDeviceToHost));
  for (int c = 0; c < 3; c++) {
    v[c].resize (m0); f[c].resize (m0);
    GFSHIP_HIP (hipMemcpy (v[c].data (), pl->vel[c], m0*sizeof (double), hipMemcpyDeviceToHost));
    GFSHIP_HIP (hipMemcpy (f[c].data (), pl->force[c], m0*sizeof (double), hipMemcpyDeviceToHost));
  }
  GFSHIP_HIP (hipMemcpy (ms.data (), pl->mass, m0*sizeof (double), hipMemcpyDeviceToHost));
  for (size_t q = 0; q < m; q++)
    where[orig[q]] = (unsigned) q;
  int k = 0;
  for (size_t o = 0; o < m; o++)
    if (al[where[o]] == 1) {
      for (int c = 0; c < 3; c++) {
	if (vel) vel[3*(size_t) k + c] = v[c][o];
	if (force) force[3*(size_t) k + c] = f[c][o];
      }
      if (mass) mass[k] = ms[o];
      k++;
    }
  return k;
}

int gfship_particles_download_volume (gfship_particles * pl, double * volume)
{
  GFSHIP_CHECK (pl && volume, GFSHIP_EINVAL, "null argument");
  GFSHIP_NO_TREE_TRACER_LIST (pl, "gfship_particles_download_volume");
  GFSHIP_CHECK (pl->particulate, GFSHIP_EINVAL, "not a list of particulates");
  if (pl->n == 0) return 0;
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  size_t m = pl->n;
  std::vector<unsigned> orig (m), where (m);
  std::vector<unsigned char> al (m);
  std::vector<double> vol (m);
  GFSHIP_HIP (hipMemcpy (orig.data (), pl->orig, m*sizeof (unsigned), hipMemcpyDeviceToHost));
  GFSHIP_HIP (hipMemcpy (al.data (), pl->alive, m, hipMemcpyDeviceToHost));
  GFSHIP_HIP (hipMemcpy (vol.data (), pl->volume, m*sizeof (double), hipMemcpyDeviceToHost));
  for (size_t q = 0; q < m; q++)
    where[orig[q]] = (unsigned) q;
  int k = 0;
  for (size_t o = 0; o < m; o++)
    if (al[where[o]] == 1)
      volume[k++] = vol[o];
  return k;
}

int gfship_particle_list_event (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  if (pl->tree) {
    if (pl->n == 0) return GFSHIP_OK;
    if (pl->sort_every > 0 &&
	(pl->events_since_sort < 0 || pl->events_since_sort >= pl->sort_every)) {
      int r = gfship_particles_sort (pl);
      if (r) return r;
    }
    if (pl->events_since_sort >= 0)
      pl->events_since_sort++;
    /* gfs_particulate_event without forces is the event of GfsParticle (:776-778) */
    if (pl->particulate && pl->nforces > 0)
      return gfship::tree_particulate_list_event (pl);
    return gfship::tree_particle_list_event (pl);
  }
  const bool migrates = pl->migrate != nullptr || (pl->dom->comm && pl->dom->has_external);
  if (pl->n == 0 && !migrates) return GFSHIP_OK;
  if (pl->sort_every > 0 &&
      (pl->events_since_sort < 0 || pl->events_since_sort >= pl->sort_every)) {
    int r = gfship_particles_sort (pl);
    if (r) return r;
  }
  if (pl->events_since_sort >= 0)
    pl->events_since_sort++;
  gfship_sim_view v = gfship_sim_view_get (pl->sim);
  gfship_domain * dom = pl->dom;
  PartArgs A;
  A.L = dom->lay[dom->depth];
  for (int d = 0; d < 6; d++) A.side[d] = dom->side[d];
  A.n = pl->n;
  for (int c = 0; c < 3; c++) {
    A.pos[c] = pl->pos[c];
    A.old[c] = pl->old[c];
    A.u[c] = c < dom->dim ? dom->fields[v.u[c]].lev[dom->depth] : nullptr;
  }
  A.alive = pl->alive;
  A.dt = v.dt;
  A.count = pl->d_count;
  A.migrate = migrates;
  int block = 256, grid = (pl->n + block - 1)/block;
  if (pl->n > 0 && pl->particulate && pl->nforces > 0) {
    int r = particulate_fluid_check (v);
    if (r) return r;
    r = particulate_event (pl, A, v);
    if (r) return r;
    return migrates ? particles_migrate (pl) : GFSHIP_OK;
  }
  if (pl->n > 0) {
    if (dom->dim == 3)
      hipLaunchKernelGGL (particle_list_event_kernel<3>, dim3 (grid), dim3 (block), 0, dom->stream,
			  A, dom->depth);
    else
      hipLaunchKernelGGL (particle_list_event_kernel<2>, dim3 (grid), dim3 (block), 0, dom->stream,
			  A, dom->depth);
    GFSHIP_HIP (hipGetLastError ());
  }
  if (migrates)
    return particles_migrate (pl);
  return GFSHIP_OK;
}

// the forces of source_particulate_event (modules/particulatecommon.c:2199-2206)
int gfship_particles_forces_on_fluid (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_NO_TREE_LIST (pl, "gfship_particles_forces_on_fluid");
  GFSHIP_CHECK (pl->particulate, GFSHIP_EUNSUPPORTED,
		"the forces on the fluid are those of particulates (gfship_particles_set_particulate)");
  gfship_sim_view v = gfship_sim_view_get (pl->sim);
  gfship_domain * dom = pl->dom;
  GFSHIP_CHECK (!dom->has_external, GFSHIP_EUNSUPPORTED,
		"GfsSourceParticulate on a box with GfsBoundaryMpi sides is not supported");
  int r = particulate_fluid_check (v);
  if (r) return r;
  if (pl->n == 0) return GFSHIP_OK;
  PartArgs A;
  A.L = dom->lay[dom->depth];
  for (int d = 0; d < 6; d++) A.side[d] = dom->side[d];
  A.n = pl->n;
  for (int c = 0; c < 3; c++) {
    A.pos[c] = pl->pos[c];
    A.old[c] = pl->old[c];
    A.u[c] = c < dom->dim ? dom->fields[v.u[c]].lev[dom->depth] : nullptr;
  }
  A.alive = pl->alive;
  A.dt = v.dt;
  A.count = pl->d_count;
  A.migrate = 0;
  return particulate_event (pl, A, v, true);
}

int gfship_particles_count (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  if (pl->n == 0) return 0;
  hipStream_t stream = pl->stream;
  GFSHIP_HIP (hipMemsetAsync (pl->d_count, 0, sizeof (unsigned), stream));
  int block = 256, grid = (pl->n + block - 1)/block;
  hipLaunchKernelGGL (count_alive_kernel, dim3 (grid), dim3 (block), 0, stream,
		      pl->alive, pl->n, pl->d_count);
  unsigned c = 0;
  GFSHIP_HIP (hipMemcpyAsync (&c, pl->d_count, sizeof (unsigned), hipMemcpyDeviceToHost, stream));
  GFSHIP_HIP (hipStreamSynchronize (stream));
  return (int) c;
}

// the survivors in creation order (the reference's list order), whatever the storage order: their
// positions (src = pl->pos) or old positions (src = pl->old), and their ids where id is given
static int particles_download (gfship_particles * pl, double * const src[3], double * pos, unsigned * id)
{
  if (pl->n == 0) return 0;
  GFSHIP_HIP (hipStreamSynchronize (pl->stream));
  size_t m = pl->n;
  std::vector<double> x (m), y (m), z (m);
  std::vector<unsigned> ids (m), orig (m), where (m);
  std::vector<unsigned char> al (m);
  GFSHIP_HIP (hipMemcpy (orig.data (), pl->orig, m*sizeof (unsigned), hipMemcpyDeviceToHost));
  GFSHIP_HIP (hipMemcpy (x.data (), src[0], m*sizeof (double), hipMemcpyDeviceToHost));
  GFSHIP_HIP (hipMemcpy (y.data (), src[1], m*sizeof (double), hipMemcpyDeviceToHost));
  GFSHIP_HIP (hipMemcpy (z.data (), src[2], m*sizeof (double), hipMemcpyDeviceToHost));
  GFSHIP_HIP (hipMemcpy (ids.data (), pl->id, m*sizeof (unsigned), hipMemcpyDeviceToHost));
  GFSHIP_HIP (hipMemcpy (al.data (), pl->alive, m, hipMemcpyDeviceToHost));
  for (size_t q = 0; q < m; q++)
    where[orig[q]] = (unsigned) q;
  int k = 0;
  for (size_t o = 0; o < m; o++) {
    size_t q = where[o];
    if (al[q] == 1) {
      pos[3*(size_t) k] = x[q]; pos[3*(size_t) k + 1] = y[q];
      pos[3*(size_t) k + 2] = pl->dim == 3 ? z[q] : 0.;
      if (id) id[k] = ids[q];
      k++;
    }
  }
  return k;
}

int gfship_particles_download (gfship_particles * pl, double * pos, unsigned * id)
{
  GFSHIP_CHECK (pl && pos && id, GFSHIP_EINVAL, "null argument");
  return particles_download (pl, pl->pos, pos, id);
}

int gfship_particles_download_old (gfship_particles * pl, double * old)
{
  GFSHIP_CHECK (pl && old, GFSHIP_EINVAL, "null argument");
  return particles_download (pl, pl->old, old, nullptr);
}

} // extern "C"

int gfship::BoxMesh::source_gather (gfship_particulate_source * s) const
{
  SourceGatherArgs A;
  A.L = L;
  A.depth = dom->depth;
  A.n = pl->n;
  for (int c = 0; c < 3; c++) {
    A.pos[c] = pl->pos[c];
    A.u[c] = c < dom->dim ? dom->fields[v.u[c]].lev[dom->depth] : nullptr;
    A.vel[c] = pl->vel[c];
    A.urel[c] = s->purel[c];
  }
  A.alive = pl->alive; A.orig = pl->orig; A.volume = pl->volume;
  A.cell = s->cell; A.rad = s->prad;
  const int block = 256, grid = (pl->n + block - 1)/block;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (particulate_source_gather_kernel<DIM>, dim3 (grid), dim3 (block), 0, dom->stream, A);
  }, dom->dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

int gfship::BoxMesh::feed_gather (int base, int np, const double * cand, unsigned * cell) const
{
  FeedGatherArgs A;
  A.L = L;
  A.depth = dom->depth;
  A.np = np; A.base = base;
  A.cand = cand;
  for (int c = 0; c < 3; c++) {
    A.u[c] = c < dom->dim ? dom->fields[v.u[c]].lev[dom->depth] : nullptr;
    A.pos[c] = pl->pos[c]; A.old[c] = pl->old[c];
    A.vel[c] = pl->vel[c]; A.force[c] = pl->force[c];
  }
  A.orig = pl->orig; A.cell = cell;
  const int block = 256, grid = (np + block - 1)/block;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (feed_gather_kernel<DIM>, dim3 (grid), dim3 (block), 0, dom->stream, A);
  }, dom->dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}
