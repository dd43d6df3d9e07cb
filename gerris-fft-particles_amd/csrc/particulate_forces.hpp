// particulate_forces.hpp -- the forces on a GfsParticulate and its event (modules/particulatecommon.c:91-842), once,
// for the lists of a uniform box (particles.hip) and of a refined tree (tree_particles.hip).
//
//   here                 | reference
//   ---------------------+---------------------------------------------------------------------------------
//   force_needs          | what the forces of a list read of the fluid (evaluated once per particle: the
//                        | reference re-evaluates the same expressions per force, same bits)
//   inertial_force       | compute_inertial_force, :285-336
//   vorticity_vector     | vorticity_vector, :146-168
//   particulate_forces   | compute_forces (:738-752) / compute_forces_onfluid (:753-765) over the list, with
//                        | compute_addedmass_force (:363-427), compute_lift_force (:455-524), compute_drag_force
//                        | (:527-588), compute_buoyancy_force (:619-653)
//   particulate_advance  | the half-step, kick and half-step of gfs_particulate_event, :828-837
//   coefficient_inputs   | the variables a GfsFunction of a GfsForceCoeff sees, :364-384, 462-485, 545-573
//
// Nothing here knows a layout, a tree or a cell search: a kernel locates the particle, gathers what the forces
// read of the fluid and passes values (the fluid velocity at the particle, the density of the fluid, the size
// of the cell) or sources that are read where they are used, in the reference's order:
//   grad (c, c2)   gfs_center_gradient (cell, c2, u[c]) (src/fluid.c:434-475), not yet divided by the size of the
//                  cell: Du/Dt divides the product with u[c2], vorticity_vector the difference;
//   ucell (c2)     u[c2] at the cell;
//   fveln (c)      Un, Vn, Wn interpolated at the particle;
//   viscosity ()   the viscosity of the fluid: ValueOf { the value of the cell } or ListViscosity { A }, the
//                  constant of the launch, which is read at its use.
// Every expression keeps the reference's operand order (the library is built with -ffp-contract=off); pow (Re, 0.5)
// of the drag law is evaluated as sqrt (Re) (correctly rounded; glibc's pow is within 0.52 ulp of it).
//
// Plain C++: a host compiler reads it with __device__ and __forceinline__ defined away
// (tests/test_particulate_forces_cpu.py).
#pragma once
#include "gfship.h"
#include <cmath>

namespace gfship {

enum { FORCE_INERTIAL = GFSHIP_FORCE_INERTIAL, FORCE_ADDEDMASS = GFSHIP_FORCE_ADDEDMASS,
       FORCE_LIFT = GFSHIP_FORCE_LIFT, FORCE_DRAG = GFSHIP_FORCE_DRAG, FORCE_BUOY = GFSHIP_FORCE_BUOY };

// the state of the particulates of a list (indexed by the creation slot o) and its forces: what ParticulateArgs
// (particles.hip) and TreeParticulateArgs (tree_particles.hip) share, filled by particulate_force_args
// (particles.hip)
struct ParticleForceArgs {
  const unsigned * orig;
  double * vel[3], * force[3], * mass;
  const double * volume, * dia;
  const double * uold[3];      // Un, Vn, Wn
  int nforces, forces[8];
  double gravity[3], viscosity;
  const double * coef[8];      // values of the GfsFunction of force f per slot; nullptr: the default
  double * cin[6];             // Rep, Urelp, Vrelp, Wrelp, Pdia per slot (coefficient inputs); [5]: the Rep of
                               // GfsForceDrag in 2-D (two-component norm, particulatecommon.c:549-556)
};

struct ValueOf { double v; __device__ __forceinline__ double operator() () const { return v; } };
struct ListViscosity {
  const ParticleForceArgs & A;
  __device__ __forceinline__ double operator() () const { return A.viscosity; }
};
// three values the caller holds
struct Value3 { const double * v; __device__ __forceinline__ double operator() (int c) const { return v[c]; } };

// what the forces of the list read of the fluid.  ONFLUID: compute_forces_onfluid skips GfsForceBuoy (:756).
// (filled through a reference: returned by value, the event kernels came out 20 to 80 instructions longer,
// DESIGN.md 11.34)
struct ForceNeeds { bool fvel, dudt, grad; };

template <bool ONFLUID>
__device__ __forceinline__ void force_needs (const ParticleForceArgs & A, ForceNeeds & need)
{
  need.fvel = need.dudt = need.grad = false;
  for (int f = 0; f < A.nforces; f++) {
    if (ONFLUID && A.forces[f] == FORCE_BUOY)
      continue;
    need.fvel = need.fvel || A.forces[f] != FORCE_BUOY;
    need.dudt = need.dudt || A.forces[f] == FORCE_INERTIAL || A.forces[f] == FORCE_ADDEDMASS;
    need.grad = need.grad || A.forces[f] == FORCE_INERTIAL || A.forces[f] == FORCE_ADDEDMASS || A.forces[f] == FORCE_LIFT;
  }
}

// compute_inertial_force, :285-336
// (fvel: the fluid velocity interpolated at the particle, computed once per particle and shared with the lift and
// drag forces: the same gfs_interpolate of the same fields)
template <int DIM, class Un, class Grad, class U>
__device__ __forceinline__ void inertial_force (double fluid_rho, double dt, double size, const double fvel[3],
						const Un & fveln, const Grad & grad, const U & ucell, double force[3])
{
  force[0] = force[1] = force[2] = 0.;
  if (!(dt > 0.))
    return;
  for (int c = 0; c < DIM; c++) {
    const double fluid_vel = fvel[c];
    const double fluid_veln = fveln (c);
    force[c] = fluid_rho*(fluid_vel - fluid_veln)/dt;
  }
  for (int c = 0; c < DIM; c++)
    for (int c2 = 0; c2 < DIM; c2++)
      force[c] += fluid_rho*grad (c, c2)*ucell (c2)/size;
}

// vorticity_vector, :146-168
template <int DIM, class Grad>
__device__ __forceinline__ void vorticity_vector (const Grad & grad, double size, double vort[3])
{
  if constexpr (DIM == 2) {
    vort[0] = 0.; vort[1] = 0.;
    vort[2] = (grad (1, 0) - grad (0, 1))/size;
  }
  else {
    vort[0] = (grad (2, 1) - grad (1, 2))/size;
    vort[1] = (grad (0, 2) - grad (2, 0))/size;
    vort[2] = (grad (1, 0) - grad (0, 1))/size;
  }
}

// the forces of the list on the particle of slot q, creation slot o, in application order: pf, and what
// compute_addedmass_force adds to the mass (:391, in compute_forces_onfluid too).  vel, mass, volume: of the
// particle at the start of the event; fvel, dudt: zero where force_needs does not ask for them
template <int DIM, bool ONFLUID, class Visc, class Grad>
__device__ __forceinline__ void particulate_forces (const ParticleForceArgs & A, int q, unsigned o, double fluid_rho,
						    const Visc & viscosity, double size, const Grad & grad,
						    const double fvel[3], const double dudt[3], const double vel[3],
						    double volume, double & mass, double pf[3])
{
  for (int f = 0; f < A.nforces; f++) {
    double force[3] = { 0., 0., 0. };
    if (ONFLUID && A.forces[f] == FORCE_BUOY)      /* :756 */
      continue;
    switch (A.forces[f]) {
    case FORCE_INERTIAL:
      force[0] = dudt[0]; force[1] = dudt[1]; force[2] = dudt[2];
      break;
    case FORCE_ADDEDMASS: {     // compute_addedmass_force, :363-427
      force[0] = dudt[0]; force[1] = dudt[1]; force[2] = dudt[2];
      const double cm = A.coef[f] ? A.coef[f][q] : 0.5;
      for (int c = 0; c < DIM; c++)
	force[c] *= cm;
      mass += fluid_rho*volume*cm;      /* :391, in compute_forces_onfluid too */
      break;
    }
    case FORCE_LIFT: {          // compute_lift_force, :455-524
      double rel[3] = { 0., 0., 0. }, vort[3];
      for (int c = 0; c < DIM; c++)
	rel[c] = fvel[c] - vel[c];
      vorticity_vector<DIM> (grad, size, vort);
      const double cl = A.coef[f] ? A.coef[f][q] : 0.5;
      if (DIM == 2) {
	force[0] = fluid_rho*cl*rel[1]*vort[2];
	force[1] = -fluid_rho*cl*rel[0]*vort[2];
      }
      else {
	force[0] = fluid_rho*cl*(rel[1]*vort[2] - rel[2]*vort[1]);
	force[1] = fluid_rho*cl*(rel[2]*vort[0] - rel[0]*vort[2]);
	force[2] = fluid_rho*cl*(rel[0]*vort[1] - rel[1]*vort[0]);
      }
      break;
    }
    case FORCE_DRAG: {          // compute_drag_force, :527-588
      double rel[3] = { 0., 0., 0. };
      for (int c = 0; c < DIM; c++)
	rel[c] = fvel[c] - vel[c];
      const double dia = A.dia[o];
      const double norm = DIM == 3 ? sqrt (rel[0]*rel[0] + rel[1]*rel[1] + rel[2]*rel[2]) :
	sqrt (rel[0]*rel[0] + rel[1]*rel[1]);
      if (viscosity () == 0)      /* :561-562: no drag in a fluid, or a cell, without viscosity */
	break;
      const double Re = norm*dia*fluid_rho/viscosity ();
      double cd;
      if (A.coef[f])
	cd = A.coef[f][q];
      else if (Re < 1e-8)
	break;
      else if (Re < 50.0)
	cd = 16.*(1. + 0.15*sqrt (Re))/Re;
      else
	cd = 48.*(1. - 2.21/sqrt (Re))/Re;
      for (int c = 0; c < DIM; c++)
	force[c] += 3./(4.*dia)*cd*norm*rel[c]*fluid_rho;
      break;
    }
    case FORCE_BUOY:            // compute_buoyancy_force, :619-653
      for (int c = 0; c < DIM; c++)
	force[c] += (mass/volume - fluid_rho)*A.gravity[c];
      break;
    }
    // compute_forces, :738-752
    for (int c = 0; c < DIM; c++)
      pf[c] = force[c]*volume + pf[c];
    if (DIM == 2) pf[2] = 0.;
  }
}

// gfs_particulate_event, :828-837
template <int DIM>
__device__ __forceinline__ void particulate_advance (double p[3], double vel[3], const double pf[3], double dt,
						     double mass)
{
  for (int c = 0; c < DIM; c++) {
    p[c] += vel[c]*dt/2.;
    vel[c] += pf[c]*dt/mass;
    p[c] += vel[c]*dt/2.;
  }
}

// the variables a GfsFunction of a GfsForceCoeff sees (:364-384,462-485,545-573), into A.cin[][q]: the particle
// Reynolds number from the relative velocity (all three components of the FttVectors), the sphere diameter and the
// viscosity (0.001 where the reference substitutes it for a zero viscosity in the added-mass and lift
// coefficients; the drag is then zero whatever its coefficient)
template <int DIM, class Visc>
__device__ __forceinline__ void coefficient_inputs (const ParticleForceArgs & A, int q, unsigned o, const double fvel[3],
						    double fluid_rho, const Visc & cell_viscosity)
{
  double rel[3] = { 0. - A.vel[0][o], 0. - A.vel[1][o], 0. - A.vel[2][o] };
  for (int c = 0; c < DIM; c++)
    rel[c] = fvel[c] - A.vel[c][o];
  const double norm = sqrt (rel[0]*rel[0] + rel[1]*rel[1] + rel[2]*rel[2]);
  const double dia = A.dia[o];
  const double cell_visc = cell_viscosity ();
  const double viscosity = cell_visc == 0 ? 0.001 : cell_visc;      /* :372-375, 461-464 */
  A.cin[0][q] = norm*dia*fluid_rho/viscosity;
  A.cin[1][q] = rel[0]; A.cin[2][q] = rel[1]; A.cin[3][q] = rel[2];
  A.cin[4][q] = dia;
  if (DIM == 2)      /* compute_drag_force takes the norm of the two components in 2-D (:549-556) */
    A.cin[5][q] = sqrt (rel[0]*rel[0] + rel[1]*rel[1])*dia*fluid_rho/viscosity;
}

} // namespace gfship
