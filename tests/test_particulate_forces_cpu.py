"""The one definition of the particulate forces (csrc/particulate_forces.hpp), on the restatement of the reference
(tests/forces_reference.py, its `sqrt' variant), without a GPU.

The header is plain C++ once __device__ and __forceinline__ are defined away, so a small program that does per
record what the event kernels do per particle -- force_needs, inertial_force, particulate_forces,
particulate_advance, coefficient_inputs -- is built with the host compiler.  The operands of a record are what the
restatement's own Box.interpolate, center_gradient, Box.value, Sim.fluid_rho and Sim.viscosity_of_u return for the
particle; given those, the program must return the velocity, force, mass and new position of particulate_event,
the force and mass of forces_on_fluid, and the variables the coefficient functions were called with, bit for bit.
The particles are those of tests/forces_cases.py on a small box (2-D depth 3, 3-D depth 2); the drag-branch
particles of forces_cases.branch_particles reach every branch of the drag law, which is asserted from the branch
list of the restatement."""
import functools
import os
import subprocess

import numpy as np
import pytest

import forces_cases as K
import forces_reference as F
import sampler_cases as SK
from conftest import ROOT

CSRC = os.path.join(ROOT, "gerris-fft-particles_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

PROGRAM = r"""
#include "particulate_forces.hpp"
#include <cstdio>
#include <vector>
using namespace gfship;
// header: dim mode np nforces forces[8] hascoef[8] gravity[3] viscosity cellvisc dt
// record: pos[3] vel[3] mass volume dia fvel[3] fveln[3] G[9] ucell[3] rho visc size coef[8]
// output: vel[3] force[3] mass pos[3] cin[6] needs (fvel + 2 dudt + 4 grad)
enum { NH = 26, NR = 38, NO = 17 };
struct Grad9 { const double * g; double operator() (int c, int c2) const { return g[3*c + c2]; } };

template <int DIM, bool ONFLUID, bool CELLVISC>
static void run (const double * h, const double * rec, int np, double * out)
{
  std::vector<double> col[3 + 3 + 3 + 8 + 6];
  for (auto & c : col) c.assign (np, 0.);
  std::vector<unsigned> orig (np);
  ParticleForceArgs A;
  A.orig = orig.data ();
  for (int c = 0; c < 3; c++) { A.vel[c] = col[c].data (); A.force[c] = col[3 + c].data (); A.uold[c] = nullptr; }
  A.mass = col[6].data (); A.volume = col[7].data (); A.dia = col[8].data ();
  A.nforces = (int) h[3];
  for (int f = 0; f < 8; f++) { A.forces[f] = (int) h[4 + f]; A.coef[f] = h[12 + f] != 0. ? col[9 + f].data () : nullptr; }
  for (int c = 0; c < 3; c++) A.gravity[c] = h[20 + c];
  A.viscosity = h[23];
  for (int k = 0; k < 6; k++) A.cin[k] = col[17 + k].data ();
  const double dt = h[25];
  for (int q = 0; q < np; q++) {
    const double * r = rec + (size_t) NR*q;
    orig[q] = q;
    for (int c = 0; c < 3; c++) col[c][q] = r[3 + c];
    col[6][q] = r[6]; col[7][q] = r[7]; col[8][q] = r[8];
    for (int f = 0; f < 8; f++) col[9 + f][q] = r[30 + f];
  }
  for (int q = 0; q < np; q++) {
    const double * r = rec + (size_t) NR*q;
    const unsigned o = orig[q];
    const double fluid_rho = r[27], size = r[29];
    double p[3] = { r[0], r[1], r[2] };
    double vel[3] = { A.vel[0][o], A.vel[1][o], A.vel[2][o] };
    double mass = A.mass[o];
    const double volume = A.volume[o];
    double pf[3] = { 0., 0., 0. };
    ForceNeeds need;
    force_needs<ONFLUID> (A, need);
    double fvel[3] = { 0., 0., 0. }, dudt[3] = { 0., 0., 0. };
    if (need.fvel)
      for (int c = 0; c < DIM; c++) fvel[c] = r[9 + c];
    const Grad9 grad = { r + 15 };
    if (need.dudt)
      inertial_force<DIM> (fluid_rho, dt, size, fvel, Value3 { r + 12 }, grad, Value3 { r + 24 }, dudt);
    if (CELLVISC) {
      coefficient_inputs<DIM> (A, q, o, r + 9, fluid_rho, ValueOf { r[28] });
      particulate_forces<DIM, ONFLUID> (A, q, o, fluid_rho, ValueOf { r[28] }, size, grad, fvel, dudt, vel, volume, mass, pf);
    }
    else {
      coefficient_inputs<DIM> (A, q, o, r + 9, fluid_rho, ListViscosity { A });
      particulate_forces<DIM, ONFLUID> (A, q, o, fluid_rho, ListViscosity { A }, size, grad, fvel, dudt, vel, volume, mass, pf);
    }
    if (!ONFLUID)
      particulate_advance<DIM> (p, vel, pf, dt, mass);
    double * w = out + (size_t) NO*q;
    for (int c = 0; c < 3; c++) { w[c] = vel[c]; w[3 + c] = pf[c]; w[7 + c] = p[c]; }
    w[6] = mass;
    for (int k = 0; k < 6; k++) w[10 + k] = A.cin[k][q];
    w[16] = (need.fvel ? 1 : 0) + (need.dudt ? 2 : 0) + (need.grad ? 4 : 0);
  }
}

template <int DIM, bool ONFLUID>
static void run_visc (const double * h, const double * rec, int np, double * out)
{
  if (h[24] != 0.) run<DIM, ONFLUID, true> (h, rec, np, out); else run<DIM, ONFLUID, false> (h, rec, np, out);
}

int main (int argc, char ** argv)
{
  if (argc < 3) return 2;
  FILE * in = fopen (argv[1], "rb"), * fo = fopen (argv[2], "wb");
  if (!in || !fo) return 1;
  double h[NH];
  if (fread (h, sizeof (double), NH, in) != NH) return 1;
  const int dim = (int) h[0], onfluid = (int) h[1], np = (int) h[2];
  std::vector<double> rec ((size_t) NR*np), out ((size_t) NO*np);
  if (fread (rec.data (), sizeof (double), rec.size (), in) != rec.size ()) return 1;
  if (dim == 2) { if (onfluid) run_visc<2, true> (h, rec.data (), np, out.data ()); else run_visc<2, false> (h, rec.data (), np, out.data ()); }
  else          { if (onfluid) run_visc<3, true> (h, rec.data (), np, out.data ()); else run_visc<3, false> (h, rec.data (), np, out.data ()); }
  fwrite (out.data (), sizeof (double), out.size (), fo);
  return fclose (fo) != 0;
}
"""

NH, NR, NO = 26, 38, 17
BOXES = {2: 3, 3: 2}                     # dim -> depth
I_, A_, L_, D_, B_ = F.INERTIAL, F.ADDEDMASS, F.LIFT, F.DRAG, F.BUOY
CONSTANT_COEFFICIENTS = {A_: 0.7, L_: 0.3, D_: 1.1}

# id -> (forces, viscosity, coeff, dt factor, particles); viscosity as in forces_cases ("uv": the constant NU, "pow2":
# the constant NU_BRANCHES, "zero", "cell": alpha and the viscosity per cell); coeff: None, "function" (per particle)
# or "constant"
CASES = {
    "inertial": ([I_], "uv", None, 1., "fill"),
    "addedmass": ([A_], "uv", None, 1., "fill"),
    "lift": ([L_], "uv", None, 1., "fill"),
    "drag": ([D_], "uv", None, 1., "fill"),
    "buoy": ([B_], "uv", None, 1., "fill"),
    "canonical": ([I_, A_, L_, D_, B_], "uv", None, 1., "fill"),            # added mass before buoyancy
    "reverse": ([B_, D_, L_, A_, I_], "uv", None, 1., "fill"),              # ... and after: the mass changes in between
    "dt0": ([I_, A_, L_, D_, B_], "uv", None, 0., "fill"),
    "nu0": ([I_, A_, L_, D_, B_], "zero", None, 1., "fill"),
    "nu0-function": ([I_, A_, L_, D_, B_], "zero", "function", 1., "fill"),
    "function": ([I_, A_, L_, D_, B_], "uv", "function", 1., "fill"),
    "function-reverse": ([B_, D_, L_, A_, I_], "uv", "function", 1., "fill"),
    "constant": ([I_, A_, L_, D_, B_], "uv", "constant", 1., "fill"),
    "cell": ([B_, D_, L_, A_, I_], "cell", None, 1., "fill"),               # variable fluid_rho and viscosity
    "cell-function": ([I_, A_, L_, D_, B_], "cell", "function", 1., "fill"),
    "branches": ([D_], "pow2", None, 1., "branches"),
}
DIMS = [2, 3]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("particulate_forces")
    src, exe = str(tmp / "particulate_forces.cpp"), str(tmp / "particulate_forces")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
                    "-D__device__=", "-D__forceinline__=inline", "-I", CSRC, "-I", INCLUDE, src, "-o", exe],
                   check=True, capture_output=True, text=True, timeout=120)

    def run(header, records):
        fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
        with open(fin, "wb") as f:
            np.ascontiguousarray(header, dtype=np.float64).tofile(f)
            np.ascontiguousarray(records, dtype=np.float64).tofile(f)
        subprocess.run([exe, fin, fout], check=True, timeout=60)
        return np.fromfile(fout, dtype=np.float64).reshape(-1, NO)
    return run


def _sim(dim, viscosity, dt_factor, which):
    level = BOXES[dim]
    box = SK.box(dim, level)
    sides = K.SIDES["closed" if dim == 2 else "periodic"]
    zero = which == "branches"
    alpha = None
    const = lambda cell: K.NU
    pow2 = lambda cell: K.NU_BRANCHES
    visc = {"uv": (const,)*3, "pow2": (pow2,)*3, "zero": (None,)*3}.get(viscosity)
    if viscosity == "cell":
        af, mf = (box.field(a) for a in K.cell_fields(dim, level))
        alpha = lambda cell: box.value(cell, af)
        visc = (lambda cell: box.value(cell, mf), None, None)
    sim = F.Sim(box, sides, K.velocity(dim, level, 0, zero=zero), dt_factor*0.05/(1 << level), alpha=alpha,
                viscosity=visc, g=K.GRAVITY, root=F.sqrt_root)
    sim.un = F.store_previous_vel(box, sim.u, sides)
    sim.set_velocity(K.velocity(dim, level, 1, zero=zero))
    return sim


@functools.lru_cache(None)
def _fluid_operands(dim, which):
    """per particle with a cell: (index in the list, cell, fvel, fveln, G, ucell, size), from the restatement"""
    sim = _sim(dim, "uv", 1., which)
    box = sim.box
    pos = (K.branch_particles if which == "branches" else K.particles)(dim, BOXES[dim])[0]
    out = []
    for q, x in enumerate(pos.tolist()):
        cell = box.locate(x)
        if cell is None:
            continue
        fvel = [box.interpolate(cell, x, sim.u[c]) for c in range(dim)] + [0.]*(3 - dim)
        fveln = [box.interpolate(cell, x, sim.un[c]) for c in range(dim)] + [0.]*(3 - dim)
        G = [[F.center_gradient(box, cell, c2, sim.u[c]) if c < dim and c2 < dim else 0. for c2 in range(3)]
             for c in range(3)]
        ucell = [box.value(cell, sim.u[c]) for c in range(dim)] + [0.]*(3 - dim)
        out.append((q, cell, fvel, fveln, G, ucell, box.cell_size(cell)))
    return tuple(out)


def _coefficients(dim, coeff, forces):
    """index in the list -> callable of (Rep, Urelp, Vrelp, Wrelp, Pdia)"""
    if coeff is None:
        return {}
    if coeff == "constant":
        return {f: (lambda *a, v=CONSTANT_COEFFICIENTS[kind]: v) for f, kind in enumerate(forces)
                if kind in CONSTANT_COEFFICIENTS}
    fns = K.coefficient_functions(dim)
    return {f: fns[kind][1] for f, kind in enumerate(forces) if kind in fns}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    assert np.isfinite(want).all(), what
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, "%s: %d values differ, first at %r: %r != %r" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@functools.lru_cache(None)
def _reference(cid, dim):
    """(header without mode, records without coefficients, coefficient callables, event results, on-fluid
    results, inputs per particle of the event and of the on-fluid evaluation, branches)"""
    forces, viscosity, coeff, dt_factor, which = CASES[cid]
    sim = _sim(dim, viscosity, dt_factor, which)
    fns = _coefficients(dim, coeff, forces)
    objects = [F.ForceCoeff(kind, fns.get(f)) for f, kind in enumerate(forces)]
    pos, ids, vel, mass, volume = (K.branch_particles if which == "branches" else K.particles)(dim, BOXES[dim])
    ops = _fluid_operands(dim, which)
    records = np.zeros((len(ops), NR))
    event, onfluid, inputs_event, inputs_onfluid, branches = [], [], [], [], []
    for k, (q, cell, fvel, fveln, G, ucell, size) in enumerate(ops):
        def particle():
            return F.Particulate(pos[q].tolist(), int(ids[q]), vel[q].tolist(), mass[q], volume[q])
        p = particle()
        records[k, 0:3], records[k, 3:6] = p.pos, p.vel
        records[k, 6:9] = p.mass, p.volume, F._diameter(p)
        records[k, 9:12], records[k, 12:15] = fvel, fveln
        records[k, 15:24] = np.array(G).reshape(-1)
        records[k, 24:27] = ucell
        records[k, 27:30] = sim.fluid_rho(cell), sim.viscosity_of_u(cell), size
        ins, br = [], []
        F.particulate_event(sim, p, objects, ins, br)
        event.append(p.vel + p.force + [p.mass] + p.pos)
        inputs_event.append(ins)
        branches.extend(name for name, _ in br)
        p, ins = particle(), []
        F.forces_on_fluid(sim, [p], objects, ins)
        onfluid.append(p.force + [p.mass])
        inputs_onfluid.append(ins)
    cellvisc = viscosity == "cell"
    constant = {"uv": K.NU, "pow2": K.NU_BRANCHES, "zero": 0., "cell": -1.}[viscosity]
    if not cellvisc:
        assert (records[:, 28] == constant).all()
    header = np.zeros(NH)
    header[0], header[2], header[3] = dim, len(ops), len(forces)
    header[4:4 + len(forces)] = forces
    for f in fns:
        header[12 + f] = 1.
    header[20:23] = K.GRAVITY
    header[23], header[24], header[25] = constant, float(cellvisc), sim.dt
    return (header, records, fns, np.array(event), np.array(onfluid), tuple(inputs_event), tuple(inputs_onfluid),
            tuple(branches))


def _run(program, cid, dim, onfluid):
    header, records, fns, *_ = _reference(cid, dim)
    forces = CASES[cid][0]
    header, records = header.copy(), records.copy()
    header[1] = float(onfluid)
    # the coefficient inputs first, as the library does: then the functions on them, then the forces
    cin = program(header, records)[:, 10:16]
    for f, fn in fns.items():
        rep = cin[:, 5] if dim == 2 and forces[f] == D_ else cin[:, 0]
        records[:, 30 + f] = [fn(*a) for a in zip(rep.tolist(), cin[:, 1].tolist(), cin[:, 2].tolist(),
                                                  cin[:, 3].tolist(), cin[:, 4].tolist())]
    return program(header, records)


def _check_inputs(got, inputs, dim, what):
    """what every coefficient function of the restatement was called with is what coefficient_inputs wrote"""
    n = 0
    for k, calls in enumerate(inputs):
        for kind, rep, u, v, w, dia in calls:
            mine = [got[k, 15] if dim == 2 and kind == D_ else got[k, 10], got[k, 11], got[k, 12], got[k, 13],
                    got[k, 14]]
            _check(mine, [rep, u, v, w, dia], (what, "inputs", k, kind))
            n += 1
    return n


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("cid", list(CASES))
def test_event_and_forces_on_fluid_are_the_restatements(program, cid, dim):
    header, records, fns, event, onfluid, inputs_event, inputs_onfluid, _ = _reference(cid, dim)
    forces = CASES[cid][0]
    assert len(records) > (90 if CASES[cid][4] == "branches" else 100)
    if CASES[cid][1] == "cell":
        assert np.unique(records[:, 27]).size > 30 and np.unique(records[:, 28]).size > 30
    got = _run(program, cid, dim, False)
    _check(got[:, 0:3], event[:, 0:3], (cid, dim, "vel"))
    _check(got[:, 3:6], event[:, 3:6], (cid, dim, "force"))
    _check(got[:, 6], event[:, 6], (cid, dim, "mass"))
    _check(got[:, 7:10], event[:, 7:10], (cid, dim, "pos"))
    ncalls = _check_inputs(got, inputs_event, dim, (cid, dim, "event"))
    # force_needs: the fluid velocity for every force but the buoyancy, Du/Dt for the inertial and added-mass
    # forces, the gradients for those two and the lift (the tree kernels read the third flag)
    needs = (any(k != B_ for k in forces) + 2*any(k in (I_, A_) for k in forces)
             + 4*any(k in (I_, A_, L_) for k in forces))
    assert (got[:, 16] == needs).all(), (cid, dim, "needs", needs, np.unique(got[:, 16]))
    got = _run(program, cid, dim, True)
    assert (got[:, 16] == needs).all(), (cid, dim, "needs on fluid", needs, np.unique(got[:, 16]))
    _check(got[:, 3:6], onfluid[:, 0:3], (cid, dim, "force on fluid"))
    _check(got[:, 6], onfluid[:, 3], (cid, dim, "mass after the forces on the fluid"))
    ncalls += _check_inputs(got, inputs_onfluid, dim, (cid, dim, "onfluid"))
    # every coefficient function was called for every particle, twice (the drag's only in a viscous fluid)
    called = [f for f in fns if not (forces[f] == D_ and CASES[cid][1] == "zero")]
    assert ncalls == 2*len(called)*len(records)
    # the cases are not degenerate: the forces differ from particle to particle, and the event moved them
    if forces and CASES[cid][3] > 0.:
        assert np.unique(event[:, 3]).size > 0.5*len(records) or CASES[cid][4] == "branches"
        assert (event[:, 7:7 + dim] != records[:, 0:dim]).any(axis=1).all()
    if A_ in forces:
        assert (event[:, 6] != records[:, 6]).all() and (onfluid[:, 3] != records[:, 6]).all()


@pytest.mark.parametrize("dim", DIMS)
def test_every_branch_of_the_drag_law_is_reached(dim):
    reached = set()
    for cid in ("branches", "nu0", "function", "canonical"):
        reached |= set(_reference(cid, dim)[7])
    assert reached == set(F.DRAG_BRANCHES), sorted(set(F.DRAG_BRANCHES) - reached)
    # and on both sides of each threshold, in the one case that is built for it
    names = _reference("branches", dim)[7]
    for name in ("below-1e-8", "below-50", "from-50"):
        assert names.count(name) >= 16, (name, names.count(name))


def test_added_mass_before_and_after_buoyancy_differ():
    """the two list orders are two cases: the buoyancy sees the mass the added-mass force has changed, or not"""
    for dim in DIMS:
        a, b = _reference("canonical", dim)[3], _reference("reverse", dim)[3]
        assert (a[:, 3:3 + dim] != b[:, 3:3 + dim]).any(axis=1).mean() > 0.9
