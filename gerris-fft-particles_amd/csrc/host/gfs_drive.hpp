// gfs_drive.hpp -- running what a simulation file describes, through the C ABI of include/gfship.h:
//   GfsSimulation   simulation_run     src/simulation.c:432-557      (run_simulation; run_tree on a refined tree)
//   GfsPoisson      poisson_run        src/simulation.c:2213-2285    (run_poisson; run_tree_poisson)
//   GfsAdvection    advection_run      src/simulation.c:2061-2116    (run_advection)
// with the reference's event loop, the fields a function of the file gives (alpha, viscosity: the refresh_*
// family), the boundary conditions, GfsInit, the resolution of GfsRefine, and gfs_simulation_write.
// Order matters: the functions of the file are compiled, and the shell pipes of the outputs are started,
// before anything touches the device.
#pragma once
#include "gfs_classes.hpp"

namespace gfs {

inline void apply_multilevel (gfship_multilevel_params * p, const std::map<std::string, std::string> & m)
{
  for (auto & kv : m) {
    const char * v = kv.second.c_str ();
    if (kv.first == "tolerance") p->tolerance = atof (v);
    else if (kv.first == "nrelax") p->nrelax = (unsigned) atol (v);
    else if (kv.first == "erelax") p->erelax = (unsigned) atol (v);
    else if (kv.first == "minlevel") p->minlevel = (unsigned) atol (v);
    else if (kv.first == "nitermax") p->nitermax = (unsigned) atol (v);
    else if (kv.first == "nitermin") p->nitermin = (unsigned) atol (v);
    else if (kv.first == "weighted") p->weighted = atoi (v);
    else if (kv.first == "beta") p->beta = atof (v);
    else if (kv.first == "omega") p->omega = atof (v);
  }
  if (p->tolerance <= 0. || p->nrelax == 0 || p->erelax == 0 || p->beta < 0.5 || p->beta > 1.) {
    fprintf (stderr, "gfship: invalid multilevel parameters\n");
    exit (1);
  }
}

// the `{ shell script }' outputs are started (popen: a fork) before the device is created; files and
// the standard streams are opened when their event first fires, as in the reference
inline void open_pipes (Run & R)
{
  for (auto & o : R.outputs)
    if (!o->format.empty () && o->format[0] == '{')
      o->open ();
}

// gfs_simulation_write (src/simulation.c:1343-1361): the file this run was read from, with the
// current GfsTime, without the objects that have done their work (GfsInit, GfsInitSpectra: events
// with t >= end are not written, simulation_write :125-137; GfsRefine: the tree follows, :113-123),
// and the cell data of the variables `list' between the braces of the GfsBox (gfs_box_write
// src/boundary.c:1819-1851).  The time is written with 17 significant digits (the reference prints
// %g, gfs_time_write src/simulation.c:1642-1660, and so cannot restart at exactly the same t).
inline void write_simulation (Run & R, FILE * fp, const std::vector<int> & list, bool binary)
{
  fprintf (fp, "# Gerris Flow Solver %dD version 1.3.2 (gfship)\n", R.dim);
  fprintf (fp, "1 %d GfsSimulation GfsBox GfsGEdge { version = 120812 variables = ", R.nedges);
  for (size_t q = 0; q < list.size (); q++)
    fprintf (fp, "%s%s", q ? "," : "", R.vars[list[q]].name.c_str ());
  fprintf (fp, " %s} {\n", binary ? "binary = 1 " : "");
  fprintf (fp, "  GfsTime { i = %u t = %.17g ", R.i, R.t);
  if (R.end < DBL_MAX) fprintf (fp, "end = %.17g ", R.end);
  if (R.iend < INT_MAX) fprintf (fp, "iend = %u ", R.iend);
  if (R.dtmax < DBL_MAX) fprintf (fp, "dtmax = %.17g ", R.dtmax);
  fputs ("}\n", fp);
  for (auto & ot : R.object_texts) {
    const std::string & c = ot.first;
    if (c == "Time" || c == "Refine" || c == "Init" || c == "InitSpectra") continue;
    fprintf (fp, "  %s\n", ot.second.c_str ());
  }
  fputs ("}\n", fp);
  std::string image;
  size_t leaves = 1;       /* size = the number of leaves (box_size, src/boundary.c:1814-1831) */
  if (R.tree_mode) {
    // a refined tree: the image of gfship_tree_snapshot_write, every cell of every level (the non-leaf cells
    // hold the result of the last gfs_cell_coarse_init)
    std::vector<int> tv;
    for (int q : list) {
      if (R.vars[q].dev < 0) {
        fprintf (stderr, "gfship: GfsOutputSimulation: the variable `%s' is not kept on a refined tree\n", R.vars[q].name.c_str ());
        exit (1);
      }
      tv.push_back (R.vars[q].dev);
    }
    image.assign (gfship_tree_snapshot_bytes (R.tree, (int) tv.size ()), '\0');
    if (image.empty ()) CHECK (-1);
    CHECK (gfship_tree_snapshot_write (R.tree, (int) tv.size (), tv.data (), &image[0], image.size ()));
    leaves = R.leaves.size ();
  }
  else {
    // the cell data: device variables straight from the device image; host-only variables (Div of a
    // GfsPoisson file ...) go through a temporary device variable
    std::vector<gfship_field> f, tmp;
    for (int q : list) {
      if (R.vars[q].dev >= 0) f.push_back (R.vars[q].dev);
      else {
        gfship_field t = gfship_field_alloc (R.dom, -1);
        CHECK (t);
        CHECK (gfship_field_upload (R.dom, t, R.level, host_of (R, q).data ()));
        f.push_back (t);
        tmp.push_back (t);
      }
    }
    image.assign (gfship_snapshot_tree_bytes (R.dom, (int) f.size ()), '\0');
    CHECK (gfship_snapshot_tree_write (R.dom, (int) f.size (), f.data (), &image[0], image.size ()));
    for (gfship_field t : tmp) gfship_field_free (R.dom, t);
    for (int l = 0; l < R.level; l++) leaves *= R.dim == 3 ? 8 : 4;
  }
  fprintf (fp, "GfsBox { id = 1 pid = -1 size = %zu x = 0 y = 0 z = 0%s%s } {\n", leaves,
           R.box_text.empty () ? "" : " ", R.box_text.c_str ());
  if (binary)
    fwrite (image.data (), 1, image.size (), fp);
  else
    gfs::tree_write_text (fp, image, list.size ());
  fputs ("}\n", fp);
  fputs (R.edges_text.c_str (), fp);
}

// ---- derived variables, src/simulation.c:660-905
inline void add_derived (Run & R)
{
  Run * pr = &R;
  auto add = [&] (const std::string & name, std::function<void (Variable &)> f) {
    int v = R.get_or_add_variable (name);
    R.vars[v].derive = f;
  };
  auto vel = [pr] (int c) -> const std::vector<double> & {
    return host_of (*pr, pr->velocity_var (c));
  };
  auto velocity2 = [pr, vel] (size_t c) {
    double s = 0.;
    for (int q = 0; q < pr->dim; q++) s += vel (q)[c]*vel (q)[c];
    return s;
  };
  add ("Velocity2", [pr, velocity2] (Variable & V) {
    for_each_cell (*pr, [&] (const Cell &, size_t c) { V.host[c] = velocity2 (c); });
  });
  add ("Velocity", [pr, velocity2] (Variable & V) {
    for_each_cell (*pr, [&] (const Cell &, size_t c) { V.host[c] = sqrt (velocity2 (c)); });
  });
  add ("Divergence", [pr, vel] (Variable & V) {
    // gfs_divergence: sum of gfs_center_gradient (u_c) / size, src/fluid.c:2356-2372
    double h = 1./pr->n ();
    size_t r = pr->n () + 2, off[3] = { 1, r, r*r };
    for_each_cell (*pr, [&] (const Cell &, size_t c) {
      double div = 0.;
      for (int q = 0; q < pr->dim; q++)
        div += (vel (q)[c + off[q]] - vel (q)[c - off[q]])/2.;
      V.host[c] = div/h;
    });
  });
  if (R.dim == 2)
    add ("Vorticity", [pr, vel] (Variable & V) {
      // gfs_vorticity, src/fluid.c:2391-2402: (dV/dx - dU/dy)/size
      double h = 1./pr->n ();
      size_t r = pr->n () + 2;
      for_each_cell (*pr, [&] (const Cell &, size_t c) {
        V.host[c] = ((vel (1)[c + 1] - vel (1)[c - 1])/2. - (vel (0)[c + r] - vel (0)[c - r])/2.)/h;
      });
    });
}

// ---- events, src/event.c:60-127,410-459
inline bool event_fires (Run & R, Event & e)
{
  if (e.dead) return false;
  if (e.t >= e.end || e.i >= e.iend || R.t > e.end || R.i > e.iend) { e.dead = true; return false; }
  if (e.end_event) {
    if (e.n == 0 && (R.t >= R.end || R.i >= R.iend)) { e.n = 1; return (e.realised = true); }
    return (e.realised = false);
  }
  if (R.t >= e.t) {
    if (e.istep < INT_MAX) {
      if (e.n == 0) { e.i = R.i + e.istep; e.n++; return (e.realised = true); }
    }
    else {
      e.n++;
      e.t = e.start + e.n*e.step;
      return (e.realised = true);
    }
  }
  if (R.i >= e.i) {
    if (e.step < DBL_MAX) {
      if (e.n == 0) { e.start = R.t; e.t = e.start + e.step; e.n = 1; return (e.realised = true); }
    }
    else {
      e.n++;
      e.i += e.istep;
      return (e.realised = true);
    }
  }
  return (e.realised = false);
}

inline void events_init (Run & R)
{
  for (auto & pe : R.events) {
    Event & e = *pe;
    if (e.end_event) e.t = e.start = DBL_MAX/2.;
    else if (e.istep < INT_MAX)
      while (e.i < R.i) { e.n++; e.i += e.istep; }
    else
      while (e.t < R.t) { e.n++; e.t = e.start + e.n*e.step; }
  }
}

inline void events_do (Run & R)
{
  invalidate_device_copies (R);
  for (auto & pe : R.events)
    if (event_fires (R, *pe))
      pe->action ();
}

// gfs_event_next, src/event.c:46-71
inline double event_next (const Event & e, double t, unsigned i)
{
  if (t < e.t) return e.t;
  if (e.t >= e.end || e.i >= e.iend || t > e.end || i > e.iend) return DBL_MAX;
  if (e.end_event) return DBL_MAX;
  if (t >= e.t) {
    if (e.istep < INT_MAX) {
      if (e.n == 0) return DBL_MAX;
    }
    else
      return e.start + (e.n + 1)*e.step;
  }
  if (i >= e.i && e.step < DBL_MAX && e.n == 0)
    return t + e.step;
  return DBL_MAX;
}

// the event loop of gfs_simulation_set_timestep (src/simulation.c:1603-1610), called back by
// libgfship from inside gfship_set_timestep
inline double next_event_hook (void * ctx, double t, unsigned i)
{
  const Run & R = *(const Run *) ctx;
  double tnext = INT_MAX;
  for (auto & pe : R.events) {
    if (pe->dead) continue;
    double next = event_next (*pe, t, i);
    if (t < next && next < tnext)
      tnext = next + 1e-9;
  }
  return tnext;
}

// ---- set-up of the device simulation
inline void set_boundary_conditions (Run & R)
{
  int n = R.n ();
  size_t nface = R.dim == 3 ? (size_t) n*n : n;
  for (int d = 0; d < 2*R.dim; d++)
    for (auto & kv : R.bc[d]) {
      int v = R.var_index (kv.first);
      if (v < 0 || R.vars[v].dev < 0) {
        fprintf (stderr, "gfship: boundary condition on unknown variable `%s'\n", kv.first.c_str ());
        exit (1);
      }
      // value at the centre of every boundary face, first tangential axis fastest
      std::vector<double> val (nface);
      int c = d/2, ta = c == 0 ? 1 : 0, tb = c == 2 ? 1 : 2;
      double h = 1./n;
      for (size_t f = 0; f < nface; f++) {
        int ijk[3] = { 1, 1, 1 };
        ijk[c] = (d & 1) ? 1 : n;
        ijk[ta] = (int) (f % n) + 1;
        if (R.dim == 3) ijk[tb] = (int) (f / n) + 1;
        double p[3];
        cell_pos (R, Cell { ijk[0], ijk[1], R.dim == 3 ? ijk[2] : 0, R.level }, p);
        p[c] += (d & 1) ? -h/2. : h/2.;      /* ftt_face_pos */
        val[f] = eval (R, kv.second.val, p, -1);
      }
      CHECK (gfship_field_set_bc (R.dom, R.vars[v].dev, d, kv.second.kind, val.data ()));
    }
}

inline void apply_init (Run & R)
{
  // gfs_init_event, src/init.c: every `var = function` in file order, on the leaf cells
  for (auto & kv : R.init) {
    int v = R.var_index (kv.first);
    std::vector<double> a = host_of (R, v);     /* copy: the function may read the variable */
    for_each_cell (R, [&] (const Cell & cell, size_t c) {
      double p[3];
      cell_pos (R, cell, p);
      a[c] = eval (R, kv.second, p, (long) c);
    });
    R.vars[v].host = a;
    if (R.vars[v].dev < 0) continue;
    if (R.tree_mode) tree_scatter (R, R.vars[v].dev, R.vars[v].host);
    else CHECK (gfship_field_upload (R.dom, R.vars[v].dev, R.level, R.vars[v].host.data ()));
    R.vars[v].host_time = (double) R.i;
  }
}

// gfs_refine_refine (src/refine.c:45-60): a cell of level l is refined while l < f (x, y, z) at its
// centre.  A function that does not ask for the same level everywhere asks for a refined tree.
inline void resolve_refine (Run & R)
{
  if (!R.refine_fn) return;
  int level = 0;
  for (;;) {
    const int n = 1 << level;
    bool yes = false, no = false;      /* not counts: 2^(3*11) cells do not fit an int */
    for (int k = 1; k <= (R.dim == 3 ? n : 1); k++)
      for (int j = 1; j <= n; j++)
        for (int i = 1; i <= n; i++) {
          double p[3] = { -0.5 + (i - 0.5)/n, -0.5 + (j - 0.5)/n, R.dim == 3 ? -0.5 + (k - 0.5)/n : 0. };
          if (level < eval (R, R.refine_fn, p, -1)) yes = true; else no = true;
        }
    if (yes && no) {
      // a statically refined tree: gfship_tree (GfsSimulation or GfsPoisson, one box, sides periodic or GfsBoundary)
      bool sides_ok = true;
      for (int d = 0; d < 2*R.dim; d++)
        if (R.side[d] != GFSHIP_SIDE_PERIODIC && R.side[d] != GFSHIP_SIDE_BOUNDARY) sides_ok = false;
      if ((R.sim_class == "Simulation" || R.sim_class == "Poisson") && sides_ok) {
        R.tree_mode = true;
        R.level = level;     /* the coarsest leaves */
        return;
      }
      fprintf (stderr, "gfship: line %d: the Refine function asks for a non-uniform tree at level %d "
               "(refined trees: GfsSimulation or GfsPoisson in one box)\n", R.refine_line, level);
      exit (1);
    }
    if (!yes) break;
    if (++level > GFSHIP_MAXLEVEL) {
      fprintf (stderr, "gfship: line %d: Refine: more than %d levels\n", R.refine_line, GFSHIP_MAXLEVEL);
      exit (1);
    }
  }
  R.level = level;
}

inline double refine_hook (double x, double y, double z, void * ctx)
{
  Run & R = *(Run *) ctx;
  double p[3] = { x, y, z };
  return eval (R, R.refine_fn, p, -1);
}

// ---- a statically refined tree
// a file that carries its tree (cell_read, src/ftt.c:1807-1866: the tree of the file IS the tree): the hook is
// asked at the centre of a cell, -0.5 + (i + 0.5)/2^l, which identifies l; a cell the file refines asks for one
// level more
struct FileTree {
  int dim;
  std::unordered_map<uint64_t, bool> leaf;      // cell -> leaf bit
  static uint64_t key (int l, int i, int j, int k) {
    return ((((uint64_t) l << 19 | (uint64_t) k) << 19 | (uint64_t) j) << 19) | (uint64_t) i;
  }
};

inline double file_refine_hook (double x, double y, double z, void * ctx)
{
  const FileTree & F = *(const FileTree *) ctx;
  for (int l = 0; l <= 19; l++) {
    const double n = (double) (1 << l), i = (x + 0.5)*n - 0.5;
    if (i != floor (i)) continue;
    const double j = (y + 0.5)*n - 0.5, k = F.dim == 3 ? (z + 0.5)*n - 0.5 : 0.;
    auto c = F.leaf.find (FileTree::key (l, (int) i, (int) j, (int) k));
    return c != F.leaf.end () && !c->second ? l + 1 : l;
  }
  return 0.;
}

typedef std::vector<std::vector<unsigned char>> TreeFlags;

// the leaves of the tree in the order of ftt_cell_traverse (pre-order, children 0..3: bit 0 = +x,
// bit 1 = -y, src/ftt.c:301-316)
inline void tree_leaves (Run & R, const TreeFlags & flag, const Cell & c)
{
  unsigned char f = flag[c.l][R.level_index (c)];
  if (f == 1)
    R.leaves.push_back (c);
  else if (f == 2)
    for (int q = 0; q < (1 << R.dim); q++)
      tree_leaves (R, flag, Cell { 2*c.i - 1 + (q & 1), 2*c.j - ((q >> 1) & 1), 2*c.k - ((q >> 2) & 1), c.l + 1 });
}

// the values of the conditions of variable `name' on the GfsBoundary sides of a tree: the GfsFunction at the
// centre of the face of every leaf ghost cell (gfs_function_face_value at ftt_face_pos), uploaded to `var'
inline void upload_tree_bc_values (Run & R, const TreeFlags & flag, const std::string & name, int var)
{
  const int depth = gfship_tree_depth (R.tree);
  for (int l = 0; l <= depth; l++) {
    const int n = 1 << l;
    std::vector<double> val (R.level_size (l), 0.);
    bool any = false;
    for (int d = 0; d < 2*R.dim; d++) {
      if (R.side[d] != GFSHIP_SIDE_BOUNDARY || !R.bc[d].count (name) || !R.bc[d][name].val) continue;
      const int c = d/2, ta = c == 0 ? 1 : 0, tb = c == 2 ? 1 : 2;
      for (int b = 1; b <= (R.dim == 3 ? n : 1); b++)
        for (int a = 1; a <= n; a++) {
          int g[3] = { 0, 0, 0 };
          g[c] = (d & 1) ? 0 : n + 1;
          g[ta] = a;
          g[tb] = R.dim == 3 ? b : 0;
          const Cell ghost = { g[0], g[1], g[2], l };
          if (flag[l][R.level_index (ghost)] != 1) continue;          /* leaf ghost cells only */
          double p[3];
          cell_pos (R, ghost, p);
          p[c] = (d & 1) ? -0.5 : 0.5;            /* the face between the ghost cell and the box */
          val[R.level_index (ghost)] = eval (R, R.bc[d][name].val, p, -1);
          any = true;
        }
    }
    if (any)
      CHECK (gfship_tree_upload (R.tree, var, l, val.data ()));
  }
}

// poisson_run (src/simulation.c:2213-2285) on a statically refined tree, sides periodic or GfsBoundary
inline int run_tree_poisson (Run & R)
{
  if (check_tree_events (R)) return 1;
  open_pipes (R);
  CHECK (gfship_tree_create_sides (&R.tree, R.dim, refine_hook, &R, R.side, R.device));
  const TreeFlags flag = tree_flags (R);
  tree_leaves (R, flag, Cell { 1, 1, 1, 0 });
  R.vars[R.var_index ("P")].dev = GFSHIP_TREE_P;
  // the conditions of P: kind per side, value of the GfsFunction at the centre of the face of every
  // leaf ghost cell (gfs_function_face_value at ftt_face_pos)
  bool dirichlet = false;
  for (int d = 0; d < 2*R.dim; d++) {
    if (R.side[d] != GFSHIP_SIDE_BOUNDARY) continue;
    for (auto & kv : R.bc[d])
      if (kv.first != "P") {
        fprintf (stderr, "gfship: a boundary condition on `%s' is not supported on a refined tree\n", kv.first.c_str ());
        return 1;
      }
    int kind = R.bc[d].count ("P") ? R.bc[d]["P"].kind : GFSHIP_BC_SYMMETRY;
    if (kind == GFSHIP_BC_DIRICHLET) dirichlet = true;
    CHECK (gfship_tree_set_bc (R.tree, d, kind));
  }
  upload_tree_bc_values (R, flag, "P", GFSHIP_TREE_BCVAL);
  apply_multilevel (gfship_tree_projection_params (R.tree, 1), R.approx_set);
  apply_init (R);
  events_init (R);
  gfship_multilevel_params * par = gfship_tree_projection_params (R.tree, 1);
  while (R.i < R.iend && R.t < R.end) {
    // correct_div, src/simulation.c:2170-2190: div = Div size^2 on the leaves; without a Dirichlet
    // condition its mean is removed (GtsRange means: sums in traversal order over the leaves)
    const std::vector<double> & Div = host_of (R, R.var_index ("Div"));
    std::vector<double> div (R.total (), 0.);
    double sum = 0., vol = 0.;
    for (size_t c = 0; c < R.leaves.size (); c++) {
      double size = 1./(1 << R.leaves[c].l);
      double a = size*size*1.;
      div[c] = Div[c]*a;
      vol += a;
    }
    if (!dirichlet) {
      for (size_t c = 0; c < R.leaves.size (); c++) sum += div[c];
      double nn = (double) R.leaves.size ();
      double ddiv = - (sum/nn)/(vol/nn);
      for (size_t c = 0; c < R.leaves.size (); c++) {
        double size = 1./(1 << R.leaves[c].l);
        div[c] += size*size*ddiv*1.;
      }
    }
    tree_scatter (R, GFSHIP_TREE_DIV, div);
    CHECK (gfship_tree_poisson_solve (R.tree, par, 1.));
    R.t = 0.;
    R.i++;
    events_do (R);
  }
  for (auto & o : R.outputs) o->close ();
  gfship_tree_destroy (R.tree);
  R.tree = nullptr;
  return 0;
}

// what a GfsSimulation on a refined tree does not do: refused before the device is touched
inline int check_tree_simulation (Run & R)
{
  auto refuse = [] (const char * what) {
    fprintf (stderr, "gfship: %s is not supported on a refined tree\n", what);
    return 1;
  };
  if (R.tracers.size () > 2) return refuse ("more than two tracers");
  for (const TracerSpec & tr : R.tracers)
    if (tr.gradient > 1) return refuse ("this gradient of a GfsVariableTracer");
  for (const TracerSpec & tr : R.tracers)
    if (tr.scheme != GFSHIP_SCHEME_GODUNOV) return refuse ("GfsVariableTracer { scheme = none }");
  for (auto & ps : R.plists)      /* tracers only: no particulates, no forces (gfship_particles_create_tree) */
    if (ps->particulate || !ps->forces.empty ()) {
      fprintf (stderr, "gfship: line %d: a GfsParticleList of GfsParticulate objects or with GfsForce objects is not "
               "supported on a refined tree (GfsParticle tracers are)\n", ps->line);
      return 1;
    }
  if (!R.init_spectra.empty ()) return refuse ("GfsInitSpectra");
  if (!R.device_vars.empty ()) return refuse ("a turbulent-viscosity variable");
  if (R.dtmax != DBL_MAX) return refuse ("Time { dtmax }");
  for (auto & kv : R.adv_set)
    if (kv.first != "cfl" && !(kv.first == "gradient" && kv.second == "gfs_center_gradient") &&
        !(kv.first == "gc" && atoi (kv.second.c_str ()) == 1))
      return refuse ("this AdvectionParams setting");
  if (check_tree_events (R)) return 1;
  for (int d = 0; d < 2*R.dim; d++)
    for (auto & kv : R.bc[d])     /* GfsBoundary sides: conditions on P and on the velocity components */
      if (kv.first != "P" && R.velocity_component (kv.first) < 0) {
        fprintf (stderr, "gfship: a boundary condition on `%s' is not supported on a refined tree (side %s)\n",
                 kv.first.c_str (), side_name[d]);
        return 1;
      }
  return 0;
}

// the tree: the one GfsRefine asks for, or the one of a file that carries its tree; flag: the flags of its cells
inline int create_tree (Run & R, TreeFlags & flag)
{
  if (!R.snapshot.has_tree) {
    CHECK (gfship_tree_create_sides (&R.tree, R.dim, refine_hook, &R, R.side, R.device));
    flag = tree_flags (R);
    return 0;
  }
  if (R.snapshot.depth > 19) {
    fprintf (stderr, "gfship: a file with more than 19 levels is not supported on a refined tree\n");
    return 1;
  }
  FileTree ft;
  ft.dim = R.dim;
  for (const gfs::TreeCell & c : R.snapshot.cells)
    ft.leaf[FileTree::key (c.level, c.i, c.j, c.k)] = c.leaf;
  if (R.refine_fn)      /* gfs_simulation_refine after the file is read: it must find nothing to add */
    for (const gfs::TreeCell & c : R.snapshot.cells) {
      const double h = 1./(1 << c.level);
      double p[3] = { -0.5 + (c.i + 0.5)*h, -0.5 + (c.j + 0.5)*h, R.dim == 3 ? -0.5 + (c.k + 0.5)*h : 0. };
      if (c.leaf && c.level < eval (R, R.refine_fn, p, -1)) {
        fprintf (stderr, "gfship: line %d: GfsRefine asks for more than the tree of the file holds "
                 "(a restart into another tree is not supported)\n", R.refine_line);
        return 1;
      }
    }
  CHECK (gfship_tree_create_sides (&R.tree, R.dim, file_refine_hook, &ft, R.side, R.device));
  flag = tree_flags (R);
  // the tree the library built must be the tree of the file: the balance (oct_new with check_neighbors) and
  // the corner rule would otherwise have added cells
  size_t cells = 0;
  bool same = true;
  for (int l = 0; l < (int) flag.size (); l++)
    for (int k = 1; k <= (R.dim == 3 ? 1 << l : 1); k++)
      for (int j = 1; j <= 1 << l; j++)
        for (int i = 1; i <= 1 << l; i++) {
          const unsigned char f = flag[l][R.level_index (Cell { i, j, k, l })];
          if (!f) continue;
          cells++;
          auto c = ft.leaf.find (FileTree::key (l, i - 1, j - 1, R.dim == 3 ? k - 1 : 0));
          if (c == ft.leaf.end () || c->second != (f == 1)) same = false;
        }
  if (!same || cells != R.snapshot.cells.size ()) {
    fprintf (stderr, "gfship: the tree of the file is not one this program builds (%zu cells in the file, %zu "
             "after the 2:1 balance and the corner rule)\n", R.snapshot.cells.size (), cells);
    return 1;
  }
  return 0;
}

inline int write_particles (Run & R);

// simulation_run (src/simulation.c:432-557) on a statically refined tree
inline int run_tree (Run & R)
{
  if (R.sim_class == "Poisson")
    return run_tree_poisson (R);
  if (check_tree_simulation (R)) return 1;
  int v = R.var_index ("Vorticity");
  if (v >= 0)
    R.vars[v].derive = [] (Variable &) {
      fprintf (stderr, "gfship: the variable Vorticity is not supported on a refined tree\n");
      exit (1);
    };
  v = R.var_index ("Divergence");
  if (v >= 0)      /* gfs_divergence on the device, then one value per leaf */
    R.vars[v].derive = [&R] (Variable & V) {
      CHECK (gfship_tree_divergence (R.tree));
      tree_gather (R, GFSHIP_TREE_DIV, V.host);
    };
  open_pipes (R);
  TreeFlags flag;
  if (create_tree (R, flag)) return 1;
  tree_leaves (R, flag, Cell { 1, 1, 1, 0 });
  R.vars[R.var_index ("P")].dev = GFSHIP_TREE_P;
  R.vars[R.var_index ("Pmac")].dev = GFSHIP_TREE_PMAC;
  R.velocity (0).dev = GFSHIP_TREE_U;
  R.velocity (1).dev = GFSHIP_TREE_V;
  if (R.dim == 3)
    R.velocity (2).dev = GFSHIP_TREE_W;
  for (const TracerSpec & tr : R.tracers) {
    int v = gfship_tree_add_tracer (R.tree, tr.gradient);
    CHECK (v);
    R.vars[R.var_index (tr.name)].dev = v;
  }
  for (int d = 0; d < 2*R.dim; d++) {
    if (R.side[d] != GFSHIP_SIDE_BOUNDARY) continue;
    if (R.bc[d].count ("P")) CHECK (gfship_tree_set_bc (R.tree, d, R.bc[d]["P"].kind));
    for (int c = 0; c < R.dim; c++)
      if (R.bc[d].count (velocity_name[c])) CHECK (gfship_tree_set_bc_u (R.tree, c, d, R.bc[d][velocity_name[c]].kind));
  }
  upload_tree_bc_values (R, flag, "P", GFSHIP_TREE_BCVAL);
  for (int c = 0; c < R.dim; c++)
    upload_tree_bc_values (R, flag, velocity_name[c], GFSHIP_TREE_BCU + c);
  for (int c = 0; c < R.dim; c++)
    if (R.source[c] != 0.)
      CHECK (gfship_tree_set_source (R.tree, c, R.source[c]));
  for (int c = 0; c < R.dim; c++)
    if (R.visc[c] != 0.) {
      CHECK (gfship_tree_set_viscosity (R.tree, c, R.visc[c]));
      apply_multilevel (gfship_tree_diffusion_params (R.tree, c), R.diff_set[c]);
    }
  apply_multilevel (gfship_tree_projection_params (R.tree, 0), R.proj_set);
  apply_multilevel (gfship_tree_projection_params (R.tree, 1), R.approx_set);
  for (auto & ps : R.plists)      /* the lists of tracers: read before any GfsInit event runs, as on a uniform box */
    CHECK (gfship_particles_create_tree (&ps->pl, R.tree, (int) ps->id.size (), ps->pos.data (), ps->id.data ()));
  double cfl = 0.8;        /* gfs_advection_params_init, src/advection.c:922-942 */
  for (auto & kv : R.adv_set)
    if (kv.first == "cfl") cfl = atof (kv.second.c_str ());
  apply_init (R);
  if (R.snapshot.has_tree) {
    // gfs_box_read -> cell_read[_binary] + gfs_cell_read[_binary]: all levels of the variables of the file; then the
    // branch time.i > 0 of simulation_run
    std::vector<int> tv;
    for (const std::string & nm : R.snapshot.variables) {
      int q = R.var_index (nm);
      if (q < 0 || R.vars[q].dev < 0) {
        fprintf (stderr, "gfship: the variable `%s' of the file is not kept on a refined tree\n", nm.c_str ());
        return 1;
      }
      tv.push_back (R.vars[q].dev);
      R.vars[q].host_time = -1.;
    }
    CHECK (gfship_tree_snapshot_read (R.tree, (int) tv.size (), tv.data (), R.snapshot.tree.data (), R.snapshot.tree.size ()));
    R.snapshot.tree.clear ();
    CHECK (gfship_tree_restart (R.tree, R.t, R.i));
  }
  events_init (R);
  CHECK (gfship_tree_set_time (R.tree, R.end, cfl));
  CHECK (gfship_tree_set_next_event (R.tree, next_event_hook, &R));
  CHECK (gfship_tree_start (R.tree));
  while (R.t < R.end && R.i < R.iend) {
    events_do (R);
    CHECK (gfship_tree_set_time (R.tree, R.end, cfl));
    CHECK (gfship_tree_step (R.tree));
    R.t = gfship_tree_time (R.tree);
    R.i = gfship_tree_iter (R.tree);
  }
  events_do (R);
  if (!R.particles_out.empty () && write_particles (R)) return 1;
  for (auto & sp : R.particulate_sources) gfship_particulate_source_destroy (sp->src);
  for (auto & ps : R.plists) gfship_particles_destroy (ps->pl);
  for (auto & o : R.outputs) o->close ();
  gfship_tree_destroy (R.tree);
  R.tree = nullptr;
  return 0;
}

// ---- the fields a GfsFunction of the file gives the simulation: alpha (GfsPhysicalParams) and the viscosity
// (GfsSourceDiffusion / GfsSourceViscosity with a function)
// f on level l: at the centres of the cells (c < 0), or at the centres of their + faces along c (the ghost
// entry in front of the first cell: its - face), the layout gfship_poisson_coefficients_alpha takes.  vals: the
// variables f reads, in its order; on a face they are interpolated (gfs_face_interpolated_value,
// src/fluid.c:2186-2198: ((x1 - 0.5) v0 + 0.5 v1)/x1 with x1 = 1 between cells of one level)
inline void function_on_level (const Run & R, const Function * f, int l, int c,
                               const std::vector<const std::vector<double> *> & vals, std::vector<double> & a)
{
  const int n = 1 << l;
  const double h = 1./n;
  a.assign (R.level_size (l), 0.);
  int lo[3] = { 1, 1, R.dim == 3 ? 1 : 0 }, hi[3] = { n, n, R.dim == 3 ? n : 0 };
  if (c >= 0) lo[c] = 0;
  const size_t off = c < 0 ? 0 : R.level_index (Cell { c == 0, c == 1, c == 2, l }) - R.level_index (Cell { 0, 0, 0, l });
  for (int k = lo[2]; k <= hi[2]; k++)
    for (int j = lo[1]; j <= hi[1]; j++)
      for (int i = lo[0]; i <= hi[0]; i++) {
        const Cell cell = { i, j, k, l };
        const size_t q0 = R.level_index (cell);
        double p[3], v[32];
        cell_pos (R, cell, p);
        if (c >= 0) p[c] += h/2.;
        for (size_t q = 0; q < vals.size (); q++) {
          const double x1 = 1., v0 = (*vals[q])[q0], v1 = (*vals[q])[q0 + off];
          v[q] = ((x1 - 0.5)*v0 + 0.5*v1)/x1;
        }
        a[q0] = f->kind == Function::CONSTANT ? f->val : f->kind == Function::VARIABLE ? v[0] :
          f->fn (p[0], p[1], p[2], R.t, v);
      }
}

// the values go to the device field `dev' of level l: allocated the first time, when the caller hands the
// field to the simulation once all of it is there (true); uploaded only after that
inline bool upload_coefficient (Run & R, gfship_field & dev, int l, const std::vector<double> & a)
{
  const bool first = dev < 0;
  if (first) {
    dev = gfship_field_alloc (R.dom, -1);
    CHECK (dev);
  }
  CHECK (gfship_field_upload (R.dom, dev, l, a.data ()));
  return first;
}

// GfsPhysicalParams { alpha }: gfs_function_face_value (alpha, face) of every leaf face.  Both projections of a
// step evaluate alpha with the same time and the same tracers (gfs_advance_tracers comes last in the
// loop body, src/simulation.c:479-548): once before every step.
inline int refresh_alpha (Run & R)
{
  if (!R.alpha || (R.alpha_static && R.alpha_dev[0] >= 0))
    return 0;
  std::vector<const std::vector<double> *> vals;
  for (int a : R.alpha->reads ()) {
    /* the values beyond the box sides are those of the boundary conditions (the reference's ghost cells
       hold them at this point: gfs_simulation_init / the end of the tracer's advection) */
    Variable & V = R.vars[a];
    CHECK (gfship_bc (R.dom, V.dev, V.dev, R.level));
    V.host_time = -1.;
    vals.push_back (&host_of (R, a));
  }
  if (vals.size () > 32) { fprintf (stderr, "gfship: too many variables in alpha\n"); return 1; }
  std::vector<double> a;
  bool first = false;
  for (int c = 0; c < R.dim; c++) {
    function_on_level (R, R.alpha, R.level, c, vals, a);
    first = upload_coefficient (R, R.alpha_dev[c], R.level, a);
  }
  if (first)
    CHECK (gfship_sim_set_alpha (R.sim, R.alpha_dev));
  return 0;
}

// GfsSourceDiffusion / GfsSourceViscosity with a function: gfs_function_face_value at every leaf face
// (diffusion_face, src/source.c:933-939), evaluated the way refresh_alpha evaluates alpha; components that
// share the function (GfsSourceViscosity) share the fields
inline int refresh_viscosity (Run & R)
{
  std::vector<double> a;
  for (int c = 0; c < R.dim; c++) {
    const Function * f = R.visc_fn[c];
    if (!f) continue;
    const bool first = R.visc_dev[c][0] < 0;
    if (!first && !depends_on_t (f))
      continue;                 /* static */
    int shared = -1;
    for (int q = 0; q < c; q++)
      if (R.visc_fn[q] == f) shared = q;
    if (shared < 0)
      for (int q = 0; q < R.dim; q++) {
        function_on_level (R, f, R.level, q, {}, a);
        upload_coefficient (R, R.visc_dev[c][q], R.level, a);
      }
    else if (first)
      for (int q = 0; q < R.dim; q++) R.visc_dev[c][q] = R.visc_dev[shared][q];
    if (first)
      CHECK (gfship_sim_set_viscosity_faces (R.sim, c, R.visc_dev[c]));
  }
  return 0;
}

// alpha at the cell centres of EVERY level (gfs_function_value (alpha, cell) under FTT_TRAVERSE_ALL,
// diffusion_mixed_coeff src/poisson.c:1321-1332): the density of the implicit diffusion
inline int refresh_alpha_cell (Run & R)
{
  bool visc = false;
  for (int c = 0; c < R.dim; c++) visc = visc || R.has_viscosity (c);
  if (!R.alpha || !(visc || R.particulate_forces ()) || (R.alpha_static && R.alpha_cell_dev >= 0))
    return 0;
  if (R.alpha_cell_dev >= 0 && R.alpha_cell_t == R.t)
    return 0;                   /* already evaluated at this time */
  R.alpha_cell_t = R.t;
  std::vector<double> a;
  bool first = false;
  for (int l = 0; l <= R.level; l++) {
    function_on_level (R, R.alpha, l, -1, {}, a);
    first = upload_coefficient (R, R.alpha_cell_dev, l, a) || first;
  }
  if (first)
    CHECK (gfship_sim_set_alpha_cell (R.sim, R.alpha_cell_dev));
  return 0;
}

// the `mu' of the GfsDiffusion of U (update_mu / gfs_diffusion_cell, src/source.c:906-946): the function of
// its GfsSourceDiffusion / GfsSourceViscosity at the centres of the leaf cells, evaluated the way
// refresh_alpha_cell evaluates alpha -- what the GfsParticleForce objects take for the viscosity at the cell
// of a particle (modules/particulatecommon.c:277-279).  Once for a function of x, y, z; before every event
// of a list with forces, at the time of the event, for a function of t
inline int refresh_viscosity_cell (Run & R)
{
  const Function * f = R.visc_fn[0];
  if (!f || !R.particulate_forces ())
    return 0;
  if (R.mu_cell_dev >= 0 && (!depends_on_t (f) || R.mu_cell_t == R.t))
    return 0;
  R.mu_cell_t = R.t;
  std::vector<double> a;
  function_on_level (R, f, R.level, -1, {}, a);
  if (upload_coefficient (R, R.mu_cell_dev, R.level, a))
    CHECK (gfship_sim_set_viscosity_cell (R.sim, R.mu_cell_dev));
  return 0;
}

// ---- a uniform box: what is refused before the device is touched; the device simulation; the three kinds of run
inline int check_run (Run & R)
{
  if (R.tree_mode)
    for (const TracerSpec & tr : R.tracers)
      if (tr.D_line) {
        fprintf (stderr, "gfship: line %d: GfsSourceDiffusion on a tracer (`%s') is not supported on a refined tree\n",
                 tr.D_line, tr.name.c_str ());
        return 1;
      }
  // a function that must not read a variable: what, where, and the first variable it reads
  auto reads_a_variable = [&R] (const Function * f, int line, const char * what) {
    const std::vector<int> used = f->reads ();
    if (!used.empty ())
      fprintf (stderr, "gfship: line %d: %s may depend on x, y, z and t (got `%s')\n", line, what,
               R.vars[used[0]].name.c_str ());
    return !used.empty ();
  };
  if (R.alpha) {
    if (R.tree_mode || R.sim_class != "Simulation") {
      fprintf (stderr, "gfship: line %d: GfsPhysicalParams { alpha } is supported for a GfsSimulation on a uniform box\n", R.alpha_line);
      return 1;
    }
    for (int v : R.alpha->reads ())
      if (!R.tracer (R.vars[v].name)) {
        /* anything else changes between the two projections of a step */
        fprintf (stderr, "gfship: line %d: alpha may depend on x, y, z, t and tracers (got `%s')\n",
                 R.alpha_line, R.vars[v].name.c_str ());
        return 1;
      }
    R.alpha_static = R.alpha->reads ().empty () && !depends_on_t (R.alpha);
  }
  bool any_visc = false;
  for (int c = 0; c < R.dim; c++) {
    any_visc = any_visc || R.has_viscosity (c);
    if (!R.visc_fn[c]) continue;
    if (R.tree_mode || R.sim_class != "Simulation") {
      fprintf (stderr, "gfship: line %d: a diffusion coefficient given as a function is supported for a GfsSimulation "
               "on a uniform box\n", R.visc_line[c]);
      return 1;
    }
    /* a coefficient that follows a tracer needs its coarse-cell values (gfs_cell_coarse_init) */
    if (reads_a_variable (R.visc_fn[c], R.visc_line[c], "the diffusion coefficient")) return 1;
  }
  /* the density of the diffusion equation is alpha on the cells of every level: a tracer's coarse-cell
     values would have to follow gfs_cell_coarse_init */
  if (R.alpha && any_visc && !R.tree_mode &&
      reads_a_variable (R.alpha, R.alpha_line, "together with a SourceDiffusion alpha")) return 1;
  /* the density of the fluid at a particle is alpha at the centre of its cell, evaluated on the host */
  if (R.alpha && R.particulate_forces () && !R.tree_mode &&
      reads_a_variable (R.alpha, R.alpha_line, "together with GfsParticulate forces alpha")) return 1;
  return 0;
}

// the domain, the simulation and everything the file sets in them, up to the state the run starts from
inline int create_simulation (Run & R, gfship_field & div)
{
  CHECK (gfship_domain_create (&R.dom, R.dim, R.level, R.side, R.device));
  CHECK (gfship_sim_create (&R.sim, R.dom));
  R.vars[R.var_index ("P")].dev = gfship_sim_variable (R.sim, GFSHIP_VAR_P, 0);
  R.vars[R.var_index ("Pmac")].dev = gfship_sim_variable (R.sim, GFSHIP_VAR_PMAC, 0);
  for (int c = 0; c < R.dim; c++)
    R.velocity (c).dev = gfship_sim_variable (R.sim, GFSHIP_VAR_U, c);
  for (const TracerSpec & tr : R.tracers) {
    int k = gfship_sim_add_tracer (R.sim);
    CHECK (k);
    R.vars[R.var_index (tr.name)].dev = gfship_sim_variable (R.sim, GFSHIP_VAR_TRACER, k);
    const TracerSpec & spec = R.tracers[(size_t) k];
    CHECK (gfship_sim_set_tracer_gradient (R.sim, k, spec.gradient));
    CHECK (gfship_sim_set_tracer_scheme (R.sim, k, spec.scheme));
    if (spec.D != 0.) {
      CHECK (gfship_sim_set_tracer_diffusion (R.sim, k, spec.D));
      apply_multilevel (gfship_sim_tracer_diffusion_params (R.sim, k), spec.diff_set);
    }
  }
  for (const std::string & dv : R.device_vars) {
    gfship_field f = gfship_field_alloc (R.dom, -1);
    CHECK (f);
    R.vars[R.var_index (dv)].dev = f;
  }
  if (R.sim_class == "Poisson") {
    div = gfship_field_alloc (R.dom, -1);     /* the temporary `div` of poisson_run */
    CHECK (div);
  }
  apply_multilevel (gfship_sim_projection_params (R.sim), R.proj_set);
  apply_multilevel (gfship_sim_approx_projection_params (R.sim), R.approx_set);
  gfship_advection_params * adv = gfship_sim_advection_params (R.sim);
  for (auto & kv : R.adv_set) {
    if (kv.first == "cfl") adv->cfl = atof (kv.second.c_str ());
    else if (kv.first == "gc") adv->gc = atoi (kv.second.c_str ());
    else if (kv.first == "gradient") {
      if (gradient_kind (kv.second) >= 0) adv->gradient = gradient_kind (kv.second);
      else { fprintf (stderr, "gfship: unsupported gradient `%s'\n", kv.second.c_str ()); return 1; }
    }
  }
  for (int c = 0; c < R.dim; c++)
    if (R.source[c] != 0.)
      CHECK (gfship_sim_set_source (R.sim, c, R.source[c]));
  /* alpha at the cell centres first: with it a viscosity and alpha go together */
  if (refresh_alpha_cell (R)) return 1;
  for (int c = 0; c < R.dim; c++) {
    if (R.visc[c] != 0.) CHECK (gfship_sim_set_viscosity (R.sim, c, R.visc[c]));
    if (R.has_viscosity (c)) apply_multilevel (gfship_sim_diffusion_params (R.sim, c), R.diff_set[c]);
  }
  if (refresh_viscosity (R) || refresh_viscosity_cell (R)) return 1;
  // the particle lists: created (and the previous velocity of the GfsForceCoeff objects stored)
  // while the fields still hold the zeros of a fresh simulation, like the reference, which reads
  // the list before any GfsInit event runs (gfs_force_coeff_read, :181-187)
  for (auto & ps : R.plists) {
    int np = (int) ps->id.size ();
    CHECK (gfship_particles_create (&ps->pl, R.sim, np, ps->pos.data (), ps->id.data ()));
    if (ps->idlast) CHECK (gfship_particles_set_idlast (ps->pl, ps->idlast));
    if (ps->particulate) {
      CHECK (gfship_particles_set_particulate (ps->pl, ps->vel.data (), ps->mass.data (), ps->volume.data ()));
      /* gravity of GfsForceBuoy = the GfsSource intensities on U, V, W (compute_buoyancy_force) */
      CHECK (gfship_particles_set_forces (ps->pl, (int) ps->forces.size (), ps->forces.data (), R.source));
      for (size_t f = 0; f < ps->force_functions.size (); f++)
        if (!ps->force_functions[f].empty ())
          CHECK (gfship_particles_set_force_coefficient (ps->pl, (int) f, ps->force_functions[f].c_str ()));
    }
  }
  // GfsSourceParticulate: the kernel of its list, and <list>_Fx/_Fy/_Fz as velocity source (mac_value and
  // centered_value of the object, modules/particulatecommon.c:2029-2079)
  for (auto & sp : R.source_particulates) {
    CHECK (gfship_particles_set_kernel (sp->ps->pl, sp->rkernel, sp->kernel.empty () ? nullptr : sp->kernel.c_str ()));
    gfship_field F[3] = { -1, -1, -1 };
    for (int c = 0; c < R.dim; c++) F[c] = R.vars[sp->fvar[c]].dev;
    CHECK (gfship_sim_set_source_fields (R.sim, F));
  }
  // GfsSourceParticulateVol / ...Mass: the function compiled for the device, with the device variables it names
  for (auto & sp : R.particulate_sources) {
    std::vector<const char *> names;
    std::vector<gfship_field> fields;
    for (const std::string & nm : sp->reads) {
      names.push_back (nm.c_str ());
      fields.push_back (R.vars[R.var_index (nm)].dev);
    }
    if (gfship_particulate_source_create (&sp->src, sp->ps->pl, sp->kind, sp->function.empty () ? nullptr : sp->function.c_str (),
                                          (int) names.size (), names.data (), fields.data ()) < 0) {
      fprintf (stderr, "gfship: line %d: %s\n", sp->line, gfship_last_error ());
      return 1;
    }
    gfship_field urel[3] = { -1, -1, -1 };
    for (int c = 0; c < R.dim; c++) urel[c] = R.vars[sp->urel[c]].dev;
    CHECK (gfship_particulate_source_set_fields (sp->src, R.vars[sp->rad].dev, urel,
                                                 sp->deposit >= 0 ? R.vars[sp->deposit].dev : -1));
  }
  // GfsFeedParticle: mass and volume compiled for the device, with the device variables they name
  for (auto & sp : R.feed_particles) {
    std::vector<const char *> names;
    std::vector<gfship_field> fields;
    for (const std::string & nm : sp->reads) {
      names.push_back (nm.c_str ());
      fields.push_back (R.vars[R.var_index (nm)].dev);
    }
    if (gfship_feed_particle_create (&sp->handle, sp->ps->pl, sp->mass.empty () ? nullptr : sp->mass.c_str (),
                                     sp->volume.empty () ? nullptr : sp->volume.c_str (), (int) names.size (),
                                     names.data (), fields.data ()) < 0) {
      fprintf (stderr, "gfship: line %d: %s\n", sp->line, gfship_last_error ());
      return 1;
    }
  }
  // GfsDropletToParticle: the function compiled for the device, with the device variables it names
  for (auto & sp : R.droplet_to_particles) {
    std::vector<const char *> names;
    std::vector<gfship_field> fields;
    for (const std::string & nm : sp->reads) {
      names.push_back (nm.c_str ());
      fields.push_back (R.vars[R.var_index (nm)].dev);
    }
    if (gfship_droplet_to_particle_create (&sp->handle, sp->ps->pl, R.vars[sp->c].dev, sp->min, sp->reset, sp->density,
                                           sp->function.empty () ? nullptr : sp->function.c_str (), (int) names.size (),
                                           names.data (), fields.data ()) < 0) {
      fprintf (stderr, "gfship: line %d: %s\n", sp->line, gfship_last_error ());
      return 1;
    }
  }
  set_boundary_conditions (R);
  apply_init (R);
  for (auto & is : R.init_spectra) {
    gfship_init_spectra_params p = is.first;
    if (p.level < 0) p.level = R.level;
    gfship_field v[3];
    for (int c = 0; c < 3; c++) {
      int q = R.var_index (is.second[c]);
      if (q < 0 || R.vars[q].dev < 0) {
        fprintf (stderr, "gfship: GfsInitSpectra: `%s' is not a variable of the simulation\n", is.second[c].c_str ());
        return 1;
      }
      v[c] = R.vars[q].dev;
      R.vars[q].host_time = -1.;
    }
    CHECK (gfship_init_spectra (R.dom, &p, v));
  }
  return 0;
}

// the cell data the file came with (gfs_box_read -> ftt_cell_read_binary / ftt_cell_read +
// gfs_cell_read*, src/boundary.c:1925-1944): all levels of the variables of `variables = ...'
inline int read_cell_data (Run & R)
{
  if (R.snapshot.depth != R.level) {
    fprintf (stderr, "gfship: the cell data of the file is refined to level %d\n", R.snapshot.depth);
    return 1;
  }
  std::vector<gfship_field> f, tmp;
  std::vector<int> host_only;
  for (const std::string & nm : R.snapshot.variables) {
    int q = R.get_or_add_variable (nm);
    if (R.vars[q].dev >= 0) { f.push_back (R.vars[q].dev); R.vars[q].host_time = -1.; host_only.push_back (-1); }
    else {
      gfship_field t = gfship_field_alloc (R.dom, -1);
      CHECK (t);
      f.push_back (t); tmp.push_back (t); host_only.push_back (q);
    }
  }
  CHECK (gfship_snapshot_tree_read (R.dom, (int) f.size (), f.data (), R.snapshot.tree.data (),
                                    R.snapshot.tree.size ()));
  for (size_t k = 0; k < f.size (); k++)
    if (host_only[k] >= 0) {
      Variable & V = R.vars[host_only[k]];
      V.host.assign (R.total (), 0.);
      CHECK (gfship_field_download (R.dom, f[k], R.level, V.host.data ()));
    }
  for (gfship_field t : tmp) gfship_field_free (R.dom, t);
  R.snapshot.tree.clear ();
  if (R.sim_class == "Simulation")
    CHECK (gfship_sim_restart (R.sim, R.t, R.i));
  return 0;
}

// poisson_run, src/simulation.c:2213-2285 (P has a Dirichlet condition somewhere, or the
// mean of Div is removed by correct_div: only the Dirichlet case is supported here)
inline int run_poisson (Run & R, gfship_field div)
{
  gfship_field p = R.vars[R.var_index ("P")].dev;
  bool dirichlet = false;
  for (int d = 0; d < 2*R.dim; d++)
    if (R.bc[d].count ("P") && R.bc[d]["P"].kind == GFSHIP_BC_DIRICHLET) dirichlet = true;
  if (!dirichlet) { fprintf (stderr, "gfship: GfsPoisson needs a Dirichlet condition on P\n"); return 1; }
  gfship_field res = gfship_field_alloc (R.dom, -1), dia = gfship_field_alloc (R.dom, -1);
  CHECK (res); CHECK (dia);
  CHECK (gfship_bc (R.dom, p, p, R.level));
  gfship_multilevel_params * par = gfship_sim_approx_projection_params (R.sim);
  while (R.i < R.iend && R.t < R.end) {
    {
      /* correct_div with a Dirichlet condition: rescale_div only, div = Div*size*size*fraction
         (src/simulation.c:2156-2162,2170-2211) */
      const std::vector<double> & Div = host_of (R, R.var_index ("Div"));
      std::vector<double> scaled (R.total (), 0.);
      double size = 1./R.n ();
      for_each_cell (R, [&] (const Cell &, size_t c) { scaled[c] = Div[c]*(size*size*1.); });
      CHECK (gfship_field_upload (R.dom, div, R.level, scaled.data ()));
    }
    CHECK (gfship_poisson_coefficients (R.dom));
    for (int l = 0; l <= R.level; l++)
      CHECK (gfship_field_fill (R.dom, dia, l, 0.));
    CHECK (gfship_poisson_solve (R.dom, par, p, div, res, dia, 1.));
    R.t = 0.;         /* sim->time.t = sim->tnext, and tnext stays 0. (src/simulation.c:1014,2269) */
    R.i++;
    events_do (R);
  }
  return 0;
}

// variable_stream_function_event, src/variable.c:1041-1086: psi at the four corners of every
// leaf -> MAC velocities, centred velocities = means of the two faces, BC
inline void set_stream_function_velocity (Run & R)
{
  const int n = R.n ();
  std::vector<double> un[2], uc[2];
  for (int c = 0; c < 2; c++) { un[c].assign (R.total (), 0.); uc[c].assign (R.total (), 0.); }
  for (int j = 1; j <= n; j++)
    for (int i = 1; i <= n; i++) {
      double o[3], p[3] = { 0., 0., 0. };
      cell_pos (R, Cell { i, j, 0, R.level }, o);
      double h = (1./n)/2.;
      p[0] = o[0] - h; p[1] = o[1] - h; double psi0 = eval (R, R.stream_function, p, -1);
      p[0] = o[0] + h; p[1] = o[1] - h; double psi1 = eval (R, R.stream_function, p, -1);
      p[0] = o[0] + h; p[1] = o[1] + h; double psi2 = eval (R, R.stream_function, p, -1);
      p[0] = o[0] - h; p[1] = o[1] + h; double psi3 = eval (R, R.stream_function, p, -1);
      double hh = 2.*h;
      double f0 = (psi2 - psi1)*1./hh, f1 = (psi3 - psi0)*1./hh;
      double f2 = (psi3 - psi2)*1./hh, f3 = (psi0 - psi1)*1./hh;
      un[0][R.idx (i, j, 0)] = f0;
      if (i == 1) un[0][R.idx (0, j, 0)] = f1;
      un[1][R.idx (i, j, 0)] = f2;
      if (j == 1) un[1][R.idx (i, 0, 0)] = f3;
      uc[0][R.idx (i, j, 0)] = (f0 + f1)/2.;
      uc[1][R.idx (i, j, 0)] = (f2 + f3)/2.;
    }
  for (int c = 0; c < 2; c++) {
    gfship_field fu = R.velocity (c).dev;
    CHECK (gfship_field_upload (R.dom, gfship_sim_variable (R.sim, GFSHIP_VAR_UN, c), R.level, un[c].data ()));
    CHECK (gfship_field_upload (R.dom, fu, R.level, uc[c].data ()));
    CHECK (gfship_bc (R.dom, fu, fu, R.level));
    R.velocity (c).host_time = -1.;
  }
}

// advection_run, src/simulation.c:2061-2116, with the velocity of a GfsVariableStreamFunction.
// Without one the velocity stays the zeros of a fresh simulation; that is accepted where no tracer
// reads it (every GfsVariableTracer has scheme = none: test/diffusion).  advection_run ignores the
// default scheme (:2078), so min_cfl (:1537-1554) is then G_MAXDOUBLE and the step is G_MAXINT, cut by
// dtmax and the events.
inline int run_advection (Run & R)
{
  bool advected = false;
  for (const TracerSpec & tr : R.tracers) advected = advected || tr.scheme == GFSHIP_SCHEME_GODUNOV;
  if (!R.stream_function && advected) {
    fprintf (stderr, "gfship: GfsAdvection needs a GfsVariableStreamFunction (prescribed velocity)\n");
    return 1;
  }
  if (!advected)
    gfship_sim_advection_params (R.sim)->cfl = DBL_MAX;
  if (R.stream_function)
    set_stream_function_velocity (R);
  CHECK (gfship_sim_set_time (R.sim, R.end, R.dtmax));
  CHECK (gfship_sim_set_next_event (R.sim, next_event_hook, &R));
  for (const TracerSpec & tr : R.tracers) {
    gfship_field ft = R.vars[R.var_index (tr.name)].dev;
    CHECK (gfship_bc (R.dom, ft, ft, R.level));
  }
  while (R.t < R.end && R.i < R.iend) {
    events_do (R);
    CHECK (gfship_sim_set_time (R.sim, R.end, R.dtmax));
    CHECK (gfship_sim_advection_step (R.sim));
    R.t = gfship_sim_time (R.sim);
    R.i = gfship_sim_iter (R.sim);
  }
  events_do (R);
  return 0;
}

// simulation_run, src/simulation.c:432-557
inline int run_simulation (Run & R)
{
  CHECK (gfship_sim_set_time (R.sim, R.end, R.dtmax));
  CHECK (gfship_sim_set_next_event (R.sim, next_event_hook, &R));
  if (refresh_alpha (R)) return 1;
  if (refresh_alpha_cell (R) || refresh_viscosity (R)) return 1;
  CHECK (gfship_sim_start (R.sim));
  if (R.alpha && !R.alpha_static) invalidate_device_copies (R);   /* the half step of the tracers */
  while (R.t < R.end && R.i < R.iend) {
    events_do (R);
    /* a GfsEventStop may just have set time.end = time.t: the reference still completes this
       iteration of the loop and stops at the next test of its condition */
    CHECK (gfship_sim_set_time (R.sim, R.end, R.dtmax));
    if (refresh_alpha (R)) return 1;
    if (refresh_alpha_cell (R) || refresh_viscosity (R)) return 1;
    CHECK (gfship_sim_step (R.sim));
    R.t = gfship_sim_time (R.sim);
    R.i = gfship_sim_iter (R.sim);
  }
  events_do (R);
  return 0;
}

// --particles FILE: the lists as gfs_event_list_write / gfs_particle_write / gfs_particulate_write print them
// (src/event.c:2508-2524, src/particle.c:88-99, modules/particulatecommon.c:907-921)
inline int write_particles (Run & R)
{
  FILE * fp = fopen (R.particles_out.c_str (), "w");
  if (!fp) { fprintf (stderr, "gfship: cannot open `%s'\n", R.particles_out.c_str ()); return 1; }
  for (auto & ps : R.plists) {
    int m = gfship_particles_slots (ps->pl);
    CHECK (m);
    std::vector<double> pos (3*(size_t) std::max (m, 1)), vel (pos.size ()), force (pos.size ()), mass (std::max (m, 1)),
      volume (std::max (m, 1));
    std::vector<unsigned> id (std::max (m, 1));
    int k = gfship_particles_download (ps->pl, pos.data (), id.data ());
    CHECK (k);
    if (ps->particulate) {
      CHECK (gfship_particles_download_particulate (ps->pl, vel.data (), mass.data (), force.data ()));
      CHECK (gfship_particles_download_volume (ps->pl, volume.data ()));      /* a GfsSourceParticulateVol changes them */
    }
    fprintf (fp, "GfsParticleList %s {\n", ps->particulate ? "GfsParticulate" : "GfsParticle");
    for (int q = 0; q < k; q++) {
      fprintf (fp, "    %s %d %g %g %g", ps->particulate ? "GfsParticulate" : "GfsParticle", (int) id[q],
               pos[3*q], pos[3*q + 1], pos[3*q + 2]);
      if (ps->particulate) {
        fprintf (fp, " %g %g %g %g %g", mass[q], volume[q], vel[3*q], vel[3*q + 1], vel[3*q + 2]);
        fprintf (fp, " %g %g %g", force[3*q], force[3*q + 1], force[3*q + 2]);
      }
      fputc ('\n', fp);
    }
    fputs ("}\n", fp);
  }
  fclose (fp);
  return 0;
}

// The three time loops (run_tree, run_advection, run_simulation) stay written out: they differ in the calls
// around the step, and one loop taking those as a callable came out no shorter and less plain than the three.
inline int run (Run & R)
{
  R.clock0 = std::chrono::steady_clock::now ();
  /* the functions of the file are compiled (a child `cc') before anything touches the GPU: a file
     whose functions do not compile exits here without a device context or handles left behind */
  add_derived (R);
  R.functions.resolve (R.var_names ());
  resolve_refine (R);
  if (check_run (R)) return 1;
  if (R.tree_mode)
    return run_tree (R);
  open_pipes (R);
  gfship_field div = -1;
  if (create_simulation (R, div)) return 1;
  if (R.snapshot.has_tree && read_cell_data (R)) return 1;
  events_init (R);
  if (R.sim_class == "Poisson" ? run_poisson (R, div) :
      R.sim_class == "Advection" ? run_advection (R) : run_simulation (R))
    return 1;
  if (!R.particles_out.empty () && write_particles (R)) return 1;
  for (auto & sp : R.particulate_sources) gfship_particulate_source_destroy (sp->src);
  for (auto & sp : R.feed_particles) gfship_feed_particle_destroy (sp->handle);
  for (auto & sp : R.droplet_to_particles) gfship_droplet_to_particle_destroy (sp->handle);
  for (auto & ps : R.plists) gfship_particles_destroy (ps->pl);
  for (auto & o : R.outputs) o->close ();
  gfship_sim_destroy (R.sim);
  gfship_domain_destroy (R.dom);
  return 0;
}

} // namespace gfs
