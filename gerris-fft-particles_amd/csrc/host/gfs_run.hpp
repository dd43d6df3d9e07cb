// gfs_run.hpp -- the model of a run of the .gfs front end (gfsrun.cpp) and its host copies of the fields.
//
// What a simulation file turns into before a device exists: the variables, the events with their outputs, the
// specifications of tracers, particle lists and sources, all in `Run'; and the helpers everything else stands
// on: the host copy of a variable, a GfsFunction at a cell, the loop over the leaf cells, the position and the
// volume of a cell, and the gather / scatter between the levels of a refined tree and one value per leaf.
// One translation unit includes this, then gfs_classes.hpp (the classes of the file) and gfs_drive.hpp (the run).
#pragma once
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <functional>
#include <sstream>
#include <fcntl.h>
#include <sys/types.h>
#include <sys/wait.h>
#include <unistd.h>
#include "gfship.h"
#include "gfs_text.hpp"
#include "gfs_snapshot.hpp"
#include <unordered_map>
#include "gfs_function.hpp"

#define CHECK(call) do { int rc_ = (call); if (rc_ < 0) {			\
      fprintf (stderr, "gfship: %s failed: %s\n", #call, gfship_last_error ()); exit (1); } } while (0)

namespace gfs {

// what an event action says when the library refuses: the library's own message
[[noreturn]] inline void die_last_error ()
{
  fprintf (stderr, "gfship: %s\n", gfship_last_error ());
  exit (1);
}
inline void must (int rc) { if (rc != GFSHIP_OK) die_last_error (); }

inline const char * const side_name[6] = { "right", "left", "top", "bottom", "front", "back" };
inline const char * const velocity_name[3] = { "U", "V", "W" };

// ---- variables: the reference's domain->variables list (P, Pmac, U, V[, W], then the ones the file
// adds).  Device variables live in libgfship; the others are host arrays used by Init, outputs
// and EventStop only.
struct Variable {
  std::string name;
  gfship_field dev = -1;          // -1: host only
  std::vector<double> host;       // (n+2)^dim with ghosts, [k][j][i]
  double host_time = -1.;         // simulation step the host copy of a device variable is from
  std::function<void (Variable &)> derive;   // derived variables (Velocity, Divergence ...)
};

struct Event {                     // GfsEvent, src/event.c:60-169
  double t = 0., start = 0., end = DBL_MAX, step = DBL_MAX;
  unsigned i = 0, istart = 0, iend = INT_MAX, istep = INT_MAX;
  unsigned n = 0;
  bool end_event = false, realised = false, dead = false;
  std::string cls;
  int line = 0;
  std::function<void ()> action;
};

// Shell commands of the file (GfsEventScript) run in a helper process forked at program start, before
// anything touches the GPU: a process that has initialised the device never forks or execs.  The
// helper reads { length, script } records and answers with the status of system ().
struct ShellServer {
  int to = -1, from = -1;
  pid_t pid = -1;
  void start () {
    int a[2], b[2];
    if (pipe (a) != 0 || pipe (b) != 0) return;
    fflush (stdout); fflush (stderr);
    pid = fork ();
    if (pid == 0) {
      ::close (a[1]); ::close (b[0]);
      for (;;) {
        size_t len = 0;
        if (read (a[0], &len, sizeof (len)) != (ssize_t) sizeof (len)) _exit (0);
        std::string script (len, '\0');
        size_t got = 0;
        while (got < len) {
          ssize_t q = read (a[0], &script[got], len - got);
          if (q <= 0) _exit (0);
          got += (size_t) q;
        }
        int status = system (script.c_str ());
        if (write (b[1], &status, sizeof (status)) != (ssize_t) sizeof (status)) _exit (0);
      }
    }
    ::close (a[0]); ::close (b[1]);
    if (pid < 0) { ::close (a[1]); ::close (b[0]); return; }
    to = a[1]; from = b[0];
    fcntl (to, F_SETFD, FD_CLOEXEC); fcntl (from, F_SETFD, FD_CLOEXEC);
  }
  int run (const std::string & script) {
    if (to < 0) return -1;
    size_t len = script.size ();
    int status = -1;
    if (write (to, &len, sizeof (len)) != (ssize_t) sizeof (len) ||
        write (to, script.data (), len) != (ssize_t) len ||
        read (from, &status, sizeof (status)) != (ssize_t) sizeof (status))
      return -1;
    return status;
  }
  void stop () {
    if (to >= 0) { ::close (to); ::close (from); to = from = -1; }
    if (pid > 0) { int st; waitpid (pid, &st, 0); pid = -1; }
  }
};
inline ShellServer g_shell;

struct Output {                    // GfsOutput, src/output.c:143-212
  std::string format;             // stdout, stderr, a file name or a { shell script }
  FILE * fp = nullptr;
  bool pipe = false;
  FILE * open () {
    if (fp) return fp;
    if (format == "stdout") fp = stdout;
    else if (format == "stderr") fp = stderr;
    else if (!format.empty () && format[0] == '{') {
      std::string script = format.substr (1, format.size () - 2);
      fflush (stdout);
      fp = popen (script.c_str (), "w");
      pipe = true;
    }
    else
      fp = fopen (format.c_str (), "w");
    if (!fp) { fprintf (stderr, "gfship: cannot open output `%s'\n", format.c_str ()); exit (1); }
    return fp;
  }
  void close () {
    if (!fp) return;
    if (pipe) pclose (fp);
    else if (fp != stdout && fp != stderr) fclose (fp);
    else fflush (fp);
    fp = nullptr;
  }
};

struct BcSpec { int kind = GFSHIP_BC_SYMMETRY; Function * val = nullptr; };

// GfsVariableTracer { gradient = .. scheme = godunov | none }, and the GfsSourceDiffusion on it: the constant,
// the line it stands on (0: none), its GfsMultilevelParams
struct TracerSpec {
  std::string name;
  int gradient = 1;                              // 0 gfs_center_gradient, 1 van Leer (default)
  int scheme = GFSHIP_SCHEME_GODUNOV;
  double D = 0.;
  int D_line = 0;
  std::map<std::string, std::string> diff_set;
};

// GfsParticleList (modules/particulatecommon.c:980-1093) of GfsParticle (src/particle.c:46-99) or
// GfsParticulate (:844-905) objects, with the list's GfsParticleForce objects
struct ParticleSpec {
  bool particulate = false;
  std::vector<unsigned> id;
  std::vector<double> pos, vel, mass, volume;    // 3 per particle for pos / vel
  std::vector<int> forces;                       // GFSHIP_FORCE_* in file order
  std::vector<std::string> force_functions;      // the GfsFunction of a GfsForceCoeff ("" = none)
  std::string name;                              // the optional `*name' of the event (gfs_event_read, src/event.c:198-203)
  int line = 0;                                  // of the GfsParticleList in the file
  int idlast = 0;                                // the integer that may end the list (:1087-1090)
  gfship_particles * pl = nullptr;
};

// GfsSourceParticulate (modules/particulatecommon.c:2230-2350): the list, rkernel, the text of kernel and
// the variables <list>_Fx, _Fy[, _Fz]
struct SourceParticulateSpec {
  ParticleSpec * ps = nullptr;
  double rkernel = 0.;
  std::string kernel;                            // "" = the constant 0 of source_particulate_init
  int fvar[3] = { -1, -1, -1 };
};

// GfsSourceParticulateVol / GfsSourceParticulateMass (modules/particulatecommon.c:2734-3047): the list, the text
// of the function with the variables of the run it names, and the variables Rad, Urelp, Vrelp[, Wrelp] and the
// optional deposit variable (-1: none), all kept on the device
struct ParticulateSourceSpec {
  ParticleSpec * ps = nullptr;
  int kind = GFSHIP_PARTICULATE_SOURCE_VOLUME;
  int line = 0;
  std::string function;                          // "" = the constant 0 of source_particulatevol_init
  std::vector<std::string> reads;
  int rad = -1, urel[3] = { -1, -1, -1 }, deposit = -1;
  gfship_particulate_source * src = nullptr;
};

// GfsFeedParticle (modules/particulatecommon.c:2375-2647): the list, the host functions nparts, xfeed, yfeed, zfeed
// (nullptr: the default of gfs_feed_particle_init, 1 for nparts and 0 for the others) and the texts of mass and
// volume with the device variables they name
struct FeedParticleSpec {
  ParticleSpec * ps = nullptr;
  int line = 0;
  Function * np = nullptr, * feed[3] = { nullptr, nullptr, nullptr };
  std::string mass, volume;                      // "" = the constant 0
  std::vector<std::string> reads;
  gfship_feed_particle * handle = nullptr;
};

// GfsDropletToParticle (modules/particulatecommon.c:1163-1527): the list, the variable, min, reset and density
// (gfs_droplet_to_particle_init, :1492-1497), and the text of the optional function with the device variables it
// names
struct DropletToParticleSpec {
  ParticleSpec * ps = nullptr;
  int line = 0;
  int c = -1;                                    // the variable
  int min = 20;
  double reset = 0., density = 1.;
  std::string function;                          // "" = none
  std::vector<std::string> reads;
  gfship_droplet_to_particle * handle = nullptr;
};

// a cell: its indices on its level (1..2^l inside the box; k = 0 in 2-D)
struct Cell { int i, j, k, l; };

struct Run {
  int dim = 2, level = 0, device = 0;
  std::string sim_class = "Simulation";
  int side[6] = { GFSHIP_SIDE_BOUNDARY, GFSHIP_SIDE_BOUNDARY, GFSHIP_SIDE_BOUNDARY,
                  GFSHIP_SIDE_BOUNDARY, GFSHIP_SIDE_BOUNDARY, GFSHIP_SIDE_BOUNDARY };
  std::map<std::string, BcSpec> bc[6];       // per side: variable name -> condition
  // GfsTime, src/simulation.c:1660-1670
  double t = 0., end = DBL_MAX, dtmax = DBL_MAX;
  unsigned i = 0, iend = INT_MAX;
  std::map<std::string, std::string> proj_set, approx_set, adv_set;
  double visc[3] = { 0., 0., 0. };
  // GfsSourceDiffusion / GfsSourceViscosity with a GfsFunction of x, y, z, t: evaluated at the face centres
  // (diffusion_face, src/source.c:933-939) before every step unless it does not depend on t
  Function * visc_fn[3] = { nullptr, nullptr, nullptr };
  int visc_line[3] = { 0, 0, 0 };
  gfship_field visc_dev[3][3] = { { -1, -1, -1 }, { -1, -1, -1 }, { -1, -1, -1 } };
  gfship_field alpha_cell_dev = -1;      // alpha at the cell centres of every level (with a viscosity or particle forces)
  double alpha_cell_t = 0., mu_cell_t = 0.;   // the time alpha_cell_dev and mu_cell_dev were last evaluated at
  gfship_field mu_cell_dev = -1;         // the viscosity function of U at the leaf centres (with particle forces)
  bool has_viscosity (int c) const { return visc[c] != 0. || visc_fn[c] != nullptr; }
  std::map<std::string, std::string> diff_set[3];
  std::vector<TracerSpec> tracers;
  TracerSpec * tracer (const std::string & name) {
    for (TracerSpec & tr : tracers) if (tr.name == name) return &tr;
    return nullptr;
  }
  Function * stream_function = nullptr;          // GfsVariableStreamFunction (2-D, GfsAdvection)
  std::vector<std::pair<std::string, Function *>> init;   // Init {} { var = f }
  double source[3] = { 0., 0., 0. };    // GfsSource intensities on U, V, W
  // GfsPhysicalParams { alpha = f }: the inverse of the density, a function of x, y, z, t and tracers,
  // evaluated on the faces before every step (gfs_function_face_value, src/utils.c:1268-1297)
  Function * alpha = nullptr;
  int alpha_line = 0;
  gfship_field alpha_dev[3] = { -1, -1, -1 };
  bool alpha_static = false;             // no variable and no t in it: evaluated once
  std::vector<Variable> vars;
  std::vector<std::string> device_vars;   // variables of the file that live on the device (GfsVariableTurbulentViscosity)
  std::vector<std::unique_ptr<Event>> events;
  std::vector<std::unique_ptr<Output>> outputs;
  std::vector<std::unique_ptr<ParticleSpec>> plists;
  std::vector<std::unique_ptr<SourceParticulateSpec>> source_particulates;
  std::vector<std::unique_ptr<ParticulateSourceSpec>> particulate_sources;
  std::vector<std::unique_ptr<FeedParticleSpec>> feed_particles;
  std::vector<std::unique_ptr<DropletToParticleSpec>> droplet_to_particles;
  // a variable of the file that is kept on the device: those of the simulation, the tracers and device_vars
  bool on_device (const std::string & name) const {
    if (name == "P" || name == "Pmac" || velocity_component (name) >= 0) return true;
    for (const TracerSpec & tr : tracers) if (tr.name == name) return true;
    return std::find (device_vars.begin (), device_vars.end (), name) != device_vars.end ();
  }
  ParticleSpec * plist_by_name (const std::string & name) const {
    for (auto & ps : plists) if (!ps->name.empty () && ps->name == name) return ps.get ();
    return nullptr;
  }
  bool particulate_forces () const {      // a list of GfsParticulate with GfsParticleForce objects
    for (auto & ps : plists) if (!ps->forces.empty ()) return true;
    return false;
  }
  std::vector<std::pair<gfship_init_spectra_params, std::vector<std::string>>> init_spectra;
  std::string particles_out;                     // --particles FILE: the lists at the end of the run
  Function * refine_fn = nullptr;                // GfsRefine given as a function
  int refine_line = 0;
  // the text of the file, kept to write it back (GfsOutputSimulation): objects of the body, the
  // parameters of the GfsBox, the edges; and the cell data the file came with (a snapshot)
  std::vector<std::pair<std::string, std::string>> object_texts;   // class, text
  std::string box_text, edges_text;
  int nedges = 0;
  gfs::SimulationFile snapshot;
  FunctionSet functions;
  gfship_domain * dom = nullptr;
  gfship_sim * sim = nullptr;
  // a Refine function that asks for a non-uniform tree (one periodic box): gfship_tree.  The
  // host copy of a variable is then one value per leaf, the leaves in the order of
  // ftt_cell_traverse (src/ftt.c:689-926)
  bool tree_mode = false;
  gfship_tree * tree = nullptr;
  std::vector<Cell> leaves;
  size_t level_index (const Cell & c) const {
    size_t r = (1 << c.l) + 2;
    return c.i + r*(c.j + (dim == 3 ? r*(size_t) c.k : 0));
  }
  size_t level_size (int l) const { size_t r = (1 << l) + 2; return dim == 3 ? r*r*r : r*r; }
  std::chrono::steady_clock::time_point clock0;

  int n () const { return 1 << level; }
  size_t total () const { return tree_mode ? leaves.size () : level_size (level); }
  size_t idx (int i, int j, int k) const { return level_index (Cell { i, j, k, level }); }
  int var_index (const std::string & name) const {
    for (size_t q = 0; q < vars.size (); q++)
      if (vars[q].name == name) return (int) q;
    return -1;
  }
  int get_or_add_variable (const std::string & name) {
    int v = var_index (name);
    if (v >= 0) return v;
    Variable nv;
    nv.name = name;
    vars.push_back (nv);
    return (int) vars.size () - 1;
  }
  std::vector<std::string> var_names () const {
    std::vector<std::string> r;
    for (const Variable & v : vars) r.push_back (v.name);
    return r;
  }
  // the velocity: the component a name stands for (-1: none; W in 3-D only), and the variable of a component
  int velocity_var (int c) const { return var_index (velocity_name[c]); }
  int velocity_component (const std::string & name) const {
    for (int c = 0; c < dim; c++) if (name == velocity_name[c]) return c;
    return -1;
  }
  Variable & velocity (int c) { return vars[velocity_var (c)]; }
};

inline bool depends_on_t (const Function * f) { return f->kind == Function::COMPILED && f->uses_t; }

// ---- a refined tree: the levels of a device variable <-> one value per leaf; the flags of the cells
inline void tree_gather (Run & R, int var, std::vector<double> & leaf)
{
  std::vector<std::vector<double>> lev (gfship_tree_depth (R.tree) + 1);
  for (size_t c = 0; c < R.leaves.size (); c++) {
    int l = R.leaves[c].l;
    if (lev[l].empty ()) {          /* a level is downloaded once */
      lev[l].resize (R.level_size (l));
      CHECK (gfship_tree_download (R.tree, var, l, lev[l].data ()));
    }
    leaf[c] = lev[l][R.level_index (R.leaves[c])];
  }
}

inline void tree_scatter (Run & R, int var, const std::vector<double> & leaf)
{
  int depth = gfship_tree_depth (R.tree);
  for (int l = 0; l <= depth; l++) {
    std::vector<double> lev (R.level_size (l), 0.);
    bool any = false;
    for (size_t c = 0; c < R.leaves.size (); c++)
      if (R.leaves[c].l == l) { lev[R.level_index (R.leaves[c])] = leaf[c]; any = true; }
    if (any)
      CHECK (gfship_tree_upload (R.tree, var, l, lev.data ()));
  }
}

inline std::vector<std::vector<unsigned char>> tree_flags (Run & R)
{
  int depth = gfship_tree_depth (R.tree);
  std::vector<std::vector<unsigned char>> flag (depth + 1);
  for (int l = 0; l <= depth; l++) {
    flag[l].resize (R.level_size (l));
    CHECK (gfship_tree_flags (R.tree, l, flag[l].data ()));
  }
  return flag;
}

// ---- host copies of the fields
inline std::vector<double> & host_of (Run & R, int v)
{
  Variable & V = R.vars[v];
  const bool stale = V.host.size () != R.total () || V.host_time != (double) R.i;
  if (V.dev >= 0) {
    if (stale) {
      V.host.resize (R.total ());
      if (R.tree_mode) tree_gather (R, V.dev, V.host);
      else CHECK (gfship_field_download (R.dom, V.dev, R.level, V.host.data ()));
      V.host_time = (double) R.i;
    }
  }
  else if (V.derive) {
    if (stale) {
      V.host.assign (R.total (), 0.);
      V.derive (V);
      V.host_time = (double) R.i;
    }
  }
  else if (V.host.size () != R.total ())
    V.host.assign (R.total (), 0.);
  return V.host;
}

inline void invalidate_device_copies (Run & R)
{
  for (Variable & V : R.vars)
    if (V.dev >= 0 || V.derive)
      V.host_time = -1.;
}

// ftt_cell_pos on the unit box centred on the origin, src/ftt.c:349-367
inline void cell_pos (const Run & R, const Cell & c, double p[3])
{
  double h = 1./(1 << c.l);
  p[0] = -0.5 + (c.i - 0.5)*h;
  p[1] = -0.5 + (c.j - 0.5)*h;
  p[2] = R.dim == 3 ? -0.5 + (c.k - 0.5)*h : 0.;
}

// gfs_cell_volume
inline double cell_volume (const Run & R, const Cell & c)
{
  double h = 1./(1 << c.l);
  return R.dim == 3 ? h*h*h : h*h;
}

inline double eval (Run & R, const Function * f, const double p[3], long cell)
{
  switch (f->kind) {
  case Function::CONSTANT: return f->val;
  case Function::VARIABLE:
    if (cell < 0) { fprintf (stderr, "gfship: a variable cannot be used in a boundary value\n"); exit (1); }
    return host_of (R, f->var)[cell];
  case Function::COMPILED: {
    double v[32];
    if (f->args.size () > 32) { fprintf (stderr, "gfship: too many variables in a function\n"); exit (1); }
    for (size_t q = 0; q < f->args.size (); q++) {
      if (cell < 0) { fprintf (stderr, "gfship: a variable cannot be used in a boundary value\n"); exit (1); }
      v[q] = host_of (R, f->args[q])[cell];
    }
    return f->fn (p[0], p[1], p[2], R.t, v);
  }
  default: break;
  }
  fprintf (stderr, "gfship: unresolved function\n");
  exit (1);
}

// the leaf cells, each with its index in the host copy of a variable
template <class F> void for_each_cell (const Run & R, F f)
{
  if (R.tree_mode) {
    for (size_t c = 0; c < R.leaves.size (); c++)
      f (R.leaves[c], c);
    return;
  }
  int n = R.n ();
  for (int k = 1; k <= (R.dim == 3 ? n : 1); k++)
    for (int j = 1; j <= n; j++)
      for (int i = 1; i <= n; i++) {
        Cell c = { i, j, R.dim == 3 ? k : 0, R.level };
        f (c, R.level_index (c));
      }
}

// a GfsFunction on every leaf cell
inline std::vector<double> function_values (Run & R, const Function * f)
{
  std::vector<double> a (R.total (), 0.);
  for_each_cell (R, [&] (const Cell & cell, size_t c) {
    double p[3];
    cell_pos (R, cell, p);
    a[c] = eval (R, f, p, (long) c);
  });
  return a;
}

// gfs_domain_norm_variable with volume weights, src/domain.c:2197-2232, fluid.c:2139-2171
inline gfship_norm norm_of (const Run & R, const std::vector<double> & a)
{
  gfship_norm nm = { 0., 0., 0., 0., 0. };
  for_each_cell (R, [&] (const Cell & cell, size_t c) {
    double w = cell_volume (R, cell), val = a[c];
    nm.bias += w*val;
    val = fabs (val);
    if (val > nm.infty) nm.infty = val;
    nm.first += w*val;
    nm.second += w*val*val;
    nm.w += w;
  });
  if (nm.w > 0.) {
    nm.bias /= nm.w;
    nm.first /= nm.w;
    nm.second = sqrt (nm.second/nm.w);
  }
  else
    nm.infty = 0.;
  return nm;
}

// defined in gfs_drive.hpp, used by the actions of gfs_classes.hpp
inline int refresh_alpha_cell (Run & R); /* the fields of the fluid an event of a list with forces reads */
inline int refresh_viscosity_cell (Run & R);
inline void write_simulation (Run & R, FILE * fp, const std::vector<int> & list, bool binary);

} // namespace gfs
