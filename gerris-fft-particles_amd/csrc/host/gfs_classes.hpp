// gfs_classes.hpp -- the classes of a simulation file the front end knows: one reader per class or family of
// classes, and the table that names them (class_table, at the end: THE list of what is supported).
//
// A reader takes the text of its object from the Reader, in the order the reference reads it, and leaves what
// it found in the Run; the reader of an event class also sets the action of the event, which is all that later
// talks to the device.  parse_object builds what the event classes share -- the event, its parameters, its
// output -- as the row of the table says, calls the reader, adds the event and checks that the object ends.
#pragma once
#include "gfs_run.hpp"

namespace gfs {

// the { block } that comes next, as a reader of its own: its messages name the line in the file
inline Reader block (Reader & r)
{
  int l0 = r.line ();
  return Reader (r.braces (), "simulation file", l0);
}

inline void read_event_params (Reader & r, Event & e)
{
  // gfs_event_read, src/event.c:171-300
  if (r.peek (false) != '{') return;
  auto m = r.assignments ();
  bool set_start = m.count ("start"), set_end = m.count ("end"), set_step = m.count ("step"),
    set_istart = m.count ("istart"), set_iend = m.count ("iend"), set_istep = m.count ("istep");
  for (auto & kv : m)
    if (kv.first != "start" && kv.first != "end" && kv.first != "step" && kv.first != "istart" &&
        kv.first != "iend" && kv.first != "istep")
      r.fail ("unknown event parameter `" + kv.first + "'");
  if (set_end) e.end = atof (m["end"].c_str ());
  if (set_step) e.step = atof (m["step"].c_str ());
  if (set_istart) e.istart = (unsigned) atol (m["istart"].c_str ());
  if (set_iend) e.iend = (unsigned) atol (m["iend"].c_str ());
  if (set_istep) e.istep = (unsigned) atol (m["istep"].c_str ());
  if (set_start) {
    if (m["start"] == "end") {
      e.end_event = true;
      if (set_end || set_step || set_istart || set_iend || set_istep)
        r.fail ("no other parameter can be set for an `end' event");
    }
    else
      e.start = atof (m["start"].c_str ());
  }
  if (set_step && set_istep) r.fail ("step and istep cannot be set simultaneously");
  if (set_step) e.istep = INT_MAX;
  if (set_step && e.step <= 0.) r.fail ("step must be strictly positive");
  if (!set_step && !set_istep && set_end) r.fail ("expecting a number (step or istep)");
  if (set_end && e.end <= e.start) r.fail ("end must be larger than start");
  if (e.start < 0. && set_step) e.start = 0.;
  if (set_start || !set_istart) e.t = e.start;
  else e.t = e.start = DBL_MAX/2.;
  if (!set_istep && !set_step && set_iend) r.fail ("expecting a number (istep or step)");
  if (set_istart && e.iend <= e.istart) r.fail ("iend must be larger than istart");
  if (set_istart || !set_start) e.i = e.istart;
  else e.i = e.istart = INT_MAX/2;
}

inline void read_multilevel (Reader & r, std::map<std::string, std::string> & set)
{
  // gfs_multilevel_params_read, src/poisson.c:70-126
  static const char * keys[] = { "tolerance", "nrelax", "erelax", "minlevel", "nitermax",
                                 "nitermin", "weighted", "beta", "omega", "function", nullptr };
  auto m = r.assignments ();
  for (auto & kv : m) {
    bool ok = false;
    for (const char ** k = keys; *k; k++) ok = ok || kv.first == *k;
    if (!ok) r.fail ("unknown keyword `" + kv.first + "'");
    set[kv.first] = kv.second;
  }
}

inline Output * read_output (Run & R, Reader & r)
{
  R.outputs.emplace_back (new Output);
  Output * o = R.outputs.back ().get ();
  if (r.peek (false) == '{')
    o->format = "{" + r.braces () + "}";
  else
    o->format = r.word (false);
  return o;
}

inline double rate (double a, double b, unsigned n)
{
  if (a > 0. && b > 0. && n > 0) return exp (log (b/a)/n);
  return 0.;
}

inline void stats_write (const gfship_multilevel_params * par, FILE * fp)
{
  // gfs_multilevel_params_stats_write, src/poisson.c:142-172
  fprintf (fp,
           "    niter: %4d\n"
           "    residual.bias:   % 10.3e % 10.3e\n"
           "    residual.first:  % 10.3e % 10.3e %6.2g\n"
           "    residual.second: % 10.3e % 10.3e %6.2g\n"
           "    residual.infty:  % 10.3e % 10.3e %6.2g\n",
           par->niter, par->residual_before.bias, par->residual.bias,
           par->residual_before.first, par->residual.first,
           rate (par->residual.first, par->residual_before.first, par->niter),
           par->residual_before.second, par->residual.second,
           rate (par->residual.second, par->residual_before.second, par->niter),
           par->residual_before.infty, par->residual.infty,
           rate (par->residual.infty, par->residual_before.infty, par->niter));
}

// the scalar of a GfsOutputScalar: { v = function ... }, src/output.c:1670-1830
struct ScalarSpec { Function * f = nullptr; std::string name; Function * w = nullptr; std::string format; };

inline ScalarSpec read_scalar (Run & R, Reader & r)
{
  ScalarSpec s;
  Reader b = block (r);
  while (!b.eof ()) {
    std::string k = b.word ();
    b.expect ('=');
    if (k == "v") {
      FunctionText t = b.function ();
      s.f = R.functions.add (t, b.line ());
      s.name = t.text;       /* gfs_function_description */
    }
    else if (k == "w")
      s.w = R.functions.add (b.function (), b.line ());
    else if (k == "format")
      s.format = b.word ();
    else if (k == "min" || k == "max" || k == "maxlevel")
      b.word ();
    else
      b.fail ("unsupported GfsOutputScalar keyword `" + k + "'");
  }
  if (!s.f) r.fail ("expecting `v = ...'");
  return s;
}

// the gradient functions of GfsAdvectionParams / GfsVariableTracer (src/advection.c:944-1032):
// gfs_center_gradient, and the limited gradients of src/fluid.c:522-690
inline int gradient_kind (const std::string & name)
{
  static const char * names[] = { "gfs_center_gradient", "gfs_center_van_leer_gradient",
                                  "gfs_center_minmod_gradient", "gfs_center_superbee_gradient",
                                  "gfs_center_sweby_gradient" };
  for (int k = 0; k < 5; k++)
    if (name == names[k]) return k;
  return -1;
}

// ---- the readers.  What parse_object hands them: the class as the file spells it (without Gfs), its line, and
// for the event classes the event (parameters read where the row says so) and the output
struct Object {
  std::string cls;
  int line = 0;
  Event * e = nullptr;
  Output * o = nullptr;
};

inline void read_time (Run & R, Reader & r, Object &)
{
  auto m = r.assignments ();
  for (auto & kv : m) {
    const char * v = kv.second.c_str ();
    if (kv.first == "t") R.t = atof (v);
    else if (kv.first == "i") R.i = (unsigned) atol (v);
    else if (kv.first == "end") R.end = atof (v);
    else if (kv.first == "iend") R.iend = (unsigned) atol (v);
    else if (kv.first == "dtmax") R.dtmax = atof (v);
    else r.fail ("unknown GfsTime keyword `" + kv.first + "'");
  }
}

inline void read_refine (Run & R, Reader & r, Object & ob)
{
  FunctionText t = r.function ();
  char * endp;
  long l = strtol (t.text.c_str (), &endp, 10);
  if (t.block || *endp != '\0') {
    // GfsRefine with a function of the position (refine_maxlevel, src/refine.c:34-43): accepted
    // when it asks for the same level everywhere (resolve_refine: e.g. test/periodic/periodic.gfs
    // with BOX = 0), or for a tree gfship_tree builds
    R.refine_fn = R.functions.add (t, ob.line);
    R.refine_line = ob.line;
  }
  else {
    if (l < 0 || l > GFSHIP_MAXLEVEL)
      r.fail ("Refine: level out of range (got `" + t.text + "')");
    R.level = (int) l;
  }
}

inline void read_gmodule (Run &, Reader & r, Object &)
{
  std::string name = r.word (false);
  if (r.peek (false) == '{') r.braces ();
  /* GfsParticleList / GfsParticulate / GfsForce*, the spectra and GfsInitSpectra are built in (libgfship) */
  if (name != "particulates" && name != "fft" && name != "turbulence")
    fprintf (stderr, "gfship: GModule %s ignored (the Poisson and diffusion solvers are libgfship's)\n",
             name.c_str ());
}

inline void read_projection_params (Run & R, Reader & r, Object & ob)
{
  read_multilevel (r, ob.cls == "ProjectionParams" ? R.proj_set : R.approx_set);
}

inline void read_advection_params (Run & R, Reader & r, Object &)
{
  auto m = r.assignments ();
  for (auto & kv : m)
    if (kv.first == "cfl" || kv.first == "gradient" || kv.first == "gc")
      R.adv_set[kv.first] = kv.second;
    else
      r.fail ("unsupported GfsAdvectionParams keyword `" + kv.first + "'");
}

inline void read_init (Run & R, Reader & r, Object &)
{
  Event e;
  read_event_params (r, e);
  Reader b = block (r);
  while (!b.eof ()) {
    std::string name = b.word ();
    b.expect ('=');
    Function * f = R.functions.add (b.function (), b.line ());
    R.get_or_add_variable (name);
    R.init.emplace_back (name, f);
  }
}

// GfsSourceDiffusion [{ event }] variable coefficient [{ multilevel }];  GfsSourceViscosity: the same on U, V[, W]
inline void read_source_diffusion (Run & R, Reader & r, Object & ob)
{
  Event e;
  read_event_params (r, e);
  std::vector<std::string> comps;
  if (ob.cls == "SourceDiffusion") comps.push_back (r.word (false));
  else comps.assign (velocity_name, velocity_name + R.dim);
  const int fline = r.line ();
  FunctionText t = r.function ();
  /* a number keeps the constant-coefficient path; anything else is a GfsFunction of x, y, z, t */
  const bool constant = !t.block && Reader::is_number (t.text);
  Function * fn = constant ? nullptr : R.functions.add (t, fline);
  std::map<std::string, std::string> par;
  if (r.peek (false) == '{') read_multilevel (r, par);
  for (const std::string & v : comps) {
    int c = R.velocity_component (v);
    TracerSpec * tr = R.tracer (v);
    if (c < 0 && ob.cls == "SourceDiffusion" && tr) {
      // GfsSourceDiffusion on a declared tracer (gfs_tracer_advection_diffusion, src/timestep.c:1039-1048):
      // a constant coefficient
      if (tr->D_line) {
        fprintf (stderr, "gfship: line %d: only one diffusion source can be specified for a given variable "
                 "(`%s' has one on line %d)\n", fline, v.c_str (), tr->D_line);     /* src/source.c:1047 */
        exit (1);
      }
      if (!constant) {
        fprintf (stderr, "gfship: line %d: the diffusion coefficient of a tracer must be a constant (got `%s' "
                 "for `%s')\n", fline, t.text.c_str (), v.c_str ());
        exit (1);
      }
      tr->D = atof (t.text.c_str ());
      tr->D_line = fline;
      tr->diff_set = par;
      continue;
    }
    if (c < 0) r.fail ("diffusion is supported on the velocity components only (got `" + v + "')");
    R.visc[c] = constant ? atof (t.text.c_str ()) : 0.;
    R.visc_fn[c] = fn;
    R.visc_line[c] = fline;
    R.diff_set[c] = par;
  }
}

inline void read_source (Run & R, Reader & r, Object &)
{
  // GfsSource [{ event }] U|V|W intensity (src/source.c:405-446): a constant intensity on a velocity
  // component
  Event e;
  read_event_params (r, e);
  std::string v = r.word (false);
  int c = R.velocity_component (v);
  if (c < 0) r.fail ("GfsSource is supported on the velocity components only (got `" + v + "')");
  FunctionText t = r.function ();
  if (t.block || !Reader::is_number (t.text))
    r.fail ("only a constant intensity is supported");
  R.source[c] += atof (t.text.c_str ());        /* several sources on a variable add up */
}

inline void read_physical_params (Run & R, Reader & r, Object &)
{
  // gfs_physical_params_read, src/simulation.c:1760-1835: g, L constants, alpha a GfsFunction
  Reader b = block (r);
  while (!b.eof ()) {
    std::string key = b.word ();
    b.expect ('=');
    if (key == "alpha") {
      R.alpha = R.functions.add (b.function (), b.line ());
      R.alpha_line = b.line ();
    }
    else if (key == "L" || key == "g") {
      FunctionText t = b.function ();
      if (t.block || !Reader::is_number (t.text) || atof (t.text.c_str ()) != 1.)
        b.fail ("GfsPhysicalParams: only " + key + " = 1 is supported (got `" + t.text + "')");
    }
    else
      b.fail ("unknown keyword `" + key + "'");
  }
}

inline void read_variable_tracer (Run & R, Reader & r, Object &)
{
  TracerSpec tr;
  tr.name = r.word (false);
  if (r.peek (false) == '{') {
    auto m = r.assignments ();
    for (auto & kv : m)
      if (kv.first == "gradient" && gradient_kind (kv.second) >= 0) tr.gradient = gradient_kind (kv.second);
      else if (kv.first == "scheme" && (kv.second == "godunov" || kv.second == "none"))
        tr.scheme = kv.second == "none" ? GFSHIP_SCHEME_NONE : GFSHIP_SCHEME_GODUNOV;    /* src/advection.c:1009-1018 */
      else
        r.fail ("unsupported GfsVariableTracer parameter " + kv.first + " = " + kv.second);
  }
  R.tracers.push_back (tr);
  R.get_or_add_variable (tr.name);
}

inline void read_variable_stream_function (Run & R, Reader & r, Object &)
{
  // GfsVariableStreamFunction name function (2-D; src/variable.c:905-1120)
  if (R.dim != 2) r.fail ("GfsVariableStreamFunction is 2-D only");
  Event e;
  read_event_params (r, e);
  std::string name = r.word (false);
  R.get_or_add_variable (name);
  R.stream_function = R.functions.add (r.function (), r.line ());
}

inline void read_event_stop (Run & R, Reader & r, Object & ob)
{
  // gfs_event_stop_read / _event, src/event.c:1737-1835
  std::string vname = r.word (false);
  double max = r.number ();
  std::string dname;
  if (!r.at_end_of_object ()) dname = r.word (false);
  int v = R.var_index (vname);
  if (v < 0) r.fail ("unknown variable `" + vname + "'");
  int dv = dname.empty () ? -1 : R.get_or_add_variable (dname);
  auto oldv = std::make_shared<std::vector<double>> ();
  auto last = std::make_shared<double> (-1.);
  ob.e->action = [&R, v, dv, max, oldv, last] () {
    const std::vector<double> & cur = host_of (R, v);
    if (*last >= 0.) {
      std::vector<double> d (R.total (), 0.);
      for_each_cell (R, [&] (const Cell &, size_t c) { d[c] = (*oldv)[c] - cur[c]; });
      gfship_norm nm = norm_of (R, d);
      if (nm.infty <= max)
        R.end = R.t;
      if (dv >= 0) R.vars[dv].host = d;
    }
    *oldv = cur;
    *last = R.t;
  };
}

// the objects of a GfsParticleList: GfsParticle id x y z | GfsParticulate id x y z mass volume u v w [fx fy fz]
inline void read_particles (Reader & b, const std::string & item, ParticleSpec * ps)
{
  auto numeric = [] (char c) { return (c >= '0' && c <= '9') || c == '-' || c == '+' || c == '.'; };
  bool first = true;
  while (!b.eof ()) {
    // every object starts with its class (gfs_event_read, src/event.c:171-196)
    std::string k = strip_gfs (b.word ());
    if (k != "Particle" && k != "Particulate")
      b.fail ("expecting GfsParticle or GfsParticulate in a GfsParticleList (got `" + k + "')");
    if (!item.empty () && k != item)
      b.fail ("the list holds Gfs" + item + " objects");
    bool particulate = k == "Particulate";
    if (!first && particulate != ps->particulate)
      b.fail ("mixed lists of GfsParticle and GfsParticulate are not supported");
    ps->particulate = particulate;
    first = false;
    if (b.peek (false) == '{') b.braces ();          /* per-object event parameters: the list's apply */
    ps->id.push_back ((unsigned) b.number ());
    for (int c = 0; c < 3; c++) ps->pos.push_back (b.number ());
    if (particulate) {
      ps->mass.push_back (b.number ());
      ps->volume.push_back (b.number ());           /* physical_params.L = 1 */
      for (int c = 0; c < 3; c++) ps->vel.push_back (b.number ());
      for (int c = 0; c < 3 && numeric (b.peek (false)); c++)
        b.number ();                                 /* force: recomputed at every event */
    }
  }
}

// the GfsParticleForce objects of a list
inline void read_particle_forces (Reader & b, ParticleSpec * ps)
{
  while (!b.eof ()) {
    std::string k = strip_gfs (b.word ());
    int kind = k == "ForceInertial" ? GFSHIP_FORCE_INERTIAL : k == "ForceAddedMass" ? GFSHIP_FORCE_ADDEDMASS :
      k == "ForceLift" ? GFSHIP_FORCE_LIFT : k == "ForceDrag" ? GFSHIP_FORCE_DRAG :
      k == "ForceBuoy" ? GFSHIP_FORCE_BUOY : 0;
    if (!kind) b.fail ("unsupported GfsParticleForce `" + k + "'");
    // gfs_force_coeff_read, modules/particulatecommon.c:189-207: what follows on the line is the
    // GfsFunction of the coefficient (variables Rep, Urelp, Vrelp, Wrelp, Pdia): compiled for the
    // device when the list is created
    std::string fn;
    char c = b.peek (false);
    if (c != 0 && c != '\n') {
      if (kind == GFSHIP_FORCE_INERTIAL || kind == GFSHIP_FORCE_BUOY)
        b.fail ("Gfs" + k + " takes no coefficient");
      fn = b.function ().text;
    }
    ps->forces.push_back (kind);
    ps->force_functions.push_back (fn);
  }
}

inline void read_particle_list (Run & R, Reader & r, Object & ob)
{
  // gfs_event_list_read (src/event.c:2446-2506) + gfs_particle_list_read
  // (modules/particulatecommon.c:1022-1093):
  //   GfsParticleList { event } [GfsParticle|GfsParticulate] { objects } [{ forces }] [idlast]
  std::string ename;
  if (r.peek (false) == '*') ename = r.word (false).substr (1);     /* optional name, src/event.c:198-203 */
  read_event_params (r, *ob.e);
  R.plists.emplace_back (new ParticleSpec);
  ParticleSpec * ps = R.plists.back ().get ();
  ps->name = ename;
  ps->line = ob.line;
  std::string item;
  if (r.peek (false) != '{') item = strip_gfs (r.word (false));
  Reader objects = block (r);
  read_particles (objects, item, ps);
  if (r.peek (false) == '{') {
    Reader forces = block (r);
    read_particle_forces (forces, ps);
    if (!ps->forces.empty () && !ps->particulate)
      r.fail ("GfsParticleForce objects act on GfsParticulate objects");
    if (ps->forces.size () > 8) r.fail ("at most 8 forces");
  }
  char c = r.peek (false);
  if ((c >= '0' && c <= '9') || c == '-' || c == '+' || c == '.')
    ps->idlast = atoi (r.word (false).c_str ());                                         /* idlast, :1087-1090 */
  ob.e->action = [ps, &R] () {
    /* the forces read the density and the viscosity of the fluid at the time of the event */
    if (ps->pl && !ps->forces.empty () && (refresh_alpha_cell (R) || refresh_viscosity_cell (R)))
      exit (1);
    if (ps->pl) must (gfship_particle_list_event (ps->pl));
  };
}

// LIST: the `*name' of a GfsParticleList of GfsParticulate objects read above (gfs_object_from_name), with the
// messages of the readers of the reference (particulate_field_read, :1959-1984, and the like)
inline ParticleSpec * read_particulate_list_name (Run & R, Reader & r, const Object & ob)
{
  if (r.at_end_of_object () || r.peek (false) == '{')
    r.fail ("expecting a string (object name)");
  const std::string lname = r.word (false);
  ParticleSpec * ps = R.plist_by_name (lname);
  if (!ps) {
    if (R.var_index (lname) >= 0)
      r.fail ("object '" + lname + "' is not a GfsParticleList");
    r.fail ("unknown object '" + lname + "'");
  }
  if (!ps->particulate)
    r.fail ("the list `" + lname + "' holds GfsParticle objects: Gfs" + ob.cls + " needs GfsParticulate objects");
  return ps;
}

inline void read_particulate_field (Run & R, Reader & r, Object & ob)
{
  // particulate_field_read (modules/particulatecommon.c:1959-1984):  GfsParticulateField [{ event }] NAME LIST
  // source_particulate_read (:2230-2318):  GfsSourceParticulate [{ event }] LIST { rkernel = R kernel = FUNCTION }
  // LIST is the `*name' of a GfsParticleList read above (gfs_object_from_name)
  const bool field = ob.cls == "ParticulateField";
  if (!field) ob.e->istep = 1;                  /* source_particulate_init, :2342-2350 */
  read_event_params (r, *ob.e);
  std::string vname;
  if (field) vname = r.word (false);            /* gfs_variable_read: the name of the variable */
  ParticleSpec * ps = read_particulate_list_name (R, r, ob);
  if (field) {
    const int v = R.get_or_add_variable (vname);
    R.device_vars.push_back (vname);
    ob.e->action = [&R, ps, v] () {
      must (gfship_particulate_field (ps->pl, R.vars[v].dev));
      R.vars[v].host_time = -1.;
    };
    return;
  }
  if (!R.source_particulates.empty ())
    r.fail ("one GfsSourceParticulate per simulation (the velocity takes one set of source fields)");
  R.source_particulates.emplace_back (new SourceParticulateSpec);
  SourceParticulateSpec * sp = R.source_particulates.back ().get ();
  sp->ps = ps;
  if (r.peek (false) != '{') r.fail ("expecting an opening brace");
  Reader b = block (r);
  while (!b.eof ()) {
    if (b.peek () == '{' || b.peek () == '=') b.fail ("expecting a keyword");
    const std::string k = b.word ();
    if (k != "rkernel" && k != "kernel") b.fail ("unknown keyword `" + k + "'");
    if (b.peek (false) != '=') b.fail ("expecting '='");
    b.expect ('=');
    if (k == "rkernel") sp->rkernel = atof (b.word ().c_str ());
    else sp->kernel = b.function ().text;
  }
  static const char * comp[3] = { "_Fx", "_Fy", "_Fz" };
  for (int c = 0; c < R.dim; c++) {
    const std::string fname = ps->name + comp[c];
    if (R.var_index (fname) < 0) R.device_vars.push_back (fname);
    sp->fvar[c] = R.get_or_add_variable (fname);
  }
  ob.e->action = [&R, sp] () {
    /* the forces read the density and the viscosity of the fluid at the time of the event */
    if (refresh_alpha_cell (R) || refresh_viscosity_cell (R))
      exit (1);
    gfship_field F[3] = { -1, -1, -1 };
    for (int c = 0; c < R.dim; c++) {
      F[c] = R.vars[sp->fvar[c]].dev;
      R.vars[sp->fvar[c]].host_time = -1.;
    }
    must (gfship_source_particulate_event (sp->ps->pl, F));
  };
}

inline void read_source_particulate_change (Run & R, Reader & r, Object & ob)
{
  // source_particulatevol_read (modules/particulatecommon.c:2752-2804), source_particulatemass_read (:2908-2962):
  //   GfsSourceParticulateVol | GfsSourceParticulateMass [{ event }] LIST FUNCTION [VARIABLE]
  // the parent class is gfs_source_generic: no variable comes before the list; LIST is the `*name' of a
  // GfsParticleList read above.  The function runs on the device (gfship_particulate_source_create): the
  // variables it names are bound from the device variables of the run
  const bool vol = ob.cls == "SourceParticulateVol";
  ob.e->istep = 1;                              /* source_generic_init, src/source.c:149-152 */
  read_event_params (r, *ob.e);
  ParticleSpec * ps = read_particulate_list_name (R, r, ob);
  R.particulate_sources.emplace_back (new ParticulateSourceSpec);
  ParticulateSourceSpec * sp = R.particulate_sources.back ().get ();
  sp->ps = ps;
  sp->kind = vol ? GFSHIP_PARTICULATE_SOURCE_VOLUME : GFSHIP_PARTICULATE_SOURCE_MASS;
  sp->line = ob.line;
  // a variable of the object: made where it is missing (gfs_domain_get_or_add_variable) and kept on the device
  auto device_variable = [&R] (const std::string & name) {
    const int v = R.get_or_add_variable (name);
    if (!R.on_device (name)) R.device_vars.push_back (name);
    return v;
  };
  sp->rad = device_variable ("Rad");             /* :2785-2793 */
  sp->urel[0] = device_variable ("Urelp");
  sp->urel[1] = device_variable ("Vrelp");
  if (R.dim == 3) sp->urel[2] = device_variable ("Wrelp");
  if (r.at_end_of_object ())
    r.fail ("expecting an expression");          /* gfs_function_read */
  const FunctionText t = r.function ();
  if (t.block || !Reader::is_number (t.text) || atof (t.text.c_str ()) != 0.)
    sp->function = t.text;
  std::string dname;
  if (!r.at_end_of_object ()) {
    dname = r.word (false);
    /* volsource must exist (gfs_variable_from_name, :2798); dmdtvariable is made (:2955) */
    if (vol && R.var_index (dname) < 0)
      r.fail ("unknown variable `" + dname + "'");
    sp->deposit = device_variable (dname);
  }
  for (const std::string & id : FunctionSet::identifiers (t.text)) {
    if (id == "Wrelp" && R.dim == 2)
      r.fail ("Wrelp is not a variable in 2-D");
    if (id == "Rad" || id == "Urelp" || id == "Vrelp" || id == "Wrelp" || id == "x" || id == "y" || id == "z" ||
        id == "t" || R.var_index (id) < 0)
      continue;                                  /* anything else is left to the compiler of the device */
    if (id == dname)
      r.fail ("the function of Gfs" + ob.cls + " names `" + dname + "', the variable its sources are deposited "
              "into: it would read a sum that depends on the order of the particles");
    if (!R.on_device (id))
      r.fail ("the function of Gfs" + ob.cls + " reads `" + id +
              "', which is not kept on the device (the variables of the simulation, tracers and the variables "
              "of GfsParticulateField, GfsSourceParticulate and these classes are)");
    sp->reads.push_back (id);
  }
  ob.e->action = [&R, sp] () {
    must (gfship_particulate_source_event (sp->src));
    for (int v : { sp->rad, sp->urel[0], sp->urel[1], sp->urel[2], sp->deposit })
      if (v >= 0) R.vars[v].host_time = -1.;
  };
}

inline void read_feed_particle (Run & R, Reader & r, Object & ob)
{
  // gfs_feed_particle_read (modules/particulatecommon.c:2435-2575):
  //   GfsFeedParticle [{ event }] LIST { nparts = F xfeed = F yfeed = F zfeed = F velx = F vely = F velz = F
  //                                      mass = F volume = F }
  // LIST is the `*name' of a GfsParticleList read above.  nparts and the three positions are evaluated without a
  // cell (gfs_function_value (f, NULL), :2381-2383, :2411): functions of the host; velx, vely, velz are read and
  // never evaluated (:2388-2392); mass and volume are evaluated at the cell of the candidate, on the device
  // (gfship_feed_particle_create), with the device variables of the run they name
  read_event_params (r, *ob.e);
  ParticleSpec * ps = read_particulate_list_name (R, r, ob);
  R.feed_particles.emplace_back (new FeedParticleSpec);
  FeedParticleSpec * sp = R.feed_particles.back ().get ();
  sp->ps = ps;
  sp->line = ob.line;
  if (r.peek (false) != '{') r.fail ("expecting an opening brace");
  Reader b = block (r);
  static const char * keywords[] = { "nparts", "xfeed", "yfeed", "zfeed", "velx", "vely", "velz", "mass", "volume" };
  while (!b.eof ()) {
    if (b.peek () == '{' || b.peek () == '=') b.fail ("expecting a keyword");
    const std::string k = b.word ();
    int q = 0;
    while (q < 9 && k != keywords[q]) q++;
    if (q == 9) b.fail ("unknown keyword `" + k + "'");
    if (b.peek (false) != '=') b.fail ("expecting '='");
    b.expect ('=');
    const int line = b.line ();
    const FunctionText t = b.function ();
    if (q < 4) {
      /* the reference would read the variable at the cell NULL */
      for (const std::string & id : FunctionSet::identifiers (t.text))
        if (R.var_index (id) >= 0)
          b.fail ("`" + k + "' of GfsFeedParticle is evaluated without a cell: it cannot read the variable `" + id + "'");
      (q == 0 ? sp->np : sp->feed[q - 1]) = R.functions.add (t, line);
    }
    else if (q >= 7) {
      if (t.block || !Reader::is_number (t.text) || atof (t.text.c_str ()) != 0.)
        (q == 7 ? sp->mass : sp->volume) = t.text;
      for (const std::string & id : FunctionSet::identifiers (t.text)) {
        if (id == "x" || id == "y" || id == "z" || id == "t" || R.var_index (id) < 0)
          continue;                                /* anything else is left to the compiler of the device */
        if (!R.on_device (id))
          b.fail ("`" + k + "' of GfsFeedParticle reads `" + id +
                  "', which is not kept on the device (the variables of the simulation, tracers and the variables "
                  "of GfsParticulateField, GfsSourceParticulate, GfsSourceParticulateVol and ...Mass are)");
        if (std::find (sp->reads.begin (), sp->reads.end (), id) == sp->reads.end ())
          sp->reads.push_back (id);
      }
    }
  }
  ob.e->action = [&R, sp] () {
    const double nowhere[3] = { 0., 0., 0. };
    /* guint np = gfs_function_value (feedp->np, NULL), once (:2411); then x, y, z of every candidate in that
       order (:2381-2383): the order a function with state sees */
    const unsigned np = sp->np ? (unsigned) eval (R, sp->np, nowhere, -1) : 1u;
    std::vector<double> pos (3*(size_t) np, 0.);
    for (unsigned i = 0; i < np; i++)
      for (int c = 0; c < 3; c++)
        if (sp->feed[c]) pos[3*(size_t) i + c] = eval (R, sp->feed[c], nowhere, -1);
    must (gfship_feed_particle_event (sp->handle, (int) np, pos.data ()));
  };
}

// the variable of a GfsDropletToParticle or of a GfsRemoveDroplets, and the variables its function names: they must
// exist and be kept on the device
inline int read_droplet_variable (Run & R, Reader & r, const Object & ob)
{
  if (r.at_end_of_object () || r.peek (false) == '{')
    r.fail ("expecting a string (variable)");
  const std::string vname = r.word (false);
  const int v = R.var_index (vname);
  if (v < 0) r.fail ("unknown variable `" + vname + "'");
  if (!R.on_device (vname))
    r.fail ("Gfs" + ob.cls + " works on `" + vname +
            "', which is not kept on the device (the variables of the simulation, tracers and the variables "
            "of GfsParticulateField, GfsSourceParticulate, GfsSourceParticulateVol and ...Mass are)");
  return v;
}

inline void droplet_function_reads (Run & R, Reader & r, const Object & ob, const std::string & text,
                                    std::vector<std::string> & reads)
{
  for (const std::string & id : FunctionSet::identifiers (text)) {
    if (id == "x" || id == "y" || id == "z" || id == "t" || R.var_index (id) < 0)
      continue;                                    /* anything else is left to the compiler of the device */
    if (!R.on_device (id))
      r.fail ("the function of Gfs" + ob.cls + " reads `" + id +
              "', which is not kept on the device (the variables of the simulation, tracers and the variables "
              "of GfsParticulateField, GfsSourceParticulate, GfsSourceParticulateVol and ...Mass are)");
    if (std::find (reads.begin (), reads.end (), id) == reads.end ())
      reads.push_back (id);
  }
}

inline void read_droplet_to_particle (Run & R, Reader & r, Object & ob)
{
  // gfs_droplet_to_particle_read (modules/particulatecommon.c:1407-1467):
  //   GfsDropletToParticle [{ event }] LIST VARIABLE [{ min = I reset = X density = X }] [FUNCTION]
  // LIST is the `*name' of a GfsParticleList read above; the droplets of VARIABLE (or of FUNCTION, evaluated at
  // every cell on the device) smaller than min cells join the list (gfship_droplet_to_particle_create)
  read_event_params (r, *ob.e);
  ParticleSpec * ps = read_particulate_list_name (R, r, ob);
  R.droplet_to_particles.emplace_back (new DropletToParticleSpec);
  DropletToParticleSpec * sp = R.droplet_to_particles.back ().get ();
  sp->ps = ps;
  sp->line = ob.line;
  sp->c = read_droplet_variable (R, r, ob);
  if (r.peek (false) == '{') {                   /* gts_file_assign_variables, :1448-1461 */
    Reader b = block (r);
    while (!b.eof ()) {
      if (b.peek () == '{' || b.peek () == '=') b.fail ("expecting a keyword");
      const std::string k = b.word ();
      if (k != "min" && k != "reset" && k != "density") b.fail ("unknown identifier `" + k + "'");
      if (b.peek (false) != '=') b.fail ("expecting `='");
      b.expect ('=');
      const std::string w = b.word ();
      char * end = nullptr;
      if (k == "min") {
        const long m = strtol (w.c_str (), &end, 10);
        if (w.empty () || *end != '\0') b.fail ("expecting an integer (min)");
        sp->min = (int) m;
      }
      else {
        if (!Reader::is_number (w)) b.fail ("expecting a number (" + k + ")");
        (k == "reset" ? sp->reset : sp->density) = atof (w.c_str ());
      }
    }
  }
  if (!r.at_end_of_object ()) {                  /* :1463-1466 */
    const FunctionText t = r.function ();
    sp->function = t.text;
    droplet_function_reads (R, r, ob, t.text, sp->reads);
  }
  ob.e->action = [&R, sp] () {
    /* mass = volume/alpha at the cell of the new particle: alpha at the time of the event */
    if (refresh_alpha_cell (R))
      exit (1);
    must (gfship_droplet_to_particle_event (sp->handle, nullptr));
    R.vars[sp->c].host_time = -1.;
  };
}

inline void read_remove_droplets (Run & R, Reader & r, Object & ob)
{
  // gfs_remove_droplets_read (src/event.c:2155-2190):  GfsRemoveDroplets [{ event }] VARIABLE MIN [FUNCTION [VAL]]
  // the droplets of FUNCTION (or of VARIABLE) smaller than MIN cells get VARIABLE = VAL (gfship_remove_droplets).
  // FUNCTION: the name of a variable (gfs_function_get_variable, :2138); the library has no entry that evaluates
  // any other function into a temporary variable
  read_event_params (r, *ob.e);
  const int c = read_droplet_variable (R, r, ob);
  if (r.at_end_of_object ()) r.fail ("expecting an integer (min)");
  const std::string w = r.word (false);
  char * end = nullptr;
  const long min = strtol (w.c_str (), &end, 10);
  if (w.empty () || *end != '\0') r.fail ("expecting an integer (min)");
  int mask = c;
  double val = 0.;
  if (!r.at_end_of_object ()) {
    const std::string f = r.word (false);
    mask = R.var_index (f);
    if (mask < 0 && Reader::is_number (f))
      r.fail ("the function of GfsRemoveDroplets is the name of a variable here: the constant `" + f +
              "' is not supported");
    if (mask < 0)
      r.fail ("the function of GfsRemoveDroplets is the name of a variable here: `" + f + "' is none");
    if (!R.on_device (f))
      r.fail ("the function of GfsRemoveDroplets reads `" + f +
              "', which is not kept on the device (the variables of the simulation, tracers and the variables "
              "of GfsParticulateField, GfsSourceParticulate, GfsSourceParticulateVol and ...Mass are)");
    if (!r.at_end_of_object ()) val = r.number ();
  }
  ob.e->action = [&R, c, mask, min, val] () {
    must (gfship_remove_droplets (R.dom, R.vars[mask].dev, R.vars[c].dev, (int) min, val));
    R.vars[c].host_time = -1.;
  };
}

// the optional level that ends the outputs of modules/fft.c
inline void skip_level (Reader & r)
{
  char c = r.peek (false);
  if (c >= '0' && c <= '9') r.number ();
}

inline void read_output_energy_spectra (Run & R, Reader & r, Object & ob)
{
  // GfsOutputEnergySpectra (modules/fft.c:1360-1530): file { x0 = .. x1 = .. ... } [level]; the box
  // is transformed whole at the finest level
  if (r.peek (false) == '{') r.braces ();
  skip_level (r);
  Output * o = ob.o;
  ob.e->action = [&R, o] () {
    int nk = gfship_energy_spectra_bins (R.dom);
    std::vector<double> Ek ((size_t) std::max (nk, 1));
    gfship_field u[3];
    for (int c = 0; c < R.dim; c++) u[c] = R.velocity (c).dev;
    double Etot = 0., deltak = 0.;
    if (nk < 0) die_last_error ();
    must (gfship_energy_spectra (R.dom, R.dim, u, Ek.data (), &Etot, &deltak));
    // write_energy_spectra, modules/fft.c:1340-1348
    FILE * fp = o->open ();
    fprintf (fp, "# Total energy = %g \n", Etot);
    fputs ("# 1:k 2:Ek \n", fp);
    for (int i = 1; i < nk; i++)
      fprintf (fp, "%g %g \n", deltak*sqrt ((double) i), Ek[i]);
    fflush (fp);
  };
}

inline void read_output_spectra (Run & R, Reader & r, Object & ob)
{
  // GfsOutputSpectra (modules/fft.c:1101-1226): file v { x0 = .. x1 = .. ... } [level]; the 3-D box is
  // transformed whole at the finest level
  std::string vname = r.word (false);
  int v = R.var_index (vname);
  if (v < 0) r.fail ("unknown variable `" + vname + "'");
  // { x0 = .. y0 = .. z0 = .. x1 = .. y1 = .. z1 = .. }: a box that is flat in one direction is a plane
  // (realdim == 2, modules/fft.c:1119-1141); anything else is taken as the whole box
  int normal = -1;
  double plane_pos = 0.;
  if (r.peek (false) == '{') {
    auto m = r.assignments ();
    const char * lo[3] = { "x0", "y0", "z0" }, * hi[3] = { "x1", "y1", "z1" };
    for (int c = 0; c < 3; c++)
      if (m.count (lo[c]) && m.count (hi[c]) && atof (m[lo[c]].c_str ()) == atof (m[hi[c]].c_str ())) {
        if (normal >= 0) r.fail ("GfsOutputSpectra: FFT in 1 dimension is not implemented (modules/fft.c:1142)");
        normal = c;
        plane_pos = atof (m[lo[c]].c_str ());
      }
  }
  skip_level (r);
  if (R.dim != 3) r.fail ("GfsOutputSpectra: the 3-D box or one of its planes is transformed");
  Output * o = ob.o;
  ob.e->action = [&R, o, v, normal, plane_pos] () {
    const int N = gfship_output_spectra_side (R.dom);
    if (N <= 0) die_last_error ();
    // the whole box: N x N x (N/2 + 1) modes; a plane: the two in-plane directions, both with signed k
    const int nh = N/2 + 1, nl = normal >= 0 ? 1 : nh;
    std::vector<double> F ((size_t) 2*N*N*nl);
    double ks = 0.;
    must (normal >= 0 ? gfship_output_spectra_plane (R.dom, R.vars[v].dev, normal, plane_pos, F.data (), &ks) :
          gfship_output_spectra (R.dom, R.vars[v].dev, F.data (), &ks));
    // write_spectra, modules/fft.c:1047-1085 (L = 1).  For a plane order_array sorts by descending size, so the
    // two in-plane directions come first, in coordinate order; the flat direction is last (one point, k = 0):
    // N*N rows
    const int ca = normal == 0 ? 1 : 0, cb = normal == 2 ? 1 : 2, cl = normal >= 0 ? normal : 2;
    FILE * fp = o->open ();
    fprintf (fp, "# %i \n", normal >= 0 ? N*N : N*N*N);
    fputs ("# 1:kx 2:ky 3:kz 4:real 5:img\n", fp);
    for (int i = 0; i < N; i++)
      for (int j = 0; j < N; j++)
        for (int l = 0; l < nl; l++) {
          double k[3];
          k[cl] = ks*l;
          k[normal >= 0 ? ca : 0] = ks*(i < nh ? i : i - N);
          k[normal >= 0 ? cb : 1] = ks*(j < nh ? j : j - N);
          const size_t q = 2*(((size_t) i*N + j)*nl + l);
          fprintf (fp, "%g %g %g %g %g\n", k[0], k[1], k[2], F[q]*1., F[q + 1]*1.);
        }
    fflush (fp);
  };
}

inline void read_variable_turbulent_viscosity (Run & R, Reader & r, Object & ob)
{
  // GfsVariableTurbulentViscosity [{ event }] name Cs (modules/turbulence.c:1068-1084): the Smagorinsky
  // eddy viscosity of the leaf cells, refreshed by its event (default: every step)
  if (r.peek (false) == '{') read_event_params (r, *ob.e);
  else { ob.e->istep = 1; ob.e->start = 0.; }
  std::string name = r.word (false);
  const double Cs = r.number ();
  const int v = R.get_or_add_variable (name);
  R.device_vars.push_back (name);
  ob.e->action = [&R, v, Cs] () {
    gfship_field u[3] = { -1, -1, -1 };
    for (int c = 0; c < R.dim; c++) u[c] = R.velocity (c).dev;
    if (R.dim == 2) u[2] = u[1];
    must (gfship_turbulent_viscosity (R.dom, u, Cs, 1, R.vars[v].dev));
    R.vars[v].host_time = -1.;      /* the host copy, if any, is out of date */
  };
}

inline void read_init_spectra (Run & R, Reader & r, Object &)
{
  // gfs_init_spectra_read, modules/turbulence.c:277-346:
  //   GfsInitSpectra { event } { x0 y0 z0 L E } { alpha epsilon c1 c2 c3 [ReL kmax seed] } [level] U V W
  Event e;
  read_event_params (r, e);
  gfship_init_spectra_params p;
  memset (&p, 0, sizeof (p));
  p.kmax = DBL_MAX; p.ReL = 0.; p.seed = 0.;
  auto read = [&r] (std::initializer_list<std::pair<const char *, double *>> keys) {
    for (auto & kv : r.assignments ()) {
      double * v = nullptr;
      for (auto & k : keys) if (kv.first == k.first) v = k.second;
      if (!v) r.fail ("unknown GfsInitSpectra keyword `" + kv.first + "'");
      *v = atof (kv.second.c_str ());
    }
  };
  read ({ { "x0", &p.x0 }, { "y0", &p.y0 }, { "z0", &p.z0 }, { "L", &p.L }, { "E", &p.E } });
  read ({ { "alpha", &p.alpha }, { "epsilon", &p.epsilon }, { "c1", &p.c1 }, { "c2", &p.c2 }, { "c3", &p.c3 },
          { "ReL", &p.ReL }, { "kmax", &p.kmax }, { "seed", &p.seed } });
  p.level = -1;                                   /* default: the depth of the domain */
  char c0 = r.peek (false);
  if (c0 >= '0' && c0 <= '9') p.level = (int) r.number ();
  std::vector<std::string> names;
  for (int c = 0; c < 3; c++) names.push_back (r.word (false));
  if (R.dim != 3) r.fail ("GfsInitSpectra only works in 3-D (modules/turbulence.c:747)");
  R.init_spectra.emplace_back (p, names);
}

inline void read_event_script (Run &, Reader & r, Object & ob)
{
  std::string script = r.braces ();
  ob.e->action = [script] () {
    fflush (stdout);
    if (g_shell.run (script) != 0)      /* in the helper forked before the device was touched */
      fprintf (stderr, "gfship: EventScript returned a non-zero status\n");
  };
}

inline void read_output_time (Run & R, Reader &, Object & ob)
{
  Output * o = ob.o;
  ob.e->action = [&R, o] () {
    // time_event, src/output.c:370-392
    double real = std::chrono::duration<double> (std::chrono::steady_clock::now () - R.clock0).count ();
    fprintf (o->open (), "step: %7u t: %15.8f dt: %13.6e cpu: %15.8f real: %15.8f\n",
             R.i, R.t, R.tree ? gfship_tree_dt (R.tree) : R.sim ? gfship_sim_advection_params (R.sim)->dt : 0., real, real);
    fflush (o->fp);
  };
}

inline void read_output_solver_stats (Run & R, Reader &, Object & ob)
{
  Output * o = ob.o;
  const bool diffusion = ob.cls == "OutputDiffusionStats";
  ob.e->action = [&R, o, diffusion] () {
    FILE * fp = o->open ();
    if (diffusion) {
      // gfs_output_diffusion_stats_event, src/output.c:560-600
      for (int c = 0; c < R.dim; c++)
        if (R.has_viscosity (c)) {
          fprintf (fp, "%s diffusion\n", velocity_name[c]);
          stats_write (gfship_sim_diffusion_params (R.sim, c), fp);
        }
      // ... then the tracers, in the order of domain->variables, once their solver has run (:551)
      for (size_t k = 0; k < R.tracers.size (); k++)
        if (R.tracers[k].D != 0. && gfship_sim_tracer_diffusion_params (R.sim, (int) k)->niter > 0) {
          fprintf (fp, "%s diffusion\n", R.tracers[k].name.c_str ());
          stats_write (gfship_sim_tracer_diffusion_params (R.sim, (int) k), fp);
        }
    }
    else {
      // projection_stats_event, src/output.c:486-500
      const gfship_multilevel_params * p = R.tree ? gfship_tree_projection_params (R.tree, 0) :
        gfship_sim_projection_params (R.sim);
      if (p->niter > 0) {
        fprintf (fp, "MAC projection        before     after       rate\n");
        stats_write (p, fp);
      }
      fprintf (fp, "Approximate projection\n");
      stats_write (R.tree ? gfship_tree_projection_params (R.tree, 1) :
                   gfship_sim_approx_projection_params (R.sim), fp);
    }
    fflush (fp);
  };
}

// GfsOutputScalarNorm, GfsOutputScalarSum, GfsOutputScalarStats
inline void read_output_scalar (Run & R, Reader & r, Object & ob)
{
  Output * o = ob.o;
  ScalarSpec s = read_scalar (R, r);
  std::string kind = ob.cls;
  ob.e->action = [&R, o, s, kind] () {
    std::vector<double> a = function_values (R, s.f);
    FILE * fp = o->open ();
    if (kind == "OutputScalarNorm") {
      // gfs_output_scalar_norm_event, src/output.c:1966-1986
      gfship_norm nm = norm_of (R, a);
      fprintf (fp, "%s time: %g first: % 10.3e second: % 10.3e infty: % 10.3e\n",
               s.name.c_str (), R.t, nm.first, nm.second, nm.infty);
    }
    else if (kind == "OutputScalarSum") {
      // gfs_output_scalar_sum_event, src/output.c:2089-2123
      double sum = 0.;
      for_each_cell (R, [&] (const Cell & cell, size_t c) {
        double w = cell_volume (R, cell);
        if (s.w) { double p[3]; cell_pos (R, cell, p); w = eval (R, s.w, p, (long) c); }
        sum += w*a[c];
      });
      if (!s.format.empty ()) {
        std::string f = "%s time: " + s.format + " sum: " + s.format + "\n";
        fprintf (fp, f.c_str (), s.name.c_str (), R.t, sum);
      }
      else
        fprintf (fp, "%s time: %g sum: % 15.6e\n", s.name.c_str (), R.t, sum);
    }
    else {
      // gfs_output_scalar_stats_event, src/output.c:2030-2060 (GtsRange: min, avg, stddev, max)
      double mn = DBL_MAX, mx = -DBL_MAX, sum = 0., sum2 = 0.;
      size_t nn = 0;
      for_each_cell (R, [&] (const Cell &, size_t c) {
        mn = std::min (mn, a[c]); mx = std::max (mx, a[c]);
        sum += a[c]; sum2 += a[c]*a[c]; nn++;
      });
      double avg = sum/nn, sd = sqrt (std::max (0., (sum2 - sum*sum/nn)/nn));
      fprintf (fp, "%s time: %g min: %10.3e avg: %10.3e | %10.3e max: %10.3e\n",
               s.name.c_str (), R.t, mn, avg, sd, mx);
    }
    fflush (fp);
  };
}

inline void read_output_error_norm (Run & R, Reader & r, Object & ob)
{
  // gfs_output_error_norm_read / _event, src/output.c:2780-3035
  Output * o = ob.o;
  ScalarSpec s = read_scalar (R, r);
  Function * ref = nullptr, * w = nullptr;
  int unbiased = 0, relative = 0, ev = -1;
  Reader b = block (r);
  while (!b.eof ()) {
    std::string k = b.word ();
    b.expect ('=');
    if (k == "s") ref = R.functions.add (b.function (), b.line ());
    else if (k == "w") w = R.functions.add (b.function (), b.line ());
    else if (k == "unbiased") unbiased = atoi (b.word ().c_str ());
    else if (k == "relative") relative = atoi (b.word ().c_str ());
    else if (k == "v") ev = R.get_or_add_variable (b.word ());
    else b.fail ("unknown identifier `" + k + "'");
  }
  if (!ref) r.fail ("expecting `s = ...'");
  if (w) r.fail ("weighted error norms are not supported");
  ob.e->action = [&R, o, s, ref, unbiased, relative, ev] () {
    std::vector<double> val = function_values (R, s.f), sol = function_values (R, ref), err (R.total (), 0.);
    for_each_cell (R, [&] (const Cell &, size_t c) { err[c] = val[c] - sol[c]; });
    gfship_norm snorm = { 0., 0., 0., 0., 0. };
    if (relative) snorm = norm_of (R, sol);
    gfship_norm nm = norm_of (R, err);
    if (unbiased) {
      for_each_cell (R, [&] (const Cell &, size_t c) { err[c] -= nm.bias; });
      nm = norm_of (R, err);
    }
    if (ev >= 0) { R.vars[ev].host = err; }
    if (relative) {
      if (snorm.first > 0.) nm.first /= snorm.first;
      if (snorm.second > 0.) nm.second /= snorm.second;
      if (snorm.infty > 0.) nm.infty /= snorm.infty;
    }
    FILE * fp = o->open ();
    if (!s.format.empty ()) {
      const std::string & f = s.format;
      std::string fmt = "%s time: " + f + " first: " + f + " second: " + f + " infty: " + f +
        " bias: " + f + "\n";
      fprintf (fp, fmt.c_str (), s.name.c_str (), R.t, nm.first, nm.second, nm.infty, nm.bias);
    }
    else
      fprintf (fp, "%s time: %g first: %10.3e second: %10.3e infty: %10.3e bias: %10.3e\n",
               s.name.c_str (), R.t, nm.first, nm.second, nm.infty, nm.bias);
    fflush (fp);
  };
}

inline void read_output_location (Run & R, Reader & r, Object & ob)
{
  // gfs_output_location_read / _event, src/output.c:1037-1203
  Output * o = ob.o;
  auto pts = std::make_shared<std::vector<double>> ();
  if (r.peek (false) == '{') {
    std::istringstream in (r.braces ());
    double x;
    while (in >> x) pts->push_back (x);
  }
  else {
    std::string w = r.word (false);
    if (Reader::is_number (w)) {
      pts->push_back (atof (w.c_str ()));
      pts->push_back (r.number ());
      pts->push_back (r.number ());
    }
    else {
      std::ifstream in (w);
      if (!in) r.fail ("cannot open file `" + w + "'");
      double x;
      while (in >> x) pts->push_back (x);
    }
  }
  if (pts->size () % 3) r.fail ("expecting x y z triplets");
  if (r.peek (false) == '{') r.braces ();     /* label, precision: defaults only */
  auto first = std::make_shared<bool> (true);
  const int line = ob.line;
  ob.e->action = [&R, o, pts, first, line] () {
    FILE * fp = o->open ();
    int np = (int) pts->size ()/3;
    if (*first) {
      fputs ("# 1:t 2:x 3:y 4:z", fp);
      int nv = 5;
      for (const Variable & V : R.vars)
        if (!V.derive) fprintf (fp, " %d:%s", nv++, V.name.c_str ());
      fputc ('\n', fp);
      *first = false;
    }
    std::vector<std::vector<double>> cols;
    std::vector<unsigned char> inside (np, 1);
    for (Variable & V : R.vars) {
      if (V.derive) continue;
      std::vector<double> out (np, 0.);
      if (R.tree) {         /* a refined tree samples the variables it keeps on the device (GFSHIP_TREE_*) */
        if (V.dev < 0) {
          fprintf (stderr, "gfship: line %d: GfsOutputLocation: the variable `%s' is not kept on a refined tree\n",
                   line, V.name.c_str ());
          exit (1);
        }
        CHECK (gfship_tree_interpolate (R.tree, V.dev, np, pts->data (), out.data (), inside.data ()));
        cols.push_back (out);
        continue;
      }
      gfship_field f = V.dev;
      gfship_field tmp = -1;
      if (f < 0) {          /* host-only variable: sample it through a scratch device field */
        tmp = gfship_field_alloc (R.dom, -1);
        CHECK (tmp);
        size_t vi = &V - &R.vars[0];
        CHECK (gfship_field_upload (R.dom, tmp, R.level, host_of (R, (int) vi).data ()));
        CHECK (gfship_bc (R.dom, tmp, tmp, R.level));
        f = tmp;
      }
      CHECK (gfship_field_interpolate (R.dom, f, np, pts->data (), out.data (), inside.data ()));
      if (tmp >= 0) gfship_field_free (R.dom, tmp);
      cols.push_back (out);
    }
    for (int q = 0; q < np; q++) {
      if (!inside[q]) continue;
      fprintf (fp, "%g %g %g %g", R.t, (*pts)[3*q], (*pts)[3*q + 1], (*pts)[3*q + 2]);
      for (auto & c : cols) fprintf (fp, " %g", c[q]);
      fputc ('\n', fp);
    }
    fflush (fp);
  };
}

inline void read_output_simulation (Run & R, Reader & r, Object & ob)
{
  // gfs_output_simulation (src/output.c:1354-1470, parameters :1480-1555): format = gfs (the
  // default: a simulation file with the cell data, text or `binary = 1') or text (columns)
  Output * o = ob.o;
  std::string format = "gfs", variables;
  bool binary = false;
  if (r.peek (false) == '{') {
    Reader b = block (r);
    while (!b.eof ()) {
      std::string k = b.word ();
      b.expect ('=');
      std::string v = b.word ();
      if (k == "format") format = v;
      else if (k == "binary") binary = atoi (v.c_str ()) != 0;
      else if (k == "variables") variables = v;
      else if (k == "depth" || k == "solid" || k == "precision") ;
      else b.fail ("unknown GfsOutputSimulation keyword `" + k + "'");
    }
    if (format != "gfs" && format != "text")
      r.fail ("GfsOutputSimulation: format `" + format + "' is not produced (gfs and text are)");
  }
  ob.e->action = [&R, o, format, binary, variables] () {
    FILE * fp = o->open ();
    std::vector<int> list;
    if (variables.empty ()) {
      for (size_t q = 0; q < R.vars.size (); q++)
        if (!R.vars[q].derive) list.push_back ((int) q);
    }
    else
      for (const std::string & nm : gfs::split_commas (variables)) {
        int q = R.var_index (nm);
        if (q < 0) { fprintf (stderr, "gfship: GfsOutputSimulation: unknown variable `%s'\n", nm.c_str ()); exit (1); }
        list.push_back (q);
      }
    if (format == "text") {
      fputs ("# 1:x 2:y 3:z", fp);
      int nv = 4;
      for (int q : list) fprintf (fp, " %d:%s", nv++, R.vars[q].name.c_str ());
      fputc ('\n', fp);
      for_each_cell (R, [&] (const Cell & cell, size_t c) {
        double p[3];
        cell_pos (R, cell, p);
        fprintf (fp, "%g %g %g", p[0], p[1], p[2]);
        for (int q : list) fprintf (fp, " %g", host_of (R, q)[c]);
        fputc ('\n', fp);
      });
    }
    else
      write_simulation (R, fp, list, binary);
    o->close ();
  };
}

inline void read_not_produced (Run &, Reader & r, Object & ob)
{
  r.rest_of_object ();
  fprintf (stderr, "gfship: line %d: %s is not produced (skipped)\n", ob.line, ob.cls.c_str ());
}

// ---- the table: every class of the body of a simulation file this front end reads.  Anything else fails loudly
// with the line number.  Beside these: one GfsBox (periodic through self edges `1 1 right'), with
// GfsBoundary { GfsBcDirichlet | GfsBcNeumann } sides (parse_box, below).
enum ClassFlags {
  EVENT = 1,              // an event: parse_object makes it and adds it to the run
  PARAMS = 2,             //   ... and reads its `{ start = .. step = .. }' first (otherwise the reader does)
  OUTPUT = 4,             //   ... and then its output (stdout, a file name, a { shell script })
  TREE = 8,               // the event is allowed on a refined tree in a GfsSimulation
  TREE_POISSON = 16,      // ... in a GfsPoisson
  TREE_POISSON_SKIP = 32  // ... in a GfsPoisson it is skipped with a message
};
const unsigned OUT = EVENT | PARAMS | OUTPUT, ON_TREES = TREE | TREE_POISSON;

struct ClassRow {
  const char * name;
  void (* read) (Run &, Reader &, Object &);
  unsigned flags;
};

inline const ClassRow class_table[] = {
  { "Time", read_time, 0 },
  { "Refine", read_refine, 0 },                           // an integer, or a function of x, y, z (a refined tree)
  { "GModule", read_gmodule, 0 },                         // fft, turbulence, particulates: built in; others ignored
  { "ApproxProjectionParams", read_projection_params, 0 },
  { "ProjectionParams", read_projection_params, 0 },
  { "AdvectionParams", read_advection_params, 0 },
  { "Init", read_init, 0 },
  { "SourceDiffusion", read_source_diffusion, 0 },        // on U, V, W: a constant or a function of x, y, z, t;
  { "SourceViscosity", read_source_diffusion, 0 },        //   on a declared tracer: a constant
  { "Source", read_source, 0 },                           // a constant on U, V, W
  { "PhysicalParams", read_physical_params, 0 },          // alpha
  { "VariableTracer", read_variable_tracer, 0 },          // { gradient = .. scheme = godunov | none }
  { "VariableStreamFunction", read_variable_stream_function, 0 },    // GfsAdvection
  { "EventStop", read_event_stop, EVENT | PARAMS | TREE },
  { "ParticleList", read_particle_list, EVENT | TREE },   // of GfsParticle / GfsParticulate, with GfsForce*; on a
                                                          //   tree: GfsParticle without forces (check_tree_simulation)
  { "ParticulateField", read_particulate_field, EVENT },  // on a list named `*NAME'
  { "SourceParticulate", read_particulate_field, EVENT },
  { "SourceParticulateVol", read_source_particulate_change, EVENT },     // LIST FUNCTION [VARIABLE]: the volumes and
  { "SourceParticulateMass", read_source_particulate_change, EVENT },    //   the masses of a list change (uniform boxes)
  { "FeedParticle", read_feed_particle, EVENT },          // LIST { nparts xfeed yfeed zfeed mass volume }: particles
                                                          //   join a list of particulates (uniform boxes)
  { "DropletToParticle", read_droplet_to_particle, EVENT },   // LIST VARIABLE [{ min reset density }] [FUNCTION]: small
                                                          //   droplets of a tracer join a list (uniform boxes)
  { "RemoveDroplets", read_remove_droplets, EVENT },      // VARIABLE MIN [VARIABLE [VAL]] (uniform boxes)
  { "OutputEnergySpectra", read_output_energy_spectra, OUT },
  { "OutputSpectra", read_output_spectra, OUT },
  { "VariableTurbulentViscosity", read_variable_turbulent_viscosity, EVENT },
  { "InitSpectra", read_init_spectra, 0 },
  { "EventScript", read_event_script, EVENT | PARAMS | ON_TREES },
  { "OutputTime", read_output_time, OUT | ON_TREES },
  { "OutputProjectionStats", read_output_solver_stats, OUT | ON_TREES },
  { "OutputDiffusionStats", read_output_solver_stats, OUT },
  { "OutputScalarNorm", read_output_scalar, OUT | ON_TREES },
  { "OutputScalarSum", read_output_scalar, OUT | ON_TREES },
  { "OutputScalarStats", read_output_scalar, OUT | ON_TREES },
  { "OutputErrorNorm", read_output_error_norm, OUT | ON_TREES },
  { "OutputLocation", read_output_location, OUT | TREE }, // on a tree: gfship_tree_interpolate
  { "OutputSimulation", read_output_simulation, OUT | TREE | TREE_POISSON_SKIP },    // gfs (text or binary), text
  { "OutputPPM", read_not_produced, 0 },
  { "OutputGRD", read_not_produced, 0 },
  { "OutputTiming", read_not_produced, 0 },
  { "OutputBalance", read_not_produced, 0 },
  { "OutputSolidStats", read_not_produced, 0 },
  { "OutputAdaptStats", read_not_produced, 0 },
};

inline const ClassRow * find_class (const std::string & cls)
{
  for (const ClassRow & row : class_table)
    if (cls == row.name) return &row;
  return nullptr;
}

inline void parse_object (Run & R, Reader & r)
{
  Object ob;
  ob.line = r.line ();
  ob.cls = strip_gfs (r.word ());
  const ClassRow * row = find_class (ob.cls);
  if (!row) r.fail ("unsupported object `" + ob.cls + "'");
  std::unique_ptr<Event> e (row->flags & EVENT ? new Event : nullptr);
  if (e) { e->cls = ob.cls; e->line = ob.line; }
  ob.e = e.get ();
  if (row->flags & PARAMS) read_event_params (r, *e);
  if (row->flags & OUTPUT) ob.o = read_output (R, r);
  row->read (R, r, ob);
  if (e) R.events.push_back (std::move (e));
  if (!r.at_end_of_object ())
    r.fail ("unexpected text after " + ob.cls);
}

// the events of the file on a refined tree: refused with the line unless the table allows them
inline int check_tree_events (Run & R)
{
  const bool poisson = R.sim_class == "Poisson";
  for (auto & e : R.events) {
    const unsigned flags = find_class (e->cls)->flags;
    if (poisson && (flags & TREE_POISSON_SKIP)) {
      fprintf (stderr, "gfship: line %d: Gfs%s is not written for a refined tree (skipped)\n", e->line, e->cls.c_str ());
      e->action = [] () {};
    }
    else if (!(flags & (poisson ? TREE_POISSON : TREE))) {
      fprintf (stderr, "gfship: line %d: Gfs%s is not supported on a refined tree\n", e->line, e->cls.c_str ());
      return 1;
    }
  }
  return 0;
}

// ---- the file: its head, the objects of its body, the GfsBox and the edges
inline int side_from_name (const std::string & s)
{
  for (int d = 0; d < 6; d++)
    if (s == side_name[d]) return d;
  return -1;
}

inline void parse_box (Run & R, Reader & r)
{
  // gfs_box_read, src/domain.c:3608-3730
  std::string cls = strip_gfs (r.word ());
  if (cls != "Box") r.fail ("expecting GfsBox");
  int l0 = r.line ();
  const std::string raw = r.braces ();
  Reader b (raw, "simulation file", l0);
  while (!b.eof ()) {
    b.peek ();
    const size_t o0 = b.offset ();
    std::string k = b.word ();
    b.expect ('=');
    int d = side_from_name (k);
    if (d < 0) {
      if (k == "id" || k == "pid" || k == "size" || k == "x" || k == "y" || k == "z") { b.word (); continue; }
      b.fail ("unknown GfsBox keyword `" + k + "'");
    }
    if (d >= 2*R.dim) b.fail ("direction `" + k + "' does not exist in 2-D");
    std::string bcls = strip_gfs (b.word ());
    if (bcls != "Boundary") b.fail ("unsupported boundary class `" + bcls + "'");
    R.side[d] = GFSHIP_SIDE_BOUNDARY;
    if (b.peek (false) == '{') {
      int l1 = b.line ();
      Reader c (b.braces (), "simulation file", l1);
      while (!c.eof ()) {
        // gfs_bc_value_read, src/boundary.c:130-180
        std::string bc = strip_gfs (c.word ());
        BcSpec spec;
        if (bc == "BcDirichlet") spec.kind = GFSHIP_BC_DIRICHLET;
        else if (bc == "BcNeumann") spec.kind = GFSHIP_BC_NEUMANN;
        else c.fail ("unsupported boundary condition `" + bc + "'");
        std::string v = c.word ();
        spec.val = R.functions.add (c.function (), c.line ());
        R.bc[d][v] = spec;
      }
    }
    // kept for GfsOutputSimulation: the boundaries as the file has them (new lines folded)
    std::string piece = raw.substr (o0, b.offset () - o0);
    for (char & ch : piece) if (ch == '\n') ch = ' ';
    R.box_text += (R.box_text.empty () ? "" : " ") + piece;
  }
}

// whole-word -D substitution (the test scripts of the reference do this with sed / m4)
inline std::string substitute (const std::string & text, const std::map<std::string, std::string> & defs)
{
  if (defs.empty ()) return text;
  std::string out;
  size_t p = 0;
  while (p < text.size ()) {
    if (isalpha ((unsigned char) text[p]) || text[p] == '_') {
      size_t b = p;
      while (p < text.size () && (isalnum ((unsigned char) text[p]) || text[p] == '_')) p++;
      std::string id = text.substr (b, p - b);
      auto it = defs.find (id);
      out += it != defs.end () ? it->second : id;
    }
    else
      out += text[p++];
  }
  return out;
}

inline void parse_file (Run & R, const std::string & text, const std::string & name)
{
  Reader r (text, name);
  // `nboxes nedges SimClass BoxClass EdgeClass { graph parameters } {`, src/simulation.c:1563-1600
  int nboxes = (int) r.number ();
  int nedges = (int) r.number ();
  R.sim_class = strip_gfs (r.word ());
  r.word (); r.word ();
  if (r.peek () != '{') r.fail ("expecting an opening brace");
  r.braces ();
  if (nboxes != 1)
    r.fail ("one GfsBox per process: multi-box files map to one box per GPU through "
            "gfship/distributed.py, not through this front end");
  if (R.sim_class != "Simulation" && R.sim_class != "Poisson" && R.sim_class != "Advection")
    r.fail ("unsupported simulation class Gfs" + R.sim_class);
  // default variables of gfs_simulation_init (src/simulation.c:958-985)
  R.get_or_add_variable ("P");
  R.get_or_add_variable ("Pmac");
  for (int c = 0; c < R.dim; c++) R.get_or_add_variable (velocity_name[c]);
  if (R.sim_class == "Poisson") R.get_or_add_variable ("Div");
  {
    int l0 = r.line ();
    const std::string body_text = r.braces ();
    Reader body (body_text, name, l0);
    while (!body.eof ()) {
      const size_t o0 = body.offset ();      /* eof () has skipped the space in front */
      parse_object (R, body);
      std::string text = body_text.substr (o0, body.offset () - o0);
      std::string cls = strip_gfs (Reader (text, name).word ());
      R.object_texts.emplace_back (cls, text);
    }
  }
  parse_box (R, r);
  R.nedges = nedges;
  for (int e = 0; e < nedges; e++) {
    int a = (int) r.number (), b = (int) r.number ();
    std::string dn = r.word ();
    int d = side_from_name (dn);
    if (a != 1 || b != 1 || d < 0 || d >= 2*R.dim || (d & 1))
      r.fail ("expecting a periodic self edge `1 1 right|top|front'");
    R.side[d] = R.side[d + 1] = GFSHIP_SIDE_PERIODIC;
    R.edges_text += "1 1 " + dn + "\n";
  }
}

} // namespace gfs
