// gfsrun.cpp -- `gfship2D` / `gfship3D`: run a Gerris simulation file (.gfs) on libgfship.
//
// The host side of the drop-in: it reads the reference's simulation-file format, builds the
// domain and the simulation through the C ABI of include/gfship.h (nothing else is called),
// and drives the reference's event loop:
//   GfsSimulation   simulation_run     src/simulation.c:432-557
//   GfsPoisson      poisson_run        src/simulation.c:2213-2285
// with the events and outputs the reference's own test cases use (test/poisson, test/lid,
// test/reynolds, test/periodic ...), printed in the reference's formats so that the awk/python
// checks of test/*/*.sh read them unchanged.  What is supported is the table at the end of gfs_classes.hpp (one
// row per class of the file); anything else fails loudly with the line number.  --particles FILE writes the
// particle lists at the end of the run the way the reference prints them.
//
//   gfship2D [-D NAME=VALUE ...] [--device N] [--particles FILE] file.gfs     (gfship3D for three dimensions)
#include "gfs_run.hpp"        // the model: variables, events, outputs, the specs, Run; the host copies of the fields
#include "gfs_classes.hpp"    // one reader per class of the file, and the table of them
#include "gfs_drive.hpp"      // the run: set-up of the device simulation, the event loop, the time loops

using namespace gfs;

// --check: parse, compile the functions and describe the run without touching a device
int check (Run & R)
{
  add_derived (R);
  R.functions.resolve (R.var_names ());
  resolve_refine (R);
  printf ("class Gfs%s dim %d level %d%s\n", R.sim_class.c_str (), R.dim, R.level,
	  R.tree_mode ? " (coarsest leaves of a refined tree)" : "");
  if (R.tree_mode && R.sim_class == "Simulation" && check_tree_events (R))
    return 1;               /* an event that is refused on a refined tree, with its line */
  if (R.tree_mode)        /* no host copies of fields without the tree, which needs the device */
    R.init.clear ();
  printf ("sides");
  for (int d = 0; d < 2*R.dim; d++)
    printf (" %s=%s", side_name[d], R.side[d] == GFSHIP_SIDE_PERIODIC ? "periodic" : "boundary");
  printf ("\ntime t %g i %u end %g iend %u\n", R.t, R.i, R.end, R.iend);
  double p[3] = { 0.125, -0.25, R.dim == 3 ? 0.375 : 0. };
  for (auto & kv : R.init) {
    if (!kv.second->reads ().empty ()) printf ("init %s = <function of variables>\n", kv.first.c_str ());
    else printf ("init %s (0.125,-0.25,%g) = %.17g\n", kv.first.c_str (), p[2], eval (R, kv.second, p, -1));
  }
  for (int d = 0; d < 2*R.dim; d++)
    for (auto & kv : R.bc[d])
      printf ("bc %s %s %s %.17g\n", side_name[d], kv.first.c_str (),
	      kv.second.kind == GFSHIP_BC_DIRICHLET ? "dirichlet" : "neumann",
	      eval (R, kv.second.val, p, -1));
  for (int c = 0; c < R.dim; c++)
    if (R.visc[c] != 0.) printf ("viscosity %d %g\n", c, R.visc[c]);
    else if (R.visc_fn[c]) printf ("viscosity %d function\n", c);
  for (auto & e : R.events)
    printf ("event %s line %d start %g step %g istep %u end_event %d\n", e->cls.c_str (), e->line,
	    e->start, e->step == DBL_MAX ? -1. : e->step, e->istep == INT_MAX ? 0 : e->istep,
	    (int) e->end_event);
  return 0;
}

int main (int argc, char ** argv)
{
  Run R;
  bool check_only = false;
  // dimension from the program name, like gerris2D / gerris3D
  std::string prog = argv[0];
  R.dim = prog.find ("3D") != std::string::npos ? 3 : 2;
  std::map<std::string, std::string> defs;
  std::string file;
  for (int a = 1; a < argc; a++) {
    std::string s = argv[a];
    if (s == "-2") R.dim = 2;
    else if (s == "-3") R.dim = 3;
    else if (s == "--device" && a + 1 < argc) R.device = atoi (argv[++a]);
    else if (s == "--check") check_only = true;
    else if (s == "--particles" && a + 1 < argc) R.particles_out = argv[++a];
    else if (s.compare (0, 2, "-D") == 0) {
      std::string d = s.size () > 2 ? s.substr (2) : (a + 1 < argc ? argv[++a] : "");
      size_t eq = d.find ('=');
      if (eq == std::string::npos) defs[d] = "1";
      else defs[d.substr (0, eq)] = d.substr (eq + 1);
    }
    else if (s == "-h" || s == "--help") {
      printf ("Usage: %s [-2|-3] [-DNAME=VALUE] [--device N] [--particles FILE] file.gfs\n", argv[0]);
      return 0;
    }
    else file = s;
  }
  if (file.empty ()) { fprintf (stderr, "gfship: no simulation file given\n"); return 1; }
  g_shell.start ();
  struct ShellStop { ~ShellStop () { g_shell.stop (); } } shell_stop;
  std::stringstream ss;
  if (file == "-")                       /* `gerris2D -': the simulation file on standard input */
    ss << std::cin.rdbuf ();
  else {
    std::ifstream in (file);
    if (!in) { fprintf (stderr, "gfship: cannot open `%s'\n", file.c_str ()); return 1; }
    ss << in.rdbuf ();
  }
  try {
    // a file with cell data (a snapshot written by GfsOutputSimulation): the data is cut out
    // before the text is parsed
    R.snapshot = gfs::split_simulation_file (ss.str (), file, R.dim);
    parse_file (R, substitute (R.snapshot.text, defs), file);
    R.snapshot.text.clear ();
    for (const std::string & nm : R.snapshot.variables)
      R.get_or_add_variable (nm);        /* gfs_domain_add_variable of domain_read, src/domain.c:283-293 */
    if (R.snapshot.has_tree && !R.snapshot.uniform) {
      /* the tree of the file is the tree (cell_read, src/ftt.c:1807-1866): gfship_tree */
      if (R.sim_class != "Simulation") {
	fprintf (stderr, "gfship: cell data on a refined tree is read for a GfsSimulation only\n");
	return 1;
      }
      R.tree_mode = true;
      R.level = R.snapshot.depth;
      for (const gfs::TreeCell & c : R.snapshot.cells)
	if (c.leaf && c.level < R.level) R.level = c.level;      /* the coarsest leaves */
    }
    else if (R.snapshot.has_tree && R.level == 0 && R.snapshot.depth > 0)
      R.level = R.snapshot.depth;        /* no GfsRefine in a file that carries its tree */
    return check_only ? check (R) : run (R);
  }
  catch (const ParseError & e) {
    fprintf (stderr, "gfship: %s\n", e.what ());
    return 1;
  }
}
