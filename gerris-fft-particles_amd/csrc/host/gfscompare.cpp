// gfscompare.cpp -- gfshipcompare2D / gfshipcompare3D: difference between the solutions of two
// simulation files for one variable, the way the reference's tools/gfscompare.c does it for two
// files with any two trees (uniform boxes, refined quadtrees / octrees, of different depths):
//
//   gfshipcompare3D [-C] [-w] [-v] [-H] FILE1 FILE2 VAR
//
//   difference_tree + inject (tools/gfscompare.c:153-214): every cell of FILE1 is located in FILE2 at its own
//     level; where FILE2 is coarser the parent takes over.  A cell none of whose children got an error gets
//     e = VAR(FILE1, cell) - VAR(FILE2, located cell) -- the located cell may be a non-leaf cell of FILE2: the
//     value its record holds is used -- and hands it to all its descendants.  The norms run over the leaves
//     of FILE1 (difference, :244-268);
//   -C  --constant      subtract the weighted mean of e first: "apply a constant shift to one of
//                       the field, minimizing the error between the two fields (useful for
//                       pressure)" (difference_constant :223-243, :657-669);
//   -w  --not-weighted  weights 1 instead of the cell volumes (:239,:266);
//   -v  --verbose       prints the norms of both fields and
//                       "total err first: %10.3e second: %10.3e infty: %10.3e w: %g" on stderr
//                       (:567-595, :683-686; gfs_norm_add / gfs_norm_update src/fluid.c:2139-2171);
//   -H  --histogram     "(error, volume fraction)" pairs on stdout (:268-269).
// Exit status 0; 1 when the files cannot be compared (another dimension, no cell data, unknown variable).
// Host arithmetic over two files: no device is involved.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <sstream>
#include <unordered_map>
#include "gfs_snapshot.hpp"

using namespace gfs;

struct Norm { double bias = 0., first = 0., second = 0., infty = -1e300, w = 0.; };

static void norm_add (Norm & n, double val, double weight)   /* gfs_norm_add, src/fluid.c:2139-2154 */
{
  n.bias += weight*val;
  val = fabs (val);
  if (weight != 0. && val > n.infty) n.infty = val;
  n.first += weight*val;
  n.second += weight*val*val;
  n.w += weight;
}

static void norm_update (Norm & n)                           /* gfs_norm_update, :2156-2171 */
{
  if (n.w > 0.) {
    n.bias /= n.w;
    n.first /= n.w;
    n.second = sqrt (n.second/n.w);
  }
  else
    n.infty = 0.;
}

static bool load (const char * name, int dim, SimulationFile & F)
{
  std::ifstream in (name, std::ios::binary);
  if (!in) { fprintf (stderr, "gfscompare: cannot open file `%s'\n", name); return false; }
  std::stringstream ss;
  ss << in.rdbuf ();
  try {
    F = split_simulation_file (ss.str (), name, dim);
  }
  catch (const ParseError & e) {
    fprintf (stderr, "gfscompare: file `%s' is not a valid simulation file\n%s\n", name, e.what ());
    return false;
  }
  if (!F.has_tree) {
    fprintf (stderr, "gfscompare: file `%s' holds no cell data\n", name);
    return false;
  }
  return true;
}

static int variable_index (const SimulationFile & F, const std::string & v)
{
  for (size_t q = 0; q < F.variables.size (); q++)
    if (F.variables[q] == v) return (int) q;
  return -1;
}

int main (int argc, char ** argv)
{
  std::string prog = argv[0];
  const int dim = prog.find ("3D") != std::string::npos ? 3 : 2;
  bool constant = false, weighted = true, verbose = false, histogram = false;
  std::vector<const char *> pos;
  for (int a = 1; a < argc; a++) {
    std::string s = argv[a];
    if (s == "-C" || s == "--constant") constant = true;
    else if (s == "-w" || s == "--not-weighted") weighted = false;
    else if (s == "-v" || s == "--verbose") verbose = true;
    else if (s == "-H" || s == "--histogram") histogram = true;
    else if (s == "-h" || s == "--help") {
      fprintf (stderr,
	       "Usage: gfscompare [OPTION] FILE1 FILE2 VAR\n"
	       "Computes the difference between the solutions in FILE1 and FILE2\n"
	       "for variable VAR.\n\n"
	       "  -C    --constant    apply a constant shift to one of the field, minimizing\n"
	       "                      the error between the two fields (useful for pressure)\n"
	       "  -w    --not-weighted do not use area-weighted norm estimation\n"
	       "  -H    --histogram   output (error,volume) pairs for each cell used\n"
	       "                      to compute the error norms\n"
	       "  -v    --verbose     display difference statistics and other info\n"
	       "  -h    --help        display this help and exit\n");
      return 0;
    }
    else if (!s.empty () && s[0] == '-') {
      fprintf (stderr, "gfscompare: option `%s' is not available here\n"
	       "Try `gfscompare --help' for more information.\n", s.c_str ());
      return 1;
    }
    else pos.push_back (argv[a]);
  }
  if (pos.size () < 1) { fprintf (stderr, "gfscompare: missing FILE1\nTry `gfscompare --help' for more information.\n"); return 1; }
  if (pos.size () < 2) { fprintf (stderr, "gfscompare: missing FILE2\nTry `gfscompare --help' for more information.\n"); return 1; }
  if (pos.size () < 3) { fprintf (stderr, "gfscompare: missing VAR\nTry `gfscompare --help' for more information.\n"); return 1; }
  SimulationFile F1, F2;
  if (!load (pos[0], dim, F1) || !load (pos[1], dim, F2)) return 1;
  const std::string var = pos[2];
  int v1 = variable_index (F1, var), v2 = variable_index (F2, var);
  if (v1 < 0) { fprintf (stderr, "gfscompare: unknown variable `%s' for `%s'\nTry `gfscompare --help' for more information.\n", var.c_str (), pos[0]); return 1; }
  if (v2 < 0) { fprintf (stderr, "gfscompare: unknown variable `%s' for `%s'\nTry `gfscompare --help' for more information.\n", var.c_str (), pos[1]); return 1; }
  const size_t rec1 = tree_record (F1.variables.size ()), rec2 = tree_record (F2.variables.size ());
  auto value = [] (const SimulationFile & F, size_t rec, size_t cell, int v) {
    double x;
    memcpy (&x, F.tree.data () + cell*rec + 12 + 8*(size_t) v, 8);
    return x;
  };
  auto volume = [dim] (const TreeCell & c) {       /* ftt_cell_volume */
    const double h = 1./(1 << c.level);
    return dim == 3 ? h*h*h : h*h;
  };
  if (verbose)
    for (int f = 0; f < 2; f++) {
      const SimulationFile & F = f ? F2 : F1;
      Norm n;
      double mn = 1e300, mx = -1e300, sum = 0., sum2 = 0., cnt = 0.;
      for (const TreeCell & c : F.cells) {
	if (!c.leaf) continue;
	const double v = value (F, f ? rec2 : rec1, c.rec, f ? v2 : v1);
	norm_add (n, v, volume (c));
	if (v < mn) mn = v;
	if (v > mx) mx = v;
	sum += v; sum2 += v*v; cnt += 1.;
      }
      norm_update (n);
      double mean = sum/cnt;
      double sd = sqrt (fmax (0., sum2/cnt - mean*mean));
      fprintf (stderr, "%s:\n  first: %g second: %g infty: %g w: %g\n  min: %g avg: %g | %g max: %g\n",
	       pos[f], n.first, n.second, n.infty, n.w, mn, mean, sd, mx);
    }
  // gfs_domain_locate (FILE2, centre of the cell, its level): the cell of FILE2 with the same level and coordinates,
  // if FILE2 is refined that far there
  auto key = [] (const TreeCell & c) {
    return ((((uint64_t) c.level << 19 | (uint64_t) c.k) << 19 | (uint64_t) c.j) << 19) | (uint64_t) c.i;
  };
  if (F1.depth > 19 || F2.depth > 19) { fprintf (stderr, "gfscompare: the files are not comparable\n"); return 1; }
  std::unordered_map<uint64_t, size_t> in2;
  in2.reserve (F2.cells.size ()*2);
  for (const TreeCell & c : F2.cells) in2[key (c)] = c.rec;
  const int nc = dim == 3 ? 8 : 4;
  const std::vector<TreeCell> & C1 = F1.cells;
  std::vector<double> err (C1.size (), 0.);
  struct Walk {
    const std::vector<TreeCell> & C;
    int nc;
    void skip (size_t & q) const { const bool leaf = C[q++].leaf; if (!leaf) for (int n = 0; n < nc; n++) skip (q); }
  } walk = { C1, nc };
  std::function<bool (size_t &)> difference_tree = [&] (size_t & q) -> bool {
    const size_t me = q;
    auto located = in2.find (key (C1[me]));
    if (located == in2.end ()) {     /* ftt_cell_level (locate) != level */
      walk.skip (q);
      return false;
    }
    bool added = false;
    q++;
    if (!C1[me].leaf)
      for (int n = 0; n < nc; n++)
	if (difference_tree (q)) added = true;
    if (!added) {
      const double e = value (F1, rec1, me, v1) - value (F2, rec2, located->second, v2);
      for (size_t d = me; d < q; d++) err[d] = e;      /* inject: the records of a subtree follow each other */
    }
    return true;
  };
  {
    size_t q = 0;
    if (!difference_tree (q)) { fprintf (stderr, "gfscompare: the files are not comparable\n"); return 1; }
  }
  std::vector<double> e, ew;
  for (const TreeCell & c : C1)
    if (c.leaf) {
      e.push_back (err[c.rec]);
      ew.push_back (weighted ? volume (c) : 1.);
    }
  double shift = 0.;
  if (constant) {
    double sum = 0., weight = 0.;
    for (size_t q = 0; q < e.size (); q++) { sum += ew[q]*e[q]; weight += ew[q]; }
    shift = weight > 0. ? sum/weight : 0.;
  }
  Norm n;
  for (size_t q = 0; q < e.size (); q++) {
    norm_add (n, e[q] - shift, ew[q]);
    if (histogram) printf ("%g %g\n", e[q], 1.);
  }
  norm_update (n);
  if (verbose)
    fprintf (stderr, "total err first: %10.3e second: %10.3e infty: %10.3e w: %g\n",
	     n.first, n.second, n.infty, n.w);
  return 0;
}
