// gfs_snapshot.hpp -- a Gerris simulation file that carries cell data (what GfsOutputSimulation
// writes and `gerris' restarts from): taking the file apart and putting one together.
//
//   # Gerris Flow Solver 3D version ...
//   1 3 GfsSimulation GfsBox GfsGEdge { version = 120812 variables = P,Pmac,U,V,W binary = 1 } {
//     GfsTime { i = 12 t = 0.3 } ...objects...
//   }
//   GfsBox { id = 1 pid = -1 size = 4096 x = 0 y = 0 z = 0 ... } {
//   <cell tree: ftt_cell_write_binary / ftt_cell_write, src/ftt.c:1728-1799>}
//   1 1 right
//
// (simulation_write src/simulation.c:77-170, domain_write src/domain.c:168-209, gfs_box_write
// src/boundary.c:1819-1851).  The tree is binary (`binary = 1': guint flags, double -1., one double
// per variable, pre-order) or text (one line per cell: `flags -1 v1 v2 ...' in %g).  The tree is whatever the
// leaf bits of the records say (a uniform box or a refined quadtree / octree).  Shared by the front end (restart,
// OutputSimulation) and by the comparison tool; host code only.
#pragma once
#include "gfs_text.hpp"
#include <cstdint>
#include <cstdio>

namespace gfs {

// a cell of the tree of a file: its level, its integer coordinates on that level (0-based, growing with x, y, z;
// k = 0 in 2-D), whether it is a leaf, and the index of its record in the image (= its position in file order)
struct TreeCell { int level, i, j, k; bool leaf; size_t rec; };

struct SimulationFile {
  std::string text;                     // the file without the cell data (what the parser reads)
  bool has_tree = false, binary = false;
  std::vector<std::string> variables;   // variables = a,b,c of the graph parameters
  std::string tree;                     // the cell data as the binary image (converted if text)
  int dim = 0, depth = -1;              // depth: the deepest level of the tree
  bool uniform = true;                  // every leaf is on that level
  std::vector<TreeCell> cells;          // the tree of the file, taken from its leaf bits, in file order
};

inline std::vector<std::string> split_commas (const std::string & s)
{
  std::vector<std::string> out;
  size_t b = 0;
  while (b <= s.size ()) {
    size_t e = s.find (',', b);
    if (e == std::string::npos) e = s.size ();
    if (e > b) out.push_back (s.substr (b, e - b));
    b = e + 1;
  }
  return out;
}

inline size_t tree_record (size_t nvars) { return 4 + 8 + 8*nvars; }

// The tree of a binary image: the records are walked in pre-order (cell_read_binary, src/ftt.c:1913-1975: a
// cell without the leaf bit is followed by its FTT_CELLS children, whose ids must be 0 .. FTT_CELLS - 1 in turn).
// Returns the cells in file order; throws if the image ends inside the tree.
inline std::vector<TreeCell> tree_view (const char * p, size_t avail, size_t rec, int dim,
					const std::string & name)
{
  std::vector<TreeCell> out;
  struct Frame { int level, i, j, k, next; };
  std::vector<Frame> stack;
  const int nc = dim == 3 ? 8 : 4;
  TreeCell c = { 0, 0, 0, 0, false, 0 };
  unsigned expect = 0;
  for (;;) {
    if ((out.size () + 1)*rec > avail) throw ParseError (name + ": truncated cell data");
    uint32_t flags;
    memcpy (&flags, p + out.size ()*rec, 4);
    if ((flags & 7u) != expect)
      throw ParseError (name + ": FTT_CELL_ID (cell) != (flags & FTT_FLAG_ID): make sure the file has " +
			std::to_string (dim) + " spatial dimensions");
    c.leaf = (flags & 16u) != 0;
    c.rec = out.size ();
    out.push_back (c);
    if (!c.leaf) {
      if (c.level >= 30) throw ParseError (name + ": the tree of the cell data is too deep");
      stack.push_back ({ c.level, c.i, c.j, c.k, 0 });
    }
    while (!stack.empty () && stack.back ().next == nc) stack.pop_back ();
    if (stack.empty ()) break;
    Frame & f = stack.back ();
    const int n = f.next++;     /* child n: bit 0 = +x half, bit 1 = -y half, bit 2 = -z half */
    c.level = f.level + 1;
    c.i = 2*f.i + (n & 1);
    c.j = 2*f.j + 1 - ((n >> 1) & 1);
    c.k = dim == 3 ? 2*f.k + 1 - ((n >> 2) & 1) : 0;
    expect = (unsigned) n;
  }
  return out;
}

// a text tree (ftt_cell_write + gfs_cell_write) into the binary image; returns the characters used
inline size_t tree_text_to_binary (const std::string & s, size_t b, size_t nvars, int dim,
				   std::string & out, int & depth)
{
  size_t p = b;
  depth = -1;
  // iterative pre-order walk: the stack holds the number of children still to come per level
  std::vector<int> todo;
  int level = 0;
  auto number = [&] (double & v) -> bool {
    while (p < s.size () && isspace ((unsigned char) s[p])) p++;
    char * end;
    v = strtod (s.c_str () + p, &end);
    if (end == s.c_str () + p) return false;
    p = (size_t) (end - s.c_str ());
    return true;
  };
  for (;;) {
    double f, m;
    if (!number (f) || !number (m)) throw ParseError ("cell data: expecting `flags -1 values...'");
    if (m != -1.) throw ParseError ("cell data: solid fractions (mixed cells) are not supported");
    uint32_t flags = (uint32_t) f;
    out.append ((const char *) &flags, 4);
    out.append ((const char *) &m, 8);
    for (size_t v = 0; v < nvars; v++) {
      double x;
      if (!number (x)) throw ParseError ("cell data: expecting a number");
      out.append ((const char *) &x, 8);
    }
    if (level > depth) depth = level;
    if (flags & 16u) {
      // next sibling, or up
      while (!todo.empty () && --todo.back () == 0) { todo.pop_back (); level--; }
      if (todo.empty ()) break;
    }
    else {
      todo.push_back (dim == 3 ? 8 : 4);
      level++;
    }
  }
  return p - b;
}

// Cuts the cell data out of the text of a simulation file.  dim: 2 or 3 (the program's).
inline SimulationFile split_simulation_file (const std::string & all, const std::string & name,
					     int dim)
{
  SimulationFile F;
  F.dim = dim;
  Reader r (all, name);
  r.number (); r.number ();
  r.word (); r.word (); r.word ();
  {
    int l0 = r.line ();
    Reader g (r.braces (), name, l0);
    while (!g.eof ()) {
      std::string k = g.word ();
      g.expect ('=');
      std::string v = g.word ();
      if (k == "variables") F.variables = split_commas (v);
      else if (k == "binary") F.binary = atoi (v.c_str ()) != 0;
    }
  }
  r.braces ();                       // the simulation body
  if (r.eof ()) { F.text = all; return F; }
  r.word ();                         // GfsBox
  r.braces ();                       // its parameters
  if (r.peek (false) != '{') { F.text = all; return F; }
  // `{', then the data, then `}'
  size_t open = all.find ('{', r.offset ());
  size_t b = open + 1;
  size_t used;
  const size_t rec = tree_record (F.variables.size ());
  if (F.binary) {
    if (b >= all.size () || all[b] != '\n') throw ParseError (name + ": expecting a newline before the binary cell data");
    b++;
    F.cells = tree_view (all.data () + b, all.size () - b, rec, dim, name);
    used = F.cells.size ()*rec;
    F.tree.assign (all, b, used);
  }
  else {
    used = tree_text_to_binary (all, b, F.variables.size (), dim, F.tree, F.depth);
    F.cells = tree_view (F.tree.data (), F.tree.size (), rec, dim, name);
  }
  F.depth = 0;
  for (const TreeCell & c : F.cells)
    if (c.level > F.depth) F.depth = c.level;
  for (const TreeCell & c : F.cells)
    if (c.leaf && c.level != F.depth) F.uniform = false;
  size_t close = b + used;
  while (close < all.size () && isspace ((unsigned char) all[close])) close++;
  if (close >= all.size () || all[close] != '}')
    throw ParseError (name + ": expecting a closing brace after the cell data "
		      "(make sure the file has " + std::to_string (dim) + " spatial dimensions)");
  F.has_tree = true;
  F.text = all.substr (0, open) + all.substr (close + 1);
  return F;
}

// the leaves of variable v of a binary image, in the order of the file (the traversal order)
inline std::vector<double> tree_leaves (const std::string & tree, size_t nvars, size_t v)
{
  const size_t rec = tree_record (nvars);
  std::vector<double> out;
  for (size_t o = 0; o + rec <= tree.size (); o += rec) {
    uint32_t flags;
    memcpy (&flags, tree.data () + o, 4);
    if (flags & 16u) {
      double x;
      memcpy (&x, tree.data () + o + 12 + 8*v, 8);
      out.push_back (x);
    }
  }
  return out;
}

// ftt_cell_write + gfs_cell_write (text) of a binary image
inline void tree_write_text (FILE * fp, const std::string & tree, size_t nvars)
{
  const size_t rec = tree_record (nvars);
  for (size_t o = 0; o + rec <= tree.size (); o += rec) {
    uint32_t flags;
    memcpy (&flags, tree.data () + o, 4);
    fprintf (fp, "%u -1", flags);
    for (size_t v = 0; v < nvars; v++) {
      double x;
      memcpy (&x, tree.data () + o + 12 + 8*v, 8);
      fprintf (fp, " %g", x);
    }
    fputc ('\n', fp);
  }
}

} // namespace gfs
