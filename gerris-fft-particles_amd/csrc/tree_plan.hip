// tree_plan.hip -- the planner of a refined tree (tree_plan.hpp): plain host C++, no device call and no kernel.
// It is a .hip file so that build.sh compiles it with the flags of the rest (-ffp-contract=off: the coefficient
// stream td is floating point computed here, and the host checks must round as the kernels do).
//
//  * the tree: refinement with the neighbour and corner rules, the match of the ghost trees, the tables of Topo,
//    the traversals and their lists (plan_tree);
//  * the sweep of gfs_relax on a level in dependency levels and its compiled stencils (plan_sweep): the host
//    derives, from the very stencil code the kernels run (tree.hpp with a recording reader), which cells each cell
//    reads;
//  * a whole relax loop as one list of nodes (plan_loop) and as a flow plan (plan_flow);
//  * the face sets (plan_faces); the reference's diffusion coefficients (diffusion_weights_exact);
//  * the host checks of all this, and the digests of the plans (the lab entries at the end).
//
// Restated here: src/ftt.c:45-83,169-192,689-926,2013-2074,2152-2215, src/ftt_internal.c:1-42,
// src/poisson.c:604-632,826-853,1070-1089,1280-1303,1350-1390.
#include "gfship_internal.hpp"
#include "tree_plan.hpp"
#include "tree_tape.hpp"
#include <algorithm>
#include <array>
#include <cstring>
#include <functional>
#include <new>

namespace gfship { namespace tree {

namespace {

// ---- tree construction and lists -------------------------------------------------------------------

struct Builder {
  int dim = 2;
  std::vector<std::vector<unsigned char>> flag;     // per level, (n + 2)^dim
  int r (int l) const { return (1 << l) + 2; }
  size_t idx (int l, int i, int j, int k) const { return i + (size_t) r (l)*(j + (dim == 3 ? (size_t) r (l)*k : 0)); }
  // cells of the dense levels allocated so far; the limit of gfship_tree_create (32-bit cell indices
  // times the number of directions in the tables) is enforced BEFORE a level is allocated: a Refine
  // function asking for level 10 in 3-D would otherwise allocate 1, 8.6, 68 GB on the host first
  long long total = 0;
  bool too_large = false;
  static constexpr long long MAX_CELLS = 1ll << 27;
  bool ensure (int l) {
    if ((int) flag.size () <= l) flag.resize (l + 1);
    if (flag[l].empty ()) {
      const long long cells = (long long) r (l)*r (l)*(dim == 3 ? r (l) : 1);
      if (total + cells > MAX_CELLS) { too_large = true; return false; }
      total += cells;
      flag[l].assign ((size_t) cells, NONE);
    }
    return true;
  }
  // oct_new with check_neighbors, src/ftt.c:45-83
  int refine_single (int l, int i, int j, int k) {
    if (l + 1 > GFSHIP_MAXLEVEL) return GFSHIP_EUNSUPPORTED;
    static const int di[6] = { 1, -1, 0, 0, 0, 0 }, dj[6] = { 0, 0, 1, -1, 0, 0 }, dk[6] = { 0, 0, 0, 0, 1, -1 };
    const int n = 1 << l;
    for (int d = 0; d < 2*dim; d++) {
      const int ni = i + di[d], nj = j + dj[d], nk = k + dk[d];
      if (ni < 1 || nj < 1 || ni > n || nj > n || (dim == 3 && (nk < 1 || nk > n)))
	continue;                   // the ghost trees are matched at the end (gfs_domain_match)
      if (flag[l][idx (l, ni, nj, nk)] == NONE) {
	const int pi = (ni + 1)/2, pj = (nj + 1)/2, pk = (nk + 1)/2;
	if (flag[l - 1][idx (l - 1, pi, pj, pk)] == LEAF) {
	  int e = refine_single (l - 1, pi, pj, pk);
	  if (e) return e;
	}
      }
    }
    if (!ensure (l + 1)) return GFSHIP_EUNSUPPORTED;
    flag[l][idx (l, i, j, k)] = NODE;
    for (int c = 0; c < (1 << dim); c++)
      flag[l + 1][idx (l + 1, 2*i - 1 + (c & 1), 2*j - ((c >> 1) & 1), 2*k - ((c >> 2) & 1))] = LEAF;
    return 0;
  }
  // ftt_cell_refine (src/ftt.c:169-192) with refine_maxlevel (src/refine.c:35-38)
  int refine_rec (int l, int i, int j, int k, gfship_refine_fn fn, void * ctx) {
    if (flag[l][idx (l, i, j, k)] == LEAF) {
      const double h = 1./(1 << l);
      const double x = -0.5 + (i - 0.5)*h, y = -0.5 + (j - 0.5)*h, z = dim == 3 ? -0.5 + (k - 0.5)*h : 0.;
      if (!(l < (* fn) (x, y, z, ctx)))
	return 0;
      int e = refine_single (l, i, j, k);
      if (e) return e;
    }
    for (int c = 0; c < (1 << dim); c++) {
      int e = refine_rec (l + 1, 2*i - 1 + (c & 1), 2*j - ((c >> 1) & 1), 2*k - ((c >> 2) & 1), fn, ctx);
      if (e) return e;
    }
    return 0;
  }
};

typedef std::function<void (Cell)> CellFn;
enum { T_ALL, T_LEAFS, T_NON_LEAFS, T_LEVEL, T_LEVEL_LEAFS, T_LEVEL_NON_LEAFS };

// ftt_cell_traverse, src/ftt.c:689-926 (pre-order; the post-order loops are done level by level)
void traverse (const Topo & T, Cell c, int flags, int max_depth, const CellFn & fn)
{
  const bool leaf = T.leaf (c);
  bool visit = false, descend = !leaf;
  if (flags == T_ALL || flags == T_LEAFS || flags == T_NON_LEAFS) {
    if (max_depth >= 0 && c.l > max_depth)
      return;
    visit = flags == T_ALL || (flags == T_LEAFS ? leaf : !leaf);
  }
  else if (flags == T_LEVEL) {
    visit = c.l == max_depth;
    descend = !visit && !leaf;
  }
  else if (flags == T_LEVEL_LEAFS) {
    visit = c.l == max_depth || leaf;
    descend = !visit;
  }
  else {
    visit = c.l == max_depth && !leaf;
    descend = !visit && !leaf;
  }
  if (visit)
    fn (c);
  if (descend)
    for (int k = 0; k < T.nc (); k++) {
      const Cell ch = T.child (c, k);
      if (exists (ch))
	traverse (T, ch, flags, max_depth, fn);
    }
}

// ftt_refine_corner, src/ftt.c:2013-2074
bool refine_corner (const Topo & T, Cell cell)
{
  static const int perp2[4][2] = { {2, 3}, {2, 3}, {1, 0}, {1, 0} };
  static const int perp3[6][4][2] =
    {{{4,2},{4,3},{5,2},{5,3}}, {{4,2},{4,3},{5,2},{5,3}},
     {{4,1},{4,0},{5,1},{5,0}}, {{4,1},{4,0},{5,1},{5,0}},
     {{2,1},{2,0},{3,1},{3,0}}, {{2,1},{2,0},{3,1},{3,0}}};
  for (int i = 0; i < T.nd (); i++) {
    const Cell nb = T.neighbor (cell, i);
    if (exists (nb) && !T.leaf (nb))
      for (int j = 0; j < T.ncd (); j++) {
	const Cell c = T.child_direction (nb, i ^ 1, j);
	if (exists (c)) {
	  if (T.dim == 2) {
	    const Cell nc = T.neighbor (c, perp2[i][j]);
	    if (exists (nc) && !T.leaf (nc))
	      return true;
	  }
	  else
	    for (int w = 0; w < 2; w++) {
	      const Cell nc = T.neighbor (c, perp3[i][j][w]);
	      if (exists (nc) && !T.leaf (nc))
		return true;
	    }
	  if (!T.leaf (c))
	    return true;
	}
      }
  }
  return false;
}

// traverse_face, src/ftt_internal.c:1-42 (leaves, max_depth = -1; the FTT_FLAG_TRAVERSED check
// only matters for the second pass, whose neighbours are ghost cells)
void traverse_face (const Topo & T, Cell cell, int d, std::vector<FaceRec> & out)
{
  FaceRec f = { cell, T.neighbor (cell, d), d };
  if (!exists (f.neighbor))
    return;
  if (T.leaf (cell) && !T.leaf (f.neighbor)) {
    const Cell coarse = cell, node = f.neighbor;
    f.d = d ^ 1;
    f.neighbor = coarse;
    for (int i = 0; i < T.ncd (); i++) {
      f.cell = T.child_direction (node, f.d, i);
      if (exists (f.cell))
	out.push_back (f);
    }
  }
  else
    out.push_back (f);
}

bool touches_side (const Topo & T, Cell c, int d)
{
  const int i = T.ci (c), j = T.cj (c), k = T.ck (c), n = T.n (c.l);
  return (d == 0 && i == n) || (d == 1 && i == 1) || (d == 2 && j == n) || (d == 3 && j == 1) ||
    (d == 4 && k == n) || (d == 5 && k == 1);
}

// ftt_face_traverse (src/ftt.c:2152-2215) as called by gfs_domain_face_traverse: kind 0 = FTT_XYZ,
// 1 + c = component c
void face_list (const Topo & T, const std::vector<Cell> & leaves, int kind, std::vector<FaceRec> & out)
{
  if (kind == 0) {
    for (Cell c : leaves)
      for (int d = 0; d < T.nd (); d += 2)
	traverse_face (T, c, d, out);
    for (int d = 1; d < T.nd (); d += 2)
      for (Cell c : leaves)
	if (touches_side (T, c, d))
	  traverse_face (T, c, d, out);
  }
  else {
    const int c0 = kind - 1;
    for (Cell c : leaves)
      traverse_face (T, c, 2*c0, out);
    for (Cell c : leaves)
      if (touches_side (T, c, 2*c0 + 1))
	traverse_face (T, c, 2*c0 + 1, out);
  }
}

// every ghost position of level l, side by side: fn (side, G, I, O) with the places in the level of the ghost
// cell, of its periodic image and of the cell it touches
template <class F> void ghost_positions (int dim, int l, F fn)
{
  const int n = 1 << l, r = n + 2;
  for (int side = 0; side < 2*dim; side++)
    for (int tb = 1; tb <= (dim == 3 ? n : 1); tb++)
      for (int ta = 1; ta <= n; ta++) {
	int g[3], im[3], own[3];
	const int a = side/2, o1 = a == 0 ? 1 : 0, o2 = a == 2 ? 1 : 2;
	g[a] = (side & 1) ? 0 : n + 1;
	im[a] = (side & 1) ? n : 1;
	own[a] = (side & 1) ? 1 : n;
	g[o1] = im[o1] = own[o1] = ta;
	g[o2] = im[o2] = own[o2] = dim == 3 ? tb : 0;
	fn (side, g[0] + r*(g[1] + r*g[2]), im[0] + r*(im[1] + r*im[2]), own[0] + r*(own[1] + r*own[2]));
      }
}

// the ghost cells of a selection of the traversal and their periodic images
void ghost_list (const Topo & T, const int * sides, int flags, int max_depth, std::vector<Ghost> & out)
{
  for (int l = 0; l <= T.depth; l++) {
    if (max_depth >= 0 && l > max_depth)
      break;
    ghost_positions (T.dim, l, [&] (int side, int G, int I, int O) {
	const unsigned char f = T.flag[T.off[l] + G];
	if (f == NONE)
	  return;
	const bool take = flags == T_LEAFS ? f == LEAF : (l == max_depth || f == LEAF);
	if (take)      /* GfsBoundary: the cell the ghost touches */
	  out.push_back ({ T.off[l] + G, T.off[l] + (sides[side] != GFSHIP_SIDE_PERIODIC ? O : I), side, l });
      });
  }
}

struct Recorder {           // which cells does the stencil read?
  std::vector<int> * out;
  inline double operator() (const Topo & T, Cell c) const { out->push_back (T.gi (c)); return 1.; }
};

// ---- dependency levels -----------------------------------------------------------------------------
// The sequential program [copies of the ghosts][sweep 0 in tree order][copies][sweep 1] ... scheduled into levels
// that keep the order of every read after the write it must see, and of every write after the reads of the value
// it replaces (RAW, WAR, WAW): wlev / rlev are the levels of the last write / of the last read since of a cell
struct LevelScheduler {
  std::vector<int> wlev, rlev;
  int nlev = 0;
  explicit LevelScheduler (int ncell) : wlev (ncell, 0), rlev (ncell, 0) {}
  int ghost (const Ghost & G)
  {
    const int L = std::max (wlev[G.img], std::max (rlev[G.g], wlev[G.g])) + 1;
    rlev[G.img] = std::max (rlev[G.img], L);
    wlev[G.g] = L; rlev[G.g] = 0;
    nlev = std::max (nlev, L);
    return L;
  }
  int cell (int w, const int * reads, const int * reads_end)
  {
    int L = std::max (rlev[w], wlev[w]);
    for (const int * g = reads; g < reads_end; g++) L = std::max (L, wlev[*g]);
    L++;
    for (const int * g = reads; g < reads_end; g++) rlev[*g] = std::max (rlev[*g], L);
    wlev[w] = L; rlev[w] = 0;
    nlev = std::max (nlev, L);
    return L;
  }
};

// chunks: consecutive items of one level whose streams fit the LDS.  off: the start of each item in ti / td / tv
// (3 per item, + the end); bounds: the first item of each level, + the end.  The first item of each chunk goes to
// `chunk'; false: one item larger than the LDS (cannot happen)
bool lds_chunks (const std::vector<int> & off, const std::vector<int> & bounds, std::vector<int> & chunk)
{
  for (size_t L = 0; L + 1 < bounds.size (); L++) {
    int c = bounds[L];
    while (c < bounds[L + 1]) {
      chunk.push_back (c);
      int e = c;
      while (e < bounds[L + 1]) {
	const size_t bytes = 8*(size_t) (off[3*(e + 1) + 2] - off[3*c + 2]) +
	  8*(size_t) (off[3*(e + 1) + 1] - off[3*c + 1]) + 4*(size_t) (off[3*(e + 1)] - off[3*c]) + 8;
	if (bytes > TAPE_LDS_BYTES)
	  break;
	e++;
      }
      if (e == c) return false;
      c = e;
    }
  }
  return true;
}

// ---- compiled stencils -----------------------------------------------------------------------------

struct TapeOut { std::vector<int> ti, tv; std::vector<double> td; };

// interpolate_1D1 / interpolate_2D1 in the coarse cell A towards the fine cell (face: fine -> A in
// direction dface), src/fluid.c:178-245: the terms of p.b go to the streams, p.a is returned
double tape_interpolation_gen (const Topo & T, Cell fine, Cell A, int dface, TapeOut & o)
{
  const int id = T.id (fine);
  int dirs[2], ndirs;
  if (T.dim == 2) { dirs[0] = perpendicular (dface, id); ndirs = 1; }
  else { dirs[0] = perpendicular3 (dface, id, 0); dirs[1] = perpendicular3 (dface, id, 1); ndirs = 2; }
  double pa = 1.;
  const size_t nt_at = o.ti.size ();
  o.ti.push_back (0);
  int nt = 0;
  for (int w = 0; w < ndirs; w++) {
    const Cell nb = T.neighbor (A, dirs[w]);
    if (!exists (nb))
      continue;
    double x2 = 1.;
    std::vector<int> idx;
    int cnt = 0;
    if (T.leaf (nb))
      idx.push_back (T.gi (nb));
    else {
      for (int i = 0; i < T.ncd (); i++) {
	const Cell ch = T.child_direction (nb, dirs[w] ^ 1, i);
	if (exists (ch)) { idx.push_back (T.gi (ch)); cnt++; }
      }
      if (cnt > 0)
	x2 = 3./4.;
      else
	idx.push_back (T.gi (A));       /* average_neighbor_value falls back on the cell of the face */
    }
    const double a = (1./4.)/x2;
    o.td.push_back (a);
    o.ti.push_back (cnt);
    for (int g : idx) o.tv.push_back (g);
    pa -= a;
    nt++;
  }
  o.ti[nt_at] = nt;
  return pa;
}

// gradient_fine_coarse across the face fine -> A: the coefficient 2 p.a/3, the cell `first' whose value it
// multiplies (or that takes 2/3), then the interpolation
void tape_item_gen (const Topo & T, Cell fine, Cell A, int dface, Cell first, TapeOut & o)
{
  const size_t at = o.td.size ();
  o.td.push_back (0.);
  o.tv.push_back (T.gi (first));
  o.td[at] = 2.*tape_interpolation_gen (T, fine, A, dface, o)/3.;
}

// one cell of the sweep of level max_level: what face_gradient (tree.hpp) does for each direction
void tape_cell_gen (const Topo & T, Cell cell, int max_level, TapeOut & o)
{
  o.tv.push_back (T.gi (cell));          /* the value of the cell itself */
  for (int d = 0; d < T.nd (); d++) {
    const Cell nb = T.neighbor (cell, d);
    if (!exists (nb)) { o.ti.push_back (K_NONE); continue; }
    if (nb.l < cell.l) {
      o.ti.push_back (K_FC);
      tape_item_gen (T, cell, nb, d, nb, o);
    }
    else if (cell.l == max_level || T.leaf (nb)) {
      o.ti.push_back (K_SAME);
      o.tv.push_back (T.gi (nb));
    }
    else {
      o.ti.push_back (K_DEEP);
      const size_t n_at = o.ti.size ();
      o.ti.push_back (0);
      int nch = 0;
      for (int i = 0; i < T.ncd (); i++) {
	const Cell ch = T.child_direction (nb, d ^ 1, i);
	if (!exists (ch))
	  continue;
	tape_item_gen (T, ch, cell, d ^ 1, ch, o);
	nch++;
      }
      o.ti[n_at] = nch;
    }
  }
}

// ---- the diffusion coefficients of a tree ----------------------------------------------------
// gfs_diffusion_coefficients with a constant D (src/poisson.c:1280-1303,826-853,1350-1390): diffusion_coef
// over the faces of the leaves -- f[d].v = w on the cell of a face, = w on the neighbour of the same level,
// += w/(FTT_CELLS/2) on a coarser neighbour -- then face_coeff_from_below on the non-leaf cells, children
// first: (c0 + c1 + c2 + c3)/4, and 0 on every face of a cell with exactly one non-zero face towards an interior
// neighbour.  In 2-D all of this is exactly w; in 3-D (w/4 + w/4) + w/4 and the sums of four children may
// round on the way.  Written once for two arithmetics: A::V = double (the coefficients of one w, as the reference
// computes them: the host check) or the form of the expression in w (WArithForm, below).
template <class A>
void diffusion_coefficients_gen (const Topo & T, A & ar, std::vector<typename A::V> & f)
{
  const int nd = T.nd ();
  int ncell = 0;
  for (int l = 0; l <= T.depth; l++) ncell += T.lsize (l);
  f.assign ((size_t) ncell*nd, ar.zero ());
  auto at = [&] (Cell c, int d) -> typename A::V & { return f[(size_t) T.gi (c)*nd + d]; };
  // diffusion_coef, ftt_face_traverse of the leaves: a coarse leaf sees the faces of its fine neighbours
  // from the fine side (each face once)
  for (int l = 0; l <= T.depth; l++)
    for (int q = 0; q < T.lsize (l); q++) {
      const Cell c = { l, q };
      if (T.flag[T.gi (c)] != LEAF || !T.interior (c)) continue;
      for (int d = 0; d < nd; d++) {
	const Cell nb = T.neighbor (c, d);
	if (!exists (nb)) continue;
	if (nb.l < c.l) {
	  at (c, d) = ar.leaf ();
	  at (nb, d ^ 1) = ar.addq (at (nb, d ^ 1));
	}
	else if (T.leaf (nb)) {
	  at (c, d) = ar.leaf ();
	  at (nb, d ^ 1) = ar.leaf ();
	}
	else if (!T.interior (nb))      /* a refined ghost cell: its children are not leaves of the traversal */
	  for (int i = 0; i < T.ncd (); i++) {
	    const Cell ch = T.child_direction (nb, d ^ 1, i);
	    if (!exists (ch)) continue;
	    at (ch, d ^ 1) = ar.leaf ();
	    at (c, d) = ar.addq (at (c, d));
	  }
      }
    }
  // face_coeff_from_below, the interior non-leaf cells from the deepest level up
  for (int l = T.depth; l >= 0; l--)
    for (int q = 0; q < T.lsize (l); q++) {
      const Cell c = { l, q };
      if (T.flag[T.gi (c)] != NODE || !T.interior (c)) continue;
      unsigned neighbors = 0;
      for (int d = 0; d < nd; d++) {
	typename A::V ch[4];
	int n = 0;
	for (int i = 0; i < T.ncd (); i++) {
	  const Cell cc = T.child_direction (c, d, i);
	  ch[i] = exists (cc) ? at (cc, d) : ar.zero ();
	  n += exists (cc);
	}
	at (c, d) = ar.below (ch, T.ncd (), n);
	const Cell nb = T.neighbor (c, d);
	if (ar.nonzero (at (c, d)) && exists (nb) && T.interior (nb))
	  neighbors++;
      }
      if (neighbors == 1)
	for (int d = 0; d < nd; d++) at (c, d) = ar.zero ();
    }
}

struct WArithDouble {       // the reference's arithmetic for one w
  typedef double V;
  double w, q;
  V zero () const { return 0.; }
  V leaf () const { return w; }
  V addq (V a) const { return a + q; }
  V below (const V * c, int nc, int) const
  {
    double f = 0.;
    for (int i = 0; i < nc; i++) f += c[i];
    return f/nc;
  }
  bool nonzero (V a) const { return a != 0.; }
};

// The form of a coefficient as an expression in w: EXACT (= w for every w > 0), ZERO, a sum of k quarters (k < 0
// stores -k), or anything else (OTHER).  Four equal addends summed from 0 give four times the addend exactly in
// binary floating point: 2x is exact, fl (3x) is off by at most half an ulp of 4x, and when it is off by exactly that
// (a tie, 3M = 2 mod 4 for the mantissa M of x) M is even and fl (fl (3x) + x) rounds back to 4x.  So the coarse side
// of a fine-coarse face, 0 + w/4 + w/4 + w/4 + w/4 (3-D) or 0 + w/2 + w/2 (2-D), is w, and so is
// face_coeff_from_below of children that are all w -- whatever w is, although (w + w) + w itself may round.
struct WArithForm {
  typedef int V;
  enum { ZERO = 0, EXACT = 1, OTHER = 2 };
  int ncd;                          /* FTT_CELLS/2 */
  V zero () const { return ZERO; }
  V leaf () const { return EXACT; }
  V addq (V a) const
  {
    const int k = a == ZERO ? 1 : a < 0 ? - a + 1 : 0;      /* quarters so far + 1, or 0: not a sum of quarters */
    if (k == 0) return OTHER;
    return k == ncd ? EXACT : - k;
  }
  V below (const V * c, int nc, int n) const
  {
    bool all = n == nc && (nc == 2 || nc == 4);
    for (int i = 0; i < nc; i++) all = all && c[i] == EXACT;
    if (all) return EXACT;
    for (int i = 0; i < nc; i++) if (c[i] != ZERO) return OTHER;
    return ZERO;
  }
  bool nonzero (V a) const { return a != ZERO; }
};

struct WDirect {            // the coefficients f[d].v of a cell from an array of them (the host check)
  const double * f;
  inline double operator() (const Topo & T, Cell c, int d) const { return f[(size_t) T.gi (c)*T.nd () + d]; }
};

// ---- the flow plan (tree_flow.hpp) -----------------------------------------------------------------

// the stencil of one cell read back from the streams tape_cell_gen wrote
struct FlowTerm { double a; int cnt; int idx[4]; };
struct FlowItem { double c; int g; int nt; FlowTerm t[2]; };            /* FC, or one child of a DEEP face */
struct FlowFace { int kind; int g; FlowItem fc; int nch; FlowItem ch[4]; };

bool flow_parse_interp (const int *& ti, const double *& td, const int *& tv, int dim, FlowItem & it)
{
  it.nt = *ti++;
  if (it.nt < 0 || it.nt > dim - 1) return false;
  for (int t = 0; t < it.nt; t++) {
    FlowTerm & T = it.t[t];
    T.a = *td++;
    T.cnt = *ti++;
    if (T.cnt < 0 || T.cnt > (dim == 3 ? 4 : 2)) return false;
    const int n = T.cnt == 0 ? 1 : T.cnt;
    for (int k = 0; k < n; k++) T.idx[k] = *tv++;
  }
  return true;
}

bool flow_parse_cell (const int * ti, const double * td, const int * tv, int dim, int & self, FlowFace * f)
{
  self = *tv++;
  for (int d = 0; d < 2*dim; d++) {
    FlowFace & F = f[d];
    F.kind = *ti++;
    F.nch = 0;
    if (F.kind == K_NONE) continue;
    if (F.kind == K_SAME) F.g = *tv++;
    else if (F.kind == K_FC) {
      F.fc.c = *td++;
      F.fc.g = *tv++;
      if (!flow_parse_interp (ti, td, tv, dim, F.fc)) return false;
    }
    else if (F.kind == K_DEEP) {
      F.nch = *ti++;
      if (F.nch < 0 || F.nch > (dim == 3 ? 4 : 2)) return false;
      for (int i = 0; i < F.nch; i++) {
	F.ch[i].c = *td++;
	F.ch[i].g = *tv++;
	if (!flow_parse_interp (ti, td, tv, dim, F.ch[i])) return false;
      }
    }
    else return false;
  }
  return true;
}

struct FlowBuilder {
  int dim;
  int width = FLOW_WIDTH;
  std::vector<int> wlev, wop, rlev;                 /* per cell: level and operation of its last write; last read */
  std::vector<std::vector<FlowRec>> lev;            /* lev[L - 1]: the operations of level L */
  std::vector<std::array<int, 3>> cls;              /* of which CELL | FC, CHILD | SUM, GHOST */
  bool padded = true;                               /* a level has room for every kind to start at a multiple of 64 */
  std::vector<double> ct;
  bool ok = true;

  int constant (double c)
  {
    for (size_t i = 0; i < ct.size (); i++)
      if (!memcmp (&ct[i], &c, sizeof (double))) return (int) i;
    if (ct.size () >= FLOW_NCONST) { ok = false; return 0; }
    ct.push_back (c);
    return (int) ct.size () - 1;
  }
  int slot (int L, int i) const { return ((L - 1) % FLOW_NBUF)*width + i; }   /* result i of level L */
  void need (int L) { if ((int) lev.size () < L) { lev.resize (L); cls.resize (L, std::array<int, 3> { { 0, 0, 0 } }); } }
  static int class_of (int kind) { return kind == F_CELL ? 0 : kind == F_FC || kind == F_CHILD ? 1 : 2; }
  // room on level L for a0 / a1 / a2 more operations of the three classes
  bool room (int L, int a0, int a1, int a2) const
  {
    int c0 = a0, c1 = a1, c2 = a2;
    if (L >= 1 && L <= (int) cls.size ()) { c0 += cls[L - 1][0]; c1 += cls[L - 1][1]; c2 += cls[L - 1][2]; }
    if (!padded) return c0 + c1 + c2 <= width;
    return (c0 + 63)/64*64 + (c1 + 63)/64*64 + c2 <= width;
  }
  int ready (const FlowItem & it) const           /* first level an FC / CHILD may run at */
  {
    int L = wlev[it.g];
    for (int t = 0; t < it.nt; t++)
      for (int k = 0; k < (it.t[t].cnt == 0 ? 1 : it.t[t].cnt); k++)
	L = std::max (L, wlev[it.t[t].idx[k]]);
    return L + 1;
  }
  int ref (int g, int L)                           /* the input g of an operation of level L */
  {
    rlev[g] = std::max (rlev[g], L);
    /* level 0: the values before the loop; a value at most FLOW_PD + 1 levels old is still in the LDS */
    return wlev[g] > 0 && L - wlev[g] <= FLOW_PD + 1 ? FLOW_LDS_REF (slot (wlev[g], wop[g])) : 8*g;
  }
  int emit (int L, const FlowRec & r)
  {
    need (L);
    lev[L - 1].push_back (r);
    cls[L - 1][class_of (r.w0 & 7)]++;
    return (int) lev[L - 1].size () - 1;
  }
  static FlowRec blank (int kind)
  {
    FlowRec r;
    r.w0 = kind; r.out_g = -1;
    for (int j = 0; j < FLOW_NIN; j++) r.in[j] = FLOW_NONE;
    return r;
  }
  int emit_item (int kind, const FlowItem & it, int L)
  {
    const int TS = dim == 3 ? 4 : 2;
    FlowRec r = blank (kind);
    r.w0 |= it.nt << 3;
    r.w0 |= (unsigned) constant (it.c) << 11;
    r.in[0] = ref (it.g, L);
    for (int t = 0; t < it.nt; t++) {
      r.w0 |= it.t[t].cnt << (5 + 3*t);
      r.w0 |= (unsigned) constant (it.t[t].a) << (18 + 7*t);
      for (int k = 0; k < (it.t[t].cnt == 0 ? 1 : it.t[t].cnt); k++)
	r.in[1 + TS*t + k] = ref (it.t[t].idx[k], L);
    }
    return emit (L, r);
  }
  void ghost (int g, int img, double s)
  {
    int L = std::max (wlev[img], std::max (rlev[g], wlev[g])) + 1;
    for (int tries = 0; !room (L, 0, 0, 1); L++) if (++tries > 1000000) { ok = false; return; }
    FlowRec r = blank (F_GHOST);
    r.w0 |= (unsigned) constant (s) << 11;
    r.out_g = 8*g;
    r.in[0] = ref (img, L);
    const int i = emit (L, r);
    wlev[g] = L; wop[g] = i; rlev[g] = 0;
  }
  void cell (int g, int self, const FlowFace * f, int cell_level, bool reads_self)
  {
    int L = std::max (rlev[g], wlev[g]) + 1;
    int nfc = 0, nsum = 0, n2 = 0;      /* FC and SUM one level before the cell's, CHILD two levels before */
    if (reads_self) L = std::max (L, wlev[self] + 1);
    for (int d = 0; d < 2*dim; d++) {
      const FlowFace & F = f[d];
      if (F.kind == K_SAME) L = std::max (L, wlev[F.g] + 1);
      else if (F.kind == K_FC) { L = std::max (L, ready (F.fc) + 1); nfc++; }
      else if (F.kind == K_DEEP) {
	for (int i = 0; i < F.nch; i++) { L = std::max (L, ready (F.ch[i]) + 2); n2++; }
	nsum++;
      }
    }
    if (n2) L = std::max (L, 3); else if (nfc + nsum) L = std::max (L, 2);
    for (int tries = 0; !room (L, 1, 0, 0) || ((nfc || nsum) && !room (L - 1, 0, nfc, nsum)) || (n2 && !room (L - 2, 0, n2, 0)); L++)
      if (++tries > 1000000) { ok = false; return; }
    FlowRec r = blank (F_CELL);
    r.w0 |= (unsigned) cell_level << 15;
    r.out_g = 8*g;
    if (reads_self) { r.w0 |= 1u << 20; r.in[0] = ref (self, L); }
    for (int d = 0; d < 2*dim; d++) {
      const FlowFace & F = f[d];
      if (F.kind == K_SAME) {
	r.w0 |= FK_SAME << (3 + 2*d);
	r.in[1 + d] = ref (F.g, L);
      }
      else if (F.kind == K_FC) {
	r.w0 |= FK_PAIR << (3 + 2*d);
	r.in[1 + d] = FLOW_LDS_REF (slot (L - 1, emit_item (F_FC, F.fc, L - 1)));
      }
      else if (F.kind == K_DEEP) {
	FlowRec s = blank (F_SUM);
	s.w0 |= F.nch << 3;
	for (int i = 0; i < F.nch; i++)
	  s.in[i] = FLOW_LDS_REF (slot (L - 2, emit_item (F_CHILD, F.ch[i], L - 2)));
	r.w0 |= FK_PAIR << (3 + 2*d);
	r.in[1 + d] = FLOW_LDS_REF (slot (L - 1, emit (L - 1, s)));
      }
    }
    const int i = emit (L, r);
    wlev[g] = L; wop[g] = i; rlev[g] = 0;
  }
};

// the loop of nrelax sweeps of the sweep S (its cells in the order S.g, a valid sequential order) with
// the copies of the ghosts between the sweeps, as a flow plan; none when the loop does not fit
// the format (the caller keeps the tape kernels)
std::optional<FlowProgram> plan_flow (int ncell, int dim, const SweepPlan & S, unsigned nrelax, const Sgn6 & sg,
				      const int * cell_level_of, bool reads_self, bool debug, int width)
{
  FlowBuilder B;
  B.dim = dim;
  B.width = width;
  B.padded = width >= 256;      /* narrower plans (lab) pack the kinds: three kinds at multiples of 64 need the room */
  B.wlev.assign (ncell, 0); B.wop.assign (ncell, 0); B.rlev.assign (ncell, 0);
  const size_t nc = S.g.size ();
  std::vector<FlowFace> faces (nc*6);
  std::vector<int> selfs (nc);
  for (size_t c = 0; c < nc; c++)
    if (!flow_parse_cell (S.ti.data () + S.cell_off[3*c], S.td.data () + S.cell_off[3*c + 1],
			  S.tv.data () + S.cell_off[3*c + 2], dim, selfs[c], &faces[6*c]))
      return std::nullopt;
  for (unsigned sw = 0; sw < nrelax && B.ok; sw++) {
    for (const Ghost & G : S.ghosts) B.ghost (G.g, G.img, sg.s[G.side]);
    for (size_t c = 0; c < nc && B.ok; c++)
      B.cell (S.g[c], selfs[c], &faces[6*c], cell_level_of[S.g[c]], reads_self);
  }
  if (!B.ok || (int) B.lev.size () > FLOW_MAXLEV) return std::nullopt;
  int nmixed = 0;      /* levels where CELL and FC / CHILD (or CELL and the short kinds) share a wavefront */
  {
    // the operations of a level sorted by kind (stable); the inputs that name an operation of the level by its
    // place follow.  An input of level L in buffer b was produced by the level L' in [L - FLOW_PD - 1, L - 1]
    // with (L' - 1) % FLOW_NBUF == b (FLOW_NBUF = FLOW_PD + 2: one such level).
    static const int order_of[8] = { 0, 1, 1, 2, 3, 4, 4, 4 };       /* CELL, FC / CHILD, SUM, GHOST */
    const int nl = (int) B.lev.size ();
    std::vector<std::vector<int>> place (nl);      /* place[L - 1][old] = new */
    for (int L = 1; L <= nl; L++) {
      std::vector<FlowRec> & ops = B.lev[L - 1];
      std::vector<int> idx (ops.size ());
      for (size_t i = 0; i < idx.size (); i++) idx[i] = (int) i;
      std::stable_sort (idx.begin (), idx.end (), [&] (int a, int b) {
	  return order_of[ops[a].w0 & 7] < order_of[ops[b].w0 & 7]; });
      // where the level has room, a kind starts at a multiple of 64: a wavefront with two kinds runs the
      // branchy arithmetic, twice the time of the others, and the level waits for it.  CELL | FC, CHILD |
      // SUM, GHOST (the last two are short and share)
      int count[3] = { 0, 0, 0 };
      for (const FlowRec & r : ops) count[std::min (order_of[r.w0 & 7], 2)]++;
      int base[3] = { 0, count[0], count[0] + count[1] };
      {
	const int b1 = (count[0] + 63)/64*64, b2a = (b1 + count[1] + 63)/64*64, b2b = (count[0] + count[1] + 63)/64*64;
	if (count[1] + count[2] > 0 && b1 + count[1] + count[2] <= width) {
	  base[1] = b1;
	  base[2] = count[2] > 0 && b2a + count[2] <= width ? b2a : b1 + count[1];
	}
	else if (count[2] > 0 && b2b + count[2] <= width)
	  base[2] = b2b;
      }
      const int total = std::max (base[2] + count[2], std::max (base[1] + count[1], count[0]));
      if ((count[1] > 0 && base[1] % 64) || (count[2] > 0 && count[0] + count[1] > 0 && base[2] % 64 && count[1] == 0)) nmixed++;
      place[L - 1].resize (ops.size ());
      std::vector<FlowRec> sorted (total, FlowBuilder::blank (F_NOP));
      int rank[3] = { 0, 0, 0 };
      for (size_t i = 0; i < idx.size (); i++) {
	const int k = std::min (order_of[ops[idx[i]].w0 & 7], 2);
	const int at = base[k] + rank[k]++;
	sorted[at] = ops[idx[i]];
	place[L - 1][idx[i]] = at;
      }
      ops.swap (sorted);
    }
    for (int L = 1; L <= nl; L++)
      for (FlowRec & r : B.lev[L - 1])
	for (int j = 0; j < FLOW_NIN; j++)
	  if (FLOW_IS_LDS (r.in[j]) && r.in[j] != FLOW_NONE) {
	    const int sl = FLOW_LDS_ADDR (r.in[j]) >> 4, b = sl/width, i = sl % width;
	    int Lp = -1;
	    for (int q = L - 1; q >= std::max (1, L - FLOW_PD - 1); q--)
	      if ((q - 1) % FLOW_NBUF == b) Lp = q;
	    if (Lp < 0 || i >= (int) place[Lp - 1].size ()) return std::nullopt;
	    r.in[j] = FLOW_LDS_REF (b*width + place[Lp - 1][i]);
	  }
  }
  FlowProgram F;
  F.width = width;
  if (debug) fprintf (stderr, "gfship_tree: flow plan: %d of %zu levels have a wavefront with two kinds\n", nmixed, B.lev.size ());
  {
    // places in the order of the plan
    std::vector<int> pos (ncell, -1);
    std::vector<int> & gidx = F.gidx;
    auto place_of = [&] (int g) { if (pos[g] < 0) { pos[g] = (int) gidx.size (); gidx.push_back (g); } return pos[g]; };
    for (auto & l : B.lev) for (FlowRec & r : l) if (r.out_g >= 0) place_of (r.out_g/8);
    for (auto & l : B.lev) for (FlowRec & r : l)
      for (int j = 0; j < FLOW_NIN; j++) if (!FLOW_IS_LDS (r.in[j])) place_of (r.in[j]/8);
    for (auto & l : B.lev) for (FlowRec & r : l) {
      if (r.out_g >= 0) r.out_g = 8*pos[r.out_g/8];
      for (int j = 0; j < FLOW_NIN; j++) if (!FLOW_IS_LDS (r.in[j])) r.in[j] = 8*pos[r.in[j]/8];
    }
    if (gidx.empty ()) gidx.push_back (0);
    F.npos = (int) gidx.size ();
    while (gidx.size () < FLOW_WIDTH + 64) gidx.push_back (gidx[0]);      /* spare places the idle lanes load (not unpacked) */
  }
  F.nlev = (int) B.lev.size ();
  F.lev_off.assign (1, 0);
  for (const auto & l : B.lev) {
    F.rec.insert (F.rec.end (), l.begin (), l.end ());
    F.lev_off.push_back ((int) F.rec.size ());
  }
  F.nops = (int) F.rec.size ();
  for (int k = 0; k < FLOW_PD + 2; k++) {        /* the records the kernel loads ahead of the last level */
    F.rec.push_back (FlowBuilder::blank (F_NOP));
    F.lev_off.push_back ((int) F.rec.size ());
  }
  for (int k = 0; k < FLOW_WIDTH; k++) F.rec.push_back (FlowBuilder::blank (F_NOP));      /* what the idle lanes read */
  F.nct = (int) B.ct.size ();
  F.ct = std::move (B.ct);
  if (F.ct.empty ()) F.ct.push_back (0.);
  return F;
}

// the kernel's program on the host, with its timing: the global inputs of level L are read BEFORE the
// stores of level L - 1 (they are loaded a level ahead), the operations of a level run backwards, the
// stores of a level land after its loads.  Returns the number of hazards: a store of level L - 1 or L
// onto a cell that level L reads from global memory (which the schedule must exclude).
long long flow_emulate (const FlowProgram & F, int dim, std::vector<double> & u, const std::vector<double> & rhs,
			double omega, int op, double w)
{
  long long hazards = 0;
  std::vector<double> up (F.npos), rp (F.npos);
  for (int p = 0; p < F.npos; p++) { up[p] = u[F.gidx[p]]; rp[p] = rhs[F.gidx[p]]; }
  std::vector<FlowPair> lo (FLOW_LDS_SLOTS, FlowPair { 0., 0. });
  std::vector<std::vector<double>> pre (FLOW_NBUF, std::vector<double> ((size_t) FLOW_WIDTH*(FLOW_NIN + 1)));
  std::vector<int> stored_at (F.npos, -10);
  auto prefetch = [&] (int L, std::vector<double> & v) {      /* what flow_prefetch loads for level L (0-based) */
    if (L >= F.nlev) return;
    for (int i = F.lev_off[L]; i < F.lev_off[L + 1]; i++) {
      const FlowRec & r = F.rec[i];
      double * vi = &v[(size_t) (i - F.lev_off[L])*(FLOW_NIN + 1)];
      for (int j = 0; j < FLOW_NIN; j++)
	vi[j] = up[std::max (r.in[j], 0)/8];
      vi[FLOW_NIN] = rp[std::max (r.out_g, 0)/8];
    }
  };
  for (int L = 0; L < FLOW_PD; L++) prefetch (L, pre[L % FLOW_NBUF]);
  std::vector<std::pair<int, double>> late;      /* the stores of the level before: issued during this one */
  for (int L = 0; L < F.nlev; L++) {
    prefetch (L + FLOW_PD, pre[(L + FLOW_PD) % FLOW_NBUF]);
    for (auto & st : late) {
      if (stored_at[st.first] == L - 1) hazards++;      /* two stores of one level onto one cell */
      up[st.first] = st.second;
      stored_at[st.first] = L - 1;
    }
    late.clear ();
    std::vector<std::pair<int, double>> stores;
    std::vector<FlowPair> cur (FLOW_WIDTH, FlowPair { 0., 0. });
    for (int i = F.lev_off[L + 1]; i-- > F.lev_off[L]; ) {
      const FlowRec & r = F.rec[i];
      const double * vi = &pre[L % FLOW_NBUF][(size_t) (i - F.lev_off[L])*(FLOW_NIN + 1)];
      double x[FLOW_NIN], y[FLOW_NIN];
      for (int j = 0; j < FLOW_NIN; j++) {
	const int sl = FLOW_LDS_ADDR (r.in[j]) >> 4;
	if (FLOW_IS_LDS (r.in[j]) && r.in[j] != FLOW_NONE && sl/F.width == L % FLOW_NBUF)
	  hazards++;       /* an input in the buffer this level writes */
	const FlowPair p = lo[sl];
	x[j] = FLOW_IS_LDS (r.in[j]) ? p.x : vi[j];
	y[j] = p.y;
      }
      // the wavefront of this operation: the 64 operations around it (flow_eval_wave)
      const int w0i = F.lev_off[L] + (i - F.lev_off[L])/64*64, w1i = std::min (w0i + 64, F.lev_off[L + 1]);
      int first = F_NOP;      /* the kind of the first operation that is not a NOP, as flow_eval_wave takes it */
      for (int q = w0i; q < w1i && first == F_NOP; q++) first = flow_class (F.rec[q].w0 & 7);
      bool uniform = true, any3 = false;
      for (int q = w0i; q < w1i; q++) {
	const unsigned qw = F.rec[q].w0;
	if (flow_class (qw & 7) != first && flow_class (qw & 7) != F_NOP) uniform = false;
	if (flow_class (qw & 7) == F_FC)
	  for (int t = 0; t < dim - 1; t++)
	    if (t < (int) ((qw >> 3) & 3) && ((qw >> (5 + 3*t)) & 7) == 3) any3 = true;
      }
      struct AnyHost { bool v; bool operator() (bool) const { return v; } } any = { any3 };
      FlowPair o = { 0., 0. };
#define FLOW_EMU(D)							\
      o = !uniform ? flow_eval<D> (r.w0, x, y, vi[FLOW_NIN], F.ct.data (), omega, op, w) : \
	first == F_CELL ? flow_eval_uniform<D, F_CELL> (r.w0, x, y, vi[FLOW_NIN], F.ct.data (), omega, op, w, any) : \
	first == F_FC ? flow_eval_uniform<D, F_FC> (r.w0, x, y, vi[FLOW_NIN], F.ct.data (), omega, op, w, any) : \
	first == F_SUM ? flow_eval_uniform<D, F_SUM> (r.w0, x, y, vi[FLOW_NIN], F.ct.data (), omega, op, w, any) : \
	flow_eval_uniform<D, F_GHOST> (r.w0, x, y, vi[FLOW_NIN], F.ct.data (), omega, op, w, any)
      if ((r.w0 & 7) != F_NOP) { if (dim == 3) { FLOW_EMU (3); } else { FLOW_EMU (2); } }
#undef FLOW_EMU
      cur[i - F.lev_off[L]] = o;
      if (r.out_g >= 0) stores.push_back ({ r.out_g/8, o.x });
      for (int j = 0; j < FLOW_NIN; j++)
	if (!FLOW_IS_LDS (r.in[j]) && stored_at[r.in[j]/8] >= L - FLOW_PD - 1)
	  hazards++;         /* the load was issued in level L - FLOW_PD, beside the stores of L - FLOW_PD - 1 */
    }
    late = stores;
    for (int i = 0; i < F.width; i++) lo[(size_t) (L % FLOW_NBUF)*F.width + i] = cur[i];
  }
  for (auto & st : late) up[st.first] = st.second;
  for (int p = 0; p < F.npos; p++) u[F.gidx[p]] = up[p];
  return hazards;
}

} // namespace

// ---- the plans -------------------------------------------------------------------------------------

static int plan_tree (int dim, gfship_refine_fn refine, void * ctx, const int * side, TreePlan & P)
{
  GFSHIP_CHECK (dim == 2 || dim == 3, GFSHIP_EINVAL, "gfship_tree_create: dim = %d", dim);
  // gfs_refine_refine + gfs_simulation_refine, src/refine.c:45-60, src/simulation.c:1203-1233
  Builder B;
  B.dim = dim;
  B.ensure (0);
  B.flag[0][B.idx (0, 1, 1, 1)] = LEAF;
  int e = B.refine_rec (0, 1, 1, 1, refine, ctx);
  GFSHIP_CHECK (!B.too_large, GFSHIP_EUNSUPPORTED,
		"gfship_tree_create: more than 2^27 cells in the dense levels of the tree");
  GFSHIP_CHECK (e == 0, e, "gfship_tree_create: more than %d levels", GFSHIP_MAXLEVEL);
  for (int d = 0; d < 2*dim; d++) {
    P.side[d] = side ? side[d] : GFSHIP_SIDE_PERIODIC;
    GFSHIP_CHECK (P.side[d] == GFSHIP_SIDE_PERIODIC || P.side[d] == GFSHIP_SIDE_BOUNDARY, GFSHIP_EINVAL,
		  "gfship_tree_create: side %d: periodic or boundary", d);
    if (P.side[d] == GFSHIP_SIDE_BOUNDARY) P.has_boundary = true;
  }
  Topo & H = P.H;      /* (Builder::ensure has kept the cells of the dense levels below 2^27) */
  H.dim = dim;
  H.depth = (int) B.flag.size () - 1;
  int off = 0;
  for (int l = 0; l <= H.depth; l++) {
    H.off[l] = off;
    off += H.lsize (l);
  }
  H.off[H.depth + 1] = off;
  P.ncell = off;
  P.hflag.assign (off, NONE);
  auto flatten = [&] () {
    for (int l = 0; l <= H.depth; l++)
      std::copy (B.flag[l].begin (), B.flag[l].end (), P.hflag.begin () + H.off[l]);
  };
  flatten ();
  H.flag = P.hflag.data ();
  for (int l = H.depth - 2; l >= 0; l--) {
    // the refinements of a level are applied while the level is traversed (simulation.c:1105-1109)
    traverse (H, root_cell (H), T_LEVEL, l, [&] (Cell c) {
	if (H.leaf (c) && refine_corner (H, c)) {
	  (void) B.refine_single (c.l, H.ci (c), H.cj (c), H.ck (c));
	  flatten ();
	}
      });
  }
  // gfs_domain_match: the ghost trees of the periodic sides mirror the cells they face; both cells
  // of a periodic pair must be at the same refinement
  for (int l = 0; l <= H.depth; l++) {
    unsigned char * f = P.hflag.data () + H.off[l];
    bool differs = false;
    ghost_positions (dim, l, [&] (int sd, int G, int I, int O) {
	if (P.side[sd] != GFSHIP_SIDE_PERIODIC)      /* the ghost tree of a GfsBoundary matches its side */
	  f[G] = f[O];
	else if (f[O] != f[I])
	  differs = true;
	else
	  f[G] = f[I];
      });
    GFSHIP_CHECK (!differs, GFSHIP_EUNSUPPORTED,
		  "gfship_tree_create: the refinement differs across a periodic side (level %d)", l);
  }
  {
    // the tables of Topo (tree.hpp), from the computed answers
    const int nd = H.nd ();
    P.h_nbtab.assign ((size_t) P.ncell*nd, -1);
    P.h_child0.assign (P.ncell, 0);
    P.h_cmask.assign (P.ncell, 0);
    P.h_idtab.assign (P.ncell, 0);
    for (int l = 0; l <= H.depth; l++)
      for (int q = 0; q < H.lsize (l); q++) {
	const int g = H.off[l] + q;
	if (P.hflag[g] == NONE)
	  continue;
	const Cell c = { l, q };
	for (int d = 0; d < nd; d++) {
	  const Cell nb = H.neighbor (c, d);
	  P.h_nbtab[(size_t) g*nd + d] = !exists (nb) ? -1 : nb.l == l ? nb.q : - nb.q - 2;
	}
	P.h_idtab[g] = (unsigned char) (H.id (c) | (H.interior (c) ? 8 : 0));
	if (l < H.depth) {
	  const int rr = H.r (l + 1);
	  P.h_child0[g] = 2*H.ci (c) - 1 + rr*(2*H.cj (c) + (dim == 3 ? rr*2*H.ck (c) : 0));
	  for (int k = 0; k < H.nc (); k++)
	    if (exists (H.child (c, k)))
	      P.h_cmask[g] |= (unsigned char) (1 << k);
	}
      }
    H.nbtab = P.h_nbtab.data ();
    H.child0 = P.h_child0.data ();
    H.cmask = P.h_cmask.data ();
    H.idtab = P.h_idtab.data ();
  }
  traverse (H, root_cell (H), T_LEAFS, -1, [&] (Cell c) { P.hleaves.push_back (c); });
  P.hnonleaf.resize (H.depth);
  for (int l = 0; l < H.depth; l++)
    traverse (H, root_cell (H), T_LEVEL_NON_LEAFS, l, [&] (Cell c) { P.hnonleaf[l].push_back (c); });
  ghost_list (H, P.side, T_LEAFS, -1, P.hghost_leaves);
  return GFSHIP_OK;
}

// dependency levels of an exact-order sweep over `order': a cell runs after every earlier cell
// it reads (it must see the new value) and after every earlier cell that reads it (which must
// still see the old one)
static int plan_sweep (const TreePlan & P, int m, bool debug, SweepPlan & S)
{
  const Topo & T = P.H;
  std::vector<Cell> order;
  traverse (T, root_cell (T), T_LEVEL_LEAFS, m, [&] (Cell c) { order.push_back (c); });
  std::vector<int> pos (P.ncell, -1);
  for (size_t k = 0; k < order.size (); k++)
    pos[T.gi (order[k])] = (int) k;
  std::vector<int> lev (order.size (), 0), minlev (order.size (), 0), reads;
  Recorder R = { &reads };
  int nlev = 0;
  for (size_t k = 0; k < order.size (); k++) {
    reads.clear ();
    relax_cell (T, order[k], R, 0., 1., m);
    int L = minlev[k];
    for (int g : reads) {
      const int p = pos[g];
      if (p >= 0 && p < (int) k)
	L = std::max (L, lev[p] + 1);
    }
    lev[k] = L;
    for (int g : reads) {
      const int p = pos[g];
      if (p > (int) k)
	minlev[p] = std::max (minlev[p], L + 1);
    }
    nlev = std::max (nlev, L + 1);
  }
  ghost_list (T, P.side, T_LEVEL_LEAFS, m, S.ghosts);
  if (debug) {
    // what pipelining the nrelax sweeps of a loop would give
    const int nrelax = 4;
    LevelScheduler sched (P.ncell);
    std::vector<std::vector<int>> rd (order.size ());
    for (size_t k = 0; k < order.size (); k++) {
      reads.clear ();
      relax_cell (T, order[k], R, 0., 1., m);
      rd[k] = reads;
    }
    for (int sw = 0; sw < nrelax; sw++) {
      for (const Ghost & G : S.ghosts) sched.ghost (G);
      for (size_t k = 0; k < order.size (); k++)
	sched.cell (T.gi (order[k]), rd[k].data (), rd[k].data () + rd[k].size ());
    }
    fprintf (stderr, "gfship_tree: sweep of level %d: %zu cells, %d dependency levels per sweep, %d x %d = %d sequential, %d pipelined\n",
	     m, order.size (), nlev, nrelax, nlev, nrelax*nlev, sched.nlev);
  }
  S.nlev = nlev;
  S.lev_off.assign (nlev + 1, 0);
  for (size_t k = 0; k < order.size (); k++)
    S.lev_off[lev[k] + 1]++;
  for (int L = 0; L < nlev; L++)
    S.lev_off[L + 1] += S.lev_off[L];
  S.cells.resize (order.size ());
  std::vector<int> cur (S.lev_off.begin (), S.lev_off.end () - 1);
  for (size_t k = 0; k < order.size (); k++)
    S.cells[cur[lev[k]]++] = order[k];
  // the compiled stencils
  TapeOut o;
  for (size_t c = 0; c < S.cells.size (); c++) {
    S.cell_off.push_back ((int) o.ti.size ()); S.cell_off.push_back ((int) o.td.size ()); S.cell_off.push_back ((int) o.tv.size ());
    tape_cell_gen (T, S.cells[c], m, o);
  }
  S.cell_off.push_back ((int) o.ti.size ()); S.cell_off.push_back ((int) o.td.size ()); S.cell_off.push_back ((int) o.tv.size ());
  S.ti = std::move (o.ti); S.td = std::move (o.td); S.tv = std::move (o.tv);
  if (!lds_chunks (S.cell_off, S.lev_off, S.chunk)) return GFSHIP_EUNSUPPORTED;
  S.chunk.push_back ((int) S.cells.size ());
  S.g.resize (S.cells.size ());
  for (size_t c = 0; c < S.cells.size (); c++) S.g[c] = T.gi (S.cells[c]);
  return 0;
}

// The relax loop of level m as one program: [copies of the ghosts][sweep 0 in tree order][copies]
// [sweep 1] ... [sweep nrelax - 1] in the levels of LevelScheduler: the results are those of the sequential
// program, and sweep s + 1 follows sweep s a few levels behind instead of waiting for its end
int plan_loop (const TreePlan & T, const SweepPlan & S, int m, unsigned nrelax, const Sgn6 & sg, int flow_width,
	       bool debug, LoopPlan & P)
{
  P = LoopPlan ();
  const size_t nc = S.g.size ();
  // the cells were sorted by single-sweep dependency level; the sequential order inside a sweep is
  // the tree order: recover it from the positions the sweep plan kept (sorted is stable per level,
  // and any order consistent with the single-sweep levels is a valid sequential order)
  struct Node { int kind, idx, sweep, level; };   /* kind 0: cell idx of the sweep, 1: ghost idx */
  std::vector<Node> nodes;
  nodes.reserve (nrelax*(nc + S.ghosts.size ()));
  LevelScheduler sched (T.ncell);
  for (unsigned sw = 0; sw < nrelax; sw++) {
    for (size_t q = 0; q < S.ghosts.size (); q++)
      nodes.push_back ({ 1, (int) q, (int) sw, sched.ghost (S.ghosts[q]) });
    for (size_t c = 0; c < nc; c++)
      nodes.push_back ({ 0, (int) c, (int) sw,
	    sched.cell (S.g[c], S.tv.data () + S.cell_off[3*c + 2], S.tv.data () + S.cell_off[3*(c + 1) + 2]) });
  }
  std::stable_sort (nodes.begin (), nodes.end (), [] (const Node & a, const Node & b) { return a.level < b.level; });
  std::vector<int> & ti = P.ti, & tv = P.tv, & node_off = P.node_off, & node_g = P.node_g, bounds;
  std::vector<double> & td = P.td;
  for (const Node & N : nodes) {
    if (P.node_level.empty () || N.level != P.node_level.back ()) bounds.push_back ((int) P.node_level.size ());
    P.node_level.push_back (N.level);
    node_off.push_back ((int) ti.size ()); node_off.push_back ((int) td.size ()); node_off.push_back ((int) tv.size ());
    if (N.kind == 1) {
      const Ghost & G = S.ghosts[N.idx];
      ti.push_back (K_GHOST);
      td.push_back (sg.s[G.side]);
      tv.push_back (G.img);
      node_g.push_back (G.g);
    }
    else {
      const int c = N.idx;
      ti.insert (ti.end (), S.ti.begin () + S.cell_off[3*c], S.ti.begin () + S.cell_off[3*(c + 1)]);
      td.insert (td.end (), S.td.begin () + S.cell_off[3*c + 1], S.td.begin () + S.cell_off[3*(c + 1) + 1]);
      tv.insert (tv.end (), S.tv.begin () + S.cell_off[3*c + 2], S.tv.begin () + S.cell_off[3*(c + 1) + 2]);
      node_g.push_back (S.g[c]);
    }
  }
  bounds.push_back ((int) nodes.size ());
  node_off.push_back ((int) ti.size ()); node_off.push_back ((int) td.size ()); node_off.push_back ((int) tv.size ());
  if (!lds_chunks (node_off, bounds, P.chunk)) return GFSHIP_EUNSUPPORTED;
  for (int d = 0; d < 6; d++) P.sg[d] = sg.s[d];
  P.chunk.push_back ((int) nodes.size ());
  P.nlev = sched.nlev;
  for (int k = 0; k < P.nchunks (); k++) {
    const int c0 = P.chunk[k], c1 = P.chunk[k + 1];
    const int v[8] = { c0, c1, node_off[3*c0], node_off[3*c1], node_off[3*c0 + 1], node_off[3*c1 + 1],
		       node_off[3*c0 + 2], node_off[3*c1 + 2] };
    P.desc.insert (P.desc.end (), v, v + 8);
  }
  for (int q = 0; q < 8; q++) P.desc.push_back (0);          /* the descriptor read past the last chunk */
  for (size_t c = 0; c < nodes.size (); c++) {
    P.rec.push_back (node_off[3*c]); P.rec.push_back (node_off[3*c + 1]); P.rec.push_back (node_off[3*c + 2]);
    P.rec.push_back (node_g[c]);
  }
  for (int q = 0; q < 4; q++) P.rec.push_back (0);
  P.nrelax = nrelax;
  {
    // the same loop as a flow plan (tree_flow.hpp)
    std::vector<int> level_of (T.ncell, 0);
    for (int l = 0; l <= T.H.depth; l++)
      for (int g = T.H.off[l]; g < T.H.off[l + 1]; g++) level_of[g] = l;
    const int fw = std::min (FLOW_WIDTH, flow_width);      /* lab: operations per level (a multiple of 64 up to 512) */
    /* a level costs about the same whatever its width: the widest plan wins on octrees; the levels of a quadtree
       are narrow, 256 operations per level are as few levels and fewer idle wavefronts (measured: 11.5 against
       12.5 ms per step on the quadtree bench) */
    const int width = fw ? fw : T.H.dim == 2 ? 256 : FLOW_WIDTH;
    P.flow = plan_flow (T.ncell, T.H.dim, S, nrelax, sg, level_of.data (), T.H.dim == 2, debug, width);
  }
  if (debug)
    fprintf (stderr, "gfship_tree: relax loop of level %d: %u sweeps, %d nodes in %d levels, %d chunks; flow plan: %d operations in %d levels, %d constants\n",
	     m, nrelax, P.nnodes (), P.nlev, P.nchunks (), P.flow ? P.flow->nops : -1, P.flow ? P.flow->nlev : -1,
	     P.flow ? P.flow->nct : -1);
  return 0;
}

static FacePlan plan_faces (const TreePlan & P, int kind)
{
  const Topo & T = P.H;
  FacePlan F;
  face_list (T, P.hleaves, kind, F.faces);
  std::vector<int> leafpos (P.ncell, -1);
  for (size_t k = 0; k < P.hleaves.size (); k++)
    leafpos[T.gi (P.hleaves[k])] = (int) k;
  std::vector<std::vector<int>> inc (P.hleaves.size ());
  for (size_t k = 0; k < F.faces.size (); k++) {
    const int a = leafpos[T.gi (F.faces[k].cell)], b = leafpos[T.gi (F.faces[k].neighbor)];
    if (a >= 0) inc[a].push_back ((int) (k << 1));
    if (b >= 0) inc[b].push_back ((int) (k << 1 | 1));
  }
  F.inc_off.assign (inc.size () + 1, 0);
  for (size_t k = 0; k < inc.size (); k++) {
    F.inc_off[k + 1] = F.inc_off[k] + (int) inc[k].size ();
    F.inc.insert (F.inc.end (), inc[k].begin (), inc[k].end ());
  }
  return F;
}

bool diffusion_weights_exact (const Topo & T)
{
  WArithForm ar = { T.ncd () };
  std::vector<int> form;
  diffusion_coefficients_gen (T, ar, form);
  struct ZeroReader { double operator() (const Topo &, Cell) const { return 0.; } };
  struct WRecord {          // which f[d].v does the stencil read?
    std::vector<size_t> * out;
    double operator() (const Topo & T, Cell c, int d) const { out->push_back ((size_t) T.gi (c)*T.nd () + d); return 1.; }
  };
  std::vector<size_t> read;
  ZeroReader zr;
  WRecord wr = { &read };
  for (int l = 0; l <= T.depth; l++)
    for (int q = 0; q < T.lsize (l); q++) {
      const Cell c = { l, q };
      if (T.flag[T.gi (c)] == NONE || !T.interior (c)) continue;
      read.clear ();
      (void) diffusion_relax_cell (T, c, zr, 0., wr, l);           /* a cell of the sweep of its own level */
      if (T.leaf (c))
	(void) diffusion_residual_cell (T, c, zr, 0., wr);         /* a leaf on the finer levels, residual, rhs */
      for (size_t k : read)
	if (form[k] != WArithForm::EXACT) return false;
    }
  return true;
}

// the contacts of the leaves for gfs_domain_tag_droplets.  From a leaf, ftt_cell_neighbors (src/ftt.h:432-480) gives
// in each direction the cell of its level or the coarser leaf: a leaf of its level is a contact without a gate; a
// coarser leaf k is a contact whose gate is the parent N of the leaf, the cell of the level of k that k sees there
// (tag_cell_fraction, src/domain.c:3577, tests c on N before it looks at the children of N, :3587-3593); a cell of
// its level with children is the same contact seen from its coarse end, taken from the fine one
int plan_droplets (const TreePlan & P, DropletPlan & out)
{
  const Topo & T = P.H;
  const size_t nl = P.hleaves.size ();
  GFSHIP_CHECK (P.ncell < (1 << 30), GFSHIP_EUNSUPPORTED, "gfs_domain_tag_droplets: the tree has 2^30 cells or more");
  std::vector<int> leafpos (P.ncell, -1);
  for (size_t k = 0; k < nl; k++)
    leafpos[T.gi (P.hleaves[k])] = (int) k;
  out = DropletPlan ();
  out.cells.assign (P.ncell, 0xFFFFFFFFu);
  for (int l = 0; l <= T.depth; l++)
    for (int q = 0; q < T.lsize (l); q++) {
      const Cell c = { l, q };
      if (T.flag[T.gi (c)] != NONE && T.interior (c)) out.cells[T.gi (c)] = (unsigned) T.gi (c);
    }
  out.on_side.assign (nl, 0);
  std::vector<std::vector<DropContact>> con (nl);
  for (size_t p = 0; p < nl; p++) {
    const Cell c = P.hleaves[p];
    for (int d = 0; d < T.nd (); d++) {
      if (touches_side (T, c, d)) {
	out.on_side[p] = 1;
	if (P.side[d] != GFSHIP_SIDE_PERIODIC) continue;
	/* match_periodic_bc, :3689-3698: the leaf across the box; gfship_tree_create has made the refinement of the
	   two sides equal, so that it is a leaf of this level */
	const int n = T.n (c.l), a = d >> 1;
	int x[3] = { T.ci (c), T.cj (c), T.ck (c) };
	x[a] = x[a] == n ? 1 : n;
	const Cell o = T.make (c.l, x[0], x[1], x[2]);
	GFSHIP_CHECK (exists (o) && leafpos[T.gi (o)] >= 0, GFSHIP_EUNSUPPORTED,
		      "gfs_domain_tag_droplets: the refinement differs across a periodic side");
	const unsigned q = (unsigned) leafpos[T.gi (o)];
	if (q < p) {
	  out.periodic.push_back ((unsigned) p);
	  out.periodic.push_back (q);
	}
	continue;
      }
      const Cell nb = T.neighbor (c, d);
      if (!exists (nb) || !T.interior (nb) || !T.leaf (nb)) continue;
      const unsigned q = (unsigned) leafpos[T.gi (nb)];
      if (nb.l == c.l) {
	if (q < p) con[p].push_back (DropContact { q, -1 });
	continue;
      }
      /* nb is a coarser leaf: the gate is the parent of c */
      const Cell N = T.make (c.l - 1, (T.ci (c) + 1)/2, (T.cj (c) + 1)/2, T.dim == 3 ? (T.ck (c) + 1)/2 : 0);
      GFSHIP_CHECK (exists (N) && nb.l == c.l - 1, GFSHIP_EUNSUPPORTED, "gfs_domain_tag_droplets: the tree is not graded");
      if (q < p) con[p].push_back (DropContact { q, T.gi (N) << 1 | 1 });
      else con[q].push_back (DropContact { (unsigned) p, T.gi (N) << 1 });
      out.ngated++;
    }
  }
  out.con_off.assign (nl + 1, 0);
  for (size_t p = 0; p < nl; p++) {
    out.con_off[p + 1] = out.con_off[p] + (int) con[p].size ();
    out.con.insert (out.con.end (), con[p].begin (), con[p].end ());
  }
  return GFSHIP_OK;
}

// DESIGN.md 11.41 on the host, a test aid (gfship_tree_host_tag_droplets): the steps of tree_droplets.hip in their
// order, which must stay in step with that file -- the components of the contacts that are symmetric
// (tdrop_block_kernel, tdrop_cross_kernel), the one-way contacts until nothing changes and parent[root] = L[root]
// (tdrop_oneway_kernel), then the periodic pairs (tdrop_periodic_kernel), the ranks
unsigned droplet_tags_host (const TreePlan & P, const DropletPlan & D, const double * c, std::vector<unsigned> & tag)
{
  const Topo & T = P.H;
  const unsigned nl = (unsigned) P.hleaves.size (), none = 0xFFFFFFFFu;
  std::vector<unsigned> parent (nl), L (nl);
  for (unsigned p = 0; p < nl; p++)
    parent[p] = L[p] = c[T.gi (P.hleaves[p])] > 1e-4 ? p : none;
  auto find = [&] (unsigned x) { while (parent[x] != x) x = parent[x]; return x; };
  auto unite = [&] (unsigned a, unsigned b) {
    a = find (a); b = find (b);
    if (a != b) parent[a > b ? a : b] = a > b ? b : a;
  };
  std::vector<std::pair<unsigned, unsigned>> oneway;      /* (f, k) */
  for (unsigned p = 0; p < nl; p++)
    for (int o = D.con_off[p]; o < D.con_off[p + 1]; o++) {
      const unsigned q = D.con[o].other;
      const int gate = D.con[o].gate;
      if (parent[p] == none || parent[q] == none) continue;
      if (gate < 0 || c[gate >> 1] > 1e-4) unite (p, q);
      else oneway.push_back ((gate & 1) ? std::make_pair (p, q) : std::make_pair (q, p));
    }
  for (bool changed = true; changed; ) {
    changed = false;
    for (const auto & r : oneway) {
      const unsigned f = find (r.first), k = find (r.second);
      if (L[f] < L[k]) { L[k] = L[f]; changed = true; }
    }
  }
  for (unsigned p = 0; p < nl; p++)
    if (parent[p] == p) parent[p] = L[p];
  for (size_t o = 0; o + 1 < D.periodic.size (); o += 2)
    if (parent[D.periodic[o]] != none && parent[D.periodic[o + 1]] != none)
      unite (D.periodic[o], D.periodic[o + 1]);
  std::vector<unsigned> rank (nl, 0);
  unsigned n = 0;
  for (unsigned p = 0; p < nl; p++)
    if (parent[p] == p) rank[p] = n++;
  tag.assign (nl, 0);
  for (unsigned p = 0; p < nl; p++)
    if (parent[p] != none) tag[p] = 1 + rank[find (p)];
  return n;
}

// no exception crosses the C ABI: a tree too large for the host comes back as an error
int plan_tree_create (int dim, gfship_refine_fn refine, void * ctx, const int * side, TreePlans & h)
try {
  h.sw = read_switches ();
  int e = plan_tree (dim, refine, ctx, side, h.T);
  if (e) return e;
  h.sweep.resize (h.T.H.depth + 1);
  for (int m = 0; m <= h.T.H.depth; m++)
    if ((e = plan_sweep (h.T, m, h.sw.tree_debug, h.sweep[m]))) return e;
  for (int k = 0; k < 1 + dim; k++)
    h.faces[k] = plan_faces (h.T, k);
  return GFSHIP_OK;
}
catch (const std::bad_alloc &) {
  set_error ("gfship_tree_create: out of host memory while the tree was built");
  return GFSHIP_EUNSUPPORTED;
}

// ---- the host checks -------------------------------------------------------------------------------

namespace {


const int new_tree_bc[6] = { };      /* GFSHIP_BC_SYMMETRY on every side: the conditions of a new tree */

struct HostReader {
  const double * p;
  double operator() (const Topo & T, Cell c) const { return p[T.gi (c)]; }
};

// pseudo-random values in [-1, 1] (xorshift)
void random_fill (unsigned long long seed, std::vector<double> & u, std::vector<double> & rhs)
{
  for (size_t g = 0; g < u.size (); g++) {
    seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
    u[g] = (double) (seed % 2000001)/1e6 - 1.;
    seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
    rhs[g] = (double) (seed % 2000001)/1e6 - 1.;
  }
}

// The items of a plan (the cells of a sweep plan, the nodes of a loop plan) as the tape kernels run them: the items
// of a level -- `items' holds (level, item), sorted by level -- backwards, the stores of a level after its loads.
// off: 3 per item, g: the cell an item writes; op 0: relax, op 1: diffusion_relax with the weight w
void run_levels (const Topo & T, const std::vector<int> & ti, const std::vector<double> & td, const std::vector<int> & tv,
		 const std::vector<int> & off, const std::vector<int> & g_of, const std::vector<std::pair<int, int>> & items,
		 std::vector<double> & u, const std::vector<double> & rhs, double omega, int op, double w)
{
  size_t k0 = 0;
  while (k0 < items.size ()) {
    size_t k1 = k0;
    while (k1 < items.size () && items[k1].first == items[k0].first) k1++;
    std::vector<std::pair<int, double>> out;
    for (size_t q = k1; q-- > k0; ) {
      const int k = items[q].second;
      std::vector<double> vals;
      for (int v = off[3*k + 2]; v < off[3*(k + 1) + 2]; v++) vals.push_back (u[tv[v]]);
      TapeCursor cur = { ti.data () + off[3*k], td.data () + off[3*k + 1], vals.data () };
      const int g = g_of[k];
      double x;
      if (*cur.ti == K_GHOST)
	x = (*cur.td)*(*cur.tv);
      else if (op == 0) {
	const double self = *cur.tv++;
	double ga, gb;
	tape_cell (cur, T.nd (), T.dim, T.ncd (), ga, gb);
	x = 0.;
	if (ga != 0.)
	  x = T.dim == 2 ? (1. - omega)*self + omega*(gb - rhs[g])/ga : (gb - rhs[g])/ga;
      }
      else {      /* t_relax_nodes, op 1 */
	cur.tv++;
	double ga, gb;
	tape_cell (cur, T.nd (), T.dim, T.ncd (), ga, gb, w);
	int l = 0;
	while (g >= T.off[l + 1]) l++;
	const double h = 1./(1 << l);
	const double aa = 1.*h*h;
	ga = 1. + ga/aa;
	x = (gb/aa + rhs[g])/ga;
      }
      out.push_back ({ g, x });
    }
    for (auto & kv : out) u[kv.first] = kv.second;      /* the level's stores after its loads */
    k0 = k1;
  }
}

struct CheckStats { long long updates = 0, sweep_levels = 0, loop_levels = 0, differ = 0, hazards = 0, no_flow = 0; };

// For every level m the relax loop of nrelax sweeps on pseudo-random values, several ways on the host, compared bit
// for bit: (1) the reference's program: copies of the ghosts, the cells in tree order through the stencil code that
// walks the tree (tree.hpp), sweep after sweep; (2) sweep after sweep through the compiled stencils, the cells of a
// dependency level in REVERSE order; (3) the plan of the whole loop, the nodes of a level in reverse order; (4) the
// flow plan with the kernel's timing of loads and stores.
// op 0: relax with the conditions of P, all four; op 1: diffusion_relax with the conditions of U -- (1) with the
// coefficients fdir as the reference computes them, (3) and (4) with w on every face as the device runs them
int check_loops (const TreePlans & tr, unsigned nrelax, int op, double w, const std::vector<double> & fdir, CheckStats & st)
{
  const Topo & T = tr.T.H;
  const int ncell = tr.T.ncell;
  const Sgn6 sg = op == 0 ? homogeneous_signs (tr.T.side, new_tree_bc) : homogeneous_signs_u (tr.T.side, new_tree_bc, 0);
  const double omega = 1.;
  for (int m = 0; m <= T.depth; m++) {
    const SweepPlan & S = tr.sweep[m];
    LoopPlan P;
    int e = plan_loop (tr.T, S, m, nrelax, sg, tr.sw.flow_width, tr.sw.tree_debug, P);
    if (e) return e;
    std::vector<double> u0 (ncell), rhs (ncell);
    random_fill (88172645463325252ull + (op == 0 ? 1 : 7)*m, u0, rhs);
    std::vector<double> a = u0, b = u0, c3 = u0, c4 = u0;
    std::vector<Cell> order;
    traverse (T, root_cell (T), T_LEVEL_LEAFS, m, [&] (Cell c) { order.push_back (c); });
    for (unsigned sw = 0; sw < nrelax; sw++) {      /* (1) */
      for (const Ghost & G : S.ghosts) a[G.g] = sg.s[G.side]*a[G.img];
      HostReader R = { a.data () };
      for (Cell c : order) {
	const int g = T.gi (c);
	a[g] = op == 0 ? relax_cell (T, c, R, rhs[g], omega, m) :
	  diffusion_relax_cell (T, c, R, rhs[g], WDirect { fdir.data () }, m);
      }
    }
    if (op == 0) {      /* (2), the dependency levels recomputed from the read sets */
      LevelScheduler sched (ncell);
      std::vector<std::pair<int, int>> items;
      for (size_t c = 0; c < S.g.size (); c++)
	items.push_back ({ sched.cell (S.g[c], S.tv.data () + S.cell_off[3*c + 2], S.tv.data () + S.cell_off[3*(c + 1) + 2]),
	      (int) c });
      std::stable_sort (items.begin (), items.end (), [] (const std::pair<int, int> & p, const std::pair<int, int> & q) {
	  return p.first < q.first; });
      st.sweep_levels += (long long) sched.nlev*nrelax;
      for (unsigned sw = 0; sw < nrelax; sw++) {
	for (const Ghost & G : S.ghosts) b[G.g] = sg.s[G.side]*b[G.img];
	run_levels (T, S.ti, S.td, S.tv, S.cell_off, S.g, items, b, rhs, omega, 0, 1.);
      }
    }
    else
      b = a;
    {      /* (3) */
      std::vector<std::pair<int, int>> items;
      for (int k = 0; k < P.nnodes (); k++) items.push_back ({ P.node_level[k], k });
      st.loop_levels += P.nlev;
      run_levels (T, P.ti, P.td, P.tv, P.node_off, P.node_g, items, c3, rhs, omega, op, w);
    }
    if (P.flow) {      /* (4) */
      const long long hz = flow_emulate (*P.flow, T.dim, c4, rhs, omega, op, w);
      st.hazards += hz;
      if (op == 0 && tr.sw.tree_debug) {
	long long nd4 = 0;
	for (int g = 0; g < ncell; g++) nd4 += memcmp (&a[g], &c4[g], sizeof (double)) != 0;
	fprintf (stderr, "gfship_tree: flow plan of level %d: %lld hazards, %lld values differ\n", m, hz, nd4);
	int widest = 0;
	for (int L = 0; L < P.flow->nlev; L++)
	  widest = std::max (widest, P.flow->lev_off[L + 1] - P.flow->lev_off[L]);
	fprintf (stderr, "gfship_tree: flow plan of level %d: %d levels, widest %d\n", m, P.flow->nlev, widest);
      }
    }
    else {
      st.no_flow++;
      c4 = a;
    }
    st.updates += (long long) order.size ()*nrelax;
    for (int g = 0; g < ncell; g++)
      if (memcmp (&a[g], &b[g], sizeof (double)) || memcmp (&a[g], &c3[g], sizeof (double)) ||
	  memcmp (&a[g], &c4[g], sizeof (double)))
	st.differ++;
  }
  return 0;
}

// FNV-1a-64 over the members of the elements of an array, the length first
struct Fnv {
  unsigned long long h = 14695981039346656037ull;
  template <class X> std::enable_if_t<std::is_arithmetic<X>::value> put (X x)
  {
    for (size_t i = 0; i < sizeof x; i++) { h ^= ((const unsigned char *) &x)[i]; h *= 1099511628211ull; }
  }
  void put (const Cell & c) { put (c.l); put (c.q); }
  void put (const Ghost & G) { put (G.g); put (G.img); put (G.side); put (G.l); }
  void put (const FaceRec & f) { put (f.cell); put (f.neighbor); put (f.d); }
  void put (const FlowRec & r) { put (r.w0); put (r.out_g); for (int j = 0; j < FLOW_NIN; j++) put (r.in[j]); }
  template <class X> void array (const std::vector<X> & v)
  {
    put ((unsigned long long) v.size ());
    for (const X & x : v) put (x);
  }
};

} // namespace

} } // namespace gfship::tree

using namespace gfship;
using namespace gfship::tree;

extern "C" {

/* Host-side self-check of the plans of a tree, without a device (for the CPU tests): check_loops with op 0.
   stats[0] = cells of all sweeps, [1] = dependency levels sweep after sweep, [2] = levels of the loop
   plans, [3] = cells whose results differ + hazards of the flow plans (0 when the plans are right). */
int gfship_tree_host_check (int dim, gfship_refine_fn refine, void * ctx, const int * side,
			    unsigned nrelax, long long stats[4])
{
  GFSHIP_CHECK (refine && stats && nrelax >= 1, GFSHIP_EINVAL, "gfship_tree_host_check: bad argument");
  TreePlans tr;
  int e = plan_tree_create (dim, refine, ctx, side, tr);
  if (e) return e;
  CheckStats st;
  e = check_loops (tr, nrelax, 0, 1., { }, st);
  stats[0] = st.updates; stats[1] = st.sweep_levels; stats[2] = st.loop_levels; stats[3] = st.differ + st.hazards;
  return e;
}

// gfship_tree_host_check for the diffusion relax (op 1) with the coefficients of one w
int gfship_tree_host_check_diffusion (int dim, gfship_refine_fn refine, void * ctx, const int * side,
				      unsigned nrelax, double w, long long stats[6])
{
  GFSHIP_CHECK (refine && stats && nrelax >= 1 && w > 0., GFSHIP_EINVAL, "gfship_tree_host_check_diffusion: bad argument");
  TreePlans tr;
  int e = plan_tree_create (dim, refine, ctx, side, tr);
  if (e) return e;
  const Topo & T = tr.T.H;
  // the coefficients as the reference computes them for this w (the plans of the device take w on every face)
  std::vector<double> fdir;
  WArithDouble ard = { w, w/(T.nc ()/2) };
  diffusion_coefficients_gen (T, ard, fdir);
  long long not_w = 0;
  for (double a : fdir)
    if (a != 0. && a != w) not_w++;
  if (!diffusion_weights_exact (T)) not_w = - not_w - 1;      /* the tree would be refused */
  CheckStats st;
  e = check_loops (tr, nrelax, 1, w, fdir, st);
  stats[0] = st.updates; stats[1] = st.loop_levels; stats[2] = not_w; stats[3] = st.differ; stats[4] = st.hazards;
  stats[5] = st.no_flow;
  return e;
}

/* The droplet plan of a tree and the closed form of gfs_domain_tag_droplets on it, without a device (for the CPU
   tests; see gfship.h) */
int gfship_tree_host_tag_droplets (int dim, gfship_refine_fn refine, void * ctx, const int * side, long long ncell,
				   const double * c, long long nleaves, unsigned * tags, unsigned * n, long long counts[3])
try {
  GFSHIP_CHECK (refine && c && tags && n && counts, GFSHIP_EINVAL, "gfship_tree_host_tag_droplets: bad argument");
  TreePlans tr;
  int e = plan_tree_create (dim, refine, ctx, side, tr);
  if (e) return e;
  GFSHIP_CHECK (ncell == tr.T.ncell && nleaves == (long long) tr.T.hleaves.size (), GFSHIP_EINVAL,
		"gfship_tree_host_tag_droplets: the tree has %d cells and %zu leaves", tr.T.ncell, tr.T.hleaves.size ());
  DropletPlan D;
  if ((e = plan_droplets (tr.T, D))) return e;
  std::vector<unsigned> tag;
  *n = droplet_tags_host (tr.T, D, c, tag);
  std::copy (tag.begin (), tag.end (), tags);
  counts[0] = (long long) D.con.size (); counts[1] = D.ngated; counts[2] = (long long) D.periodic.size ()/2;
  return GFSHIP_OK;
}
catch (const std::bad_alloc &) {
  set_error ("gfship_tree_host_tag_droplets: out of host memory");
  return GFSHIP_EUNSUPPORTED;
}

/* lab: FNV-1a-64 digests of everything a device tree of these arguments uploads, with the Poisson loop plans of
   nrelax sweeps on every level (see gfship.h) */
int gfship_tree_host_plan_digest (int dim, gfship_refine_fn refine, void * ctx, const int * side,
				  unsigned nrelax, unsigned long long out[5])
{
  GFSHIP_CHECK (refine && out && nrelax >= 1, GFSHIP_EINVAL, "gfship_tree_host_plan_digest: bad argument");
  TreePlans tr;
  int e = plan_tree_create (dim, refine, ctx, side, tr);
  if (e) return e;
  Fnv f[5];
  auto add = [&] (int k, const auto &... v) { (f[k].array (v), ...); };
  const TreePlan & T = tr.T;
  add (0, T.hflag, T.h_nbtab, T.h_child0, T.h_cmask, T.h_idtab, T.hleaves);
  for (const std::vector<Cell> & nl : T.hnonleaf) add (0, nl);
  add (0, T.hghost_leaves);
  for (int m = 0; m <= T.H.depth; m++) {
    const SweepPlan & S = tr.sweep[m];
    add (1, S.cells, S.lev_off, S.ghosts, S.ti, S.td, S.tv, S.cell_off, S.chunk);
    LoopPlan P;
    if ((e = plan_loop (T, S, m, nrelax, homogeneous_signs (T.side, new_tree_bc), tr.sw.flow_width, tr.sw.tree_debug, P))) return e;
    add (2, P.ti, P.td, P.tv, P.node_off, P.node_g, P.chunk, P.desc, P.rec);
    f[3].put (P.flow ? 1 : 0);
    if (P.flow) {
      const FlowProgram & F = *P.flow;
      f[3].put (F.width); f[3].put (F.npos); f[3].put (F.nlev); f[3].put (F.nct);
      add (3, F.gidx, F.rec, F.lev_off, F.ct);
    }
  }
  for (int k = 0; k < 1 + dim; k++)
    add (4, tr.faces[k].faces, tr.faces[k].inc_off, tr.faces[k].inc);
  for (int k = 0; k < 5; k++) out[k] = f[k].h;
  return GFSHIP_OK;
}

}
