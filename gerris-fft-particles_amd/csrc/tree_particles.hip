// tree_particles.hip -- the point sampler (GfsOutputLocation) and the Lagrangian tracers (GfsParticle in a
// GfsParticleList) on a statically refined quadtree / octree.
//
// One thread per point or particle.  locate = the descent of ftt_cell_locate (src/ftt.c:1535-1574) over the tables
// of the tree (cmask, child0) to the leaf that holds the point; interpolate = gfs_interpolate (src/fluid.c:2697-2710).
// On a refined tree the cells of a corner are found by a walk (do_path, :2925-2981) that meets coarser
// neighbours, deeper neighbours and T-junctions (cell_corner_neighbor, :2813-2846; t_junction_interpolator,
// :2879-2923, which calls gfs_cell_corner_interpolator of the coarse neighbour again).  The tree is static: that
// walk is done ONCE on the host (Walker below), in the reference's order of operations, and its result is kept as
// rows of (cell, weight) pairs, CSR, keyed by (leaf, corner).  The device sums weight * value along a row, in row
// order (gfs_cell_corner_value, :3081-3101).
//
// A corner whose walk finds exactly the cells of the uniform box -- the 2^dim cells of the leaf's own level around
// the corner, those with two or more coordinates in the ghost layer absent -- needs no row: all its weights are
// equal and the kernel does the arithmetic of particles.hip (interpolate ()).  A byte per cell of
// the dense levels says which corners of a leaf read the table, an int where the rows of the leaf start.
//
// Pinned bit for bit on tests/tree_sampler_reference.py (a restatement of the reference on explicit cell trees,
// written from the reference) in tests/test_gpu_tree_sampler.py.
//
// GfsParticulate with forces on a tree (gfship_particulates_create_tree): the force arithmetic of
// particulate_forces.hpp, which the kernels of particles.hip call too, on the locate / interpolate above, with
// gfs_center_gradient (src/fluid.c:434-475) of Du/Dt and of the vorticity taken at the leaf through
// tree::center_gradient (tree.hpp) -- a coarser neighbour at x = 3/2, a neighbour with children at x = 3/4.  Pinned
// on tests/tree_forces_reference.py in tests/test_gpu_tree_particulates.py.
//
// The events of a list of particulates that run on a box too (void fraction, spreading, sources, feed) keep here the
// kernels that walk the tree and TreeMesh, which launches them; their host side is particle_events.hpp.
#include "particle_events.hpp"
#include "particulate_forces.hpp"
#include "tree_particles.hpp"
#include <cmath>
#include <cstdlib>
#include <vector>

namespace gfship {

using tree::Topo;
using tree::Cell;
using tree::exists;

namespace {

// GfsInterpolator (src/fluid.h): at most 7 cells in 2-D, 29 in 3-D (g_assert of interpolator_merge, :2861-2863)
constexpr int INTER_MAX = 29;
struct Inter { int n; int c[INTER_MAX + 3]; double w[INTER_MAX + 3]; };

struct SamplerTables {       // device
  unsigned char * corner_bits = nullptr;     // [cell]: bit ic = corner ic of the leaf reads its row of the table
  int * row_base = nullptr;                  // [cell]: the first row of the leaf (its corners with a bit, in order)
  int * row_ptr = nullptr;                   // [rows + 1]
  int * col = nullptr;                       // [entries]: Topo::gi of the cell
  double * w = nullptr;                      // [entries]
  long long stats[5] = { 0, 0, 0, 0, 0 };
};

void sampler_tables_free (void * p)
{
  SamplerTables * S = (SamplerTables *) p;
  (void) hipFree (S->corner_bits); (void) hipFree (S->row_base); (void) hipFree (S->row_ptr);
  (void) hipFree (S->col); (void) hipFree (S->w);
  delete S;
}

// corner[i], src/fluid.c:2588-2605
const int corner2[4][3] = { {1, 3, -1}, {0, 3, -1}, {0, 2, -1}, {1, 2, -1} };
const int corner3[8][3] = { {1, 3, 4}, {0, 3, 4}, {0, 2, 4}, {1, 2, 4}, {1, 3, 5}, {0, 3, 5}, {0, 2, 5}, {1, 2, 5} };
// path[i][j], src/fluid.c:2938-2954
const int path2[4][2][3] = { {{1,2,1}, {2,1,2}}, {{2,-1,3}, {-1,2,0}}, {{1,-2,3}, {-2,1,0}}, {{-1,-2,2}, {-2,-1,1}} };
const int path3[8][3][4] = {
  {{1,2,3,1},    {2,1,3,2},    {3,1,2,4}},
  {{2,3,-1,3},   {3,2,-1,5},   {-1,2,3,0}},
  {{1,-2,3,3},   {3,-2,1,6},   {-2,3,1,0}},
  {{3,-1,-2,7},  {-2,-1,3,1},  {-1,-2,3,2}},
  {{2,1,-3,6},   {1,2,-3,5},   {-3,1,2,0}},
  {{2,-1,-3,7},  {-1,2,-3,4},  {-3,2,-1,1}},
  {{1,-2,-3,7},  {-2,1,-3,4},  {-3,1,-2,2}},
  {{-1,-2,-3,6}, {-2,-1,-3,5}, {-3,-1,-2,3}} };
// b[FTT_CELL_ID][d] of ftt_cell_neighbor_is_brother, src/ftt.h:624-631
const int brother2[4][4] = { {1,0,0,1}, {0,1,0,1}, {1,0,1,0}, {0,1,1,0} };
const int brother3[8][6] = { {1,0,0,1,0,1}, {0,1,0,1,0,1}, {1,0,1,0,0,1}, {0,1,1,0,0,1},
			     {1,0,0,1,1,0}, {0,1,0,1,1,0}, {1,0,1,0,1,0}, {0,1,1,0,1,0} };

// gfs_cell_corner_interpolator (src/fluid.c:3015-3069) and what it calls, max_level = -1, centered, no solid
struct Walker {
  const Topo & T;
  bool overflow = false;
  explicit Walker (const Topo & t) : T (t) {}

  // cells with two or three coordinates in the ghost layer do not exist in the reference (every side has a cell
  // tree of its own whose root knows the box and nothing else, src/boundary.c:652-685)
  int ghost_coordinates (Cell c) const {
    const int n = T.n (c.l), i = T.ci (c), j = T.cj (c), k = T.ck (c);
    return (i < 1 || i > n) + (j < 1 || j > n) + (T.dim == 3 && (k < 1 || k > n));
  }
  Cell absent_if_edge (Cell c) const {
    if (exists (c) && ghost_coordinates (c) > 1) c.q = -1;
    return c;
  }
  Cell neighbor (Cell c, int d) const { return absent_if_edge (T.neighbor (c, d)); }
  Cell child_corner (Cell c, const int d[3]) const { return absent_if_edge (T.child_corner (c, d[0], d[1], d[2])); }
  Cell parent (Cell c) const { return T.make (c.l - 1, (T.ci (c) + 1)/2, (T.cj (c) + 1)/2, T.dim == 3 ? (T.ck (c) + 1)/2 : 1); }
  bool boundary (Cell c) const { return !T.interior (c); }          /* GFS_CELL_IS_BOUNDARY */
  bool neighbor_is_brother (Cell c, int d) const {                  /* src/ftt.h:620-638 */
    if (c.l == 0) return false;
    return T.dim == 2 ? brother2[T.id (c)][d] : brother3[T.id (c)][d];
  }

  // cell_corner_neighbor, :2813-2846
  Cell corner_neighbor (Cell cell, const int d[3], bool & t_junction) const {
    const Cell nb = neighbor (cell, d[0]);
    if (!exists (nb))
      return nb;
    if (nb.l < cell.l) {               /* neighbor is at a shallower level */
      const Cell cc = child_corner (parent (cell), d);
      if (!(cc.l == cell.l && cc.q == cell.q))
	t_junction = true;
      return nb;
    }
    if (T.leaf (nb))
      return nb;
    const int d1[3] = { d[0] ^ 1, d[1], d[2] };      /* neighbor is at a deeper level */
    const Cell n = child_corner (nb, d1);
    return exists (n) ? n : nb;
  }

  // interpolator_merge, :2848-2870
  void merge (Inter & a, const Inter & b) {
    for (int i = 0; i < b.n; i++) {
      int j = 0;
      while (j < a.n && b.c[i] != a.c[j]) j++;
      if (j < a.n)
	a.w[j] += b.w[i];
      else {
	if (j >= (T.dim == 2 ? 7 : INTER_MAX)) { overflow = true; return; }
	a.c[j] = b.c[i];
	a.w[j] = b.w[i];
	a.n++;
      }
    }
  }
  static void scale (Inter & a, double b) { for (int i = 0; i < a.n; i++) a.w[i] *= b; }

  // t_junction_interpolator, :2879-2923
  void t_junction (Cell cell, const int d[3], Cell n, Inter & inter) {
    int d1[3] = { d[0] ^ 1, d[1], d[2] };
    Inter a;
    if (T.dim == 2) {
      corner_interpolator (n, d1, inter);
      d1[1] = d[1] ^ 1;
      corner_interpolator (n, d1, a);
      merge (inter, a);
      scale (inter, 0.5);
      return;
    }
    corner_interpolator (n, d1, inter);
    if (neighbor_is_brother (cell, d[1])) {
      d1[1] = d[1] ^ 1;
      corner_interpolator (n, d1, a);
      merge (inter, a);
      if (neighbor_is_brother (cell, d[2])) {
	d1[2] = d[2] ^ 1;
	corner_interpolator (n, d1, a);
	merge (inter, a);
	d1[1] = d[1];
	corner_interpolator (n, d1, a);
	merge (inter, a);
	scale (inter, 0.25);
      }
      else
	scale (inter, 0.5);
    }
    else {
      d1[2] = d[2] ^ 1;
      corner_interpolator (n, d1, a);
      merge (inter, a);
      scale (inter, 0.5);
    }
  }

  // do_path, :2925-2981
  bool do_path (Cell cell, int i, Cell n[8], const int d[3], Inter & inter) {
    for (int j = 0; j < T.dim; j++) {
      const int * P = T.dim == 2 ? path2[i][j] : path3[i][j];
      const int k = P[T.dim];
      if (!exists (n[k])) {
	bool tj = false;
	int d1[3] = { -1, -1, -1 };
	for (int l = 0; l < T.dim; l++)
	  d1[l] = P[l] < 0 ? (d[- P[l] - 1] ^ 1) : d[P[l] - 1];
	n[k] = corner_neighbor (cell, d1, tj);
	if (tj) {
	  t_junction (cell, d1, n[k], inter);
	  return true;
	}
	if (exists (n[k]) && do_path (n[k], k, n, d, inter))
	  return true;
      }
    }
    return false;
  }

  // gfs_cell_corner_interpolator, :3015-3069; n_out (optional): the cells of the walk when it met no T-junction
  bool corner_interpolator (Cell cell, const int d[3], Inter & inter, Cell * n_out = nullptr) {
    Cell n[8];
    while (!T.leaf (cell)) {           /* :3028-3031 */
      const Cell ch = child_corner (cell, d);
      if (!exists (ch)) break;
      cell = ch;
    }
    n[0] = cell;
    for (int i = 1; i < T.nc (); i++) n[i].l = 0, n[i].q = -1;
    inter.n = 0;
    if (do_path (cell, 0, n, d, inter))
      return true;
    double w = 0.;
    int boundaries = 0;
    inter.n = 0;
    for (int i = 0; i < T.nc (); i++)
      if (exists (n[i])) {
	/* distance (), :2983-2992 */
	const double a = 1./(T.size (n[i])*(T.dim == 2 ? 0.707106781185 : 0.866025403785) + 1e-12);
	inter.c[inter.n] = T.gi (n[i]);
	inter.w[inter.n++] = a;
	w += a;
	if (boundary (n[i]))
	  boundaries++;
      }
    if (inter.n == T.dim + 1 && boundaries == T.dim) {   /* corners of domain, :3057-3065 */
      w -= inter.w[0];
      for (int i = 0; i < inter.n - 1; i++) {
	inter.c[i] = inter.c[i + 1];
	inter.w[i] = inter.w[i + 1];
      }
      inter.n--;
    }
    scale (inter, 1./w);
    if (n_out)
      for (int i = 0; i < T.nc (); i++) n_out[i] = n[i];
    return false;
  }

  // does the walk of this corner of a leaf give what the arithmetic of the uniform box gives?  The cells of the
  // leaf's level at the 2^dim offsets towards the corner, present exactly where at most one coordinate is in the
  // ghost layer.  (Then all sizes are equal and so are the weights, the sums and the domain-corner rule.)
  bool uniform_corner (Cell leaf, const int d[3], const Cell n[8]) const {
    const int r = T.r (leaf.l), nn = T.n (leaf.l);
    const int ijk[3] = { T.ci (leaf), T.cj (leaf), T.dim == 3 ? T.ck (leaf) : 1 };
    const int sg[3] = { d[0] == 0 ? 1 : -1, d[1] == 2 ? 1 : -1, d[2] == 4 ? 1 : -1 };
    for (int m = 0; m < T.nc (); m++) {
      int out = 0, p[3];
      for (int a = 0; a < 3; a++) {
	p[a] = ijk[a] + (a < T.dim && (m & (1 << a)) ? sg[a] : 0);
	if (a < T.dim && (p[a] < 1 || p[a] > nn)) out++;
      }
      const int q = p[0] + r*(p[1] + (T.dim == 3 ? r*p[2] : 0));
      if (out <= 1) {
	if (!(exists (n[m]) && n[m].l == leaf.l && n[m].q == q)) return false;
      }
      else if (exists (n[m]))
	return false;
    }
    return true;
  }
};

int sampler_build (gfship_tree * tr, const TreeView & V, SamplerTables ** out)
{
  (void) tr;
  const Topo & T = V.H;
  const int nc = T.nc ();
  std::vector<unsigned char> bits (V.ncell, 0);
  std::vector<int> base (V.ncell, 0), ptr (1, 0), col;
  std::vector<double> w;
  Walker W (T);
  int longest = 0;
  for (int t = 0; t < V.nleaves; t++) {
    const Cell leaf = V.hleaves[t];
    const int g = T.gi (leaf);
    base[g] = (int) ptr.size () - 1;
    for (int ic = 0; ic < nc; ic++) {
      const int * d = T.dim == 2 ? corner2[ic] : corner3[ic];
      Inter I;
      Cell n[8];
      const bool tj = W.corner_interpolator (leaf, d, I, n);
      GFSHIP_CHECK (!W.overflow && I.n <= (T.dim == 2 ? 7 : INTER_MAX), GFSHIP_EUNSUPPORTED,
		    "a corner interpolator of this tree has more than %d cells (GfsInterpolator, src/fluid.h)",
		    T.dim == 2 ? 7 : INTER_MAX);
      if (!tj && W.uniform_corner (leaf, d, n))
	continue;
      bits[g] |= (unsigned char) (1 << ic);
      for (int e = 0; e < I.n; e++) {
	GFSHIP_CHECK (I.c[e] >= 0 && I.c[e] < V.ncell, GFSHIP_EINVAL, "corner interpolator: cell %d out of range", I.c[e]);
	col.push_back (I.c[e]);
	w.push_back (I.w[e]);
      }
      if (I.n > longest) longest = I.n;
      ptr.push_back ((int) col.size ());
    }
  }
  SamplerTables * S = new SamplerTables;
  S->stats[0] = (long long) V.nleaves*nc;
  S->stats[1] = (long long) ptr.size () - 1;
  S->stats[2] = (long long) col.size ();
  S->stats[3] = (long long) (bits.size () + base.size ()*sizeof (int) + ptr.size ()*sizeof (int) +
			     col.size ()*(sizeof (int) + sizeof (double)));
  S->stats[4] = longest;
  if (col.empty ()) { col.push_back (0); w.push_back (0.); }      /* no empty allocation */
  auto up = [] (void ** dst, const void * src, size_t bytes) -> hipError_t {
    hipError_t e = hipMalloc (dst, bytes);
    if (e == hipSuccess) e = hipMemcpy (*dst, src, bytes, hipMemcpyHostToDevice);
    return e;
  };
  hipError_t e = up ((void **) &S->corner_bits, bits.data (), bits.size ());
  if (e == hipSuccess) e = up ((void **) &S->row_base, base.data (), base.size ()*sizeof (int));
  if (e == hipSuccess) e = up ((void **) &S->row_ptr, ptr.data (), ptr.size ()*sizeof (int));
  if (e == hipSuccess) e = up ((void **) &S->col, col.data (), col.size ()*sizeof (int));
  if (e == hipSuccess) e = up ((void **) &S->w, w.data (), w.size ()*sizeof (double));
  if (e != hipSuccess) {
    sampler_tables_free (S);
    return hip_fail (e, "the tables of the tree sampler", __FILE__, __LINE__);
  }
  *out = S;
  return GFSHIP_OK;
}

int sampler_get (gfship_tree * tr, TreeView * V, SamplerTables ** S)
{
  tree_view (tr, V);
  GFSHIP_HIP (hipSetDevice (V->device));
  if (!*V->sampler) {
    SamplerTables * built = nullptr;
    int r = sampler_build (tr, *V, &built);
    if (r) return r;
    *V->sampler = built;
    *V->sampler_free = sampler_tables_free;
  }
  *S = (SamplerTables *) *V->sampler;
  return GFSHIP_OK;
}

// ---- device ------------------------------------------------------------------------------------------

struct TreeSamp {
  Topo T;
  const unsigned char * corner_bits;
  const int * row_base, * row_ptr, * col;
  const double * w;
};

template <int NV> struct Vars { const double * p[NV]; };    // the arrays (all levels) of NV variables

// ftt_cell_locate (root, target, -1): tree_locate, tree_particles.hpp, over S.T

// gfs_interpolate (src/fluid.c:2697-2710) of NV variables at p inside the leaf c; v[]: the arrays of all levels
template <int DIM, int NV>
__device__ void tree_interpolate (const TreeSamp & S, const Vars<NV> & v, const Leaf & c,
				  const double p_[3], double (& out)[NV])
{
  constexpr int NC = 4*(DIM - 1);
  const int n = 1 << c.l, r = n + 2;
  const double h = 1./n;
  const int cell[3] = { c.i, c.j, c.k };
  bool outm[3], outp[3];    // is cell - 1 / cell + 1 a ghost along each axis?
#pragma unroll
  for (int a = 0; a < DIM; a++) {
    outm[a] = cell[a] - 1 < 1;
    outp[a] = cell[a] + 1 > n;
  }
  const double a_ = 1./(h*(DIM == 2 ? 0.707106781185 : 0.866025403785) + 1e-12);
  // corner directions, src/fluid.c:2588-2605
  const int c2[4][3] = { {-1,-1,0}, {1,-1,0}, {1,1,0}, {-1,1,0} };
  const int c3[8][3] = { {-1,-1,1}, {1,-1,1}, {1,1,1}, {-1,1,1},
			 {-1,-1,-1}, {1,-1,-1}, {1,1,-1}, {-1,1,-1} };
  double f[NV][NC + 1];
  // the corners of the uniform box: the 3^DIM cells of the leaf's level around the leaf (all of them allocated)
#pragma unroll
  for (int cv = 0; cv < NV; cv++) {
    const double * __restrict__ vl = v.p[cv] + c.g;
    double nb[DIM == 3 ? 27 : 9];
#pragma unroll
    for (int dz = (DIM == 3 ? -1 : 0); dz <= (DIM == 3 ? 1 : 0); dz++)
#pragma unroll
      for (int dy = -1; dy <= 1; dy++)
#pragma unroll
	for (int dx = -1; dx <= 1; dx++)
	  nb[(dx + 1) + 3*(dy + 1) + 9*(DIM == 3 ? dz + 1 : 0)] = vl[dx + dy*r + dz*r*r];
#pragma unroll
    for (int ic = 0; ic < NC; ic++) {
      int sg[3];
#pragma unroll
      for (int a = 0; a < 3; a++) sg[a] = DIM == 2 ? c2[ic][a] : c3[ic][a];
      double wsum = 0., w0 = 0.;
      int cnt = 0, boundaries = 0;
      bool ex[1 << DIM];
#pragma unroll
      for (int m = 0; m < (1 << DIM); m++) {
	int o = 0;
#pragma unroll
	for (int a = 0; a < DIM; a++)
	  if (m & (1 << a))
	    o += (sg[a] < 0 ? outm[a] : outp[a]) ? 1 : 0;
	ex[m] = o <= 1;
	if (ex[m]) {
	  if (cnt == 0) w0 = a_;
	  cnt++;
	  wsum += a_;
	  if (o > 0) boundaries++;
	}
      }
      const bool skip0 = (cnt == DIM + 1 && boundaries == DIM);   // domain corner: drop the central cell
      if (skip0)
	wsum -= w0;
      const double scale = 1./wsum;
      double s = 0.;
#pragma unroll
      for (int m = 0; m < (1 << DIM); m++) {
	const int ox = (m & 1) ? sg[0] : 0, oy = (m & 2) ? sg[1] : 0, oz = (DIM == 3 && (m & 4)) ? sg[2] : 0;
	const double val = nb[(ox + 1) + 3*(oy + 1) + 9*(DIM == 3 ? oz + 1 : 0)];
	if (ex[m] && !(skip0 && m == 0)) {
	  const double wm = a_*scale;
	  s += wm*val;
	}
      }
      f[cv][ic] = s;
    }
    f[cv][NC] = nb[1 + 3 + (DIM == 3 ? 9 : 0)];
  }
  // the corners at a change of level: gfs_cell_corner_value (:3081-3101) along the row of the table, one read of
  // (cell, weight) for all the variables
  const unsigned bits = S.corner_bits[c.g];
  if (bits) {
    int row = S.row_base[c.g];
#pragma unroll
    for (int ic = 0; ic < NC; ic++)
      if ((bits >> ic) & 1u) {
	const int e0 = S.row_ptr[row], e1 = S.row_ptr[row + 1];
	row++;
	double s[NV];
#pragma unroll
	for (int cv = 0; cv < NV; cv++) s[cv] = 0.;
	for (int e = e0; e < e1; e++) {
	  const int g = S.col[e];
	  const double we = S.w[e];
#pragma unroll
	  for (int cv = 0; cv < NV; cv++)
	    s[cv] += we*v.p[cv][g];
	}
#pragma unroll
	for (int cv = 0; cv < NV; cv++) f[cv][ic] = s[cv];
      }
  }
  // gfs_interpolate_from_corners, src/fluid.c:2640-2683
  const double o[3] = { -0.5 + (cell[0] - 0.5)*h, -0.5 + (cell[1] - 0.5)*h,
			DIM == 3 ? -0.5 + (cell[2] - 0.5)*h : 0. };
  const double size = h/2.;
  double p[3];
  p[0] = (p_[0] - o[0])/size;
  p[1] = (p_[1] - o[1])/size;
  p[2] = DIM == 3 ? (p_[2] - o[2])/size : 0.;
#pragma unroll
  for (int cv = 0; cv < NV; cv++) {
    const double (& F)[NC + 1] = f[cv];
    if (DIM == 2) {
      double x = (p[0] + p[1])/2., y = (p[1] - p[0])/2., val = F[4];
      if (x > 0.)
	val += x*(F[2] - F[4]);
      else
	val -= x*(F[0] - F[4]);
      if (y > 0.)
	val += y*(F[3] - F[4]);
      else
	val -= y*(F[1] - F[4]);
      out[cv] = val;
    }
    else {
      double k[8];
      k[0] = - F[0] + F[1] + F[2] - F[3] - F[4] + F[5] + F[6] - F[7];
      k[1] = - F[0] - F[1] + F[2] + F[3] - F[4] - F[5] + F[6] + F[7];
      k[2] =   F[0] + F[1] + F[2] + F[3] - F[4] - F[5] - F[6] - F[7];
      k[3] =   F[0] - F[1] + F[2] - F[3] + F[4] - F[5] + F[6] - F[7];
      k[4] = - F[0] + F[1] + F[2] - F[3] + F[4] - F[5] - F[6] + F[7];
      k[5] = - F[0] - F[1] + F[2] + F[3] + F[4] + F[5] - F[6] - F[7];
      k[6] =   F[0] - F[1] + F[2] - F[3] - F[4] + F[5] - F[6] + F[7];
      k[7] =   F[0] + F[1] + F[2] + F[3] + F[4] + F[5] + F[6] + F[7];
      out[cv] = (k[0]*p[0] + k[1]*p[1] + k[2]*p[2] +
		 k[3]*p[0]*p[1] + k[4]*p[0]*p[2] + k[5]*p[1]*p[2] +
		 k[6]*p[0]*p[1]*p[2] +
		 k[7])/8.;
    }
  }
}

// GfsOutputLocation (src/output.c:1182-1199)
template <int DIM>
__global__ void __launch_bounds__(256)
tree_sample_kernel (TreeSamp S, int np, const double * __restrict__ pos, const double * __restrict__ v,
		    double * __restrict__ out, unsigned char * __restrict__ inside)
{
  const int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= np) return;
  const double p[3] = { pos[3*(size_t) q], pos[3*(size_t) q + 1], DIM == 3 ? pos[3*(size_t) q + 2] : 0. };
  Leaf c;
  if (!tree_locate<DIM> (S, p, c)) {
    inside[q] = 0;
    out[q] = 0.;
    return;
  }
  Vars<1> vv;
  vv.p[0] = v;
  double r[1];
  tree_interpolate<DIM, 1> (S, vv, c, p, r);
  inside[q] = 1;
  out[q] = r[0];
}

struct TreePartArgs {
  int side[6];
  int n;
  double * pos[3];
  double * old[3];
  unsigned char * alive;
  const double * u[3];
  double dt;
};

// gfs_particle_bc, modules/particulatecommon.c:3326-3395, of a particle that went from po (in the leaf c0) to p:
// false if it is taken off the list; a periodic side puts it back (p and po change)
template <int DIM>
__device__ __forceinline__ bool tree_particle_bc (const TreeSamp & S, const int (& side)[6], const Leaf & c0,
						  double (& p)[3], double (& po)[3])
{
  bool keep = true;
  Leaf cn;
  if (!tree_locate<DIM> (S, p, cn)) {
    // boundarycell (:3151-3186): from the leaf of pos_old over the ftt_cell_face neighbours (same level, leaf or not,
    // or coarser) to the cell whose neighbour is a boundary cell
    int d = 0;
    Cell cc = { c0.l, c0.q };
    for (int guard = 0; guard < 4*(1 << S.T.depth); guard++) {
      const double h = 1./(1 << cc.l);
      const double cellpos[3] = { -0.5 + (S.T.ci (cc) - 0.5)*h, -0.5 + (S.T.cj (cc) - 0.5)*h,
				  DIM == 3 ? -0.5 + (S.T.ck (cc) - 0.5)*h : 0. };
      check_intersection<DIM> (cellpos, po, p, &d, h);
      const Cell nb = S.T.neighbor (cc, d);
      if (!exists (nb) || !S.T.interior (nb))
	break;
      cc = nb;
    }
    if (side[d] != GFSHIP_SIDE_PERIODIC)
      keep = false;                 /* taken off the list, nothing puts it back */
    else {
      // periodic_bc_particle (:3189-3214), box of size 1 matching itself
      const double size = 1.;
      const double normal = (double) (d ^ 1) - (double) d;
      double box_face = 0., box_face_nbr = 0.;
      box_face += normal*size/2.;
      box_face_nbr -= normal*size/2.;
      const double tolerance = size/1.e8;
      const double distance = (p[d/2] - box_face)*normal;
      p[d/2] = box_face_nbr + distance + normal*tolerance;
      po[d/2] = p[d/2];
    }
  }
  return keep;
}

// gfs_particle_list_event (modules/particulatecommon.c:980-1015) of GfsParticle tracers
template <int DIM>
__global__ void __launch_bounds__(256)
tree_particle_list_event_kernel (TreeSamp S, TreePartArgs A)
{
  const int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= A.n) return;
  if (A.alive[q] != 1) return;
  double p[3] = { A.pos[0][q], A.pos[1][q], DIM == 3 ? A.pos[2][q] : 0. };
  Leaf c0;
  // remove_particles_not_in_domain, :955-969
  if (!tree_locate<DIM> (S, p, c0)) {
    A.alive[q] = 0;
    return;
  }
  Vars<DIM> uu;
#pragma unroll
  for (int a = 0; a < DIM; a++) uu.p[a] = A.u[a];
  // gfs_particle_event (src/particle.c:31-44): pos_old = pos; gfs_domain_advect_point (src/domain.c:2764-2788)
  double po[3] = { p[0], p[1], p[2] };
  {
    double p1[3] = { p[0], p[1], p[2] }, vel[DIM];
    tree_interpolate<DIM, DIM> (S, uu, c0, po, vel);
#pragma unroll
    for (int a = 0; a < DIM; a++)
      p1[a] += A.dt*vel[a]/2.;
    Leaf c1;
    if (tree_locate<DIM> (S, p1, c1)) {
      tree_interpolate<DIM, DIM> (S, uu, c1, p1, vel);
#pragma unroll
      for (int a = 0; a < DIM; a++)
	p[a] += A.dt*vel[a];
    }
  }
  const bool keep = tree_particle_bc<DIM> (S, A.side, c0, p, po);
#pragma unroll
  for (int a = 0; a < DIM; a++) {
    A.pos[a][q] = p[a];
    A.old[a][q] = po[a];
  }
  if (!keep)
    A.alive[q] = 0;
}

// ---------------------------------------------------------------------------------------------
// GfsParticulate with forces on a tree (modules/particulatecommon.c:91-842): the forces of particulate_forces.hpp with
// the cell search, the interpolation and gfs_center_gradient of a tree.  fluid_rho = 1. (a tree has no alpha), the
// viscosity is the constant of GfsSourceDiffusion {} U.
// ---------------------------------------------------------------------------------------------
struct TreeListArgs { TreePartArgs P; };
struct TreeParticulateArgs : TreeListArgs, ParticleForceArgs {};      // uold: GFSHIP_TREE_UPREV ...

struct DevValue {            // GFS_VALUEI (cell, v)
  const double * p;
  __device__ __forceinline__ double operator() (const Topo & T, Cell c) const { return p[T.gi (c)]; }
};

// the sources of particulate_forces.hpp on a tree: the gradients the kernel has filled, u[c2] at the leaf
template <int DIM>
struct TreeGradient {
  const double (* g)[DIM];
  __device__ __forceinline__ double operator() (int c, int c2) const { return g[c][c2]; }
};
struct TreeCellU {
  const TreePartArgs & P; int g;
  __device__ __forceinline__ double operator() (int c2) const { return P.u[c2][g]; }
};

// the variables a GfsFunction of a GfsForceCoeff sees: coefficient_inputs (particulate_forces.hpp) at the
// particle's leaf
// (particulate_coeff_inputs_kernel, particles.hip, is this kernel on a box)
template <int DIM>
__global__ void __launch_bounds__(256)
tree_particulate_coeff_inputs_kernel (TreeSamp S, TreeParticulateArgs A)
{
  const TreePartArgs & P = A.P;
  const int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= P.n) return;
  if (P.alive[q] != 1) return;
  const double p[3] = { P.pos[0][q], P.pos[1][q], DIM == 3 ? P.pos[2][q] : 0. };
  Leaf c0;
  if (!tree_locate<DIM> (S, p, c0)) return;
  const unsigned o = A.orig[q];
  Vars<DIM> uu;
#pragma unroll
  for (int a = 0; a < DIM; a++) uu.p[a] = P.u[a];
  double fvel[DIM];
  tree_interpolate<DIM, DIM> (S, uu, c0, p, fvel);
  coefficient_inputs<DIM> (A, q, o, fvel, 1., ListViscosity { A });
}

// gfs_particulate_event (:768-842) in a gfs_particle_list_event (:980-1015)
// ONFLUID: compute_forces_onfluid (:753-765) in source_particulate_event (:2199-2206), as in particles.hip: every
// force of the list but GfsForceBuoy; `force' is written, and `mass' (compute_addedmass_force, :391); the particle
// does not move and stays on the list; a particle without a leaf gets the zero force and keeps its mass
// (particulate_list_event_kernel, particles.hip, is this kernel on a box)
template <int DIM, bool ONFLUID = false>
__global__ void __launch_bounds__(256)
tree_particulate_list_event_kernel (TreeSamp S, TreeParticulateArgs A)
{
  const TreePartArgs & P = A.P;
  const int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= P.n) return;
  if (P.alive[q] != 1) return;
  double p[3] = { P.pos[0][q], P.pos[1][q], DIM == 3 ? P.pos[2][q] : 0. };
  Leaf c0;
  // remove_particles_not_in_domain, :955-969
  if (!tree_locate<DIM> (S, p, c0)) {
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
  const Cell cell = { c0.l, c0.q };
  const double size = 1./(1 << c0.l);      /* ftt_cell_size of the leaf */
  const double fluid_rho = 1.;
  const double dt = P.dt;
  double po[3] = { p[0], p[1], p[2] };
  double vel[3] = { A.vel[0][o], A.vel[1][o], A.vel[2][o] };
  double mass = A.mass[o];
  const double volume = A.volume[o];
  double pf[3] = { 0., 0., 0. };
  // what several forces need -- the fluid velocity at the particle, Du/Dt, the gradients of the velocity at the
  // leaf -- is evaluated once
  ForceNeeds need;
  force_needs<ONFLUID> (A, need);
  double fvel[3] = { 0., 0., 0. }, fveln[3] = { 0., 0., 0. }, dudt[3] = { 0., 0., 0. };
  if (need.dudt) {
    // U and Un at the particle in one pass over the corner rows of the leaf
    Vars<2*DIM> uu;
#pragma unroll
    for (int a = 0; a < DIM; a++) { uu.p[a] = P.u[a]; uu.p[DIM + a] = A.uold[a]; }
    double r[2*DIM];
    tree_interpolate<DIM, 2*DIM> (S, uu, c0, p, r);
#pragma unroll
    for (int a = 0; a < DIM; a++) { fvel[a] = r[a]; fveln[a] = r[DIM + a]; }
  }
  else if (need.fvel) {
    Vars<DIM> uu;
#pragma unroll
    for (int a = 0; a < DIM; a++) uu.p[a] = P.u[a];
    double r[DIM];
    tree_interpolate<DIM, DIM> (S, uu, c0, p, r);
#pragma unroll
    for (int a = 0; a < DIM; a++) fvel[a] = r[a];
  }
  // grad[c][c2] = gfs_center_gradient (cell, c2, u[c]) (src/fluid.c:434-475; not yet divided by the size of the
  // leaf: Du/Dt divides the product with u[c2], vorticity_vector the difference)
  double grad[DIM][DIM];
#pragma unroll
  for (int c = 0; c < DIM; c++)
#pragma unroll
    for (int c2 = 0; c2 < DIM; c2++)
      grad[c][c2] = 0.;
  if (need.grad) {
    // (no unroll request on the loop over the rows: the stencil code holds loops over the children of a face, the
    // early unroll pass cannot take the loop around them and a later one does -- the build log shows no scratch,
    // DESIGN.md 11.28; spelling the rows out by hand sends the tables of the tree to scratch)
    for (int c = 0; c < DIM; c++) {
      DevValue uc = { P.u[c] };
#pragma unroll
      for (int c2 = 0; c2 < DIM; c2++)
	grad[c][c2] = tree::center_gradient (S.T, cell, c2, uc);
    }
  }
  const TreeGradient<DIM> G = { grad };
  if (need.dudt)
    inertial_force<DIM> (fluid_rho, dt, size, fvel, Value3 { fveln }, G, TreeCellU { P, c0.g }, dudt);
  particulate_forces<DIM, ONFLUID> (A, q, o, fluid_rho, ListViscosity { A }, size, G, fvel, dudt, vel, volume, mass, pf);
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
  const bool keep = tree_particle_bc<DIM> (S, P.side, c0, p, po);
#pragma unroll
  for (int a = 0; a < DIM; a++) {
    P.pos[a][q] = p[a];
    P.old[a][q] = po[a];
  }
  if (!keep)
    P.alive[q] = 0;
}

// key of the sort: the leaf that holds the particle (its index in the concatenated levels), dead or outside last
// (particle_keys_kernel, particles.hip, is this kernel on a box)
template <int DIM>
__global__ void __launch_bounds__(256)
tree_particle_keys_kernel (TreeSamp S, int n, const double * __restrict__ x, const double * __restrict__ y,
			   const double * __restrict__ z, const unsigned char * __restrict__ alive,
			   unsigned * __restrict__ key, unsigned * __restrict__ slot)
{
  const int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= n) return;
  unsigned k = 0xFFFFFFFFu;
  if (alive[q] == 1) {
    const double p[3] = { x[q], y[q], DIM == 3 ? z[q] : 0. };
    Leaf c;
    if (tree_locate<DIM> (S, p, c))
      k = (unsigned) c.g;
  }
  key[q] = k;
  slot[q] = q;
}

// ---------------------------------------------------------------------------------------------
// Two-way coupling on a tree (GfsParticulateField, GfsSourceParticulate): the records and the sort
// of coupling.hip and the serial sums of cell_sums.hpp on TreeCells -- the leaf of a tree, its index in the
// concatenated levels (Topo::gi), as the cell of a key, the cellvol of the leaf's own level -- and the pruned descent
// as a walk of the tree itself.
// ---------------------------------------------------------------------------------------------

// gfs_cell_reset on the interior leaves of every level, for up to three variables
__global__ void __launch_bounds__(256)
tree_reset_leaves_kernel (Topo T, const Cell * __restrict__ cells, int n, double * a0, double * a1, double * a2)
{
  const int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int g = T.gi (cells[t]);
  a0[g] = 0.;
  if (a1) a1[g] = 0.;
  if (a2) a2[g] = 0.;
}

// key of the leaf that holds each particle, (leaf << 32 | creation slot); pad (leaf = number of cells of the tree)
// for the particles that are off the list or have no leaf (:1949-1950)
// (field_keys_kernel, coupling.hip, is this kernel on a box)
template <int DIM>
__global__ void __launch_bounds__(256)
tree_field_keys_kernel (TreeSamp S, int n, const double * __restrict__ x, const double * __restrict__ y,
			const double * __restrict__ z, const unsigned char * __restrict__ alive,
			const unsigned * __restrict__ orig, unsigned long long pad, unsigned long long * __restrict__ key)
{
  const int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= n) return;
  unsigned long long k = pad;
  if (alive[q] == 1) {
    const double p[3] = { x[q], y[q], DIM == 3 ? z[q] : 0. };
    Leaf c;
    if (tree_locate<DIM> (S, p, c))
      k = (unsigned long long) c.g;
  }
  key[q] = k << 32 | orig[q];
}

// ---------------------------------------------------------------------------------------------
// GfsSourceParticulateVol / GfsSourceParticulateMass on a tree (modules/particulatecommon.c:2734-3047; DESIGN.md
// 11.32): the passes of particulate_sources.hip with the leaf of a tree as the cell.
// ---------------------------------------------------------------------------------------------

struct TreeSourceGatherArgs {
  int n;
  const double * pos[3];
  const unsigned char * alive;
  const unsigned * orig;
  const double * u[3], * vel[3], * volume;
  unsigned * cell;
  double * rad, * urel[3];
};

// update_vol / update_mass (:2806-2824, :2964-2982) up to the call of the function: gfs_domain_locate (pos, -1), the
// radius, gfs_interpolate of the velocity and the relative velocity of one particle, stored at its creation slot
// (particulate_source_gather_kernel, particles.hip, is this kernel on a box)
template <int DIM>
__global__ void __launch_bounds__(256)
tree_particulate_source_gather_kernel (TreeSamp S, TreeSourceGatherArgs A)
{
  const int q = blockIdx.x*blockDim.x + threadIdx.x;
  if (q >= A.n) return;
  const unsigned o = A.orig[q];
  const double p[3] = { A.pos[0][q], A.pos[1][q], DIM == 3 ? A.pos[2][q] : 0. };
  Leaf c;
  if (A.alive[q] != 1 || !tree_locate<DIM> (S, p, c)) {
    A.cell[o] = PSOURCE_NO_CELL;
    return;
  }
  A.cell[o] = (unsigned) c.g;
  A.rad[o] = pow (3.0*A.volume[o]/4.0/M_PI, 1./3.);      /* :2812, :2970, the device's pow */
  Vars<DIM> uu;
#pragma unroll
  for (int a = 0; a < DIM; a++) uu.p[a] = A.u[a];
  double fvel[DIM];
  tree_interpolate<DIM, DIM> (S, uu, c, p, fvel);
#pragma unroll
  for (int a = 0; a < DIM; a++)
    A.urel[a][o] = fvel[a] - A.vel[a][o];
}

// GfsFeedParticle on a list of a tree: feed_particulate (:2377-2393) for one candidate per thread,
// gfs_domain_locate (pos, -1) -- the leaf, whatever its level; no wrap of a periodic side -- then vel[c] =
// gfs_interpolate (cell, pos, u[c]) with the corner interpolators of the event kernels (vel.z = 0. in 2-D); the slot
// is that of a new object (pos_old = 0, force = 0) whose fate the ordered passes of feed_particle.hip decide
// (feed_gather_kernel, particles.hip, is this kernel on a box)
struct TreeFeedGatherArgs {
  int np, base;
  const double * cand;
  const double * u[3];
  double * pos[3], * old[3], * vel[3], * force[3];
  unsigned * orig, * cell;
};

template <int DIM>
__global__ void __launch_bounds__(256)
tree_feed_gather_kernel (TreeSamp S, TreeFeedGatherArgs A)
{
  const int i = blockIdx.x*blockDim.x + threadIdx.x;
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
  double vel[3] = { 0., 0., 0. };
  unsigned cell = PSOURCE_NO_CELL;
  /* the readers of a list of a quadtree take z = 0. for the walk of the tree: so does the candidate */
  const double q[3] = { p[0], p[1], DIM == 3 ? p[2] : 0. };
  Leaf c;
  if (tree_locate<DIM> (S, q, c)) {
    cell = (unsigned) c.g;
    Vars<DIM> uu;
#pragma unroll
    for (int a = 0; a < DIM; a++) uu.p[a] = A.u[a];
    double fvel[DIM];
    tree_interpolate<DIM, DIM> (S, uu, c, q, fvel);
#pragma unroll
    for (int a = 0; a < DIM; a++) vel[a] = fvel[a];
  }
  A.cell[i] = cell;
#pragma unroll
  for (int a = 0; a < 3; a++)
    A.vel[a][s] = vel[a];
}

// gfs_cell_reset with max_depth = 1 (:2844, :3004): the few interior cells of levels 0 and 1 the traversal reaches
struct TreeSourceResetCells { int n, g[9]; };

__global__ void __launch_bounds__(64)
tree_particulate_source_reset_kernel (TreeSourceResetCells C, double * __restrict__ a)
{
  const int t = threadIdx.x;
#pragma unroll
  for (int m = 0; m < 9; m++)
    if (t == m && m < C.n) a[C.g[m]] = 0.;
}

struct TreeSpreadArgs {
  int o0, nchunk, stride;
  double rkernel;
  const unsigned * where;
  const unsigned char * alive;
  const double * pos[3];
  const double * rb;
  unsigned long long pad;       // key of an unused slot: leaf = number of cells of the tree
  unsigned long long * key;
  double * q[3];
  int * cnt, * flag;
};

// step 1: the leaves the kernel of each particle of the chunk reaches, in traversal order.
// ftt_cell_traverse_condition (src/ftt.c:948-986), FTT_PRE_ORDER, FTT_TRAVERSE_LEAFS, over the tree itself: the root
// passes cond_kernel or nothing is visited; a cell that passes is visited if it is a leaf and sends the descent into
// its children 0 .. FTT_CELLS - 1 otherwise.  The state of the walk is the cell at hand (level, integer coordinates
// from the low corner) and the next child to try: the child id of a cell is in the low bits of its coordinates
// (bit 0: +x, bit 1: -y, bit 2: -z), so going up continues with id + 1 -- no stack
template <int DIM>
__global__ void __launch_bounds__(256)
tree_spread_emit_kernel (TreeSamp S, TreeSpreadArgs A)
{
  const int t = blockIdx.x*blockDim.x + threadIdx.x;
  if (t >= A.nchunk) return;
  const Topo & T = S.T;
  const unsigned o = (unsigned) (A.o0 + t);
  const unsigned s = A.where[o];
  const size_t base = (size_t) t*A.stride;
  int cnt = 0;
  if (A.alive[s] == 1) {
    const double p[3] = { A.pos[0][s], A.pos[1][s], DIM == 3 ? A.pos[2][s] : 0. };
    const double rb = A.rb[o];
    auto index = [&] (int l, int x, int y, int z) -> int {
      const int r = (1 << l) + 2;
      return T.off[l] + (x + 1) + r*((y + 1) + (DIM == 3 ? r*(z + 1) : 0));
    };
    auto visit = [&] (int l, int x, int y, int z, int g) {
      if (cnt < A.stride) {
	const double cellsize = 1./(double) (1 << l);
	A.key[base + cnt] = (unsigned long long) g << 32 | o;
	// distance_normalization (:2089-2099).  In 3-D the line `pos1->z = 0.' comes before
	// `pos1->z = (pos1->z - pos2->z)/rb': z is (0. - pos.z)/rb, whatever the cell
	A.q[0][base + cnt] = (-0.5 + (x + 0.5)*cellsize - p[0])/rb;
	A.q[1][base + cnt] = (-0.5 + (y + 0.5)*cellsize - p[1])/rb;
	A.q[2][base + cnt] = DIM == 3 ? (0. - p[2])/rb : 0.;
      }
      cnt++;
    };
    int l = 0, x = 0, y = 0, z = 0;      /* the cell whose children are tried */
    const int root[3] = { 0, 0, 0 };
    if (cond_kernel<DIM> (0, root, p, A.rkernel)) {
      const int g0 = index (0, 0, 0, 0);
      if (T.depth == 0 || T.cmask[g0] == 0)
	visit (0, 0, 0, 0, g0);
      else {
	int n = 0;                       /* the next child of (l, x, y, z) to try */
	unsigned mask = T.cmask[g0];     /* its children */
	for (;;) {
	  if (n == (1 << DIM)) {         /* all children done: up, and on with the next brother */
	    if (l == 0) break;
	    n = ((x & 1) | ((y & 1) ? 0 : 2) | (DIM == 3 && !(z & 1) ? 4 : 0)) + 1;
	    x >>= 1; y >>= 1; z >>= 1;
	    l--;
	    mask = T.cmask[index (l, x, y, z)];
	    continue;
	  }
	  const int k = n++;
	  if (!((mask >> k) & 1u))
	    continue;
	  const int cx[3] = { 2*x + (k & 1), 2*y + ((k & 2) ? 0 : 1), DIM == 3 ? 2*z + ((k & 4) ? 0 : 1) : 0 };
	  if (!cond_kernel<DIM> (l + 1, cx, p, A.rkernel))
	    continue;
	  const int g = index (l + 1, cx[0], cx[1], cx[2]);
	  const unsigned cm = l + 1 < T.depth ? T.cmask[g] : 0u;
	  if (cm == 0)
	    visit (l + 1, cx[0], cx[1], cx[2], g);
	  else {
	    l++;
	    x = cx[0]; y = cx[1]; z = cx[2];
	    n = 0;
	    mask = cm;
	  }
	}
      }
    }
  }
  if (cnt > A.stride) {      /* cannot happen (tree_kernel_stride); reported, never written */
    *A.flag = 1;
    cnt = A.stride;
  }
  A.cnt[t] = cnt;
  for (int j = cnt; j < A.stride; j++)
    A.key[base + j] = A.pad << 32 | 0xFFFFFFFFull;
}

TreeSamp tree_samp (const TreeView & V, const SamplerTables * S)
{
  TreeSamp A;
  A.T = V.D;
  A.corner_bits = S->corner_bits;
  A.row_base = S->row_base; A.row_ptr = S->row_ptr; A.col = S->col;
  A.w = S->w;
  return A;
}

// u[c] = the array of GFSHIP_TREE_U, _V, _W of the tree for c < dim
void tree_velocity (gfship_tree * tr, int dim, const double * (& u)[3])
{
  const int uvar[3] = { GFSHIP_TREE_U, GFSHIP_TREE_V, GFSHIP_TREE_W };
  for (int c = 0; c < 3; c++)
    u[c] = c < dim ? tree_variable (tr, uvar[c]) : nullptr;
}

// the leaves of a refined tree as the mesh of a list (particle_events.hpp)
struct TreeMesh {
  static constexpr bool TREE = true;
  gfship_particles * pl;
  TreeView V;
  SamplerTables * S = nullptr;
  int dim = 0;
  hipStream_t stream = nullptr;
  double t = 0., dt = 0.;
  unsigned long long ncell = 0;
  explicit TreeMesh (gfship_particles * p) : pl (p) {}
  // the view of the tree; sampler: also the tables its kernels read, on the device of the tree
  int init (bool sampler = true) {
    if (sampler) {
      int r = sampler_get (pl->tree, &V, &S);
      if (r) return r;
    }
    else
      tree_view (pl->tree, &V);
    dim = V.H.dim; stream = V.stream; t = V.t; dt = V.dt; ncell = (unsigned long long) V.ncell;
    return GFSHIP_OK;
  }
  template <int DIM> TreeCells<DIM> cells () const { return TreeCells<DIM> { V.D }; }
  const double * alpha () const { return nullptr; }      /* a tree has no alpha */
  // gfs_cell_reset on the interior leaves of every level, for up to three variables
  int reset_leaves (double * a0, double * a1 = nullptr, double * a2 = nullptr) const {
    const int block = 256;
    hipLaunchKernelGGL (tree_reset_leaves_kernel, dim3 ((V.nleaves + block - 1)/block), dim3 (block), 0, stream, V.D,
			V.dleaves, V.nleaves, a0, a1, a2);
    GFSHIP_HIP (hipGetLastError ());
    return GFSHIP_OK;
  }
  // feed: the variables a function of a GfsFeedParticle may read (tree_feed_variable)
  int arrays (const std::vector<gfship_field> & vars, std::vector<const double *> & out, bool feed = false) const {
    for (int var : vars) {
      const double * a = !feed || tree_feed_variable (pl, var) ? tree_variable (pl->tree, var) : nullptr;
      GFSHIP_CHECK (a != nullptr, GFSHIP_EINVAL, "the tree has no variable %d", var);
      out.push_back (a);
    }
    return GFSHIP_OK;
  }
  int compile_spatial (const char * text, RtcKernel ** k) const {
    GFSHIP_HIP (hipSetDevice (V.device));
    return rtc_compile_spatial_on (V.device, text, k);
  }
  int launch_source (const gfship_particulate_source * s, const std::vector<const double *> & read) const {
    return rtc_launch_tree_source (s->fn, stream, pl->n, dim, V.H.depth, V.H.off, s->cell, s->prad, s->purel, t,
				   (int) read.size (), read.data (), s->src);
  }
  int launch_cell (RtcKernel * k, int np, const unsigned * cell, const std::vector<const double *> & read,
		   double * out) const {
    return rtc_launch_tree_cell (k, stream, np, V.H.depth, V.H.off, cell, t, (int) read.size (), read.data (), out);
  }

  // record slots per particle: the bound of BoxMesh::kernel_stride (coupling.hip) per level -- the centres of the
  // leaves of level l that pass cond_kernel lie within rho_l = rkernel + (h_l/2) sqrt (dim) of the particle along every
  // axis and are h_l apart -- summed over the levels that hold interior leaves; on a uniform tree the stride of the box
  unsigned long long kernel_stride (double rkernel) const {
    bool has[GFSHIP_MAXLEVEL + 1] = {};
    for (int t = 0; t < V.nleaves; t++) has[V.hleaves[t].l] = true;
    unsigned long long sum = 0;
    for (int l = 0; l <= V.H.depth; l++)
      if (has[l]) {
	const double n = (double) (1 << l), h = 1./n;
	const double rho = rkernel + h/2.*sqrt ((double) V.H.dim);
	double m = floor (2.*rho/h) + 2.;
	if (!(m < n)) m = n;
	const unsigned long long s = (unsigned long long) m;
	sum += V.H.dim == 3 ? s*s*s : s*s;
	if (sum > COUPLING_RECORD_CAP) break;      /* refused by stride_check: no need to go on (nor to overflow) */
      }
    return sum;
  }
  int stride_check (double rkernel) const {
    const unsigned long long stride = kernel_stride (rkernel);
    GFSHIP_CHECK (stride <= COUPLING_RECORD_CAP, GFSHIP_EUNSUPPORTED,
		  "GfsSourceParticulate: a kernel of rkernel = %g may reach %llu leaves of this tree or more, more than "
		  "the %llu records of a chunk", rkernel, stride, (unsigned long long) COUPLING_RECORD_CAP);
    return GFSHIP_OK;
  }

  int field_keys (unsigned long long * key) const {
    const int block = 256, grid = (pl->n + block - 1)/block;
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      hipLaunchKernelGGL (tree_field_keys_kernel<DIM>, dim3 (grid), dim3 (block), 0, stream, tree_samp (V, S), pl->n,
			  pl->pos[0], pl->pos[1], pl->pos[2], pl->alive, pl->orig, ncell, key);
    }, dim == 3);
    GFSHIP_HIP (hipGetLastError ());
    return GFSHIP_OK;
  }
  int spread_emit (int o0, int nchunk, int stride) const {
    TreeSpreadArgs A;
    A.o0 = o0; A.nchunk = nchunk; A.stride = stride; A.rkernel = pl->rkernel;
    A.where = pl->where; A.alive = pl->alive; A.rb = pl->rb;
    for (int c = 0; c < 3; c++) { A.pos[c] = pl->pos[c]; A.q[c] = pl->cq[c]; }
    A.pad = ncell; A.key = pl->ckey; A.cnt = pl->ccnt; A.flag = pl->cflag;
    const int block = 256;
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      hipLaunchKernelGGL (tree_spread_emit_kernel<DIM>, dim3 ((nchunk + block - 1)/block), dim3 (block), 0, stream,
			  tree_samp (V, S), A);
    }, dim == 3);
    GFSHIP_HIP (hipGetLastError ());
    return GFSHIP_OK;
  }
  int source_gather (gfship_particulate_source * s) const {
    TreeSourceGatherArgs G;
    G.n = pl->n;
    tree_velocity (pl->tree, dim, G.u);
    for (int c = 0; c < 3; c++) {
      G.pos[c] = pl->pos[c];
      G.vel[c] = pl->vel[c];
      G.urel[c] = s->purel[c];
    }
    G.alive = pl->alive; G.orig = pl->orig; G.volume = pl->volume;
    G.cell = s->cell; G.rad = s->prad;
    const int block = 256, grid = (pl->n + block - 1)/block;
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      hipLaunchKernelGGL (tree_particulate_source_gather_kernel<DIM>, dim3 (grid), dim3 (block), 0, stream,
			  tree_samp (V, S), G);
    }, dim == 3);
    GFSHIP_HIP (hipGetLastError ());
    return GFSHIP_OK;
  }
  int feed_gather (int base, int np, const double * cand, unsigned * cell) const {
    TreeFeedGatherArgs A;
    A.np = np; A.base = base;
    A.cand = cand;
    tree_velocity (pl->tree, dim, A.u);
    for (int c = 0; c < 3; c++) {
      A.pos[c] = pl->pos[c]; A.old[c] = pl->old[c];
      A.vel[c] = pl->vel[c]; A.force[c] = pl->force[c];
    }
    A.orig = pl->orig; A.cell = cell;
    const int block = 256, grid = (np + block - 1)/block;
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      hipLaunchKernelGGL (tree_feed_gather_kernel<DIM>, dim3 (grid), dim3 (block), 0, stream, tree_samp (V, S), A);
    }, dim == 3);
    GFSHIP_HIP (hipGetLastError ());
    return GFSHIP_OK;
  }
};

} // namespace

// does the tree have the variable `var' for a function to read at a leaf?  tree_has_variable, but not the variables
// of an octree alone on a quadtree: the arrays of W, its gradients and its face values are allocated there too, and
// nothing ever writes them
bool tree_feed_variable (gfship_particles * pl, int var)
{
  static const int octree_only[] = { GFSHIP_TREE_W, GFSHIP_TREE_GZ, GFSHIP_TREE_GMACZ, GFSHIP_TREE_UN4, GFSHIP_TREE_UN5,
				     GFSHIP_TREE_BCW, GFSHIP_TREE_WPREV, GFSHIP_TREE_FZ, GFSHIP_TREE_WRELP };
  if (pl->dim == 2)
    for (int v : octree_only)
      if (var == v) return false;
  return tree_has_variable (pl->tree, var);
}

int tree_particle_list_event (gfship_particles * pl)
{
  TreeView V;
  SamplerTables * S;
  int r = sampler_get (pl->tree, &V, &S);
  if (r) return r;
  TreePartArgs A;
  for (int d = 0; d < 6; d++) A.side[d] = d < 2*V.H.dim ? V.side[d] : GFSHIP_SIDE_PERIODIC;
  A.n = pl->n;
  tree_velocity (pl->tree, V.H.dim, A.u);
  for (int c = 0; c < 3; c++) {
    A.pos[c] = pl->pos[c];
    A.old[c] = pl->old[c];
  }
  A.alive = pl->alive;
  A.dt = V.dt;
  const int block = 256, grid = (pl->n + block - 1)/block;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (tree_particle_list_event_kernel<DIM>, dim3 (grid), dim3 (block), 0, V.stream, tree_samp (V, S), A);
  }, V.H.dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  return GFSHIP_OK;
}

// gfs_particle_list_event (modules/particulatecommon.c:980-1015) of a list of GfsParticulate with forces;
// onfluid: the forces on the fluid alone (tree_particulate_list_event_kernel <ONFLUID>), Un, Vn, Wn stay
static int tree_particulate_event (gfship_particles * pl, bool onfluid)
{
  TreeView V;
  SamplerTables * S;
  int r = sampler_get (pl->tree, &V, &S);
  if (r) return r;
  const int dim = V.H.dim;
  TreeParticulateArgs A;
  TreePartArgs & P = A.P;
  for (int d = 0; d < 6; d++) P.side[d] = d < 2*dim ? V.side[d] : GFSHIP_SIDE_PERIODIC;
  P.n = pl->n;
  tree_velocity (pl->tree, dim, P.u);
  for (int c = 0; c < 3; c++) {
    P.pos[c] = pl->pos[c];
    P.old[c] = pl->old[c];
    A.uold[c] = c < dim ? V.uprev[c] : nullptr;
  }
  P.alive = pl->alive;
  P.dt = V.dt;
  particulate_force_args (pl, A);
  bool reads_un = false;
  for (int f = 0; f < pl->nforces; f++)
    if (pl->forces[f] == GFSHIP_FORCE_INERTIAL || pl->forces[f] == GFSHIP_FORCE_ADDEDMASS)
      reads_un = true;
  GFSHIP_CHECK (!reads_un || V.uprev[0], GFSHIP_EINVAL, "the tree has no Un, Vn, Wn (gfship_particles_set_forces)");
  A.viscosity = V.viscosity;
  const int block = 256, grid = (pl->n + block - 1)/block;
  const TreeSamp TS = tree_samp (V, S);
  r = particulate_coefficients (pl, A, V.stream, V.t, [&] {
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      hipLaunchKernelGGL (tree_particulate_coeff_inputs_kernel<DIM>, dim3 (grid), dim3 (block), 0, V.stream, TS, A);
    }, dim == 3);
  });
  if (r) return r;
  if (onfluid) {
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      hipLaunchKernelGGL ((tree_particulate_list_event_kernel<DIM, true>), dim3 (grid), dim3 (block), 0, V.stream, TS, A);
    }, dim == 3);
    GFSHIP_HIP (hipGetLastError ());
    return GFSHIP_OK;
  }
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (tree_particulate_list_event_kernel<DIM>, dim3 (grid), dim3 (block), 0, V.stream, TS, A);
  }, dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  // the velocity of this step for the inertial force of the next one (:1003-1012: only for GfsForceInertial objects)
  for (int f = 0; f < pl->nforces; f++)
    if (pl->forces[f] == GFSHIP_FORCE_INERTIAL)
      return tree_previous_vel (pl->tree);
  return GFSHIP_OK;
}

int tree_particulate_list_event (gfship_particles * pl) { return tree_particulate_event (pl, false); }

int tree_particle_keys (gfship_particles * pl, int * bits)
{
  TreeView V;
  SamplerTables * S;
  int r = sampler_get (pl->tree, &V, &S);
  if (r) return r;
  const int block = 256, grid = (pl->n + block - 1)/block;
  with_bools ([&] (auto D3) {
    constexpr int DIM = decltype (D3)::value ? 3 : 2;
    hipLaunchKernelGGL (tree_particle_keys_kernel<DIM>, dim3 (grid), dim3 (block), 0, V.stream, tree_samp (V, S), pl->n,
			pl->pos[0], pl->pos[1], pl->pos[2], pl->alive, pl->key, pl->slot);
  }, V.H.dim == 3);
  GFSHIP_HIP (hipGetLastError ());
  /* the bits of a cell index (+1 so that the all-ones key of the dead sorts last) */
  int b = 0;
  while (b < 31 && (V.ncell >> b)) b++;
  *bits = b + 1;
  return GFSHIP_OK;
}

// gfship_feed_particle_event on a list of particulates of a tree
int tree_feed_event (gfship_feed_particle * f, int np, const double * pos)
{
  gfship_particles * pl = f->pl;
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_feed_particle_event");
  if (np == 0) return GFSHIP_OK;
  TreeMesh M (pl);
  int r = M.init ();
  if (r) return r;
  return feed_event_body (M, f, np, pos);
}

// source_particulatevol_event (:2834-2852) / source_particulatemass_event (:2993-3012) on a list of a tree
int tree_particulate_source_event (gfship_particulate_source * s, double * info)
{
  gfship_particles * pl = s->pl;
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_particulate_source_event");
  TreeMesh M (pl);
  int r = M.init ();
  if (r) return r;
  const TreeView & V = M.V;
  const int dim = V.H.dim;
  const bool volume = s->kind == GFSHIP_PARTICULATE_SOURCE_VOLUME;
  double * D = nullptr, * R = nullptr, * U[3] = { nullptr, nullptr, nullptr };
  if (s->deposit >= 0 && (r = tree_source_variable (pl->tree, s->deposit, &D))) return r;
  if (s->rad >= 0 && (r = tree_source_variable (pl->tree, s->rad, &R))) return r;
  for (int c = 0; c < dim; c++)
    if (s->urel[c] >= 0 && (r = tree_source_variable (pl->tree, s->urel[c], &U[c]))) return r;
  std::vector<const double *> read;
  if ((r = M.arrays (s->read, read))) return r;
  if (D) {
    /* gfs_domain_cell_traverse (..., FTT_TRAVERSE_ALL | FTT_TRAVERSE_LEAFS, 1, gfs_cell_reset): the interior cells of
       levels 0 and 1 for a volume, the leaves among them for a mass; every deeper cell keeps what it holds */
    TreeSourceResetCells C;
    C.n = 0;
    for (int l = 0; l <= 1 && l <= V.H.depth; l++)
      for (int k = 1; k <= (dim == 3 ? V.H.n (l) : 1); k++)
	for (int j = 1; j <= V.H.n (l); j++)
	  for (int i = 1; i <= V.H.n (l); i++) {
	    const Cell c = V.H.make (l, i, j, k);
	    if (exists (c) && (volume || V.H.leaf (c)))
	      C.g[C.n++] = V.H.gi (c);
	  }
    if (C.n > 0) {
      hipLaunchKernelGGL (tree_particulate_source_reset_kernel, dim3 (1), dim3 (64), 0, V.stream, C, D);
      GFSHIP_HIP (hipGetLastError ());
    }
  }
  return source_event_body (M, s, D, R, U, read, info);
}

} // namespace gfship

using namespace gfship;

extern "C" {

int gfship_tree_interpolate (gfship_tree * tr, int var, int np, const double * pos, double * out,
			     unsigned char * inside)
{
  GFSHIP_CHECK (tr && pos && out && inside && np >= 0, GFSHIP_EINVAL, "invalid argument");
  const double * v = tree_variable (tr, var);
  GFSHIP_CHECK (v != nullptr, GFSHIP_EINVAL, "gfship_tree_interpolate: %d is not a variable of a tree", var);
  if (np == 0) return GFSHIP_OK;
  TreeView V;
  SamplerTables * S;
  int r = sampler_get (tr, &V, &S);
  if (r) return r;
  double * dpos = nullptr, * dout = nullptr;
  unsigned char * din = nullptr;
  GFSHIP_HIP (hipMalloc ((void **) &dpos, 3*(size_t) np*sizeof (double)));
  GFSHIP_HIP (hipMalloc ((void **) &dout, (size_t) np*sizeof (double)));
  GFSHIP_HIP (hipMalloc ((void **) &din, (size_t) np));
  hipError_t e = hipMemcpyAsync (dpos, pos, 3*(size_t) np*sizeof (double), hipMemcpyHostToDevice, V.stream);
  if (e == hipSuccess) {
    const int block = 256, grid = (np + block - 1)/block;
    with_bools ([&] (auto D3) {
      constexpr int DIM = decltype (D3)::value ? 3 : 2;
      hipLaunchKernelGGL (tree_sample_kernel<DIM>, dim3 (grid), dim3 (block), 0, V.stream, tree_samp (V, S), np, dpos, v,
			  dout, din);
    }, V.H.dim == 3);
    e = hipGetLastError ();
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync (out, dout, (size_t) np*sizeof (double), hipMemcpyDeviceToHost, V.stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync (inside, din, (size_t) np, hipMemcpyDeviceToHost, V.stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize (V.stream);
  if (e != hipSuccess)
    r = hip_fail (e, "gfship_tree_interpolate", __FILE__, __LINE__);
  (void) hipFree (dpos); (void) hipFree (dout); (void) hipFree (din);
  return r;
}

int gfship_tree_sampler_stats (gfship_tree * tr, long long stats[5])
{
  GFSHIP_CHECK (tr && stats, GFSHIP_EINVAL, "invalid argument");
  TreeView V;
  SamplerTables * S;
  int r = sampler_get (tr, &V, &S);
  if (r) return r;
  for (int k = 0; k < 5; k++) stats[k] = S->stats[k];
  return GFSHIP_OK;
}

int gfship_particles_create_tree (gfship_particles ** out, gfship_tree * tr, int np, const double * pos,
				  const unsigned * id)
{
  GFSHIP_CHECK (out && tr && (np == 0 || (pos && id)) && np >= 0, GFSHIP_EINVAL, "invalid argument");
  *out = nullptr;
  TreeView V;
  SamplerTables * S;
  int r = sampler_get (tr, &V, &S);
  if (r) return r;
  gfship_particles * pl = new gfship_particles;
  pl->tree = tr;
  pl->stream = V.stream;
  pl->dim = V.H.dim;
  r = particles_alloc (pl, np, pos, id);
  if (r) {
    gfship_particles_destroy (pl);
    return r;
  }
  *out = pl;
  return GFSHIP_OK;
}

// a GfsParticleList of GfsParticulate on a tree: modules/particulatecommon.c:1022-1093 with the members of
// GfsParticulate (modules/particulatecommon.h:35-48; gfs_particulate_read, :844-905)
int gfship_particulates_create_tree (gfship_particles ** out, gfship_tree * tr, int np, const double * pos,
				     const unsigned * id, const double * vel, const double * mass, const double * volume)
{
  GFSHIP_CHECK (out != nullptr, GFSHIP_EINVAL, "invalid argument");
  *out = nullptr;
  GFSHIP_CHECK (tr && np >= 0 && (np == 0 || (pos && id && vel && mass && volume)), GFSHIP_EINVAL, "invalid argument");
  gfship_particles * pl = nullptr;
  int r = gfship_particles_create_tree (&pl, tr, np, pos, id);
  if (r) return r;
  const double none[3] = { 0., 0., 0. };
  r = particulate_alloc (pl, np ? vel : none, np ? mass : none, np ? volume : none);
  if (r) {
    gfship_particles_destroy (pl);
    return r;
  }
  *out = pl;
  return GFSHIP_OK;
}

// ---- two-way coupling on a tree --------------------------------------------------------------------

// GfsParticulateField: particulate_field_event, modules/particulatecommon.c:1934-1957
int gfship_tree_particulate_field (gfship_particles * pl, int var)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_tree_particulate_field");
  GFSHIP_CHECK (var == GFSHIP_TREE_VF, GFSHIP_EINVAL, "the variable of a GfsParticulateField is GFSHIP_TREE_VF");
  TreeMesh M (pl);
  int r = M.init ();
  if (r) return r;
  double * a = nullptr;
  if ((r = tree_coupling_variable (pl->tree, var, &a))) return r;
  /* gfs_cell_reset on the leaves (:1944-1945) */
  if ((r = M.reset_leaves (a))) return r;
  return particulate_field_body (M, pl, a);
}

// the forces of source_particulate_event (:2199-2206)
int gfship_tree_particles_forces_on_fluid (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_tree_particles_forces_on_fluid");
  if (pl->n == 0) return GFSHIP_OK;
  return tree_particulate_event (pl, true);
}

// rkernel and kernel of a GfsSourceParticulate (source_particulate_read, :2271-2289)
int gfship_tree_particles_set_kernel (gfship_particles * pl, double rkernel, const char * function)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_tree_particles_set_kernel");
  TreeMesh M (pl);
  M.init (false);
  return set_kernel_body (M, pl, rkernel, function);
}

// source_particulate_event from the stored forces (:2208-2222) into GFSHIP_TREE_FX ...
int gfship_tree_particles_spread_forces (gfship_particles * pl)
{
  GFSHIP_CHECK (pl != nullptr, GFSHIP_EINVAL, "null particle list");
  GFSHIP_TREE_PARTICULATES_ONLY (pl, "gfship_tree_particles_spread_forces");
  TreeMesh M (pl);
  int r = M.init ();
  if (r) return r;
  double * Fa[3] = { nullptr, nullptr, nullptr };
  for (int c = 0; c < M.dim; c++)
    if ((r = tree_coupling_variable (pl->tree, GFSHIP_TREE_FX + c, &Fa[c]))) return r;
  /* gfs_cell_reset on the leaves (:2189-2191) */
  if ((r = M.reset_leaves (Fa[0], Fa[1], Fa[2]))) return r;
  return spread_forces_body (M, pl, Fa, nullptr);
}

// source_particulate_event, :2177-2228
int gfship_tree_source_particulate_event (gfship_particles * pl)
{
  int r = gfship_tree_particles_forces_on_fluid (pl);
  if (r) return r;
  return gfship_tree_particles_spread_forces (pl);
}

} // extern "C"
