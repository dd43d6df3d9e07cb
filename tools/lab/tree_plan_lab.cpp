// tree_plan_lab.cpp -- the planner of refined trees (csrc/tree_plan.hip) on its own, without the rest of the
// library and without a device: it makes no HIP call, so this program links nothing but tree_plan.hip.
// A place to run the planner under a host tool (a sanitizer, a profiler, a debugger).
//
//   hipcc -O2 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -Iinclude -Igerris-fft-particles_amd/csrc \
//         gerris-fft-particles_amd/csrc/tree_plan.hip tools/lab/tree_plan_lab.cpp -o tools/lab/tree_plan_lab
//
// It builds the quadtree 4/6 and the octree 3/4, periodic and with GfsBoundary sides, plans loops of 4 and 40
// sweeps (the digests of gfship_tree_host_plan_digest) and runs both host checks; exit status 1 if a check fails.
#include "gfship.h"
#include <cstdarg>
#include <cstdio>

namespace gfship {
// the library's error text (domain.hip), here on stderr
void set_error (const char * fmt, ...)
{
  va_list ap;
  va_start (ap, fmt);
  vfprintf (stderr, fmt, ap);
  va_end (ap);
  fputc ('\n', stderr);
}
}

static bool inside (double x, double y, double z) { return x >= -0.25 && x <= 0.25 && y >= -0.25 && y <= 0.25 && z >= -0.25 && z <= 0.25; }
static double quadtree (double x, double y, double, void *) { return inside (x, y, 0.) ? 6 : 4; }
static double octree (double x, double y, double z, void *) { return inside (x, y, z) ? 4 : 3; }

int main ()
{
  const int walls[6] = { GFSHIP_SIDE_BOUNDARY, GFSHIP_SIDE_BOUNDARY, GFSHIP_SIDE_BOUNDARY, GFSHIP_SIDE_BOUNDARY,
			 GFSHIP_SIDE_BOUNDARY, GFSHIP_SIDE_BOUNDARY };
  int bad = 0;
  for (int dim = 2; dim <= 3; dim++)
    for (const int * side : { (const int *) nullptr, walls })
      for (unsigned nrelax : { 4u, 40u }) {
	gfship_refine_fn refine = dim == 2 ? quadtree : octree;
	unsigned long long dig[5];
	long long st[4], sd[6];
	int e = gfship_tree_host_plan_digest (dim, refine, nullptr, side, nrelax, dig);
	if (!e) e = gfship_tree_host_check (dim, refine, nullptr, side, nrelax, st);
	if (!e) e = gfship_tree_host_check_diffusion (dim, refine, nullptr, side, nrelax, 0.37, sd);
	if (e) { printf ("dim %d: error %d\n", dim, e); bad = 1; continue; }
	printf ("dim %d, %s, %2u sweeps: digests %016llx %016llx %016llx %016llx %016llx; %lld updates, %lld values differ; "
		"diffusion: %lld differ, %lld hazards, %lld levels without a flow plan\n", dim, side ? "walls   " : "periodic",
		nrelax, dig[0], dig[1], dig[2], dig[3], dig[4], st[0], st[3], sd[3], sd[4], sd[5]);
	if (st[0] <= 0 || st[3] || sd[3] || sd[4] || sd[5]) bad = 1;
      }
  return bad;
}
