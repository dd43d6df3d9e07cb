// rtc.hip -- GfsFunction objects of the particle forces on the device.
//
// A GfsForceCoeff of the reference may carry a GfsFunction (modules/particulatecommon.c:166-210): C
// text of the simulation file -- an expression or a { block } with a return -- that gerris compiles
// with the host compiler and calls per particle with the variables Rep, Urelp, Vrelp, Wrelp, Pdia
// set in the particle's cell (:378-384,478-485,566-573).  Here the same text is compiled for the
// GPU the domain lives on with hipRTC (the runtime-compilation library of ROCm, opened with dlopen:
// a run without such functions never loads it) into a kernel that evaluates the function for every
// particle of the list; the event kernel then reads the coefficients from an array.  Same C
// arithmetic (-ffp-contract=off); the device's libm (pow, exp ...) in place of glibc's.
#include "gfship_internal.hpp"
#include <hip/hiprtc.h>
#include <dlfcn.h>
#include <string>
#include <vector>

namespace gfship {

struct RtcApi {
  void * handle = nullptr;
  hiprtcResult (* CreateProgram) (hiprtcProgram *, const char *, const char *, int, const char **,
				  const char **) = nullptr;
  hiprtcResult (* CompileProgram) (hiprtcProgram, int, const char **) = nullptr;
  hiprtcResult (* GetProgramLogSize) (hiprtcProgram, size_t *) = nullptr;
  hiprtcResult (* GetProgramLog) (hiprtcProgram, char *) = nullptr;
  hiprtcResult (* GetCodeSize) (hiprtcProgram, size_t *) = nullptr;
  hiprtcResult (* GetCode) (hiprtcProgram, char *) = nullptr;
  hiprtcResult (* DestroyProgram) (hiprtcProgram *) = nullptr;
  const char * (* GetErrorString) (hiprtcResult) = nullptr;
};

static RtcApi g_rtc;

static int rtc_load ()
{
  if (g_rtc.handle) return GFSHIP_OK;
  const char * names[] = { "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so", "libhiprtc.so.7" };
  void * h = nullptr;
  for (const char * nm : names)
    if ((h = dlopen (nm, RTLD_NOW | RTLD_GLOBAL)))
      break;
  GFSHIP_CHECK (h != nullptr, GFSHIP_EUNSUPPORTED,
		"a GfsFunction of a particle force needs hipRTC: cannot open libhiprtc.so: %s", dlerror ());
#define SYM(field, name) do { \
    *(void **) &g_rtc.field = dlsym (h, name); \
    GFSHIP_CHECK (g_rtc.field != nullptr, GFSHIP_EUNSUPPORTED, "libhiprtc: no symbol %s", name); \
  } while (0)
  SYM (CreateProgram, "hiprtcCreateProgram");
  SYM (CompileProgram, "hiprtcCompileProgram");
  SYM (GetProgramLogSize, "hiprtcGetProgramLogSize");
  SYM (GetProgramLog, "hiprtcGetProgramLog");
  SYM (GetCodeSize, "hiprtcGetCodeSize");
  SYM (GetCode, "hiprtcGetCode");
  SYM (DestroyProgram, "hiprtcDestroyProgram");
  SYM (GetErrorString, "hiprtcGetErrorString");
#undef SYM
  g_rtc.handle = h;
  return GFSHIP_OK;
}

struct RtcKernel {
  hipModule_t mod = nullptr;
  hipFunction_t fn = nullptr;
};

void rtc_free (RtcKernel * k)
{
  if (!k) return;
  if (k->mod) (void) hipModuleUnload (k->mod);
  delete k;
}

// the text of a GfsFunction -- an expression or a { block } with a return -- as the body of the device
// function whose head is `signature', followed by the kernel `kernel_src' that calls it; compiled for the
// GPU `device' (that of the domain, or of the tree), `entry' is the kernel's name
static int rtc_compile (int device, const char * text, const char * signature,
			const char * kernel_src, const char * entry, RtcKernel ** out)
{
  GFSHIP_CHECK (text && out, GFSHIP_EINVAL, "null argument");
  *out = nullptr;
  int r = rtc_load ();
  if (r) return r;
  std::string t (text);
  size_t a = t.find_first_not_of (" \t\n\r"), b = t.find_last_not_of (" \t\n\r");
  GFSHIP_CHECK (a != std::string::npos, GFSHIP_EINVAL, "empty function");
  t = t.substr (a, b - a + 1);
  const bool block = t[0] == '{';
  std::string src = "#ifndef M_PI\n#define M_PI 3.14159265358979323846\n#endif\n";
  src += signature;
  if (block)
    src += t + "\n";
  else
    src += "{ return (" + t + "); }\n";
  src += kernel_src;
  hipDeviceProp_t prop;
  GFSHIP_HIP (hipGetDeviceProperties (&prop, device));
  const std::string arch = std::string ("--offload-arch=") + prop.gcnArchName;
  const char * opts[] = { arch.c_str (), "-ffp-contract=off", "-fno-fast-math", "-O2" };
  hiprtcProgram prog;
  hiprtcResult e = g_rtc.CreateProgram (&prog, src.c_str (), "gfs_function.hip", 0, nullptr, nullptr);
  GFSHIP_CHECK (e == HIPRTC_SUCCESS, GFSHIP_EHIP, "hiprtcCreateProgram: %s", g_rtc.GetErrorString (e));
  e = g_rtc.CompileProgram (prog, 4, opts);
  if (e != HIPRTC_SUCCESS) {
    size_t ls = 0;
    std::string log;
    if (g_rtc.GetProgramLogSize (prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
      log.resize (ls);
      (void) g_rtc.GetProgramLog (prog, &log[0]);
    }
    (void) g_rtc.DestroyProgram (&prog);
    set_error ("the function `%s' does not compile for the device:\n%s", text, log.c_str ());
    return GFSHIP_EINVAL;
  }
  size_t cs = 0;
  e = g_rtc.GetCodeSize (prog, &cs);
  std::vector<char> code (cs);
  if (e == HIPRTC_SUCCESS) e = g_rtc.GetCode (prog, code.data ());
  (void) g_rtc.DestroyProgram (&prog);
  GFSHIP_CHECK (e == HIPRTC_SUCCESS, GFSHIP_EHIP, "hiprtcGetCode: %s", g_rtc.GetErrorString (e));
  RtcKernel * k = new RtcKernel;
  hipError_t he = hipModuleLoadData (&k->mod, code.data ());
  if (he == hipSuccess) he = hipModuleGetFunction (&k->fn, k->mod, entry);
  if (he != hipSuccess) {
    rtc_free (k);
    return hip_fail (he, "loading the compiled function", __FILE__, __LINE__);
  }
  *out = k;
  return GFSHIP_OK;
}

// the kernel around a GfsFunction of the variables of gfs_force_coeff_read (:189-207) and the time, compiled for
// `device' (the list of a tree has no domain: the device is all the compilation needs)
int rtc_compile_coefficient_on (int device, const char * text, RtcKernel ** out)
{
  return rtc_compile (device, text,
    "static __device__ double gfship_f (double Rep, double Urelp, double Vrelp, double Wrelp,\n"
    "                                   double Pdia, double t)\n",
    "extern \"C\" __global__ void gfship_coeff (int n, const unsigned char * alive,\n"
    "    const double * rep, const double * urel, const double * vrel, const double * wrel,\n"
    "    const double * pdia, double t, double * out)\n"
    "{\n"
    "  int q = blockIdx.x*blockDim.x + threadIdx.x;\n"
    "  if (q >= n || alive[q] != 1) return;\n"
    "  out[q] = gfship_f (rep[q], urel[q], vrel[q], wrel[q], pdia[q], t);\n"
    "}\n", "gfship_coeff", out);
}

int rtc_compile_coefficient (gfship_domain * dom, const char * text, RtcKernel ** out)
{
  GFSHIP_CHECK (dom != nullptr, GFSHIP_EINVAL, "null argument");
  return rtc_compile_coefficient_on (dom->device, text, out);
}

// the kernel function of a GfsSourceParticulate (modules/particulatecommon.c:2271-2289): a GfsFunction
// (spatial) of x, y, z and t (gfs_function_spatial_value, src/utils.c:1476-1494), evaluated at the
// normalised distances of the records of the spreading (coupling.hip): record r belongs to particle
// r/stride of the chunk and is in use if r%stride < cnt[r/stride]
int rtc_compile_spatial_on (int device, const char * text, RtcKernel ** out)
{
  return rtc_compile (device, text,
    "static __device__ double gfship_f (double x, double y, double z, double t)\n",
    "extern \"C\" __global__ void gfship_spatial (long nrec, int stride, const int * cnt,\n"
    "    const double * qx, const double * qy, const double * qz, double t, double * out)\n"
    "{\n"
    "  long r = (long) blockIdx.x*blockDim.x + threadIdx.x;\n"
    "  if (r >= nrec || (int) (r%stride) >= cnt[r/stride]) return;\n"
    "  out[r] = gfship_f (qx[r], qy[r], qz[r], t);\n"
    "}\n", "gfship_spatial", out);
}

int rtc_compile_spatial (gfship_domain * dom, const char * text, RtcKernel ** out)
{
  GFSHIP_CHECK (dom != nullptr, GFSHIP_EINVAL, "null argument");
  return rtc_compile_spatial_on (dom->device, text, out);
}

int rtc_launch_spatial (RtcKernel * k, hipStream_t stream, long nrec, int stride, const int * cnt,
			const double * x, const double * y, const double * z, double t, double * out)
{
  if (nrec <= 0) return GFSHIP_OK;
  void * args[] = { &nrec, &stride, &cnt, &x, &y, &z, &t, &out };
  GFSHIP_HIP (hipModuleLaunchKernel (k->fn, (unsigned) ((nrec + 255)/256), 1, 1, 256, 1, 1, 0, stream, args,
				     nullptr));
  return GFSHIP_OK;
}

// the function of a GfsSourceParticulateVol / ...Mass (modules/particulatecommon.c:2826, 2984:
// gfs_function_value (source, cell) right after the particle wrote Rad, Urelp ... into its cell): the values
// of the particle for those four, the centre of the cell for x, y, z, and the value at the cell of every other
// variable it names.  One thread per creation slot; cell[o] is the linear number of the cell, i fastest.
// particle = false: the same kernel around a plain spatial GfsFunction at the cell (the mass and the volume of a
// GfsFeedParticle, feed_particle.hip): no Rad, Urelp ... among its variables nor among the kernel's arguments
static int compile_cell_function (gfship_domain * dom, bool particle, const char * text, int nf,
				  const char * const * names, RtcKernel ** out)
{
  GFSHIP_CHECK (dom != nullptr, GFSHIP_EINVAL, "null argument");
  const bool d3 = dom->dim == 3;
  std::string sig = "static __device__ double gfship_f (";
  if (particle) {
    sig += "double Rad, double Urelp, double Vrelp, ";
    if (d3) sig += "double Wrelp, ";
  }
  sig += "double x, double y, double z, double t";
  std::string params, values;
  for (int q = 0; q < nf; q++) {
    sig += std::string (", double ") + names[q];
    params += "    const double * f" + std::to_string (q) + ",\n";
    values += ", f" + std::to_string (q) + "[idx]";
  }
  sig += ")\n";
  std::string kern =
    "extern \"C\" __global__ void gfship_psource (int n, unsigned nside, int xo, long sy, long sz,\n"
    "    const unsigned * cell,";
  if (particle) {
    kern += " const double * rad, const double * urel, const double * vrel,\n";
    if (d3) kern += "    const double * wrel,\n";
  }
  else
    kern += "\n";
  kern += "    double t,\n" + params + "    double * out)\n"
    "{\n"
    "  int o = blockIdx.x*blockDim.x + threadIdx.x;\n"
    "  if (o >= n) return;\n"
    "  const unsigned c = cell[o];\n"
    "  if (c == 0xFFFFFFFFu) return;\n"
    "  const int i = (int) (c % nside) + 1, j = (int) ((c/nside) % nside) + 1;\n";
  kern += d3 ? "  const int k = (int) (c/(nside*nside)) + 1;\n" : "  const int k = 0;\n";
  kern +=
    "  const long idx = xo + i + sy*j + sz*k;\n"
    "  (void) idx;\n"
    "  const double h = 1./nside;\n"      /* ftt_cell_pos: dyadic, exact */
    "  out[o] = gfship_f (";
  if (particle) {
    kern += "rad[o], urel[o], vrel[o], ";
    if (d3) kern += "wrel[o], ";
  }
  kern += "-0.5 + (i - 0.5)*h, -0.5 + (j - 0.5)*h, ";
  kern += d3 ? "-0.5 + (k - 0.5)*h" : "0.";
  kern += ", t" + values + ");\n}\n";
  return rtc_compile (dom->device, text, sig.c_str (), kern.c_str (), "gfship_psource", out);
}

int rtc_compile_source (gfship_domain * dom, const char * text, int nf, const char * const * names,
			RtcKernel ** out)
{
  return compile_cell_function (dom, true, text, nf, names, out);
}

// the mass and the volume of a GfsFeedParticle (modules/particulatecommon.c:2394-2395: gfs_function_value
// (feedp->mass, cell)): the centre of the cell for x, y, z, the time, and the value at the cell of every variable
// the text names.  One thread per candidate; cell[o] as for a source
int rtc_compile_cell (gfship_domain * dom, const char * text, int nf, const char * const * names,
		      RtcKernel ** out)
{
  return compile_cell_function (dom, false, text, nf, names, out);
}

int rtc_launch_cell (RtcKernel * k, hipStream_t stream, int n, const Layout & L, const unsigned * cell,
		     double t, int nf, const double * const * fields, double * out)
{
  if (n <= 0) return GFSHIP_OK;
  unsigned nside = (unsigned) L.n;
  int xo = L.xo;
  long sy = L.sy, sz = L.sz;
  std::vector<const double *> f (fields, fields + nf);
  std::vector<void *> args = { &n, &nside, &xo, &sy, &sz, &cell, &t };
  for (int q = 0; q < nf; q++) args.push_back (&f[q]);
  args.push_back (&out);
  GFSHIP_HIP (hipModuleLaunchKernel (k->fn, (unsigned) ((n + 255)/256), 1, 1, 256, 1, 1, 0, stream, args.data (),
				     nullptr));
  return GFSHIP_OK;
}

int rtc_launch_source (RtcKernel * k, hipStream_t stream, int n, const Layout & L, const unsigned * cell,
		       const double * rad, const double * const urel[3], double t, int nf,
		       const double * const * fields, double * out)
{
  if (n <= 0) return GFSHIP_OK;
  unsigned nside = (unsigned) L.n;
  int xo = L.xo;
  long sy = L.sy, sz = L.sz;
  const double * u = urel[0], * v = urel[1], * w = urel[2];
  std::vector<const double *> f (fields, fields + nf);
  std::vector<void *> args = { &n, &nside, &xo, &sy, &sz, &cell, &rad, &u, &v };
  if (L.dim == 3) args.push_back (&w);
  args.push_back (&t);
  for (int q = 0; q < nf; q++) args.push_back (&f[q]);
  args.push_back (&out);
  GFSHIP_HIP (hipModuleLaunchKernel (k->fn, (unsigned) ((n + 255)/256), 1, 1, 256, 1, 1, 0, stream, args.data (),
				     nullptr));
  return GFSHIP_OK;
}

// the same function on a list of a tree (update_vol / update_mass with cell = the leaf of gfs_domain_locate
// (pos, -1)): cell[o] is the index of the leaf in the concatenated levels.  Its level is the last one whose offset
// is not beyond it (level_of, cell_sums.hpp; the loop has constant bounds, so the offsets are read from the
// kernel arguments with constant indices), its integer coordinates come from its index in the dense (2^l + 2)^dim
// level, and ftt_cell_pos is -0.5 + (i - 0.5)*2^-l, dyadic and exact.  The variables are arrays of all levels
struct TreeSourceOffsets { int v[GFSHIP_MAXLEVEL + 2]; };

// particle = false: the same kernel around a plain spatial GfsFunction at the leaf (the mass and the volume of a
// GfsFeedParticle on a list of a tree, feed_particle.hip): no Rad, Urelp ... among its variables nor among the
// kernel's arguments, as in compile_cell_function
static int compile_tree_cell_function (int device, int dim, bool particle, const char * text, int nf,
				       const char * const * names, RtcKernel ** out)
{
  const bool d3 = dim == 3;
  std::string sig = "static __device__ double gfship_f (";
  if (particle) {
    sig += "double Rad, double Urelp, double Vrelp, ";
    if (d3) sig += "double Wrelp, ";
  }
  sig += "double x, double y, double z, double t";
  std::string params, values;
  for (int q = 0; q < nf; q++) {
    sig += std::string (", double ") + names[q];
    params += "    const double * f" + std::to_string (q) + ",\n";
    values += ", f" + std::to_string (q) + "[g]";
  }
  sig += ")\n";
  const std::string maxlevel = std::to_string (GFSHIP_MAXLEVEL);
  std::string kern =
    "struct gfship_offsets { int v[" + maxlevel + " + 2]; };\n"
    "extern \"C\" __global__ void gfship_tree_psource (int n, int depth, gfship_offsets off,\n"
    "    const unsigned * cell,";
  if (particle) {
    kern += " const double * rad, const double * urel, const double * vrel,\n";
    if (d3) kern += "    const double * wrel,\n";
  }
  else
    kern += "\n";
  kern += "    double t,\n" + params + "    double * out)\n"
    "{\n"
    "  int o = blockIdx.x*blockDim.x + threadIdx.x;\n"
    "  if (o >= n) return;\n"
    "  const unsigned g = cell[o];\n"
    "  if (g == 0xFFFFFFFFu) return;\n"
    "  int l = 0, base = off.v[0];\n"
    "#pragma unroll\n"
    "  for (int m = 1; m <= " + maxlevel + "; m++)\n"
    "    if (m <= depth && (int) g >= off.v[m]) { l = m; base = off.v[m]; }\n"
    "  const unsigned q = g - (unsigned) base, r = (1u << l) + 2u;\n"
    "  const int i = (int) (q % r), j = (int) ((q/r) % r);\n";
  kern += d3 ? "  const int k = (int) (q/(r*r));\n" : "  const int k = 0;\n";
  kern +=
    "  (void) k;\n"
    "  const double h = 1./(double) (1u << l);\n"      /* ftt_cell_pos: dyadic, exact */
    "  out[o] = gfship_f (";
  if (particle) {
    kern += "rad[o], urel[o], vrel[o], ";
    if (d3) kern += "wrel[o], ";
  }
  kern += "-0.5 + (i - 0.5)*h, -0.5 + (j - 0.5)*h, ";
  kern += d3 ? "-0.5 + (k - 0.5)*h" : "0.";
  kern += ", t" + values + ");\n}\n";
  return rtc_compile (device, text, sig.c_str (), kern.c_str (), "gfship_tree_psource", out);
}

int rtc_compile_tree_source (int device, int dim, const char * text, int nf, const char * const * names,
			     RtcKernel ** out)
{
  return compile_tree_cell_function (device, dim, true, text, nf, names, out);
}

// the mass and the volume of a GfsFeedParticle on a list of a tree (gfs_function_value (feedp->mass, cell) with cell =
// the leaf of gfs_domain_locate (pos, -1), modules/particulatecommon.c:2382, 2394-2395)
int rtc_compile_tree_cell (int device, int dim, const char * text, int nf, const char * const * names,
			   RtcKernel ** out)
{
  return compile_tree_cell_function (device, dim, false, text, nf, names, out);
}

int rtc_launch_tree_cell (RtcKernel * k, hipStream_t stream, int n, int depth, const int * off,
			  const unsigned * cell, double t, int nf, const double * const * fields, double * out)
{
  if (n <= 0) return GFSHIP_OK;
  TreeSourceOffsets O;
  for (int l = 0; l < GFSHIP_MAXLEVEL + 2; l++) O.v[l] = off[l];
  std::vector<const double *> f (fields, fields + nf);
  std::vector<void *> args = { &n, &depth, &O, &cell, &t };
  for (int q = 0; q < nf; q++) args.push_back (&f[q]);
  args.push_back (&out);
  GFSHIP_HIP (hipModuleLaunchKernel (k->fn, (unsigned) ((n + 255)/256), 1, 1, 256, 1, 1, 0, stream, args.data (),
				     nullptr));
  return GFSHIP_OK;
}

int rtc_launch_tree_source (RtcKernel * k, hipStream_t stream, int n, int dim, int depth, const int * off,
			    const unsigned * cell, const double * rad, const double * const urel[3], double t,
			    int nf, const double * const * fields, double * out)
{
  if (n <= 0) return GFSHIP_OK;
  TreeSourceOffsets O;
  for (int l = 0; l < GFSHIP_MAXLEVEL + 2; l++) O.v[l] = off[l];
  const double * u = urel[0], * v = urel[1], * w = urel[2];
  std::vector<const double *> f (fields, fields + nf);
  std::vector<void *> args = { &n, &depth, &O, &cell, &rad, &u, &v };
  if (dim == 3) args.push_back (&w);
  args.push_back (&t);
  for (int q = 0; q < nf; q++) args.push_back (&f[q]);
  args.push_back (&out);
  GFSHIP_HIP (hipModuleLaunchKernel (k->fn, (unsigned) ((n + 255)/256), 1, 1, 256, 1, 1, 0, stream, args.data (),
				     nullptr));
  return GFSHIP_OK;
}

int rtc_launch_coefficient (RtcKernel * k, hipStream_t stream, int n, const unsigned char * alive,
			    const double * rep, const double * const rel[3], const double * pdia,
			    double t, double * out)
{
  if (n <= 0) return GFSHIP_OK;
  const double * u = rel[0], * v = rel[1], * w = rel[2];
  void * args[] = { &n, &alive, &rep, &u, &v, &w, &pdia, &t, &out };
  GFSHIP_HIP (hipModuleLaunchKernel (k->fn, (unsigned) ((n + 255)/256), 1, 1, 256, 1, 1, 0, stream, args,
				     nullptr));
  return GFSHIP_OK;
}

} // namespace gfship
