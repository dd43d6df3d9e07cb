// tree_flow.hpp -- the relax loop of a tree level (src/poisson.c:1070-1089 over the cells of
// T_LEVEL_LEAFS, src/poisson.c:604-632) as a dataflow program of fixed-format micro-operations.
// This file holds the kernels and is included by tree.hip inside its anonymous namespace; the record format and
// the arithmetic of one operation, which the host's emulator shares, are in tree_flow_ops.hpp; the planner
// (FlowBuilder, plan_flow) and the emulator (flow_emulate) are in tree_plan.hip.
//
// Why: t_relax_nodes interprets the stencil of a cell from a variable-length tape, one thread per
// cell -- a coarse leaf with fine neighbours is a chain of ~100 dependent LDS reads, and the slowest
// thread of a dependency level sets its time (8-10 us per level on the fine levels of the octree
// bench).  Here the stencil of a cell is cut where its expression tree
// branches (same floating-point operations in the same order):
//   FC     gradient_fine_coarse towards a coarser neighbour (src/fluid.c:283-309 through
//          interpolate_1D1 / interpolate_2D1, :178-245): the pair (nb, na) of one face;
//   CHILD  the same expression seen from the coarse side, one fine cell behind a face of a coarser
//          leaf (src/fluid.c:795-829): the pair of one child;
//   SUM    the sum over the children of that face, in child order (:812-826);
//   CELL   the sums over the faces in direction order and the new value (relax, src/poisson.c:507-557;
//          diffusion_relax, :1471-1498);
//   GHOST  the copy of a ghost cell between two sweeps (homogeneous condition or periodic image).
// Every operation has at most nine inputs at fixed places of a 48-byte record, all independent
// loads, and is scheduled as a node of its own: CHILD one level before its SUM, FC / SUM one level
// before their CELL.  A level holds at most `width' (<= 512) operations: thread t of the workgroup executes
// operation t of the level and leaves its result in LDS (a ring of FLOW_NBUF buffers indexed by the level)
// for the operations of the next levels -- that is how the pairs travel, and how a cell value reaches
// the neighbours that follow it closely.  Older values are read from global memory one level ahead of
// their use (the workgroup's own stores of earlier levels are ordered before these loads by the barrier:
// same CU, no acknowledgement needed); the record of a level is loaded three levels ahead.  An extra
// wavefront does the stores, a level late, from the LDS.  What is left on the chain of a level: the LDS
// reads of its fresh inputs, the arithmetic of ONE micro-operation, an LDS write, a barrier.
//
// The loop runs on copies of the values and of the right-hand side laid out in the order of the plan
// (t_flow_pack / t_flow_unpack around it): see FlowProgram (tree_plan.hpp).
//
// The schedule keeps the order of the sequential program as plan_loop does (a read follows the write
// it must see, a write follows the reads of the value it replaces, one level at least), so that the
// single image in global memory is right for every load; gfship_tree_host_check runs the plan on the
// host with the kernel's timing of loads and stores (and its choice of the branch-free arithmetic per
// wavefront) and compares with the reference's program.
//
// Measured (octree bench, tools/tree_bench.py 3 4 2: 39 712 leaves, levels 4-6; profiles/r03_tree_flow.txt;
// DESIGN.md 11.15 has the whole account): the loop of the finest level 3.43 ms (t_relax_nodes_pf, 349 levels of
// the tape plan) -> 0.79 ms (681 levels of 512 operations), the cycle 6.6 -> 1.5 ms.  A level costs 1.0-1.2 us
// whatever its width: every wavefront of a level wants the vector memory pipeline (14 loads per thread), then the
// LDS, then the vector ALU (~100 instructions around ~40 f64 operations and one division) and the barrier keeps
// them in step.  What paid, in order: fixed-format operations with independent loads instead of the tape (2.7 x);
// even and odd wavefronts in different orders (17 %); the kinds of a level at multiples of 64, i.e. no wavefront
// with two kinds (14 %); the working copies in plan order (18 % on the finest loop).  Tried without a gain, and left
// in or out as said: loads two levels ahead (out: 15-fold unrolling, 224 VGPRs); the storing wavefront (in); the
// working copies read into the L2 once at the start (in); the lines of the record stream touched eight levels
// ahead by LDS-DMA loads (out); 128 / 256 / 384 operations per level (GFSHIP_FLOW_WIDTH; 256 is the default on
// quadtrees); on quadtrees a CELL with the FC / CHILD / SUM of its faces in the same operation (out: 38 % fewer
// levels, each twice as expensive); a select-free CELL / FC (out: 5 % slower).

struct FlowAnyDev {
  __device__ inline bool operator() (bool b) const { return __any (b); }
};

// One level of one wavefront: the inputs from the LDS, the arithmetic.  A wavefront of one kind reads only
// what that kind can use (FC / CHILD: nine values; CELL: the values and the pairs of its faces; SUM: pairs) --
// the reads of the LDS are a third of the time of a level when every lane reads ten pairs.
template <int DIM>
__device__ inline FlowPair flow_eval_wave (const FlowRec & r, const double * v, const FlowPair * lo,
					   const double * ct, double omega, int op, double w)
{
  constexpr int NIN = FlowShape<DIM>::NIN;
  const unsigned w0 = r.w0;
  const int kind = flow_class (w0 & 7);
  const unsigned long long busy = __ballot (kind != F_NOP);
  FlowPair o = { 0., 0. };
  if (busy == 0ull)
    return o;
  const int first = __builtin_amdgcn_readlane (kind, __ffsll ((long long) busy) - 1);
  const FlowAnyDev any;
  double x[NIN], y[NIN];
#define FLOW_X(j) { const double px = *(const double *) ((const char *) lo + FLOW_LDS_ADDR (r.in[j])); \
    x[j] = FLOW_IS_LDS (r.in[j]) ? px : v[j]; y[j] = 0.; }
#define FLOW_XY(j) { const FlowPair p = *(const FlowPair *) ((const char *) lo + FLOW_LDS_ADDR (r.in[j])); \
    x[j] = FLOW_IS_LDS (r.in[j]) ? p.x : v[j]; y[j] = p.y; }
  if (__ballot (kind != F_NOP && kind != first) != 0ull) {
#pragma unroll
    for (int j = 0; j < NIN; j++) FLOW_XY (j)
    return flow_eval<DIM> (w0, x, y, v[FLOW_NIN], ct, omega, op, w);
  }
#pragma unroll
  for (int j = 0; j < NIN; j++) { x[j] = 0.; y[j] = 0.; }
  if (first == F_CELL) {
    if (DIM == 2) FLOW_X (0)
#pragma unroll
    for (int j = 1; j <= 2*DIM; j++) FLOW_XY (j)
    return flow_eval_uniform<DIM, F_CELL> (w0, x, y, v[FLOW_NIN], ct, omega, op, w, any);
  }
  if (first == F_FC) {
#pragma unroll
    for (int j = 0; j < 1 + (DIM - 1)*FlowShape<DIM>::TS; j++) FLOW_X (j)
    return flow_eval_uniform<DIM, F_FC> (w0, x, y, v[FLOW_NIN], ct, omega, op, w, any);
  }
  if (first == F_SUM) {
#pragma unroll
    for (int j = 0; j < (DIM == 3 ? 4 : 2); j++) FLOW_XY (j)
    return flow_eval_uniform<DIM, F_SUM> (w0, x, y, v[FLOW_NIN], ct, omega, op, w, any);
  }
  FLOW_X (0)
  return flow_eval_uniform<DIM, F_GHOST> (w0, x, y, v[FLOW_NIN], ct, omega, op, w, any);
#undef FLOW_X
#undef FLOW_XY
}

// The loads of the kernel are unconditional (an idle thread loads the last record of the level and turns it
// into a NOP, an input that comes from LDS loads cell 0 from global memory and the other way round, selects
// afterwards): straight-line code in which the compiler counts the outstanding loads exactly -- behind
// branches it waits for everything, records and old values just issued included.

// the record of thread tid on level L (the plan ends with NOP levels for the loads ahead of the last level);
// only the words the dimension uses are loaded (a loaded word that nobody reads leaves a free register with a
// load pending on it: the next write to it waits for the load)
template <int DIM>
__device__ inline FlowRec flow_load_rec (const FlowRec * rec, const int * loff, int L, int tid)
{
  typedef int int4v __attribute__((ext_vector_type(4)));
  typedef int int3v __attribute__((ext_vector_type(3)));
  const int a = loff[L], b = loff[L + 1];      /* from the LDS: from global memory the load of the record would wait for this one */
  const bool valid = a + tid < b;
  const int * q = (const int *) (rec + a + tid);      /* an idle lane reads on (the array ends with spare records): every
							 lane at the same address is the slowest access there is */
  FlowRec r;
  const int4v q0 = *(const int4v *) q;
  r.w0 = valid ? (unsigned) q0.x : (unsigned) F_NOP;
  r.out_g = valid ? q0.y : -1;
  r.in[0] = valid ? q0.z : FLOW_NONE;
  r.in[1] = valid ? q0.w : FLOW_NONE;
#pragma unroll
  for (int j = 2; j < FLOW_NIN; j++) r.in[j] = FLOW_NONE;
  if (DIM == 3) {
    const int4v q1 = *(const int4v *) (q + 4);
    const int3v q2 = *(const int3v *) (q + 8);
    r.in[2] = valid ? q1.x : FLOW_NONE; r.in[3] = valid ? q1.y : FLOW_NONE;
    r.in[4] = valid ? q1.z : FLOW_NONE; r.in[5] = valid ? q1.w : FLOW_NONE;
    r.in[6] = valid ? q2.x : FLOW_NONE; r.in[7] = valid ? q2.y : FLOW_NONE; r.in[8] = valid ? q2.z : FLOW_NONE;
  }
  else {
    const int3v q1 = *(const int3v *) (q + 4);
    r.in[2] = valid ? q1.x : FLOW_NONE; r.in[3] = valid ? q1.y : FLOW_NONE; r.in[4] = valid ? q1.z : FLOW_NONE;
  }
  return r;
}

template <int DIM>
__device__ inline void flow_prefetch (const FlowRec & r, const double * u, const double * rhs, double * v, int idle)
{
  /* idle: 8 tid -- an input that is not in global memory loads a place of its own (the copies have 576 at least) */
#pragma unroll
  for (int j = 0; j < FlowShape<DIM>::NIN; j++)
    v[j] = *(const double *) ((const char *) u + (unsigned) (r.in[j] < 0 ? idle : r.in[j]));
  v[FLOW_NIN] = *(const double *) ((const char *) rhs + (unsigned) (r.out_g < 0 ? idle : r.out_g));
}

// the whole relax loop: one workgroup, one operation per thread and level
template <int DIM>
__global__ void __launch_bounds__(FLOW_WIDTH + 64)
t_relax_flow (const FlowRec * __restrict__ rec, const int * __restrict__ lev_off, int nlev,
	      const double * __restrict__ ctab, int nct, double * u, const double * __restrict__ rhs, int npos,
	      double omega, int op, double w)
{
  __shared__ FlowPair lo[FLOW_LDS_SLOTS];
  __shared__ int lout[FLOW_NBUF*FLOW_WIDTH];
  __shared__ int loff[FLOW_MAXLEV + FLOW_PD + 4];
  __shared__ double ct[FLOW_NCONST];
  const int tid = threadIdx.x;
  if (tid < nct) ct[tid] = ctab[tid];
  const int width = blockDim.x - 64;      /* the width the plan was made for; the last wavefront stores */
  for (int q = tid; q < FLOW_LDS_SLOTS; q += blockDim.x) lo[q] = FlowPair { 0., 0. };
  for (int q = tid; q < FLOW_NBUF*FLOW_WIDTH; q += blockDim.x) lout[q] = -1;
  for (int q = tid; q < nlev + FLOW_PD + 3; q += blockDim.x) loff[q] = lev_off[q];
  // The copies the loop works on were written by other compute units: the first load of each of their lines
  // comes from memory (a microsecond), and a level cannot be shorter than the loads it issued a level ago.
  // Read them once, all lanes, pipelined: afterwards they are in this XCD's L2 (and the stores of the loop
  // update them there).
  double warm = 0.;
  for (int q = tid*16; q < npos; q += blockDim.x*16)
    warm += ((const volatile double *) u)[q] + ((const volatile double *) rhs)[q];
  if (warm == 1.2345678e-300) ct[FLOW_NCONST - 1] = warm;      /* (keeps the loads) */
  __syncthreads ();
  if (tid >= width) {
    // The storing wavefront: the wavefronts that compute leave result and place in the LDS, and this one
    // stores the results of level L - 1 while level L is computed.  vmcnt counts loads and stores together,
    // in issue order: a wavefront that stored its own results would not get at the values it loaded
    // afterwards before those stores are acknowledged.
    const int lane = tid - width;
    __syncthreads ();
    for (int L = 0; L <= nlev; L++) {
      if (L >= 1) {
	const int base = ((L - 1) % FLOW_NBUF)*width;
	int g[FLOW_WIDTH/64];
	double xv[FLOW_WIDTH/64];
#pragma unroll
	for (int i = 0; i < FLOW_WIDTH/64; i++) {      /* every read of the LDS first, then the stores */
	  const int k = lane + 64*i;
	  g[i] = lout[base + (k < width ? k : 0)];
	  xv[i] = lo[base + (k < width ? k : 0)].x;
	  if (k >= width) g[i] = -1;
	}
#pragma unroll
	for (int i = 0; i < FLOW_WIDTH/64; i++)
	  if (g[i] >= 0)
	    *(double *) ((char *) u + (unsigned) g[i]) = xv[i];
      }
      if (L < nlev) __syncthreads ();
    }
    return;
  }
  // In level L: the record of L + 3 is loaded, the old values of L + 1 (its record came two levels ago) are
  // loaded, L is evaluated from registers and LDS.  Four records and two sets of old values rotate through
  // fixed registers: the loop is written out four levels at a time, no copies (a copy of a set would wait
  // for its loads).  vmcnt counts in issue order: what a level waits for was issued a level ago at least.
  // The stores of the levels before L - 1 were issued before the barrier that ended L - 1: the loads of this
  // level see them (same CU, in order); younger values come from the LDS.
  FlowRec r0 = flow_load_rec<DIM> (rec, loff, 0, tid);
  FlowRec r1 = flow_load_rec<DIM> (rec, loff, 1, tid);
  FlowRec r2 = flow_load_rec<DIM> (rec, loff, 2, tid);
  FlowRec r3;
  double v0[FLOW_NIN + 1], v1[FLOW_NIN + 1];
  flow_prefetch<DIM> (r0, u, rhs, v0, 8*tid);
  flow_prefetch<DIM> (r1, u, rhs, v1, 8*tid);      /* (loaded again in level 0; keeps v1 defined for the lab switches) */
  __syncthreads ();
  // FLOW_LAB (lab only): 1 no arithmetic, 2 no loads of old values, 4 no loads of records (wrong results);
  // 32 the times of the parts of eight levels printed (s_memtime); 64 every wavefront in the same order
#ifndef FLOW_LAB
#define FLOW_LAB 0
#endif
#if FLOW_LAB & 32
#define FLOW_TS(L, k) if ((tid & 63) == 0 && (L) >= 300 && (L) < 308)	\
    tstamp[tid >> 6][(L) - 300][k] = __builtin_amdgcn_s_memtime ();
#else
#define FLOW_TS(L, k)
#endif
#define FLOW_LOADS(L, R0, R1, R3, V1)					\
    if (!(FLOW_LAB & 2)) flow_prefetch<DIM> (R1, u, rhs, V1, 8*tid);	\
    if (!(FLOW_LAB & 4)) R3 = flow_load_rec<DIM> (rec, loff, (L) + 3, tid); else R3 = R0;
#define FLOW_COMPUTE(L, R0, V0) {					\
    FLOW_TS (L, 2)							\
    FlowPair o = { V0[0] + V0[1], V0[2] };				\
    if (!(FLOW_LAB & 1)) o = flow_eval_wave<DIM> (R0, V0, lo, ct, omega, op, w); \
    if ((FLOW_LAB & 32) && o.x == 1.2345e-300) ct[FLOW_NCONST - 4] = o.x; \
    FLOW_TS (L, 3)							\
    lo[buf*width + tid] = o;						\
    lout[buf*width + tid] = R0.out_g;					\
    buf = buf == FLOW_NBUF - 1 ? 0 : buf + 1;				\
  }
  // Two orders of a level.  Every wavefront of a level wants the vector memory pipeline, then the LDS, then
  // the vector ALU, and the barrier keeps them in step: three units, one busy at a time (measured with
  // s_memtime, FLOW_LAB=32: 900 cycles to issue the 14 loads of a level, 850 for the reads of the LDS, 950 to
  // 1900 of arithmetic, the rest waiting for the slowest).  So the odd wavefronts issue their loads AFTER
  // their arithmetic (their old values then have the barrier and the next level's LDS reads to arrive):
  // they compute while the even ones load, and the other way round.
#define FLOW_STEP_A(L, R0, R1, R3, V0, V1) {				\
    FLOW_TS (L, 0)							\
    FLOW_LOADS (L, R0, R1, R3, V1)					\
    FLOW_TS (L, 1)							\
    FLOW_COMPUTE (L, R0, V0)						\
    __syncthreads ();							\
    FLOW_TS (L, 4)							\
  }
#define FLOW_STEP_B(L, R0, R1, R3, V0, V1) {				\
    FLOW_TS (L, 0)							\
    FLOW_TS (L, 1)							\
    FLOW_COMPUTE (L, R0, V0)						\
    FLOW_LOADS (L, R0, R1, R3, V1)					\
    __syncthreads ();							\
    FLOW_TS (L, 4)							\
  }
  int buf = 0;
#if FLOW_LAB & 32
  __shared__ unsigned long long tstamp[8][8][5];
#endif
  if ((tid >> 6) & 1 & !(FLOW_LAB & 64)) {
    for (int L = 0; L < nlev; L += 4) {
      FLOW_STEP_B (L, r0, r1, r3, v0, v1);
      if (L + 1 >= nlev) break;
      FLOW_STEP_B (L + 1, r1, r2, r0, v1, v0);
      if (L + 2 >= nlev) break;
      FLOW_STEP_B (L + 2, r2, r3, r1, v0, v1);
      if (L + 3 >= nlev) break;
      FLOW_STEP_B (L + 3, r3, r0, r2, v1, v0);
    }
  }
  else {
    for (int L = 0; L < nlev; L += 4) {
      FLOW_STEP_A (L, r0, r1, r3, v0, v1);
      if (L + 1 >= nlev) break;
      FLOW_STEP_A (L + 1, r1, r2, r0, v1, v0);
      if (L + 2 >= nlev) break;
      FLOW_STEP_A (L + 2, r2, r3, r1, v0, v1);
      if (L + 3 >= nlev) break;
      FLOW_STEP_A (L + 3, r3, r0, r2, v1, v0);
    }
  }
#undef FLOW_STEP_A
#undef FLOW_STEP_B
#undef FLOW_LOADS
#undef FLOW_COMPUTE
#if FLOW_LAB & 32
  __syncthreads ();
  if (tid == 0 && nlev > 320)
    for (int wv = 0; wv < width/64; wv++)
      for (int q = 0; q < 8; q++) {
	const unsigned long long * t = tstamp[wv][q];
	printf ("flow lab: wave %d level %d kind %d: issue %llu gather %llu eval %llu barrier %llu | next start +%llu\n", wv, 300 + q,
		(int) (rec[loff[300 + q] + min (wv*64, loff[301 + q] - loff[300 + q] - 1)].w0 & 7),
		t[1] - t[0], t[2] - t[1], t[3] - t[2], t[4] - t[3], q < 7 ? tstamp[wv][q + 1][0] - t[4] : 0ull);
      }
#endif
}

// into / out of the order of the plan
__global__ void t_flow_pack (const int * __restrict__ gidx, int n, const double * __restrict__ u,
			     const double * __restrict__ rhs, double * __restrict__ up, double * __restrict__ rp)
{
  const int p = blockIdx.x*blockDim.x + threadIdx.x;
  if (p < n) {
    const int g = gidx[p];
    up[p] = u[g];
    rp[p] = rhs[g];
  }
}

__global__ void t_flow_unpack (const int * __restrict__ gidx, int n, const double * __restrict__ up, double * __restrict__ u)
{
  const int p = blockIdx.x*blockDim.x + threadIdx.x;
  if (p < n)
    u[gidx[p]] = up[p];
}

