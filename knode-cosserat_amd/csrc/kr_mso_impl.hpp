// kr_mso_impl.hpp - persistent multiple shooting with OVERLAPPED time steps (round 3).
//
// kr_ms_impl.hpp spends, in its steady state, two sweeps of (N-1)/4 dependent grid points on every time step: the
// forward-difference sweep at the predicted start x0(t) that yields the Newton correction, and a second sweep at the
// corrected unknowns x1(t) that measures the (by then negligible) residual and streams the accepted state out.  In the
// second sweep only the four unperturbed lanes do anything useful; the 54 forward-difference lanes recompute a
// Jacobian nobody uses once the residual test has accepted the sweep - which is what happens on 97 % of the steps.
//
// Here the verifying sweep of step t and the Jacobian sweep of step t + 1 are ONE sweep of the same wavefront:
//     lanes  0..57   forward-difference sweep of step t + 1 from its predicted start x0(t+1)   (as before)
//     lanes 58..61   re-integrate step t from x1(t), one lane per sub-interval, and stream the state out
// The start values of step t + 1 only need the UNKNOWNS of step t (known after its Newton update), and its BDF2
// history record at grid point j only needs the state of step t at j - so the verifying lanes run one grid point
// ahead and leave the twelve leading slots (q w v u) of every grid point they produce in an LDS tile; the
// forward-difference lanes pick them up at the end of the same trip and form the history record of their next grid point
// themselves (round 5: two raw tiles, time level t in tile t & 1 - a precombined record cost the four verifying lanes a
// divergent block of 30 fp64 instructions, 15 LDS stores and 6 LDS loads per trip, and a store from a lone wavefront is
// the most expensive instruction there is: LABBOOK, "what a store costs a lone wavefront").  Per time step that leaves
// one sweep and one condensation; the discrete equations, the Newton iteration, the stopping rule and the stored states
// are those of kr_ms_impl.hpp (cosserat_ode.py:188-213 inside knode.py:70-100).
//
// Acceptance of step t is still a measured quantity of a sweep at the stored unknowns: the residual test, else the
// chord update through the factors of step t's last condensation (which are only overwritten afterwards).  If
// neither accepts, the Jacobian work for step t + 1 is thrown away, the chord update is applied, the tile the rejected
// sweep wrote over is put back and step t continues with plain forward-difference sweeps.  Put back from where: the
// fp64 kernels at one wavefront per SIMD PARK that tile in registers before every merged sweep (one generation of one
// tile is all a roll-back needs - the other tile is not written by the sweep) and store an accepted state's leading
// slots only where the state has a reader: the last three states of a ring call, every state of a full trajectory.
// Interior steps of a ring run then leave only the interval-start records in HBM, and a rod that gives up flushes its
// two tiles on the way out.  The other kernels (fp32, two wavefronts per SIMD) copy every accepted tile to HBM in one
// pass of the wavefront and rebuild both tiles from there.
// Everything beyond that - a step that does not converge from the predicted or from the warm start - is left to
// kr_ms_impl.hpp's kernel, launched behind this one: a rod that gives up writes the step it stopped at to
// SimArgs::resume and the second kernel resumes there with the full ladder (warm start, damped single shooting).
//
// Serves: Euler sweeps, diagonal material matrices, MLP off, any N whose history fits the LDS (4 rods per CU).
#pragma once
#include "kr_ms_impl.hpp"

namespace kr {

constexpr int MSO_B0 = 7 + 17 * (MS_P - 1);  // 58: first of the four lanes that re-integrate the step under verification
#ifndef KR_MSO_LAG
#define KR_MSO_LAG 1
#endif
// grid points the verifying lanes run ahead of the lanes that consume their records.  2 (-DKR_MSO_LAG=2: a compile-time probe)
// lets the next trip's tile reads go out under this trip's arithmetic - measured 40.8 M against 42.1 M rod-steps/s (one more
// trip per sweep, and the pinned hand-over keeps the compiler from pairing trips)
constexpr int MSO_LAG = KR_MSO_LAG;
// -DKR_MSO_PROBE_EARLY_READS (a compile-time probe, TIMING ONLY - the results are wrong): a full trip reads BOTH tiles of
// the next grid point in front of the verifying lanes' store block, so no read waits for a store of its own trip.  The
// merged-sweep ticks of the stamped build of it (make dbg DBGFLAGS="-DKR_MS_STAMPS -DKR_MSO_PROBE_EARLY_READS") are the
// most that hiding the tile round trip can give (LABBOOK, "merged trip").
// -DKR_MSO_PROBE_NO_TILE_STORES, -DKR_MSO_PROBE_ONE_TILE_STORE (compile-time probes, TIMING ONLY - the results are wrong):
// the verifying lanes of a full trip leave their tile store out, or store the first 16 bytes of the 96, so the
// forward-difference lanes read leading slots that are two time levels old (finite values; the event counts of a sine
// run stay what they are).  What the merged-sweep ticks of the stamped builds lose is what the store block costs a
// trip, and what one store of it costs (LABBOOK, "what a merged trip waits for": 200 ticks, 27 per store).
// -DKR_MSO_TRIP_WAITS=0 (a compile-time probe; same results): the tile reads value by value, a counted wait per read.
// -DKR_MSO_TRIP_CARRY=1 (a compile-time probe; same results): the scale 2 / h.h of a trip's rotation is formed behind
// the Euler update of the trip before and carried in a register (rot_scale / ode_eval_s, rod_device.hpp), so that no
// trip opens with that serial chain.  Measured: 0.4 k ticks per step off the merged sweep on its own, 0.35 k ON it
// beside the one-wait reads, which take 0.88 k off alone - the two do not add, and the reads are what is built.
// -DKR_MSO_PROBE_NO_TILE_PASS (a compile-time probe, TIMING ONLY): a lean ring step leaves out the pass that copies the
// accepted tile of leading slots to HBM, whatever the kernel.  Right only while no verification is rejected and no rod
// gives up - true of the headline run, whose event counts say so - and WRONG in general: without the park (below) a
// roll-back and the take-over kernel read those slots back from HBM.  With -DKR_MSO_PARK=0 on the fp64 kernels it is the
// price of the pass alone: what the verdict's ticks of the stamped build lose (LABBOOK, "the roll-back tile in registers").
// -DKR_MSO_PARK=0 (a compile-time switch; same results): no park - every accepted step copies its tile to HBM and a
// roll-back reads both tiles back from there, as the fp32 kernels and two wavefronts per SIMD still do.
#ifndef KR_MSO_PARK
#define KR_MSO_PARK 1
#endif
#ifndef KR_MSO_TRIP_WAITS
#define KR_MSO_TRIP_WAITS 1
#endif
#ifndef KR_MSO_TRIP_CARRY
#define KR_MSO_TRIP_CARRY 0
#endif
static_assert(MSO_B0 + MS_P <= WAVE, "the verifying lanes must fit beside the forward-difference lanes");

template <typename T, int HS>
__host__ __device__ inline size_t mso_lds_elems(int N) {
  return ms_lds_elems<T, HS>(N, true, false) + 80;  // + XsB: the unknowns of the step under verification
}

// Hand-offs between lanes of ONE wavefront through LDS need no hardware wait: the LDS unit serves a wavefront's
// accesses in order, and the compiler tracks the counters of the loads it consumes.  What is needed is that the
// compiler does not move LDS accesses across the hand-off - a wavefront-scope fence.  (wave_sync()'s workgroup-scope
// fence also waits for every outstanding global store, i.e. for the records a sweep has just streamed out.)
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// 16-byte vector loads / stores through pointers the CALLER knows to be LDS.  The tiles of leading slots are picked by the
// parity of a time level, and behind such a select the compiler no longer proves the address space: it fell back to
// flat_load / flat_store (24 + 12 per pair of trips) until the accesses said so themselves.
#define KR_LDS __attribute__((address_space(3)))
// sched_barrier mask: everything may be scheduled across but LDS accesses (bits 7..9: all DS, DS read, DS write)
#define KR_SCHED_ALL_BUT_DS 0x047f
template <typename T, int NV>
__device__ __forceinline__ void lds_load_vec(const T* src, T (&v)[NV]) {
  using V = typename Vec16<T>::type;
  constexpr int n = Vec16<T>::n;
  static_assert(NV % n == 0, "vector load needs a multiple of 16 bytes");
  const KR_LDS V* s = (const KR_LDS V*)src;
#pragma unroll
  for (int c = 0; c < NV / n; ++c) {
    const V x = s[c];
#pragma unroll
    for (int e = 0; e < n; ++e) v[c * n + e] = x[e];
  }
}
template <typename T, int NV>
__device__ __forceinline__ void lds_store_vec(T* dst, const T (&v)[NV]) {
  using V = typename Vec16<T>::type;
  constexpr int n = Vec16<T>::n;
  static_assert(NV % n == 0, "vector store needs a multiple of 16 bytes");
  KR_LDS V* d = (KR_LDS V*)dst;
#pragma unroll
  for (int c = 0; c < NV / n; ++c) {
    V x;
#pragma unroll
    for (int e = 0; e < n; ++e) x[e] = v[c * n + e];
    d[c] = x;
  }
}

// The twelve leading slots of one grid point as the 16-byte tuples the LDS reads deliver (six in fp64).
// Read value by value, every pair of products that consumes one read gets a counted wait of its own - a staircase
// lgkmcnt(5) .. (0) that hides nothing when the reads went out fifty instructions earlier and only takes issue slots
// from a lone wavefront.  lead_pin() names all tuples of a tile in one empty asm in front of their first use: one wait.
template <typename T>
struct LeadTile {
  using V = typename Vec16<T>::type;
  static constexpr int NT = 12 / Vec16<T>::n;
  V t[NT];
};
template <typename T>
__device__ __forceinline__ void lds_load_lead(const T* src, LeadTile<T>& x) {
  using V = typename Vec16<T>::type;
  const KR_LDS V* s = (const KR_LDS V*)src;
#pragma unroll
  for (int c = 0; c < LeadTile<T>::NT; ++c) x.t[c] = s[c];
}
__device__ __forceinline__ void lead_pin(LeadTile<double>& x) {
  asm volatile("" : "+v"(x.t[0]), "+v"(x.t[1]), "+v"(x.t[2]), "+v"(x.t[3]), "+v"(x.t[4]), "+v"(x.t[5]));
}
template <typename T>
__device__ __forceinline__ void lead_unpack(const LeadTile<T>& x, T (&v)[12]) {
  constexpr int n = Vec16<T>::n;
#pragma unroll
  for (int c = 0; c < LeadTile<T>::NT; ++c) {
#pragma unroll
    for (int e = 0; e < n; ++e) v[c * n + e] = x.t[c][e];
  }
}

// A wavefront-uniform value in scalar registers OF ITS OWN.  The kernel argument arrives through one wide scalar load,
// and the compiler keeps what it needs from it as sub-registers of that 16-register tuple: when scalar registers run
// out the WHOLE tuple goes to the lanes of a spill register and every use of one member brings all sixteen back
// (16 v_readlane for a pointer test).  Values that went through here are allocated - and, if need be, spilled - one by one.
template <typename U>
__device__ __forceinline__ U own_sgpr(U v) {
  asm volatile("" : "+s"(v));
  return v;
}

// ... for a pointer into global memory (a kernel argument's pointer is known to be one; behind the asm it no longer
// would be, and its accesses would turn into flat_load / flat_store)
template <typename U>
__device__ __forceinline__ U* own_sgpr_global(U* p) {
  uintptr_t v = (uintptr_t)p;
  asm volatile("" : "+s"(v));
  return (U*)(__attribute__((address_space(1))) U*)v;
}

// One of four values by the lane's place in its quad, as three selects on the values.  (Written as a chain of
// conditional expressions the compiler emits a ladder of nested exec-mask blocks with one move in each; the wavefront
// that runs this kernel alone on its SIMD pays full latency for every instruction of such a ladder.)
template <typename T>
__device__ __forceinline__ T quad_pick(int kp, T v0, T v1, T v2, T v3) {
  T v = v3;
  v = kp == 2 ? v2 : v;
  v = kp == 1 ? v1 : v;
  v = kp == 0 ? v0 : v;
  return v;
}

// wave_sum_f64 of K independent values, stage by stage: the K moves of a stage stand between a sum's addition and the
// DPP move that reads it, where one sum after the other pays the wait states of every move.  Each sum keeps
// wave_sum_f64's order of additions.
template <int K>
__device__ __forceinline__ void wave_sum_f64_staged(double (&v)[K]) {
  auto stage = [&](auto ctrl) {
    double o[K];
#pragma unroll
    for (int k = 0; k < K; ++k) o[k] = quad_xor<decltype(ctrl)::value>(v[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += o[k];
  };
  stage(std::integral_constant<int, 0xB1>{});
  stage(std::integral_constant<int, 0x4E>{});
  stage(std::integral_constant<int, 0x141>{});  // row_half_mirror
  stage(std::integral_constant<int, 0x140>{});  // row_mirror
  int lo[K], hi[K];
  double s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const long long b = __double_as_longlong(v[k]);
    lo[k] = (int)(b & 0xFFFFFFFFll);
    hi[k] = (int)(b >> 32);
    s[k] = 0.0;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int l = __builtin_amdgcn_readlane(lo[k], 16 * r), h = __builtin_amdgcn_readlane(hi[k], 16 * r);
      s[k] += __longlong_as_double(((long long)h << 32) | (unsigned int)l);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = s[k];
}

// ms_pred_update for this kernel (every step it hands over has converged).  While the fitted recurrence is in use and
// predicted the step to better than 1e-3 (ms_pred_update's poly_eval == false) no polynomial order is measured: every
// em[p] is 3.0e38f there, the order-choice loop ends at nxt = pmax and eb = 3.0e38f.  That case is written out straight -
// the error of the fit, keep or refit, the two decisions, the level shift, in ms_pred_update's order and with its
// expressions; every other case is ms_pred_update itself.
template <typename T, int NC>
__device__ __forceinline__ void mso_pred_update(MsPred<T, NC>& Q, int order, int predictor, int lane, const T* Xs,
                                                MsStamps& stamps) {
  // (wavefront-uniform by construction; said so, so that the two forms are two branches and not two masked passes)
  if (!__builtin_amdgcn_readfirstlane((int)(order == MS_ORDER_LP && Q.lp_good))) {
    ms_pred_update<T>(Q, order, KR_ST_CONVERGED, predictor, lane, Xs, stamps);
    return;
  }
#ifdef KR_MS_STAMPS
  unsigned long long tpu;
  KR_STAMP(tpu);
#endif
  float err_lp = 0.f;
  if (Q.lp_have) {
#pragma unroll
    for (int q = 0; q < MS_EPL; ++q) {
      const int e = lane + q * WAVE;
      if (e < MS_NE) {
        const double x = (double)Xs[e];
        double b[NC];
        lp_basis<T, NC>(Q.Hx[q], b);
        err_lp = fmaxf(err_lp, update_ratio(x - lp_eval<NC>(Q.lpa, b), x));
      }
    }
  }
  const float em_lp = wave_max_nonneg(err_lp);
#ifdef KR_MS_STAMPS
  KR_STAMP_ADD(stamps.a1, tpu);  // error of the fit in use
#endif
  const bool lp_tested = Q.lp_have;
  const bool keep_fit = lp_tested && em_lp < 1.0e-3f && Q.lp_age < 3;
  Q.lp_age = keep_fit ? Q.lp_age + 1 : 0;
  Q.lp_have = keep_fit;
  if (!keep_fit && predictor >= MS_ORDER_LP && Q.avail >= NC - 1) {
    double Sn[lp_nsum<NC>()];
#pragma unroll
    for (int k = 0; k < lp_nsum<NC>(); ++k) Sn[k] = 0.0;
#pragma unroll
    for (int q = 0; q < MS_EPL; ++q) {
      const int e = lane + q * WAVE;
      if (e < MS_NE) {
        const double x = (double)Xs[e];
        double b[NC];
        lp_basis<T, NC>(Q.Hx[q], b);
        const double w = (double)__builtin_amdgcn_rcpf(fmaxf(fabsf((float)x), 1.0f));
        lp_accumulate<NC>(Sn, b, x, w);
      }
    }
    if constexpr (sizeof(T) == 8) {
      wave_sum_f64_staged(Sn);
    } else {
#pragma unroll
      for (int k = 0; k < lp_nsum<NC>(); ++k) Sn[k] = wave_sum_f64(Sn[k]);
    }
    double a[NC];
    if (lp_solve<NC>(Sn, a)) {
#pragma unroll
      for (int k = 0; k < NC; ++k) Q.lpa[k] = a[k];
      Q.lp_have = true;
    }
  }
#ifdef KR_MS_STAMPS
  KR_STAMP_ADD(stamps.a2, tpu);  // refit (every fourth step)
#endif
  Q.next_order = Q.avail < predictor ? Q.avail : (predictor < MS_HLEV ? predictor : MS_HLEV - 1);  // pmax
  Q.lp_good = lp_tested && Q.lp_have && em_lp < 1.0e-3f;
  if (lp_tested && Q.lp_have && (em_lp < 3.0e38f || Q.lp_good)) Q.next_order = MS_ORDER_LP;
#ifdef KR_MS_STAMPS
  stamps.osum += (unsigned long long)order; stamps.olast = order;
  for (int p = 0; p < MS_HLEV; ++p) stamps.em[p] = 3.0e38f;
  KR_STAMP_ADD(stamps.a3, tpu);  // choice of the next order
#endif
#pragma unroll
  for (int q = 0; q < MS_EPL; ++q) {
    const int e = lane + q * WAVE;
#pragma unroll
    for (int k = MS_HLEV - 1; k > 0; --k) Q.Hx[q][k] = Q.Hx[q][k - 1];
    if (e < MS_NE) Q.Hx[q][0] = Xs[e];  // MS_YP == 19: Xs is the same flat vector
  }
  if (Q.avail < MS_HLEV - 1) ++Q.avail;
}

// The park of the fp64 kernels at one wavefront per SIMD (mso_sim_kernel, PARK): one tile of leading slots in registers,
// lane per grid point like the plain persistent kernel's regP.  Free functions, called from discarded-or-not
// `if constexpr` branches only, so that the kernels without a park do not even see a closure of them.
template <typename T>
struct MsoPark { T v[MS_NPL][12]; };
struct MsoNoPark { };
// (every lane reads: a lane past the last grid point takes that one again, and no read stands under a mask)
template <typename T>
__device__ __forceinline__ void mso_park_take(MsoPark<T>& park, const T* lt, int lane, int N) {
#pragma unroll
  for (int q = 0; q < MS_NPL; ++q) {
    const int j = lane + q * WAVE;
    lds_load_vec<T, 12>(lt + (size_t)(j < N ? j : N - 1) * 12, park.v[q]);
  }
}
template <typename T>
__device__ __forceinline__ void mso_park_restore(const MsoPark<T>& park, T* lt, int lane, int N) {
#pragma unroll
  for (int q = 0; q < MS_NPL; ++q) {
    const int j = lane + q * WAVE;
    if (j < N) lds_store_vec<T, 12>(lt + (size_t)j * 12, park.v[q]);
  }
  wave_sync_lds();
}

#ifdef KR_MS_STAMPS
struct MsoStats { unsigned long long total = 0, sweeps = 0, merged = 0, quick = 0, chord = 0, rejects = 0, retries = 0, rebuilds = 0, t_sweep = 0, t_alg = 0, t_pred = 0, t_verdict = 0, t_cond = 0, t_fin = 0, t_upd = 0, t_v1 = 0, t_v2 = 0, t_c1 = 0, t_c2 = 0, t_copy = 0; };
#endif

// OCC: workgroups per CU the register allocation leaves room for.  OCC = 2 (fp32, batches beyond one rod per SIMD)
// runs two rods on every SIMD, whose issue-bound sweeps and latency-bound algebra overlap (as kr_ms_impl.hpp's OCC).
// PSRC: where a rod's constants come from - the kernel argument itself (RodConst<T>, all rods alike) or a per-rod
// table (RodTable<T>, kr_tab_impl.hpp); see rod_src_row (rod_device.hpp).
// PSRC = RodTableLoads<T> (kr_load_impl.hpp): the tip wrench of step t is loads[rod][t].  A merged sweep holds two time
// levels - the verifying lanes close step tA - 1 against ITS wrench while the forward-difference lanes condense step tA -
// so there are two sets of six slots, step t's in set t & 1: set 0 is the cold block's own F_tip / M_tip, set 1 lies in
// the part of the record area this kernel leaves unused (it keeps 12 of a record's HS slots, the odd tile).  Every read
// of the wrench names the step it belongs to (cold_of), so a rejected verification, the rebuild, a plain step and a chord
// update find their step's values whatever sweep they run in; a set is written once per step, at the hand-over.
// PSRC = RodTableBnd<T> (kr_bnd_impl.hpp): the same with the whole boundary of step t, bnd[rod][t] = p0 h0 q0 w0 F_tip
// M_tip: two sets of 19 slots, set 0 the cold block's first 19.  The base slots are read by ms_pred_guess only (row 0 of
// the step's unknowns), which takes cold_of(its step); the areas Xs / XsB swap roles without a copy, so the step under
// verification keeps the row 0 it was given.
// PSRC = RodTableBndKp<T> (kr_kp_impl.hpp): the boundary kernel that also writes kp[tB][rod][k], the complete record of
// the k-th marked grid point, wherever a verifying lane holds the record of a marked point: in every trip (complete,
// lean and predicated alike - a lean step stores nothing else there) and, for the last grid point, in the verdict's
// block beside the tip.  A rejected sweep has written its key points; the sweep that verifies the step again, or the
// take-over launch from resume[rod] on, overwrites them - the tip's rule.
template <typename T, bool DIAG, int HS, int OCC = 1, typename PSRC = RodConst<T>>
__global__ __launch_bounds__(WAVE * MS_WPB, OCC) void mso_sim_kernel(const PSRC Pa, const SimArgs<T> A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int N = rod_src_N<T>(Pa);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = threadIdx.x / WAVE;
  const int64_t rod = (int64_t)blockIdx.x * MS_WPB + wv;
  if (rod >= A.B) return;  // whole wavefront; there is no workgroup barrier in this kernel
  const auto& Pc = rod_src_row<T>(Pa, rod);
  const size_t rod_elems = (size_t)N * KR_SLOTS;
  // the members of the argument every step uses (the rest is read where a cold path needs it)
  T* const a_states = own_sgpr_global(A.states);
  const int64_t a_slot_elems = own_sgpr(A.slot_elems);
  const int a_ring = own_sgpr(A.ring);
  T* const a_tip = own_sgpr_global(A.tip);
  int32_t* const a_status = own_sgpr_global(A.status);
  const int a_residual_test = own_sgpr(A.residual_test), a_predictor = own_sgpr(A.predictor);
  const T hc1 = own_sgpr(A.hc1), hc2 = own_sgpr(A.hc2);
  const int T_steps = own_sgpr((int)A.T_steps);  // (step indices are 32-bit: the host refuses a call of 2^31 steps or more)
  // key-point records (PSRC = RodTableBndKp<T>): pointer, K and the mask of the marked grid points are kernel arguments
  using KPSRC = rod_src_keypoints<T, PSRC>;
  constexpr bool KP = KPSRC::value;
  // the forms of the step's ends that only the fp64 kernels at one wavefront per SIMD take (the others keep their text)
  constexpr bool TRIM = OCC == 1 && sizeof(T) == 8 && MSO_LAG == 1;
  // ... and that keep the tile a verification overwrites in registers instead of copying every accepted tile to HBM
  constexpr bool PARK = TRIM && KR_MSO_PARK != 0;
  const unsigned long long kp_lo = KPSRC::lo(Pa), kp_hi = KPSRC::hi(Pa);
  const MsLds<T> L = ms_carve<T, HS>(reinterpret_cast<T*>(smem_raw) + (size_t)wv * mso_lds_elems<T, HS>(N), N, true, false);
  T* const Es = L.Es;
  T* const XB = L.XB;
  T* const Tm = L.Tm;
  // The unknowns of the step the forward-difference lanes work on (Xs) and of the step the verifying lanes re-integrate
  // (XsB), [P][19] each, are two areas that change roles when a step is handed over: nothing is copied.  Which is which
  // is an offset from one base (not a select between two pointers, DESIGN rule 4: the accesses stay LDS accesses).
  T* const X0 = L.Xs;
  const ptrdiff_t X_d = (L.c12 + (size_t)N * 12) - L.Xs;
  int xsel = 0;
  T* Xs = X0;
  T* XsB = X0 + X_d;
  T* const EsB = Es + MSO_B0 * MS_YP;     // their end states: the Es slots of lanes 58..61
  const MsRole R = ms_role(lane, N);
  const int iv = R.iv, col = R.col;
  const bool isA = lane < MSO_B0;
  const bool isB = lane >= MSO_B0 && lane < MSO_B0 + MS_P;
  const int ib = isB ? lane - MSO_B0 : 0;
  const int s_l = isB ? ms_interval_start(ib, R.sbase, R.srem) : R.s_i;
  const int len_l = isB ? R.sbase + (ib < R.srem ? 1 : 0) : R.len_i;
  // (key points) the interval a verifying lane walks, one grid point per trip: bit kk of kp_marks = grid point s_l + kk is
  // marked (an interval has at most 32 grid points at N <= 128), kp_rank0 = the marked points below s_l
  unsigned kp_marks = 0;
  int kp_rank0 = 0;
  if constexpr (KP) {
    kp_marks = keypoint_window(kp_lo, kp_hi, s_l);
    kp_rank0 = keypoint_rank(kp_lo, kp_hi, s_l);
  }
  ms_cold_fill<T>(rod_src_mem<T>(Pa, rod), L.cold, lane);
  wave_sync();

  auto slot_ptr = [&](int slot) -> T* { return a_states + (int64_t)slot * a_slot_elems + rod * rod_elems; };
  auto state_ptr = [&](int k) -> T* { return slot_ptr(a_ring ? k % 3 : k); };  // (cold paths; the sweep's slot is rsA)
  // The BDF2 history (knode.py:74-75) is kept RAW: two tiles of leading slots (q w v u of every grid point), tile (t & 1)
  // for the state at time level t.  A lane forms the record it needs - hc1 * newest + hc2 * older, then av / au - itself,
  // right after the read: 30 instructions that every lane of the wavefront shares, where a precombined record cost the
  // four verifying lanes the same 30 instructions in a divergent block of their own plus 9 more 16-byte LDS stores and
  // 6 loads per trip (a wavefront-instruction costs the same with 4 lanes active as with 64, and an LDS store ~13 cycles).
  T* const lead0 = L.c12;                    // [N][12] states at even time levels
  const ptrdiff_t lead_d = L.hist - L.c12;  // states at odd time levels: the first 12 N elements of the record area
  // (offset arithmetic, not a select between two pointers: the compiler turned such selects into a table in scratch)
  auto lead_of = [&](int t) -> T* { return lead0 + (ptrdiff_t)(t & 1) * lead_d; };
  // both tiles of step t's history from the states in HBM
  auto rebuild = [&](int t) {
    const T* cur = state_ptr(t);
    const T* prv = t > 0 ? state_ptr(t - 1) : (A.prev_init ? A.prev_init + rod * rod_elems : cur);
    T* const lc = lead_of(t);
    T* const lp = lead_of(t - 1);
    for (int j = lane; j < N; j += WAVE) {
      T cv[12], pv[12];
      load_hist_vec<T, 12>(cur + (size_t)j * KR_SLOTS, cv);
      load_hist_vec<T, 12>(prv + (size_t)j * KR_SLOTS, pv);
      lds_store_vec<T, 12>(lc + (size_t)j * 12, cv);
      lds_store_vec<T, 12>(lp + (size_t)j * 12, pv);
    }
    wave_sync();
  };
  // The park (PARK): what a roll-back needs is ONE generation of ONE tile.  The merged sweep that verifies step tB
  // writes level tB + 1 over level tB - 1 in lead_of(tB + 1), grid point by grid point (the trips' store blocks and the
  // verdict's block for the last grid point), and nothing else in either tile: level tB in lead_of(tB) stands.  So the
  // tile that is about to be overwritten is taken into registers, lane per grid point like the plain persistent
  // kernel's regP, at the hand-over that makes the coming sweep a merged one; a rejected verification writes it back,
  // and no accepted state of a lean step goes to HBM at all.  The values are the raw copies rebuild() would have read.
  std::conditional_t<PARK, MsoPark<T>, MsoNoPark> park;
  static_assert(!PARK || MS_NPL * WAVE >= 128, "the park holds every grid point the planner serves (one_wave_range)");
  if constexpr (PARK) {
#pragma unroll
    for (int q = 0; q < MS_NPL; ++q) {
#pragma unroll
      for (int c = 0; c < 12; ++c) park.v[q][c] = T(0);
    }
  }
  // the cold slots a step rewrites: [W0, W0 + WN) - the wrench (loads), the whole boundary (bnd) or none
  using WSRC = rod_src_step_slots<T, PSRC>;
  constexpr int W0 = WSRC::first, WN = WSRC::count;
  constexpr bool LOADS = WN > 0;
  static_assert(!LOADS || (W0 + WN == CD_TDIRS && (W0 == CD_FTIP || W0 == CD_P0)), "the per-step slots end with F_tip, M_tip");
  // the second set lives behind the odd tile in the record area: N (HS - 12) free slots, and the planner serves
  // N >= 2 MS_P + 1 (one_wave_range) - 54 (fp64) or 72 (fp32) slots for the 6 or 19 of a set
  static_assert(!LOADS || (HS >= 18 && (2 * MS_P + 1) * (HS - 12) >= WN), "the second set lives behind the odd tile in the record area");
  // the cold block as step t sees it: L.cold itself, or (loads, odd t) moved so that W0 .. W0 + WN - 1 fall on the second
  // set (offset arithmetic like lead_of; only those slots may be read through it)
  const ptrdiff_t wr_d = LOADS ? (L.hist + (size_t)N * 12) - (L.cold + W0) : 0;
  auto cold_of = [&](int t) -> const T* {
    if constexpr (LOADS) return L.cold + (ptrdiff_t)(t & 1) * wr_d;
    else return L.cold;
  };
  // where ms_pred_guess finds the base state of step t (row 0 of the unknowns): the step's set when a step rewrites it
  auto base_of = [&](int t) -> const T* {
    if constexpr (LOADS && W0 < CD_FTIP) return L.cold + (ptrdiff_t)(t & 1) * wr_d;
    else return L.cold;
  };
  const T* wrench = nullptr;  // loads only: [T_steps][WN] of this rod
  if constexpr (LOADS) wrench = WSRC::hist(Pa) + rod * A.T_steps * WN;
  const T* ctl = A.ctl + rod * A.T_steps * 4;
  auto load_fc = [&](int t) -> V3<T> {  // rhoA g + tendon force of step t (cosserat_ode.py:151,195)
    V3<T> tf{T(0), T(0), T(0)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const T tt = ctl[(size_t)t * 4 + k];
      tf.x += tt * L.cold[CD_TDIRS + k * 3 + 0];
      tf.y += tt * L.cold[CD_TDIRS + k * 3 + 1];
      tf.z += tt * L.cold[CD_TDIRS + k * 3 + 2];
    }
    return {L.cold[CD_RHOAG] + tf.x, L.cold[CD_RHOAG + 1] + tf.y, L.cold[CD_RHOAG + 2] + tf.z};
  };

  const T* s0 = state_ptr(0);
  const T* sp0 = A.prev_init ? A.prev_init + rod * rod_elems : s0;
  MsPred<T> Q;
  double* img = A.pred_io ? A.pred_io + (size_t)rod * MS_PRED_ROWS * WAVE : nullptr;
  if (img && A.pred_load) ms_pred_load<T>(Q, img, lane);
  else ms_pred_init<T>(Q, lane, R, s0, sp0, A.prev_init != nullptr, a_predictor);
  V3<T> vlast, ulast;  // z of the last grid point is never touched by a sweep (cosserat_ode.py:198-201)
  {
    const T* cl = s0 + (size_t)(N - 1) * KR_SLOTS;
    vlast = {cl[SL_V], cl[SL_V + 1], cl[SL_V + 2]};
    ulast = {cl[SL_U], cl[SL_U + 1], cl[SL_U + 2]};
  }
  const T tol = own_sgpr(A.tol), tolA = own_sgpr(A.tolA), fd_eps = own_sgpr(A.fd_eps);
  const int maxit = own_sgpr(A.maxit);
  T kappa = Q.kappa;
  T Gguess = lane < 6 ? A.G[rod * 6 + lane] : T(0);
  MsStamps stamps;
#ifdef KR_MS_STAMPS
  MsoStats st;
  unsigned long long t_begin, tq;
  KR_STAMP(t_begin);
  tq = t_begin;
#endif

  rebuild(0);

  // ---- state of the iteration -----------------------------------------------------------------------------------
  int tA = 0;            // step the forward-difference lanes work on (unknowns: Xs)
  int rsA = 0;           // slot of `states` the state at time level tA goes to (ring: tA mod 3, advanced with tA, never divided)
  bool merged = false;   // the coming sweep also re-integrates step tA - 1 from XsB and streams it out
  int it = 0;            // forward-difference sweeps spent on step tA
  int order = Q.next_order;
  bool retried = false;  // step tA has been restarted from the reference's warm start
  T dn_prev = T(-1);     // update norm of the previous iteration of step tA
  bool have_fac = false, below = false;
  float amp = -1.f;      // update norm per unit of residual norm at the last condensation
  // of the step under verification (tA - 1)
  T dnB = T(-1);
  float ampB = -1.f;
  bool belowB = false;
  int itB = 0, orderB = 0;
  bool pred_skip = false;  // the predictor has already consumed step tA (a verifying sweep of it was rejected)
  bool reverify = false;   // the coming merged sweep verifies step tA - 1 for the second time (after a chord update)
  int resume_at = T_steps;
  T Xreg[MS_P - 1][2];
#pragma unroll
  for (int g = 0; g < MS_P - 1; ++g) Xreg[g][0] = Xreg[g][1] = T(0);
  // (tensions are requested one step before they are needed: a load from HBM takes longer than what lies between
  // the hand-over of a step and the sweep that follows)
  V3<T> fcA = load_fc(0), fcB = fcA;
  V3<T> fcN = load_fc(T_steps > 1 ? 1 : 0);
  T wN = T(0);  // loads, lanes 0..WN-1: the values of step tA + 1, requested like fcN
  if constexpr (LOADS) {
    if (lane < WN) {
      L.cold[W0 + lane] = wrench[lane];  // step 0 (set 0; the fences of the start values below come before any read)
      wN = wrench[(size_t)(T_steps > 1 ? 1 : 0) * WN + lane];
    }
    if constexpr (W0 < CD_FTIP) wave_sync_lds();  // (the base slots are read back by other lanes in ms_pred_guess)
  }
  // av = hk_a + hk_b v_h, au = hk_c u_h (diagonal material matrices): kept in registers so that forming a history
  // record inside a sweep does not go back to the parameter table
  static_assert(DIAG, "the in-sweep history record assumes diagonal material matrices");
  T hk_a[3], hk_b[3], hk_c[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    hk_a[c] = L.cold[CD_KSEI + 4 * c] * L.cold[CD_KSEV + c];
    hk_b[c] = -L.cold[CD_KSEI + 4 * c] * L.cold[CD_BSE + 4 * c];
    hk_c[c] = -L.cold[CD_KBTI + 4 * c] * L.cold[CD_BBT + 4 * c];
  }

  ms_pred_guess<T>(Q, order, lane, base_of(0), Xs);
  wave_sync_lds();
  if (order <= 0 && lane < 6) Xs[0 * MS_YP + 7 + lane] = Gguess;  // caller's guess (knode.py:67,89)
  wave_sync_lds();

  // p rows, scaled update norm and the per-lane pieces of an update of the unknowns X from base end states Eb(g)
  // (A: Es slot of the interval's unperturbed lane; B: EsB) - the tail both the chord and the Newton update share.
  // Returns the norm; the updated unknowns are left in U, one value per lane and family: newPG for the owner of a p row
  // or of a component of G (no lane owns both), newY[g - 1] for the owner of a row of Y_g.  Other lanes hold there
  // what the clamped reads gave them; apply() stores under the owners' masks.
  struct Upd { T newPG, newY[MS_P - 1]; };

  while (true) {
    const bool runA = tA < T_steps;  // (false only for the sweep that verifies the last step)
    const int tB = tA - 1;
    // ---- start state of this lane -------------------------------------------------------------------------------
    T yr[19];
    {
      const T* src = isB ? XsB + ib * MS_YP : Xs + iv * MS_YP;
#pragma unroll
      for (int q = 0; q < 19; ++q) yr[q] = src[q];
    }
    const T hstep = (isA && col > 0) ? fd_eps * fmax(fabs(Xs[iv * MS_YP + (R.comp > 0 ? R.comp : 3)]), T(1)) : T(1);
    // (comp is -1 in every lane that perturbs nothing, the verifying and the idle lanes included.  Compared afresh in
    //  every sweep: as loop invariants the sixteen masks q == comp lived in 32 scalar registers, i.e. in a spill register)
    int comp = R.comp;
    asm volatile("" : "+v"(comp));
#pragma unroll
    for (int q = 3; q < 19; ++q) yr[q] += q == comp ? hstep : T(0);
    RodState<T> y = rows_to_state(yr);
    const V3<T> fc = isB ? fcB : fcA;
    // the verifying lanes run MSO_LAG grid points ahead of the forward-difference lanes that consume their records
    const int lag = (isA && merged) ? MSO_LAG : 0;
    const bool act = isB ? merged : (isA && runA);
    const int trips = R.lmax + ((merged && runA) ? MSO_LAG : 0);
    T* const out_rod = slot_ptr(rsA);  // state tB + 1 (used by the verifying lanes only)
    T* const kp_out = KPSRC::at(Pa, tB, A.B, rod);  // ... and its key-point records, [K][KR_SLOTS] (key-point kernels only)
    // grid point this lane evaluates in trip k (clamped to its interval: lanes outside their range keep evaluating
    // their first / last point and do not advance)
    auto point_of = [&](int k) -> int {
      const int kk = k - lag;
      return s_l + (kk < 0 ? 0 : (kk < len_l ? kk : len_l - 1));
    };
    // History record of this lane's step at grid point j from the two tiles.  The forward-difference lanes work on step
    // tA (newest state: tile tA & 1), the verifying lanes on step tB = tA - 1 (newest: the other tile; at the grid points
    // they have not reached yet tile tA & 1 still holds the state at level tB - 1, behind them the state they are
    // producing).  The tile addresses differ per lane; the arithmetic is the same for all.
    const T* const lead_n = lead_of(isB ? tB : tA);      // this lane's newest state
    const T* const lead_o = lead_of(isB ? tB + 1 : tB);  // ... and the one before it (same parity as two levels on)
    // (the rounding of a record is written out - one product, one fused multiply-add - so that it does not depend on
    //  where the compiler's contraction finds the two halves: the merged trip forms them a store block apart)
    auto hist_older = [&](const T (&lb)[12], T (&pb)[12]) __attribute__((always_inline)) {
#pragma unroll
      for (int c = 0; c < 12; ++c) pb[c] = hc2 * lb[c];
    };
    auto hist_newest = [&](const T (&la)[12], const T (&pb)[12]) __attribute__((always_inline)) -> RodHist<T> {
      T raw[12];
#pragma unroll
      for (int c = 0; c < 12; ++c) raw[c] = fma(hc1, la[c], pb[c]);
      RodHist<T> h;
      h.qh = {raw[0], raw[1], raw[2]};
      h.wh = {raw[3], raw[4], raw[5]};
      h.vh = {raw[6], raw[7], raw[8]};
      h.uh = {raw[9], raw[10], raw[11]};
      h.av = {hk_b[0] * raw[6] + hk_a[0], hk_b[1] * raw[7] + hk_a[1], hk_b[2] * raw[8] + hk_a[2]};  // (Kse + c0 Bse)^-1 (Kse v* - Bse v_h)
      h.au = {hk_c[0] * raw[9], hk_c[1] * raw[10], hk_c[2] * raw[11]};                                       // -(Kbt + c0 Bbt)^-1 Bbt u_h
      return h;
    };
    auto hist_form = [&](const T (&la)[12], const T (&lb)[12]) __attribute__((always_inline)) -> RodHist<T> {
      T pb[12];
      hist_older(lb, pb);
      return hist_newest(la, pb);
    };
    auto hist_at = [&](int j) __attribute__((always_inline)) -> RodHist<T> {
      T la[12], lb[12];
      lds_load_vec<T, 12>(lead_n + (size_t)j * 12, la);
      lds_load_vec<T, 12>(lead_o + (size_t)j * 12, lb);
      return hist_form(la, lb);
    };
    RodHist<T> hst = hist_at(point_of(0));
    // a step of a ring call whose state nobody reads as a complete record (the last three states of a call stay complete)
    const bool lean = a_ring && tB + 4 <= T_steps;
    if (!merged) {
      // plain forward-difference sweep (start-up, rough inputs, after a rejection): the branch-free body of
      // kr_ms_impl.hpp, two grid points per trip so that the scheduler overlaps neighbours; every interval has
      // sbase or sbase + 1 segments, so only the last grid point needs a predicate
      auto fd_point = [&](int j, T dsl) __attribute__((always_inline)) {
        RodState<T> k1;
        V3<T> v, u;
        ode_eval<T, DIAG>(Pc, y, hst, fc, k1, v, u);
        hst = hist_at(j + 1);  // (grid point N - 1 has leading slots too; its record is not used)
        y = state_axpy(y, dsl, k1);
      };
#pragma unroll 2
      for (int t = 0; t < R.sbase; ++t) fd_point(R.s_i + t, Pc.ds);
      if (R.srem) fd_point(R.s_i + (R.len_i > R.sbase ? R.sbase : R.sbase - 1), R.len_i > R.sbase ? Pc.ds : T(0));
    } else {
      // one trip of the merged sweep.  FULL: every active lane is inside its interval (no predicates, no clamped
      // indices) - true for the trips MSO_LAG .. sbase - 1, i.e. all but the first and last few.
      //
      // What a lone wavefront must not do is wait for the tile round trip (the verifying lanes' six stores, then the reads
      // of the next grid point's leading slots) with nothing else to issue.  The LDS returns in order, so the first use of
      // ANY read issued behind the stores waits for the stores too.  Hence, per trip:
      //   * the OLDER tile of the next grid point is read at the head of the trip and its half of the record (hc2 * older)
      //     is formed IN FRONT of the store block: no lane's older tile changes at that grid point before the next trip
      //     (static during the sweep for the forward-difference lanes; a verifying lane replaces slot j + 1 in trip k + 1)
      //   * the NEWEST tile is read right behind the stores and consumed behind the rest of this trip's arithmetic (the
      //     bulk of ode_eval and the Euler update need only the current record)
      // In a predicated trip past a lane's interval the clamped older read is that of the slot the lane has just written,
      // taken before the store: such a lane's record feeds an evaluation that is multiplied by dsl = 0.
      T* const lead_w = lead_of(tB + 1);               // the tile the verifying lanes write: state tB + 1 over state tB - 1
#if KR_MSO_TRIP_CARRY
      // (probe) 2 / h.h of the state the coming evaluation sees (behind the forward-difference perturbation), carried from trip to trip
      T rs = rot_scale(y.h0, y.h1, y.h2, y.h3);
#endif
      auto trip = [&](int k, auto full_tag, auto lean_tag) __attribute__((always_inline)) {
        constexpr int FORM = decltype(full_tag)::value;  // 0: predicated, 1: FULL, 2: trip 0
        constexpr bool FULL = FORM == 1;
        constexpr bool FIRST = TRIM && FORM == 2;
        constexpr bool LEAN = decltype(lean_tag)::value;  // (FULL trips: the loop exists once per value; others test `lean`)
        const int kk = k - lag;
        // (trip 0: no forward-difference lane is live - kk = -1 - and every lane stands at the start of its interval; the
        //  verifying lanes move on to their second grid point, the others read the records of their first again: functions
        //  of isB alone, not of the clamps)
        const bool live = FIRST ? isB : FULL ? act : (act && kk >= 0 && kk < len_l);
        const int j = FIRST ? s_l : FULL ? s_l + kk : point_of(k);
        const int eo = j * 12;                                       // elements in front of grid point j in a tile
        const int en = FIRST ? (s_l + ((isB && len_l > 1) ? 1 : 0)) * 12 : FULL ? eo + 12 : point_of(k + 1) * 12;  // ... of the grid point of the next trip
        T la[12], lb[12], pb[12];
        // (one wait per tile in the fp64 kernels.  fp32 keeps the value-by-value reads: its staircase is three steps, and
        //  with the pins the fp32 headline call measured 0.7 % SLOWER in every one of three rounds, 52.9 against 53.3 M)
#ifdef KR_MSO_PROBE_EARLY_READS
        constexpr bool TUPLES = false;
#else
        constexpr bool TUPLES = KR_MSO_TRIP_WAITS && MSO_LAG < 2 && OCC == 1 && sizeof(T) == 8;
#endif
        LeadTile<T> ta, tb;
        if constexpr (TUPLES) {
          lds_load_lead<T>(lead_o + en, tb);
          // (the reads stay at the head of the trip: behind a pin alone the scheduler sinks them to four instructions in
          //  front of their wait.  Only LDS accesses are held - a full barrier here cost 0.3 k ticks per step of the 0.9 k.)
          __builtin_amdgcn_sched_barrier(KR_SCHED_ALL_BUT_DS);
        } else if constexpr (MSO_LAG >= 2) {
          // what the next trip reads was written a trip ago - requested now, under the arithmetic of this one
          lds_load_vec<T, 12>(lead_n + en, la);
          lds_load_vec<T, 12>(lead_o + en, lb);
        } else {
          lds_load_vec<T, 12>(lead_o + en, lb);
#ifdef KR_MSO_PROBE_EARLY_READS
          // TIMING PROBE, results are wrong: the newest tile too is read in front of the store block, so the
          // forward-difference lanes see leading slots that are two time levels old
          if constexpr (FULL) lds_load_vec<T, 12>(lead_n + en, la);
#endif
        }
        RodState<T> k1;
        V3<T> v, u;
#if KR_MSO_TRIP_CARRY
        ode_eval_s<T, DIAG>(Pc, y, hst, fc, k1, v, u, rs);
#else
        ode_eval<T, DIAG>(Pc, y, hst, fc, k1, v, u);
#endif
        // (formed in front of the verifying lanes' block: behind it the wait for the reads would also wait for its stores)
        if constexpr (MSO_LAG >= 2) {
          hst = hist_form(la, lb);
          // (pinned: the compiler otherwise sinks the arithmetic - and with it the wait - behind the block)
          asm volatile("" : "+v"(hst.qh.x), "+v"(hst.qh.y), "+v"(hst.qh.z), "+v"(hst.wh.x), "+v"(hst.wh.y), "+v"(hst.wh.z));
          asm volatile("" : "+v"(hst.vh.x), "+v"(hst.vh.y), "+v"(hst.vh.z), "+v"(hst.uh.x), "+v"(hst.uh.y), "+v"(hst.uh.z));
          asm volatile("" : "+v"(hst.av.x), "+v"(hst.av.y), "+v"(hst.av.z), "+v"(hst.au.x), "+v"(hst.au.y), "+v"(hst.au.z));
        } else {
          // (pinned: the products - and the wait for the older tile - stay in front of the block)
          if constexpr (TUPLES) {
            // (the one wait comes where the asm stands.  v and u need nothing from the tile: named in front of it they
            //  are finished under the reads, which keeps the cover of the last read what the staircase's first step had)
            asm volatile("" ::"v"(v.x), "v"(v.y), "v"(v.z), "v"(u.x), "v"(u.y), "v"(u.z));
            lead_pin(tb);
            lead_unpack<T>(tb, lb);
          }
          hist_older(lb, pb);
          asm volatile("" : "+v"(pb[0]), "+v"(pb[1]), "+v"(pb[2]), "+v"(pb[3]), "+v"(pb[4]), "+v"(pb[5]), "+v"(pb[6]), "+v"(pb[7]),
                            "+v"(pb[8]), "+v"(pb[9]), "+v"(pb[10]), "+v"(pb[11]));
        }
        if (isB && live) {
          // the accepted-to-be state of step tB at grid point j: to HBM; its leading slots replace those of the state
          // two levels back in LDS (this lane has already read them: its record of grid point j was formed a trip ago)
          T rec[KR_SLOTS];
          record_from(y, v, u, rec);
          T lead[12];
#pragma unroll
          for (int c = 0; c < 12; ++c) lead[c] = rec[c];
          // On a 3-slot ring nobody reads the states of the call's interior steps - except this kernel when it rolls a
          // step back and the kernel launched behind it when it takes a rod over, and both need only the twelve leading
          // slots of every record (v and u of the last grid point, which no sweep touches, are among them) plus the full
          // records at the interval starts (predictor).  The leading slots are what this sweep leaves in its tile: once the step is accepted
          // the whole tile goes out in one pass of the wavefront (below, 2 x 6 stores from all lanes instead of 6 stores
          // from four lanes in every trip; with the park not even that - the tiles are flushed when a rod gives up); interior records of interior steps store nothing here (an interval start is
          // the grid point of trip 0, the last grid point's record is the verdict's and as lean as these: the trailing
          // predicated trips are interior too), all others only their remaining sixteen slots or, in a predicated trip, the whole record.
          if constexpr (FULL) {
            if constexpr (!LEAN) {  // the rest of the record (p h n m); its leading slots follow with the tile
              T rest[KR_SLOTS - 12];
#pragma unroll
              for (int c = 0; c < KR_SLOTS - 12; ++c) rest[c] = rec[12 + c];
              store_vec<T, KR_SLOTS - 12>(out_rod + (size_t)j * KR_SLOTS + 12, rest);
            }
          } else {
            if (!(lean && k >= R.sbase)) store_record(out_rod + (size_t)j * KR_SLOTS, rec);  // (verifying lanes: kk = k)
          }
          // a marked grid point: the complete record, lean step or not (with the record's other stores, in front of the
          // tile's: no read of the next trip waits behind it)
          //  (a live verifying lane is at grid point j = s_l + kk, 0 <= kk < len_l <= 32)
          if constexpr (KP) store_keypoint_window(kp_out, kp_marks, kp_rank0, kk, rec);
#ifdef KR_MSO_PROBE_NO_TILE_STORES
          if constexpr (!FULL)  // TIMING PROBE, results are wrong
#endif
#ifdef KR_MSO_PROBE_ONE_TILE_STORE
          if constexpr (FULL) {  // TIMING PROBE, results are wrong
            T l2[Vec16<T>::n];
#pragma unroll
            for (int c = 0; c < Vec16<T>::n; ++c) l2[c] = lead[c];
            lds_store_vec<T, Vec16<T>::n>(lead_w + eo, l2);
          } else
#endif
          lds_store_vec<T, 12>(lead_w + eo, lead);
        }
        // history record of the next trip.  A forward-difference lane reads the leading slots a verifying lane wrote
        // MSO_LAG - 1 trips ago (for MSO_LAG = 1: above, in this trip); a verifying lane reads slots it has not
        // replaced yet.  (FULL: j + 1 <= N - 1 is a valid grid point even where it lies past the lane's interval.)
        if constexpr (MSO_LAG < 2) {
#ifdef KR_MSO_PROBE_EARLY_READS
          if constexpr (!FULL)
#endif
          {
            if constexpr (TUPLES) lds_load_lead<T>(lead_n + en, ta);
            else lds_load_vec<T, 12>(lead_n + en, la);
          }
          // (the reads stay right behind the block: left alone, the scheduler sinks them to ~20 instructions in front of
          //  their first use.  Two wavefronts per SIMD hide that themselves, and the barrier costs them scratch.)
          if constexpr (OCC == 1) __builtin_amdgcn_sched_barrier(0);
        }
        const T dsl = live ? Pc.ds : T(0);  // (a lane outside its range evaluates finite data and adds nothing)
        y = state_axpy(y, dsl, k1);
        if constexpr (MSO_LAG < 2) {
          // (pinned behind the Euler update: the first use of the newest tile, i.e. the wait for the stores in front of
          //  its reads, comes when everything that needs only the current record has been issued)
          //  (through the products, which are single registers: a value pinned inside a 16-byte read costs a copy)
          asm volatile("" : "+v"(pb[0]), "+v"(pb[1]), "+v"(pb[2]), "+v"(pb[3]), "+v"(pb[4]), "+v"(pb[5]), "+v"(pb[6]), "+v"(pb[7]),
                            "+v"(pb[8]), "+v"(pb[9]), "+v"(pb[10]), "+v"(pb[11]), "+v"(y.p.z), "+v"(y.h3), "+v"(y.n.z), "+v"(y.m.z),
                            "+v"(y.q.z), "+v"(y.w.z));
#if KR_MSO_TRIP_CARRY
          // (probe) the scale of the next evaluation's rotation, from the state that evaluation will see (a predicated
          // trip's dsl = 0 has left y as it was): its serial chain issues under the record forming below
          rs = rot_scale(y.h0, y.h1, y.h2, y.h3);
#endif
          if constexpr (TUPLES) {
            lead_pin(ta);
            lead_unpack<T>(ta, la);
          }
          hst = hist_newest(la, pb);
        }
      };
      int k = 0;
      for (; k < MSO_LAG && k < trips; ++k) trip(k, std::integral_constant<int, 2>{}, std::false_type{});
      // (the loop of full trips once for ring-lean steps and once for complete records: no test of `lean` inside a trip)
      // (two trips per pass written out: the pins are convergent operations, and a loop that holds one is not unrolled
      //  with a remainder by the compiler)
      auto full_trips = [&](auto lean_tag) __attribute__((always_inline)) {
        for (; k + 1 < R.sbase; k += 2) {
          trip(k, std::true_type{}, lean_tag);
          trip(k + 1, std::true_type{}, lean_tag);
        }
        if (k < R.sbase) {
          trip(k, std::true_type{}, lean_tag);
          ++k;
        }
      };
      if (lean) full_trips(std::true_type{});
      else full_trips(std::false_type{});
      // The FINAL trip of a sweep that also runs step tA (k = lmax): no verifying lane is live (theirs ended a trip ago),
      // nobody reads a record again in this sweep and hst is dead behind it - the evaluation and the Euler update of
      // the forward-difference lanes whose interval has lmax segments, nothing else: no tile read, no record, no store
      // block.  (Without step tA the last trip is the verifying lanes' own and stays the generic one.)
      const bool own_final = TRIM && runA;
      for (; k < trips - (own_final ? 1 : 0); ++k) trip(k, std::false_type{}, std::false_type{});
      if (own_final) {
        const bool live = isA && R.lmax - 1 < len_l;  // (kk = lmax - 1: the last segment of a longest interval)
        RodState<T> k1;
        V3<T> v, u;
        ode_eval<T, DIAG>(Pc, y, hst, fc, k1, v, u);
        const T dsl = live ? Pc.ds : T(0);
        y = state_axpy(y, dsl, k1);
      }
    }
#ifdef KR_MS_STAMPS
    KR_STAMP_ADD(st.t_sweep, tq);
    st.sweeps += 1;
    if (merged) st.merged += 1;
#endif

    // Lane roles of the algebra between two sweeps.  They are functions of the lane index, and as loop invariants the
    // compiler kept each of them - a 64-bit mask per predicate - in scalar registers across the sweep, i.e. in the lanes
    // of a spill register, two v_readlane per use.  Formed from a lane index the compiler cannot see through, they
    // are recomputed here, once per sweep, for one or two instructions each.
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int kp = ln & 3;
    const int r = 3 + (ln >> 2);
    const bool plane = ln < 3 * (MS_P - 1);
    const int pi = plane ? ln / 3 : 0;  // term i = 0 .. P-2
    const int prow = plane ? ln - 3 * pi : 0;
    const bool glane = ln >= WAVE - 6;  // six lanes own the base wrench in the update step
    T er[19];
    state_to_rows(y, er);
    T d[6];
    T updY[MS_P - 1];
    T* dYb = XB;
    float dnf = 0.f;
    bool finite = true;
    Upd U;

    // Tail of an update: the p rows dY_g[p] = sum_{i<g} (c_i[p] + A_i[p,:] dY_i[3:]) (one term per lane), then the
    // scaled maximum norm over every unknown.  eb0: first Es slot (in lanes) of the base end states, ebs: slots
    // between consecutive intervals' base states; X: the unknowns the update belongs to.
    auto finish = [&](const T* X, auto base_slot) -> float {
      T* sp = Tm;  // [P-1][3] partial sums (the 6x6 solve has consumed Tm)
      if (kp == 0) {
#pragma unroll
        for (int g = 1; g < MS_P - 1; ++g) dYb[g * MS_YP + r] = updY[g - 1];
      }
      wave_sync_lds();
      if (plane) {
        // Every read below is unconditional, from a slot this launch has written, and the terms a lane does not have
        // are dropped by selects on the VALUES (never by a product with zero: DESIGN section 6).  Term 0 has the six
        // columns of A_0 with dG: its lane reads the Es slots of lanes 1..16 and row 1 of dYb like the others read
        // theirs, takes d[] for the first six elements and keeps its two sums as they stand behind the sixth
        // (what follows there is fma(0, 0, s) = s in the form with per-element conditions).
        const bool p0 = pi == 0;
        const int l0 = p0 ? 0 : 7 + 17 * (pi - 1);
        const int drow = p0 ? 1 : pi;
        T s = Es[base_slot(pi) * MS_YP + prow] - X[(pi + 1) * MS_YP + prow];
        T av[16], dv[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          av[c] = Es[(l0 + 1 + c) * MS_YP + prow];
          dv[c] = dYb[drow * MS_YP + 3 + c];
        }
        __builtin_amdgcn_sched_barrier(0);
        T s2 = T(0);
#pragma unroll
        for (int c = 0; c < 6; c += 2) {
          s = fma(av[c], p0 ? d[c] : dv[c], s);
          s2 = fma(av[c + 1], p0 ? d[c + 1] : dv[c + 1], s2);
        }
        const T s_6 = s, s2_6 = s2;
#pragma unroll
        for (int c = 6; c < 16; c += 2) {
          s = fma(av[c], dv[c], s);
          s2 = fma(av[c + 1], dv[c + 1], s2);
        }
        s = p0 ? s_6 : s;
        s2 = p0 ? s2_6 : s2;
        sp[pi * 3 + prow] = s + s2;
      }
      wave_sync_lds();
      // Every lane reads its operands from clamped indices and forms the update ratio of what it read; the selects come
      // last, on the ratios (never NaN).  A read under its own mask is a block of its own for every element.  The ratios
      // are pinned: left alone the compiler puts each of them back under its mask.
      const T xp = X[(pi + 1) * MS_YP + prow];  // lanes 0 .. 3 (P-1) - 1 own Y_{pi+1}[prow] (the others: row 1, element 0)
      T up = T(0);
#pragma unroll
      for (int i = 0; i < MS_P - 1; ++i) {
        const T t = sp[i * 3 + prow];
        up += i <= pi ? t : T(0);
      }
      const int kg = glane ? ln - (WAVE - 6) : 0;  // the last six lanes own G
      const T xg = X[0 * MS_YP + 7 + kg];
      T ug = d[5];  // (pinned: as a plain chain of selects it becomes a table in scratch memory, indexed by kg)
      asm volatile("" : "+v"(ug));
      ug = kg == 4 ? d[4] : ug;
      ug = kg == 3 ? d[3] : ug;
      asm volatile("" : "+v"(ug));
      ug = kg == 2 ? d[2] : ug;
      ug = kg == 1 ? d[1] : ug;
      asm volatile("" : "+v"(ug));
      ug = kg == 0 ? d[0] : ug;
      const T newP = xp + up, newG = xg + ug;
      U.newPG = plane ? newP : newG;
      // (the maximum of this lane's ratios on their bit patterns: they are non-negative and never NaN, so the order of
      //  the patterns is the order of the values, and an integer maximum needs no canonicalising of pinned operands)
      float np = update_ratio(up, xp), ng = update_ratio(ug, xg);
      asm volatile("" : "+v"(np), "+v"(ng));
      unsigned nb = plane ? __float_as_uint(np) : (glane ? __float_as_uint(ng) : 0u);
#pragma unroll
      for (int g = 1; g < MS_P; ++g) {  // one lane of the quad owns Y_g[r]
        const T xy = X[g * MS_YP + r];
        float ny = update_ratio(updY[g - 1], xy);
        U.newY[g - 1] = xy + updY[g - 1];
        asm volatile("" : "+v"(ny));
        nb = max(nb, ((g - 1) & 3) == kp ? __float_as_uint(ny) : 0u);
      }
      const float nf = __uint_as_float(nb);
      return wave_max_nonneg(nf);  // +inf if any update is not finite
    };
    auto apply = [&](T* X) {
      // (the owners' masks afresh from the lane index: kept across finish() they would sit in a spill register)
      int la = ln;
      asm volatile("" : "+v"(la));
      const bool pl = la < 3 * (MS_P - 1), gl = la >= WAVE - 6;
      const int pa = pl ? la / 3 : 0;
      if (pl || gl) X[pl ? (pa + 1) * MS_YP + (la - 3 * pa) : 0 * MS_YP + 7 + (la - (WAVE - 6))] = U.newPG;
#pragma unroll
      for (int g = 1; g < MS_P; ++g)
        if (g - 1 == (la & 3)) X[g * MS_YP + r] = U.newY[g - 1];
    };

    // =============================================================================================================
    // verdict on the step under verification
    // =============================================================================================================
    // End states through Es.  EsB is the Es area of lanes 58..61, so the verifying lanes' end states and the base end
    // states of the forward-difference sweep are ONE round of 19 stores under the union of both masks: in a merged sweep
    // it is issued here, and the Newton block below stores (and fences) only behind a plain sweep.  (The chord update
    // reads the forward-difference COLUMNS of the last condensation from Es and the verifying lanes' slots, not the base
    // slots 0, 7, 24, 41; after a rejection the next sweep writes them again before anything reads them.)
    const bool es_stored = merged;
    if (merged) {
      if (isB || (isA && col == 0)) {
#pragma unroll
        for (int q = 0; q < 19; ++q) Es[ln * MS_YP + q] = er[q];
      }
      if (isB) {
        if (ib == MS_P - 1) {  // the last grid point: y from the sweep, z untouched
          T rec[KR_SLOTS];
          record_from(y, vlast, ulast, rec);
          // (a lean ring step: the leading slots go out with the tile - at once, or with the park when the rod gives up - and slots 12.. of this
          //  record have no reader - rebuild and the take-over kernel read q w v u here, full records at interval starts)
          if (!lean) store_record(out_rod + (size_t)(N - 1) * KR_SLOTS, rec);
          if constexpr (KP) store_keypoint(kp_out, kp_lo, kp_hi, N - 1, rec);
          T lead[12];
#pragma unroll
          for (int c = 0; c < 12; ++c) lead[c] = rec[c];
          lds_store_vec<T, 12>(lead_of(tB + 1) + (size_t)(N - 1) * 12, lead);
          if (a_tip) {
            T* tp = a_tip + (rod * T_steps + tB) * 3;
            tp[0] = y.p.x; tp[1] = y.p.y; tp[2] = y.p.z;
          }
        }
      }
      wave_sync_lds();
#ifdef KR_MS_STAMPS
      unsigned long long tv;
      { KR_STAMP(tv); st.t_v1 += tv - tq; }  // end states of the verifying lanes, record of the last grid point
#endif
      // residual of the sweep: interface jumps E_g - Y_{g+1} and the tip condition, one component per lane
      float rn = 0.f;
      if (ln < 3 * MS_YP) {
        const int g = ln / MS_YP, q = ln - MS_YP * g;
        const T x = XsB[(g + 1) * MS_YP + q];
        rn = update_ratio(EsB[g * MS_YP + q] - x, x);
      } else if (ln < 3 * MS_YP + 6) {
        const int k = ln - 3 * MS_YP;
        const T e = EsB[(MS_P - 1) * MS_YP + 7 + k];
        rn = update_ratio(cold_of(tB)[CD_FTIP + k] - e, e);
      }
      rn = wave_max_nonneg(rn);
#ifdef KR_MS_STAMPS
      KR_STAMP_ADD(st.t_v2, tv);  // residual norm
#endif
      const float est = ampB * rn;
      // residual test (kr_ms_impl.hpp: audited factor 256 on the measured update / residual ratio)
      bool accepted = a_residual_test != 0 && ampB > 0.f && T(256) * (T)est <= tol;
      float dnv = est;
#ifdef KR_MS_STAMPS
      if (accepted) st.quick += 1;
#endif
      if (!accepted) {
        // chord update through the factors of step tB's last condensation: forward-difference columns in Es,
        // X_g pairs in registers, T^-1 in LDS
        T* ach = XB;             // a_g, g = 1 .. P-1: [g][19]
        T* rt = XB + 4 * MS_YP;  // tip right-hand side [6]
        dYb = XB + MS_YP * 8;
        T areg[MS_P - 1];
        areg[0] = EsB[0 * MS_YP + r] - XsB[1 * MS_YP + r];  // a_1 = c_0
        constexpr bool HOP = TRIM;
        if constexpr (!HOP) {
          if (kp == 0) ach[1 * MS_YP + r] = areg[0];
          wave_sync_lds();
        }
#pragma unroll
        for (int g = 1; g < MS_P; ++g) {
          const int l0 = 7 + 17 * (g - 1);
          T av[4], xv[4];
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            av[cc] = Es[(l0 + 1 + 4 * kp + cc) * MS_YP + r];
            // (the first hop: the lanes of step 1 form the elements of a_1 = c_0 they need themselves - the subtraction
            //  above on the same operands - so that nothing goes through ach behind a fence)
            if (HOP && g == 1) xv[cc] = EsB[0 * MS_YP + 3 + 4 * kp + cc] - XsB[1 * MS_YP + 3 + 4 * kp + cc];
            else xv[cc] = ach[g * MS_YP + 3 + 4 * kp + cc];
          }
          const T e0 = EsB[g * MS_YP + r];
          const T ynext = g < MS_P - 1 ? XsB[(g + 1) * MS_YP + r] : T(0);
          T part = fma(av[0], xv[0], av[1] * xv[1]) + fma(av[2], xv[2], av[3] * xv[3]);
          part += quad_xor<0xB1>(part);
          part += quad_xor<0x4E>(part);
          if (g < MS_P - 1) {
            areg[g] = e0 - ynext + part;
            if (kp == 0) ach[(g + 1) * MS_YP + r] = areg[g];
          } else if (kp == 0 && r >= 7 && r < 13) {
            rt[r - 7] = cold_of(tB)[CD_FTIP + (r - 7)] - e0 - part;
          }
          wave_sync_lds();
        }
        if constexpr (HOP) {
          // d = T^-1 rt, one component per lane (lanes 0 .. 5; the others form component 0 again) and six broadcasts, as
          // the Newton path hands out x6: 6 multiply-adds and 6 reads of T^-1 per lane where every lane had 36 of each.
          // The chain of a component is the same, j ascending from zero.
          const int di = ln < 6 ? ln : 0;
          T acc = T(0);
#pragma unroll
          for (int j = 0; j < 6; ++j) acc = fma(L.Ti[di * 6 + j], rt[j], acc);
          d[0] = lane_bcast<0>(acc); d[1] = lane_bcast<1>(acc); d[2] = lane_bcast<2>(acc);
          d[3] = lane_bcast<3>(acc); d[4] = lane_bcast<4>(acc); d[5] = lane_bcast<5>(acc);
        } else {
          T rtv[6];
#pragma unroll
          for (int j = 0; j < 6; ++j) rtv[j] = rt[j];
#pragma unroll
          for (int i = 0; i < 6; ++i) {
            T acc = T(0);
#pragma unroll
            for (int j = 0; j < 6; ++j) acc = fma(L.Ti[i * 6 + j], rtv[j], acc);
            d[i] = acc;
          }
        }
        {
          const T dd0 = quad_pick<T>(kp, T(0), d[1], d[3], d[5]);  // (the a column is the new one)
          const T dd1 = quad_pick<T>(kp, d[0], d[2], d[4], T(0));
#pragma unroll
          for (int g = 1; g < MS_P; ++g) {
            T sx = fma(Xreg[g - 1][1], dd1, Xreg[g - 1][0] * dd0);
            sx += quad_xor<0xB1>(sx);
            sx += quad_xor<0x4E>(sx);
            updY[g - 1] = areg[g - 1] + sx;
          }
        }
        dnv = finish(XsB, [](int g) { return MSO_B0 + g; });
        accepted = dnv <= 3.0e38f && (T)dnv <= T(0.5) * tol;
#ifdef KR_MS_STAMPS
        st.chord += 1;
#endif
      }
      if (accepted) {
        // leading slots of the accepted state: tile -> HBM, every grid point in one pass of the wavefront.  With the
        // park a lean ring step has no reader for them (a roll-back restores from registers, a rod that gives up
        // flushes its two tiles behind the loop): only the states that stay complete - the last three of a ring call,
        // every one of a full trajectory - take the pass.
        bool tile_pass = true;
#ifdef KR_MSO_PROBE_NO_TILE_PASS
        tile_pass = !lean;  // TIMING PROBE, wrong as soon as a verification is rejected or a rod gives up
#else
        if constexpr (PARK) tile_pass = !lean;
#endif
        if (tile_pass) {
          const T* const lt = lead_of(tB + 1);
          for (int j = ln; j < N; j += WAVE) {
            T lv[12];
            lds_load_vec<T, 12>(lt + (size_t)j * 12, lv);
            store_vec<T, 12>(out_rod + (size_t)j * KR_SLOTS, lv);
          }
        }
        if (!belowB && dnB > T(0)) {  // contraction constant where this step first got below the tolerance
          const T floor_dn = T(64) * (sizeof(T) == 8 ? T(2.2e-16) : T(1.2e-7));
          const T kq = fmax((T)dnv, floor_dn) * fast_rcp(dnB * dnB);
          kappa = fmin(fmax(kq, T(1e-4)), T(1));
        }
        if (ln == 0 && a_status) a_status[rod * T_steps + tB] = KR_ST_CONVERGED;
        if (ln < 6) Gguess = XsB[0 * MS_YP + 7 + ln];
        pred_skip = false;
        reverify = false;
        merged = false;
        if (!runA) break;  // that was the last step
      } else {
        // Rejected: the sweep stored a state that is not within the tolerance.  Take the chord update (when it is
        // finite), drop the work done for step tA, put the history of step tB back and carry on with plain
        // forward-difference sweeps at the updated unknowns.
#ifdef KR_MS_STAMPS
        st.rejects += 1;
#endif
        const bool ok = dnv <= 3.0e38f;
        if (ok) apply(XsB);
        wave_sync_lds();
        if (ok && !reverify && itB + 2 <= maxit) {
          // First rejection of this step, and the chord update is a proper Newton-type correction (its factors are one
          // iteration old): verify AGAIN in a merged sweep instead of falling back to two plain ones.  The history of
          // step tB comes back (from the park, else from HBM), the forward-difference lanes repeat their sweep of step tA from the same
          // start (what they computed above used a history that was off by this correction) - everything else is as
          // it was when the rejected sweep began, so a rejection costs one merged sweep instead of two plain sweeps
          // plus the restart of step tA.  In a short launch the slowest rod sets the time, and the slowest rod is the
          // one with rejections.
          reverify = true;
          itB += 1;
          dnB = (T)dnv;
          if constexpr (PARK) {
            // lead_of(tB) holds level tB: the rejected sweep wrote lead_of(tB + 1) only.  The park holds level tB - 1 as
            // taken at the hand-over of step tB, and stays valid for the sweep that verifies again.
            mso_park_restore<T>(park, lead_of(tB + 1), lane, N);
          } else {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");  // the records streamed out above are re-read below
            rebuild(tB);
          }
#ifdef KR_MS_STAMPS
          st.rebuilds += 1;
          KR_STAMP_ADD(st.t_alg, tq);
#endif
          continue;
        }
        reverify = false;
        for (int e = ln; e < MS_NE; e += WAVE) Xs[e] = XsB[e];
        tA = tB;
        rsA = a_ring ? (rsA == 0 ? 2 : rsA - 1) : rsA - 1;
        fcN = fcA;
        fcA = fcB;
        if constexpr (LOADS) {  // (set tA & 1 still holds this step's wrench; the next hand-over writes the other set again)
          if (lane < WN) wN = wrench[(size_t)(tA + 1 < T_steps ? tA + 1 : tA) * WN + lane];
        }
        order = orderB;
        it = itB;
        dn_prev = ok ? (T)dnv : T(-1);
        have_fac = ok;
        amp = ampB;
        below = false;
        pred_skip = true;
        merged = false;
        if constexpr (PARK) {
          // (tA is the rejected step again.)  lead_of(tA) holds level tA - a rejected sweep, first or second, writes
          // lead_of(tA + 1) only, and a first rejection's restore went there too; the park still holds level tA - 1 from
          // the hand-over of this step (no hand-over since): the plain sweeps below find step tA's history.
          mso_park_restore<T>(park, lead_of(tA + 1), lane, N);
        } else {
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");  // the records streamed out above are re-read below
          rebuild(tA);
        }
#ifdef KR_MS_STAMPS
        st.rebuilds += 1;
        KR_STAMP_ADD(st.t_alg, tq);
#endif
        // (giving up here: level tA in lead_of(tA), level tA - 1 just restored in lead_of(tA - 1) - the flush behind the loop)
        if (it >= maxit) { resume_at = tA; break; }
        continue;
      }
    }

    // =============================================================================================================
    // Newton update of step tA from the forward-difference sweep (kr_ms_impl.hpp, "full" branch)
    // =============================================================================================================
#ifdef KR_MS_STAMPS
    { unsigned long long t_; KR_STAMP(t_); st.t_verdict += t_ - tq; }
    unsigned long long tq2;
    KR_STAMP(tq2);
#endif
    ++it;
    float res_full;
    {
      const int l0own = iv == 0 ? 0 : 7 + 17 * (iv - 1);
      if (!es_stored) {  // (a merged sweep's end states are in Es since the verdict)
        if (isA && col == 0) {
#pragma unroll
          for (int q = 0; q < 19; ++q) Es[ln * MS_YP + q] = er[q];
        }
        wave_sync_lds();
      }
      res_full = ms_residual_norm<T>(Es, Xs, cold_of(tA), ln);
      if (isA && col > 0) {
        const T ih = fast_rcp(hstep);
        T e0[19];  // all loads first: the compiler cannot tell that they never alias the stores below
#pragma unroll
        for (int q = 0; q < 19; ++q) e0[q] = Es[l0own * MS_YP + q];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 19; ++q) Es[ln * MS_YP + q] = (er[q] - e0[q]) * ih;
      }
      wave_sync_lds();
    }
#ifdef KR_MS_STAMPS
    unsigned long long tc;
    { KR_STAMP(tc); st.t_c1 += tc - tq2; }  // end states, residual norm, forward-difference columns through Es
#endif
    dYb = XB;
    {
      const T c0 = Es[0 * MS_YP + r] - Xs[1 * MS_YP + r];
      const T da = Es[(2 * kp) * MS_YP + r];      // lanes 1..6 hold the columns of A_0 (lane 0: E_0, unused)
      const T db = Es[(2 * kp + 1) * MS_YP + r];  // (lane 7 is E_1: masked below)
      Xreg[0][0] = kp == 0 ? c0 : da;
      Xreg[0][1] = kp == 3 ? T(0) : db;
      store_pair(XB + r * 8 + 2 * kp, Xreg[0][0], Xreg[0][1]);
    }
    wave_sync_lds();
#pragma unroll
    for (int g = 1; g < MS_P; ++g) {
      const T* xcur = XB + ((g - 1) & 1) * (MS_YP * 8);
      T* xnext = XB + (g & 1) * (MS_YP * 8);
      const int l0 = 7 + 17 * (g - 1);  // unperturbed lane of interval g
      const T e0 = Es[l0 * MS_YP + r];
      T n0 = T(0), n1 = T(0), n2 = T(0), n3 = T(0);
      if (g < MS_P - 1) {
        const T cg = e0 - Xs[(g + 1) * MS_YP + r];
        n0 = kp == 0 ? cg : T(0);
      }
      {
        T av[16], xa[16], xb[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          av[c] = Es[(l0 + 1 + c) * MS_YP + r];
          load_pair(xcur + (3 + c) * 8 + 2 * kp, xa[c], xb[c]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 16; c += 2) {
          n0 = fma(av[c], xa[c], n0);
          n1 = fma(av[c], xb[c], n1);
          n2 = fma(av[c + 1], xa[c + 1], n2);
          n3 = fma(av[c + 1], xb[c + 1], n3);
        }
        n0 += n2;
        n1 += n3;
      }
      if (g < MS_P - 1) {
        Xreg[g][0] = n0;
        Xreg[g][1] = n1;
        store_pair(xnext + r * 8 + 2 * kp, n0, n1);
      } else if (r >= 7 && r < 13) {
        // tip rows: [n;m](E_{P-1} + A_{P-1} dY_{P-1}) = [F_tip; M_tip]  ->  row [rhs | T] of T dG = rhs
        if (kp == 0) n0 = cold_of(tA)[CD_FTIP + (r - 7)] - e0 - n0;  // F_tip (3) and M_tip (3) are adjacent
        store_pair(Tm + (r - 7) * 8 + 2 * kp, n0, n1);
      }
      wave_sync_lds();
    }
#ifdef KR_MS_STAMPS
    KR_STAMP_ADD(st.t_c2, tc);  // condensation chain
#endif
    {
      T a6[6][7];
      // rows [rhs | T] from Tm (which nothing overwrites before finish()): once for the solve, once more if a row moves
      auto fill6 = [&](T (&m)[6][7]) {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          T row[8];
          load_hist_vec<T, 8>(Tm + i * 8, row);
#pragma unroll
          for (int k = 0; k < 6; ++k) m[i][k] = row[1 + k];
          m[i][6] = ln < 6 ? (ln == i ? T(1) : T(0)) : row[0];  // lanes 0..5: unit vectors -> columns of T^-1
        }
      };
      fill6(a6);
      T x6[6];
      solve6_uniform(a6, x6, fill6);
      if (ln < 6) {
#pragma unroll
        for (int i = 0; i < 6; ++i) L.Ti[i * 6 + ln] = x6[i];
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) d[i] = lane_bcast<6>(x6[i]);
      have_fac = true;
    }
    {
      const T dd0 = quad_pick<T>(kp, T(1), d[1], d[3], d[5]);
      const T dd1 = quad_pick<T>(kp, d[0], d[2], d[4], T(0));
#pragma unroll
      for (int g = 1; g < MS_P; ++g) {
        T s = fma(Xreg[g - 1][1], dd1, Xreg[g - 1][0] * dd0);
        s += quad_xor<0xB1>(s);  // lanes ^1
        s += quad_xor<0x4E>(s);  // lanes ^2
        updY[g - 1] = s;
      }
    }
#ifdef KR_MS_STAMPS
    KR_STAMP_ADD(st.t_cond, tq2);
#endif
    dnf = finish(Xs, [](int g) { return g == 0 ? 0 : 7 + 17 * (g - 1); });
#ifdef KR_MS_STAMPS
    KR_STAMP_ADD(st.t_fin, tq2);
#endif
    finite = dnf <= 3.0e38f;
    const T dn = (T)dnf;
    if (res_full > 0.f && finite) amp = dnf / res_full;
    if (finite && !below && dn <= tol) {
      below = true;
      if (dn_prev > T(0)) {
        const T floor_dn = T(64) * (sizeof(T) == 8 ? T(2.2e-16) : T(1.2e-7));
        const T kq = fmax(dn, floor_dn) * fast_rcp(dn_prev * dn_prev);
        kappa = fmin(fmax(kq, T(1e-4)), T(1));
      }
    }
    bool next_final = false;
    if (finite) {
      apply(Xs);
      // will the sweep at the updated unknowns be the accepted one?  (quadratic contraction, kr_ms_impl.hpp)
      next_final = predict_final<T>(dn, dn_prev, tol, tolA) || (kappa > T(0) && T(4) * kappa * dn * dn <= tol);
      dn_prev = dn;
    }
    wave_sync_lds();
#ifdef KR_MS_STAMPS
    KR_STAMP_ADD(st.t_alg, tq);
#endif
    if (!finite || (it >= maxit && !(next_final && dn <= T(1e-2)))) {
      // no root from this start: once more from the reference's warm start (knode.py:89), then give the rod to the
      // kernel with the damped fallback
      if (order > 0 && !retried) {
        retried = true;
        order = 0;
        ms_pred_guess<T>(Q, 0, ln, base_of(tA), Xs);
        wave_sync_lds();
        if (ln < 6) Xs[0 * MS_YP + 7 + ln] = Gguess;
        wave_sync_lds();
        it = 0; dn_prev = T(-1); have_fac = false; amp = -1.f; below = false;
#ifdef KR_MS_STAMPS
        st.retries += 1;
#endif
        continue;
      }
      // (giving up here: behind a plain sweep of step tA both tiles are its history as they were - a plain sweep writes
      //  no tile; behind a merged sweep the verdict has ACCEPTED step tA - 1, whose sweep left level tA complete in
      //  lead_of(tA) and never touched level tA - 1 in lead_of(tA - 1).  Either way lead_of(t) holds level t for both.)
      resume_at = tA;
      break;
    }
    if (next_final && dn <= T(1e-2)) {
      // hand step tA to the verifying lanes and move the forward-difference lanes on to step tA + 1
      xsel ^= 1;
      Xs = X0 + xsel * X_d;
      XsB = X0 + (1 - xsel) * X_d;
#ifdef KR_MS_STAMPS
      { unsigned long long t_; KR_STAMP(t_); st.t_copy += t_ - tq; }
#endif
      dnB = dn; ampB = amp; belowB = below; itB = it; orderB = order;
      // the coming sweep verifies step tA and writes level tA + 1 over level tA - 1: that tile into the park (requested
      // here, in front of the predictor's algebra, which does not touch the tiles)
      if constexpr (PARK) mso_park_take<T>(park, lead_of(tA + 1), lane, N);
      if (!pred_skip) {
        // (two wavefronts per SIMD: the second copy of the refit cost the fp32 instantiation 12 B more scratch)
        if constexpr (OCC == 1) mso_pred_update<T>(Q, order, a_predictor, lane, XsB, stamps);
        else ms_pred_update<T>(Q, order, KR_ST_CONVERGED, a_predictor, lane, XsB, stamps);
      }
#ifdef KR_MS_STAMPS
      { unsigned long long t_; KR_STAMP(t_); st.t_upd += t_ - tq; }
#endif
      tA += 1;
      rsA = a_ring ? (rsA == 2 ? 0 : rsA + 1) : rsA + 1;
      fcB = fcA;
      if (tA < T_steps) {
        fcA = fcN;
        fcN = load_fc(tA + 1 < T_steps ? tA + 1 : tA);
        if constexpr (LOADS) {
          // the step handed over above keeps set (tA - 1) & 1; the set written here last served step tA - 2, accepted
          // before this hand-over (the fences of the start values below come before any read)
          if (lane < WN) {
            L.cold[W0 + wr_d * (tA & 1) + lane] = wN;
            wN = wrench[(size_t)(tA + 1 < T_steps ? tA + 1 : tA) * WN + lane];
          }
          if constexpr (W0 < CD_FTIP) wave_sync_lds();  // (the base slots are read back by other lanes in ms_pred_guess)
        }
        order = Q.next_order;
        ms_pred_guess<T>(Q, order, lane, base_of(tA), Xs);
        wave_sync_lds();
        if (order <= 0 && lane < 6) Xs[0 * MS_YP + 7 + lane] = XsB[0 * MS_YP + 7 + lane];  // warm start: the G just found
        wave_sync_lds();
      }
      it = 0; retried = false; below = false; dn_prev = T(-1);
      merged = true;
#ifdef KR_MS_STAMPS
      KR_STAMP_ADD(st.t_pred, tq);
#endif
    }
  }

  if constexpr (PARK) {
    // A rod that gives up hands the take-over kernel the leading slots of levels resume_at and resume_at - 1 (its
    // history of the step it resumes; kr_ms_impl.hpp, regP): lean steps have not stored them.  Tile lead_of(t) holds
    // level t for both (see the two places that set resume_at).  At step 0 the older level is the caller's prev_init,
    // which stays the caller's.
    if (resume_at < T_steps) {
      const T* const lc = lead_of(resume_at);
      const T* const lp = lead_of(resume_at - 1);
      T* const oc = state_ptr(resume_at);
      T* const op = resume_at > 0 ? state_ptr(resume_at - 1) : nullptr;
      for (int j = lane; j < N; j += WAVE) {
        T lv[12];
        lds_load_vec<T, 12>(lc + (size_t)j * 12, lv);
        store_vec<T, 12>(oc + (size_t)j * KR_SLOTS, lv);
        if (op) {
          lds_load_vec<T, 12>(lp + (size_t)j * 12, lv);
          store_vec<T, 12>(op + (size_t)j * KR_SLOTS, lv);
        }
      }
    }
  }
  if (lane < 6) A.G[rod * 6 + lane] = Gguess;
  if (lane == 0 && A.resume) A.resume[rod] = (int32_t)resume_at;
  // A rod handed over to the take-over kernel does not save: that kernel rebuilds the predictor from the stored states
  // when it resumes (t0 > 0) and, for a rod that gave up at step 0, must still find the image of the PREVIOUS call
  // (not one that already contains the rejected step); it saves its own image at the end.
  if (img && (resume_at >= T_steps || !A.resume)) {
    Q.kappa = kappa;
    ms_pred_save<T>(Q, img, lane);
  }
#ifdef KR_MS_STAMPS
  if (lane == 0 && A.dbg) {
    unsigned long long te;
    KR_STAMP(te);
    unsigned long long* dd = A.dbg + rod * 24;
    dd[0] = te - t_begin; dd[1] = st.t_sweep; dd[2] = st.t_alg; dd[3] = st.t_pred; dd[4] = st.sweeps;
    dd[5] = st.merged; dd[6] = st.quick; dd[7] = st.chord; dd[8] = st.rejects; dd[9] = st.retries; dd[10] = st.rebuilds;
    dd[11] = (unsigned long long)resume_at;
    dd[12] = st.t_verdict; dd[13] = st.t_cond; dd[14] = st.t_fin; dd[15] = st.t_upd;
    dd[16] = stamps.a1; dd[17] = stamps.a2; dd[18] = stamps.a3; dd[19] = st.t_v1; dd[20] = st.t_v2; dd[21] = st.t_c1; dd[22] = st.t_c2; dd[23] = st.t_copy;
  }
#endif
}

// The kernel counts steps in 32 bits (SimArgs::resume always did; the planner refuses T_steps >= 2^31); offsets into
// `states`, `ctl`, `tip` and `status` are formed in 64 bits.
template <typename T, int OCC, typename PSRC>
static int launch_mso_inst(const PSRC& P, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  return launch(at, mso_sim_kernel<T, true, hs_phys<T>(), OCC, PSRC>, dim3((unsigned)((a.B + MS_WPB - 1) / MS_WPB)), dim3(WAVE * MS_WPB),
                p.smem[0], P, a);
}
template <typename T>
int launch_mso_sim(kr_handle* h, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  if constexpr (sizeof(T) == 4) {  // (two wavefronts per SIMD: fp32 only)
    if (p.occ == 2) return launch_mso_inst<T, 2>(consts<T>(h), p, a, at);
  }
  return launch_mso_inst<T, 1>(consts<T>(h), p, a, at);
}

}  // namespace kr
