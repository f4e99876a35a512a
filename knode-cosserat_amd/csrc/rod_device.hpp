// rod_device.hpp - device-side Cosserat-rod physics for gfx950.
//
// One function, ode_eval<T,DIAG>, evaluates the arc-length derivative of the
// rod state at one grid point: the computation of CosseratRod.ODE
// (reference cosserat_ode.py:114-166) and of CosseratRodTorch.ODE_parallel
// (cosserat_ode_torch.py:217-306), written on named scalars so that the whole
// state lives in VGPRs and every uniform parameter in SGPRs.
//
// Algebraic regrouping relative to the reference (same real-number result,
// rounding-level differences only):
//   * R x is formed as x + s*(M x) with s = 2/(h.h), so the division overlaps
//     with the M-products instead of heading the dependency chain;
//   * n_s = R (rhoA (w x q + q_t) + C q|q|) - (rhoA g + f_tendon): one rotation
//     instead of two (cosserat_ode.py:151,155 rotate the drag separately);
//   * v = (Kse+c0 Bse)^-1 R^T n + av with av = (Kse+c0 Bse)^-1 (Kse v* - Bse v_h)
//     precomputed per grid point and time step (RodHist), likewise u;
//   * DIAG=true uses only the diagonals of (Kse+c0 Bse)^-1, (Kbt+c0 Bbt)^-1 and
//     rhoJ - the host selects it when all parameter matrices really are
//     diagonal, which is the case for every preset of knode.setup_robot.  It is
//     a template parameter so that the inner loop needs ~15 uniform doubles
//     (30 SGPRs) instead of spilling the full parameter block to VGPR lanes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/knode_rod.h"

namespace kr {

// slot map of the packed state record (see knode_rod.h)
enum : int { SL_Q = 0, SL_W = 3, SL_V = 6, SL_U = 9, SL_P = 12, SL_H = 15, SL_N = 19, SL_M = 22, SL_USED = 25 };

template <typename T>
struct V3 {
  T x, y, z;
};
template <typename T>
__device__ __forceinline__ V3<T> operator+(V3<T> a, V3<T> b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
template <typename T>
__device__ __forceinline__ V3<T> operator-(V3<T> a, V3<T> b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
template <typename T>
__device__ __forceinline__ V3<T> operator*(T s, V3<T> a) { return {s * a.x, s * a.y, s * a.z}; }
template <typename T>
__device__ __forceinline__ V3<T> cross(V3<T> a, V3<T> b) {
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
// a + s*b
template <typename T>
__device__ __forceinline__ V3<T> axpy(T s, V3<T> b, V3<T> a) { return {a.x + s * b.x, a.y + s * b.y, a.z + s * b.z}; }

// Uniform (per-launch) constants; passed by value as a kernel argument so the
// compiler keeps them in SGPRs.  Filled on the host in double and rounded.
template <typename T>
struct RodConst {
  T c0, c1, c2, ds, rhoA;
  T Ksei[9], Kbti[9], Bse[9], Bbt[9], rhoJ[9];
  T Kse_vstar[3], rhoAg[3], C[3], Ftip[3], Mtip[3];
  T tdirs[12];
  T p0[3], h0[4], q0[3], w0[3];
  int N;
  int diag;
};

// Per-rod constants (kr_param_table): rows[b] belongs to rod b.  The table lives in global memory, is written by the
// host only and never changes while a kernel that reads it is running - so the kernel sees it through the CONSTANT
// address space, and the pointer carries that in its type from the kernel argument on (a cast inside the kernel is
// folded away with the pointer's global origin, and the reads then are vector loads the compiler repeats after every
// store).  N is shared by all rows (it fixes the data layout and the LDS carve-up), so it travels beside the pointer.
#define KR_CONSTANT_AS __attribute__((address_space(4)))
template <typename T>
struct RodTable {
  const KR_CONSTANT_AS RodConst<T>* rows;
  int N;
};
// A table plus a tip-wrench history (kr_simulate_batch_loads, kr_load_impl.hpp): loads[B][T_steps][6] = F_tip (3),
// M_tip (3) of rod b while it solves step t, in place of Ftip / Mtip of the rod's row.  The pointer rides in the
// parameter source, i.e. in the kernel arguments of the loads instantiations alone.
template <typename T>
struct RodTableLoads : RodTable<T> {
  const T* loads;
};
// A table plus a boundary history (kr_simulate_batch_boundary, kr_bnd_impl.hpp): bnd[B][T_steps][19] = p0 (3), h0 (4),
// q0 (3), w0 (3), F_tip (3), M_tip (3) of rod b while it solves step t - the base state and the tip wrench, in the order
// of the LDS cold block's first 19 slots - in place of those values of the rod's row.
template <typename T>
struct RodTableBnd : RodTable<T> {
  const T* bnd;
};
// Which slots of the cold block (kr_ms_impl.hpp, CD_*) a step rewrites from a history that rides in the parameter source:
// [first, first + count), read from hist(P)[rod][t][count].  count = 0: none, the block is filled once per launch.
template <typename T, typename PSRC>
struct rod_src_step_slots {
  static constexpr int first = 0, count = 0;
  static __device__ __forceinline__ const T* hist(const PSRC&) { return nullptr; }
};
template <typename T>
struct rod_src_step_slots<T, RodTableLoads<T>> {
  static constexpr int first = 13, count = 6;  // CD_FTIP, F_tip and M_tip
  static __device__ __forceinline__ const T* hist(const RodTableLoads<T>& P) { return P.loads; }
};
template <typename T>
struct rod_src_step_slots<T, RodTableBnd<T>> {
  static constexpr int first = 0, count = 19;  // CD_P0 .. CD_MTIP + 3: the whole boundary
  static __device__ __forceinline__ const T* hist(const RodTableBnd<T>& P) { return P.bnd; }
};
// The boundary source plus key-point records (kr_simulate_batch_keypoints, kr_kp_impl.hpp): kp[T_steps][B][K][KR_SLOTS]
// receives, for every step t, the complete record of the K marked grid points of the state that step writes.  The point
// set is a 128-bit mask (N <= 128 in every kernel that takes a table): bit j of (lo, hi) marks grid point j, and the
// rank of a marked point - its index k in kp - is the number of marked points below it.  Pointer, K and mask are kernel
// arguments of the key-point instantiations alone and wavefront-uniform: testing a grid point reads no memory.
template <typename T>
struct RodTableBndKp : RodTableBnd<T> {
  T* kp;
  int K;
  unsigned long long mask_lo, mask_hi;
};
template <typename T>
struct rod_src_step_slots<T, RodTableBndKp<T>> {
  static constexpr int first = 0, count = 19;  // the boundary one
  static __device__ __forceinline__ const T* hist(const RodTableBndKp<T>& P) { return P.bnd; }
};
// Whether a parameter source carries key-point records, and where rod `rod` of a batch of B finds those of step t
template <typename T, typename PSRC>
struct rod_src_keypoints {
  static constexpr bool value = false;
  static __device__ __forceinline__ T* at(const PSRC&, int64_t, int64_t, int64_t) { return nullptr; }
  static __device__ __forceinline__ unsigned long long lo(const PSRC&) { return 0; }
  static __device__ __forceinline__ unsigned long long hi(const PSRC&) { return 0; }
};
template <typename T>
struct rod_src_keypoints<T, RodTableBndKp<T>> {
  static constexpr bool value = true;
  static __device__ __forceinline__ T* at(const RodTableBndKp<T>& P, int64_t t, int64_t B, int64_t rod) {
    return P.kp + ((t * B + rod) * P.K) * 28;  // (KR_SLOTS; the records of one rod and step are contiguous)
  }
  static __device__ __forceinline__ unsigned long long lo(const RodTableBndKp<T>& P) { return P.mask_lo; }
  static __device__ __forceinline__ unsigned long long hi(const RodTableBndKp<T>& P) { return P.mask_hi; }
};
// What a persistent kernel takes as its first argument: the launch-uniform RodConst<T> by value (every rod alike), or a
// RodTable<T>.  rod_src_row yields the constants of one rod for the kernel's arithmetic: the kernel argument itself,
// or - table - a local copy of the rod's row, read ONCE, unconditionally, where the kernel starts: scalar loads (the
// address is wavefront-uniform, the memory constant) whose results the compiler keeps in SGPRs like those of the
// kernel argument.  (Reading the row in place instead leaves the loads where the values are used: unlike the
// kernel-argument segment the row is not known to be dereferenceable, so a load under a condition inside a sweep
// cannot be hoisted out of it, and every trip pays s_load + s_waitcnt on the dependent chain of a lone wavefront.)
// rod_src_mem is the row in memory, for accesses with a per-lane index (ms_cold_fill), which would force the local
// copy into scratch.  `rod` must be the same in every lane of the wavefront.
template <typename T>
__device__ __forceinline__ int rod_src_N(const RodConst<T>& P) { return P.N; }
template <typename T>
__device__ __forceinline__ int rod_src_N(const RodTable<T>& P) { return P.N; }
template <typename T>
__device__ __forceinline__ const RodConst<T>& rod_src_mem(const RodConst<T>& P, int64_t) { return P; }
template <typename T>
__device__ __forceinline__ const RodConst<T>& rod_src_mem(const RodTable<T>& Tb, int64_t rod) {
  const int row = __builtin_amdgcn_readfirstlane((int)rod);  // (uniform anyway; this lets the compiler know)
  return *(const RodConst<T>*)(Tb.rows + row);
}
template <typename T>
__device__ __forceinline__ const RodConst<T>& rod_src_row(const RodConst<T>& P, int64_t) { return P; }
template <typename T>
__device__ __forceinline__ RodConst<T> rod_src_row(const RodTable<T>& Tb, int64_t rod) {
  constexpr int NT = 5 + 5 * 9 + 5 * 3 + 12 + 3 + 4 + 3 + 3;  // the T-typed members, which lead the struct
  static_assert(offsetof(RodConst<T>, N) == NT * sizeof(T), "RodConst: the T-typed members must be contiguous");
  const int row = __builtin_amdgcn_readfirstlane((int)rod);
  const KR_CONSTANT_AS T* src = (const KR_CONSTANT_AS T*)(Tb.rows + row);
  RodConst<T> P;
  T* dst = reinterpret_cast<T*>(&P);
#pragma unroll
  for (int i = 0; i < NT; ++i) dst[i] = src[i];
  P.N = Tb.N;
  P.diag = 1;  // (the host admits only rows with diagonal material matrices)
  return P;
}

template <typename T>
__device__ __forceinline__ V3<T> matvec(const T (&A)[9], V3<T> x) {
  return {A[0] * x.x + A[1] * x.y + A[2] * x.z, A[3] * x.x + A[4] * x.y + A[5] * x.z,
          A[6] * x.x + A[7] * x.y + A[8] * x.z};
}
template <typename T>
__device__ __forceinline__ V3<T> diagvec(const T (&A)[9], V3<T> x) {
  return {A[0] * x.x, A[4] * x.y, A[8] * x.z};
}
template <typename T, bool DIAG>
__device__ __forceinline__ V3<T> mv(const T (&A)[9], V3<T> x) {
  if constexpr (DIAG) return diagvec(A, x);
  else return matvec(A, x);
}
// A x + b
template <typename T, bool DIAG>
__device__ __forceinline__ V3<T> mv_add(const T (&A)[9], V3<T> x, V3<T> b) {
  if constexpr (DIAG) return {fma(A[0], x.x, b.x), fma(A[4], x.y, b.y), fma(A[8], x.z, b.z)};
  else {
    V3<T> t = matvec(A, x);
    return t + b;
  }
}

// y = [p h n m q w] of one grid point
template <typename T>
struct RodState {
  V3<T> p;
  T h0, h1, h2, h3;
  V3<T> n, m, q, w;
};
// Per-grid-point constants of one time step: the BDF2 history terms the physics
// needs ((q_h, w_h) from yh rows 13..18 and zh = (v_h, u_h)) plus the two
// iterate-independent parts of the constitutive law,
//   av = (Kse+c0 Bse)^-1 (Kse v* - Bse v_h),   au = -(Kbt+c0 Bbt)^-1 Bbt u_h,
// so that v = (Kse+c0 Bse)^-1 R^T n + av and u = (Kbt+c0 Bbt)^-1 R^T m + au.
template <typename T>
struct RodHist {
  V3<T> qh, wh, vh, uh, av, au;
};

// av, au from the raw history (full matrices; runs once per grid point and time step)
template <typename T>
__device__ __forceinline__ void hist_derive(const RodConst<T>& P, RodHist<T>& h) {
  V3<T> bv = matvec(P.Bse, h.vh);
  V3<T> t{P.Kse_vstar[0] - bv.x, P.Kse_vstar[1] - bv.y, P.Kse_vstar[2] - bv.z};
  h.av = matvec(P.Ksei, t);
  V3<T> bu = matvec(P.Bbt, h.uh);
  V3<T> t2 = matvec(P.Kbti, bu);
  h.au = {-t2.x, -t2.y, -t2.z};
}

// 1/x by the hardware estimate and two Newton steps (full precision for normal
// x; skips the scale/fixup sequence of IEEE division, which the rod never needs)
__device__ __forceinline__ double fast_rcp(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ float fast_rcp(float x) {
  float r = __builtin_amdgcn_rcpf(x);
  r = fmaf(fmaf(-x, r, 1.0f), r, r);
  return r;
}

// Un-normalised quaternion rotation, cosserat_ode.py:133-137: R = I + (2 / h.h) M(h), entries formed
// directly from (s b, s c, s d) with s = 2 / h.h: 31 operations to build, 9 per product (the sweep applies
// it five times per grid point, and the sweeps are bound by the fp64 instruction count).
template <typename T>
struct Rot {
  T r00, r01, r02, r10, r11, r12, r20, r21, r22;
  // R x + y
  __device__ __forceinline__ V3<T> apply_add(V3<T> x, V3<T> y) const {
    return {fma(r00, x.x, fma(r01, x.y, fma(r02, x.z, y.x))), fma(r10, x.x, fma(r11, x.y, fma(r12, x.z, y.y))),
            fma(r20, x.x, fma(r21, x.y, fma(r22, x.z, y.z)))};
  }
  __device__ __forceinline__ V3<T> apply(V3<T> x) const {  // R x
    return {fma(r00, x.x, fma(r01, x.y, r02 * x.z)), fma(r10, x.x, fma(r11, x.y, r12 * x.z)),
            fma(r20, x.x, fma(r21, x.y, r22 * x.z))};
  }
  __device__ __forceinline__ V3<T> applyT(V3<T> x) const {  // R^T x
    return {fma(r00, x.x, fma(r10, x.y, r20 * x.z)), fma(r01, x.x, fma(r11, x.y, r21 * x.z)),
            fma(r02, x.x, fma(r12, x.y, r22 * x.z))};
  }
};

// (the scale s = 2 / h.h apart from the entries: it is the one serial chain of the rotation - four products, the
// estimate, two Newton steps, the doubling - and a caller that knows the quaternion of its next evaluation early can
// form it there, under other work, and hand it to ode_eval_s)
template <typename T>
__device__ __forceinline__ T rot_scale(T a, T b, T c, T d) {
  return T(2) * fast_rcp(fma(a, a, fma(b, b, fma(c, c, d * d))));
}
template <typename T>
__device__ __forceinline__ Rot<T> make_rot_s(T a, T b, T c, T d, T s) {
  Rot<T> R;
  const T sb = s * b, sc = s * c, sd = s * d;
  R.r00 = fma(-sc, c, fma(-sd, d, T(1)));
  R.r01 = fma(sb, c, -sd * a);
  R.r02 = fma(sb, d, sc * a);
  R.r10 = fma(sb, c, sd * a);
  R.r11 = fma(-sb, b, fma(-sd, d, T(1)));
  R.r12 = fma(sc, d, -sb * a);
  R.r20 = fma(sb, d, -sc * a);
  R.r21 = fma(sc, d, sb * a);
  R.r22 = fma(-sb, b, fma(-sc, c, T(1)));
  return R;
}
template <typename T>
__device__ __forceinline__ Rot<T> make_rot(T a, T b, T c, T d) {
  return make_rot_s(a, b, c, d, rot_scale(a, b, c, d));
}

// a x b + c and c - a x b with the products fused
template <typename T>
__device__ __forceinline__ V3<T> cross_add(V3<T> a, V3<T> b, V3<T> c) {
  return {fma(a.y, b.z, fma(-a.z, b.y, c.x)), fma(a.z, b.x, fma(-a.x, b.z, c.y)), fma(a.x, b.y, fma(-a.y, b.x, c.z))};
}
template <typename T>
__device__ __forceinline__ V3<T> cross_sub(V3<T> c, V3<T> a, V3<T> b) {
  return {fma(-a.y, b.z, fma(a.z, b.y, c.x)), fma(-a.z, b.x, fma(a.x, b.z, c.y)), fma(-a.x, b.y, fma(a.y, b.x, c.z))};
}

// ys (same struct as the state) and z = [v u]; fconst = rhoA*g + tendon force.  s: rot_scale of y's quaternion.
template <typename T, bool DIAG>
__device__ __forceinline__ void ode_eval_s(const RodConst<T>& P, const RodState<T>& y, const RodHist<T>& hst,
                                           V3<T> fconst, RodState<T>& ys, V3<T>& v, V3<T>& u, T s) {
  const Rot<T> R = make_rot_s(y.h0, y.h1, y.h2, y.h3, s);

  // solved constitutive law, cosserat_ode.py:140-141
  V3<T> Rtn = R.applyT(y.n);
  V3<T> Rtm = R.applyT(y.m);
  v = mv_add<T, DIAG>(P.Ksei, Rtn, hst.av);
  u = mv_add<T, DIAG>(P.Kbti, Rtm, hst.au);

  // BDF2 time derivatives, cosserat_ode.py:146-148
  const V3<T> qt = axpy(P.c0, y.q, hst.qh);
  const V3<T> wt = axpy(P.c0, y.w, hst.wh);
  const V3<T> vt = axpy(P.c0, v, hst.vh);
  const V3<T> ut = axpy(P.c0, u, hst.uh);

  // rod state derivatives, cosserat_ode.py:151-158
  ys.p = R.apply(v);
  V3<T> drag{P.C[0] * y.q.x * fabs(y.q.x), P.C[1] * y.q.y * fabs(y.q.y), P.C[2] * y.q.z * fabs(y.q.z)};
  V3<T> fin = axpy(P.rhoA, cross_add(y.w, y.q, qt), drag);
  ys.n = R.apply_add(fin, V3<T>{-fconst.x, -fconst.y, -fconst.z});
  V3<T> Jw = mv<T, DIAG>(P.rhoJ, y.w);
  const V3<T> pxn = cross(ys.p, y.n);
  ys.m = R.apply_add(mv_add<T, DIAG>(P.rhoJ, wt, cross(y.w, Jw)), V3<T>{-pxn.x, -pxn.y, -pxn.z});
  ys.q = cross_add(y.w, v, cross_sub(vt, u, y.q));
  ys.w = cross_sub(ut, u, y.w);

  // quaternion derivative, cosserat_ode.py:161-165
  const V3<T> hu{T(0.5) * u.x, T(0.5) * u.y, T(0.5) * u.z};
  ys.h0 = fma(-hu.x, y.h1, fma(-hu.y, y.h2, -hu.z * y.h3));
  ys.h1 = fma(hu.x, y.h0, fma(hu.z, y.h2, -hu.y * y.h3));
  ys.h2 = fma(hu.y, y.h0, fma(-hu.z, y.h1, hu.x * y.h3));
  ys.h3 = fma(hu.z, y.h0, fma(hu.y, y.h1, -hu.x * y.h2));
}
template <typename T, bool DIAG>
__device__ __forceinline__ void ode_eval(const RodConst<T>& P, const RodState<T>& y, const RodHist<T>& hst,
                                         V3<T> fconst, RodState<T>& ys, V3<T>& v, V3<T>& u) {
  ode_eval_s<T, DIAG>(P, y, hst, fconst, ys, v, u, rot_scale(y.h0, y.h1, y.h2, y.h3));
}

// y + a*k  (Euler update / RK stage argument)
template <typename T>
__device__ __forceinline__ RodState<T> state_axpy(const RodState<T>& y, T a, const RodState<T>& k) {
  RodState<T> r;
  r.p = axpy(a, k.p, y.p);
  r.h0 = y.h0 + a * k.h0;
  r.h1 = y.h1 + a * k.h1;
  r.h2 = y.h2 + a * k.h2;
  r.h3 = y.h3 + a * k.h3;
  r.n = axpy(a, k.n, y.n);
  r.m = axpy(a, k.m, y.m);
  r.q = axpy(a, k.q, y.q);
  r.w = axpy(a, k.w, y.w);
  return r;
}

// exp(x) for the activations: one rounding-level-accurate, short instruction sequence instead of the
// library routine (the MLP evaluates 128 activations per lane per call, so ocml's ~100-instruction
// fp64 expm1/tanh dominated the matrix-core evaluator).  x = k ln2 + r, |r| <= ln2/2, Taylor to
// degree 13 (remainder 2e-16), scaled by 2^k with v_ldexp.
__device__ __forceinline__ double fast_exp(double x) {
  x = fmin(fmax(x, -745.0), 709.0);
  const double k = __builtin_rint(x * 1.4426950408889634);
  double r = fma(-k, 6.93147180369123816490e-01, x);
  r = fma(-k, 1.90821492927058770002e-10, r);
  double p = 1.0 / 6227020800.0;
  p = fma(p, r, 1.0 / 479001600.0);
  p = fma(p, r, 1.0 / 39916800.0);
  p = fma(p, r, 1.0 / 3628800.0);
  p = fma(p, r, 1.0 / 362880.0);
  p = fma(p, r, 1.0 / 40320.0);
  p = fma(p, r, 1.0 / 5040.0);
  p = fma(p, r, 1.0 / 720.0);
  p = fma(p, r, 1.0 / 120.0);
  p = fma(p, r, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return __builtin_ldexp(p, (int)k);
}
__device__ __forceinline__ float fast_exp(float x) { return __expf(x); }  // v_exp_f32 on x*log2(e)

// Block form: the same arithmetic on N independent values with the loops ordered coefficient-major,
// so that the dependent FMA chain of one value (9.5 cycles per fp64 op) is interleaved with the
// chains of the others instead of being executed back to back.
template <int N>
__device__ __forceinline__ void fast_exp_block(const double (&xin)[N], double (&y)[N]) {
  double k[N], r[N], p[N];
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const double x = fmin(fmax(xin[e], -745.0), 709.0);
    k[e] = __builtin_rint(x * 1.4426950408889634);
    r[e] = fma(-k[e], 6.93147180369123816490e-01, x);
  }
#pragma unroll
  for (int e = 0; e < N; ++e) {
    r[e] = fma(-k[e], 1.90821492927058770002e-10, r[e]);
    p[e] = 1.0 / 6227020800.0;
  }
  constexpr double c[13] = {1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0,
                            1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0};
#pragma unroll
  for (int j = 0; j < 13; ++j)
#pragma unroll
    for (int e = 0; e < N; ++e) p[e] = fma(p[e], r[e], c[j]);
#pragma unroll
  for (int e = 0; e < N; ++e) y[e] = __builtin_ldexp(p[e], (int)k[e]);
}
template <int N>
__device__ __forceinline__ void fast_exp_block(const float (&xin)[N], float (&y)[N]) {
#pragma unroll
  for (int e = 0; e < N; ++e) y[e] = __expf(xin[e]);
}

// exp(x) - 1 for x <= 0.  fp64: literally the reference's np.exp(x) - 1 (cosserat_ode.py:94);
// fp32: torch's ELU uses expm1, so keep relative accuracy for small |x| with a short series.
__device__ __forceinline__ double elu_neg(double x) { return fast_exp(x) - 1.0; }
__device__ __forceinline__ float elu_neg(float x) {
  // both sides evaluated, one v_cndmask picks: as a conditional expression around __expf the compiler emitted a
  // divergent branch per value (4 nested exec-mask regions per activation block, ~750 cycles for four values)
  float series = x * (1.f + x * (0.5f + x * (0.16666667f + x * (0.041666668f + x * 0.0083333338f))));
  float ex = __builtin_amdgcn_exp2f(x * 1.44269504088896341f) - 1.f;
  // (opaque to the optimiser from here on: it turns a select between two "expensive" expressions back into a branch)
  asm volatile("" : "+v"(series), "+v"(ex));
  return x > -0.25f ? series : ex;
}

// activation functions of the residual MLP, cosserat_ode.py:92-106
template <typename T>
__device__ __forceinline__ T activate(int code, T x) {
  switch (code) {
    case KR_ACT_TANH: {  // 1 - 2/(e^{2x}+1): absolute error at rounding level, no cancellation blow-up
      const T e = fast_exp(T(2) * x);
      return T(1) - T(2) * fast_rcp(e + T(1));
    }
    case KR_ACT_SOFTPLUS: return log1p(fast_exp(-fabs(x))) + fmax(x, T(0));
    case KR_ACT_RELU: return fmax(x, T(0));
    case KR_ACT_ELU: {  // max(x, 0) + (exp(min(x, 0)) - 1): nothing for the compiler to turn into a branch (elu_neg(0) == 0)
      const T e = elu_neg(fmin(x, T(0)));
      return fmax(x, T(0)) + e;
    }
    default: return x;
  }
}
template <typename T>
__device__ __forceinline__ T activate_grad(int code, T pre) {  // d act / d pre
  switch (code) {
    case KR_ACT_TANH: {
      const T e = fast_exp(T(2) * pre);
      const T t = T(1) - T(2) * fast_rcp(e + T(1));
      return T(1) - t * t;
    }
    case KR_ACT_SOFTPLUS: return fast_rcp(T(1) + fast_exp(-pre));
    case KR_ACT_RELU: return pre > T(0) ? T(1) : T(0);
    case KR_ACT_ELU: return pre > T(0) ? T(1) : fast_exp(pre);
    default: return T(1);
  }
}

// activation of N independent values at once (see fast_exp_block); ACT is a compile-time code
template <typename T, int ACT, int N>
__device__ __forceinline__ void activate_block(T (&x)[N]) {
  if constexpr (ACT == KR_ACT_ELU) {
    T xm[N], ex[N];
#pragma unroll
    for (int e = 0; e < N; ++e) xm[e] = fmin(x[e], T(0));
    if constexpr (sizeof(T) == 8) {
      fast_exp_block<N>(xm, ex);
#pragma unroll
      for (int e = 0; e < N; ++e) x[e] = x[e] > T(0) ? x[e] : ex[e] - T(1);
    } else {
      // max(x, 0) + elu_neg(min(x, 0)): no select for the compiler to turn into a divergent branch per value
      // (elu_neg(0) is exactly 0, so positive inputs pass unchanged)
#pragma unroll
      for (int e = 0; e < N; ++e) x[e] = fmax(x[e], T(0)) + elu_neg(xm[e]);
    }
  } else if constexpr (ACT == KR_ACT_TANH) {
    T t2[N], ex[N];
#pragma unroll
    for (int e = 0; e < N; ++e) t2[e] = T(2) * x[e];
    fast_exp_block<N>(t2, ex);
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = T(1) - T(2) * fast_rcp(ex[e] + T(1));
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] = activate<T>(ACT, x[e]);
  }
}

// reference-order accessors: y rows 0..18 = p h n m q w; z rows = v u
template <typename T>
__device__ __forceinline__ void state_to_rows(const RodState<T>& s, T (&r)[19]) {
  r[0] = s.p.x; r[1] = s.p.y; r[2] = s.p.z;
  r[3] = s.h0; r[4] = s.h1; r[5] = s.h2; r[6] = s.h3;
  r[7] = s.n.x; r[8] = s.n.y; r[9] = s.n.z;
  r[10] = s.m.x; r[11] = s.m.y; r[12] = s.m.z;
  r[13] = s.q.x; r[14] = s.q.y; r[15] = s.q.z;
  r[16] = s.w.x; r[17] = s.w.y; r[18] = s.w.z;
}
template <typename T>
__device__ __forceinline__ RodState<T> rows_to_state(const T (&r)[19]) {
  RodState<T> s;
  s.p = {r[0], r[1], r[2]};
  s.h0 = r[3]; s.h1 = r[4]; s.h2 = r[5]; s.h3 = r[6];
  s.n = {r[7], r[8], r[9]};
  s.m = {r[10], r[11], r[12]};
  s.q = {r[13], r[14], r[15]};
  s.w = {r[16], r[17], r[18]};
  return s;
}

}  // namespace kr
