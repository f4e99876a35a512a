// kr_adj.hip - the adjoint of one solved implicit BDF2 step (MLP off) and the backward pass over a stored rollout.
//
//   kr_step_vjp_batch      cotangent of state_next -> gradients with respect to state_cur, state_prev, the tensions and
//                          the boundary data (base state, tip wrench) of the step        (knode.py:70-100, one pass of the loop)
//   kr_simulate_vjp_batch  the same composed over the T steps of a stored trajectory     (knode.py:55-102)
//
// The step solves r(G) = [F_tip - n_{N-1}, M_tip - m_{N-1}] = 0 for the base wrench G by sweeping
// y_{j+1} = y_j + ds f(y_j, hist_j, tf) from y_0 = [p0, h0, G, q0, w0] (cosserat_ode.py:188-213).  Its derivative is that
// of the sweep at fixed G plus the implicit-function term through G:
//
//   pass 1  carries SEVEN cotangent vectors back along the rod at once: the caller's g (seed 0) and the six unit seeds
//           on (n, m) of the tip.  lambda_{N-1} = seed, lambda_j = g_y[j] + lambda_{j+1} + J_j^T [ds lambda_{j+1}; g_z[j]].
//           The (n, m) rows of lambda_0 are a = dL/dG at fixed tip condition (seed 0) and the rows of
//           M = d(n, m)_{N-1} / dG (seeds 1..6).
//   solve   M^T nu = -a (6 x 6, partial pivoting): nu is the cotangent the tip condition puts on (n, m)_{N-1}.
//   pass 2  carries the one combined cotangent (g, plus nu on the tip's (n, m)) and emits, point by point, the columns of
//           J_j^T in the history (q, w, v, u of c1 cur + c2 prev) and in the tendon force.  The (n, m) rows of its lambda_0
//           are zero up to rounding: |.|_inf / |a|_inf is reported as `resid`.
//
// Nothing is re-solved: the states are read from state_next.  Arithmetic is fp64 whatever the element type of the arrays.
//
// Mapping: one wavefront per rod, four rods per workgroup, no LDS.  The per-point derivative is forward mode on dual
// numbers (kr_point_dual.hpp): lane l evaluates the point map once with the tangent along ONE input direction - lanes
// 0..18 the components of y, 19..30 the twelve history values f reads, 31..33 the tendon force - and so owns component l
// of J^T x for any x: a dot product of its 25 output tangents with x.  A lane below 19 keeps component l of every
// cotangent vector in a register; the dot product fetches the others lane by lane (v_readlane with a constant lane).
// The recursion is serial in j and the rods are independent: no atomics, no cross-wavefront traffic, and a rod's result
// does not depend on the batch it rides in.
#include "kr_adj_impl.hpp"

namespace kr {

template <typename T>
__global__ __launch_bounds__(64 * ADJ_RODS_PER_WG) void step_vjp_kernel(const RodConst<double> P, const AdjArgs<T> A) {
  const int lane = threadIdx.x & 63;
  const int64_t rod = (int64_t)blockIdx.x * ADJ_RODS_PER_WG + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (rod >= A.B) return;  // (the whole wavefront: nothing below crosses wavefronts)
  const int N = P.N;
  const int64_t rec0 = rod * N;
  const int dir = lane < 19 ? lane : lane + 13;  // lanes 19..30 -> 32..43 (history q w v u), 31..33 -> 44..46 (tendon force)
  const int yslot = adj_yslot(lane < 19 ? lane : 0);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  bool bad = false;
  double tens[4], tf[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    tens[k] = (double)A.tens[rod * A.tens_stride + k];
    bad |= !isfinite(tens[k]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) tf[c] = tens[0] * P.tdirs[c] + tens[1] * P.tdirs[3 + c] + tens[2] * P.tdirs[6 + c] + tens[3] * P.tdirs[9 + c];

  // ---- the tip record: seeds; everything of it that no sweep reads is still checked ----
  const T* gN = A.g_next + (rec0 + N - 1) * KR_SLOTS;
  {
    const T* yN = A.next + (rec0 + N - 1) * KR_SLOTS;
    const T* cN = A.cur + (rec0 + N - 1) * KR_SLOTS;
    const T* pN = A.prev + (rec0 + N - 1) * KR_SLOTS;
#pragma unroll
    for (int k = 0; k < SL_USED; ++k) bad |= !isfinite((double)yN[k]) | !isfinite((double)gN[k]);
#pragma unroll
    for (int k = 0; k < 12; ++k) bad |= !isfinite((double)cN[k]) | !isfinite((double)pN[k]);
  }
  const double g_tip = (double)gN[yslot];

  // ---- pass 1: seven cotangent vectors ----
  double lam[ADJ_SEEDS];
  lam[0] = g_tip;
#pragma unroll
  for (int s = 1; s < ADJ_SEEDS; ++s) lam[s] = lane == 6 + s ? 1.0 : 0.0;
  for (int j = N - 2; j >= 0; --j) {
    double d[25];
    adj_point(P, A, rec0 + j, dir, tf, d, bad);
    const T* g = A.g_next + (rec0 + j) * KR_SLOTS;
    double gz[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) gz[k] = (double)g[SL_V + k];
#pragma unroll
    for (int k = 0; k < SL_USED; ++k) bad |= !isfinite((double)g[k]);
    double acc = P.ds * adj_dot19(lam[0], d, 0.0);
#pragma unroll
    for (int k = 0; k < 6; ++k) acc = fma(gz[k], d[19 + k], acc);
    lam[0] = ((double)g[yslot] + lam[0]) + acc;
#pragma unroll
    for (int s = 1; s < ADJ_SEEDS; ++s) lam[s] = lam[s] + P.ds * adj_dot19(lam[s], d, 0.0);
  }
  double a[6], m[6][6], nu[6];
  a[0] = adj_bcast<7>(lam[0]); a[1] = adj_bcast<8>(lam[0]); a[2] = adj_bcast<9>(lam[0]);
  a[3] = adj_bcast<10>(lam[0]); a[4] = adj_bcast<11>(lam[0]); a[5] = adj_bcast<12>(lam[0]);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    m[k][0] = adj_bcast<7>(lam[1 + k]); m[k][1] = adj_bcast<8>(lam[1 + k]); m[k][2] = adj_bcast<9>(lam[1 + k]);
    m[k][3] = adj_bcast<10>(lam[1 + k]); m[k][4] = adj_bcast<11>(lam[1 + k]); m[k][5] = adj_bcast<12>(lam[1 + k]);
  }
  double anorm = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    anorm = fmax(anorm, fabs(a[k]));
    bad |= !isfinite(a[k]);
#pragma unroll
    for (int l = 0; l < 6; ++l) bad |= !isfinite(m[k][l]);
  }
  bad = __any(bad);  // (uniform already: every lane read the same values)
  const bool solved = adj_solve6(m, a, nu);
  const int st = bad ? KR_ST_NONFINITE : (solved ? KR_ST_CONVERGED : KR_ST_MAXIT);
  if (A.status && lane == 0) A.status[rod * A.st_stride] = st;

  T* oc = A.g_cur ? A.g_cur + rec0 * KR_SLOTS : nullptr;
  T* op = A.g_prev ? A.g_prev + rec0 * KR_SLOTS : nullptr;
  T* ot = A.g_tens ? A.g_tens + rod * A.g_tens_stride : nullptr;
  T* ob = A.g_bnd ? A.g_bnd + rod * KR_BND : nullptr;

  if (st != KR_ST_CONVERGED) {  // no gradient: NaN in every value that carries one, zero where the structure is zero
    if (lane < KR_SLOTS) {
      const T fill = lane < 12 ? (T)nan : (T)0;
      for (int j = 0; j < N; ++j) {
        if (oc) oc[(int64_t)j * KR_SLOTS + lane] = fill;
        if (op) op[(int64_t)j * KR_SLOTS + lane] = fill;
      }
    }
    if (ot && lane < 4) ot[lane] = (T)nan;
    if (ob && lane < KR_BND) ob[lane] = (T)nan;
    if (A.resid && lane == 0) A.resid[rod * A.st_stride] = nan;
    return;
  }

  // ---- pass 2: the combined cotangent; emits the input gradients ----
  const double c1 = P.c1, c2 = P.c2;
  double nu_l = 0.0;  // nu of this lane's row of (n, m)
#pragma unroll
  for (int k = 0; k < 6; ++k) nu_l = lane == 7 + k ? nu[k] : nu_l;
  double lm = g_tip + nu_l;
  double gtf = 0.0;
  // the tip record: no f is evaluated there; v, u of state_next are those of state_cur (the z[:, N-1] the reference never
  // writes), so their cotangent passes straight through
  if (lane < KR_SLOTS) {
    const bool pass = lane >= SL_V && lane < SL_P;
    const T gv = gN[pass ? lane : 0];
    if (oc) oc[(int64_t)(N - 1) * KR_SLOTS + lane] = pass ? gv : (T)0;
    if (op) op[(int64_t)(N - 1) * KR_SLOTS + lane] = (T)0;
  }
  for (int j = N - 2; j >= 0; --j) {
    double d[25];
    bool unused = false;
    adj_point(P, A, rec0 + j, dir, tf, d, unused);
    const T* g = A.g_next + (rec0 + j) * KR_SLOTS;
    double acc = P.ds * adj_dot19(lm, d, 0.0);
#pragma unroll
    for (int k = 0; k < 6; ++k) acc = fma((double)g[SL_V + k], d[19 + k], acc);
    // lanes 0..18: component `lane` of J_j^T [ds lambda_{j+1}; g_z[j]] in y; 19..30: in the history; 31..33: in tf
    lm = ((double)g[yslot] + lm) + acc;  // (meaningful in lanes 0..18, and read from there only)
    gtf += acc;                           // (... in lanes 31..33)
    if (lane >= 19 && lane < KR_SLOTS + 19) {
      const int slot = lane - 19;  // 0..11: the history slots; 12..27: structurally zero and the pads
      const T vc = slot < 12 ? (T)(c1 * acc) : (T)0, vp = slot < 12 ? (T)(c2 * acc) : (T)0;
      if (oc) oc[(int64_t)j * KR_SLOTS + slot] = vc;
      if (op) op[(int64_t)j * KR_SLOTS + slot] = vp;
    }
  }
  // lambda_0: the (n, m) rows are the total derivative with respect to G - zero at the root
  const double r7 = adj_bcast<7>(lm), r8 = adj_bcast<8>(lm), r9 = adj_bcast<9>(lm), r10 = adj_bcast<10>(lm),
               r11 = adj_bcast<11>(lm), r12 = adj_bcast<12>(lm);
  const double rmax = fmax(fmax(fmax(fabs(r7), fabs(r8)), fmax(fabs(r9), fabs(r10))), fmax(fabs(r11), fabs(r12)));
  if (A.resid && lane == 0) A.resid[rod * A.st_stride] = anorm > 0.0 ? rmax / anorm : 0.0;
  if (ot) {
    const double t0 = adj_bcast<31>(gtf), t1 = adj_bcast<32>(gtf), t2 = adj_bcast<33>(gtf);
    if (lane < 4) ot[lane] = (T)(P.tdirs[3 * lane] * t0 + P.tdirs[3 * lane + 1] * t1 + P.tdirs[3 * lane + 2] * t2);
  }
  if (ob && lane < 19) {
    // KR_BND order: p0 (3), h0 (4), q0 (3), w0 (3), F_tip (3), M_tip (3); y rows: p h n m q w.  The tip wrench enters
    // the tip condition only, (n, m)_{N-1} = (F_tip, M_tip): its gradient is -nu
    const int k = lane < 7 ? lane : (lane < 13 ? lane + 6 : lane - 6);
    ob[k] = (T)(lane >= 7 && lane < 13 ? -nu_l : lm);
  }
}

template <typename T>
static int launch_step_vjp(kr_handle* h, const AdjArgs<T>& A, hipStream_t s) {
  const int64_t grid = (A.B + ADJ_RODS_PER_WG - 1) / ADJ_RODS_PER_WG;
  hipLaunchKernelGGL((step_vjp_kernel<T>), dim3((unsigned)grid), dim3(64 * ADJ_RODS_PER_WG), 0, s, h->cd, A);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

// The backward pass over a stored rollout, DEFINED as this composition of step adjoints (t = T - 1 .. 0):
//   step adjoint of (states[t - 1], states[t], states[t + 1], ctl[:, t]) with g_next = g_states[t + 1]
//   g_states[t] += g_cur;  g_states[t - 1] += g_prev  (in this order, in the element type of the arrays)
template <typename T>
static int simulate_vjp(kr_handle* h, int64_t B, int64_t T_steps, const T* ctl, const T* states, const T* prev_init, T* g_states,
                        T* g_prev_init, T* g_ctl, T* g_bnd, double* resid, int32_t* status, hipStream_t s) {
  const int64_t slot = B * h->params.N * KR_SLOTS;
  const size_t bnd_off = (size_t)2 * slot * sizeof(T);
  if (int rc = ensure_ws(h, bnd_off + (size_t)B * KR_BND * sizeof(T))) return rc;
  T* w_cur = static_cast<T*>(h->ws);
  T* w_prev = w_cur + slot;
  T* w_bnd = w_prev + slot;
  if (g_bnd) KR_HIP(hipMemsetAsync(g_bnd, 0, (size_t)B * KR_BND * sizeof(T), s));
  for (int64_t t = T_steps - 1; t >= 0; --t) {
    const bool into_init = t == 0 && prev_init != nullptr;
    AdjArgs<T> A{};
    A.B = B;
    A.prev = t > 0 ? states + (t - 1) * slot : (prev_init ? prev_init : states);
    A.cur = states + t * slot;
    A.next = states + (t + 1) * slot;
    A.tens = ctl + t * 4;
    A.tens_stride = T_steps * 4;
    A.g_next = g_states + (t + 1) * slot;
    A.g_cur = w_cur;
    A.g_prev = into_init ? g_prev_init : w_prev;
    A.g_tens = g_ctl ? g_ctl + t * 4 : nullptr;
    A.g_tens_stride = T_steps * 4;
    A.g_bnd = g_bnd ? w_bnd : nullptr;
    A.resid = resid ? resid + t : nullptr;
    A.status = status ? status + t : nullptr;
    A.st_stride = T_steps;
    if (int rc = launch_step_vjp<T>(h, A, s)) return rc;
    if (int rc = launch_add<T>(g_states + t * slot, w_cur, slot, s)) return rc;
    if (!into_init)
      if (int rc = launch_add<T>(g_states + (t > 0 ? t - 1 : 0) * slot, w_prev, slot, s)) return rc;
    if (g_bnd)
      if (int rc = launch_add<T>(g_bnd, w_bnd, B * KR_BND, s)) return rc;
  }
  return KR_OK;
}

static int adj_refuse(const char* api, int scheme, int use_nn) {
  if (use_nn != 0) {
    set_error(std::string(api) + ": the adjoint with the MLP on is not served (the network's input Jacobian is not part of the "
              "per-point derivative); nothing falls back to the physics alone");
    return KR_E_UNSUPPORTED;
  }
  if (scheme == KR_RK4) {
    set_error(std::string(api) + ": the adjoint of the RK4 sweep is not served; nothing falls back to the Euler sweep");
    return KR_E_UNSUPPORTED;
  }
  if (scheme != KR_EULER) {
    set_error(std::string(api) + ": scheme must be KR_EULER");
    return KR_E_ARG;
  }
  return KR_OK;
}

}  // namespace kr

using namespace kr;

#define KR_ADJ_ARG(cond, msg) \
  if (cond) {                 \
    set_error(msg);           \
    return KR_E_ARG;          \
  }

extern "C" int kr_step_vjp_batch(kr_handle* h, int64_t B, int scheme, const void* state_prev, const void* state_cur,
                                 const void* state_next, const void* tensions, const void* g_next, void* g_cur, void* g_prev,
                                 void* g_tensions, void* g_bnd, double* resid, int32_t* status, int use_nn, int dtype, void* stream) {
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_ADJ_ARG(B < 1 || B > 0x7FFFFFFFll, "kr_step_vjp_batch: B must be in [1, 2^31 - 1]");
  KR_ADJ_ARG(!state_prev || !state_cur || !state_next || !tensions || !g_next, "kr_step_vjp_batch: null pointer argument");
  if (int rc = adj_refuse("kr_step_vjp_batch", scheme, use_nn)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  if (dtype == KR_F32) {
    AdjArgs<float> A{B, (const float*)state_prev, (const float*)state_cur, (const float*)state_next, (const float*)tensions, 4,
                     (const float*)g_next, (float*)g_cur, (float*)g_prev, (float*)g_tensions, 4, (float*)g_bnd, resid, status, 1};
    return launch_step_vjp<float>(h, A, s);
  }
  AdjArgs<double> A{B, (const double*)state_prev, (const double*)state_cur, (const double*)state_next, (const double*)tensions, 4,
                    (const double*)g_next, (double*)g_cur, (double*)g_prev, (double*)g_tensions, 4, (double*)g_bnd, resid, status, 1};
  return launch_step_vjp<double>(h, A, s);
}

extern "C" int kr_simulate_vjp_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, const void* states,
                                     const void* state_prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd,
                                     double* resid, int32_t* status, int use_nn, int dtype, void* stream) {
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_ADJ_ARG(B < 1 || B > 0x7FFFFFFFll, "kr_simulate_vjp_batch: B must be in [1, 2^31 - 1]");
  KR_ADJ_ARG(T < 1, "kr_simulate_vjp_batch: T < 1");
  KR_ADJ_ARG(!ctl || !states || !g_states, "kr_simulate_vjp_batch: null pointer argument");
  if (int rc = adj_refuse("kr_simulate_vjp_batch", scheme, use_nn)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  if (dtype == KR_F32)
    return simulate_vjp<float>(h, B, T, (const float*)ctl, (const float*)states, (const float*)state_prev_init, (float*)g_states,
                               (float*)g_prev_init, (float*)g_ctl, (float*)g_bnd, resid, status, s);
  return simulate_vjp<double>(h, B, T, (const double*)ctl, (const double*)states, (const double*)state_prev_init, (double*)g_states,
                              (double*)g_prev_init, (double*)g_ctl, (double*)g_bnd, resid, status, s);
}
