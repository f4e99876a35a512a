// kr_adj_nn.hip - the adjoint of one solved implicit BDF2 step with the residual MLP on, and the backward pass over a
// stored rollout of the KNODE model (physics plus network in every sweep).
//
//   kr_step_vjp_nn_batch      kr_step_vjp_batch with the network in the point map           (knode.py:70-100)
//   kr_simulate_vjp_nn_batch  the same composed over the T steps of a stored trajectory      (knode.py:55-102)
//
// With the network the point map is (y_s, z) = f_phys(y, hist, tf) + NN(x), x = [y (19), z_phys (6), tf (3)]
// (cosserat_ode.py:178-184, nn_input_history = 0).  With Jn[25][28] = dNN/dx at the stored point the 25 x 34 Jacobian
// the recursion of kr_adj.hip applies becomes J = Jp + Jn X, X = [identity on y; rows 19..24 of Jp; identity on tf]:
// per point a lane's tangents d[o] gain its own column of Jn (y and tf lanes) and sum_k Jn[o][19 + k] d[19 + k] over the six
// z columns - applied to a cotangent w as own (Jn^T w)[col] + sum_k d[19 + k] (Jn^T w)[19 + k], see adj_nn_column.  Pass 1, the 6 x 6 solve, pass 2 and the outputs are those of kr_adj.hip, whose kernel this
// one repeats with these additions (step_vjp_kernel keeps its text: the MLP-off call is bit for bit what it was).
//
// Jn is not formed here: a step is three launches,
//   nn_rows_kernel              x[Q][32] (fp64) of the Q = B (N - 1) stored points: y from state_next, z_phys from the physics at
//                               (y, c1 cur + c2 prev, tf)
//   mlp_input_jacobian*_kernel  Jn of every row on the fp64 matrix cores (kr_nnjac.hip), stored [Q][28][25]: a lane's column
//                               is contiguous
//   step_vjp_nn_kernel          the recursion, one wavefront per rod
// Pass 2 also emits, per point, the row (x_j, c_j) of the weight gradient: c_j = [ds lambda_{j+1} (19); g_z[j] (6)] is the
// cotangent that reaches the network's output at point j, and dL/dW is the ordinary MLP backward pass over these rows.
#include "kr_adj_impl.hpp"

namespace kr {

constexpr int NNA_IN = 28, NNA_ROW = 32, NNA_JAC = 25 * 28;

template <typename T>
struct AdjNn {
  const double* xrows;  // [B (N - 1)][NNA_ROW]: the network's input at every stored point
  const double* jt;     // [B (N - 1)][28][25]: Jn, a column contiguous
  T *nn_x, *nn_g;       // [B][N - 1][NNA_ROW], nullable
};

// The 47 inputs of the point map at the stored state of record `rec`: y of state_next, the history c1 cur + c2 prev on
// its twelve leading slots, the tendon force (values only).  adj_point (kr_adj_impl.hpp) assembles the same values and is
// left as it is: routed through this helper the compiler schedules step_vjp_kernel<float> differently, and that kernel
// keeps its text.
template <typename T>
__device__ __forceinline__ void adj_point_values(const RodConst<double>& P, const AdjArgs<T>& A, int64_t rec, const double (&tf)[3],
                                                 Dual (&in)[47]) {
  const T* y = A.next + rec * KR_SLOTS;
  const T* c = A.cur + rec * KR_SLOTS;
  const T* p = A.prev + rec * KR_SLOTS;
#pragma unroll
  for (int k = 0; k < 19; ++k) in[k].v = (double)y[adj_yslot(k)];
#pragma unroll
  for (int k = 19; k < 32; ++k) in[k].v = 0.0;  // (history of p, h, n, m: no equation reads it)
#pragma unroll
  for (int k = 0; k < 12; ++k) in[32 + k].v = P.c1 * (double)c[k] + P.c2 * (double)p[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) in[44 + k].v = tf[k];
}

// x of every stored point of every rod, one thread per point
template <typename T>
__global__ __launch_bounds__(256) void nn_rows_kernel(const RodConst<double> P, const AdjArgs<T> A, double* __restrict__ xrows) {
  const int N = P.N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.B * (N - 1)) return;
  const int64_t rod = i / (N - 1), rec = rod * N + i % (N - 1);
  double tens[4], tf[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) tens[k] = (double)A.tens[rod * A.tens_stride + k];
#pragma unroll
  for (int c = 0; c < 3; ++c) tf[c] = tens[0] * P.tdirs[c] + tens[1] * P.tdirs[3 + c] + tens[2] * P.tdirs[6 + c] + tens[3] * P.tdirs[9 + c];
  Dual in[47], out[25];
  adj_point_values(P, A, rec, tf, in);
#pragma unroll
  for (int k = 0; k < 47; ++k) in[k].d = 0.0;
  point_map_dual(P, in, false, out);  // (the values of adj_point: z_phys = out[19..24].v)
  double* x = xrows + i * NNA_ROW;
#pragma unroll
  for (int k = 0; k < 19; ++k) x[k] = in[k].v;
#pragma unroll
  for (int k = 0; k < 6; ++k) x[19 + k] = out[19 + k].v;
#pragma unroll
  for (int k = 0; k < 3; ++k) x[25 + k] = tf[k];
#pragma unroll
  for (int k = NNA_IN; k < NNA_ROW; ++k) x[k] = 0.0;
}

// The network's part of J^T w, w = [ds lambda; g_z] (25 values), without ever forming the lane's 25 network tangents:
//   sum_o w_o (Jn X)[o][lane's direction] = own u[col] + sum_k d[19 + k] u[19 + k],      u = Jn^T w  (28 values)
// Lane c < 25 forms u[c] from column c of Jn (lanes 19..24, the history lanes, hold the six z columns for everybody), lanes
// 31..33 the tf columns 25..27: 25 loads of the lane's own contiguous column per point, and six broadcasts per cotangent.
// `own`: lanes 0..18 and 31..33, whose input direction IS an input of the network.
template <typename T>
__device__ __forceinline__ void adj_nn_column(const AdjNn<T>& NN, int64_t q, int lane, double (&jc)[25], bool& bad) {
  const int col = lane < 25 ? lane : (lane >= 31 && lane < 34 ? lane - 6 : 0);  // (an index, not a choice between pointers)
  const double* __restrict__ J = NN.jt + q * NNA_JAC + col * 25;
#pragma unroll
  for (int o = 0; o < 25; ++o) {
    jc[o] = J[o];
    bad = bad || !isfinite(jc[o]);
  }
}
// acc += sum_{o < 19} x_o d[o], un += sum_{o < 19} x_o jc[o]  (adj_dot19 with the network's column riding on its broadcasts)
template <int O = 0>
__device__ __forceinline__ void adj_dot19_nn(double x, const double (&d)[25], const double (&jc)[25], double& acc, double& un) {
  if constexpr (O < 19) {
    const double b = adj_bcast<O>(x);
    acc = fma(b, d[O], acc);
    un = fma(b, jc[O], un);
    adj_dot19_nn<O + 1>(x, d, jc, acc, un);
  }
}
__device__ __forceinline__ double adj_nn_term(double u, bool own, const double (&d)[25]) {
  double r = own ? u : 0.0;
  r = fma(d[19], adj_bcast<19>(u), r); r = fma(d[20], adj_bcast<20>(u), r); r = fma(d[21], adj_bcast<21>(u), r);
  r = fma(d[22], adj_bcast<22>(u), r); r = fma(d[23], adj_bcast<23>(u), r); r = fma(d[24], adj_bcast<24>(u), r);
  return r;
}

template <typename T>
__global__ __launch_bounds__(64 * ADJ_RODS_PER_WG) void step_vjp_nn_kernel(const RodConst<double> P, const AdjArgs<T> A, const AdjNn<T> NN) {
  const int lane = threadIdx.x & 63;
  const int64_t rod = (int64_t)blockIdx.x * ADJ_RODS_PER_WG + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (rod >= A.B) return;  // (the whole wavefront: nothing below crosses wavefronts)
  const int N = P.N;
  const int64_t rec0 = rod * N;
  const int64_t q0 = rod * (N - 1);  // first row of this rod in the network arrays
  const bool own = lane < 19 || (lane >= 31 && lane < 34);
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
    double jc[25];
    adj_nn_column(NN, q0 + j, lane, jc, bad);
    if (lane < NNA_IN) bad = bad || !isfinite(NN.xrows[(q0 + j) * NNA_ROW + lane]);
    const T* g = A.g_next + (rec0 + j) * KR_SLOTS;
    double gz[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) gz[k] = (double)g[SL_V + k];
#pragma unroll
    for (int k = 0; k < SL_USED; ++k) bad |= !isfinite((double)g[k]);
    double acc = 0.0, un = 0.0;
    adj_dot19_nn(lam[0], d, jc, acc, un);
    acc *= P.ds;
    un *= P.ds;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      acc = fma(gz[k], d[19 + k], acc);
      un = fma(gz[k], jc[19 + k], un);
    }
    lam[0] = ((double)g[yslot] + lam[0]) + (acc + adj_nn_term(un, own, d));
#pragma unroll
    for (int s = 1; s < ADJ_SEEDS; ++s) {
      double as = 0.0, us = 0.0;
      adj_dot19_nn(lam[s], d, jc, as, us);
      lam[s] = (lam[s] + P.ds * as) + adj_nn_term(P.ds * us, own, d);  // (the physics sum first, as step_vjp_kernel forms it)
    }
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
  bad = __any(bad);  // (lanes read different columns of Jn and different entries of x: this is what makes it uniform)
  const bool solved = adj_solve6(m, a, nu);
  const int st = bad ? KR_ST_NONFINITE : (solved ? KR_ST_CONVERGED : KR_ST_MAXIT);
  if (A.status && lane == 0) A.status[rod * A.st_stride] = st;

  T* oc = A.g_cur ? A.g_cur + rec0 * KR_SLOTS : nullptr;
  T* op = A.g_prev ? A.g_prev + rec0 * KR_SLOTS : nullptr;
  T* ot = A.g_tens ? A.g_tens + rod * A.g_tens_stride : nullptr;
  T* ob = A.g_bnd ? A.g_bnd + rod * KR_BND : nullptr;

  T* ox = NN.nn_x ? NN.nn_x + q0 * NNA_ROW : nullptr;
  T* og = NN.nn_g ? NN.nn_g + q0 * NNA_ROW : nullptr;
  if (st != KR_ST_CONVERGED) {  // no gradient: NaN in every value that carries one, zero where the structure is zero
    if (lane < NNA_ROW)
      for (int j = 0; j < N - 1; ++j) {  // (the rows keep their inputs; their cotangents carry no gradient)
        if (ox) ox[(int64_t)j * NNA_ROW + lane] = lane < NNA_IN ? (T)NN.xrows[(q0 + j) * NNA_ROW + lane] : (T)0;
        if (og) og[(int64_t)j * NNA_ROW + lane] = lane < 25 ? (T)nan : (T)0;
      }
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
    double jc[25];
    adj_nn_column(NN, q0 + j, lane, jc, unused);
    const T* g = A.g_next + (rec0 + j) * KR_SLOTS;
    if (lane < NNA_ROW) {  // the row of the weight gradient: the network's input and the cotangent that reaches its output
      const int zs = lane >= 19 && lane < 25 ? SL_V + lane - 19 : 0;
      const double cz = (double)g[zs];
      if (ox) ox[(int64_t)j * NNA_ROW + lane] = lane < NNA_IN ? (T)NN.xrows[(q0 + j) * NNA_ROW + lane] : (T)0;
      if (og) og[(int64_t)j * NNA_ROW + lane] = lane < 19 ? (T)(P.ds * lm) : (lane < 25 ? (T)cz : (T)0);
    }
    double acc = 0.0, un = 0.0;
    adj_dot19_nn(lm, d, jc, acc, un);
    acc *= P.ds;
    un *= P.ds;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      acc = fma((double)g[SL_V + k], d[19 + k], acc);
      un = fma((double)g[SL_V + k], jc[19 + k], un);
    }
    acc += adj_nn_term(un, own, d);
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


// rows, Jacobian, adjoint: the three launches of one step.  ws: xrows [Q][32] then jt [Q][700], doubles
template <typename T>
static int launch_step_vjp_nn(kr_handle* h, const AdjArgs<T>& A, T* nn_x, T* nn_g, double* ws, hipStream_t s) {
  const int64_t Q = A.B * (h->params.N - 1);
  double* xrows = ws;
  double* jt = ws + Q * NNA_ROW;
  hipLaunchKernelGGL((nn_rows_kernel<T>), dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, h->cd, A, xrows);
  KR_HIP(hipGetLastError());
  if (int rc = launch_nnjac<double>(h, Q, xrows, NNA_ROW, jt, 1, s)) return rc;
  const AdjNn<T> NN{xrows, jt, nn_x, nn_g};
  const int64_t grid = (A.B + ADJ_RODS_PER_WG - 1) / ADJ_RODS_PER_WG;
  hipLaunchKernelGGL((step_vjp_nn_kernel<T>), dim3((unsigned)grid), dim3(64 * ADJ_RODS_PER_WG), 0, s, h->cd, A, NN);
  KR_HIP(hipGetLastError());
  return KR_OK;
}
static size_t nn_ws_doubles(const kr_handle* h, int64_t B) { return (size_t)B * (h->params.N - 1) * (NNA_ROW + NNA_JAC); }

// kr_simulate_vjp_batch's composition (kr_adj.hip) with the network's three launches per step
template <typename T>
static int simulate_vjp_nn(kr_handle* h, int64_t B, int64_t T_steps, const T* ctl, const T* states, const T* prev_init, T* g_states,
                           T* g_prev_init, T* g_ctl, T* g_bnd, double* resid, int32_t* status, T* nn_x, T* nn_g, hipStream_t s) {
  const int64_t slot = B * h->params.N * KR_SLOTS;
  const int64_t rows = B * (h->params.N - 1) * NNA_ROW;
  const size_t head = ((size_t)(2 * slot + B * KR_BND) * sizeof(T) + 255) / 256 * 256;
  if (int rc = ensure_ws(h, head + nn_ws_doubles(h, B) * sizeof(double))) return rc;
  T* w_cur = static_cast<T*>(h->ws);
  T* w_prev = w_cur + slot;
  T* w_bnd = w_prev + slot;
  double* w_nn = reinterpret_cast<double*>(static_cast<char*>(h->ws) + head);
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
    if (int rc = launch_step_vjp_nn<T>(h, A, nn_x ? nn_x + t * rows : nullptr, nn_g ? nn_g + t * rows : nullptr, w_nn, s)) return rc;
    if (int rc = launch_add<T>(g_states + t * slot, w_cur, slot, s)) return rc;
    if (!into_init)
      if (int rc = launch_add<T>(g_states + (t > 0 ? t - 1 : 0) * slot, w_prev, slot, s)) return rc;
    if (g_bnd)
      if (int rc = launch_add<T>(g_bnd, w_bnd, B * KR_BND, s)) return rc;
  }
  return KR_OK;
}

static int adj_nn_refuse(const kr_handle* h, const char* api, int scheme) {
  if (int rc = nnjac_check(h, api)) return rc;
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

extern "C" int kr_step_vjp_nn_batch(kr_handle* h, int64_t B, int scheme, const void* state_prev, const void* state_cur,
                                    const void* state_next, const void* tensions, const void* g_next, void* g_cur, void* g_prev,
                                    void* g_tensions, void* g_bnd, double* resid, int32_t* status, void* nn_x, void* nn_g,
                                    int dtype, void* stream) {
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_ADJ_ARG(B < 1 || B > 0x7FFFFFFFll, "kr_step_vjp_nn_batch: B must be in [1, 2^31 - 1]");
  KR_ADJ_ARG(!state_prev || !state_cur || !state_next || !tensions || !g_next, "kr_step_vjp_nn_batch: null pointer argument");
  if (int rc = adj_nn_refuse(h, "kr_step_vjp_nn_batch", scheme)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  if (int rc = ensure_ws(h, nn_ws_doubles(h, B) * sizeof(double))) return rc;
  double* ws = static_cast<double*>(h->ws);
  if (dtype == KR_F32) {
    AdjArgs<float> A{B, (const float*)state_prev, (const float*)state_cur, (const float*)state_next, (const float*)tensions, 4,
                     (const float*)g_next, (float*)g_cur, (float*)g_prev, (float*)g_tensions, 4, (float*)g_bnd, resid, status, 1};
    return launch_step_vjp_nn<float>(h, A, (float*)nn_x, (float*)nn_g, ws, s);
  }
  AdjArgs<double> A{B, (const double*)state_prev, (const double*)state_cur, (const double*)state_next, (const double*)tensions, 4,
                    (const double*)g_next, (double*)g_cur, (double*)g_prev, (double*)g_tensions, 4, (double*)g_bnd, resid, status, 1};
  return launch_step_vjp_nn<double>(h, A, (double*)nn_x, (double*)nn_g, ws, s);
}

extern "C" int kr_simulate_vjp_nn_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, const void* states,
                                        const void* state_prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd,
                                        double* resid, int32_t* status, void* nn_x, void* nn_g, int dtype, void* stream) {
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_ADJ_ARG(B < 1 || B > 0x7FFFFFFFll, "kr_simulate_vjp_nn_batch: B must be in [1, 2^31 - 1]");
  KR_ADJ_ARG(T < 1, "kr_simulate_vjp_nn_batch: T < 1");
  KR_ADJ_ARG(!ctl || !states || !g_states, "kr_simulate_vjp_nn_batch: null pointer argument");
  if (int rc = adj_nn_refuse(h, "kr_simulate_vjp_nn_batch", scheme)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  if (dtype == KR_F32)
    return simulate_vjp_nn<float>(h, B, T, (const float*)ctl, (const float*)states, (const float*)state_prev_init, (float*)g_states,
                                  (float*)g_prev_init, (float*)g_ctl, (float*)g_bnd, resid, status, (float*)nn_x, (float*)nn_g, s);
  return simulate_vjp_nn<double>(h, B, T, (const double*)ctl, (const double*)states, (const double*)state_prev_init,
                                 (double*)g_states, (double*)g_prev_init, (double*)g_ctl, (double*)g_bnd, resid, status,
                                 (double*)nn_x, (double*)nn_g, s);
}
