// kr_adj_impl.hpp - what the three forms of the step adjoint share: the argument blocks, the lane helpers, the per-point
// tangents of the physics on dual numbers, the network's and the parameters' additions to them, the 6 x 6 solve, the ONE
// composition over a stored rollout with its accumulation kernel, and the ONE path from a C entry point to a launch
// (adj_step_entry, adj_simulate_entry).  The forms are kr_adj.hip (MLP off), kr_adj_par.hip (MLP off, with the gradient of
// the material parameters), kr_adj_nn.hip (the network's input Jacobian added to the per-point derivative), kr_adj_tab.hip
// (MLP off, rod b with row b of a parameter table, without and with the parameter gradient) and kr_adj_bank.hip (MLP on, rod
// b with row b of a table and network net_of_rod[b] of a bank); the mapping is described in kr_adj.hip.  The recursion of one
// rod, the body of every step kernel, is kr_adj_body.inc.
#pragma once
#include "kr_internal.hpp"
#include "kr_point_dual.hpp"

namespace kr {

template <typename T>
struct AdjArgs {
  int64_t B;
  const T *prev, *cur, *next;  // [B][N][KR_SLOTS]
  const T* tens;               // tensions of rod b at tens[b * tens_stride .. + 4]
  int64_t tens_stride;
  const T* g_next;             // [B][N][KR_SLOTS]
  T *g_cur, *g_prev;           // [B][N][KR_SLOTS], nullable
  T* g_tens;                   // rod b at g_tens[b * g_tens_stride .. + 4], nullable
  int64_t g_tens_stride;
  T* g_bnd;                    // [B][KR_BND], nullable
  double* resid;               // rod b at resid[b * st_stride], nullable
  int32_t* status;             // rod b at status[b * st_stride], nullable
  int64_t st_stride;
};

constexpr int ADJ_RODS_PER_WG = 4;
constexpr int ADJ_SEEDS = 7;

template <int SRC>
__device__ __forceinline__ double adj_bcast(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), SRC), hi = __builtin_amdgcn_readlane((int)(b >> 32), SRC);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// sum over o < 19 of x_o d[o], x_o = component o of the vector whose components lanes 0..18 hold in `x`
template <int O = 0>
__device__ __forceinline__ double adj_dot19(double x, const double (&d)[25], double acc) {
  if constexpr (O < 19) return adj_dot19<O + 1>(x, d, fma(adj_bcast<O>(x), d[O], acc));
  else return acc;
}
// row r of y (reference order p h n m q w) -> slot of the packed record
__device__ __forceinline__ int adj_yslot(int r) { return r < 13 ? r + 12 : r - 13; }

// One grid point: the tangents d[25] of (y_s, z) along this lane's input direction, at the stored state of point j.
// `bad` collects a value that is not finite among everything read.
template <typename T>
__device__ __forceinline__ void adj_point(const RodConst<double>& P, const AdjArgs<T>& A, int64_t rec, int dir, const double (&tf)[3],
                                          double (&d)[25], bool& bad) {
  Dual in[47], out[25];
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
#pragma unroll
  for (int k = 0; k < 47; ++k) {
    bad |= !isfinite(in[k].v);
    in[k].d = k == dir ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) bad |= !isfinite((double)y[SL_V + k]);
  point_map_dual(P, in, false, out);
#pragma unroll
  for (int o = 0; o < 25; ++o) d[o] = out[o].d;
}

// nu of M^T nu = -a: Gaussian elimination with partial pivoting, every lane the same arithmetic on the same values.
// m[k][l] = d(n, m)_k / dG_l.  false: a pivot that is zero, not finite, or below 1e-13 of the largest entry.
__device__ __forceinline__ bool adj_solve6(const double (&m)[6][6], const double (&a)[6], double (&nu)[6]) {
  double w[6][7];
  double amax = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      w[r][c] = m[c][r];
      amax = fmax(amax, fabs(m[c][r]));
    }
    w[r][6] = -a[r];
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int p = c;
    double best = fabs(w[c][c]);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double v = fabs(w[r][c]);
      if (v > best) { best = v; p = r; }
    }
    ok = ok && best > 1e-13 * amax && isfinite(best);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const bool sw = r == p;
#pragma unroll
      for (int k = c; k < 7; ++k) {
        const double top = w[c][k], low = w[r][k];
        w[c][k] = sw ? low : top;
        w[r][k] = sw ? top : low;
      }
    }
    const double inv = 1.0 / w[c][c];
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double f = w[r][c] * inv;
#pragma unroll
      for (int k = c + 1; k < 7; ++k) w[r][k] = fma(-f, w[c][k], w[r][k]);
    }
  }
#pragma unroll
  for (int r = 5; r >= 0; --r) {
    double s = w[r][6];
#pragma unroll
    for (int k = r + 1; k < 6; ++k) s = fma(-w[r][k], nu[k], s);
    nu[r] = s / w[r][r];
  }
  return ok;
}

// ---- the gradient of the material parameters (kr_adj_par.hip) ----
// What the parameter kernel takes beside AdjArgs: the output and the parameters that kr_derive turns into the constants of
// the point map (Bse, Bbt, C and c0 are in RodConst as they are).
template <typename T>
struct AdjPar {
  T* g_par;  // [B][KR_PAR]
  double E, r, rho, vstar[3], g[3];
};
constexpr int ADJ_PAR_LANE0 = 34;  // lane ADJ_PAR_LANE0 + k: direction k of E, r, rho, vstar[3], g[3], Bse[9], Bbt[9], C[3]
constexpr int ADJ_PAR_DIRS = 30;

// The constants the point map reads, as dual numbers (point_map_dual's PC)
struct RodConstDual {
  double c0;
  Dual rhoA;
  Dual Ksei[9], Kbti[9], Bse[9], Bbt[9], rhoJ[9];
  Dual Kse_vstar[3], rhoAg[3], C[3];
};

// d(M^-1) = -M^-1 dM M^-1 with dM = diag(dk) + c0 sel (sel: the unit tangent of a B entry, or zero)
__device__ __forceinline__ void adj_dinv3(const double (&Mi)[9], const double (&dk)[3], double c0, const double (&sel)[9], double (&o)[9]) {
  double t[9];  // dM M^-1
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double a = dk[i] * Mi[3 * i + j];
#pragma unroll
      for (int l = 0; l < 3; ++l) a = fma(c0 * sel[3 * i + l], Mi[3 * l + j], a);
      t[3 * i + j] = a;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[3 * i + j] = -(Mi[3 * i] * t[j] + Mi[3 * i + 1] * t[3 + j] + Mi[3 * i + 2] * t[6 + j]);
}

// The constants with their tangents along direction k (k outside 0..29: no tangent): the chain of kr_derive
// (cosserat_ode.py:58-78) - G = E / 2.6, A = pi r^2, J = pi r^4 (1/4, 1/4, 1/2), Kse = (G A, G A, E A), Kbt = (E J, E J, G J),
// the inverses of Kse + c0 Bse and Kbt + c0 Bbt, Kse vstar, rho A, rho A g, rho J.  The VALUES are those of P.
template <typename T>
__device__ __forceinline__ void adj_par_consts(const RodConst<double>& P, const AdjPar<T>& Q, int k, RodConstDual& D) {
  const double pi = 3.14159265358979323846;
  const double sE = k == 0 ? 1.0 : 0.0, sr = k == 1 ? 1.0 : 0.0, srho = k == 2 ? 1.0 : 0.0;
  const double r2 = Q.r * Q.r, r3 = r2 * Q.r, r4 = r2 * r2;
  const double A = pi * r2, G = Q.E / 2.6, dA = sr * 2.0 * pi * Q.r, dG = sE / 2.6;
  const double J[3] = {pi * r4 / 4, pi * r4 / 4, pi * r4 / 2};
  const double dJ[3] = {sr * pi * r3, sr * pi * r3, sr * 2.0 * pi * r3};
  const double Kse[3] = {G * A, G * A, Q.E * A};
  const double dKse[3] = {dG * A + G * dA, dG * A + G * dA, sE * A + Q.E * dA};
  const double dKbt[3] = {sE * J[0] + Q.E * dJ[0], sE * J[1] + Q.E * dJ[1], dG * J[2] + G * dJ[2]};
  double sBse[9], sBbt[9], dKsei[9], dKbti[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    sBse[e] = k == 9 + e ? 1.0 : 0.0;
    sBbt[e] = k == 18 + e ? 1.0 : 0.0;
  }
  adj_dinv3(P.Ksei, dKse, P.c0, sBse, dKsei);
  adj_dinv3(P.Kbti, dKbt, P.c0, sBbt, dKbti);
  const double drhoA = srho * A + Q.rho * dA;
  D.c0 = P.c0;
  D.rhoA = {P.rhoA, drhoA};
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    D.Ksei[e] = {P.Ksei[e], dKsei[e]};
    D.Kbti[e] = {P.Kbti[e], dKbti[e]};
    D.Bse[e] = {P.Bse[e], sBse[e]};
    D.Bbt[e] = {P.Bbt[e], sBbt[e]};
    D.rhoJ[e] = {P.rhoJ[e], e % 4 == 0 ? srho * J[e / 4] + Q.rho * dJ[e / 4] : 0.0};
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    D.Kse_vstar[i] = {P.Kse_vstar[i], dKse[i] * Q.vstar[i] + (k == 3 + i ? Kse[i] : 0.0)};
    D.rhoAg[i] = {P.rhoAg[i], drhoA * Q.g[i] + (k == 6 + i ? P.rhoA : 0.0)};
    D.C[i] = {P.C[i], k == 27 + i ? 1.0 : 0.0};
  }
}

// One grid point along a parameter direction: the tangents d[25] of (y_s, z) with the INPUTS held fixed and the constants
// carrying the tangent, and the values val[25] of (y_s, z) themselves (what d ds / d L multiplies).
template <typename T>
__device__ __forceinline__ void adj_point_par(const RodConstDual& D, double c1, double c2, const AdjArgs<T>& A, int64_t rec,
                                              const double (&tf)[3], double (&d)[25], double (&val)[25]) {
  double in[47];  // (plain inputs: the tangent runs along the constants alone)
  Dual out[25];
  const T* y = A.next + rec * KR_SLOTS;
  const T* c = A.cur + rec * KR_SLOTS;
  const T* p = A.prev + rec * KR_SLOTS;
#pragma unroll
  for (int k = 0; k < 19; ++k) in[k] = (double)y[adj_yslot(k)];
#pragma unroll
  for (int k = 19; k < 32; ++k) in[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) in[32 + k] = c1 * (double)c[k] + c2 * (double)p[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) in[44 + k] = tf[k];
  point_map_dual(D, in, false, out);
#pragma unroll
  for (int o = 0; o < 25; ++o) {
    d[o] = out[o].d;
    val[o] = out[o].v;
  }
}

// ---- the network's input Jacobian in the per-point derivative (kr_adj_nn.hip) ----
constexpr int NNA_IN = 28, NNA_ROW = 32, NNA_JAC = 25 * 28;

template <typename T>
struct AdjNn {
  const double* xrows;  // [B (N - 1)][NNA_ROW]: the network's input at every stored point
  const double* jt;     // [B (N - 1)][28][25]: Jn, a column contiguous
  T *nn_x, *nn_g;       // [B][N - 1][NNA_ROW], nullable
};

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

// The 47 inputs of the point map at the stored state of record `rec`: y of state_next, the history c1 cur + c2 prev on
// its twelve leading slots, the tendon force (values only), for nn_rows_kernel (kr_adj_nn.hip) and nn_rows_bank_kernel
// (kr_adj_bank.hip).  adj_point above assembles the same values and is left as it is: routed through this helper the compiler schedules step_vjp_kernel<float> differently,
// and that kernel keeps its text.
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

// ---- a rod's table row in place (kr_adj_tab.hip, kr_adj_bank.hip) ----
// this wavefront's rod (the body's own statement: the same value, so the compiler keeps one)
__device__ __forceinline__ int64_t adj_tab_rod() {
  return (int64_t)blockIdx.x * ADJ_RODS_PER_WG + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}
__device__ __forceinline__ const RodConst<double>& adj_tab_row(const KR_CONSTANT_AS RodConst<double>* rows, int64_t rod) {
  const int row = __builtin_amdgcn_readfirstlane((int)rod);
  return *(const RodConst<double>*)(rows + row);
}

template <typename T>
__global__ __launch_bounds__(256) void adj_add_kernel(T* dst, const T* src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = dst[i] + src[i];
}

template <typename T>
static int launch_add(T* dst, const T* src, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL((adj_add_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, src, n);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

// dst[b][k] = src[b][k], k < KR_BND, the rows of dst `stride` elements apart: the step's boundary gradient put where a
// per-step rollout keeps it (kr_adj_tab.hip: adj_put_kernel; n = B KR_BND)
int launch_put(float* dst, const float* src, int64_t n, int64_t stride, hipStream_t s);
int launch_put(double* dst, const double* src, int64_t n, int64_t stride, hipStream_t s);

int launch_step_vjp_plain(kr_handle* h, const AdjArgs<float>& A, hipStream_t s);   // (kr_adj.hip: step_vjp_kernel)
int launch_step_vjp_plain(kr_handle* h, const AdjArgs<double>& A, hipStream_t s);

// The backward pass over a stored rollout, DEFINED as this composition of step adjoints (t = T - 1 .. 0):
//   step adjoint of (states[t - 1], states[t], states[t + 1], ctl[:, t]) with g_next = g_states[t + 1]
//   g_states[t] += g_cur;  g_states[t - 1] += g_prev  (in this order, in the element type of the arrays)
//   g_bnd += the step's, g_par += the step's (from zero, t = T - 1 first)
//   bnd_per_step (the table form): g_bnd is [B][T][KR_BND] and g_bnd[b][t] = the step's, copied instead of added
// The workspace is a T-typed head (w_cur, w_prev, w_bnd) and, at the next 256-byte boundary, the tail_bytes the form asks
// for: w_par[B][KR_PAR] of T with g_par, the network's rows and Jacobians (doubles) with the MLP on.
// launch(h, A, tail, t, s): the step adjoint of step t (tail: null when tail_bytes is 0)
template <typename T, typename Launch>
static int simulate_vjp_steps(kr_handle* h, int64_t B, int64_t T_steps, const T* ctl, const T* states, const T* prev_init, T* g_states,
                              T* g_prev_init, T* g_ctl, T* g_bnd, T* g_par, double* resid, int32_t* status, size_t tail_bytes,
                              hipStream_t s, Launch launch, bool bnd_per_step = false) {
  const int64_t slot = B * h->params.N * KR_SLOTS;
  const size_t head = ((size_t)(2 * slot + B * KR_BND) * sizeof(T) + 255) / 256 * 256;
  if (int rc = ensure_ws(h, head + tail_bytes)) return rc;
  T* w_cur = static_cast<T*>(h->ws);
  T* w_prev = w_cur + slot;
  T* w_bnd = w_prev + slot;
  void* tail = tail_bytes ? static_cast<char*>(h->ws) + head : nullptr;
  T* w_par = static_cast<T*>(tail);  // (read with g_par only)
  if (g_bnd && !bnd_per_step) KR_HIP(hipMemsetAsync(g_bnd, 0, (size_t)B * KR_BND * sizeof(T), s));
  if (g_par) KR_HIP(hipMemsetAsync(g_par, 0, (size_t)B * KR_PAR * sizeof(T), s));
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
    if (int rc = launch(h, A, tail, t, s)) return rc;
    if (int rc = launch_add<T>(g_states + t * slot, w_cur, slot, s)) return rc;
    if (!into_init)
      if (int rc = launch_add<T>(g_states + (t > 0 ? t - 1 : 0) * slot, w_prev, slot, s)) return rc;
    if (g_bnd)
      if (int rc = bnd_per_step ? launch_put(g_bnd + t * KR_BND, w_bnd, B * KR_BND, T_steps * KR_BND, s)
                                : launch_add<T>(g_bnd, w_bnd, B * KR_BND, s))
        return rc;
    if (g_par)
      if (int rc = launch_add<T>(g_par, w_par, B * KR_PAR, s)) return rc;
  }
  return KR_OK;
}

// The refusals of the MLP-off forms: use_nn, then the scheme (the scheme half is the MLP-on form's too)
int adj_refuse(const char* api, int scheme, int use_nn);  // (kr_adj.hip)
// The refusals of the table forms: the table against the handle (device, N, del_t), then the scheme
int adj_tab_refuse(const char* api, const kr_handle* h, const kr_param_table* t, int scheme);  // (kr_adj_tab.hip)

// ---- from a C entry point to its launch ----
// What a caller with two mistakes hears of first: handle, dtype, B, (T,) null pointers, the form's refusal, stream ordering.
#define KR_ADJ_ARG(cond, msg) \
  if (cond) {                 \
    set_error(msg);           \
    return KR_E_ARG;          \
  }

// A step call.  refuse(api): the form's refusals; launch(h, A, s): the form's step adjoint of AdjArgs<float or double>.
template <typename Refuse, typename Launch>
static int adj_step_entry(const char* api, kr_handle* h, int64_t B, const void* state_prev, const void* state_cur, const void* state_next,
                          const void* tensions, const void* g_next, void* g_cur, void* g_prev, void* g_tensions, void* g_bnd,
                          double* resid, int32_t* status, int dtype, void* stream, Refuse refuse, Launch launch) {
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_ADJ_ARG(B < 1 || B > 0x7FFFFFFFll, std::string(api) + ": B must be in [1, 2^31 - 1]");
  KR_ADJ_ARG(!state_prev || !state_cur || !state_next || !tensions || !g_next, std::string(api) + ": null pointer argument");
  if (int rc = refuse(api)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  auto run = [&](auto* elem) {
    using T = std::remove_pointer_t<decltype(elem)>;
    const AdjArgs<T> A{B, (const T*)state_prev, (const T*)state_cur, (const T*)state_next, (const T*)tensions, 4,
                       (const T*)g_next, (T*)g_cur, (T*)g_prev, (T*)g_tensions, 4, (T*)g_bnd, resid, status, 1};
    return launch(h, A, s);
  };
  return dtype == KR_F32 ? run((float*)nullptr) : run((double*)nullptr);
}

// A rollout call: simulate_vjp_steps in the element type of the arrays.  tail_bytes, launch: as there.
template <typename Refuse, typename Launch>
static int adj_simulate_entry(const char* api, kr_handle* h, int64_t B, int64_t T_steps, const void* ctl, const void* states,
                              const void* prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd, void* g_par,
                              double* resid, int32_t* status, int dtype, void* stream, Refuse refuse, size_t tail_bytes, Launch launch,
                              bool bnd_per_step = false) {
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_ADJ_ARG(B < 1 || B > 0x7FFFFFFFll, std::string(api) + ": B must be in [1, 2^31 - 1]");
  KR_ADJ_ARG(T_steps < 1, std::string(api) + ": T < 1");
  KR_ADJ_ARG(!ctl || !states || !g_states, std::string(api) + ": null pointer argument");
  if (int rc = refuse(api)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  auto run = [&](auto* elem) {
    using T = std::remove_pointer_t<decltype(elem)>;
    return simulate_vjp_steps<T>(h, B, T_steps, (const T*)ctl, (const T*)states, (const T*)prev_init, (T*)g_states, (T*)g_prev_init,
                                 (T*)g_ctl, (T*)g_bnd, (T*)g_par, resid, status, tail_bytes, s, launch, bnd_per_step);
  };
  return dtype == KR_F32 ? run((float*)nullptr) : run((double*)nullptr);
}

}  // namespace kr
