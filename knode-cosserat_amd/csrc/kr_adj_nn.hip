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
// z columns - applied to a cotangent w as own (Jn^T w)[col] + sum_k d[19 + k] (Jn^T w)[19 + k], see adj_nn_column
// (kr_adj_impl.hpp).  Pass 1, the 6 x 6 solve, pass 2 and the outputs are those of kr_adj.hip: the kernel is the same text,
// kr_adj_body.inc, with NNON on, and these additions are its `if constexpr (NNON)` statements (with NNON off they leave no
// trace: the MLP-off call is bit for bit what it was).  The rollout call is kr_adj.hip's composition, simulate_vjp_steps,
// with the three launches below per step and their doubles in its workspace tail.
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

// (adj_point_values, the 47 inputs of the point map at a stored record: kr_adj_impl.hpp, shared with kr_adj_bank.hip)
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

template <typename T>
__global__ __launch_bounds__(64 * ADJ_RODS_PER_WG) void step_vjp_nn_kernel(const RodConst<double> P, const AdjArgs<T> A, const AdjNn<T> NN) {
  constexpr bool PAR = false, NNON = true;
  const AdjPar<T> Q{};  // (named in the discarded PAR statements only)
#include "kr_adj_body.inc"
}

// rows, Jacobian, adjoint: the three launches of step t.  ws: xrows [Q][32] then jt [Q][700], doubles; nn_x, nn_g: of step 0
template <typename T>
static int launch_step_vjp_nn(kr_handle* h, const AdjArgs<T>& A, void* nn_x, void* nn_g, int64_t t, void* ws, hipStream_t s) {
  const int64_t Q = A.B * (h->params.N - 1);
  double* xrows = static_cast<double*>(ws);
  double* jt = xrows + Q * NNA_ROW;
  hipLaunchKernelGGL((nn_rows_kernel<T>), dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, h->cd, A, xrows);
  KR_HIP(hipGetLastError());
  if (int rc = launch_nnjac<double>(h, Q, xrows, NNA_ROW, jt, 1, s)) return rc;
  const AdjNn<T> NN{xrows, jt, nn_x ? static_cast<T*>(nn_x) + t * Q * NNA_ROW : nullptr,
                    nn_g ? static_cast<T*>(nn_g) + t * Q * NNA_ROW : nullptr};
  const int64_t grid = (A.B + ADJ_RODS_PER_WG - 1) / ADJ_RODS_PER_WG;
  hipLaunchKernelGGL((step_vjp_nn_kernel<T>), dim3((unsigned)grid), dim3(64 * ADJ_RODS_PER_WG), 0, s, h->cd, A, NN);
  KR_HIP(hipGetLastError());
  return KR_OK;
}
static size_t nn_ws_bytes(const kr_handle* h, int64_t B) { return (size_t)B * (h->params.N - 1) * (NNA_ROW + NNA_JAC) * sizeof(double); }

// nnjac_check's refusals, then the scheme half of adj_refuse
static int adj_nn_refuse(const kr_handle* h, const char* api, int scheme) {
  if (int rc = nnjac_check(h, api)) return rc;
  return adj_refuse(api, scheme, 0);
}

}  // namespace kr

using namespace kr;

extern "C" int kr_step_vjp_nn_batch(kr_handle* h, int64_t B, int scheme, const void* state_prev, const void* state_cur,
                                    const void* state_next, const void* tensions, const void* g_next, void* g_cur, void* g_prev,
                                    void* g_tensions, void* g_bnd, double* resid, int32_t* status, void* nn_x, void* nn_g,
                                    int dtype, void* stream) {
  return adj_step_entry("kr_step_vjp_nn_batch", h, B, state_prev, state_cur, state_next, tensions, g_next, g_cur, g_prev, g_tensions,
                        g_bnd, resid, status, dtype, stream, [=](const char* api) { return adj_nn_refuse(h, api, scheme); },
                        [=](kr_handle* hh, const auto& A, hipStream_t s) {
                          if (int rc = ensure_ws(hh, nn_ws_bytes(hh, A.B))) return rc;
                          return launch_step_vjp_nn(hh, A, nn_x, nn_g, 0, hh->ws, s);
                        });
}

// kr_simulate_vjp_batch's composition (simulate_vjp_steps) with the network's three launches per step, their doubles in its tail
extern "C" int kr_simulate_vjp_nn_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, const void* states,
                                        const void* state_prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd,
                                        double* resid, int32_t* status, void* nn_x, void* nn_g, int dtype, void* stream) {
  return adj_simulate_entry("kr_simulate_vjp_nn_batch", h, B, T, ctl, states, state_prev_init, g_states, g_prev_init, g_ctl, g_bnd,
                            nullptr, resid, status, dtype, stream, [=](const char* api) { return adj_nn_refuse(h, api, scheme); },
                            h ? nn_ws_bytes(h, B) : 0,
                            [=](kr_handle* hh, const auto& A, void* ws, int64_t t, hipStream_t s) {
                              return launch_step_vjp_nn(hh, A, nn_x, nn_g, t, ws, s);
                            });
}
