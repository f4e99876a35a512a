// kr_adj_bank.hip - the step adjoint of a heterogeneous batch with the MLP on: rod b takes row b of a parameter table AND
// network net_of_rod[b] of a bank.  The backward side of kr_simulate_batch_bank / kr_simulate_batch_bank_keypoints.
//
//   kr_step_vjp_bank_batch      kr_step_vjp_nn_batch with row b's constants and network net_of_rod[b], per rod
//   kr_simulate_vjp_bank_batch  the same composed over the T steps of a stored trajectory; the boundary gradient summed over
//                               the steps or kept per step, as in kr_simulate_vjp_table_batch
//
// The recursion is kr_adj_body.inc once more (PAR off, NNON on), its names bound per rod before the include as kr_adj_tab.hip
// binds them: P is the rod's row in place, through the constant address space.  The network never enters the recursion - it
// reads Jn and x of the rod's points from two arrays - so "a network per rod" is a matter of which rows those arrays hold
// where.  The Jacobian kernels (kr_nnjac.hip) take ONE network per launch and stay as they are; the rows are ordered by
// network instead:
//   host, once per call   pos = the stable permutation of the rods by net_of_rod (rod b is the pos[b]-th rod in network
//                         order), uploaded once; the rods of network k are then the slots first[k] .. first[k] + count[k] - 1
//   nn_rows_bank_kernel   x of rod b's N - 1 points at rows pos[b] (N - 1) ..., from row b's constants
//   Jacobian              one launch of the existing kernel per network that has rods, on its contiguous range of rows, with
//                         the bank's fp64 descriptor moved by k * stride; a network without rods launches nothing
//   step_vjp_bank_kernel  the body addresses xrows / jt AND nn_x / nn_g through q0 = rod (N - 1): the kernel hands it an AdjNn
//                         whose xrows and jt are moved by (pos[b] - b) (N - 1) rows and whose nn_x, nn_g are not, so the emitted
//                         rows stay in rod order and the body needs no new statement
// A rod's rows, Jacobians and recursion do not depend on the slot: a row of the Jacobian kernels gives the same bits wherever
// in a launch it sits (kr_nnjac.hip), so a rod's bits depend neither on the batch, nor on its place in it, nor on which other
// networks are present.  No atomics.  The rollout is simulate_vjp_steps with this unit's launches; its workspace tail is the
// MLP-on form's (x and Jn) plus the permutation.
#include "kr_adj_impl.hpp"

#include <vector>

namespace kr {

// What the bank kernels take in place of the by-value RodConst<double>: the rows and the permutation, both written by the host
// only and never while a kernel reads them (constant address space from the kernel argument on, like RodTable's pointers)
struct AdjBank {
  const KR_CONSTANT_AS RodConst<double>* rows;  // [B]
  const KR_CONSTANT_AS int32_t* pos;            // [B]: rod b's slot in network order
  int N;                                        // the table's (every row's) N
};

// x of every stored point of every rod, one thread per point: nn_rows_kernel with the rod's own row, written at the rod's slot
template <typename T>
__global__ __launch_bounds__(256) void nn_rows_bank_kernel(const AdjBank TB, const AdjArgs<T> A, double* __restrict__ xrows) {
  const int N = TB.N;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.B * (N - 1)) return;  // (before the row is bound: no row beyond the table's last is addressed)
  const int64_t rod = i / (N - 1), pt = i % (N - 1), rec = rod * N + pt;
  const RodConst<double>& P = *(const RodConst<double>*)(TB.rows + rod);
  double tens[4], tf[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) tens[k] = (double)A.tens[rod * A.tens_stride + k];
#pragma unroll
  for (int c = 0; c < 3; ++c) tf[c] = tens[0] * P.tdirs[c] + tens[1] * P.tdirs[3 + c] + tens[2] * P.tdirs[6 + c] + tens[3] * P.tdirs[9 + c];
  Dual in[47], out[25];
  adj_point_values(P, A, rec, tf, in);
#pragma unroll
  for (int k = 0; k < 47; ++k) in[k].d = 0.0;
  point_map_dual(P, in, false, out);
  double* x = xrows + ((int64_t)TB.pos[rod] * (N - 1) + pt) * NNA_ROW;
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
__global__ __launch_bounds__(64 * ADJ_RODS_PER_WG) void step_vjp_bank_kernel(const AdjBank TB, const AdjArgs<T> A, const AdjNn<T> NA) {
  constexpr bool PAR = false, NNON = true;
  if (adj_tab_rod() >= A.B) return;
  const RodConst<double>& P = adj_tab_row(TB.rows, adj_tab_rod());
  const AdjPar<T> Q{};
  AdjNn<T> NN = NA;
  {
    // rod b's rows of x and Jn lie at slot pos[b]; the body addresses them through q0 = b (N - 1)
    const int row = __builtin_amdgcn_readfirstlane((int)adj_tab_rod());
    const int64_t shift = ((int64_t)TB.pos[row] - row) * (TB.N - 1);
    NN.xrows += shift * NNA_ROW;
    NN.jt += shift * NNA_JAC;
  }
#include "kr_adj_body.inc"
}

// What a call works out on the host before anything is queued: the permutation and the ranges of the networks
struct BankOrder {
  std::vector<int32_t> pos;     // [B]
  std::vector<int64_t> first;   // [K]: first slot of network k
  std::vector<int64_t> count;   // [K]: rods of network k
};
static BankOrder bank_order(const int32_t* net_of_rod, int64_t B, int K) {
  BankOrder o;
  o.pos.resize((size_t)B);
  o.first.assign((size_t)K, 0);
  o.count.assign((size_t)K, 0);
  for (int64_t b = 0; b < B; ++b) ++o.count[net_of_rod[b]];
  for (int k = 1; k < K; ++k) o.first[k] = o.first[k - 1] + o.count[k - 1];
  std::vector<int64_t> next = o.first;
  for (int64_t b = 0; b < B; ++b) o.pos[(size_t)b] = (int32_t)next[net_of_rod[b]]++;
  return o;
}

// the bank's fp64 descriptor of network k: every buffer k * stride bytes behind network 0's (mlp_src_net's rule, on the host)
static MlpDev<double> bank_net(const kr_mlp_bank* bank, int k) {
  MlpDev<double> M = bank->md;
  const size_t off = (size_t)k * bank->stride;
  auto at = [off](auto* p) { return p ? reinterpret_cast<decltype(p)>(reinterpret_cast<const unsigned char*>(p) + off) : p; };
  for (int l = 0; l < KR_MAX_LAYERS; ++l) {
    M.Wt[l] = at(M.Wt[l]); M.b[l] = at(M.b[l]);
    M.wfrag[l] = at(M.wfrag[l]); M.bfrag[l] = at(M.bfrag[l]);
    M.jfrag[l] = at(M.jfrag[l]);
    M.wq[l] = at(M.wq[l]); M.bq[l] = at(M.bq[l]);
    M.w32[l] = at(M.w32[l]); M.b32[l] = at(M.b32[l]);
  }
  return M;
}

static size_t bank_nn_bytes(int N, int64_t B) { return (size_t)B * (N - 1) * (NNA_ROW + NNA_JAC) * sizeof(double); }
static size_t bank_ws_bytes(int N, int64_t B) { return bank_nn_bytes(N, B) + (size_t)B * sizeof(int32_t); }

// ws: xrows [Q][32], jt [Q][700] (doubles, in network order), then pos [B] (int32).  The permutation is uploaded by the first
// launch of a call (`uploaded`), behind whatever the stream still runs on this workspace, and has been read from the caller's
// side when the copy returns (a pageable source is staged before hipMemcpyAsync returns; the stream is waited for as the
// forward bank call does).
template <typename T>
static int launch_step_vjp_bank(const kr_param_table* t, const kr_mlp_bank* bank, const BankOrder& o, bool& uploaded, const AdjArgs<T>& A,
                                void* nn_x, void* nn_g, int64_t step, void* ws, hipStream_t s) {
  const int N = t->N;
  const int64_t Q = A.B * (N - 1);
  double* xrows = static_cast<double*>(ws);
  double* jt = xrows + Q * NNA_ROW;
  int32_t* pos = reinterpret_cast<int32_t*>(static_cast<char*>(ws) + bank_nn_bytes(N, A.B));
  if (!uploaded) {
    KR_HIP(hipMemcpyAsync(pos, o.pos.data(), sizeof(int32_t) * (size_t)A.B, hipMemcpyHostToDevice, s));
    KR_HIP(hipStreamSynchronize(s));
    uploaded = true;
  }
  const AdjBank TB{(const KR_CONSTANT_AS RodConst<double>*)t->rows_d, (const KR_CONSTANT_AS int32_t*)pos, N};
  hipLaunchKernelGGL((nn_rows_bank_kernel<T>), dim3((unsigned)((Q + 255) / 256)), dim3(256), 0, s, TB, A, xrows);
  KR_HIP(hipGetLastError());
  for (int k = 0; k < bank->K; ++k) {
    if (!o.count[k]) continue;
    const int64_t r0 = o.first[k] * (N - 1);
    if (int rc = launch_nnjac<double>(bank_net(bank, k), o.count[k] * (N - 1), xrows + r0 * NNA_ROW, NNA_ROW, jt + r0 * NNA_JAC, 1, s))
      return rc;
  }
  const AdjNn<T> NN{xrows, jt, nn_x ? static_cast<T*>(nn_x) + step * Q * NNA_ROW : nullptr,
                    nn_g ? static_cast<T*>(nn_g) + step * Q * NNA_ROW : nullptr};
  const int64_t grid = (A.B + ADJ_RODS_PER_WG - 1) / ADJ_RODS_PER_WG;
  hipLaunchKernelGGL((step_vjp_bank_kernel<T>), dim3((unsigned)grid), dim3(64 * ADJ_RODS_PER_WG), 0, s, TB, A, NN);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

// The refusals of the bank form, after the handle, the table, the bank, the dtype and the state pointers: the index array,
// the table's (adj_tab_refuse: device, N, del_t, then the scheme - which is moved behind the network's checks here by asking
// it for the Euler scheme first), the bank's device, the indices, then what is not served.
static int adj_bank_refuse(const char* api, const kr_handle* h, const kr_param_table* t, const kr_mlp_bank* bank, const int32_t* net_of_rod,
                           int scheme) {
  const std::string who = std::string(api) + ": ";
  if (!net_of_rod) {
    set_error(who + "null pointer argument: net_of_rod_host");
    return KR_E_ARG;
  }
  if (int rc = adj_tab_refuse(api, h, t, KR_EULER)) return rc;
  if (bank->device != h->device) {
    set_error(who + "network bank: device of the bank differs from the handle's");
    return KR_E_ARG;
  }
  for (int64_t b = 0; b < t->B; ++b)
    if (net_of_rod[b] < 0 || net_of_rod[b] >= bank->K) {
      set_error(who + "network bank: rod " + std::to_string(b) + " asks for network " + std::to_string(net_of_rod[b]) + ", the bank holds " +
                std::to_string(bank->K));
      return KR_E_ARG;
    }
  if (int rc = adj_refuse(api, scheme, 0)) return rc;
  return nnjac_check(bank->md, t->nn_input_history, api);
}

}  // namespace kr

using namespace kr;

extern "C" int kr_step_vjp_bank_batch(kr_handle* h, const kr_param_table* t, const kr_mlp_bank* bank, const int32_t* net_of_rod_host,
                                      int scheme, const void* state_prev, const void* state_cur, const void* state_next,
                                      const void* tensions, const void* g_next, void* g_cur, void* g_prev, void* g_tensions, void* g_bnd,
                                      double* resid, int32_t* status, void* nn_x, void* nn_g, int dtype, void* stream) {
  const char* api = "kr_step_vjp_bank_batch";
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(!t, std::string(api) + ": null parameter table");
  KR_ADJ_ARG(!bank, std::string(api) + ": null network bank");
  BankOrder o;
  bool uploaded = false;
  return adj_step_entry(api, h, t->B, state_prev, state_cur, state_next, tensions, g_next, g_cur, g_prev, g_tensions, g_bnd, resid,
                        status, dtype, stream, [=](const char* a) { return adj_bank_refuse(a, h, t, bank, net_of_rod_host, scheme); },
                        [=, &o, &uploaded](kr_handle* hh, const auto& A, hipStream_t s) {
                          if (int rc = ensure_ws(hh, bank_ws_bytes(t->N, A.B))) return rc;
                          o = bank_order(net_of_rod_host, A.B, bank->K);
                          return launch_step_vjp_bank(t, bank, o, uploaded, A, nn_x, nn_g, 0, hh->ws, s);
                        });
}

extern "C" int kr_simulate_vjp_bank_batch(kr_handle* h, const kr_param_table* t, const kr_mlp_bank* bank, const int32_t* net_of_rod_host,
                                          int64_t T, int scheme, const void* ctl, const void* states, const void* state_prev_init,
                                          void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd, int bnd_per_step, double* resid,
                                          int32_t* status, void* nn_x, void* nn_g, int dtype, void* stream) {
  const char* api = "kr_simulate_vjp_bank_batch";
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(!t, std::string(api) + ": null parameter table");
  KR_ADJ_ARG(!bank, std::string(api) + ": null network bank");
  KR_ADJ_ARG(bnd_per_step != 0 && bnd_per_step != 1, std::string(api) + ": bnd_per_step must be 0 or 1");
  BankOrder o;
  bool uploaded = false;
  return adj_simulate_entry(api, h, t->B, T, ctl, states, state_prev_init, g_states, g_prev_init, g_ctl, g_bnd, nullptr, resid, status,
                            dtype, stream, [=](const char* a) { return adj_bank_refuse(a, h, t, bank, net_of_rod_host, scheme); },
                            bank_ws_bytes(t->N, t->B),
                            [=, &o, &uploaded](kr_handle*, const auto& A, void* ws, int64_t step, hipStream_t s) {
                              if (!uploaded) o = bank_order(net_of_rod_host, A.B, bank->K);
                              return launch_step_vjp_bank(t, bank, o, uploaded, A, nn_x, nn_g, step, ws, s);
                            },
                            bnd_per_step != 0);
}
