// kr_adj_tab.hip - the step adjoint of a heterogeneous batch (MLP off): rod b takes row b of a parameter table.
//
//   kr_step_vjp_table_batch      kr_step_vjp_par_batch with row b's parameters in place of the handle's, per rod
//   kr_simulate_vjp_table_batch  the same composed over the T steps of a stored trajectory; the boundary gradient summed
//                                over the steps or kept per step ([b][t]: the gradient with respect to bnd[b][t] of
//                                kr_simulate_batch_boundary, its last six columns with respect to loads[b][t])
//
// The kernels are kr_adj_body.inc once more, without and with PAR.  The body reads two names, P and Q; here they are bound
// per rod instead of per launch: P is the rod's row IN PLACE, a reference into the table through the constant address space
// (the rod index is wavefront-uniform, so every read of a constant is a scalar load of a uniform address), Q the nine doubles
// E, r, rho, vstar, g of the table's `par` array, which kr_derive consumed and the rows therefore do not hold.  The wavefront
// leaves before it binds either if its rod is beyond B: no row beyond the table's last is ever addressed.
// Why in place: the handle kernels do not hold their ~90 constants in registers either - they re-read the kernel-argument
// segment with scalar loads where the point map needs them - so the table form is the same instruction stream with another
// base address (LABBOOK, "Step adjoint for heterogeneous batches", has the ISA counts of this against a copy in SGPRs, which
// lands in scratch, and a copy in LDS, which costs 160 VGPRs).
// As in kr_adj_par.hip every output but g_par comes from the kernel without PAR, launched first, and the PAR kernel then runs
// with those pointers null: g_par or not, the other outputs are the same bits.
// The rollout is simulate_vjp_steps (kr_adj_impl.hpp) with this unit's launch; per-step boundary gradients are the step's g_bnd
// copied to [b][t] by adj_put_kernel instead of added.
#include "kr_adj_impl.hpp"

namespace kr {

constexpr int ADJ_TAB_PAR = 9;  // doubles per row of kr_param_table::par: E, r, rho, vstar[3], g[3]

// What a table kernel takes in place of the by-value RodConst<double> (and AdjPar<T>).  Like RodTable's, the pointers carry
// the constant address space from the kernel argument on.
template <typename T>
struct AdjTab {
  const KR_CONSTANT_AS RodConst<double>* rows;  // [B]
  const KR_CONSTANT_AS double* par;             // [B][ADJ_TAB_PAR]; read by the PAR kernel only
  T* g_par;                                     // [B][KR_PAR]; written by the PAR kernel only
};

// (adj_tab_rod, adj_tab_row - this wavefront's rod and its row in place: kr_adj_impl.hpp, shared with kr_adj_bank.hip)

template <typename T>
__global__ __launch_bounds__(64 * ADJ_RODS_PER_WG) void step_vjp_tab_kernel(const AdjTab<T> TB, const AdjArgs<T> A) {
  constexpr bool PAR = false, NNON = false;
  if (adj_tab_rod() >= A.B) return;
  const RodConst<double>& P = adj_tab_row(TB.rows, adj_tab_rod());
  const AdjPar<T> Q{};
  const AdjNn<T> NN{};
#include "kr_adj_body.inc"
}

// (one wavefront per SIMD, as step_vjp_par_kernel)
template <typename T>
__global__ __launch_bounds__(64 * ADJ_RODS_PER_WG) __attribute__((amdgpu_waves_per_eu(1, 1))) void step_vjp_tab_par_kernel(const AdjTab<T> TB, const AdjArgs<T> A) {
  constexpr bool PAR = true, NNON = false;
  if (adj_tab_rod() >= A.B) return;
  const RodConst<double>& P = adj_tab_row(TB.rows, adj_tab_rod());
  AdjPar<T> Q;
  {
    const KR_CONSTANT_AS double* q = TB.par + (int64_t)__builtin_amdgcn_readfirstlane((int)adj_tab_rod()) * ADJ_TAB_PAR;
    Q.g_par = TB.g_par;
    Q.E = q[0]; Q.r = q[1]; Q.rho = q[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Q.vstar[i] = q[3 + i];
      Q.g[i] = q[6 + i];
    }
  }
  const AdjNn<T> NN{};
#include "kr_adj_body.inc"
}

template <typename T>
static int launch_step_vjp_tab(const kr_param_table* t, const AdjArgs<T>& A, void* g_par, hipStream_t s) {
  AdjTab<T> TB{};
  TB.rows = (const KR_CONSTANT_AS RodConst<double>*)t->rows_d;
  TB.par = (const KR_CONSTANT_AS double*)t->par;
  const int64_t grid = (A.B + ADJ_RODS_PER_WG - 1) / ADJ_RODS_PER_WG;
  hipLaunchKernelGGL((step_vjp_tab_kernel<T>), dim3((unsigned)grid), dim3(64 * ADJ_RODS_PER_WG), 0, s, TB, A);
  KR_HIP(hipGetLastError());
  if (!g_par) return KR_OK;
  AdjArgs<T> Ap = A;  // (reads only; g_par is all this launch writes)
  Ap.g_cur = Ap.g_prev = Ap.g_tens = Ap.g_bnd = nullptr;
  Ap.resid = nullptr;
  Ap.status = nullptr;
  TB.g_par = static_cast<T*>(g_par);
  hipLaunchKernelGGL((step_vjp_tab_par_kernel<T>), dim3((unsigned)grid), dim3(64 * ADJ_RODS_PER_WG), 0, s, TB, Ap);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

// dst[b][k] = src[b][k], k < KR_BND, the rows of dst `stride` elements apart (a per-step rollout: dst = g_bnd + t KR_BND, stride =
// T KR_BND).  A kernel of its own, so that AdjArgs and the step kernels stay what they are.
template <typename T>
__global__ __launch_bounds__(256) void adj_put_kernel(T* dst, const T* src, int64_t n, int64_t stride) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i / KR_BND * stride + i % KR_BND] = src[i];
}
template <typename T>
static int launch_put_t(T* dst, const T* src, int64_t n, int64_t stride, hipStream_t s) {
  hipLaunchKernelGGL((adj_put_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, src, n, stride);
  KR_HIP(hipGetLastError());
  return KR_OK;
}
int launch_put(float* dst, const float* src, int64_t n, int64_t stride, hipStream_t s) { return launch_put_t(dst, src, n, stride, s); }
int launch_put(double* dst, const double* src, int64_t n, int64_t stride, hipStream_t s) { return launch_put_t(dst, src, n, stride, s); }

// The refusals of the table form: the table against the handle, then the scheme.  (No use_nn: the calls differentiate the
// physics alone and do not read the handle's network, so nn_input_history is not compared.)
int adj_tab_refuse(const char* api, const kr_handle* h, const kr_param_table* t, int scheme) {
  const char* f = t->device != h->device ? "device" : t->N != h->params.N ? "N" : t->del_t != h->params.del_t ? "del_t" : nullptr;
  if (f) {
    set_error(std::string(api) + ": parameter table: " + f + " of the table differs from the handle's");
    return KR_E_ARG;
  }
  return adj_refuse(api, scheme, 0);
}

}  // namespace kr

using namespace kr;

extern "C" int kr_step_vjp_table_batch(kr_handle* h, const kr_param_table* t, int scheme, const void* state_prev, const void* state_cur,
                                       const void* state_next, const void* tensions, const void* g_next, void* g_cur, void* g_prev,
                                       void* g_tensions, void* g_bnd, void* g_par, double* resid, int32_t* status, int dtype,
                                       void* stream) {
  const char* api = "kr_step_vjp_table_batch";
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(!t, std::string(api) + ": null parameter table");
  return adj_step_entry(api, h, t->B, state_prev, state_cur, state_next, tensions, g_next, g_cur, g_prev, g_tensions, g_bnd, resid,
                        status, dtype, stream, [=](const char* a) { return adj_tab_refuse(a, h, t, scheme); },
                        [=](kr_handle*, const auto& A, hipStream_t s) { return launch_step_vjp_tab(t, A, g_par, s); });
}

extern "C" int kr_simulate_vjp_table_batch(kr_handle* h, const kr_param_table* t, int64_t T, int scheme, const void* ctl,
                                           const void* states, const void* state_prev_init, void* g_states, void* g_prev_init,
                                           void* g_ctl, void* g_bnd, int bnd_per_step, void* g_par, double* resid, int32_t* status,
                                           int dtype, void* stream) {
  const char* api = "kr_simulate_vjp_table_batch";
  KR_ADJ_ARG(!h, "null handle");
  KR_ADJ_ARG(!t, std::string(api) + ": null parameter table");
  KR_ADJ_ARG(bnd_per_step != 0 && bnd_per_step != 1, std::string(api) + ": bnd_per_step must be 0 or 1");
  const size_t tail = g_par ? (size_t)t->B * KR_PAR * (dtype == KR_F32 ? sizeof(float) : sizeof(double)) : 0;
  return adj_simulate_entry(api, h, t->B, T, ctl, states, state_prev_init, g_states, g_prev_init, g_ctl, g_bnd, g_par, resid, status,
                            dtype, stream, [=](const char* a) { return adj_tab_refuse(a, h, t, scheme); }, tail,
                            [=](kr_handle*, const auto& A, void* w_par, int64_t, hipStream_t s) { return launch_step_vjp_tab(t, A, w_par, s); },
                            bnd_per_step != 0);
}
