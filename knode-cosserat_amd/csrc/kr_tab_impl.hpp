// kr_tab_impl.hpp - heterogeneous batches: the one-wavefront persistent kernels fed from a per-rod parameter table.
//
// Every batched entry point takes its rod from the handle: one RodConst<T> by value in the kernel-argument segment, the
// same for all B rods.  kr_simulate_batch_table gives rod b row b of a table in global memory instead - the reference's
// "one true rod, eight mismatched models" (knode.py:6-53, physics_multitrain.py) in one launch rather than eight.
//
// The multiple-shooting kernels own one rod per wavefront, so a rod's constants stay wave-uniform; only their origin
// changes.  mso_sim_kernel (kr_mso_impl.hpp) and ms_sim_kernel (kr_ms_impl.hpp) are instantiated here with
// PSRC = RodTable<T>: the wavefront copies its row into SGPRs once, unconditionally, in the prologue, through the
// constant address space (rod_src_row, rod_device.hpp) - scalar loads from memory the compiler knows to be invariant,
// which is what the loads of the by-value kernel argument are too.  The cold part of the row goes through the LDS
// `cold` block as before (ms_cold_fill reads the row in memory).  tools/tab_asm_compare.py puts every loop of a table
// kernel next to its plain twin: the same fp64 instruction counts, no scalar memory instruction inside a loop, no
// scratch where the plain kernel has none.
//
// Served: Euler sweeps, diagonal material matrices on every row, 8 <= N - 1, N <= 128, one wavefront per rod;
// MLP off (overlapped kernel + take-over launch, or the plain persistent kernel for overlap = 0) or an MLP the
// persistent one-wavefront kernel serves (one network, the handle's, for all rods).  Everything else is refused.
#pragma once
#include "kr_mso_impl.hpp"

namespace kr {

// np.linspace(0, L_b, N) along z, h = (1, 0, 0, 0), v = (0, 0, 1): init_straight_kernel with the length of rod b
template <typename T>
__global__ void init_straight_tab_kernel(int N, const double* __restrict__ Ls, int64_t B, T* __restrict__ state) {
  const int64_t pts = B * (int64_t)N;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pts; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % N);
    const double L = Ls[i / N];
    T rec[KR_SLOTS];
#pragma unroll
    for (int k = 0; k < KR_SLOTS; ++k) rec[k] = T(0);
    rec[SL_P + 2] = (T)((double)j * (L / (double)(N - 1)));
    if (j == N - 1) rec[SL_P + 2] = (T)L;
    rec[SL_H] = T(1);
    rec[SL_V + 2] = T(1);
    store_record(state + i * KR_SLOTS, rec);
  }
}

template <typename T>
int launch_tab_init_straight(kr_handle* h, const kr_param_table* t, T* state, hipStream_t s) {
  hipLaunchKernelGGL((init_straight_tab_kernel<T>), dim3(grid_for(t->B * t->N)), dim3(256), 0, s, t->N, t->L, t->B, state);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

static inline int tab_refuse(const std::string& why) {
  set_error("kr_simulate_batch_table: " + why + " (not served with a parameter table; nothing falls back to the handle's parameters)");
  return KR_E_UNSUPPORTED;
}

template <typename T>
int launch_tab_sim(kr_handle* h, const kr_param_table* t, int scheme, int use_nn, const SimArgs<T>& a, hipStream_t s) {
  constexpr int HS = hs_phys<T>();
  const int N = t->N;
  if (scheme != KR_EULER) return tab_refuse("only Euler sweeps (scheme = KR_EULER)");
  if (N - 1 < 2 * MS_P || N > MS_NPL * WAVE) return tab_refuse("N = " + std::to_string(N) + ", the one-wavefront persistent kernels serve 9 <= N <= 128");
  if (h->ms_mode == 0 || h->persistent == 0) return tab_refuse("options ms_mode = 0 / persistent = 0 select kernels without a table form");
  if (h->ms_mode != 1 && a.B > (int64_t)h->ms_batch_limit) return tab_refuse("B exceeds option ms_batch_limit");
  if (h->waves_per_rod > 1) return tab_refuse("option waves_per_rod = " + std::to_string(h->waves_per_rod) + ", table calls run one wavefront per rod");
  if (a.B > (int64_t)0x7fffffff) return tab_refuse("B >= 2^31");
  const MlpDev<T>& M = mlpdev<T>(h);
  if (use_nn) {
    if (M.n_layers <= 0) { set_error("use_nn requested but no MLP was set (kr_set_mlp)"); return KR_E_STATE; }
    if (!M.mfma_ok || !M.jvp_ok || h->params.nn_input_history) return tab_refuse("an MLP the persistent one-wavefront kernel does not evaluate");
  }
  const RodTable<T> tab{(const KR_CONSTANT_AS RodConst<T>*)table_rows<T>(t), N};
  const dim3 grid((unsigned)((a.B + MS_WPB - 1) / MS_WPB)), block(WAVE * MS_WPB);
  h->last_waves_per_rod = 1;
  h->last_overlap = 0;
  if (use_nn) {
    const size_t smem = ms_lds_bytes<T, HS>(N, true, true);
    if (smem > (size_t)h->lds_limit) return tab_refuse("the rod's history does not fit the LDS with the MLP on");
    auto kern = ms_sim_kernel<T, true, KR_EULER, HS, true, 1, RodTable<T>>;
    if (int rc = dyn_lds(reinterpret_cast<const void*>(kern), smem)) return rc;
    hipLaunchKernelGGL(kern, grid, block, smem, s, tab, a, M);
    KR_HIP(hipGetLastError());
    return KR_OK;
  }
  const size_t smem = ms_lds_bytes<T, HS>(N, true);
  if (smem > (size_t)h->lds_limit) return tab_refuse("the rod's history does not fit the LDS");
  SimArgs<T> a2 = a;
  const size_t smem_o = sizeof(T) * mso_lds_elems<T, HS>(N) * MS_WPB;
  if (h->overlap && smem_o <= (size_t)h->lds_limit) {
    // two launches, as launch_sim_persistent: the overlapped kernel, then the take-over launch for what it left behind
    if (int rc = ensure_resume(h, a.B)) return rc;
    a2.resume = static_cast<int32_t*>(h->resume_buf);
    if (int rc = mso_check_steps(a.T_steps)) return rc;
    auto ko = mso_sim_kernel<T, true, HS, 1, RodTable<T>>;
    if (int rc = dyn_lds(reinterpret_cast<const void*>(ko), smem_o)) return rc;
    hipLaunchKernelGGL(ko, grid, block, smem_o, s, tab, a2);
    KR_HIP(hipGetLastError());
    h->last_overlap = 1;
  }
  auto kern = ms_sim_kernel<T, true, KR_EULER, HS, false, 1, RodTable<T>>;
  if (int rc = dyn_lds(reinterpret_cast<const void*>(kern), smem)) return rc;
  hipLaunchKernelGGL(kern, grid, block, smem, s, tab, a2, M);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

}  // namespace kr
