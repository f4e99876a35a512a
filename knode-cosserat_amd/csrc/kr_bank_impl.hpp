// kr_bank_impl.hpp - per-rod networks: the MLP-on persistent one-wavefront kernel fed from a parameter table AND a
// bank of K packed networks.
//
// The reference's model-mismatch experiment loads, for every model variant, that variant's OWN trained network before
// it simulates (physics_multitrain.py:181-199: setup_robot(robot, mod), then nn_path = saved_models/..._{mod}_..._{seed}.pth),
// and repeats that for every seed.  With one network per handle that is one kr_set_mlp and one launch per (mod, seed);
// kr_simulate_batch_bank runs rod b with row b of the table and network net_of_rod[b] of the bank in ONE launch.
//
// ms_sim_kernel (kr_ms_impl.hpp) owns one rod per wavefront and fetches its weight fragments through the pointers of
// MlpDev<T>; nothing is staged per workgroup.  A rod's network therefore is a wave-uniform base address, as a rod's
// constants are a wave-uniform table row: the kernel is instantiated here with PSRC = RodTable<T>, MSRC = MlpBank<T>,
// reads its index once in the prologue (a scalar load through the constant address space) and moves the bank's base
// pointers by index * stride (mlp_src_net).  Every sweep variant - low-precision first sweep, base-only storing
// sweeps, the fp32 and fp64 three-layer chains, the two-layer chain, the damped single-shooting fallback - takes that
// descriptor where it took the kernel argument.  tools/bank_asm_compare.py puts the loops of each bank kernel next to
// those of its one-network table twin (kr_tab_*).
//
// Served: what kr_simulate_batch_table serves with the MLP on.  Everything else is refused.
#pragma once
#include "kr_tab_impl.hpp"

namespace kr {

static inline int bank_refuse(const std::string& why) {
  set_error("kr_simulate_batch_bank: " + why + " (not served with a network bank; nothing falls back to the handle's MLP)");
  return KR_E_UNSUPPORTED;
}

template <typename T>
int launch_bank_sim(kr_handle* h, const kr_param_table* t, const kr_mlp_bank* bk, const int32_t* net_idx, int scheme,
                    const SimArgs<T>& a, hipStream_t s) {
  constexpr int HS = hs_phys<T>();
  const int N = t->N;
  if (scheme != KR_EULER) return bank_refuse("only Euler sweeps (scheme = KR_EULER)");
  if (N - 1 < 2 * MS_P || N > MS_NPL * WAVE) return bank_refuse("N = " + std::to_string(N) + ", the one-wavefront persistent kernel serves 9 <= N <= 128");
  if (h->ms_mode == 0 || h->persistent == 0) return bank_refuse("options ms_mode = 0 / persistent = 0 select kernels without a bank form");
  if (h->ms_mode != 1 && a.B > (int64_t)h->ms_batch_limit) return bank_refuse("B exceeds option ms_batch_limit");
  if (h->waves_per_rod > 1) return bank_refuse("option waves_per_rod = " + std::to_string(h->waves_per_rod) + ", bank calls run one wavefront per rod");
  if (a.B > (int64_t)0x7fffffff) return bank_refuse("B >= 2^31");
  const MlpDev<T>& M0 = bank_net0<T>(bk);
  if (!M0.mfma_ok || !M0.jvp_ok || h->params.nn_input_history || !h->mfma_mlp)
    return bank_refuse("a network shape the persistent one-wavefront kernel does not evaluate");
  const size_t smem = ms_lds_bytes<T, HS>(N, true, true);
  if (smem > (size_t)h->lds_limit) return bank_refuse("the rod's history does not fit the LDS with the MLP on");
  const RodTable<T> tab{(const KR_CONSTANT_AS RodConst<T>*)table_rows<T>(t), N};
  const MlpBank<T> bank{M0, (const KR_CONSTANT_AS int32_t*)net_idx, (unsigned long long)bk->stride};
  const dim3 grid((unsigned)((a.B + MS_WPB - 1) / MS_WPB)), block(WAVE * MS_WPB);
  auto kern = ms_sim_kernel<T, true, KR_EULER, HS, true, 1, RodTable<T>, MlpBank<T>>;
  if (int rc = dyn_lds(reinterpret_cast<const void*>(kern), smem)) return rc;
  hipLaunchKernelGGL(kern, grid, block, smem, s, tab, a, bank);
  KR_HIP(hipGetLastError());
  h->last_waves_per_rod = 1;
  h->last_overlap = 0;
  return KR_OK;
}

}  // namespace kr
