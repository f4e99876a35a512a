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
// Served: what kr_simulate_batch_table serves with the MLP on (plan_simulate, kr_plan.hip).  Everything else is refused.
#pragma once
#include "kr_tab_impl.hpp"

namespace kr {

// (the MLP-on arm of launch_one_wave_src with the bank for a network: its own launch, so that this unit holds that one
// kernel and not the MLP-off table kernels of kr_tab_*)
template <typename T>
int launch_bank_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  const auto tab = table_src<T, RodTable<T>>(src.table);
  const MlpBank<T> bank{bank_net0<T>(src.bank), (const KR_CONSTANT_AS int32_t*)src.net_idx, (unsigned long long)src.bank->stride};
  return launch(at, ms_sim_kernel<T, true, KR_EULER, hs_phys<T>(), true, 1, RodTable<T>, MlpBank<T>>, dim3((unsigned)((a.B + MS_WPB - 1) / MS_WPB)),
                dim3(WAVE * MS_WPB), p.smem[0], tab, a, bank);
}

}  // namespace kr
