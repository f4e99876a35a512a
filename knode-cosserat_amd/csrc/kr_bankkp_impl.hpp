// kr_bankkp_impl.hpp - per-rod networks with per-step boundary data and key-point records: the MLP-on persistent
// one-wavefront kernel fed from a parameter table, a boundary history, a key-point destination AND a bank of K packed
// networks.
//
// The evaluation half of the reference's experiment rolls every trained network out and scores it at key points against
// a recorded run (physics_multitrain.py:180-233), and does the same during training to pick the best weights
// (physics_train.py:136-167).  kr_simulate_batch_bank runs rod b with network net_of_rod[b] but from a frozen boundary
// and with nothing but the full history or the tips to score from; kr_simulate_batch_keypoints has the moving base, the
// wrench history and the records of K grid points, but one network for all rods.
// kr_simulate_batch_bank_keypoints is both at once.
//
// In ms_sim_kernel (kr_ms_impl.hpp) the rod's source PSRC and the network's source MSRC are independent template
// parameters: the cold-slot and key-point traits (rod_src_step_slots, rod_src_keypoints, rod_device.hpp) are keyed on
// PSRC alone, mlp_src_net on MSRC alone.  The kernel is instantiated here with PSRC = RodTableBndKp<T>,
// MSRC = MlpBank<T>; everything kr_kp_impl.hpp says about the records and kr_bank_impl.hpp says about the network's
// base address holds.  K = 0 is served: the mask is empty, store_keypoint (kr_sim_impl.hpp) stores nothing and the kp
// pointer is never dereferenced - the bank form of the boundary call.
// tools/bank_kp_asm_compare.py puts the loops of each kernel next to those of its bank twin (kr_bank_*) and its MLP-on
// key-point twin (kr_kp_*).
//
// Served: what kr_simulate_batch_bank serves (plan_simulate, kr_plan.hip).  Everything else is refused.
#pragma once
#include "kr_tab_impl.hpp"

namespace kr {

// launch_bank_sim with the source struct of launch_kp_sim
template <typename T>
int launch_bankkp_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  static_assert(rod_src_step_slots<T, RodTableBndKp<T>>::count == KR_BND, "knode_rod.h: KR_BND values per rod and step");
  static_assert(KR_SLOTS == 28, "rod_src_keypoints: the records of kp are KR_SLOTS wide");
  auto tab = table_src<T, RodTableBndKp<T>>(src.table);
  tab.bnd = static_cast<const T*>(src.hist);
  tab.kp = static_cast<T*>(src.kp.kp);
  tab.K = src.kp.K;
  tab.mask_lo = src.kp.mask_lo;
  tab.mask_hi = src.kp.mask_hi;
  const MlpBank<T> bank{bank_net0<T>(src.bank), (const KR_CONSTANT_AS int32_t*)src.net_idx, (unsigned long long)src.bank->stride};
  return launch(at, ms_sim_kernel<T, true, KR_EULER, hs_phys<T>(), true, 1, RodTableBndKp<T>, MlpBank<T>>, dim3((unsigned)((a.B + MS_WPB - 1) / MS_WPB)),
                dim3(WAVE * MS_WPB), p.smem[0], tab, a, bank);
}

}  // namespace kr
