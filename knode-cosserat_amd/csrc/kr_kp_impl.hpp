// kr_kp_impl.hpp - key-point records: the one-wavefront persistent kernels fed from a per-rod parameter table and a
// boundary history (kr_bnd_impl.hpp) that also write kp[T][B][K][KR_SLOTS], the complete record of K chosen grid points
// of the state every step writes.
//
// A simulate call returns either the full history, states[T + 1][B][N][KR_SLOTS], or - on a 3-slot ring - the tips, and
// an interior step of a ring call stores nothing but the twelve leading slots of each record: p and h of an interior
// grid point never leave the registers.  Everything computed from a trajectory (the device metrics of kr_score.hip, the
// reference's key points and markers, a tip orientation) needs the states at a few grid points for every step.  The
// verifying lanes of mso_sim_kernel and the storing lanes of ms_sim_kernel hold the complete record of every grid point
// they pass; kr_simulate_batch_keypoints stores it a second time where the grid point is marked.
//
// mso_sim_kernel (kr_mso_impl.hpp) and ms_sim_kernel (kr_ms_impl.hpp) are instantiated here with
// PSRC = RodTableBndKp<T> (rod_device.hpp): the boundary source plus the kp pointer, K and the point set, which
// therefore are kernel arguments of these instantiations alone.  rod_src_step_slots of the new source is the boundary
// one, so everything kr_bnd_impl.hpp says about the base and the wrench holds here.
//   * The point set is a 128-bit mask in four scalar registers (N <= 128); the rank of a marked point - its index in kp -
//     is the population count of the mask below it, which is why the host wants idx strictly increasing.  Testing a grid
//     point reads no memory (store_keypoint, kr_sim_impl.hpp).
//   * A record goes to kp at every site that has it in registers to stream it into the state: mso_sim_kernel in the
//     verifying lanes' block of every trip (complete, lean and predicated) and in the verdict's block beside the tip for
//     the last grid point; ms_sim_kernel in the storing sweeps with the MLP off and on, at the last grid point and in the
//     damped fallback, as the first launch and as the take-over launch from resume[rod] on.
//   * A sweep that is later rejected has written its key points and the sweep that replaces it overwrites them: the
//     tip's rule.  Ring and full-history calls run the same stores, so they give the same kp.
// tools/kp_asm_compare.py puts every loop of a key-point kernel next to its boundary twin.
//
// Served: what kr_simulate_batch_boundary serves (plan_simulate, kr_plan.hip).  Everything else is refused.
#pragma once
#include "kr_tab_impl.hpp"

namespace kr {

// launch_bnd_sim with the key-point records
template <typename T>
int launch_kp_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  static_assert(rod_src_step_slots<T, RodTableBndKp<T>>::count == KR_BND, "knode_rod.h: KR_BND values per rod and step");
  static_assert(KR_SLOTS == 28, "rod_src_keypoints: the records of kp are KR_SLOTS wide");
  auto tab = table_src<T, RodTableBndKp<T>>(src.table);
  tab.bnd = static_cast<const T*>(src.hist);
  tab.kp = static_cast<T*>(src.kp.kp);
  tab.K = src.kp.K;
  tab.mask_lo = src.kp.mask_lo;
  tab.mask_hi = src.kp.mask_hi;
  return launch_one_wave_src<T>(h, tab, p, a, at);
}

}  // namespace kr
