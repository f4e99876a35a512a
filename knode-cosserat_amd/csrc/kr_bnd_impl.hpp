// kr_bnd_impl.hpp - per-step boundary data: the one-wavefront persistent kernels fed from a per-rod parameter table AND a
// boundary history bnd[B][T][KR_BND] = p0 (3), h0 (4), q0 (3), w0 (3), F_tip (3), M_tip (3).
//
// The reference keeps the base state as four plain attributes (cosserat_ode.py:44-47) that the residual reads at every
// solve (:194), exactly as it reads F_tip / M_tip: a caller whose rod sits on a moving platform, a carriage or the wrist
// of an arm assigns robot.p0 / h0 / q0 / w0 between two steps of knode.simulate's loop.  Every other simulate call here
// freezes the base for the whole call; kr_simulate_batch_boundary gives rod b, while it solves step t, bnd[b][t] - the
// base and the wrench in one array, in the order of the LDS cold block's first 19 slots, so the kernels have one
// pointer and one layout and no branch on "is there a wrench".
//
// mso_sim_kernel (kr_mso_impl.hpp) and ms_sim_kernel (kr_ms_impl.hpp) are instantiated here with
// PSRC = RodTableBnd<T>: the table of kr_tab_impl.hpp plus the pointer, which therefore is a kernel argument of these
// instantiations alone.  rod_src_step_slots (rod_device.hpp) names the cold slots a step rewrites - [CD_FTIP, + 6) for
// the loads kernels, [0, 19) here - and the code that does it is the loads kernels':
//   * ms_sim_kernel: 19 lanes store bnd[t] before ms_pred_guess of step t (which copies the base slots into row 0 of the
//     unknowns) and request bnd[t + 1]; as the take-over launch it starts at the rod's resume step with that step's values.
//     The retry from the warm start and the damped fallback read the cold block, i.e. the current step's values.
//   * mso_sim_kernel keeps two sets, step t's in set t & 1; every ms_pred_guess and every read of the wrench names its step.
// No sweep reads the base slots from the cold block: the base enters through row 0 of the unknowns alone.
// A base value that is not finite: ms_sim_kernel tests the 13 values where it stores them and reports KR_ST_NONFINITE
// from that step on (a NaN p0 reaches no equation - the damped fallback would report the step solved over NaN positions);
// mso_sim_kernel hands such a rod over at that step.
// tools/bnd_asm_compare.py puts every loop of a boundary kernel next to its loads twin.
//
// Served: what kr_simulate_batch_loads serves (plan_simulate, kr_plan.hip).  Everything else is refused.
#pragma once
#include "kr_tab_impl.hpp"

namespace kr {

// launch_load_sim with the boundary history
template <typename T>
int launch_bnd_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  static_assert(rod_src_step_slots<T, RodTableBnd<T>>::count == KR_BND, "knode_rod.h: KR_BND values per rod and step");
  auto tab = table_src<T, RodTableBnd<T>>(src.table);
  tab.bnd = static_cast<const T*>(src.hist);
  return launch_one_wave_src<T>(h, tab, p, a, at);
}

}  // namespace kr
