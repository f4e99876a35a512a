// kr_load_impl.hpp - per-step tip loads: the one-wavefront persistent kernels fed from a per-rod parameter table AND a
// wrench history loads[B][T][6].
//
// The reference keeps the tip wrench as two plain attributes (cosserat_ode.py:28-29) that the residual reads at every
// solve (:206-207), so a caller who assigns robot.F_tip / robot.M_tip between two steps of knode.simulate's loop - a
// payload picked up, a push against the tip - gets the trajectory under that history.  Every other simulate call here
// freezes the wrench for the whole call; kr_simulate_batch_loads gives rod b, while it solves step t, loads[b][t].
//
// mso_sim_kernel (kr_mso_impl.hpp) and ms_sim_kernel (kr_ms_impl.hpp) are instantiated here with
// PSRC = RodTableLoads<T>: the table of kr_tab_impl.hpp plus the pointer, which therefore is a kernel argument of these
// instantiations alone (SimArgs and every other kernel's argument offsets stay as they are).  The kernels read the
// wrench from the LDS cold block only; the loads forms rewrite its six slots once per step, outside the sweeps:
//   * ms_sim_kernel runs its steps in sequence: six lanes store loads[t] before the first sweep of step t and request
//     loads[t + 1], as the tensions are requested one step ahead.  As the take-over launch it starts at the rod's
//     resume step and loads that step's wrench.
//   * mso_sim_kernel holds two time levels in a merged sweep, so it keeps two sets of slots, step t's in set t & 1, and
//     every read names its step (see the comment at the kernel).
// tools/loads_asm_compare.py puts every loop of a loads kernel next to its table twin.
//
// Served: what kr_simulate_batch_table serves (plan_simulate, kr_plan.hip).  Everything else is refused.
#pragma once
#include "kr_tab_impl.hpp"

namespace kr {

// launch_tab_sim with the wrench history
template <typename T>
int launch_load_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  auto tab = table_src<T, RodTableLoads<T>>(src.table);
  tab.loads = static_cast<const T*>(src.hist);
  return launch_one_wave_src<T>(h, tab, p, a, at);
}

}  // namespace kr
