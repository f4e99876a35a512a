// kr_mswn_impl.hpp - several wavefronts per rod WITH the residual MLP inside the sweeps: host side of the NN
// instantiations of msw_sim_kernel (kr_msw_impl.hpp).  Own translation units (kr_mswn_f32.hip / kr_mswn_f64.hip) so
// that the largest kernels of the library compile in parallel with the others.
//
// Why: with the MLP on, one grid point costs ~20 k cycles of network evaluation (mlp_jvp.hpp) in a dependent chain
// exchange -> base chain -> act' -> JVP layers -> exchange, 43 % of which a lone wavefront spends waiting, and a
// sweep is 25 such points at four sub-intervals per wavefront.  Two wavefronts per rod cut the chain to 14 points
// (seven sub-intervals) and put two wavefronts on every SIMD at B = 1024, whose waits overlap; the distributed
// condensation between them costs a few thousand cycles per iteration, which is nothing here.  The records of the
// BDF2 history move from LDS to global memory for that (see msw_sim_kernel), so that four rods fit a CU.
#pragma once
#include "kr_ms_impl.hpp"

namespace kr {

// (when this form is chosen: plan_simulate, kr_plan.hip; the history workspace is in a.hist_ws)
template <typename T>
int launch_msw_nn_sim(kr_handle* h, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  return p.W == 2 ? launch_msw_sim_inst<T, true, 2, true>(h, p, a, at) : launch_msw_sim_inst<T, true, 4, true>(h, p, a, at);
}

// MLP off, long rods (HM = 1: history records in LDS, the two newest states read from A.states): the form for rods whose
// leading slots of two states do not fit the LDS next to everything else (N = 400: 77 KB on top of 38 KB of records and
// 19 KB per wavefront)
template <typename T>
int launch_msw_gh_sim(kr_handle* h, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  if (p.W == 2)
    return p.diag ? launch_msw_sim_inst<T, true, 2, false, 1, 1>(h, p, a, at) : launch_msw_sim_inst<T, false, 2, false, 1, 1>(h, p, a, at);
  return p.diag ? launch_msw_sim_inst<T, true, 4, false, 1, 1>(h, p, a, at) : launch_msw_sim_inst<T, false, 4, false, 1, 1>(h, p, a, at);
}

}  // namespace kr
