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
// Served: one wavefront per rod, MLP off (overlapped kernel + take-over launch, or the plain persistent kernel) or the
// handle's network for all rods; plan_simulate (kr_plan.hip) holds the rules and refuses everything else.
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
  return launch(s, init_straight_tab_kernel<T>, dim3(grid_for(t->B * t->N)), dim3(256), 0, t->N, t->L, t->B, state);
}

// A plan of plan_table carried out on the kernels of one parameter source PSRC (RodTable<T> or a struct derived from it):
// the MLP-on persistent kernel; or - KR_FAM_MSO - two launches, as with the handle's constants: the overlapped kernel, then
// the take-over launch for what it left behind (a.resume); or - KR_FAM_MS_SIM - the one-wavefront persistent kernel alone.
// The unit that calls it holds these three instantiations.
template <typename T, typename PSRC>
int launch_one_wave_src(kr_handle* h, const PSRC& tab, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  constexpr int HS = hs_phys<T>();
  const dim3 grid((unsigned)((a.B + MS_WPB - 1) / MS_WPB)), block(WAVE * MS_WPB);
  if (p.nn) return launch(at, ms_sim_kernel<T, true, KR_EULER, HS, true, 1, PSRC>, grid, block, p.smem[0], tab, a, mlpdev<T>(h));
  if (p.family == KR_FAM_MSO)
    if (int rc = launch_mso_inst<T, 1>(tab, p, a, at)) return rc;
  return launch(at, ms_sim_kernel<T, true, KR_EULER, HS, false, 1, PSRC>, grid, block, p.smem[p.family == KR_FAM_MSO ? 1 : 0], tab, a,
                mlpdev<T>(h));
}

// the table part of every source struct
template <typename T, typename PSRC>
PSRC table_src(const kr_param_table* t) {
  PSRC tab{};
  tab.rows = (const KR_CONSTANT_AS RodConst<T>*)table_rows<T>(t);
  tab.N = t->N;
  return tab;
}

template <typename T>
int launch_tab_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at) {
  return launch_one_wave_src<T>(h, table_src<T, RodTable<T>>(src.table), p, a, at);
}

}  // namespace kr
