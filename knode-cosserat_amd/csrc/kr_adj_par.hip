// kr_adj_par.hip - the step adjoint with the gradient of the rod's material parameters (MLP off).
//
//   kr_step_vjp_par_batch      kr_step_vjp_batch plus g_par[B][KR_PAR]: d(loss) / d(E, r, rho, L, vstar, g, Bse, Bbt, C, tendon_dirs)
//   kr_simulate_vjp_par_batch  the same composed over the T steps of a stored trajectory, g_par summed over the steps
//
// A parameter theta enters a solved step through the point map alone (no parameter is in the base state or in the tip
// condition, so the 6 x 6 solve and nu are those of kr_adj.hip) and, for L, through ds = L / (N - 1):
//
//   g_par[k] = sum_j [ds lambda_{j+1}; g_z[j]] . d(y_s, z)_j / d theta_k  +  (d ds / d theta_k) sum_j lambda_{j+1} . y_s,j
//
// with lambda the total adjoint that pass 2 carries.  The kernel is kr_adj_body.inc with PAR on: passes 1 and
// 2 of kr_adj.hip, statement for statement, and in pass 2 a SECOND evaluation of the point map per grid point on dual numbers
// whose constants carry the tangent (point_map_dual on RodConstDual): lane 34 + k takes direction k of the thirty
// E, r, rho, vstar[3], g[3], Bse[9], Bbt[9], C[3] and accumulates its dot product exactly as lanes 31..33 accumulate the
// tendon-force cotangent.  The constants' tangents are derived in the kernel, once per rod and call, from the parameters
// themselves (adj_par_consts: the chain of kr_derive, the two inverses by d(M^-1) = -M^-1 dM M^-1).  L costs one more dot
// product per point; tendon_dirs is tensions (x) the tendon-force cotangent.
// Every OTHER output of the two calls comes from kr_adj.hip's own kernel, launched first: that is what makes them bit for bit
// the existing call's.  This kernel then runs with those output pointers null and writes g_par alone.  (One kernel for
// everything was measured first: the recursion's statements are the same text, but compiled beside the second evaluation
// they are contracted into fused multiply-adds differently, and at B = 1024, N = 100, T = 64 g_ctl differed in its last
// bits.)  With g_par == NULL only the first launch happens: the call IS the existing call.
// The rollout call is kr_adj.hip's composition, simulate_vjp_steps, whose workspace tail holds the step's g_par.
#include "kr_adj_impl.hpp"

namespace kr {

// One wavefront per SIMD is all the register file holds of this kernel (as of step_vjp_kernel: 264 VGPRs there); saying so lets
// the allocator use the whole file, and the fp32 instantiation then keeps no scratch slot behind its SGPR spills.
template <typename T>
__global__ __launch_bounds__(64 * ADJ_RODS_PER_WG) __attribute__((amdgpu_waves_per_eu(1, 1))) void step_vjp_par_kernel(const RodConst<double> P, const AdjArgs<T> A, const AdjPar<T> Q) {
  constexpr bool PAR = true, NNON = false;
  const AdjNn<T> NN{};  // (named in the discarded NNON statements only)
#include "kr_adj_body.inc"
}

template <typename T>
static int launch_step_vjp_par(kr_handle* h, const AdjArgs<T>& A, void* g_par, hipStream_t s) {
  if (int rc = launch_step_vjp_plain(h, A, s)) return rc;  // every output but g_par: the existing kernel, bit for bit
  if (!g_par) return KR_OK;
  AdjArgs<T> Ap = A;  // (reads only; g_par is all this launch writes)
  Ap.g_cur = Ap.g_prev = Ap.g_tens = Ap.g_bnd = nullptr;
  Ap.resid = nullptr;
  Ap.status = nullptr;
  AdjPar<T> Q{};
  Q.g_par = static_cast<T*>(g_par);
  const kr_params& p = h->params;
  Q.E = p.E; Q.r = p.r; Q.rho = p.rho;
  for (int i = 0; i < 3; ++i) {
    Q.vstar[i] = p.vstar[i];
    Q.g[i] = p.g[i];
  }
  const int64_t grid = (A.B + ADJ_RODS_PER_WG - 1) / ADJ_RODS_PER_WG;
  hipLaunchKernelGGL((step_vjp_par_kernel<T>), dim3((unsigned)grid), dim3(64 * ADJ_RODS_PER_WG), 0, s, h->cd, Ap, Q);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

}  // namespace kr

using namespace kr;

extern "C" int kr_step_vjp_par_batch(kr_handle* h, int64_t B, int scheme, const void* state_prev, const void* state_cur,
                                     const void* state_next, const void* tensions, const void* g_next, void* g_cur, void* g_prev,
                                     void* g_tensions, void* g_bnd, void* g_par, double* resid, int32_t* status, int dtype,
                                     void* stream) {
  return adj_step_entry("kr_step_vjp_par_batch", h, B, state_prev, state_cur, state_next, tensions, g_next, g_cur, g_prev, g_tensions,
                        g_bnd, resid, status, dtype, stream, [=](const char* api) { return adj_refuse(api, scheme, 0); },
                        [=](kr_handle* hh, const auto& A, hipStream_t s) { return launch_step_vjp_par(hh, A, g_par, s); });
}

// (the rollout's tail is w_par[B][KR_PAR], the step's parameter gradient that simulate_vjp_steps adds to g_par)
extern "C" int kr_simulate_vjp_par_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, const void* states,
                                         const void* state_prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd,
                                         void* g_par, double* resid, int32_t* status, int dtype, void* stream) {
  const size_t tail = g_par ? (size_t)B * KR_PAR * (dtype == KR_F32 ? sizeof(float) : sizeof(double)) : 0;
  return adj_simulate_entry("kr_simulate_vjp_par_batch", h, B, T, ctl, states, state_prev_init, g_states, g_prev_init, g_ctl, g_bnd, g_par,
                            resid, status, dtype, stream, [=](const char* api) { return adj_refuse(api, scheme, 0); }, tail,
                            [](kr_handle* hh, const auto& A, void* w_par, int64_t, hipStream_t s) { return launch_step_vjp_par(hh, A, w_par, s); });
}
