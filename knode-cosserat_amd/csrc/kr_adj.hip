// kr_adj.hip - the adjoint of one solved implicit BDF2 step (MLP off) and the backward pass over a stored rollout.
//
//   kr_step_vjp_batch      cotangent of state_next -> gradients with respect to state_cur, state_prev, the tensions and
//                          the boundary data (base state, tip wrench) of the step        (knode.py:70-100, one pass of the loop)
//   kr_simulate_vjp_batch  the same composed over the T steps of a stored trajectory     (knode.py:55-102)
//
// The step solves r(G) = [F_tip - n_{N-1}, M_tip - m_{N-1}] = 0 for the base wrench G by sweeping
// y_{j+1} = y_j + ds f(y_j, hist_j, tf) from y_0 = [p0, h0, G, q0, w0] (cosserat_ode.py:188-213).  Its derivative is that
// of the sweep at fixed G plus the implicit-function term through G:
//
//   pass 1  carries SEVEN cotangent vectors back along the rod at once: the caller's g (seed 0) and the six unit seeds
//           on (n, m) of the tip.  lambda_{N-1} = seed, lambda_j = g_y[j] + lambda_{j+1} + J_j^T [ds lambda_{j+1}; g_z[j]].
//           The (n, m) rows of lambda_0 are a = dL/dG at fixed tip condition (seed 0) and the rows of
//           M = d(n, m)_{N-1} / dG (seeds 1..6).
//   solve   M^T nu = -a (6 x 6, partial pivoting): nu is the cotangent the tip condition puts on (n, m)_{N-1}.
//   pass 2  carries the one combined cotangent (g, plus nu on the tip's (n, m)) and emits, point by point, the columns of
//           J_j^T in the history (q, w, v, u of c1 cur + c2 prev) and in the tendon force.  The (n, m) rows of its lambda_0
//           are zero up to rounding: |.|_inf / |a|_inf is reported as `resid`.
//
// Nothing is re-solved: the states are read from state_next.  Arithmetic is fp64 whatever the element type of the arrays.
//
// Mapping: one wavefront per rod, four rods per workgroup, no LDS.  The per-point derivative is forward mode on dual
// numbers (kr_point_dual.hpp): lane l evaluates the point map once with the tangent along ONE input direction - lanes
// 0..18 the components of y, 19..30 the twelve history values f reads, 31..33 the tendon force - and so owns component l
// of J^T x for any x: a dot product of its 25 output tangents with x.  A lane below 19 keeps component l of every
// cotangent vector in a register; the dot product fetches the others lane by lane (v_readlane with a constant lane).
// The recursion is serial in j and the rods are independent: no atomics, no cross-wavefront traffic, and a rod's result
// does not depend on the batch it rides in.
//
// The recursion is written once, in kr_adj_body.inc, and compiled into this unit's kernel with both of its forms off, into
// kr_adj_par.hip's with PAR and into kr_adj_nn.hip's with NNON.  The rollout loop (simulate_vjp_steps) and the path from a C
// entry point to a launch (adj_step_entry, adj_simulate_entry) are likewise written once, in kr_adj_impl.hpp; a unit
// supplies its refusals and its launch.
#include "kr_adj_impl.hpp"

namespace kr {

template <typename T>
__global__ __launch_bounds__(64 * ADJ_RODS_PER_WG) void step_vjp_kernel(const RodConst<double> P, const AdjArgs<T> A) {
  constexpr bool PAR = false, NNON = false;
  const AdjPar<T> Q{};  // (Q, NN: named in the discarded PAR and NNON statements only)
  const AdjNn<T> NN{};
#include "kr_adj_body.inc"
}

template <typename T>
static int launch_step_vjp(kr_handle* h, const AdjArgs<T>& A, hipStream_t s) {
  const int64_t grid = (A.B + ADJ_RODS_PER_WG - 1) / ADJ_RODS_PER_WG;
  hipLaunchKernelGGL((step_vjp_kernel<T>), dim3((unsigned)grid), dim3(64 * ADJ_RODS_PER_WG), 0, s, h->cd, A);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

int launch_step_vjp_plain(kr_handle* h, const AdjArgs<float>& A, hipStream_t s) { return launch_step_vjp<float>(h, A, s); }
int launch_step_vjp_plain(kr_handle* h, const AdjArgs<double>& A, hipStream_t s) { return launch_step_vjp<double>(h, A, s); }

int adj_refuse(const char* api, int scheme, int use_nn) {
  if (use_nn != 0) {
    set_error(std::string(api) + ": the adjoint with the MLP on is not served (the network's input Jacobian is not part of the "
              "per-point derivative); nothing falls back to the physics alone");
    return KR_E_UNSUPPORTED;
  }
  if (scheme == KR_RK4) {
    set_error(std::string(api) + ": the adjoint of the RK4 sweep is not served; nothing falls back to the Euler sweep");
    return KR_E_UNSUPPORTED;
  }
  if (scheme != KR_EULER) {
    set_error(std::string(api) + ": scheme must be KR_EULER");
    return KR_E_ARG;
  }
  return KR_OK;
}

}  // namespace kr

using namespace kr;

extern "C" int kr_step_vjp_batch(kr_handle* h, int64_t B, int scheme, const void* state_prev, const void* state_cur,
                                 const void* state_next, const void* tensions, const void* g_next, void* g_cur, void* g_prev,
                                 void* g_tensions, void* g_bnd, double* resid, int32_t* status, int use_nn, int dtype, void* stream) {
  return adj_step_entry("kr_step_vjp_batch", h, B, state_prev, state_cur, state_next, tensions, g_next, g_cur, g_prev, g_tensions, g_bnd,
                        resid, status, dtype, stream, [=](const char* api) { return adj_refuse(api, scheme, use_nn); },
                        [](kr_handle* hh, const auto& A, hipStream_t s) { return launch_step_vjp(hh, A, s); });
}

// The backward pass over a stored rollout: the composition of step adjoints stated at simulate_vjp_steps (kr_adj_impl.hpp)
extern "C" int kr_simulate_vjp_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, const void* states,
                                     const void* state_prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd,
                                     double* resid, int32_t* status, int use_nn, int dtype, void* stream) {
  return adj_simulate_entry("kr_simulate_vjp_batch", h, B, T, ctl, states, state_prev_init, g_states, g_prev_init, g_ctl, g_bnd, nullptr,
                            resid, status, dtype, stream, [=](const char* api) { return adj_refuse(api, scheme, use_nn); }, 0,
                            [](kr_handle* hh, const auto& A, void*, int64_t, hipStream_t s) { return launch_step_vjp(hh, A, s); });
}
