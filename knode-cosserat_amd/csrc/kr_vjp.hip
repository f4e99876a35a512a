// kr_vjp.hip - derivatives of the physics of one grid point, y -> (y_s, z): what autograd propagates through
// CosseratRodTorch.ODE_parallel (reference cosserat_ode_torch.py:264-306, uncut graph) and through the op-by-op graph of
// CosseratRodTorch.getResidualEuler / ODE (:137-213, :325-367 - a graph that is CUT in two places, see below).
//
//   kr_ode_vjp_batch       (g_ys, g_z) -> J^T g with respect to y, yh, zh and the tendon force     (backward of ODE_parallel)
//   kr_ode_jacobian_batch  the 25 x 19 Jacobian d(y_s, z) / dy of every row                        (adjoint sweep of a14)
//
// Method: forward-mode automatic differentiation on dual numbers, in fp64 whatever the dtype of the arrays (the torch graph
// this replaces ran in fp64 too).  One thread evaluates the point map once with the tangent set to ONE input direction
// (19 + 19 + 6 + 3 = 47 of them per row), so a row takes 47 threads; thread (row, i) then owns component i of J^T g, or
// column i of the Jacobian - no reduction across threads, no atomics.  47 evaluations of ~400 flops per row is nothing:
// no caller of the reference differentiates with respect to these inputs (its training loops feed data), and the adjoint
// sweep handles N - 1 rows per call.
//
// `cut` reproduces the reference's graph where it differs from the function it evaluates: CosseratRodTorch.ODE assembles
// the quadratic part of the rotation matrix (:159-162) and the quaternion-rate matrix Omega(u) (:185-189) with
// torch.tensor([...]), i.e. as new leaves - through R, h is seen only via the factor 2 / (h . h), and h_s sees h but
// not u.  cut = 0 differentiates everything (ODE_parallel builds both with torch.stack, so its graph is complete).
#include "kr_internal.hpp"
#include "kr_point_dual.hpp"

namespace kr {

template <typename T>
struct VjpArgs {
  int64_t Q;
  const T *y, *yh, *zh, *tf;      // [Q][19], [Q][19], [Q][6], [Q][3]
  const T *g_ys, *g_z;            // VJP: cotangents [Q][19], [Q][6]
  T *o_y, *o_yh, *o_zh, *o_tf;    // VJP: J^T g per input block (any may be null)
  T* jac;                         // Jacobian mode: [Q][25][19]
  int cut, ndir;                  // ndir: 47 (VJP) or 19 (Jacobian: directions of y only)
};

template <typename T, bool JAC>
__global__ __launch_bounds__(256) void ode_vjp_kernel(const RodConst<double> P, const VjpArgs<T> A) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = t / A.ndir;
  const int dir = (int)(t - row * A.ndir);
  if (row >= A.Q) return;
  Dual in[47], out[25];
#pragma unroll
  for (int k = 0; k < 19; ++k) in[k] = {(double)A.y[row * 19 + k], 0.0};
#pragma unroll
  for (int k = 0; k < 19; ++k) in[19 + k] = {(double)A.yh[row * 19 + k], 0.0};
#pragma unroll
  for (int k = 0; k < 6; ++k) in[38 + k] = {(double)A.zh[row * 6 + k], 0.0};
#pragma unroll
  for (int k = 0; k < 3; ++k) in[44 + k] = {(double)A.tf[row * 3 + k], 0.0};
#pragma unroll
  for (int k = 0; k < 47; ++k) in[k].d = k == dir ? 1.0 : 0.0;
  point_map_dual(P, in, A.cut != 0, out);
  if constexpr (JAC) {
#pragma unroll
    for (int o = 0; o < 25; ++o) A.jac[(row * 25 + o) * 19 + dir] = (T)out[o].d;
  } else {
    double acc = 0.0;
#pragma unroll
    for (int o = 0; o < 19; ++o) acc = fma((double)A.g_ys[row * 19 + o], out[o].d, acc);
#pragma unroll
    for (int o = 0; o < 6; ++o) acc = fma((double)A.g_z[row * 6 + o], out[19 + o].d, acc);
    if (dir < 19) { if (A.o_y) A.o_y[row * 19 + dir] = (T)acc; }
    else if (dir < 38) { if (A.o_yh) A.o_yh[row * 19 + dir - 19] = (T)acc; }
    else if (dir < 44) { if (A.o_zh) A.o_zh[row * 6 + dir - 38] = (T)acc; }
    else if (A.o_tf) A.o_tf[row * 3 + dir - 44] = (T)acc;
  }
}

template <typename T, bool JAC>
static int launch_vjp(kr_handle* h, const VjpArgs<T>& A, hipStream_t s) {
  const int64_t threads = A.Q * A.ndir;
  const int64_t grid = (threads + 255) / 256;
  if (grid > 0x7fffffff) { set_error("Q too large"); return KR_E_ARG; }
  hipLaunchKernelGGL((ode_vjp_kernel<T, JAC>), dim3((unsigned)grid), dim3(256), 0, s, h->cd, A);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

}  // namespace kr

using namespace kr;

extern "C" {

int kr_ode_vjp_batch(kr_handle* h, int64_t Q, const void* y, const void* yh, const void* zh, const void* tf,
                     const void* g_dys, const void* g_z, int cut, void* g_y, void* g_yh, void* g_zh, void* g_tf,
                     int dtype, void* stream) {
  if (!h) { set_error("null handle"); return KR_E_ARG; }
  if (dtype != KR_F32 && dtype != KR_F64) { set_error("dtype must be KR_F32 or KR_F64"); return KR_E_ARG; }
  if (Q < 0) { set_error("Q < 0"); return KR_E_ARG; }
  if (Q == 0) return KR_OK;
  if (!y || !yh || !zh || !tf || !g_dys || !g_z) { set_error("null pointer argument"); return KR_E_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  if (dtype == KR_F32) {
    VjpArgs<float> A{Q, (const float*)y, (const float*)yh, (const float*)zh, (const float*)tf, (const float*)g_dys,
                     (const float*)g_z, (float*)g_y, (float*)g_yh, (float*)g_zh, (float*)g_tf, nullptr, cut, 47};
    return launch_vjp<float, false>(h, A, s);
  }
  VjpArgs<double> A{Q, (const double*)y, (const double*)yh, (const double*)zh, (const double*)tf, (const double*)g_dys,
                    (const double*)g_z, (double*)g_y, (double*)g_yh, (double*)g_zh, (double*)g_tf, nullptr, cut, 47};
  return launch_vjp<double, false>(h, A, s);
}

int kr_ode_jacobian_batch(kr_handle* h, int64_t Q, const void* y, const void* yh, const void* zh, const void* tf, int cut,
                          void* jac, int dtype, void* stream) {
  if (!h) { set_error("null handle"); return KR_E_ARG; }
  if (dtype != KR_F32 && dtype != KR_F64) { set_error("dtype must be KR_F32 or KR_F64"); return KR_E_ARG; }
  if (Q < 0) { set_error("Q < 0"); return KR_E_ARG; }
  if (Q == 0) return KR_OK;
  if (!y || !yh || !zh || !tf || !jac) { set_error("null pointer argument"); return KR_E_ARG; }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  if (dtype == KR_F32) {
    VjpArgs<float> A{Q, (const float*)y, (const float*)yh, (const float*)zh, (const float*)tf, nullptr, nullptr, nullptr,
                     nullptr, nullptr, nullptr, (float*)jac, cut, 19};
    return launch_vjp<float, true>(h, A, s);
  }
  VjpArgs<double> A{Q, (const double*)y, (const double*)yh, (const double*)zh, (const double*)tf, nullptr, nullptr, nullptr,
                    nullptr, nullptr, nullptr, (double*)jac, cut, 19};
  return launch_vjp<double, true>(h, A, s);
}

}  // extern "C"
