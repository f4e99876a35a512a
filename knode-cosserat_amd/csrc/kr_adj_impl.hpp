// kr_adj_impl.hpp - what the step adjoint's kernels share: the argument block, the lane helpers, the per-point tangents
// of the physics on dual numbers, the 6 x 6 solve and the accumulation kernel of the rollout.  Used by kr_adj.hip (MLP off)
// and kr_adj_nn.hip (the network's input Jacobian added to the per-point derivative); the mapping is described in kr_adj.hip.
#pragma once
#include "kr_internal.hpp"
#include "kr_point_dual.hpp"

namespace kr {

template <typename T>
struct AdjArgs {
  int64_t B;
  const T *prev, *cur, *next;  // [B][N][KR_SLOTS]
  const T* tens;               // tensions of rod b at tens[b * tens_stride .. + 4]
  int64_t tens_stride;
  const T* g_next;             // [B][N][KR_SLOTS]
  T *g_cur, *g_prev;           // [B][N][KR_SLOTS], nullable
  T* g_tens;                   // rod b at g_tens[b * g_tens_stride .. + 4], nullable
  int64_t g_tens_stride;
  T* g_bnd;                    // [B][KR_BND], nullable
  double* resid;               // rod b at resid[b * st_stride], nullable
  int32_t* status;             // rod b at status[b * st_stride], nullable
  int64_t st_stride;
};

constexpr int ADJ_RODS_PER_WG = 4;
constexpr int ADJ_SEEDS = 7;

template <int SRC>
__device__ __forceinline__ double adj_bcast(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), SRC), hi = __builtin_amdgcn_readlane((int)(b >> 32), SRC);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// sum over o < 19 of x_o d[o], x_o = component o of the vector whose components lanes 0..18 hold in `x`
template <int O = 0>
__device__ __forceinline__ double adj_dot19(double x, const double (&d)[25], double acc) {
  if constexpr (O < 19) return adj_dot19<O + 1>(x, d, fma(adj_bcast<O>(x), d[O], acc));
  else return acc;
}
// row r of y (reference order p h n m q w) -> slot of the packed record
__device__ __forceinline__ int adj_yslot(int r) { return r < 13 ? r + 12 : r - 13; }

// One grid point: the tangents d[25] of (y_s, z) along this lane's input direction, at the stored state of point j.
// `bad` collects a value that is not finite among everything read.
template <typename T>
__device__ __forceinline__ void adj_point(const RodConst<double>& P, const AdjArgs<T>& A, int64_t rec, int dir, const double (&tf)[3],
                                          double (&d)[25], bool& bad) {
  Dual in[47], out[25];
  const T* y = A.next + rec * KR_SLOTS;
  const T* c = A.cur + rec * KR_SLOTS;
  const T* p = A.prev + rec * KR_SLOTS;
#pragma unroll
  for (int k = 0; k < 19; ++k) in[k].v = (double)y[adj_yslot(k)];
#pragma unroll
  for (int k = 19; k < 32; ++k) in[k].v = 0.0;  // (history of p, h, n, m: no equation reads it)
#pragma unroll
  for (int k = 0; k < 12; ++k) in[32 + k].v = P.c1 * (double)c[k] + P.c2 * (double)p[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) in[44 + k].v = tf[k];
#pragma unroll
  for (int k = 0; k < 47; ++k) {
    bad |= !isfinite(in[k].v);
    in[k].d = k == dir ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) bad |= !isfinite((double)y[SL_V + k]);
  point_map_dual(P, in, false, out);
#pragma unroll
  for (int o = 0; o < 25; ++o) d[o] = out[o].d;
}

// nu of M^T nu = -a: Gaussian elimination with partial pivoting, every lane the same arithmetic on the same values.
// m[k][l] = d(n, m)_k / dG_l.  false: a pivot that is zero, not finite, or below 1e-13 of the largest entry.
__device__ __forceinline__ bool adj_solve6(const double (&m)[6][6], const double (&a)[6], double (&nu)[6]) {
  double w[6][7];
  double amax = 0.0;
#pragma unroll
  for (int r = 0; r < 6; ++r) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      w[r][c] = m[c][r];
      amax = fmax(amax, fabs(m[c][r]));
    }
    w[r][6] = -a[r];
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int p = c;
    double best = fabs(w[c][c]);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double v = fabs(w[r][c]);
      if (v > best) { best = v; p = r; }
    }
    ok = ok && best > 1e-13 * amax && isfinite(best);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const bool sw = r == p;
#pragma unroll
      for (int k = c; k < 7; ++k) {
        const double top = w[c][k], low = w[r][k];
        w[c][k] = sw ? low : top;
        w[r][k] = sw ? top : low;
      }
    }
    const double inv = 1.0 / w[c][c];
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double f = w[r][c] * inv;
#pragma unroll
      for (int k = c + 1; k < 7; ++k) w[r][k] = fma(-f, w[c][k], w[r][k]);
    }
  }
#pragma unroll
  for (int r = 5; r >= 0; --r) {
    double s = w[r][6];
#pragma unroll
    for (int k = r + 1; k < 6; ++k) s = fma(-w[r][k], nu[k], s);
    nu[r] = s / w[r][r];
  }
  return ok;
}

template <typename T>
__global__ __launch_bounds__(256) void adj_add_kernel(T* dst, const T* src, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = dst[i] + src[i];
}


template <typename T>
static int launch_add(T* dst, const T* src, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL((adj_add_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dst, src, n);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

}  // namespace kr
