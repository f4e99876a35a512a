// kr_score.hip - the evaluation metrics of the reference's drivers on the device: per rod the exact
// dynamic-time-warping distance of two paths of 3-vectors (physics_multitrain.py:213, physics_train.py:159 without
// FastDTW's coarse-path restriction) and the position + zyx-Euler mean squared error x 1000 (physics_multitrain.py:215-222),
// read from the packed states where a simulate call left them.  All arithmetic fp64; T is the element type of the inputs.
//
//   dtw_kernel       one wavefront per rod, systolic: the columns of b are served in stripes of 64, lane l owns column
//                    64 s + l of stripe s and at step k fills row k - l of it, so a stripe takes Ta + 63 steps.  A cell
//                    needs its own lane's previous value (up), the neighbour lane's previous value (left, one DPP
//                    wave shift per step) and that shift's result of the step before (diag): the dependent chain of a
//                    step is shift, two minima, one add and a select - no LDS access (DESIGN.md section 4 rule 2).
//                    Off the chain: the samples of a are staged in the LDS once (fp64, structure of arrays, zero pads
//                    at both ends so that no read is predicated) and lane l reads row k + 1 - l one step ahead; lane 63
//                    leaves the last column of a stripe in the LDS, lane 0 of the next stripe reads it one step ahead
//                    (in place: row k - 63 is written after row k was read).  LDS: 32 Ta + 3.5 KB.
//   pose_mse_kernel  one workgroup of 256 threads per rod, threads stride over the T N grid-point records, slots
//                    12..19 (p, h, and one slot of n that is not used) of a record by aligned 16-byte loads, two fp64
//                    partial sums per thread, a fixed-order tree over the workgroup: no atomics.
#include "kr_internal.hpp"

namespace kr {

constexpr int DTW_WAVE_SHR1 = 0x138;  // DPP wave_shr:1 - lane l reads lane l - 1, lane 0 keeps `old`

// value of lane l - 1; lane 0 receives its own `first`
__device__ __forceinline__ double from_lane_below(double v, double first) {
  const long long b = __double_as_longlong(v), f = __double_as_longlong(first);
  const int lo = __builtin_amdgcn_update_dpp((int)(f & 0xFFFFFFFFll), (int)(b & 0xFFFFFFFFll), DTW_WAVE_SHR1, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(f >> 32), (int)(b >> 32), DTW_WAVE_SHR1, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// LDS of one rod: the samples of a as three arrays of DTW_PAD + Ta + DTW_PAD doubles (row i at DTW_PAD + i; the pads are
// zero, so every lane may read its row of every step, also before its first and after its last), then the edge column,
// Ta + DTW_PAD doubles
constexpr int DTW_PAD = 64;
__host__ __device__ constexpr size_t dtw_lds_doubles(int Ta) { return 3 * (size_t)(Ta + 2 * DTW_PAD) + (size_t)(Ta + DTW_PAD); }

template <typename T>
__global__ __launch_bounds__(64) void dtw_kernel(const T* __restrict__ a, int Ta, int64_t a_rod, int64_t a_step,
                                                 const T* __restrict__ b, int Tb, int64_t b_rod, int64_t b_step,
                                                 double* __restrict__ dist) {
  extern __shared__ __align__(16) double dtw_lds[];
  const int rows = Ta + 2 * DTW_PAD;
  double* ax = dtw_lds;
  double* ay = ax + rows;
  double* az = ay + rows;
  // edge[i]: D of row i in the column left of the current stripe - inf left of column 0 and beyond the last row; lane
  // 63 replaces it by its own column for the next stripe
  double* edge = az + rows;
  const int lane = threadIdx.x;
  const int64_t rod = blockIdx.x;
  const double inf = __builtin_inf();
  {
    const T* ar = a + rod * a_rod;
    for (int i = lane; i < rows; i += 64) {
      double x = 0.0, y = 0.0, z = 0.0;
      const int r = i - DTW_PAD;
      if ((unsigned)r < (unsigned)Ta) {  // (rows beyond the sequence's ends are not loaded)
        const T* s = ar + (int64_t)r * a_step;
        x = (double)s[0];
        y = (double)s[1];
        z = (double)s[2];
      }
      ax[i] = x;
      ay[i] = y;
      az[i] = z;
    }
    for (int i = lane; i < Ta + DTW_PAD; i += 64) edge[i] = inf;
  }
  __syncthreads();
  const int stripes = (Tb + 63) >> 6;
  const int steps = Ta + 63;
  double D = inf;
  for (int s = 0; s < stripes; ++s) {
    const int j = s * 64 + lane;
    const bool col = j < Tb;
    double bx = 0.0, by = 0.0, bz = 0.0;
    if (col) {  // (columns beyond the sequence's end are not loaded)
      const T* p = b + rod * b_rod + (int64_t)j * b_step;
      bx = (double)p[0];
      by = (double)p[1];
      bz = (double)p[2];
    }
    const bool feeds = s + 1 < stripes && lane == 63;  // column 64 s + 63 is the next stripe's edge
    D = inf;                                           // row -1 of every column
    double diag = (s == 0 && lane == 0) ? 0.0 : inf;   // D[-1][-1] = 0, every other cell of row -1 / column -1 is inf
    const double* rx = ax + (DTW_PAD - lane);          // row k - lane of step k at rx[k]
    const double* ry = ay + (DTW_PAD - lane);
    const double* rz = az + (DTW_PAD - lane);
    // one step: the operands of step k (c*, first) were fetched during step k - 1, those of step k + 1 (n*, nfirst) are
    // fetched here
    auto step = [&](int k, double cx, double cy, double cz, double first, double& nx, double& ny, double& nz,
                    double& nfirst) {
      nx = rx[k + 1];
      ny = ry[k + 1];
      nz = rz[k + 1];
      nfirst = edge[k + 1];
      const int i = k - lane;
      const bool act = col && (unsigned)i < (unsigned)Ta;
      const double left = from_lane_below(D, first);
      const double cost = (fabs(cx - bx) + fabs(cy - by)) + fabs(cz - bz);
      const double d = cost + fmin(fmin(D, left), diag);
      diag = left;
      D = act ? d : D;
      if (feeds && act) edge[i] = D;  // (row k - 63: lane 0 read it 64 steps ago)
    };
    double x0 = rx[0], y0 = ry[0], z0 = rz[0], f0 = edge[0], x1, y1, z1, f1;
    int k = 0;
    for (; k + 1 < steps; k += 2) {
      step(k, x0, y0, z0, f0, x1, y1, z1, f1);
      step(k + 1, x1, y1, z1, f1, x0, y0, z0, f0);
    }
    if (k < steps) step(k, x0, y0, z0, f0, x1, y1, z1, f1);
  }
  if (lane == ((Tb - 1) & 63)) dist[rod] = D;  // (the owner of the last column keeps its last row's value)
}

// slots 12..18 of one record: p[3], h[4]
template <typename T>
__device__ __forceinline__ void load_pose(const T* rec, double (&p)[3], double (&q)[4]);
template <>
__device__ __forceinline__ void load_pose<double>(const double* rec, double (&p)[3], double (&q)[4]) {
  const double2* r = reinterpret_cast<const double2*>(rec + 12);  // record = 224 bytes, slot 12 at byte 96
  const double2 v0 = r[0], v1 = r[1], v2 = r[2], v3 = r[3];
  p[0] = v0.x; p[1] = v0.y; p[2] = v1.x;
  q[0] = v1.y; q[1] = v2.x; q[2] = v2.y; q[3] = v3.x;
}
template <>
__device__ __forceinline__ void load_pose<float>(const float* rec, double (&p)[3], double (&q)[4]) {
  const float4* r = reinterpret_cast<const float4*>(rec + 12);  // record = 112 bytes, slot 12 at byte 48
  const float4 v0 = r[0], v1 = r[1];
  p[0] = v0.x; p[1] = v0.y; p[2] = v0.z;
  q[0] = v0.w; q[1] = v1.x; q[2] = v1.y; q[3] = v1.z;
}

// SciPy's Rotation.from_quat(q, scalar_first=True).as_euler("zyx") in closed form (knode_rod.h); host twin:
// krod_eval.euler_zyx
__device__ __forceinline__ void euler_zyx(const double (&q)[4], double (&e)[3]) {
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  e[0] = atan2(2.0 * (w * z - x * y), 1.0 - 2.0 * (y * y + z * z));
  e[1] = asin(fmin(fmax(2.0 * (x * z + w * y), -1.0), 1.0));
  e[2] = atan2(2.0 * (w * x - y * z), 1.0 - 2.0 * (x * x + y * y));
}

constexpr int MSE_THREADS = 256;

template <typename T>
__global__ __launch_bounds__(MSE_THREADS) void pose_mse_kernel(int64_t B, int64_t T_states, int N, const T* __restrict__ states,
                                                               const T* __restrict__ ref, int64_t ref_B,
                                                               double* __restrict__ mse, double* __restrict__ parts) {
  __shared__ double sum_p[MSE_THREADS], sum_e[MSE_THREADS];
  const int tid = threadIdx.x;
  const int64_t rod = blockIdx.x;
  const int64_t ref_rod = ref_B == 1 ? 0 : rod;
  const int64_t samples = T_states * N;
  double sp = 0.0, se = 0.0;
  for (int64_t id = tid; id < samples; id += MSE_THREADS) {
    const int64_t t = id / N;
    const int64_t jj = id - t * N;
    double p[3], q[4], pr[3], qr[4], e[3], er[3];
    load_pose(states + ((t * B + rod) * N + jj) * KR_SLOTS, p, q);
    load_pose(ref + ((t * ref_B + ref_rod) * N + jj) * KR_SLOTS, pr, qr);
    euler_zyx(q, e);
    euler_zyx(qr, er);
    for (int r = 0; r < 3; ++r) {
      const double dp = p[r] - pr[r], de = e[r] - er[r];
      sp += dp * dp;
      se += de * de;
    }
  }
  sum_p[tid] = sp;
  sum_e[tid] = se;
  __syncthreads();
  for (int half = MSE_THREADS / 2; half > 0; half >>= 1) {  // fixed order: reproducible bit for bit
    if (tid < half) {
      sum_p[tid] += sum_p[tid + half];
      sum_e[tid] += sum_e[tid + half];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double tp = sum_p[0], te = sum_e[0];
    if (parts) { parts[2 * rod] = tp; parts[2 * rod + 1] = te; }
    mse[rod] = (tp + te) / (double)(6 * samples) * 1000.0;  // np.mean(...) * 1000
  }
}

template <typename T>
static int launch_dtw(int64_t B, const T* a, int Ta, int64_t ars, int64_t ass, const T* b, int Tb, int64_t brs, int64_t bss,
                      double* dist, hipStream_t s) {
  const size_t smem = sizeof(double) * dtw_lds_doubles(Ta);
  if (int rc = dyn_lds(reinterpret_cast<const void*>(&dtw_kernel<T>), smem)) return rc;
  hipLaunchKernelGGL(dtw_kernel<T>, dim3((unsigned)B), dim3(64), smem, s, a, Ta, ars, ass, b, Tb, brs, bss, dist);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

}  // namespace kr

using namespace kr;

#define KR_SCORE_ARG(cond, msg) \
  if (cond) {                   \
    set_error(msg);             \
    return KR_E_ARG;            \
  }

extern "C" int kr_dtw_batch(kr_handle* h, int64_t B, const void* a, int64_t Ta, int64_t a_rod_stride, int64_t a_step_stride,
                            const void* b, int64_t Tb, int64_t b_rod_stride, int64_t b_step_stride, double* dist, int dtype,
                            void* stream) {
  KR_SCORE_ARG(!h, "null handle");
  KR_SCORE_ARG(!a || !b || !dist, "kr_dtw_batch: null pointer argument");
  KR_SCORE_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_SCORE_ARG(B < 1, "kr_dtw_batch: B < 1");
  KR_SCORE_ARG(Ta < 1 || Tb < 1, "kr_dtw_batch: Ta and Tb must be >= 1");
  KR_SCORE_ARG(a_rod_stride < 0 || a_step_stride < 0 || b_rod_stride < 0 || b_step_stride < 0,
               "kr_dtw_batch: strides must be >= 0");
  if (Ta > KR_DTW_MAX_LEN || Tb > KR_DTW_MAX_LEN || B > 0x7FFFFFFFll) {
    set_error("kr_dtw_batch: sequences of " + std::to_string(Ta) + " and " + std::to_string(Tb) + " samples: at most " +
              std::to_string(KR_DTW_MAX_LEN) + " samples per sequence are served (and at most 2^31 - 1 rods)");
    return KR_E_UNSUPPORTED;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  return dtype == KR_F32 ? launch_dtw<float>(B, (const float*)a, (int)Ta, a_rod_stride, a_step_stride, (const float*)b, (int)Tb,
                                             b_rod_stride, b_step_stride, dist, s)
                         : launch_dtw<double>(B, (const double*)a, (int)Ta, a_rod_stride, a_step_stride, (const double*)b,
                                              (int)Tb, b_rod_stride, b_step_stride, dist, s);
}

// kr_pose_mse_batch (P = the handle's N) and kr_pose_mse_points_batch (P given): one kernel, P records per rod and step
static int pose_mse_impl(const std::string& who, kr_handle* h, int64_t B, int64_t T, int64_t P, const void* states, const void* ref_states,
                         int64_t ref_B, double* mse, double* parts, int dtype, void* stream) {
  KR_SCORE_ARG(!h, "null handle");
  KR_SCORE_ARG(!states || !ref_states || !mse, who + ": null pointer argument");
  KR_SCORE_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_SCORE_ARG(B < 1, who + ": B < 1");
  KR_SCORE_ARG(T < 1, who + ": T < 1");
  KR_SCORE_ARG(P < 1 || P > 0x7FFFFFFFll, who + ": P must be >= 1 (and below 2^31)");
  KR_SCORE_ARG(ref_B != 1 && ref_B != B, who + ": ref_B must be 1 or B");
  KR_SCORE_ARG(((uintptr_t)states | (uintptr_t)ref_states) & 15, who + ": states and ref_states must be 16-byte aligned");
  if (B > 0x7FFFFFFFll) {
    set_error(who + ": at most 2^31 - 1 rods");
    return KR_E_UNSUPPORTED;
  }
  const int N = (int)P;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  if (dtype == KR_F32)
    hipLaunchKernelGGL(pose_mse_kernel<float>, dim3((unsigned)B), dim3(MSE_THREADS), 0, s, B, T, N, (const float*)states,
                       (const float*)ref_states, ref_B, mse, parts);
  else
    hipLaunchKernelGGL(pose_mse_kernel<double>, dim3((unsigned)B), dim3(MSE_THREADS), 0, s, B, T, N, (const double*)states,
                       (const double*)ref_states, ref_B, mse, parts);
  KR_HIP(hipGetLastError());
  return KR_OK;
}

extern "C" int kr_pose_mse_batch(kr_handle* h, int64_t B, int64_t T, const void* states, const void* ref_states, int64_t ref_B,
                                 double* mse, double* parts, int dtype, void* stream) {
  KR_SCORE_ARG(!h, "null handle");
  return pose_mse_impl("kr_pose_mse_batch", h, B, T, h->params.N, states, ref_states, ref_B, mse, parts, dtype, stream);
}

extern "C" int kr_pose_mse_points_batch(kr_handle* h, int64_t B, int64_t T, int64_t P, const void* records, const void* ref_records,
                                        int64_t ref_B, double* mse, double* parts, int dtype, void* stream) {
  return pose_mse_impl("kr_pose_mse_points_batch", h, B, T, P, records, ref_records, ref_B, mse, parts, dtype, stream);
}
