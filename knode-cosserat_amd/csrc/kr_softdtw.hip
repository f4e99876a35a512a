// kr_softdtw.hip - soft-DTW (M. Cuturi, M. Blondel 2017) of two paths of 3-vectors per rod and its gradient with respect
// to the first path, as krod_eval.softdtw_grad states it (include/knode_rod.h): the differentiable form of kr_score.hip's
// metric, written where the rollout adjoint reads its cotangent.  All arithmetic fp64; T is the element type of the inputs
// and of the gradient.
//
//   softdtw_kernel   one wavefront per rod.
//     stage     the samples of a into the LDS (fp64, structure of arrays, zero pads at both ends so that no read is
//               predicated), both sequences looked through for a sample that is not finite: such a rod ends with NaN.
//     forward   dtw_kernel's systolic sweep (kr_score.hip): columns of b in stripes of 64, lane l owns column 64 s + l and
//               fills row k - l at step k; up is the lane's own previous value, left one DPP wave shift, diag that shift's
//               result of the step before; the last column of a stripe goes to the next one through the LDS edge.  The cell
//               is R = c + softmin(up, left, diag) = c + (m - gamma log(sum exp((m - r) / gamma))): three exp and one log,
//               software sequences, are the dependent chain of a step; the samples of a, the edge and the cost are fetched
//               or formed one step ahead of it, the table's store follows it.  A predecessor outside the table (+inf) is
//               taken out by a select, never by exp(-inf), and a lane without a cell feeds constants to exp and log.
//     table     the backward sweep needs every cell; kept is Q = R - c, the softmin before the cost is added (R is one add
//               away, and the weights below want Q): in the LDS, row-major (row stride Tb rounded up to even: the lanes of
//               a step never share a bank pair), while the staging and the table fit SD_LDS_WITH_TABLE, else in the rod's slice of the caller's workspace, stripe-major, step-major, lane-minor
//               (cell of lane l at step k of stripe s at (s (Ta + 63) + k) 64 + l): a step is one contiguous 512-byte
//               store of the wavefront and the backward sweep reads it the same way.
//     backward  the mirrored sweep: last stripe first, steps descending, so lane l again has row k - l at step k; down
//               (i + 1, j) is the lane's own previous cell, right (i, j + 1) comes from the lane above by the opposite
//               wave shift, diag (i + 1, j + 1) is that shift's result of the step before - Q and E of the three
//               successors travel in registers; column 64 s of a stripe goes to lane 63 of the stripe before it through
//               two LDS edges.  E = sum E(p, q) exp((Q(p, q) - R(i, j)) / gamma) over the successors inside the table (a
//               select, not a sentinel), the last cell is 1.  Q(p, q) is the statement's R(p, q) - c(p, q) without the
//               rounding of adding c and taking it off again: where one predecessor carries the minimum alone (a hard
//               table, gamma far below the gaps between paths) Q(p, q) IS that predecessor's R, the exponent is 0 and E is
//               1 along the warp path to the last bit, where R(p, q) - R(i, j) - c(p, q) leaves ulp(R) / gamma per cell.
//     gradient  g_a[i] = sum_j E(i, j) dc(i, j)/da_i: at a step the 64 lanes hold 64 different rows, so each adds its term
//               to its row's three sums in the LDS - no two lanes touch one address in a step, steps are in program order:
//               row i is summed over j in DECREASING j, always, whatever B and wherever the rod stands.  No atomics.
//               (krod_eval sums in increasing j; the difference is within the rounding of a sum of n terms.)
#include "kr_internal.hpp"

namespace kr {

constexpr int SD_WAVE_SHR1 = 0x138;  // DPP wave_shr:1 - lane l reads lane l - 1, lane 0 keeps `old`
constexpr int SD_WAVE_SHL1 = 0x130;  // DPP wave_shl:1 - lane l reads lane l + 1, lane 63 keeps `old`
constexpr int SD_PAD = 64;           // rows a lane may read before the first / after the last row
// The table stays in the LDS while everything fits a quarter of a CU's 160 KB: four rods, one per SIMD, stay resident.  A
// larger table in the LDS would leave SIMDs idle in a batch; in the workspace its stores and loads are off the chain anyway.
constexpr size_t SD_LDS_WITH_TABLE = 40 * 1024;

// value of the neighbour lane (CTRL: which); the lane without one receives its own `first`
template <int CTRL>
__device__ __forceinline__ double sd_from_lane(double v, double first) {
  const long long b = __double_as_longlong(v), f = __double_as_longlong(first);
  const int lo = __builtin_amdgcn_update_dpp((int)(f & 0xFFFFFFFFll), (int)(b & 0xFFFFFFFFll), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(f >> 32), (int)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// a product the compiler may not fuse into the add that follows (the unit is built with -ffp-contract=fast; the squared
// cost is (dx dx + dy dy) + dz dz in exactly this rounding, so that a 1 x 1 table returns the host's bits)
__device__ __forceinline__ double sd_square(double x) {
  double p = x * x;
  asm volatile("" : "+v"(p));
  return p;
}

__device__ __forceinline__ double sd_cost(bool squared, double dx, double dy, double dz) {
  const double l1 = (fabs(dx) + fabs(dy)) + fabs(dz);
  const double sq = (sd_square(dx) + sd_square(dy)) + sd_square(dz);
  return squared ? sq : l1;
}

// d cost / d a_k: sign(d) with sign(0) = 0, or 2 d
__device__ __forceinline__ double sd_dcost(bool squared, double d) {
  const double sgn = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
  return squared ? 2.0 * d : sgn;
}

// LDS of one rod, in doubles: x, y, z of a (row i at SD_PAD + i, zero pads), two edge columns (row i at SD_PAD + i: the
// forward sweep reads rows 0 .. Ta + 63 of the first, the backward sweep rows -64 .. Ta - 1 of both), the three
// gradient sums per row, then the table
struct SdLayout {
  size_t rows, a, edge, gsum, table, total;  // offsets and total in doubles
  size_t stride, cells;                      // of the table in the LDS: doubles per row, doubles in all
  bool table_in_lds;
};
__host__ __device__ inline size_t sd_table_doubles_ws(int Ta, int Tb) { return (size_t)((Tb + 63) >> 6) * (size_t)(Ta + 63) * 64; }
__host__ __device__ inline SdLayout sd_layout(int Ta, int Tb) {
  SdLayout L;
  L.rows = (size_t)Ta + 2 * SD_PAD;
  L.a = 0;
  L.edge = 3 * L.rows;
  L.gsum = 5 * L.rows;
  L.table = 5 * L.rows + 3 * (size_t)Ta;
  // Row-major with an EVEN row stride: at a step lane l addresses row k - l, column 64 s + l, so neighbouring lanes lie
  // stride - 1 doubles apart - an odd number, and 32 lanes fall into 32 different bank pairs whatever Tb (with the stride
  // Tb itself, Tb = 33 or 65 would put every lane of a step into one pair).
  L.stride = ((size_t)Tb + 1) & ~(size_t)1;
  L.cells = (size_t)Ta * L.stride;
  L.table_in_lds = sizeof(double) * (L.table + L.cells) <= SD_LDS_WITH_TABLE;
  L.total = L.table;  // (the launch adds the table when it is in the LDS and the gradient is asked for)
  return L;
}

// TLDS: the table of Q is in the LDS (sd_layout's table_in_lds), else in the rod's slice of the workspace.  `grad` = 0:
// value only - the same forward instructions, nothing stored for a backward sweep and none run.
template <typename T, bool TLDS>
__global__ __launch_bounds__(64) void softdtw_kernel(const T* __restrict__ a, int Ta, int64_t a_rod, int64_t a_step,
                                                     const T* __restrict__ b, int Tb, int64_t b_rod, int64_t b_step,
                                                     double gamma, int squared_cost, double* __restrict__ value,
                                                     T* __restrict__ g, int64_t g_rod, int64_t g_step,
                                                     double* __restrict__ ws, int grad) {
  extern __shared__ __align__(16) double sd_lds[];
  const SdLayout L = sd_layout(Ta, Tb);
  const int rows = (int)L.rows;
  double* ax = sd_lds + L.a;
  double* ay = ax + rows;
  double* az = ay + rows;
  double* edgeR = sd_lds + L.edge + SD_PAD;  // indexed by the row, -64 .. Ta + 63; forward: R, backward: Q
  double* edgeE = edgeR + rows;  // (never initialised: every value that comes from it is used behind a select - see `vr`, `vd`)
  double* gx = sd_lds + L.gsum;
  double* gy = gx + Ta;
  double* gz = gy + Ta;
  const int lane = threadIdx.x;
  const int64_t rod = blockIdx.x;
  const int stripes = (Tb + 63) >> 6;
  const int steps = Ta + 63;
  double* table = TLDS ? sd_lds + L.table : ws + (size_t)rod * sd_table_doubles_ws(Ta, Tb);
  const double inf = __builtin_inf();
  const bool squared = squared_cost != 0;
  const double inv_gamma = 1.0 / gamma;
  const T* ar = a + rod * a_rod;
  const T* br = b + rod * b_rod;
  T* gr = grad ? g + rod * g_rod : nullptr;

  // ---- stage a, look through both sequences for a sample that is not finite ----
  bool bad = false;
  for (int i = lane; i < rows; i += 64) {
    double x = 0.0, y = 0.0, z = 0.0;
    const int r = i - SD_PAD;
    if ((unsigned)r < (unsigned)Ta) {  // (nothing but the Ta samples is read)
      const T* s = ar + (int64_t)r * a_step;
      x = (double)s[0];
      y = (double)s[1];
      z = (double)s[2];
      bad = bad || !(isfinite(x) && isfinite(y) && isfinite(z));
    }
    ax[i] = x;
    ay[i] = y;
    az[i] = z;
    edgeR[i - SD_PAD] = inf;  // column -1: +inf in every row
  }
  for (int j = lane; j < Tb; j += 64) {
    const T* s = br + (int64_t)j * b_step;
    bad = bad || !(isfinite((double)s[0]) && isfinite((double)s[1]) && isfinite((double)s[2]));
  }
  for (int i = lane; i < 3 * Ta; i += 64) gx[i] = 0.0;
  if (__ballot(bad) != 0ull) {  // (the whole wavefront leaves together)
    const double nan = __builtin_nan("");
    if (lane == 0) value[rod] = nan;
    if (grad)
      for (int i = lane; i < Ta; i += 64) {
        T* o = gr + (int64_t)i * g_step;
        o[0] = (T)nan;
        o[1] = (T)nan;
        o[2] = (T)nan;
      }
    return;
  }
  __syncthreads();

  const double* rx = ax + (SD_PAD - lane);  // row k - lane of step k at rx[k]
  const double* ry = ay + (SD_PAD - lane);
  const double* rz = az + (SD_PAD - lane);

  // ---- forward ----
  double R = inf;
  for (int s = 0; s < stripes; ++s) {
    const int j = s * 64 + lane;
    const bool col = j < Tb;
    double bx = 0.0, by = 0.0, bz = 0.0;
    if (col) {  // (columns beyond the sequence's end are not loaded)
      const T* p = br + (int64_t)j * b_step;
      bx = (double)p[0];
      by = (double)p[1];
      bz = (double)p[2];
    }
    const bool feeds = s + 1 < stripes && lane == 63;  // column 64 s + 63 is the next stripe's edge
    R = inf;                                           // row -1 of every column
    double diag = (s == 0 && lane == 0) ? 0.0 : inf;   // R(-1, -1) = 0, every other cell of row -1 / column -1 is inf
    double* cell = TLDS ? table + j : table + ((size_t)s * steps * 64 + lane);  // TLDS: row i at cell[i stride]; else step k at cell[64 k]
    // one step: the operands of step k (c*, first) were fetched during step k - 1, those of step k + 1 are fetched here
    auto step = [&](int k, double cx, double cy, double cz, double first, double& nx, double& ny, double& nz, double& nfirst) {
      nx = rx[k + 1];
      ny = ry[k + 1];
      nz = rz[k + 1];
      nfirst = edgeR[k + 1];
      const int i = k - lane;
      const bool act = col && (unsigned)i < (unsigned)Ta;
      const double left = sd_from_lane<SD_WAVE_SHR1>(R, first);
      const double cost = sd_cost(squared, cx - bx, cy - by, cz - bz);
      const double up = R;
      const double m = fmin(fmin(up, left), diag);
      const double mm = act ? m : 0.0;  // (a lane without a cell: finite arguments, its result is dropped)
      const double eu = (act && up < inf) ? exp((mm - up) * inv_gamma) : 0.0;
      const double el = (act && left < inf) ? exp((mm - left) * inv_gamma) : 0.0;
      const double ed = (act && diag < inf) ? exp((mm - diag) * inv_gamma) : 0.0;
      const double sum = act ? (eu + el) + ed : 1.0;
      const double q = mm - gamma * log(sum);
      diag = left;
      R = act ? cost + q : R;
      if (act) {
        if (grad) cell[TLDS ? (size_t)i * L.stride : (size_t)k * 64] = q;
        if (feeds) edgeR[i] = R;  // (row k - 63: lane 0 read it 64 steps ago)
      }
    };
    double x0 = rx[0], y0 = ry[0], z0 = rz[0], f0 = edgeR[0], x1, y1, z1, f1;
    int k = 0;
    for (; k + 1 < steps; k += 2) {
      step(k, x0, y0, z0, f0, x1, y1, z1, f1);
      step(k + 1, x1, y1, z1, f1, x0, y0, z0, f0);
    }
    if (k < steps) step(k, x0, y0, z0, f0, x1, y1, z1, f1);
  }
  if (lane == ((Tb - 1) & 63)) value[rod] = R;  // (the owner of the last column keeps its last row's value)
  if (!grad) return;
  __syncthreads();  // (the table and the edge are read by other lanes than wrote them)

  // ---- backward ----
  for (int s = stripes - 1; s >= 0; --s) {
    const int j = s * 64 + lane;
    const bool col = j < Tb;
    const bool right_in = j + 1 < Tb;
    double bx = 0.0, by = 0.0, bz = 0.0;
    if (col) {
      const T* p = br + (int64_t)j * b_step;
      bx = (double)p[0];
      by = (double)p[1];
      bz = (double)p[2];
    }
    const bool feeds = s > 0 && lane == 0;  // column 64 s is the edge of the stripe before
    // the lane's own previous cell (i + 1, j) and the lane above's cell of the step before (i + 1, j + 1): Q, E
    double Qs = 0.0, Es = 0.0, Qd = 0.0, Ed = 0.0;
    const double* cell = TLDS ? table + (col ? j : Tb - 1) : table + ((size_t)s * steps * 64 + lane);
    // the table's entry of step k (TLDS: of a row inside the table whatever k, what a lane without a cell reads is dropped)
    auto own = [&](int k) -> double {
      if (TLDS) {
        const int i = k - lane;
        return cell[(size_t)(i < 0 ? 0 : (i < Ta ? i : Ta - 1)) * L.stride];
      }
      return cell[(size_t)(k < 0 ? 0 : k) * 64];
    };
    auto step = [&](int k, double cx, double cy, double cz, double fQ, double fE, double q, double& nx, double& ny, double& nz,
                    double& nfQ, double& nfE, double& nq) {
      nx = rx[k - 1];
      ny = ry[k - 1];
      nz = rz[k - 1];
      nfQ = edgeR[k - 64];
      nfE = edgeE[k - 64];
      nq = own(k - 1);
      const int i = k - lane;
      const bool act = col && (unsigned)i < (unsigned)Ta;
      const double Qr = sd_from_lane<SD_WAVE_SHL1>(Qs, fQ);
      const double Er = sd_from_lane<SD_WAVE_SHL1>(Es, fE);
      const double dx = cx - bx, dy = cy - by, dz = cz - bz;
      const double r = sd_cost(squared, dx, dy, dz) + q;  // R(i, j), the forward sweep's add
      const bool down_in = act && i + 1 < Ta;
      const bool vr = act && right_in, vd = down_in && right_in;
      // (a successor outside the table: a constant to exp, its term taken out)
      const double wdown = exp(down_in ? (Qs - r) * inv_gamma : 0.0);
      const double wright = exp(vr ? (Qr - r) * inv_gamma : 0.0);
      const double wdiag = exp(vd ? (Qd - r) * inv_gamma : 0.0);
      const double tdown = down_in ? Es * wdown : 0.0;
      const double tright = vr ? Er * wright : 0.0;
      const double tdiag = vd ? Ed * wdiag : 0.0;
      const bool last = i == Ta - 1 && j == Tb - 1;  // its one successor is (Ta, Tb): E = 1, R the same, c = 0
      const double E = last ? 1.0 : (tdown + tright) + tdiag;
      Qd = Qr;
      Ed = Er;
      if (act) {
        Qs = q;
        Es = E;
        gx[i] += E * sd_dcost(squared, dx);
        gy[i] += E * sd_dcost(squared, dy);
        gz[i] += E * sd_dcost(squared, dz);
        if (feeds) {  // (row k: lane 63 of this stripe read it 63 steps ago, reads row k - 64 at the most from here on)
          edgeR[i] = q;
          edgeE[i] = E;
        }
      }
    };
    int k = steps - 1;
    double x0 = rx[k], y0 = ry[k], z0 = rz[k], fQ0 = edgeR[k - 63], fE0 = edgeE[k - 63], q0 = own(k);
    double x1, y1, z1, fQ1, fE1, q1;
    for (; k >= 1; k -= 2) {
      step(k, x0, y0, z0, fQ0, fE0, q0, x1, y1, z1, fQ1, fE1, q1);
      step(k - 1, x1, y1, z1, fQ1, fE1, q1, x0, y0, z0, fQ0, fE0, q0);
    }
    if (k == 0) step(0, x0, y0, z0, fQ0, fE0, q0, x1, y1, z1, fQ1, fE1, q1);
  }
  __syncthreads();
  for (int i = lane; i < Ta; i += 64) {  // written, not added: 3 elements per sample, nothing else
    T* o = gr + (int64_t)i * g_step;
    o[0] = (T)gx[i];
    o[1] = (T)gy[i];
    o[2] = (T)gz[i];
  }
}

template <typename T>
static int launch_softdtw(int64_t B, const T* a, int Ta, int64_t ars, int64_t ass, const T* b, int Tb, int64_t brs, int64_t bss,
                          double gamma, int cost, double* value, T* g, int64_t grs, int64_t gss, void* ws, hipStream_t s) {
  const SdLayout L = sd_layout(Ta, Tb);
  const int grad = g != nullptr;
  // (value only takes the kernel the call with the gradient takes for these lengths: the same forward instructions)
  if (L.table_in_lds) {
    const size_t smem = sizeof(double) * (L.total + (grad ? L.cells : 0));
    if (int rc = dyn_lds(reinterpret_cast<const void*>(&softdtw_kernel<T, true>), smem)) return rc;
    hipLaunchKernelGGL((softdtw_kernel<T, true>), dim3((unsigned)B), dim3(64), smem, s, a, Ta, ars, ass, b, Tb, brs, bss, gamma, cost,
                       value, g, grs, gss, static_cast<double*>(nullptr), grad);
  } else {
    const size_t smem = sizeof(double) * L.total;
    if (int rc = dyn_lds(reinterpret_cast<const void*>(&softdtw_kernel<T, false>), smem)) return rc;
    hipLaunchKernelGGL((softdtw_kernel<T, false>), dim3((unsigned)B), dim3(64), smem, s, a, Ta, ars, ass, b, Tb, brs, bss, gamma, cost,
                       value, g, grs, gss, static_cast<double*>(ws), grad);
  }
  KR_HIP(hipGetLastError());
  return KR_OK;
}

}  // namespace kr

using namespace kr;

#define KR_SD_ARG(cond, msg) \
  if (cond) {                \
    set_error(msg);          \
    return KR_E_ARG;         \
  }

extern "C" size_t kr_softdtw_ws_bytes(int64_t B, int64_t Ta, int64_t Tb, int need_grad) {
  if (B < 1 || Ta < 1 || Tb < 1 || !need_grad || Ta > KR_SOFTDTW_MAX_LEN || Tb > KR_SOFTDTW_MAX_LEN) return 0;
  if (sd_layout((int)Ta, (int)Tb).table_in_lds) return 0;
  return (size_t)B * sd_table_doubles_ws((int)Ta, (int)Tb) * sizeof(double);  // (a multiple of 512)
}

extern "C" int kr_softdtw_batch(kr_handle* h, int64_t B, const void* a, int64_t Ta, int64_t a_rod_stride, int64_t a_step_stride,
                                const void* b, int64_t Tb, int64_t b_rod_stride, int64_t b_step_stride, double gamma, int cost,
                                double* value, void* g_a, int64_t g_rod_stride, int64_t g_step_stride, void* ws, int dtype,
                                void* stream) {
  KR_SD_ARG(!h, "null handle");
  KR_SD_ARG(!a || !b || !value, "kr_softdtw_batch: null pointer argument");
  KR_SD_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_SD_ARG(B < 1, "kr_softdtw_batch: B < 1");
  KR_SD_ARG(Ta < 1 || Tb < 1, "kr_softdtw_batch: Ta and Tb must be >= 1");
  KR_SD_ARG(a_rod_stride < 0 || a_step_stride < 0 || b_rod_stride < 0 || b_step_stride < 0,
            "kr_softdtw_batch: the strides of a and b must be >= 0");
  KR_SD_ARG(g_a && (g_rod_stride <= 0 || g_step_stride <= 0), "kr_softdtw_batch: the strides of g_a must be > 0");
  KR_SD_ARG(!(std::isfinite(gamma) && gamma > 0.0), "kr_softdtw_batch: gamma must be finite and > 0");
  KR_SD_ARG(cost != 0 && cost != 1, "kr_softdtw_batch: cost must be 0 (L1) or 1 (squared Euclidean)");
  if (Ta > KR_SOFTDTW_MAX_LEN || Tb > KR_SOFTDTW_MAX_LEN || B > 0x7FFFFFFFll) {
    set_error("kr_softdtw_batch: sequences of " + std::to_string(Ta) + " and " + std::to_string(Tb) + " samples: at most " +
              std::to_string(KR_SOFTDTW_MAX_LEN) + " samples per sequence are served (and at most 2^31 - 1 rods)");
    return KR_E_UNSUPPORTED;
  }
  KR_SD_ARG(!ws && kr_softdtw_ws_bytes(B, Ta, Tb, g_a != nullptr) != 0, "kr_softdtw_batch: ws is NULL, kr_softdtw_ws_bytes is not 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  return dtype == KR_F32
             ? launch_softdtw<float>(B, (const float*)a, (int)Ta, a_rod_stride, a_step_stride, (const float*)b, (int)Tb, b_rod_stride,
                                     b_step_stride, gamma, cost, value, (float*)g_a, g_rod_stride, g_step_stride, ws, s)
             : launch_softdtw<double>(B, (const double*)a, (int)Ta, a_rod_stride, a_step_stride, (const double*)b, (int)Tb,
                                      b_rod_stride, b_step_stride, gamma, cost, value, (double*)g_a, g_rod_stride, g_step_stride, ws, s);
}
