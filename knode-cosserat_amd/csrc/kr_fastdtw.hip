// kr_fastdtw.hip - FastDTW (radius r, L1 point distance) per rod on the device: the metric the reference's drivers print
// (physics_multitrain.py:211-213, physics_train.py:159), as krod_eval._fastdtw states it - distance and, optionally, the
// level-0 warp path, bit for bit.  All arithmetic fp64; T is the element type of the inputs.
//
//   fastdtw_kernel   one wavefront per rod.
//     stage     both sequences into the LDS (fp64, structure of arrays), a non-finite sample ends the rod with NaN;
//               then the pyramid: level l + 1 = pairwise means of level l, lengths Ta >> l, Tb >> l, all levels kept.
//     per level, deepest first: a DTW restricted to one column interval [lo, hi] per row (the window of
//               krod_eval._expand_window is exactly that), swept like kr_score.hip's dtw_kernel - columns in stripes of
//               64, lane l owns column 64 s + l and fills row r0 + k - l at step k, left neighbour by one DPP wave shift -
//               over the rows r0 .. r1 that have a cell in the stripe only, and with three changes: a cell outside its
//               row's interval is +inf, the predecessor is the FIRST minimum in the
//               order up, left, diagonal (two bits), and a lane collects the bits of 16 rows in one register and stores
//               them once (LDS, or the caller's workspace when the table of level 0 does not fit).
//               Then lane 0 walks the pointers back from the last cell - at most n + m - 1 steps, only "left" in row 0 and
//               only "up" in column 0 whatever the bits say - and leaves the first and last column of every row; the
//               next finer level's intervals follow from them in parallel: rows 2 c and 2 c + 1 get
//               [2 (jmin[c - r] - r), 2 (jmax[c + r] + r) + 1], clipped (the path is monotone, so the extremes over the
//               rows within r of c are those of the outermost rows).
//     level 0   the distance is the last cell's; the walk back runs only when the path is asked for.
#include "kr_internal.hpp"

namespace kr {

constexpr int FD_WAVE_SHR1 = 0x138;  // DPP wave_shr:1 - lane l reads lane l - 1, lane 0 keeps `old`
constexpr int FD_PAD = 64;           // rows a lane may read before the first / after the last row of a level
constexpr int FD_MAX_LEVELS = 16;
constexpr size_t FD_LDS_WITH_TABLE = 64 * 1024;  // the back-pointer table stays in the LDS while everything fits this

// value of lane l - 1; lane 0 receives its own `first`
__device__ __forceinline__ double fd_from_lane_below(double v, double first) {
  const long long b = __double_as_longlong(v), f = __double_as_longlong(first);
  const int lo = __builtin_amdgcn_update_dpp((int)(f & 0xFFFFFFFFll), (int)(b & 0xFFFFFFFFll), FD_WAVE_SHR1, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp((int)(f >> 32), (int)(b >> 32), FD_WAVE_SHR1, 0xF, 0xF, false);
  return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// samples of all levels of a sequence of T0 samples: T0 + T0 / 2 + ... < 2 T0
__host__ __device__ constexpr int fd_pyramid(int T0) { return 2 * T0; }
// deepest level: the first whose shorter sequence has fewer than r + 2 samples
__host__ __device__ inline int fd_levels(int Ta, int Tb, int r) {
  int l = 0;
  while (l + 1 < FD_MAX_LEVELS && (Ta >> l) >= r + 2 && (Tb >> l) >= r + 2) ++l;
  return l;
}
// back-pointer words (one per lane and 16 rows of a stripe) of the level-0 table, the largest
__host__ __device__ inline size_t fd_table_words(int Ta, int Tb) {
  return (size_t)((Tb + 63) >> 6) * (size_t)((Ta + 15) >> 4) * 64;
}

// LDS of one rod, in this order (sizes in bytes, every block a multiple of 8)
struct FdLayout {
  size_t a, b, edge, win, ext, walk, table, total;
  bool table_in_lds;
};
__host__ __device__ inline FdLayout fd_layout(int Ta, int Tb) {
  FdLayout L;
  size_t at = 0;
  L.a = at;     at += sizeof(double) * 3 * (size_t)(fd_pyramid(Ta) + 2 * FD_PAD);  // x, y, z of a, zero pads at both ends
  L.b = at;     at += sizeof(double) * 3 * (size_t)fd_pyramid(Tb);                 // x, y, z of b
  L.edge = at;  at += sizeof(double) * (size_t)(Ta + FD_PAD + 1);                  // column left of the stripe, rows 0 .. Ta + 64
  L.win = at;   at += sizeof(int2) * (size_t)(Ta + 2 * FD_PAD);                    // [lo, hi] per row, empty pads at both ends
  L.ext = at;   at += sizeof(int2) * (size_t)(Ta / 2 + 1);                         // [jmin, jmax] per row of a coarse path
  L.walk = at;  at += sizeof(int2) * (size_t)(Ta + Tb);                            // the level-0 path, last cell first
  L.table = at;
  const size_t table = sizeof(uint32_t) * fd_table_words(Ta, Tb);
  L.table_in_lds = at + table <= FD_LDS_WITH_TABLE;
  L.total = L.table_in_lds ? at + table : at;
  return L;
}

// TLDS: the back-pointer table is in the LDS (fd_layout's table_in_lds), else in the rod's slice of the workspace
template <typename T, bool TLDS>
__global__ __launch_bounds__(64) void fastdtw_kernel(const T* __restrict__ a, int Ta, int64_t a_rod, int64_t a_step,
                                                     const T* __restrict__ b, int Tb, int64_t b_rod, int64_t b_step,
                                                     int radius, double* __restrict__ dist, int32_t* __restrict__ path,
                                                     int32_t* __restrict__ path_len, uint32_t* __restrict__ ws,
                                                     size_t ws_words_per_rod) {
  extern __shared__ __align__(16) unsigned char fd_lds[];
  const FdLayout L = fd_layout(Ta, Tb);
  const int a_len = fd_pyramid(Ta) + 2 * FD_PAD, b_len = fd_pyramid(Tb);
  double* ax = reinterpret_cast<double*>(fd_lds + L.a);
  double* ay = ax + a_len;
  double* az = ay + a_len;
  double* bxs = reinterpret_cast<double*>(fd_lds + L.b);
  double* bys = bxs + b_len;
  double* bzs = bys + b_len;
  double* edge = reinterpret_cast<double*>(fd_lds + L.edge);
  int2* win = reinterpret_cast<int2*>(fd_lds + L.win);
  int2* ext = reinterpret_cast<int2*>(fd_lds + L.ext);
  int2* walk = reinterpret_cast<int2*>(fd_lds + L.walk);
  const int lane = threadIdx.x;
  const int64_t rod = blockIdx.x;
  uint32_t* table = TLDS ? reinterpret_cast<uint32_t*>(fd_lds + L.table) : ws + (size_t)rod * ws_words_per_rod;
  const double inf = __builtin_inf();

  // ---- stage level 0 (fp64) and look for a sample that is not finite ----
  bool bad = false;
  {
    const T* ar = a + rod * a_rod;
    for (int i = lane; i < a_len; i += 64) {
      double x = 0.0, y = 0.0, z = 0.0;
      const int r = i - FD_PAD;
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
    }
    const T* br = b + rod * b_rod;
    for (int j = lane; j < b_len; j += 64) {
      double x = 0.0, y = 0.0, z = 0.0;
      if (j < Tb) {
        const T* s = br + (int64_t)j * b_step;
        x = (double)s[0];
        y = (double)s[1];
        z = (double)s[2];
        bad = bad || !(isfinite(x) && isfinite(y) && isfinite(z));
      }
      bxs[j] = x;
      bys[j] = y;
      bzs[j] = z;
    }
  }
  if (__any(bad)) {  // (uniform: the whole wavefront leaves)
    if (lane == 0) {
      dist[rod] = __builtin_nan("");
      if (path_len) path_len[rod] = 0;
    }
    return;
  }
  __syncthreads();

  // ---- the pyramid: level l at offset Ta + Ta / 2 + ... (l terms), lengths Ta >> l ----
  const int deepest = fd_levels(Ta, Tb, radius);
  {
    int oa = 0, ob = 0;
    for (int l = 0; l < deepest; ++l) {
      const int n = Ta >> l, m = Tb >> l;
      double* sx = ax + FD_PAD + oa;
      double* sy = ay + FD_PAD + oa;
      double* sz = az + FD_PAD + oa;
      for (int i = lane; i < (n >> 1); i += 64) {
        sx[n + i] = (sx[2 * i] + sx[2 * i + 1]) / 2.0;
        sy[n + i] = (sy[2 * i] + sy[2 * i + 1]) / 2.0;
        sz[n + i] = (sz[2 * i] + sz[2 * i + 1]) / 2.0;
      }
      for (int j = lane; j < (m >> 1); j += 64) {
        bxs[ob + m + j] = (bxs[ob + 2 * j] + bxs[ob + 2 * j + 1]) / 2.0;
        bys[ob + m + j] = (bys[ob + 2 * j] + bys[ob + 2 * j + 1]) / 2.0;
        bzs[ob + m + j] = (bzs[ob + 2 * j] + bzs[ob + 2 * j + 1]) / 2.0;
      }
      oa += n;
      ob += m;
      __syncthreads();
    }
  }

  double result = inf;
  for (int l = deepest; l >= 0; --l) {
    const int n = Ta >> l, m = Tb >> l;
    int oa = 0, ob = 0;
    for (int k = 0; k < l; ++k) {
      oa += Ta >> k;
      ob += Tb >> k;
    }
    // ---- the window of this level: every cell on the deepest level, else from the coarse path's extremes ----
    for (int i = lane; i < n + 2 * FD_PAD; i += 64) {
      const int fi = i - FD_PAD;
      int2 w = make_int2(1, 0);  // (empty: rows outside the level)
      if ((unsigned)fi < (unsigned)n) {
        if (l == deepest) {
          w = make_int2(0, m - 1);
        } else {
          const int cn = n >> 1, c = fi >> 1;  // (c == cn: the dropped last sample's row, reached through the radius)
          const int lo = ext[max(c - radius, 0)].x - radius;
          const int hi = ext[min(c + radius, cn - 1)].y + radius;
          w = make_int2(max(2 * lo, 0), min(2 * hi + 1, m - 1));
        }
      }
      win[i] = w;
    }
    for (int i = lane; i < n + FD_PAD + 1; i += 64) edge[i] = inf;
    __syncthreads();

    // ---- the banded table, stripe by stripe ----
    const int stripes = (m + 63) >> 6;
    const int blocks = (n + 15) >> 4;
    int prev_r0 = 0;
    for (int s = 0; s < stripes; ++s) {
      const int c0 = s * 64;
      const int j = c0 + lane;
      const bool col = j < m;
      // the rows that have a cell in this stripe: from the first whose interval reaches column c0 to the last whose
      // interval starts at or before column c0 + 63 (the intervals move right with the row, never left)
      int r0 = n, r1 = -1;
      for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const int2 wi = win[FD_PAD + i];  // (empty beyond the last row)
        const unsigned long long reach = __ballot(i < n && wi.y >= c0), start = __ballot(i < n && wi.x <= c0 + 63);
        if (r0 == n && reach) r0 = base + __builtin_ctzll(reach);
        if (start) r1 = base + 63 - __builtin_clzll(start);
      }
      const int steps = (r1 - r0 + 1) + min(64, m - c0) - 1;  // (the last column of the stripe fills row r1 in the last one)
      double bx = 0.0, by = 0.0, bz = 0.0;
      if (col) {
        bx = bxs[ob + j];
        by = bys[ob + j];
        bz = bzs[ob + j];
      }
      const bool feeds = s + 1 < stripes && lane == 63;  // column 64 s + 63 is the next stripe's edge
      double D = inf;                                    // the row above the first, in every column
      // lane 0: D[r0 - 1][c0 - 1] - 0 in front of the first cell, the previous stripe's last column where that stripe had
      // the row (a row it skipped keeps an older stripe's value in `edge`: its cell there is outside the window)
      double diag = inf;
      if (lane == 0) {
        if (s == 0 && r0 == 0) diag = 0.0;
        else if (s > 0 && r0 - 1 >= prev_r0) diag = edge[r0 - 1];
      }
      prev_r0 = r0;
      uint32_t bits = 0;
      const double* rx = ax + (FD_PAD + oa + r0 - lane);  // row r0 + k - lane of step k at rx[k]
      const double* ry = ay + (FD_PAD + oa + r0 - lane);
      const double* rz = az + (FD_PAD + oa + r0 - lane);
      const int2* rw = win + (FD_PAD + r0 - lane);
      const double* re = edge + r0;
      uint32_t* tcol = table + (size_t)s * blocks * 64 + lane;
      // one step: the operands of step k (c*, first, w) were fetched during step k - 1, those of step k + 1 are fetched here
      auto step = [&](int k, double cx, double cy, double cz, double first, int2 w, double& nx, double& ny, double& nz,
                      double& nfirst, int2& nw) {
        nx = rx[k + 1];
        ny = ry[k + 1];
        nz = rz[k + 1];
        nfirst = re[k + 1];
        nw = rw[k + 1];
        const int i = r0 + k - lane;
        const bool row = i >= r0 && i <= r1;
        const bool act = col && j >= w.x && j <= w.y;  // (rows outside r0 .. r1 and the pads have no cell here)
        const double left = fd_from_lane_below(D, first);
        const double cost = (fabs(cx - bx) + fabs(cy - by)) + fabs(cz - bz);
        // the first minimum in the order up, left, diagonal
        const bool up_wins = D <= left && D <= diag;
        const bool left_wins = left <= diag;
        const double pred = up_wins ? D : (left_wins ? left : diag);
        const uint32_t code = up_wins ? 0u : (left_wins ? 1u : 2u);
        const double d = pred + cost;
        diag = left;
        D = act ? d : inf;
        const int sub = i & 15;
        bits = (sub == 0 ? 0u : bits) | ((act ? code : 0u) << (2 * sub));
        if (row && col && (sub == 15 || i == r1)) tcol[(size_t)(i >> 4) * 64] = bits;
        if (feeds && row) edge[i] = D;  // (row r0 + k - 63: lane 0 read it 64 steps ago)
        if (act && i == n - 1 && j == m - 1) result = d;
      };
      double x0 = rx[0], y0 = ry[0], z0 = rz[0], f0 = re[0], x1, y1, z1, f1;
      int2 w0 = rw[0], w1;
      int k = 0;
      for (; k + 1 < steps; k += 2) {
        step(k, x0, y0, z0, f0, w0, x1, y1, z1, f1, w1);
        step(k + 1, x1, y1, z1, f1, w1, x0, y0, z0, f0, w0);
      }
      if (k < steps) step(k, x0, y0, z0, f0, w0, x1, y1, z1, f1, w1);
    }
    __syncthreads();

    // ---- walk back: lane 0, at most n + m - 1 cells ----
    const bool want_walk = l > 0 || path != nullptr;
    int count = 0;
    if (want_walk && lane == 0) {
      int i = n - 1, j = m - 1;
      const int cap = n + m - 1;
      int last_row = -1;
      for (int t = 0; t < cap; ++t) {
        if (l > 0) {
          if (i != last_row) ext[i].y = j;  // (first visit of a row: its largest column)
          ext[i].x = j;
          last_row = i;
        } else {
          walk[t] = make_int2(i, j);
        }
        ++count;
        if (i == 0 && j == 0) break;
        const uint32_t word = table[((size_t)(j >> 6) * blocks + (size_t)(i >> 4)) * 64 + (j & 63)];
        uint32_t code = (word >> (2 * (i & 15))) & 3u;
        if (i == 0) code = 1u;       // row 0: left only
        else if (j == 0) code = 0u;  // column 0: up only
        if (code != 1u) --i;
        if (code != 0u) --j;
      }
    }
    __syncthreads();
    if (l == 0 && path != nullptr) {
      count = __shfl(count, 0);
      int32_t* out = path + rod * 2 * ((int64_t)Ta + Tb - 1);
      for (int p = lane; p < count; p += 64) {
        const int2 cell = walk[count - 1 - p];
        out[2 * p] = cell.x;
        out[2 * p + 1] = cell.y;
      }
      if (lane == 0) path_len[rod] = count;
    }
  }
  if (lane == ((Tb - 1) & 63)) dist[rod] = result;  // (the owner of the last column saw the last cell)
}

template <typename T>
static int launch_fastdtw(int64_t B, const T* a, int Ta, int64_t ars, int64_t ass, const T* b, int Tb, int64_t brs, int64_t bss,
                          int radius, double* dist, int32_t* path, int32_t* path_len, void* ws, hipStream_t s) {
  const FdLayout L = fd_layout(Ta, Tb);
  if (L.table_in_lds) {
    if (int rc = dyn_lds(reinterpret_cast<const void*>(&fastdtw_kernel<T, true>), L.total)) return rc;
    hipLaunchKernelGGL((fastdtw_kernel<T, true>), dim3((unsigned)B), dim3(64), L.total, s, a, Ta, ars, ass, b, Tb, brs, bss, radius,
                       dist, path, path_len, static_cast<uint32_t*>(nullptr), (size_t)0);
  } else {
    if (int rc = dyn_lds(reinterpret_cast<const void*>(&fastdtw_kernel<T, false>), L.total)) return rc;
    hipLaunchKernelGGL((fastdtw_kernel<T, false>), dim3((unsigned)B), dim3(64), L.total, s, a, Ta, ars, ass, b, Tb, brs, bss, radius,
                       dist, path, path_len, static_cast<uint32_t*>(ws), (fd_table_words(Ta, Tb) + 3) / 4 * 4);
  }
  KR_HIP(hipGetLastError());
  return KR_OK;
}

}  // namespace kr

using namespace kr;

#define KR_FD_ARG(cond, msg) \
  if (cond) {                \
    set_error(msg);          \
    return KR_E_ARG;         \
  }

extern "C" size_t kr_fastdtw_ws_bytes(int64_t B, int64_t Ta, int64_t Tb, int radius) {
  if (B < 1 || Ta < 1 || Tb < 1 || radius < 1 || Ta > KR_FASTDTW_MAX_LEN || Tb > KR_FASTDTW_MAX_LEN) return 0;
  if (fd_layout((int)Ta, (int)Tb).table_in_lds) return 0;
  return (size_t)B * ((fd_table_words((int)Ta, (int)Tb) + 3) / 4 * 4) * sizeof(uint32_t);
}

extern "C" int kr_fastdtw_batch(kr_handle* h, int64_t B, const void* a, int64_t Ta, int64_t a_rod_stride, int64_t a_step_stride,
                                const void* b, int64_t Tb, int64_t b_rod_stride, int64_t b_step_stride, int radius, double* dist,
                                int32_t* path, int32_t* path_len, void* ws, int dtype, void* stream) {
  KR_FD_ARG(!h, "null handle");
  KR_FD_ARG(!a || !b || !dist, "kr_fastdtw_batch: null pointer argument");
  KR_FD_ARG(dtype != KR_F32 && dtype != KR_F64, "dtype must be KR_F32 or KR_F64");
  KR_FD_ARG(B < 1, "kr_fastdtw_batch: B < 1");
  KR_FD_ARG(Ta < 1 || Tb < 1, "kr_fastdtw_batch: Ta and Tb must be >= 1");
  KR_FD_ARG(a_rod_stride < 0 || a_step_stride < 0 || b_rod_stride < 0 || b_step_stride < 0,
            "kr_fastdtw_batch: strides must be >= 0");
  KR_FD_ARG(radius < 1, "kr_fastdtw_batch: radius must be >= 1 (radius 0 leaves rows without a window)");
  KR_FD_ARG((path == nullptr) != (path_len == nullptr), "kr_fastdtw_batch: path and path_len go together (both or neither)");
  if (radius > KR_FASTDTW_MAX_RADIUS || Ta > KR_FASTDTW_MAX_LEN || Tb > KR_FASTDTW_MAX_LEN || B > 0x7FFFFFFFll) {
    set_error("kr_fastdtw_batch: sequences of " + std::to_string(Ta) + " and " + std::to_string(Tb) + " samples, radius " +
              std::to_string(radius) + ": at most " + std::to_string(KR_FASTDTW_MAX_LEN) + " samples per sequence and radius " +
              std::to_string(KR_FASTDTW_MAX_RADIUS) + " are served (and at most 2^31 - 1 rods)");
    return KR_E_UNSUPPORTED;
  }
  KR_FD_ARG(!ws && kr_fastdtw_ws_bytes(B, Ta, Tb, radius) != 0, "kr_fastdtw_batch: ws is NULL, kr_fastdtw_ws_bytes is not 0");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  return dtype == KR_F32
             ? launch_fastdtw<float>(B, (const float*)a, (int)Ta, a_rod_stride, a_step_stride, (const float*)b, (int)Tb, b_rod_stride,
                                     b_step_stride, radius, dist, path, path_len, ws, s)
             : launch_fastdtw<double>(B, (const double*)a, (int)Ta, a_rod_stride, a_step_stride, (const double*)b, (int)Tb,
                                      b_rod_stride, b_step_stride, radius, dist, path, path_len, ws, s);
}
