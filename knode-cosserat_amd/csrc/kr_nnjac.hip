// kr_nnjac.hip - the input Jacobian of the residual MLP, Jn[25][28] = dNN/dx, on Q rows at once.
//
//   kr_mlp_input_jacobian_batch   x[Q][28] -> jac[Q][25][28]        (the network of cosserat_ode.py:90-112, nn_input_history = 0)
//
// The step adjoint with the network on needs Jn at every stored grid point of every rod: Q = B (N - 1) rows per step, a
// throughput problem that does not belong in the adjoint's serial chain.  It is the chain rule in matrix form,
//
//   one hidden layer    Jn = W2 diag(act'(a1)) W1                              a1 = W1 x + b1
//   two hidden layers   Jn = W3 diag(act'(a2)) W2 diag(act'(a1)) W1            a2 = W2 act(a1) + b2
//
// evaluated on v_mfma_f64_16x16x4_f64 with the diagonal factors folded into the B operand.  Everything is fp64: the
// pre-activations (from MlpDev<double>::Wt / b), the activation derivatives, the products.  `dtype` of the entry point is
// the element type of x and jac only.
//
// Operand maps of the instruction (lane l, f = l & 15, g = l >> 4): A holds A[row f][k g], B holds B[k g][col f], C / D
// hold rows g + 4 reg of column f - NOT the f32 form's 4 g + reg.  That row map is what makes the three-factor chain
// cheap: register `reg` of the tile t of a product is row 16 t + 4 reg + g, which is exactly what the B operand of k-step
// 4 t + reg of the next product wants, so the intermediate H2 x 28 matrix goes from accumulator to operand in place.
//
// Mapping.  Weights live in LDS per workgroup (4 wavefronts), zero-padded: the k index (hidden unit) is the slow one, so
// both operands are read as 16 consecutive doubles per quarter-wave.
//   jac2 (28 -> H -> 25, H <= 512): the hidden layer is cut into chunks of 64 units (W1, W2 of 512 units are 256 KB in
//        fp64, the LDS holds 160); a workgroup carries 16 rows (4 per wavefront, 16 accumulator tiles each) through all
//        chunks, so a chunk read from L2 is used 16 times and every MFMA operand load 4 times.  46 KB of LDS; 328 registers
//        (VGPRs and AGPRs, the 16 accumulator tiles among them): one workgroup per CU, a wavefront per SIMD with 16
//        independent MFMA chains each.
//   jac3 (28 -> H1 -> H2 -> 25, H1, H2 <= 64): all three matrices stay in LDS for the whole launch (74 KB, 2 workgroups
//        per CU by LDS and by registers); a wavefront takes one row at a time.
// A row's arithmetic does not depend on where in the batch it sits: the same row gives the same bits in any call.
// A row with a value of x that is not finite (NaN or an infinity) comes back NaN in every entry.
#include "kr_internal.hpp"

namespace kr {

constexpr int NJ_IN = 28, NJ_OUT = 25;
constexpr int NJ_WAVES = 4;
constexpr int NJ_KC = 64;    // jac2: hidden units per LDS chunk; jac3: the padded hidden width
constexpr int NJ_ROWS = 4;   // jac2: rows per wavefront
constexpr int NJ_S1 = 33;    // LDS stride of a W1 row (k-major, 32 input columns + 1: the forward pass reads it down a column)
constexpr int NJ_JAC = NJ_OUT * NJ_IN;

typedef double nj_d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ nj_d4 nj_mfma(double a, double b, nj_d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// activation and its derivative at the pre-activation a, both to a few ulps RELATIVE (1 - tanh^2 would lose the
// derivative's digits for |a| > 1)
__device__ __forceinline__ void nj_act(int code, double a, double& h, double& d) {
  switch (code) {
    case KR_ACT_TANH: {
      const double e = exp(-2.0 * fabs(a)), r = 1.0 / (1.0 + e);
      h = copysign((1.0 - e) * r, a);
      d = 4.0 * e * r * r;
      break;
    }
    case KR_ACT_SOFTPLUS: {
      const double e = exp(-fabs(a)), r = 1.0 / (1.0 + e);
      h = log1p(e) + fmax(a, 0.0);
      d = a >= 0.0 ? r : e * r;
      break;
    }
    case KR_ACT_RELU:
      h = a > 0.0 ? a : (a <= 0.0 ? 0.0 : a);
      d = a > 0.0 ? 1.0 : (a <= 0.0 ? 0.0 : a);  // (a NaN stays one)
      break;
    case KR_ACT_ELU:
      h = a > 0.0 ? a : expm1(a);
      d = a > 0.0 ? 1.0 : exp(a);
      break;
    default:
      h = a;
      d = 1.0;
  }
}

template <typename T>
struct NjArgs {
  int64_t Q;
  const T* x;        // row q at x[q * x_stride .. + 28]
  int64_t x_stride;
  T* jac;            // [Q][700]: transposed ? [28][25] (a column contiguous: what the adjoint's lanes read) : [25][28]
  int transposed;
};

// one accumulator tile to memory: tile (t, c) holds rows 16 t + g + 4 reg of columns 16 c + f
template <typename T>
__device__ __forceinline__ void nj_store(const NjArgs<T>& A, int64_t q, int t, int c, int lane, const nj_d4& acc, bool poison) {
  const int col = 16 * c + (lane & 15);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  T* out = A.jac + q * NJ_JAC;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int o = 16 * t + (lane >> 4) + 4 * r;
    if (o < NJ_OUT && col < NJ_IN) out[A.transposed ? col * NJ_OUT + o : o * NJ_IN + col] = poison ? (T)nan : (T)acc[r];
  }
}

constexpr int NJ2_LDS = NJ_KC * NJ_S1 + NJ_KC * 32 + NJ_KC + NJ_WAVES * NJ_ROWS * (32 + NJ_KC);  // doubles

template <typename T>
__global__ __launch_bounds__(64 * NJ_WAVES) void mlp_input_jacobian_kernel(const MlpDev<double> M, const NjArgs<T> A) {
  __shared__ double lds[NJ2_LDS];
  double* W1s = lds;                       // [k][NJ_S1]: W1[k0 + k][i]
  double* W2s = W1s + NJ_KC * NJ_S1;       // [k][32]:    W2[o][k0 + k]
  double* b1s = W2s + NJ_KC * 32;          // [k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* xs = b1s + NJ_KC + wave * NJ_ROWS * (32 + NJ_KC);  // [r][32]
  double* ds = xs + NJ_ROWS * 32;                            // [r][NJ_KC]: act'(a1) of the chunk
  const int H = M.dims[1], act = M.acts[0];
  const int op1 = M.out_pad[0], op2 = M.out_pad[1];
  const double* __restrict__ Wt1 = M.Wt[0];
  const double* __restrict__ Wt2 = M.Wt[1];
  const double* __restrict__ bb1 = M.b[0];
  const int f = lane & 15, g = lane >> 4;
  constexpr int WG_ROWS = NJ_WAVES * NJ_ROWS;

  for (int64_t base = (int64_t)blockIdx.x * WG_ROWS; base < A.Q; base += (int64_t)gridDim.x * WG_ROWS) {
    const int64_t q0 = base + wave * NJ_ROWS;
    bool poison[NJ_ROWS];  // a row with a value that is not finite: every entry NaN (an infinity alone would pass relu' / elu')
#pragma unroll
    for (int r = 0; r < NJ_ROWS; ++r) {
      const int64_t q = q0 + r < A.Q ? q0 + r : A.Q - 1;  // (a row past the end repeats the last one and is not stored)
      const double xv = lane < NJ_IN ? (double)A.x[q * A.x_stride + lane] : 0.0;
      if (lane < 32) xs[r * 32 + lane] = xv;
      poison[r] = __any(!isfinite(xv));
    }
    nj_d4 acc[NJ_ROWS][2][2];
#pragma unroll
    for (int r = 0; r < NJ_ROWS; ++r)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][t][c] = nj_d4{0.0, 0.0, 0.0, 0.0};

    for (int k0 = 0; k0 < H; k0 += NJ_KC) {
      __syncthreads();  // the chunk before is used up (and, first time round, nothing)
      for (int e = tid; e < NJ_KC * 32; e += 64 * NJ_WAVES) {
        const int k = e % NJ_KC, i = e / NJ_KC;
        W1s[k * NJ_S1 + i] = (i < NJ_IN && k0 + k < H) ? Wt1[(size_t)i * op1 + k0 + k] : 0.0;
        const int k2 = e >> 5, o = e & 31;
        W2s[e] = (o < NJ_OUT && k0 + k2 < H) ? Wt2[(size_t)(k0 + k2) * op2 + o] : 0.0;
      }
      if (tid < NJ_KC) b1s[tid] = k0 + tid < H ? bb1[k0 + tid] : 0.0;
      __syncthreads();
      // the chunk's pre-activations of this wavefront's rows: lane = hidden unit
#pragma unroll
      for (int r = 0; r < NJ_ROWS; ++r) {
        double a = b1s[lane];
#pragma unroll
        for (int i = 0; i < NJ_IN; ++i) a = fma(W1s[lane * NJ_S1 + i], xs[r * 32 + i], a);
        double h, d;
        nj_act(act, a, h, d);
        ds[r * NJ_KC + lane] = d;
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll 4
      for (int s = 0; s < NJ_KC / 4; ++s) {
        const int kk = 4 * s + g;
        const double a0 = W2s[kk * 32 + f], a1 = W2s[kk * 32 + 16 + f];
        const double b0 = W1s[kk * NJ_S1 + f], b1 = W1s[kk * NJ_S1 + 16 + f];
#pragma unroll
        for (int r = 0; r < NJ_ROWS; ++r) {
          const double dv = ds[r * NJ_KC + kk];
          const double e0 = b0 * dv, e1 = b1 * dv;
          acc[r][0][0] = nj_mfma(a0, e0, acc[r][0][0]);
          acc[r][0][1] = nj_mfma(a0, e1, acc[r][0][1]);
          acc[r][1][0] = nj_mfma(a1, e0, acc[r][1][0]);
          acc[r][1][1] = nj_mfma(a1, e1, acc[r][1][1]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < NJ_ROWS; ++r)
      if (q0 + r < A.Q) {
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int c = 0; c < 2; ++c) nj_store(A, q0 + r, t, c, lane, acc[r][t][c], poison[r]);
      }
  }
}

constexpr int NJ3_WAVE = 32 + 3 * NJ_KC;  // doubles of a wavefront's own LDS: x, act(a1), act'(a1), act'(a2)
constexpr int NJ3_LDS = NJ_KC * NJ_S1 + NJ_KC * NJ_KC + NJ_KC * 32 + 2 * NJ_KC + NJ_WAVES * NJ3_WAVE;

template <typename T>
__global__ __launch_bounds__(64 * NJ_WAVES) void mlp_input_jacobian3_kernel(const MlpDev<double> M, const NjArgs<T> A) {
  extern __shared__ double lds3[];
  double* W1s = lds3;                      // [h1][NJ_S1]: W1[h1][i]
  double* W2s = W1s + NJ_KC * NJ_S1;       // [h1][64]:    W2[h2][h1]
  double* W3s = W2s + NJ_KC * NJ_KC;       // [h2][32]:    W3[o][h2]
  double* b1s = W3s + NJ_KC * 32;
  double* b2s = b1s + NJ_KC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* xs = b2s + NJ_KC + wave * NJ3_WAVE;
  double* h1s = xs + 32;
  double* d1s = h1s + NJ_KC;
  double* d2s = d1s + NJ_KC;
  const int H1 = M.dims[1], H2 = M.dims[2], act1 = M.acts[0], act2 = M.acts[1];
  const int op1 = M.out_pad[0], op2 = M.out_pad[1], op3 = M.out_pad[2];
  const double* __restrict__ Wt1 = M.Wt[0];
  const double* __restrict__ Wt2 = M.Wt[1];
  const double* __restrict__ Wt3 = M.Wt[2];
  const int f = lane & 15, g = lane >> 4;

  for (int e = tid; e < NJ_KC * NJ_KC; e += 64 * NJ_WAVES) {
    const int k = e >> 6, c = e & 63;  // W2s: k = h1, c = h2
    W2s[e] = (k < H1 && c < H2) ? Wt2[(size_t)k * op2 + c] : 0.0;
    if (e < NJ_KC * 32) {
      const int k1 = e % NJ_KC, i = e / NJ_KC;
      W1s[k1 * NJ_S1 + i] = (i < NJ_IN && k1 < H1) ? Wt1[(size_t)i * op1 + k1] : 0.0;
      const int k3 = e >> 5, o = e & 31;
      W3s[e] = (o < NJ_OUT && k3 < H2) ? Wt3[(size_t)k3 * op3 + o] : 0.0;
    }
  }
  if (tid < NJ_KC) {
    b1s[tid] = tid < H1 ? M.b[0][tid] : 0.0;
    b2s[tid] = tid < H2 ? M.b[1][tid] : 0.0;
  }
  __syncthreads();

  for (int64_t q = (int64_t)blockIdx.x * NJ_WAVES + wave; q < A.Q; q += (int64_t)gridDim.x * NJ_WAVES) {
    const double xv = lane < NJ_IN ? (double)A.x[q * A.x_stride + lane] : 0.0;
    if (lane < 32) xs[lane] = xv;
    const bool poison = __any(!isfinite(xv));  // (every entry of such a row is NaN: an infinity alone would pass relu' / elu')
    __builtin_amdgcn_wave_barrier();
    {  // forward: lane = unit.  A padded unit has zero weights in the NEXT matrix, whatever its activation is
      double a = b1s[lane];
#pragma unroll
      for (int i = 0; i < NJ_IN; ++i) a = fma(W1s[lane * NJ_S1 + i], xs[i], a);
      double h, d;
      nj_act(act1, a, h, d);
      h1s[lane] = h;
      d1s[lane] = d;
      __builtin_amdgcn_wave_barrier();
      double a2 = b2s[lane];
#pragma unroll 8
      for (int k = 0; k < NJ_KC; ++k) a2 = fma(W2s[k * NJ_KC + lane], h1s[k], a2);
      nj_act(act2, a2, h, d);
      d2s[lane] = d;
      __builtin_amdgcn_wave_barrier();
    }
    // P = W2 diag(d1) W1: [64][32] in 4 x 2 tiles
    nj_d4 p[4][2];
#pragma unroll
    for (int t = 0; t < 4; ++t) p[t][0] = p[t][1] = nj_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int s = 0; s < NJ_KC / 4; ++s) {
      const int kk = 4 * s + g;
      const double dv = d1s[kk];
      const double e0 = W1s[kk * NJ_S1 + f] * dv, e1 = W1s[kk * NJ_S1 + 16 + f] * dv;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double a = W2s[kk * NJ_KC + 16 * t + f];
        p[t][0] = nj_mfma(a, e0, p[t][0]);
        p[t][1] = nj_mfma(a, e1, p[t][1]);
      }
    }
    // Jn = W3 diag(d2) P: register `reg` of tile t of P is row 4 (4 t + reg) + g - the B operand of k-step 4 t + reg
    nj_d4 j[2][2];
    j[0][0] = j[0][1] = j[1][0] = j[1][1] = nj_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < NJ_KC / 4; ++s) {
      const int kk = 4 * s + g;
      const double dv = d2s[kk];
      const double e0 = p[s >> 2][0][s & 3] * dv, e1 = p[s >> 2][1][s & 3] * dv;
      const double a0 = W3s[kk * 32 + f], a1 = W3s[kk * 32 + 16 + f];
      j[0][0] = nj_mfma(a0, e0, j[0][0]);
      j[0][1] = nj_mfma(a0, e1, j[0][1]);
      j[1][0] = nj_mfma(a1, e0, j[1][0]);
      j[1][1] = nj_mfma(a1, e1, j[1][1]);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int c = 0; c < 2; ++c) nj_store(A, q, t, c, lane, j[t][c], poison);
    __builtin_amdgcn_wave_barrier();  // (the row's LDS is rewritten by the next one)
  }
}

// The shapes served, and the refusals that come before anything is launched
int nnjac_check(const kr_handle* h, const char* api) {
  if (h->mlp_d.n_layers <= 0) {
    set_error(std::string(api) + ": no MLP was set (kr_set_mlp)");
    return KR_E_STATE;
  }
  return nnjac_check(h->mlp_d, h->params.nn_input_history, api);
}
// (the same for a descriptor that is not the handle's: a network of a bank)
int nnjac_check(const MlpDev<double>& M, int nn_input_history, const char* api) {
  const std::string who = std::string(api) + ": ";
  auto refuse = [&](const std::string& why) {
    set_error(who + why + "; nothing falls back to another evaluator");
    return KR_E_UNSUPPORTED;
  };
  if (nn_input_history != 0) return refuse("nn_input_history = 1 (the 53-wide input) is not served");
  const int n = M.n_layers;
  if (n != 2 && n != 3) return refuse("a network of " + std::to_string(n) + " layers is not served (one or two hidden layers only)");
  if (M.dims[0] != NJ_IN || M.dims[n] != NJ_OUT) return refuse("the network must map 28 inputs to 25 outputs");
  if (n == 2 && (M.dims[1] < 1 || M.dims[1] > 512)) return refuse("one hidden layer of more than 512 units is not served");
  if (n == 3 && (M.dims[1] < 1 || M.dims[1] > NJ_KC || M.dims[2] < 1 || M.dims[2] > NJ_KC))
    return refuse("two hidden layers of more than 64 units are not served");
  if (M.acts[n - 1] != KR_ACT_NONE) return refuse("an activation on the last layer is not served");
  for (int k = 0; k < n - 1; ++k)
    if (M.acts[k] < KR_ACT_NONE || M.acts[k] > KR_ACT_ELU) return refuse("unknown activation code");
  return KR_OK;
}

// x rows (stride x_stride) -> jac rows of 700; the caller has passed nnjac_check
template <typename T>
int launch_nnjac(kr_handle* h, int64_t Q, const T* x, int64_t x_stride, T* jac, int transposed, hipStream_t s) {
  return launch_nnjac<T>(h->mlp_d, Q, x, x_stride, jac, transposed, s);
}
template <typename T>
int launch_nnjac(const MlpDev<double>& M, int64_t Q, const T* x, int64_t x_stride, T* jac, int transposed, hipStream_t s) {
  NjArgs<T> A{Q, x, x_stride, jac, transposed};
  if (M.n_layers == 2) {
    const int64_t groups = (Q + NJ_WAVES * NJ_ROWS - 1) / (NJ_WAVES * NJ_ROWS);
    const unsigned grid = (unsigned)(groups < 3072 ? groups : 3072);
    return launch(s, mlp_input_jacobian_kernel<T>, dim3(grid), dim3(64 * NJ_WAVES), 0, M, A);
  }
  const int64_t groups = (Q + NJ_WAVES - 1) / NJ_WAVES;
  const unsigned grid = (unsigned)(groups < 512 ? groups : 512);
  return launch(s, mlp_input_jacobian3_kernel<T>, dim3(grid), dim3(64 * NJ_WAVES), NJ3_LDS * sizeof(double), M, A);
}
template int launch_nnjac<float>(kr_handle*, int64_t, const float*, int64_t, float*, int, hipStream_t);
template int launch_nnjac<double>(kr_handle*, int64_t, const double*, int64_t, double*, int, hipStream_t);
template int launch_nnjac<double>(const MlpDev<double>&, int64_t, const double*, int64_t, double*, int, hipStream_t);

}  // namespace kr

using namespace kr;

extern "C" int kr_mlp_input_jacobian_batch(kr_handle* h, int64_t Q, const void* x, void* jac, int dtype, void* stream) {
  if (!h) {
    set_error("null handle");
    return KR_E_ARG;
  }
  if (dtype != KR_F32 && dtype != KR_F64) {
    set_error("dtype must be KR_F32 or KR_F64");
    return KR_E_ARG;
  }
  if (Q < 1) {
    set_error("kr_mlp_input_jacobian_batch: Q < 1");
    return KR_E_ARG;
  }
  if (!x || !jac) {
    set_error("kr_mlp_input_jacobian_batch: null pointer argument");
    return KR_E_ARG;
  }
  if (int rc = nnjac_check(h, "kr_mlp_input_jacobian_batch")) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = order_stream(h, s)) return rc;
  if (dtype == KR_F32) return launch_nnjac<float>(h, Q, (const float*)x, NJ_IN, (float*)jac, 0, s);
  return launch_nnjac<double>(h, Q, (const double*)x, NJ_IN, (double*)jac, 0, s);
}
