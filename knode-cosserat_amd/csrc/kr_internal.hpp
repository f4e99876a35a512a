// kr_internal.hpp - host-side handle and launch declarations shared by the
// translation units of libknode_rod.so.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/knode_rod.h"
#include "rod_device.hpp"

namespace kr {

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what);
#define KR_HIP(expr)                                   \
  do {                                                 \
    hipError_t _e = (expr);                            \
    if (_e != hipSuccess) return kr::hip_fail(_e, #expr); \
  } while (0)

// Packed MLP on the device: per layer a transposed weight matrix
// Wt[in][out_pad] (out_pad = out rounded up to 16) and bias b[out_pad], in
// both precisions, so that for a fixed input unit the weights of 16 output
// units are contiguous and can be fetched with scalar loads.
template <typename T>
struct MlpDev {
  int n_layers;
  int dims[KR_MAX_LAYERS + 1];
  int out_pad[KR_MAX_LAYERS];
  int acts[KR_MAX_LAYERS];
  const T* Wt[KR_MAX_LAYERS];
  const T* b[KR_MAX_LAYERS];
  int max_dim;  // widest activation vector (incl. input and output)
  // matrix-core form (mlp_mfma.hpp): weights / biases pre-packed in MFMA fragment order
  const T* wfrag[KR_MAX_LAYERS];
  const T* bfrag[KR_MAX_LAYERS];
  int ksteps[KR_MAX_LAYERS];   // k-steps (of 4 inputs) per output tile
  int otiles[KR_MAX_LAYERS];   // 16-unit output tiles (hidden layers: a multiple of 4)
  int mfma_ok;                 // the network has a shape the matrix-core evaluator supports
  // Jacobian-vector-product chain of the multiple-shooting sweeps (mlp_jvp.hpp): bf16 A fragments
  // [tile][k-step of 32][lane][8], shared by both precisions
  const void* jfrag[KR_MAX_LAYERS];
  int jksteps[KR_MAX_LAYERS];
  // base chain of the same evaluator (v_mfma_f64_4x4x4_4b for both precisions): fp32 A fragments
  // [tile][k-group of 16 inputs][lane][4 k-steps], biases [tile][lane] in that instruction's D layout
  const float* wq[KR_MAX_LAYERS];
  const float* bq[KR_MAX_LAYERS];
  int kgroups[KR_MAX_LAYERS];
  int jvp_ok;                  // shape served by mlp_jvp.hpp (second hidden layer <= 64 (MJ_ACT_SLOTS - 1) = 192 units)
  // fp32 base chain of the same evaluator for in -> H1 <= 64 -> H2 <= 64 -> 25 (mlp_jvp_tile3f, v_mfma_f32_4x4x1_16B): lane l
  // owns row l of the weight matrix, [k-group of 4][lane][4] f32; biases per row [64]
  const float* w32[KR_MAX_LAYERS];
  const float* b32[KR_MAX_LAYERS];
  int f32_ok;
};

}  // namespace kr

struct kr_handle {
  int device = 0;
  kr_params params{};
  kr_derived derived{};
  kr::RodConst<float> cf{};
  kr::RodConst<double> cd{};
  // MLP
  kr::MlpDev<float> mlp_f{};
  kr::MlpDev<double> mlp_d{};
  struct kr_mlp_plan* mlp_plan = nullptr;  // packed buffers + gather plan of the current network shape (kr_api.hip)
  // lazily grown scratch (history fallback, MLP activation spill)
  void* ws = nullptr;
  void* pred_buf = nullptr;   // predictor images of the one-launch-per-step multiple-shooting path
  size_t pred_bytes = 0;
  int grad_ordered = 0;       // kr_mlp_backward sums its partial gradients in a fixed order, without atomics (option "mlp_grad_ordered")
  int grad_accumulate = 0;    // kr_mlp_backward / kr_loss_rows_fwd_bwd add to dW, db, loss instead of zeroing them first
  int keep_predictor = 0;     // kr_simulate_batch resumes from / leaves behind the predictor image (option)
  int64_t pred_valid_B = 0;   // batch size the image in pred_buf was written for (0: none)
  int pred_valid_W = 1;       // ... and the wavefronts per rod of the kernel that wrote it
  int pred_valid_nn = 0;      // ... and whether the MLP was on (the image layout depends on the predictor's tap count)
  size_t ws_bytes = 0;
  int lds_limit = 160 * 1024;
  int ms_mode = -1;          // multiple-shooting step kernel: -1 auto (by batch size), 0 off, 1 forced
  // auto mode: multiple shooting when B <= this.  Measured (B = 2048 .. 8192, N = 100, fp64): 27.7 M rod-steps/s at
  // every batch size against 10.2 M for the 8-rods-per-wavefront kernel, so there is no limit by default
  int ms_batch_limit = 1 << 30;
  int predictor = 8;         // highest extrapolation order kr_simulate_batch may use (per-step launches: <= 2)
  int last_sim_path = 0;     // what the last kr_simulate_batch did: 0 one single-shooting launch per step,
                             // 1 one multiple-shooting launch per step, 2 one persistent launch for all steps
  int waves_per_rod = 0;     // per-step launches: wavefronts that share a rod (kr_msw_impl.hpp): 0 auto, 1, 2 or 4
  int last_waves_per_rod = 1;  // what the last step launch used
  void* loss_scratch = nullptr;  // per-workgroup loss partials of the fused forward + loss kernel
  // kr_train_epoch: the MFMA weight fragments in `frag_ws` mirror the flat parameter vector `frag_params` (the epoch's tail
  // kernel writes every updated parameter to both); another workspace, vector or network means packing afresh
  const void* frag_ws = nullptr;
  const void* frag_params = nullptr;
  uint64_t frag_net = 0;
  void* dbg = nullptr;       // diagnostic cycle-counter buffer (kr_debug_buffer)
  int fused_mlp = 1;         // training: fused MFMA forward/backward kernels (kr_mlp_fused.hip) when the shape allows
  int mfma_mlp = 1;          // evaluate the in-sweep MLP on the matrix cores when its shape allows
  int persistent = 1;        // kr_simulate_batch: run all steps in one launch when the multiple-shooting kernel applies
  int residual_test = 1;     // accept a storing sweep from its residual alone when the estimate is 256 x below the tolerance
  int overlap = 1;           // ... and overlap the verifying sweep of step t with the Jacobian sweep of step t + 1 (kr_mso_impl.hpp)
  int last_overlap = 0;      // the last kr_simulate_batch ran the overlapped kernel
  int msw_overlap = 1;       // several wavefronts per rod: the persistent kernel with overlapped steps (kr_mswo_impl.hpp)
  int nn_lowp_first = 1;     // fp64, MLP on, persistent one-wavefront kernel: first sweep of a three-sweep step on the fp32 base chain
  int nn_base_only_store = 1;  // fp64, MLP on, persistent one-wavefront kernel: storing sweeps without forward-difference columns
  void* resume_buf = nullptr;  // int32 per rod (SimArgs::resume)
  size_t resume_cap = 0;
  void* net_idx_buf = nullptr;  // int32 per rod: the network of rod b of a kr_simulate_batch_bank call (MlpBank::net_of_rod)
  size_t net_idx_cap = 0;
  void* hist_ws = nullptr;     // history records [B][N][12] of the several-wavefront persistent kernel with the MLP on
  size_t hist_ws_cap = 0;
  // Stream ordering of the handle's scratch (ws, pred_buf, resume_buf, hist_ws, loss_scratch are shared by its calls):
  // a call on another stream than the previous one first waits for everything queued on that one (kr::order_stream)
  hipStream_t last_stream = nullptr;
  bool have_last_stream = false;
  hipEvent_t order_event = nullptr;
};

// Per-rod parameter table (kr_param_table_create): row b = the constants of rod b, derived like the handle's own and
// uploaded in both precisions.  Immutable after creation.
struct kr_param_table {
  int device = 0;
  int64_t B = 0;
  // what every row shares with the handle it is used with
  int N = 0;
  int nn_input_history = 0;
  double del_t = 0;
  kr::RodConst<float>* rows_f = nullptr;   // [B], device
  kr::RodConst<double>* rows_d = nullptr;  // [B], device
  double* L = nullptr;                     // [B], device: rod lengths (kr_state_init_straight_table)
  double* par = nullptr;                   // [B][9], device: E, r, rho, vstar[3], g[3] - what kr_derive consumed (kr_adj_tab.hip)
};

// Bank of K networks of one shape (kr_mlp_bank_create): every network packed like the handle's own (the gather plan
// and mlp_pack_kernel of kr_set_mlp), the K packed images `stride` bytes apart in one arena - network k's buffers are
// those of network 0 (mf / md) moved by k * stride.  Changed only by kr_mlp_bank_repack, ordered on its stream; shape,
// K, stride and every address stay what creation made them.
struct kr_mlp_bank {
  int device = 0;
  int K = 0;
  kr::MlpDev<float> mf{};    // descriptor of network 0
  kr::MlpDev<double> md{};
  size_t stride = 0;         // bytes, a multiple of 256
  unsigned char* arena = nullptr;  // [K][stride], device (owned by `plan`)
  struct kr_mlp_plan* plan = nullptr;  // the gather plan creation packed with, kept for kr_mlp_bank_repack (kr_api.hip)
};

namespace kr {

// What a bank kernel takes in place of the by-value MlpDev<T> (ms_sim_kernel, MSRC): rod b runs network
// net_of_rod[b].  Like the rows of a parameter table the index array is written by the host only and never changes
// while a kernel reads it: constant address space, from the kernel argument on (mlp_src_net, kr_ms_impl.hpp).
template <typename T>
struct MlpBank : MlpDev<T> {  // (the base: the descriptor of network 0)
  const KR_CONSTANT_AS int32_t* net_of_rod;  // [B], every entry in [0, K): checked on the host before the launch
  unsigned long long stride;                 // bytes between the packed images of two networks
};

int ensure_ws(kr_handle* h, size_t bytes);
// Makes work queued on `s` from here on run after everything the handle's previous calls queued on ANOTHER stream (an
// event on that stream's tail; nothing at all when the stream did not change).  Every entry point that launches calls it.
int order_stream(kr_handle* h, hipStream_t s);
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for a kernel that needs more than 48 KB of dynamic LDS, once per
// (host thread, device, kernel, size): the attribute belongs to the device's copy of the kernel, so the cache is keyed
// by the current device too.  The prepare_* functions go through the same cache, so the first timed launch finds it set.
int dyn_lds(const void* kern, size_t smem);

template <typename T>
inline const RodConst<T>& consts(const kr_handle* h);
template <>
inline const RodConst<float>& consts<float>(const kr_handle* h) { return h->cf; }
template <>
inline const RodConst<double>& consts<double>(const kr_handle* h) { return h->cd; }
template <typename T>
inline const MlpDev<T>& mlpdev(const kr_handle* h);
template <>
inline const MlpDev<float>& mlpdev<float>(const kr_handle* h) { return h->mlp_f; }
template <>
inline const MlpDev<double>& mlpdev<double>(const kr_handle* h) { return h->mlp_d; }

// kr_sim.hip
template <typename T>
int launch_init_straight(kr_handle* h, int64_t B, T* state, hipStream_t s);
template <typename T>
int launch_pack(kr_handle* h, int64_t B, const T* y_fm, const T* z_fm, T* state, hipStream_t s);
template <typename T>
int launch_unpack(kr_handle* h, int64_t B, const T* state, T* y_fm, T* z_fm, hipStream_t s);
template <typename T>
int launch_unpack50(kr_handle* h, int64_t B, const T* st, const T* m1, const T* m2, T* out, hipStream_t s);
template <typename T>
int launch_tip(kr_handle* h, int64_t B, const T* state, T* tip, hipStream_t s);

// doubles per rod of a predictor image (kr_ms_impl.hpp: MS_PRED_ROWS x 64 lanes)
constexpr size_t KR_PRED_IMG_DOUBLES = 24 * 64;

template <typename T>
struct StepArgs {
  int64_t B;
  const T* prev2;   // optional: state two steps back (quadratic predictor); may alias `next` (read first)
  const T* prev;
  const T* cur;
  T* next;
  T* G;             // [B][6] in/out (residual mode: in only)
  const T* tens;    // tensions of rod b at tens[b*tens_stride .. +4]
  int64_t tens_stride;
  T* r_out;         // residual mode: [B][6]
  T* tip;           // optional: tip[b*tip_stride .. +3]
  int64_t tip_stride;
  int32_t* status;  // optional: status[b*st_stride]
  int32_t* iters;
  int64_t st_stride;
  T* hist_ws;       // global history fallback [B][N][HS]
  T* act_ws;        // MLP activation spill (global) or nullptr
  T tol, tolA, fd_eps;
  T hc1, hc2;       // history = hc1*cur + hc2*prev (c1, c2 of BDF2, or 1, 0 for explicit history)
  int maxit;
  int mode;         // 0 = Newton step, 1 = single residual sweep
  int pred_order;   // initial guess: 0 = caller's G / current state, 1 = linear, 2 = quadratic extrapolation in time
  // multiple-shooting kernel inside kr_simulate_batch: image of the start-value predictor (MsPred, kr_ms_impl.hpp),
  // [B][MS_PRED_ROWS][64] doubles, read and rewritten by every launch; nullptr = extrapolate from the states
  double* pred = nullptr;
  int pred_reset = 0;     // first step of a simulate call: build the predictor from cur / prev
  int pred_has_prev = 0;  // ... prev is a real earlier state
  int pred_limit = 0;     // the handle's "predictor" option
  int residual_test = 1;  // option "residual_test": see kr_set_option (knode_rod.h)
  // residual mode, RK4 only: explicit midpoint histories [B][N][KR_SLOTS] (record j = between grid points j and j + 1);
  // nullptr = the linear interpolation knode.simulate forms (knode.py:80-81)
  const T* mid = nullptr;
};
// persistent multi-step form (kr_ms_impl.hpp)
template <typename T>
struct SimArgs {
  int64_t B, T_steps;
  T* states;            // [(T+1) or 3][B][N][KR_SLOTS]
  int64_t slot_elems;   // B*N*KR_SLOTS
  int ring;
  const T* prev_init;   // state before states[0] (nullable: y_prev = y, knode.py:65-66)
  const T* ctl;         // [B][T][4]
  T* G;                 // [B][6] in/out
  T* tip;               // [B][T][3] nullable
  int32_t* status;      // [B][T] nullable
  T tol, tolA, fd_eps, hc1, hc2;
  int maxit, predictor;
  unsigned long long* dbg;  // diagnostic builds (-DKR_MS_STAMPS): [B][24] cycle counters, else unused
  double* pred_io;          // predictor image [B][KR_PRED_IMG_DOUBLES]: saved at the end (nullable)
  int pred_load;            // ... and loaded at the start instead of building the predictor from the states
  // Two-launch form (kr_mso_impl.hpp): the overlapped kernel leaves, per rod, the first step it did NOT finish
  // (T_steps: all done); the one-wavefront persistent kernel launched behind it with the same arguments resumes
  // exactly there with its full fallback ladder.  nullptr: every rod starts at step 0.
  int32_t* resume = nullptr;
  int residual_test = 1;  // option "residual_test"
  T* hist_ws = nullptr;   // kr_msw_impl.hpp, MLP on: [B][N][12] history records (global memory instead of LDS)
  int nn_lowp = 1;        // option "nn_lowp_first" (MsSolveArgs::lowp_allowed)
  int nn_base_only = 1;   // option "nn_base_only_store" (MsSolveArgs::bo_allowed)
};

template <typename T>
inline const RodConst<T>* table_rows(const kr_param_table* t);
template <>
inline const RodConst<float>* table_rows<float>(const kr_param_table* t) { return t->rows_f; }
template <>
inline const RodConst<double>* table_rows<double>(const kr_param_table* t) { return t->rows_d; }
template <typename T>
inline const MlpDev<T>& bank_net0(const kr_mlp_bank* bk);
template <>
inline const MlpDev<float>& bank_net0<float>(const kr_mlp_bank* bk) { return bk->mf; }
template <>
inline const MlpDev<double>& bank_net0<double>(const kr_mlp_bank* bk) { return bk->md; }

// ---- which kernel a call runs (kr_plan.hip: the rules of DESIGN.md section 5, each stated once) -----------------------
enum SimFamily {
  KR_FAM_SS,          // one launch per step, single shooting, 8 rods per wavefront (kr_sim_impl.hpp)
  KR_FAM_MS_STEP,     // one launch per step, multiple shooting, MLP off (kr_ms_impl.hpp)
  KR_FAM_MS_STEP_NN,  // ... with the MLP inside the sweeps (kr_msn_*.hip)
  KR_FAM_MSW_STEP,    // ... on W = 2 / 4 wavefronts per rod (kr_msw_impl.hpp)
  KR_FAM_MS_SIM,      // all steps in one launch, one wavefront per rod (kr_ms_impl.hpp)
  KR_FAM_MSO,         // the overlapped kernel (kr_mso_impl.hpp), then KR_FAM_MS_SIM (OCC = 1) for the steps it left behind
  KR_FAM_MSW_SIM,     // all steps in one launch on W wavefronts per rod, MLP off (history mode `hm` 0 / 1)
  KR_FAM_MSW_NN_SIM,  // ... with the MLP on (kr_mswn_*.hip)
  KR_FAM_MSWO         // ... with overlapped steps (kr_mswo_impl.hpp)
};
// Where a rod's constants, its per-step data and its network come from: one kind per simulate entry point.  Every kind
// but the first is a table call (SimSrc::table) served by the one-wavefront persistent kernels only (plan_table).
enum SimKind { KR_SRC_HANDLE, KR_SRC_TABLE, KR_SRC_LOADS, KR_SRC_BOUNDARY, KR_SRC_KEYPOINTS, KR_SRC_BANK, KR_SRC_BANK_KEYPOINTS };
// (the kinds whose network comes from a bank)
constexpr bool sim_kind_banked(int kind) { return kind == KR_SRC_BANK || kind == KR_SRC_BANK_KEYPOINTS; }
// ... and how a kind is spoken of: its entry point, the word for it in a refusal, and the end of the refusal sentence
struct SimKindText {
  const char *api, *word, *tail;
};
constexpr SimKindText kSimKindText[] = {
    {"kr_simulate_batch", "", ""},
    {"kr_simulate_batch_table", "table", "not served with a parameter table; nothing falls back to the handle's parameters"},
    {"kr_simulate_batch_loads", "loads", "not served with per-step tip loads; nothing falls back to a frozen wrench"},
    {"kr_simulate_batch_boundary", "boundary", "not served with per-step boundary data; nothing falls back to a frozen base or wrench"},
    {"kr_simulate_batch_keypoints", "key-point", "not served with key-point records; nothing falls back to a call without them"},
    {"kr_simulate_batch_bank", "bank", "not served with a network bank; nothing falls back to the handle's MLP"},
    {"kr_simulate_batch_bank_keypoints", "bank key-point",
     "not served with a network bank and per-step boundary data; nothing falls back to the handle's MLP or a frozen boundary"},
};
// kr_simulate_batch_keypoints / _bank_keypoints: kp[T][B][K][KR_SLOTS] of the call's element type and the marked grid
// points, bit j of (mask_lo, mask_hi) = grid point j (the bank form also with K = 0: no pointer, an empty mask)
struct KpDst {
  void* kp = nullptr;
  int K = 0;
  unsigned long long mask_lo = 0, mask_hi = 0;
};
// The source of one call: what its kind needs, nothing else set
struct SimSrc {
  int kind = KR_SRC_HANDLE;
  const kr_param_table* table = nullptr;  // every kind but KR_SRC_HANDLE
  const void* hist = nullptr;             // KR_SRC_LOADS: loads[B][T][6]; KR_SRC_BOUNDARY / _KEYPOINTS / _BANK_KEYPOINTS: bnd[B][T][KR_BND]; element type of the call
  KpDst kp;                               // KR_SRC_KEYPOINTS / _BANK_KEYPOINTS: where the key-point records go
  const kr_mlp_bank* bank = nullptr;      // KR_SRC_BANK / _BANK_KEYPOINTS
  const int32_t* net_idx = nullptr;       // ... and the device copy of the caller's index array
};
struct SimPlan {
  int rc = KR_OK;     // KR_OK, or what a refused call returns (`why` says why)
  int path = 0;       // what last_sim_path reports: 0 / 1 one launch per step (single / multiple shooting), 2 persistent
  int family = KR_FAM_SS;
  int W = 1;          // wavefronts per rod
  int occ = 1;        // workgroups per CU the instantiation is built for (2: fp32, B > 1024)
  int hm = 0;         // KR_FAM_MSW_SIM: where the time history lives (msw_sim_kernel)
  int rods_per_wg = 0;  // KR_FAM_MS_STEP*: rods (= wavefronts) per workgroup
  bool diag = true, nn = false, nn_hist = false, gt = false, overlap = false;
  int scheme = KR_EULER;
  size_t smem[2] = {0, 0};  // dynamic LDS of the launch (KR_FAM_MSO: of the overlapped kernel, of the take-over launch)
  size_t hist_ws_bytes = 0; // KR_FAM_MSW_NN_SIM: the history workspace [B][N][12] (SimArgs::hist_ws)
  char why[256] = "";
};
struct PlanQuery {
  int64_t B, T_steps;
  int scheme, use_nn;
  int source = KR_SRC_HANDLE;          // SimSrc::kind
  int N = 0;                           // table calls: the table's
  const kr_mlp_bank* bank = nullptr;   // bank calls
  // the aliasing rule of KR_FAM_MSWO with its tiles in HBM
  const void* prev_init = nullptr;
  const void* states = nullptr;
  int64_t slot_elems = 0;
};
// the query of a simulate call on `src` (simulate_impl, kr_api.hip)
inline PlanQuery plan_query(const SimSrc& src, int64_t B, int64_t T_steps, int scheme, int use_nn, const void* prev_init = nullptr,
                            const void* states = nullptr, int64_t slot_elems = 0) {
  PlanQuery q{B, T_steps, scheme, use_nn, src.kind, src.table ? src.table->N : 0, src.bank};
  q.prev_init = prev_init; q.states = states; q.slot_elems = slot_elems;
  return q;
}
template <typename T>
SimPlan plan_simulate(const kr_handle* h, const PlanQuery& q);
// kr_step_batch, kr_residual_* (mode 1) and the steps of a kr_simulate_batch that takes one launch per step
template <typename T>
SimPlan plan_step(const kr_handle* h, int64_t B, int scheme, int use_nn, int mode);
// The start-value predictor image of a simulate call: one per wavefront of a rod, KR_PRED_IMG_DOUBLES each
// (SimArgs::pred_io / pred_load, StepArgs::pred / pred_reset)
struct PredImage {
  bool use = false, load = false;  // the kernels get the buffer; ... and start from the image the call before left in it
  int64_t rows = 0;                // images in the buffer
};
PredImage plan_pred_image(const kr_handle* h, const SimPlan& p, int64_t B);
// What the last calls ran (options last_sim_path / last_overlap / last_waves_per_rod) and what they left in the image
// buffer: written by these two only, after the launches succeeded
void note_sim_plan(kr_handle* h, const SimPlan& p, const PredImage& im, int64_t B);
void note_step_plan(kr_handle* h, const SimPlan& p);  // a step or residual call

// Where a launch goes: stream `s`, or - kr_simulate_prepare - nowhere: the kernel is resolved in the code object and its
// dynamic LDS limit set, which is the one-time host work of its first launch.
struct LaunchAt {
  hipStream_t s;
  bool prepare_only;
};
template <typename... P, typename... A>
inline int launch(const LaunchAt& at, void (*kern)(P...), dim3 grid, dim3 block, size_t smem, const A&... args) {
  if (at.prepare_only) {
    hipFuncAttributes fa;
    KR_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kern)));
  }
  if (int rc = dyn_lds(reinterpret_cast<const void*>(kern), smem)) return rc;
  if (at.prepare_only) return KR_OK;
  hipLaunchKernelGGL(kern, grid, block, smem, at.s, args...);
  KR_HIP(hipGetLastError());
  return KR_OK;
}
template <typename... P, typename... A>
inline int launch(hipStream_t s, void (*kern)(P...), dim3 grid, dim3 block, size_t smem, const A&... args) {
  return launch(LaunchAt{s, false}, kern, grid, block, smem, args...);
}

// The launchers: each maps a plan to the template instantiation it names and launches it, in the unit that holds the
// kernel.
template <typename T>
int launch_step(kr_handle* h, const SimPlan& p, const StepArgs<T>& a, hipStream_t s);            // kr_sim_*.hip
template <typename T>
int launch_ms_step_nn(kr_handle* h, const SimPlan& p, const StepArgs<T>& a, hipStream_t s);      // kr_msn_*.hip
template <typename T>
int launch_ms_sim(kr_handle* h, const SimPlan& p, bool take_over, const SimArgs<T>& a, const LaunchAt& at);  // kr_sim_*.hip
template <typename T>
int launch_msw_sim(kr_handle* h, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);     // kr_sim_*.hip (hm = 0)
template <typename T>
int launch_msw_gh_sim(kr_handle* h, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);  // kr_mswn_*.hip (hm = 1)
template <typename T>
int launch_msw_nn_sim(kr_handle* h, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);  // kr_mswn_*.hip
template <typename T>
int launch_mso_sim(kr_handle* h, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);     // kr_mso_*.hip
template <typename T>
int launch_mswo_sim(kr_handle* h, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);    // kr_mswo_*.hip
template <typename T>
int launch_tab_init_straight(kr_handle* h, const kr_param_table* t, T* state, hipStream_t s);   // kr_tab_*.hip
// the table kinds, one signature: each fills its kernels' source struct from `src` (launch_one_wave_src, kr_tab_impl.hpp)
template <typename T>
int launch_tab_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);  // kr_tab_*.hip
template <typename T>
int launch_load_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);  // kr_load_*.hip
template <typename T>
int launch_bnd_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);  // kr_bnd_*.hip
template <typename T>
int launch_kp_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);  // kr_kp_*.hip
template <typename T>
int launch_bank_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);  // kr_bank_*.hip
template <typename T>
int launch_bankkp_sim(kr_handle* h, const SimSrc& src, const SimPlan& p, const SimArgs<T>& a, const LaunchAt& at);  // kr_bankkp_*.hip
int ensure_resume(kr_handle* h, int64_t B);
int ensure_hist_ws(kr_handle* h, size_t bytes);

// A persistent plan (path 2) carried out: the handle's buffers the plan asks for, then the launcher(s) of its family
template <typename T>
inline int launch_sim(kr_handle* h, const SimPlan& p, const SimSrc& src, SimArgs<T> a, const LaunchAt& at) {
  if (p.family == KR_FAM_MSO) {  // (the overlapped kernel leaves, per rod, the first step it did not finish)
    if (int rc = ensure_resume(h, a.B)) return rc;
    a.resume = static_cast<int32_t*>(h->resume_buf);
  }
  if (p.hist_ws_bytes) {
    if (int rc = ensure_hist_ws(h, p.hist_ws_bytes)) return rc;
    a.hist_ws = static_cast<T*>(h->hist_ws);
  }
  switch (src.kind) {
    case KR_SRC_TABLE: return launch_tab_sim<T>(h, src, p, a, at);
    case KR_SRC_LOADS: return launch_load_sim<T>(h, src, p, a, at);
    case KR_SRC_BOUNDARY: return launch_bnd_sim<T>(h, src, p, a, at);
    case KR_SRC_KEYPOINTS: return launch_kp_sim<T>(h, src, p, a, at);
    case KR_SRC_BANK: return launch_bank_sim<T>(h, src, p, a, at);
    case KR_SRC_BANK_KEYPOINTS: return launch_bankkp_sim<T>(h, src, p, a, at);
    default: break;  // (KR_SRC_HANDLE: by family)
  }
  switch (p.family) {
    case KR_FAM_MSO:
      if (int rc = launch_mso_sim<T>(h, p, a, at)) return rc;
      return launch_ms_sim<T>(h, p, true, a, at);
    case KR_FAM_MS_SIM: return launch_ms_sim<T>(h, p, false, a, at);
    case KR_FAM_MSWO: return launch_mswo_sim<T>(h, p, a, at);
    case KR_FAM_MSW_NN_SIM: return launch_msw_nn_sim<T>(h, p, a, at);
    case KR_FAM_MSW_SIM: return p.hm ? launch_msw_gh_sim<T>(h, p, a, at) : launch_msw_sim<T>(h, p, a, at);
    default: set_error("launch_sim: not a persistent plan"); return KR_E_STATE;
  }
}

// kr_mlp_fused.hip: fused fp32 MLP forward / backward for training
bool fused_mlp_supported(int n_layers, const int32_t* dims, const int32_t* acts, int in_pad);
size_t fused_ws_bytes(int n_layers, const int32_t* dims, int64_t Q);
// loss fused into the epilogue of the forward kernel (kr_mlp_forward_loss); all device pointers
struct FusedLoss {
  const float* base;         // [Q][25] parameter-free part of the prediction
  const float* target_rows;  // [Q][25]
  float* dout;               // [Q][32] gradient with respect to the MLP outputs
  float* loss;               // the four-term loss is ADDED here
  void* scratch;             // 4096 floats of the handle: per-workgroup partials
  float ds, inv_denom;
  int K;
};
// do_pack = false: the fragments in ws are current (kr_train_epoch keeps them so); n_partials != nullptr: the loss
// partials stay in fl->scratch, *n_partials of them, for the caller's next kernel
int fused_mlp_forward(int64_t Q, int n_layers, const int32_t* dims, const int32_t* acts, const float* const* W,
                      const float* const* b, const float* x, float* out, void* ws, hipStream_t s,
                      const FusedLoss* fl = nullptr, bool do_pack = true, int* n_partials = nullptr);
// leave != nullptr: no reduction launch - the slabs of partial gradients are described there (dW, db unused)
// ordered: the slab sum in a fixed order, without atomics (option "mlp_grad_ordered": reduce_slabs_ordered_kernel)
struct FusedSlabs {
  const float* slab;
  int nslab, P, nparams;
  int poff[6];
};
int fused_mlp_backward(int64_t Q, int n_layers, const int32_t* dims, const int32_t* acts, const float* const* W,
                       const float* x, const float* dout, void* ws, float* const* dW, float* const* db, hipStream_t s,
                       FusedSlabs* leave = nullptr, bool ordered = false);
// kr_train_epoch: flat parameter / gradient / moment vectors in nn.Linear order (W1, b1, W2, b2, ...), g with one
// trailing loss slot
struct FusedEpoch {
  int64_t Q;
  int K, n_layers;
  const int32_t* dims;
  const int32_t* acts;
  float *p, *g, *m, *v;
  const float* lower;
  double* sched;
  const float *x, *base, *target_rows;
  float* dout;
  void* ws;
  void* loss_scratch;
  float ds, inv_denom;
  double beta1, beta2, eps, weight_decay, factor, threshold, min_lr;
  int patience;
  int64_t step;
  float* loss_log;
  int phase;
  bool pack;
};
int fused_train_epoch(const FusedEpoch& E, hipStream_t s);
void fused_set_debug(void* dev_u64x48);  // diagnostic build: where the fused kernels add their phase stamps

// kr_nnjac.hip: the MLP's input Jacobian on the fp64 matrix cores.  nnjac_check: the refusals of a call that needs it
// (no network: KR_E_STATE; a shape or input it does not serve: KR_E_UNSUPPORTED), message prefixed with `api`.
// launch_nnjac: rows x (x_stride elements apart) -> jac[Q][700], transposed ? [28][25] : [25][28]
int nnjac_check(const kr_handle* h, const char* api);
template <typename T>
int launch_nnjac(kr_handle* h, int64_t Q, const T* x, int64_t x_stride, T* jac, int transposed, hipStream_t s);
// The same for a descriptor that is not the handle's - network k of a bank, the bank's fp64 descriptor moved by k * stride
// (kr_adj_bank.hip; the descriptor form is instantiated for double only)
int nnjac_check(const MlpDev<double>& M, int nn_input_history, const char* api);
template <typename T>
int launch_nnjac(const MlpDev<double>& M, int64_t Q, const T* x, int64_t x_stride, T* jac, int transposed, hipStream_t s);

// kr_ode.hip
template <typename T>
int launch_mlp_eval(kr_handle* h, int64_t Q, const T* x, T* out, hipStream_t s);
template <typename T>
int launch_ode_batch(kr_handle* h, int64_t Q, const T* y, const T* yh, const T* zh, const T* tf, T* dys, T* z,
                     int use_nn, hipStream_t s);

}  // namespace kr
