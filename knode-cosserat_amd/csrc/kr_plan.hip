// kr_plan.hip - which kernel a call runs: the selection rules of DESIGN.md section 5, each stated once, as a plan the
// launchers of the kernel units carry out.  Holds no kernel (the kernel headers are included for their LDS-size
// functions, which stay next to the kernels' own carving of the LDS).
#define KR_MS_NO_INST
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "kr_mswo_impl.hpp"

namespace kr {
namespace {

// Every rod resident at once (a second round of workgroups would wait for the first to finish all its steps): 256 CUs,
// as many workgroups of `bytes` on each as its LDS takes.
bool all_resident(const kr_handle* h, size_t bytes, int64_t B) {
  return bytes <= (size_t)h->lds_limit && B <= 256 * (int64_t)((size_t)h->lds_limit / bytes);
}
// options ms_mode / ms_batch_limit: multiple shooting forced (1), off (0), or - auto - up to a batch size (no limit by
// default: faster at every batch size)
bool ms_wanted(const kr_handle* h, int64_t B) {
  return h->ms_mode == 1 || (h->ms_mode != 0 && B <= (int64_t)h->ms_batch_limit);
}
// what the one-wavefront persistent kernels serve: enough segments to cut, two grid points per lane in registers
bool one_wave_range(int N) { return N - 1 >= 2 * MS_P && N <= MS_NPL * WAVE; }
// sub-intervals per wavefront: 4 on the first, 3 on the others, two segments each at least
bool msw_long_enough(int N, int W) { return N - 1 >= 2 * (4 + 3 * (W - 1)); }
// an MLP the matrix-core evaluator of the per-step kernels serves (no per-lane activation buffers there) ...
template <typename T>
bool net_in_sweeps(const kr_handle* h, const MlpDev<T>& M) {
  return M.n_layers > 0 && M.mfma_ok && !h->params.nn_input_history;
}
// ... and one the persistent kernels evaluate: they carry the base + JVP evaluator only
template <typename T>
bool net_persistent(const kr_handle* h, const MlpDev<T>& M) {
  return net_in_sweeps(h, M) && M.jvp_ok;
}

template <typename T>
size_t msw_step_bytes(int N, int W) {
  return sizeof(T) * (W == 2 ? msw_lds_elems<T, 2>(N) : msw_lds_elems<T, 4>(N));
}
template <typename T>
size_t msw_sim_bytes(int N, int W, bool nn, int hm) {
  return sizeof(T) * (W == 2 ? msw_sim_lds_elems<T, 2>(N, nn, hm) : msw_sim_lds_elems<T, 4>(N, nn, hm));
}
template <typename T>
size_t mswo_bytes(int N, int W, bool gt) {
  if (gt) return sizeof(T) * (W == 2 ? mswo_lds_elems<T, 2, true>(N) : mswo_lds_elems<T, 4, true>(N));
  return sizeof(T) * (W == 2 ? mswo_lds_elems<T, 2, false>(N) : mswo_lds_elems<T, 4, false>(N));
}

// Wavefronts per rod of the MLP-off kernels (0: one).  Auto: batches that leave SIMDs idle (one wavefront per
// SIMD at most, B W <= 1024); the option "waves_per_rod" forces 1 / 2 / 4.  Measured, fp64, us per step
// (tools/msw_timing.py; persistent = all steps of kr_simulate_batch in one launch):
//     N    B    persistent W=1   per step W=4   persistent W=2   persistent W=4
//    40  256        20.5            25.5            18.2             18.6
//    64  256        26.9             -              21.4             20.3
//   100  256        35.9            30.3            26.9             23.6
//   100  512        36.5             -              29.5              -
//   128  256     (47.7 per step)    32.6            31.1             25.6
//   400  256    (115 per step)      59.5             -              52.6     (persistent: the long-rod form, HM = 1)
template <typename T>
int msw_waves(const kr_handle* h, int scheme, int use_nn, int64_t B, int mode) {
  const int N = consts<T>(h).N;
  if (use_nn || scheme != KR_EULER || mode != 0 || h->ms_mode == 0) return 0;
  auto fits = [&](int W) {  // the one-launch-per-step kernel
    return msw_long_enough(N, W) && B * W <= 1024 && all_resident(h, msw_step_bytes<T>(N, W), B);
  };
  auto fits_sim = [&](int W) { return all_resident(h, msw_sim_bytes<T>(N, W, false, 0), B); };  // ... and its persistent form
  if (h->waves_per_rod == 1) return 0;
  if (h->waves_per_rod == 2) return fits(2) ? 2 : 0;
  if (h->waves_per_rod == 4) return fits(4) ? 4 : 0;
  if (N <= MS_NPL * WAVE) {
    // the persistent one-wavefront kernel serves these: several wavefronts only where their own persistent form fits
    // and the rod is long enough for the shorter chains to pay for the distributed condensation
    if (N >= 56 && fits(4) && fits_sim(4)) return 4;
    if (N >= 32 && fits(2) && fits_sim(2)) return 2;
    return 0;
  }
  if (fits(4)) return 4;
  if (fits(2)) return 2;
  return 0;
}

template <typename T>
bool msw_nn_fits(const kr_handle* h, int W, int64_t B) {
  const int N = consts<T>(h).N;
  if (!msw_long_enough(N, W)) return false;
  // One wavefront per SIMD at most.  The kernel and its evaluator use all 512 registers of a SIMD lane; instantiations
  // limited to 256 (two wavefronts per SIMD, which B = 1024 would need) were built and measured: everything live in
  // the sweep is then spilled around every evaluator call and the scratch traffic of eight wavefronts per CU makes a
  // step 1.9 x SLOWER than one wavefront per rod (fp64 1.88 against 1.00 ms, fp32 1.01 against 0.57 ms at B = 1024).
  if (B * W > 1024) return false;
  return all_resident(h, msw_sim_bytes<T>(N, W, true, 2), B);
}
// Wavefronts per rod of the persistent kernel with the MLP on (0: one)
template <typename T>
int msw_nn_waves(const kr_handle* h, int scheme, int64_t B) {
  if (scheme != KR_EULER || !consts<T>(h).diag || !net_persistent(h, mlpdev<T>(h))) return 0;
  if (h->waves_per_rod == 1) return 0;
  if (h->waves_per_rod == 2) return msw_nn_fits<T>(h, 2, B) ? 2 : 0;
  if (h->waves_per_rod == 4) return msw_nn_fits<T>(h, 4, B) ? 4 : 0;
  if (msw_nn_fits<T>(h, 4, B)) return 4;
  if (msw_nn_fits<T>(h, 2, B)) return 2;
  return 0;
}

SimPlan refused(int rc, const char* fmt, ...) {
  SimPlan p;
  p.rc = rc;
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(p.why, sizeof p.why, fmt, ap);
  va_end(ap);
  return p;
}
constexpr const char* kNoMlp = "use_nn requested but no MLP was set (kr_set_mlp)";

// KR_FAM_MSO where the overlapped kernel serves the problem (Euler, diagonal matrices, MLP off, its LDS fits), else the
// one-wavefront persistent kernel alone.  `smem`: of that kernel.
template <typename T>
SimPlan plan_one_wave(const kr_handle* h, SimPlan p, const PlanQuery& q, int N, size_t smem, bool two_per_simd_ok) {
  const size_t smem_o = sizeof(T) * mso_lds_elems<T, hs_phys<T>()>(N) * MS_WPB;
  // fp32, more rods than SIMDs, and two workgroups fit the LDS of a CU: the two-wavefronts-per-SIMD instantiation
  const bool occ2 = two_per_simd_ok && sizeof(T) == 4 && q.B > 1024 && q.scheme == KR_EULER && p.diag;
  if (q.scheme == KR_EULER && p.diag && h->overlap && smem_o <= (size_t)h->lds_limit) {
    // two launches: the overlapped kernel (one sweep per step in the steady state), then the persistent kernel for
    // the rods that left steps behind (a rod that finished exits at once)
    if (q.T_steps > (int64_t)0x7fffffff)
      return refused(KR_E_ARG, "T_steps = %lld: the overlapped persistent kernel counts steps in 32 bits (T_steps < 2^31)", (long long)q.T_steps);
    p.family = KR_FAM_MSO;
    p.overlap = true;
    p.occ = occ2 && 2 * smem_o <= (size_t)h->lds_limit ? 2 : 1;
    p.smem[0] = smem_o;
    p.smem[1] = smem;
    return p;
  }
  p.family = KR_FAM_MS_SIM;
  p.occ = occ2 && 2 * smem <= (size_t)h->lds_limit ? 2 : 1;
  p.smem[0] = smem;
  return p;
}

// kr_simulate_batch_table / _bank / _bank_keypoints / _loads / _boundary / _keypoints (a table call whose tip wrench, or whose base state and tip
// wrench, vary in time, the latter also with key-point records: the same plan, the loads, boundary or key-point instantiations of the same kernels): the one-wavefront persistent kernels only, and a refusal (never the handle's own
// parameters or network) for everything they do not serve
template <typename T>
SimPlan plan_table(const kr_handle* h, const PlanQuery& q) {
  const bool bank = sim_kind_banked(q.source);
  const SimKindText& text = kSimKindText[q.source];
  const char* const word = text.word;
  char what[128];
  auto refuse = [&](const char* w) { return refused(KR_E_UNSUPPORTED, "%s: %s (%s)", text.api, w, text.tail); };
  if (q.scheme != KR_EULER) return refuse("only Euler sweeps (scheme = KR_EULER)");
  if (!one_wave_range(q.N)) {
    std::snprintf(what, sizeof what, "N = %d, the one-wavefront persistent %s 9 <= N <= 128", q.N, bank ? "kernel serves" : "kernels serve");
    return refuse(what);
  }
  if (h->ms_mode == 0 || h->persistent == 0) {
    std::snprintf(what, sizeof what, "options ms_mode = 0 / persistent = 0 select kernels without a %s form", word);
    return refuse(what);
  }
  if (!ms_wanted(h, q.B)) return refuse("B exceeds option ms_batch_limit");
  if (h->waves_per_rod > 1) {
    std::snprintf(what, sizeof what, "option waves_per_rod = %d, %s calls run one wavefront per rod", h->waves_per_rod, word);
    return refuse(what);
  }
  if (q.B > (int64_t)0x7fffffff) return refuse("B >= 2^31");
  const bool nn = bank || q.use_nn;
  if (bank) {
    if (!net_persistent(h, bank_net0<T>(q.bank)) || !h->mfma_mlp) return refuse("a network shape the persistent one-wavefront kernel does not evaluate");
  } else if (nn) {
    if (mlpdev<T>(h).n_layers <= 0) return refused(KR_E_STATE, "%s", kNoMlp);
    if (!net_persistent(h, mlpdev<T>(h))) return refuse("an MLP the persistent one-wavefront kernel does not evaluate");
  }
  const size_t smem = ms_lds_bytes<T, hs_phys<T>()>(q.N, true, nn);
  if (smem > (size_t)h->lds_limit) return refuse(nn ? "the rod's history does not fit the LDS with the MLP on" : "the rod's history does not fit the LDS");
  SimPlan p;
  p.path = 2;
  p.scheme = KR_EULER;
  p.nn = nn;
  if (!nn) return plan_one_wave<T>(h, p, q, q.N, smem, false);  // (no table form of the two-wavefronts-per-SIMD instantiation)
  p.family = KR_FAM_MS_SIM;
  p.smem[0] = smem;
  return p;
}

}  // namespace

template <typename T>
SimPlan plan_step(const kr_handle* h, int64_t B, int scheme, int use_nn, int mode) {
  const RodConst<T>& P = consts<T>(h);
  const MlpDev<T>& M = mlpdev<T>(h);
  if (scheme != KR_EULER && scheme != KR_RK4) return refused(KR_E_ARG, "unknown scheme");
  SimPlan p;
  p.scheme = scheme;
  p.diag = P.diag != 0;
  p.nn = use_nn != 0;
  if (const int W = msw_waves<T>(h, scheme, use_nn, B, mode)) {  // several wavefronts per rod
    p.path = 1;
    p.family = KR_FAM_MSW_STEP;
    p.W = W;
    p.smem[0] = msw_step_bytes<T>(P.N, W);
    return p;
  }
  // multiple shooting: Newton steps only, enough segments to cut, and as many rods per workgroup as the LDS history of N
  // grid points allows (ms_wpb)
  const int wpb = ms_wpb<T, hs_phys<T>()>(P.N, p.nn, (size_t)h->lds_limit);
  if (mode == 0 && (!use_nn || net_in_sweeps(h, M)) && ms_wanted(h, B) && P.N - 1 >= 2 * MS_P && wpb > 0) {
    p.path = 1;
    p.family = use_nn ? KR_FAM_MS_STEP_NN : KR_FAM_MS_STEP;
    p.rods_per_wg = wpb;
    p.smem[0] = ms_lds_bytes<T, hs_phys<T>()>(P.N, false, p.nn, wpb);
    return p;
  }
  if (use_nn && M.n_layers <= 0) return refused(KR_E_STATE, "%s", kNoMlp);
  p.family = KR_FAM_SS;  // (launch_step_mem places history and activations in LDS or the workspace)
  p.nn_hist = use_nn && h->params.nn_input_history;
  return p;
}

template <typename T>
SimPlan plan_simulate(const kr_handle* h, const PlanQuery& q) {
  if (q.source != KR_SRC_HANDLE) return plan_table<T>(h, q);
  const RodConst<T>& P = consts<T>(h);
  // one launch per step unless a persistent form applies (the per-step plan also holds the refusals: unknown scheme, no MLP)
  const SimPlan per_step = plan_step<T>(h, q.B, q.scheme, q.use_nn, 0);
  if (per_step.rc != KR_OK || h->ms_mode == 0 || h->persistent == 0) return per_step;
  SimPlan p;
  p.path = 2;
  p.scheme = q.scheme;
  p.diag = P.diag != 0;
  p.nn = q.use_nn != 0;
  if (const int W = msw_waves<T>(h, q.scheme, q.use_nn, q.B, 0)) {  // several wavefronts per rod, MLP off
    p.W = W;
    if (h->msw_overlap && P.diag) {
      static const int force_gt = std::getenv("KR_MSWO_GT") ? std::atoi(std::getenv("KR_MSWO_GT")) : -1;  // (tests: 1 = tiles in HBM, 0 = never)
      const size_t b_lds = mswo_bytes<T>(P.N, W, false), b_gt = mswo_bytes<T>(P.N, W, true);
      const bool gt = force_gt == 1 || (force_gt != 0 && !all_resident(h, b_lds, q.B));
      bool ok = all_resident(h, gt ? b_gt : b_lds, q.B);
      if (ok && gt && q.prev_init) {
        // The GT form reads the state before states[0] while step 0 is being verified, i.e. while the slot of state 1 is written:
        // a caller's prev_init inside that slot (knode_rod.h allows it to point into the ring) takes the plain form, which
        // consumes it before its first store.
        const T* s1 = static_cast<const T*>(q.states) + q.slot_elems;
        const T* pi = static_cast<const T*>(q.prev_init);
        if (pi >= s1 && pi < s1 + q.slot_elems) ok = false;
      }
      if (ok) {
        p.family = KR_FAM_MSWO;
        p.overlap = true;
        p.gt = gt;
        p.smem[0] = gt ? b_gt : b_lds;
        return p;
      }
    }
    // everything in LDS, else (long rods) the form that reads the two newest states from A.states
    p.family = KR_FAM_MSW_SIM;
    for (p.hm = 0; p.hm <= 1; ++p.hm) {
      p.smem[0] = msw_sim_bytes<T>(P.N, W, false, p.hm);
      if (all_resident(h, p.smem[0], q.B)) return p;
    }
    return per_step;  // (the several-wavefront step kernel, W as here)
  }
  if (q.use_nn) {
    if (const int W = msw_nn_waves<T>(h, q.scheme, q.B)) {  // several wavefronts per rod, MLP on (kr_mswn_*.hip)
      p.family = KR_FAM_MSW_NN_SIM;
      p.W = W;
      p.smem[0] = msw_sim_bytes<T>(P.N, W, true, 2);
      p.hist_ws_bytes = (size_t)q.B * P.N * HS_LEAN * sizeof(T);  // its history records live in global memory
      return p;
    }
    // MLP inside the sweeps of the one-wavefront kernel: Euler sweeps and diagonal material matrices only; everything
    // else takes one launch per step
    if (!net_persistent(h, mlpdev<T>(h)) || q.scheme != KR_EULER || !P.diag) return per_step;
  }
  const size_t smem = ms_lds_bytes<T, hs_phys<T>()>(P.N, true, p.nn);
  if (!one_wave_range(P.N) || smem > (size_t)h->lds_limit || !ms_wanted(h, q.B)) return per_step;
  if (!q.use_nn) return plan_one_wave<T>(h, p, q, P.N, smem, true);
  p.family = KR_FAM_MS_SIM;
  p.smem[0] = smem;
  return p;
}

// A persistent kernel saves and loads the image where the caller keeps the predictor between calls (keep_predictor).
// With one launch per step the multiple-shooting kernels carry their predictor from launch to launch through it, so it
// is handed over wherever multiple shooting is wanted (the single-shooting kernel does not read it).  Never more than
// 1 GB of it.  It does not depend on the parameters or on which network wrote it.
PredImage plan_pred_image(const kr_handle* h, const SimPlan& p, int64_t B) {
  PredImage im;
  im.rows = B * p.W;
  const bool wanted = p.path == 2 ? h->keep_predictor != 0 : h->predictor > 2 && ms_wanted(h, B);
  im.use = wanted && (size_t)im.rows * KR_PRED_IMG_DOUBLES * sizeof(double) <= ((size_t)1 << 30);
  im.load = im.use && h->keep_predictor && h->pred_valid_B == B && h->pred_valid_W == p.W && h->pred_valid_nn == (p.nn ? 1 : 0);
  return im;
}

void note_sim_plan(kr_handle* h, const SimPlan& p, const PredImage& im, int64_t B) {
  h->last_sim_path = p.path;
  h->last_overlap = p.overlap ? 1 : 0;
  h->last_waves_per_rod = p.W;
  if (!im.use) return;
  h->pred_valid_B = p.path ? B : 0;  // (single-shooting steps left the image of an older trajectory in the buffer)
  h->pred_valid_W = p.W;
  h->pred_valid_nn = p.nn ? 1 : 0;
}
void note_step_plan(kr_handle* h, const SimPlan& p) {
  h->last_waves_per_rod = p.W;
  if (p.path == 1) h->last_sim_path = 1;  // (a multiple-shooting kernel took it)
}

template SimPlan plan_step<float>(const kr_handle*, int64_t, int, int, int);
template SimPlan plan_step<double>(const kr_handle*, int64_t, int, int, int);
template SimPlan plan_simulate<float>(const kr_handle*, const PlanQuery&);
template SimPlan plan_simulate<double>(const kr_handle*, const PlanQuery&);

}  // namespace kr
