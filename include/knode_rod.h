/*
 * knode_rod.h - C ABI of libknode_rod.so, the MI355X (gfx950) backend for the
 * KNODE-Cosserat rod hot path.
 *
 * The reference (hsiehScalAR/KNODE-Cosserat) is pure Python and defines no FFI;
 * its "interface" for this path is the duck-typed surface of
 *   knode_cosserat/cosserat_ode.py        (class CosseratRod)
 *   knode_cosserat/cosserat_ode_torch.py  (class CosseratRodTorch)
 *   knode_cosserat/knode.py               (setup_robot, simulate)
 * Every entry point below names the reference function (file:line) it
 * replaces.  The Python shims in knode-cosserat_amd/ bind these symbols with
 * ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.
 *  - every function returns 0 on success, <0 on error (KR_E_*);
 *    kr_last_error() gives the message of the calling thread's last error.
 *  - all array arguments are DEVICE pointers owned by the caller unless the
 *    name ends in _host; `stream` is a hipStream_t passed as void* (NULL = the
 *    null stream).  Calls are asynchronous on that stream.
 *  - one handle per (device, parameter set); a handle is not thread-safe,
 *    distinct handles are.  A handle may be used with several streams from
 *    ONE host thread: its calls share per-handle scratch (predictor images,
 *    resume steps of the two-launch simulate, history workspaces, loss
 *    partials), so a call on another stream than the handle's previous call
 *    is made to wait for everything that call's stream had queued (an event,
 *    no host synchronisation) - calls on one handle never overlap on the
 *    device; use one handle per stream for concurrency.  LIFETIME: the
 *    handle keeps the hipStream_t of its previous call to record that event
 *    on; a stream must therefore stay alive until the handle's NEXT call has
 *    returned (or the handle is destroyed) - destroy streams after the handle
 *    has moved on, not between two of its calls.  The current HIP
 *    device of the calling thread must be the handle's (KR_E_ARG otherwise).
 *  - dtype selects the arithmetic type of the call: KR_F32 or KR_F64.  All
 *    floating-point array arguments of a call have that element type.
 *
 * Rod state in HBM ("packed state", one record per grid point):
 *    state[b][j][KR_SLOTS]     b < B rods, j < N grid points
 *    slot  0.. 2  q   (y rows 13..15)     slot 12..14  p (y rows 0..2)
 *    slot  3.. 5  w   (y rows 16..18)     slot 15..18  h (y rows 3..6)
 *    slot  6.. 8  v   (z rows 0..2)       slot 19..21  n (y rows 7..9)
 *    slot  9..11  u   (z rows 3..5)       slot 22..24  m (y rows 10..12)
 *    slot 25..27  padding (kept zero)
 * The twelve leading slots are exactly what the BDF2 history terms of the next
 * step need (cosserat_ode.py:146-148 uses only q_t, w_t, v_t, u_t), so the
 * solver reads 96 contiguous bytes (fp64) per grid point and writes one
 * 16-byte-aligned record.  kr_state_pack / kr_state_unpack convert from/to
 * the reference's feature-major arrays y[19][N], z[6][N].
 */
#ifndef KNODE_ROD_H
#define KNODE_ROD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KR_SLOTS 28
#define KR_NY 19
#define KR_NZ 6
#define KR_MAX_LAYERS 8

enum { KR_F32 = 0, KR_F64 = 1 };
enum { KR_EULER = 0, KR_RK4 = 1 };
/* activation codes, cosserat_ode.py:99-108 */
enum { KR_ACT_NONE = 0, KR_ACT_TANH = 1, KR_ACT_SOFTPLUS = 2, KR_ACT_RELU = 3, KR_ACT_ELU = 4 };
/* per-rod solver status written by kr_step_batch */
enum { KR_ST_CONVERGED = 0, KR_ST_MAXIT = 1, KR_ST_NONFINITE = 2 };

enum {
  KR_OK = 0,
  KR_E_ARG = -1,     /* bad argument (null pointer, size, enum) */
  KR_E_HIP = -2,     /* HIP runtime error */
  KR_E_STATE = -3,   /* call order (e.g. NN requested but kr_set_mlp never called) */
  KR_E_UNSUPPORTED = -4
};

/* Independent rod parameters, cosserat_ode.py:15-47 (NumPy class) /
 * cosserat_ode_torch.py:14-45 (torch twin).  Matrices are row-major 3x3. */
typedef struct kr_params {
  double L;              /* rod length */
  int32_t N;             /* grid points; segments = N-1; ds = L/(N-1) */
  int32_t nn_input_history; /* 0: MLP input [y,z,tf] (28); 1: [y,yh,z,zh,tf] (53) */
  double E, r, rho;      /* Young's modulus, radius, density */
  double vstar[3];
  double g[3];
  double Bse[9];
  double Bbt[9];
  double C[3];
  double del_t;
  double F_tip[3];
  double M_tip[3];
  double tendon_dirs[12]; /* 4 x 3 */
  double p0[3];
  double h0[4];
  double q0[3];
  double w0[3];
} kr_params;

/* Dependent terms, cosserat_ode.py:58-78; returned so that the Python shim can
 * expose the attributes estimate_state.py and the drivers read. */
typedef struct kr_derived {
  double A, G, ds, c0, c1, c2, rhoA;
  double J[9], Kse[9], Kbt[9];
  double Kse_plus_c0_Bse_inv[9];
  double Kbt_plus_c0_Bbt_inv[9];
  double Kse_vstar[3];
  double rhoAg[3];
  double rhoJ[9];
} kr_derived;

typedef struct kr_handle kr_handle;

/* ---- library / handle ------------------------------------------------- */
const char* kr_last_error(void);
int kr_version(void);
/* fills the struct with the reference's class defaults (cosserat_ode.py:15-47) */
int kr_default_params(kr_params* out);
/* applies knode.setup_robot (knode.py:6-53); mod NULL or "" = no modifier.
 * Unknown mod -> KR_E_ARG, like the reference's exception. */
int kr_apply_preset(kr_params* inout, const char* mod);
/* The legacy ("original") parameter set of knode_cosserat_realworld/prepare.py:35-73
 * (setup_robot_original: del_t 0.005, L 0.4, E 209e9, r 0.0012, rho 8000, Bbt 5e-4 I) with its own
 * modifiers None|nsw|short|damping|diameter|youngs|dampstiff|lengthstiff. */
int kr_apply_preset_original(kr_params* inout, const char* mod);

int kr_create(const kr_params* p, int device, kr_handle** out);
int kr_destroy(kr_handle* h);
/* Solver options (integers):
 *   "ms_mode"        -1 auto (default) / 0 off / 1 forced: multiple-shooting form of the time-step
 *                    kernel (one rod per wavefront, 4 sub-intervals) for small batches
 *   "ms_batch_limit" auto mode uses it when B <= limit (default: no limit - it is the faster kernel at
 *                    every batch size measured; lower it to send large batches to the single-shooting kernel)
 *   "persistent"     1 (default) / 0: kr_simulate_batch runs all steps in one launch when the
 *                    multiple-shooting kernel applies
 *   "waves_per_rod"  0 auto (default) / 1 / 2 / 4: wavefronts that share one rod (7 or 13 sub-intervals instead of 4) -
 *                    for batches that would leave SIMDs idle (B waves_per_rod <= 1024).  With the MLP on: the persistent
 *                    form of kr_simulate_batch only (Euler sweeps, a network the matrix-core evaluator serves).
 *                    "last_waves_per_rod" / "last_sim_path" (read-only) tell what the last call ran.
 *   "mlp_grad_accumulate" 0 (default) / 1: see kr_adam_step
 *   "mlp_grad_ordered" 0 (default) / 1: kr_mlp_backward adds up its per-workgroup partial gradients in a fixed order by
 *     plain stores instead of float atomics: the gradient is then bit for bit the same in every call on the same inputs
 *     (the default's 32 adders per parameter arrive in any order).  Needs a network the fused training kernels serve
 *     (KR_E_UNSUPPORTED otherwise: nothing falls back to the atomics).  krod_grad.weight_grads sets it for its calls.
 *   "keep_predictor" 0 (default) / 1: kr_simulate_batch leaves the state of its start-value predictor behind
 *                    and the next call with the same batch size resumes from it - for a simulation that is
 *                    advanced by several calls, each continuing where the previous one stopped
 *                    (states[0] of a call = the last state of the one before).  Setting it to 0 drops
 *                    the stored state.
 *   "residual_test"  1 (default) / 0: the multiple-shooting kernels may accept a storing sweep from its RESIDUAL alone.
 *                    The documented stopping rule is on the Newton update (|dG|, |dY_i| <= tol max(1, |.|)); forming
 *                    that update costs a condensation.  With the option on, a storing sweep that follows an update
 *                    <= 1e-2 is first judged by amp x |residual|, amp = |update| / |residual| measured at the preceding
 *                    full iteration of the same solve, and accepted when 256 x that estimate is below the tolerance
 *                    (the two residuals point in different directions, so the ratio is only indicative: audited at
 *                    most 39 x off over 8 workloads x 1024 rods x 300 steps - DESIGN.md section 4; the factor 256 is
 *                    the margin).  status still reports "converged"; with 0 every accepted sweep carries a measured
 *                    update (Newton, or chord within 1 %) below the tolerance, at ~5 % of the throughput.
 *   "nn_base_only_store" 1 (default) / 0: MLP on, persistent one-wavefront kernel: a storing sweep that follows an update
 *                    <= 1e-2 evaluates the network at the unperturbed inputs only (no forward-difference columns: half an
 *                    evaluation) and is judged by the residual test above (audited with the MLP on: at most 46 x off) or,
 *                    failing that, by a CHORD update through the factors of the last full sweep - accepted below HALF
 *                    the tolerance, otherwise applied as the iteration's update; after two such sweeps the next one is
 *                    full.  0: every sweep carries its columns (~15 % slower; tools/bo_check.py compares the two).
 *   "nn_lowp_first"  1 (default) / 0: fp64 sweeps, MLP on: the FIRST sweep of a step whose predecessor needed two
 *                    corrections evaluates the network's base chain in fp32 (the accepted state never comes from it).
 *   "overlap"        1 (default) / 0: persistent form only - verify step t on spare lanes of the Jacobian sweep of
 *                    step t + 1 (kr_mso_impl.hpp; Euler sweeps, MLP off, diagonal material matrices)
 *   "msw_overlap"    1 (default) / 0: the same overlap where a rod owns 2 or 4 wavefronts (kr_mswo_impl.hpp; Euler
 *                    sweeps, MLP off, diagonal material matrices; the three tiles of leading slots in the LDS where
 *                    they fit beside the condensation tiles, else read from the states themselves: long rods)
 *   "predictor"      0..8: how kr_simulate_batch may form the initial guess of each step (default 8;
 *                    0 = the reference's warm start).  1..7: highest order of polynomial time
 *                    extrapolation; the persistent kernel picks, rod by rod and step by step, the
 *                    order <= this that would have predicted the step just solved best.  8 adds a
 *                    three-tap linear recurrence fitted per rod to the last steps, used whenever
 *                    it predicted the step just solved better than every polynomial.  One launch
 *                    per step uses min(this, 2).  The guess never changes the solution, only the
 *                    number of Newton sweeps. */
int kr_set_option(kr_handle* h, const char* name, int value);
/* reads an option back; additionally "last_sim_path": what the last kr_simulate_batch did -
 * 0 one single-shooting launch per step, 1 one multiple-shooting launch per step, 2 one
 * persistent launch for all steps */
int kr_get_option(kr_handle* h, const char* name, int* value);
/* Diagnostics (NULL switches them off).  While a buffer is set, kr_simulate_batch with one launch per step
 * writes the number of Newton sweeps of every rod and step into it as int32 [B][T]; in builds with
 * -DKR_MS_STAMPS (make dbg) the persistent kernel fills it as uint64 [B][24] with per-rod cycle counters
 * {total, sweep, algebra, prologue, iterations, ...} instead (tools/ms_stamps.py). */
int kr_debug_buffer(kr_handle* h, void* dev_ptr);
/* CosseratRod.compute_intermediate_terms, cosserat_ode.py:58-78 */
int kr_set_params(kr_handle* h, const kr_params* p);
int kr_get_derived(const kr_handle* h, kr_derived* out);
/* same derivation without a handle or a GPU (host arithmetic only) */
int kr_derive(const kr_params* p, kr_derived* out);

/* Residual MLP, cosserat_ode.py:90-112 / cosserat_ode_torch.py:60-62,131-134.
 * dims[n_layers+1]; W[k] is row-major [dims[k+1]][dims[k]] float32 (the dtype
 * the reference trains and stores), b[k] is [dims[k+1]]; acts[k] is applied
 * after layer k.  src_on_device: 0 = host pointers, 1 = device pointers.
 * The library keeps its own packed copies.  n_layers = 0 switches the MLP off.
 * Lifetime of the sources: host sources (src_on_device = 0) are copied before the call returns.  Device sources
 * (src_on_device = 1) are NOT: the call records their addresses and one pack launch on `stream` reads them, so every W[k]
 * and b[k] must stay valid and unmodified until `stream` has reached that launch - free or overwrite them only by work
 * ordered after it on the same stream (or after synchronising with it).  A caller that pushes live training weights every
 * iteration (krod_grad.simulate_tips_nn) runs the optimizer step on the stream it gave here. */
int kr_set_mlp(kr_handle* h, int n_layers, const int32_t* dims, const int32_t* acts,
               const float* const* W, const float* const* b, int src_on_device, void* stream);

/* CosseratRod.get_nn_output (cosserat_ode.py:90-112) on Q rows:
 * x[Q][dims[0]] -> out[Q][25], row-major, f32 or f64 arithmetic. */
int kr_mlp_eval_batch(kr_handle* h, int64_t Q, const void* x, void* out, int dtype, void* stream);

/* The input Jacobian of the residual MLP (CosseratRod.get_nn_output, cosserat_ode.py:90-112; the network enters the point
 * map as (y_s, z) = f_phys + NN(x), x = [y (19), z_phys (6), tf (3)], cosserat_ode.py:178-184; differentiating the solved
 * step of knode.py:70-100 through it needs dNN/dx at every stored grid point): x[Q][28] -> jac[Q][25][28], row-major,
 * jac[q][o][i] = d NN_o / d x_i at row q.  The chain W3 diag(act'(a2)) W2 diag(act'(a1)) W1 (one hidden layer: W2
 * diag(act'(a1)) W1) is formed on the fp64 matrix cores with the weights in LDS; pre-activations, activation derivatives
 * (tanh, softplus, relu, elu, none) and products are fp64 whatever `dtype`, which is the element type of x and jac only.
 * Shapes served: 28 -> H -> 25 with H <= 512 and 28 -> H1 -> H2 -> 25 with H1, H2 <= 64, any widths in range (padded with
 * zero weights), no activation on the last layer, nn_input_history = 0.
 * One launch, no workspace of the handle, no atomics: a row's result does not depend on the batch it rides in.  A value
 * of x that is not finite (NaN or an infinity) is ordinary input: every entry of that row comes back NaN, the call
 * returns KR_OK.
 * Refusals, each with a message, nothing launched and no output byte written: KR_E_STATE without a network (kr_set_mlp);
 * KR_E_UNSUPPORTED for nn_input_history = 1, a shape outside the two families or an activation on the last layer -
 * nothing falls back to another evaluator; KR_E_ARG for a null handle, x or jac, Q < 1, a bad dtype. */
int kr_mlp_input_jacobian_batch(kr_handle* h, int64_t Q, const void* x, void* jac, int dtype, void* stream);

/* ---- batched per-segment derivative ----------------------------------- */
/* CosseratRodTorch.ODE_parallel (cosserat_ode_torch.py:217-322) and, row by
 * row, CosseratRod.ODE (cosserat_ode.py:114-186).
 * y[Q][19], yh[Q][19], zh[Q][6], tf[Q][3] -> dys[Q][19], z[Q][6], row-major.
 * use_nn != 0 adds the MLP correction (needs kr_set_mlp). */
int kr_ode_batch(kr_handle* h, int64_t Q, const void* y, const void* yh, const void* zh, const void* tf,
                 void* dys, void* z, int use_nn, int dtype, void* stream);

/* Derivatives of the PHYSICS of kr_ode_batch (use_nn = 0), what torch autograd propagates through
 * CosseratRodTorch.ODE_parallel (cosserat_ode_torch.py:264-306) and through the op-by-op graph of
 * CosseratRodTorch.getResidualEuler / ODE (:137-213, :325-367).  fp64 forward-mode differentiation on the
 * device whatever `dtype` (the element type of the arrays).
 *   kr_ode_vjp_batch: cotangents g_dys[Q][19], g_z[Q][6] -> J^T g with respect to y, yh, zh, tf
 *     (g_y[Q][19], g_yh[Q][19], g_zh[Q][6], g_tf[Q][3]; any of the four may be NULL).
 *   kr_ode_jacobian_batch: jac[Q][25][19] = d(dys, z) / dy of every row.
 * cut != 0 reproduces the reference's ODE graph where it differs from the function it evaluates: the quadratic part of
 * the rotation matrix (:159-162) and the quaternion-rate matrix (:185-189) are built with torch.tensor([...]), i.e.
 * as leaves - h is then seen through 2 / (h . h) only, and h_s does not see u.  cut = 0: the complete derivative
 * (ODE_parallel's graph). */
int kr_ode_vjp_batch(kr_handle* h, int64_t Q, const void* y, const void* yh, const void* zh, const void* tf,
                     const void* g_dys, const void* g_z, int cut, void* g_y, void* g_yh, void* g_zh, void* g_tf,
                     int dtype, void* stream);
int kr_ode_jacobian_batch(kr_handle* h, int64_t Q, const void* y, const void* yh, const void* zh, const void* tf,
                          int cut, void* jac, int dtype, void* stream);

/* ---- packed state helpers --------------------------------------------- */
/* knode.py:58-66: straight rod along +z, unit quaternion, v = e3 */
int kr_state_init_straight(kr_handle* h, int64_t B, void* state, int dtype, void* stream);
/* y_fm[B][19][N], z_fm[B][6][N] (reference layout) <-> state[B][N][KR_SLOTS] */
int kr_state_pack(kr_handle* h, int64_t B, const void* y_fm, const void* z_fm, void* state, int dtype, void* stream);
int kr_state_unpack(kr_handle* h, int64_t B, const void* state, void* y_fm, void* z_fm, int dtype, void* stream);
/* rows [y; z; yh; zh] of one knode.simulate trajectory entry (knode.py:96):
 * out[B][50][N] from state (step k) and the two states before it */
int kr_state_unpack50(kr_handle* h, int64_t B, const void* state, const void* state_m1, const void* state_m2,
                      void* out, int dtype, void* stream);
/* tip[B][3] = p of the last grid point */
int kr_state_tip(kr_handle* h, int64_t B, const void* state, void* tip, int dtype, void* stream);

/* ---- shooting residual ------------------------------------------------- */
/* CosseratRod.getResidualEuler / getResidualRK4 (cosserat_ode.py:188-255):
 * one sweep from the guessed base wrench G[B][6]; writes the swept state into
 * state_next (the reference mutates y, z in place) and r[B][6] =
 * [F_tip - n(L), M_tip - m(L)].  History terms come from state_cur, state_prev
 * (knode.py:74-75).  tensions[B][4].
 * hist_is_explicit != 0: state_cur holds the history terms yh, zh themselves
 * (packed like a state) and state_prev is ignored - the calling convention of
 * the reference method, which receives yh, zh as arguments. */
int kr_residual_batch(kr_handle* h, int64_t B, int scheme, const void* G, const void* state_prev,
                      const void* state_cur, void* state_next, const void* tensions, void* r, int use_nn,
                      int hist_is_explicit, int dtype, void* stream);
/* getResidualRK4 with the CALLER'S midpoint histories (cosserat_ode.py:215-255: stages 2 and 3 read
 * yh_int[:, j], zh_int[:, j], lines 225 and 233-234).  hist holds yh, zh and hist_mid holds yh_int, zh_int, both
 * packed like a state ([B][N][KR_SLOTS]; record j of hist_mid belongs to the midpoint between grid points j and
 * j + 1, record N-1 is not read).  hist_mid == NULL gives kr_residual_batch(..., hist_is_explicit = 1), i.e. the
 * linear interpolation knode.simulate hands over (knode.py:80-81).  scheme must be KR_RK4 when hist_mid is given
 * (the Euler sweep ignores the midpoints, cosserat_ode.py:188-213). */
int kr_residual_mid_batch(kr_handle* h, int64_t B, int scheme, const void* G, const void* hist, const void* hist_mid,
                          void* state_next, const void* tensions, void* r, int use_nn, int dtype, void* stream);

/* ---- one implicit time step -------------------------------------------- */
/* Body of the loop in knode.simulate (knode.py:70-100) for B rods: BDF2
 * history from (state_cur, state_prev), shooting solve for G (Newton with a
 * forward-difference Jacobian instead of MINPACK hybrd; same root), final
 * swept state into state_next.  G[B][6] is read as the initial guess and
 * overwritten with the solution.  tol: stop when |dG|_inf <= tol*max(1,|G|_inf)
 * (<=0 selects 1e-8 for f64 - the class of the reference's fsolve xtol=1.49e-8 - and 1e-5 for f32); maxit <= 0 selects 30.
 * status[B], iters[B] (int32) may be NULL.  A step that plain Newton does not solve within maxit sweeps (from the
 * predicted and from the caller's start) is redone by damped Newton with its OWN cap of 8 x maxit sweeps
 * (backtracking rejections count as sweeps); iters reports the sum of both phases.
 * Initial guess: predictor = 0 starts Newton from the caller's G (the
 * reference's warm start, knode.py:89); 1 / 2 extrapolate the unknowns linearly /
 * quadratically in time from state_cur, state_prev (and state_prev2, may be
 * NULL; it may alias state_next, it is read before anything is written);
 * -1 = the highest order the given states allow (prev == cur means "no history").
 * FAILED STEPS.  Values that are not finite are ordinary input, not an error: the call returns KR_OK and every entry of
 * status / iters is written.  A rod whose tensions, states or parameters make its update non-finite reports
 * KR_ST_NONFINITE (a finite input that merely overflows the arithmetic reports KR_ST_NONFINITE or KR_ST_MAXIT), with
 * 1 <= iters <= maxit + 8 maxit - the two caps above; a non-finite update ends either phase at once, and backtracking
 * never runs past its cap on a NaN norm.  Its G and state_next are then the last iterate and its sweep (NaN where the
 * input reached them) and carry no meaning.  Whatever the kernel family (eight rods of single shooting share a
 * wavefront), status, iters, G and state_next of every OTHER rod are bit for bit those of the call without the failing
 * rod's bad values.  Nothing of a failed step stays in the handle: the next call is not affected. */
int kr_step_batch(kr_handle* h, int64_t B, int scheme, const void* state_prev, const void* state_cur,
                  void* state_next, void* G, const void* tensions, double tol, int maxit, int32_t* status,
                  int32_t* iters, int use_nn, const void* state_prev2, int predictor, int dtype, void* stream);

/* T steps of the above in one call.  ctl[B][T][4]; states[(T+1)][B][N][KR_SLOTS]
 * with states[0] the initial condition (e.g. kr_state_init_straight) - step t
 * writes states[t+1]; if ring != 0, `states` holds only 3 slots used
 * cyclically (slot (t+1)%3) for tip-only runs: on return they hold the complete
 * last three states of the call (states T, T-1, T-2); what passes through them
 * before that is scratch of the library (the persistent kernels write interior
 * states only as far as they may have to re-read them: records at the starts of
 * their sub-intervals, and the twelve leading slots when a rod is handed from one
 * kernel to the next).  tip[B][T][3] may be NULL.
 * status[B][T] may be NULL.  Replaces knode.simulate (knode.py:55-102).
 * state_prev_init: NULL = the reference's start (y_prev = y before the first
 * step, knode.py:65-66); otherwise the packed state one step before states[0],
 * which makes a second call continue a run exactly (it may point into the ring).
 * When the multiple-shooting kernel applies (see kr_set_option) all T steps run
 * in ONE launch: every wavefront keeps its rod's history in LDS / registers.
 * FAILED STEPS (this call and its table / bank / loads / boundary / key-point forms).  Values that are not finite are ordinary input: the call
 * returns KR_OK and every entry of status[B][T] is written.  A rod whose inputs stop being finite at step t0 (a NaN
 * tension or tip load of that step; a NaN parameter of its table row: t0 = 0) reports 0 before t0 and KR_ST_NONFINITE at
 * t0, whichever kernel family runs the call; a finite input that overflows the arithmetic reports a nonzero status at
 * t0 (and, entering the sweeps, on every later step).  Its tips and states before t0 (states 0 .. t0) are those of
 * the run without the bad value, bit for bit - the
 * prefetch of step t0's inputs and, in the overlapped kernels, the sweep that carries step t0 next to the verification
 * of step t0 - 1 do not reach back.  From t0 on the rod's outputs carry no meaning: where the bad value enters the
 * sweeps (tensions, parameters other than the tip wrench) the stored states are NaN and every later step reports a
 * nonzero status (KR_ST_NONFINITE in every kernel today; rely on "nonzero").  A tip wrench (loads[b][t0], F_tip / M_tip
 * of a row) enters the tip condition only: the state stored for the failed step is the finite sweep of the last finite
 * iterate, and later steps whose own wrench is finite solve from it and may report 0 again - status 2 at t0 is the
 * only mark that the trajectory from there on is not the rod's.
 * kr_simulate_batch_boundary: a non-finite base value (p0, h0, q0, w0 of bnd[b][t0]) enters the sweeps - the rod reports
 * 0 before t0, KR_ST_NONFINITE at t0 and nonzero afterwards; a non-finite wrench value of bnd[b][t0] behaves as
 * documented for loads; every other rod is bit for bit the clean call.
 * kr_simulate_batch_keypoints: kp follows the states it copies.  Every kp[t][b][k] is written for every rod and step; a
 * rod that fails at t0 has, in kp[0 .. t0 - 1], the clean run's records bit for bit, and from t0 on what its states hold
 * (NaN where the bad value enters the sweeps); every other rod's records are bit for bit those of the clean call.
 * Every OTHER rod's status, tips, G and states are bit for bit those of the call without the bad value, in every kernel
 * family; on a ring its last three states are complete.  Nothing of a failed step stays behind in the handle's scratch,
 * the history workspace or (keep_predictor = 0) the predictor images; with keep_predictor = 1 the failing rod's own
 * image holds its failed steps, the other rods' images are those of the clean run.
 * No kernel reads a state slot, a tip or a status entry before it has written it: what the output buffers hold when
 * the call starts (states[0] excepted) has no influence on any result. */
/* Optional: the host-side one-time work of the first kr_simulate_batch call for batches of B rods (per-batch scratch
 * allocation, kernel lookup in the code object, LDS limits: ~0.4 ms) ahead of time, so that a latency-critical first
 * call does not carry it.  Launches nothing.  No counterpart in the reference. */
int kr_simulate_prepare(kr_handle* h, int64_t B, int dtype);
int kr_simulate_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, void* states, int ring,
                      void* G, void* tip, double tol, int maxit, int32_t* status, int use_nn,
                      const void* state_prev_init, int dtype, void* stream);

/* ---- heterogeneous batches: per-rod parameter tables ------------------- */
/* Every call above takes its rod from the handle: B rods are B copies of one parameter set.  A parameter table gives
 * rod b of a simulate call its own kr_params - the reference's "one true rod, several mismatched models" experiment
 * (knode.setup_robot with its mods, knode.py:6-53, walked one model at a time by physics_multitrain.py), parameter
 * sweeps, system identification, domain randomisation - in ONE launch instead of one handle and one launch per rod.
 *
 * Shared with the handle (a row that differs: KR_E_ARG): N, del_t, nn_input_history.  The MLP is the handle's
 * (kr_set_mlp), one network for all rods.
 * Per rod: every other field of kr_params (L - hence ds -, E, r, rho, vstar, g, Bse, Bbt, C, F_tip, M_tip, tendon_dirs,
 * p0, h0, q0, w0).
 * Served (anything else: KR_E_UNSUPPORTED with a message that names the rule - never a silent fallback to the handle's
 * parameters): diagonal Bse / Bbt on every row (every preset qualifies); scheme KR_EULER; 9 <= N <= 128; MLP off, or an
 * MLP the persistent one-wavefront kernel evaluates; KR_F32 and KR_F64.  Table calls always run one wavefront per rod
 * in one persistent launch (last_sim_path 2, last_waves_per_rod 1): the overlapped kernel with its take-over launch, or
 * the plain persistent kernel for MLP-on and overlap = 0.  Options residual_test, overlap, predictor, keep_predictor,
 * nn_* mean what they mean for kr_simulate_batch; waves_per_rod = 2 / 4, ms_mode = 0 and persistent = 0 are refused.
 * NOT served with a table: several wavefronts per rod, N > 128, single shooting, RK4, full material matrices, one
 * launch per step, kr_step_batch / kr_residual_* / kr_ode_batch, per-rod N / del_t, training (independent trainings of
 * several rod models share an epoch's launches through kr_train_bank_*, below).  A per-rod MLP is served
 * by kr_simulate_batch_bank (below), not by kr_simulate_batch_table. */
typedef struct kr_param_table kr_param_table;

/* Host arithmetic only (no handle, no GPU - like kr_derive): may rods_host[0..B) ride in one launch with `base`?
 * KR_OK, or KR_E_ARG / KR_E_UNSUPPORTED with *bad_rod (nullable) = the first offending row (-1: the fault is not in a
 * row) and kr_last_error() naming the field. */
int kr_param_table_check(const kr_params* base, int64_t B, const kr_params* rods_host, int64_t* bad_rod);
/* Checks the rows against the handle's parameters, derives every row exactly as kr_set_params derives the handle's own
 * constants (fp64, then rounded to fp32) and uploads both precisions.  The table belongs to the handle's device and is
 * immutable; destroy it after the last call that uses it has finished on its stream. */
int kr_param_table_create(kr_handle* h, int64_t B, const kr_params* rods_host, kr_param_table** out);
int kr_param_table_destroy(kr_param_table* t);
/* kr_state_init_straight / kr_simulate_batch with rod b taking row b of the table (B = the table's B). */
int kr_state_init_straight_table(kr_handle* h, const kr_param_table* t, void* state, int dtype, void* stream);
int kr_simulate_batch_table(kr_handle* h, const kr_param_table* t, int64_t T, int scheme, const void* ctl, void* states,
                            int ring, void* G, void* tip, double tol, int maxit, int32_t* status, int use_nn,
                            const void* state_prev_init, int dtype, void* stream);

/* ---- heterogeneous batches: per-rod networks (banks) ------------------- */
/* The reference's model-mismatch experiment does not run one network for all models: for every mod it calls
 * setup_robot(robot, mod) and then loads THAT model's own trained network from saved_models/..._{mod}_..._{seed}.pth
 * before it simulates, for every seed (physics_multitrain.py:181-199).  A bank holds K networks of ONE shape;
 * kr_simulate_batch_bank runs rod b with row b of a parameter table and network net_of_rod[b] of the bank - the
 * (mod, seed) grid, a seed sweep, a checkpoint comparison or an ensemble in ONE launch instead of one kr_set_mlp and
 * one launch per network.
 *
 * Shared by all K networks: n_layers, dims, acts (what a wavefront needs of its network then is one base address).
 * Served (anything else: KR_E_UNSUPPORTED with a message that names the rule - never served from the handle's own
 * MLP): what kr_simulate_batch_table serves with the MLP on - scheme KR_EULER; 9 <= N <= 128; diagonal material
 * matrices (the table's rule); nn_input_history = 0; a shape the persistent one-wavefront kernel evaluates
 * (28 -> H -> 25, or 28 -> H1 <= 64 -> H2 <= 192 -> 25 with one activation on both hidden layers; no output
 * activation; option mfma_mlp on); the rod fits the LDS; KR_F32 and KR_F64.  A bank call always runs one wavefront per
 * rod in one persistent launch (last_sim_path 2, last_waves_per_rod 1, last_overlap 0).  Options residual_test,
 * predictor, keep_predictor, nn_* mean what they mean for kr_simulate_batch_table; waves_per_rod = 2 / 4,
 * ms_mode = 0 and persistent = 0 are refused.
 * NOT served with a bank: RK4, several wavefronts per rod, N > 128, single shooting, kr_ode_batch / kr_step_batch,
 * networks of differing shape in one bank, training (kr_train_bank_*, below, trains K networks in one call per epoch).
 * The handle's own MLP (kr_set_mlp) is neither read nor changed by a bank or a bank call. */
typedef struct kr_mlp_bank kr_mlp_bank;

/* Host arithmetic only (no handle, no GPU - like kr_param_table_check): is a bank of K networks of this one shape
 * served for rods with the shared fields of `base` (N, nn_input_history)?  KR_OK, KR_E_ARG (K < 1, a malformed shape)
 * or KR_E_UNSUPPORTED with kr_last_error() naming the rule. */
int kr_mlp_bank_check(const kr_params* base, int K, int n_layers, const int32_t* dims, const int32_t* acts);
/* W, b: K * n_layers pointers, network-major (W[k * n_layers + l] = layer l of network k), each laid out as for
 * kr_set_mlp; src_on_device as there.  Every network is packed exactly as kr_set_mlp packs the handle's own (the same
 * gather plan, the same kernel): entry k is bit-identical to what kr_set_mlp would have produced for network k.  The
 * K packed images lie a constant stride apart in one allocation.
 * Source lifetime: the bank has finished reading W and b - host or device - when this call returns (it synchronises
 * `stream`); the caller may free or overwrite them at once.
 * The bank belongs to the handle's device and is changed only by kr_mlp_bank_repack, ordered on its stream; it may be
 * used with any handle on that device.  Destroy it after the last call that uses it has finished on its stream. */
int kr_mlp_bank_create(kr_handle* h, int K, int n_layers, const int32_t* dims, const int32_t* acts,
                       const float* const* W, const float* const* b, int src_on_device, void* stream,
                       kr_mlp_bank** out);
int kr_mlp_bank_destroy(kr_mlp_bank* bank);
/* In-place refresh: packs K = the bank's K networks of the bank's shape into the existing bank (W, b as for
 * kr_mlp_bank_create: K * n_layers pointers, network-major), with the gather plan and the kernel creation used - the
 * result is bit-identical to a fresh kr_mlp_bank_create from the same weights.  Allocates nothing.  With
 * src_on_device = 1 it does not synchronise: the pack launches are ordered on `stream` like any other call, a simulate
 * call queued behind it on the handle sees the new weights, one queued before it the old ones, and the sources must
 * stay unchanged until the launches have run.  With host sources the call returns when they have been read.
 * This is how live weights of a training reach a closed-loop evaluation (physics_train.py:136-167: evaluate() every
 * 50 epochs) without a host copy.  KR_E_ARG: a NULL among the K * n_layers pointers (named), a bank of another device. */
int kr_mlp_bank_repack(kr_handle* h, kr_mlp_bank* bank, const float* const* W, const float* const* b, int src_on_device,
                       void* stream);
/* kr_simulate_batch_table with the MLP on (there is no use_nn), rod b evaluating network net_of_rod_host[b].
 * net_of_rod_host: HOST array of B = the table's B entries.  Every entry is range-checked on the host BEFORE anything
 * is copied or launched (KR_E_ARG naming the first bad rod; no output buffer is touched), then the array is copied to
 * the device: the kernel never sees an index outside [0, K).  The array has been read when the call returns.
 * t is required: build a table of identical rows when only the networks vary. */
int kr_simulate_batch_bank(kr_handle* h, const kr_param_table* t, const kr_mlp_bank* bank,
                           const int32_t* net_of_rod_host, int64_t T, int scheme, const void* ctl, void* states,
                           int ring, void* G, void* tip, double tol, int maxit, int32_t* status,
                           const void* state_prev_init, int dtype, void* stream);
/* The evaluation half of the reference's experiment rolls every trained network out and scores it at key points
 * against a recorded run (physics_multitrain.py:180-233), and does the same during training to pick the best weights
 * (physics_train.py:136-167).  kr_simulate_batch_bank_keypoints is kr_simulate_batch_bank in which rod b also solves
 * step t with bnd[b][t] - the KR_BND values, meaning exactly what they mean for kr_simulate_batch_boundary (below) -
 * and which writes kp[T][B][K][KR_SLOTS] exactly as kr_simulate_batch_keypoints (below) does: a grid of trained
 * networks scored from K records per step instead of the full history, under a tip disturbance or on a moving base.
 * K may be 0 HERE, with idx_host and kp both NULL: the bank form of the boundary call (kr_keypoints_check itself keeps
 * refusing K = 0).  For K >= 1 the rule for idx_host is kr_keypoints_check's and kp must be 16-byte aligned.
 * t, bank, net_of_rod_host and bnd are required.  Every argument check - NULLs, the network index range, the idx rule,
 * a table that does not match the handle - and every refusal of the planner is made on the host BEFORE anything is
 * copied or launched: KR_E_ARG naming the first bad entry, or KR_E_UNSUPPORTED naming the rule; no output buffer is
 * touched.  ring, state_prev_init, keep_predictor, a call cut into pieces (bnd sliced like ctl, kp like tip), failed
 * steps and last_sim_path / last_waves_per_rod / last_overlap = 2 / 1 / 0 are as for the two parents.
 * Served and refused: exactly as kr_simulate_batch_bank, with messages that name this call. */
int kr_simulate_batch_bank_keypoints(kr_handle* h, const kr_param_table* t, const kr_mlp_bank* bank,
                                     const int32_t* net_of_rod_host, int64_t T, int scheme, const void* ctl,
                                     const void* bnd, int K, const int32_t* idx_host, void* kp, void* states, int ring,
                                     void* G, void* tip, double tol, int maxit, int32_t* status,
                                     const void* state_prev_init, int dtype, void* stream);

/* ---- per-step tip loads: a wrench history per rod ---------------------- */
/* Every simulate call above freezes the tip wrench for the whole call (the handle's F_tip / M_tip, or the rod's table
 * row).  In the reference the wrench is a pair of plain attributes (cosserat_ode.py:28-29) that getResidualEuler reads
 * at every solve (:206-207): a caller who picks up a payload, pushes against the tip or probes a trained model under a
 * disturbance assigns robot.F_tip / robot.M_tip between two steps of knode.simulate's loop.  Here that history is a
 * second time-varying input next to ctl, and the whole experiment - heterogeneous rods included - stays one launch.
 *
 * kr_simulate_batch_table with the tip wrench of every rod and step given like ctl:
 * loads[B][T][6] = F_tip (3), M_tip (3).  The solve of step t (the one that reads ctl[b][t] and writes states[t+1])
 * uses loads[b][t] in its tip condition r = [F - n(L), M - m(L)] - the reference with robot.F_tip / robot.M_tip
 * assigned before that solve.  The values REPLACE F_tip / M_tip of the rod's table row (they are not added to them);
 * everything else of the row is used as in kr_simulate_batch_table.  Element type = dtype, like ctl.  A call cut into
 * pieces (state_prev_init, keep_predictor) slices loads like ctl.
 * t is required (KR_E_ARG without it, or without loads): build a table of identical rows when only the loads vary.
 * Served: exactly what kr_simulate_batch_table serves - one wavefront per rod in one persistent launch; scheme
 * KR_EULER; 9 <= N <= 128; diagonal material matrices; MLP off (the overlapped kernel with its take-over launch, or
 * with overlap = 0 the plain persistent kernel) or the handle's MLP where that kernel evaluates it; KR_F32 and KR_F64;
 * ring, state_prev_init and the options keep_predictor, residual_test, predictor, nn_* as there.  Afterwards
 * last_sim_path = 2, last_waves_per_rod = 1, last_overlap as for the table call.  Everything the table call refuses is
 * refused here with KR_E_UNSUPPORTED and a message that names the rule; no output buffer is touched.
 * NOT served with loads: a network bank (kr_simulate_batch_bank_keypoints takes the wrench in bnd), several wavefronts per rod, N > 128, RK4, one launch per step, kr_step_batch
 * (per-step launches take their wrench from kr_set_params).  A distributed load along the rod is outside this call
 * (a moving base: kr_simulate_batch_boundary below).  The first call of a shape does the one-time host work kr_simulate_prepare does for
 * kr_simulate_batch itself. */
int kr_simulate_batch_loads(kr_handle* h, const kr_param_table* t, int64_t T, int scheme, const void* ctl,
                            const void* loads, void* states, int ring, void* G, void* tip, double tol, int maxit,
                            int32_t* status, int use_nn, const void* state_prev_init, int dtype, void* stream);

/* ---- per-step boundary data: a moving base per rod --------------------- */
/* The other half of the boundary data.  Every simulate call above freezes the base of the rod for the whole call: p0,
 * h0, q0, w0 come from the handle or from the rod's table row.  In the reference they are plain attributes
 * (cosserat_ode.py:44-47) that getResidualEuler reads at every solve (:194), exactly as it reads F_tip / M_tip: a
 * caller whose rod sits on a moving platform, on a carriage or at the wrist of an arm assigns them between two steps of
 * knode.simulate's loop (a base velocity q0 / w0 with a base that never moves is not a motion).
 *
 * kr_simulate_batch_loads with bnd[B][T][KR_BND] in place of loads: per rod and step p0 (3), h0 (4), q0 (3), w0 (3),
 * F_tip (3), M_tip (3) - base and wrench in ONE array (the kernels have one pointer and one layout; a caller without a
 * wrench history repeats the row's F_tip / M_tip in the last six columns).  The solve of step t (the one that reads
 * ctl[b][t] and writes states[t+1]) uses bnd[b][t] for the base state and the tip condition - the reference with the
 * six attributes assigned before that solve.  The values REPLACE those of the rod's row (they are not added to them),
 * and h0 is NOT normalised, as in the reference.  Record 0 of states[t+1] then holds p0, h0, q0, w0 of step t exactly.
 * states[0] is the caller's and need not agree with bnd[b][0] (the reference starts from the straight rod in the same
 * way).  Element type = dtype, like ctl.  A call cut into pieces (state_prev_init, keep_predictor) slices bnd like ctl.
 * t and bnd are required (KR_E_ARG without either).
 * Served and refused: exactly as kr_simulate_batch_loads, with messages that name this call; no output buffer of a
 * refused call is touched.  Afterwards last_sim_path = 2, last_waves_per_rod = 1, last_overlap as for the table call.
 * Deriving q0 / w0 from a pose history is the caller's: the values are used as given, consistent or not.
 * Failed steps: see FAILED STEPS at kr_simulate_batch. */
#define KR_BND 19 /* p0 (3), h0 (4), q0 (3), w0 (3), F_tip (3), M_tip (3): the order of the cold block */
int kr_simulate_batch_boundary(kr_handle* h, const kr_param_table* t, int64_t T, int scheme, const void* ctl,
                               const void* bnd, void* states, int ring, void* G, void* tip, double tol, int maxit,
                               int32_t* status, int use_nn, const void* state_prev_init, int dtype, void* stream);

/* ---- key-point records: states at chosen grid points from a tip-only run -- */
/* A simulate call returns the full history (states[T + 1][B][N][KR_SLOTS]: 22.9 MB per step at B = 1024, N = 100, fp64)
 * or, on a 3-slot ring, the tip positions and the last three states; interior steps of a ring run leave only the records
 * at the starts of the kernel's sub-intervals (leading slots are written when a rod is handed over).  What is computed from a trajectory - the metrics below (kr_dtw_batch,
 * kr_pose_mse_points_batch), the reference's key points ([3, 5, 7, 9], [2, 6, 9], markers [1, 3, 6, 9]), a tip
 * orientation - needs the states at a few grid points for every step.
 *
 * kr_simulate_batch_boundary with one more output, kp[T][B][K][KR_SLOTS]: kp[t][b][k] is the complete record, pad zeros
 * included, of grid point idx[k] of the state step t writes - what a full-history call leaves in states[t + 1][b][idx[k]],
 * bit for bit, on a ring as with the full history.  Element type = dtype; kp must be 16-byte aligned.
 * idx_host: K grid points on the HOST, 1 <= K <= KR_KEYPOINTS_MAX, strictly increasing, each in [0, N) (the kernels find
 * the place of a marked point by counting the marked points below it).  Anything else: KR_E_ARG with a message that names
 * the first bad entry, decided on the host before anything is copied or launched; no output buffer is touched.
 * kr_keypoints_check applies the same rule without a handle (host arithmetic only, like kr_param_table_check).
 * t, bnd and kp are required (KR_E_ARG without one); a caller with a fixed boundary repeats the row's p0 h0 q0 w0 F_tip
 * M_tip on every step, as advised above.  tip, status, G, states (ring or full), keep_predictor and state_prev_init mean
 * what they mean for the boundary call; a call cut into pieces slices kp like tip (kp is time-major: a piece of n steps
 * from step t0 writes kp + t0 * B * K * KR_SLOTS).  A sweep that is later rejected has written its key points and the
 * sweep that replaces it overwrites them, like the tip: nothing of a rejected sweep stays in kp.
 * Served and refused: exactly as kr_simulate_batch_boundary, with messages that name this call; no output buffer of a
 * refused call is touched.  Afterwards last_sim_path = 2, last_waves_per_rod = 1, last_overlap as for the table call.
 * A network bank: served by kr_simulate_batch_bank_keypoints (above).  NO key-point form: several wavefronts per rod,
 * N > 128, RK4, one launch per step.
 * Failed steps: see FAILED STEPS at kr_simulate_batch. */
#define KR_KEYPOINTS_MAX 16
int kr_keypoints_check(int N, int K, const int32_t* idx_host);
int kr_simulate_batch_keypoints(kr_handle* h, const kr_param_table* t, int64_t T, int scheme, const void* ctl,
                                const void* bnd, int K, const int32_t* idx_host, void* kp,
                                void* states, int ring, void* G, void* tip, double tol, int maxit, int32_t* status,
                                int use_nn, const void* state_prev_init, int dtype, void* stream);

/* ---- KNODE one-step-ahead training path -------------------------------- */
/* CosseratRodTorch.parallelGetNextSegmentEuler (cosserat_ode_torch.py:401-437)
 * and, with idx = 1..N-1, getNextSegmentEuler (:370-399), plus the four-term
 * loss of physics_train.py:252-259.  Defined in round 1 as three calls so that
 * torch autograd only sees dense tensors:
 *
 * kr_next_segment_physics: for every (s, k): j = idx[k]-1, row = s*K+k
 *    x[row][in_pad]   MLP input  [y_j, z_phys, tf] (or the 53-wide history form), zero padded
 *    base[row][25]    [y_j + ds*ys_phys, z_phys]    (prediction without the MLP)
 * Gs[S][25][N], yh[S][19][N], zh[S][6][N] feature-major (reference layout),
 * tensions[S][4], idx[K] int32 on device. f32 or f64. */
int kr_next_segment_physics(kr_handle* h, int64_t S, int K, const void* Gs, const void* yh, const void* zh,
                            const void* tensions, const int32_t* idx, void* x, int in_pad, void* base,
                            int dtype, void* stream);

/* MLP forward over Q rows on the matrix cores (fp32 MFMA: exact fp32, the
 * reference's training precision): out[Q][32] (columns 0..dims[n_layers]-1 valid -
 * 25 for the rod's MLP, at most 32 - the rest zero) = MLP(x[Q][in_pad]); keeps pre-activations and activations of
 * the hidden layers in `ws` (kr_mlp_ws_bytes) for the backward pass.  Weights
 * are the caller's device tensors (torch parameters), row-major like nn.Linear:
 * W[k][dims[k+1]][dims[k]], b[k][dims[k+1]]; acts[n_layers-1] must be NONE. */
size_t kr_mlp_ws_bytes(int n_layers, const int32_t* dims, int64_t Q);
int kr_mlp_forward(kr_handle* h, int64_t Q, int n_layers, const int32_t* dims, const int32_t* acts,
                   const float* const* W, const float* const* b, const float* x, int in_pad, float* out,
                   void* ws, void* stream);
/* dW[k], db[k] (overwritten) from dout[Q][32] = d loss / d out and the `ws` of
 * the matching forward call. */
int kr_mlp_backward(kr_handle* h, int64_t Q, int n_layers, const int32_t* dims, const int32_t* acts,
                    const float* const* W, const float* x, int in_pad, const float* dout, const void* ws,
                    float* const* dW, float* const* db, void* stream);

/* pred[row][25] = base + [ds*out[:19], out[19:]] (row = s*K + k); four-term
 * loss of physics_train.py:252-259 against target[S][25][N] at columns idx[k]
 * (z rows against idx[k]-1, :259): for every s the sum of four nn.MSELoss
 * (mean) terms - p rows, n/m/q/w rows, quaternion_to_euler(h rows), z rows -
 * summed over s and divided by `denom`.  Writes pred, *loss and
 * dout[row][32] = d loss / d out (columns 25..31 zero).  out is [rows][32]. */
int kr_loss_fwd_bwd(kr_handle* h, int64_t S, int K, const float* base, const float* out, const float* target,
                    const int32_t* idx, double denom, float* pred, float* loss, float* dout, void* stream);

/* torch.optim.Adam (amsgrad off) on one flat fp32 parameter vector - physics_train.py:199,289-296 - followed by
 * the reference's clamp (physics_train.py:299-304: params = max(params, lower), lower[i] = 0 for weight-matrix
 * entries and -inf for biases; NULL = no clamp) and by zeroing grads[0 .. n_zero) for the next epoch
 * (n_zero >= n covers trailing slots of the same buffer, e.g. the loss).  step = 1, 2, ... (bias correction).
 * With the option "mlp_grad_accumulate" = 1, kr_mlp_backward and kr_loss_rows_fwd_bwd add into dW / db / loss
 * instead of zeroing them first, so that this call is the only one that touches the buffers between epochs. */
int kr_adam_step(kr_handle* h, int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                 const float* lower, double lr, double beta1, double beta2, double eps, double weight_decay,
                 int64_t step, int64_t n_zero, void* stream);
/* kr_adam_step with the learning rate and torch.optim.lr_scheduler.ReduceLROnPlateau(mode "min", relative
 * threshold, cooldown 0) kept on the DEVICE - physics_train.py:206 creates the scheduler, :296-297 call
 * optimizer.step(); scheduler.step(total_loss) every epoch - so that an epoch needs no host round trip.
 * sched: 6 doubles in device memory, initialised by the caller to {lr, lr, +inf, 0, 0, 0}: [0]/[1] learning rate
 * of odd / even steps (step s uses sched[(s-1)&1], the rate of step s+1 goes to sched[s&1]), [2] best loss,
 * [3] bad epochs in a row, [4] loss of the step just taken, [5] reductions so far.  The loss is read from
 * grads[loss_index] (the trailing slot of the flat buffer, already all-reduced) before that slot is zeroed;
 * loss_log (nullable, device) receives it as a float.  Note: the fp32 step size is formed as lr * (1 / bias
 * correction) on the device; kr_adam_step forms lr / bias correction on the host - the same to rounding. */
int kr_adam_plateau_step(kr_handle* h, int64_t n, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                         const float* lower, double* sched, double beta1, double beta2, double eps,
                         double weight_decay, int64_t step, int64_t n_zero, int64_t loss_index, double factor,
                         int patience, double threshold, double min_lr, float* loss_log, void* stream);

/* ONE EPOCH of the one-step-ahead training loop on one rank - the body of physics_train.py:283-304 / :388-401 for the
 * epoch's whole data set: prediction of every scored row from the MLP, the four-term loss, loss.backward() restricted to
 * the MLP, optimizer.step() (Adam), scheduler.step(total_loss) (ReduceLROnPlateau), the weight clamp - as 3 kernel launches
 * (forward + loss, backward, optimizer tail) and no host round trip.  It is kr_mlp_forward_loss + kr_mlp_backward +
 * kr_adam_plateau_step with the glue between them removed: the loss partials and the per-workgroup gradient slabs are
 * added up inside the optimizer launch (fixed order, no atomics: an epoch is reproducible bit for bit), and that launch
 * also writes every updated parameter into the MFMA fragment buffers of `ws`, so the next epoch starts without a packing
 * launch.
 *   params, grads, exp_avg, exp_avg_sq, lower: flat fp32 vectors in nn.Linear order W1 [out][in], b1, W2, b2, (W3, b3);
 *   grads has ONE trailing slot (the loss) and must be zero on entry of phase 0 / 1 (every update leaves it so);
 *   x [S*K][in_pad], base, target_rows [S*K][25], dout [S*K][32] (scratch), ws (kr_mlp_ws_bytes), sched, the Adam and
 *   plateau arguments, step, loss_log: as in kr_mlp_forward_loss and kr_adam_plateau_step.
 *   phase 0: the whole epoch.  phase 1: everything up to the update - grads then holds the summed gradients and the loss,
 *   ready for a data-parallel all-reduce - and phase 2: the update from grads as they stand (after the all-reduce).
 *   repack != 0: the caller changed `params` since the last call (a loaded checkpoint): fragments are packed afresh.
 *   They are also packed whenever ws, params or the network differ from the handle's previous call, and after any
 *   kr_mlp_forward[_loss] / kr_adam[_plateau]_step on the same ws / params.  "Differ" is judged by ADDRESS: a ws or
 *   params buffer that was freed and allocated again at the same address with other contents needs repack = 1 on its
 *   first call (a trainer object passes it on its first epoch).
 * KR_E_UNSUPPORTED for networks the fused training kernels do not serve (use the three separate calls). */
int kr_train_epoch(kr_handle* h, int64_t S, int K, int n_layers, const int32_t* dims, const int32_t* acts, float* params,
                   float* grads, float* exp_avg, float* exp_avg_sq, const float* lower, double* sched, const float* x,
                   int in_pad, const float* base, const float* target_rows, double denom, float* dout, void* ws,
                   double beta1, double beta2, double eps, double weight_decay, int64_t step, double factor,
                   int patience, double threshold, double min_lr, float* loss_log, int phase, int repack, void* stream);
/* n_epochs consecutive epochs of phase 0 queued by ONE call (the loop of physics_train.py:306-408 on one rank): epoch e runs
 * as kr_train_epoch(..., step + e, ..., loss_log + e, phase 0, repack for e = 0 only) - same launches, same results bit for
 * bit; what it saves is the caller's per-epoch host work (a Python / ctypes caller needs longer to issue an epoch than the
 * GPU to run it: 135 us against 128 at BASELINE cfg3).  loss_log must hold n_epochs floats (or be NULL). */
int kr_train_epochs(kr_handle* h, int64_t n_epochs, int64_t S, int K, int n_layers, const int32_t* dims, const int32_t* acts,
                    float* params, float* grads, float* exp_avg, float* exp_avg_sq, const float* lower, double* sched,
                    const float* x, int in_pad, const float* base, const float* target_rows, double denom, float* dout, void* ws,
                    double beta1, double beta2, double eps, double weight_decay, int64_t step, double factor, int patience,
                    double threshold, double min_lr, float* loss_log, int repack, void* stream);

/* ---- banks of trainings: n_nets independent KNODE trainings per epoch call ---- */
/* The reference trains a grid of networks, not one: physics_multitrain.py:140-157 starts one physics_train.py process
 * per (data set, model variant, seed), each running the epoch loop of physics_train.py:306-408 on its own imperfect rod
 * model, two processes at a time.  At the reference's own size (train_len 30, 4 key points: 116 rows) an epoch of
 * kr_train_epoch occupies 1 and then 8 of the chip's 256 compute units, three launches in a row.  A bank of trainings
 * runs n_nets such trainings in the SAME three launches per epoch, training k in blockIdx.y = k of every kernel.
 *
 * Shared by all trainings: the network shape (n_layers, dims, acts), K, in_pad, denom (the loss weights depend on K and
 * denom only), the Adam and plateau constants and the step count.
 * Per training: everything in kr_train_bank_net - parameters, gradients, moments, the clamp, the schedule (the learning
 * rate lives in sched: every training has its own plateau history), the data rows (S may differ between trainings), ds
 * of the rod model that produced them, the loss log.
 * Served: exactly what kr_train_epoch serves in phase 0 with the LDS-resident forward kernels - 28 -> H1 <= 512 -> 25 and
 * 28 -> H1 <= 64 -> H2 <= 64 -> 25, one activation on the hidden layers, none after the last, in_pad 32, n_nets <= 65535.
 * Anything else: KR_E_UNSUPPORTED, or KR_E_ARG for malformed input, with kr_last_error() naming the rule and the first
 * offending network; nothing is launched and no buffer is touched.
 * Result: training k performs the arithmetic of kr_train_epoch(s) on the same buffers in the same order (its row blocks
 * are dealt out over the workgroups kr_train_epoch would launch for its S alone) - params, moments, sched and the logged
 * losses are bit-identical to the training run alone.
 * NOT served with a bank of trainings: phases 1 / 2 (data parallel), networks of differing shape, the generic GEMM path
 * (other shapes, two-layer networks with H1 > 512), S = 0.
 * The bank owns its scratch (weight fragments, activation images, gradient slabs, loss partials, dout) in one device
 * allocation sized from each training's real need; it neither reads nor changes the handle's own training state, and
 * calls are ordered on the handle like every other call. */
typedef struct kr_train_bank kr_train_bank;
typedef struct kr_train_bank_net {      /* one training; all pointers DEVICE, owned by the caller */
  int64_t S;                            /* window steps x trajectories of THIS training; rows = S * K */
  double  ds;                           /* arc-length step of the rod that produced x / base (kr_get_derived().ds) */
  float *params, *grads, *exp_avg, *exp_avg_sq;   /* as kr_train_epoch; grads has its trailing loss slot, zero on entry */
  const float* lower;                   /* nullable */
  double* sched;                        /* 6 doubles, as kr_adam_plateau_step */
  const float *x, *base, *target_rows;  /* [S*K][in_pad], [S*K][25], [S*K][25] */
  float* loss_log;                      /* nullable; epoch e of a call writes loss_log[log_offset + e] */
} kr_train_bank_net;

/* Host arithmetic only (no handle, no GPU - like kr_param_table_check): may these trainings ride in one bank?  KR_OK, or
 * KR_E_ARG / KR_E_UNSUPPORTED with kr_last_error() naming the rule and, where the fault is in a row, the network. */
int kr_train_bank_check(int n_nets, const kr_train_bank_net* nets_host, int K, int n_layers,
                        const int32_t* dims, const int32_t* acts, int in_pad, double denom);
/* kr_train_bank_check, then allocates the bank's scratch and writes the per-training kernel arguments to the device
 * (synchronous copies; nothing is launched).  The pointers of nets_host are kept: the buffers must outlive the bank.
 * nets_host itself has been read when the call returns.  Destroy the bank after its last call has finished. */
int kr_train_bank_create(kr_handle* h, int n_nets, const kr_train_bank_net* nets_host, int K, int n_layers,
                         const int32_t* dims, const int32_t* acts, int in_pad, double denom, kr_train_bank** out);
/* n_epochs epochs of every training, queued as n_epochs x 3 launches; epoch e uses step + e and logs to
 * loss_log[log_offset + e].  The first call on a bank packs the weight fragments from params (one more launch);
 * repack != 0 packs again (the caller wrote some params from outside, e.g. loaded a checkpoint) - later epochs rely on
 * the tail's own fragment update, as kr_train_epoch does.  Arguments are checked before anything is queued. */
int kr_train_bank_epochs(kr_handle* h, kr_train_bank* bank, int64_t n_epochs, int64_t step, double beta1, double beta2,
                         double eps, double weight_decay, double factor, int patience, double threshold, double min_lr,
                         int64_t log_offset, int repack, void* stream);
int kr_train_bank_destroy(kr_train_bank* bank);

/* The same loss against pre-gathered targets: the states a training set is scored against never
 * change between epochs, so kr_gather_targets extracts rows[S*K][25] once (y rows at column idx[k],
 * z rows at idx[k]-1) and kr_loss_rows_fwd_bwd reads them contiguously.  pred may be NULL. */
int kr_gather_targets(kr_handle* h, int64_t S, int K, const float* target, const int32_t* idx, float* rows,
                      void* stream);
int kr_loss_rows_fwd_bwd(kr_handle* h, int64_t S, int K, const float* base, const float* out,
                         const float* target_rows, double denom, float* pred, float* loss, float* dout,
                         void* stream);

/* kr_mlp_forward followed by kr_loss_rows_fwd_bwd (pred = NULL) over the Q = S*K rows of a training set in ONE
 * call - physics_train.py:250-259 / 345-352 from the MLP inputs to the loss and d loss / d out.  Where the fused
 * kernels serve the network the loss runs in the epilogue of the forward kernel (the MLP outputs never reach HBM);
 * otherwise the two kernels run back to back through `out` ([Q][32] scratch, always required).  Same meaning of
 * loss / dout / the option "mlp_grad_accumulate" as kr_loss_rows_fwd_bwd; ws as for kr_mlp_forward. */
int kr_mlp_forward_loss(kr_handle* h, int64_t S, int K, int n_layers, const int32_t* dims, const int32_t* acts,
                        const float* const* W, const float* const* b, const float* x, int in_pad, const float* base,
                        const float* target_rows, double denom, float* out, float* loss, float* dout, void* ws,
                        void* stream);

/* Full-state estimate from measured poses, knode_cosserat_realworld/estimate_state.py:158-242 (with compute_v_u
 * :48-95, compute_angular_velocities :97-123, compute_internal_forces_and_moments :126-156): data[T][7][N]
 * (positions, quaternions at the handle's N grid points), tensions[T][4] -> est[T][25][N], fp64, device pointers.
 * ws: kr_estimate_ws_bytes(T, N) bytes of device scratch.  Uses the handle's parameters (L, del_t, C, Bse, Bbt, ...). */
size_t kr_estimate_ws_bytes(int64_t T, int N);
int kr_estimate_state(kr_handle* h, int64_t T, const double* data, const double* tensions, double* est, void* ws,
                      void* stream);

/* ---- evaluation metrics of a batch ------------------------------------- */
/* What the reference's drivers compute on the host from every simulated trajectory, one rod at a time
 * (physics_multitrain.py:213-222, physics_train.py:136-167), as device kernels that read the packed states where a
 * simulate call left them: two doubles per rod come back instead of a trajectory.
 * All metric arithmetic is fp64 whatever `dtype`, which is only the element type of the inputs; outputs are double.
 * The calls use none of the handle's scratch; kr_pose_mse_batch takes N from the handle, kr_pose_mse_points_batch
 * and kr_dtw_batch read no parameter at all.
 * Two tip metrics: kr_dtw_batch, the exact DTW, and kr_fastdtw_batch, FastDTW - what the reference calls
 * (fastdtw(a, b)[0], radius 1) - whose warp path is traced back on every level of its pyramid on the device.  The
 * exact distance is the quantity FastDTW approximates and a lower bound of it; the two differ on a good share of
 * ordinary paths.  Parity of krod_eval's statement of FastDTW with the third-party package stays unpinned
 * (krod_eval.py): kr_fastdtw_batch is bit-identical to krod_eval, whatever that parity is. */
#define KR_DTW_MAX_LEN 4096

/* Exact dynamic-time-warping distance, L1 point distance, between 3-vectors - what
 * krod_eval.dtw_distance(a, b) computes (the metric of physics_multitrain.py:213 / physics_train.py:159
 * without FastDTW's coarse-path restriction).  Sample i of rod b of sequence a is the 3 consecutive elements at
 * a + b*a_rod_stride + i*a_step_stride (strides in ELEMENTS, >= 0; rod stride 0 = one sequence shared by all rods).
 * This reads simulate's tip[B][T][3] (rod T*3, step 3) and equally one grid point of a full state history
 * states[T+1][B][N][KR_SLOTS] (pointer to slot 12 of that point in states[0]; rod N*KR_SLOTS, step B*N*KR_SLOTS),
 * or one key point of kp[T][B][K][KR_SLOTS] (pointer to slot 12 of kp[0][0][k]; rod K*KR_SLOTS, step B*K*KR_SLOTS).
 * dist[B].
 * The recurrence is cost = (|dx| + |dy|) + |dz|, D = cost + min(min(up, left), diag) in exactly this order: the
 * result is bit-identical to krod_eval.dtw_distance on the same (upcast) samples.  A NaN sample is not propagated the
 * way NumPy's minimum does.  Nothing but the Ta, Tb samples of each rod is read.
 * 1 <= Ta, Tb <= KR_DTW_MAX_LEN; longer: KR_E_UNSUPPORTED, nothing is launched and dist is left untouched.
 * One wavefront per rod; no scratch in global memory. */
int kr_dtw_batch(kr_handle* h, int64_t B,
                 const void* a, int64_t Ta, int64_t a_rod_stride, int64_t a_step_stride,
                 const void* b, int64_t Tb, int64_t b_rod_stride, int64_t b_step_stride,
                 double* dist, int dtype, void* stream);

/* FastDTW (S. Salvador, P. Chan 2007), L1 point distance between 3-vectors, as krod_eval._fastdtw states it - the
 * metric of physics_multitrain.py:211-213 / physics_train.py:159 at radius 1.  a, b and their strides: exactly as for
 * kr_dtw_batch.  dist[B]; path[B][Ta + Tb - 1][2] and path_len[B] (both nullable, but only together): the level-0 warp
 * path of every rod as (i, j) pairs from (0, 0) to (Ta - 1, Tb - 1); entries past path_len[b] are left untouched.
 * The algorithm: level l + 1 of the pyramid is x[i] = (x[2i] + x[2i + 1]) / 2 per component for i < len / 2 (an odd
 * last sample is dropped), descending while both lengths are >= radius + 2; the deepest level is an exact DTW; every
 * level's recurrence is cost = (|dx| + |dy|) + |dz|, predecessor = the FIRST minimum in the order up (i - 1, j), left
 * (i, j - 1), diagonal, D = predecessor + cost, cells outside the level's window +inf; the window of the next finer
 * level gives fine rows 2c and 2c + 1 the columns [2 lo, 2 hi + 1] (clipped), lo = min(j) - radius, hi = max(j) + radius
 * over the cells of the coarse path with |i - c| <= radius.  dist, path_len and path are bit-identical to
 * krod_eval.fastdtw_distance / fastdtw_path on the same (upcast) samples; with a radius that covers the whole table
 * dist is kr_dtw_batch's.
 * A rod with a sample that is not finite in either sequence gets dist = NaN and path_len = 0 (its path entries are
 * left untouched); the call returns KR_OK and every other rod's outputs are bit for bit those of the clean call.
 * ws: caller-owned device scratch of kr_fastdtw_ws_bytes(B, Ta, Tb, radius) bytes (the back-pointers of level 0 where
 * they do not fit the LDS; 0 for short sequences - ws may then be NULL; always a multiple of 16).  The call uses none
 * of the handle's scratch; two calls in flight need two workspaces.  Nothing outside the Ta, Tb samples of a rod, its
 * outputs and its slice of ws is touched.
 * KR_E_ARG: a null handle, a, b or dist; B, Ta or Tb < 1; a negative stride; radius < 1 (radius 0 leaves rows without a
 * window in the host statement); only one of path / path_len; ws NULL while the size is nonzero.  KR_E_UNSUPPORTED:
 * radius > KR_FASTDTW_MAX_RADIUS or a length > KR_FASTDTW_MAX_LEN.  In every refusal nothing is launched and no
 * output byte is written.
 * One wavefront per rod: a banded form of kr_dtw_batch's sweep per level, two bits of back-pointer per cell, one walk
 * back per level (at level 0 only when the path is asked for). */
#define KR_FASTDTW_MAX_LEN 1024
#define KR_FASTDTW_MAX_RADIUS 8
size_t kr_fastdtw_ws_bytes(int64_t B, int64_t Ta, int64_t Tb, int radius);
int kr_fastdtw_batch(kr_handle* h, int64_t B,
                     const void* a, int64_t Ta, int64_t a_rod_stride, int64_t a_step_stride,
                     const void* b, int64_t Tb, int64_t b_rod_stride, int64_t b_step_stride,
                     int radius, double* dist, int32_t* path, int32_t* path_len, void* ws,
                     int dtype, void* stream);

/* Soft-DTW (M. Cuturi, M. Blondel 2017) between 3-vectors and its gradient with respect to a: the differentiable form of
 * kr_dtw_batch's metric - a loss on a simulated tip path against a recorded one that is not sample-aligned with it, and
 * its cotangent written where kr_simulate_vjp_* reads it.  A training loss, not a reported metric.  It is what
 * krod_eval.softdtw_grad(a, b, gamma, cost) states; 1-based table indices, all arithmetic fp64 whatever dtype:
 *   cost      c(i,j) = (|dx| + |dy|) + |dz| (cost = 0, the metric's own point distance, kr_dtw_batch's order) or
 *             (dx dx + dy dy) + dz dz (cost = 1), d = a_i - b_j
 *   forward   R(0,0) = 0, every other cell of row 0 and column 0 +inf;  R(i,j) = c(i,j) + softmin(R(i-1,j), R(i,j-1),
 *             R(i-1,j-1)),  softmin(r) = m - gamma log(sum_k exp((m - r_k) / gamma)), m = min r, an infinite entry
 *             contributing 0;  value = R(Ta,Tb)
 *   backward  E(Ta+1,Tb+1) = 1, R(Ta+1,Tb+1) = R(Ta,Tb); row Ta+1 and column Tb+1 otherwise R = -inf, E = 0, and c = 0
 *             there;  E(i,j) = sum over (p,q) in {(i+1,j), (i,j+1), (i+1,j+1)} of E(p,q) exp((R(p,q) - R(i,j) - c(p,q)) / gamma)
 *             (every exponent <= 0)
 *   gradient  g_a[i][k] = sum_j E(i,j) dc(i,j)/da_ik,  dc/da = sign(a_ik - b_jk) with sign(0) = 0 (cost = 0), 2 (a_ik - b_jk)
 *             (cost = 1)
 * The device is held to the statement by derived bounds, not bit for bit (exp and log are the device's): with n = Ta + Tb - 1
 * and eps = 2^-52, |value - exact| <= tolR = 16 n eps (max |R| + gamma ln 3) and |g_a[i][k] - exact| <= n (3 tolR / gamma +
 * 8 eps) sum_j E(i,j) |dc/da_ik| (tests/test_gpu_softdtw.py; measured ratios in LABBOOK.md).  As gamma -> 0 the value tends
 * to kr_dtw_batch's distance from below: dtw - n gamma ln 3 <= value <= dtw up to tolR.  A 1 x 1 table is exact: value =
 * c(1,1) and g_a = dc/da bit for bit.  The kernel forms a weight's exponent as (Q(p,q) - R(i,j)) / gamma with Q = R - c the
 * softmin the forward sweep kept BEFORE adding c, which is the statement's exponent without the rounding of adding c and
 * taking it off again (ulp(R) / gamma per cell): in a hard table (gamma far below the gaps between warp paths) E is 1 on the
 * path and g_a a sum of signs to the last bit, where the statement evaluated in fp64 drifts by n ulp(R) / gamma.
 * a, b and their strides: exactly as for kr_dtw_batch (in ELEMENTS, >= 0, b's rod stride 0 = one reference for all rods).
 * value[B], double.  g_a (nullable; element type = dtype): sample i of rod r is WRITTEN - not added to - as the 3
 * consecutive elements at g_a + r*g_rod_stride + i*g_step_stride (strides in elements, > 0), nothing else: one call writes
 * straight into slots 12..14 of the last record of g[t + 1] of a zeroed cotangent history g[T+1][B][N][KR_SLOTS] (pointer
 * to slot 12 of record N - 1 of g[1]; rod N*KR_SLOTS, step B*N*KR_SLOTS), which kr_simulate_vjp_* takes as g_states: no
 * trajectory and no table leaves the device between the forward rollout and the backward pass.  g_a == NULL: value only,
 * nothing of the backward sweep runs; value has the bits of the call with the gradient.
 * A rod with a sample that is not finite in either sequence gets value = NaN and NaN in all its g_a entries; the call
 * returns KR_OK and every other rod's outputs are bit for bit those of the clean call.  The sums of the gradient are formed
 * in a fixed order without atomics: a rod's outputs are the same bits from run to run, for any B and wherever it stands.
 * That order is the DEVICE's: the sum over j of a row is taken in DECREASING j (the backward sweep meets the columns that
 * way), where krod_eval.softdtw_grad, the definition, sums in increasing j - a difference within the rounding of a sum of
 * Tb terms, inside the bound above, and the reason g_a is held to the statement by a bound and not bit for bit.
 * ws: caller-owned device scratch of kr_softdtw_ws_bytes(B, Ta, Tb, need_grad) bytes (the table of the cells for the backward
 * sweep where it does not fit the LDS; 0 for value only and for short sequences - ws may then be NULL; always a multiple
 * of 16).  The call uses none of the handle's scratch and reads no parameter; two calls in flight need two workspaces.
 * Nothing outside the Ta, Tb samples of a rod, its outputs and its slice of ws is touched.
 * KR_E_ARG: a null handle, a, b or value; B, Ta or Tb < 1; a negative stride of a or b; a stride of g_a <= 0 with g_a given;
 * gamma not finite or <= 0; cost not 0 or 1; a bad dtype; ws NULL while the size is nonzero.  KR_E_UNSUPPORTED: a length
 * > KR_SOFTDTW_MAX_LEN.  In every refusal nothing is launched and no output byte is written.
 * One wavefront per rod: kr_dtw_batch's sweep with the longer cell, every R kept, and the mirrored sweep back. */
#define KR_SOFTDTW_MAX_LEN 1024
size_t kr_softdtw_ws_bytes(int64_t B, int64_t Ta, int64_t Tb, int need_grad);
int kr_softdtw_batch(kr_handle* h, int64_t B,
                     const void* a, int64_t Ta, int64_t a_rod_stride, int64_t a_step_stride,
                     const void* b, int64_t Tb, int64_t b_rod_stride, int64_t b_step_stride,
                     double gamma, int cost, double* value,
                     void* g_a, int64_t g_rod_stride, int64_t g_step_stride,
                     void* ws, int dtype, void* stream);

/* physics_multitrain.py:215-222 per rod: mse[b] = 1000 * mean over the first T states and the handle's N grid points
 * of the 3 squared position errors and the 3 squared zyx-Euler-angle errors (6*T*N terms).
 * states[T][B][N][KR_SLOTS] (the first T slots of a full history), ref_states[T][ref_B][N][KR_SLOTS], ref_B = 1 or B;
 * both 16-byte aligned.  parts[B][2] (nullable): the two sums (position, Euler) before the division.
 * The angles are SciPy's Rotation.from_quat(q, scalar_first=True).as_euler('zyx') (extrinsic) in closed form: with
 * (w, x, y, z) = q / |q|
 *     a = atan2(2(wz - xy), 1 - 2(y^2 + z^2)),  b = asin(clamp(2(xz + wy), -1, 1)),  c = atan2(2(wx - yz), 1 - 2(x^2 + y^2))
 * (2.7e-15 from SciPy 1.15.3 on 20 000 random non-unit quaternions with |b| < 1.4) - not
 * Utils.transformations.quaternion_to_euler and not the fp32 short forms of the training loss.  There is no
 * gimbal-lock branch: within ~1e-6 of b = +-pi/2 SciPy zeroes one angle and warns, the closed form does not.
 * The sums are formed in a fixed order without atomics: a call is reproducible bit for bit. */
int kr_pose_mse_batch(kr_handle* h, int64_t B, int64_t T, const void* states, const void* ref_states,
                      int64_t ref_B, double* mse, double* parts, int dtype, void* stream);
/* The same with the number of points per rod as an argument instead of the handle's N: records[T][B][P][KR_SLOTS],
 * ref_records[T][ref_B][P][KR_SLOTS] - the kp of kr_simulate_batch_keypoints (P = K) against a reference gathered at the
 * same points.  With P = N it returns bit for bit what kr_pose_mse_batch returns. */
int kr_pose_mse_points_batch(kr_handle* h, int64_t B, int64_t T, int64_t P, const void* records, const void* ref_records,
                             int64_t ref_B, double* mse, double* parts, int dtype, void* stream);

/* ---- adjoint of a solved step, backward pass over a stored rollout ------------------------------------------------- */
/* The derivative of one pass of the loop in knode.simulate (knode.py:70-100) - BDF2 history, shooting solve of the Euler
 * sweep (cosserat_ode.py:188-213) for the base wrench G - at its CONVERGED solution, MLP off: given the cotangent
 * g_next[B][N][KR_SLOTS] of state_next (all 25 values of every grid point, packed like a state) it returns the gradients
 * with respect to everything the step read.  The reference carries the differentiable sweep
 * (CosseratRodTorch.getResidualEuler) but never takes it through the solve; this call does, by the implicit-function
 * theorem: nothing is re-solved, the states are read from state_next as kr_step_batch / kr_simulate_batch left them
 * (solve with tol ~1e-12: the adjoint is that of the exact root, and the distance to it enters the gradient at first order).
 * The mathematics, with y_0 = [p0, h0, G, q0, w0], y_{j+1} = y_j + ds f(y_j, hist_j, tf), hist = c1 cur + c2 prev (the
 * twelve leading slots q w v u; f reads nothing else of the history), tf = tensions @ tendon_dirs:
 *   sweep      lambda_{N-1} = g_y[N-1];  lambda_j = g_y[j] + lambda_{j+1} + J_j^T [ds lambda_{j+1}; g_z[j]], J_j the complete
 *              Jacobian of the point map (that of kr_ode_vjp_batch with cut = 0);  a = (n, m) rows of lambda_0
 *   implicit   M = d(n, m)_{N-1} / dG from the same sweep seeded with the six unit vectors on the tip's (n, m);
 *              M^T nu = -a;  the total adjoint is the sweep seeded with g plus nu on the tip's (n, m)
 *   outputs    g_cur[j][0..11] = c1 ghat_j, g_prev[j][0..11] = c2 ghat_j, ghat_j = the history columns of J_j^T applied to
 *              the total adjoint; slots 12..24 are zero (no equation reads them) and the pads are zero; v, u of the LAST
 *              grid point of state_next are a copy of state_cur's (the z[:, N-1] the reference never writes), so
 *              g_cur[N-1][6..11] = g_next[N-1][6..11].  When state_prev aliases state_cur (the reference's first step,
 *              knode.py:65-66) the gradient of that one state is g_cur + g_prev.
 *              g_tensions[B][4] = tendon_dirs . sum_j (tendon-force column of J_j^T ...)
 *              g_bnd[B][KR_BND], in the order of kr_simulate_batch_boundary: lambda_0 rows of p0, h0, q0, w0, then the
 *              gradient with respect to F_tip, M_tip, which is -nu (the wrench enters the tip condition only)
 *              resid[B]: |(n, m) rows of the total adjoint's lambda_0|_inf / |a|_inf - zero in exact arithmetic, the
 *              measure of the 6 x 6 solve (0 when a = 0)
 * Outputs are overwritten; g_cur, g_prev, g_tensions, g_bnd, resid, status may each be NULL.  No output may overlap an
 * input.  state_prev may alias state_cur.  Parameters: the handle's (diagonal or full Bse / Bbt, any N >= 2).
 * Arithmetic is fp64 whatever `dtype`, which is the element type of the arrays only: the KR_F32 call returns the KR_F64
 * call on the upcast inputs, rounded to float, bit for bit.  One wavefront per rod, no atomics, none of the handle's
 * scratch: a rod's outputs do not depend on the batch it rides in.
 * status[B]: KR_ST_CONVERGED; KR_ST_MAXIT when the 6 x 6 solve rejects a pivot of M (zero, or below 1e-13 of M's largest
 * entry); KR_ST_NONFINITE when any value the step adjoint reads of that rod (the 25 used slots of state_next and g_next,
 * the twelve leading slots of state_cur / state_prev, the tensions) or M is not finite.  Such values are ordinary input:
 * the call returns KR_OK; a rod with a nonzero status gets NaN in every gradient value (g_cur / g_prev slots 0..11,
 * g_tensions, g_bnd, resid; the structurally zero slots stay zero) and every other rod's outputs are bit for bit those
 * of the clean call.  Nothing of it stays in the handle.
 * KR_E_UNSUPPORTED, with a message, nothing launched and no output byte written: use_nn != 0 (the network's input
 * Jacobian is not part of the per-point derivative yet), scheme == KR_RK4.  KR_E_ARG: a null handle, state or g_next or
 * tensions pointer; B < 1; a bad dtype. */
int kr_step_vjp_batch(kr_handle* h, int64_t B, int scheme,
                      const void* state_prev, const void* state_cur, const void* state_next, const void* tensions,
                      const void* g_next, void* g_cur, void* g_prev, void* g_tensions, void* g_bnd,
                      double* resid, int32_t* status, int use_nn, int dtype, void* stream);

/* The backward pass over a stored rollout of kr_simulate_batch (knode.py:55-102 with the step of knode.py:70-100 and
 * the sweep of cosserat_ode.py:188-213): ctl[B][T][4] and the FULL history states[T+1][B][N][KR_SLOTS] of that call (a
 * ring of three slots does not hold what is needed), state_prev_init as given to it (NULL: y_prev = y before the first
 * step).  g_states[T+1][B][N][KR_SLOTS] is in/out: on entry the direct dL/dstates[t] (a tip loss: slots 12..14 of the last
 * record of the states it scores), on return the total adjoint of every stored state - g_states[0] is the gradient with
 * respect to the initial condition.
 * The result is DEFINED as this composition of kr_step_vjp_batch calls and equals it bit for bit: for t = T-1 .. 0 the
 * step adjoint of (states[t-1], states[t], states[t+1], ctl[:, t]) with g_next = g_states[t+1]; then
 * g_states[t] += g_cur and g_states[t-1] += g_prev, in this order, in the element type of the arrays.  Step 0's g_prev
 * goes into g_states[0] when state_prev_init is NULL, otherwise it is written to g_prev_init[B][N][KR_SLOTS] (nullable).
 * g_ctl[B][T][4] = g_tensions of step t; g_bnd[B][KR_BND] = the sum over the steps, t = T-1 first (the handle's
 * boundary is constant in time; kr_simulate_vjp_table_batch keeps it per step); resid[B][T], status[B][T] per step.  g_prev_init, g_ctl, g_bnd, resid, status may be
 * NULL.  A rod whose step t0 reports a nonzero status has NaN in g_ctl[b][t0] and, through g_states[t0], in every
 * earlier step's outputs; other rods are bit for bit the clean call.
 * One launch per step plus the accumulations; uses the handle's scratch (two state-sized buffers).
 * Refusals as for kr_step_vjp_batch, and KR_E_ARG for T < 1 or a null ctl, states or g_states. */
int kr_simulate_vjp_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, const void* states,
                          const void* state_prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd,
                          double* resid, int32_t* status, int use_nn, int dtype, void* stream);

/* ---- the adjoint with the residual MLP on ---------------------------------------------------------------------------------
 * kr_step_vjp_batch for the KNODE model, physics plus network in every sweep (knode.py:70-100 with the point map of
 * cosserat_ode.py:178-184 inside the sweep of cosserat_ode.py:188-213): (y_s, z) = f_phys(y, hist, tf) + NN(x),
 * x = [y (19), z_phys (6), tf (3)].  With Jn[25][28] = dNN/dx at the stored point (kr_mlp_input_jacobian_batch) the point
 * Jacobian of the recursion stated at kr_step_vjp_batch becomes J = Jp + Jn X, X = [identity on the y columns; rows 19..24
 * of Jp, the z_phys tangents; identity on the tf columns]; pass 1, the 6 x 6 solve, pass 2 and every output are as there.
 * Arguments: those of kr_step_vjp_batch without use_nn (the network is the handle's, kr_set_mlp), plus two nullable
 * outputs nn_x[B][N-1][32], nn_g[B][N-1][32] of the arrays' element type: row (b, j) holds the network's input x_j
 * (28 values, then zeros) and the cotangent that reaches its output at point j, c_j = [ds lambda_{j+1} (19); g_z[j] (6)]
 * (25 values, then zeros), lambda the total adjoint.  The gradient of the loss with respect to the network's weights is
 * the ordinary MLP backward pass over these rows (kr_mlp_forward + kr_mlp_backward), summed over points, rods and steps.
 * Three launches (the rows x, their Jacobians on the fp64 matrix cores, the recursion with one wavefront per rod); the
 * handle's scratch holds x and Jn: B (N-1) (32 + 700) doubles, 0.6 GB at B = 1024, N = 100.  Arithmetic is fp64 whatever
 * `dtype`; the KR_F32 call is the KR_F64 call on the upcast inputs, rounded, bit for bit.  A rod's outputs do not depend
 * on the batch it rides in.  status as for kr_step_vjp_batch, with the rod's x and Jn among the values read: a rod with
 * a nonzero status gets NaN gradients and NaN in its nn_g rows (its nn_x rows keep the inputs), every other rod's
 * outputs are bit for bit those of the clean call.
 * Refusals, each with a message, nothing launched and no output byte written: KR_E_STATE without a network;
 * KR_E_UNSUPPORTED for scheme == KR_RK4, nn_input_history = 1, a network outside the shapes of
 * kr_mlp_input_jacobian_batch or with an activation on its last layer; KR_E_ARG for a null handle, state, g_next or
 * tensions pointer, B < 1, a bad dtype. */
int kr_step_vjp_nn_batch(kr_handle* h, int64_t B, int scheme,
                         const void* state_prev, const void* state_cur, const void* state_next, const void* tensions,
                         const void* g_next, void* g_cur, void* g_prev, void* g_tensions, void* g_bnd,
                         double* resid, int32_t* status, void* nn_x, void* nn_g, int dtype, void* stream);

/* kr_simulate_vjp_batch for the KNODE model (knode.py:55-102 with the step of knode.py:70-100 and the sweep of
 * cosserat_ode.py:188-213, network on, cosserat_ode.py:178-184): DEFINED as the same composition of kr_step_vjp_nn_batch
 * calls and equal to it bit for bit; per step it launches the rows, the Jacobians, the recursion and the accumulations.
 * nn_x, nn_g[T][B][N-1][32] (nullable): the rows of step t.  Scratch: two state-sized buffers and the step call's.
 * Refusals as for kr_step_vjp_nn_batch, and KR_E_ARG for T < 1 or a null ctl, states or g_states. */
int kr_simulate_vjp_nn_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, const void* states,
                             const void* state_prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd,
                             double* resid, int32_t* status, void* nn_x, void* nn_g, int dtype, void* stream);

/* ---- the adjoint with the gradient of the rod's material parameters ----------------------------------------------------
 * kr_step_vjp_batch (MLP off, Euler sweep, the handle's parameters, diagonal or full Bse / Bbt, any N >= 2, fp64
 * arithmetic whatever `dtype`, one wavefront per rod, no atomics, a rod's outputs independent of the batch it rides in)
 * with one more nullable output, g_par[B][KR_PAR]: the gradient with respect to the parameters kr_derive starts from,
 * in the order and row-major layout of struct kr_params -
 *   E [0], r [1], rho [2], L [3], vstar [4..6], g [7..9], Bse [10..18], Bbt [19..27], C [28..30], tendon_dirs [31..42]
 * (del_t and N are not differentiated).  With lambda the total adjoint of the recursion stated at kr_step_vjp_batch (the
 * sweep seeded with g plus nu on the tip's (n, m)) and c_j = [ds lambda_{j+1}; g_z[j]]:
 *   g_par[k] = sum_{j = 0..N-2} c_j . d(y_s, z)_j / d theta_k  +  (d ds / d theta_k) sum_j lambda_{j+1} . y_s,j
 * d(y_s, z)_j / d theta_k is the TOTAL derivative of the point map through kr_derive (G = E / 2.6, A = pi r^2, J ~ r^4,
 * Kse, Kbt, the two inverses (K + c0 B)^-1, Kse vstar, rho A, rho A g, rho J) at fixed inputs; each of the nine entries of
 * Bse and of Bbt is an independent variable (a symmetric parametrisation sums the two mirrored entries); d ds / d L =
 * 1 / (N - 1) and zero for every other parameter; tendon_dirs enters tf = tensions @ tendon_dirs alone, so
 * g_par[31 + 3 i + c] = tensions[i] * (the tendon-force cotangent)[c] - exactly zero for a tendon without tension.  No
 * parameter enters the base state or the tip condition: the 6 x 6 solve and nu are those of kr_step_vjp_batch.
 * Every other output is bit for bit that of kr_step_vjp_batch (use_nn = 0) on the same inputs - it is written by that
 * call's kernel, launched first; a second launch repeats the recursion and writes g_par alone - and with g_par == NULL the
 * call IS that call.  A rod with a nonzero status gets NaN in all KR_PAR values; every other rod's outputs
 * are bit for bit those of the clean call.  The KR_F32 call is the KR_F64 call on the upcast inputs, rounded to float.
 * Refusals as for kr_step_vjp_batch (KR_E_UNSUPPORTED for scheme == KR_RK4; KR_E_ARG for a null handle, state, g_next or
 * tensions pointer, B < 1, a bad dtype), each with a message, nothing launched and no output byte written.
 * Not served: the MLP-on form (kr_step_vjp_nn_batch has no g_par); RK4; del_t.  Every rod of a call shares the handle's
 * parameters, and g_par is per rod only because the states are: per-rod parameters (table, loads, boundary) are served by
 * kr_step_vjp_table_batch / kr_simulate_vjp_table_batch below, a bank (the MLP on, without g_par) by
 * kr_step_vjp_bank_batch / kr_simulate_vjp_bank_batch below them. */
#define KR_PAR 43
int kr_step_vjp_par_batch(kr_handle* h, int64_t B, int scheme,
                          const void* state_prev, const void* state_cur, const void* state_next, const void* tensions,
                          const void* g_next, void* g_cur, void* g_prev, void* g_tensions, void* g_bnd, void* g_par,
                          double* resid, int32_t* status, int dtype, void* stream);

/* kr_simulate_vjp_batch (MLP off) with g_par[B][KR_PAR] (nullable): DEFINED as the same composition of
 * kr_step_vjp_par_batch calls and equal to it bit for bit; g_par = the sum over the steps of the step's g_par, t = T-1
 * first, from zero, in the element type of the arrays (the parameters are constant in time).  The initial state adds no
 * parameter term: no step reads p of an earlier state (the only slots that scale with L), and v = e3 of the straight rod
 * is a constant - the caller's states[0] is an input like any other, its gradient is g_states[0].  A rod whose step t0
 * reports a nonzero status has NaN in all of its g_par.  With g_par == NULL the call IS kr_simulate_vjp_batch.
 * Scratch: that call's plus B * KR_PAR values.  Refusals as for kr_step_vjp_par_batch, and KR_E_ARG for T < 1 or a null
 * ctl, states or g_states. */
int kr_simulate_vjp_par_batch(kr_handle* h, int64_t B, int64_t T, int scheme, const void* ctl, const void* states,
                              const void* state_prev_init, void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd,
                              void* g_par, double* resid, int32_t* status, int dtype, void* stream);

/* ---- the adjoint of a heterogeneous batch: per-rod parameters, per-step boundary data --------------------------------------
 * kr_step_vjp_par_batch (one pass of the loop of knode.py:70-100 around the sweep of cosserat_ode.py:188-213, MLP off, Euler
 * sweep) with rod b taking row b of a parameter table (kr_param_table_create) in place of the handle's parameters: the
 * backward side of kr_simulate_batch_table / _loads / _boundary.  B is the table's B; every array is shaped as there.
 * Rod b's outputs are the step adjoint stated at kr_step_vjp_batch and kr_step_vjp_par_batch with P = row b (c0, c1, c2,
 * ds, the material constants, tendon_dirs) and, for g_par, row b's E, r, rho, vstar, g (kept by the table in one more device
 * array of nine doubles per row; nothing a forward kernel receives changed).  Table rows are diagonal and 9 <= N <= 128
 * (kr_param_table_check).  The call takes no bnd or loads array: record 0 of state_next holds the base values the step used
 * exactly (kr_simulate_batch_boundary), they are read from there like every other state value, and the tip wrench enters
 * no derivative - g_bnd[b] IS the gradient with respect to the KR_BND boundary values rod b's step used, wherever they came
 * from (its row, loads[b][t], bnd[b][t]).
 * Arithmetic is fp64 whatever `dtype`; the KR_F32 call is the KR_F64 call on the upcast inputs, rounded, bit for bit.  One
 * wavefront per rod, no atomics, none of the handle's scratch; the row is read in place with scalar loads (the rod index is
 * wavefront-uniform) and no row beyond the table's last is addressed.  A rod's outputs do not depend on the batch or on its
 * position in it.  g_par[B][KR_PAR] is nullable: NULL skips the second launch, and with it every other output is bit for bit
 * that of the call without it, written by the kernel without g_par, launched first (the rule of kr_step_vjp_par_batch).
 * status, NaN rules and nullable outputs per rod as for kr_step_vjp_batch / kr_step_vjp_par_batch.
 * Refusals, each with a message, nothing launched and no output byte written, in this order: KR_E_ARG for a null handle, a
 * null table, a bad dtype, a null state, g_next or tensions pointer; KR_E_ARG for a table of another device or whose N or
 * del_t differ from the handle's (the handle lends its device, its stream ordering and, for the rollout, its scratch: a
 * "carrier"; its own parameters are not read); KR_E_UNSUPPORTED for scheme == KR_RK4.  There is no use_nn: the calls
 * differentiate the physics alone and do not read the handle's network.
 * Not served: g_par with the MLP on (the MLP-on form of a table and a bank is kr_step_vjp_bank_batch below, without g_par);
 * RK4; full matrices in a row; del_t. */
int kr_step_vjp_table_batch(kr_handle* h, const kr_param_table* t, int scheme,
                            const void* state_prev, const void* state_cur, const void* state_next, const void* tensions,
                            const void* g_next, void* g_cur, void* g_prev, void* g_tensions, void* g_bnd, void* g_par,
                            double* resid, int32_t* status, int dtype, void* stream);

/* kr_simulate_vjp_par_batch for the table form (knode.py:55-102): DEFINED as the same composition of
 * kr_step_vjp_table_batch calls and equal to it bit for bit; g_par (nullable) = the sum over the steps of the step's,
 * t = T-1 first, from zero.  g_bnd (nullable):
 *   bnd_per_step == 0   g_bnd[B][KR_BND], the sum over the steps from zero, t = T-1 first: the gradient with respect to the
 *                       row's constant boundary values (a kr_simulate_batch_table rollout)
 *   bnd_per_step == 1   g_bnd[B][T][KR_BND], entry [b][t] = the g_bnd of step t, bit for bit: the gradient with respect to
 *                       bnd[b][t] of kr_simulate_batch_boundary, and its last six columns the gradient with respect to
 *                       loads[b][t] of kr_simulate_batch_loads
 * A rod whose step t0 reports a nonzero status has NaN in g_bnd[b][t0] and, through g_states[t0], in every earlier step's
 * outputs (bnd_per_step == 1; in all of g_bnd[b] otherwise).  Scratch: that of kr_simulate_vjp_par_batch.
 * Refusals as for kr_step_vjp_table_batch, with KR_E_ARG for T < 1 after the dtype, for a null ctl, states or g_states, and
 * for a bnd_per_step other than 0 or 1. */
int kr_simulate_vjp_table_batch(kr_handle* h, const kr_param_table* t, int64_t T, int scheme, const void* ctl,
                                const void* states, const void* state_prev_init, void* g_states, void* g_prev_init,
                                void* g_ctl, void* g_bnd, int bnd_per_step, void* g_par, double* resid, int32_t* status,
                                int dtype, void* stream);

/* ---- the adjoint of a heterogeneous batch with the MLP on: per-rod parameters AND per-rod networks -------------------------
 * kr_step_vjp_nn_batch (knode.py:70-100 with the point map of cosserat_ode.py:178-184 inside the sweep of
 * cosserat_ode.py:188-213) with rod b taking row b of a parameter table in place of the handle's parameters and network
 * net_of_rod_host[b] of a bank (kr_mlp_bank_create) in place of the handle's network: the backward side of
 * kr_simulate_batch_bank / kr_simulate_batch_bank_keypoints - the reference's experiment of model-mismatch variants, each with
 * its own trained network (physics_multitrain.py:181-199), differentiated in one call.  B is the table's B;
 * net_of_rod_host[B] is a HOST array of int32, every entry in [0, K), read before the call returns, as
 * kr_simulate_batch_bank takes it.  Every other argument is that of kr_step_vjp_nn_batch; nn_x, nn_g[B][N-1][32] (nullable)
 * are in ROD order: the rows of network k's weight gradient are those of the rods with net_of_rod_host[b] == k.  Like the
 * table form the call takes no bnd or loads array - record 0 of state_next holds the base values the step used - and g_bnd[b]
 * is the gradient with respect to the KR_BND boundary values rod b's step used, wherever they came from.
 * Launches: the rows x of every stored point from the rod's own row, written in NETWORK order (the stable permutation of the
 * rods by net_of_rod_host, computed on the host once per call and kept in the handle's scratch); the Jacobians on the fp64
 * matrix cores, one launch of kr_mlp_input_jacobian_batch's kernel per network that has rods, on that network's contiguous
 * range of rows (a network without rods launches nothing); the recursion with one wavefront per rod, the row read in place
 * with scalar loads.  Scratch: that of kr_step_vjp_nn_batch plus B int32.  Arithmetic is fp64 whatever `dtype`; the KR_F32
 * call is the KR_F64 call on the upcast inputs, rounded, bit for bit.  No atomics.  A rod's outputs depend neither on the
 * batch, nor on its position in it, nor on which other networks are present.  status, NaN rules and nullable outputs per rod
 * as for kr_step_vjp_nn_batch / kr_step_vjp_table_batch.
 * Refusals, each with a message, nothing launched and no output byte written, in this order: KR_E_ARG for a null handle,
 * table or bank; a bad dtype; a null state, g_next, tensions or net_of_rod_host pointer; a table or a bank of another device,
 * or a table whose N or del_t differ from the handle's (a carrier, as for the table form); an entry of net_of_rod_host outside
 * [0, K); then KR_E_UNSUPPORTED for scheme == KR_RK4, for a table of nn_input_history = 1 (the 53-wide input), for a bank
 * whose shape kr_mlp_input_jacobian_batch does not serve, and for an activation on the last layer.  The calls read neither the
 * handle's parameters nor the handle's network.
 * Not served: g_par with the network on; full matrices in a row; RK4; the 53-wide input. */
int kr_step_vjp_bank_batch(kr_handle* h, const kr_param_table* t, const kr_mlp_bank* bank, const int32_t* net_of_rod_host,
                           int scheme, const void* state_prev, const void* state_cur, const void* state_next,
                           const void* tensions, const void* g_next, void* g_cur, void* g_prev, void* g_tensions, void* g_bnd,
                           double* resid, int32_t* status, void* nn_x, void* nn_g, int dtype, void* stream);

/* kr_simulate_vjp_nn_batch for the bank form (knode.py:55-102): DEFINED as the same composition of kr_step_vjp_bank_batch
 * calls and equal to it bit for bit.  g_bnd (nullable) with bnd_per_step == 0 is [B][KR_BND], the sum over the steps from
 * zero, t = T-1 first; with bnd_per_step == 1 it is [B][T][KR_BND], entry [b][t] = the g_bnd of step t, bit for bit - the
 * gradient with respect to bnd[b][t] of kr_simulate_batch_bank_keypoints: a base trajectory and a wrench history per rod,
 * with the network on.  nn_x, nn_g[T][B][N-1][32] (nullable): the rows of step t, in rod order.  Scratch: that of
 * kr_simulate_vjp_nn_batch plus the permutation (B int32).  Refusals as for kr_step_vjp_bank_batch, with KR_E_ARG for T < 1
 * after the dtype, for a null ctl, states or g_states, and for a bnd_per_step other than 0 or 1. */
int kr_simulate_vjp_bank_batch(kr_handle* h, const kr_param_table* t, const kr_mlp_bank* bank, const int32_t* net_of_rod_host,
                               int64_t T, int scheme, const void* ctl, const void* states, const void* state_prev_init,
                               void* g_states, void* g_prev_init, void* g_ctl, void* g_bnd, int bnd_per_step, double* resid,
                               int32_t* status, void* nn_x, void* nn_g, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KNODE_ROD_H */
