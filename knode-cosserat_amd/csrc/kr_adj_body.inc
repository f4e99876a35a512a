// kr_adj_body.inc - the step adjoint of one rod per wavefront: the ONE text of the recursion, the body of step_vjp_kernel
// (kr_adj.hip, where the mapping is described), of step_vjp_par_kernel (kr_adj_par.hip) and of step_vjp_nn_kernel
// (kr_adj_nn.hip).  Included INSIDE the kernel, as text, so that each kernel is compiled from the statements it always had.
// In scope are the kernel's arguments P (RodConst<double>) and A (AdjArgs<T>), and two forms:
//   constexpr bool PAR   the gradient of the material parameters goes into Q.g_par; Q (AdjPar<T>) is read only where PAR holds
//   constexpr bool NNON  the network's input Jacobian joins the per-point derivative and pass 2 emits the rows of the weight
//                        gradient; NN (AdjNn<T>) is read only where NNON holds
// The table kernels (kr_adj_tab.hip) include this text as it is: they bind P to the rod's row and Q to the rod's parameters
// before the include, per rod instead of per launch, so the body needs no form for them.
// A kernel without a form declares an empty Q / NN.  PAR and NNON are not dependent on T, so a discarded branch is still
// type-checked (jc exists in every form), and whatever a form alone needs folds to a constant without it (q0, own): a
// live declaration moves the register allocation of the kernels that never read it.
  const int lane = threadIdx.x & 63;
  const int64_t rod = (int64_t)blockIdx.x * ADJ_RODS_PER_WG + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (rod >= A.B) return;  // (the whole wavefront: nothing below crosses wavefronts)
  const int N = P.N;
  const int64_t rec0 = rod * N;
  const int64_t q0 = NNON ? rod * (N - 1) : 0;  // first row of this rod in the network arrays
  const bool own = NNON && (lane < 19 || (lane >= 31 && lane < 34));
  const int dir = lane < 19 ? lane : lane + 13;  // lanes 19..30 -> 32..43 (history q w v u), 31..33 -> 44..46 (tendon force)
  const int yslot = adj_yslot(lane < 19 ? lane : 0);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);

  bool bad = false;
  double tens[4], tf[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    tens[k] = (double)A.tens[rod * A.tens_stride + k];
    bad |= !isfinite(tens[k]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) tf[c] = tens[0] * P.tdirs[c] + tens[1] * P.tdirs[3 + c] + tens[2] * P.tdirs[6 + c] + tens[3] * P.tdirs[9 + c];

  // ---- the tip record: seeds; everything of it that no sweep reads is still checked ----
  const T* gN = A.g_next + (rec0 + N - 1) * KR_SLOTS;
  {
    const T* yN = A.next + (rec0 + N - 1) * KR_SLOTS;
    const T* cN = A.cur + (rec0 + N - 1) * KR_SLOTS;
    const T* pN = A.prev + (rec0 + N - 1) * KR_SLOTS;
#pragma unroll
    for (int k = 0; k < SL_USED; ++k) bad |= !isfinite((double)yN[k]) | !isfinite((double)gN[k]);
#pragma unroll
    for (int k = 0; k < 12; ++k) bad |= !isfinite((double)cN[k]) | !isfinite((double)pN[k]);
  }
  const double g_tip = (double)gN[yslot];

  // ---- pass 1: seven cotangent vectors ----
  double lam[ADJ_SEEDS];
  lam[0] = g_tip;
#pragma unroll
  for (int s = 1; s < ADJ_SEEDS; ++s) lam[s] = lane == 6 + s ? 1.0 : 0.0;
  for (int j = N - 2; j >= 0; --j) {
    double d[25];
    adj_point(P, A, rec0 + j, dir, tf, d, bad);
    double jc[25];
    if constexpr (NNON) {
      adj_nn_column(NN, q0 + j, lane, jc, bad);
      if (lane < NNA_IN) bad = bad || !isfinite(NN.xrows[(q0 + j) * NNA_ROW + lane]);
    }
    const T* g = A.g_next + (rec0 + j) * KR_SLOTS;
    double gz[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) gz[k] = (double)g[SL_V + k];
#pragma unroll
    for (int k = 0; k < SL_USED; ++k) bad |= !isfinite((double)g[k]);
    if constexpr (NNON) {
      double acc = 0.0, un = 0.0;
      adj_dot19_nn(lam[0], d, jc, acc, un);
      acc *= P.ds;
      un *= P.ds;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        acc = fma(gz[k], d[19 + k], acc);
        un = fma(gz[k], jc[19 + k], un);
      }
      lam[0] = ((double)g[yslot] + lam[0]) + (acc + adj_nn_term(un, own, d));
#pragma unroll
      for (int s = 1; s < ADJ_SEEDS; ++s) {
        double as = 0.0, us = 0.0;
        adj_dot19_nn(lam[s], d, jc, as, us);
        lam[s] = (lam[s] + P.ds * as) + adj_nn_term(P.ds * us, own, d);  // (the physics sum first, as without the network)
      }
    } else {
      double acc = P.ds * adj_dot19(lam[0], d, 0.0);
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = fma(gz[k], d[19 + k], acc);
      lam[0] = ((double)g[yslot] + lam[0]) + acc;
#pragma unroll
      for (int s = 1; s < ADJ_SEEDS; ++s) lam[s] = lam[s] + P.ds * adj_dot19(lam[s], d, 0.0);
    }
  }
  double a[6], m[6][6], nu[6];
  a[0] = adj_bcast<7>(lam[0]); a[1] = adj_bcast<8>(lam[0]); a[2] = adj_bcast<9>(lam[0]);
  a[3] = adj_bcast<10>(lam[0]); a[4] = adj_bcast<11>(lam[0]); a[5] = adj_bcast<12>(lam[0]);
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    m[k][0] = adj_bcast<7>(lam[1 + k]); m[k][1] = adj_bcast<8>(lam[1 + k]); m[k][2] = adj_bcast<9>(lam[1 + k]);
    m[k][3] = adj_bcast<10>(lam[1 + k]); m[k][4] = adj_bcast<11>(lam[1 + k]); m[k][5] = adj_bcast<12>(lam[1 + k]);
  }
  double anorm = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    anorm = fmax(anorm, fabs(a[k]));
    bad |= !isfinite(a[k]);
#pragma unroll
    for (int l = 0; l < 6; ++l) bad |= !isfinite(m[k][l]);
  }
  bad = __any(bad);  // (uniform already without the network; with it lanes read different columns of Jn and entries of x)
  const bool solved = adj_solve6(m, a, nu);
  const int st = bad ? KR_ST_NONFINITE : (solved ? KR_ST_CONVERGED : KR_ST_MAXIT);
  if (A.status && lane == 0) A.status[rod * A.st_stride] = st;

  T* oc = A.g_cur ? A.g_cur + rec0 * KR_SLOTS : nullptr;
  T* op = A.g_prev ? A.g_prev + rec0 * KR_SLOTS : nullptr;
  T* ot = A.g_tens ? A.g_tens + rod * A.g_tens_stride : nullptr;
  T* ob = A.g_bnd ? A.g_bnd + rod * KR_BND : nullptr;

  T* ox = NN.nn_x ? NN.nn_x + q0 * NNA_ROW : nullptr;
  T* og = NN.nn_g ? NN.nn_g + q0 * NNA_ROW : nullptr;
  if (st != KR_ST_CONVERGED) {  // no gradient: NaN in every value that carries one, zero where the structure is zero
    if constexpr (NNON)
      if (lane < NNA_ROW)
        for (int j = 0; j < N - 1; ++j) {  // (the rows keep their inputs; their cotangents carry no gradient)
          if (ox) ox[(int64_t)j * NNA_ROW + lane] = lane < NNA_IN ? (T)NN.xrows[(q0 + j) * NNA_ROW + lane] : (T)0;
          if (og) og[(int64_t)j * NNA_ROW + lane] = lane < 25 ? (T)nan : (T)0;
        }
    if (lane < KR_SLOTS) {
      const T fill = lane < 12 ? (T)nan : (T)0;
      for (int j = 0; j < N; ++j) {
        if (oc) oc[(int64_t)j * KR_SLOTS + lane] = fill;
        if (op) op[(int64_t)j * KR_SLOTS + lane] = fill;
      }
    }
    if (ot && lane < 4) ot[lane] = (T)nan;
    if (ob && lane < KR_BND) ob[lane] = (T)nan;
    if (A.resid && lane == 0) A.resid[rod * A.st_stride] = nan;
    if constexpr (PAR)
      if (lane < KR_PAR) Q.g_par[rod * KR_PAR + lane] = (T)nan;
    return;
  }

  // ---- pass 2: the combined cotangent; emits the input gradients ----
  const double c1 = P.c1, c2 = P.c2;
  double nu_l = 0.0;  // nu of this lane's row of (n, m)
#pragma unroll
  for (int k = 0; k < 6; ++k) nu_l = lane == 7 + k ? nu[k] : nu_l;
  double lm = g_tip + nu_l;
  double gtf = 0.0;
  // (PAR) this lane's parameter direction: its dot products with the constants' tangents, and lambda . y_s for L
  RodConstDual PD;
  double gpar = 0.0, gL = 0.0;
  if constexpr (PAR) adj_par_consts(P, Q, lane - ADJ_PAR_LANE0, PD);
  // the tip record: no f is evaluated there; v, u of state_next are those of state_cur (the z[:, N-1] the reference never
  // writes), so their cotangent passes straight through
  if (lane < KR_SLOTS) {
    const bool pass = lane >= SL_V && lane < SL_P;
    const T gv = gN[pass ? lane : 0];
    if (oc) oc[(int64_t)(N - 1) * KR_SLOTS + lane] = pass ? gv : (T)0;
    if (op) op[(int64_t)(N - 1) * KR_SLOTS + lane] = (T)0;
  }
  for (int j = N - 2; j >= 0; --j) {
    double d[25];
    bool unused = false;
    adj_point(P, A, rec0 + j, dir, tf, d, unused);
    double jc[25];
    if constexpr (NNON) adj_nn_column(NN, q0 + j, lane, jc, unused);
    const T* g = A.g_next + (rec0 + j) * KR_SLOTS;
    double acc;
    if constexpr (NNON) {
      if (lane < NNA_ROW) {  // the row of the weight gradient: the network's input and the cotangent that reaches its output
        const int zs = lane >= 19 && lane < 25 ? SL_V + lane - 19 : 0;
        const double cz = (double)g[zs];
        if (ox) ox[(int64_t)j * NNA_ROW + lane] = lane < NNA_IN ? (T)NN.xrows[(q0 + j) * NNA_ROW + lane] : (T)0;
        if (og) og[(int64_t)j * NNA_ROW + lane] = lane < 19 ? (T)(P.ds * lm) : (lane < 25 ? (T)cz : (T)0);
      }
      double un = 0.0;
      acc = 0.0;
      adj_dot19_nn(lm, d, jc, acc, un);
      acc *= P.ds;
      un *= P.ds;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        acc = fma((double)g[SL_V + k], d[19 + k], acc);
        un = fma((double)g[SL_V + k], jc[19 + k], un);
      }
      acc += adj_nn_term(un, own, d);
    } else {
      acc = P.ds * adj_dot19(lm, d, 0.0);
#pragma unroll
      for (int k = 0; k < 6; ++k) acc = fma((double)g[SL_V + k], d[19 + k], acc);
    }
    if constexpr (PAR) {
      double dp[25], val[25];
      adj_point_par(PD, c1, c2, A, rec0 + j, tf, dp, val);
      double accp = P.ds * adj_dot19(lm, dp, 0.0);
#pragma unroll
      for (int k = 0; k < 6; ++k) accp = fma((double)g[SL_V + k], dp[19 + k], accp);
      gpar += accp;                    // (meaningful in lanes 34..63)
      gL = adj_dot19(lm, val, gL);     // lambda_{j+1} . y_s,j, the same in every lane
    }
    // lanes 0..18: component `lane` of J_j^T [ds lambda_{j+1}; g_z[j]] in y; 19..30: in the history; 31..33: in tf
    lm = ((double)g[yslot] + lm) + acc;  // (meaningful in lanes 0..18, and read from there only)
    gtf += acc;                           // (... in lanes 31..33)
    if (lane >= 19 && lane < KR_SLOTS + 19) {
      const int slot = lane - 19;  // 0..11: the history slots; 12..27: structurally zero and the pads
      const T vc = slot < 12 ? (T)(c1 * acc) : (T)0, vp = slot < 12 ? (T)(c2 * acc) : (T)0;
      if (oc) oc[(int64_t)j * KR_SLOTS + slot] = vc;
      if (op) op[(int64_t)j * KR_SLOTS + slot] = vp;
    }
  }
  // lambda_0: the (n, m) rows are the total derivative with respect to G - zero at the root
  const double r7 = adj_bcast<7>(lm), r8 = adj_bcast<8>(lm), r9 = adj_bcast<9>(lm), r10 = adj_bcast<10>(lm),
               r11 = adj_bcast<11>(lm), r12 = adj_bcast<12>(lm);
  const double rmax = fmax(fmax(fmax(fabs(r7), fabs(r8)), fmax(fabs(r9), fabs(r10))), fmax(fabs(r11), fabs(r12)));
  if (A.resid && lane == 0) A.resid[rod * A.st_stride] = anorm > 0.0 ? rmax / anorm : 0.0;
  if (ot) {
    const double t0 = adj_bcast<31>(gtf), t1 = adj_bcast<32>(gtf), t2 = adj_bcast<33>(gtf);
    if (lane < 4) ot[lane] = (T)(P.tdirs[3 * lane] * t0 + P.tdirs[3 * lane + 1] * t1 + P.tdirs[3 * lane + 2] * t2);
  }
  if (ob && lane < 19) {
    // KR_BND order: p0 (3), h0 (4), q0 (3), w0 (3), F_tip (3), M_tip (3); y rows: p h n m q w.  The tip wrench enters
    // the tip condition only, (n, m)_{N-1} = (F_tip, M_tip): its gradient is -nu
    const int k = lane < 7 ? lane : (lane < 13 ? lane + 6 : lane - 6);
    ob[k] = (T)(lane >= 7 && lane < 13 ? -nu_l : lm);
  }
  if constexpr (PAR) {
    // KR_PAR order: E, r, rho, L, vstar, g, Bse, Bbt, C, tendon_dirs.  L enters ds = L / (N - 1) alone; tendon_dirs enters
    // tf = tensions @ tendon_dirs alone
    T* opar = Q.g_par + rod * KR_PAR;
    const double t0 = adj_bcast<31>(gtf), t1 = adj_bcast<32>(gtf), t2 = adj_bcast<33>(gtf);
    if (lane >= ADJ_PAR_LANE0) {
      const int k = lane - ADJ_PAR_LANE0;
      opar[k < 3 ? k : k + 1] = (T)gpar;
    }
    if (lane == 0) opar[3] = (T)(gL / (double)(N - 1));
    if (lane < 12) {
      const int i = lane / 3, c = lane - 3 * i;
      const double ti = i == 0 ? tens[0] : (i == 1 ? tens[1] : (i == 2 ? tens[2] : tens[3]));
      opar[31 + lane] = (T)(ti * (c == 0 ? t0 : (c == 1 ? t1 : t2)));
    }
  }
