// kr_mlp_fused_bodies.inc - the bodies of the kernels an epoch of kr_train_epoch launches, as text: included once by the
// one-network kernel and once by its bank form (kr_mlp_fused.hip), each under its own meaning of
//   KR_BX / KR_NBX   the workgroup's index and the number of workgroups that share the network's work:
//                    blockIdx.x / gridDim.x in the one-network kernels, network k's own decomposition in the bank kernels;
//   KR_TE            (tail) where the per-epoch fields are read: the TailArgs themselves, or the bank's TailStep;
// and with the arguments named A (FusedArgs), P (PackArgs), T (TailArgs) in scope.  Text, not functions: handing the kernel
// arguments to an inlined function by reference changes the code hipcc generates for the EXISTING kernels (fwd2: 193 -> 217
// VGPRs; tools/tab_asm_compare.py part 1), and this form leaves their token stream as it was.
// Select a body with KR_BODY_<NAME> before the #include.

#ifdef KR_BODY_PACK
  const int tid = KR_BX * blockDim.x + threadIdx.x, nth = KR_NBX * blockDim.x;
  for (int k = 0; k < P.L; ++k) {
    const float* __restrict__ W = P.W[k];
    const int in = P.in[k], out = P.out[k], ks = P.ks[k];
    const int n = P.tiles[k] * ks * 64;
    for (int i = tid; i < n; i += nth) {
      // element i = ((t * ks / 4 + s / 4) * 64 + lane) * 4 + s % 4: four consecutive k-steps of a lane are ONE 16-byte load
      const int e = i & 3, lane = (i >> 2) & 63, g = (i >> 8) % (ks / 4), t = (i >> 8) / (ks / 4);
      const int s = 4 * g + e;
      const int uo = 16 * t + (lane & 15), q = lane >> 4;
      const int ui = k == 0 ? 4 * s + q : 16 * (s / 4) + 4 * q + (s % 4);
      P.wf[k][i] = (uo < out && ui < in) ? W[(size_t)uo * in + ui] : 0.f;
    }
    const int nb = P.tiles[k] * 4 * 64;
    for (int i = tid; i < nb; i += nth) {
      const int lane = i & 63, r = (i >> 6) & 3, t = i >> 8;
      const int u = 16 * t + 4 * (lane >> 4) + r;
      P.bf[k][i] = u < out ? P.b[k][u] : 0.f;
    }
    if (k > 0) {
      const int kst = P.kst[k];
      const int nt = P.in_tiles[k] * kst * 64;
      for (int i = tid; i < nt; i += nth) {
        const int e = i & 3, lane = (i >> 2) & 63, g = (i >> 8) % (kst / 4), ti = (i >> 8) / (kst / 4);
        const int s = 4 * g + e;
        const int ui = 16 * ti + (lane & 15), q = lane >> 4;
        const int uo = P.natural[k] ? 4 * s + q : 16 * (s / 4) + 4 * q + (s % 4);
        P.wt[k][i] = (uo < out && ui < in) ? W[(size_t)uo * in + ui] : 0.f;
      }
    }
  }
#endif  // KR_BODY_PACK

#ifdef KR_BODY_FWD2
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c1 = A.c1;
  float* const wl0 = wg_lds;
  float* const wl1 = wl0 + c1 * 2048;
  float* const bl1 = wl1 + c1 * 2048;
  float* const bl2 = bl1 + 64 * c1;
  float* const to = bl2 + 32 + wv * FW2_OUT;
  {
    const int t = threadIdx.x;
    const f4* s0 = reinterpret_cast<const f4*>(A.wf[0]);
    const f4* s1 = reinterpret_cast<const f4*>(A.wf[1]);
    f4* d0 = reinterpret_cast<f4*>(wl0);
    f4* d1 = reinterpret_cast<f4*>(wl1);
    for (int i = t; i < c1 * 512; i += 64 * FW2) { d0[i] = s0[i]; d1[i] = s1[i]; }
    for (int u = t; u < 64 * c1; u += 64 * FW2) bl1[u] = A.bfr[0][((u >> 4) * 4 + (u & 3)) * 64 + 16 * ((u & 15) >> 2)];
    if (t < 32) bl2[t] = A.bfr[1][((t >> 4) * 4 + (t & 3)) * 64 + 16 * ((t & 15) >> 2)];
  }
  __syncthreads();
  const int64_t nblk = (A.Q + FR - 1) / FR;
  const bool with_loss = A.lbase != nullptr;
  const int gid = KR_BX * FW2 + wv;
  const int c = lane & 15, g = lane >> 4;
  float loss_part = 0.f;
  for (int64_t rb = gid; rb < nblk; rb += (int64_t)KR_NBX * FW2) {
    float bin[FT][8];
#pragma unroll
    for (int s = 0; s < FT; ++s) {
      const int64_t row = rb * FR + 16 * s + c;
      const float* xr = A.x + (row < A.Q ? row : A.Q - 1) * F_LDX + g;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float v = xr[4 * k];
        bin[s][k] = row < A.Q ? v : 0.f;
      }
    }
    constexpr int LNV = (FR * 25 / 4 + 63) / 64;
    f4 lvb[LNV], lvt[LNV];
    if (with_loss) {
      const int64_t e0 = rb * FR * 25, eN = A.Q * 25;
      const f4* sb = reinterpret_cast<const f4*>(A.lbase + e0);
      const f4* st = reinterpret_cast<const f4*>(A.ltarget + e0);
#pragma unroll
      for (int q = 0; q < LNV; ++q) {
        const int i = lane + 64 * q;
        lvb[q] = f4{0.f, 0.f, 0.f, 0.f};
        lvt[q] = f4{1.f, 0.f, 0.f, 0.f};
        if (i < FR * 25 / 4) {
          if (e0 + 4 * i + 3 < eN) {
            lvb[q] = sb[i];
            lvt[q] = st[i];
          } else {
            for (int cc = 0; cc < 4; ++cc)
              if (e0 + 4 * i + cc < eN) { lvb[q][cc] = A.lbase[e0 + 4 * i + cc]; lvt[q][cc] = A.ltarget[e0 + 4 * i + cc]; }
          }
        }
      }
    }
    f4 oacc[2][FT];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const f4 b = *reinterpret_cast<const f4*>(bl2 + 16 * o + 4 * g);
#pragma unroll
      for (int s = 0; s < FT; ++s) oacc[o][s] = b;
    }
    for (int ch = 0; ch < c1; ++ch) {
      FChunk h;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const f4 b = *reinterpret_cast<const f4*>(bl1 + 64 * ch + 16 * o + 4 * g);
#pragma unroll
        for (int s = 0; s < FT; ++s) h.a[o][s] = b;
      }
      facc<4, 8>(h.a, wl0, 8, 4 * ch, 0, lane, [&](int s, int k) { return bin[s][k]; });
      chunk_act_only<ACT>(h);
      facc<2, 16>(oacc, wl1, 16 * c1, 0, 16 * ch, lane, [&](int s, int k) { return h.a[k >> 2][s][k & 3]; });
    }
    fwd2_epilogue(A, to, lvb, lvt, oacc, rb, lane, loss_part);
  }
  if (with_loss) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) loss_part += __shfl_xor(loss_part, m, 64);
    if (lane == 0) A.lpart[gid] = loss_part;
  }
#endif  // KR_BODY_FWD2

#ifdef KR_BODY_FWD3
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* const wl = wg_lds;
  {
    const int t = threadIdx.x;
    const f4* s0 = reinterpret_cast<const f4*>(A.wf[0]);
    const f4* s1 = reinterpret_cast<const f4*>(A.wf[1]);
    const f4* s2 = reinterpret_cast<const f4*>(A.wf[2]);
    f4* d = reinterpret_cast<f4*>(wl);
    for (int i = t; i < FW3_W1 / 4; i += 64 * FW3) d[FW3_W0 / 4 + i] = s0[i];
    for (int i = t; i < (FW3_W2 - FW3_W1) / 4; i += 64 * FW3) d[FW3_W1 / 4 + i] = s1[i];
    for (int i = t; i < (FW3_B - FW3_W2) / 4; i += 64 * FW3) d[FW3_W2 / 4 + i] = s2[i];
    if (t < 160) {  // compact biases out of the bias fragments: b[u] sits at fragment slot ((u / 16) 4 + u % 4) 64 + 16 ((u % 16) / 4)
      const int k = t < 64 ? 0 : t < 128 ? 1 : 2, u = t - 64 * k;
      wl[FW3_B + t] = A.bfr[k][((u >> 4) * 4 + (u & 3)) * 64 + 16 * ((u & 15) >> 2)];
    }
  }
  __syncthreads();
  float* const tx = wg_lds + FW3_FRAG + wv * FW3_WAVE;
  float* const tbt = tx + 2 * FR * F_LDX;
  const int gid = KR_BX * FW3 + wv;
  fwd_rows<ACT, true>(A, tx, tbt, wl, lane, gid, (int64_t)KR_NBX * FW3, gid);
#endif  // KR_BODY_FWD3

#ifdef KR_BODY_BWD3
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* const tu = wg_lds + wv * BW3_LDS;  // dOUT^T, then A1, then dZ1
  float* const tv = tu + 64 * TP;           // A2, then dZ2, then X^T
  float* const wl3 = wg_lds + BW3 * BW3_LDS;  // W3^T fragments: 4 x 8 x 64
  float* const wl2 = wl3 + B3A_WT;            // W2^T fragments: 4 x 16 x 64
  {
    const f4* s3 = reinterpret_cast<const f4*>(A.wt[2]);
    const f4* s2 = reinterpret_cast<const f4*>(A.wt[1]);
    f4* d3 = reinterpret_cast<f4*>(wl3);
    f4* d2 = reinterpret_cast<f4*>(wl2);
    for (int i = threadIdx.x; i < B3A_WT / 4; i += 64 * BW3) d3[i] = s3[i];
    for (int i = threadIdx.x; i < B3B_WT / 4; i += 64 * BW3) d2[i] = s2[i];
  }
  __syncthreads();
  const int64_t nblk = (A.Q + FR - 1) / FR;
  const int64_t wave0 = (int64_t)KR_BX * BW3 + wv, nwaves = (int64_t)KR_NBX * BW3;
  f4 aW1[4][2], aW2[4][4], aW3[2][4];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
#pragma unroll
    for (int i = 0; i < 2; ++i) aW1[o][i] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) aW2[o][i] = f4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int i = 0; i < 4; ++i) aW3[o][i] = f4{0.f, 0.f, 0.f, 0.f};
  float pb1 = 0.f, pb2 = 0.f, pbo = 0.f;
  for (int64_t rb = wave0; rb < nblk; rb += nwaves) {
    stage_rows_T(A.dout, rb * FR, A.Q, tu, lane);
    FChunk d2;
    {
      FChunk h1;
      {
        FChunk h;
        chunk_undump(h, A.a2d, rb, lane);
        chunk_undump(h1, A.a1d, rb, lane);
        chunk_to_T(tv, h, lane);  // A2
      }
      fsync();
      if (lane < 32) pbo += row_sum_T(tu, lane);
      wgrad_T<2, 4>(aW3, tu, tv, lane);  // dW3 += dOUT^T A2
      chunk_zero(d2);
      float bd[FT][8];
      load_bops_T(bd, tu, lane);
      fsync();
      chunk_to_T(tu, h1, lane);  // A1 over dOUT^T
      facc<4, 8>(d2.a, wl3, 8, 0, 0, lane, [&](int s, int k) { return bd[s][k]; });
    }
    chunk_mul_grad_T<ACT>(d2, tv, lane);
    fsync();
    chunk_to_T(tv, d2, lane);  // dZ2 (A2 is consumed)
    fsync();
    pb2 += row_sum_T(tv, lane);
    wgrad_T<4, 4>(aW2, tv, tu, lane);  // dW2 += dZ2^T A1
    fsync();
    // ---- what used to be the second pass
    stage_rows_T(A.x, rb * FR, A.Q, tv, lane);  // X^T over dZ2 (its first 32 rows)
    FChunk d1;
    chunk_zero(d1);
    facc<4, 16>(d1.a, wl2, 16, 0, 0, lane, [&](int s, int k) { return d2.a[k >> 2][s][k & 3]; });
    chunk_mul_grad_T<ACT>(d1, tu, lane);
    fsync();
    chunk_to_T(tu, d1, lane);  // dZ1 (A1 is consumed)
    fsync();
    pb1 += row_sum_T(tu, lane);
    wgrad_T<4, 2>(aW1, tu, tv, lane);  // dW1 += dZ1^T X
    fsync();
  }
  wg_tree_sum<BW3>(aW2, aW3, pb2, pbo, wg_lds, wv, lane);
  {
    f4 none[1][1] = {{f4{0.f, 0.f, 0.f, 0.f}}};
    float unused = 0.f;
    wg_tree_sum<BW3>(aW1, none, pb1, unused, wg_lds, wv, lane);
  }
  if (wv != 0) return;
  float* slab = A.slab + (size_t)KR_BX * A.P;
  wgrad_flush<2, 4>(aW3, slab + A.poff[4], A.nout, A.h2, 0, 0, lane);
  wgrad_flush<4, 4>(aW2, slab + A.poff[2], A.h2, A.h1, 0, 0, lane);
  wgrad_flush<4, 2>(aW1, slab + A.poff[0], A.h1, A.in, 0, 0, lane);
  if (lane < A.h1) slab[A.poff[1] + lane] = pb1;
  if (lane < A.h2) slab[A.poff[3] + lane] = pb2;
  if (lane < A.nout) slab[A.poff[5] + lane] = pbo;
#endif  // KR_BODY_BWD3

#ifdef KR_BODY_BWD2
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* const ts = wg_lds + wv * B2_LDS;  // X^T, then dOUT^T, then X^T again
  float* const tu = ts + 32 * TP;          // A1
  float* const tv = tu;                    // dZ1 (A1 is consumed when it is written)
  float* const wl0 = wg_lds + WPB * B2_LDS;
  float* const wl1 = wl0 + 4 * 8 * 64;
  float* const bl = wl1 + 4 * 8 * 64;
  const int64_t nblk = (A.Q + FR - 1) / FR;
  const int nchunk = A.c1;
  const int chunk = KR_BX % nchunk;
  const int64_t group = KR_BX / nchunk, ngroups = KR_NBX / nchunk;
  {
    const f4* s0 = reinterpret_cast<const f4*>(A.wf[0] + (size_t)4 * chunk * 8 * 64);
    const f4* s1 = reinterpret_cast<const f4*>(A.wt[1] + (size_t)4 * chunk * 8 * 64);
    const f4* s2 = reinterpret_cast<const f4*>(A.bfr[0] + (size_t)4 * chunk * 4 * 64);
    f4* d0 = reinterpret_cast<f4*>(wl0);
    f4* d1 = reinterpret_cast<f4*>(wl1);
    f4* d2 = reinterpret_cast<f4*>(bl);
    for (int i = threadIdx.x; i < 512; i += 64 * WPB) { d0[i] = s0[i]; d1[i] = s1[i]; }
    for (int i = threadIdx.x; i < 256; i += 64 * WPB) d2[i] = s2[i];
  }
  __syncthreads();
  f4 aW1[4][2], aWo[2][4];
#pragma unroll
  for (int o = 0; o < 4; ++o)
#pragma unroll
    for (int i = 0; i < 2; ++i) aW1[o][i] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int i = 0; i < 4; ++i) aWo[o][i] = f4{0.f, 0.f, 0.f, 0.f};
  float pb1 = 0.f, pbo = 0.f;
  // the rows of X and dOUT of a block are requested while the previous block finishes (registers: the fragments in the
  // LDS freed 45 of them); X is staged twice from the same registers
  f4 xr[RNV], dr[RNV];
  {
    const int64_t rb = group * WPB + wv;
    rows_request(xr, A.x, rb * FR, rb < nblk ? A.Q : 0, lane);
    rows_request(dr, A.dout, rb * FR, rb < nblk ? A.Q : 0, lane);
  }
  for (int64_t rb = group * WPB + wv; rb < nblk; rb += ngroups * WPB) {
    rows_to_T(xr, ts, lane);
    fsync();
    {
      FChunk h1;
      float bin[FT][8];
      load_bops_T(bin, ts, lane);
      chunk_set_bias(h1, bl, 0, lane);
      facc<4, 8>(h1.a, wl0, 8, 0, 0, lane, [&](int s, int k) { return bin[s][k]; });
      fsync();
      rows_to_T(dr, ts, lane);
      chunk_act_only<ACT>(h1);
      chunk_to_T(tu, h1, lane);  // A1 chunk
    }
    fsync();
    if (chunk == 0 && lane < 32) pbo += row_sum_T(ts, lane);
    wgrad_T<2, 4>(aWo, ts, tu, lane);  // dW2[:, chunk] += dOUT^T A1
    // dZ1 = (W2^T[chunk] dOUT) * act'(Z1)
    FChunk d1;
    chunk_zero(d1);
    {
      float bd[FT][8];
      load_bops_T(bd, ts, lane);
      facc<4, 8>(d1.a, wl1, 8, 0, 0, lane, [&](int s, int k) { return bd[s][k]; });
    }
    chunk_mul_grad_T<ACT>(d1, tu, lane);
    fsync();
    rows_to_T(xr, ts, lane);
    {
      const int64_t rn = rb + ngroups * WPB;
      rows_request(xr, A.x, rn * FR, rn < nblk ? A.Q : 0, lane);
      rows_request(dr, A.dout, rn * FR, rn < nblk ? A.Q : 0, lane);
    }
    chunk_to_T(tv, d1, lane);
    fsync();
    pb1 += row_sum_T(tv, lane);
    wgrad_T<4, 2>(aW1, tv, ts, lane);  // dW1[chunk] += dZ1^T X
    fsync();
  }
  wg_tree_sum(aW1, aWo, pb1, pbo, wg_lds, wv, lane);
  if (wv != 0) return;
  float* slab = A.slab + (size_t)group * A.P;  // one slab per group of row-block streams; its chunks write disjoint parts
  wgrad_flush<2, 4>(aWo, slab + A.poff[2], A.nout, A.h1, 0, 64 * chunk, lane);
  wgrad_flush<4, 2>(aW1, slab + A.poff[0], A.h1, A.in, 64 * chunk, 0, lane);
  if (64 * chunk + lane < A.h1) slab[A.poff[1] + 64 * chunk + lane] = pb1;
  if (chunk == 0 && lane < A.nout) slab[A.poff[3] + lane] = pbo;
#endif  // KR_BODY_BWD2

#ifdef KR_BODY_TAIL
  __shared__ __attribute__((aligned(16))) float red[TAIL_G][64];
  __shared__ float lred[TAIL_T];
  const int tid = threadIdx.x, c0 = KR_BX * 64;
  // the optimizer state of this workgroup's parameters is requested first, so that it travels with the slabs
  float g_in = 0.f, p_in = 0.f, m_in = 0.f, v_in = 0.f, lo_in = 0.f;
  if (tid < 64 && c0 + tid <= T.nparams) {
    g_in = T.g[c0 + tid];
    if (T.update && c0 + tid < T.nparams) {
      p_in = T.p[c0 + tid];
      m_in = T.m[c0 + tid];
      v_in = T.v[c0 + tid];
      if (T.lower) lo_in = T.lower[c0 + tid];
    }
  }
  {
    const int l16 = tid & 15, sg = tid >> 4;
    f4 a0 = f4{0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
    if (c0 + 4 * l16 < T.P) {
      const float* src = T.slab + c0 + 4 * l16;
      int w = sg;
      for (; w + 3 * TAIL_G < T.nslab; w += 4 * TAIL_G) {
        const f4 v0 = *reinterpret_cast<const f4*>(src + (size_t)w * T.P);
        const f4 v1 = *reinterpret_cast<const f4*>(src + (size_t)(w + TAIL_G) * T.P);
        const f4 v2 = *reinterpret_cast<const f4*>(src + (size_t)(w + 2 * TAIL_G) * T.P);
        const f4 v3 = *reinterpret_cast<const f4*>(src + (size_t)(w + 3 * TAIL_G) * T.P);
        a0 = a0 + v0; a1 = a1 + v1; a2 = a2 + v2; a3 = a3 + v3;
      }
      for (; w < T.nslab; w += TAIL_G) a0 = a0 + *reinterpret_cast<const f4*>(src + (size_t)w * T.P);
    }
    *reinterpret_cast<f4*>(&red[sg][4 * l16]) = (a0 + a1) + (a2 + a3);
  }
  const bool loss_blk = T.nparams >= c0 && T.nparams < c0 + 64;  // (uniform over the workgroup)
  float lsum = 0.f;
  if (loss_blk && T.nlpart > 0) {
    for (int j = tid; j < T.nlpart; j += TAIL_T) lsum += T.lpart[j];
    lred[tid] = lsum;
  }
  __syncthreads();
  if (loss_blk && T.nlpart > 0) {
    for (int o = TAIL_T / 2; o > 0; o >>= 1) {
      if (tid < o) lred[tid] += lred[tid + o];
      __syncthreads();
    }
    lsum = lred[0];
  }
  if (T.nslab > 0) {  // 64 x TAIL_G partial sums -> 64 x 4 (every thread of the first four wavefronts adds sixteen)
    float part = 0.f;
    if (tid < 256) {
#pragma unroll
      for (int k = 0; k < TAIL_G / 4; ++k) part += red[(tid >> 6) * (TAIL_G / 4) + k][tid & 63];
    }
    __syncthreads();
    if (tid < 256) red[tid >> 6][tid & 63] = part;
    __syncthreads();
  }
  if (tid >= 64) return;
  const int i = c0 + tid;
  if (i > T.nparams) return;
  if (i == T.nparams) {  // the loss slot
    const float cur_f = g_in + lsum;
    if (!T.update) {
      T.g[i] = cur_f;
      return;
    }
    const double lr = T.sched[KR_TE.parity];
    const double cur = (double)cur_f;
    double best = T.sched[2], bad = T.sched[3], nred = T.sched[5];
    if (cur < best * (1.0 - KR_TE.threshold)) { best = cur; bad = 0.0; }
    else bad += 1.0;
    double next = lr;
    if (bad > (double)KR_TE.patience) {
      const double cand = fmax(lr * KR_TE.factor, KR_TE.min_lr);
      if (lr - cand > 1e-8) { next = cand; nred += 1.0; }
      bad = 0.0;
    }
    T.sched[KR_TE.parity ^ 1] = next;
    T.sched[2] = best; T.sched[3] = bad; T.sched[4] = cur; T.sched[5] = nred;
    if (KR_TE.loss_log) *KR_TE.loss_log = cur_f;
    T.g[i] = 0.f;
    return;
  }
  float gi = g_in;
  if (T.nslab > 0) gi += (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  if (!T.update) {
    T.g[i] = gi;
    return;
  }
  float pi = p_in;
  {
    const float step_size = (float)(T.sched[KR_TE.parity] * (double)KR_TE.inv_bc1);
    if (KR_TE.wd != 0.f) gi = fmaf(KR_TE.wd, pi, gi);
    const float mi = fmaf(KR_TE.b1, m_in, (1.f - KR_TE.b1) * gi);
    const float vi = fmaf(KR_TE.b2, v_in, (1.f - KR_TE.b2) * gi * gi);
    T.m[i] = mi;
    T.v[i] = vi;
    const float denom = sqrtf(vi) * KR_TE.inv_sqrt_bc2 + KR_TE.eps;
    pi -= step_size * (mi / denom);
    if (T.lower) pi = fmaxf(pi, lo_in);
    T.p[i] = pi;
    T.g[i] = 0.f;
  }
  int seg = 0;
#pragma unroll
  for (int k = 1; k < 6; ++k)
    if (i >= T.poff[k]) seg = k;
  const int k = seg >> 1, r = i - T.poff[seg];
  if (seg & 1) {  // bias b_k[u]: bf[(t*4 + r4)*64 + lane] = b[16 t + 4 (lane >> 4) + r4] for the sixteen lanes of a quad
    const int u = r;
    float* dst = T.bf[k] + ((size_t)(u >> 4) * 4 + (u & 3)) * 64 + 16 * ((u & 15) >> 2);
#pragma unroll
    for (int c = 0; c < 16; ++c) dst[c] = pi;
  } else {
    const int in = T.in[k], uo = r / in, ui = r - uo * in;
    {
      const int sfw = k == 0 ? ui >> 2 : 4 * (ui >> 4) + (ui & 3);
      const int q = k == 0 ? ui & 3 : (ui & 15) >> 2;
      const int lane = 16 * q + (uo & 15);
      T.wf[k][(((size_t)(uo >> 4) * (T.ks[k] >> 2) + (sfw >> 2)) * 64 + lane) * 4 + (sfw & 3)] = pi;
    }
    if (k > 0) {
      const int st = T.natural[k] ? uo >> 2 : 4 * (uo >> 4) + (uo & 3);
      const int q = T.natural[k] ? uo & 3 : (uo & 15) >> 2;
      const int lane = 16 * q + (ui & 15);
      T.wt[k][(((size_t)(ui >> 4) * (T.kst[k] >> 2) + (st >> 2)) * 64 + lane) * 4 + (st & 3)] = pi;
    }
  }
#endif  // KR_BODY_TAIL
