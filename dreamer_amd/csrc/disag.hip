// Latent-disagreement ensemble (Plan2Explore, Sekar et al. 2020, as DreamerV3's expl.Disag): K small dr_mlp3 heads
// predict the posterior sample z_t from the hidden state h_t; the spread of their predictions is an intrinsic reward
// on imagined states (include/dreamer_hip.h).  Two row kernels (the disagreement of a row, the squared
// error and its gradient) and the composition of the members' forward / backward on the GEMM layer.  f32 in both
// precision modes: no GemmBf16Scope is opened here, and the weight-gradient products keep their three terms.
#include <algorithm>
#include <cstdio>

#include "engine_util.h"

// ---------------------------------------------------------------------------
// row kernels: one wave per row, DG_ROWS rows per workgroup; columns j = lane, lane + 64, ... summed per lane in
// ascending order, then wave_sum's fixed tree (4 DPP levels, 3 adds of the row totals)
// ---------------------------------------------------------------------------
#define DG_ROWS 4

// population std over the K members of column p[k * ks].  Deviations from member 0 (exactly 0 where the members
// agree, whatever K), minus their mean; scaled by 2^-e (e = exponent of the largest, exact) before the squares, so
// 1e-20 does not vanish in them and 1e+15 does not overflow.  A NaN / Inf member gives NaN.
__device__ __forceinline__ float disag_col_std(int K, const float* __restrict__ p, long long ks) {
  float dev[DR_DISAG_MAX_MEMBERS];
  const float p0 = p[0];
  dev[0] = p0 - p0;  // 0, or NaN for a non-finite member 0 (also at K = 1)
  float s = dev[0];
#pragma unroll
  for (int k = 1; k < DR_DISAG_MAX_MEMBERS; ++k) {
    dev[k] = 0.f;
    if (k < K) {
      dev[k] = p[k * ks] - p0;
      s += dev[k];
    }
  }
  const float mean = s / (float)K;
  float amax = 0.f, chk = 0.f;
#pragma unroll
  for (int k = 0; k < DR_DISAG_MAX_MEMBERS; ++k)
    if (k < K) {
      dev[k] = dev[k] - mean;
      amax = fmaxf(amax, fabsf(dev[k]));
      chk += dev[k] * 0.f;  // NaN iff a deviation is NaN / Inf (fmaxf drops NaN)
    }
  if (!(chk == 0.f)) return chk;
  if (amax == 0.f) return 0.f;
  const int e = (int)((__float_as_uint(amax) >> 23) & 0xFFu) - 127;
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < DR_DISAG_MAX_MEMBERS; ++k)
    if (k < K) {
      const float r = ldexpf(dev[k], -e);
      ss += r * r;
    }
  return ldexpf(sqrtf(ss / (float)K), e);
}

// d[m] = mean over the L columns of the members' std; optionally rew = w_ext * rew + w_int * d in place on a strided
// reward array (include/dreamer_hip.h, dr_disag_fwd)
__global__ __launch_bounds__(64 * DG_ROWS) void k_disag_var(int K, int M, int L, const float* __restrict__ pred,
                                                            long long kstride, long long ldp, float* d_out, float* rew,
                                                            int rew_T, int rew_skip, long long rew_sb,
                                                            long long rew_st, float w_ext, float w_int) {
  const int row = blockIdx.x * DG_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* p = pred + (long long)row * ldp;
  float acc = 0.f;
#pragma unroll 2  // (two columns' K loads in flight per lane; the default unroll took 203 VGPRs)
  for (int j = lane; j < L; j += 64) acc += disag_col_std(K, p + j, kstride);
  const float d = wave_sum(acc) / (float)L;
  if (lane != 0) return;
  if (d_out) d_out[row] = d;
  if (!rew) return;
  long long at;
  if (rew_T > 0) {
    const int b = row / rew_T, t = row % rew_T;
    if (t < rew_skip) return;
    at = b * rew_sb + (long long)(t - rew_skip) * rew_st;
  } else {
    at = row * rew_st;
  }
  const float a = w_ext * rew[at], c = w_int * d;
  rew[at] = a + c;
}

// g[k][m][j] = (p_k - z) * scale (scale = 2 / (K M L)), rowsum[k][m] = sum_j (p_k - z)^2
__global__ __launch_bounds__(64 * DG_ROWS) void k_disag_mse(int M, int L, const float* __restrict__ pred,
                                                            long long kstride, long long ldp,
                                                            const float* __restrict__ z, long long ldz, float scale,
                                                            float* __restrict__ g, float* __restrict__ rowsum) {
  const int row = blockIdx.x * DG_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63, k = blockIdx.y;
  if (row >= M) return;
  const float* p = pred + k * kstride + (long long)row * ldp;
  const float* zr = z + (long long)row * ldz;
  float* gr = g + ((long long)k * M + row) * L;
  float acc = 0.f;
  for (int j = lane; j < L; j += 64) {
    const float diff = p[j] - zr[j];
    gr[j] = diff * scale;
    acc += diff * diff;
  }
  acc = wave_sum(acc);
  if (lane == 0) rowsum[(long long)k * M + row] = acc;
}

// losses[1 + k] = (sum_m rowsum[k][m]) / (M L), losses[0] = their mean.  One 256-thread workgroup: per member the
// rows m = tid, tid + 256, ... per thread in ascending order, wave_sum, the four wave totals in order; members in order
__global__ __launch_bounds__(256) void k_disag_loss(int K, int M, int L, const float* __restrict__ rowsum,
                                                    float* __restrict__ losses) {
  __shared__ float part[4];
  const int tid = threadIdx.x;
  const float n = (float)((double)M * (double)L);
  float total = 0.f;
  for (int k = 0; k < K; ++k) {
    float t = 0.f;
    for (int m = tid; m < M; m += 256) t += rowsum[(long long)k * M + m];
    t = wave_sum(t);
    if ((tid & 63) == 0) part[tid >> 6] = t;
    __syncthreads();
    if (tid == 0) {
      const float lk = (((part[0] + part[1]) + part[2]) + part[3]) / n;
      losses[1 + k] = lk;
      total += lk;
    }
    __syncthreads();
  }
  if (tid == 0) losses[0] = total / (float)K;
}

static int disag_var(int K, int M, int L, const float* pred, long long kstride, long long ldp, float* d_out, float* rew,
                     int rew_T, int rew_skip, long long rew_sb, long long rew_st, float w_ext, float w_int,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_disag_var, dim3(dr_cdiv(M, DG_ROWS)), dim3(64 * DG_ROWS), 0, s, K, M, L, pred, kstride, ldp,
                     d_out, rew, rew_T, rew_skip, rew_sb, rew_st, w_ext, w_int);
  return dr_check_launch("disag_var");
}
static int disag_mse(int K, int M, int L, const float* pred, long long kstride, long long ldp, const float* z,
                     long long ldz, float* g, float* rowsum, float* losses, hipStream_t s) {
  const float scale = (float)(2.0 / ((double)K * (double)M * (double)L));
  hipLaunchKernelGGL(k_disag_mse, dim3(dr_cdiv(M, DG_ROWS), K), dim3(64 * DG_ROWS), 0, s, M, L, pred, kstride, ldp, z,
                     ldz, scale, g, rowsum);
  DR_TRY(dr_check_launch("disag_mse"));
  hipLaunchKernelGGL(k_disag_loss, dim3(1), dim3(256), 0, s, K, M, L, rowsum, losses);
  return dr_check_launch("disag_loss");
}

// ---------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------
struct DisagWs {
  // forward: layer 0 of all members side by side ([M][K W]: member k = columns k W ..), its LN-SiLU; layers 3 / 6
  // member-major ([K][M][W], [K][M][L])
  float *p1, *x1, *p2, *x2, *pred;
  // training: dL/dp [K][M][L], the row sums, per group of <= 4 members the layer-6 / layer-3 input gradients and
  // the LN-backward outputs of layer 4 ([4][M][W] each), layer 1's for all members ([M][K W])
  float *g, *rowsum, *gx2, *gp2, *gy2, *xh2, *gx1, *gp1, *gy1, *xh1;
  void* tn;
  size_t tn_bytes;
};
static void disag_carve(Carve& c, int K, int W, int Hd, int L, int M, int train, bool own_pred, DisagWs& w) {
  const long long KW = (long long)K * W, m = M;
  memset(&w, 0, sizeof(w));
  w.p1 = c.f(m * KW); w.x1 = c.f(m * KW);
  w.p2 = c.f(m * KW); w.x2 = c.f(m * KW);
  if (own_pred) w.pred = c.f(m * K * L);
  if (!train) return;
  const long long g4 = 4 * m * W;
  w.g = c.f(m * K * L); w.rowsum = c.f(m * K);
  w.gx2 = c.f(g4); w.gp2 = c.f(g4); w.gy2 = c.f(g4); w.xh2 = c.f(g4); w.gx1 = c.f(g4);
  w.gp1 = c.f(m * KW); w.gy1 = c.f(m * KW); w.xh1 = c.f(m * KW);
  size_t mx = std::max(op_gemm_tn_split3_ws_bytes(L, W, M), op_gemm_tn_split3_ws_bytes(W, W, M));
  mx = std::max(tn_group_bytes(mx, 4), op_gemm_tn_split3_ws_bytes((int)KW, Hd, M));
  w.tn_bytes = mx;
  w.tn = c.raw(mx);
}

static int disag_check(const char* fn, const dr_ensemble* e, int Hd, int L, int M) {
  if (!e || e->K < 1 || e->K > DR_DISAG_MAX_MEMBERS || e->W < 1 || Hd < 1 || L < 1 || M < 1) {
    dr_set_error("%s: needs 1 <= K <= %d and positive W, Hd, L, M", fn, DR_DISAG_MAX_MEMBERS);
    return DR_E_INVALID;
  }
  if ((long long)M * e->K * std::max(e->W, L) >= (1LL << 30)) {
    dr_set_error("%s: M K max(W, L) must stay below 2^30", fn);
    return DR_E_INVALID;
  }
  for (int k = 0; k < e->K; ++k) {
    const dr_mlp3& m = e->m[k];
    const float* ptrs[] = {m.l0.w, m.l0.b, m.n1.w, m.n1.b, m.l3.w, m.l3.b, m.n4.w, m.n4.b, m.l6.w, m.l6.b};
    for (const float* p : ptrs)
      if (!p) {
        dr_set_error("%s: member %d has a null parameter", fn, k);
        return DR_E_INVALID;
      }
    if (m.l0.w != e->m[0].l0.w + (long long)k * e->W * Hd || m.l0.b != e->m[0].l0.b + (long long)k * e->W) {
      dr_set_error("%s: the members' l0 parameters must be contiguous (member %d)", fn, k);
      return DR_E_INVALID;
    }
  }
  return DR_OK;
}

extern "C" size_t dr_disag_workspace_bytes(int K, int W, int Hd, int L, int M, int train) {
  if (K < 1 || K > DR_DISAG_MAX_MEMBERS || W < 1 || Hd < 1 || L < 1 || M < 1) return 0;
  Carve c(nullptr);
  DisagWs w;
  disag_carve(c, K, W, Hd, L, M, train, true, w);
  return c.off;
}

// the members' forward: layer 0 of all members as one product (N = K W), layers 3 and 6 in grouped launches of up to
// four members, the LayerNorm + SiLU of the previous layer over the member's column slice on load
static int disag_forward(const dr_ensemble* e, int Hd, int L, int M, const float* h, long long ldh, const DisagWs& w,
                         float* pred, hipStream_t s) {
  const int K = e->K, W = e->W;
  const long long KW = (long long)K * W;
  DR_TRY(run(G_NT, AM_PLAIN, lin(M, (int)KW, Hd, h, ldh, e->m[0].l0.w, Hd, e->m[0].l0.b, w.p1, KW), s));
  GemmArgs p[4];
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int n = std::min(4, K - k0);
    for (int i = 0; i < n; ++i) {
      const int k = k0 + i;
      const dr_mlp3& m = e->m[k];
      p[i] = lin_ln(M, W, W, w.p1 + (long long)k * W, KW, m.n1, m.l3.w, m.l3.b, w.p2 + (long long)k * M * W, W);
      p[i].a_out = w.x1 + (long long)k * W; p[i].ld_aout = KW;
    }
    DR_TRY(gemm_launch(G_NT, AM_LNSILU, p, n, s));
  }
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int n = std::min(4, K - k0);
    for (int i = 0; i < n; ++i) {
      const int k = k0 + i;
      const dr_mlp3& m = e->m[k];
      p[i] = lin_ln(M, L, W, w.p2 + (long long)k * M * W, W, m.n4, m.l6.w, m.l6.b, pred + (long long)k * M * L, L);
      p[i].a_out = w.x2 + (long long)k * M * W; p[i].ld_aout = W;
    }
    DR_TRY(gemm_launch(G_NT, AM_LNSILU, p, n, s));
  }
  return DR_OK;
}

extern "C" int dr_disag_fwd(const dr_ensemble* e, int Hd, int L, int M, const float* h, long long ldh, float* pred_out,
                            float* disag_out, float* rew, int rew_T, int rew_skip, long long rew_sb, long long rew_st,
                            float w_ext, float w_int, void* ws, size_t ws_bytes, hipStream_t stream) {
  DR_TRY(disag_check(__func__, e, Hd, L, M));
  DR_REQUIRE(h && ldh >= Hd && ws, "null input or workspace, or a row stride below Hd");
  DR_REQUIRE(pred_out || disag_out || rew, "no output asked for");
  DR_REQUIRE(!rew || (rew_T >= 0 && rew_skip >= 0 && (rew_T == 0 || rew_skip < rew_T)), "bad reward row mapping");
  Carve c(ws);
  DisagWs w;
  disag_carve(c, e->K, e->W, Hd, L, M, 0, pred_out == nullptr, w);
  WS_CHECK(c, ws_bytes);
  float* pred = pred_out ? pred_out : w.pred;
  DR_TRY(disag_forward(e, Hd, L, M, h, ldh, w, pred, stream));
  if (!disag_out && !rew) return DR_OK;
  return disag_var(e->K, M, L, pred, (long long)M * L, L, disag_out, rew, rew_T, rew_skip, rew_sb, rew_st, w_ext,
                   w_int, stream);
}

extern "C" int dr_disag_train_grads(const dr_ensemble* e, int Hd, int L, int M, const float* h, long long ldh,
                                    const float* z, long long ldz, const dr_ensemble* g, float* losses, void* ws,
                                    size_t ws_bytes, hipStream_t stream) {
  DR_TRY(disag_check(__func__, e, Hd, L, M));
  DR_REQUIRE(g && g->K == e->K && g->W == e->W, "the gradient ensemble must have the weights' K and W");
  DR_TRY(disag_check(__func__, g, Hd, L, M));
  DR_REQUIRE(h && ldh >= Hd && z && ldz >= L && losses && ws, "null operand, or a row stride below the width");
  hipStream_t s = stream;
  const int K = e->K, W = e->W;
  const long long KW = (long long)K * W, MW = (long long)M * W;
  Carve c(ws);
  DisagWs w;
  disag_carve(c, K, W, Hd, L, M, 1, true, w);
  WS_CHECK(c, ws_bytes);
  DR_TRY(disag_forward(e, Hd, L, M, h, ldh, w, w.pred, s));
  DR_TRY(disag_mse(K, M, L, w.pred, (long long)M * L, L, z, ldz, w.g, w.rowsum, losses, s));
  GemmArgs p[4];
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int n = std::min(4, K - k0);
    // through layer 6 (the weight as stored: an NN product), LayerNorm 4 + SiLU, layer 3, LayerNorm 1 + SiLU
    for (int i = 0; i < n; ++i)
      p[i] = bwd_in(M, W, L, w.g + (long long)(k0 + i) * M * L, L, e->m[k0 + i].l6.w, W, w.gx2 + i * MW, W, 0);
    DR_TRY(gemm_launch(G_NN, AM_PLAIN, p, n, s));
    for (int i = 0; i < n; ++i) {
      const dr_mlp3& m = e->m[k0 + i];
      DR_TRY(op_ln_silu_bwd(M, W, w.gx2 + i * MW, W, w.p2 + (k0 + i) * MW, W, m.n4.w, m.n4.b, w.gp2 + i * MW, W,
                            w.gy2 + i * MW, w.xh2 + i * MW, s));
    }
    for (int i = 0; i < n; ++i)
      p[i] = bwd_in(M, W, W, w.gp2 + i * MW, W, e->m[k0 + i].l3.w, W, w.gx1 + i * MW, W, 0);
    DR_TRY(gemm_launch(G_NN, AM_PLAIN, p, n, s));
    for (int i = 0; i < n; ++i) {
      const long long col = (long long)(k0 + i) * W;
      const dr_mlp3& m = e->m[k0 + i];
      DR_TRY(op_ln_silu_bwd(M, W, w.gx1 + i * MW, W, w.p1 + col, KW, m.n1.w, m.n1.b, w.gp1 + col, KW, w.gy1 + col,
                            w.xh1 + col, s));
    }
    // weight gradients of layers 6 and 3 (one grouped launch each), then the bias / LayerNorm column sums
    for (int i = 0; i < n; ++i)
      p[i] = bwd_w(L, W, M, w.g + (long long)(k0 + i) * M * L, L, w.x2 + (k0 + i) * MW, W, g->m[k0 + i].l6.w);
    DR_TRY(tn_launch(p, n, w.tn, w.tn_bytes, s));
    for (int i = 0; i < n; ++i)
      p[i] = bwd_w(W, W, M, w.gp2 + i * MW, W, w.x1 + (long long)(k0 + i) * W, KW, g->m[k0 + i].l3.w);
    DR_TRY(tn_launch(p, n, w.tn, w.tn_bytes, s));
    for (int i = 0; i < n; ++i) {
      const long long col = (long long)(k0 + i) * W;
      const dr_mlp3& gm = g->m[k0 + i];
      const float* gk = w.g + (long long)(k0 + i) * M * L;
      ColsumJob cj[6] = {
          {L, gk, L, nullptr, 0, gm.l6.b},
          {W, w.gp2 + i * MW, W, nullptr, 0, gm.l3.b},
          {W, w.gy2 + i * MW, W, w.xh2 + i * MW, W, gm.n4.w},
          {W, w.gy2 + i * MW, W, nullptr, 0, gm.n4.b},
          {W, w.gy1 + col, KW, w.xh1 + col, KW, gm.n1.w},
          {W, w.gy1 + col, KW, nullptr, 0, gm.n1.b},
      };
      DR_TRY(op_colsum_multi(M, cj, 6, s));
    }
  }
  // layer 0 of all members at once: dW0 [K W][Hd] = gp1^T h, db0 = column sums of gp1
  GemmArgs g0 = bwd_w((int)KW, Hd, M, w.gp1, KW, h, ldh, g->m[0].l0.w);
  DR_TRY(tn_launch(&g0, 1, w.tn, w.tn_bytes, s));
  return op_colsum(M, (int)KW, w.gp1, KW, nullptr, 0, g->m[0].l0.b, 0, s);
}

// ---------------------------------------------------------------------------
// Test hook (tests/test_gpu_disag.py): one of the two row kernels alone on caller-made predictions, through the
// launchers above.  Not in the public header.
//   var  v K M L kstride ldp rew_T rew_skip rew_sb rew_st; num w_ext w_int   ptrs pred d rew        (d or rew optional)
//   mse  v K M L kstride ldp ldz                                             ptrs pred z g rowsum losses
// ---------------------------------------------------------------------------
enum { DG_VAR, DG_MSE, DG_COUNT };
static int disag_run(int op, const int* v, const double* num, void* const* ptrs, hipStream_t s) {
  DR_REQUIRE(v && ptrs, "null descriptor or pointer array");
  DR_REQUIRE(op >= 0 && op < DG_COUNT, "unknown op");
  const int K = v[0], M = v[1], L = v[2];
  DR_REQUIRE(K >= 1 && K <= DR_DISAG_MAX_MEMBERS && M >= 1 && L >= 1, "needs 1 <= K <= 16 and positive M, L");
  DR_REQUIRE(v[4] >= L && (K == 1 || v[3] >= (long long)(M - 1) * v[4] + L), "member or row stride below the data");
  auto F = [&](int i) { return (float*)ptrs[i]; };
  if (op == DG_VAR) {
    DR_REQUIRE(ptrs[0] && (ptrs[1] || ptrs[2]), "null operand");
    DR_REQUIRE(!ptrs[2] || (num && v[5] >= 0 && v[6] >= 0 && (v[5] == 0 || v[6] < v[5])), "bad reward row mapping");
    return disag_var(K, M, L, F(0), v[3], v[4], F(1), F(2), v[5], v[6], v[7], v[8], num ? (float)num[0] : 0.f,
                     num ? (float)num[1] : 0.f, s);
  }
  DR_REQUIRE(ptrs[0] && ptrs[1] && ptrs[2] && ptrs[3] && ptrs[4], "null operand");
  DR_REQUIRE(v[5] >= L, "row stride below L");
  return disag_mse(K, M, L, F(0), v[3], v[4], F(1), v[5], F(2), F(3), F(4), s);
}

extern "C" int dr_internal_disag_run(int op, const int* v, const double* num, void* const* ptrs, void* stream,
                                     char* msg, int msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  const int rc = disag_run(op, v, num, ptrs, (hipStream_t)stream);
  if (rc != DR_OK && msg && msg_cap > 0) snprintf(msg, msg_cap, "%s", dr_last_error());
  return rc;
}
