// Generic fused f32 GEMM for libdreamer_hip (see gemm.h).
//
// Tile: BM x BN per 256-thread workgroup (4 waves, 2x2 or 1x4), BK = 32.
// Operands are staged through LDS with a row stride of BK+2 floats, which
// makes the MFMA fragment reads (16 rows x 4 k per wave-instruction)
// conflict-free for ds_read_b32.  The next K-slice is prefetched into
// registers while the current one feeds the MFMAs.  Every product is an
// exact f32 fma (v_mfma_f32_16x16x4_f32), so results differ from the CPU
// oracle only by summation order.
#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <stdint.h>
#include <string.h>

#include "gemm.h"
#include "conv.h"  // dr_internal_gemm_run: weight planes and bf16 rows as the engine's callers make them

#include <algorithm>

#define BK 32
#define LDS_K (BK + 2)

struct GemmBatch {
  GemmArgs p[4];
};

// Grouped launches pack their problems' tiles into one linear grid (npack > 0):
// block b -> XCD-ordered logical tile over the concatenated tile lists, then
// (problem z, tile within z).  Without packing a blockIdx.z slice is sized for
// the largest problem and the smaller problems' surplus workgroups idle in it.
// Returns -1 for padding blocks; npack == 0 keeps blockIdx.z (lt = -2: the
// caller computes its tile from its own problem).
template <int BM, int BN>
__device__ __forceinline__ int dr_pack_tile(const GemmBatch& gb, int npack, int& z) {
  z = blockIdx.z;
  if (npack <= 0) return -2;
  int tot = 0;
  for (int i = 0; i < npack; ++i) tot += ((gb.p[i].M + BM - 1) / BM) * ((gb.p[i].N + BN - 1) / BN);
  int lt = dr_xcd_tile(blockIdx.x, tot);
  if (lt < 0) return -1;
  z = 0;
  for (int i = 0; i + 1 < npack; ++i) {
    const int ti = ((gb.p[i].M + BM - 1) / BM) * ((gb.p[i].N + BN - 1) / BN);
    if (lt < ti) break;
    lt -= ti;
    z = i + 1;
  }
  return lt;
}

static thread_local int g_gemm_bf16 = 0;
GemmBf16Scope::GemmBf16Scope(bool on) : prev(g_gemm_bf16) { g_gemm_bf16 = on ? 1 : 0; }
GemmBf16Scope::~GemmBf16Scope() { g_gemm_bf16 = prev; }

GemmArgs gemm_args() {
  GemmArgs g;
  memset(&g, 0, sizeof(g));
  g.bf16 = g_gemm_bf16;
  g.ksplitA = INT_MAX;
  g.ksplitB = INT_MAX;
  g.nsplitB = INT_MAX;
  g.nsplitY = INT_MAX;
  g.alpha = 1.0f;
  g.nb = 1;
  return g;
}

template <int AMODE>
__device__ __forceinline__ float load_a_mk(const GemmArgs& g, int m, int k, float mean, float rstd) {
  if (AMODE == AM_PLAIN) {
    if (k < g.ksplitA) return g.A[(long long)m * g.lda + k];
    return g.A2[(long long)m * g.lda2 + (k - g.ksplitA)];
  } else if (AMODE == AM_LNSILU) {
    float v = g.A[(long long)m * g.lda + k];
    float x = (v - mean) * rstd;
    x = x * g.ln_g[k] + g.ln_b[k];
    return x / (1.0f + expf(-x));
  } else if (AMODE == AM_CONV) {
    // NHWC activations, K ordered (ky, kx, ci) -- weights repacked to match
    const int hw = g.oh * g.ow;
    const int f = m / hw, pix = m - f * hw;
    const int oy = pix / g.ow, ox = pix - oy * g.ow;
    const int tap = k / g.cin, ci = k - tap * g.cin;
    const int iy = 2 * oy - 1 + (tap >> 2), ix = 2 * ox - 1 + (tap & 3);
    if (iy < 0 || iy >= g.ih || ix < 0 || ix >= g.iw) return 0.0f;
    return g.A[(((long long)f * g.ih + iy) * g.iw + ix) * g.cin + ci];
  } else {
    // first layer: NCHW frames from the replay ring (u8) or an f32 tensor,
    // K ordered like the PyTorch weight (ci, ky, kx)
    const int hw = g.oh * g.ow;
    const int f = m / hw, pix = m - f * hw;
    const int oy = pix / g.ow, ox = pix - oy * g.ow;
    const int ci = k >> 4, iy = 2 * oy - 1 + ((k >> 2) & 3), ix = 2 * ox - 1 + (k & 3);
    if (iy < 0 || iy >= g.ih || ix < 0 || ix >= g.iw) return 0.0f;
    const long long off = ((long long)ci * g.ih + iy) * g.iw + ix;
    const int b = f % g.nb, t = f / g.nb + g.src.t0;
    float v;
    if (g.src.ring) {
      const long long slot = (g.src.starts[b] + t) % g.src.ring_cap;
      v = (float)g.src.ring[slot * (long long)g.cin * g.ih * g.iw + off];
    } else {
      v = g.src.obs[(long long)b * g.src.stride_b + (long long)t * g.src.stride_t + off];
    }
    if (g.src.raw255) v = v / 255.0f - 0.5f;  // Dreamer.py:251 (IEEE div, then sub)
    return v;
  }
}

__device__ __forceinline__ float load_b(const GemmArgs& g, bool kn, int n, int k) {
  if (!kn) return dr_g(g.W)[(long long)n * g.ldb + k];
  if (k >= g.ksplitB) return dr_g(g.W2)[(long long)(k - g.ksplitB) * g.ldb2 + n];
  if (n >= g.nsplitB) return dr_g(g.W2)[(long long)k * g.ldb2 + (n - g.nsplitB)];
  return dr_g(g.W)[(long long)k * g.ldb + n];
}

template <int BM, int BN, int AMODE, bool A_KM, bool B_KN>
__global__ __launch_bounds__(256) void k_gemm(GemmBatch gb) {
  const GemmArgs& g = gb.p[blockIdx.z];  // kernarg pointers: the compiler keeps them global
  const int tiles_n = (g.N + BN - 1) / BN;
  const int tiles_m = (g.M + BM - 1) / BM;
  if ((int)blockIdx.x >= tiles_m * tiles_n) return;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int M = g.M, N = g.N, K = g.K;

  __shared__ float As[BM][LDS_K];
  __shared__ float Bs[BN][LDS_K];
  __shared__ float s_mean[BM], s_rstd[BM];

  if (AMODE == AM_LNSILU) {
    for (int r = wave; r < BM; r += 4) {
      const int m = m0 + r;
      float mean = 0.f, rstd = 0.f;
      if (m < M) {
        const float* row = g.A + (long long)m * g.lda;
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s += row[k];
        mean = wave_sum(s) / (float)K;
        float v = 0.f;
        for (int k = lane; k < K; k += 64) {
          const float d = row[k] - mean;
          v += d * d;
        }
        rstd = 1.0f / sqrtf(wave_sum(v) / (float)K + 1e-5f);
      }
      if (lane == 0) {
        s_mean[r] = mean;
        s_rstd[r] = rstd;
      }
    }
    __syncthreads();
  }

  constexpr int NA = BM * BK / 256, NB = BN * BK / 256;
  float ra[NA], rb[NB];
  const bool store_a = (g.a_out != nullptr) && (tn == 0);

  auto load_tiles = [&](int k0) {
    if (!A_KM) {
      const int kk = tid & 31, mb = tid >> 5;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int ml = mb + 8 * i, m = m0 + ml, k = k0 + kk;
        float v = 0.f;
        if (m < M && k < K) {
          v = load_a_mk<AMODE>(g, m, k, (AMODE == AM_LNSILU) ? s_mean[ml] : 0.f,
                               (AMODE == AM_LNSILU) ? s_rstd[ml] : 0.f);
          if (store_a) g.a_out[(long long)m * g.ld_aout + k] = v;
        }
        ra[i] = v;
      }
    } else {
      const int ml = tid % BM, kb = tid / BM;
#pragma unroll
      for (int i = 0; i < NA; ++i) {
        const int k = k0 + kb + (256 / BM) * i, m = m0 + ml;
        ra[i] = (m < M && k < K) ? g.A[(long long)k * g.lda + m] : 0.f;
      }
    }
    if (!B_KN) {
      const int kk = tid & 31, nb = tid >> 5;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int n = n0 + nb + 8 * i, k = k0 + kk;
        rb[i] = (n < N && k < K) ? load_b(g, false, n, k) : 0.f;
      }
    } else {
      const int nl = tid % BN, kb = tid / BN;
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int k = k0 + kb + (256 / BN) * i, n = n0 + nl;
        rb[i] = (n < N && k < K) ? load_b(g, true, n, k) : 0.f;
      }
    }
  };
  auto store_tiles = [&]() {
    if (!A_KM) {
      const int kk = tid & 31, mb = tid >> 5;
#pragma unroll
      for (int i = 0; i < NA; ++i) As[mb + 8 * i][kk] = ra[i];
    } else {
      const int ml = tid % BM, kb = tid / BM;
#pragma unroll
      for (int i = 0; i < NA; ++i) As[ml][kb + (256 / BM) * i] = ra[i];
    }
    if (!B_KN) {
      const int kk = tid & 31, nb = tid >> 5;
#pragma unroll
      for (int i = 0; i < NB; ++i) Bs[nb + 8 * i][kk] = rb[i];
    } else {
      const int nl = tid % BN, kb = tid / BN;
#pragma unroll
      for (int i = 0; i < NB; ++i) Bs[nl][kb + (256 / BN) * i] = rb[i];
    }
  };

  constexpr int WAVES_M = (BM >= 32) ? 2 : 1, WAVES_N = 4 / WAVES_M;
  constexpr int WTM = BM / WAVES_M, WTN = BN / WAVES_N;
  constexpr int FM = WTM / 16, FN = WTN / 16;
  static_assert(FM >= 1 && FN >= 1, "tile too small for 4 waves");
  const int wm0 = (wave / WAVES_N) * WTM, wn0 = (wave % WAVES_N) * WTN;
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fk = lane >> 4;
  load_tiles(0);
  for (int k0 = 0; k0 < K; k0 += BK) {
    __syncthreads();
    store_tiles();
    __syncthreads();
    if (k0 + BK < K) load_tiles(k0 + BK);
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      float a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = As[wm0 + i * 16 + fr][kk + fk];
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = Bs[wn0 + j * 16 + fr][kk + fk];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // epilogue: lane holds D[row = 4*(lane>>4) + r][col = lane & 15]
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm0 + i * 16 + fk * 4 + r;
        const int n = n0 + wn0 + j * 16 + fr;
        if (m >= M || n >= N) continue;
        float v = (g.alpha == 1.0f) ? acc[i][j][r] : g.alpha * acc[i][j][r];
        if (g.bias) v = v + g.bias[n];
        if (g.addend) v = v + g.addend[(long long)m * g.ld_add + n];
        if (g.act == 1) v = v / (1.0f + expf(-v));
        else if (g.act == 2) v = 1.0f / (1.0f + expf(-v));
        float* dst;
        if (g.out_conv) {
          const int hw = g.oh * g.ow;
          const int f = m / hw, pix = m - f * hw;
          dst = g.Y + ((long long)f * N + n) * hw + pix;
        } else if (n < g.nsplitY) {
          dst = g.Y + (long long)m * g.ldy + n;
        } else {
          dst = g.Y2 + (long long)m * g.ldy2 + (n - g.nsplitY);
        }
        if (g.accumulate) *dst = *dst + v;
        else *dst = v;
      }
}

// ---------------------------------------------------------------------------
// Skinny GEMM for per-step activations (M up to a few thousand rows, N
// moderate): a workgroup owns MT rows x NT columns and splits K over its 8
// waves.  Operands go straight from global memory into MFMA fragments -- each
// lane loads 4 consecutive k (one float4) of its row / weight row, and the
// 16-k chunk's k order is permuted identically for A and B, so MFMA step c of
// a chunk sums k = k0 + c + {0,4,8,12}.  No LDS staging of the weights and no
// barriers in the K loop; the weight chunk is prefetched one step ahead.
// With LayerNorm+SiLU on load, the MT input rows are staged once in LDS (one
// global pass) and the row statistics come from there.  The 8 partial
// accumulators are reduced through LDS in fixed order (deterministic), then
// either the element epilogue or a fused row epilogue runs:
//   EPI_SAMPLE  softmax / 1% unimix / argmax(p_hat / Exp(1)) / one-hot STE per
//               latent group (VAE.py:88-98, DynamicsPredictors.py:33-39)
//   EPI_ACTOR   mu, clamp(log_sig), softplus + 1e-3, tanh(mu + eps*sigma)
//               (Agent.py:196-210)
// ---------------------------------------------------------------------------
#ifdef DR_PHASE_TIMING
__device__ long long dr_tbuf_gemm[1024 * DR_TS_SLOTS];
extern "C" int dr_debug_tbuf_gemm(long long* out, int n) {  // read, then clear
  const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(dr_tbuf_gemm), (size_t)n * sizeof(long long));
  static long long zeros[1024 * DR_TS_SLOTS];
  return rc | (int)hipMemcpyToSymbol(HIP_SYMBOL(dr_tbuf_gemm), zeros, sizeof(zeros));
}
#endif
#define SK_LN_MAXF 33280  // floats of staged LayerNorm rows (MT * (K + 4)); 130 KB of the 160 KB LDS
// float4 per lane per staged row of an MT x NT skinny tile: 4 (K <= 1024) on
// the 16-row tiles of up to 32 columns; the 48-column tile holds 6 weight rows
// per wave in registers and stages K <= 256, like the 64-row tiles
constexpr __host__ __device__ int sk_stage_vecs(int mt, int nt) { return (mt == 16 && nt <= 32) ? 4 : 1; }
// hot operands of a skinny problem as wave-uniform scalars (see dr_uni)
struct SkOps {
  const float *A, *A2, *W, *W2;
  int lda, lda2, ksA, ldb, ldb2, ksB, nsB, M, N, K;
};

template <bool B_KN, bool VEC>
__device__ __forceinline__ void skinny_load_b(const SkOps& o, int n, int kq, float (&b)[4]) {
  if (!B_KN && VEC) {
    const bool ok = (n < o.N) && (kq < o.K);
    float4 v = dr_ld4(o.W, ok ? (unsigned)(n * o.ldb + kq) : 0u);
    if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
    b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
    return;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = kq + c;
    const bool ok = (n < o.N) && (k < o.K);
    float v;
    if (!B_KN) {
      v = dr_ld1(o.W, ok ? (unsigned)(n * o.ldb + k) : 0u);
    } else if (k >= o.ksB) {  // KN second segment: rows past ksplitB or columns past nsplitB
      v = dr_ld1(o.W2, ok ? (unsigned)((k - o.ksB) * o.ldb2 + n) : 0u);
    } else if (n >= o.nsB) {
      v = dr_ld1(o.W2, ok ? (unsigned)(k * o.ldb2 + n - o.nsB) : 0u);
    } else {
      v = dr_ld1(o.W, ok ? (unsigned)(k * o.ldb + n) : 0u);
    }
    b[c] = ok ? v : 0.f;
  }
}

// A rows: the 16-k chunk starting at k16 lies in one segment (A below ksA, A2
// above) unless ksA is not a multiple of 16, in which case lanes pick theirs
template <bool VEC>
__device__ __forceinline__ void skinny_load_a(const SkOps& o, int m, int k16, int kq, float (&a)[4]) {
  if (VEC) {
    const bool ok = (m < o.M) && (kq < o.K);
    float4 v;
    if (k16 + 16 <= o.ksA) {
      v = dr_ld4(o.A, ok ? (unsigned)(m * o.lda + kq) : 0u);
    } else if (k16 >= o.ksA) {
      v = dr_ld4(o.A2, ok ? (unsigned)(m * o.lda2 + kq - o.ksA) : 0u);
    } else {
      const float* src = (kq < o.ksA) ? o.A + (long long)m * o.lda + kq : o.A2 + (long long)m * o.lda2 + (kq - o.ksA);
      v = dr_ld4(ok ? src : o.A, 0u);
    }
    if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
    a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = kq + c;
      const bool ok = (m < o.M) && (k < o.K);
      float v;
      if (k < o.ksA) v = dr_ld1(o.A, ok ? (unsigned)(m * o.lda + k) : 0u);
      else v = dr_ld1(o.A2, ok ? (unsigned)(m * o.lda2 + k - o.ksA) : 0u);
      a[c] = ok ? v : 0.f;
    }
  }
}

__device__ __forceinline__ float epi_act(const GemmArgs& g, float v) {
  if (g.act == 1) return v / (1.0f + expf(-v));
  if (g.act == 2) return 1.0f / (1.0f + expf(-v));
  return v;
}

// GruBwdEpi: the gru_cell backward of one (row, unit) from the final dL/dh',
// on operands already in registers (r, u, n, hn = W_hn h + b_hn, hv = h,
// o_old = dL/dh before this step's addend)
__device__ __forceinline__ void gru_bwd_apply(const GruBwdEpi& e, int m, int j, float g, float r, float u, float n,
                                              float hn, float hv, float o_old) {
  const int Hd = e.Hd;
  // h' = (h - n)*u + n
  const float g_hmn = g * u;
  const float g_u = g * (hv - n);
  const float g_n = g + (-g_hmn);
  // n = tanh(in + hn*r)
  const float g_pn = g_n * (1.0f - n * n);
  const float g_r = g_pn * hn;
  const float g_hn = g_pn * r;
  const float g_pr = g_r * (1.0f - r) * r;
  const float g_pu = g_u * (1.0f - u) * u;
  DR_GLOBAL float* gib = dr_g(e.gi) + (long long)m * 3 * Hd;
  DR_GLOBAL float* ghb = dr_g(e.gh) + (long long)m * 3 * Hd;
  gib[j] = g_pr;
  gib[Hd + j] = g_pu;
  gib[2 * Hd + j] = g_pn;
  ghb[j] = g_pr;
  ghb[Hd + j] = g_pu;
  ghb[2 * Hd + j] = g_hn;
  if (e.gi16) {
    DR_GLOBAL unsigned short* gi16 = dr_g(e.gi16) + (long long)m * 3 * Hd;
    DR_GLOBAL unsigned short* gh16 = dr_g(e.gh16) + (long long)m * 3 * Hd;
    gi16[j] = __builtin_bit_cast(unsigned short, (__bf16)g_pr);
    gi16[Hd + j] = __builtin_bit_cast(unsigned short, (__bf16)g_pu);
    gi16[2 * Hd + j] = __builtin_bit_cast(unsigned short, (__bf16)g_pn);
    gh16[j] = __builtin_bit_cast(unsigned short, (__bf16)g_pr);
    gh16[Hd + j] = __builtin_bit_cast(unsigned short, (__bf16)g_pu);
    gh16[2 * Hd + j] = __builtin_bit_cast(unsigned short, (__bf16)g_hn);
  }
  dr_g(e.ho)[(long long)m * e.ldo + j] = o_old + g_hmn;
}

// ... loading them itself (the epilogues that do not prefetch)
__device__ __noinline__ void gru_bwd_elem(const GruBwdEpi& e, int m, int j, float g) {
  const long long i = (long long)m * e.Hd + j;
  const float r = dr_g(e.r)[i], u = dr_g(e.u)[i], n = dr_g(e.n)[i], hn = dr_g(e.ghn)[i];
  const float hv = e.h ? dr_g(e.h)[(long long)m * e.ldh + j] : 0.0f;
  gru_bwd_apply(e, m, j, g, r, u, n, hn, hv, dr_g(e.ho)[(long long)m * e.ldo + j]);
}

__device__ __forceinline__ void epilogue_store_b(const GemmArgs& g, int m, int n, float acc, float bias) {
  float v = (g.alpha == 1.0f) ? acc : g.alpha * acc;
  if (g.bias) v = v + bias;
  if (g.addend) v = v + dr_g(g.addend)[(long long)m * g.ld_add + n];
  v = epi_act(g, v);
  DR_GLOBAL float* dst;
  if (n < g.nsplitY) dst = dr_g(g.Y) + (long long)m * g.ldy + n;
  else dst = dr_g(g.Y2) + (long long)m * g.ldy2 + (n - g.nsplitY);
  const float fin = g.accumulate ? *dst + v : v;
  *dst = fin;
  if (g.gb.Hd > 0 && n < g.gb.Hd) gru_bwd_elem(g.gb, m, n, fin);
}

// epilogue_store_b with its memory operands read ahead of the K loop
// (k_gemm_skinny, AM_LNBWD): the same arithmetic on the same values.  Nothing
// else in the launch writes them -- element (m, n) of Y and of dL/dh belongs to
// this thread alone; should dL/dh alias the output element, the stored value
// is taken, as a read after the store would see it
struct SkEpiPf {
  float dst, r, u, n, hn, h, o;
};
__device__ __forceinline__ DR_GLOBAL float* sk_epi_dst(const GemmArgs& g, int m, int n) {
  if (n < g.nsplitY) return dr_g(g.Y) + (long long)m * g.ldy + n;
  return dr_g(g.Y2) + (long long)m * g.ldy2 + (n - g.nsplitY);
}
__device__ __forceinline__ SkEpiPf sk_epi_prefetch(const GemmArgs& g, int m, int n, bool ok) {
  SkEpiPf p = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (!ok) return p;
  if (g.accumulate) p.dst = *sk_epi_dst(g, m, n);
  const GruBwdEpi& e = g.gb;
  if (e.Hd > 0 && n < e.Hd) {
    const long long i = (long long)m * e.Hd + n;
    p.r = dr_g(e.r)[i];
    p.u = dr_g(e.u)[i];
    p.n = dr_g(e.n)[i];
    p.hn = dr_g(e.ghn)[i];
    if (e.h) p.h = dr_g(e.h)[(long long)m * e.ldh + n];
    p.o = dr_g(e.ho)[(long long)m * e.ldo + n];
  }
  return p;
}
__device__ __forceinline__ void epilogue_store_pf(const GemmArgs& g, int m, int n, float acc, float bias,
                                                  const SkEpiPf& p) {
  float v = (g.alpha == 1.0f) ? acc : g.alpha * acc;
  if (g.bias) v = v + bias;
  if (g.addend) v = v + dr_g(g.addend)[(long long)m * g.ld_add + n];
  v = epi_act(g, v);
  DR_GLOBAL float* dst = sk_epi_dst(g, m, n);
  const float fin = g.accumulate ? p.dst + v : v;
  *dst = fin;
  if (g.gb.Hd > 0 && n < g.gb.Hd) {
    const DR_GLOBAL float* o = dr_g(g.gb.ho) + (long long)m * g.gb.ldo + n;
    gru_bwd_apply(g.gb, m, n, fin, p.r, p.u, p.n, p.hn, p.h, o == dst ? fin : p.o);
  }
}

#define DR_SKW 8  // waves per skinny-GEMM workgroup (K split over them; 4 measured slower, r05)
// k_gemm_skinny's tile predicates, one definition for the kernel and the planner (which sizes the dynamic LDS).
#define SK_FN constexpr __host__ __device__
SK_FN int sk_kpad(int K) { return K + ((8 - (K & 15)) & 15); }  // LDS row stride, 8 mod 16 dwords
// staged: the tile's A and weight rows in LDS, prologue on the way (the K test first: the product stays an int)
SK_FN bool sk_staged(int amode, int mt, int nt, int K, bool vec, bool b_kn) {
  return (amode == AM_LNSILU || amode == AM_LNBWD || amode == AM_STEBWD) && vec && !b_kn &&
         ((K >> 2) <= 64 * sk_stage_vecs(mt, nt)) && ((mt + nt) * sk_kpad(K) <= SK_LN_MAXF);
}
// direct path: float4 per lane per LayerNorm row held in LDS, and whether the rows are
SK_FN int sk_ln_vecs(int mt) { return (mt == 16) ? 8 : 2; }
SK_FN bool sk_ln_lds(int amode, int mt, int K, bool vec) {
  return (amode == AM_LNSILU) && vec && ((K >> 2) <= 64 * sk_ln_vecs(mt)) && (mt * sk_kpad(K) <= SK_LN_MAXF);
}
// floats of the wave-partial reduction slab; of a tile's dynamic LDS: max(slab, staged tile or LN rows)
SK_FN int sk_red_floats(int mt, int nt) { return DR_SKW * (mt / 16) * (nt / 16) * 4 * 64; }
SK_FN int sk_lds_floats(int amode, int mt, int nt, int K, bool vec, bool b_kn) {
  const int rows = sk_staged(amode, mt, nt, K, vec, b_kn) ? (mt + nt) * sk_kpad(K)
                                                          : sk_ln_lds(amode, mt, K, vec) ? mt * sk_kpad(K) : 0;
  return rows > sk_red_floats(mt, nt) ? rows : sk_red_floats(mt, nt);
}
template <int MT, int NT, int AMODE, bool B_KN, bool VEC, int EPI>
__global__ __launch_bounds__(64 * DR_SKW) void k_gemm_skinny(GemmBatch gb, int npack) {
  constexpr int NWAVE = DR_SKW, NTH = 64 * DR_SKW, FT = MT / 16, FN = NT / 16;
  __shared__ GemmArgs s_args;
  int pz;
  const int plt = dr_pack_tile<MT, NT>(gb, npack, pz);
  if (plt == -1) return;
  dr_stage_args(gb.p[pz], s_args, threadIdx.x);
  const GemmArgs& g = s_args;
  SkOps o;
  o.M = dr_uni(g.M); o.N = dr_uni(g.N); o.K = dr_uni(g.K);
  o.A = dr_uni(g.A); o.A2 = dr_uni(g.A2); o.W = dr_uni(g.W);
  o.lda = dr_uni((int)g.lda); o.lda2 = dr_uni((int)g.lda2); o.ksA = dr_uni(g.ksplitA); o.ldb = dr_uni((int)g.ldb);
  o.W2 = dr_uni(g.W2); o.ldb2 = dr_uni((int)g.ldb2); o.ksB = dr_uni(g.ksplitB); o.nsB = dr_uni(g.nsplitB);
  const int M = o.M, N = o.N, K = o.K;
  const int tiles_n = (N + NT - 1) / NT;
  const int tiles_m = (M + MT - 1) / MT;
  // logical tiles column-major: the row tiles reading one weight slice are
  // adjacent and share an XCD's L2
  const int lt = plt >= 0 ? plt : dr_xcd_tile(blockIdx.x, tiles_m * tiles_n);
  if (lt < 0) return;
  const int tn = lt / tiles_m, tm = lt - tn * tiles_m;
  const int m0 = tm * MT, n0 = tn * NT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  DR_TS(dr_tbuf_gemm, 0);

  // dynamic LDS, sized by the host for this launch (sk_lds_floats):
  // [ max(reduction slab, staged LN rows) | LN gamma (K) | LN beta (K) ]
  constexpr int RED = sk_red_floats(MT, NT);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  __shared__ float s_mean[MT], s_rstd[MT];
  __shared__ float s_out[MT][NT + 1];
  // bias of the output columns this thread finalises, issued now and waited
  // for only in the epilogue
  constexpr int NEPI = (FT * FN * 256 + NTH - 1) / NTH;
  float ebias[NEPI];
  {
    const float* bias = dr_uni(g.bias);
#pragma unroll
    for (int i = 0; i < NEPI; ++i) {
      const int x = tid + NTH * i;
      const int n = n0 + ((x >> 8) % FN) * 16 + (x & 15);
      const bool ok = bias && x < FT * FN * 256 && n < N;
      const float v = dr_ld1(ok ? bias : o.W, ok ? (unsigned)n : 0u);
      ebias[i] = ok ? v : 0.f;
    }
  }
  // LayerNorm-backward products (the BPTT's hidden-state gradient): what the
  // epilogue reads per output element -- the accumulate read of dst and the
  // fused GRU backward's saves (r, u, n, hn, h) and dL/dh -- issued now as
  // well, so the epilogue pays no memory round trip after the K loop
  constexpr bool PFE = (AMODE == AM_LNBWD) && (EPI == EPI_NONE);
  SkEpiPf pf[PFE ? NEPI : 1];
  if (PFE) {
#pragma unroll
    for (int i = 0; i < NEPI; ++i) {
      const int x = tid + NTH * i;
      const int l = x & 63, e = (x >> 6) & 3, tj = x >> 8;
      const int t = tj / FN, j = tj - t * FN;
      const int m = m0 + t * 16 + 4 * (l >> 4) + e, n = n0 + j * 16 + (l & 15);
      pf[i] = sk_epi_prefetch(g, m, n, x < FT * FN * 256 && m < M && n < N);
    }
  }

  // Philox state of the sampler / actor epilogues, fetched now (not after the K loop)
  unsigned long long rng_seed = 0, rng_off = 0;
  if ((EPI == EPI_SAMPLE || EPI == EPI_ACTOR) && g.epi != EPI_NONE && !g.noise.q && !g.noise.eps && g.noise.rng) {
    rng_seed = g.noise.rng[0];
    rng_off = g.noise.rng[1];
  }
  const int kw = ((K + NWAVE * 16 - 1) / (NWAVE * 16)) * 16;
  const int kb = wave * kw;
  const int ke = min(K, kb + kw);

  // ---- operand path ---------------------------------------------------
  // Staged (LayerNorm-SiLU A, NT, 16-byte aligned, K <= 1024): every row of the A tile and of
  // the weight tile is read by one wave with coalesced 1 KB row pieces
  // (lane -> float4 column), all loads issued before the first wait; the
  // LayerNorm-SiLU prologue (rows in registers: DPP statistics, one
  // normalise + activate per element) runs on the way; both tiles land in LDS
  // with a padded stride (K + 4 floats: the 16 rows an MFMA fragment reads
  // fall in distinct banks); the K loop then reads fragments from LDS.
  // Direct (otherwise): each lane loads its MFMA fragments from global memory.
  const int KP = sk_kpad(K);  // row stride = 8 mod 16 dwords: ds_read_b128 fragments conflict-free
  const int K4 = K >> 2;
  constexpr int RPW = MT / NWAVE;                    // A rows per wave
  constexpr int BPW = (NT + NWAVE - 1) / NWAVE;      // weight rows per wave
  constexpr int SV = sk_stage_vecs(MT, NT);          // float4 per lane per staged row (K <= 256 * SV)
  float* a_out = dr_uni(g.a_out);
  const int ld_aout = dr_uni((int)g.ld_aout);
  const bool store_a = (a_out != nullptr) && (tn == 0);
  // (measured: staging pays only where the LayerNorm needs the barrier anyway;
  // a plain GEMM is faster with direct fragment loads, profiles/r01_v5_kbench.txt)
  const bool staged = sk_staged(AMODE, MT, NT, K, VEC, B_KN);
  // with few accumulator tiles, alternate 16-k chunks between two accumulator
  // sets so consecutive MFMAs are independent (40-cycle result latency)
  constexpr bool DUAL = FT * FN < 4;
  f32x4 acc[FT][FN], acc2[FT][FN];
#pragma unroll
  for (int t = 0; t < FT; ++t)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[t][j] = acc2[t][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  DR_TS(dr_tbuf_gemm, 1);
  if (staged) {
    float* sA = smem;
    float* sB = smem + MT * KP;
    constexpr int PRW = (AMODE == AM_LNBWD || AMODE == AM_STEBWD) ? RPW : 1;
    float4 xa[RPW][SV], xb[BPW][SV], gv[SV], bv[SV], xp[PRW][SV];
    const float* lg = dr_uni(g.ln_g);
    const float* lb = dr_uni(g.ln_b);
    const float* pre = dr_uni(g.pre);
    const int ld_pre = dr_uni((int)g.ld_pre);
#pragma unroll
    for (int i = 0; i < SV; ++i) {
      if (64 * i >= K4) break;  // wave-uniform: no dummy loads past the row
      const int k4 = lane + 64 * i, k = 4 * k4;
      const bool okk = k4 < K4;
#pragma unroll
      for (int rr = 0; rr < RPW; ++rr) {
        const int m = m0 + wave + NWAVE * rr;
        const bool ok = okk && m < M;
        const bool seg1 = k < o.ksA;
        const float* base = seg1 ? o.A : o.A2;
        const unsigned e = ok ? (unsigned)(seg1 ? m * o.lda + k : m * o.lda2 + k - o.ksA) : 0u;
        xa[rr][i] = dr_ld4(ok ? base : o.W, e);
        if (!ok) xa[rr][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (AMODE == AM_LNBWD || AMODE == AM_STEBWD) {
          xp[rr][i] = dr_ld4(pre, ok ? (unsigned)(m * ld_pre + k) : 0u);
          if (!ok) xp[rr][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int jj = 0; jj < BPW; ++jj) {
        const int nl = wave + NWAVE * jj, n = n0 + nl;
        const bool ok = okk && nl < NT && n < N;
        xb[jj][i] = dr_ld4(o.W, ok ? (unsigned)(n * o.ldb + k) : 0u);
        if (!ok) xb[jj][i] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      if (AMODE == AM_LNSILU || AMODE == AM_LNBWD) {
        gv[i] = dr_ld4(lg, okk ? (unsigned)k : 0u);
        bv[i] = dr_ld4(lb, okk ? (unsigned)k : 0u);
      }
    }
    DR_TS(dr_tbuf_gemm, 2);
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
      const int ml = wave + NWAVE * rr, m = m0 + ml;
      if (AMODE == AM_LNSILU) {
        float sm = 0.f;
#pragma unroll
        for (int i = 0; i < SV; ++i) {
          if (64 * i >= K4) break;
          sm += (xa[rr][i].x + xa[rr][i].y) + (xa[rr][i].z + xa[rr][i].w);
        }
        const float mean = wave_sum(sm) / (float)K;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < SV; ++i) {
          if (64 * i >= K4) break;
          if (lane + 64 * i < K4) {
            const float dx = xa[rr][i].x - mean, dy = xa[rr][i].y - mean;
            const float dz = xa[rr][i].z - mean, dw = xa[rr][i].w - mean;
            sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
          }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)K + 1e-5f);
#pragma unroll
        for (int i = 0; i < SV; ++i) {
          if (64 * i >= K4) break;
          float4& x = xa[rr][i];
          x.x = dr_silu_fast((x.x - mean) * rstd * gv[i].x + bv[i].x);
          x.y = dr_silu_fast((x.y - mean) * rstd * gv[i].y + bv[i].y);
          x.z = dr_silu_fast((x.z - mean) * rstd * gv[i].z + bv[i].z);
          x.w = dr_silu_fast((x.w - mean) * rstd * gv[i].w + bv[i].w);
          if (m >= M) x = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      if (AMODE == AM_STEBWD) {
        // straight-through softmax backward: a group of C classes is C/4
        // consecutive lanes of one float4 chunk (K % C == 0, host-checked)
        const int gl = dr_uni(g.C) >> 2;
#pragma unroll
        for (int i = 0; i < SV; ++i) {
          if (64 * i >= K4) break;
          float4& x = xa[rr][i];
          const float4& sv = xp[rr][i];
          const float gx = 0.99f * x.x, gy = 0.99f * x.y, gz = 0.99f * x.z, gw = 0.99f * x.w;
          float dot = (gx * sv.x + gy * sv.y) + (gz * sv.z + gw * sv.w);
          for (int o = 1; o < gl; o <<= 1) dot += __shfl_xor(dot, o, 64);
          x.x = sv.x * (gx - dot);
          x.y = sv.y * (gy - dot);
          x.z = sv.z * (gz - dot);
          x.w = sv.w * (gw - dot);
          if (m >= M) x = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      if (AMODE == AM_LNBWD) {
        // SiLU(LayerNorm(pre)) backward (ops.hip k_ln_silu_bwd, restated on
        // registers): x_hat, y, s = sigmoid(y), dy = gx * s(1 + y(1 - s)),
        // dx_hat = dy*gamma, g_pre = rstd (dx_hat - mean(dx_hat) - x_hat mean(dx_hat x_hat))
        const int PR = (AMODE == AM_LNBWD) ? rr : 0;
        float sm = 0.f;
#pragma unroll
        for (int i = 0; i < SV; ++i) {
          if (64 * i >= K4) break;
          sm += (xp[PR][i].x + xp[PR][i].y) + (xp[PR][i].z + xp[PR][i].w);
        }
        const float mean = wave_sum(sm) / (float)K;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < SV; ++i) {
          if (64 * i >= K4) break;
          if (lane + 64 * i < K4) {
            const float dx = xp[PR][i].x - mean, dy = xp[PR][i].y - mean;
            const float dz = xp[PR][i].z - mean, dw = xp[PR][i].w - mean;
            sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
          }
        }
        const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)K + 1e-5f);
        float c1 = 0.f, c2 = 0.f;
        float* sgy = dr_uni(g.sv_gy);
        float* sxh = dr_uni(g.sv_xh);
        const int ld_sv = dr_uni((int)g.ld_sv);
        const bool save = sgy && tn == 0 && m < M;
#pragma unroll
        for (int i = 0; i < SV; ++i) {
          if (64 * i >= K4) break;
          const int k4 = lane + 64 * i;
          const bool okk = k4 < K4;
          float4 xh, gy;
          float* xhp = &xh.x;
          float* gyp = &gy.x;
          const float* pp = &xp[PR][i].x;
          const float* gxp = &xa[rr][i].x;
          const float* gg = &gv[i].x;
          const float* bb4 = &bv[i].x;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float x_h = (pp[c] - mean) * rstd;
            const float y = x_h * gg[c] + bb4[c];
            const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(y * -1.4426950408889634f));
            const float gyv = gxp[c] * (sg * (1.0f + y * (1.0f - sg)));
            const float gxh = gyv * gg[c];
            xhp[c] = x_h;
            gyp[c] = gxh;  // keep dx_hat for the last pass
            if (okk) {
              c1 += gxh;
              c2 += gxh * x_h;
            }
            if (save && okk) {
              dr_g(sgy)[(unsigned)(m * ld_sv + 4 * k4 + c)] = gyv;
              dr_g(sxh)[(unsigned)(m * ld_sv + 4 * k4 + c)] = x_h;
            }
          }
          xa[rr][i] = gy;   // dx_hat
          xp[PR][i] = xh;   // x_hat
        }
        c1 = wave_sum(c1) / (float)K;
        c2 = wave_sum(c2) / (float)K;
#pragma unroll
        for (int i = 0; i < SV; ++i) {
          if (64 * i >= K4) break;
          float4& x = xa[rr][i];
          const float4& h = xp[PR][i];
          x.x = rstd * (x.x - c1 - h.x * c2);
          x.y = rstd * (x.y - c1 - h.y * c2);
          x.z = rstd * (x.z - c1 - h.z * c2);
          x.w = rstd * (x.w - c1 - h.w * c2);
          if (m >= M) x = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int i = 0; i < SV; ++i) {
        if (64 * i >= K4) break;
        const int k4 = lane + 64 * i;
        if (k4 < K4) {
          *reinterpret_cast<float4*>(&sA[ml * KP + 4 * k4]) = xa[rr][i];
          if (store_a && m < M) dr_st4(a_out, (unsigned)(m * ld_aout + 4 * k4), xa[rr][i]);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < BPW; ++jj) {
      const int nl = wave + NWAVE * jj;
      if (nl >= NT) break;
#pragma unroll
      for (int i = 0; i < SV; ++i) {
        if (64 * i >= K4) break;
        const int k4 = lane + 64 * i;
        if (k4 < K4) *reinterpret_cast<float4*>(&sB[nl * KP + 4 * k4]) = xb[jj][i];
      }
    }
    DR_TS(dr_tbuf_gemm, 6);
    __syncthreads();
    DR_TS(dr_tbuf_gemm, 3);
    for (int k16 = kb; k16 < ke; k16 += 16) {
      const int kq = k16 + 4 * q;
      const bool okq = kq < K;
      f32x4 (&ac)[FT][FN] = (DUAL && (((k16 - kb) >> 4) & 1)) ? acc2 : acc;
      float4 fa[FT], fb[FN];
#pragma unroll
      for (int t = 0; t < FT; ++t) {
        fa[t] = *reinterpret_cast<const float4*>(&sA[(t * 16 + r) * KP + (okq ? kq : 0)]);
        if (!okq) fa[t] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        fb[j] = *reinterpret_cast<const float4*>(&sB[(j * 16 + r) * KP + (okq ? kq : 0)]);
        if (!okq) fb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int t = 0; t < FT; ++t)
#pragma unroll
        for (int j = 0; j < FN; ++j) ac[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t].x, fb[j].x, ac[t][j], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < FT; ++t)
#pragma unroll
        for (int j = 0; j < FN; ++j) ac[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t].y, fb[j].y, ac[t][j], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < FT; ++t)
#pragma unroll
        for (int j = 0; j < FN; ++j) ac[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t].z, fb[j].z, ac[t][j], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < FT; ++t)
#pragma unroll
        for (int j = 0; j < FN; ++j) ac[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t].w, fb[j].w, ac[t][j], 0, 0, 0);
    }
  } else if (AMODE != AM_LNBWD) {  // (the LayerNorm-backward prologue exists only staged: plan_skinny's guard)
    // K loop in batches of PRE 16-k chunks: every load of a batch is issued
    // before its first MFMA, so a wave pays one memory round trip per batch
    // (one in total for K <= PRE*16*8 = 1024).  The first batch of weights (and
    // of plain A rows) is issued before the LayerNorm staging.
    constexpr int PRE = (FT >= 4) ? 4 : 8;
    float bb[PRE][FN][4];
    float aa[PRE][FT][4];
    auto load_batch = [&](int kc) {
  #pragma unroll
      for (int p = 0; p < PRE; ++p) {
        const int k16 = kc + 16 * p;
        const int kq = k16 + 4 * q;
        const bool live = k16 < ke;
  #pragma unroll
        for (int j = 0; j < FN; ++j) {
          if (live) {
            skinny_load_b<B_KN, VEC>(o, n0 + j * 16 + r, kq, bb[p][j]);
          } else {
  #pragma unroll
            for (int c = 0; c < 4; ++c) bb[p][j][c] = 0.f;
          }
        }
        if (AMODE != AM_LNSILU) {
  #pragma unroll
          for (int t = 0; t < FT; ++t) {
            if (live) {
              skinny_load_a<VEC>(o, m0 + t * 16 + r, k16, kq, aa[p][t]);
            } else {
  #pragma unroll
              for (int c = 0; c < 4; ++c) aa[p][t][c] = 0.f;
            }
          }
        }
      }
    };
    if (kb < ke) load_batch(kb);

    // direct path: LayerNorm (when K > 1024) from global memory; large-K rows
    // staged (K <= 256 * LNV) like the staged path's A tile
    constexpr int LNV = sk_ln_vecs(MT);
    const bool ln_lds = sk_ln_lds(AMODE, MT, K, VEC);
    if (AMODE == AM_LNSILU) {
      if (ln_lds) {
        const float* lg = dr_uni(g.ln_g);
        const float* lb = dr_uni(g.ln_b);
        float4 xv[RPW][LNV], gv[LNV], bv[LNV];
  #pragma unroll
        for (int i = 0; i < LNV; ++i) {
          if (64 * i >= K4) break;  // wave-uniform: no dummy loads past the row
          const int k4 = lane + 64 * i;
          const bool okk = k4 < K4;
          gv[i] = dr_ld4(lg, okk ? (unsigned)(4 * k4) : 0u);
          bv[i] = dr_ld4(lb, okk ? (unsigned)(4 * k4) : 0u);
  #pragma unroll
          for (int rr = 0; rr < RPW; ++rr) {
            const int m = m0 + wave + NWAVE * rr;
            const bool ok = okk && m < M;
            xv[rr][i] = dr_ld4(o.A, ok ? (unsigned)(m * o.lda + 4 * k4) : 0u);
            if (!ok) xv[rr][i] = make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
  #pragma unroll
        for (int rr = 0; rr < RPW; ++rr) {
          const int ml = wave + NWAVE * rr, m = m0 + ml;
          float sm = 0.f;
  #pragma unroll
          for (int i = 0; i < LNV; ++i) {
            if (64 * i >= K4) break;
            sm += (xv[rr][i].x + xv[rr][i].y) + (xv[rr][i].z + xv[rr][i].w);
          }
          const float mean = wave_sum(sm) / (float)K;
          float sq = 0.f;
  #pragma unroll
          for (int i = 0; i < LNV; ++i) {
            if (64 * i >= K4) break;
            if (lane + 64 * i < K4) {
              const float dx = xv[rr][i].x - mean, dy = xv[rr][i].y - mean;
              const float dz = xv[rr][i].z - mean, dw = xv[rr][i].w - mean;
              sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
          }
          const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)K + 1e-5f);
  #pragma unroll
          for (int i = 0; i < LNV; ++i) {
            if (64 * i >= K4) break;
            const int k4 = lane + 64 * i;
            if (k4 < K4) {
              float4 y;
              y.x = dr_silu_fast((xv[rr][i].x - mean) * rstd * gv[i].x + bv[i].x);
              y.y = dr_silu_fast((xv[rr][i].y - mean) * rstd * gv[i].y + bv[i].y);
              y.z = dr_silu_fast((xv[rr][i].z - mean) * rstd * gv[i].z + bv[i].z);
              y.w = dr_silu_fast((xv[rr][i].w - mean) * rstd * gv[i].w + bv[i].w);
              if (m >= M) y = make_float4(0.f, 0.f, 0.f, 0.f);
              *reinterpret_cast<float4*>(&smem[ml * KP + 4 * k4]) = y;
              if (store_a && m < M) dr_st4(a_out, (unsigned)(m * ld_aout + 4 * k4), y);
            }
          }
        }
      } else {
        for (int rr = wave; rr < MT; rr += NWAVE) {
          const int m = m0 + rr;
          float mean = 0.f, rstd = 0.f;
          if (m < M) {
            const DR_GLOBAL float* row = dr_g(o.A) + (long long)m * o.lda;
            float s = 0.f, v = 0.f;
            for (int k = lane; k < K; k += 64) s += row[k];
            mean = wave_sum(s) / (float)K;
            for (int k = lane; k < K; k += 64) {
              const float d = row[k] - mean;
              v += d * d;
            }
            rstd = 1.0f / sqrtf(wave_sum(v) / (float)K + 1e-5f);
          }
          if (lane == 0) {
            s_mean[rr] = mean;
            s_rstd[rr] = rstd;
          }
        }
      }
      __syncthreads();
    }

    const float* lg = dr_uni(g.ln_g);
    const float* lb = dr_uni(g.ln_b);
    for (int kc = kb; kc < ke; kc += PRE * 16) {
      if (kc != kb) load_batch(kc);
      if (AMODE == AM_LNSILU) {
  #pragma unroll
        for (int p = 0; p < PRE; ++p) {
          const int k16 = kc + 16 * p;
          const int kq = k16 + 4 * q;
          const bool live = k16 < ke;
  #pragma unroll
          for (int t = 0; t < FT; ++t) {
            const int ml = t * 16 + r, m = m0 + ml;
            if (!live) {
  #pragma unroll
              for (int c = 0; c < 4; ++c) aa[p][t][c] = 0.f;
            } else if (ln_lds) {
              if (m < M && kq < K) {
                const float4 v = *reinterpret_cast<const float4*>(&smem[ml * KP + kq]);
                aa[p][t][0] = v.x; aa[p][t][1] = v.y; aa[p][t][2] = v.z; aa[p][t][3] = v.w;
              } else {
                aa[p][t][0] = aa[p][t][1] = aa[p][t][2] = aa[p][t][3] = 0.f;
              }
            } else {
              skinny_load_a<VEC>(o, m, k16, kq, aa[p][t]);
            }
          }
        }
      }
  #pragma unroll
      for (int p = 0; p < PRE; ++p) {
        if (kc + 16 * p >= ke) break;
        const int kq = kc + 16 * p + 4 * q;
  #pragma unroll
        for (int t = 0; t < FT; ++t) {
          const int ml = t * 16 + r, m = m0 + ml;
          if (AMODE == AM_LNSILU && !ln_lds) {  // global fallback: transform on the fly
            const float mean = s_mean[ml], rstd = s_rstd[ml];
  #pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int k = kq + c;
              if (m < M && k < K) {
                float x = (aa[p][t][c] - mean) * rstd;
                x = x * dr_ld1(lg, (unsigned)k) + dr_ld1(lb, (unsigned)k);
                aa[p][t][c] = dr_silu_fast(x);
              }
            }
          }
          if (store_a && m < M && !(AMODE == AM_LNSILU && ln_lds)) {
  #pragma unroll
            for (int c = 0; c < 4; ++c)
              if (kq + c < K) dr_g(a_out)[(unsigned)(m * ld_aout + kq + c)] = aa[p][t][c];
          }
        }
        f32x4 (&ac)[FT][FN] = (DUAL && (p & 1)) ? acc2 : acc;
  #pragma unroll
        for (int c = 0; c < 4; ++c)
  #pragma unroll
          for (int t = 0; t < FT; ++t)
  #pragma unroll
            for (int j = 0; j < FN; ++j)
              ac[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[p][t][c], bb[p][j][c], ac[t][j], 0, 0, 0);
      }
    }
  }
  if (DUAL) {
#pragma unroll
    for (int t = 0; t < FT; ++t)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[t][j] += acc2[t][j];
  }
  DR_TS(dr_tbuf_gemm, 4);
  if (staged || AMODE == AM_LNSILU) __syncthreads();  // smem held the staged rows
#pragma unroll
  for (int t = 0; t < FT; ++t)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) smem[(((wave * FT + t) * FN + j) * 4 + e) * 64 + lane] = acc[t][j][e];
  __syncthreads();
  DR_TS(dr_tbuf_gemm, 5);
  // element (t, j, e, l): D[row 4*(l>>4)+e][col l&15] of tile (t, j)
#pragma unroll
  for (int i = 0; i < NEPI; ++i) {
    const int x = tid + NTH * i;
    if (x >= FT * FN * 256) break;
    const int l = x & 63, e = (x >> 6) & 3, tj = x >> 8;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NWAVE; ++w) v += smem[((w * FT * FN + tj) * 4 + e) * 64 + l];
    const int t = tj / FN, j = tj - t * FN;
    const int ml = t * 16 + 4 * (l >> 4) + e, nl = j * 16 + (l & 15);
    const int m = m0 + ml, n = n0 + nl;
    if (PFE) {
      if (m < M && n < N) epilogue_store_pf(g, m, n, v, ebias[i], pf[i]);
    } else if (EPI == EPI_NONE || g.epi == EPI_NONE) {
      if (m < M && n < N) epilogue_store_b(g, m, n, v, ebias[i]);
    } else {
      if (m < M && n < N) {
        float y = v + ebias[i];
        if (g.Y) dr_g(g.Y)[(long long)m * g.ldy + n] = y;
        s_out[ml][nl] = y;
      }
    }
  }
  if (EPI == EPI_SAMPLE) {
    // groups of C classes inside this NT-column tile; W lanes per group
    __syncthreads();
    const int C = g.C;
    int W = 1;
    while (W < C) W <<= 1;
    const int gpr = NT / C;                // groups per row in this tile
    const int npairs = MT * gpr;           // (row, group) pairs
    const int per_wave = 64 / W;
    for (int pbase = wave * per_wave; pbase < npairs; pbase += NWAVE * per_wave) {
      const int pidx = pbase + lane / W, c = lane % W;
      const bool valid = pidx < npairs;
      const int ml = valid ? pidx / gpr : 0, gl = valid ? pidx - ml * gpr : 0;
      const int m = m0 + ml, grp = (n0 / C) + gl;
      const bool act = valid && c < C && m < M && (n0 + gl * C + c) < N;
      const float x = act ? s_out[ml][gl * C + c] : -INFINITY;
      const float mx = group_max(x, W);
      const float ex = act ? expf(x - mx) : 0.0f;
      const float se = group_sum(ex, W);
      const float p = ex / se;
      const float pu = act ? (0.99f * p + g.unimix) : 0.0f;
      const float sp = group_sum(pu, W);
      const float ph = pu / sp;
      float qv = 1.0f;
      const int Rg = g.R;
      if (act) {
        if (g.noise.q) qv = dr_g(g.noise.q)[((long long)g.step * M * Rg + (long long)m * Rg + grp) * C + c];
        else qv = dr_exp1_k(rng_seed, rng_off, (uint32_t)(g.noise.stream + g.step), (uint32_t)(g.noise.row0 + m),
                            (uint32_t)(grp * C + c));
      }
      float best = act ? ph / qv : -INFINITY;
      int bi = act ? c : 0x7fffffff;
      group_argmax(best, bi, W);
      if (act) {
        dr_g(g.z_out)[(long long)m * g.ldz + grp * C + c] = (c == bi) ? ((1.0f + pu) - pu) : 0.0f;
        if (g.soft_out) dr_g(g.soft_out)[(long long)m * g.ld_soft + grp * C + c] = p;
        if (g.idx_out && c == 0) dr_g(g.idx_out)[m * Rg + grp] = bi;
        if (g.zval_out && c == bi) dr_g(g.zval_out)[m * Rg + grp] = (1.0f + pu) - pu;
      }
    }
    DR_TS(dr_tbuf_gemm, 7);
  } else if (EPI == EPI_ACTOR && g.epi == EPI_ACTOR) {
    __syncthreads();
    const int A = g.na;
    for (int x = tid; x < MT * A; x += NTH) {
      const int ml = x / A, i = x - ml * A, m = m0 + ml;
      if (m >= M) continue;
      const float muv = s_out[ml][i];
      const float lr = s_out[ml][A + i];
      const float ls = fminf(fmaxf(lr, -5.0f), 2.0f);
      const float sg = dr_softplus(ls) + 1e-3f;
      float av;
      if (g.det) {
        av = tanhf(muv);
      } else {
        float e;
        if (g.noise.eps) e = dr_g(g.noise.eps)[((long long)g.step * M + m) * A + i];
        else e = dr_normal_k(rng_seed, rng_off, (uint32_t)(g.noise.stream + g.step), (uint32_t)(g.noise.row0 + m),
                             (uint32_t)i);
        if (g.eps_save) dr_g(g.eps_save)[(long long)m * A + i] = e;
        av = tanhf(muv + e * sg);
      }
      if (g.act_out) dr_g(g.act_out)[(long long)m * g.ld_act + i] = av;
      if (g.mu_out) dr_g(g.mu_out)[(long long)m * g.ld_mu + i] = muv;
      if (g.sig_out) dr_g(g.sig_out)[(long long)m * g.ld_sig + i] = sg;
      if (g.ls_save) dr_g(g.ls_save)[(long long)m * g.ld_ls + i] = lr;
    }
  }
}

__device__ __forceinline__ void epilogue_store(const GemmArgs& g, int m, int n, float acc) {
  epilogue_store_b(g, m, n, acc, g.bias ? dr_g(g.bias)[n] : 0.f);
}

// ---------------------------------------------------------------------------
// The categorical-sampler head as its own kernel: logits = SiLU(LN(x)) W^T + b
// (K <= 256), then per group of C = 32 classes softmax, 1 % unimix,
// argmax(p_hat / Exp(1)) and the straight-through one-hot (VAE.py:77-99 on
// latent_mapper.3; DynamicsPredictors.py:31-40 on logit_net.6).  It runs once
// per warm-start / imagination step, 46 times per epoch, and the general
// skinny kernel spent 15.3 us on it at 256 rows (8 waves splitting a K of only
// 200, an 8-way LDS reduction, 512 workgroups in two dispatch rounds).  Here a
// workgroup of 4 waves owns 16 rows x 64 columns (two groups): the 16 rows and
// 64 weight rows are read once into LDS with every load issued before the
// first wait, the LayerNorm-SiLU runs on the way (a wave per row, DPP
// statistics), wave w then accumulates output columns 16w..16w+15 over the
// whole K (two accumulators alternating per 16-k chunk: consecutive MFMAs are
// independent), and the logits pass through LDS to the sampler, two (row,
// group) pairs per wave instruction.  256 rows = 256 workgroups, one round.
// ---------------------------------------------------------------------------
#define LS_MT 16
#define LS_NT 64
#define LS_KMAX 256
#define LS_SO (LS_NT + 4)  // logit row stride: float4 rows, the 16 x 4 fragment writes hit 64 banks
static size_t ln_sample_lds_bytes(int K) {
  const int KP = ((K + 15) & ~15) + 8;  // 8 mod 16 dwords: conflict-free ds_read_b128 fragments
  return sizeof(float) * ((size_t)(LS_MT + LS_NT) * KP + (size_t)LS_MT * LS_SO);
}

// NK = K16 / 16 k-chunks, a compile-time count: the fragment reads of the
// whole K are ds_read_b128s the compiler can issue ahead of the MFMA chain.
// Nothing after the first barrier loads from global memory: the sampler noise
// (explicit q, or the Philox draws computed while the tile loads are in
// flight) is in registers before the LayerNorm, and every load is branch-free
// (a load inside a branch is waited for at the join, one round trip each).
template <int NK>
__global__ __launch_bounds__(256) void k_ln_gemm_sample(GemmArgs ga) {
  __shared__ GemmArgs g;
  dr_stage_args(ga, g, threadIdx.x);
  const int M = dr_uni(g.M), N = dr_uni(g.N), K = dr_uni(g.K);
  const int tiles_m = (M + LS_MT - 1) / LS_MT, tiles_n = N / LS_NT;
  // row tiles reading one weight slice are adjacent (one XCD's L2)
  const int lt = dr_xcd_tile(blockIdx.x, tiles_m * tiles_n);
  if (lt < 0) return;
  const int tn = lt / tiles_m, tm = lt - tn * tiles_m;
  const int m0 = tm * LS_MT, n0 = tn * LS_NT;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  DR_TS(dr_tbuf_gemm, 0);
  constexpr int K16 = 16 * NK, KP = K16 + 8;
  const int K4 = K >> 2;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sA = smem;                  // [LS_MT][KP]   SiLU(LN(x)) rows
  float* sB = smem + LS_MT * KP;     // [LS_NT][KP]   weight rows
  float* sO = sB + LS_NT * KP;       // [LS_MT][LS_SO] logits
  const float* A = dr_uni(g.A);
  const float* W = dr_uni(g.W);
  const int lda = dr_uni((int)g.lda), ldb = dr_uni((int)g.ldb);
  // every global load of the tile, issued together: 4 LayerNorm rows, 16
  // weight rows, gamma / beta (one float4 per lane each: K <= 256), the bias
  // of the column this lane finalises and the sampler noise / Philox state
  // the Philox state through the scalar cache (lgkmcnt): the draws below do
  // not wait for the tile loads
  typedef const __attribute__((address_space(4))) unsigned long long* dr_cu64;
  const unsigned long long* rngp = g.noise.rng ? g.noise.rng : reinterpret_cast<const unsigned long long*>(W);
  const unsigned long long rng_seed = ((dr_cu64)rngp)[0], rng_off = ((dr_cu64)rngp)[1];
  const bool okk = lane < K4;
  const unsigned ek = okk ? (unsigned)(4 * lane) : 0u;
  float4 xa[4], xb[16];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wave + 4 * i;
    const bool ok = okk && m < M;
    xa[i] = dr_ld4(A, ok ? (unsigned)m * (unsigned)lda + 4u * lane : 0u);
    if (!ok) xa[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int n = n0 + 16 * wave + j;
    xb[j] = dr_ld4(W, okk ? (unsigned)n * (unsigned)ldb + 4u * lane : 0u);
    if (!okk) xb[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const float4 gv = dr_ld4(dr_uni(g.ln_g), ek), bv = dr_ld4(dr_uni(g.ln_b), ek);
  const float* bias = dr_uni(g.bias);
  const int ncol = n0 + 16 * wave + r;
  const float bcol = dr_ld1(bias ? bias : W, bias ? (unsigned)ncol : 0u);
  // sampler: 16 rows x 2 groups = 32 (row, group) pairs, 8 lanes per pair
  // and 4 consecutive classes per lane: lane -> row 4 wave + lane / 16, group
  // (lane / 8) % 2, classes 4 (lane % 8) .. + 3
  constexpr int C = 32;
  const int Rg = dr_uni(g.R), sub = lane & 7, ml_s = 4 * wave + (lane >> 4), gl_s = (lane >> 3) & 1;
  const int m_s = m0 + ml_s, grp_s = (n0 >> 5) + gl_s, c_s = 4 * sub;
  const bool act_s = m_s < M;
  const float* qsrc = dr_uni(g.noise.q);
  const bool explicit_q = qsrc != nullptr;
  // explicit q: one float4 per lane, loaded branch-free (from W, unused, in
  // Philox mode) into registers of its own -- a load in a branch, or one
  // whose registers the Philox branch overwrites, is waited for right there
  const float* qb = explicit_q ? qsrc + (long long)g.step * M * Rg * C : W;
  const float4 qx = dr_ld4(qb, explicit_q ? (unsigned)(((act_s ? m_s : 0) * Rg + grp_s) * C + c_s) : 0u);
  float4 qn = make_float4(1.f, 1.f, 1.f, 1.f);
  float* a_out = dr_uni(g.a_out);
  const int ld_aout = dr_uni((int)g.ld_aout);
  const bool store_a = a_out != nullptr && tn == 0;
  DR_TS(dr_tbuf_gemm, 1);
  if (!explicit_q) {
    // Philox Exp(1) draws (VALU only) while the tile loads are in flight
    const uint32_t stream = (uint32_t)(g.noise.stream + g.step), row = (uint32_t)(g.noise.row0 + m_s);
    const uint32_t e0 = (uint32_t)(grp_s * C + c_s);
    qn.x = dr_exp1_k(rng_seed, rng_off, stream, row, e0);
    qn.y = dr_exp1_k(rng_seed, rng_off, stream, row, e0 + 1);
    qn.z = dr_exp1_k(rng_seed, rng_off, stream, row, e0 + 2);
    qn.w = dr_exp1_k(rng_seed, rng_off, stream, row, e0 + 3);
  }
  // LayerNorm (eps 1e-5) + SiLU of this wave's 4 rows, as the skinny kernel's prologue
  const bool in16 = lane < (K16 >> 2);  // lanes that write the zero-padded K16 row
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ml = wave + 4 * i, m = m0 + ml;
    float4 x = xa[i];
    const float mean = wave_sum(okk ? (x.x + x.y) + (x.z + x.w) : 0.f) / (float)K;
    float sq = 0.f;
    if (okk) {
      const float dx = x.x - mean, dy = x.y - mean, dz = x.z - mean, dw = x.w - mean;
      sq = (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)K + 1e-5f);
    float4 y;
    y.x = dr_silu_fast((x.x - mean) * rstd * gv.x + bv.x);
    y.y = dr_silu_fast((x.y - mean) * rstd * gv.y + bv.y);
    y.z = dr_silu_fast((x.z - mean) * rstd * gv.z + bv.z);
    y.w = dr_silu_fast((x.w - mean) * rstd * gv.w + bv.w);
    if (!okk || m >= M) y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in16) *reinterpret_cast<float4*>(&sA[ml * KP + 4 * lane]) = y;
    if (store_a && okk && m < M) dr_st4(a_out, (unsigned)m * (unsigned)ld_aout + 4u * lane, y);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (in16) *reinterpret_cast<float4*>(&sB[(16 * wave + j) * KP + 4 * lane]) = xb[j];
  DR_TS(dr_tbuf_gemm, 2);
  __syncthreads();
  DR_TS(dr_tbuf_gemm, 3);
  // wave w: output columns 16w..16w+15 of the 16 rows, the whole K; two
  // accumulators alternating per 16-k chunk (consecutive MFMAs independent)
  f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
  const float* pa = sA + r * KP + 4 * q;
  const float* pb = sB + (16 * wave + r) * KP + 4 * q;
#pragma unroll
  for (int kc = 0; kc < NK; ++kc) {
    const float4 a = *reinterpret_cast<const float4*>(pa + 16 * kc);
    const float4 b = *reinterpret_cast<const float4*>(pb + 16 * kc);
    f32x4& t = acc[kc & 1];
    t = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, t, 0, 0, 0);
    t = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, t, 0, 0, 0);
  }
  DR_TS(dr_tbuf_gemm, 4);
  // logits: lane (r, q) holds rows 4q..4q+3 of column ncol
  float* Y = dr_uni(g.Y);
  const long long ldy = g.ldy;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ml = 4 * q + e, m = m0 + ml;
    const float v = (acc[0][e] + acc[1][e]) + bcol;
    sO[ml * LS_SO + 16 * wave + r] = v;
    if (Y && m < M) dr_g(Y)[(long long)m * ldy + ncol] = v;
  }
  __syncthreads();
  DR_TS(dr_tbuf_gemm, 5);
  // the sampler (softmax, 1 % unimix, argmax(p_hat / q), straight-through
  // one-hot): 8-lane DPP reductions, no loads, no LDS permutes
  const float unimix = g.unimix;
  float x[4];
  {
    const float4 xv = *reinterpret_cast<const float4*>(&sO[ml_s * LS_SO + gl_s * C + c_s]);
    x[0] = xv.x, x[1] = xv.y, x[2] = xv.z, x[3] = xv.w;
  }
  if (explicit_q) qn = qx;
  const float qv[4] = {qn.x, qn.y, qn.z, qn.w};
  float mx = act_s ? fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])) : -INFINITY;
  mx = group_max(mx, 8);
  float ex[4], pu[4], p[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) ex[t] = act_s ? expf(x[t] - mx) : 0.0f;
  const float se = group_sum((ex[0] + ex[1]) + (ex[2] + ex[3]), 8);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    p[t] = ex[t] / se;
    pu[t] = act_s ? (0.99f * p[t] + unimix) : 0.0f;
  }
  const float sp = group_sum((pu[0] + pu[1]) + (pu[2] + pu[3]), 8);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  if (act_s) {
    best = (pu[0] / sp) / qv[0];
    bi = c_s;
#pragma unroll
    for (int t = 1; t < 4; ++t) {
      const float v = (pu[t] / sp) / qv[t];
      bi = v > best ? c_s + t : bi;  // ties keep the lower class
      best = fmaxf(best, v);
    }
  }
  group_argmax(best, bi, 8);
  if (act_s) {
    float4 z;
    z.x = (c_s + 0 == bi) ? ((1.0f + pu[0]) - pu[0]) : 0.0f;
    z.y = (c_s + 1 == bi) ? ((1.0f + pu[1]) - pu[1]) : 0.0f;
    z.z = (c_s + 2 == bi) ? ((1.0f + pu[2]) - pu[2]) : 0.0f;
    z.w = (c_s + 3 == bi) ? ((1.0f + pu[3]) - pu[3]) : 0.0f;
    *(DR_GLOBAL dr_f4*)(dr_g(g.z_out) + ((long long)m_s * g.ldz + grp_s * C + c_s)) = dr_f4{z.x, z.y, z.z, z.w};
    if (g.soft_out)
      *(DR_GLOBAL dr_f4*)(dr_g(g.soft_out) + ((long long)m_s * g.ld_soft + grp_s * C + c_s)) = dr_f4{p[0], p[1], p[2], p[3]};
    if (g.idx_out && sub == 0) dr_g(g.idx_out)[m_s * Rg + grp_s] = bi;
    if (g.zval_out && (unsigned)(bi - c_s) < 4u) {
      const int t = bi - c_s;
      const float pb = t == 0 ? pu[0] : t == 1 ? pu[1] : t == 2 ? pu[2] : pu[3];
      dr_g(g.zval_out)[m_s * Rg + grp_s] = (1.0f + pb) - pb;
    }
  }
  DR_TS(dr_tbuf_gemm, 6);
}

// ---------------------------------------------------------------------------
// Tile GEMM for the mid-size problems (M >= 256 rows or TN weight gradients):
// BM x BN output tile, 4 waves (2 x 2), K in chunks of 32 double-buffered
// through LDS (rows padded to 36 floats, fragments read as float4 along k).
// Operand layouts: A [M][K] (MK) or [K][M] (KM), B [N][K] (NK) or [K][N]
// (KN); MK/NK rows load as float4 (VEC), KM/KN as coalesced scalars
// transposed into LDS.  Optional deterministic split-K: each split writes a
// partial tile to splitk_ws and k_splitk_finish sums the splits in order and
// applies the epilogue.
// ---------------------------------------------------------------------------
#define DR_TILE_SPLITS 4  // = DR_SPLITK_MAX (engine_util.h): scratch sized for it

__device__ __forceinline__ float tile_b_kn(const GemmArgs& g, const float* W, int ldb, int n, int k) {
  if (k >= g.ksplitB) return dr_g(g.W2)[(long long)(k - g.ksplitB) * g.ldb2 + n];
  if (n >= g.nsplitB) return dr_g(g.W2)[(long long)k * g.ldb2 + (n - g.nsplitB)];
  return dr_ld1(W, (unsigned)(k * ldb + n));
}
// the same element as tile_b_kn as ONE branch-free load (address by select):
// a load inside a branch is waited for before the branch joins, which turned
// the tile kernel's load-ahead ring into one round trip per chunk
__device__ __forceinline__ float tile_b_kn_ld(const GemmArgs& g, const float* W, int ldb, int n, int k) {
  const bool w2k = k >= g.ksplitB, w2n = n >= g.nsplitB;
  const float* base = (w2k || w2n) ? g.W2 : W;
  const long long e = w2k ? (long long)(k - g.ksplitB) * g.ldb2 + n
                          : (w2n ? (long long)k * g.ldb2 + (n - g.nsplitB) : (long long)k * ldb + n);
  return dr_g(base)[e];
}

// NW waves: 4 as 2 x 2 (32 x 32 wave tiles at 64 x 64), 8 as 4 x 2 (16 x 16
// wave tiles at 64 x 32: two waves per SIMD hide the per-chunk barrier and
// LDS latency that one wave per SIMD exposes at these short K ranges)
template <int BM, int BN, int KC, bool A_KM, bool B_KN, bool VEC, int NW = 4>
__global__ __launch_bounds__(64 * NW) void k_gemm_tile(GemmBatch gb, int splits, int npack) {
  constexpr int NTH = 64 * NW;
  constexpr int TLDS = KC + 8;  // = 8 mod 16 dwords: conflict-free ds_read_b128 fragments
  constexpr int KQ = KC / 4;  // float4 per row piece
  __shared__ GemmArgs s_args;
  int pz;
  const int plt = dr_pack_tile<BM, BN>(gb, npack, pz);
  if (plt == -1) return;
  dr_stage_args(gb.p[pz], s_args, threadIdx.x);
  const GemmArgs& g = s_args;
  const int M = dr_uni(g.M), N = dr_uni(g.N), K = dr_uni(g.K);
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const int lt = plt >= 0 ? plt : dr_xcd_tile(blockIdx.x, tiles_m * tiles_n);
  if (lt < 0) return;
  const int tn = lt / tiles_m, tm = lt - tn * tiles_m;  // m-tiles sharing a weight slice are adjacent
  const int m0 = tm * BM, n0 = tn * BN;
  const int nch = (K + KC - 1) / KC;
  const int per = (nch + splits - 1) / splits;
  const int c0 = blockIdx.y * per, c1 = min(nch, c0 + per);
  const float* A = dr_uni(g.A);
  const float* W = dr_uni(g.W);
  const int lda = dr_uni((int)g.lda), ldb = dr_uni((int)g.ldb);
  const int ksA = dr_uni(g.ksplitA);
  const float* A2 = dr_uni(g.A2);
  const int lda2 = dr_uni((int)g.lda2);

  __shared__ __attribute__((aligned(16))) float As[2][BM][TLDS];
  __shared__ __attribute__((aligned(16))) float Bs[2][BN][TLDS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  // row-major loader (MK / NK): thread -> (row prow + RS i, float4 quad)
  constexpr int RS = NTH / KQ;
  constexpr int APT = BM * KQ / NTH, BPT = BN * KQ / NTH;
  // transposed loader (KM / KN): thread -> (m = tid % BM, k quad tid / BM + AQ i):
  // four scalar loads down k, each coalesced over the wave's consecutive m,
  // land as ONE float4 row piece in LDS -- the same [m][k] layout and
  // conflict-free ds_write_b128 as the row-major path (a transposing scatter
  // of float4-along-m loads hits one LDS bank 16 times)
  constexpr int AQ = NTH / BM, BQ = NTH / BN;
  constexpr int APTT = KQ / AQ, BPTT = KQ / BQ;
  static_assert(APT >= 1 && BPT >= 1 && AQ >= 1 && BQ >= 1, "tile");
  static_assert(A_KM ? APTT == APT : true, "loader");
  static_assert(B_KN ? BPTT == BPT : true, "loader");
  // register ring: chunk loads are issued PIPE chunks ahead of their use
  constexpr int PIPE = 3;
  float4 ra[PIPE][APT], rb[PIPE][BPT];
  // every load is issued unconditionally (out-of-range elements read a valid
  // address) and zeroed at the LDS store by these masks: loads under a
  // condition were each waited for before the next could issue
  unsigned mka[PIPE], mkb[PIPE];  // bit (4 i + cc) of A / B: element in range
  const int quad = tid % KQ, prow = tid / KQ;
  auto load = [&](int c, int sl) {
    const int k0 = c * KC;
    unsigned ma = 0u, mb = 0u;
#pragma unroll
    for (int i = 0; i < APT; ++i) {
      if (!A_KM) {
        const int m = m0 + prow + RS * i, k = k0 + 4 * quad;
        if (VEC) {
          const bool ok = m < M && k < K;
          const bool s1 = k < ksA;
          const float* base = s1 ? A : A2;
          const unsigned e = ok ? (unsigned)(s1 ? m * lda + k : m * lda2 + k - ksA) : 0u;
          ra[sl][i] = dr_ld4(ok ? base : W, e);
          ma |= ok ? (15u << (4 * i)) : 0u;
        } else {
          // (unaligned operands, rare: conditional scalar loads as before)
          float* v = &ra[sl][i].x;
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) {
            const int kk = k + cc;
            v[cc] = (m < M && kk < K) ? ((kk < ksA) ? dr_ld1(A, (unsigned)(m * lda + kk))
                                                    : dr_ld1(A2, (unsigned)(m * lda2 + kk - ksA)))
                                      : 0.f;
          }
          ma |= 15u << (4 * i);
        }
      } else {
        const int m = m0 + tid % BM, k = k0 + 4 * (tid / BM + AQ * i);
        float* v = &ra[sl][i].x;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const bool ok = k + cc < K && m < M;
          v[cc] = dr_ld1(A, ok ? (unsigned)((k + cc) * lda + m) : 0u);
          ma |= ok ? (1u << (4 * i + cc)) : 0u;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      if (!B_KN) {
        const int n = n0 + prow + RS * i, k = k0 + 4 * quad;
        if (VEC) {
          const bool ok = n < N && k < K;
          rb[sl][i] = dr_ld4(W, ok ? (unsigned)(n * ldb + k) : 0u);
          mb |= ok ? (15u << (4 * i)) : 0u;
        } else {
          float* v = &rb[sl][i].x;
#pragma unroll
          for (int cc = 0; cc < 4; ++cc) v[cc] = (n < N && k + cc < K) ? dr_ld1(W, (unsigned)(n * ldb + k + cc)) : 0.f;
          mb |= 15u << (4 * i);
        }
      } else {
        const int n = n0 + tid % BN, k = k0 + 4 * (tid / BN + BQ * i);
        float* v = &rb[sl][i].x;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
          const bool ok = k + cc < K && n < N;
          v[cc] = tile_b_kn_ld(g, W, ldb, ok ? n : 0, ok ? k + cc : 0);
          mb |= ok ? (1u << (4 * i + cc)) : 0u;
        }
      }
    }
    mka[sl] = ma;
    mkb[sl] = mb;
  };
  auto masked = [](float4 v, unsigned m, int i) {
    const unsigned b = m >> (4 * i);
    return make_float4(b & 1u ? v.x : 0.f, b & 2u ? v.y : 0.f, b & 4u ? v.z : 0.f, b & 8u ? v.w : 0.f);
  };
  auto store = [&](int sl, int buf) {
#pragma unroll
    for (int i = 0; i < APT; ++i) {
      const float4 v = masked(ra[sl][i], mka[sl], i);
      if (!A_KM) {
        *reinterpret_cast<float4*>(&As[buf][prow + RS * i][4 * quad]) = v;
      } else {
        *reinterpret_cast<float4*>(&As[buf][tid % BM][4 * (tid / BM + AQ * i)]) = v;
      }
    }
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
      const float4 v = masked(rb[sl][i], mkb[sl], i);
      if (!B_KN) {
        *reinterpret_cast<float4*>(&Bs[buf][prow + RS * i][4 * quad]) = v;
      } else {
        *reinterpret_cast<float4*>(&Bs[buf][tid % BN][4 * (tid / BN + BQ * i)]) = v;
      }
    }
  };

  constexpr int WGM = NW / 2;  // waves along M (2 along N)
  constexpr int WTM = BM / WGM, WTN = BN / 2, FM = WTM / 16, FN = WTN / 16;
  static_assert(FM >= 1 && FN >= 1, "wave tile");
  const int wm0 = (wave >> 1) * WTM, wn0 = (wave & 1) * WTN;
  const int r = lane & 15, q = lane >> 4;
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // (a split past the last chunk, c0 >= c1, loads chunk 0 and computes nothing)
  const int clast = max(c1 - 1, 0);
#pragma unroll
  for (int u = 0; u < PIPE; ++u) load(min(c0 + u, clast), u);
  if (c0 < c1) store(0, 0);
  __syncthreads();
  for (int cb = c0; cb < c1; cb += PIPE) {
#pragma unroll
    for (int u = 0; u < PIPE; ++u) {
      const int c = cb + u;
      if (c >= c1) break;
      const int buf = (c - c0) & 1;
      load(min(c + PIPE, clast), u);  // slot u was stored to LDS last iteration; past the end: unused
#pragma unroll
      for (int s = 0; s < KC; s += 16) {
        float4 a[FM], b[FN];
#pragma unroll
        for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const float4*>(&As[buf][wm0 + 16 * i + r][s + 4 * q]);
#pragma unroll
        for (int j = 0; j < FN; ++j) b[j] = *reinterpret_cast<const float4*>(&Bs[buf][wn0 + 16 * j + r][s + 4 * q]);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].x, b[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].y, b[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].z, b[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i].w, b[j].w, acc[i][j], 0, 0, 0);
      }
      if (c + 1 < c1) store((u + 1) % PIPE, buf ^ 1);
      dr_lds_barrier();  // keeps the PIPE-ahead loads in flight
    }
  }
  float* part = g.splitk_ws;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + wm0 + 16 * i + 4 * q + e, n = n0 + wn0 + 16 * j + r;
        if (m >= M || n >= N) continue;
        if (splits == 1) epilogue_store(g, m, n, acc[i][j][e]);
        else dr_g(part)[((long long)blockIdx.y * M + m) * N + n] = acc[i][j][e];
      }
}

// ---------------------------------------------------------------------------
// bf16 perf-mode tile GEMM (GemmArgs.bf16): NT, f32 operands in HBM rounded to
// bf16 (RNE) as they are staged into LDS, v_mfma_f32_16x16x32_bf16 with f32
// accumulation, the f32 tile kernel's epilogue / split-K.  K chunks of 64:
// a thread stages units of 8 consecutive k (two float4 loads -> one 16-byte
// LDS row piece); rows are 40 dwords (8 mod 16): conflict-free ds_read_b128
// fragments, lane (r, q) reading k = 8q..8q+7 of its row.
// ---------------------------------------------------------------------------
typedef __bf16 dr_bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ uint32_t dr_pack_bf16x2(float a, float b) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  const bf16x2_t v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(uint32_t, v);
}

template <int BM, int BN, int NW>
__global__ __launch_bounds__(64 * NW) void k_gemm_tile_b16(GemmBatch gb, int splits) {
  constexpr int NTH = 64 * NW, KC = 64, UPR = KC / 8, TL = KC / 2 + 8;
  __shared__ GemmArgs s_args;
  dr_stage_args(gb.p[blockIdx.z], s_args, threadIdx.x);
  const GemmArgs& g = s_args;
  const int M = dr_uni(g.M), N = dr_uni(g.N), K = dr_uni(g.K);
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  const int lt = dr_xcd_tile(blockIdx.x, tiles_m * tiles_n);
  if (lt < 0) return;
  const int tn = lt / tiles_m, tm = lt - tn * tiles_m;
  const int m0 = tm * BM, n0 = tn * BN;
  const int nch = (K + KC - 1) / KC;
  const int per = (nch + splits - 1) / splits;
  const int c0 = blockIdx.y * per, c1 = min(nch, c0 + per);
  const float* A = dr_uni(g.A);
  const float* A2 = dr_uni(g.A2);
  const float* W = dr_uni(g.W);
  const int lda = dr_uni((int)g.lda), lda2 = dr_uni((int)g.lda2), ldb = dr_uni((int)g.ldb);
  const int ksA = dr_uni(g.ksplitA);
  __shared__ __attribute__((aligned(16))) uint32_t As[2][BM][TL];
  __shared__ __attribute__((aligned(16))) uint32_t Bs[2][BN][TL];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  constexpr int APT = (BM * UPR + NTH - 1) / NTH, BPT = (BN * UPR + NTH - 1) / NTH;
  // the chunk in flight stays f32 in registers, masked and rounded to bf16 at
  // the LDS store (rounding in the loader waited for the loads at once, so the
  // next chunk's loads did not overlap this chunk's MFMAs); macros, not
  // lambdas: capturing lambdas left the kernel's scalars in scratch memory
  typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
  f32x4 ra0[APT], ra1[APT], rb0[BPT], rb1[BPT];
  unsigned mka = 0u, mkb = 0u;
#define B16_LOAD(C_)                                                                                 \
  do {                                                                                               \
    const int k0 = (C_) * KC;                                                                        \
    mka = mkb = 0u;                                                                                  \
    _Pragma("unroll") for (int i = 0; i < APT; ++i) {                                                \
      const int u = tid + NTH * i, row = u / UPR, k = k0 + 8 * (u - row * UPR), m = m0 + row;        \
      const bool ok = u < BM * UPR && m < M && k < K;                                                \
      const bool s1 = k < ksA;                                                                       \
      const float* base = ok ? (s1 ? A : A2) : W;                                                    \
      const unsigned e = ok ? (unsigned)(s1 ? m * lda + k : m * lda2 + k - ksA) : 0u;                \
      ra0[i] = *(const DR_GLOBAL f32x4*)((const DR_GLOBAL char*)base + (e << 2));                    \
      ra1[i] = *(const DR_GLOBAL f32x4*)((const DR_GLOBAL char*)base + ((e + 4u) << 2));             \
      mka |= ok ? (1u << i) : 0u;                                                                    \
    }                                                                                                \
    _Pragma("unroll") for (int i = 0; i < BPT; ++i) {                                                \
      const int u = tid + NTH * i, row = u / UPR, k = k0 + 8 * (u - row * UPR), n = n0 + row;        \
      const bool ok = u < BN * UPR && n < N && k < K;                                                \
      const unsigned e = ok ? (unsigned)(n * ldb + k) : 0u;                                          \
      rb0[i] = *(const DR_GLOBAL f32x4*)((const DR_GLOBAL char*)W + (e << 2));                       \
      rb1[i] = *(const DR_GLOBAL f32x4*)((const DR_GLOBAL char*)W + ((e + 4u) << 2));                \
      mkb |= ok ? (1u << i) : 0u;                                                                    \
    }                                                                                                \
  } while (0)
#define B16_PACK(X0_, X1_, OK_)                                                                      \
  (u32x4_t){dr_pack_bf16x2((OK_) ? (X0_)[0] : 0.f, (OK_) ? (X0_)[1] : 0.f),                          \
            dr_pack_bf16x2((OK_) ? (X0_)[2] : 0.f, (OK_) ? (X0_)[3] : 0.f),                          \
            dr_pack_bf16x2((OK_) ? (X1_)[0] : 0.f, (OK_) ? (X1_)[1] : 0.f),                          \
            dr_pack_bf16x2((OK_) ? (X1_)[2] : 0.f, (OK_) ? (X1_)[3] : 0.f)}
#define B16_STORE(BUF_)                                                                              \
  do {                                                                                               \
    _Pragma("unroll") for (int i = 0; i < APT; ++i) {                                                \
      const int u = tid + NTH * i, row = u / UPR, uc = u - row * UPR;                                \
      const bool ok = (mka >> i) & 1u;                                                               \
      if (u < BM * UPR) *reinterpret_cast<u32x4_t*>(&As[BUF_][row][4 * uc]) = B16_PACK(ra0[i], ra1[i], ok); \
    }                                                                                                \
    _Pragma("unroll") for (int i = 0; i < BPT; ++i) {                                                \
      const int u = tid + NTH * i, row = u / UPR, uc = u - row * UPR;                                \
      const bool ok = (mkb >> i) & 1u;                                                               \
      if (u < BN * UPR) *reinterpret_cast<u32x4_t*>(&Bs[BUF_][row][4 * uc]) = B16_PACK(rb0[i], rb1[i], ok); \
    }                                                                                                \
  } while (0)
  constexpr int WGM = NW / 2;
  constexpr int WTM = BM / WGM, WTN = BN / 2, FM = WTM / 16, FN = WTN / 16;
  static_assert(FM >= 1 && FN >= 1, "wave tile");
  const int wm0 = (wave >> 1) * WTM, wn0 = (wave & 1) * WTN;
  const int r = lane & 15, q = lane >> 4;
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int clast = max(c1 - 1, 0);  // (a split past the last chunk loads chunk 0 and computes nothing)
  B16_LOAD(min(c0, clast));
  if (c0 < c1) B16_STORE(0);
  __syncthreads();
  for (int c = c0; c < c1; ++c) {
    const int buf = (c - c0) & 1;
    B16_LOAD(min(c + 1, clast));  // in flight while this chunk's MFMAs run (past the end: unused)
#pragma unroll
    for (int s = 0; s < KC / 32; ++s) {
      uint4 a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const uint4*>(&As[buf][wm0 + 16 * i + r][16 * s + 4 * q]);
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = *reinterpret_cast<const uint4*>(&Bs[buf][wn0 + 16 * j + r][16 * s + 4 * q]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(dr_bf16x8, a[i]),
                                                              __builtin_bit_cast(dr_bf16x8, b[j]), acc[i][j], 0, 0, 0);
    }
    if (c + 1 < c1) B16_STORE(buf ^ 1);
    __syncthreads();
  }
#undef B16_LOAD
#undef B16_PACK
#undef B16_STORE
  float* part = g.splitk_ws;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + wm0 + 16 * i + 4 * q + e, n = n0 + wn0 + 16 * j + r;
        if (m >= M || n >= N) continue;
        if (splits == 1) epilogue_store(g, m, n, acc[i][j][e]);
        else dr_g(part)[((long long)blockIdx.y * M + m) * N + n] = acc[i][j][e];
      }
}

// ---------------------------------------------------------------------------
// Per-step chain products at 128-512 rows (GRU hidden product, heads' first
// layers, BPTT input gradients): NT, f32 MFMA, no LDS staging.  Every wave of
// the workgroup computes the WHOLE BM x BN tile over its own run of 32-k
// blocks (K split over the waves), so no operand fragment is shared between
// waves: each lane loads its MFMA fragments straight from L2 into registers
// (lane (r, q) reads 8 consecutive k of row r: a 16-row x 128-B coalesced
// line per pair of float4 loads), D blocks ahead in a register ring, with no
// barrier in the K loop.  The 8 k of a lane feed 8 consecutive MFMAs; A and B
// use the same k order, so the sum is the product's.  The NW partial tiles
// meet once in LDS at the end.  K % 8 == 0, ksplitA % 8 == 0 (a lane's 8-run
// never straddles A / A2), 16-byte aligned rows (host-checked: wk_ok).
// ---------------------------------------------------------------------------
// npack > 0: the npack problems' tiles are packed into one linear grid (no
// workgroups of a smaller problem idle in a blockIdx.z slice sized for the
// largest: a grouped launch of the GRU hidden product (456 tiles) with a
// 56-tile Linear ran 21.7 us against 12.3 for the product alone)
template <int BM, int BN, int NW, int D, int KMAP = 0>
__global__ __launch_bounds__(64 * NW) void k_gemm_wk(GemmBatch gb, int splits, int npack) {
  constexpr int NTH = 64 * NW, FM = BM / 16, FN = BN / 16, NT4 = FM * FN * 256;
  static_assert(FM * FN >= 4, "at least 4 independent accumulators per wave (40-cycle MFMA latency)");
  __shared__ GemmArgs s_args;
  __shared__ __attribute__((aligned(16))) float red[NW][FM * FN * 4][64];
  int z = blockIdx.z, lt = -1;
  if (npack > 0) {
    int tot = 0;
    for (int i = 0; i < npack; ++i) tot += ((gb.p[i].M + BM - 1) / BM) * ((gb.p[i].N + BN - 1) / BN);
    lt = dr_xcd_tile(blockIdx.x, tot);
    if (lt < 0) return;
    z = 0;
    for (int i = 0; i + 1 < npack; ++i) {
      const int ti = ((gb.p[i].M + BM - 1) / BM) * ((gb.p[i].N + BN - 1) / BN);
      if (lt < ti) break;
      lt -= ti;
      z = i + 1;
    }
  }
  dr_stage_args(gb.p[z], s_args, threadIdx.x);
  const GemmArgs& g = s_args;
  const int M = dr_uni(g.M), N = dr_uni(g.N), K = dr_uni(g.K);
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + BN - 1) / BN;
  if (npack == 0) lt = dr_xcd_tile(blockIdx.x, tiles_m * tiles_n);
  if (lt < 0) return;
  const int tn = lt / tiles_m, tm = lt - tn * tiles_m;  // m-tiles sharing a weight slice are adjacent
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  const float* A = dr_uni(g.A);
  const float* A2 = dr_uni(g.A2);
  const float* W = dr_uni(g.W);
  const int lda = dr_uni((int)g.lda), lda2 = dr_uni((int)g.lda2), ldb = dr_uni((int)g.ldb);
  const int ksA = dr_uni(g.ksplitA);

  // bias of the outputs this thread finalises: issued now, waited for at the end
  constexpr int NEPI = (NT4 + NTH - 1) / NTH;
  float ebias[NEPI];
  {
    const float* bias = dr_uni(g.bias);
#pragma unroll
    for (int i = 0; i < NEPI; ++i) {
      const int x = tid + NTH * i, l = x & 63, tj = x >> 8;
      const int n = n0 + (tj % FN) * 16 + (l & 15);
      const bool ok = bias && splits == 1 && x < NT4 && n < N;
      const float v = dr_ld1(ok ? bias : W, ok ? (unsigned)n : 0u);
      ebias[i] = ok ? v : 0.f;
    }
  }

  // this workgroup's 32-k blocks (split-K over blockIdx.y), then this wave's
  const int nkb = (K + 31) >> 5;
  const int per = (nkb + splits - 1) / splits;
  const int kb0 = min(nkb, (int)blockIdx.y * per), kb1 = min(nkb, kb0 + per);
  const int nbg = kb1 - kb0;
  const int b0 = kb0 + (nbg * wave) / NW, b1 = kb0 + (nbg * (wave + 1)) / NW;
  const int blast = max(min(b1, nkb) - 1, 0);  // loads past this wave's run re-read its last block (unused)

  // per-lane row offsets (rows past M / N read row M-1 / N-1: valid addresses, outputs discarded)
  unsigned oa[FM], oa2[FM], ob[FN];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = min(m0 + 16 * i + r, M - 1);
    oa[i] = (unsigned)(m * lda);
    oa2[i] = (unsigned)(m * lda2);
  }
#pragma unroll
  for (int j = 0; j < FN; ++j) ob[j] = (unsigned)(min(n0 + 16 * j + r, N - 1) * ldb);

  f32x4 ra[D][FM][2], rb[D][FN][2];
  // KMAP 0: lane q reads k = 8q..8q+7 of the block (two float4, one 32-B run);
  // KMAP 1: k = 4q..4q+3 and 16+4q..16+4q+3 (each instruction a 64-B run per row)
  constexpr int KL = KMAP == 0 ? 8 : 4, KH = KMAP == 0 ? 4 : 16;
  auto load = [&](int b, int sl) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int k = 32 * b + KL * q + KH * h;
      const int kk = k < K ? k : 0;  // lanes past K re-read k = 0 (zeroed before use)
      const bool s1 = kk < ksA;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const float* base = s1 ? A : A2;
        const unsigned e = s1 ? oa[i] + (unsigned)kk : oa2[i] + (unsigned)(kk - ksA);
        ra[sl][i][h] = *(const DR_GLOBAL f32x4*)((const DR_GLOBAL char*)base + (e << 2));
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const unsigned e = ob[j] + (unsigned)kk;
        rb[sl][j][h] = *(const DR_GLOBAL f32x4*)((const DR_GLOBAL char*)W + (e << 2));
      }
    }
  };
  f32x4 acc[1][FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[0][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < D; ++u) load(min(b0 + u, blast), u);
  const int nbw = b1 - b0;
  const bool ktail = (K & 31) != 0;
  for (int bb = 0; bb < nbw; bb += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      if (bb + u >= nbw) break;
      const int b = b0 + bb + u;
      if (ktail && b == nkb - 1) {  // the K tail: zero the runs past K
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          if (32 * b + KL * q + KH * h < K) continue;
#pragma unroll
          for (int i = 0; i < FM; ++i) ra[u][i][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < FN; ++j) rb[u][j][h] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
      }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int i = 0; i < FM; ++i)
#pragma unroll
            for (int j = 0; j < FN; ++j)
              acc[0][i][j] =
                  __builtin_amdgcn_mfma_f32_16x16x4f32(ra[u][i][h][c], rb[u][j][h][c], acc[0][i][j], 0, 0, 0);
      load(min(b + D, blast), u);  // unconditional: a load under a branch is waited for at once
    }
  }
  // the NW partial tiles meet in LDS; element (t, e, l) of tile t = (i, j):
  // D[row 4 (l >> 4) + e][col l & 15]
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const f32x4 v = acc[0][i][j];
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wave][(i * FN + j) * 4 + e][lane] = v[e];
    }
  __syncthreads();
  float* part = g.splitk_ws;
#pragma unroll
  for (int ii = 0; ii < NEPI; ++ii) {
    const int x = tid + NTH * ii;
    if (x >= NT4) break;
    const int l = x & 63, e = (x >> 6) & 3, tj = x >> 8;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[w][tj * 4 + e][l];
    const int t = tj / FN, j = tj - t * FN;
    const int m = m0 + t * 16 + 4 * (l >> 4) + e, n = n0 + j * 16 + (l & 15);
    if (m >= M || n >= N) continue;
    if (splits == 1) epilogue_store_b(g, m, n, v, ebias[ii]);
    else dr_g(part)[((long long)blockIdx.y * M + m) * N + n] = v;
  }
}

// ---------------------------------------------------------------------------
// The wave-K chain kernel on the bf16 MFMA (v_mfma_f32_16x16x32_bf16).  Same
// work split as k_gemm_wk<32, 32, 4> -- every wave computes the whole 32 x 32
// tile over its own run of 32-k chunks, fragments straight from L2 into a
// register ring, the partial tiles met once in LDS -- but the products run on
// bf16 planes: W pre-split once per call into [K/32][3][Np][32]
// (op_nt_repack_split3, RNE), the A rows split in registers as they arrive
// (split3_pair: truncation, exact residuals).  NTP = 3: the six products of
// order >= 2^-16 (conv_split.hip's f32-accurate scheme, 2.67x the f32 MFMA
// rate); NTP = 1: A rounded to bf16 (RNE) times plane 0 (bf16 perf mode).
// Lane (r, q) loads k = 8q .. 8q + 7 of its rows -- the MFMA fragment -- and
// the accumulator holds row r, columns 4q .. 4q + 3 (B fragment first).
// ---------------------------------------------------------------------------
typedef unsigned wk_u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 wk_bf16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x4 wk_mfma(wk_u32x4 a, wk_u32x4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(wk_bf16x8, a), __builtin_bit_cast(wk_bf16x8, b),
                                                  c, 0, 0, 0);
}
__device__ __forceinline__ unsigned wk_pack_rne(float x0, float x1) {
  typedef __bf16 b2 __attribute__((ext_vector_type(2)));
  const b2 v = {(__bf16)x0, (__bf16)x1};
  return __builtin_bit_cast(unsigned, v);
}

template <int NTP, int D, int NW = 4, int FM = 2, bool A16 = false>
__global__ __launch_bounds__(64 * NW) void k_gemm_wks3(GemmBatch gb, int npack) {
  static_assert(!A16 || NTP == 1, "bf16 A copies feed the one-term form only");
  constexpr int FN = 2, BM = 16 * FM, NTH = 64 * NW, NT4 = FM * FN * 256;
  __shared__ GemmArgs s_args;
  __shared__ __attribute__((aligned(16))) float red[NW][FM * FN * 4][64];
  int z = 0;
  const int plt = dr_pack_tile<BM, 32>(gb, npack, z);
  if (plt == -1) return;
  dr_stage_args(gb.p[z], s_args, threadIdx.x);
  const GemmArgs& g = s_args;
  const int M = dr_uni(g.M), N = dr_uni(g.N), K = dr_uni(g.K);
  const int tiles_m = (M + BM - 1) / BM, tiles_n = (N + 31) / 32;
  const int lt = plt >= 0 ? plt : dr_xcd_tile(blockIdx.x, tiles_m * tiles_n);
  if (lt < 0) return;
  const int tn = lt / tiles_m, tm = lt - tn * tiles_m;  // row tiles of one weight slice adjacent
  const int m0 = tm * BM, n0 = tn * 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
  const float* A = dr_uni(g.A);
  const unsigned short* A16p = dr_uni(g.A16);
  const int lda = dr_uni((int)g.lda);
  const unsigned short* wr = dr_uni(g.wsplit);
  const int Np = dr_uni(g.wsplit_np);
  // bias of the outputs this thread finalises (waited for at the end)
  constexpr int NEPI = (NT4 + NTH - 1) / NTH;
  float ebias[NEPI];
  {
    const float* bias = dr_uni(g.bias);
#pragma unroll
    for (int i = 0; i < NEPI; ++i) {
      const int x = tid + NTH * i, l = x & 63, e = (x >> 6) & 3, tj = x >> 8;
      const int n = n0 + (tj % FN) * 16 + 4 * (l >> 4) + e;
      const bool ok = bias && x < NT4 && n < N;
      ebias[i] = ok ? dr_ld1(bias, (unsigned)n) : 0.f;
    }
  }
  const int nkc = (K + 31) >> 5;
  const int c0 = (nkc * wave) / NW, c1 = (nkc * (wave + 1)) / NW;
  const int clast = max(c1 - 1, 0);
  unsigned oa[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) oa[i] = (unsigned)(min(m0 + 16 * i + r, M - 1) * lda);
  unsigned ob[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) ob[j] = (unsigned)(n0 + 16 * j + r) * 32u + 8u * q;  // within a plane (Np >= n rows)
  f32x4 ra[A16 ? 1 : D][FM][2];
  wk_u32x4 ra16[A16 ? D : 1][FM];
  wk_u32x4 rb[D][NTP][FN];
  auto load = [&](int c, int sl) {
    const int k = 32 * c + 8 * q;
    const unsigned kk = k < K ? (unsigned)k : 0u;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      if constexpr (A16) {
        ra16[sl][i] = *(const DR_GLOBAL wk_u32x4*)((const DR_GLOBAL char*)A16p + ((oa[i] + kk) << 1));
      } else {
        ra[sl][i][0] = *(const DR_GLOBAL f32x4*)((const DR_GLOBAL char*)A + ((oa[i] + kk) << 2));
        ra[sl][i][1] = *(const DR_GLOBAL f32x4*)((const DR_GLOBAL char*)A + ((oa[i] + kk + 4) << 2));
      }
    }
#pragma unroll
    for (int p = 0; p < NTP; ++p)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const unsigned e = (unsigned)((c * 3 + p) * Np) * 32u + ob[j];
        rb[sl][p][j] = *(const DR_GLOBAL wk_u32x4*)((const DR_GLOBAL char*)wr + (e << 1));
      }
  };
  constexpr int NA = 1;
  f32x4 acc[NA][FM][FN];
#pragma unroll
  for (int a3 = 0; a3 < NA; ++a3)
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[a3][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < D; ++u) load(min(c0 + u, clast), u);
  const int ncw = c1 - c0;
  for (int cc = 0; cc < ncw; cc += D) {
#pragma unroll
    for (int u = 0; u < D; ++u) {
      if (cc + u >= ncw) break;
      const int c = c0 + cc + u;
      const bool kin = 32 * c + 8 * q < K;  // K % 8 == 0: a lane's 8-run is all in or all out
      wk_u32x4 a[NTP][FM];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if constexpr (A16) {
          a[0][i] = kin ? ra16[u][i] : (wk_u32x4){0u, 0u, 0u, 0u};
          continue;
        }
        f32x4 x0 = ra[A16 ? 0 : u][i][0], x1 = ra[A16 ? 0 : u][i][1];
        if (!kin) x0 = x1 = (f32x4){0.f, 0.f, 0.f, 0.f};
        if constexpr (NTP == 3) {
          unsigned h[4], m[4], l[4];
          split3_pair(x0[0], x0[1], h[0], m[0], l[0]);
          split3_pair(x0[2], x0[3], h[1], m[1], l[1]);
          split3_pair(x1[0], x1[1], h[2], m[2], l[2]);
          split3_pair(x1[2], x1[3], h[3], m[3], l[3]);
          a[0][i] = (wk_u32x4){h[0], h[1], h[2], h[3]};
          a[1 % NTP][i] = (wk_u32x4){m[0], m[1], m[2], m[3]};
          a[2 % NTP][i] = (wk_u32x4){l[0], l[1], l[2], l[3]};
        } else {
          a[0][i] = (wk_u32x4){wk_pack_rne(x0[0], x0[1]), wk_pack_rne(x0[2], x0[3]), wk_pack_rne(x1[0], x1[1]),
                               wk_pack_rne(x1[2], x1[3])};
        }
      }
#define DR_WK3(PA, PB, X)                        \
  _Pragma("unroll") for (int i = 0; i < FM; ++i) _Pragma("unroll") for (int j = 0; j < FN; ++j) acc[X][i][j] = \
      wk_mfma(rb[u][PB][j], a[PA][i], acc[X][i][j]);
      if constexpr (NTP == 3) {  // the six products of order >= 2^-16, smallest first
        DR_WK3(2 % NTP, 0, 0)
        DR_WK3(1 % NTP, 1 % NTP, 0)
        DR_WK3(0, 2 % NTP, 0)
        DR_WK3(1 % NTP, 0, 0)
        DR_WK3(0, 1 % NTP, 0)
      }
      DR_WK3(0, 0, 0)
#undef DR_WK3
      // unconditional: a load under a branch is waited for at once
      load(min(c + D, clast), u);
    }
  }
  // partial tiles meet in LDS; element (t, e, l) of tile t = (i, j): row 16 i + (l & 15), column 16 j + 4 (l >> 4) + e
  {
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const f32x4 v = acc[0][i][j];
#pragma unroll
        for (int e = 0; e < 4; ++e) red[wave][(i * FN + j) * 4 + e][lane] = v[e];
      }
  }
  __syncthreads();
#pragma unroll
  for (int ii = 0; ii < NEPI; ++ii) {
    const int x = tid + NTH * ii;
    if (x >= NT4) break;
    const int l = x & 63, e = (x >> 6) & 3, tj = x >> 8;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += red[w][tj * 4 + e][l];
    const int t = tj / FN, j = tj - t * FN;
    const int m = m0 + t * 16 + (l & 15), n = n0 + j * 16 + 4 * (l >> 4) + e;
    if (m >= M || n >= N) continue;
    epilogue_store_b(g, m, n, v, ebias[ii]);
  }
}

__global__ __launch_bounds__(256) void k_splitk_finish(GemmBatch gb, int splits) {
  // the problem's arguments staged in LDS: read straight from the by-value
  // batch at a run-time index, the 624-byte GemmArgs was copied to scratch
  // per thread (2.6 KB per lane, ~370 us per WM-step finish, r04g)
  __shared__ GemmArgs s_args;
  dr_stage_args(gb.p[blockIdx.z], s_args, threadIdx.x);
  const GemmArgs& g = s_args;
  const long long MN = (long long)g.M * g.N;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= MN) return;
  float v = 0.f;
  for (int sp = 0; sp < splits; ++sp) v += dr_g(g.splitk_ws)[sp * MN + i];
  const int m = (int)(i / g.N), n = (int)(i - (long long)m * g.N);
  epilogue_store(g, m, n, v);
}

// ---------------------------------------------------------------------------
// k_mlp2_tail: LN-SiLU -> Linear -> LN-SiLU -> Linear (+ epilogue), one launch
// ---------------------------------------------------------------------------
#define MLP2_KMAX 208  // K1, K2 <= 208 (the reference heads are 200 wide)
#define MLP2_NC 128
struct Mlp2Batch {
  Mlp2Args p[3];
};

// SiLU(LayerNorm(row)) of a row held one float4 per lane (k = 4 lane)
__device__ __forceinline__ float4 mlp2_ln_silu(float4 x, bool ok, int K, const float* gam, const float* bet, int k) {
  const float mean = wave_sum(ok ? (x.x + x.y) + (x.z + x.w) : 0.f) / (float)K;
  float sq = 0.f;
  if (ok) {
    const float dx = x.x - mean, dy = x.y - mean, dz = x.z - mean, dw = x.w - mean;
    sq = (dx * dx + dy * dy) + (dz * dz + dw * dw);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)K + 1e-5f);
  if (!ok) return make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 gv = dr_ld4(gam, (unsigned)k), bv = dr_ld4(bet, (unsigned)k);
  return make_float4(dr_silu_fast((x.x - mean) * rstd * gv.x + bv.x), dr_silu_fast((x.y - mean) * rstd * gv.y + bv.y),
                     dr_silu_fast((x.z - mean) * rstd * gv.z + bv.z), dr_silu_fast((x.w - mean) * rstd * gv.w + bv.w));
}

// [16 rows] x [16 cols of W] over K (padded to 16): lane (r, q) holds 4
// consecutive k of weight row n (loaded up front by mlp2_wload) and reads the
// matching 4 k of LDS row r; four accumulator chains keep consecutive MFMAs
// independent
#define MLP2_KS (MLP2_KMAX / 16)
__device__ __forceinline__ void mlp2_wload(float4 (&wv)[MLP2_KS], const float* W, int ldw, int n, bool nok, int K,
                                           int q) {
  const int ks = (K + 15) >> 4;
#pragma unroll
  for (int s = 0; s < MLP2_KS; ++s) {
    const int k = 16 * s + 4 * q;
    const bool ok = s < ks && nok && k < K;
    wv[s] = dr_ld4(W, ok ? (unsigned)(n * ldw + k) : 0u);
    if (!ok) wv[s] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
template <int LP>
__device__ __forceinline__ f32x4 mlp2_tile(const float (*ys)[LP], const float4 (&wv)[MLP2_KS], int K, int r, int q) {
  const int ks = (K + 15) >> 4;
  f32x4 c[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) c[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < MLP2_KS; ++s) {
    if (s < ks) {
      const float4 a = *reinterpret_cast<const float4*>(&ys[r][16 * s + 4 * q]);
      c[s & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wv[s].x, c[s & 3], 0, 0, 0);
      c[s & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wv[s].y, c[s & 3], 0, 0, 0);
      c[s & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wv[s].z, c[s & 3], 0, 0, 0);
      c[s & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wv[s].w, c[s & 3], 0, 0, 0);
    }
  }
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (c[0][e] + c[1][e]) + (c[2][e] + c[3][e]);
  return o;
}

// the same tile on ONE accumulator chain, k ascending: k_gemm_tile's order per output element (the critics'
// LN-SiLU layers ran there: k_ln_silu_rows, whose row arithmetic is mlp2_ln_silu's, then the 64 x 64 tile GEMM),
// so a head that asks for it keeps that route's bits.  (The tile GEMM pads K to 32 with zero products, which add
// nothing.)
template <int LP>
__device__ __forceinline__ f32x4 mlp2_tile1(const float (*ys)[LP], const float4 (&wv)[MLP2_KS], int K, int r, int q) {
  const int ks = (K + 15) >> 4;
  f32x4 c = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < MLP2_KS; ++s) {
    if (s < ks) {
      const float4 a = *reinterpret_cast<const float4*>(&ys[r][16 * s + 4 * q]);
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wv[s].x, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wv[s].y, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wv[s].z, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wv[s].w, c, 0, 0, 0);
    }
  }
  return c;
}

__global__ __launch_bounds__(512) void k_mlp2_tail(Mlp2Batch mb) {
  __shared__ Mlp2Args s_a;
  dr_stage_args(mb.p[blockIdx.z], s_a, threadIdx.x);
  const Mlp2Args& a = s_a;
  const GemmArgs& g = a.e;
  const int M = dr_uni(a.M), K1 = dr_uni(a.K1), K2 = dr_uni(a.K2), N = dr_uni(g.N);
  const int n0 = blockIdx.x * MLP2_NC, m0 = blockIdx.y * 16;
  if (n0 >= N || m0 >= M) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  constexpr int LP = MLP2_KMAX + 8;  // 8 mod 16 dwords: conflict-free ds_read_b128 fragments
  __shared__ __attribute__((aligned(16))) float ys[16][LP];
  __shared__ __attribute__((aligned(16))) float hs[16][LP];
  __shared__ float so[16][MLP2_NC + 1];
  const bool c0 = blockIdx.x == 0;
  const int k = 4 * lane;
  const int ncols = min(MLP2_NC, N - n0);
  // every global operand of this wave is issued before the first use: its two
  // input rows, its (up to) two W3 tiles, its W6 tile
  const float* X = dr_uni(a.X);
  const int ldx = dr_uni((int)a.ldx);
  float4 xr[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wave + 8 * i;
    const bool ok = m < M && k < K1;
    xr[i] = dr_ld4(X, ok ? (unsigned)(m * ldx + k) : 0u);
  }
  const int nt3 = (K2 + 15) >> 4;
  float4 w3[2][MLP2_KS];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = (wave + 8 * i) * 16 + r;
    mlp2_wload(w3[i], a.W3, K1, n, wave + 8 * i < nt3 && n < K2, K1, q);
  }
  const int ntd = (ncols + 15) >> 4;
  float4 w6[MLP2_KS];
  {
    const int nl = wave * 16 + r;
    mlp2_wload(w6, dr_uni(g.W), dr_uni((int)g.ldb), n0 + nl, wave < ntd && nl < ncols, K2, q);
  }

  // A: y1 = SiLU(LN1(X)), two rows per wave
  {
    const int KP = (K1 + 15) & ~15;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rr = wave + 8 * i, m = m0 + rr;
      const bool ok = m < M && k < K1;
      const float4 y = mlp2_ln_silu(xr[i], ok, K1, a.ln1_g, a.ln1_b, k);
      if (k < KP) *reinterpret_cast<float4*>(&ys[rr][k]) = y;
      if (c0 && a.a1_out && ok) dr_st4(a.a1_out, (unsigned)(m * a.ld_a1 + k), y);
    }
  }
  __syncthreads();
  // B: h2 = y1 W3^T + b3 (16-column tiles over the 8 waves)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int tj = wave + 8 * i;
    if (tj < nt3) {
      const int n = tj * 16 + r;
      const f32x4 acc = mlp2_tile<LP>(ys, w3[i], K1, r, q);
      const float bv = (n < K2 && a.b3) ? dr_ld1(a.b3, (unsigned)n) : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ml = 4 * q + e, m = m0 + ml;
        const float v = (n < K2) ? acc[e] + bv : 0.f;
        hs[ml][n] = v;
        if (c0 && a.pre2 && m < M && n < K2) dr_g(a.pre2)[(long long)m * a.ld_pre2 + n] = v;
      }
    }
  }
  __syncthreads();
  // C: y2 = SiLU(LN4(h2)), back into ys
  {
    const int KP = (K2 + 15) & ~15;
    for (int rr = wave; rr < 16; rr += 8) {
      const int m = m0 + rr;
      const bool ok = k < K2;
      float4 x = ok ? *reinterpret_cast<const float4*>(&hs[rr][k]) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 y = mlp2_ln_silu(x, ok, K2, a.ln4_g, a.ln4_b, k);
      if (m >= M) y = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < KP) *reinterpret_cast<float4*>(&ys[rr][k]) = y;
      if (c0 && a.a2_out && ok && m < M) dr_st4(a.a2_out, (unsigned)(m * a.ld_a2 + k), y);
    }
  }
  __syncthreads();
  // D: out = y2 W6^T + b6 for columns [n0, n0 + 128): one 16-column tile per wave
  if (wave < ntd) {
    const int nl = wave * 16 + r, n = n0 + nl;
    const f32x4 acc = mlp2_tile<LP>(ys, w6, K2, r, q);
    const float bv = (nl < ncols && g.bias) ? dr_ld1(g.bias, (unsigned)n) : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) so[4 * q + e][nl] = acc[e] + bv;
  }
  __syncthreads();
  // E: epilogue
  if (g.epi == EPI_SAMPLE) {
    const int C = g.C;
    int W = 1;
    while (W < C) W <<= 1;
    const int gpr = ncols / C, npairs = 16 * gpr, per_wave = 64 / W;
    for (int pbase = wave * per_wave; pbase < npairs; pbase += 8 * per_wave) {
      const int pidx = pbase + lane / W, c = lane % W;
      const bool valid = pidx < npairs;
      const int ml = valid ? pidx / gpr : 0, gl = valid ? pidx - ml * gpr : 0;
      const int m = m0 + ml, grp = (n0 / C) + gl;
      const bool act = valid && c < C && m < M;
      const float x = act ? so[ml][gl * C + c] : -INFINITY;
      if (act && g.Y) dr_g(g.Y)[(long long)m * g.ldy + n0 + gl * C + c] = x;
      const float mx = group_max(x, W);
      const float ex = act ? expf(x - mx) : 0.0f;
      const float se = group_sum(ex, W);
      const float p = ex / se;
      const float pu = act ? (0.99f * p + g.unimix) : 0.0f;
      const float sp = group_sum(pu, W);
      const float ph = pu / sp;
      float qv = 1.0f;
      const int Rg = g.R;
      if (act) {
        if (g.noise.q) qv = dr_g(g.noise.q)[((long long)g.step * M * Rg + (long long)m * Rg + grp) * C + c];
        else qv = dr_exp1(g.noise.rng, (uint32_t)(g.noise.stream + g.step), (uint32_t)(g.noise.row0 + m),
                          (uint32_t)(grp * C + c));
      }
      float best = act ? ph / qv : -INFINITY;
      int bi = act ? c : 0x7fffffff;
      group_argmax(best, bi, W);
      if (act) {
        dr_g(g.z_out)[(long long)m * g.ldz + grp * C + c] = (c == bi) ? ((1.0f + pu) - pu) : 0.0f;
        if (g.soft_out) dr_g(g.soft_out)[(long long)m * g.ld_soft + grp * C + c] = p;
        if (g.idx_out && c == 0) dr_g(g.idx_out)[m * Rg + grp] = bi;
        if (g.zval_out && c == bi) dr_g(g.zval_out)[m * Rg + grp] = (1.0f + pu) - pu;
      }
    }
  } else if (g.epi == EPI_ACTOR) {
    const int A = g.na;
    for (int x = tid; x < 16 * A; x += 512) {
      const int ml = x / A, i = x - ml * A, m = m0 + ml;
      if (m >= M) continue;
      const float muv = so[ml][i];
      const float lr = so[ml][A + i];
      const float ls = fminf(fmaxf(lr, -5.0f), 2.0f);
      const float sg = dr_softplus(ls) + 1e-3f;
      float av;
      if (g.det) {
        av = tanhf(muv);
      } else {
        float e;
        if (g.noise.eps) e = dr_g(g.noise.eps)[((long long)g.step * M + m) * A + i];
        else e = dr_normal(g.noise.rng, (uint32_t)(g.noise.stream + g.step), (uint32_t)(g.noise.row0 + m),
                           (uint32_t)i);
        if (g.eps_save) dr_g(g.eps_save)[(long long)m * A + i] = e;
        av = tanhf(muv + e * sg);
      }
      if (g.act_out) dr_g(g.act_out)[(long long)m * g.ld_act + i] = av;
      if (g.mu_out) dr_g(g.mu_out)[(long long)m * g.ld_mu + i] = muv;
      if (g.sig_out) dr_g(g.sig_out)[(long long)m * g.ld_sig + i] = sg;
      if (g.ls_save) dr_g(g.ls_save)[(long long)m * g.ld_ls + i] = lr;
    }
  } else {
    for (int x = tid; x < 16 * ncols; x += 512) {
      const int ml = x / ncols, nl = x - ml * ncols, m = m0 + ml;
      if (m >= M) continue;
      dr_g(g.Y)[(long long)m * g.ldy + n0 + nl] = epi_act(g, so[ml][nl]);
    }
  }
}

// what k_mlp2_tail takes: both hidden widths staged as float4 rows of at most
// MLP2_KMAX floats, 16-byte aligned operands, a plain, sampler or actor epilogue
bool mlp2_widths_ok(int K1, int K2) {
  return !(K1 < 4 || K2 < 4 || K1 > MLP2_KMAX || K2 > MLP2_KMAX || K1 % 4 || K2 % 4);
}
bool mlp2_ok(const Mlp2Args& a) {
  const GemmArgs& g = a.e;
  const bool al = !(((uintptr_t)a.X | (uintptr_t)a.W3 | (uintptr_t)g.W | (uintptr_t)a.ln1_g | (uintptr_t)a.ln1_b |
                     (uintptr_t)a.ln4_g | (uintptr_t)a.ln4_b) & 15) &&
                  !((uintptr_t)a.a1_out & 15) && !((uintptr_t)a.a2_out & 15);
  return !(a.M < 1 || a.K1 < 4 || a.K2 < 4 || a.K1 > MLP2_KMAX || a.K2 > MLP2_KMAX || a.K1 % 4 || a.K2 % 4 ||
           a.ldx % 4 || g.ldb % 4 || a.ld_a1 % 4 || a.ld_a2 % 4 || g.K != a.K2 || g.N < 1 || !al ||
           (g.epi == EPI_SAMPLE && (g.C < 1 || g.C > 32 || 32 % g.C != 0 || MLP2_NC % g.C != 0)) ||
           (g.epi == EPI_ACTOR && (g.N != 2 * g.na || g.N > 16)) || (g.epi == EPI_NONE && !g.Y) ||
           g.accumulate || g.addend || g.alpha != 1.0f);
}

int mlp2_launch(const Mlp2Args* probs, int count, hipStream_t s) {
  if (count < 1 || count > 3) {
    dr_set_error("mlp2_launch: bad problem count %d", count);
    return DR_E_INVALID;
  }
  Mlp2Batch mb;
  int gx = 1, gy = 1;
  for (int i = 0; i < count; ++i) {
    const Mlp2Args& a = probs[i];
    const GemmArgs& g = a.e;
    if (!mlp2_ok(a)) {
      dr_set_error("mlp2_launch: unsupported problem (M=%d K1=%d K2=%d N=%d epi=%d)", a.M, a.K1, a.K2, g.N, g.epi);
      return DR_E_INVALID;
    }
    mb.p[i] = a;
    gx = std::max(gx, dr_cdiv(g.N, MLP2_NC));
    gy = std::max(gy, dr_cdiv(a.M, 16));
  }
  hipLaunchKernelGGL(k_mlp2_tail, dim3(gx, gy, count), dim3(512), 0, s, mb);
  return dr_check_launch("mlp2_tail");
}

// ---------------------------------------------------------------------------
// k_heads_tail: k_mlp2_tail's layers for 1 to 4 heads over the same rows (the
// reward, continue and critic heads over the imagined states), a workgroup per
// 32 rows and head computing ALL output columns of its rows: the middle layer
// once, each weight fragment loaded once for both 16-row groups, and the
// bucket expectation (k_bucket_value) straight from the logits in the tile.
// Per row and per output element the arithmetic is k_mlp2_tail's (the same
// LayerNorm reduction, the same f32 MFMA chains in the same k order, the same
// bias add) and k_bucket_value's, so neither the tile height nor the column
// blocking changes a bit; with chain1 the products run on one accumulator
// chain instead, the order of the tile GEMM the critics' layers ran on.  Outputs: e.Y (logits or the activated value, may be
// NULL with buckets) and val (symexp of the bucket expectation), both through
// the row map m = b rm_h1 + t -> b (rm_h1 - rm_k0) + t - rm_k0, t >= rm_k0
// (rm_h1 = 0: row m): the [B][H] layouts of the rewards and continues.
// ---------------------------------------------------------------------------
#define HT_RG 2
#define HT_ROWS (16 * HT_RG)
struct HeadTailBatch {
  HeadTail p[DR_HT_HEADS];
};

__device__ __forceinline__ long long ht_row(const HeadTail& h, int m) {
  if (h.rm_h1 <= 0) return m;
  const int b = m / h.rm_h1, t = m - b * h.rm_h1;
  return t < h.rm_k0 ? -1LL : (long long)b * (h.rm_h1 - h.rm_k0) + (t - h.rm_k0);
}

__global__ __launch_bounds__(512) void k_heads_tail(HeadTailBatch hb) {
  __shared__ HeadTail s_h;
  dr_stage_args(hb.p[blockIdx.y], s_h, threadIdx.x);
  const Mlp2Args& a = s_h.a;
  const GemmArgs& g = a.e;
  const int M = dr_uni(a.M), K1 = dr_uni(a.K1), K2 = dr_uni(a.K2), N = dr_uni(g.N);
  const int m0 = blockIdx.x * HT_ROWS;
  if (m0 >= M) return;
  const bool one = dr_uni(s_h.chain1) != 0;  // k_gemm_tile's accumulation order instead of k_mlp2_tail's
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = lane & 15, q = lane >> 4;
  constexpr int LP = MLP2_KMAX + 8;  // 8 mod 16 dwords: conflict-free ds_read_b128 fragments
  constexpr int SP = DR_HT_NMAX + 1;
  constexpr int HSO = HT_ROWS * (LP > SP ? LP : SP);
  __shared__ __attribute__((aligned(16))) float ys[HT_ROWS][LP];
  __shared__ __attribute__((aligned(16))) float hso[HSO];  // h2 rows, then (h2 is dead) the output rows
  float(*hs)[LP] = reinterpret_cast<float(*)[LP]>(hso);
  float(*so)[SP] = reinterpret_cast<float(*)[SP]>(hso);
  const int k = 4 * lane;
  const float* X = dr_uni(a.X);
  const int ldx = dr_uni((int)a.ldx);
  float4 xr[2 * HT_RG];
#pragma unroll
  for (int i = 0; i < 2 * HT_RG; ++i) {
    const int m = m0 + wave + 8 * i;
    const bool ok = m < M && k < K1;
    xr[i] = dr_ld4(X, ok ? (unsigned)(m * ldx + k) : 0u);
  }
  const int nt3 = (K2 + 15) >> 4;
  float4 w3[2][MLP2_KS];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = (wave + 8 * i) * 16 + r;
    mlp2_wload(w3[i], a.W3, K1, n, wave + 8 * i < nt3 && n < K2, K1, q);
  }
  // A: y1 = SiLU(LN1(X)), four rows per wave
  {
    const int KP = (K1 + 15) & ~15;
#pragma unroll
    for (int i = 0; i < 2 * HT_RG; ++i) {
      const int rr = wave + 8 * i, m = m0 + rr;
      const bool ok = m < M && k < K1;
      const float4 y = mlp2_ln_silu(xr[i], ok, K1, a.ln1_g, a.ln1_b, k);
      if (k < KP) *reinterpret_cast<float4*>(&ys[rr][k]) = y;
      if (a.a1_out && ok) dr_st4(a.a1_out, (unsigned)(m * a.ld_a1 + k), y);
    }
  }
  __syncthreads();
  // B: h2 = y1 W3^T + b3 (16-column tiles over the 8 waves, each on both row groups)
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int tj = wave + 8 * i;
    if (tj < nt3) {
      const int n = tj * 16 + r;
      const float bv = (n < K2 && a.b3) ? dr_ld1(a.b3, (unsigned)n) : 0.f;
#pragma unroll
      for (int rg = 0; rg < HT_RG; ++rg) {
        const f32x4 acc = one ? mlp2_tile1<LP>(ys + 16 * rg, w3[i], K1, r, q) : mlp2_tile<LP>(ys + 16 * rg, w3[i], K1, r, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ml = 16 * rg + 4 * q + e, m = m0 + ml;
          const float v = (n < K2) ? acc[e] + bv : 0.f;
          hs[ml][n] = v;
          if (a.pre2 && m < M && n < K2) dr_g(a.pre2)[(long long)m * a.ld_pre2 + n] = v;
        }
      }
    }
  }
  // the last Linear's fragments of this wave's (up to) two 16-column tiles: in flight across the LayerNorm
  const int ntd = (N + 15) >> 4;
  float4 w6[2][MLP2_KS];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int n = (wave + 8 * i) * 16 + r;
    mlp2_wload(w6[i], dr_uni(g.W), dr_uni((int)g.ldb), n, wave + 8 * i < ntd && n < N, K2, q);
  }
  __syncthreads();
  // C: y2 = SiLU(LN4(h2)), back into ys
  {
    const int KP = (K2 + 15) & ~15;
    for (int rr = wave; rr < HT_ROWS; rr += 8) {
      const int m = m0 + rr;
      const bool ok = k < K2;
      float4 x = ok ? *reinterpret_cast<const float4*>(&hs[rr][k]) : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 y = mlp2_ln_silu(x, ok, K2, a.ln4_g, a.ln4_b, k);
      if (m >= M) y = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < KP) *reinterpret_cast<float4*>(&ys[rr][k]) = y;
      if (a.a2_out && ok && m < M) dr_st4(a.a2_out, (unsigned)(m * a.ld_a2 + k), y);
    }
  }
  __syncthreads();
  // D: out = y2 W6^T + b6, every column of the head
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int tj = wave + 8 * i;
    if (tj < ntd) {
      const int n = tj * 16 + r;
      const float bv = (n < N && g.bias) ? dr_ld1(g.bias, (unsigned)n) : 0.f;
#pragma unroll
      for (int rg = 0; rg < HT_RG; ++rg) {
        const f32x4 acc = one ? mlp2_tile1<LP>(ys + 16 * rg, w6[i], K2, r, q) : mlp2_tile<LP>(ys + 16 * rg, w6[i], K2, r, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) so[16 * rg + 4 * q + e][n] = acc[e] + bv;
      }
    }
  }
  __syncthreads();
  // E: the stores
  if (g.Y) {
    for (int x = tid; x < HT_ROWS * N; x += 512) {
      const int ml = x / N, nl = x - ml * N, m = m0 + ml;
      if (m >= M) continue;
      const long long o = ht_row(s_h, m);
      if (o >= 0) dr_g(g.Y)[o * g.ldy + nl] = epi_act(g, so[ml][nl]);
    }
  }
  if (s_h.buckets) {  // k_bucket_value on the row in LDS, one wave per row
    const float* bk = dr_uni(s_h.buckets);
    for (int rr = wave; rr < HT_ROWS; rr += 8) {
      const int m = m0 + rr;
      if (m >= M) break;
      const float* l = so[rr];
      float mx = -INFINITY;
      for (int c = lane; c < N; c += 64) mx = fmaxf(mx, l[c]);
      mx = wave_max(mx);
      float se = 0.f;
      for (int c = lane; c < N; c += 64) se += expf(l[c] - mx);
      se = wave_sum(se);
      float acc = 0.f;
      for (int c = lane; c < N; c += 64) acc += (expf(l[c] - mx) / se) * dr_g(bk)[c];
      acc = wave_sum(acc);
      const long long o = ht_row(s_h, m);
      if (lane == 0 && o >= 0) dr_g(s_h.val)[o] = dr_symexp(acc);
    }
  }
}

bool heads_tail_ok(const HeadTail& h) {
  const Mlp2Args& a = h.a;
  const GemmArgs& g = a.e;
  const bool al = !(((uintptr_t)a.X | (uintptr_t)a.W3 | (uintptr_t)g.W | (uintptr_t)a.ln1_g | (uintptr_t)a.ln1_b |
                     (uintptr_t)a.ln4_g | (uintptr_t)a.ln4_b | (uintptr_t)a.a1_out | (uintptr_t)a.a2_out) & 15);
  return al && mlp2_widths_ok(a.K1, a.K2) && a.M >= 1 && a.X && a.W3 && g.W && a.ln1_g && a.ln1_b && a.ln4_g &&
         a.ln4_b && a.ldx % 4 == 0 && a.ldx >= a.K1 && (long long)a.M * a.ldx < (1LL << 31) && g.ldb % 4 == 0 &&
         g.ldb >= a.K2 && a.ld_a1 % 4 == 0 && a.ld_a2 % 4 == 0 && (long long)a.M * a.ld_a1 < (1LL << 31) &&
         (long long)a.M * a.ld_a2 < (1LL << 31) && g.K == a.K2 && g.N >= 1 && g.N <= DR_HT_NMAX &&
         g.epi == EPI_NONE && !g.accumulate && !g.addend && g.alpha == 1.0f && (g.Y || h.buckets) &&
         (!h.buckets || h.val) && h.rm_h1 >= 0 && h.rm_k0 >= 0 && (h.rm_h1 == 0 || h.rm_k0 < h.rm_h1);
}

int heads_tail_launch(const HeadTail* heads, int count, hipStream_t s) {
  if (count < 1 || count > DR_HT_HEADS) {
    dr_set_error("heads_tail_launch: bad head count %d", count);
    return DR_E_INVALID;
  }
  HeadTailBatch hb;
  int M = 0;
  for (int i = 0; i < count; ++i) {
    if (!heads_tail_ok(heads[i])) {
      const Mlp2Args& a = heads[i].a;
      dr_set_error("heads_tail_launch: unsupported head %d (M=%d K1=%d K2=%d N=%d)", i, a.M, a.K1, a.K2, a.e.N);
      return DR_E_INVALID;
    }
    hb.p[i] = heads[i];
    M = std::max(M, heads[i].a.M);
  }
  hipLaunchKernelGGL(k_heads_tail, dim3(dr_cdiv(M, HT_ROWS), count), dim3(512), 0, s, hb);
  return dr_check_launch("heads_tail");
}


// SiLU(LayerNorm(x)) of whole rows, one wave per row: the staged prologue of
// k_gemm_skinny (same lane -> k mapping and summation order, so the same
// values) as its own pass for tall products, whose consumers then run a plain
// tile GEMM on the result instead of re-normalising the rows per column tile
template <int LNV>
__global__ __launch_bounds__(256) void k_ln_silu_rows(int M, int K, const float* __restrict__ X, int ldx,
                                                      const float* __restrict__ gam, const float* __restrict__ bet,
                                                      float* __restrict__ Y, int ldy) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + wave;
  if (m >= M) return;  // whole waves: wave_sum stays within a live wave
  const int K4 = K >> 2;
  float4 xv[LNV], gv[LNV], bv[LNV];
#pragma unroll
  for (int i = 0; i < LNV; ++i) {
    const int k4 = lane + 64 * i;
    const bool ok = k4 < K4;
    xv[i] = ok ? *reinterpret_cast<const float4*>(X + (long long)m * ldx + 4 * k4) : make_float4(0.f, 0.f, 0.f, 0.f);
    gv[i] = ok ? *reinterpret_cast<const float4*>(gam + 4 * k4) : make_float4(0.f, 0.f, 0.f, 0.f);
    bv[i] = ok ? *reinterpret_cast<const float4*>(bet + 4 * k4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float sm = 0.f;
#pragma unroll
  for (int i = 0; i < LNV; ++i) sm += (xv[i].x + xv[i].y) + (xv[i].z + xv[i].w);
  const float mean = wave_sum(sm) / (float)K;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < LNV; ++i) {
    if (lane + 64 * i < K4) {
      const float dx = xv[i].x - mean, dy = xv[i].y - mean, dz = xv[i].z - mean, dw = xv[i].w - mean;
      sq += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)K + 1e-5f);
#pragma unroll
  for (int i = 0; i < LNV; ++i) {
    const int k4 = lane + 64 * i;
    if (k4 < K4) {
      float4 y;
      y.x = dr_silu_fast((xv[i].x - mean) * rstd * gv[i].x + bv[i].x);
      y.y = dr_silu_fast((xv[i].y - mean) * rstd * gv[i].y + bv[i].y);
      y.z = dr_silu_fast((xv[i].z - mean) * rstd * gv[i].z + bv[i].z);
      y.w = dr_silu_fast((xv[i].w - mean) * rstd * gv[i].w + bv[i].w);
      *reinterpret_cast<float4*>(Y + (long long)m * ldy + 4 * k4) = y;
    }
  }
}

// ---- Host side.  gemm_plan decides the route of a batch; gemm_launch validates
// the arguments, plans, and runs the plan's steps (one switch per family).
static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the problems a route covers, in batch order
struct PlanProbs {
  const GemmArgs* p[4];
  int mask = 0, n = 0;
  void add(const GemmArgs* g, int i) { p[n++] = g; mask |= 1 << i; }
  const GemmArgs& operator[](int i) const { return *p[i]; }
};
static void plan_fail(GemmPlan& pl, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(pl.err, sizeof(pl.err), fmt, ap);
  va_end(ap);
  pl.rc = DR_E_INVALID;
}
static GemmStep& plan_step(GemmPlan& pl, int family, int mask, int gx, int gy, int gz, int block) {
  GemmStep& st = pl.step[pl.nsteps++] = GemmStep{};
  st.family = family; st.mask = mask; st.gx = gx; st.gy = gy; st.gz = gz; st.block = block;
  return st;
}
// 16-byte rows of k runs of kq floats: A (with its second segment) and / or W
static bool rows_aligned(const GemmArgs& g, int kq, bool a, bool w) {
  if (a && (g.K % kq != 0 || g.lda % 4 != 0 || !aligned16(g.A))) return false;
  if (a && g.ksplitA < g.K && (g.ksplitA % kq != 0 || g.lda2 % 4 != 0 || !aligned16(g.A2))) return false;
  return !w || (g.ldb % 4 == 0 && aligned16(g.W));
}
// tiles of the largest problem (a blockIdx.z slice) and of all (a packed grid); every problem with split-K
// scratch; the batch's most rows and shallowest K
struct TileCount { int maxt, tot; bool ws; int maxM, minK; };
static TileCount tile_count(const PlanProbs& q, int bm, int bn) {
  TileCount c = {0, 0, true, 0, 1 << 30};
  for (int i = 0; i < q.n; ++i) {
    const int t = dr_cdiv(q[i].M, bm) * dr_cdiv(q[i].N, bn);
    c.maxt = std::max(c.maxt, t);
    c.tot += t;
    c.ws = c.ws && q[i].splitk_ws != nullptr;
    c.maxM = std::max(c.maxM, q[i].M);
    c.minK = std::min(c.minK, q[i].K);
  }
  return c;
}
// split-K of the tile kernels, every problem with scratch: about two workgroups
// per CU over the problems' real tiles (the grid's surplus blocks of the
// smaller problems exit at once)
static int splitk_count(const PlanProbs& q, int tot, int kc) {
  int nch = 1 << 30;
  for (int i = 0; i < q.n; ++i) nch = std::min(nch, dr_cdiv(q[i].K, kc));
  int splits = std::max(1, std::min(DR_TILE_SPLITS, dr_cdiv(512, tot)));
  splits = std::min(splits, std::max(1, nch / 2));  // at least 2 chunks per split
  for (int i = 0; i < q.n; ++i)
    while (splits > 1 && (long long)splits * q[i].M * q[i].N > q[i].splitk_floats) --splits;
  return splits;
}

// the skinny kernel addresses A, A2, W and a_out with 32-bit element offsets
static bool skinny_offsets_ok(const GemmArgs& g, bool b_kn) {
  const long long lim = 1LL << 30;
  return (long long)g.M * g.lda < lim && (long long)g.M * g.lda2 < lim && (long long)(b_kn ? g.K : g.N) * g.ldb < lim &&
         !(g.W2 && (long long)(g.K + g.N) * g.ldb2 >= lim) && !(g.a_out && (long long)g.M * g.ld_aout >= lim);
}

// Rows of a skinny tile: 16 up to 64 rows, else 64 -- and
// 16-row tiles past 64 rows while the grid stays within ~2.5 dispatch
// rounds: a B = 256 per-step product (N = 200) then spreads over 208
// workgroups instead of 52 (K = 1624: 19.3 -> 8.4 us, profiles/r02_kbench_B256.txt)
// (also the staged LayerNorm- and softmax-STE-backward prologues:
// at 64-row tiles a B = 256 LN-backward product ran on 52 workgroups, 16.5 us)
static int skinny_tile_rows(const PlanProbs& q, int amode, int maxM, bool sample) {
  if (maxM <= 64) return 16;
  if (amode != AM_PLAIN && amode != AM_LNSILU && amode != AM_LNBWD && amode != AM_STEBWD) return 64;
  return tile_count(q, 16, sample ? 32 : 16).tot <= 640 ? 16 : 64;
}

// k_gemm_skinny; false where the batch does not take it
static bool plan_skinny(GemmPlan& pl, const PlanProbs& q, int amode, bool b_kn) {
  int maxM = 0, epi = EPI_NONE;
  bool vec = true;
  for (int i = 0; i < q.n; ++i) {
    const GemmArgs& g = q[i];
    if (g.out_conv) return false;
    if ((g.epi == EPI_SAMPLE) != (q[0].epi == EPI_SAMPLE)) return false;  // 32-column tiles for all or none
    if (g.epi != EPI_NONE) epi = g.epi;
    maxM = g.M > maxM ? g.M : maxM;
    if (!skinny_offsets_ok(g, b_kn)) return false;
    vec = vec && rows_aligned(g, 4, true, !b_kn);
  }
  // fused row epilogues are validated for M <= 4096 (gemm_plan); plain
  // epilogues take any M the 32-bit offsets allow (64-row tiles past 64 rows)
  if (maxM > (epi == EPI_NONE ? (1 << 20) : 4096)) return false;
  const int mt = skinny_tile_rows(q, amode, maxM, epi == EPI_SAMPLE);
  // 16-column tiles by default; 32-column tiles when the 16-column grid would
  // exceed one workgroup per CU (these 512-thread tiles hold 1 per CU by VGPRs,
  // so a second dispatch round costs more than the wider tile's extra MFMAs)
  bool wide = mt == 16 && tile_count(q, 16, 16).tot > 256;
  // The staged LayerNorm-backward tile holds one workgroup per CU, so its grid
  // is never left between one and two dispatch rounds: where the 32-column
  // grid has more than 256 and fewer than 512 tiles (a full round plus a tail
  // that costs a whole second one) and 48 columns bring it to at most 256,
  // the tile is 16 x 48.  B = 256, N = 600 (the BPTT's hidden-state gradient
  // with the GRU backward in its epilogue): 304 tiles -> 208.  The tile stages
  // K <= 256 (sk_stage_vecs); a shape it cannot stage keeps 32 columns.
  bool wide48 = false;
  if (amode == AM_LNBWD && epi == EPI_NONE && wide && vec) {
    const int t32 = tile_count(q, 16, 32).tot;
    wide48 = t32 > 256 && t32 < 512 && tile_count(q, 16, 48).tot <= 256;
    for (int i = 0; i < q.n; ++i) wide48 = wide48 && sk_staged(amode, 16, 48, q[i].K, vec, b_kn);
  }
  // the backward prologues exist only on the staged path (A and weight rows of
  // the tile in LDS, sk_staged): a tile whose rows do not fit
  // would read the raw operand.  At K = 1024 (the STE backward of a 32 x 32
  // latent) the 32-column tile does not fit (48 x 1032 floats), so a B = 512
  // grid (416 16-column tiles) stays on 16 columns
  const bool bwd = amode == AM_LNBWD || amode == AM_STEBWD;
  if (bwd && wide && !wide48 && epi != EPI_SAMPLE)
    for (int i = 0; i < q.n; ++i) wide = wide && sk_staged(amode, 16, 32, q[i].K, vec, b_kn);
  const int nt = epi == EPI_SAMPLE ? 32 : (epi == EPI_ACTOR || mt == 64) ? 16 : wide48 ? 48 : wide ? 32 : 16;
  int lds = 0;
  for (int i = 0; i < q.n; ++i) {
    if (bwd && !sk_staged(amode, mt, nt, q[i].K, vec, b_kn)) return false;
    lds = std::max(lds, sk_lds_floats(amode, mt, nt, q[i].K, vec, b_kn));
  }
  const TileCount tc = tile_count(q, mt, nt);
  if (tc.maxt == 0) return true;
  const int npack = q.n > 1 ? q.n : 0;
  GemmStep& st =
      plan_step(pl, GF_SKINNY, q.mask, dr_xcd_grid(npack ? tc.tot : tc.maxt), 1, npack ? 1 : q.n, 64 * DR_SKW);
  st.bm = mt; st.bn = nt; st.amode = amode; st.b_kn = b_kn; st.vec = vec; st.epi = epi; st.npack = npack;
  st.lds = lds * (int)sizeof(float);
  return true;
}

// mid-size GEMMs: LDS double-buffered tile kernel (k_gemm_tile, or bf16 mode's
// k_gemm_tile_b16: kc = 64, no packed grid, split-K under 256 tiles only),
// split-K when the tile grid is too small to fill the chip and every problem
// brought scratch for it (partials + k_splitk_finish)
static void plan_tile(GemmPlan& pl, const PlanProbs& q, int family, int bm, int bn, int kc, int nw, bool a_km,
                      bool b_kn, bool no_ws) {
  const TileCount tc = tile_count(q, bm, bn);
  if (tc.maxt == 0) return;
  const bool b16 = family == GF_TILE_B16;
  long long maxMN = 0;
  bool vec = true;
  for (int i = 0; i < q.n; ++i) {
    maxMN = std::max(maxMN, (long long)q[i].M * q[i].N);
    vec = vec && rows_aligned(q[i], 4, !a_km, !b_kn);
  }
  const int splits = (!no_ws && tc.ws && (!b16 || tc.tot < 256)) ? splitk_count(q, tc.tot, kc) : 1;
  const int npack = (!b16 && q.n > 1) ? q.n : 0;
  GemmStep& st = plan_step(pl, family, q.mask, dr_xcd_grid(npack ? tc.tot : tc.maxt), splits, npack ? 1 : q.n, 64 * nw);
  st.bm = bm; st.bn = bn; st.kc = kc; st.nw = nw; st.a_km = a_km; st.b_kn = b_kn; st.vec = b16 || vec; st.bf16 = b16;
  st.splits = splits; st.npack = npack; st.no_ws = no_ws;
  if (splits > 1) plan_step(pl, GF_SPLITK_FINISH, q.mask, (int)((maxMN + 255) / 256), 1, q.n, 256).splits = splits;
}

// wave-K chain kernel: 8-wide k runs on 16-byte boundaries in every operand
// (ksplitA on an 8 boundary); b16: k_gemm_tile_b16's test, every problem bf16 as well
static bool chain_ok(const PlanProbs& q, bool b16) {
  for (int i = 0; i < q.n; ++i) {
    const GemmArgs& g = q[i];
    if (!rows_aligned(g, 8, true, true) || g.W2 || g.epi != EPI_NONE || g.out_conv) return false;
    if (b16 ? !g.bf16 : (g.K < 8 || g.M < 1 || g.N < 1)) return false;
  }
  return true;
}
static bool b16_ok(const PlanProbs& q) { return chain_ok(q, true); }

// every problem with pre-split weight planes and the wave-K shape (NT, no second
// A segment or B segment, K % 8 == 0, 16-byte aligned rows, 32-bit offsets)
static bool wks3_ok(const PlanProbs& q) {
  for (int i = 0; i < q.n; ++i) {
    const GemmArgs& g = q[i];
    if (!g.wsplit || g.wsplit_np < ((g.N + 31) & ~31) || g.K < 8 || !rows_aligned(g, 8, true, false) ||
        ((uintptr_t)g.wsplit & 15) || g.ksplitA < g.K || g.W2 || g.epi != EPI_NONE || g.out_conv || g.M < 1 || g.N < 1 ||
        (long long)g.M * g.lda >= (1LL << 30) || (long long)((g.K + 31) / 32) * 3 * g.wsplit_np * 32 >= (1LL << 30))
      return false;
  }
  return true;
}
// 4 waves per 32 x 32 (bf16: 16 x 32) tile, each over its own run of
// k-chunks through a register ring (r04g: 8 waves, whole-wave prefetch and A
// planes measured slower, profiles/r04g_ab_wks3.txt, r04t_ab_aplanes.txt)
// (r06o / r06p: the K loop fully unrolled -- the rolled loop's back edge makes
// the compiler wait for every outstanding load at each chunk, so the ring never
// overlaps loads with MFMAs; unrolled, the waits are per slot -- bitwise the
// same epoch, and no faster: B = 256 fp32 596 -> 596 k, bf16 909 -> 900 k (864 k
// unrolled for short K too), B = 128 fp32 446 -> 454 k; not kept,
// profiles/r06p_ab_wks3_unroll.txt.  The per-wave latency chain is not what
// bounds these launches.)
// (r05w: 64-row tiles, each weight plane read by half as many row tiles,
// measured slower -- 548 k vs 566 k fp32, 776 k vs 803 k bf16 at B = 256)
// register-ring depth (K chunks in flight per wave).  1: the fp32 kernel at 83
// VGPRs (4 waves per SIMD) instead of 140 (3), bf16 48 instead of 86 (7 / 4):
// fp32 headline 581 -> 592 k, bf16 818 -> 828 k; depth 3 / 4 slower still
// than 2 (profiles/r05zf_ab_wks3_depth.txt)
#define DR_WKS3_D 1
// 16-row fragments per tile: 2 (32 x 32 tiles) for the fp32 products, 1 for
// bf16 mode's (16 x 32 tiles: 828 -> 838 k bf16 headline; fp32 595 -> 587 k,
// kept at 2; 8 or 2 waves per tile: +0.2 % / -6 %, profiles/r05zh_ab_wks3_shape.txt)
// (64-column tiles, half the A re-reads: fp32 32 x 64 596 -> 567 k, 16 x 64
// 567 k, bf16 16 x 64 917 -> 899 k; not kept, profiles/r06w_ab_wks3_columns.txt)
#define DR_WKS3_NW 4  // waves per tile (each a 1/NW share of K)
#define DR_WKS3_FM 2
#define DR_WKS3_FM_B16 1
// (GF_WK: the wave-K chain kernel on 32 x 32 tiles, 4 waves, ring depth 2, no split-K)
static void plan_wave(GemmPlan& pl, const PlanProbs& q, int family, bool bf16, bool no_ws) {
  const int fm = family == GF_WK ? 2 : bf16 ? DR_WKS3_FM_B16 : DR_WKS3_FM, nw = family == GF_WK ? 4 : DR_WKS3_NW;
  const TileCount tc = tile_count(q, 16 * fm, 32);
  if (tc.maxt == 0) return;
  const int npack = q.n > 1 ? q.n : 0;
  // bf16 A copies from the producers where every problem of the batch has one
  // (bitwise the same epoch; bf16 headline B = 256 891 -> 909 k, profiles/r06n_ab_a16_convT_cls.txt)
  bool a16 = family == GF_WKS3 && bf16;
  for (int i = 0; i < q.n && a16; ++i) a16 = q[i].A16 && ((uintptr_t)q[i].A16 & 15) == 0 && q[i].lda % 8 == 0;
  GemmStep& st = plan_step(pl, family, q.mask, dr_xcd_grid(npack ? tc.tot : tc.maxt), 1, 1, 64 * nw);
  st.bm = 16 * fm; st.bn = 32; st.nw = nw; st.vec = 1; st.bf16 = family == GF_WKS3 && bf16; st.a16 = a16;
  st.splits = 1; st.npack = npack; st.no_ws = no_ws;
}

static bool tile_offsets_ok(const PlanProbs& q) {
  const long long lim = 1LL << 30;
  for (int i = 0; i < q.n; ++i) {
    const GemmArgs& g = q[i];
    const long long arows = std::max((long long)g.M, (long long)g.K), brows = std::max((long long)g.N, (long long)g.K);
    if (arows * g.lda >= lim || arows * g.lda2 >= lim || brows * g.ldb >= lim) return false;
    if (g.epi != EPI_NONE || g.out_conv) return false;
  }
  return true;
}

// tall NT products (>= 1024 rows) whose caller split the weights into planes,
// f32 mode: the split3 tall GEMM of conv_split.hip (k_gemm_split3) with the
// data-gradient epilogue (accumulate, split output).  The world-model
// backward's K = 200 input gradients ran on the f32 tile kernel at ~21 TF/s.
int op_gemm_nt_split3_ex(int M, int N, int K, const float* A, int lda, const float* A2, int lda2, int ksA,
                         const void* wr, const float* bias, int act, float* Y, int ldy, int accumulate, float* Y2,
                         int ldy2, int nsplitY, float* part, size_t part_floats, hipStream_t s, int splits_fixed);
static bool s3_tall_ok(const GemmArgs& g) {
  const bool seg = g.ksplitA < g.K;  // second A segment (A2 at k >= ksplitA)
  return g.wsplit && !g.bf16 && g.M >= 1024 && g.epi == EPI_NONE && !g.out_conv && !g.W2 && !g.addend &&
         g.alpha == 1.0f && (g.act == 0 || g.act == 1) &&
         (!seg || (g.A2 && aligned16(g.A2) && g.ksplitA % 4 == 0 && g.lda2 % 4 == 0 &&
                   (long long)g.M * g.lda2 < (1LL << 31))) &&
         g.wsplit_np == (g.N + 127) / 128 * 128 &&
         g.N % 4 == 0 && g.K % 4 == 0 && g.lda % 4 == 0 && g.ldy % 4 == 0 && aligned16(g.A) && aligned16(g.Y) &&
         (!g.bias || aligned16(g.bias)) && (g.nsplitY >= g.N || (g.Y2 && aligned16(g.Y2) && g.ldy2 % 4 == 0 &&
                                                                  g.nsplitY % 4 == 0)) &&
         (long long)g.M * g.lda < (1LL << 31) && g.lda < INT_MAX && g.ldy < INT_MAX && g.ldy2 < INT_MAX;
}

// The route of validated problems sharing (amode, layout), in this order.
// bf16 mode's chain products without weight planes on k_gemm_tile_b16 (the
// f32 wave-K kernel measured 723.3 k against 730.5 k bf16 headline,
// profiles/r03zf_ab_bf16_chain_route.txt)
static void plan_route(GemmPlan& pl, int amode, bool a_km, bool b_kn, PlanProbs q) {
  const bool nt = !a_km && !b_kn;
  if (amode == AM_PLAIN && nt) {
    // problems of the batch that qualify run one after another on the split3
    // tall GEMM, the rest as a (smaller) batch below
    // (the 200-wide, K <= 1024 problems on the wave-K split3 kernel's 32 x 32
    // tiles instead -- it fills the chip where 64 x 64 tiles leave ~450 waves
    // -- measured the same WM step, r06t: not kept)
    PlanProbs rest;
    for (int i = 0; i < q.n; ++i) {  // (q is the whole batch here: bit i = problem i)
      if (s3_tall_ok(q[i])) plan_step(pl, GF_S3_TALL, 1 << i, 0, 0, 0, 0);
      else rest.add(q.p[i], i);
    }
    if (rest.n == 0) return;
    q = rest;
  }
  if (amode == AM_PLAIN && tile_offsets_ok(q)) {
    const TileCount t64 = tile_count(q, 64, 64);
    const int maxM = t64.maxM, minK = t64.minK;
    // per-step products at 128-512 rows with a deep K (BPTT input gradients,
    // K = 1800; the heads' first layers, K = 1624) or a wide N (the GRU's
    // hidden product): 32 x 32 tiles, K chunks of 64, split-K only while the
    // tile grid is under one workgroup per CU.  Against the 16/64-row skinny
    // tiles, which re-read the weights per row tile and the activations per
    // 16 columns: 44 -> 32 us (BPTT, 2 problems), 23 -> 15 us (heads, 3
    // problems, split-K 4), profiles/r02h_kbench_tile_B256.txt
    // shallow-K products the caller gave weight planes (the BPTT's actor
    // input gradient, K = 200, N = 1624): the wave-K split3 kernel
    const bool step_rows = nt && maxM >= 128 && maxM <= 512;
    if (step_rows && minK < 512 && wks3_ok(q)) return plan_wave(pl, q, GF_WKS3, b16_ok(q), false);
    if (step_rows) {
      const int tiles32 = tile_count(q, 32, 32).tot;
      // (f32 under ~112 tiles -- one per-step Linear of 200 outputs, K = 1624 --
      // the 16-row skinny tiles spread wider: 8.4 against 13.0 us)
      if ((minK >= 1024 && (tiles32 >= 112 || b16_ok(q))) || (minK >= 512 && tiles32 >= 256)) {
        const bool no_ws = tiles32 >= 256;
        // f32: the wave-K kernel (32 x 32 tiles, 4 waves, no split-K: heads
        // 15.8 -> 13.0 us, BPTT 32.2 -> 25.7, GRU hidden product 13.3 -> 12.3,
        // profiles/r03g_kbench_wk.txt); the LDS tile kernel stays for the
        // shapes the wave-K kernel does not take
        if (wks3_ok(q)) plan_wave(pl, q, GF_WKS3, b16_ok(q), no_ws);
        else if (b16_ok(q)) plan_tile(pl, q, GF_TILE_B16, 32, 32, 64, 4, false, false, no_ws);
        else if (chain_ok(q, false)) plan_wave(pl, q, GF_WK, false, no_ws);
        else plan_tile(pl, q, GF_TILE, 32, 32, 64, 4, false, false, no_ws);
        return;
      }
    }
    // weight gradients (TN) and tall, deep products go to the tile kernel --
    // when it can fill the chip: a per-step product at B = 256 (16 tiles of
    // 64 x 64, no split-K scratch) runs on 52+ skinny 64-row workgroups instead
    // tall products with a small K (M >= 1024: the world-model heads' and
    // decoder's layers over B (T - 1) rows, the critic's over B (H + 1)): the
    // 64-row skinny tiles re-read the weights per row tile and run 16 columns
    // per workgroup (480 us for the decoder's 3584 x 4096 x 200 product)
    const bool tall = nt && maxM >= 1024 && t64.tot >= 256;
    if (a_km || (maxM >= 256 && minK >= 512 && (t64.ws || t64.tot >= 128)) || tall) {
      // tall NT products with a deep K (the encoder feature projection, the
      // critic's first layer over B*(H+1) rows): 8 waves as 4 x 2 over 64 x 64
      // with K chunks of 64 -- 198 -> 171 us (M 8192, K 4096), 51 -> 47 us
      // (M 4096, K 1624), profiles/r02m_kbench_tall_tiles.txt
      if (nt && minK >= 1024 && b16_ok(q)) plan_tile(pl, q, GF_TILE_B16, 64, 64, 64, 8, false, false, false);
      else if (nt && minK >= 1024) plan_tile(pl, q, GF_TILE, 64, 64, 64, 8, false, false, false);
      else plan_tile(pl, q, GF_TILE, 64, 64, 32, 4, a_km, b_kn, false);
      return;
    }
  }
  if (amode == AM_LNBWD || amode == AM_STEBWD) {
    if (nt && plan_skinny(pl, q, amode, false)) return;
    plan_fail(pl, amode == AM_LNBWD ? "gemm: LayerNorm-backward prologue needs the staged NT skinny path"
                                    : "gemm: softmax-STE-backward prologue needs the staged NT skinny path");
    return;
  }
  if (!a_km && (amode == AM_PLAIN || amode == AM_LNSILU) && plan_skinny(pl, q, amode, b_kn)) return;
  long long work = 0;
  for (int i = 0; i < q.n; ++i) work += (long long)q[i].M * q[i].N;
  // large problems: 64x64 tiles; small (per-step, M = batch rows): 32x32 tiles
  // so that the launch spreads over more CUs.
  const int bt = work >= 256LL * 1024 ? 64 : 32;
  const TileCount tc = tile_count(q, bt, bt);
  if (tc.maxt == 0) return;
  GemmStep& st = plan_step(pl, GF_LEGACY, q.mask, tc.maxt, 1, q.n, 256);
  st.bm = st.bn = bt; st.amode = amode; st.a_km = a_km; st.b_kn = b_kn;
}

// the sampler-head kernel's shape: one LN-SiLU NT problem, C = 32, K <= 256
static bool ln_sample_ok(const GemmArgs& g) {
  return g.epi == EPI_SAMPLE && g.C == 32 && g.R * g.C == g.N && g.N % LS_NT == 0 && g.K > 0 && g.K % 4 == 0 &&
         g.K <= LS_KMAX && g.M > 0 && g.M <= 65536 && g.ln_g && g.ln_b && g.ksplitA >= g.K && !g.addend &&
         g.alpha == 1.0f && g.act == 0 && !g.accumulate && !g.W2 && aligned16(g.A) && aligned16(g.W) &&
         aligned16(g.ln_g) && aligned16(g.ln_b) && g.lda % 4 == 0 && g.ldb % 4 == 0 &&
         (!g.a_out || (aligned16(g.a_out) && g.ld_aout % 4 == 0)) && skinny_offsets_ok(g, false) &&
         (long long)g.M * g.ldz < (1LL << 31) && aligned16(g.z_out) && g.ldz % 4 == 0 &&
         (!g.soft_out || (aligned16(g.soft_out) && g.ld_soft % 4 == 0)) && (!g.noise.q || aligned16(g.noise.q));
}

// tall LN-SiLU products (M >= 1024 rows: the world-model heads / decoder over
// B (T - 1) rows, the critic over B (H + 1)) whose transformed rows are saved
// anyway (a_out): normalise once, then the plain GEMM on the saved rows
static bool tall_ln_ok(const GemmArgs* probs, int count) {
  for (int i = 0; i < count; ++i) {
    const GemmArgs& g = probs[i];
    if (g.M < 1024 || g.epi != EPI_NONE || !g.a_out || g.K % 4 || g.K > 1024 || g.K < 4 || g.ksplitA < g.K ||
        g.lda % 4 || g.ld_aout % 4 || ((uintptr_t)g.A | (uintptr_t)g.a_out | (uintptr_t)g.ln_g | (uintptr_t)g.ln_b) & 15 ||
        (long long)g.M * std::max(g.lda, g.ld_aout) >= (1LL << 31))
      return false;
  }
  return true;
}
// a problem as the steps after its k_ln_silu_rows pre-pass see it
static void after_ln_rows(GemmArgs& g) {
  g.A = g.a_out; g.lda = g.ld_aout;
  g.ln_g = g.ln_b = nullptr; g.a_out = nullptr;
}

static void plan_build(GemmPlan& pl, GemmLayout lay, int amode, const GemmArgs* probs, int count) {
  if (count < 1 || count > 4) return plan_fail(pl, "gemm_launch: bad problem count %d", count);
  GemmArgs pp[4];
  if (lay == G_NT && amode == AM_LNSILU && tall_ln_ok(probs, count)) {
    for (int i = 0; i < count; ++i) {
      plan_step(pl, GF_LN_ROWS, 1 << i, (probs[i].M + 3) / 4, 1, 1, 256).kc = probs[i].K <= 256 ? 1 : 4;
      after_ln_rows(pp[i] = probs[i]);
    }
    pl.ln_pre = 1; probs = pp; amode = AM_PLAIN;
  }
  if (lay == G_NT && amode == AM_LNSILU && count == 1 && ln_sample_ok(probs[0])) {
    const GemmArgs& g = probs[0];
    GemmStep& st = plan_step(pl, GF_LN_SAMPLE, 1, dr_xcd_grid(dr_cdiv(g.M, LS_MT) * (g.N / LS_NT)), 1, 1, 256);
    st.bm = LS_MT; st.bn = LS_NT; st.kc = (g.K + 15) >> 4; st.amode = AM_LNSILU; st.vec = 1; st.epi = EPI_SAMPLE;
    st.lds = (int)ln_sample_lds_bytes(g.K);
    return;
  }
  PlanProbs q;
  for (int i = 0; i < count; ++i) {
    const GemmArgs& g = probs[i];
    if (g.epi == EPI_SAMPLE && (g.C < 1 || g.C > 32 || 32 % g.C != 0 || g.N != g.R * g.C))
      return plan_fail(pl, "gemm_launch: sampler epilogue needs C | 32 and N == R*C (C=%d R=%d N=%d)", g.C, g.R, g.N);
    if (g.epi == EPI_ACTOR && (g.N != 2 * g.na || g.na > 8))
      return plan_fail(pl, "gemm_launch: actor epilogue needs N == 2A <= 16");
    if (g.epi != EPI_NONE && (lay != G_NT || (amode != AM_PLAIN && amode != AM_LNSILU) || g.M > 4096 ||
                              !skinny_offsets_ok(g, false)))
      return plan_fail(pl, "gemm_launch: fused epilogues need the NT skinny path");
    q.add(&g, i);
  }
  for (int i = 0; i < count; ++i)
    if (probs[i].M < 0 || probs[i].N < 0 || probs[i].K < 0) return plan_fail(pl, "gemm_launch: negative dims");
  if (lay != G_NT) return plan_route(pl, AM_PLAIN, lay == G_TN, true, q);
  if (amode < AM_PLAIN || amode > AM_STEBWD) return plan_fail(pl, "gemm_launch: bad amode");
  // The staged backward prologues (AM_LNBWD, AM_STEBWD) run on 16-row tiles
  // (K <= 1024) when the problem has at most 64 rows or its 16 x 16 grid stays
  // within ~2.5 dispatch rounds (skinny_tile_rows), else on 64-row tiles (K <= 256).
  // (The 16 x 48 LayerNorm-backward tile plan_skinny picks for a grid between one
  // and two rounds stages K <= 256 as well; wider K keeps 32 columns.)
  const int maxM = tile_count(q, 16, 16).maxM;
  const bool r16 = maxM <= 4096 && skinny_tile_rows(q, amode, maxM, false) == 16;
  const int lim = r16 ? 1024 : 256;  // staged rows per lane: SV = 4 (MT 16) / 1 (MT 64)
  for (int i = 0; i < count && (amode == AM_LNBWD || amode == AM_STEBWD); ++i) {
    const GemmArgs& g = probs[i];
    const bool rows = g.K % 4 == 0 && g.K <= lim && g.lda % 4 == 0 && g.ld_pre % 4 == 0 && g.ldb % 4 == 0 &&
                      (((uintptr_t)g.A | (uintptr_t)g.pre | (uintptr_t)g.W) & 15) == 0;
    const int gl = g.C / 4;
    if (amode == AM_LNBWD && (!rows || (((uintptr_t)g.ln_g | (uintptr_t)g.ln_b) & 15)))
      return plan_fail(pl, "gemm_launch: AM_LNBWD needs K %% 4 == 0, K <= %d, 16-byte aligned rows (K=%d)", lim, g.K);
    if (amode == AM_STEBWD && (!rows || g.C < 4 || g.C % 4 || (gl & (gl - 1)) || gl > 64 || g.K % g.C || !r16))
      return plan_fail(pl, "gemm_launch: AM_STEBWD needs 16-row tiles (gemm_bwd_rows16), K %% C == 0, C/4 a power "
                           "of two, K <= %d, 16-byte aligned rows (K=%d C=%d)", lim, g.K, g.C);
  }
  plan_route(pl, amode, false, false, q);
}
GemmPlan gemm_plan(GemmLayout lay, int amode, const GemmArgs* probs, int count) {
  GemmPlan pl;
  pl.rc = DR_OK; pl.err[0] = 0; pl.ln_pre = 0; pl.nsteps = 0;
  plan_build(pl, lay, amode, probs, count);
  return pl;
}

int gemm_bwd_fusable(const GemmPlan& pl) {
  if (pl.rc != DR_OK || pl.nsteps > 1) return 0;
  return pl.nsteps == 0 ? 16 : pl.step[0].family == GF_SKINNY ? pl.step[0].bm : 0;  // (no tile at all: no launch)
}

// ---- executor: the plan's steps, exactly the kernel instantiations named there
// opt in to more than the default 64 KB of dynamic LDS (once per kernel instantiation)
template <auto KERNEL>
static void lds_opt_in(int bytes) {
  static const bool raised = [bytes] {
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return true;
  }();
  (void)raised;
}
template <int MT, int NT, int AMODE, bool B_KN, int EPI>
static void launch_skinny(const GemmStep& st, const GemmBatch& gb, hipStream_t s) {
  constexpr auto kv = k_gemm_skinny<MT, NT, AMODE, B_KN, true, EPI>;
  constexpr auto ks = k_gemm_skinny<MT, NT, AMODE, B_KN, false, EPI>;
  if (st.lds > 64 * 1024) lds_opt_in<kv>(150 * 1024), lds_opt_in<ks>(150 * 1024);
  hipLaunchKernelGGL((st.vec ? kv : ks), dim3(st.gx, st.gy, st.gz), dim3(st.block), st.lds, s, gb, st.npack);
}
template <int AMODE, bool B_KN>
static void exec_skinny(const GemmStep& st, const GemmBatch& gb, hipStream_t s) {
#define DR_SK(mt, nt, e) launch_skinny<mt, nt, AMODE, B_KN, e>(st, gb, s)
  const bool r64 = st.bm == 64;
  if (st.epi == EPI_SAMPLE) return r64 ? DR_SK(64, 32, EPI_SAMPLE) : DR_SK(16, 32, EPI_SAMPLE);
  if (st.epi == EPI_ACTOR) return r64 ? DR_SK(64, 16, EPI_ACTOR) : DR_SK(16, 16, EPI_ACTOR);
  if (r64) return DR_SK(64, 16, EPI_NONE);
  if constexpr (AMODE == AM_LNBWD)
    if (st.bn == 48) return DR_SK(16, 48, EPI_NONE);
  return st.bn == 32 ? DR_SK(16, 32, EPI_NONE) : DR_SK(16, 16, EPI_NONE);
#undef DR_SK
}

// k_gemm_skinny (the A-modes and layouts plan_route sends there) or the legacy k_gemm of one (amode, layout)
template <int AMODE, bool A_KM, bool B_KN>
static void exec_mode(const GemmStep& st, const GemmBatch& gb, hipStream_t s) {
  if constexpr (!A_KM && AMODE != AM_CONV && AMODE != AM_CONV_SRC)
    if (st.family == GF_SKINNY) return exec_skinny<AMODE, B_KN>(st, gb, s);
  hipLaunchKernelGGL((st.bm == 64 ? k_gemm<64, 64, AMODE, A_KM, B_KN> : k_gemm<32, 32, AMODE, A_KM, B_KN>),
                     dim3(st.gx, st.gy, st.gz), dim3(st.block), 0, s, gb);
}
template <int BM, int BN, int KC, bool A_KM, bool B_KN, int NW = 4>
static void launch_tile2(const GemmStep& st, const GemmBatch& gb, hipStream_t s) {
  constexpr auto kv = k_gemm_tile<BM, BN, KC, A_KM, B_KN, true, NW>;
  constexpr auto ks = k_gemm_tile<BM, BN, KC, A_KM, B_KN, false, NW>;
  hipLaunchKernelGGL((st.vec ? kv : ks), dim3(st.gx, st.gy, st.gz), dim3(st.block), 0, s, gb, st.splits, st.npack);
}
template <int NK>
static void launch_ln_sample_nk(const GemmStep& st, const GemmArgs& g, hipStream_t s) {
  if (st.lds > 64 * 1024) lds_opt_in<k_ln_gemm_sample<NK>>((int)ln_sample_lds_bytes(16 * NK));
  hipLaunchKernelGGL(k_ln_gemm_sample<NK>, dim3(st.gx), dim3(st.block), st.lds, s, g);
}

static int exec_step(const GemmStep& st, const GemmBatch& gb, hipStream_t s) {
  const dim3 grid(st.gx, st.gy, st.gz), blk(st.block);
  const GemmArgs& g = gb.p[0];
  switch (st.family) {
    case GF_LN_ROWS:
      hipLaunchKernelGGL((st.kc == 1 ? k_ln_silu_rows<1> : k_ln_silu_rows<4>), grid, blk, 0, s, g.M, g.K, g.A,
                         (int)g.lda, g.ln_g, g.ln_b, g.a_out, (int)g.ld_aout);
      return dr_check_launch("ln_silu_rows");
    case GF_LN_SAMPLE: {  // ln_sample_ok: 0 < K <= LS_KMAX, so kc = 1 .. 16
#define DR_LS(n) launch_ln_sample_nk<n>, launch_ln_sample_nk<n + 1>, launch_ln_sample_nk<n + 2>, launch_ln_sample_nk<n + 3>
      static void (*const nk[16])(const GemmStep&, const GemmArgs&, hipStream_t) = {DR_LS(1), DR_LS(5), DR_LS(9),
                                                                                    DR_LS(13)};
#undef DR_LS
      nk[st.kc - 1](st, g, s);
      return dr_check_launch("ln_gemm_sample");
    }
    case GF_S3_TALL:
      return op_gemm_nt_split3_ex(g.M, g.N, g.K, g.A, (int)g.lda, g.A2, (int)g.lda2, g.ksplitA < g.K ? g.ksplitA : g.K,
                                  g.wsplit, g.bias, g.act, g.Y, (int)g.ldy, g.accumulate, g.Y2, (int)g.ldy2,
                                  g.nsplitY < g.N ? g.nsplitY : INT_MAX, g.splitk_ws,
                                  g.splitk_ws ? (size_t)g.splitk_floats : 0, s, 0);
    case GF_TILE:
      if (st.bm == 32) launch_tile2<32, 32, 64, false, false, 4>(st, gb, s);
      else if (st.nw == 8) launch_tile2<64, 64, 64, false, false, 8>(st, gb, s);
      else if (st.a_km) launch_tile2<64, 64, 32, true, true>(st, gb, s);
      else if (st.b_kn) launch_tile2<64, 64, 32, false, true>(st, gb, s);
      else launch_tile2<64, 64, 32, false, false>(st, gb, s);
      break;
    case GF_TILE_B16:
      hipLaunchKernelGGL((st.bm == 32 ? k_gemm_tile_b16<32, 32, 4> : k_gemm_tile_b16<64, 64, 8>), grid, blk, 0, s, gb,
                         st.splits);
      break;
    case GF_SPLITK_FINISH: hipLaunchKernelGGL(k_splitk_finish, grid, blk, 0, s, gb, st.splits); break;
    case GF_WK: hipLaunchKernelGGL((k_gemm_wk<32, 32, 4, 2, 1>), grid, blk, 0, s, gb, 1, st.npack); break;
    case GF_WKS3:
      hipLaunchKernelGGL((st.a16    ? k_gemm_wks3<1, DR_WKS3_D, DR_WKS3_NW, DR_WKS3_FM_B16, true>
                          : st.bf16 ? k_gemm_wks3<1, DR_WKS3_D, DR_WKS3_NW, DR_WKS3_FM_B16>
                                    : k_gemm_wks3<3, DR_WKS3_D, DR_WKS3_NW, DR_WKS3_FM>),
                         grid, blk, 0, s, gb, st.npack);
      break;
    case GF_SKINNY:
    case GF_LEGACY:
      switch (st.amode) {
        case AM_LNSILU: exec_mode<AM_LNSILU, false, false>(st, gb, s); break;
        case AM_CONV: exec_mode<AM_CONV, false, false>(st, gb, s); break;
        case AM_CONV_SRC: exec_mode<AM_CONV_SRC, false, false>(st, gb, s); break;
        case AM_LNBWD: exec_mode<AM_LNBWD, false, false>(st, gb, s); break;
        case AM_STEBWD: exec_mode<AM_STEBWD, false, false>(st, gb, s); break;
        default:
          if (st.a_km) exec_mode<AM_PLAIN, true, true>(st, gb, s);
          else if (st.b_kn) exec_mode<AM_PLAIN, false, true>(st, gb, s);
          else exec_mode<AM_PLAIN, false, false>(st, gb, s);
      }
      break;
  }
  return DR_OK;
}

int gemm_launch(GemmLayout lay, int amode, const GemmArgs* probs, int count, hipStream_t s) {
  return gemm_run(gemm_plan(lay, amode, probs, count), probs, count, s);
}
int gemm_run(const GemmPlan& pl, const GemmArgs* probs, int count, hipStream_t s) {
  if (pl.rc != DR_OK) return dr_set_error("%s", pl.err), pl.rc;
  for (int k = 0; k < pl.nsteps; ++k) {
    const GemmStep& st = pl.step[k];
    GemmBatch gb;
    for (int i = 0, n = 0; i < count; ++i) {
      if (!(st.mask >> i & 1)) continue;
      GemmArgs& g = gb.p[n++] = probs[i];  // the one copy of the problem: the kernel's argument
      if (pl.ln_pre && st.family != GF_LN_ROWS) after_ln_rows(g);
      if (st.no_ws) g.splitk_ws = nullptr;
    }
    DR_TRY(exec_step(st, gb, s));
    if (st.family == GF_LN_SAMPLE) return DR_OK;
  }
  return dr_check_launch("gemm");
}

// internal (not in dreamer_hip.h), for the tests: one problem of a batch from the 17 ints tests/test_gemm_plan_host.py
// gives per problem (flags and the misalignment nibbles mis0 / mis1 as that file names them; strides the list leaves
// out follow lda, ldb or ldy).  Both hooks below fill their GemmArgs here, so the batch the planner is asked about on
// the host is the batch that runs; only the pointer source differs: ptr(slot, nibble, on) for the 15 slots A, A2, W,
// Y, ln_g, ln_b, a_out, pre, splitk_ws, wsplit, A16, W2, addend, bias, z_out.  num / xp (NULL = neutral): the fields
// the 17 ints do not carry, in the order of the GX_* / GP_* lists.
enum { GX_ALPHA, GX_ACT, GX_LDY2, GX_NSPLITY, GX_KSPLITB, GX_NSPLITB, GX_LD_ADD, GX_LD_PRE, GX_LD_SV, GX_LD_SOFT, GX_LD_MU,
       GX_LD_SIG, GX_LD_ACT, GX_GB_LDH, GX_GB_LDO, GX_GB_HD, GX_OHOW, GX_UNIMIX, GX_DET, GX_STEP, GX_LDB2, GX_COUNT = 24 };
enum { GP_Y2, GP_SV_GY, GP_SV_XH, GP_SOFT, GP_IDX, GP_ZVAL, GP_Q, GP_EPS, GP_MU, GP_SIG, GP_ACT, GP_GB_H, GP_GB_R, GP_GB_U,
       GP_GB_N, GP_GB_GHN, GP_GB_GI, GP_GB_GH, GP_GB_HO, GP_COUNT = 24 };
template <class PtrSource>
static GemmArgs hook_args(const int* v, PtrSource ptr, const double* num, void* const* xp) {
  const int fl = v[11];
  GemmArgs g = gemm_args();
  g.M = v[0]; g.N = v[1]; g.K = v[2]; g.C = v[8]; g.R = v[9]; g.na = v[10];
  g.bf16 = (fl >> 7) & 1; g.epi = (fl >> 8) & 3; g.out_conv = (fl >> 11) & 1; g.accumulate = (fl >> 13) & 1;
  g.A = ptr(0, 0, true); g.lda = v[3];
  g.A2 = ptr(1, 1, fl & 1); g.lda2 = v[4]; g.ksplitA = v[5];
  g.W = ptr(2, 2, true); g.ldb = v[6];
  g.Y = ptr(3, 3, true); g.ldy = v[7];
  g.ln_g = ptr(4, 4, fl & 2); g.ln_b = ptr(5, 5, fl & 2);
  g.a_out = ptr(6, 6, fl & 4); g.ld_aout = v[16];
  g.pre = ptr(7, 7, fl & 8); g.ld_pre = v[3];
  g.splitk_ws = ptr(8, -1, fl & 16); g.splitk_floats = v[12];
  g.wsplit = (const unsigned short*)ptr(9, 8, fl & 32); g.wsplit_np = v[13];
  g.A16 = (const unsigned short*)ptr(10, 9, fl & 64);
  g.W2 = ptr(11, -1, fl & 1024); g.ldb2 = v[6];
  g.addend = ptr(12, -1, fl & 4096); g.ld_add = v[7];
  g.bias = ptr(13, 10, fl & 16384);
  g.z_out = ptr(14, 11, g.epi == EPI_SAMPLE); g.ldz = v[7];
  if (num) {
    g.alpha = (float)num[GX_ALPHA]; g.act = (int)num[GX_ACT];
    g.ldy2 = (long long)num[GX_LDY2]; g.nsplitY = (int)num[GX_NSPLITY];
    g.ksplitB = (int)num[GX_KSPLITB]; g.nsplitB = (int)num[GX_NSPLITB]; g.ldb2 = (long long)num[GX_LDB2];
    g.ld_add = (long long)num[GX_LD_ADD]; g.ld_pre = (long long)num[GX_LD_PRE]; g.ld_sv = (long long)num[GX_LD_SV];
    g.ld_soft = (long long)num[GX_LD_SOFT]; g.ld_mu = (long long)num[GX_LD_MU]; g.ld_sig = (long long)num[GX_LD_SIG];
    g.ld_act = (long long)num[GX_LD_ACT];
    g.gb.ldh = (long long)num[GX_GB_LDH]; g.gb.ldo = (long long)num[GX_GB_LDO]; g.gb.Hd = (int)num[GX_GB_HD];
    g.oh = (int)num[GX_OHOW]; g.ow = 1;  // the kernels use the product alone
    g.unimix = (float)num[GX_UNIMIX]; g.det = (int)num[GX_DET]; g.step = (int)num[GX_STEP];
  }
  if (xp) {
    auto f = [&](int k) { return (float*)xp[k]; };
    g.Y2 = f(GP_Y2); g.sv_gy = f(GP_SV_GY); g.sv_xh = f(GP_SV_XH);
    g.soft_out = f(GP_SOFT); g.idx_out = (int*)xp[GP_IDX]; g.zval_out = f(GP_ZVAL);
    g.noise.q = f(GP_Q); g.noise.eps = f(GP_EPS);
    g.mu_out = f(GP_MU); g.sig_out = f(GP_SIG); g.act_out = f(GP_ACT);
    g.gb.h = f(GP_GB_H); g.gb.r = f(GP_GB_R); g.gb.u = f(GP_GB_U); g.gb.n = f(GP_GB_N); g.gb.ghn = f(GP_GB_GHN);
    g.gb.gi = f(GP_GB_GI); g.gb.gh = f(GP_GB_GH); g.gb.ho = f(GP_GB_HO);
  }
  return g;
}
// the plan's steps (GemmStep as ints) to out; their count, or -rc and the message in msg
static int hook_steps(const GemmPlan& pl, int* out, int out_steps, char* msg, int msg_cap) {
  if (pl.rc != DR_OK) snprintf(msg, msg_cap, "%s", pl.err);
  static_assert(sizeof(GemmStep) == 21 * sizeof(int), "GemmStep is copied out as 21 ints");
  for (int k = 0; pl.rc == DR_OK && k < pl.nsteps && k < out_steps; ++k)
    memcpy(out + 21 * k, &pl.step[k], sizeof(GemmStep));
  return pl.rc != DR_OK ? -pl.rc : pl.nsteps;
}

// The plan of a batch on dummy pointers (problem and slot in the high word, the misalignment nibble in the low bits):
// pure host code.  Writes the steps to out; returns their count, or -rc and the message in msg.
extern "C" int dr_internal_gemm_plan(int lay, int amode, int count, const int* in, int* out, int out_steps, char* msg,
                                     int msg_cap) {
  GemmArgs pr[4];
  for (int i = 0; i < count && i < 4; ++i) {
    const int* v = in + 17 * i;
    auto ptr = [&](int slot, int nib, bool on) {  // nib: 0-7 of mis0, 8-11 of mis1, -1 aligned
      const int mis = nib < 0 ? 0 : (v[14 + nib / 8] >> (4 * (nib % 8))) & 15;
      return on ? (float*)(((uintptr_t)(16 * i + slot + 1) << 32) + mis) : nullptr;
    };
    pr[i] = hook_args(v, ptr, nullptr, nullptr);
  }
  return hook_steps(gemm_plan((GemmLayout)lay, amode, pr, count), out, out_steps, msg, msg_cap);
}

// Its twin on real device memory: the same 17 ints per problem, ptrs = 15 device pointers per problem in the slot
// order above (the caller has applied the misalignment nibbles; a slot whose flag is off is ignored), num / xp =
// GX_COUNT doubles / GP_COUNT pointers per problem (either may be NULL).  Plans the batch, copies the steps out as
// the plan hook does and runs that plan on `stream`.  Where the flags ask for weight planes or a bf16 copy of A, they
// are made first, as the engine's callers make them (op_nt_repack_split3, op_to_bf16_2d), into the wsplit / A16 slot:
// planes of wsplit_np rows ([K/32][3][wsplit_np][32]; a row count other than the engine's padding goes through
// op_repack_multi, the same element code), A16 as M rows of lda.  Returns the step count, or -rc and the message;
// nothing is launched for a batch the planner refuses.
extern "C" int dr_internal_gemm_run(int lay, int amode, int count, const int* in, void* const* ptrs, const double* num,
                                    void* const* xp, void* stream, int* out, int out_steps, char* msg, int msg_cap) {
  hipStream_t s = (hipStream_t)stream;
  GemmArgs pr[4];
  for (int i = 0; i < count && i < 4; ++i) {
    auto ptr = [&](int slot, int, bool on) { return on ? (float*)ptrs[15 * i + slot] : nullptr; };
    pr[i] = hook_args(in + 17 * i, ptr, num ? num + GX_COUNT * i : nullptr, xp ? xp + GP_COUNT * i : nullptr);
  }
  const GemmPlan pl = gemm_plan((GemmLayout)lay, amode, pr, count);
  const int n = hook_steps(pl, out, out_steps, msg, msg_cap);
  if (n < 0) return n;
  int rc = DR_OK;
  for (int i = 0; i < count && rc == DR_OK; ++i) {
    const GemmArgs& g = pr[i];
    if (g.wsplit && g.wsplit_np > 0 && g.N > 0 && g.K > 0) {
      if (g.wsplit_np == (g.N + 127) / 128 * 128) {
        rc = op_nt_repack_split3(g.N, g.K, g.W, (int)g.ldb, (void*)g.wsplit, s);
      } else {
        RepackJob j = rj_nt(g.N, g.K, g.W, (int)g.ldb, (void*)g.wsplit);
        j.c = g.wsplit_np; j.total = (long long)((g.K + 31) / 32) * 32 * g.wsplit_np;
        rc = op_repack_multi(&j, 1, s);
      }
    }
    if (rc == DR_OK && g.A16 && g.M > 0 && g.lda > 0) rc = op_to_bf16_2d(g.M, (int)g.lda, g.A, g.lda, (void*)g.A16, s);
  }
  if (rc == DR_OK) rc = gemm_run(pl, pr, count, s);
  if (rc != DR_OK) return snprintf(msg, msg_cap, "%s", dr_last_error()), -rc;
  return n;
}
