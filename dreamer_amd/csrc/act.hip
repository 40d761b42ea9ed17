// The acting step in ONE launch: the per-env-step device
// work of Dreamer.rollout_policy / evaluate_agent / Run (Dreamer.py:177-226,
// 295-322, 374-401) for n_env = 1 ... DR_ACT_MAX_ENVS environments at once:
//
//   h' = GRU(z, h, a)               WorldModel.observe_step -> SequenceModel   (h' = 0 at an
//                                   episode start, Dreamer.py:186-187, 222)
//   z' = Encoder.encode(h', obs)    encoder + latent_mapper + categorical sampler (VAE.py:57-99)
//   a  = Actor.act(h', z')          Agent.py:202-210
//
// At these batch sizes every stage is a handful of dot products, so the
// unfused path (about 20 launches per env step) is launch- and dependency-
// latency bound.  Here one cooperative grid of ACT_NB workgroups walks the
// stages with a grid barrier between dependent ones; inside a stage a wave
// owns one output row (dense) or one output channel of a 2-row pixel block
// (conv), holds that row's weights in registers (loads issued together: one
// round trip) while the rows of the batch pass through it, reads the stage
// input from LDS and reduces with DPP.  f32 VALU arithmetic (no MFMA: no weight
// fragment has more than 16 rows to serve).
//
// Two kernels share everything but their encoder stages (the skeleton: ActCommon
// and the act_prologue ... act_finish helpers below):
//   k_act_batch<NE>  pixel frames, four conv stages        dr_act_step (one row), dr_act_batch
//   k_act_vec<NE>    vector observations, two dense stages dr_act_vec
// Every output of every row is summed over k = lane + 64 j, j ascending, then
// wave_sum, whatever n_env and NE are, so a row's bits do not depend on the
// batch it travels in.
//
// Barrier: monotonic arrival counters per launch (zeroed by the host before
// the launch); round k is complete when the top counter reaches k * ACT_GROUPS.
// Polling uses agent-scope loads; a bounded spin turns a lost workgroup into
// NaN outputs instead of a hung GPU.
#include "common.h"
#include "ops.h"
#include "engine_util.h"

#include <string.h>

#define ACT_NB 128
#define ACT_NT 256
#define ACT_SPIN_LIMIT (1 << 22)
#define ACT_BAR_BYTES (4 * 32 * 17)  // 8 group counters, the top counter, 8 generations (128 B apart)

// What both kernels take: the model, the rows' previous state and noise, the
// outputs, and the workspace of the shared stages.  Each kernel's argument
// struct embeds it first and adds its observation pointer and encoder scratch.
struct alignas(16) ActCommon {
  dr_dims d;
  dr_world_model wm;
  dr_actor ac;
  const unsigned char* first;  // [n_env] on the device: 1 = episode start (h' = 0); NULL: first_mask
  unsigned first_mask;         // bit e: row e starts an episode (the host's copy, read when first is NULL)
  int n_env, det;
  const float *z_prev, *h, *a_prev;  // [n_env][L], [n_env][hidden], [n_env][A]; a starting row's are not read
  dr_noise noise;
  float *z_out, *h_out, *a_out, *mu_out, *sig_out, *logits_out;
  int* status;  // caller's status word (may be NULL): set to 1 if a grid barrier timed out
  // workspace (gi ... prea: one copy per row)
  unsigned* bar;
  float *gi, *gh, *hn, *pre1, *prea;
  int* fail;
  int spin_limit;  // polls before a grid barrier gives up (ACT_SPIN_LIMIT; 0 under DREAMER_ACT_FORCE=timeout)
  long long* ts;  // workgroup 0's stage timestamps (100 MHz wall clock), for profiling
};

// XCD-hierarchical grid barrier (MI355X_MICROARCH.md "barrier-xcd"): the
// workgroups of group x = blockIdx % 8 (the XCD the dispatcher deals them to;
// placement only affects speed) count on their own line; the last arriver of a
// group carries the group to the top counter and, once all 8 groups arrived,
// publishes the round on the group's generation line, which the other members
// poll.  Arrivals are agent-scope releases, every exit an agent-scope acquire.
// bar: [0..8) group counters, [16] top counter, [32..40) generations (128-B apart).
#define ACT_GROUPS 8
__device__ __forceinline__ bool act_sync(unsigned* bar, unsigned& round, int* s_ok, int spin_limit) {
  __syncthreads();
  if (threadIdx.x == 0) {
    ++round;
    const int x = blockIdx.x % ACT_GROUPS;
    const unsigned per = ACT_NB / ACT_GROUPS;
    unsigned* cnt = bar + 32 * x;
    unsigned* top = bar + 32 * ACT_GROUPS;
    unsigned* gen = bar + 32 * (ACT_GROUPS + 1 + x);
    int ok = 1, spins = 0;
    const unsigned old = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (old + 1 == round * per) {  // group leader
      __hip_atomic_fetch_add(top, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      while (__hip_atomic_load(top, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < round * ACT_GROUPS) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > spin_limit) {
          ok = 0;
          break;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(gen, round, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      while (__hip_atomic_load(gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < round) {
        __builtin_amdgcn_s_sleep(1);
        if (++spins > spin_limit) {
          ok = 0;
          break;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    *s_ok = ok;
  }
  __syncthreads();
  return *s_ok != 0;
}
#define ACT_TS(a, i)                                                        \
  do {                                                                      \
    if (blockIdx.x == 0 && threadIdx.x == 0) (a).ts[i] = wall_clock64();    \
  } while (0)

// Stage helpers.  Work is split into wave tasks over the whole grid (ACT_NB x
// 4 waves); a task issues every global load it needs before its first FMA,
// so it pays one memory round trip, and reads its stage input from LDS (each
// workgroup stages the input map / vector it needs).

// k4 s2 p1 conv + bias + SiLU, for every frame of the batch.  Workgroup b owns
// a block of 2 output rows (pb = b % NPB) and 4 output channels (one per wave):
// it stages the 6 input rows the block reads into an LDS slab (NHWC; rows
// outside the map are zero padding), each wave holds its channel's weight row
// [ci][ky][kx] in registers (k = lane + 64 j: coalesced, all issued before the
// first FMA), then every pixel is one LDS gather + FMA per k and a wave
// reduction.  cout == 4 * ACT_NB / NPB.
// Done with run-time map shapes this costs 10-20 us per frame, nearly all of
// it index arithmetic (about ten VALU instructions per FMA) and one-at-a-time
// reductions, so the map shape is a compile-time constant (IW x IW x CIN;
// act_dims_ok pins it):
//  - the slab has a zero pad column on either side of a row, so no gather
//    needs a bounds test, and k = lane + 64 j moves the address by 4 j floats,
//    so every gather is one LDS read at lane base + immediate and one FMA;
//    the strides spread a pixel's 64 gather addresses over all 32 banks;
//  - the pixel loop is unrolled, which lets the 2 x OW independent reduction
//    chains overlap; lane p keeps pixel p and the SiLU + store happen once;
//  - two slabs: frame e + 1 is fetched into registers before frame e's pixels
//    are computed and written to the other slab after them.
// Each output is sum over k = lane + 64 j (j ascending) then wave_sum.
// FRAME: the input is the u8 HWC frame, normalised x/255 - 0.5 (Dreamer.py:251).
template <int IW, int CIN, bool FRAME>
struct ActSlab {
  // channel stride CS = 4 (mod 32) and row stride SR = 16 (mod 32): the 64 gather addresses of a pixel,
  // ky SR + kx CS + (lane >> 4), then fall on 32 distinct banks, two lanes each
  static constexpr int CS = CIN % 4 == 0 ? CIN + 4 : CIN + 1, RW = IW + 2;
  static constexpr int SR = RW * CS + (48 - (RW * CS) % 32) % 32, SIZE = 6 * SR, STRIDE = SIZE;
  static_assert(CS % 32 == 4 && SR % 32 == 16, "bank spread");
  static constexpr int N4 = 6 * IW * CIN / 4, NV = (N4 + ACT_NT - 1) / ACT_NT;
  float4 v[NV];  // this thread's share of the 6 input rows, 4 consecutive elements each
  // in: the f32 NHWC map, or frame: the u8 HWC frame (x / 255 - 0.5, Dreamer.py:251); rows outside the map are zero
  __device__ __forceinline__ void load(int pb, const float* in, const unsigned char* frame) {
    const int y0 = 4 * pb - 1;
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i4 = threadIdx.x + u * ACT_NT, e = i4 < N4 ? 4 * i4 : 0;
      const int r = e / (IW * CIN), rem = e - r * (IW * CIN), y = y0 + r;
      const bool ok = i4 < N4 && y >= 0 && y < IW;
      const int src = min(max(y, 0), IW - 1) * (IW * CIN) + rem;  // always inside the map: the load is unconditional
      if constexpr (FRAME) {
        const unsigned wd = *reinterpret_cast<const unsigned*>(frame + src);
        const float4 f = make_float4((float)(wd & 255u) / 255.0f - 0.5f, (float)((wd >> 8) & 255u) / 255.0f - 0.5f,
                                     (float)((wd >> 16) & 255u) / 255.0f - 0.5f, (float)(wd >> 24) / 255.0f - 0.5f);
        v[u] = ok ? f : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        const float4 f = *reinterpret_cast<const float4*>(in + src);
        v[u] = ok ? f : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  }
  __device__ __forceinline__ void store(float* xs) const {
#pragma unroll
    for (int u = 0; u < NV; ++u) {
      const int i4 = threadIdx.x + u * ACT_NT;
      if (i4 >= N4) break;
      if constexpr (CIN % 4 == 0) {  // the 4 elements are channels of one pixel, 16-byte aligned in the slab
        const int e = 4 * i4, r = e / (IW * CIN), rem = e - r * (IW * CIN), px = rem / CIN, ch = rem - px * CIN;
        *reinterpret_cast<float4*>(xs + r * SR + (px + 1) * CS + ch) = v[u];
      } else {
        const float c[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = 4 * i4 + q, r = e / (IW * CIN), rem = e - r * (IW * CIN), px = rem / CIN, ch = rem - px * CIN;
          xs[r * SR + (px + 1) * CS + ch] = c[q];
        }
      }
    }
  }
  // the pad columns: cells 0 and IW + 1 of the 6 rows
  static __device__ __forceinline__ void pads(float* xs) {
    for (int i = threadIdx.x; i < 12 * CS; i += ACT_NT) {
      const int r = i / (2 * CS), c = i - r * 2 * CS;
      xs[r * SR + (c < CS ? c : (IW + 1) * CS + c - CS)] = 0.f;
    }
  }
};
// dynamic LDS the batched conv stages need: two slabs of the largest map (conv4's, 8 x 8 x 128)
#define ACT_BATCH_CONV_LDS (2 * ActSlab<8, 128, false>::STRIDE)

template <int KJ, bool NCHW, int IW, int CIN>
__device__ __forceinline__ void act_conv_pixels_t(int cout, int pb, int co, const float (&wv)[KJ], float bias,
                                                  const float* xs, float* out) {
  constexpr int CS = ActSlab<IW, CIN, false>::CS, SR = ActSlab<IW, CIN, false>::SR, OW = IW / 2, K = CIN * 16;
  static_assert(K % 64 == 0 || KJ == 1, "a partial k batch only where it is the only one");
  static_assert(2 * OW <= 64, "one pixel per lane");
  const int lane = threadIdx.x & 63;
  // k = lane + 64 j -> (ci, ky, kx) = ((lane >> 4) + 4 j, (lane >> 2) & 3, lane & 3); lanes past K hold a zero
  // weight and read cell 0 of the pixel's window
  const float* xb = xs + (lane < K ? ((lane >> 2) & 3) * SR + (lane & 3) * CS + (lane >> 4) : 0);
  float mine = 0.f;
#pragma unroll
  for (int pl = 0; pl < 2 * OW; ++pl) {
    const int po = 2 * (pl / OW) * SR + 2 * (pl % OW) * CS;  // (a constant after unrolling)
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < KJ; ++j) acc = fmaf(wv[j], xb[po + 4 * j], acc);
    acc = wave_sum(acc);
    if (lane == pl) mine = acc + bias;
  }
  if (lane < 2 * OW) {
    const int p = (2 * pb + lane / OW) * OW + lane % OW;
    out[NCHW ? co * OW * OW + p : p * cout + co] = mine / (1.0f + expf(-mine));
  }
}

// frame e's input at in + e * in_ld (or frames + e * IW * IW * CIN), its output at out + e * out_ld
template <int KJ, bool FRAME, bool NCHW, int IW, int CIN>
__device__ __forceinline__ void act_conv_rows(int n_env, int cout, const float* in, long long in_ld,
                                              const unsigned char* frames, const float* __restrict__ w,
                                              const float* __restrict__ b, float* out, long long out_ld, float* xs) {
  using Slab = ActSlab<IW, CIN, FRAME>;
  static_assert(2 * Slab::STRIDE <= ACT_BATCH_CONV_LDS, "slab pair");
  constexpr int NPB = IW / 4;
  const int pb = blockIdx.x % NPB, co = (blockIdx.x / NPB) * 4 + (threadIdx.x >> 6);
  float wv[KJ];  // the channel's weight row [ci][ky][kx], k = lane + 64 j
#pragma unroll
  for (int j = 0; j < KJ; ++j) {
    const int k = (threadIdx.x & 63) + 64 * j;
    wv[j] = (k < CIN * 16 && co < cout) ? w[(long long)co * (CIN * 16) + k] : 0.f;
  }
  const float bias = co < cout ? b[co] : 0.f;
  __syncthreads();  // the previous readers of xs are done
  Slab::pads(xs);
  Slab::pads(xs + Slab::STRIDE);
  Slab s;
  s.load(pb, in, frames);
  s.store(xs);
  for (int e = 0; e < n_env; ++e) {
    __syncthreads();  // slab e is whole, and the other slab's readers (frame e - 1) are done
    const bool more = e + 1 < n_env;
    if (more)
      s.load(pb, FRAME ? nullptr : in + (e + 1) * in_ld, FRAME ? frames + (long long)(e + 1) * IW * IW * CIN : nullptr);
    if (co < cout)
      act_conv_pixels_t<KJ, NCHW, IW, CIN>(cout, pb, co, wv, bias, xs + (e & 1) * Slab::STRIDE, out + e * out_ld);
    if (more) s.store(xs + ((e + 1) & 1) * Slab::STRIDE);
  }
}

// y_r[o] = b[o] + W[o][0:K] . x_r for up to NE input rows x_r in LDS (xs + r *
// xld, outputs y + r * yld; bit r of `rows` set = row r is live): one wave task
// per output row, k = lane + 64 j (coalesced row reads, KJ loads in flight per
// batch).  The output row's weights are loaded once and stay in registers
// while every live input row accumulates against them -- per input row the
// same k order and reduction whatever NE is, so the same bits.
template <int KJ, int NE>
__device__ __forceinline__ void act_dense_rows(int nout, int K, const float* __restrict__ W, long long ldw,
                                               const float* __restrict__ b, const float* xs, int xld, float* y,
                                               long long yld, unsigned rows, int gw, int nw) {
  const int lane = threadIdx.x & 63;
  for (int o = gw; o < nout; o += nw) {
    const float* wr = W + (long long)o * ldw;
    float acc[NE];
#pragma unroll
    for (int r = 0; r < NE; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 64 * KJ) {
      float wv[KJ];
#pragma unroll
      for (int j = 0; j < KJ; ++j) {
        const int k = k0 + lane + 64 * j;
        wv[j] = k < K ? wr[k] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < NE; ++r) {
        if (!((rows >> r) & 1u)) continue;
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
          const int k = k0 + lane + 64 * j;
          acc[r] = fmaf(wv[j], k < K ? xs[r * xld + k] : 0.f, acc[r]);
        }
      }
    }
    const float bias = b ? b[o] : 0.f;
#pragma unroll
    for (int r = 0; r < NE; ++r) {
      if (!((rows >> r) & 1u)) continue;
      const float v = wave_sum(acc[r]);
      if (lane == 0) y[r * yld + o] = v + bias;
    }
  }
}

// dst[i] = src(i) for i < n, every load of a thread issued before its first
// LDS store (one memory round trip per U * ACT_NT elements)
template <int U, typename Src>
__device__ __forceinline__ void act_stage(float* dst, int n, Src src) {
  for (int i0 = threadIdx.x; i0 < n; i0 += U * ACT_NT) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * ACT_NT;
      v[u] = i < n ? src(i) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * ACT_NT;
      if (i < n) dst[i] = v[u];
    }
  }
}

// SiLU(LayerNorm(x)) of an n-vector (n <= 256) by one wave, x read once into
// registers (torch LayerNorm, eps 1e-5); result into dst (LDS)
__device__ __forceinline__ void act_ln_silu(const float* x, int n, const float* g, const float* bb, float* dst) {
  const int lane = threadIdx.x & 63;
  float xv[4], gv[4], bv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = lane + 64 * j;
    xv[j] = i < n ? x[i] : 0.f;
    gv[j] = i < n ? g[i] : 0.f;
    bv[j] = i < n ? bb[i] : 0.f;
  }
  const float mean = wave_sum((xv[0] + xv[1]) + (xv[2] + xv[3])) / (float)n;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float dx = lane + 64 * j < n ? xv[j] - mean : 0.f;
    q += dx * dx;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)n + 1e-5f);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int i = lane + 64 * j;
    if (i < n) {
      const float v = (xv[j] - mean) * rstd * gv[j] + bv[j];
      dst[i] = v / (1.0f + expf(-v));
    }
  }
}

// one output per thread (n <= ACT_NT rows, K % 4 == 0): y[t] = b[t] + W[t] . x,
// the thread's weight row loaded KQ float4 at a time (one round trip per
// 4 KQ weights), x broadcast from LDS
template <int KQ>
__device__ __forceinline__ void act_rows(int n, int K, const float* __restrict__ W, const float* __restrict__ b, const float* xs,
                         float* y) {
  const int t = threadIdx.x;
  if (t >= n) return;
  const float4* wr = reinterpret_cast<const float4*>(W + (long long)t * K);
  float acc = 0.f;
  for (int j0 = 0; 4 * j0 < K; j0 += KQ) {
    float4 w4[KQ];
#pragma unroll
    for (int j = 0; j < KQ; ++j) w4[j] = 4 * (j0 + j) < K ? wr[j0 + j] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < KQ; ++j) {
      const int k = min(4 * (j0 + j), K - 4);  // past K: w4 is zero, any in-range x
      acc = fmaf(w4[j].x, xs[k], acc);
      acc = fmaf(w4[j].y, xs[k + 1], acc);
      acc = fmaf(w4[j].z, xs[k + 2], acc);
      acc = fmaf(w4[j].w, xs[k + 3], acc);
    }
  }
  y[t] = acc + b[t];
}

// element j of h' from the GRU pre-activations (torch gru_cell order r, z, n)
__device__ __forceinline__ float act_gru_gates(const float* gi, const float* gh, int Hd, int j, float hv) {
  const float rr = 1.0f / (1.0f + expf(-(gh[j] + gi[j])));
  const float uu = 1.0f / (1.0f + expf(-(gh[Hd + j] + gi[Hd + j])));
  const float nn = tanhf(gi[2 * Hd + j] + gh[2 * Hd + j] * rr);
  return (hv - nn) * uu + nn;
}

// One wave, one latent group of one row: SiLU(LN(pre1)), the group's C
// latent_mapper.3 logits and the categorical sampler.  q: the row's explicit
// Exp(1) variates [R][C] or NULL (Philox keyed by `row`); z_out / logits_out:
// the row's [R][C].  Uses xs[0, 1280).
__device__ __forceinline__ void act_latent_group(const dr_dims& d, const dr_world_model& wm, const float* pre1, int grp,
                                                 const float* q, const unsigned long long* rng, int stream, int row,
                                                 float* z_out, float* logits_out, float* xs) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int C = d.cols;
  float* x1 = xs + wave * 256;
  float* lgs = xs + 1024 + wave * 64;
  act_ln_silu(pre1, d.enc_hidden, wm.map1.w, wm.map1.b, x1);
  // the group's C logits: the weights (k = lane + 64 j) of 16 rows per batch
  float xv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xv[j] = lane + 64 * j < d.enc_hidden ? x1[lane + 64 * j] : 0.f;
  float mylg = 0.f;
  for (int u0 = 0; u0 < C; u0 += 16) {
    float wv[16][4];
#pragma unroll
    for (int u = 0; u < 16; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = lane + 64 * j;
        wv[u][j] = (u0 + u < C && k < d.enc_hidden) ? wm.map3.w[(long long)(grp * C + u0 + u) * d.enc_hidden + k] : 0.f;
      }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc = fmaf(wv[u][j], xv[j], acc);
      acc = wave_sum(acc);
      if (lane == u0 + u) mylg = acc;
    }
  }
  if (lane < C) lgs[lane] = mylg + wm.map3.b[grp * C + lane];
  const bool act = lane < C;
  const float lg = act ? lgs[lane] : -INFINITY;
  if (act && logits_out) logits_out[grp * C + lane] = lg;
  // softmax, 1% unimix, argmax(p_hat / Exp(1)), straight-through one-hot (VAE.py:88-98)
  const float mx = wave_max(lg);
  const float ex = act ? expf(lg - mx) : 0.f;
  const float se = wave_sum(ex);
  const float p = ex / se;
  const float pu = act ? 0.99f * p + (float)(0.01 * (1.0 / C)) : 0.f;
  const float sp = wave_sum(pu);
  const float ph = pu / sp;
  float qv = 1.0f;
  if (act) {
    if (q) qv = q[(long long)grp * C + lane];
    else qv = dr_exp1(rng, (uint32_t)stream, (uint32_t)row, (uint32_t)(grp * C + lane));
  }
  float best = act ? ph / qv : -INFINITY;
  int bi = act ? lane : 0x7fffffff;
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (act) z_out[grp * C + lane] = (lane == bi) ? ((1.0f + pu) - pu) : 0.0f;
}

// One workgroup, one row's actor tail: LN-SiLU, base_net.3, LN-SiLU, the mu /
// log_sigma heads, tanh(mu + eps sigma) (Agent.py:191-210).  eps: the row's
// explicit N(0,1) variates [A] or NULL (Philox stream `stream`, keyed by
// `row`).  Uses xs[0, 3072 + 2 A).
__device__ __forceinline__ void act_actor_tail(const dr_dims& d, const dr_actor& ac, const float* prea, int det,
                                               const float* eps, const unsigned long long* rng, int stream, int row,
                                               float* a_out, float* mu_out, float* sig_out, float* xs) {
  const int wave = threadIdx.x >> 6;
  const int a1 = d.actor_h1, a2 = d.actor_h2, A = d.action;
  float* x1 = xs;          // SiLU(LN(pre1))
  float* p2 = xs + 1024;   // base_net.3 output
  float* x2 = xs + 2048;   // SiLU(LN(p2))
  if (wave == 0) act_ln_silu(prea, a1, ac.n1.w, ac.n1.b, x1);
  __syncthreads();
  act_rows<25>(a2, a1, ac.l3.w, ac.l3.b, x1, p2);
  __syncthreads();
  if (wave == 0) act_ln_silu(p2, a2, ac.n4.w, ac.n4.b, x2);
  __syncthreads();
  float* hd = xs + 3072;  // [mu (A) | log_sigma (A)]
  for (int o = wave; o < 2 * A; o += ACT_NT / 64) {
    const int lane = threadIdx.x & 63;
    const float* hw = o < A ? ac.mu.w : ac.ls.w;
    const float* hb = o < A ? ac.mu.b : ac.ls.b;
    const int oo = o < A ? o : o - A;
    float wv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wv[j] = lane + 64 * j < a2 ? hw[(long long)oo * a2 + lane + 64 * j] : 0.f;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fmaf(wv[j], lane + 64 * j < a2 ? x2[lane + 64 * j] : 0.f, acc);
    acc = wave_sum(acc);
    if (lane == 0) hd[o] = acc + hb[oo];
  }
  __syncthreads();
  if (threadIdx.x < A) {
    const int i = threadIdx.x;
    const float muv = hd[i];
    const float ls = fminf(fmaxf(hd[A + i], -5.0f), 2.0f);
    const float sg = dr_softplus(ls) + 1e-3f;
    float av;
    if (det) {
      av = tanhf(muv);
    } else {
      float e;
      if (eps) e = eps[i];
      else e = dr_normal(rng, (uint32_t)stream, (uint32_t)row, (uint32_t)i);
      av = tanhf(muv + e * sg);
    }
    a_out[i] = av;
    mu_out[i] = muv;
    sig_out[i] = sg;
  }
}

#define ACT_NW (ACT_NB * (ACT_NT / 64))
// a dense stage with at most ACT_NW / 2 output rows runs as two halves of the grid, each on half the batch
__host__ __device__ inline int act_dense_splits(int nout) { return 2 * nout <= ACT_NW ? 2 : 1; }

// y[e][o] = b[o] + W[o] . x_e for the rows e of the batch not in `skip`, in
// chunks of NE rows: stage_row(dst, e) puts x_e (K floats) into LDS
template <int KJ, int NE, typename StageRow>
__device__ __forceinline__ void act_dense_batch(int n_env, unsigned skip, int nout, int K, const float* __restrict__ W,
                                                const float* __restrict__ b, float* xs, float* y, long long yld,
                                                StageRow stage_row) {
  const int nsp = act_dense_splits(nout), bps = ACT_NB / nsp, sp = blockIdx.x / bps;
  const int per = (n_env + nsp - 1) / nsp, lo = sp * per, hi = min(n_env, lo + per);
  const int gw = (blockIdx.x - sp * bps) * (ACT_NT / 64) + (threadIdx.x >> 6), nw = bps * (ACT_NT / 64);
  for (int e0 = lo; e0 < hi; e0 += NE) {
    unsigned rows = 0;
    for (int r = 0; r < NE && e0 + r < hi; ++r)
      if (!((skip >> (e0 + r)) & 1u)) rows |= 1u << r;
    if (!rows) continue;  // (uniform over the workgroup)
    __syncthreads();      // the previous readers of xs are done
#pragma unroll
    for (int r = 0; r < NE; ++r)
      if ((rows >> r) & 1u) stage_row(xs + r * K, e0 + r);
    __syncthreads();
    act_dense_rows<KJ, NE>(nout, K, W, K, b, xs, K, y + e0 * yld, yld, rows, gw, nw);
  }
}

// ---------------------------------------------------------------------------
// The skeleton: what k_act_batch and k_act_vec do alike.  A kernel is
//   act_prologue | act_gru_pre || encoder stage | act_gru_rows || encoder stage
//   | more encoder stages | latent_mapper.0 | act_sample_rows | act_actor_l0 |
//   act_finish
// with an act_sync between the parts divided by `|`; where a stage has at most
// half as many output rows as the grid has waves (latent_mapper.0, actor
// base_net.0) act_dense_batch splits the batch over the two halves of the grid.
// The sampler runs one wave per (row, latent group), row e's actor tail runs
// in workgroup e.

// a workgroup's words of static LDS beside its copy of the arguments
struct ActShared {
  int ok;          // act_sync's verdict on the last round
  unsigned first;  // bit e: row e starts an episode
  int fail;        // act_finish's reading of the grid's fail flag
};

// the kernel arguments into LDS; returns the mask of the rows that start an episode, from first[] on the device
// or, where the entry point had the flags on the host (dr_act_step), from first_mask
template <typename Args>
__device__ __forceinline__ unsigned act_prologue(Args& a, const Args& ga, ActShared& sh) {
  static_assert(sizeof(Args) % 16 == 0 && sizeof(Args) / 16 <= ACT_NT, "argument copy");
  if (threadIdx.x < sizeof(Args) / 16)
    reinterpret_cast<int4*>(&a)[threadIdx.x] = reinterpret_cast<const int4*>(&ga)[threadIdx.x];
  if (threadIdx.x == 0) {
    unsigned m = ga.c.first_mask;
    if (ga.c.first) {
      m = 0;
      for (int e = 0; e < ga.c.n_env; ++e)
        if (ga.c.first[e]) m |= 1u << e;
    }
    sh.first = m;
  }
  __syncthreads();
  return sh.first;
}

// GRU pre-activations of the continuing rows: gi = W_ih [z; a] + b, gh = W_hh h + b
template <int NE>
__device__ __forceinline__ void act_gru_pre(const ActCommon& a, unsigned first, float* xs) {
  const int Hd = a.d.hidden, L = a.d.rows * a.d.cols, A = a.d.action;
  act_dense_batch<17, NE>(a.n_env, first, 3 * Hd, L + A, a.wm.w_ih, a.wm.b_ih, xs, a.gi, 3 * Hd,
                          [&](float* dst, int e) {
                            act_stage<5>(dst, L + A, [&](int i) {
                              return i < L ? a.z_prev[(long long)e * L + i] : a.a_prev[e * A + i - L];
                            });
                          });
  act_dense_batch<10, NE>(a.n_env, first, 3 * Hd, Hd, a.wm.w_hh, a.wm.b_hh, xs, a.gh, 3 * Hd, [&](float* dst, int e) {
    act_stage<3>(dst, Hd, [&](int i) { return a.h[e * Hd + i]; });
  });
}

// the GRU gates of every row, one element per thread over the grid; h' = 0 at an episode start (h is not read)
__device__ __forceinline__ void act_gru_rows(const ActCommon& a, unsigned first) {
  const int Hd = a.d.hidden;
  const int gt = blockIdx.x * ACT_NT + threadIdx.x;
  for (int i = gt; i < a.n_env * Hd; i += ACT_NB * ACT_NT) {
    const int e = i / Hd, j = i - e * Hd;
    const float hn = ((first >> e) & 1u) ? 0.f : act_gru_gates(a.gi + e * 3 * Hd, a.gh + e * 3 * Hd, Hd, j, a.h[i]);
    a.hn[i] = hn;
    a.h_out[i] = hn;
  }
}

// LN-SiLU, latent_mapper.3 and the categorical sampler: one wave per (row, latent group)
__device__ __forceinline__ void act_sample_rows(const ActCommon& a, float* xs) {
  const int R = a.d.rows, L = R * a.d.cols;
  const int gw = blockIdx.x * (ACT_NT / 64) + (threadIdx.x >> 6);
  for (int t = gw; t < a.n_env * R; t += ACT_NW) {
    const int e = t / R, grp = t - e * R;
    act_latent_group(a.d, a.wm, a.pre1 + e * a.d.enc_hidden, grp, a.noise.q ? a.noise.q + (long long)e * L : nullptr,
                     a.noise.rng, a.noise.stream, a.noise.row0 + e, a.z_out + (long long)e * L,
                     a.logits_out ? a.logits_out + (long long)e * L : nullptr, xs);
  }
}

// actor base_net.0 on cat(h', z') (Agent.py:191-200)
template <int NE>
__device__ __forceinline__ void act_actor_l0(const ActCommon& a, float* xs) {
  const int Hd = a.d.hidden, L = a.d.rows * a.d.cols;
  act_dense_batch<26, NE>(a.n_env, 0u, a.d.actor_h1, Hd + L, a.ac.l0.w, a.ac.l0.b, xs, a.prea, a.d.actor_h1,
                          [&](float* dst, int e) {
                            act_stage<7>(dst, Hd + L, [&](int i) {
                              return i < Hd ? a.hn[e * Hd + i] : a.z_out[(long long)e * L + i - Hd];
                            });
                          });
}

// After the last barrier: the failure path, else row e's actor tail in workgroup e.
// A barrier that timed out (a workgroup never arrived: the grid was not
// co-resident) is reported, never silent: every workgroup that saw it raises
// the status word the host checks after the step, and writes NaN to every
// output of every row (action, mu, sigma, z', h') so nothing downstream can
// mistake them for a state.
// The workgroups that run a tail also re-read the shared fail flag after the
// last barrier: a workgroup that timed out there raised it after arriving (its
// stage data is complete), but the outputs are poisoned all the same.  `status`
// stays the authoritative signal (a flag raised after this read is seen only
// there).
__device__ __forceinline__ void act_finish(const ActCommon& a, bool ok, ActShared& sh, float* xs) {
  const int N = a.n_env, Hd = a.d.hidden, L = a.d.rows * a.d.cols, A = a.d.action;
  if (blockIdx.x < N) {  // (uniform over the workgroup: every wave takes both barriers)
    if (threadIdx.x == 0) sh.fail = __hip_atomic_load(a.fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (sh.fail) ok = false;
  }
  if (!ok) {
    if (threadIdx.x == 0) {
      __hip_atomic_store(a.fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a.status) __hip_atomic_store(a.status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // every failing workgroup poisons every output after its own writes: a
    // workgroup that got past the barrier workgroup 0 gave up on still writes
    // its h' / z' slice (a forced-timeout run caught workgroup 0's NaN being
    // overwritten that way), but it cannot pass the next barrier (workgroup 0
    // never arrives), so it fails too and poisons after its writes
    const float qnan = __int_as_float(0x7fc00000);
    for (int i = threadIdx.x; i < N * A; i += ACT_NT) a.a_out[i] = a.mu_out[i] = a.sig_out[i] = qnan;
    for (int i = threadIdx.x; i < N * L; i += ACT_NT) a.z_out[i] = qnan;
    for (int i = threadIdx.x; i < N * Hd; i += ACT_NT) a.h_out[i] = qnan;
    return;
  }
  // LN-SiLU, base_net.3, LN-SiLU, mu / log_sigma heads, tanh(mu + eps sigma)
  if (blockIdx.x >= N) return;
  const int e = blockIdx.x;
  act_actor_tail(a.d, a.ac, a.prea + e * a.d.actor_h1, a.det, a.noise.eps ? a.noise.eps + e * A : nullptr, a.noise.rng,
                 a.noise.stream + 1, a.noise.row0 + e, a.a_out + e * A, a.mu_out + e * A, a.sig_out + e * A, xs);
  ACT_TS(a, 15);
}

// ---------------------------------------------------------------------------
// Pixel observations: the encoder is four conv stages, the first two beside
// the GRU stages; seven barrier rounds.
struct alignas(16) ActBatchArgs {
  ActCommon c;
  const unsigned char* frames;  // [n_env][H][W][3] u8 (env observation layout)
  float *c1, *c2, *c3, *c4;     // the conv stages' outputs, one copy per row
};

template <int NE>
__global__ __launch_bounds__(ACT_NT) void k_act_batch(ActBatchArgs ga) {
  __shared__ ActBatchArgs sa;
  __shared__ ActShared sh;
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const unsigned first = act_prologue(sa, ga, sh);
  const ActCommon& a = sa.c;
  const dr_dims& d = a.d;
  const int N = a.n_env;
  const int Hd = d.hidden;
  const int c1 = d.enc_f1, c2 = d.enc_f2, c3 = 2 * c2, c4 = 4 * c2;
  const int H0 = d.img_h, W0 = d.img_w, F = c4 * (H0 / 16) * (W0 / 16);
  const long long p1 = (long long)(H0 / 2) * (W0 / 2);
  const long long n1 = p1 * c1, n2 = p1 / 4 * c2, n3 = p1 / 16 * c3, n4 = p1 / 64 * c4;  // == F
  unsigned round = 0;
  bool ok = true;
  ACT_TS(a, 0);

  // ---- stage 1: GRU pre-activations of the continuing rows  ||  conv1 from the frames ----
  act_gru_pre<NE>(a, first, xs);
  // (map shapes as template arguments: act_dims_ok admits only 64 x 64 frames and 32 / 64 filters)
  act_conv_rows<1, true, false, 64, 3>(N, c1, nullptr, 0, sa.frames, a.wm.conv[0].w, a.wm.conv[0].b, sa.c1, n1, xs);
  ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 1);
  // ---- stage 2: conv2  ||  GRU gates ----
  if (ok) {
    act_gru_rows(a, first);
    act_conv_rows<8, false, false, 32, 32>(N, c2, sa.c1, n1, nullptr, a.wm.conv[1].w, a.wm.conv[1].b, sa.c2, n2, xs);
  }
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 2);
  if (ok)
    act_conv_rows<16, false, false, 16, 64>(N, c3, sa.c2, n2, nullptr, a.wm.conv[2].w, a.wm.conv[2].b, sa.c3, n3, xs);
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 3);
  if (ok)
    act_conv_rows<32, false, true, 8, 128>(N, c4, sa.c3, n3, nullptr, a.wm.conv[3].w, a.wm.conv[3].b, sa.c4, n4, xs);
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 4);
  // ---- stage 5: latent_mapper.0 on cat(features, h') (VAE.py:73) ----
  if (ok)
    act_dense_batch<25, NE>(N, 0u, d.enc_hidden, F + Hd, a.wm.map0.w, a.wm.map0.b, xs, a.pre1, d.enc_hidden,
                            [&](float* dst, int e) {
                              act_stage<19>(dst, F + Hd,
                                            [&](int i) { return i < F ? sa.c4[e * n4 + i] : a.hn[e * Hd + i - F]; });
                            });
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 5);
  // ---- stage 6: the sampler ----
  if (ok) act_sample_rows(a, xs);
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 6);
  // ---- stage 7: actor base_net.0 ----
  if (ok) act_actor_l0<NE>(a, xs);
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 7);
  // ---- stage 8: the failure path, or the actor tails ----
  act_finish(a, ok, sh, xs);
}

// ---------------------------------------------------------------------------
// Vector observations (dr_dims.obs_dim = D > 0, BASELINE configs[4]): the
// encoder's four conv stages are two small dense layers (conv[0] = Linear(D,
// F) + SiLU, conv[1] = Linear(F, F) + SiLU, F = 4 * enc_f2),
// which overlap the two GRU stages, so the step takes five barrier rounds
// instead of seven.  Both are act_dense_batch like every other dense stage; a
// layer's SiLU is applied where the next stage stages its input into LDS.
struct alignas(16) ActVecArgs {
  ActCommon c;
  const float* obs;  // [n_env][obs_dim] f32
  float *y0, *y1;    // the encoder layers' pre-activations [F], one copy per row
};

__device__ __forceinline__ float act_silu(float v) { return v / (1.0f + expf(-v)); }

template <int NE>
__global__ __launch_bounds__(ACT_NT) void k_act_vec(ActVecArgs ga) {
  __shared__ ActVecArgs sa;
  __shared__ ActShared sh;
  extern __shared__ __attribute__((aligned(16))) float xs[];
  const unsigned first = act_prologue(sa, ga, sh);
  const ActCommon& a = sa.c;
  const dr_dims& d = a.d;
  const int N = a.n_env;
  const int Hd = d.hidden, D = d.obs_dim, F = 4 * d.enc_f2;
  unsigned round = 0;
  bool ok = true;
  ACT_TS(a, 0);

  // ---- stage 1: GRU pre-activations of the continuing rows  ||  encoder layer 0, y0 = W0 x + b0 ----
  act_gru_pre<NE>(a, first, xs);
  act_dense_batch<4, NE>(N, 0u, F, D, a.wm.conv[0].w, a.wm.conv[0].b, xs, sa.y0, F, [&](float* dst, int e) {
    act_stage<2>(dst, D, [&](int i) { return sa.obs[(long long)e * D + i]; });
  });
  ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 1);
  // ---- stage 2: GRU gates  ||  encoder layer 1, y1 = W1 SiLU(y0) + b1 ----
  if (ok) {
    act_gru_rows(a, first);
    act_dense_batch<4, NE>(N, 0u, F, F, a.wm.conv[1].w, a.wm.conv[1].b, xs, sa.y1, F, [&](float* dst, int e) {
      act_stage<1>(dst, F, [&](int i) { return act_silu(sa.y0[e * F + i]); });
    });
  }
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 2);
  // ---- stage 3: latent_mapper.0 on cat(SiLU(y1), h') (VAE.py:73) ----
  if (ok)
    act_dense_batch<14, NE>(N, 0u, d.enc_hidden, F + Hd, a.wm.map0.w, a.wm.map0.b, xs, a.pre1, d.enc_hidden,
                            [&](float* dst, int e) {
                              act_stage<4>(dst, F + Hd, [&](int i) {
                                return i < F ? act_silu(sa.y1[e * F + i]) : a.hn[e * Hd + i - F];
                              });
                            });
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 3);
  // ---- stage 4: the sampler ----
  if (ok) act_sample_rows(a, xs);
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 4);
  // ---- stage 5: actor base_net.0 ----
  if (ok) act_actor_l0<NE>(a, xs);
  if (ok) ok = act_sync(a.bar, round, &sh.ok, a.spin_limit);
  ACT_TS(a, 5);
  // ---- stage 6: the failure path, or the actor tails ----
  act_finish(a, ok, sh, xs);
}

// ---------------------------------------------------------------------------
// Host side.

static char* act_take(char* base, size_t& off, size_t bytes) {
  const size_t o = (off + 255) & ~(size_t)255;
  off = o + bytes;
  return base ? base + o : nullptr;
}

// the shared part of a workspace (base NULL: sizes only); a kernel's encoder scratch follows it
static void act_carve(char* base, const dr_dims* d, int n_env, ActCommon& c, size_t& off) {
  const size_t n = (size_t)n_env;
  c.ts = (long long*)act_take(base, off, 16 * sizeof(long long));  // first: tools read it at offset 0
  c.bar = (unsigned*)act_take(base, off, ACT_BAR_BYTES);
  c.fail = (int*)act_take(base, off, 256);
  c.gi = (float*)act_take(base, off, 4 * n * 3 * d->hidden);
  c.gh = (float*)act_take(base, off, 4 * n * 3 * d->hidden);
  c.hn = (float*)act_take(base, off, 4 * n * d->hidden);
  c.pre1 = (float*)act_take(base, off, 4 * n * d->enc_hidden);
  c.prea = (float*)act_take(base, off, 4 * n * d->actor_h1);
}

static void act_batch_carve(char* base, const dr_dims* d, int n_env, ActBatchArgs& a, size_t& off) {
  const size_t n = (size_t)n_env, p1 = (size_t)(d->img_h / 2) * (d->img_w / 2);
  const int c1 = d->enc_f1, c2 = d->enc_f2;
  act_carve(base, d, n_env, a.c, off);
  a.c1 = (float*)act_take(base, off, 4 * n * p1 * c1);
  a.c2 = (float*)act_take(base, off, 4 * n * (p1 / 4) * c2);
  a.c3 = (float*)act_take(base, off, 4 * n * (p1 / 16) * 2 * c2);
  a.c4 = (float*)act_take(base, off, 4 * n * (p1 / 64) * 4 * c2);
}

static void act_vec_carve(char* base, const dr_dims* d, int n_env, ActVecArgs& a, size_t& off) {
  const size_t n = (size_t)n_env, F = (size_t)4 * d->enc_f2;
  act_carve(base, d, n_env, a.c, off);
  a.y0 = (float*)act_take(base, off, 4 * n * F);
  a.y1 = (float*)act_take(base, off, 4 * n * F);
}

// the entry points' arguments as the kernels take them (workspace pointers still zero)
static ActCommon act_common(const dr_dims* d, const dr_world_model* wm, const dr_actor* ac, int n_env,
                            const unsigned char* first, unsigned first_mask, const float* z_prev, const float* h,
                            const float* a_prev, dr_noise noise, int deterministic, float* z_out, float* h_out,
                            float* a_out, float* mu_out, float* sigma_out, float* logits_out, int* status) {
  // (ActCommon's members in order, up to status; the workspace members after it are zero)
  return ActCommon{*d,    *wm,   *ac,   first, first_mask, n_env,     deterministic, z_prev,     h,
                   a_prev, noise, z_out, h_out, a_out,      mu_out,    sigma_out,     logits_out, status};
}

// the stage helpers' register batches (KJ) and the LDS staging are sized for the
// CarRacing encoder (Dreamer.py:20-64 config); other shapes use the unfused calls
static bool act_dims_ok(const dr_dims* d) {
  const int F = 4 * d->enc_f2 * (d->img_h / 16) * (d->img_w / 16), L = d->rows * d->cols;
  return (d->enc_depth == 0 || d->enc_depth == 4) && d->img_h == 64 && d->img_w == 64 && d->enc_f1 == 32 &&
         d->enc_f2 == 64 && F + d->hidden <= 64 * 74 && L + d->action <= 64 * 17 && d->hidden <= 64 * 10 &&
         d->hidden + L <= 64 * 26 && d->cols <= 64 && d->rows <= ACT_NB * (ACT_NT / 64) && d->enc_hidden <= 256 &&
         d->actor_h1 <= 256 && d->actor_h2 <= 1024 && d->action <= 64;
}

// act_dims_ok's bounds on the widths the shared stages are sized for (register batches KJ, the sampler's and the
// actor tail's LDS areas), F within the latent_mapper.0 batch (F + hidden <= 64 * 14) and the observation cap; the
// dense helpers loop over K, so obs_dim need not be a multiple of anything
static bool act_vec_dims_ok(const dr_dims* d) {
  const int F = 4 * d->enc_f2, L = d->rows * d->cols;
  return d->obs_dim >= 1 && d->obs_dim <= DR_ACT_VEC_MAX_OBS && F >= 1 && F <= 256 && d->hidden >= 1 &&
         L + d->action <= 64 * 17 && d->hidden <= 64 * 10 && d->hidden + L <= 64 * 26 && d->cols >= 1 &&
         d->cols <= 64 && d->rows >= 1 && d->rows <= ACT_NB * (ACT_NT / 64) && d->enc_hidden >= 1 &&
         d->enc_hidden <= 256 && d->actor_h1 >= 1 && d->actor_h1 <= 256 && d->actor_h2 >= 1 && d->actor_h2 <= 1024 &&
         d->action >= 1 && d->action <= 64;
}

// rows a wave accumulates at once (the instantiation): the batch rounded up to a power of two, at most 8
static int act_batch_ne(int n_env) { return n_env <= 1 ? 1 : n_env <= 2 ? 2 : n_env <= 4 ? 4 : 8; }

// rows of a dense stage's input that are in LDS at once
static size_t act_chunk(int n_env, int nout) {
  const int ne = act_batch_ne(n_env), nsp = act_dense_splits(nout), per = (n_env + nsp - 1) / nsp;
  return (size_t)(per < ne ? per : ne);
}

// floats of dynamic LDS: the conv slab, or the widest dense stage's chunk of input rows
static size_t act_batch_lds(const dr_dims* d, int n_env) {
  const size_t F = (size_t)4 * d->enc_f2 * (d->img_h / 16) * (d->img_w / 16), L = (size_t)d->rows * d->cols;
  size_t n = ACT_BATCH_CONV_LDS;
  auto need = [&](size_t v) { n = v > n ? v : n; };
  need(act_chunk(n_env, 3 * d->hidden) * (L + d->action));
  need(act_chunk(n_env, 3 * d->hidden) * d->hidden);
  need(act_chunk(n_env, d->enc_hidden) * (F + d->hidden));
  need(act_chunk(n_env, d->actor_h1) * (d->hidden + L));
  return n;
}
// what an instantiation may be launched with (set once): 8 rows of the widest stage input act_dims_ok admits
#define ACT_BATCH_LDS_MAX (8 * 64 * 74 * 4)

// floats of dynamic LDS: the widest dense stage's chunk of input rows, and at least what the sampler (1280) and the
// actor tail (3072 + 2 A) use
static size_t act_vec_lds(const dr_dims* d, int n_env) {
  const size_t F = (size_t)4 * d->enc_f2, L = (size_t)d->rows * d->cols;
  size_t n = 3072 + 2 * (size_t)d->action;
  auto need = [&](size_t v) { n = v > n ? v : n; };
  need(act_chunk(n_env, 3 * d->hidden) * (L + d->action));
  need(act_chunk(n_env, 3 * d->hidden) * d->hidden);
  need(act_chunk(n_env, (int)F) * d->obs_dim);
  need(act_chunk(n_env, (int)F) * F);
  need(act_chunk(n_env, d->enc_hidden) * (F + d->hidden));
  need(act_chunk(n_env, d->actor_h1) * (d->hidden + L));
  return n;
}
// what an instantiation may be launched with (set once): 8 rows of the widest stage input act_vec_dims_ok admits
#define ACT_VEC_LDS_MAX (8 * 64 * 26 * 4)
static_assert(DR_ACT_VEC_MAX_OBS <= 64 * 26 && 3072 + 2 * 64 <= 8 * 64 * 26, "LDS bound covers every stage");

// A kernel family as act_launch needs it.
struct ActFamily {
  const void* fn[4];                           // the NE = 1, 2, 4, 8 instantiations
  size_t lds_max;                              // dynamic LDS an instantiation may be launched with
  int resident_ok[DR_ACT_MAX_ENVS + 1][64];    // per (n_env, device): 0 unknown, 1 ok, -1 too small
};

// Zeroes the barrier lines, checks co-residency and launches the instantiation
// for c.n_env rows with `lds` bytes of dynamic LDS.  name: the entry point,
// for messages; c: the ActCommon inside *args (the kernel's argument struct).
//
// A plain launch whose grid barrier needs all ACT_NB workgroups resident at
// once.  The cooperative launch would add exactly that check at +15-19 us of
// host time per env step (MI355X_MICROARCH.md coop-launch), so it is made once
// per batch size and device here instead, with the dynamic LDS that n_env
// launches (up to 147 KiB: one workgroup per CU): the occupancy API's blocks
// per CU (one lower than reported, the guide's sgpr-count margin) times the CU
// count must cover the grid, else the call fails and the caller runs the
// unfused path.  What no launch-time check can cover -- other work holding CUs
// for longer than the bounded spin -- comes back through `status` (and NaN
// outputs).
static int act_launch(const char* name, ActFamily& fam, size_t lds, ActCommon& c, void* args, hipStream_t s) {
  const char* force = getenv("DREAMER_ACT_FORCE");  // test hook (include/dreamer_hip.h)
  const bool force_timeout = force && strcmp(force, "timeout") == 0;
  const bool force_nonres = force && strcmp(force, "nonresident") == 0;
  // barrier lines + fail flag (a kernel, so a captured graph re-arms them too)
  static_assert((ACT_BAR_BYTES + 512) % 4 == 0, "barrier bytes");
  DR_TRY(op_fill((ACT_BAR_BYTES + 512) / 4, reinterpret_cast<float*>(c.bar), 0.f, s));
  const int ne = act_batch_ne(c.n_env);
  const void* fn = fam.fn[ne == 1 ? 0 : ne == 2 ? 1 : ne == 4 ? 2 : 3];
  if (lds > fam.lds_max) {
    dr_set_error("%s: stage input beyond the LDS budget", name);
    return DR_E_INVALID;
  }
  int dev = 0;
  DR_TRY_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) {
    dr_set_error("%s: device index", name);
    return DR_E_INVALID;
  }
  int& resident = fam.resident_ok[c.n_env][dev];  // (idempotent, benign race)
  if (resident == 0) {
    DR_TRY_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fam.lds_max));
    int per_cu = 0, cus = 0;
    DR_TRY_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, ACT_NT, lds));
    DR_TRY_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    resident = (long long)(per_cu - 1 > 0 ? per_cu - 1 : per_cu) * cus >= ACT_NB ? 1 : -1;
  }
  if (resident != 1 || force_nonres) {
    dr_set_error("%s: the device cannot hold the acting grid co-resident", name);
    return DR_E_UNSUPPORTED;
  }
  c.spin_limit = force_timeout ? 0 : ACT_SPIN_LIMIT;
  void* kargs[] = {args};
  DR_TRY_HIP(hipLaunchKernel(fn, dim3(ACT_NB), dim3(ACT_NT), kargs, lds, s));
  return dr_check_launch(name + 3);  // (without the dr_)
}

// dr_act_step and dr_act_batch past their argument checks: c.n_env frames through k_act_batch
static int act_batch_run(const char* name, const ActCommon& c, const unsigned char* frames, void* ws, size_t ws_bytes,
                         hipStream_t s) {
  static ActFamily fam = {{(const void*)k_act_batch<1>, (const void*)k_act_batch<2>, (const void*)k_act_batch<4>,
                           (const void*)k_act_batch<8>},
                          ACT_BATCH_LDS_MAX};
  ActBatchArgs a;
  memset(&a, 0, sizeof(a));
  a.c = c;
  a.frames = frames;
  size_t off = 0;
  act_batch_carve((char*)ws, &c.d, c.n_env, a, off);
  if (off > ws_bytes) {
    dr_set_error("%s: workspace too small", name);
    return DR_E_INVALID;
  }
  return act_launch(name, fam, act_batch_lds(&c.d, c.n_env) * 4, a.c, &a, s);
}

extern "C" size_t dr_act_batch_workspace_bytes(const dr_dims* d, int n_env) {
  if (!d || n_env < 1) return 0;
  ActBatchArgs a;
  size_t off = 0;
  act_batch_carve(nullptr, d, n_env, a, off);
  return off;
}

extern "C" size_t dr_act_step_workspace_bytes(const dr_dims* d) { return dr_act_batch_workspace_bytes(d, 1); }

// the one-row call of k_act_batch<1>: has_prev is the row's first flag, on the host
extern "C" int dr_act_step(const dr_dims* d, const dr_world_model* wm, const dr_actor* ac, const unsigned char* frame,
                           int has_prev, const float* z_prev, const float* h, const float* a_prev, dr_noise noise,
                           int deterministic, float* z_out, float* h_out, float* a_out, float* mu_out,
                           float* sigma_out, float* logits_out, int* status, void* ws, size_t ws_bytes,
                           hipStream_t s) {
  DR_REQUIRE(d && wm && ac && frame && h && z_out && h_out && a_out && mu_out && sigma_out && ws, "null argument");
  DR_REQUIRE(!has_prev || (z_prev && a_prev), "has_prev needs z_prev and a_prev");
  DR_REQUIRE(d->obs_dim == 0, "dr_act_step: pixel observations only (vector observations use dr_act_vec)");
  if (!act_dims_ok(d)) {
    dr_set_error("dr_act_step: dims outside the acting kernel (64x64 frames, encoder 32/64 filters, widths <= the "
                 "staging)");
    return DR_E_UNSUPPORTED;
  }
  DR_TRY(dims_envelope(__func__, d, ENV_GRU | ENV_SAMPLER | ENV_ACTOR));
  return act_batch_run("dr_act_step",
                       act_common(d, wm, ac, 1, nullptr, has_prev ? 0u : 1u, z_prev, h, a_prev, noise, deterministic,
                                  z_out, h_out, a_out, mu_out, sigma_out, logits_out, status),
                       frame, ws, ws_bytes, s);
}

extern "C" int dr_act_batch(const dr_dims* d, const dr_world_model* wm, const dr_actor* ac, int n_env,
                            const unsigned char* frames, const unsigned char* first, const float* z_prev,
                            const float* h, const float* a_prev, dr_noise noise, int deterministic, float* z_out,
                            float* h_out, float* a_out, float* mu_out, float* sigma_out, float* logits_out,
                            int* status, void* ws, size_t ws_bytes, hipStream_t s) {
  DR_REQUIRE(n_env >= 1, "n_env < 1");
  DR_REQUIRE(d && wm && ac && frames && first && z_prev && h && a_prev && z_out && h_out && a_out && mu_out &&
                 sigma_out && ws,
             "null argument");
  if (n_env > DR_ACT_MAX_ENVS) {
    dr_set_error("dr_act_batch: n_env above DR_ACT_MAX_ENVS");
    return DR_E_UNSUPPORTED;
  }
  if (d->obs_dim != 0 || !act_dims_ok(d)) {
    dr_set_error("dr_act_batch: dims outside the acting kernel (pixel observations, 64x64 frames, encoder 32/64 "
                 "filters, widths <= the staging)");
    return DR_E_UNSUPPORTED;
  }
  DR_TRY(dims_envelope(__func__, d, ENV_GRU | ENV_SAMPLER | ENV_ACTOR));
  return act_batch_run("dr_act_batch",
                       act_common(d, wm, ac, n_env, first, 0u, z_prev, h, a_prev, noise, deterministic, z_out, h_out,
                                  a_out, mu_out, sigma_out, logits_out, status),
                       frames, ws, ws_bytes, s);
}

extern "C" size_t dr_act_vec_workspace_bytes(const dr_dims* d, int n_env) {
  if (!d || n_env < 1) return 0;
  ActVecArgs a;
  size_t off = 0;
  act_vec_carve(nullptr, d, n_env, a, off);
  return off;
}

extern "C" int dr_act_vec(const dr_dims* d, const dr_world_model* wm, const dr_actor* ac, int n_env, const float* obs,
                          const unsigned char* first, const float* z_prev, const float* h, const float* a_prev,
                          dr_noise noise, int deterministic, float* z_out, float* h_out, float* a_out, float* mu_out,
                          float* sigma_out, float* logits_out, int* status, void* ws, size_t ws_bytes,
                          hipStream_t s) {
  DR_REQUIRE(n_env >= 1, "n_env < 1");
  DR_REQUIRE(d && wm && ac && obs && first && z_prev && h && a_prev && z_out && h_out && a_out && mu_out &&
                 sigma_out && ws,
             "null argument");
  DR_REQUIRE(d->obs_dim != 0, "dr_act_vec: vector observations only (pixel models use dr_act_step / dr_act_batch)");
  if (n_env > DR_ACT_MAX_ENVS) {
    dr_set_error("dr_act_vec: n_env above DR_ACT_MAX_ENVS");
    return DR_E_UNSUPPORTED;
  }
  if (!act_vec_dims_ok(d)) {
    dr_set_error("dr_act_vec: dims outside the acting kernel (obs_dim <= DR_ACT_VEC_MAX_OBS, 4 enc_f2 <= 256, widths "
                 "<= the staging)");
    return DR_E_UNSUPPORTED;
  }
  DR_TRY(dims_envelope(__func__, d, ENV_GRU | ENV_SAMPLER | ENV_ACTOR));
  static ActFamily fam = {{(const void*)k_act_vec<1>, (const void*)k_act_vec<2>, (const void*)k_act_vec<4>,
                           (const void*)k_act_vec<8>},
                          ACT_VEC_LDS_MAX};
  ActVecArgs a;
  memset(&a, 0, sizeof(a));
  a.c = act_common(d, wm, ac, n_env, first, 0u, z_prev, h, a_prev, noise, deterministic, z_out, h_out, a_out, mu_out,
                   sigma_out, logits_out, status);
  a.obs = obs;
  size_t off = 0;
  act_vec_carve((char*)ws, d, n_env, a, off);
  DR_REQUIRE(off <= ws_bytes, "workspace too small");
  return act_launch("dr_act_vec", fam, act_vec_lds(d, n_env) * 4, a.c, &a, s);
}
