// Perturbation saliency (saliency.py; Greydanus et al. 2018): the perturbed
// copies of u8 frames, the scores of the agent's outputs on them against the
// unperturbed copy, and the per-pixel heat map.  include/dreamer_hip.h
// "perturbation saliency" has the definitions; the arithmetic is pinned there
// (explicit fmaf chains, tables made on the host), so the host reproduces the
// u8 output from the same tables.  One-shot kernels: nothing is shared between
// workgroups, no atomics.
#include "ops.h"

#define SAL_MAX_RB 15      // widest blur radius
#define SAL_MAX_CELLS 1024 // cells of one frame's grid
#define SAL_STRIP 8        // output rows of one blur workgroup
#define SAL_VCHUNK 32      // variants one blend workgroup writes
#define SAL_MAX_LDS 65536

// the u8 frame (b = f, t = 0) of a ring source, t0 included
__device__ __forceinline__ const unsigned char* sal_frame(const dr_frames& src, int f, long long n) {
  long long slot = (src.starts[f] + src.t0) % src.ring_cap;
  if (slot < 0) slot += src.ring_cap;
  return src.ring + slot * n;
}

__device__ __forceinline__ int sal_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__device__ __forceinline__ unsigned char sal_quant(float v) {
  return (unsigned char)fminf(255.0f, fmaxf(0.0f, rintf(v)));
}

// fill = blur.  One workgroup per (strip of SAL_STRIP rows, channel, frame):
// the horizontally filtered rows y0 - rb .. y0 + SAL_STRIP - 1 + rb (row index
// clamped, as the vertical pass reads them) go to LDS, then the vertical pass
// writes the strip of A.  Both sums: fmaf chains from 0.0f in ascending k.
__global__ __launch_bounds__(256) void k_sal_blur(int H, int W, int rb, dr_frames src,
                                                  const float* __restrict__ wb, float* __restrict__ A) {
  extern __shared__ float hh[];  // [SAL_STRIP + 2 rb][W]
  __shared__ float taps[2 * SAL_MAX_RB + 1];
  const int tid = threadIdx.x;
  const int y0 = blockIdx.x * SAL_STRIP, c = blockIdx.y, f = blockIdx.z;
  const int rows = min(SAL_STRIP, H - y0);
  const int nt = 2 * rb + 1;
  if (tid < nt) taps[tid] = wb[tid];
  __syncthreads();
  const long long n = 3LL * H * W;
  const unsigned char* I = sal_frame(src, f, n) + (long long)c * H * W;
  const int lrows = rows + 2 * rb;
  for (int idx = tid; idx < lrows * W; idx += 256) {
    const int j = idx / W, x = idx - j * W;
    const unsigned char* row = I + (long long)sal_clamp(y0 - rb + j, H - 1) * W;
    float acc = 0.0f;
    for (int k = 0; k < nt; ++k) acc = fmaf(taps[k], (float)row[sal_clamp(x + k - rb, W - 1)], acc);
    hh[idx] = acc;
  }
  __syncthreads();
  float* Ac = A + (long long)f * n + (long long)c * H * W;
  for (int idx = tid; idx < rows * W; idx += 256) {
    const int j = idx / W, x = idx - j * W;
    float acc = 0.0f;
    for (int k = 0; k < nt; ++k) acc = fmaf(taps[k], hh[(j + k) * W + x], acc);
    Ac[(long long)(y0 + j) * W + x] = acc;
  }
}

// fill = mean.  One workgroup per (channel, frame): the exact integer sum of
// the channel, then one f32 division.
__global__ __launch_bounds__(256) void k_sal_mean(int HW, dr_frames src, float* __restrict__ A) {
  __shared__ unsigned part[256];
  const int tid = threadIdx.x, c = blockIdx.x, f = blockIdx.y;
  const unsigned char* I = sal_frame(src, f, 3LL * HW) + (long long)c * HW;
  unsigned acc = 0;
  for (int i = tid; i < HW; i += 256) acc += I[i];
  part[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) A[f * 3 + c] = (float)part[0] / (float)HW;
}

// Blend.  A thread owns PX consecutive pixels of one row (PX = 16: one 16-byte
// store per variant; PX = 1: the plain path) and keeps I and A - I of them in
// registers; the workgroup writes the variants g0 .. g0 + SAL_VCHUNK - 1 of its
// frame.  A is read once per workgroup.  Grid: (pixel blocks, variant chunks, F).
template <int PX>
__global__ __launch_bounds__(256) void k_sal_blend(int H, int W, int s, int Gx, int G, int mean_fill, dr_frames src,
                                                   const float* __restrict__ A, const float* __restrict__ gm,
                                                   unsigned char* __restrict__ out) {
  extern __shared__ float gml[];  // [max(H, W)]
  const int tid = threadIdx.x, f = blockIdx.z;
  const int ng = max(H, W);
  for (int i = tid; i < ng; i += 256) gml[i] = gm[i];
  __syncthreads();
  const int HW = H * W;
  const long long n = 3LL * HW;
  const long long p0 = ((long long)blockIdx.x * 256 + tid) * PX;
  if (p0 >= n) return;  // (no barrier below)
  const int c = (int)(p0 / HW);
  const int rem = (int)(p0 - (long long)c * HW);
  const int y = rem / W, x0 = rem - y * W;
  const unsigned char* I8 = sal_frame(src, f, n) + p0;
  unsigned char raw[PX];
  float I[PX], D[PX];
  if (PX == 16) {
    const uint4 v = *reinterpret_cast<const uint4*>(I8);
    const unsigned w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < PX; ++e) raw[e] = (unsigned char)(w4[e >> 2] >> (8 * (e & 3)));
  } else {
#pragma unroll
    for (int e = 0; e < PX; ++e) raw[e] = I8[e];
  }
  float a[PX];
  if (mean_fill) {
    const float am = A[f * 3 + c];
#pragma unroll
    for (int e = 0; e < PX; ++e) a[e] = am;
  } else if (PX == 16) {
    const float4* Av = reinterpret_cast<const float4*>(A + (long long)f * n + p0);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 t = Av[q];
      a[4 * q] = t.x; a[4 * q + 1] = t.y; a[4 * q + 2] = t.z; a[4 * q + 3] = t.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < PX; ++e) a[e] = A[(long long)f * n + p0 + e];
  }
#pragma unroll
  for (int e = 0; e < PX; ++e) {
    I[e] = (float)raw[e];
    D[e] = a[e] - I[e];
  }
  const int g0 = blockIdx.y * SAL_VCHUNK, g1 = min(g0 + SAL_VCHUNK, G + 1);
  unsigned char* o = out + ((long long)f * (G + 1) + g0) * n + p0;
  for (int g = g0; g < g1; ++g, o += n) {
    unsigned char q[PX];
    if (g == 0) {  // variant 0: the frame itself
#pragma unroll
      for (int e = 0; e < PX; ++e) q[e] = raw[e];
    } else {
      const int i = (g - 1) / Gx, j = (g - 1) - i * Gx;
      const int cy = i * s + s / 2, cx = j * s + s / 2;
      const float my = gml[abs(y - cy)];
#pragma unroll
      for (int e = 0; e < PX; ++e) {
        const float m = my * gml[abs(x0 + e - cx)];
        q[e] = sal_quant(fmaf(m, D[e], I[e]));
      }
    }
    if (PX == 16) {
      unsigned w4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        w4[k] = (unsigned)q[4 * k] | ((unsigned)q[4 * k + 1] << 8) | ((unsigned)q[4 * k + 2] << 16) |
                ((unsigned)q[4 * k + 3] << 24);
      *reinterpret_cast<uint4*>(o) = make_uint4(w4[0], w4[1], w4[2], w4[3]);
    } else {
#pragma unroll
      for (int e = 0; e < PX; ++e) o[e] = q[e];
    }
  }
}

extern "C" size_t dr_occlude_workspace_bytes(const dr_dims* d, int F) {
  if (!d || F <= 0 || d->img_h <= 0 || d->img_w <= 0) return 0;
  return (size_t)F * 3 * d->img_h * d->img_w * sizeof(float);
}

extern "C" int dr_occlude_frames(const dr_dims* d, const dr_frames* src, int F, int s, int fill, const float* wb,
                                 int rb, const float* gm, unsigned char* out, void* ws, size_t ws_bytes,
                                 hipStream_t st) {
  DR_REQUIRE(d && src && out && F > 0 && F <= 65535, "null argument, empty batch or more than 65535 frames");
  if (d->obs_dim > 0) {
    dr_set_error("%s: vector observations have no frames to perturb", __func__);
    return DR_E_UNSUPPORTED;
  }
  const int H = d->img_h, W = d->img_w;
  DR_REQUIRE(H > 0 && W > 0, "bad frame size");
  DR_REQUIRE(fill == 0 || fill == 1, "fill must be 0 (blur) or 1 (mean)");
  DR_REQUIRE(s > 0 && H % s == 0 && W % s == 0, "the stride must divide the frame");
  const int Gy = H / s, Gx = W / s;
  DR_REQUIRE((long long)Gy * Gx <= SAL_MAX_CELLS, "more than 1024 cells");
  DR_REQUIRE(rb >= 0 && rb <= SAL_MAX_RB, "blur radius above 15");
  DR_REQUIRE(gm && (fill == 1 || wb), "a table is NULL");
  if (!src->ring) {
    dr_set_error("%s: the source must be a u8 ring", __func__);
    return DR_E_UNSUPPORTED;
  }
  DR_REQUIRE(src->starts && src->ring_cap > 0 && src->t0 >= 0, "ring source needs starts, ring_cap and t0 >= 0");
  const int G = Gy * Gx;
  const long long n = 3LL * H * W;
  DR_REQUIRE(n * (G + 1) * F <= 0x7fffffffLL * 16, "too many output pixels");
  DR_REQUIRE(ws, "workspace required");
  const size_t blur_lds = (size_t)(SAL_STRIP + 2 * rb) * W * sizeof(float);
  if (fill == 0 && blur_lds > SAL_MAX_LDS - 256) {
    dr_set_error("%s: rows too wide for the blur's LDS strip", __func__);
    return DR_E_UNSUPPORTED;
  }
  if (ws_bytes < dr_occlude_workspace_bytes(d, F)) {
    dr_set_error("%s: workspace too small", __func__);
    return DR_E_WORKSPACE;
  }
  float* A = (float*)ws;
  if (fill == 0)
    hipLaunchKernelGGL(k_sal_blur, dim3(dr_cdiv(H, SAL_STRIP), 3, F), dim3(256), blur_lds, st, H, W, rb, *src, wb, A);
  else
    hipLaunchKernelGGL(k_sal_mean, dim3(3, F), dim3(256), 0, st, H * W, *src, A);
  DR_TRY(dr_check_launch("occlude fill"));
  const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool vec = W % 16 == 0 && al16(out) && al16(src->ring) && al16(A);
  const size_t gm_lds = (size_t)(H > W ? H : W) * sizeof(float);
  const unsigned vch = (unsigned)dr_cdiv(G + 1, SAL_VCHUNK);
  if (vec)
    hipLaunchKernelGGL(k_sal_blend<16>, dim3((unsigned)((n / 16 + 255) / 256), vch, F), dim3(256), gm_lds, st, H, W, s,
                       Gx, G, fill, *src, A, gm, out);
  else
    hipLaunchKernelGGL(k_sal_blend<1>, dim3((unsigned)((n + 255) / 256), vch, F), dim3(256), gm_lds, st, H, W, s, Gx, G,
                       fill, *src, A, gm, out);
  return dr_check_launch("occlude blend");
}

// ---------------------------------------------------------------------------
// Scores of variant g against variant 0 of the same frame.  One 256-thread
// workgroup per (f, g).  actor: a thread takes the elements tid, tid + 256, ...
// in ascending order.  KL and flips: a categorical takes W lanes (one class
// each, fixed DPP trees inside the group), the group's first lane adds its
// categoricals in ascending order.  Then wave_sum's fixed tree and the four
// wave sums in wave order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float sal_block_sum(float v, float* part) {
  v = wave_sum(v);
  __syncthreads();  // (part is reused)
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// max-subtracted log-softmax of one categorical spread over W lanes (k_latent_stats'
// form): lp = (x - max) - log(sum).  Lanes that hold no class carry act = false.
__device__ __forceinline__ float sal_logsoftmax(float x, bool act, int W) {
  const float mx = group_max(act ? x : -INFINITY, W);
  const float se = group_sum(act ? expf(x - mx) : 0.0f, W);
  return (x - mx) - logf(se);
}

// W: the power of two >= C (<= 64); a categorical takes W lanes, a pass of the
// workgroup 256 / W categoricals.
__global__ __launch_bounds__(256) void k_sal_scores(int G, int A, int R, int C, int W, const float* __restrict__ mu,
                                                    const float* __restrict__ V, const float* __restrict__ logits,
                                                    const float* __restrict__ z, float* __restrict__ actor,
                                                    float* __restrict__ value, float* __restrict__ value_delta,
                                                    float* __restrict__ kl, int* __restrict__ flips) {
  __shared__ float part[4];
  const int tid = threadIdx.x;
  const int f = blockIdx.x / G, g = blockIdx.x - f * G + 1;
  const long long r0 = (long long)f * (G + 1), rg = r0 + g;
  const long long o = (long long)f * G + (g - 1);
  if (actor) {
    float acc = 0.0f;
    for (int i = tid; i < A; i += 256) {
      const float dv = mu[rg * A + i] - mu[r0 * A + i];
      acc = acc + dv * dv;
    }
    acc = sal_block_sum(acc, part);
    if (tid == 0) actor[o] = 0.5f * acc;
  }
  if (tid == 0 && (value || value_delta)) {
    const float dv = V[rg] - V[r0];
    if (value_delta) value_delta[o] = dv;
    if (value) value[o] = 0.5f * (dv * dv);
  }
  if (!kl && !flips) return;  // (uniform)
  const long long L = (long long)R * C;
  const int gpp = 256 / W;                   // categoricals per pass
  const int gl = tid / W, j = tid - gl * W;  // categorical of the pass, class lane
  float a_kl = 0.0f, a_fl = 0.0f;            // (a count <= R < 2^24 is exact in f32)
  for (int rr = 0; rr < R; rr += gpp) {      // uniform trip count: every lane takes part in the reductions
    const int r = rr + gl;
    const bool act = r < R && j < C;
    const long long e = (long long)r * C + j;
    if (kl) {
      const float lp = sal_logsoftmax(act ? logits[r0 * L + e] : 0.0f, act, W);
      const float lq = sal_logsoftmax(act ? logits[rg * L + e] : 0.0f, act, W);
      const float p = expf(lp);
      // a class whose p underflowed adds exactly 0 (never 0 * inf)
      const float t = group_sum((act && p > 0.0f) ? p * (lp - lq) : 0.0f, W);
      if (j == 0 && r < R) a_kl = a_kl + t;
    }
    if (flips) {  // the selected class: the lowest index holding the categorical's maximum
      float b0 = act ? z[r0 * L + e] : -INFINITY, bg = act ? z[rg * L + e] : -INFINITY;
      int i0 = j, ig = j;
      group_argmax(b0, i0, W);
      group_argmax(bg, ig, W);
      if (j == 0 && r < R) a_fl = a_fl + (i0 != ig ? 1.0f : 0.0f);
    }
  }
  if (kl) {
    a_kl = sal_block_sum(a_kl, part);
    if (tid == 0) kl[o] = a_kl;
  }
  if (flips) {
    a_fl = sal_block_sum(a_fl, part);
    if (tid == 0) flips[o] = (int)a_fl;
  }
}

extern "C" int dr_saliency_scores(int F, int G, int A, int R, int C, const float* mu, const float* V,
                                  const float* logits, const float* z, float* actor, float* value,
                                  float* value_delta, float* posterior_kl, int* latent_flips, hipStream_t st) {
  DR_REQUIRE(F >= 0 && G >= 1 && A >= 1 && R >= 1 && C >= 1, "need F >= 0, G, A, R, C >= 1");
  DR_REQUIRE(R < (1 << 24) && (long long)F * G <= 0x7fffffffLL, "too many rows");
  DR_REQUIRE(C <= 64 || !(posterior_kl || latent_flips), "posterior_kl / latent_flips need C <= 64");
  DR_REQUIRE(!actor || mu, "actor needs mu");
  DR_REQUIRE(!(value || value_delta) || V, "value / value_delta need V");
  DR_REQUIRE(!posterior_kl || logits, "posterior_kl needs logits");
  DR_REQUIRE(!latent_flips || z, "latent_flips needs z");
  if (F == 0 || !(actor || value || value_delta || posterior_kl || latent_flips)) return DR_OK;
  int W = 1;
  while (W < C && W < 64) W <<= 1;
  hipLaunchKernelGGL(k_sal_scores, dim3((unsigned)(F * G)), dim3(256), 0, st, G, A, R, C, W, mu, V, logits, z, actor,
                     value, value_delta, posterior_kl, latent_flips);
  return dr_check_launch("saliency_scores");
}

// ---------------------------------------------------------------------------
// Heat map and overlay: one thread per pixel, grid (pixel blocks, F).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void sal_axis(int p, int s, int Gn, int& i0, int& i1, float& w) {
  const float fp = fminf(fmaxf(((float)(p - s / 2)) / (float)s, 0.0f), (float)(Gn - 1));
  const float fl = floorf(fp);
  i0 = (int)fl;
  i1 = min(i0 + 1, Gn - 1);
  w = fp - fl;
}

__global__ __launch_bounds__(256) void k_sal_map(int H, int W, int s, int ch, const float* __restrict__ scores,
                                                 const float* __restrict__ scale, dr_frames src,
                                                 float* __restrict__ map, unsigned char* __restrict__ overlay) {
  const int f = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int HW = H * W;
  if (p >= HW) return;
  const int y = p / W, x = p - y * W;
  const int Gy = H / s, Gx = W / s;
  int i0, i1, j0, j1;
  float wy, wx;
  sal_axis(y, s, Gy, i0, i1, wy);
  sal_axis(x, s, Gx, j0, j1, wx);
  const float* S = scores + (long long)f * Gy * Gx;
  const float uy = 1.0f - wy, ux = 1.0f - wx;
  const float bl = (((uy * ux) * S[i0 * Gx + j0] + (uy * wx) * S[i0 * Gx + j1]) + (wy * ux) * S[i1 * Gx + j0]) +
                   (wy * wx) * S[i1 * Gx + j1];
  const float m = scale[f] * bl;
  map[(long long)f * HW + p] = m;
  if (overlay) {
    const float heat = fminf(1.0f, fmaxf(0.0f, m));
    const unsigned char* I = sal_frame(src, f, 3LL * HW);
    unsigned char* O = overlay + (long long)f * 3 * HW;
    for (int c = 0; c < 3; ++c) {
      const unsigned char v = I[c * HW + p];
      const float iv = (float)v;
      O[c * HW + p] = c == ch ? (unsigned char)rintf(fmaf(heat, 255.0f - iv, iv)) : v;
    }
  }
}

extern "C" int dr_saliency_map(const dr_dims* d, int F, int s, const float* scores, const float* scale,
                               const dr_frames* frames, int ch, float* map, unsigned char* overlay, hipStream_t st) {
  DR_REQUIRE(d && scores && scale && map && F >= 0 && F <= 65535, "null argument or more than 65535 frames");
  if (d->obs_dim > 0) {
    dr_set_error("%s: vector observations have no frames", __func__);
    return DR_E_UNSUPPORTED;
  }
  const int H = d->img_h, W = d->img_w;
  DR_REQUIRE(H > 0 && W > 0 && s > 0 && H % s == 0 && W % s == 0, "the stride must divide the frame");
  DR_REQUIRE((long long)(H / s) * (W / s) <= SAL_MAX_CELLS, "more than 1024 cells");
  if (overlay) {
    DR_REQUIRE(frames && ch >= 0 && ch < 3, "the overlay needs frames and a channel 0..2");
    if (!frames->ring) {
      dr_set_error("%s: the frames must be a u8 ring", __func__);
      return DR_E_UNSUPPORTED;
    }
    DR_REQUIRE(frames->starts && frames->ring_cap > 0 && frames->t0 >= 0, "ring source needs starts, ring_cap and t0 >= 0");
  }
  if (F == 0) return DR_OK;
  dr_frames fr = {};
  if (overlay) fr = *frames;
  hipLaunchKernelGGL(k_sal_map, dim3((unsigned)dr_cdiv(H * W, 256), (unsigned)F), dim3(256), 0, st, H, W, s, ch, scores,
                     scale, fr, map, overlay);
  return dr_check_launch("saliency_map");
}

// One block of Exp(1) draws per frame (saliency.py shares it among the frame's
// variants): q[row][c] = the Philox variate of (noise.stream, noise.row0 + row, c).
__global__ __launch_bounds__(256) void k_sal_draws(long long n, int C, const unsigned long long* __restrict__ rng,
                                                   int row0, int stream, float* __restrict__ q) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long row = i / C;
  q[i] = dr_exp1(rng, (uint32_t)stream, (uint32_t)(row0 + row), (uint32_t)(i - row * C));
}

extern "C" int dr_saliency_draws(int rows, int C, dr_noise noise, float* q, hipStream_t st) {
  DR_REQUIRE(rows >= 0 && C >= 1 && q && noise.rng, "need rows >= 0, C >= 1, q and the Philox state");
  const long long n = (long long)rows * C;
  DR_REQUIRE(n <= 0x7fffffffLL, "too many draws");
  if (n == 0) return DR_OK;
  hipLaunchKernelGGL(k_sal_draws, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, C, noise.rng, noise.row0,
                     noise.stream, q);
  return dr_check_launch("saliency_draws");
}
