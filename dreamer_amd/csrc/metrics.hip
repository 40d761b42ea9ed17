// Metrics of the diagnostics on replay windows (open-loop prediction, posterior
// trace, agent trace).  Frame metrics: decoded frames against
// the true frames of the replay ring -- the per-frame squared error of the
// reconstruction term (WorldModel.py:129) and the u8 frames of a prediction
// video.  Built with -ffp-contract=off like the other elementwise code, so the
// host reproduces the u8 quantisation and every term of the sum bit for bit.
#include "ops.h"

// true value of a stored u8 pixel (Dreamer.py:251: IEEE divide, then subtract)
__device__ __forceinline__ float fm_norm(float v) { return v / 255.0f - 0.5f; }
// u8 of a normalised value: min(255, max(0, rint((x + 0.5) * 255)))
__device__ __forceinline__ unsigned char fm_quant(float x) {
  return (unsigned char)fminf(255.0f, fmaxf(0.0f, rintf((x + 0.5f) * 255.0f)));
}

// One 256-thread workgroup per frame m = b*T + t of n elements.  VEC: n % 4 ==
// 0 and every base / stride 16-byte (f32) or 4-byte (u8) aligned: a thread
// takes the 4-element groups tid, tid + 256, ... (one 16-byte load of mu, one
// 4-byte load of four u8 pixels); otherwise elements tid, tid + 256, ...
// Either way a thread adds its elements in ascending index order; the 64
// lane sums then go through wave_sum's fixed tree and the four wave sums
// through LDS in wave order.  Nothing is shared between workgroups.
template <bool VEC>
__global__ __launch_bounds__(256) void k_frame_metrics(int T, int n, int vector, const float* __restrict__ mu,
                                                       dr_frames src, float* __restrict__ sqerr,
                                                       unsigned char* __restrict__ pred,
                                                       unsigned char* __restrict__ tru) {
  __shared__ float part[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int b = m / T, t = m - b * T + src.t0;
  const float* mum = mu + (long long)m * n;
  const unsigned char* r8 = nullptr;  // u8 ring frame
  const float* rf = nullptr;          // f32 frame (the vector ring's row, or the f32 form)
  if (src.ring) {
    long long slot = (src.starts[b] + t) % src.ring_cap;
    if (slot < 0) slot += src.ring_cap;
    if (vector) rf = reinterpret_cast<const float*>(src.ring) + slot * n;
    else r8 = src.ring + slot * n;
  } else {
    rf = src.obs + (long long)b * src.stride_b + (long long)t * src.stride_t;
  }
  const bool raw = !vector && src.raw255;
  unsigned char* pm = pred ? pred + (long long)m * n : nullptr;
  unsigned char* tm = tru ? tru + (long long)m * n : nullptr;
  float acc = 0.0f;
  if (VEC) {
    for (int g = tid; g < (n >> 2); g += 256) {
      const float4 mv = reinterpret_cast<const float4*>(mum)[g];
      const float pv[4] = {mv.x, mv.y, mv.z, mv.w};
      float x[4];
      uchar4 tq;
      if (r8) {
        tq = reinterpret_cast<const uchar4*>(r8)[g];
        x[0] = fm_norm((float)tq.x); x[1] = fm_norm((float)tq.y);
        x[2] = fm_norm((float)tq.z); x[3] = fm_norm((float)tq.w);
      } else {
        const float4 fv = reinterpret_cast<const float4*>(rf)[g];
        const float v[4] = {fv.x, fv.y, fv.z, fv.w};
        unsigned char q[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x[e] = raw ? fm_norm(v[e]) : v[e];
          q[e] = fm_quant(x[e]);
        }
        tq = make_uchar4(q[0], q[1], q[2], q[3]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float dv = pv[e] - x[e];
        acc = acc + dv * dv;
      }
      if (pm) reinterpret_cast<uchar4*>(pm)[g] = make_uchar4(fm_quant(pv[0]), fm_quant(pv[1]), fm_quant(pv[2]),
                                                              fm_quant(pv[3]));
      if (tm) reinterpret_cast<uchar4*>(tm)[g] = tq;
    }
  } else {
    for (int i = tid; i < n; i += 256) {
      const float p = mum[i];
      float x;
      unsigned char q;
      if (r8) {
        q = r8[i];
        x = fm_norm((float)q);
      } else {
        x = raw ? fm_norm(rf[i]) : rf[i];
        q = fm_quant(x);
      }
      const float dv = p - x;
      acc = acc + dv * dv;
      if (pm) pm[i] = fm_quant(p);
      if (tm) tm[i] = q;
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) sqerr[m] = ((part[0] + part[1]) + part[2]) + part[3];
}

extern "C" int dr_frame_metrics(const dr_dims* d, int B, int T, const float* mu, const dr_frames* truth,
                                float* sqerr, unsigned char* pred_u8, unsigned char* true_u8, hipStream_t s) {
  DR_REQUIRE(d && mu && truth && sqerr && B > 0 && T > 0, "null argument or empty batch");
  DR_REQUIRE((long long)B * T <= 0x7fffffffLL, "too many frames");
  const int vector = d->obs_dim > 0;
  DR_REQUIRE(!vector || (!pred_u8 && !true_u8), "vector observations have no u8 frames (pred_u8 / true_u8 must be NULL)");
  DR_REQUIRE(!vector || d->obs_dim <= 1023, "obs_dim > 1023");
  DR_REQUIRE(vector || (d->img_h > 0 && d->img_w > 0), "bad frame size");
  const long long n = vector ? d->obs_dim : 3LL * d->img_h * d->img_w;
  DR_REQUIRE(n <= 0x7fffffffLL, "frame too large");
  DR_REQUIRE(truth->t0 >= 0, "negative t0");
  if (truth->ring) DR_REQUIRE(truth->starts && truth->ring_cap > 0, "ring source needs starts and ring_cap");
  else DR_REQUIRE(truth->obs, "no truth frames");
  const auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  bool vec = n % 4 == 0 && al(mu, 16) && al(pred_u8, 4) && al(true_u8, 4);
  if (truth->ring) vec = vec && al(truth->ring, vector ? 16 : 4);
  else vec = vec && al(truth->obs, 16) && truth->stride_b % 4 == 0 && truth->stride_t % 4 == 0;
  const dim3 grid((unsigned)(B * T)), block(256);
  if (vec) hipLaunchKernelGGL(k_frame_metrics<true>, grid, block, 0, s, T, (int)n, vector, mu, *truth, sqerr, pred_u8, true_u8);
  else hipLaunchKernelGGL(k_frame_metrics<false>, grid, block, 0, s, T, (int)n, vector, mu, *truth, sqerr, pred_u8, true_u8);
  return dr_check_launch("frame_metrics");
}

// ---------------------------------------------------------------------------
// Sampled futures on replay windows (futures.py): SSIM of decoded frames and
// the mean / spread of M decoded futures, both against the ring's true frames.
// ---------------------------------------------------------------------------

// the true frame (b, t) of a dr_frames source (t0 included), as k_frame_metrics reads it
struct FmTruth {
  const unsigned char* r8;  // u8 ring frame, or nullptr
  const float* rf;          // f32 frame (the vector ring's row, or the f32 form)
  bool raw;                 // rf holds 0..255
};
__device__ __forceinline__ FmTruth fm_truth(const dr_frames& src, int b, int t, int n, int vector) {
  FmTruth f = {nullptr, nullptr, false};
  const int tt = t + src.t0;
  if (src.ring) {
    long long slot = (src.starts[b] + tt) % src.ring_cap;
    if (slot < 0) slot += src.ring_cap;
    if (vector) f.rf = reinterpret_cast<const float*>(src.ring) + slot * n;
    else f.r8 = src.ring + slot * n;
  } else {
    f.rf = src.obs + (long long)b * src.stride_b + (long long)tt * src.stride_t;
  }
  f.raw = !vector && src.raw255;
  return f;
}

// u8 of a per-element standard deviation: min(255, rint(255 sqrt(var)))
__device__ __forceinline__ unsigned char fm_quant_std(float var) {
  return (unsigned char)fminf(255.0f, rintf(255.0f * sqrtf(var)));
}

// SSIM window: g_k = exp(-(k - 5)^2 / 4.5), k = 0 .. 10, normalised to sum 1 in
// double and rounded to f32 once (the literals are those f32 values exactly)
__device__ constexpr float c_ssim_w[11] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f,
                                   0x1.b43c4p-3f,   0x1.10656p-2f,  0x1.b43c4p-3f,  0x1.bff0fep-4f,
                                   0x1.26eb18p-5f,  0x1.f1fe02p-8f, 0x1.0d956cp-10f};
#define SSIM_SH 8               // frame rows staged per strip (a multiple of 4: the 16-byte loads)
#define SSIM_RB (SSIM_SH + 10)  // rows of the ring of horizontally filtered rows
#define SSIM_MAX_LDS 65536

static inline size_t ssim_lds_bytes(int W) {
  return sizeof(float) * ((size_t)2 * SSIM_SH * W + (size_t)5 * SSIM_RB * (W - 10));
}

// One 256-thread workgroup per frame m = b*T + t; the three channels in turn.
// A channel goes through LDS in strips of SSIM_SH rows, each element read from
// global memory once (VEC: 16-byte loads of mu, 4-byte loads of four u8 pixels;
// the conditions are dr_frame_metrics' plus H*W % 4 == 0):
//   1. the strip's clamped predictions p and true values x -> sp, sx [SH][W];
//   2. the window along W, taps ascending, at the W - 10 valid columns of each
//      staged row: the five planes  sum w p, w x, w p^2, w x^2, w p x  go to
//      row (frame row % SSIM_RB) of the ring f[5][SSIM_RB][W - 10];
//   3. every output row o whose rows o .. o + 10 are now in the ring (o up to
//      strip end - 11; the ring keeps the last 10 rows of the strips before):
//      the window along H, taps ascending, then the map.
// Work items of 2 and 3 are (row, column) in row-major order, item tid, tid +
// 256, ...: a thread adds its map values in ascending position order over the
// whole channel; then wave_sum's tree, the four wave sums in wave order, the
// division by the number of positions; ssim = ((ch0 + ch1) + ch2) / 3.
// Nothing is shared between workgroups.
template <bool VEC>
__global__ __launch_bounds__(256) void k_frame_ssim(int T, int H, int W, const float* __restrict__ mu, dr_frames src,
                                                    float* __restrict__ ssim, float* __restrict__ ssim_ch) {
  extern __shared__ __align__(16) float ssim_lds[];
  __shared__ float part[4];
  __shared__ float chv[3];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int b = m / T, t = m - b * T;
  const int Wv = W - 10, Hv = H - 10;
  const int n = 3 * H * W;
  float* sp = ssim_lds;
  float* sx = sp + SSIM_SH * W;
  float* f = sx + SSIM_SH * W;
  const int plane = SSIM_RB * Wv;
  const float* mum = mu + (long long)m * n;
  const FmTruth tr = fm_truth(src, b, t, n, 0);
  const float C1 = 1e-4f, C2 = 9e-4f;
  for (int ch = 0; ch < 3; ++ch) {
    float acc = 0.0f;
    for (int r0 = 0; r0 < H; r0 += SSIM_SH) {
      const int rows = min(SSIM_SH, H - r0);
      const int cnt = rows * W;
      const int e0 = (ch * H + r0) * W;  // first element of the strip in the frame
      // 1. stage the strip (the previous strip's readers of sp / sx are past the second barrier)
      if (VEC) {
        for (int g = tid; g < (cnt >> 2); g += 256) {
          const float4 mv = reinterpret_cast<const float4*>(mum + e0)[g];
          float4 xv;
          if (tr.r8) {
            const uchar4 tq = reinterpret_cast<const uchar4*>(tr.r8 + e0)[g];
            xv = make_float4(fm_norm((float)tq.x), fm_norm((float)tq.y), fm_norm((float)tq.z), fm_norm((float)tq.w));
          } else {
            xv = reinterpret_cast<const float4*>(tr.rf + e0)[g];
            if (tr.raw) xv = make_float4(fm_norm(xv.x), fm_norm(xv.y), fm_norm(xv.z), fm_norm(xv.w));
          }
          reinterpret_cast<float4*>(sp)[g] = make_float4(fminf(0.5f, fmaxf(-0.5f, mv.x)), fminf(0.5f, fmaxf(-0.5f, mv.y)),
                                                         fminf(0.5f, fmaxf(-0.5f, mv.z)), fminf(0.5f, fmaxf(-0.5f, mv.w)));
          reinterpret_cast<float4*>(sx)[g] = xv;
        }
      } else {
        for (int i = tid; i < cnt; i += 256) {
          float x;
          if (tr.r8) x = fm_norm((float)tr.r8[e0 + i]);
          else x = tr.raw ? fm_norm(tr.rf[e0 + i]) : tr.rf[e0 + i];
          sp[i] = fminf(0.5f, fmaxf(-0.5f, mum[e0 + i]));
          sx[i] = x;
        }
      }
      __syncthreads();
      // 2. along W
      for (int i = tid; i < rows * Wv; i += 256) {
        const int r = i / Wv, c = i - r * Wv;
        const float* pr = sp + r * W + c;
        const float* xr = sx + r * W + c;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, s4 = 0.0f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const float w = c_ssim_w[k], p = pr[k], x = xr[k];
          s0 = s0 + w * p;
          s1 = s1 + w * x;
          s2 = s2 + w * (p * p);
          s3 = s3 + w * (x * x);
          s4 = s4 + w * (p * x);
        }
        float* fo = f + ((r0 + r) % SSIM_RB) * Wv + c;
        fo[0] = s0;
        fo[plane] = s1;
        fo[2 * plane] = s2;
        fo[3 * plane] = s3;
        fo[4 * plane] = s4;
      }
      __syncthreads();
      // 3. along H and the map, for the output rows completed by this strip
      const int o_lo = max(0, r0 - 10), o_hi = r0 + rows - 11;  // (inclusive; empty while fewer than 11 rows are in)
      for (int i = tid; i < (o_hi - o_lo + 1) * Wv; i += 256) {
        const int ro = i / Wv, c = i - ro * Wv;
        int slot = (o_lo + ro) % SSIM_RB;
        float mp = 0.0f, mx = 0.0f, spp = 0.0f, sxx = 0.0f, spx = 0.0f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
          const float w = c_ssim_w[k];
          const float* fi = f + slot * Wv + c;
          mp = mp + w * fi[0];
          mx = mx + w * fi[plane];
          spp = spp + w * fi[2 * plane];
          sxx = sxx + w * fi[3 * plane];
          spx = spx + w * fi[4 * plane];
          slot = slot + 1 == SSIM_RB ? 0 : slot + 1;
        }
        const float vp = spp - mp * mp, vx = sxx - mx * mx, cv = spx - mp * mx;
        const float up = mp + 0.5f, ux = mx + 0.5f;
        const float num = (2.0f * up * ux + C1) * (2.0f * cv + C2);
        const float den = (up * up + ux * ux + C1) * (vp + vx + C2);
        acc = acc + num / den;
      }
      // (the next strip's stage 2 writes the ring only after its first barrier, which every reader here reaches first)
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) chv[ch] = (((part[0] + part[1]) + part[2]) + part[3]) / (float)(Hv * Wv);
    __syncthreads();
  }
  if (tid == 0) {
    ssim[m] = ((chv[0] + chv[1]) + chv[2]) / 3.0f;
    if (ssim_ch) {
      ssim_ch[(long long)m * 3 + 0] = chv[0];
      ssim_ch[(long long)m * 3 + 1] = chv[1];
      ssim_ch[(long long)m * 3 + 2] = chv[2];
    }
  }
}

extern "C" int dr_frame_ssim(const dr_dims* d, int B, int T, const float* mu, const dr_frames* truth, float* ssim,
                             float* ssim_ch, hipStream_t s) {
  DR_REQUIRE(d && mu && truth && ssim && B > 0 && T > 0, "null argument or empty batch");
  DR_REQUIRE((long long)B * T <= 0x7fffffffLL, "too many frames");
  DR_REQUIRE(d->obs_dim == 0, "SSIM needs pixel observations (obs_dim > 0 is a vector model)");
  DR_REQUIRE(d->img_h > 0 && d->img_w > 0, "bad frame size");
  const int H = d->img_h, W = d->img_w;
  DR_REQUIRE(3LL * H * W <= 0x7fffffffLL, "frame too large");
  DR_REQUIRE(truth->t0 >= 0, "negative t0");
  if (truth->ring) DR_REQUIRE(truth->starts && truth->ring_cap > 0, "ring source needs starts and ring_cap");
  else DR_REQUIRE(truth->obs, "no truth frames");
  if (H < 11 || W < 11) {
    dr_set_error("%s: frames of %d x %d are smaller than the 11 x 11 window", __func__, H, W);
    return DR_E_UNSUPPORTED;
  }
  const size_t lds = ssim_lds_bytes(W);
  if (lds > SSIM_MAX_LDS) {
    dr_set_error("%s: a strip of %d-pixel rows needs %zu bytes of LDS (limit %d)", __func__, W, lds, SSIM_MAX_LDS);
    return DR_E_UNSUPPORTED;
  }
  const auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  bool vec = ((long long)H * W) % 4 == 0 && al(mu, 16);
  if (truth->ring) vec = vec && al(truth->ring, 4);
  else vec = vec && al(truth->obs, 16) && truth->stride_b % 4 == 0 && truth->stride_t % 4 == 0;
  const dim3 grid((unsigned)(B * T)), block(256);
  if (vec) hipLaunchKernelGGL(k_frame_ssim<true>, grid, block, lds, s, T, H, W, mu, *truth, ssim, ssim_ch);
  else hipLaunchKernelGGL(k_frame_ssim<false>, grid, block, lds, s, T, H, W, mu, *truth, ssim, ssim_ch);
  return dr_check_launch("frame_ssim");
}

// Mean and spread of M decoded futures per window: one 256-thread workgroup
// per (b, t); sample m's frame is row (b*M + m)*T + t of mu.  Elements go to
// threads as in k_frame_metrics (VEC: 4-element groups tid, tid + 256, ...;
// else elements tid, tid + 256, ...), per element
//   mean = (sum_m mu_m) / (float)M            (m ascending from 0.0f)
//   var  = (sum_m (mu_m - mean)^2) / (float)M (a second pass over the M values)
// and the two frame sums -- (mean - x)^2 and var -- are reduced as sqerr is
// there.  M = 1: mean == mu and var == 0 exactly, so sqerr_mean is
// k_frame_metrics' sqerr bit for bit (same VEC class).
template <bool VEC>
__global__ __launch_bounds__(256) void k_ensemble_metrics(int Ms, int T, int n, int vector,
                                                          const float* __restrict__ mu, dr_frames src,
                                                          float* __restrict__ sqerr_mean, float* __restrict__ spread,
                                                          unsigned char* __restrict__ mean_u8,
                                                          unsigned char* __restrict__ std_u8,
                                                          float* __restrict__ mean_f32) {
  __shared__ float part[2][4];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int b = w / T, t = w - b * T;
  const FmTruth tr = fm_truth(src, b, t, n, vector);
  const float* mu0 = mu + ((long long)b * Ms * T + t) * n;  // sample 0; sample m is m * T * n further
  const long long sm = (long long)T * n;
  unsigned char* mq = mean_u8 ? mean_u8 + (long long)w * n : nullptr;
  unsigned char* sq = std_u8 ? std_u8 + (long long)w * n : nullptr;
  float* mf = mean_f32 ? mean_f32 + (long long)w * n : nullptr;
  const float fM = (float)Ms;
  float a_err = 0.0f, a_var = 0.0f;
  if (VEC) {
    for (int g = tid; g < (n >> 2); g += 256) {
      float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      for (int k = 0; k < Ms; ++k) {
        const float4 v = reinterpret_cast<const float4*>(mu0 + k * sm)[g];
        sum[0] = sum[0] + v.x; sum[1] = sum[1] + v.y; sum[2] = sum[2] + v.z; sum[3] = sum[3] + v.w;
      }
      float mean[4], var[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int e = 0; e < 4; ++e) mean[e] = sum[e] / fM;
      for (int k = 0; k < Ms; ++k) {
        const float4 v = reinterpret_cast<const float4*>(mu0 + k * sm)[g];
        const float dv[4] = {v.x - mean[0], v.y - mean[1], v.z - mean[2], v.w - mean[3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) var[e] = var[e] + dv[e] * dv[e];
      }
      float x[4];
      if (tr.r8) {
        const uchar4 tq = reinterpret_cast<const uchar4*>(tr.r8)[g];
        x[0] = fm_norm((float)tq.x); x[1] = fm_norm((float)tq.y);
        x[2] = fm_norm((float)tq.z); x[3] = fm_norm((float)tq.w);
      } else {
        const float4 fv = reinterpret_cast<const float4*>(tr.rf)[g];
        const float v[4] = {fv.x, fv.y, fv.z, fv.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = tr.raw ? fm_norm(v[e]) : v[e];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        var[e] = var[e] / fM;
        const float dv = mean[e] - x[e];
        a_err = a_err + dv * dv;
        a_var = a_var + var[e];
      }
      if (mq) reinterpret_cast<uchar4*>(mq)[g] = make_uchar4(fm_quant(mean[0]), fm_quant(mean[1]), fm_quant(mean[2]),
                                                              fm_quant(mean[3]));
      if (sq) reinterpret_cast<uchar4*>(sq)[g] = make_uchar4(fm_quant_std(var[0]), fm_quant_std(var[1]),
                                                              fm_quant_std(var[2]), fm_quant_std(var[3]));
      if (mf) reinterpret_cast<float4*>(mf)[g] = make_float4(mean[0], mean[1], mean[2], mean[3]);
    }
  } else {
    for (int i = tid; i < n; i += 256) {
      float sum = 0.0f;
      for (int k = 0; k < Ms; ++k) sum = sum + mu0[k * sm + i];
      const float mean = sum / fM;
      float var = 0.0f;
      for (int k = 0; k < Ms; ++k) {
        const float dv = mu0[k * sm + i] - mean;
        var = var + dv * dv;
      }
      var = var / fM;
      float x;
      if (tr.r8) x = fm_norm((float)tr.r8[i]);
      else x = tr.raw ? fm_norm(tr.rf[i]) : tr.rf[i];
      const float dv = mean - x;
      a_err = a_err + dv * dv;
      a_var = a_var + var;
      if (mq) mq[i] = fm_quant(mean);
      if (sq) sq[i] = fm_quant_std(var);
      if (mf) mf[i] = mean;
    }
  }
  a_err = wave_sum(a_err);
  a_var = wave_sum(a_var);
  if ((tid & 63) == 0) {
    part[0][tid >> 6] = a_err;
    part[1][tid >> 6] = a_var;
  }
  __syncthreads();
  if (tid == 0) {
    sqerr_mean[w] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    spread[w] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
  }
}

extern "C" int dr_ensemble_metrics(const dr_dims* d, int B, int M, int T, const float* mu, const dr_frames* truth,
                                   float* sqerr_mean, float* spread, unsigned char* mean_u8, unsigned char* std_u8,
                                   float* mean_f32, hipStream_t s) {
  DR_REQUIRE(d && mu && truth && sqerr_mean && spread && B > 0 && T > 0, "null argument or empty batch");
  DR_REQUIRE(M >= 1 && M <= 64, "need 1 <= M <= 64");
  DR_REQUIRE((long long)B * M * T <= 0x7fffffffLL, "too many frames");
  const int vector = d->obs_dim > 0;
  DR_REQUIRE(!vector || (!mean_u8 && !std_u8), "vector observations have no u8 frames (mean_u8 / std_u8 must be NULL)");
  DR_REQUIRE(!vector || d->obs_dim <= 1023, "obs_dim > 1023");
  DR_REQUIRE(vector || (d->img_h > 0 && d->img_w > 0), "bad frame size");
  const long long n = vector ? d->obs_dim : 3LL * d->img_h * d->img_w;
  DR_REQUIRE(n <= 0x7fffffffLL, "frame too large");
  DR_REQUIRE(truth->t0 >= 0, "negative t0");
  if (truth->ring) DR_REQUIRE(truth->starts && truth->ring_cap > 0, "ring source needs starts and ring_cap");
  else DR_REQUIRE(truth->obs, "no truth frames");
  const auto al = [](const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; };
  bool vec = n % 4 == 0 && al(mu, 16) && al(mean_u8, 4) && al(std_u8, 4) && al(mean_f32, 16);
  if (truth->ring) vec = vec && al(truth->ring, vector ? 16 : 4);
  else vec = vec && al(truth->obs, 16) && truth->stride_b % 4 == 0 && truth->stride_t % 4 == 0;
  const dim3 grid((unsigned)(B * T)), block(256);
  if (vec) hipLaunchKernelGGL(k_ensemble_metrics<true>, grid, block, 0, s, M, T, (int)n, vector, mu, *truth, sqerr_mean,
                              spread, mean_u8, std_u8, mean_f32);
  else hipLaunchKernelGGL(k_ensemble_metrics<false>, grid, block, 0, s, M, T, (int)n, vector, mu, *truth, sqerr_mean,
                          spread, mean_u8, std_u8, mean_f32);
  return dr_check_launch("ensemble_metrics");
}

// ---------------------------------------------------------------------------
// Latent statistics of the posterior trace: per row m of [M][R][C] raw logits
// (no unimix, as the loss takes them, WorldModel.py:175-181)
//   kl[m]            = sum_r KL(Cat(logits = post[m][r]) || Cat(logits = prior[m][r]))
//   post_entropy[m]  = sum_r H(softmax post[m][r]),  prior_entropy[m] likewise
// (torch.distributions.kl._kl_categorical_categorical: t = p (lp - lq), p = exp(lp)).
//
// One 256-thread workgroup per row.  A group of C classes sits on W aligned
// lanes (W a power of two, wave-uniform), E consecutive classes per lane:
// E = 4 with one 16-byte load per lane and logits array (C % 4 == 0 and 16-byte
// aligned bases: at R = C = 32 the 256 lanes read the whole row in one pass),
// E = 1 otherwise.  256 / W groups per pass, passes in ascending group order.
// Within a group: the lane's E terms in class order, then group_sum's fixed
// DPP tree.  Over the groups: lane 0 of each group keeps a running sum over
// the passes, the 64 lane sums go through wave_sum's tree and the four wave
// sums through LDS in wave order.  Nothing is shared between workgroups, so a
// row has the same bits at every M and position, and from run to run.
// ---------------------------------------------------------------------------
struct LsGroup {
  float lp[4];  // log-probabilities of the lane's classes
  float ent;    // -sum p lp over the group (every lane of the group holds it)
};

// max-subtracted log-softmax of one group spread over W lanes; inactive lanes
// (padding classes, padding groups) carry -inf and add exactly 0
template <int E>
__device__ __forceinline__ LsGroup ls_group(const float (&x)[4], bool act, int W) {
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < E; ++e) mx = fmaxf(mx, act ? x[e] : -INFINITY);
  mx = group_max(mx, W);
  float se = 0.0f;
#pragma unroll
  for (int e = 0; e < E; ++e) se = se + (act ? expf(x[e] - mx) : 0.0f);
  se = group_sum(se, W);
  // lp = (x - max) - log(sum): two groups whose logits differ by a constant get
  // the same bits (all-equal logits: lp = -log C in both, KL exactly 0)
  const float ls = logf(se);
  LsGroup g;
  float h = 0.0f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    g.lp[e] = (x[e] - mx) - ls;
    const float p = expf(g.lp[e]);
    // a class whose p underflowed adds exactly 0 (never 0 * inf)
    h = h + ((act && p > 0.0f) ? p * g.lp[e] : 0.0f);
  }
  g.ent = -group_sum(h, W);
  return g;
}

template <int E>
__global__ __launch_bounds__(256) void k_latent_stats(int R, int C, int W, const float* __restrict__ post,
                                                      const float* __restrict__ prior, float* __restrict__ kl,
                                                      float* __restrict__ post_ent, float* __restrict__ prior_ent,
                                                      float* __restrict__ kl_groups) {
  __shared__ float part[3][4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int gpp = 256 / W;               // groups per pass
  const int gl = tid / W, j = tid - gl * W;  // group of the pass, lane of the group
  const float* qm = post + (long long)m * R * C;
  const float* pm = prior ? prior + (long long)m * R * C : nullptr;
  float a_kl = 0.0f, a_hq = 0.0f, a_hp = 0.0f;
  for (int r0 = 0; r0 < R; r0 += gpp) {  // uniform trip count: every lane takes part in the DPP reductions
    const int r = r0 + gl;
    const bool act = r < R && j * E < C;
    float xq[4] = {0.0f, 0.0f, 0.0f, 0.0f}, xp[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (act) {
      const long long o = (long long)r * C + j * E;
      if (E == 4) {
        const float4 v = *reinterpret_cast<const float4*>(qm + o);
        xq[0] = v.x; xq[1] = v.y; xq[2] = v.z; xq[3] = v.w;
        if (pm) {
          const float4 u = *reinterpret_cast<const float4*>(pm + o);
          xp[0] = u.x; xp[1] = u.y; xp[2] = u.z; xp[3] = u.w;
        }
      } else {
        xq[0] = qm[o];
        if (pm) xp[0] = pm[o];
      }
    }
    const LsGroup gq = ls_group<E>(xq, act, W);
    float g_kl = 0.0f, g_hp = 0.0f;
    if (pm) {  // (uniform over the workgroup)
      const LsGroup gp = ls_group<E>(xp, act, W);
      float t = 0.0f;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const float p = expf(gq.lp[e]);
        t = t + ((act && p > 0.0f) ? p * (gq.lp[e] - gp.lp[e]) : 0.0f);
      }
      g_kl = group_sum(t, W);
      g_hp = gp.ent;
    }
    if (j == 0 && r < R) {
      a_kl = a_kl + g_kl;
      a_hq = a_hq + gq.ent;
      a_hp = a_hp + g_hp;
      if (kl_groups) kl_groups[(long long)m * R + r] = g_kl;
    }
  }
  a_kl = wave_sum(a_kl);
  a_hq = wave_sum(a_hq);
  a_hp = wave_sum(a_hp);
  if ((tid & 63) == 0) {
    part[0][tid >> 6] = a_kl;
    part[1][tid >> 6] = a_hq;
    part[2][tid >> 6] = a_hp;
  }
  __syncthreads();
  if (tid == 0) {
    post_ent[m] = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
    if (pm) {
      kl[m] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
      prior_ent[m] = ((part[2][0] + part[2][1]) + part[2][2]) + part[2][3];
    }
  }
}

extern "C" int dr_latent_stats(int M, int R, int C, const float* post_logits, const float* prior_logits, float* kl,
                               float* post_entropy, float* prior_entropy, float* kl_groups, hipStream_t s) {
  DR_REQUIRE(M >= 0 && R >= 1 && C >= 1 && C <= 64, "need M >= 0, R >= 1 and 1 <= C <= 64");
  DR_REQUIRE((long long)M * R * C <= 0x7fffffffLL * 64, "too many logits");
  DR_REQUIRE(post_logits && post_entropy, "post_logits and post_entropy are required");
  if (prior_logits) DR_REQUIRE(kl && prior_entropy, "kl and prior_entropy are required with prior_logits");
  else DR_REQUIRE(!kl && !prior_entropy && !kl_groups, "kl, prior_entropy and kl_groups need prior_logits");
  if (M == 0) return DR_OK;
  const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool v4 = C % 4 == 0 && al16(post_logits) && al16(prior_logits);
  const int per = v4 ? C / 4 : C;  // lanes a group needs
  int W = 1;
  while (W < per) W <<= 1;
  const dim3 grid((unsigned)M), block(256);
  if (v4) hipLaunchKernelGGL(k_latent_stats<4>, grid, block, 0, s, R, C, W, post_logits, prior_logits, kl, post_entropy,
                             prior_entropy, kl_groups);
  else hipLaunchKernelGGL(k_latent_stats<1>, grid, block, 0, s, R, C, W, post_logits, prior_logits, kl, post_entropy,
                          prior_entropy, kl_groups);
  return dr_check_launch("latent_stats");
}

// ---------------------------------------------------------------------------
// Agent trace on replay windows (agent_trace.py): the per-row statistics the
// loss kernels keep to themselves (k_critic_ce, k_actor_loss_grad in ops.hip emit
// means and gradients only), and the return recursion on the ring's windows.
// Three one-shot kernels: nothing is shared between workgroups, no atomics.
// ---------------------------------------------------------------------------

// Lambda returns on real rewards (Agent.py:156-172 with H = T - 1): one thread
// per window, k_lambda_returns' expressions in its order.  Rewards / continues
// are rows of [B][S] windows (row strides rew_sb / cont_sb, entries 0 .. T-2
// read); symlog != 0: the stored symlog reward goes through dr_symexp first
// (DreamerUtils.py:35-37).  R_mc is the same recursion at lam = 1, lam_c = 0
// (the expression is kept whole, so finite V give dr_lambda_returns(lam = 1)'s
// bits); td[t] = (r_t + (gamma c_t) V_{t+1}) - V_t.
__global__ __launch_bounds__(64) void k_replay_returns(int B, int T, const float* __restrict__ rew, long long rew_sb,
                                                       const float* __restrict__ cont, long long cont_sb, int symlog,
                                                       const float* __restrict__ V, float gamma, float lam, float lam_c,
                                                       float* __restrict__ Rl, float* __restrict__ Rmc,
                                                       float* __restrict__ td) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int H = T - 1;
  const float* rb = rew + (long long)b * rew_sb;
  const float* cb = cont + (long long)b * cont_sb;
  const float* vb = V + (long long)b * T;
  float* Rb = Rl + (long long)b * H;
  float* Mb = Rmc ? Rmc + (long long)b * H : nullptr;
  float* Db = td ? td + (long long)b * H : nullptr;
  float nxt = 0.0f, mc = 0.0f;
  for (int t = H - 1; t >= 0; --t) {
    const float r = symlog ? dr_symexp(rb[t]) : rb[t];
    const float gc = gamma * cb[t];
    const float v1 = vb[t + 1];
    const float boot = r + gc * v1;  // the last step's return, and the one-step target
    float v, m;
    if (t == H - 1) {
      v = boot;
      m = boot;
    } else {
      v = r + gc * ((lam_c * v1) + (lam * nxt));
      m = r + gc * ((0.0f * v1) + (1.0f * mc));
    }
    Rb[t] = v;
    if (Mb) Mb[t] = m;
    if (Db) Db[t] = boot - vb[t];
    nxt = v;
    mc = m;
  }
}

extern "C" int dr_replay_returns(int B, int T, const float* rewards, long long rew_sb, const float* continues,
                                 long long cont_sb, int rewards_symlog, const float* V, float gamma, float lam,
                                 float* R_lambda, float* R_mc, float* td, hipStream_t s) {
  DR_REQUIRE(B >= 0 && T >= 2, "need B >= 0 and T >= 2");
  DR_REQUIRE((long long)B * T <= 0x7fffffffLL, "too many rows");
  DR_REQUIRE(rew_sb >= T - 1 && cont_sb >= T - 1, "window row strides must be >= T - 1");
  DR_REQUIRE(rewards && continues && V && R_lambda, "rewards, continues, V and R_lambda are required");
  if (B == 0) return DR_OK;
  const float lam_c = (float)(1.0 - (double)lam);
  hipLaunchKernelGGL(k_replay_returns, dim3(dr_cdiv(B, 64)), dim3(64), 0, s, B, T, rewards, rew_sb, continues, cont_sb,
                     rewards_symlog, V, gamma, lam, lam_c, R_lambda, R_mc, td);
  return dr_check_launch("replay_returns");
}

// Per-row statistics of a bucket head's logits (rows m = b*T + t, row stride
// ldl): entropy H(softmax l), the spread sqrt(sum p (b - sum p b)^2) in bucket
// (symlog) units, and -- rows t < Tt -- the two-hot cross-entropy against
// symlog(target[b][t]) (Agent.py:127-135, to_twohot of DreamerUtils.py:39-50 with
// its clamps and the 1e-8; k_critic_ce's row convention, the weights in double).
// One wave per row, four rows per workgroup, like k_bucket_value.  Every sum:
// the lane's classes lane, lane + 64, ... in ascending order, then wave_sum's
// tree.  log-probabilities are (l - max) - log(sum exp(l - max)); a class whose
// probability underflowed adds exactly 0 to the entropy.  The spread takes two
// passes: the mean first, then the squared deviations.
__global__ __launch_bounds__(256) void k_value_stats(int M, int T, int Tt, int nb, const float* __restrict__ logits,
                                                     long long ldl, const float* __restrict__ buckets,
                                                     const float* __restrict__ target, float* __restrict__ entropy,
                                                     float* __restrict__ spread, float* __restrict__ ce) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;  // (whole waves leave: every lane of a working wave takes part in the DPP reductions)
  const int b = row / T, t = row - b * T;
  const float* l = logits + (long long)row * ldl;
  float mx = -INFINITY;
  for (int k = lane; k < nb; k += 64) mx = fmaxf(mx, l[k]);
  mx = wave_max(mx);
  float se = 0.0f;
  for (int k = lane; k < nb; k += 64) se = se + expf(l[k] - mx);
  se = wave_sum(se);
  const float lse = logf(se);
  if (entropy || spread) {
    float h = 0.0f, mean = 0.0f;
    for (int k = lane; k < nb; k += 64) {
      const float lp = (l[k] - mx) - lse;
      const float p = expf(lp);
      h = h + (p > 0.0f ? p * lp : 0.0f);  // never 0 * -inf
      mean = mean + p * buckets[k];
    }
    h = wave_sum(h);
    mean = wave_sum(mean);
    if (entropy && lane == 0) entropy[row] = -h;
    if (spread) {
      float var = 0.0f;
      for (int k = lane; k < nb; k += 64) {
        const float p = expf((l[k] - mx) - lse);
        const float dv = buckets[k] - mean;
        var = var + p * (dv * dv);
      }
      var = wave_sum(var);
      if (lane == 0) spread[row] = sqrtf(var);
    }
  }
  if (t < Tt) {  // (Tt > 0 only with target and ce)
    // The two-hot weights in double: an error of one f32 step in symlog(R) moves
    // w by step / (bucket spacing) and the loss by that times the gap between the
    // two neighbouring log-probabilities -- with 255 buckets ten f32 steps of the
    // loss, where k_critic_ce's f32 weights only have to serve a mean.  One
    // double log per row.
    const double x = (double)target[(long long)b * Tt + t];
    double v = log1p(fabs(x));
    v = x < 0.0 ? -v : v;  // (symlog(0) = 0 either way; NaN falls to the first bucket as in k_critic_ce)
    v = fmin(fmax(v, (double)buckets[0]), (double)buckets[nb - 1]);
    int cnt = 0;
    for (int k = lane; k < nb; k += 64) cnt += ((double)buckets[k] <= v) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    int lo = cnt - 1;
    if (lo > nb - 2) lo = nb - 2;
    if (lo < 0) lo = 0;  // ascending buckets never get here; keeps the reads in bounds for any others
    const double blo = (double)buckets[lo], bhi = (double)buckets[lo + 1];
    const double wd = (v - blo) / (bhi - blo + 1e-8);
    const float w = (float)wd, wlo = (float)(1.0 - wd);
    if (lane == 0) {
      const float ls_lo = (l[lo] - mx) - lse, ls_hi = (l[lo + 1] - mx) - lse;
      ce[(long long)b * Tt + t] = -(wlo * ls_lo + w * ls_hi);
    }
  }
}

extern "C" int dr_value_stats(int B, int T, int Tt, int nb, const float* logits, long long ldl, const float* buckets,
                              const float* target, float* entropy, float* std_symlog, float* ce, hipStream_t s) {
  DR_REQUIRE(B >= 0 && T >= 1 && Tt >= 0 && Tt <= T, "need B >= 0, T >= 1 and 0 <= Tt <= T");
  DR_REQUIRE(nb >= 2 && nb <= 1024, "need 2 <= nb <= 1024");
  DR_REQUIRE(ldl >= nb, "ldl < nb");
  DR_REQUIRE((long long)B * T <= 0x7fffffffLL, "too many rows");
  DR_REQUIRE(logits && buckets, "logits and buckets are required");
  DR_REQUIRE((target != nullptr) == (ce != nullptr), "target and ce are both NULL or both given");
  DR_REQUIRE((Tt > 0) == (target != nullptr), "target and ce go with Tt > 0 (Tt = 0: both NULL)");
  DR_REQUIRE(entropy || std_symlog || ce, "no output requested");
  const int M = B * T;
  if (M == 0) return DR_OK;
  hipLaunchKernelGGL(k_value_stats, dim3(dr_cdiv(M, 4)), dim3(256), 0, s, M, T, Tt, nb, logits, ldl, buckets, target,
                     entropy, std_symlog, ce);
  return dr_check_launch("value_stats");
}

// log-probability of the recorded action under the current actor (Agent.py:110-115):
// per dimension, TransformedDistribution(Normal(mu, sigma), TanhTransform).log_prob at
// y = clamp(a, +-(1 - 1e-6)) (the clamp in f32, so +-1 stays finite):
//   x = atanh(y);  -(x-mu)^2/(2 sigma^2) - log sigma - log sqrt(2 pi) - 2 (log 2 - x - softplus(-2x))
// k_actor_loss_grad's expressions.  One thread per row (b, t) adds the A terms
// in ascending order from 0.0f; base_entropy = sum_i ((1/2 + 1/2 log 2 pi) + log sigma_i)
// likewise (the Normal's entropy: the policy's, less the tanh correction).
__global__ __launch_bounds__(128) void k_action_logprob(int M, int T, int A, const float* __restrict__ mus,
                                                        const float* __restrict__ sigmas,
                                                        const float* __restrict__ actions, long long act_sb,
                                                        long long act_st, float* __restrict__ logp,
                                                        float* __restrict__ logp_dims, float* __restrict__ base_ent) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // (b,t)
  if (i >= M) return;
  const int b = i / T, t = i - b * T;
  const float* a = actions + (long long)b * act_sb + (long long)t * act_st;
  const float HALF_LOG_2PI = 0.91893853320467274178f;  // math.log(math.sqrt(2*math.pi))
  const float LOG2 = 0.69314718055994530942f;
  const float ENT0 = 1.41893853320467274178f;  // 1/2 + 1/2 log(2 pi)
  float acc = 0.0f, ent = 0.0f;
  for (int k = 0; k < A; ++k) {
    const long long o = (long long)i * A + k;
    const float y = fminf(fmaxf(a[k], -1.0f + 1e-6f), 1.0f - 1e-6f);
    const float x = atanhf(y);
    const float mu = mus[o], sg = sigmas[o];
    const float d = x - mu;
    const float var = sg * sg;
    const float lsg = logf(sg);
    const float lp = -(d * d) / (2.0f * var) - lsg - HALF_LOG_2PI;
    const float ladj = 2.0f * (LOG2 - x - dr_softplus(-2.0f * x));
    const float term = lp - ladj;
    if (logp_dims) logp_dims[o] = term;
    acc = acc + term;
    ent = ent + (ENT0 + lsg);
  }
  logp[i] = acc;
  if (base_ent) base_ent[i] = ent;
}

extern "C" int dr_action_logprob(int B, int T, int A, const float* mu, const float* sigma, const float* actions,
                                 long long act_sb, long long act_st, float* logp, float* logp_dims, float* base_entropy,
                                 hipStream_t s) {
  DR_REQUIRE(B >= 0 && T >= 1 && A >= 1, "need B >= 0, T >= 1 and A >= 1");
  DR_REQUIRE((long long)B * T <= 0x7fffffffLL, "too many rows");
  DR_REQUIRE(act_sb >= 0 && act_st >= 0, "negative action stride");
  DR_REQUIRE(mu && sigma && actions && logp, "mu, sigma, actions and logp are required");
  const int M = B * T;
  if (M == 0) return DR_OK;
  hipLaunchKernelGGL(k_action_logprob, dim3(dr_cdiv(M, 128)), dim3(128), 0, s, M, T, A, mu, sigma, actions, act_sb,
                     act_st, logp, logp_dims, base_entropy);
  return dr_check_launch("action_logprob");
}
