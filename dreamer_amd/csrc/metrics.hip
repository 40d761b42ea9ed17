// Frame metrics of the open-loop prediction diagnostic: decoded frames against
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
