// Metrics of the world-model diagnostics (open-loop prediction, posterior
// trace).  Frame metrics: decoded frames against
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
