// Dream trace (dream_trace.py): the per-dream and per-window statistics of
// imagined rollouts under the actor -- what train_Agent learns from
// (Dreamer.py:143-175, Agent.py:96-135) -- in one launch, and the actor's N(0,1)
// draws written out.  Nothing is shared between workgroups, no atomics, no
// waits.  f32, built with -ffp-contract=off like the other elementwise code, so
// the host reproduces every expression in its order.
#include "ops.h"

// One 256-thread workgroup per window b; its M dreams are rows n0 .. n0+M-1, n0 = b*M.
//  1. thread m < M: the return recursions of dream m backwards over t
//     (k_replay_returns' expressions at rewards_symlog = 0, i.e. k_lambda_returns'),
//     the advantages, then the discount weights forwards.
//  2. every thread: the (m, t) pairs tid, tid + 256, ... -- k_action_logprob's row sum
//     and the saturation count.
//  3. after one barrier, thread t (t, t + 256, ...) reduces step t over m = 0 .. M-1
//     in ascending order; thread 255 ranks the dreams by R_mc[.][0].
// What step 3 reads of steps 1 and 2 sits in LDS as [t][m] with the odd row
// stride MP = M | 1 (writes by m and reads by t are both free of bank
// conflicts): R_lambda H rows, logp H rows, weight H + 1 rows, R_mc[.][0] one
// row -- (3H + 2) MP floats.  All of it is computed whatever outputs are asked
// for, so a NULL output changes no other output's bits.
struct DreamStatsArgs {
  int M, H, A;
  const float *rewards, *continues, *Vt, *Vo, *mus, *sigmas, *actions, *norm;
  float gamma, lam, lam_c, sat;
  dr_dream_outputs o;
};

// mean and population variance of x[0], x[stride], ..., M terms in ascending order, two passes
__device__ __forceinline__ void dream_mean_var(const float* x, long long stride, int M, float& mean, float& var) {
  float s = 0.0f;
  for (int m = 0; m < M; ++m) s = s + x[m * stride];
  mean = s / (float)M;
  float v = 0.0f;
  for (int m = 0; m < M; ++m) {
    const float d = x[m * stride] - mean;
    v = v + d * d;
  }
  var = v / (float)M;
}

__global__ __launch_bounds__(256) void k_dream_stats(DreamStatsArgs a) {
  extern __shared__ float sm[];
  const int M = a.M, H = a.H, A = a.A, MP = M | 1;
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long n0 = (long long)b * M;
  float* sRl = sm;                // [H][MP]
  float* sLp = sRl + H * MP;      // [H][MP]
  float* sW = sLp + H * MP;       // [H+1][MP]
  float* sMc = sW + (H + 1) * MP; // [MP]
  const dr_dream_outputs& o = a.o;

  if (tid < M) {
    const long long n = n0 + tid;
    const float* rb = a.rewards + n * H;
    const float* cb = a.continues + n * H;
    const float* vb = a.Vt + n * (H + 1);
    const float* vo = a.Vo + n * (H + 1);
    const float nrm = a.norm ? a.norm[0] : 1.0f;
    float nxt = 0.0f, mc = 0.0f;
    for (int t = H - 1; t >= 0; --t) {
      const float r = rb[t];
      const float gc = a.gamma * cb[t];
      const float v1 = vb[t + 1];
      const float boot = r + gc * v1;
      float v, m;
      if (t == H - 1) {
        v = boot;
        m = boot;
      } else {
        v = r + gc * ((a.lam_c * v1) + (a.lam * nxt));
        m = r + gc * ((0.0f * v1) + (1.0f * mc));
      }
      const float adv = v - vo[t];
      if (o.R_lambda) o.R_lambda[n * H + t] = v;
      if (o.R_mc) o.R_mc[n * H + t] = m;
      if (o.adv) o.adv[n * H + t] = adv;
      if (o.adv_norm) o.adv_norm[n * H + t] = adv / nrm;
      sRl[t * MP + tid] = v;
      nxt = v;
      mc = m;
    }
    sMc[tid] = mc;
    float w = 1.0f;
    for (int t = 0; t <= H; ++t) {
      if (o.weight) o.weight[n * (H + 1) + t] = w;
      sW[t * MP + tid] = w;
      if (t < H) w = w * (a.gamma * cb[t]);
    }
  }

  const float HALF_LOG_2PI = 0.91893853320467274178f;  // k_action_logprob's constants
  const float LOG2 = 0.69314718055994530942f;
  const float ENT0 = 1.41893853320467274178f;
  for (int i = tid; i < M * H; i += 256) {
    const int m = i / H, t = i - m * H;
    const long long row = n0 * H + i;  // (n0 + m) * H + t
    const float* ar = a.actions + row * A;
    float acc = 0.0f, ent = 0.0f;
    int nsat = 0;
    for (int k = 0; k < A; ++k) {
      const long long e = row * A + k;
      const float y = fminf(fmaxf(ar[k], -1.0f + 1e-6f), 1.0f - 1e-6f);
      const float x = atanhf(y);
      const float mu = a.mus[e], sg = a.sigmas[e];
      const float d = x - mu;
      const float var = sg * sg;
      const float lsg = logf(sg);
      const float lp = -(d * d) / (2.0f * var) - lsg - HALF_LOG_2PI;
      const float ladj = 2.0f * (LOG2 - x - dr_softplus(-2.0f * x));
      const float term = lp - ladj;
      acc = acc + term;
      ent = ent + (ENT0 + lsg);
      nsat += (fabsf(ar[k]) >= a.sat) ? 1 : 0;
    }
    if (o.logp) o.logp[row] = acc;
    if (o.base_entropy) o.base_entropy[row] = ent;
    if (o.saturated) o.saturated[row] = nsat;
    sLp[t * MP + m] = acc;
  }
  __syncthreads();

  for (int t = tid; t <= H; t += 256) {
    if (o.alive) {
      float s = 0.0f;
      for (int m = 0; m < M; ++m) s = s + sW[t * MP + m];
      o.alive[(long long)b * (H + 1) + t] = s / (float)M;
    }
    if (t == H) break;
    const long long bt = (long long)b * H + t;
    float mean, var;
    if (o.reward_mean || o.reward_std) {
      dream_mean_var(a.rewards + n0 * H + t, H, M, mean, var);
      if (o.reward_mean) o.reward_mean[bt] = mean;
      if (o.reward_std) o.reward_std[bt] = sqrtf(var);
    }
    if (o.ret_mean || o.ret_std) {
      dream_mean_var(sRl + t * MP, 1, M, mean, var);
      if (o.ret_mean) o.ret_mean[bt] = mean;
      if (o.ret_std) o.ret_std[bt] = sqrtf(var);
    }
    if (o.logp_mean || o.logp_std) {
      dream_mean_var(sLp + t * MP, 1, M, mean, var);
      if (o.logp_mean) o.logp_mean[bt] = mean;
      if (o.logp_std) o.logp_std[bt] = sqrtf(var);
    }
    if (o.action_spread) {
      float s = 0.0f;
      for (int k = 0; k < A; ++k) {
        dream_mean_var(a.actions + (n0 * H + t) * A + k, (long long)H * A, M, mean, var);
        s = s + var;
      }
      o.action_spread[bt] = sqrtf(s / (float)A);
    }
  }

  if (tid == 255 && (o.best || o.worst || o.n_finite)) {
    int nf = 0, bi = 0, wi = 0;
    float bv = 0.0f, wv = 0.0f;
    for (int m = 0; m < M; ++m) {
      const float v = sMc[m];
      if (!(fabsf(v) <= 3.402823466e+38f)) continue;  // NaN, +-Inf
      if (nf == 0 || v > bv) {
        bv = v;
        bi = m;
      }
      if (nf == 0 || v < wv) {
        wv = v;
        wi = m;
      }
      ++nf;
    }
    if (o.best) o.best[b] = bi;
    if (o.worst) o.worst[b] = wi;
    if (o.n_finite) o.n_finite[b] = nf;
  }
}

extern "C" int dr_dream_stats(int B, int M, int H, int A, const float* rewards, const float* continues,
                              const float* V_target, const float* V_online, const float* mus, const float* sigmas,
                              const float* actions, float gamma, float lam, const float* norm, float sat,
                              const dr_dream_outputs* out, hipStream_t s) {
  DR_REQUIRE(B >= 0 && M >= 1 && H >= 1 && A >= 1, "need B >= 0, M >= 1, H >= 1 and A >= 1");
  DR_REQUIRE(rewards && continues && V_target && V_online && mus && sigmas && actions,
             "rewards, continues, V_target, V_online, mus, sigmas and actions are required");
  DR_REQUIRE(out, "the outputs struct is required");
  const dr_dream_outputs& o = *out;
  DR_REQUIRE(o.R_lambda || o.R_mc || o.adv || o.adv_norm || o.weight || o.logp || o.base_entropy || o.saturated ||
                 o.reward_mean || o.reward_std || o.ret_mean || o.ret_std || o.logp_mean || o.logp_std || o.alive ||
                 o.action_spread || o.best || o.worst || o.n_finite,
             "no output requested");
  const long long lds = (long long)(M | 1) * (3LL * H + 2);
  if (M > DR_DREAM_STATS_MAX_DREAMS || lds > DR_DREAM_STATS_MAX_LDS_FLOATS) {
    dr_set_error("dr_dream_stats: M = %d over %d or (M | 1) * (3 H + 2) = %lld over %d LDS floats", M,
                 DR_DREAM_STATS_MAX_DREAMS, lds, DR_DREAM_STATS_MAX_LDS_FLOATS);
    return DR_E_UNSUPPORTED;
  }
  DR_REQUIRE((long long)B * M * (H + 1) * A <= 0x7fffffffLL, "too many elements");
  if (B == 0) return DR_OK;
  DreamStatsArgs a;
  a.M = M; a.H = H; a.A = A;
  a.rewards = rewards; a.continues = continues; a.Vt = V_target; a.Vo = V_online;
  a.mus = mus; a.sigmas = sigmas; a.actions = actions; a.norm = norm;
  a.gamma = gamma; a.lam = lam; a.lam_c = (float)(1.0 - (double)lam); a.sat = sat;
  a.o = o;
  hipLaunchKernelGGL(k_dream_stats, dim3((unsigned)B), dim3(256), (size_t)lds * sizeof(float), s, a);
  return dr_check_launch("dream_stats");
}

// eps[s][row][i] = the N(0,1) Philox variate of (noise.stream + s, noise.row0 + row, i):
// what the imagination unroll's actor draws at step s in both of its forms.
__global__ __launch_bounds__(256) void k_actor_draws(long long n, int rows, int A,
                                                     const unsigned long long* __restrict__ rng, int row0, int stream,
                                                     float* __restrict__ eps) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long sr = i / A, s = sr / rows;
  eps[i] = dr_normal(rng, (uint32_t)(stream + s), (uint32_t)(row0 + (sr - s * rows)), (uint32_t)(i - sr * A));
}

extern "C" int dr_actor_draws(int steps, int rows, int A, dr_noise noise, float* eps, hipStream_t st) {
  DR_REQUIRE(steps >= 0 && rows >= 0 && A >= 1 && eps && noise.rng,
             "need steps >= 0, rows >= 0, A >= 1, eps and the Philox state");
  const long long n = (long long)steps * rows * A;
  DR_REQUIRE(n <= 0x7fffffffLL, "too many draws");
  if (n == 0) return DR_OK;
  hipLaunchKernelGGL(k_actor_draws, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, rows, A, noise.rng,
                     noise.row0, noise.stream, eps);
  return dr_check_launch("actor_draws");
}
