// Latent planning (plan.py): the CEM / MPPI search around dr_imagine_actions
// and dr_critic_fwd.  Two one-shot kernels: dr_plan_sample draws the candidate
// action sequences of an iteration, dr_plan_update scores them, ranks them and
// refits the sampling distribution.  Nothing is shared between workgroups, no
// atomics, no waits.  f32, built with -ffp-contract=off like the other
// elementwise code, so the host reproduces every expression in its order.
#include "ops.h"

// a[e][n][k][i]: the n-th actor sequence for n < N_pi, otherwise
// clamp(mean[e][k][i] + std[e][k][i] * eps, -1, 1) (one multiply, one add).
// One thread per element; the draw of an element depends on (row0 + e, n, k, i)
// alone, so an environment has the same bits at every E and position.
__global__ __launch_bounds__(256) void k_plan_sample(long long total, int N, int N_pi, int HA,
                                                     const float* __restrict__ mean, const float* __restrict__ std,
                                                     const float* __restrict__ pol, dr_noise nz,
                                                     float* __restrict__ actions) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const long long row = idx / HA;  // e * N + n
  const int j = (int)(idx - row * HA);
  const int e = (int)(row / N), n = (int)(row - (long long)e * N);
  float v;
  if (n < N_pi) {
    v = pol[((long long)e * N_pi + n) * HA + j];
  } else {
    const float eps = nz.eps ? nz.eps[idx]
                             : dr_normal(nz.rng, (uint32_t)nz.stream, (uint32_t)(nz.row0 + e) * (uint32_t)N + (uint32_t)n,
                                         (uint32_t)j);
    const long long o = (long long)e * HA + j;
    const float t = std[o] * eps;
    v = fminf(fmaxf(mean[o] + t, -1.0f), 1.0f);
  }
  actions[idx] = v;
}

extern "C" int dr_plan_sample(int E, int N, int N_pi, int H, int A, const float* mean, const float* std,
                              const float* policy_actions, dr_noise noise, float* actions, hipStream_t s) {
  DR_REQUIRE(E >= 0 && N >= 1 && H >= 1 && A >= 1, "need E >= 0, N >= 1, H >= 1 and A >= 1");
  DR_REQUIRE(N_pi >= 0 && N_pi <= N, "need 0 <= N_pi <= N");
  DR_REQUIRE(mean && std && actions, "mean, std and actions are required");
  DR_REQUIRE((policy_actions != nullptr) == (N_pi > 0), "policy_actions is NULL exactly when N_pi = 0");
  DR_REQUIRE(N_pi == N || noise.eps || noise.rng, "no noise source (noise.eps or noise.rng)");
  if (N > DR_PLAN_MAX_CANDIDATES || (long long)H * A > DR_PLAN_MAX_ELEMS) {
    dr_set_error("dr_plan_sample: N = %d over %d or H * A = %lld over %d", N, DR_PLAN_MAX_CANDIDATES, (long long)H * A,
                 DR_PLAN_MAX_ELEMS);
    return DR_E_UNSUPPORTED;
  }
  const long long total = (long long)E * N * H * A;
  DR_REQUIRE(total <= 0x7fffffffLL, "too many elements");
  if (E == 0) return DR_OK;
  hipLaunchKernelGGL(k_plan_sample, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, N, N_pi, H * A, mean,
                     std, policy_actions, noise, actions);
  return dr_check_launch("plan_sample");
}

__device__ __forceinline__ bool plan_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

// One 256-thread workgroup per environment; PER = candidates per thread (the
// host picks the smallest of 1, 2, 4, 8 that covers N).
//  1. scores: thread t takes candidates t, t + 256, ...: k_lambda_returns'
//     recursion at lam = 1 (lam_c = 0; the intermediate values it multiplies by
//     lam_c are taken as +0), kept in registers and in LDS and written out raw.
//  2. ranks by counting: candidate n's rank is the number of finite scores that
//     beat it (greater, or equal with a lower index) -- the total order needs
//     no sort.  A thread's candidates share one pass over the LDS scores, four
//     per read, every lane reading the same words (a broadcast); the pad up to
//     a multiple of four is NaN, which beats nothing.  Non-finite scores get no
//     rank.  The elite of rank j < K' puts its index into LDS slot j.
//  3. weights in LDS, W added in rank order from 0.0f by every thread for
//     itself (the same chain, so the same bits, and no further barrier).
//  4. refit: the elites' action rows are staged through LDS in rank order, as
//     many rows at a time as PLAN_STAGE floats hold (at least 8), all 256
//     threads loading (coalesced, independent loads); thread t then adds
//     elements t, t + 256, ... of [H][A] over the staged rows in rank order.
//     Two passes (mean, then squared deviations); when every elite fits one
//     stage the second pass reuses it.
constexpr int PLAN_STAGE = 8192;                      // floats: 32 KiB of LDS
constexpr int PLAN_XPT = DR_PLAN_MAX_ELEMS / 256;     // elements of [H][A] per thread

template <int PER>
__global__ __launch_bounds__(256) void k_plan_update(int N, int H, int A, int K, const float* __restrict__ rew,
                                                     const float* __restrict__ cont, const float* __restrict__ v_last,
                                                     float gamma, float temperature, float momentum, float std_min,
                                                     float std_max, const float* __restrict__ actions,
                                                     float* __restrict__ mean, float* __restrict__ std,
                                                     float* __restrict__ scores, int* __restrict__ elite_idx,
                                                     float* __restrict__ elite_w, int* __restrict__ n_elite) {
  __shared__ __attribute__((aligned(16))) float sc[DR_PLAN_MAX_CANDIDATES];
  __shared__ float ew[DR_PLAN_MAX_CANDIDATES];
  __shared__ int ei[DR_PLAN_MAX_CANDIDATES];
  __shared__ float stage[PLAN_STAGE];
  const int e = blockIdx.x, tid = threadIdx.x;
  const long long row0 = (long long)e * N;
  const int HA = H * A;
  const int N4 = (N + 3) & ~3;  // <= DR_PLAN_MAX_CANDIDATES, a multiple of 4

  float g[PER];
#pragma unroll
  for (int p = 0; p < PER; ++p) {
    const int n = tid + p * 256;
    g[p] = 0.0f;
    if (n < N) {
      const float* rb = rew + (row0 + n) * H;
      const float* cb = cont + (row0 + n) * H;
      const float vH = v_last ? v_last[row0 + n] : 0.0f;
      float nxt = rb[H - 1] + (gamma * cb[H - 1]) * vH;
#pragma unroll 4
      for (int t = H - 2; t >= 0; --t) nxt = rb[t] + (gamma * cb[t]) * ((0.0f * 0.0f) + (1.0f * nxt));
      g[p] = nxt;
      sc[n] = nxt;
      scores[row0 + n] = nxt;
    }
  }
  if (tid < N4 - N) sc[N + tid] = __uint_as_float(0x7fc00000u);
  __syncthreads();

  int rk[PER];
#pragma unroll
  for (int p = 0; p < PER; ++p) rk[p] = 0;
  int nf = 0;
  for (int m4 = 0; m4 < N4; m4 += 4) {
    const float4 v4 = *reinterpret_cast<const float4*>(sc + m4);
    const float gm[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool f = plan_finite(gm[q]);
      nf += f ? 1 : 0;
#pragma unroll
      for (int p = 0; p < PER; ++p)
        rk[p] += (f && (gm[q] > g[p] || (gm[q] == g[p] && m4 + q < tid + p * 256))) ? 1 : 0;
    }
  }
  const int Ke = K < nf ? K : nf;
#pragma unroll
  for (int p = 0; p < PER; ++p) {
    const int n = tid + p * 256;
    if (n < N && plan_finite(g[p]) && rk[p] < Ke) ei[rk[p]] = n;
  }
  __syncthreads();

  const float g0 = Ke > 0 ? sc[ei[0]] : 0.0f;
  for (int j = tid; j < Ke; j += 256) ew[j] = temperature == 0.0f ? 1.0f : expf((sc[ei[j]] - g0) / temperature);
  __syncthreads();
  float W = 0.0f;
  for (int j = 0; j < Ke; ++j) W = W + ew[j];

  for (int j = tid; j < K; j += 256) {
    elite_idx[(long long)e * K + j] = j < Ke ? ei[j] : -1;
    elite_w[(long long)e * K + j] = j < Ke ? ew[j] / W : 0.0f;
  }
  if (tid == 0) n_elite[e] = Ke;
  if (Ke == 0) return;  // (uniform) mean and std keep their bits

  const float* ab = actions + row0 * HA;
  const int per = PLAN_STAGE / HA;  // staged rows: >= 8 as HA <= DR_PLAN_MAX_ELEMS
  float acc[PLAN_XPT], m[PLAN_XPT];
#pragma unroll
  for (int q = 0; q < PLAN_XPT; ++q) acc[q] = 0.0f, m[q] = 0.0f;
  for (int pass = 0; pass < 2; ++pass) {
    for (int j0 = 0; j0 < Ke; j0 += per) {
      const int cnt = Ke - j0 < per ? Ke - j0 : per;
      if (pass == 0 || Ke > per) {  // (uniform)
        __syncthreads();            // the rows staged before have been consumed
#pragma unroll 4
        for (int idx = tid; idx < cnt * HA; idx += 256) {
          const int jj = idx / HA, x = idx - jj * HA;
          stage[idx] = ab[(long long)ei[j0 + jj] * HA + x];
        }
        __syncthreads();
      }
#pragma unroll
      for (int q = 0; q < PLAN_XPT; ++q) {
        const int x = tid + q * 256;
        if (x >= HA) continue;
        float a = acc[q];
        if (pass == 0) {
          for (int jj = 0; jj < cnt; ++jj) a = a + ew[j0 + jj] * stage[jj * HA + x];
        } else {
          for (int jj = 0; jj < cnt; ++jj) {
            const float dv = stage[jj * HA + x] - m[q];
            a = a + ew[j0 + jj] * (dv * dv);
          }
        }
        acc[q] = a;
      }
    }
    if (pass == 0) {
#pragma unroll
      for (int q = 0; q < PLAN_XPT; ++q) m[q] = acc[q] / W, acc[q] = 0.0f;
    }
  }
  const float keep = 1.0f - momentum;
#pragma unroll
  for (int q = 0; q < PLAN_XPT; ++q) {
    const int x = tid + q * 256;
    if (x >= HA) continue;
    const float sd = sqrtf(acc[q] / W);
    const long long o = (long long)e * HA + x;
    mean[o] = momentum * mean[o] + keep * m[q];
    std[o] = fminf(fmaxf(sd, std_min), std_max);
  }
}

extern "C" int dr_plan_update(int E, int N, int H, int A, int K, const float* rewards, const float* continues,
                              const float* v_last, float gamma, float temperature, float momentum, float std_min,
                              float std_max, const float* actions, float* mean, float* std, float* scores,
                              int* elite_idx, float* elite_w, int* n_elite, hipStream_t s) {
  DR_REQUIRE(E >= 0 && N >= 1 && H >= 1 && A >= 1, "need E >= 0, N >= 1, H >= 1 and A >= 1");
  DR_REQUIRE(K >= 1 && K <= N, "need 1 <= K <= N");
  DR_REQUIRE(rewards && continues && actions && mean && std && scores && elite_idx && elite_w && n_elite,
             "rewards, continues, actions, mean, std, scores, elite_idx, elite_w and n_elite are required");
  DR_REQUIRE(temperature >= 0.0f && momentum >= 0.0f && momentum < 1.0f && std_min >= 0.0f && std_min <= std_max,
             "need temperature >= 0, 0 <= momentum < 1 and 0 <= std_min <= std_max");
  if (N > DR_PLAN_MAX_CANDIDATES || (long long)H * A > DR_PLAN_MAX_ELEMS) {
    dr_set_error("dr_plan_update: N = %d over %d or H * A = %lld over %d", N, DR_PLAN_MAX_CANDIDATES, (long long)H * A,
                 DR_PLAN_MAX_ELEMS);
    return DR_E_UNSUPPORTED;
  }
  DR_REQUIRE((long long)E * N * H * A <= 0x7fffffffLL, "too many elements");
  if (E == 0) return DR_OK;
  const dim3 grid((unsigned)E), block(256);
#define PLAN_UPDATE_LAUNCH(PER)                                                                                     \
  hipLaunchKernelGGL(k_plan_update<PER>, grid, block, 0, s, N, H, A, K, rewards, continues, v_last, gamma,          \
                     temperature, momentum, std_min, std_max, actions, mean, std, scores, elite_idx, elite_w, n_elite)
  if (N <= 256) PLAN_UPDATE_LAUNCH(1);
  else if (N <= 512) PLAN_UPDATE_LAUNCH(2);
  else if (N <= 1024) PLAN_UPDATE_LAUNCH(4);
  else PLAN_UPDATE_LAUNCH(8);
#undef PLAN_UPDATE_LAUNCH
  return dr_check_launch("plan_update");
}
