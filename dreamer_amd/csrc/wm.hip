// a19/a20: the world-model training step (WorldModel.training_step,
// WorldModel.py:148-198; unroll_model 84-146; Decoder.forward
// VariationalAutoEncoder.py:139-161) as one fixed launch sequence.
//
// Rows are time-major (m = t*B + b).  The posterior scan runs per step (B
// rows); every head that does not feed the recurrence (prior, decoder, reward,
// continue) runs once over the M1 = (T-1)*B rows t >= 1 -- the only rows the
// losses read (WorldModel.py:141-145), so row t = 0 of the decoder / prior is
// never computed.  The backward mirrors it: batched head backward into dL/dh,
// dL/dz, then the reverse scan (straight-through sampler, latent_mapper, GRU),
// then the encoder convolutions over all M frames.
#include <algorithm>

#include "engine_util.h"

// ---------------------------------------------------------------------------
// small kernels of the loss
// ---------------------------------------------------------------------------
// window actions / rewards / continues -> time-major [T][B](*A)
__global__ void k_wm_gather(int B, int T, int A, dr_wm_batch bt, float* act_tm, float* rew_tm, float* cont_tm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * T) return;
  const int t = i / B, b = i - t * B;
  for (int a = 0; a < A; ++a) act_tm[(long long)i * A + a] = bt.actions[b * bt.act_sb + t * bt.act_st + a];
  rew_tm[i] = bt.rewards[b * bt.rc_sb + t * bt.rc_st];
  cont_tm[i] = bt.continues[b * bt.rc_sb + t * bt.rc_st];
}

// block-wide sum in a fixed order (deterministic)
__device__ float block_sum256(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// mask = continues[:, :T-1] (WorldModel.py:170); row i < M1 of every head /
// decoder frame is (t = i/B + 1, b) and its mask is cont_tm[i].
// stats[0] = local mask.sum() (all-reduced by a data-parallel caller)
__global__ __launch_bounds__(256) void k_wm_masksum(int M1, const float* cont_tm, float* stats) {
  __shared__ float red[256];
  float s = 0.0f;
  for (int i = threadIdx.x; i < M1; i += 256) s += cont_tm[i];
  s = block_sum256(s, red);
  if (threadIdx.x == 0) stats[0] = s;
}

// scal[0] = mask.sum() + 1e-5 (WorldModel.py:185, global); coef_row =
// beta_pred * mask / denom (the factor of every prediction-loss gradient);
// coef_obs = 2 * coef_row
__global__ __launch_bounds__(256) void k_wm_coef(int M1, const float* cont_tm, float beta_pred, const float* stats,
                                                 float* scal, float* coef_row, float* coef_obs) {
  const float denom = stats[0] + 1e-5f;
  if (threadIdx.x == 0) scal[0] = denom;
  for (int i = threadIdx.x; i < M1; i += 256) {
    const float c = beta_pred * cont_tm[i] / denom;
    coef_row[i] = c;
    coef_obs[i] = 2.0f * c;
  }
}

// KL(post || prior) per (row, latent group) (WorldModel.py:175-183;
// torch.distributions.kl._kl_categorical_categorical on normalised logits).
// MODE 0: kl_grp[row][g].  MODE 1: gradients -- dyn: d/d prior = cd*(q - p);
// rep: d/d post = cr * p * (lp - lq - KL_g), cd/cr = scal[1]/scal[2] * mask.
template <int MODE>
__global__ void k_wm_kl(int M1, int R, int C, int W, const float* __restrict__ prior, const float* __restrict__ post,
                        const float* __restrict__ cont_tm, const float* __restrict__ scal, float* kl_grp,
                        float* g_prior, float* g_post) {
  const int gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const int grp = gtid / W, c = gtid - grp * W;
  const bool valid = grp < M1 * R;
  const int row = valid ? grp / R : 0, g = valid ? grp - row * R : 0;
  const bool act = valid && c < C;
  const long long o = (long long)row * R * C + (long long)g * C + c;
  const float xp = act ? post[o] : -INFINITY;
  const float xq = act ? prior[o] : -INFINITY;
  const float mp = group_max(xp, W), mq = group_max(xq, W);
  const float ep = act ? expf(xp - mp) : 0.0f, eq = act ? expf(xq - mq) : 0.0f;
  const float sp = group_sum(ep, W), sq = group_sum(eq, W);
  // (x - max) first: exact for nearby logits, so a constant offset on a group's logits changes no bit of the result
  // (x - (max + log sum) rounds at the size of the logits: 1e-3 of absolute error at logits of 1e4)
  const float lp = (xp - mp) - logf(sp), lq = (xq - mq) - logf(sq);
  const float p = ep / sp;
  const float term = act ? p * (lp - lq) : 0.0f;
  const float klg = group_sum(term, W);
  if (MODE == 0) {
    if (act && c == 0) kl_grp[(long long)row * R + g] = klg;
  } else if (act) {
    const float m = cont_tm[row];
    const float cd = scal[1] * m, cr = scal[2] * m;
    g_prior[o] = cd * (eq / sq - p);
    g_post[o] = cr * (p * (lp - lq - klg));
  }
}

// reward two-hot log-likelihood and continue BCE per row (WorldModel.py:125-138)
// and their gradients scaled by coef_row; one wave per row
__global__ __launch_bounds__(256) void k_wm_heads(int M1, int nb, const float* __restrict__ rlog,
                                                  const float* __restrict__ clog, const float* __restrict__ rew_tm,
                                                  const float* __restrict__ cont_tm,
                                                  const float* __restrict__ buckets,
                                                  const float* __restrict__ coef_row, float* rew_row, float* cont_row,
                                                  float* g_rew, float* g_cont) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M1) return;
  const float* x = rlog + (long long)row * nb;
  float mx = -INFINITY;
  for (int j = lane; j < nb; j += 64) mx = fmaxf(mx, x[j]);
  mx = wave_max(mx);
  float se = 0.0f;
  for (int j = lane; j < nb; j += 64) se += expf(x[j] - mx);
  se = wave_sum(se);
  const float lse = mx + logf(se);
  // to_twohot (DreamerUtils.py:39-50): clamp, searchsorted(right=True) - 1, clamp <= nb-2
  const float rv = rew_tm[row];  // torch.clamp keeps NaN (-> non-finite loss -> skipped step)
  const float v = isnan(rv) ? rv : fminf(fmaxf(rv, buckets[0]), buckets[nb - 1]);
  float cnt = 0.0f;
  for (int j = lane; j < nb; j += 64) cnt += (buckets[j] <= v) ? 1.0f : 0.0f;
  int lo = (int)wave_sum(cnt) - 1;
  lo = lo > nb - 2 ? nb - 2 : (lo < 0 ? 0 : lo);
  const float blo = buckets[lo], bhi = buckets[lo + 1];
  const float w = (v - blo) / (bhi - blo + 1e-8f);
  const float coef = coef_row[row];
  for (int j = lane; j < nb; j += 64) {
    const float th = (j == lo) ? 1.0f - w : ((j == lo + 1) ? w : 0.0f);
    g_rew[(long long)row * nb + j] = coef * (expf(x[j] - mx) / se - th);
  }
  if (lane == 0) {
    rew_row[row] = (1.0f - w) * (x[lo] - lse) + w * (x[lo + 1] - lse);
    const float xc = clog[row], y = cont_tm[row];
    // binary_cross_entropy_with_logits: (1 - y) x + max(-x, 0) + log(exp(-max) + exp(-x - max))
    const float mv = fmaxf(-xc, 0.0f);
    cont_row[row] = (1.0f - y) * xc + mv + logf(expf(-mv) + expf(-xc - mv));
    g_cont[row] = coef * (1.0f / (1.0f + expf(-xc)) - y);
  }
}

// local masked sums of the loss terms: stats[1..4] = sum mask * (squared
// error, reward log-lik, continue BCE, KL) over this rank's rows
__global__ __launch_bounds__(256) void k_wm_stats(int M1, int R, int nparts, const float* __restrict__ obs_part,
                                                  const float* __restrict__ rew_row,
                                                  const float* __restrict__ cont_row,
                                                  const float* __restrict__ kl_grp, const float* __restrict__ cont_tm,
                                                  float* stats) {
  __shared__ float red[256];
  float so = 0.f, sr = 0.f, sc = 0.f, sk = 0.f;
  for (int i = threadIdx.x; i < M1; i += 256) {
    const float m = cont_tm[i];
    float o = 0.f;
    for (int j = 0; j < nparts; ++j) o += obs_part[(long long)i * nparts + j];
    float k = 0.f;
    for (int g = 0; g < R; ++g) k += kl_grp[(long long)i * R + g];
    so += o * m;
    sr += rew_row[i] * m;
    sc += cont_row[i] * m;
    sk += k * m;
  }
  so = block_sum256(so, red);
  sr = block_sum256(sr, red);
  sc = block_sum256(sc, red);
  sk = block_sum256(sk, red);
  if (threadIdx.x == 0) {
    stats[1] = so;
    stats[2] = sr;
    stats[3] = sc;
    stats[4] = sk;
  }
}

// losses (WorldModel.py:170-189) from the (global) sums and the KL-gradient
// factors of the free-bit clamp max(1, KL): d max(1, k)/dk = 1 (k > 1),
// 1/2 (k == 1), 0 (k < 1).  rows = B_global * (T - 1) (torch.mean's count).
__global__ void k_wm_final(const float* stats, int rows, dr_wm_loss_cfg cfg, float* scal, float* losses, int* skip) {
  if (threadIdx.x != 0) return;
  const float denom = stats[0] + 1e-5f;
  const float pred = (stats[1] - stats[2] + stats[3]) / denom;
  const float kl = stats[4] / (float)rows;
  // torch.max(1, kl) keeps a NaN KL (fmaxf would drop it: a finite total, no skip, and the KL gradient silently off)
  const float fb = kl < 1.0f ? 1.0f : kl;
  const float total = cfg.beta_pred * pred + cfg.beta_dyn * fb + cfg.beta_rep * fb;
  const float wk = kl > 1.0f ? 1.0f : (kl == 1.0f ? 0.5f : 0.0f);
  scal[1] = cfg.beta_dyn * wk / (float)rows;
  scal[2] = cfg.beta_rep * wk / (float)rows;
  losses[0] = total;
  losses[1] = pred;
  losses[2] = kl;
  losses[3] = kl;
  if (skip) *skip = isfinite(total) ? 0 : 1;
}

// gl = 0.99 * softmax-backward(gz) (+ extra): the straight-through sampler's
// gradient (VAE.py:92-98) plus the KL-rep gradient of the same logits
__global__ void k_ste_bwd_add(int M, int R, int C, int W, const float* __restrict__ gz, long long ldg,
                              const float* __restrict__ soft, long long lds, const float* __restrict__ extra,
                              long long lde, float* __restrict__ gl, long long ldl) {
  const int gtid = blockIdx.x * blockDim.x + threadIdx.x;
  const int grp = gtid / W, c = gtid - grp * W;
  const bool valid = grp < M * R;
  const int m = valid ? grp / R : 0, r = valid ? grp - m * R : 0;
  const bool act = valid && c < C;
  const float gs = act ? gz[(long long)m * ldg + r * C + c] * 0.99f : 0.0f;
  const float sv = act ? soft[(long long)m * lds + r * C + c] : 0.0f;
  const float dot = group_sum(gs * sv, W);
  if (act) {
    float v = sv * (gs - dot);
    if (extra) v += extra[(long long)m * lde + r * C + c];
    gl[(long long)m * ldl + r * C + c] = v;
  }
}

__global__ void k_mul_dsilu(long long n, float* __restrict__ g, const float* __restrict__ pre) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g[i] = g[i] * dr_dsilu(pre[i]);
}

// rows of a [C*P][K] matrix between the NCHW flatten order (c*P + p) and NHWC
// (p*C + c): to_nhwc: out[p*C + c] = in[c*P + p], else the inverse
__global__ void k_perm_rows(int C, int P, int K, const float* __restrict__ in, float* __restrict__ out, int to_nhwc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)C * P * K) return;
  const long long row = i / K;
  const int k = (int)(i - row * K);
  const int c = (int)(row / P), p = (int)(row - (long long)c * P);  // row in NCHW order
  const long long nh = ((long long)p * C + c) * K + k;
  if (to_nhwc) out[nh] = in[i];
  else out[i] = in[nh];
}

__global__ void k_silu(long long n, const float* __restrict__ x, float* __restrict__ y) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = dr_silu(x[i]);
}

// vector observations: decoder output mu (no Tanh) against the target rows,
// squared error per row into part[row] (one part per frame for k_wm_stats)
// and dL/dmu = coef[row] * (mu - x) (coef carries the 2 and the mask weights,
// as CT_EPI_TANH_MSE's does before its (1 - mu^2)); a wave per row
__global__ __launch_bounds__(256) void k_vec_mse(int M1, int D, const float* __restrict__ mu,
                                                 const float* __restrict__ x, const float* __restrict__ coef,
                                                 float* __restrict__ g, float* __restrict__ part) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M1) return;
  const float cf = coef[row];
  float sq = 0.f;
  for (int c = lane; c < D; c += 64) {
    const long long o = (long long)row * D + c;
    const float err = mu[o] - x[o];
    sq += err * err;
    g[o] = cf * err;
  }
  sq = wave_sum(sq);
  if (lane == 0) part[row] = sq;
}

static int blocks(long long n, int t) { return (int)((n + t - 1) / t); }

// split-K scratch for one launch's problems (disjoint slices of the pool)
static void splitk_all(GemmArgs* p, int n, float* pool, long long pool_n) {
  float* cur = pool;
  long long left = pool_n;
  for (int i = 0; i < n; ++i) give_splitk(p[i], cur, left);
}

static int perm_rows(int C, int P, int K, const float* in, float* out, int to_nhwc, hipStream_t s) {
  const long long n = (long long)C * P * K;
  hipLaunchKernelGGL(k_perm_rows, dim3(blocks(n, 256)), dim3(256), 0, s, C, P, K, in, out, to_nhwc);
  return dr_check_launch("perm_rows");
}

static int pow2_ge(int c) {
  int w = 1;
  while (w < c) w <<= 1;
  return w;
}

// ---------------------------------------------------------------------------
// launchers of the loss kernels: each owns its kernel's grid, block and group
// width, and is the only place that kernel is launched from (the step's
// stages and the dr_internal_wm_loss_run test hook both go through them)
// ---------------------------------------------------------------------------
static int wm_gather(int B, int T, int A, const dr_wm_batch& bt, float* act_tm, float* rew_tm, float* cont_tm,
                     hipStream_t s) {
  hipLaunchKernelGGL(k_wm_gather, dim3(blocks((long long)B * T, 256)), dim3(256), 0, s, B, T, A, bt, act_tm, rew_tm,
                     cont_tm);
  return dr_check_launch("wm_gather");
}
static int wm_masksum(int M1, const float* cont_tm, float* stats, hipStream_t s) {
  hipLaunchKernelGGL(k_wm_masksum, dim3(1), dim3(256), 0, s, M1, cont_tm, stats);
  return dr_check_launch("wm_masksum");
}
static int wm_coef(int M1, const float* cont_tm, float beta_pred, const float* stats, float* scal, float* coef_row,
                   float* coef_obs, hipStream_t s) {
  hipLaunchKernelGGL(k_wm_coef, dim3(1), dim3(256), 0, s, M1, cont_tm, beta_pred, stats, scal, coef_row, coef_obs);
  return dr_check_launch("wm_coef");
}
// one latent group on W = pow2 >= C lanes (group_sum / group_max reach 64 lanes: C <= 64)
static int wm_kl_fwd(int M1, int R, int C, const float* prior, const float* post, float* kl_grp, hipStream_t s) {
  DR_REQUIRE(C >= 1 && C <= 64, "latent classes must be in [1,64]");
  const int W = pow2_ge(C);
  if ((long long)M1 * R == 0) return DR_OK;
  hipLaunchKernelGGL(k_wm_kl<0>, dim3(blocks((long long)M1 * R * W, 256)), dim3(256), 0, s, M1, R, C, W, prior, post,
                     nullptr, nullptr, kl_grp, nullptr, nullptr);
  return dr_check_launch("wm_kl");
}
static int wm_kl_bwd(int M1, int R, int C, const float* prior, const float* post, const float* cont_tm,
                     const float* scal, float* g_prior, float* g_post, hipStream_t s) {
  DR_REQUIRE(C >= 1 && C <= 64, "latent classes must be in [1,64]");
  const int W = pow2_ge(C);
  if ((long long)M1 * R == 0) return DR_OK;
  hipLaunchKernelGGL(k_wm_kl<1>, dim3(blocks((long long)M1 * R * W, 256)), dim3(256), 0, s, M1, R, C, W, prior, post,
                     cont_tm, scal, nullptr, g_prior, g_post);
  return dr_check_launch("wm_kl_bwd");
}
static int wm_heads_loss(int M1, int nb, const float* rlog, const float* clog, const float* rew_tm,
                         const float* cont_tm, const float* buckets, const float* coef_row, float* rew_row,
                         float* cont_row, float* g_rew, float* g_cont, hipStream_t s) {
  DR_REQUIRE(nb >= 2, "the reward head needs at least two buckets");
  if (M1 == 0) return DR_OK;
  hipLaunchKernelGGL(k_wm_heads, dim3(blocks(M1, 4)), dim3(256), 0, s, M1, nb, rlog, clog, rew_tm, cont_tm, buckets,
                     coef_row, rew_row, cont_row, g_rew, g_cont);
  return dr_check_launch("wm_heads");
}
static int wm_stats(int M1, int R, int nparts, const float* obs_part, const float* rew_row, const float* cont_row,
                    const float* kl_grp, const float* cont_tm, float* stats, hipStream_t s) {
  hipLaunchKernelGGL(k_wm_stats, dim3(1), dim3(256), 0, s, M1, R, nparts, obs_part, rew_row, cont_row, kl_grp, cont_tm,
                     stats);
  return dr_check_launch("wm_stats");
}
static int wm_final(const float* stats, int rows, dr_wm_loss_cfg cfg, float* scal, float* losses, int* skip,
                    hipStream_t s) {
  hipLaunchKernelGGL(k_wm_final, dim3(1), dim3(64), 0, s, stats, rows, cfg, scal, losses, skip);
  return dr_check_launch("wm_final");
}
static int ste_bwd_add(int M, int R, int C, const float* gz, long long ldg, const float* soft, long long lds,
                       const float* extra, long long lde, float* gl, long long ldl, hipStream_t s) {
  DR_REQUIRE(C >= 1 && C <= 64, "latent classes must be in [1,64]");
  const int W = pow2_ge(C);
  if ((long long)M * R == 0) return DR_OK;
  hipLaunchKernelGGL(k_ste_bwd_add, dim3(blocks((long long)M * R * W, 256)), dim3(256), 0, s, M, R, C, W, gz, ldg, soft,
                     lds, extra, lde, gl, ldl);
  return dr_check_launch("ste_bwd_add");
}
static int vec_mse(int M1, int D, const float* mu, const float* x, const float* coef, float* g, float* part,
                   hipStream_t s) {
  if (M1 == 0) return DR_OK;
  hipLaunchKernelGGL(k_vec_mse, dim3(blocks(M1, 4)), dim3(256), 0, s, M1, D, mu, x, coef, g, part);
  return dr_check_launch("vec_mse");
}

// ---------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------
struct MlpBwd {  // backward scratch of one 3-layer head (and its LayerNorm saves)
  float *gx2, *gp2, *gy2, *xh2, *gx1, *gp1, *gy1, *xh1;
};
// one head MLP of the world model over the M1 rows t >= 1 (WmWs::head: prior, reward, continue)
struct HeadWs {
  float *p1, *x1, *p2, *x2, *lg;  // .0 / .3 pre-activations, their LN-SiLU outputs, the logits
  float* g;                       // dL/d logits
  float *t6, *t3, *t0;            // transposed weights
  // split3 planes (below) of the forward Linears and of the input-gradient
  // Linears; pl_f6 / pl_h6: the prior only (NULL for the reward and continue heads)
  void *pl_f0, *pl_f3, *pl_f6, *pl_h6, *pl_h3, *pl_h0;
  MlpBwd b;
};
struct WmWs {
  void* tn;         // split3 TN scratch (tn_launch)
  size_t tn_bytes;
  // encoder (all M frames): conv k's pre-activation (NHWC) and output (NHWC; the last NCHW = the flatten order)
  float *x0, *pre[DR_MAX_DEPTH], *a[DR_MAX_DEPTH], *feat;
  float *wr[DR_MAX_DEPTH], *wqe[DR_MAX_DEPTH];  // conv k repacked (forward) / as a convT (data gradient, k >= 1)
  // window data, scan tape
  float *act_tm, *rew_tm, *cont_tm, *zeros, *h_all, *z_all, *soft, *plog, *pre_m, *x_m, *sr, *su, *sn, *sghn, *gi, *gh,
      *wt;
  int* idx;
  HeadWs head[3];  // heads (M1 rows): prior, reward, continue
  // decoder: upscaler pre-activations (du1, du2 = .3 output NHWC), convT k's output pre-activation dq[k] (k < N-1;
  // vector mode: dq[0] = image_builder.0 pre, dq[1] = mu) and its SiLU dqp[k]; dgout = dL/d(pre-tanh output)
  float *du1, *dx1, *du2, *du2p, *dq[DR_MAX_DEPTH], *dqp[DR_MAX_DEPTH], *dgout, *w3p, *b3p;
  float *wqd[DR_MAX_DEPTH], *wrd[DR_MAX_DEPTH];
  // split3 bf16 weight planes (conv_split.hip) of encoder conv k (forward) and
  // of decoder convT k read as a Conv2d (its data gradient); NULL: f32 path
  void *s3e[DR_MAX_DEPTH], *s3d[DR_MAX_DEPTH];
  // ... and of decoder convT k (forward) / encoder conv k's data gradient as upsampling convs
  void *t3d[DR_MAX_DEPTH], *t3e[DR_MAX_DEPTH];
  void* e12w1;  // conv1's split3 weight planes for k_enc12_split3
  // the posterior scan's per-step products (latent_mapper.0's h-columns, W_hh)
  // as split3 planes for k_gemm_wks3 (B >= 128), as in dr_observe_scan
  void *s3m0, *s3whh;
  // ... and of the scan backward's input-gradient products (W_ih^T's latent
  // rows, W_hh^T; K = 3 Hd)
  void *s3wtb, *s3twhh;
  // split3 planes of the tall (B (T-1) / B T rows) NT products' weights: the
  // heads' input-gradient Linears (.3 / .0 of each, the prior's .6: HeadWs
  // pl_h3 / pl_h0 / pl_h6), the decoder upscaler's .3 / .0, the encoder
  // projection (forward, and its transposed input gradient) -- k_gemm_split3
  // instead of the f32 tile kernel
  void *pl_up3, *pl_up0, *pl_w0tp, *pl_map0f;
  // ... and of the forward heads / upscaler over B (T - 1) rows: the first
  // Linears (HeadWs pl_f0; upscaler.0: pl_fup0), the .3 layers (pl_f3), the
  // prior's .6 (pl_f6), upscaler.3 (permuted rows)
  void *pl_fup0, *pl_fup3;
  // loss
  float *coef_row, *coef_obs, *obs_part, *obs_bpart, *kl_grp, *rew_row, *cont_row, *scal, *stats;
  float* csp;  // per-tile channel sums of the last decoder layer's input gradient (k_conv_nhwc csum)
  // backward
  float *gH, *gZ, *glog, *gpost;
  float *gxu, *gpu, *gyu, *xhu, *dgq[DR_MAX_DEPTH], *dgu2, *dw3p, *db3p;  // dgq[k]: dL/d dq[k]
  float *ggi, *ggh, *gpre_m, *gy_m, *xh_m, *gx_s, *gh_dummy;
  float* gp[DR_MAX_DEPTH];  // dL/d pre[k]
  // transposed / permuted weights (the heads': HeadWs t6 / t3 / t0)
  float *t_up3, *t_up0, *t_map3, *t_map0, *t_whh, *w0tp;
  float *cws;  // conv weight-gradient / channel-sum scratch
  long long cws_n;
  float* sk;  // split-K partial planes of the tile GEMMs (reused launch to launch)
  long long sk_n;
};

struct WmDims {
  int B, T, M, M1, L, Hd, A, eh, nb, IH, IW, Pf, F, d1, d2, C0, dh, Fd, ph1, ph2, rh1, rh2, ch1, ch2;
  int N;                                        // VAE depth (4 = the reference, 5 = configs[3]'s deeper VAE)
  int e[DR_MAX_DEPTH + 1], cd[DR_MAX_DEPTH + 1];  // encoder / decoder channels (engine_util.h enc_chans / dec_chans)
  long long pix[DR_MAX_DEPTH + 1];              // pixels per frame at resolution level k: (IH >> k) (IW >> k)
  int Dv;  // vector observations (dr_dims.obs_dim): MLP encoder / decoder, no conv planes
  // bf16 operand terms of the split-conv kernels: 3 = f32-accurate (parity
  // mode), 1 = bf16 perf mode (dr_dims.precision)
  int terms;
};
static WmDims wm_dims(const dr_dims* d, int B, int T) {
  WmDims w;
  memset(&w, 0, sizeof(w));
  w.B = B; w.T = T; w.M = B * T; w.M1 = B * (T - 1);
  w.L = latent(d); w.Hd = d->hidden; w.A = d->action; w.eh = d->enc_hidden; w.nb = d->buckets;
  w.IH = d->img_h; w.IW = d->img_w;
  w.N = enc_chans(d, w.e);
  dec_chans(d, w.cd);
  for (int k = 0; k <= w.N; ++k) w.pix[k] = (long long)(w.IH >> k) * (w.IW >> k);
  w.Pf = (int)w.pix[w.N];
  w.F = w.e[w.N] * w.Pf;
  w.d1 = d->dec_f1; w.d2 = d->dec_f2; w.C0 = 4 * d->dec_f2; w.dh = d->dec_hidden; w.Fd = w.C0 * w.Pf;
  w.ph1 = d->prior_h1; w.ph2 = d->prior_h2; w.rh1 = d->rew_h1; w.rh2 = d->rew_h2; w.ch1 = d->cont_h1; w.ch2 = d->cont_h2;
  w.Dv = d->obs_dim > 0 ? d->obs_dim : 0;
  w.terms = d->precision == DR_PREC_BF16 ? 1 : 3;
  if (w.Dv) {  // widths of the MLP stand-ins (include/dreamer_hip.h, dr_dims.obs_dim)
    w.IH = w.IW = 0;
    w.Pf = 1;
    w.F = 4 * d->enc_f2;
    w.Fd = w.C0;
    for (int k = 0; k <= w.N; ++k) w.pix[k] = 0;
  }
  return w;
}
// one row of the head table: the head's weights and their gradients, its
// widths (Linear [h | z] -> w1 -> w2 -> nout) and in_z (0: its input is h only)
struct WmHead {
  const dr_mlp3 *m, *g;
  int w1, w2, nout, in_z;
};
// prior, reward, continue (wm / gw NULL: the widths alone, for the carve)
static void wm_heads(const WmDims& D, const dr_world_model* wm, const dr_world_model* gw, WmHead* h) {
  h[0] = {wm ? &wm->prior : nullptr, gw ? &gw->prior : nullptr, D.ph1, D.ph2, D.L, 0};
  h[1] = {wm ? &wm->reward : nullptr, gw ? &gw->reward : nullptr, D.rh1, D.rh2, D.nb, 1};
  h[2] = {wm ? &wm->cont : nullptr, gw ? &gw->cont : nullptr, D.ch1, D.ch2, 1, 1};
}
static inline int head_in(const WmDims& D, const WmHead& h) { return h.in_z ? D.Hd + D.L : D.Hd; }
// channel stride of conv k's input (the frames are padded to 4 channels) and of convT k's output (3 -> 4)
static inline int enc_cin_st(const WmDims& D, int k) { return k == 0 ? 4 : D.e[k]; }
static inline int dec_cout_st(const WmDims& D, int k) { return k == D.N - 1 ? 4 : D.cd[k + 1]; }

// the convolutions that run f32-accurate on the bf16 MFMA (3-term split):
// encoder conv k >= 1 (conv1's 4-channel input stays on the f32 MFMA) and the
// data gradient of decoder convT k (a Conv2d from cout_t to cin_t channels)
static inline bool enc_s3(const WmDims& D, int k) {
  return !D.Dv && k >= 1 && op_conv_split3_supported(D.M, D.e[k], D.IH >> k, D.IW >> k, D.e[k + 1]);
}
static inline bool dec_s3(const WmDims& D, int k) {
  const int lvl = D.N - 1 - k;  // convT k's output resolution level
  return !D.Dv && dec_cout_st(D, k) == D.cd[k + 1] &&
         op_conv_split3_supported(D.M1, D.cd[k + 1], D.IH >> lvl, D.IW >> lvl, D.cd[k]);
}

// upsampling convs on the split3 path: decoder convT k < N - 1 (forward;
// the last, 3-channel layer runs k_convT_out3) and encoder conv k >= 1's data
// gradient (an upsampling conv from e[k + 1] to e[k] channels)
static inline bool dect_s3(const WmDims& D, int k) {
  return !D.Dv && k < D.N - 1 &&
         op_convT_split3_supported(D.M1, D.cd[k], D.IH >> (D.N - k), D.IW >> (D.N - k), D.cd[k + 1], D.terms);
}
static inline bool encg_s3(const WmDims& D, int k) {
  return !D.Dv && k >= 1 &&
         op_convT_split3_supported(D.M, D.e[k + 1], D.IH >> (k + 1), D.IW >> (k + 1), D.e[k], D.terms);
}

// conv / convT weight gradient: f32-accurate split3 kernel where the shape
// allows (conv_split.hip), else the f32 MFMA kernel (wmconv.hip)
static size_t wgrad_ws_floats(int n, int h, int w, int ca, int cb) {
  size_t f = op_conv_wgrad_ws_floats(n, h, w, ca, cb);
  if (op_wgrad_split3_supported(n, h, w, ca, cb, 1)) f = std::max(f, op_wgrad_split3_ws_floats(n, h, w, ca, cb));
  return f;
}
// lo_silu: lo holds pre-activations, SiLU applied on load (the f32 kernel only)
static int wgrad(int n, int h, int w, int ca, int cb, const float* lo, int lda, const float* hi, int ldb, float* dw,
                 int cbo, float* ws, size_t ws_floats, hipStream_t s, int terms, int lo_silu = 0) {
  if (!lo_silu && op_wgrad_split3_supported(n, h, w, ca, cb, terms))
    return op_wgrad_split3(n, h, w, ca, cb, lo, lda, hi, ldb, dw, cbo, 1.0f, 0, ws, ws_floats, s, terms);
  return op_conv_wgrad(n, h, w, ca, cb, lo, lda, lo_silu, hi, ldb, dw, cbo, 1.0f, 0, ws, ws_floats, s);
}

static void mlp_bwd_carve(Carve& c, long long M1, int w1, int w2, MlpBwd& b) {
  b.gx2 = c.f(M1 * w2); b.gp2 = c.f(M1 * w2); b.gy2 = c.f(M1 * w2); b.xh2 = c.f(M1 * w2);
  b.gx1 = c.f(M1 * w1); b.gp1 = c.f(M1 * w1); b.gy1 = c.f(M1 * w1); b.xh1 = c.f(M1 * w1);
}

static long long wm_conv_scratch(const WmDims& D) {
  if (D.Dv) return 0;  // vector observations: no convolution planes
  const int n = D.M, n1 = D.M1, N = D.N;
  long long m = 0;
  auto mx = [&](long long v) { if (v > m) m = v; };
  for (int k = 0; k < N; ++k) {
    // encoder conv k: lo = output grad (res k + 1), hi = input; its bias sum
    mx(wgrad_ws_floats(n, D.IH >> (k + 1), D.IW >> (k + 1), D.e[k + 1], enc_cin_st(D, k)));
    mx(op_chan_sum_ws_floats((long long)n * D.pix[k + 1], D.e[k + 1]));
    // decoder convT k: lo = input (res N - k), hi = output grad; its bias sum
    mx(wgrad_ws_floats(n1, D.IH >> (N - k), D.IW >> (N - k), D.cd[k], dec_cout_st(D, k)));
    mx(op_chan_sum_ws_floats((long long)n1 * D.pix[N - k - 1], D.cd[k + 1]));
  }
  return m;
}

static void wm_carve(Carve& c, const dr_dims* d, const WmDims& D, WmWs& w) {
  memset(&w, 0, sizeof(w));
  const long long M = D.M, M1 = D.M1, B = D.B;
  const int L = D.L, Hd = D.Hd, A = D.A, eh = D.eh, N = D.N;
  const long long Dv = D.Dv;
  WmHead hs[3];
  wm_heads(D, nullptr, nullptr, hs);
  w.x0 = c.f(Dv ? M * Dv : M * D.pix[0] * 4);
  w.s3m0 = c.raw(op_nt_split3_ws_bytes(eh, Hd));
  w.s3whh = c.raw(op_nt_split3_ws_bytes(3 * Hd, Hd));
  w.s3wtb = c.raw(op_nt_split3_ws_bytes(L, 3 * Hd));
  for (HeadWs& h : w.head) {
    h.pl_h3 = c.raw(op_nt_split3_ws_bytes(std::max(D.ph1, std::max(D.rh1, D.ch1)),
                                          std::max(D.ph2, std::max(D.rh2, D.ch2))));
    h.pl_h0 = c.raw(op_nt_split3_ws_bytes(Hd + L, std::max(D.ph1, std::max(D.rh1, D.ch1))));
  }
  w.head[0].pl_h6 = c.raw(op_nt_split3_ws_bytes(D.ph2, L));
  if (!Dv) {
    w.pl_up3 = c.raw(op_nt_split3_ws_bytes(D.dh, D.Fd));
    w.pl_up0 = c.raw(op_nt_split3_ws_bytes(Hd + L, D.dh));
  }
  w.pl_w0tp = c.raw(op_nt_split3_ws_bytes(D.F, eh));
  {
    const int h1 = std::max(D.ph1, std::max(D.rh1, std::max(D.ch1, D.dh)));
    const int h2 = std::max(D.ph2, std::max(D.rh2, D.ch2));
    for (HeadWs& h : w.head) h.pl_f0 = c.raw(op_nt_split3_ws_bytes(h1, Hd + L));
    w.pl_fup0 = c.raw(op_nt_split3_ws_bytes(h1, Hd + L));
    for (HeadWs& h : w.head) h.pl_f3 = c.raw(op_nt_split3_ws_bytes(h2, h1));
    w.head[0].pl_f6 = c.raw(op_nt_split3_ws_bytes(L, D.ph2));
    if (!Dv) w.pl_fup3 = c.raw(op_nt_split3_ws_bytes(D.Fd, D.dh));
  }
  w.pl_map0f = c.raw(op_nt_split3_ws_bytes(eh, D.F));
  w.s3twhh = c.raw(op_nt_split3_ws_bytes(Hd, 3 * Hd));
  if (Dv) {  // MLP stand-in: layer 0 and the last layer of the conv slots, [M][F] each
    w.pre[0] = c.f(M * D.F); w.a[0] = c.f(M * D.F);
    w.pre[N - 1] = c.f(M * D.F); w.a[N - 1] = c.f(M * D.F);
  } else {
    for (int k = 0; k < N; ++k) {
      w.pre[k] = c.f(M * D.pix[k + 1] * D.e[k + 1]);
      w.a[k] = c.f(M * D.pix[k + 1] * D.e[k + 1]);
    }
  }
  w.feat = c.f(M * eh);
  for (int k = 0; k < N; ++k) {
    w.wr[k] = c.f((long long)D.e[k + 1] * 16 * enc_cin_st(D, k));
    if (k > 0) w.wqe[k] = c.f((long long)16 * D.e[k + 1] * D.e[k]);
  }
  w.act_tm = c.f(M * A); w.rew_tm = c.f(M); w.cont_tm = c.f(M);
  w.zeros = c.f(B * (L + A + Hd));
  w.h_all = c.f(M * Hd); w.z_all = c.f(M * L); w.soft = c.f(M * L); w.plog = c.f(M * L);
  w.pre_m = c.f(M * eh); w.x_m = c.f(M * eh);
  w.sr = c.f(M * Hd); w.su = c.f(M * Hd); w.sn = c.f(M * Hd); w.sghn = c.f(M * Hd);
  w.gi = c.f(B * 3 * Hd); w.gh = c.f(B * 3 * Hd);
  w.wt = c.f((long long)(L + A) * 3 * Hd);
  w.idx = c.i((long long)D.T * 2 * B * d->rows);
  for (int i = 0; i < 3; ++i) {
    HeadWs& h = w.head[i];
    h.p1 = c.f(M1 * hs[i].w1); h.x1 = c.f(M1 * hs[i].w1); h.p2 = c.f(M1 * hs[i].w2); h.x2 = c.f(M1 * hs[i].w2);
    h.lg = c.f(M1 * hs[i].nout);
  }
  w.du1 = c.f(M1 * D.dh); w.dx1 = c.f(M1 * D.dh); w.du2 = c.f(M1 * D.Fd); w.du2p = c.f(M1 * D.Fd);
  if (Dv) {  // dq[0] / dqp[0] = image_builder.0 pre / post SiLU [M1][Fd], dq[1] = the output mu [M1][Dv]
    w.dq[0] = c.f(M1 * D.Fd); w.dqp[0] = c.f(M1 * D.Fd); w.dq[1] = c.f(M1 * Dv);
    w.dgq[0] = c.f(M1 * D.Fd);
  } else {
    for (int k = 0; k + 1 < N; ++k) {  // convT k output at resolution level N - k - 1
      const long long sz = M1 * D.pix[N - k - 1] * D.cd[k + 1];
      // the last layer's input is never stored post-SiLU: its two readers (the
      // fused tanh-MSE layer, its weight gradient) apply SiLU on load -- the
      // 32-channel activation (B = 256: 470 MB) written once less
      w.dq[k] = c.f(sz); w.dqp[k] = k == N - 2 ? nullptr : c.f(sz); w.dgq[k] = c.f(sz);
    }
  }
  w.dgout = c.f(Dv ? M1 * Dv : M1 * D.pix[0] * 4);
  w.w3p = c.f((long long)D.Fd * D.dh); w.b3p = c.f(D.Fd);
  for (int k = 0; k < N; ++k) {
    w.wqd[k] = c.f((long long)16 * D.cd[k] * D.cd[k + 1]);
    w.wrd[k] = c.f((long long)16 * D.cd[k] * dec_cout_st(D, k));
  }
  for (int k = 0; k < N; ++k) {  // 3 bf16 planes = 1.5 floats per weight
    w.s3e[k] = enc_s3(D, k) ? c.f((3LL * 16 * D.e[k] * D.e[k + 1] + 1) / 2) : nullptr;
    w.s3d[k] = dec_s3(D, k) ? c.f((3LL * 16 * D.cd[k] * D.cd[k + 1] + 1) / 2) : nullptr;
    w.t3d[k] = dect_s3(D, k) ? c.f((3LL * 16 * D.cd[k] * D.cd[k + 1] + 1) / 2) : nullptr;
    w.t3e[k] = encg_s3(D, k) ? c.f((3LL * 16 * D.e[k] * D.e[k + 1] + 1) / 2) : nullptr;
  }
  w.coef_row = c.f(M1); w.coef_obs = c.f(M1);
  w.obs_part = c.f(Dv ? M1 : M1 * op_convT_mse_parts(D.IH / 2, D.IW / 2));
  // the last decoder layer's bias-gradient partials (k_convT_out3), 3 per tile
  w.obs_bpart = Dv ? nullptr : c.f(3LL * M1 * op_convT_mse_parts(D.IH / 2, D.IW / 2));
  w.csp = Dv ? nullptr : c.f(((long long)M1 * (D.IH / 2) * (D.IW / 2) + 127) / 128 * D.cd[N - 1]);
  w.kl_grp = c.f(M1 * d->rows); w.rew_row = c.f(M1); w.cont_row = c.f(M1); w.scal = c.f(8); w.stats = c.f(8);
  w.gH = c.f(M * Hd); w.gZ = c.f(M * L); w.glog = c.f(M * L); w.gpost = c.f(M1 * L);
  for (int i = 0; i < 3; ++i) w.head[i].g = c.f(M1 * hs[i].nout);
  for (int i = 0; i < 3; ++i) mlp_bwd_carve(c, M1, hs[i].w1, hs[i].w2, w.head[i].b);
  w.gxu = c.f(M1 * D.dh); w.gpu = c.f(M1 * D.dh); w.gyu = c.f(M1 * D.dh); w.xhu = c.f(M1 * D.dh);
  w.dgu2 = c.f(M1 * D.Fd);
  w.dw3p = c.f((long long)D.Fd * D.dh); w.db3p = c.f(D.Fd);
  w.ggi = c.f(M * 3 * Hd); w.ggh = c.f(M * 3 * Hd);
  w.gpre_m = c.f(M * eh); w.gy_m = c.f(M * eh); w.xh_m = c.f(M * eh);
  w.gx_s = c.f(B * eh); w.gh_dummy = c.f(B * Hd);
  if (Dv) {
    w.gp[0] = c.f(M * D.F); w.gp[N - 1] = c.f(M * D.F);
  } else {
    for (int k = 0; k < N; ++k) w.gp[k] = c.f(M * D.pix[k + 1] * D.e[k + 1]);
  }
  for (int i = 0; i < 3; ++i) {
    HeadWs& h = w.head[i];
    h.t6 = c.f((long long)hs[i].nout * hs[i].w2); h.t3 = c.f((long long)hs[i].w2 * hs[i].w1);
    h.t0 = c.f((long long)hs[i].w1 * head_in(D, hs[i]));
  }
  w.t_up3 = c.f((long long)D.Fd * D.dh); w.t_up0 = c.f((long long)D.dh * (Hd + L));
  w.t_map3 = c.f((long long)L * eh); w.t_map0 = c.f((long long)eh * (D.F + Hd));
  w.t_whh = c.f((long long)3 * Hd * Hd); w.w0tp = c.f((long long)D.F * eh);
  w.e12w1 = D.Dv ? nullptr : c.raw((size_t)D.e[1] * 64 * 6);
  w.cws_n = wm_conv_scratch(D);
  w.cws = c.f(w.cws_n);
  {
    const long long hd = D.Hd, L = D.L, eh = D.eh;
    long long mx = splitk_floats(1, L * eh + eh * (D.F + hd) + 3 * hd * (L + D.A) + 3 * hd * hd);
    mx = std::max(mx, splitk_floats(1, (long long)D.Fd * D.dh + (long long)D.dh * (hd + L)));
    mx = std::max(mx, splitk_floats(M, std::max(eh, (long long)D.dh)));
    // the forward heads' four first Linears, each with its own slice (split-K
    // of their K = Hd + L products on the split3 tall GEMM)
    mx = std::max(mx, splitk_floats(D.M1, (long long)D.ph1 + D.rh1 + D.ch1 + D.dh));
    mx = std::max(mx, splitk_floats(1, (long long)D.nb * D.rh2 + (long long)D.rh2 * D.rh1 + D.rh1 * (hd + L)));
    w.sk_n = mx;
    w.sk = c.f(w.sk_n);
  }
  {
    // split3 TN scratch: room for four of the largest weight-gradient problem
    // over K = M rows (tn_launch groups up to four per launch)
    const int hd = D.Hd, L = D.L, eh = D.eh;
    const int mn[][2] = {{D.nb, D.rh2}, {D.rh2, D.rh1}, {D.rh1, hd + L}, {1, D.ch2}, {D.ch2, D.ch1}, {D.ch1, hd + L},
                         {L, D.ph2}, {D.ph2, D.ph1}, {D.ph1, hd + L}, {D.Fd, D.dh}, {D.dh, hd + L}, {L, eh},
                         {eh, D.F + hd}, {3 * hd, L + D.A}, {3 * hd, hd}, {D.Dv, D.Fd}, {D.Fd, D.Fd}, {D.F, D.F},
                         {D.F, D.Dv}};
    size_t mx = 0;
    for (const auto& q : mn)
      if (q[0] > 0 && q[1] > 0) mx = std::max(mx, op_gemm_tn_split3_ws_bytes(q[0], q[1], M));
    w.tn_bytes = tn_group_bytes(mx, 4);
    w.tn = c.raw(w.tn_bytes);
  }
}

extern "C" size_t dr_wm_train_workspace_bytes(const dr_dims* d, int B, int T) {
  if (!d || B <= 0 || T < 2) return 0;
  Carve c(nullptr);
  WmWs w;
  wm_carve(c, d, wm_dims(d, B, T), w);
  return c.off;
}

// ---------------------------------------------------------------------------
// the training step, phase by phase: what the phases of one call share, built
// once by wm_run after the checks and the carve (cin_t / cout_t point into D:
// never copied)
// ---------------------------------------------------------------------------
struct WmCtx {
  const dr_dims* d;
  const dr_world_model *wm, *gw;  // weights / their gradients
  const dr_decoder *dec, *gd;
  WmDims D;
  WmWs w;
  WmHead head[3];  // prior, reward, continue (w.head[i] is head[i]'s workspace)
  const dr_frames* src;
  const dr_wm_batch* bt;
  dr_noise noise;
  dr_wm_loss_cfg cfg;
  float *stats, *losses;
  int rows_global, *skip;
  float *hiddens_out, *latents_out, *post_logits_out;  // optional
  hipStream_t s;
  const float *hB, *zB, *post1;  // rows t >= 1 of h_all / z_all / plog
  float *gHB, *gZB;              // ... of gH / gZ
  const int *cin_t, *cout_t;     // convT k: cd[k] -> cd[k + 1] channels
  WmCtx() = default;
  WmCtx(const WmCtx&) = delete;
};

static int silu(long long n, const float* x, float* y, hipStream_t s) {
  hipLaunchKernelGGL(k_silu, dim3(blocks(n, 256)), dim3(256), 0, s, n, x, y);
  return dr_check_launch("silu");
}
static int mul_dsilu(long long n, float* g, const float* pre, hipStream_t s) {
  hipLaunchKernelGGL(k_mul_dsilu, dim3(blocks(n, 256)), dim3(256), 0, s, n, g, pre);
  return dr_check_launch("mul_dsilu");
}
// Y[M][N] = A[M][K] W[K][N]: an input gradient against the weight as stored (the vector stand-ins' backward)
static int nn_product(int M, int N, int K, const float* A, const float* Wkn, float* Y, hipStream_t s) {
  GemmArgs g = gemm_args();
  g.M = M; g.N = N; g.K = K; g.A = A; g.lda = K; g.W = Wkn; g.ldb = N; g.Y = Y; g.ldy = N;
  return gemm_launch(G_NN, AM_PLAIN, &g, 1, s);
}

static int wm_prep(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_world_model* wm = x.wm; const dr_decoder* dec = x.dec;
  const int *cin_t = x.cin_t, *cout_t = x.cout_t;
  const int B = D.B, M = D.M, M1 = D.M1, L = D.L, Hd = D.Hd, A = D.A, eh = D.eh, F = D.F, N = D.N;
  // ---- weights: repacks, transposes, permutations (fixed for the call) ----
  if (!D.Dv) {
    // (the f32 layouts only for the layers without split planes: each repack is
    // a ~5 us launch, 13 of them per step unused, r04zd)
    for (int k = 0; k < N; ++k) {
      if (!w.s3e[k]) DR_TRY(op_conv_repack_pad(D.e[k + 1], D.e[k], enc_cin_st(D, k), wm->conv[k].w, w.wr[k], s));
      // Conv2d data gradient = upsampling conv with the weight read as [cin=co][cout=ci]
      if (k > 0 && !w.t3e[k]) DR_TRY(op_convT_repack(D.e[k + 1], D.e[k], wm->conv[k].w, w.wqe[k], s));
    }
    for (int k = 0; k < N; ++k) {
      if (k < N - 1) {
        if (!w.t3d[k]) DR_TRY(op_convT_repack(cin_t[k], cout_t[k], dec->convt[k].w, w.wqd[k], s));
      } else {
        DR_TRY(op_convT_out3_repack(cin_t[k], dec->convt[k].w, w.wqd[k], s));
      }
      // ConvTranspose2d data gradient = strided Conv2d with the weight read as [out=ci][in=co]
      if (!w.s3d[k]) DR_TRY(op_conv_repack_pad(cin_t[k], cout_t[k], dec_cout_st(D, k), dec->convt[k].w, w.wrd[k], s));
    }
    for (int k = 0; k < N; ++k) {
      if (w.s3e[k]) DR_TRY(op_conv_repack_split3(D.e[k + 1], D.e[k], wm->conv[k].w, w.s3e[k], s));
      if (w.s3d[k]) DR_TRY(op_conv_repack_split3(cin_t[k], cout_t[k], dec->convt[k].w, w.s3d[k], s));
      if (w.t3d[k]) DR_TRY(op_convT_repack_split3(cin_t[k], cout_t[k], dec->convt[k].w, w.t3d[k], s));
      if (w.t3e[k]) DR_TRY(op_convT_repack_split3(D.e[k + 1], D.e[k], wm->conv[k].w, w.t3e[k], s));
    }
  }
  // decoder.upscaler.3 rows to NHWC order (vector mode: Pf = 1, the identity), so its output is the first convT's NHWC input
  DR_TRY(perm_rows(D.C0, D.Pf, D.dh, dec->up3.w, w.w3p, 1, s));
  DR_TRY(perm_rows(D.C0, D.Pf, 1, dec->up3.b, w.b3p, 1, s));
  {
    TransposeJob tj[10];  // the heads' .6 / .3 / .0 in table order, then W_ih
    for (int i = 0; i < 3; ++i) {
      const WmHead& h = x.head[i]; const HeadWs& hw = w.head[i];
      tj[3 * i] = {h.nout, h.w2, h.nout, h.m->l6.w, hw.t6};
      tj[3 * i + 1] = {h.w2, h.w1, h.w2, h.m->l3.w, hw.t3};
      tj[3 * i + 2] = {h.w1, head_in(D, h), h.w1, h.m->l0.w, hw.t0};
    }
    tj[9] = {3 * Hd, L + A, 3 * Hd, wm->w_ih, w.wt};
    DR_TRY(op_transpose_multi(tj, 10, s));
    TransposeJob tj2[5] = {
        {D.Fd, D.dh, D.Fd, w.w3p, w.t_up3},          {D.dh, Hd + L, D.dh, dec->up0.w, w.t_up0},
        {L, eh, L, wm->map3.w, w.t_map3},            {eh, F + Hd, eh, wm->map0.w, w.t_map0},
        {3 * Hd, Hd, 3 * Hd, wm->w_hh, w.t_whh},
    };
    DR_TRY(op_transpose_multi(tj2, 5, s));
  }
  // latent_mapper.0 feature rows (of its transpose) to NHWC: dL/d conv4-out comes out NHWC
  DR_TRY(perm_rows(D.e[N], D.Pf, eh, w.t_map0, w.w0tp, 1, s));

  // ---- window data ----
  DR_TRY(wm_gather(B, D.T, A, *x.bt, w.act_tm, w.rew_tm, w.cont_tm, s));
  DR_TRY(zero(w.zeros, (long long)B * (L + A + Hd), s));
  return wm_masksum(M1, w.cont_tm, x.stats, s);
}

// vector observations, encoder stand-in: pre[0] = X W1^T + b1, a[0] = SiLU, pre[N-1] = a[0] W2^T + b2, a[N-1] = SiLU
static int wm_vec_encoder_fwd(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_world_model* wm = x.wm;
  const int M = D.M, F = D.F, Dv = D.Dv, N = D.N;
  DR_TRY(op_vec_gather(M, D.B, Dv, x.src, w.x0, s));
  DR_TRY(run(G_NT, AM_PLAIN, lin(M, F, Dv, w.x0, Dv, wm->conv[0].w, Dv, wm->conv[0].b, w.pre[0], F), s));
  DR_TRY(silu((long long)M * F, w.pre[0], w.a[0], s));
  DR_TRY(run(G_NT, AM_PLAIN, lin(M, F, F, w.a[0], F, wm->conv[1].w, F, wm->conv[1].b, w.pre[N - 1], F), s));
  return silu((long long)M * F, w.pre[N - 1], w.a[N - 1], s);
}

// ---- encoder over all M frames (VAE.py:57-75), activations kept ----
static int wm_fwd_encoder(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_world_model* wm = x.wm;
  const int B = D.B, M = D.M, Hd = D.Hd, eh = D.eh, F = D.F, IH = D.IH, IW = D.IW, N = D.N;
  // the forward's first launch: the rows' prediction-loss factors, from the (all-reduced) mask sum of wm_prep
  DR_TRY(wm_coef(D.M1, w.cont_tm, x.cfg.beta_pred, x.stats, w.scal, w.coef_row, w.coef_obs, s));
  float* aL = w.a[N - 1];  // the flattened features (NCHW; vector mode: the MLP's last activation)
  if (D.Dv) {
    DR_TRY(wm_vec_encoder_fwd(x));
  } else {
    // (conv1's weight gradient reads it; pad channel = 1: its bias gradient comes
    // out of the same product, enc_bias_fused below)
    DR_TRY(op_frames_nhwc4(M, B, IH, IW, x.src, w.x0, s, 1.0f));
    // conv1 + conv2 in one kernel from the u8 ring (k_enc12_split3_x8; bf16 mode: k_enc12_s1) with the
    // backward's saves; other shapes / sources take the per-layer kernels
    int k0 = 0;
    if (N >= 2 && w.e12w1 && w.s3e[1]) {
      // DR_E_INVALID: shape / source not covered (per-layer kernels below); any
      // other failure (a launch or occupancy query) is returned
      const int rc12 = op_enc12_split3_ex(M, B, IH, IW, D.e[1], D.e[2], x.src, wm->conv[0].w, wm->conv[0].b,
                                          wm->conv[1].w, wm->conv[1].b, w.e12w1, w.s3e[1], w.a[1], w.pre[0], w.a[0],
                                          w.pre[1], s, D.terms);
      if (rc12 == DR_OK) k0 = 2;
      else if (rc12 != DR_E_INVALID) return rc12;
    }
    for (int k = k0; k < N; ++k) {
      if (w.s3e[k])
        DR_TRY(op_conv_split3_ex(M, D.e[k], IH >> k, IW >> k, D.e[k + 1], w.a[k - 1], w.s3e[k], wm->conv[k].b, w.a[k],
                                 k == N - 1 ? 1 : 0, w.pre[k], CONV_EPI_FWD, s, D.terms));
      else
        DR_TRY(op_conv_nhwc_ex(M, enc_cin_st(D, k), IH >> k, IW >> k, D.e[k + 1], k ? w.a[k - 1] : w.x0, w.wr[k],
                               wm->conv[k].b, w.a[k], k == N - 1 ? 1 : 0, w.pre[k], CONV_EPI_FWD, s));
    }
  }
  GemmArgs g = lin(M, eh, F, aL, F, wm->map0.w, F + Hd, wm->map0.b, w.feat, eh);
  splitk_all(&g, 1, w.sk, w.sk_n);
  if (M >= 1024) {  // the feature projection on split3 planes (as the epoch's warm-start encoder)
    DR_TRY(op_nt_repack_split3(eh, F, wm->map0.w, F + Hd, w.pl_map0f, s));
    wplanes(g, w.pl_map0f);
  }
  return run(G_NT, AM_PLAIN, g, s);
}

// ---- posterior scan (unroll_model, WorldModel.py:97-107) ----
static int wm_fwd_scan(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_dims* d = x.d; const dr_world_model* wm = x.wm;
  const int B = D.B, T = D.T, L = D.L, Hd = D.Hd, A = D.A, eh = D.eh, F = D.F;
  const long long idx_stride = 2LL * B * d->rows;
  // B >= 128 (split GRU): the next step's hidden product h W_hh^T + b_hh rides
  // in the same grouped launch as latent_mapper.0 (both read only h_t)
  bool gh_pre = false;
  // B >= 128: the grouped per-step products on the split3 wave-K kernel from
  // weight planes split once per step (f32-accurate): 12.8 us per launch against
  // the f32 k_gemm_wk's 23.5 (WM step bf16 9.22 -> 9.17 ms, fp32 unchanged, r06m)
  // (bf16 mode keeps the six products here: one-term scan products measured
  // 8.46 -> 8.36 ms per bf16 WM step but took the posterior flip fraction against
  // the fp32 oracle from ~2e-4 to 1.8e-3 of its 2e-3 bound, profiles/r06z9_ab_wm_scan_one_term.txt)
  const bool planes = B >= 128 && T > 1 && Hd % 8 == 0;
  if (planes) {
    DR_TRY(split_planes(eh, Hd, wm->map0.w + F, F + Hd, w.s3m0, s));
    DR_TRY(split_planes(3 * Hd, Hd, wm->w_hh, Hd, w.s3whh, s));
  }
  for (int t = 0; t < T; ++t) {
    const long long rb = (long long)t * B;
    float* h_t = w.h_all + rb * Hd;
    float* z_t = w.z_all + rb * L;
    if (t == 0) {  // GRU from z = 0, a = 0, h = 0
      DR_TRY(gru_step(d, wm, B, w.zeros, L, w.zeros + (long long)B * L, A, w.zeros + (long long)B * (L + A), Hd, h_t,
                      Hd, w.gi, w.gh, w.sr, w.su, w.sn, w.sghn, s));
    } else {
      DR_TRY(gru_onehot(d, wm, B, w.idx + (t - 1) * idx_stride, w.act_tm + (rb - B) * A, A, h_t - (long long)B * Hd,
                        Hd, h_t, Hd, w.wt, w.sr + rb * Hd, w.su + rb * Hd, w.sn + rb * Hd, w.sghn + rb * Hd, s,
                        nullptr, 0, w.gh, gh_pre));
    }
    GemmArgs g[2];
    g[0] = lin(B, eh, Hd, h_t, Hd, wm->map0.w + F, F + Hd, nullptr, w.pre_m + rb * eh, eh);
    g[0].addend = w.feat + rb * eh;
    g[0].ld_add = eh;
    gh_pre = B >= 128 && t + 1 < T;
    if (gh_pre) g[1] = lin(B, 3 * Hd, Hd, h_t, Hd, wm->w_hh, Hd, wm->b_hh, w.gh, 3 * Hd);
    if (planes) {
      wplanes(g[0], w.s3m0);
      if (gh_pre) wplanes(g[1], w.s3whh);
    }
    DR_TRY(gemm_launch(G_NT, AM_PLAIN, g, gh_pre ? 2 : 1, s));
    GemmArgs gp = lin_ln(B, L, eh, w.pre_m + rb * eh, eh, wm->map1, wm->map3.w, wm->map3.b, w.plog + rb * L, L);
    gp.a_out = w.x_m + rb * eh;
    gp.ld_aout = eh;
    with_sampler(gp, d, x.noise, t, z_t, L, w.idx + t * idx_stride, w.soft + rb * L, L);
    DR_TRY(run(G_NT, AM_LNSILU, gp, s));
  }
  return DR_OK;
}

// ---- heads on rows t >= 1 (WorldModel.py:116-119) ----
// three grouped launches, one per layer, the heads in table order; the first
// carries decoder.upscaler.0 as its fourth problem
static int wm_fwd_heads(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_decoder* dec = x.dec;
  const int M1 = D.M1, L = D.L, Hd = D.Hd;
  const bool tall = M1 >= 1024;  // on split3 planes of the weights (gemm.hip s3_tall_ok), split per step
  GemmArgs p[4];
  for (int i = 0; i < 3; ++i) {
    const WmHead& h = x.head[i]; const HeadWs& hw = w.head[i];
    p[i] = h.in_z ? lin2(M1, h.w1, x.hB, Hd, Hd, x.zB, L, L, h.m->l0.w, h.m->l0.b, hw.p1, h.w1)
                  : lin(M1, h.w1, Hd, x.hB, Hd, h.m->l0.w, Hd, h.m->l0.b, hw.p1, h.w1);
    if (tall) {
      DR_TRY(op_nt_repack_split3(h.w1, head_in(D, h), h.m->l0.w, head_in(D, h), hw.pl_f0, s));
      wplanes(p[i], hw.pl_f0);
    }
  }
  p[3] = lin2(M1, D.dh, x.hB, Hd, Hd, x.zB, L, L, dec->up0.w, dec->up0.b, w.du1, D.dh);
  if (tall) {
    DR_TRY(op_nt_repack_split3(D.dh, Hd + L, dec->up0.w, Hd + L, w.pl_fup0, s));
    wplanes(p[3], w.pl_fup0);
    splitk_all(p, 4, w.sk, w.sk_n);
  }
  DR_TRY(gemm_launch(G_NT, AM_PLAIN, p, 4, s));
  for (int i = 0; i < 3; ++i) {
    const WmHead& h = x.head[i]; const HeadWs& hw = w.head[i];
    p[i] = lin_ln(M1, h.w2, h.w1, hw.p1, h.w1, h.m->n1, h.m->l3.w, h.m->l3.b, hw.p2, h.w2);
    p[i].a_out = hw.x1; p[i].ld_aout = h.w1;
    if (tall) {
      DR_TRY(op_nt_repack_split3(h.w2, h.w1, h.m->l3.w, h.w1, hw.pl_f3, s));
      wplanes(p[i], hw.pl_f3);
    }
  }
  DR_TRY(gemm_launch(G_NT, AM_LNSILU, p, 3, s));
  for (int i = 0; i < 3; ++i) {
    const WmHead& h = x.head[i]; const HeadWs& hw = w.head[i];
    p[i] = lin_ln(M1, h.nout, h.w2, hw.p2, h.w2, h.m->n4, h.m->l6.w, h.m->l6.b, hw.lg, h.nout);
    p[i].a_out = hw.x2; p[i].ld_aout = h.w2;
    // (the prior's 1024 outputs; the reward's 255 / continue's 1 stay on the tile kernel: no pl_f6)
    if (tall && hw.pl_f6) {
      DR_TRY(op_nt_repack_split3(h.nout, h.w2, h.m->l6.w, h.w2, hw.pl_f6, s));
      wplanes(p[i], hw.pl_f6);
    }
  }
  return gemm_launch(G_NT, AM_LNSILU, p, 3, s);
}

// vector observations, image_builder stand-in: q = SiLU(du2) Wd1^T + bd1, mu = SiLU(q) Wd2^T + bd2; squared error
// vs rows t >= 1
static int wm_vec_decoder_fwd(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_decoder* dec = x.dec;
  const int M1 = D.M1, Dv = D.Dv;
  const long long MF = (long long)M1 * D.Fd;
  DR_TRY(silu(MF, w.du2, w.du2p, s));
  DR_TRY(run(G_NT, AM_PLAIN, lin(M1, D.Fd, D.Fd, w.du2p, D.Fd, dec->convt[0].w, D.Fd, dec->convt[0].b, w.dq[0], D.Fd), s));
  DR_TRY(silu(MF, w.dq[0], w.dqp[0], s));
  DR_TRY(run(G_NT, AM_PLAIN, lin(M1, Dv, D.Fd, w.dqp[0], D.Fd, dec->convt[1].w, D.Fd, dec->convt[1].b, w.dq[1], Dv), s));
  return vec_mse(M1, Dv, w.dq[1], w.x0 + (long long)D.B * Dv, w.coef_obs, w.dgout, w.obs_part, s);
}

// convT k of the decoder over n frames: geometry, weights and bias (the caller sets the input and the outputs)
static ConvTArgs dec_convt_args(const WmDims& D, int n, int k, const float* wq, const float* bias) {
  ConvTArgs a = {};
  a.n = n; a.cin = D.cd[k]; a.h = D.IH >> (D.N - k); a.w = D.IW >> (D.N - k); a.cout = D.cd[k + 1];
  a.wq = wq; a.bias = bias;
  return a;
}

// decoder (VAE.py:139-161): upscaler.3 pre-activation in NHWC, SiLU applied by the consumers
static int wm_fwd_decoder(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_decoder* dec = x.dec;
  const int M1 = D.M1, N = D.N;
  GemmArgs g = lin_ln(M1, D.Fd, D.dh, w.du1, D.dh, dec->up1, w.w3p, w.b3p, w.du2, D.Fd);
  g.a_out = w.dx1; g.ld_aout = D.dh;
  if (M1 >= 1024 && !D.Dv) {
    DR_TRY(op_nt_repack_split3(D.Fd, D.dh, w.w3p, D.dh, w.pl_fup3, s));
    wplanes(g, w.pl_fup3);
  }
  DR_TRY(run(G_NT, AM_LNSILU, g, s));
  if (D.Dv) return wm_vec_decoder_fwd(x);
  DR_TRY(silu((long long)M1 * D.Fd, w.du2, w.du2p, s));
  for (int k = 0; k < N; ++k) {
    ConvTArgs a = dec_convt_args(D, M1, k, w.wqd[k], dec->convt[k].b);
    a.in = k ? w.dqp[k - 1] : w.du2p;
    if (k == N - 1 && k > 0) {  // SiLU of the pre-activations on load (dqp[N - 2] is not stored)
      a.in = w.dq[k - 1];
      a.silu_in = 1;
    }
    if (k < N - 1) {
      a.out = w.dq[k]; a.out2 = w.dqp[k]; a.ldc = x.cout_t[k];
      if (w.t3d[k]) DR_TRY(op_convT_split3(CT_EPI_BIAS, a, w.t3d[k], s, D.terms));
      else DR_TRY(op_convT_nhwc(CT_EPI_BIAS, a, s));
    } else {
      // Tanh + squared error against frames t >= 1 (WorldModel.py:129); writes dL/d(pre-tanh)
      a.out = w.dgout; a.ldc = 4;
      a.target = w.x0 + (long long)D.B * D.pix[0] * 4; a.tstride = 4;
      a.coef = w.coef_obs; a.part = w.obs_part; a.bpart = w.obs_bpart;
      DR_TRY(op_convT_nhwc(CT_EPI_TANH_MSE, a, s));
    }
  }
  return DR_OK;
}

// ---- losses ----
static int wm_fwd_losses(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_dims* d = x.d;
  const int M = D.M, M1 = D.M1, L = D.L, Hd = D.Hd, R = d->rows;
  DR_TRY(wm_kl_fwd(M1, R, d->cols, w.head[0].lg, x.post1, w.kl_grp, s));
  DR_TRY(wm_heads_loss(M1, D.nb, w.head[1].lg, w.head[2].lg, w.rew_tm, w.cont_tm, x.wm->buckets_rew, w.coef_row,
                       w.rew_row, w.cont_row, w.head[1].g, w.head[2].g, s));
  DR_TRY(wm_stats(M1, R, D.Dv ? 1 : op_convT_mse_parts(D.IH / 2, D.IW / 2), w.obs_part, w.rew_row, w.cont_row, w.kl_grp,
                  w.cont_tm, x.stats, s));
  if (x.hiddens_out) DR_TRY(copy2d(x.hiddens_out, Hd, w.h_all, Hd, Hd, M, s));
  if (x.latents_out) DR_TRY(copy2d(x.latents_out, L, w.z_all, L, L, M, s));
  if (x.post_logits_out) DR_TRY(copy2d(x.post_logits_out, L, w.plog, L, L, M, s));
  return DR_OK;
}

// input-gradient + weight-gradient pass of one head MLP (Linear-LN-SiLU x2 +
// Linear) over M1 rows whose input is [h | z] (in_z = 0: h only).  Adds the
// input gradient into gH/gZ rows t >= 1.
static int head_bwd(const WmCtx& x, int i) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const WmHead& h = x.head[i]; const HeadWs& hw = w.head[i]; const MlpBwd& b = hw.b;
  const dr_mlp3 &m = *h.m, &g = *h.g;
  const int w1 = h.w1, w2 = h.w2, nout = h.nout, in_z = h.in_z, n0 = head_in(D, h);
  const int M1 = D.M1, Hd = D.Hd, L = D.L;
  // tall (>= 1024 rows): the input-gradient products on split3 planes of the
  // transposed weights, split here (the weights change every step)
  const bool tall = M1 >= 1024;
  void* pl6 = tall && nout % 4 == 0 ? hw.pl_h6 : nullptr;
  void* pl3 = tall ? hw.pl_h3 : nullptr;
  void* pl0 = tall ? hw.pl_h0 : nullptr;
  if (pl6) DR_TRY(op_nt_repack_split3(w2, nout, hw.t6, nout, pl6, s));
  if (pl3) DR_TRY(op_nt_repack_split3(w1, w2, hw.t3, w2, pl3, s));
  if (pl0) DR_TRY(op_nt_repack_split3(n0, w1, hw.t0, w1, pl0, s));
  {
    GemmArgs g6 = bwd_nt(M1, w2, nout, hw.g, nout, hw.t6, b.gx2, w2, 0);
    wplanes(g6, pl6);
    DR_TRY(run(G_NT, AM_PLAIN, g6, s));
  }
  DR_TRY(lnbwd_nt(M1, w1, w2, b.gx2, w2, hw.p2, w2, m.n4, hw.t3, b.gx1, w1, 0, b.gp2, w2, b.gy2, b.xh2, nullptr, 0,
                  INT_MAX, s, nullptr, pl3, w.sk, w.sk_n));
  DR_TRY(lnbwd_nt(M1, n0, w1, b.gx1, w1, hw.p1, w1, m.n1, hw.t0, x.gHB, Hd, 1, b.gp1, w1, b.gy1, b.xh1,
                  in_z ? x.gZB : nullptr, L, in_z ? Hd : INT_MAX, s, nullptr, pl0, w.sk, w.sk_n));
  GemmArgs p[3];
  p[0] = bwd_w(nout, w2, M1, hw.g, nout, hw.x2, w2, g.l6.w);
  p[1] = bwd_w(w2, w1, M1, b.gp2, w2, hw.x1, w1, g.l3.w);
  p[2] = bwd_w(w1, n0, M1, b.gp1, w1, x.hB, Hd, g.l0.w);
  if (in_z) {
    p[2].W2 = x.zB; p[2].ldb2 = L; p[2].nsplitB = Hd;
  }
  splitk_all(p, 3, w.sk, w.sk_n);
  DR_TRY(tn_launch(p, 3, w.tn, w.tn_bytes, s, D.terms));
  ColsumJob cj[7] = {
      {nout, hw.g, nout, nullptr, 0, g.l6.b}, {w2, b.gp2, w2, nullptr, 0, g.l3.b},
      {w2, b.gy2, w2, b.xh2, w2, g.n4.w},     {w2, b.gy2, w2, nullptr, 0, g.n4.b},
      {w1, b.gp1, w1, nullptr, 0, g.l0.b},    {w1, b.gy1, w1, b.xh1, w1, g.n1.w},
      {w1, b.gy1, w1, nullptr, 0, g.n1.b},
  };
  return op_colsum_multi(M1, cj, 7, s);
}

// vector observations, image_builder stand-in backward: dgout = dL/dmu -> Wd2 / bd2 grads, dL/dq = (dgout Wd2) SiLU'(q)
// -> Wd1 / bd1 grads, dL/d du2 = (dL/dq Wd1) SiLU'(du2)  (NN products with the weights as stored)
static int wm_vec_decoder_bwd(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_decoder *dec = x.dec, *gd = x.gd;
  const int M1 = D.M1, Dv = D.Dv;
  const long long MF = (long long)M1 * D.Fd;
  DR_TRY(nn_product(M1, D.Fd, Dv, w.dgout, dec->convt[1].w, w.dgq[0], s));
  DR_TRY(mul_dsilu(MF, w.dgq[0], w.dq[0], s));
  DR_TRY(nn_product(M1, D.Fd, D.Fd, w.dgq[0], dec->convt[0].w, w.dgu2, s));
  DR_TRY(mul_dsilu(MF, w.dgu2, w.du2, s));
  GemmArgs p[2];
  p[0] = bwd_w(Dv, D.Fd, M1, w.dgout, Dv, w.dqp[0], D.Fd, gd->convt[1].w);
  p[1] = bwd_w(D.Fd, D.Fd, M1, w.dgq[0], D.Fd, w.du2p, D.Fd, gd->convt[0].w);
  splitk_all(p, 2, w.sk, w.sk_n);
  DR_TRY(tn_launch(p, 2, w.tn, w.tn_bytes, s, D.terms));
  ColsumJob cj[2] = {{Dv, w.dgout, Dv, nullptr, 0, gd->convt[1].b}, {D.Fd, w.dgq[0], D.Fd, nullptr, 0, gd->convt[0].b}};
  return op_colsum_multi(M1, cj, 2, s);
}

// decoder: image_builder.6 .. .0 (data grads as strided convs, weight grads, bias sums)
static int wm_bwd_decoder(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_decoder* gd = x.gd;
  const int *cin_t = x.cin_t, *cout_t = x.cout_t;
  const int M1 = D.M1, IH = D.IH, IW = D.IW, N = D.N;
  if (D.Dv) return wm_vec_decoder_bwd(x);
  bool csum_next = false;  // gout of this layer was summed per tile by the layer above's input-gradient conv
  for (int k = N - 1; k >= 0; --k) {
    const int ih = IH >> (N - 1 - k), iw = IW >> (N - 1 - k);  // output (high-res) size of convT k
    const int co = cout_t[k], co_st = dec_cout_st(D, k);
    float* gin = k ? w.dgq[k - 1] : w.dgu2;              // dL/d(pre-activation) of convT k's input
    const float* pre = k ? w.dq[k - 1] : w.du2;
    // input of convT k after SiLU; the last layer's is recomputed from dq (not stored)
    const bool post_silu = k == N - 1 && k > 0;
    const float* post = post_silu ? w.dq[k - 1] : k ? w.dqp[k - 1] : w.du2p;
    const float* gout = k < N - 1 ? w.dgq[k] : w.dgout;  // dL/d(convT k's output pre-activation)
    // the f32 4-channel input-gradient conv of the last layer also sums its
    // output per tile: the bias gradient of convT k - 1 without re-reading
    // that 0.5 GB gradient (csum_next below)
    const bool csum_here = !w.s3d[k] && k == N - 1 && k > 0;
    if (w.s3d[k])
      DR_TRY(op_conv_split3_ex(M1, co_st, ih, iw, cin_t[k], gout, w.s3d[k], nullptr, gin, 0, const_cast<float*>(pre),
                               CONV_EPI_DSILU, s, D.terms));
    else
      DR_TRY(op_conv_nhwc_ex(M1, co_st, ih, iw, cin_t[k], gout, w.wrd[k], nullptr, gin, 0, const_cast<float*>(pre),
                             CONV_EPI_DSILU, s, csum_here ? w.csp : nullptr));
    DR_TRY(wgrad(M1, ih / 2, iw / 2, cin_t[k], co_st, post, cin_t[k], gout, co_st, gd->convt[k].w, co, w.cws, w.cws_n,
                 s, D.terms, post_silu ? 1 : 0));
    // (the per-tile partials -- 1.5e4 / 2.9e4 rows -- go through the same
    // two-pass channel sum: one workgroup per channel over them took 40-70 us)
    if (k == N - 1 && co == 3)  // the tanh-MSE layer summed its gradient per tile (k_convT_out3)
      DR_TRY(op_chan_sum((long long)M1 * op_convT_mse_parts(ih / 2, iw / 2), 3, w.obs_bpart, 3, gd->convt[k].b, 0,
                         w.cws, w.cws_n, s));
    else if (csum_next)
      DR_TRY(op_chan_sum(((long long)M1 * ih * iw + 127) / 128, co, w.csp, co, gd->convt[k].b, 0, w.cws, w.cws_n, s));
    else
      DR_TRY(op_chan_sum((long long)M1 * ih * iw, co, gout, co_st, gd->convt[k].b, 0, w.cws, w.cws_n, s));
    csum_next = csum_here;
  }
  return DR_OK;
}

// decoder.upscaler: .3 (permuted rows) then LN-SiLU(.1) and .0 into dL/d[h | z]
static int wm_bwd_upscaler(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_decoder* gd = x.gd;
  const int M1 = D.M1, L = D.L, Hd = D.Hd;
  GemmArgs g = bwd_nt(M1, D.dh, D.Fd, w.dgu2, D.Fd, w.t_up3, w.gxu, D.dh, 0);
  splitk_all(&g, 1, w.sk, w.sk_n);
  if (M1 >= 1024) {
    DR_TRY(op_nt_repack_split3(D.dh, D.Fd, w.t_up3, D.Fd, w.pl_up3, s));
    DR_TRY(op_nt_repack_split3(Hd + L, D.dh, w.t_up0, D.dh, w.pl_up0, s));
    wplanes(g, w.pl_up3);
  }
  DR_TRY(run(G_NT, AM_PLAIN, g, s));
  DR_TRY(lnbwd_nt(M1, Hd + L, D.dh, w.gxu, D.dh, w.du1, D.dh, x.dec->up1, w.t_up0, x.gHB, Hd, 1, w.gpu, D.dh, w.gyu,
                  w.xhu, x.gZB, L, Hd, s, nullptr, M1 >= 1024 ? w.pl_up0 : nullptr, w.sk, w.sk_n));
  GemmArgs p[2];
  p[0] = bwd_w(D.Fd, D.dh, M1, w.dgu2, D.Fd, w.dx1, D.dh, w.dw3p);
  p[1] = bwd_w(D.dh, Hd + L, M1, w.gpu, D.dh, x.hB, Hd, gd->up0.w);
  p[1].W2 = x.zB; p[1].ldb2 = L; p[1].nsplitB = Hd;
  splitk_all(p, 2, w.sk, w.sk_n);
  DR_TRY(tn_launch(p, 2, w.tn, w.tn_bytes, s, D.terms));
  ColsumJob cj[4] = {
      {D.Fd, w.dgu2, D.Fd, nullptr, 0, w.db3p},
      {D.dh, w.gpu, D.dh, nullptr, 0, gd->up0.b},
      {D.dh, w.gyu, D.dh, w.xhu, D.dh, gd->up1.w},
      {D.dh, w.gyu, D.dh, nullptr, 0, gd->up1.b},
  };
  DR_TRY(op_colsum_multi(M1, cj, 4, s));
  DR_TRY(perm_rows(D.C0, D.Pf, D.dh, w.dw3p, gd->up3.w, 0, s));
  return perm_rows(D.C0, D.Pf, 1, w.db3p, gd->up3.b, 0, s);
}

// ---- backward: losses, then the heads, decoder and upscaler (rows t >= 1) into dL/dh, dL/dz ----
static int wm_bwd_heads(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_dims* d = x.d;
  const int M1 = D.M1, R = d->rows;
  DR_TRY(wm_final(x.stats, x.rows_global, x.cfg, w.scal, x.losses, x.skip, s));
  DR_TRY(wm_kl_bwd(M1, R, d->cols, w.head[0].lg, x.post1, w.cont_tm, w.scal, w.head[0].g, w.gpost, s));
  DR_TRY(zero(w.gH, (long long)D.M * D.Hd, s));
  DR_TRY(zero(w.gZ, (long long)D.M * D.L, s));
  for (int i = 0; i < 3; ++i) DR_TRY(head_bwd(x, i));
  DR_TRY(wm_bwd_decoder(x));
  return wm_bwd_upscaler(x);
}

// ---- backward through the posterior scan, t = T-1 .. 0 ----
static int wm_bwd_scan(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_dims* d = x.d; const dr_world_model *wm = x.wm, *gw = x.gw;
  const int B = D.B, T = D.T, M = D.M, M1 = D.M1, L = D.L, Hd = D.Hd, A = D.A, eh = D.eh, F = D.F, N = D.N;
  const int R = d->rows;
  // B >= 128: the per-step input-gradient products (K = 3 Hd) on the split3
  // wave-K kernel from weight planes split once per step (the f32 wave-K
  // kernel took 30.7 us per grouped launch at B = 256)
  const bool bplanes = B >= 128 && T > 1 && (3 * Hd) % 8 == 0;
  if (bplanes) {
    DR_TRY(split_planes(L, 3 * Hd, w.wt, 3 * Hd, w.s3wtb, s));
    DR_TRY(split_planes(Hd, 3 * Hd, w.t_whh, 3 * Hd, w.s3twhh, s));
  }
  for (int t = T - 1; t >= 0; --t) {
    const long long rb = (long long)t * B;
    float* gH_t = w.gH + rb * Hd;
    // straight-through sampler (+ KL-rep on rows t >= 1) -> dL/d logits
    DR_TRY(ste_bwd_add(B, R, d->cols, w.gZ + rb * L, (long long)L, w.soft + rb * L, (long long)L,
                       t > 0 ? w.gpost + (rb - B) * L : nullptr, (long long)L, w.glog + rb * L, (long long)L, s));
    // latent_mapper.3, then LN-SiLU(.1) fused into latent_mapper.0's h-columns input gradient
    DR_TRY(run(G_NT, AM_PLAIN, bwd_nt(B, eh, L, w.glog + rb * L, L, w.t_map3, w.gx_s, eh, 0), s));
    DR_TRY(lnbwd_nt(B, Hd, eh, w.gx_s, eh, w.pre_m + rb * eh, eh, wm->map1, w.t_map0 + (long long)F * eh, gH_t, Hd, 1,
                    w.gpre_m + rb * eh, eh, w.gy_m + rb * eh, w.xh_m + rb * eh, nullptr, 0, INT_MAX, s));
    // GRU (SequenceModel.py:19-24): h_t = GRU([z_{t-1}, a_{t-1}], h_{t-1})
    const float* hprev = t > 0 ? w.h_all + (rb - B) * Hd : w.zeros + (long long)B * (L + A);
    DR_TRY(op_gru_bwd(B, Hd, gH_t, Hd, hprev, Hd, w.sr + rb * Hd, w.su + rb * Hd, w.sn + rb * Hd, w.sghn + rb * Hd,
                      w.ggi + rb * 3 * Hd, w.ggh + rb * 3 * Hd, t > 0 ? gH_t - (long long)B * Hd : w.gh_dummy, Hd,
                      t > 0 ? 1 : 0, s));
    if (t > 0) {
      GemmArgs p[2];
      p[0] = bwd_nt(B, L, 3 * Hd, w.ggi + rb * 3 * Hd, 3 * Hd, w.wt, w.gZ + (rb - B) * L, L, 1);
      p[1] = bwd_nt(B, Hd, 3 * Hd, w.ggh + rb * 3 * Hd, 3 * Hd, w.t_whh, gH_t - (long long)B * Hd, Hd, 1);
      if (bplanes) {
        wplanes(p[0], w.s3wtb);
        wplanes(p[1], w.s3twhh);
      }
      DR_TRY(gemm_launch(G_NT, AM_PLAIN, p, 2, s));
    }
  }
  // scan weight gradients over all rows
  GemmArgs p[4];
  p[0] = bwd_w(L, eh, M, w.glog, L, w.x_m, eh, gw->map3.w);
  p[1] = bwd_w(eh, F + Hd, M, w.gpre_m, eh, w.a[N - 1], F, gw->map0.w);
  p[1].W2 = w.h_all; p[1].ldb2 = Hd; p[1].nsplitB = F;
  p[2] = bwd_w(3 * Hd, L + A, M1, w.ggi + (long long)B * 3 * Hd, 3 * Hd, w.z_all, L, gw->w_ih);
  p[2].W2 = w.act_tm; p[2].ldb2 = A; p[2].nsplitB = L;
  p[3] = bwd_w(3 * Hd, Hd, M1, w.ggh + (long long)B * 3 * Hd, 3 * Hd, w.h_all, Hd, gw->w_hh);
  splitk_all(p, 4, w.sk, w.sk_n);
  DR_TRY(tn_launch(p, 4, w.tn, w.tn_bytes, s, D.terms));
  ColsumJob cj[6] = {
      {L, w.glog, L, nullptr, 0, gw->map3.b},       {eh, w.gpre_m, eh, nullptr, 0, gw->map0.b},
      {eh, w.gy_m, eh, w.xh_m, eh, gw->map1.w},     {eh, w.gy_m, eh, nullptr, 0, gw->map1.b},
      {3 * Hd, w.ggi, 3 * Hd, nullptr, 0, gw->b_ih}, {3 * Hd, w.ggh, 3 * Hd, nullptr, 0, gw->b_hh},
  };
  return op_colsum_multi(M, cj, 6, s);
}

// vector observations, encoder stand-in backward: W2 / b2 grads from gL = dL/d pre[N-1], dL/d pre[0] = (gL W2)
// SiLU'(pre[0]), W1 / b1 grads
static int wm_vec_encoder_bwd(const WmCtx& x, const float* gL) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_world_model* gw = x.gw;
  const int M = D.M, F = D.F, Dv = D.Dv;
  DR_TRY(nn_product(M, F, F, gL, x.wm->conv[1].w, w.gp[0], s));
  DR_TRY(mul_dsilu((long long)M * F, w.gp[0], w.pre[0], s));
  GemmArgs p[2];
  p[0] = bwd_w(F, F, M, gL, F, w.a[0], F, gw->conv[1].w);
  p[1] = bwd_w(F, Dv, M, w.gp[0], F, w.x0, Dv, gw->conv[0].w);
  splitk_all(p, 2, w.sk, w.sk_n);
  DR_TRY(tn_launch(p, 2, w.tn, w.tn_bytes, s, D.terms));
  ColsumJob cj[2] = {{F, gL, F, nullptr, 0, gw->conv[1].b}, {F, w.gp[0], F, nullptr, 0, gw->conv[0].b}};
  return op_colsum_multi(M, cj, 2, s);
}

// ---- backward through the encoder convolutions (all M frames) ----
static int wm_bwd_encoder(const WmCtx& x) {
  const WmDims& D = x.D; const WmWs& w = x.w; hipStream_t s = x.s;
  const dr_world_model* gw = x.gw;
  const int M = D.M, eh = D.eh, F = D.F, IH = D.IH, IW = D.IW, N = D.N;
  float* gL = w.gp[N - 1];  // dL/d pre[N-1], NHWC (w0tp's rows are permuted to NHWC)
  GemmArgs g = bwd_nt(M, F, eh, w.gpre_m, eh, w.w0tp, gL, F, 0);
  if (M >= 1024) {
    DR_TRY(op_nt_repack_split3(F, eh, w.w0tp, eh, w.pl_w0tp, s));
    wplanes(g, w.pl_w0tp);
  }
  DR_TRY(run(G_NT, AM_PLAIN, g, s));
  DR_TRY(mul_dsilu((long long)M * F, gL, w.pre[N - 1], s));
  if (D.Dv) return wm_vec_encoder_bwd(x, gL);
  for (int k = N - 1; k >= 0; --k) {
    const int oh = IH >> (k + 1), ow = IW >> (k + 1);
    const int cin = enc_cin_st(D, k), cout = D.e[k + 1];
    const float* hi = k ? w.a[k - 1] : w.x0;  // conv k's input
    if (k == 0 && cin > D.e[0]) {
      // conv1: x0's pad channel holds 1, so the weight-gradient product's
      // pad column is the bias gradient -- the 0.5 GB gradient gp[0] is not
      // re-read by a channel-sum pass (op_conv_wgrad bias_out)
      DR_TRY(op_conv_wgrad(M, oh, ow, cout, cin, w.gp[0], cout, 0, hi, cin, gw->conv[0].w, D.e[0], 1.0f, 0, w.cws,
                           w.cws_n, s, gw->conv[0].b));
      continue;
    }
    DR_TRY(wgrad(M, oh, ow, cout, cin, w.gp[k], cout, hi, cin, gw->conv[k].w, D.e[k], w.cws, w.cws_n, s, D.terms));
    DR_TRY(op_chan_sum((long long)M * oh * ow, cout, w.gp[k], cout, gw->conv[k].b, 0, w.cws, w.cws_n, s));
    if (k > 0) {
      ConvTArgs a = {};
      a.n = M; a.cin = cout; a.h = oh; a.w = ow; a.cout = cin;
      a.in = w.gp[k]; a.wq = w.wqe[k]; a.out = w.gp[k - 1]; a.ldc = cin; a.pre = w.pre[k - 1];
      if (w.t3e[k]) DR_TRY(op_convT_split3(CT_EPI_DSILU, a, w.t3e[k], s, D.terms));
      else DR_TRY(op_convT_nhwc(CT_EPI_DSILU, a, s));
    }
  }
  return DR_OK;
}

static int wm_run(int phases, const dr_dims* d, const dr_world_model* wm, const dr_decoder* dec, int B, int T,
                  const dr_frames* src, const dr_wm_batch* bt, dr_noise noise, dr_wm_loss_cfg cfg, float* stats,
                  int rows_global, float* losses, int* skip, const dr_world_model* gw, const dr_decoder* gd,
                  float* hiddens_out, float* latents_out, float* post_logits_out, void* ws, size_t ws_bytes,
                  hipStream_t s) {
  DR_REQUIRE(d && wm && dec && src && bt && losses && gw && gd && stats && B > 0 && T >= 2, "null argument or T < 2");
  DR_REQUIRE(bt->actions && bt->rewards && bt->continues, "window actions / rewards / continues required");
  DR_TRY(dims_envelope("dr_wm_train", d, ENV_GRU | ENV_SAMPLER | ENV_ENCODER | ENV_DECODER));
  DR_REQUIRE(vae_depth_ok(d), "enc_depth must be 0, 4 or 5");
  DR_REQUIRE(d->obs_dim > 0 || (d->img_h % (1 << vae_depth(d)) == 0 && d->img_w % (1 << vae_depth(d)) == 0),
             "image size must be a multiple of 2^depth (16, or 32 for the 5-layer VAE)");
  DR_REQUIRE(d->enc_f1 % 8 == 0 && d->enc_f2 % 8 == 0 && d->dec_f1 % 8 == 0 && d->dec_f2 % 8 == 0,
             "encoder / decoder filter counts must be multiples of 8");
  DR_REQUIRE(d->cols <= 64, "latent classes must be <= 64");
  DR_REQUIRE(d->obs_dim == 0 || d->obs_dim % 4 == 0, "vector observations: obs_dim % 4 == 0 required");
  // the NT products that take the tile route stay f32 in both modes (on the
  // bf16 tile GEMM in bf16 mode they saved 0.1 ms but raised the posterior
  // flips 1.7e-4 -> 1.7e-3, r04p)
  GemmBf16Scope bf16_scope(false);
  WmCtx x;
  x.d = d; x.wm = wm; x.gw = gw; x.dec = dec; x.gd = gd;
  x.D = wm_dims(d, B, T);
  const WmDims& D = x.D;
  WmWs& w = x.w;
  Carve c(ws);
  wm_carve(c, d, D, w);
  WS_CHECK(c, ws_bytes);
  if (D.terms == 3) {  // the biases of the layers routed to the six-product kernels (forward and backward)
    for (int k = 0; k < D.N; ++k) {
      if (w.s3e[k]) DR_TRY(conv_bias_aligned(__func__, "conv", k, wm->conv[k].b));
      if (w.t3d[k]) DR_TRY(conv_bias_aligned(__func__, "convt", k, dec->convt[k].b));
    }
  }
  wm_heads(D, wm, gw, x.head);
  x.src = src; x.bt = bt; x.noise = noise; x.cfg = cfg; x.stats = stats;
  x.rows_global = rows_global > 0 ? rows_global : D.M1;
  x.losses = losses; x.skip = skip;
  x.hiddens_out = hiddens_out; x.latents_out = latents_out; x.post_logits_out = post_logits_out;
  x.s = s;
  x.hB = w.h_all + (long long)B * D.Hd; x.zB = w.z_all + (long long)B * D.L;
  x.gHB = w.gH + (long long)B * D.Hd; x.gZB = w.gZ + (long long)B * D.L;
  x.cin_t = D.cd; x.cout_t = D.cd + 1;
  x.post1 = w.plog + (long long)B * D.L;

  if (phases & DR_WM_PREP) DR_TRY(wm_prep(x));
  if (phases & DR_WM_FWD) {
    DR_TRY(wm_fwd_encoder(x));
    DR_TRY(wm_fwd_scan(x));
    DR_TRY(wm_fwd_heads(x));
    DR_TRY(wm_fwd_decoder(x));
    DR_TRY(wm_fwd_losses(x));
  }
  const bool bwd_heads = (phases & (DR_WM_BWD | DR_WM_BWD_HEADS)) != 0;
  const bool bwd_scan = (phases & (DR_WM_BWD | DR_WM_BWD_SCAN)) != 0;
  const bool bwd_enc = (phases & (DR_WM_BWD | DR_WM_BWD_ENC)) != 0;
  if (!(bwd_heads || bwd_scan || bwd_enc)) return DR_OK;
  if (bwd_heads) DR_TRY(wm_bwd_heads(x));
  if (bwd_scan) DR_TRY(wm_bwd_scan(x));
  if (bwd_enc) DR_TRY(wm_bwd_encoder(x));
  return DR_OK;
}

extern "C" int dr_wm_train_phase(const dr_dims* d, const dr_world_model* wm, const dr_decoder* dec, int B, int T,
                                 const dr_frames* src, const dr_wm_batch* bt, dr_noise noise, dr_wm_loss_cfg cfg,
                                 int phases, float* stats, int rows_global, float* losses, int* skip,
                                 const dr_world_model* gw, const dr_decoder* gd, float* hiddens_out,
                                 float* latents_out, float* post_logits_out, void* ws, size_t ws_bytes,
                                 hipStream_t s) {
  return wm_run(phases, d, wm, dec, B, T, src, bt, noise, cfg, stats, rows_global, losses, skip, gw, gd, hiddens_out,
                latents_out, post_logits_out, ws, ws_bytes, s);
}

extern "C" int dr_wm_train_grads(const dr_dims* d, const dr_world_model* wm, const dr_decoder* dec, int B, int T,
                                 const dr_frames* src, const dr_wm_batch* bt, dr_noise noise, dr_wm_loss_cfg cfg,
                                 float* losses, int* skip, const dr_world_model* gw, const dr_decoder* gd,
                                 float* hiddens_out, float* latents_out, float* post_logits_out, void* ws,
                                 size_t ws_bytes, hipStream_t s) {
  DR_REQUIRE(d && B > 0 && T >= 2, "null argument or T < 2");
  Carve c(ws);
  WmWs w;
  wm_carve(c, d, wm_dims(d, B, T), w);
  WS_CHECK(c, ws_bytes);
  return wm_run(DR_WM_PREP | DR_WM_FWD | DR_WM_BWD, d, wm, dec, B, T, src, bt, noise, cfg, w.stats, 0, losses, skip,
                gw, gd, hiddens_out, latents_out, post_logits_out, ws, ws_bytes, s);
}

// Per-window loss of the last DR_WM_FWD on this workspace (prioritised replay,
// DESIGN.md 5n): the terms of k_wm_stats restricted to window b, the KL without
// the free-bit clamp.  Reads obs_part, rew_row, cont_row, kl_grp and cont_tm;
// the backward stages write none of the five, so it may follow a whole step.
// One wave per window, lane t over the steps (row i = (t - 1) B + b).
__global__ __launch_bounds__(256) void k_wm_window_scores(int B, int T1, int R, int nparts,
                                                          const float* __restrict__ obs_part,
                                                          const float* __restrict__ rew_row,
                                                          const float* __restrict__ cont_row,
                                                          const float* __restrict__ kl_grp,
                                                          const float* __restrict__ cont_tm, dr_wm_loss_cfg cfg,
                                                          float* __restrict__ scores) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= B) return;
  float sp = 0.f, sm = 0.f, sk = 0.f;
  for (int t = lane; t < T1; t += 64) {
    const long long i = (long long)t * B + b;
    const float m = cont_tm[i];
    float o = 0.f;
    for (int j = 0; j < nparts; ++j) o += obs_part[i * nparts + j];
    float k = 0.f;
    for (int g = 0; g < R; ++g) k += kl_grp[i * R + g];
    sp += m * ((o - rew_row[i]) + cont_row[i]);
    sm += m;
    sk += m * k;
  }
  sp = wave_sum(sp);
  sm = wave_sum(sm);
  sk = wave_sum(sk);
  if (lane == 0) {
    const float pred = sp / (sm + 1e-5f);
    const float kl = sk / (float)T1;
    scores[b] = cfg.beta_pred * pred + (cfg.beta_dyn + cfg.beta_rep) * kl;
  }
}

static int wm_window_scores(int B, int T1, int R, int nparts, const float* obs_part, const float* rew_row,
                            const float* cont_row, const float* kl_grp, const float* cont_tm, dr_wm_loss_cfg cfg,
                            float* scores, hipStream_t s) {
  hipLaunchKernelGGL(k_wm_window_scores, dim3(blocks(B, 4)), dim3(256), 0, s, B, T1, R, nparts, obs_part, rew_row,
                     cont_row, kl_grp, cont_tm, cfg, scores);
  return dr_check_launch("wm_window_scores");
}

extern "C" int dr_wm_window_scores(const dr_dims* d, int B, int T, dr_wm_loss_cfg cfg, void* ws, size_t ws_bytes,
                                   float* scores_out, hipStream_t s) {
  DR_REQUIRE(d && ws && scores_out && B > 0 && T >= 2, "null argument or T < 2");
  const WmDims D = wm_dims(d, B, T);
  Carve c(ws);
  WmWs w;
  wm_carve(c, d, D, w);
  WS_CHECK(c, ws_bytes);
  return wm_window_scores(B, T - 1, d->rows, D.Dv ? 1 : op_convT_mse_parts(D.IH / 2, D.IW / 2), w.obs_part, w.rew_row,
                          w.cont_row, w.kl_grp, w.cont_tm, cfg, scores_out, s);
}

// ===========================================================================
// a20  Decoder.forward (VariationalAutoEncoder.py:139-161), inference
// ===========================================================================
struct DecWs {
  float *u1, *u2, *q[DR_MAX_DEPTH], *w3p, *b3p, *wq[DR_MAX_DEPTH];
};
static void dec_carve(Carve& c, const dr_dims* d, int M, DecWs& w) {
  memset(&w, 0, sizeof(w));
  const WmDims D = wm_dims(d, 1, 2);
  const int N = D.N;
  w.u1 = c.f((long long)M * D.dh);
  w.u2 = c.f((long long)M * D.Fd);
  if (D.Dv) {
    w.q[0] = c.f((long long)M * D.Fd);
  } else {
    for (int k = 0; k + 1 < N; ++k) w.q[k] = c.f((long long)M * D.pix[N - k - 1] * D.cd[k + 1]);
  }
  w.w3p = c.f((long long)D.Fd * D.dh);
  w.b3p = c.f(D.Fd);
  for (int k = 0; k < N; ++k) w.wq[k] = c.f((long long)16 * D.cd[k] * D.cd[k + 1]);
}

extern "C" size_t dr_decoder_workspace_bytes(const dr_dims* d, int M) {
  if (!d || M <= 0) return 0;
  Carve c(nullptr);
  DecWs w;
  dec_carve(c, d, M, w);
  return c.off;
}

extern "C" int dr_decoder_fwd(const dr_dims* d, const dr_decoder* dec, int M, const float* h, long long ldh,
                              const float* z, long long ldz, float* mu, void* ws, size_t ws_bytes, hipStream_t s) {
  DR_REQUIRE(d && dec && h && z && mu && M > 0, "null argument or empty batch");
  DR_REQUIRE(vae_depth_ok(d), "enc_depth must be 0, 4 or 5");
  DR_REQUIRE(d->obs_dim > 0 || (d->img_h % (1 << vae_depth(d)) == 0 && d->img_w % (1 << vae_depth(d)) == 0),
             "image size must be a multiple of 2^depth (16, or 32 for the 5-layer VAE)");
  DR_TRY(dims_envelope(__func__, d, ENV_DECODER));
  DR_REQUIRE(d->dec_f1 % 8 == 0 && d->dec_f2 % 8 == 0, "decoder filter counts must be multiples of 8");
  Carve c(ws);
  DecWs w;
  dec_carve(c, d, M, w);
  WS_CHECK(c, ws_bytes);
  const WmDims D = wm_dims(d, 1, 2);
  const int* cin_t = D.cd;
  const int* cout_t = D.cd + 1;
  const int Hd = D.Hd, L = D.L, N = D.N;
  if (D.Dv) {  // vector observations: upscaler, then the image_builder MLP stand-in -> mu [M][D]
    DR_TRY(run(G_NT, AM_PLAIN, lin2(M, D.dh, h, ldh, Hd, z, ldz, L, dec->up0.w, dec->up0.b, w.u1, D.dh), s));
    GemmArgs g = lin_ln(M, D.Fd, D.dh, w.u1, D.dh, dec->up1, dec->up3.w, dec->up3.b, w.u2, D.Fd);
    g.act = 1;
    DR_TRY(run(G_NT, AM_LNSILU, g, s));
    GemmArgs g1 = lin(M, D.Fd, D.Fd, w.u2, D.Fd, dec->convt[0].w, D.Fd, dec->convt[0].b, w.q[0], D.Fd);
    g1.act = 1;
    DR_TRY(run(G_NT, AM_PLAIN, g1, s));
    return run(G_NT, AM_PLAIN, lin(M, D.Dv, D.Fd, w.q[0], D.Fd, dec->convt[1].w, D.Fd, dec->convt[1].b, mu, D.Dv), s);
  }
  DR_TRY(perm_rows(D.C0, D.Pf, D.dh, dec->up3.w, w.w3p, 1, s));
  DR_TRY(perm_rows(D.C0, D.Pf, 1, dec->up3.b, w.b3p, 1, s));
  for (int k = 0; k + 1 < N; ++k) DR_TRY(op_convT_repack(cin_t[k], cout_t[k], dec->convt[k].w, w.wq[k], s));
  DR_TRY(op_convT_out3_repack(cin_t[N - 1], dec->convt[N - 1].w, w.wq[N - 1], s));
  // upscaler: cat(h, flatten z) -> Linear -> LN -> SiLU -> Linear (rows permuted to NHWC); its SiLU runs in convT1's loader
  DR_TRY(run(G_NT, AM_PLAIN, lin2(M, D.dh, h, ldh, Hd, z, ldz, L, dec->up0.w, dec->up0.b, w.u1, D.dh), s));
  {
    GemmArgs g = lin_ln(M, D.Fd, D.dh, w.u1, D.dh, dec->up1, w.w3p, w.b3p, w.u2, D.Fd);
    g.act = 1;  // upscaler.4 SiLU
    DR_TRY(run(G_NT, AM_LNSILU, g, s));
  }
  for (int k = 0; k < N; ++k) {
    ConvTArgs a = dec_convt_args(D, M, k, w.wq[k], dec->convt[k].b);
    a.in = k ? w.q[k - 1] : w.u2;
    if (k < N - 1) {
      a.out = w.q[k]; a.silu_out = 1; a.ldc = cout_t[k];
      DR_TRY(op_convT_nhwc(CT_EPI_BIAS, a, s));
    } else {
      a.out = mu; a.ldc = 3;
      DR_TRY(op_convT_out3(a, s));
    }
  }
  return DR_OK;
}

// ===========================================================================
// Test hook of the loss stage and of the reverse scan's row kernels
// (tests/test_gpu_wm_loss.py): run exactly one of them on caller-made
// operands, through the launcher the step itself uses (above; ops.h for the
// row kernels of ops.hip).  Not in the public header.
//
// v: ints, num: doubles, ptrs: device pointers; per op (tests/wm_loss_ref.py
// mirrors the op codes):
//   WL_GATHER          v B T A act_sb act_st rc_sb rc_st; ptrs actions rewards continues act_tm rew_tm cont_tm
//   WL_PREP            k_wm_masksum then k_wm_coef.  v M1 set_stats0; num beta_pred stats0 (written over stats[0]
//                      between the two when set_stats0: the all-reduced mask sum of a data-parallel caller);
//                      ptrs cont_tm stats scal coef_row coef_obs
//   WL_KL_FWD          v M1 R C; ptrs prior post kl_grp
//   WL_HEADS           v M1 nb; ptrs rlog clog rew_tm cont_tm buckets coef_row rew_row cont_row g_rew g_cont
//   WL_STATS           v M1 R nparts; ptrs obs_part rew_row cont_row kl_grp cont_tm stats
//   WL_FINAL           v rows; num beta_pred beta_dyn beta_rep; ptrs stats scal losses skip (skip may be NULL)
//   WL_KL_BWD          v M1 R C; ptrs prior post cont_tm scal g_prior g_post
//   WL_STE_BWD_ADD     v M R C ldg lds lde ldl; ptrs gz soft extra gl (extra may be NULL)
//   WL_VEC_MSE         v M1 D; ptrs mu x coef g part
//   WL_WINDOW_SCORES   v B T1 R nparts; num beta_pred beta_dyn beta_rep; ptrs obs_part rew_row cont_row kl_grp
//                      cont_tm scores
//   WL_GRU_BWD         v B Hd ldg ldh ldo accumulate; ptrs g_hp h sr su sn sghn g_gi g_gh gh_out (h may be NULL)
//   WL_LN_SILU_BWD     v M K ldgx ldp ldgp; ptrs gx pre gamma beta g_pre gy xhat g_pre16 (gy and xhat both or
//                      neither; g_pre16 may be NULL)
//   WL_SOFTMAX_STE_BWD v M R C ldg lds; ptrs gz soft gl
//   WL_COLSUM_MULTI    v M njobs accumulate, then (N ldx ldy) per job; ptrs (X Y out) per job (Y may be NULL).
//                      accumulate (one job only): op_colsum, the one caller of colsum_slab that adds to `out`
// A size, stride or pointer combination that is refused returns DR_E_INVALID
// before anything is launched, dr_set_error's text in msg.
// ===========================================================================
enum {
  WL_GATHER, WL_PREP, WL_KL_FWD, WL_HEADS, WL_STATS, WL_FINAL, WL_KL_BWD, WL_STE_BWD_ADD, WL_VEC_MSE,
  WL_WINDOW_SCORES, WL_GRU_BWD, WL_LN_SILU_BWD, WL_SOFTMAX_STE_BWD, WL_COLSUM_MULTI, WL_COUNT
};

static int wm_loss_run(int op, const int* v, const double* num, void* const* ptrs, hipStream_t s) {
  DR_REQUIRE(v && ptrs, "null descriptor or pointer array");
  DR_REQUIRE(op >= 0 && op < WL_COUNT, "unknown op");
  auto F = [&](int i) { return (float*)ptrs[i]; };
  // every slot 0 .. n - 1 but those in the `optional` bit mask must be set
  auto given = [&](int n, unsigned optional) {
    for (int i = 0; i < n; ++i)
      if (!ptrs[i] && !(optional >> i & 1)) return false;
    return true;
  };
  const bool grouped = op == WL_KL_FWD || op == WL_KL_BWD || op == WL_STE_BWD_ADD || op == WL_SOFTMAX_STE_BWD;
  if (grouped) {
    DR_REQUIRE(v[0] >= 1 && v[1] >= 1, "rows and latent groups must be positive");
    DR_REQUIRE(v[2] >= 1 && v[2] <= 64, "latent classes must be in [1,64]");
  }
  const bool scalars = op == WL_PREP || op == WL_FINAL || op == WL_WINDOW_SCORES;
  DR_REQUIRE(!scalars || num, "this op reads its scalars from num");
  switch (op) {
    case WL_GATHER: {
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1 && v[2] >= 0, "B, T must be positive, A non-negative");
      DR_REQUIRE(given(6, 0), "null operand");
      dr_wm_batch bt = {};
      bt.actions = F(0); bt.act_sb = v[3]; bt.act_st = v[4];
      bt.rewards = F(1); bt.continues = F(2); bt.rc_sb = v[5]; bt.rc_st = v[6];
      return wm_gather(v[0], v[1], v[2], bt, F(3), F(4), F(5), s);
    }
    case WL_PREP: {
      DR_REQUIRE(v[0] >= 1, "M1 must be positive");
      DR_REQUIRE(given(5, 0), "null operand");
      DR_TRY(wm_masksum(v[0], F(0), F(1), s));
      if (v[1]) {
        const float f = (float)num[1];
        DR_TRY_HIP(hipMemsetD32Async((hipDeviceptr_t)F(1), __builtin_bit_cast(int, f), 1, s));
      }
      return wm_coef(v[0], F(0), (float)num[0], F(1), F(2), F(3), F(4), s);
    }
    case WL_KL_FWD:
      DR_REQUIRE(given(3, 0), "null operand");
      return wm_kl_fwd(v[0], v[1], v[2], F(0), F(1), F(2), s);
    case WL_HEADS:
      DR_REQUIRE(v[0] >= 1 && v[1] >= 2, "M1 must be positive, nb at least 2");
      DR_REQUIRE(given(10, 0), "null operand");
      return wm_heads_loss(v[0], v[1], F(0), F(1), F(2), F(3), F(4), F(5), F(6), F(7), F(8), F(9), s);
    case WL_STATS:
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1 && v[2] >= 1, "M1, R, nparts must be positive");
      DR_REQUIRE(given(6, 0), "null operand");
      return wm_stats(v[0], v[1], v[2], F(0), F(1), F(2), F(3), F(4), F(5), s);
    case WL_FINAL: {
      DR_REQUIRE(v[0] >= 1, "rows must be positive");
      DR_REQUIRE(given(4, 1u << 3), "null operand");
      const dr_wm_loss_cfg cfg = {(float)num[0], (float)num[1], (float)num[2]};
      return wm_final(F(0), v[0], cfg, F(1), F(2), (int*)ptrs[3], s);
    }
    case WL_KL_BWD:
      DR_REQUIRE(given(6, 0), "null operand");
      return wm_kl_bwd(v[0], v[1], v[2], F(0), F(1), F(2), F(3), F(4), F(5), s);
    case WL_STE_BWD_ADD: {
      const int L = v[1] * v[2];
      DR_REQUIRE(v[3] >= L && v[4] >= L && v[6] >= L && (!ptrs[2] || v[5] >= L), "row stride below R * C");
      DR_REQUIRE(given(4, 1u << 2), "null operand");
      return ste_bwd_add(v[0], v[1], v[2], F(0), v[3], F(1), v[4], F(2), v[5], F(3), v[6], s);
    }
    case WL_VEC_MSE:
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1, "M1, D must be positive");
      DR_REQUIRE(given(5, 0), "null operand");
      return vec_mse(v[0], v[1], F(0), F(1), F(2), F(3), F(4), s);
    case WL_WINDOW_SCORES: {
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1 && v[2] >= 1 && v[3] >= 1, "B, T - 1, R, nparts must be positive");
      DR_REQUIRE(given(6, 0), "null operand");
      const dr_wm_loss_cfg cfg = {(float)num[0], (float)num[1], (float)num[2]};
      return wm_window_scores(v[0], v[1], v[2], v[3], F(0), F(1), F(2), F(3), F(4), cfg, F(5), s);
    }
    case WL_GRU_BWD:
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1, "B, Hd must be positive");
      DR_REQUIRE(v[2] >= v[1] && v[4] >= v[1] && (!ptrs[1] || v[3] >= v[1]), "row stride below Hd");
      DR_REQUIRE(given(9, 1u << 1), "null operand");
      return op_gru_bwd(v[0], v[1], F(0), v[2], F(1), v[3], F(2), F(3), F(4), F(5), F(6), F(7), F(8), v[4], v[5], s);
    case WL_LN_SILU_BWD:
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1, "M, K must be positive");
      DR_REQUIRE(v[2] >= v[1] && v[3] >= v[1] && v[4] >= v[1], "row stride below K");
      DR_REQUIRE(given(8, 7u << 5), "null operand");
      DR_REQUIRE(!ptrs[5] == !ptrs[6], "gy and xhat are written together: both or neither");
      return op_ln_silu_bwd(v[0], v[1], F(0), v[2], F(1), v[3], F(2), F(3), F(4), v[4], F(5), F(6), s,
                            (unsigned short*)ptrs[7]);
    case WL_SOFTMAX_STE_BWD:
      DR_REQUIRE(v[3] >= v[1] * v[2] && v[4] >= v[1] * v[2], "row stride below R * C");
      DR_REQUIRE(given(3, 0), "null operand");
      return op_softmax_ste_bwd(v[0], v[1], v[2], F(0), v[3], F(1), v[4], F(2), s);
    case WL_COLSUM_MULTI: {
      const int M = v[0], n = v[1], acc = v[2];
      DR_REQUIRE(M >= 1 && n >= 1 && n <= DR_MAX_CSJOBS, "M must be positive, 1 to DR_MAX_CSJOBS jobs");
      DR_REQUIRE(!acc || n == 1, "accumulate: one job (op_colsum)");
      ColsumJob cj[DR_MAX_CSJOBS];
      for (int j = 0; j < n; ++j) {
        const int N = v[3 + 3 * j], ldx = v[4 + 3 * j], ldy = v[5 + 3 * j];
        const float *X = F(3 * j), *Y = F(3 * j + 1);
        float* out = F(3 * j + 2);
        DR_REQUIRE(N >= 1 && X && out, "a job needs N >= 1, X and out");
        DR_REQUIRE(ldx >= N && (!Y || ldy >= N), "row stride below N");
        cj[j] = {N, X, ldx, Y, ldy, out};
      }
      if (acc) return op_colsum(M, cj[0].N, cj[0].X, cj[0].ldx, cj[0].Y, cj[0].ldy, cj[0].out, 1, s);
      return op_colsum_multi(M, cj, n, s);
    }
  }
  return DR_OK;
}

extern "C" int dr_internal_wm_loss_run(int op, const int* v, const double* num, void* const* ptrs, void* stream,
                                       char* msg, int msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  const int rc = wm_loss_run(op, v, num, ptrs, (hipStream_t)stream);
  if (rc != DR_OK && msg && msg_cap > 0) snprintf(msg, msg_cap, "%s", dr_last_error());
  return rc;
}
