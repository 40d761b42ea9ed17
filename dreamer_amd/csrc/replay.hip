// Prioritised ("curious") replay: window sampling, per-slot probabilities and
// the priority update, all on the device (the semantics are in
// include/dreamer_hip.h).  One priority (f32) and one visit count (i32) per
// ring slot; slot i stands for the window that starts at i.
//
// Every sum is float64 in a fixed order, so the same inputs give the same
// bits: a chunk of RP_CHUNK slots is summed four slots per lane (one 16-byte
// load), then over the 256 lanes by a Hillis-Steele scan in LDS; the chunk
// sums are summed per lane over a contiguous run of chunks and scanned the
// same way.  No float atomics anywhere; the LDS integer min / max below pick
// an index, which does not depend on the order they arrive in.
#include "common.h"

#define RP_THREADS 256
#define RP_CHUNK 1024  // slots per chunk: 256 lanes x one float4

static inline int rp_chunks(long long cap) { return (int)((cap + RP_CHUNK - 1) / RP_CHUNK); }

// what a kernel needs to weigh a slot
struct RpRing {
  long long cap, size, next_idx, S;
  const float* priority;
  double p_floor;
};

// valid start (Buffer.py:33-48 with the straddle made exact)
__device__ __forceinline__ bool rp_valid(const RpRing& r, long long i) {
  if (i < 0 || i >= r.size - r.S + 1) return false;
  return !(r.size == r.cap && i < r.next_idx && r.next_idx < i + r.S);
}
// w_i: the stored priority (non-finite or <= 0: p_floor) of a valid start, else 0
__device__ __forceinline__ double rp_weight(const RpRing& r, long long i, float p) {
  if (!rp_valid(r, i)) return 0.0;
  const bool ok = (__float_as_uint(p) & 0x7f800000u) != 0x7f800000u && p > 0.0f;
  return ok ? (double)p : r.p_floor;
}
// the four weights of lane `tid` of chunk `c` (slots past cap weigh 0)
__device__ __forceinline__ void rp_load4(const RpRing& r, int c, int tid, long long& i0, double w[4]) {
  i0 = (long long)c * RP_CHUNK + 4 * tid;
  float p[4] = {0.f, 0.f, 0.f, 0.f};
  if (i0 + 3 < r.cap) {
    const float4 v = *reinterpret_cast<const float4*>(r.priority + i0);
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
  } else {
    for (int k = 0; k < 4; ++k)
      if (i0 + k < r.cap) p[k] = r.priority[i0 + k];
  }
  for (int k = 0; k < 4; ++k) w[k] = i0 + k < r.cap ? rp_weight(r, i0 + k, p[k]) : 0.0;
}

// inclusive scan of one double per lane over the 256 lanes (fixed order);
// returns the lane's inclusive value, *total the sum of all lanes
__device__ double rp_scan256(double v, double* sh, double* total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < RP_THREADS; o <<= 1) {
    const double a = tid >= o ? sh[tid - o] : 0.0;
    __syncthreads();
    if (tid >= o) sh[tid] += a;
    __syncthreads();
  }
  const double incl = sh[tid];
  *total = sh[RP_THREADS - 1];
  __syncthreads();
  return incl;
}

// stage 1: sums[c] = the weights of chunk c
__global__ __launch_bounds__(RP_THREADS) void k_replay_chunk_sums(RpRing r, double* __restrict__ sums) {
  __shared__ double sh[RP_THREADS];
  long long i0;
  double w[4];
  rp_load4(r, blockIdx.x, threadIdx.x, i0, w);
  double total;
  rp_scan256(((w[0] + w[1]) + w[2]) + w[3], sh, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// The running sum over the chunks, the same in the draws and in the
// normalising pass (so both see the same W): lane t owns chunks
// [t per, (t + 1) per).  Returns the lane's inclusive sum and its own run's
// sum (*seg); *W the total.
__device__ double rp_chunk_scan(const double* __restrict__ sums, int nchunks, int per, double* sh, double* seg,
                                double* W) {
  const int c0 = threadIdx.x * per;
  double s = 0.0;
  for (int k = 0; k < per; ++k)
    if (c0 + k < nchunks) s += sums[c0 + k];
  *seg = s;
  return rp_scan256(s, sh, W);
}

// 53-bit uniform in [0, 1) from two Philox words
__device__ __forceinline__ double rp_u53(uint32_t hi, uint32_t lo) {
  const unsigned long long m = ((unsigned long long)(hi >> 5) << 26) | (unsigned long long)(lo >> 6);
  return (double)m * (1.0 / 9007199254740992.0);
}

// stage 2: one workgroup per draw.  The start is the least slot i of positive
// weight whose running sum C_i exceeds u W; where rounding leaves none, the
// last slot of positive weight.  A slot of weight 0 is never returned.
__global__ __launch_bounds__(RP_THREADS) void k_replay_draw(RpRing r, int nchunks, int per,
                                                            const double* __restrict__ sums,
                                                            const double* __restrict__ u_in,
                                                            const unsigned long long* __restrict__ rng, int stream_id,
                                                            long long* __restrict__ starts_out,
                                                            float* __restrict__ prob_out) {
  __shared__ double sh[RP_THREADS];
  __shared__ double s_base, s_w;
  __shared__ int s_first, s_last;
  const int tid = threadIdx.x, b = blockIdx.x;
  if (tid == 0) {
    s_first = 0x7fffffff;
    s_last = -1;
  }
  // ---- chunk level ----
  const int c0 = tid * per;
  double seg, W;
  const double incl_t = rp_chunk_scan(sums, nchunks, per, sh, &seg, &W);  // (its barriers also publish s_first / s_last)
  double u;
  if (u_in) {
    u = u_in[b];
  } else {
    const dr_u4 x = dr_rand4(rng, (uint32_t)stream_id, (uint32_t)b, 0u);
    u = rp_u53(x.x, x.y);
  }
  const double target = u * W;
  {
    // the lane's exclusive base, to rounding: only chunks (and below, slots) of
    // positive weight are candidates, so an ulp here can move a draw that sits
    // on a boundary to its neighbour but never to an invalid slot
    double run = tid == 0 ? 0.0 : incl_t - seg;
    for (int k = 0; k < per; ++k) {
      const int c = c0 + k;
      if (c >= nchunks) break;
      const double sc = sums[c];
      run += sc;
      if (sc > 0.0) {
        atomicMax(&s_last, c);
        if (run > target) atomicMin(&s_first, c);
      }
    }
  }
  __syncthreads();
  const bool fell = s_first == 0x7fffffff;  // rounding left u W >= C_last
  const int chunk = fell ? s_last : s_first;
  if (chunk < 0) {  // no valid start: the host refuses this before any launch
    if (tid == 0) {
      starts_out[b] = 0;
      if (prob_out) prob_out[b] = 0.0f;
    }
    return;
  }
  if (chunk >= c0 && chunk < c0 + per) {  // the owner publishes the chunk's exclusive base
    double run = tid == 0 ? 0.0 : incl_t - seg;
    for (int c = c0; c < chunk; ++c) run += sums[c];
    s_base = run;
  }
  __syncthreads();
  const double rem = target - s_base;
  if (tid == 0) {  // every lane read s_first / s_last before the barrier above
    s_first = 0x7fffffff;
    s_last = -1;
  }
  // ---- slot level, inside the chunk ----
  long long i0;
  double w[4];
  rp_load4(r, chunk, tid, i0, w);
  const double s4 = ((w[0] + w[1]) + w[2]) + w[3];
  double ctot;
  const double incl4 = rp_scan256(s4, sh, &ctot);
  {
    double run = tid == 0 ? 0.0 : incl4 - s4;
    for (int k = 0; k < 4; ++k) {
      run += w[k];
      if (w[k] > 0.0) {
        atomicMax(&s_last, 4 * tid + k);
        if (!fell && run > rem) atomicMin(&s_first, 4 * tid + k);
      }
    }
  }
  __syncthreads();
  const int e = s_first == 0x7fffffff ? s_last : s_first;  // s_last >= 0: the chunk's sum is positive
  if (e >= 4 * tid && e < 4 * tid + 4) s_w = w[e - 4 * tid];
  __syncthreads();
  if (tid == 0) {
    starts_out[b] = (long long)chunk * RP_CHUNK + e;
    if (prob_out) prob_out[b] = (float)(s_w / W);
  }
}

// prob[i] = w_i / W for every slot (the same W as the draws)
__global__ __launch_bounds__(RP_THREADS) void k_replay_normalise(RpRing r, int nchunks, int per,
                                                                 const double* __restrict__ sums,
                                                                 float* __restrict__ prob) {
  __shared__ double sh[RP_THREADS];
  const int tid = threadIdx.x;
  double seg, W;
  rp_chunk_scan(sums, nchunks, per, sh, &seg, &W);
  long long i0;
  double w[4];
  rp_load4(r, blockIdx.x, tid, i0, w);
  for (int k = 0; k < 4; ++k)
    if (i0 + k < r.cap) prob[i0 + k] = W > 0.0 ? (float)(w[k] / W) : 0.0f;
}

extern "C" size_t dr_replay_sample_workspace_bytes(long long cap) {
  if (cap <= 0) return 0;
  return (size_t)rp_chunks(cap) * sizeof(double);
}

static int rp_stage1(const char* fn, long long cap, long long size, long long next_idx, int S, const float* priority,
                     double p_floor, void* ws, size_t ws_bytes, hipStream_t s, RpRing* out) {
  if (!(cap > 0 && size >= 0 && size <= cap && next_idx >= 0 && next_idx < cap && S >= 1)) {
    dr_set_error("%s: need cap > 0, 0 <= size <= cap, 0 <= next_idx < cap and S >= 1", fn);
    return DR_E_INVALID;
  }
  if (cap > (1LL << 30)) {
    dr_set_error("%s: cap over 2^30 slots", fn);
    return DR_E_UNSUPPORTED;
  }
  if (!priority || !ws || ((uintptr_t)priority & 15) || ((uintptr_t)ws & 7)) {
    dr_set_error("%s: priority (16-byte aligned) and ws (8-byte aligned) are required", fn);
    return DR_E_INVALID;
  }
  if (!(p_floor > 0.0)) {
    dr_set_error("%s: p_floor must be > 0", fn);
    return DR_E_INVALID;
  }
  if (ws_bytes < dr_replay_sample_workspace_bytes(cap)) {
    dr_set_error("%s: workspace too small (%zu < %zu)", fn, ws_bytes, dr_replay_sample_workspace_bytes(cap));
    return DR_E_WORKSPACE;
  }
  const RpRing r = {cap, size, next_idx, (long long)S, priority, p_floor};
  hipLaunchKernelGGL(k_replay_chunk_sums, dim3(rp_chunks(cap)), dim3(RP_THREADS), 0, s, r, (double*)ws);
  *out = r;
  return dr_check_launch("replay_chunk_sums");
}

extern "C" int dr_replay_sample(long long cap, long long size, long long next_idx, int S, int B,
                                const float* priority, double p_floor, const double* u,
                                const unsigned long long* rng, int stream_id, long long* starts_out, float* prob_out,
                                void* ws, size_t ws_bytes, hipStream_t s) {
  DR_REQUIRE(B >= 0 && starts_out, "need B >= 0 and starts_out");
  DR_REQUIRE(u || rng, "no uniforms (u or rng)");
  if (B == 0) return DR_OK;
  RpRing r;
  DR_TRY(rp_stage1(__func__, cap, size, next_idx, S, priority, p_floor, ws, ws_bytes, s, &r));
  const int n = rp_chunks(cap), per = (n + RP_THREADS - 1) / RP_THREADS;
  hipLaunchKernelGGL(k_replay_draw, dim3(B), dim3(RP_THREADS), 0, s, r, n, per, (const double*)ws, u, rng, stream_id,
                     starts_out, prob_out);
  return dr_check_launch("replay_draw");
}

extern "C" int dr_replay_probabilities(long long cap, long long size, long long next_idx, int S,
                                       const float* priority, double p_floor, float* prob_out, void* ws,
                                       size_t ws_bytes, hipStream_t s) {
  DR_REQUIRE(prob_out, "prob_out is required");
  RpRing r;
  DR_TRY(rp_stage1(__func__, cap, size, next_idx, S, priority, p_floor, ws, ws_bytes, s, &r));
  const int n = rp_chunks(cap), per = (n + RP_THREADS - 1) / RP_THREADS;
  hipLaunchKernelGGL(k_replay_normalise, dim3(n), dim3(RP_THREADS), 0, s, r, n, per, (const double*)ws, prob_out);
  return dr_check_launch("replay_normalise");
}

// Priority update.  One lane per row b; the batch's starts and scores pass
// through LDS in tiles of 256, and every lane scans all of them: the number of
// rows with its start, the largest |score| among them, whether one of them is
// non-finite, and whether a row before it holds the same start.  The first row
// of a start (the owner) alone writes the slot, so no two lanes write one
// address and nothing depends on the order of the rows: a count and a maximum
// do not.  The formula runs in float64 and is rounded once.
__global__ __launch_bounds__(RP_THREADS) void k_replay_priority_update(long long cap, int B,
                                                                       const long long* __restrict__ starts,
                                                                       const float* __restrict__ scores, double c,
                                                                       double beta, double alpha, double eps,
                                                                       float p_new, float* __restrict__ priority,
                                                                       int* __restrict__ visits) {
  __shared__ long long sh_s[RP_THREADS];
  __shared__ float sh_a[RP_THREADS];
  const int b = blockIdx.x * RP_THREADS + threadIdx.x;
  const long long mine = b < B ? starts[b] : -1;
  int count = 0;
  bool owner = true, bad = false;
  float mx = 0.0f;
  for (int t0 = 0; t0 < B; t0 += RP_THREADS) {
    const int j = t0 + threadIdx.x;
    sh_s[threadIdx.x] = j < B ? starts[j] : -1;
    sh_a[threadIdx.x] = j < B ? fabsf(scores[j]) : 0.0f;  // |NaN| = NaN, |inf| = inf
    __syncthreads();
    const int n = min(RP_THREADS, B - t0);
    for (int k = 0; k < n; ++k) {
      if (sh_s[k] != mine) continue;
      ++count;
      if (t0 + k < b) owner = false;
      const float a = sh_a[k];
      if ((__float_as_uint(a) & 0x7f800000u) == 0x7f800000u) bad = true;
      else mx = fmaxf(mx, a);
    }
    __syncthreads();
  }
  if (b >= B || !owner || mine < 0 || mine >= cap) return;
  const int v = visits[mine] + count;
  visits[mine] = v;
  priority[mine] = bad ? p_new : (float)(c * pow(beta, (double)v) + pow((double)mx + eps, alpha));
}

extern "C" int dr_replay_priority_update(long long cap, int B, const long long* starts, const float* scores, double c,
                                         double beta, double alpha, double eps, double p_new, float* priority,
                                         int* visits, hipStream_t s) {
  DR_REQUIRE(cap > 0 && B >= 0 && starts && scores && priority && visits, "null argument or empty ring");
  DR_REQUIRE(beta > 0.0 && beta <= 1.0 && alpha > 0.0 && eps > 0.0 && c >= 0.0 && p_new > 0.0,
             "need 0 < beta <= 1, alpha > 0, eps > 0, c >= 0 and p_new > 0");
  if (B == 0) return DR_OK;
  hipLaunchKernelGGL(k_replay_priority_update, dim3((B + RP_THREADS - 1) / RP_THREADS), dim3(RP_THREADS), 0, s, cap, B,
                     starts, scores, c, beta, alpha, eps, (float)p_new, priority, visits);
  return dr_check_launch("replay_priority_update");
}
