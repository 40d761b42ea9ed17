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
//
// Episode-aware replay (replay_episodes = "respect") adds the
// span pass at the end of the file: span[i] = how many slots from i on belong
// to one stream, a reverse segmented scan over the ring in the same chunks.
// With a span array the weight of slot i is masked by span[i] >= S instead of
// rp_valid; without one (the entry points of 5n) nothing here changes.
#include "common.h"

#define RP_THREADS 256
#define RP_CHUNK 1024  // slots per chunk: 256 lanes x one float4

static inline int rp_chunks(long long cap) { return (int)((cap + RP_CHUNK - 1) / RP_CHUNK); }

// what a kernel needs to weigh a slot
struct RpRing {
  long long cap, size, next_idx, S;
  const float* priority;  // NULL (only with span): every valid start weighs 1
  double p_floor;
  const int* span;  // NULL: rp_valid; else slot i is a valid start iff span[i] >= S
};

// valid start (Buffer.py:33-48 with the straddle made exact)
__device__ __forceinline__ bool rp_valid(const RpRing& r, long long i) {
  if (i < 0 || i >= r.size - r.S + 1) return false;
  return !(r.size == r.cap && i < r.next_idx && r.next_idx < i + r.S);
}
// w_i: the stored priority (non-finite or <= 0: p_floor) of a valid start, else 0
__device__ __forceinline__ double rp_weight(const RpRing& r, long long i, float p, int span) {
  if (r.span ? (long long)span < r.S : !rp_valid(r, i)) return 0.0;
  if (!r.priority) return 1.0;
  const bool ok = (__float_as_uint(p) & 0x7f800000u) != 0x7f800000u && p > 0.0f;
  return ok ? (double)p : r.p_floor;
}
// the four weights of lane `tid` of chunk `c` (slots past cap weigh 0)
__device__ __forceinline__ void rp_load4(const RpRing& r, int c, int tid, long long& i0, double w[4]) {
  i0 = (long long)c * RP_CHUNK + 4 * tid;
  float p[4] = {0.f, 0.f, 0.f, 0.f};
  int sp[4] = {0, 0, 0, 0};
  if (i0 + 3 < r.cap) {
    if (r.priority) {
      const float4 v = *reinterpret_cast<const float4*>(r.priority + i0);
      p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    }
    if (r.span) {
      const int4 v = *reinterpret_cast<const int4*>(r.span + i0);
      sp[0] = v.x; sp[1] = v.y; sp[2] = v.z; sp[3] = v.w;
    }
  } else {
    for (int k = 0; k < 4; ++k)
      if (i0 + k < r.cap) {
        if (r.priority) p[k] = r.priority[i0 + k];
        if (r.span) sp[k] = r.span[i0 + k];
      }
  }
  for (int k = 0; k < 4; ++k) w[k] = i0 + k < r.cap ? rp_weight(r, i0 + k, p[k], sp[k]) : 0.0;
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

static int rp_check_ring(const char* fn, long long cap, long long size, long long next_idx, int S) {
  if (!(cap > 0 && size >= 0 && size <= cap && next_idx >= 0 && next_idx < cap && S >= 1)) {
    dr_set_error("%s: need cap > 0, 0 <= size <= cap, 0 <= next_idx < cap and S >= 1", fn);
    return DR_E_INVALID;
  }
  if (cap > (1LL << 30)) {
    dr_set_error("%s: cap over 2^30 slots", fn);
    return DR_E_UNSUPPORTED;
  }
  return DR_OK;
}

// span == NULL: the entry points of 5n (priority required).  With a span
// array the priority may be NULL.
static int rp_stage1(const char* fn, long long cap, long long size, long long next_idx, int S, const float* priority,
                     double p_floor, const int* span, bool masked, void* ws, size_t ws_bytes, hipStream_t s,
                     RpRing* out) {
  DR_TRY(rp_check_ring(fn, cap, size, next_idx, S));
  if (masked) {
    if (!span || !ws || ((uintptr_t)span & 15) || ((uintptr_t)priority & 15) || ((uintptr_t)ws & 7)) {
      dr_set_error("%s: span (16-byte aligned) and ws (8-byte aligned) are required; priority, if given, 16-byte aligned",
                   fn);
      return DR_E_INVALID;
    }
  } else if (!priority || !ws || ((uintptr_t)priority & 15) || ((uintptr_t)ws & 7)) {
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
  const RpRing r = {cap, size, next_idx, (long long)S, priority, p_floor, masked ? span : nullptr};
  hipLaunchKernelGGL(k_replay_chunk_sums, dim3(rp_chunks(cap)), dim3(RP_THREADS), 0, s, r, (double*)ws);
  *out = r;
  return dr_check_launch("replay_chunk_sums");
}

static int rp_sample(const char* fn, long long cap, long long size, long long next_idx, int S, int B,
                     const float* priority, double p_floor, const int* span, bool masked, const double* u,
                     const unsigned long long* rng, int stream_id, long long* starts_out, float* prob_out, void* ws,
                     size_t ws_bytes, hipStream_t s) {
  DR_REQUIRE(B >= 0 && starts_out, "need B >= 0 and starts_out");
  DR_REQUIRE(u || rng, "no uniforms (u or rng)");
  if (B == 0) return DR_OK;
  RpRing r;
  DR_TRY(rp_stage1(fn, cap, size, next_idx, S, priority, p_floor, span, masked, ws, ws_bytes, s, &r));
  const int n = rp_chunks(cap), per = (n + RP_THREADS - 1) / RP_THREADS;
  hipLaunchKernelGGL(k_replay_draw, dim3(B), dim3(RP_THREADS), 0, s, r, n, per, (const double*)ws, u, rng, stream_id,
                     starts_out, prob_out);
  return dr_check_launch("replay_draw");
}

static int rp_probabilities(const char* fn, long long cap, long long size, long long next_idx, int S,
                            const float* priority, double p_floor, const int* span, bool masked, float* prob_out,
                            void* ws, size_t ws_bytes, hipStream_t s) {
  DR_REQUIRE(prob_out, "prob_out is required");
  RpRing r;
  DR_TRY(rp_stage1(fn, cap, size, next_idx, S, priority, p_floor, span, masked, ws, ws_bytes, s, &r));
  const int n = rp_chunks(cap), per = (n + RP_THREADS - 1) / RP_THREADS;
  hipLaunchKernelGGL(k_replay_normalise, dim3(n), dim3(RP_THREADS), 0, s, r, n, per, (const double*)ws, prob_out);
  return dr_check_launch("replay_normalise");
}

extern "C" int dr_replay_sample(long long cap, long long size, long long next_idx, int S, int B,
                                const float* priority, double p_floor, const double* u,
                                const unsigned long long* rng, int stream_id, long long* starts_out, float* prob_out,
                                void* ws, size_t ws_bytes, hipStream_t s) {
  return rp_sample(__func__, cap, size, next_idx, S, B, priority, p_floor, nullptr, false, u, rng, stream_id,
                   starts_out, prob_out, ws, ws_bytes, s);
}

extern "C" int dr_replay_probabilities(long long cap, long long size, long long next_idx, int S,
                                       const float* priority, double p_floor, float* prob_out, void* ws,
                                       size_t ws_bytes, hipStream_t s) {
  return rp_probabilities(__func__, cap, size, next_idx, S, priority, p_floor, nullptr, false, prob_out, ws, ws_bytes,
                          s);
}

extern "C" int dr_replay_sample_spans(long long cap, long long size, long long next_idx, int S, int B,
                                      const float* priority, double p_floor, const int* span, const double* u,
                                      const unsigned long long* rng, int stream_id, long long* starts_out,
                                      float* prob_out, void* ws, size_t ws_bytes, hipStream_t s) {
  return rp_sample(__func__, cap, size, next_idx, S, B, priority, p_floor, span, true, u, rng, stream_id, starts_out,
                   prob_out, ws, ws_bytes, s);
}

extern "C" int dr_replay_probabilities_spans(long long cap, long long size, long long next_idx, int S,
                                             const float* priority, double p_floor, const int* span,
                                             float* prob_out, void* ws, size_t ws_bytes, hipStream_t s) {
  return rp_probabilities(__func__, cap, size, next_idx, S, priority, p_floor, span, true, prob_out, ws, ws_bytes, s);
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

// ---- episode-aware replay: the window spans ------------------
// span[i] = j* - i + 1 for i < size, j* the least stop >= i (the semantics are
// in include/dreamer_hip.h); 0 for i >= size.  A reverse segmented scan in the
// chunks of the sampler: stage 1 leaves each chunk's least stop, stage 2 takes
// the least stop behind its chunk from those and finishes inside the chunk by a
// suffix minimum over the lanes in LDS.  Everything is an integer minimum or an
// integer sum in a fixed order: the same inputs give the same bits.
#define RP_NO_STOP 0x7fffffff

struct RpStops {
  long long cap, size, newest;  // newest: the slot written last (-1: none)
  const float* continues;
  const unsigned char* first;  // NULL: all 0
};

// Bit k of the result: slot i0 + k (lane `tid` of chunk `c`) is a stop.  One
// float4 of continues and one 4-byte word of first flags per lane.  first[j + 1]
// ends slot j, so the lane's own four bytes end slots i0 - 1 .. i0 + 2; the
// byte that ends i0 + 3 is the next lane's first one (through sh_f), for the
// last lane the first byte of the next chunk.
__device__ __forceinline__ unsigned rp_stops4(const RpStops& r, int c, int tid, unsigned char* sh_f, long long& i0) {
  i0 = (long long)c * RP_CHUNK + 4 * tid;
  float ct[4] = {1.f, 1.f, 1.f, 1.f};
  unsigned fb = 0;  // first[i0 + k] in byte k
  if (i0 + 3 < r.cap) {
    const float4 v = *reinterpret_cast<const float4*>(r.continues + i0);
    ct[0] = v.x; ct[1] = v.y; ct[2] = v.z; ct[3] = v.w;
    if (r.first) fb = *reinterpret_cast<const unsigned*>(r.first + i0);
  } else {
    for (int k = 0; k < 4; ++k)
      if (i0 + k < r.cap) {
        ct[k] = r.continues[i0 + k];
        if (r.first) fb |= (unsigned)r.first[i0 + k] << (8 * k);
      }
  }
  sh_f[tid] = (fb & 0xffu) != 0;
  __syncthreads();
  bool next_first;
  if (tid + 1 < RP_THREADS) next_first = sh_f[tid + 1] != 0;
  else next_first = r.first && i0 + 4 < r.cap && r.first[i0 + 4] != 0;
  __syncthreads();
  unsigned m = 0;
  for (int k = 0; k < 4; ++k) {
    const long long j = i0 + k;
    if (j >= r.cap) break;
    const bool f = k < 3 ? ((fb >> (8 * (k + 1))) & 0xffu) != 0 : next_first;
    if (!(ct[k] >= 0.5f) || f || j == r.cap - 1 || j == r.newest) m |= 1u << k;  // (a NaN continue is a stop)
  }
  return m;
}

// stage 1: mins[c] = the least stop of chunk c (RP_NO_STOP: none)
__global__ __launch_bounds__(RP_THREADS) void k_replay_chunk_stops(RpStops r, int* __restrict__ mins) {
  __shared__ unsigned char sh_f[RP_THREADS];
  __shared__ int s_min;
  if (threadIdx.x == 0) s_min = RP_NO_STOP;
  long long i0;
  const unsigned m = rp_stops4(r, blockIdx.x, threadIdx.x, sh_f, i0);  // (its barriers also publish s_min)
  if (m) atomicMin(&s_min, (int)i0 + __ffs(m) - 1);
  __syncthreads();
  if (threadIdx.x == 0) mins[blockIdx.x] = s_min;
}

// stage 2: the spans of chunk c, and counts[c] = how many of them are >= S
__global__ __launch_bounds__(RP_THREADS) void k_replay_spans(RpStops r, int S, int nchunks,
                                                             const int* __restrict__ mins, int* __restrict__ span,
                                                             int* __restrict__ counts) {
  __shared__ unsigned char sh_f[RP_THREADS];
  __shared__ int sh[RP_THREADS];
  __shared__ int s_after;
  const int tid = threadIdx.x, c = blockIdx.x;
  if (tid == 0) s_after = RP_NO_STOP;
  long long i0;
  const unsigned m = rp_stops4(r, c, tid, sh_f, i0);  // (its barriers also publish s_after)
  // the least stop behind this chunk (the last slot of the ring is one, so only the last chunk has none)
  int after = RP_NO_STOP;
  for (int k = c + 1 + tid; k < nchunks; k += RP_THREADS) after = min(after, mins[k]);
  if (after != RP_NO_STOP) atomicMin(&s_after, after);
  // inclusive suffix minimum of the lanes' least stops
  sh[tid] = m ? (int)i0 + __ffs(m) - 1 : RP_NO_STOP;
  __syncthreads();
  for (int o = 1; o < RP_THREADS; o <<= 1) {
    const int a = tid + o < RP_THREADS ? sh[tid + o] : RP_NO_STOP;
    __syncthreads();
    sh[tid] = min(sh[tid], a);
    __syncthreads();
  }
  int nxt = min(tid + 1 < RP_THREADS ? sh[tid + 1] : RP_NO_STOP, s_after);  // the least stop behind the lane's slots
  __syncthreads();
  int out[4] = {0, 0, 0, 0}, cnt = 0;
  for (int k = 3; k >= 0; --k) {
    const long long j = i0 + k;
    if (j >= r.cap) continue;
    if ((m >> k) & 1u) nxt = (int)j;
    out[k] = j < r.size ? nxt - (int)j + 1 : 0;  // nxt >= j: slot cap - 1 is a stop
    cnt += out[k] >= S;
  }
  if (i0 + 3 < r.cap) {
    *reinterpret_cast<int4*>(span + i0) = make_int4(out[0], out[1], out[2], out[3]);
  } else {
    for (int k = 0; k < 4; ++k)
      if (i0 + k < r.cap) span[i0 + k] = out[k];
  }
  sh[tid] = cnt;
  __syncthreads();
  for (int o = RP_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  if (tid == 0) counts[c] = sh[0];
}

// stage 3 (one workgroup): n_valid = the sum of the chunks' counts
__global__ __launch_bounds__(RP_THREADS) void k_replay_span_count(int nchunks, const int* __restrict__ counts,
                                                                  long long* __restrict__ n_valid) {
  __shared__ long long sh[RP_THREADS];
  const int tid = threadIdx.x;
  long long s = 0;
  for (int k = tid; k < nchunks; k += RP_THREADS) s += counts[k];
  sh[tid] = s;
  __syncthreads();
  for (int o = RP_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  if (tid == 0) *n_valid = sh[0];
}

extern "C" size_t dr_replay_spans_workspace_bytes(long long cap) {
  if (cap <= 0) return 0;
  return ((size_t)rp_chunks(cap) * 2 * sizeof(int) + 7) & ~(size_t)7;  // the chunks' least stops, then their counts
}

extern "C" int dr_replay_spans(long long cap, long long size, long long next_idx, const float* continues,
                               const unsigned char* first, int S, int* span_out, long long* n_valid_out, void* ws,
                               size_t ws_bytes, hipStream_t s) {
  DR_TRY(rp_check_ring(__func__, cap, size, next_idx, S));
  if (!continues || !span_out || !ws || ((uintptr_t)continues & 15) || ((uintptr_t)span_out & 15) ||
      ((uintptr_t)first & 3) || ((uintptr_t)ws & 7) || ((uintptr_t)n_valid_out & 7)) {
    dr_set_error("%s: continues and span_out (16-byte aligned) and ws (8-byte aligned) are required; first, if given, "
                 "4-byte aligned", __func__);
    return DR_E_INVALID;
  }
  if (ws_bytes < dr_replay_spans_workspace_bytes(cap)) {
    dr_set_error("%s: workspace too small (%zu < %zu)", __func__, ws_bytes, dr_replay_spans_workspace_bytes(cap));
    return DR_E_WORKSPACE;
  }
  const long long newest = size == 0 ? -1 : size < cap ? size - 1 : (next_idx - 1 + cap) % cap;
  const RpStops r = {cap, size, newest, continues, first};
  const int n = rp_chunks(cap);
  int* mins = (int*)ws;
  int* counts = mins + n;
  hipLaunchKernelGGL(k_replay_chunk_stops, dim3(n), dim3(RP_THREADS), 0, s, r, mins);
  DR_TRY(dr_check_launch("replay_chunk_stops"));
  hipLaunchKernelGGL(k_replay_spans, dim3(n), dim3(RP_THREADS), 0, s, r, S, n, (const int*)mins, span_out, counts);
  DR_TRY(dr_check_launch("replay_spans"));
  if (!n_valid_out) return DR_OK;
  hipLaunchKernelGGL(k_replay_span_count, dim3(1), dim3(RP_THREADS), 0, s, n, (const int*)counts, n_valid_out);
  return dr_check_launch("replay_span_count");
}
