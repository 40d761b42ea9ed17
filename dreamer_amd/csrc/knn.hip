// Fused k-nearest-neighbour search and the particle-entropy reward built on it (APT, Liu & Abbeel 2021; config key
// explore = "entropy"; include/dreamer_hip.h).  The Mq x Nb distance matrix is never written: a
// workgroup owns 128 query rows and a contiguous range of 128-row bank tiles (grid.y splits the bank), accumulates
// x.y on the exact-f32 MFMA, forms the Gram distance in the tile epilogue and merges it into per-row k-best lists
// held in LDS.  A second kernel merges the splits' lists in a fixed order, recomputes the k chosen distances in the
// direct form and sorts them; a row kernel turns them into the entropy reward.  No atomics, no host synchronisation.
#include <algorithm>
#include <cstdio>
#include <type_traits>

#include "engine_util.h"

#define KN_BM 128        // query rows of a workgroup
#define KN_BN 128        // bank rows of a tile
// columns of a staged chunk BK and its LDS row pitch BK + 4 (4 * odd: the 16 rows x 4 k of an MFMA operand read hit 64
// banks): 32 / 36 where rows can be fetched as float4 (D and both strides multiples of 4, 16-byte aligned bases: a
// thread moves four float4 per operand and chunk, 128-byte row segments), else 16 / 20 with scalar fetches.  The two
// forms stage the same values and run the same chains: the same bits.
#define KN_STAGE (2 * KN_BM * 36)
#define KN_DP 65         // pitch of the 128 x 64 epilogue image
#define KN_LP 33         // pitch of a row's k-best list
#define KN_MAX_SPLIT 64  // bank splits (= lanes of the merging wave)
#define KN_ROWS 4        // rows (waves) per workgroup of the merge kernel

__device__ __forceinline__ bool kn_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }
// (d2, index) order; an empty slot (+inf, -1) counts as index INT_MAX
__device__ __forceinline__ bool kn_less(float da, int ia, float db, int ib) {
  return da < db || (da == db && (unsigned)ia < (unsigned)ib);
}

// ---------------------------------------------------------------------------
// Stage 1.  4 waves as 2 x 2, each a 64 x 64 block of the 128 x 128 tile (4 x 4 fragments of v_mfma_f32_16x16x4_f32,
// one accumulator per output element: the dot product of a pair is the k-ascending fmaf chain from 0 whatever the
// tile, the split, the batch or the fetch width).  Squared norms and finite flags of the tile's 128 + 128 rows come
// from the same staged chunks, one thread per row, as the same chain (fmaf(v, v, n), k ascending): bit-identical
// rows give |x|^2 = |y|^2 = x.y and a Gram distance of exactly 0.  Columns past D and rows past Mq / Nb are staged as 0.
// Epilogue, per half of the tile's columns: the two waves holding it write eligible distances (+inf otherwise) to an
// LDS image; thread r < 128 scans row r's 64 candidates in ascending bank index against the row's current k-th
// distance (held in a register) and inserts the few that beat it.  Candidates arrive in ascending index within a
// split, so a tie with a held entry loses and the list stays in (d2, index) order.
// ---------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_knn_tile(int D, int k, int Mq, const float* __restrict__ q, long long ldq,
                                                     const int* __restrict__ qg, int Nb,
                                                     const float* __restrict__ bank, long long ldb,
                                                     const int* __restrict__ bg, int tiles_per_split,
                                                     float* __restrict__ part_d2, int* __restrict__ part_idx) {
  constexpr int KN_BK = VEC ? 32 : 16, KN_LD = KN_BK + 4;
  __shared__ __attribute__((aligned(16))) float s_stage[KN_STAGE];  // chunk of A, chunk of B; epilogue image
  __shared__ float s_ld[KN_BM * KN_LP];
  __shared__ int s_li[KN_BM * KN_LP];
  __shared__ float s_na[KN_BM], s_nb[KN_BN];
  __shared__ int s_qg[KN_BM], s_bg[KN_BN];
  __shared__ unsigned char s_qok[KN_BM], s_bok[KN_BN];
  static_assert(KN_STAGE >= KN_BM * KN_DP && KN_STAGE >= 2 * KN_BM * KN_LD, "staging buffers and epilogue image");
  float* As = s_stage;
  float* Bs = s_stage + KN_BM * KN_LD;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int m0 = blockIdx.x * KN_BM;
  const int ntiles = (Nb + KN_BN - 1) / KN_BN;
  const int t_begin = blockIdx.y * tiles_per_split, t_end = min(ntiles, t_begin + tiles_per_split);
  const bool grouped = qg != nullptr && bg != nullptr;
  const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
  const int fr = lane & 15, fk = lane >> 4;

  if (tid < KN_BM) {
    for (int n = 0; n < k; ++n) {
      s_ld[tid * KN_LP + n] = INFINITY;
      s_li[tid * KN_LP + n] = -1;
    }
    s_qg[tid] = (grouped && m0 + tid < Mq) ? qg[m0 + tid] : 0;
  }
  float thr = INFINITY;  // thread r < 128: the k-th distance of row r's list

  constexpr int NL = VEC ? 4 : 8;  // fetches per operand, chunk and thread
  constexpr int LW = VEC ? 4 : 1, LC = KN_BK / LW, LR = 256 / LC;
  typedef typename std::conditional<VEC, float4, float>::type fetch_t;
  fetch_t ra[NL], rb[NL];
  const int lk = (tid % LC) * LW, lr = tid / LC;

  for (int tile = t_begin; tile < t_end; ++tile) {
    const int n0 = tile * KN_BN;
    auto load_chunk = [&](int k0) {
      const int kk = k0 + lk;
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int r = lr + LR * i, m = m0 + r, n = n0 + r;
        ra[i] = (m < Mq && kk < D) ? *reinterpret_cast<const fetch_t*>(q + (long long)m * ldq + kk) : fetch_t{};
        rb[i] = (n < Nb && kk < D) ? *reinterpret_cast<const fetch_t*>(bank + (long long)n * ldb + kk) : fetch_t{};
      }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float nrm = 0.f;  // this thread's row: A row tid (tid < 128) or B row tid - 128
    float chk = 0.f;  // fmaf(v, 0, chk): 0 while every value is finite, NaN after a NaN / Inf

    load_chunk(0);
    for (int k0 = 0; k0 < D; k0 += KN_BK) {
      __syncthreads();  // the previous chunk's reads (or the previous tile's scan) are done
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        *reinterpret_cast<fetch_t*>(As + (lr + LR * i) * KN_LD + lk) = ra[i];
        *reinterpret_cast<fetch_t*>(Bs + (lr + LR * i) * KN_LD + lk) = rb[i];
      }
      __syncthreads();
      if (k0 + KN_BK < D) load_chunk(k0 + KN_BK);
      {
        const float4* row = reinterpret_cast<const float4*>(s_stage + tid * KN_LD);  // A rows then B rows
#pragma unroll
        for (int c = 0; c < KN_BK / 4; ++c) {
          const float4 v = row[c];
          nrm = __builtin_fmaf(v.x, v.x, nrm);
          nrm = __builtin_fmaf(v.y, v.y, nrm);
          nrm = __builtin_fmaf(v.z, v.z, nrm);
          nrm = __builtin_fmaf(v.w, v.w, nrm);
          chk = __builtin_fmaf(v.x, 0.f, chk);
          chk = __builtin_fmaf(v.y, 0.f, chk);
          chk = __builtin_fmaf(v.z, 0.f, chk);
          chk = __builtin_fmaf(v.w, 0.f, chk);
        }
      }
#pragma unroll
      for (int kk = 0; kk < KN_BK; kk += 4) {
        float a[4], b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = As[(wm0 + i * 16 + fr) * KN_LD + kk + fk];
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = Bs[(wn0 + j * 16 + fr) * KN_LD + kk + fk];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
    }
    const bool ok = chk == 0.f;
    if (tid < KN_BM) {
      s_na[tid] = nrm;
      s_qok[tid] = ok && m0 + tid < Mq;
    } else {
      const int r = tid - KN_BM;
      s_nb[r] = nrm;
      s_bok[r] = ok && n0 + r < Nb;
      s_bg[r] = (grouped && n0 + r < Nb) ? bg[n0 + r] : 0;
    }
    __syncthreads();  // norms visible; the last chunk's operand reads are done, the staging buffers are free

    float* img = s_stage;
    for (int half = 0; half < 2; ++half) {
      if ((wave & 1) == half) {
        // lane holds D[row = 4 (lane >> 4) + r][col = lane & 15] of each fragment
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ml = wm0 + i * 16 + fk * 4 + r;
            const float na = s_na[ml];
            const bool qok = s_qok[ml];
            const int gq = s_qg[ml];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int nl = wn0 + j * 16 + fr;
              const float xy = acc[i][j][r];
              float d = (na + s_nb[nl]) - 2.f * xy;
              d = d < 0.f ? 0.f : d;
              const bool el = qok && s_bok[nl] && !(grouped && s_bg[nl] == gq);
              img[ml * KN_DP + (nl - wn0)] = el ? d : INFINITY;
            }
          }
      }
      __syncthreads();
      if (tid < KN_BM) {
        const float* cand = img + tid * KN_DP;
        float* ld = s_ld + tid * KN_LP;
        int* li = s_li + tid * KN_LP;
        for (int c8 = 0; c8 < 64; c8 += 8) {
          float v[8];  // (eight LDS reads in flight, then the compares)
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = cand[c8 + u];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const float d = v[u];
            if (d < thr) {  // false for +inf and NaN
              int p = k - 1;
              while (p > 0 && ld[p - 1] > d) {
                ld[p] = ld[p - 1];
                li[p] = li[p - 1];
                --p;
              }
              ld[p] = d;
              li[p] = n0 + half * 64 + c8 + u;
              thr = ld[k - 1];
            }
          }
        }
      }
      __syncthreads();
    }
  }
  if (tid < KN_BM && m0 + tid < Mq) {
    const long long at = ((long long)blockIdx.y * Mq + (m0 + tid)) * k;
    for (int n = 0; n < k; ++n) {
      part_d2[at + n] = s_ld[tid * KN_LP + n];
      part_idx[at + n] = s_li[tid * KN_LP + n];
    }
  }
}

// ---------------------------------------------------------------------------
// Stage 2.  One wave per query row.  (a) the S splits' lists, each in (d2, index) order, are merged k times: lane s
// holds split s's head, the smallest head by (d2, index) is taken (a fixed butterfly, no ties between distinct
// indices), its lane advances.  (b) each chosen pair's distance is recomputed as sum (x - y)^2: columns lane-strided
// in ascending order per lane, then wave_sum's fixed tree.  (c) lane n ranks its entry among the chosen by
// (recomputed d2, index) and writes it at its rank; the slots past the eligible count hold +inf / -1.  A query row
// with a NaN / Inf value writes NaN / -1.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64 * KN_ROWS) void k_knn_merge(int D, int k, int Mq, const float* __restrict__ q,
                                                            long long ldq, const float* __restrict__ bank,
                                                            long long ldb, int S, const float* __restrict__ part_d2,
                                                            const int* __restrict__ part_idx,
                                                            float* __restrict__ d2_out, int* __restrict__ idx_out) {
  const int row = blockIdx.x * KN_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= Mq) return;
  const float* x = q + (long long)row * ldq;
  bool fin = true;
  for (int j = lane; j < D; j += 64) fin = fin && kn_finite(x[j]);
  const bool qok = __ballot(!fin) == 0ull;
  float* dout = d2_out + (long long)row * k;
  int* iout = idx_out + (long long)row * k;
  if (!qok) {
    if (lane < k) {
      dout[lane] = __int_as_float(0x7FC00000);
      iout[lane] = -1;
    }
    return;
  }
  // (a)
  const long long base = ((long long)lane * Mq + row) * k;
  int head = 0, my_idx = -1;
  for (int n = 0; n < k; ++n) {
    float hd = INFINITY;
    int hi = -1;
    if (lane < S && head < k) {
      hd = part_d2[base + head];
      hi = part_idx[base + head];
    }
    float bd = hd;
    int bi = hi;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float od = __shfl_xor(bd, off, 64);
      const int oi = __shfl_xor(bi, off, 64);
      if (kn_less(od, oi, bd, bi)) {
        bd = od;
        bi = oi;
      }
    }
    if (bi >= 0 && hi == bi) ++head;  // a bank row lives in one split
    if (lane == n) my_idx = bi;
  }
  // (b)
  float my_d = INFINITY;
  for (int n = 0; n < k; ++n) {
    const int j = __shfl(my_idx, n, 64);
    if (j < 0) break;  // wave-uniform; the chosen come first
    const float* y = bank + (long long)j * ldb;
    float acc = 0.f;
    for (int c = lane; c < D; c += 64) {
      const float df = x[c] - y[c];
      acc += df * df;
    }
    acc = wave_sum(acc);
    if (lane == n) my_d = acc;
  }
  // (c)
  int rank = 0;
  for (int n = 0; n < k; ++n) {
    const float od = __shfl(my_d, n, 64);
    const int oi = __shfl(my_idx, n, 64);
    if (oi >= 0 && kn_less(od, oi, my_d, my_idx)) ++rank;
  }
  if (lane < k) {
    if (my_idx >= 0) {
      dout[rank] = my_d;
      iout[rank] = my_idx;
    } else {
      dout[lane] = INFINITY;
      iout[lane] = -1;
    }
  }
}

// ---------------------------------------------------------------------------
// Entropy row kernel: one thread per row.  k_m = filled slots, d = (sum_n sqrt(d2[n])) / k_m in slot order,
// e = log1pf(d); k_m = 0: e = 0, or NaN for a non-finite query row (its slots hold NaN).  The reward rewrite is
// k_disag_var's (disag.hip).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_knn_entropy(int k, int M, const float* __restrict__ d2,
                                                     const int* __restrict__ idx, float* ent_out, float* rew,
                                                     int rew_T, int rew_skip, long long rew_sb, long long rew_st,
                                                     float w_ext, float w_int) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  const float* dr = d2 + (long long)row * k;
  const int* ir = idx + (long long)row * k;
  float sum = 0.f;
  int km = 0;
  for (int n = 0; n < k; ++n)
    if (ir[n] >= 0) {
      sum += sqrtf(dr[n]);
      ++km;
    }
  float e;
  if (km > 0) e = log1pf(sum / (float)km);
  else e = (dr[0] != dr[0]) ? dr[0] : 0.f;
  if (ent_out) ent_out[row] = e;
  if (!rew) return;
  long long at;
  if (rew_T > 0) {
    const int b = row / rew_T, t = row % rew_T;
    if (t < rew_skip) return;
    at = b * rew_sb + (long long)(t - rew_skip) * rew_st;
  } else {
    at = row * rew_st;
  }
  const float a = w_ext * rew[at], c = w_int * e;
  rew[at] = a + c;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// bank splits: enough workgroups for two per CU of a 256-CU device, at most one split per bank tile.  A function of
// (Mq, Nb) alone; the result does not depend on it (a pair's distance is the same in every split).
static int knn_plan_split(int Mq, int Nb) {
  const int tm = dr_cdiv(Mq, KN_BM), tn = dr_cdiv(Nb, KN_BN);
  return std::max(1, std::min(std::min(tn, KN_MAX_SPLIT), dr_cdiv(512, tm)));
}

struct KnnWs {
  float *part_d2, *d2;
  int *part_idx, *idx;
};
static void knn_carve(Carve& c, int Mq, int k, int S, KnnWs& w) {
  const long long n = (long long)Mq * k;
  w.part_d2 = c.f(n * S);
  w.part_idx = c.i(n * S);
  w.d2 = c.f(n);  // the final lists where the caller asks for none (dr_state_entropy_fwd)
  w.idx = c.i(n);
}

static int knn_check(const char* fn, int D, int k, int Mq, const float* q, long long ldq, int Nb, const float* bank,
                     long long ldb, const void* ws) {
  if (k < 1 || k > DR_KNN_MAX_K) {
    dr_set_error("%s: k = %d is outside 1 .. %d", fn, k, DR_KNN_MAX_K);
    return DR_E_INVALID;
  }
  if (D < 1 || Mq < 1 || Nb < 1) {
    dr_set_error("%s: needs positive D, Mq, Nb", fn);
    return DR_E_INVALID;
  }
  if (!q || !bank || !ws || ldq < D || ldb < D) {
    dr_set_error("%s: null queries, bank or workspace, or a row stride below D", fn);
    return DR_E_INVALID;
  }
  return DR_OK;
}

// split = 0: the planner's
static int knn_run(int D, int k, int Mq, const float* q, long long ldq, const int* qg, int Nb, const float* bank,
                   long long ldb, const int* bg, float* d2_out, int* idx_out, int split, const KnnWs& w,
                   hipStream_t s) {
  const int tn = dr_cdiv(Nb, KN_BN);
  const int S = split > 0 ? split : knn_plan_split(Mq, Nb);
  const int per = dr_cdiv(tn, S);  // trailing splits may be empty: their lists stay +inf / -1
  const bool vec = D % 4 == 0 && ldq % 4 == 0 && ldb % 4 == 0 && (((uintptr_t)q | (uintptr_t)bank) & 15) == 0;
  const dim3 grid(dr_cdiv(Mq, KN_BM), S);
  if (vec)
    hipLaunchKernelGGL(k_knn_tile<true>, grid, dim3(256), 0, s, D, k, Mq, q, ldq, qg, Nb, bank, ldb, bg, per,
                       w.part_d2, w.part_idx);
  else
    hipLaunchKernelGGL(k_knn_tile<false>, grid, dim3(256), 0, s, D, k, Mq, q, ldq, qg, Nb, bank, ldb, bg, per,
                       w.part_d2, w.part_idx);
  DR_TRY(dr_check_launch("knn_tile"));
  hipLaunchKernelGGL(k_knn_merge, dim3(dr_cdiv(Mq, KN_ROWS)), dim3(64 * KN_ROWS), 0, s, D, k, Mq, q, ldq, bank, ldb, S,
                     w.part_d2, w.part_idx, d2_out ? d2_out : w.d2, idx_out ? idx_out : w.idx);
  return dr_check_launch("knn_merge");
}
static int knn_entropy(int k, int M, const float* d2, const int* idx, float* ent_out, float* rew, int rew_T,
                       int rew_skip, long long rew_sb, long long rew_st, float w_ext, float w_int, hipStream_t s) {
  hipLaunchKernelGGL(k_knn_entropy, dim3(dr_cdiv(M, 256)), dim3(256), 0, s, k, M, d2, idx, ent_out, rew, rew_T,
                     rew_skip, rew_sb, rew_st, w_ext, w_int);
  return dr_check_launch("knn_entropy");
}

extern "C" size_t dr_knn_workspace_bytes(int Mq, int Nb, int D, int k) {
  if (k < 1 || k > DR_KNN_MAX_K || D < 1 || Mq < 1 || Nb < 1) return 0;
  Carve c(nullptr);
  KnnWs w;
  knn_carve(c, Mq, k, knn_plan_split(Mq, Nb), w);
  return c.off;
}

extern "C" int dr_knn(int D, int k, int Mq, const float* q, long long ldq, const int* qg, int Nb, const float* bank,
                      long long ldb, const int* bg, float* d2_out, int* idx_out, void* ws, size_t ws_bytes,
                      hipStream_t stream) {
  DR_TRY(knn_check(__func__, D, k, Mq, q, ldq, Nb, bank, ldb, ws));
  DR_REQUIRE(d2_out && idx_out, "null output");
  Carve c(ws);
  KnnWs w;
  knn_carve(c, Mq, k, knn_plan_split(Mq, Nb), w);
  WS_CHECK(c, ws_bytes);
  return knn_run(D, k, Mq, q, ldq, qg, Nb, bank, ldb, bg, d2_out, idx_out, 0, w, stream);
}

extern "C" int dr_state_entropy_fwd(int D, int k, int Mq, const float* q, long long ldq, const int* qg, int Nb,
                                    const float* bank, long long ldb, const int* bg, float* d2_out, int* idx_out,
                                    float* ent_out, float* rew, int rew_T, int rew_skip, long long rew_sb,
                                    long long rew_st, float w_ext, float w_int, void* ws, size_t ws_bytes,
                                    hipStream_t stream) {
  DR_TRY(knn_check(__func__, D, k, Mq, q, ldq, Nb, bank, ldb, ws));
  DR_REQUIRE(d2_out || idx_out || ent_out || rew, "no output asked for");
  DR_REQUIRE(!rew || (rew_T >= 0 && rew_skip >= 0 && (rew_T == 0 || rew_skip < rew_T)), "bad reward row mapping");
  Carve c(ws);
  KnnWs w;
  knn_carve(c, Mq, k, knn_plan_split(Mq, Nb), w);
  WS_CHECK(c, ws_bytes);
  DR_TRY(knn_run(D, k, Mq, q, ldq, qg, Nb, bank, ldb, bg, d2_out, idx_out, 0, w, stream));
  if (!ent_out && !rew) return DR_OK;
  return knn_entropy(k, Mq, d2_out ? d2_out : w.d2, idx_out ? idx_out : w.idx, ent_out, rew, rew_T, rew_skip, rew_sb,
                     rew_st, w_ext, w_int, stream);
}

// ---------------------------------------------------------------------------
// Test hook (tests/test_gpu_knn.py).  Not in the public header.
//   knn  v D k Mq Nb ldq ldb split(0: planned); num ws_bytes            ptrs q qg bank bg d2 idx ws
//   ent  v k M rew_T rew_skip rew_sb rew_st;    num w_ext w_int         ptrs d2 idx ent rew          (ent or rew optional)
//   plan v Mq Nb                                                         returns the planned split count in *(int*)ptrs[0] (host)
// ---------------------------------------------------------------------------
enum { KN_OP_KNN, KN_OP_ENT, KN_OP_PLAN, KN_OP_COUNT };
static int knn_hook(int op, const int* v, const double* num, void* const* ptrs, hipStream_t s) {
  DR_REQUIRE(v && ptrs, "null descriptor or pointer array");
  DR_REQUIRE(op >= 0 && op < KN_OP_COUNT, "unknown op");
  if (op == KN_OP_PLAN) {
    DR_REQUIRE(v[0] >= 1 && v[1] >= 1 && ptrs[0], "needs positive Mq, Nb and an output");
    *(int*)ptrs[0] = knn_plan_split(v[0], v[1]);
    return DR_OK;
  }
  if (op == KN_OP_ENT) {
    const int k = v[0], M = v[1];
    DR_REQUIRE(k >= 1 && k <= DR_KNN_MAX_K && M >= 1, "needs 1 <= k <= 32 and positive M");
    DR_REQUIRE(ptrs[0] && ptrs[1] && (ptrs[2] || ptrs[3]), "null operand");
    DR_REQUIRE(!ptrs[3] || (num && v[2] >= 0 && v[3] >= 0 && (v[2] == 0 || v[3] < v[2])), "bad reward row mapping");
    return knn_entropy(k, M, (const float*)ptrs[0], (const int*)ptrs[1], (float*)ptrs[2], (float*)ptrs[3], v[2], v[3],
                       v[4], v[5], num ? (float)num[0] : 0.f, num ? (float)num[1] : 0.f, s);
  }
  const int D = v[0], k = v[1], Mq = v[2], Nb = v[3], split = v[6];
  DR_TRY(knn_check(__func__, D, k, Mq, (const float*)ptrs[0], v[4], Nb, (const float*)ptrs[2], v[5], ptrs[6]));
  DR_REQUIRE(ptrs[4] && ptrs[5] && num, "null output or workspace size");
  DR_REQUIRE(split >= 0 && split <= KN_MAX_SPLIT, "split outside 0 .. 64");
  Carve c(ptrs[6]);
  KnnWs w;
  knn_carve(c, Mq, k, split > 0 ? split : knn_plan_split(Mq, Nb), w);
  WS_CHECK(c, (size_t)num[0]);
  return knn_run(D, k, Mq, (const float*)ptrs[0], v[4], (const int*)ptrs[1], Nb, (const float*)ptrs[2], v[5],
                 (const int*)ptrs[3], (float*)ptrs[4], (int*)ptrs[5], split, w, s);
}

extern "C" int dr_internal_knn_run(int op, const int* v, const double* num, void* const* ptrs, void* stream, char* msg,
                                   int msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  const int rc = knn_hook(op, v, num, ptrs, (hipStream_t)stream);
  if (rc != DR_OK && msg && msg_cap > 0) snprintf(msg, msg_cap, "%s", dr_last_error());
  return rc;
}
