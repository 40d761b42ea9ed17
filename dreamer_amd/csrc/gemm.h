// Generic fused f32 GEMM on the exact-f32 MFMA (v_mfma_f32_16x16x4_f32).
//   Y[m][n] (+)= act( alpha * sum_k opA(m,k) * opB(k,n) + bias[n] + addend[m][n] )
// A operand: row-major [M][K] ("MK", optional 2nd K-segment, optional
// LayerNorm+SiLU applied on load, or conv im2col) or [K][M] ("KM").
// B operand: [N][K] ("NK": Y = A W^T, forward Linear) or [K][N] ("KN":
// Y = A W, backward input-grad / weight-grad), optional 2nd segment.
#pragma once
#include "common.h"

enum { AM_PLAIN = 0, AM_LNSILU = 1, AM_CONV = 2, AM_CONV_SRC = 3, AM_LNBWD = 4, AM_STEBWD = 5 };
// AM_STEBWD (NT skinny only): A = d/d(logits) of the straight-through
// categorical sample (DynamicsPredictors.py:31-40) given dL/dz = A-argument
// rows and the unimixed softmax `pre` rows: per group of C classes,
// a = s * (0.99 g - sum_group(0.99 g * s))  (ops.hip k_softmax_ste_bwd).
// AM_LNBWD (NT skinny only): A = d/d(pre) of SiLU(LayerNorm(pre)) given the
// upstream gradient gx = A-argument rows; the LN input `pre` and gamma/beta
// (ln_g/ln_b) come from the fields below.  a_out receives g_pre, sv_gy /
// sv_xh the SiLU-input gradient and x_hat (for the LayerNorm parameter grads).

// Fused GRU backward (SequenceModel.py:19-24 -> torch gru_cell) on the FINAL
// value of an accumulated hidden-state gradient g = dL/dh' (the last GEMM that
// adds into it, engine.hip's BPTT): for output (m, j < Hd) the epilogue writes
// gi[m][{r,u,n}] / gh[m][{r,u,n}] and adds dL/dh through h' = (h - n) u + n to
// ho[m][j] -- ops.hip k_gru_bwd's arithmetic, one launch fewer per BPTT step.
struct GruBwdEpi {
  const float* h; long long ldh;        // h (NULL = zeros)
  const float *r, *u, *n, *ghn;          // forward saves [M][Hd]
  float *gi, *gh;                        // [M][3 Hd]
  float* ho; long long ldo;              // dL/dh (+=)
  int Hd, pad_;
  unsigned short *gi16, *gh16;           // optional bf16 (RNE) copies of gi / gh (bf16 mode's GemmArgs.A16)
};

struct alignas(16) GemmArgs {
  int M, N, K;
  // A
  const float* A; long long lda;
  const float* A2; long long lda2; int ksplitA;  // MK: k >= ksplitA reads A2[m][k-ksplitA]
  const float* ln_g; const float* ln_b;          // AM_LNSILU (LN width == K)
  float* a_out; long long ld_aout;               // optional copy of the transformed A (n-tile 0 writes)
  const float* pre; long long ld_pre;            // AM_LNBWD: LayerNorm input rows
  float* splitk_ws; long long splitk_floats;     // optional scratch for split-K partials (tile GEMM)
  float* sv_gy; float* sv_xh; long long ld_sv;   // AM_LNBWD: optional saves (n-tile 0 writes)
  // conv im2col (k4 s2 p1), A = NCHW activations [frame][cin][ih][iw]
  int cin, ih, iw, oh, ow;
  dr_frames src;                                 // AM_CONV_SRC: frames, f = t*nb + b
  int nb;
  // B
  const float* W; long long ldb;
  const float* W2; long long ldb2; int ksplitB; int nsplitB;  // KN: k>=ksplitB | n>=nsplitB -> W2
  // epilogue
  const float* bias; const float* addend; long long ld_add;
  float* Y; long long ldy;
  float* Y2; long long ldy2; int nsplitY;        // n >= nsplitY -> Y2[m][n-nsplitY]
  int accumulate, act, out_conv;                 // act 1 = SiLU, 2 = sigmoid; out_conv: Y NCHW [frame][N][oh*ow]
  float alpha;
  // fused epilogues of the skinny kernel (epi != EPI_NONE; Y may be NULL)
  int epi;
  dr_noise noise; int step;
  // EPI_SAMPLE: rows of R groups x C classes -> straight-through one-hot
  int R, C; float unimix;
  float* z_out; long long ldz; int* idx_out; float* soft_out; long long ld_soft;
  float* zval_out;  // optional compact [M][R] straight-through value at idx
  // EPI_ACTOR: columns [mu (A) | log_sig (A)] -> clamp, softplus, tanh(mu + eps*sigma)
  int na, det;
  float* act_out; long long ld_act; float* mu_out; long long ld_mu; float* sig_out; long long ld_sig;
  float* eps_save; float* ls_save; long long ld_ls;
  // bf16 perf mode (dr_dims.precision): NT products that take the tile route
  // run on v_mfma_f32_16x16x32_bf16 with operands rounded to bf16 as they are
  // staged (f32 accumulation, f32 in / out); set by the engine per call
  int bf16;
  GruBwdEpi gb;  // gb.Hd > 0: fused GRU backward on the stored values (see GruBwdEpi)
  // NT B operand also given as bf16 planes [K/32][3][wsplit_np][32] (conv.h
  // op_nt_repack_split3 of W): per-step chain products then run on the bf16
  // MFMA -- f32-accurate 3-term split (fp32 mode) or plane 0 alone (bf16 mode)
  const unsigned short* wsplit; int wsplit_np, pad2_;
  // bf16 mode: A also given rounded to bf16 (RNE, row stride lda) by its
  // producer -- k_gemm_wks3<1> then loads 8 bf16 per lane instead of 8 f32 and
  // skips the rounding (bitwise the same products)
  const unsigned short* A16;
};

enum { EPI_NONE = 0, EPI_SAMPLE = 1, EPI_ACTOR = 2 };

enum GemmLayout { G_NT = 0, G_NN = 1, G_TN = 2 };

GemmArgs gemm_args();  // zero-initialised with neutral defaults
// While alive, gemm_args() returns bf16 = on (the engine's bf16 perf mode
// around the imagination-epoch entry points); restores the previous value.
struct GemmBf16Scope {
  explicit GemmBf16Scope(bool on);
  ~GemmBf16Scope();
  int prev;
};
// Launch up to 4 problems sharing layout/A-mode in one dispatch.
int gemm_launch(GemmLayout lay, int amode, const GemmArgs* probs, int count, hipStream_t s);

// The route of a batch, decided on the host before anything is launched (gemm_launch: validate, plan, run the steps)
enum GemmFamily {     // kernel<template selector from GemmStep>
  GF_LEGACY = 0,      // k_gemm<bm, bn, amode, a_km, b_kn>
  GF_SKINNY,          // k_gemm_skinny<bm, bn, amode, b_kn, vec, epi>
  GF_TILE,            // k_gemm_tile<bm, bn, kc, a_km, b_kn, vec, nw>
  GF_TILE_B16,        // k_gemm_tile_b16<bm, bn, nw>
  GF_WK,              // k_gemm_wk<bm, bn, nw, 2, 1>
  GF_WKS3,            // k_gemm_wks3<bf16 ? 1 : 3 planes, 1, nw, bm / 16, a16>
  GF_LN_SAMPLE,       // k_ln_gemm_sample<kc> (kc = 16-k chunks)
  GF_S3_TALL,         // conv_split.hip's split3 tall GEMM, one problem
  GF_LN_ROWS,         // k_ln_silu_rows<kc> pre-pass of one problem (kc = float4 per lane)
  GF_SPLITK_FINISH    // k_splitk_finish over the preceding tile step's partials
};
struct GemmStep {     // all int: dr_internal_gemm_plan copies it out as it is
  int family, bm, bn, kc, nw, amode, a_km, b_kn, vec, epi, bf16, a16;
  int mask;           // problems of the batch it covers (bit i), passed in batch order
  int gx, gy, gz, block, lds;  // grid, block, dynamic LDS bytes
  int splits, npack, no_ws;    // no_ws: the problems' split-K scratch withheld from the kernel
};
struct GemmPlan {
  int rc; char err[192];  // DR_OK, or the error gemm_launch reports with `err`
  int ln_pre, nsteps; // ln_pre: GF_LN_ROWS steps first; every later step reads their a_out as A (AM_PLAIN)
  GemmStep step[10];  // <= 4 LN pre-passes, 4 tall split3, 1 batch, 1 split-K finish
};
// Pure host code: no HIP call, no pointer dereferenced (alignment and null tests only).
GemmPlan gemm_plan(GemmLayout lay, int amode, const GemmArgs* probs, int count);
// Runs a plan of these problems (gemm_launch = gemm_plan + gemm_run; a caller that asks the plan first runs that one).
int gemm_run(const GemmPlan& pl, const GemmArgs* probs, int count, hipStream_t s);
// Rows of the skinny tile (16 or 64) the plan of one AM_LNBWD / AM_STEBWD problem, all its fields set, runs it on;
// 0 where the planner rejects the fused prologue.
int gemm_bwd_fusable(const GemmPlan& pl);

// The tail of the reference's 3-layer heads (Linear, LN, SiLU, Linear, LN,
// SiLU, Linear -- DynamicsPredictors.py:15-23, Agent.py:180-190) from the
// first Linear's output X on, in ONE launch:
//   y1 = SiLU(LN1(X)); h2 = y1 W3^T + b3; y2 = SiLU(LN4(h2)); out = y2 W6^T + b6
// followed by `e`'s epilogue (plain / activation store to e.Y, or EPI_SAMPLE,
// or EPI_ACTOR).  A workgroup owns 16 rows x 128 output columns and computes
// y1, h2, y2 for its rows itself (the two small layers are recomputed by
// each column block instead of a grid-wide seam).  K1, K2 <= 256.
struct alignas(16) Mlp2Args {
  int M, K1, K2, pad_;
  const float* X; long long ldx;     // [M][K1] first Linear's output (pre-LN1)
  const float* ln1_g; const float* ln1_b;
  const float* W3; const float* b3;  // [K2][K1]
  const float* ln4_g; const float* ln4_b;
  float* a1_out; long long ld_a1;    // optional y1 (column block 0 writes)
  float* pre2; long long ld_pre2;    // optional h2
  float* a2_out; long long ld_a2;    // optional y2
  GemmArgs e;                        // last Linear: e.N, e.W [N][K2] (e.ldb), e.bias, epilogue
};
bool mlp2_ok(const Mlp2Args& a);  // the shapes and alignments mlp2_launch takes
bool mlp2_widths_ok(int K1, int K2);  // its rule for the two hidden widths alone (host only)

// The same tail for 1 to DR_HT_HEADS heads over the same rows in ONE launch (k_heads_tail): a workgroup computes
// all e.N <= DR_HT_NMAX output columns of its 32 rows, so the middle layer runs once; k_mlp2_tail's arithmetic
// per row and per output element.  e.Y (optional with buckets): the last Linear's output through e.act;
// buckets / val: symexp(sum(softmax(out) * buckets)) per row (k_bucket_value's arithmetic) from the tile, no
// logits round trip.  Both stores take the row map m = b rm_h1 + t -> b (rm_h1 - rm_k0) + t - rm_k0 for
// t >= rm_k0, rows with t < rm_k0 are not stored (rm_h1 = 0: row m).  a1_out / pre2 / a2_out as Mlp2Args.
#define DR_HT_HEADS 4
#define DR_HT_NMAX 256
struct alignas(16) HeadTail {
  Mlp2Args a;            // a.e.epi == EPI_NONE
  const float* buckets;  // [e.N] or NULL
  float* val;            // with buckets
  int rm_h1, rm_k0;
  int chain1;            // 1: one MFMA accumulator chain per tile, k ascending (k_gemm_tile's sums); 0: k_mlp2_tail's four
  int pad_;
};
bool heads_tail_ok(const HeadTail& h);
int heads_tail_launch(const HeadTail* heads, int count, hipStream_t s);
int mlp2_launch(const Mlp2Args* probs, int count, hipStream_t s);
