// Test hook of the recurrent step's and the actor head's row kernels (tests/test_gpu_step_ops.py): run one launcher
// of gru.h / ops.h on caller-made operands -- the launchers the engine itself calls, nothing copied or instantiated
// here.  Host code only.  Not in the public header.
#include <cstdio>

#include "gru.h"
#include "ops.h"

// op codes, mirrored by tests/step_ops_ref.py
enum {
  SO_GRU, SO_ONEHOT_INDEX, SO_ZGATHER_ADD, SO_GRU_FWD, SO_SAMPLE, SO_ACTOR_HEAD, SO_ACTOR_HEAD_BWD_X, SO_SIGMOID,
  SO_MEAN, SO_TRANSPOSE, SO_TRANSPOSE_MULTI, SO_COPY2D, SO_COPY2D_MULTI, SO_FILL, SO_VEC_GATHER, SO_COUNT
};

// v (ints), num (doubles) and ptrs (device pointers; an optional operand's slot may be NULL) per op:
//   gru               v B Hd R C A ldz lda ldh ldo gh_ready
//                     ptrs idx zval z a h wt b_ih w_hh b_hh hout hout16 sr su sn sghn gh_ws
//                     (optional: z -- needed only where idx marks a dense group --, h, hout16, the four saves
//                     together, gh_ws; a when A == 0)
//   onehot_index      v M R C ldz                         ptrs z idx zval
//   zgather_add       v M N R C ldz ldw ldb ldo           ptrs idx zval z wt base out          (optional: z)
//   gru_fwd           v B Hd ldh ldo                      ptrs gi gh h hout sr su sn sghn      (optional: h, the saves)
//   sample            v M R C ldl ldz lds step            ptrs logits q z idx soft             (optional: idx, soft)
//   actor_head        v M A ldm ldl lda ldmu lds step det ptrs mu_raw ls_raw eps a mu sigma eps_save
//                     (optional: the four outputs; eps when det)
//   actor_head_bwd_x  v M A N ldga ldgl lda ldl ldh ldx   ptrs g_a g_mu_l g_sig_l a ls_raw eps g_heads wt gx
//                     (optional: g_a, g_mu_l, g_sig_l; a and eps when g_a is NULL)
//   sigmoid           v M ldx ostride                     ptrs x out
//   mean              v n                                 ptrs x out
//   transpose         v rows cols                         ptrs in out
//   transpose_multi   v n then (rows cols ldo) per job    ptrs (in out) per job
//   copy2d            v dp sp width rows                  ptrs dst src
//   copy2d_multi      v n then (dp sp width rows) per job ptrs (dst src) per job
//   fill              v n; num value                      ptrs x
//   vec_gather        v n nb D ring_cap stride_b stride_t t0   ptrs ring starts obs X   (ring or obs)
// The noise is always explicit (dr_noise.q / .eps): the Philox paths have their own test.
static int step_run(int op, const int* v, const double* num, void* const* ptrs, hipStream_t s) {
  DR_REQUIRE(v && ptrs, "null descriptor");
  auto F = [&](int i) { return (float*)ptrs[i]; };
  auto given = [&](int n, unsigned optional) {
    for (int i = 0; i < n; ++i)
      if (!ptrs[i] && !((optional >> i) & 1u)) return false;
    return true;
  };
  switch (op) {
    case SO_GRU: {
      const int B = v[0], Hd = v[1], R = v[2], C = v[3], A = v[4];
      DR_REQUIRE(B >= 1 && Hd >= 1 && R >= 1 && C >= 1 && A >= 0, "B, Hd, R, C must be positive, A non-negative");
      DR_REQUIRE(v[5] >= R * C && v[6] >= A && (!ptrs[4] || v[7] >= Hd) && v[8] >= Hd, "row stride below the width");
      DR_REQUIRE(given(16, (1u << 2) | (A == 0 ? 1u << 3 : 0u) | (1u << 4) | (0x3Fu << 10)), "null operand");
      DR_REQUIRE(!ptrs[11] == !ptrs[12] && !ptrs[11] == !ptrs[13] && !ptrs[11] == !ptrs[14],
                 "the four saves are written together: all or none");
      GruArgs g = {};
      g.B = B; g.Hd = Hd; g.R = R; g.C = C; g.A = A;
      g.idx = (const int*)ptrs[0]; g.zval = F(1);
      g.z = F(2); g.ldz = v[5];
      g.a = F(3); g.lda = v[6];
      g.h = F(4); g.ldh = v[7];
      g.wt = F(5); g.b_ih = F(6); g.w_hh = F(7); g.b_hh = F(8);
      g.hout = F(9); g.hout16 = (unsigned short*)ptrs[10]; g.ldo = v[8];
      g.sr = F(11); g.su = F(12); g.sn = F(13); g.sghn = F(14);
      g.gh_ws = F(15); g.gh_ready = v[9];
      return op_gru_fused(g, s);
    }
    case SO_ONEHOT_INDEX:
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1, "M, R must be positive");
      DR_REQUIRE(v[3] >= v[1] * v[2], "row stride below R * C");
      DR_REQUIRE(given(3, 0), "null operand");
      return op_onehot_index(v[0], v[1], v[2], F(0), v[3], (int*)ptrs[1], F(2), s);
    case SO_ZGATHER_ADD:
      DR_REQUIRE(given(6, 1u << 2), "null operand");
      return op_zgather_add(v[0], v[1], v[2], v[3], (const int*)ptrs[0], F(1), F(2), v[4], F(3), v[5], F(4), v[6], F(5),
                            v[7], s);
    case SO_GRU_FWD:
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1, "B, Hd must be positive");
      DR_REQUIRE((!ptrs[2] || v[2] >= v[1]) && v[3] >= v[1], "row stride below Hd");
      DR_REQUIRE(given(8, (1u << 2) | (0xFu << 4)), "null operand");
      DR_REQUIRE(!ptrs[4] == !ptrs[5] && !ptrs[4] == !ptrs[6] && !ptrs[4] == !ptrs[7],
                 "the four saves are written together: all or none");
      return op_gru_fwd(v[0], v[1], F(0), F(1), F(2), v[2], F(3), v[3], F(4), F(5), F(6), F(7), s);
    case SO_SAMPLE: {
      DR_REQUIRE(v[0] >= 1 && v[1] >= 1, "M, R must be positive");
      DR_REQUIRE(v[6] >= 0, "step must be non-negative");
      DR_REQUIRE(v[2] < 1 || (v[3] >= v[1] * v[2] && v[4] >= v[1] * v[2] && (!ptrs[4] || v[5] >= v[1] * v[2])),
                 "row stride below R * C");
      DR_REQUIRE(v[2] < 1 || v[2] > 64 || given(5, 3u << 3), "null operand");
      dr_noise nz = {};
      nz.q = F(1);
      return op_sample(v[0], v[1], v[2], F(0), v[3], &nz, v[6], F(2), v[4], (int*)ptrs[3], F(4), v[5], s);
    }
    case SO_ACTOR_HEAD: {
      const int A = v[1], det = v[8];
      DR_REQUIRE(v[0] >= 1 && A >= 1, "M, A must be positive");
      DR_REQUIRE(v[7] >= 0, "step must be non-negative");
      DR_REQUIRE(v[2] >= A && v[3] >= A && (!ptrs[3] || v[4] >= A) && (!ptrs[4] || v[5] >= A) && (!ptrs[5] || v[6] >= A),
                 "row stride below A");
      DR_REQUIRE(given(7, (det ? 1u << 2 : 0u) | (0xFu << 3)), "null operand");
      dr_noise nz = {};
      nz.eps = F(2);
      return op_actor_head(v[0], A, F(0), v[2], F(1), v[3], &nz, v[7], det, F(3), v[4], F(4), v[5], F(5), v[6], F(6),
                           s);
    }
    case SO_ACTOR_HEAD_BWD_X: {
      const int A = v[1];
      DR_REQUIRE(v[0] >= 1, "M must be positive");
      if (A >= 1 && A <= 8 && v[2] >= 1) {
        DR_REQUIRE((!ptrs[0] || (v[3] >= A && v[5] >= A)) && ((!ptrs[1] && !ptrs[2]) || v[4] >= A) && v[6] >= A &&
                       v[7] >= 2 * A && v[8] >= v[2], "row stride below the width");
        DR_REQUIRE(given(9, 7u | (ptrs[0] ? 0u : (1u << 3) | (1u << 5))), "null operand");
      }
      return op_actor_head_bwd_x(v[0], A, v[2], F(0), v[3], F(1), F(2), v[4], F(3), v[5], F(4), v[6], F(5), F(6), v[7],
                                 F(7), F(8), v[8], s);
    }
    case SO_SIGMOID:
      DR_REQUIRE(v[0] >= 1, "M must be positive");
      DR_REQUIRE(given(2, 0), "null operand");
      return op_sigmoid(v[0], F(0), v[1], F(1), v[2], s);
    case SO_MEAN:
      DR_REQUIRE(v[0] <= 0 || given(2, 0), "null operand");
      return op_mean(v[0], F(0), F(1), s);
    case SO_TRANSPOSE:
      DR_REQUIRE(v[0] <= 0 || v[1] <= 0 || given(2, 0), "null operand");
      return op_transpose(v[0], v[1], F(0), F(1), s);
    case SO_TRANSPOSE_MULTI: {
      const int n = v[0];
      DR_REQUIRE(n >= 1 && n <= 16, "1 to 16 jobs can be described");
      TransposeJob tj[16];
      for (int j = 0; j < n; ++j) {
        DR_REQUIRE(n > DR_MAX_TJOBS || (ptrs[2 * j] && ptrs[2 * j + 1]), "null operand");
        tj[j] = {v[1 + 3 * j], v[2 + 3 * j], v[3 + 3 * j], F(2 * j), F(2 * j + 1)};
      }
      return op_transpose_multi(tj, n, s);
    }
    case SO_COPY2D:
      DR_REQUIRE(v[2] >= 1 && v[3] >= 1 && v[0] >= v[2] && v[1] >= v[2], "width, rows positive, pitches >= width");
      DR_REQUIRE(given(2, 0), "null operand");
      return op_copy2d(F(0), v[0], F(1), v[1], v[2], v[3], s);
    case SO_COPY2D_MULTI: {
      const int n = v[0];
      DR_REQUIRE(n >= 1 && n <= 8, "1 to 8 jobs can be described");
      Copy2dJob cj[8];
      for (int j = 0; j < n; ++j) {
        const int* d = v + 1 + 4 * j;
        DR_REQUIRE(d[0] >= d[2] && d[1] >= d[2], "pitch below width");
        DR_REQUIRE(n > DR_COPY_MAX || d[3] <= 0 || (ptrs[2 * j] && ptrs[2 * j + 1]), "null operand");
        cj[j] = {F(2 * j), d[0], F(2 * j + 1), d[1], d[2], d[3], 0, 0};
      }
      return op_copy2d_multi(cj, n, s);
    }
    case SO_FILL:
      DR_REQUIRE(num, "fill reads its value from num");
      DR_REQUIRE(v[0] >= 1, "n must be positive");
      DR_REQUIRE(given(1, 0), "null operand");
      return op_fill(v[0], F(0), (float)num[0], s);
    case SO_VEC_GATHER: {
      DR_REQUIRE(v[0] >= 1, "n must be positive");
      DR_REQUIRE(ptrs[3], "null operand");
      dr_frames src = {};
      src.ring = (const unsigned char*)ptrs[0];
      src.ring_cap = v[3];
      src.starts = (const long long*)ptrs[1];
      src.obs = F(2);
      src.stride_b = v[4]; src.stride_t = v[5];
      src.t0 = v[6];
      return op_vec_gather(v[0], v[1], v[2], &src, F(3), s);
    }
  }
  dr_set_error("dr_internal_step_run: unknown op %d", op);
  return DR_E_INVALID;
}

extern "C" int dr_internal_step_run(int op, const int* v, const double* num, void* const* ptrs, void* stream,
                                    char* msg, int msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  const int rc = step_run(op, v, num, ptrs, (hipStream_t)stream);
  if (rc != DR_OK && msg && msg_cap > 0) snprintf(msg, msg_cap, "%s", dr_last_error());
  return rc;
}
