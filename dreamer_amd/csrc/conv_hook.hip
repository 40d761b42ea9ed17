// Test hook of the convolution family (tests/test_gpu_conv_routes.py): run one op of conv.h on caller-made operands
// and say which kernel instantiation ran.  Not in the public header.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "conv.h"

thread_local const char* dr_conv_form_last = nullptr;

// formatted once per call site and instantiation and kept for the life of the process (DR_CONV_NOTE's static)
const char* dr_conv_form(const char* fmt, ...) {
  char buf[96];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return strdup(buf);
}

// descriptor ints (CV_*), doubles (CN_*) and pointer slots (CP_*), mirrored by tests/conv_ref.py
enum {
  CV_OP, CV_N, CV_CA, CV_CB, CV_H, CV_W, CV_EPI, CV_NCHW, CV_TERMS, CV_LDA, CV_LDB, CV_LDC, CV_TSTRIDE, CV_CBO,
  CV_SILU_IN, CV_SILU_OUT, CV_LO_SILU, CV_FLAGS, CV_ACC, CV_WS_FLOATS, CV_CIN_RAW, CV_COUNT
};
enum {
  COP_CONV, COP_CONV_S3, COP_CONVT, COP_CONVT_S3, COP_CONVT_OUT3, COP_WGRAD, COP_WGRAD_S3, COP_CHAN_SUM,
  COP_CHAN_SUM_FINAL
};
enum {
  CF_BIAS = 1, CF_PRE = 2, CF_CSUM = 4, CF_OUT2 = 8, CF_TARGET = 16, CF_COEF = 32, CF_PART = 64, CF_BPART = 128,
  CF_BIAS_OUT = 256, CF_NO_REPACK = 512, CF_WS = 1024
};
enum {
  CP_IN, CP_W, CP_WR, CP_BIAS, CP_OUT, CP_PRE, CP_CSUM, CP_OUT2, CP_TARGET, CP_COEF, CP_PART, CP_BPART, CP_WS, CP_HI,
  CP_BIAS_OUT, CP_COUNT
};
enum { CN_SCALE, CN_PAD, CN_COUNT };

// The ints: op kind; n; cin (conv, upsampling conv) / ca (weight gradient) / C (channel sums); cout / cb; h, w (the
// conv's input frame, the upsampling conv's and the weight gradient's low-resolution frame; channel sums: rows = n,
// partial rows nb = n); epi; out_nchw; terms; lda, ldb (weight gradient; channel sums: ldx = lda); ldc; tstride; cbo;
// silu_in, silu_out, lo_silu; flags (CF_*: which optional operands are given); accumulate; the floats behind the
// workspace pointer; the weight's own input channels where op_conv_repack_pad pads them (0: cin).
// num: scale (weight gradients), pad (unused by these ops: op_frames_nhwc4's pad channel is made by the caller).
// ptrs: CP_* device pointers; a slot whose flag is off is ignored.  ptrs == NULL: nothing is launched, *ws_need
// alone is reported.
//
// With ptrs: the weight in PyTorch layout (CP_W: Conv2d [cout][cin][4][4] for the convs, [cin][cout][4][4] for the
// upsampling convs -- a ConvTranspose2d weight, or a Conv2d weight read as its data gradient) is repacked into CP_WR
// as the op needs (op_conv_repack_pad / op_conv_repack_split3 / op_convT_repack / op_convT_repack_split3 /
// op_convT_out3_repack; CF_NO_REPACK skips it), then exactly one op runs.  Returns the op's code; on refusal the
// dr_set_error text is in msg.  form: the kernel that op launched last before its reduction / final pass (the
// weight gradients note their product kernel, the channel sums their partial-sum kernel), "" when none was.
extern "C" int dr_internal_conv_run(const int* v, const double* num, void* const* ptrs, void* stream,
                                    long long* ws_need, char* form, int form_cap, char* msg, int msg_cap) {
  hipStream_t s = (hipStream_t)stream;
  if (form && form_cap > 0) form[0] = 0;
  if (msg && msg_cap > 0) msg[0] = 0;
  if (!v) return DR_E_INVALID;
  const int op = v[CV_OP], n = v[CV_N], ca = v[CV_CA], cb = v[CV_CB], h = v[CV_H], w = v[CV_W], fl = v[CV_FLAGS];
  long long need = 0;
  if (op == COP_WGRAD) need = (long long)op_conv_wgrad_ws_floats(n, h, w, ca, cb);
  else if (op == COP_WGRAD_S3) need = (long long)op_wgrad_split3_ws_floats(n, h, w, ca, cb);
  else if (op == COP_CHAN_SUM) need = (long long)op_chan_sum_ws_floats(n, ca);
  if (ws_need) *ws_need = need;
  if (!ptrs) return DR_OK;
  auto P = [&](int slot, int flag) { return !flag || (fl & flag) ? (float*)ptrs[slot] : nullptr; };
  const float* in = P(CP_IN, 0);
  const float* wraw = P(CP_W, 0);
  float* wr = P(CP_WR, 0);
  float* out = P(CP_OUT, 0);
  const bool repack = !(fl & CF_NO_REPACK);
  const float scale = num ? (float)num[CN_SCALE] : 1.0f;
  const size_t ws_floats = (size_t)v[CV_WS_FLOATS];
  dr_conv_form_last = nullptr;
  int rc = DR_OK;
  ConvTArgs a = {};
  a.n = n; a.cin = ca; a.h = h; a.w = w; a.cout = cb;
  a.in = in; a.silu_in = v[CV_SILU_IN]; a.wq = wr; a.bias = P(CP_BIAS, CF_BIAS);
  a.out = out; a.out2 = P(CP_OUT2, CF_OUT2); a.silu_out = v[CV_SILU_OUT]; a.ldc = v[CV_LDC];
  a.pre = P(CP_PRE, CF_PRE); a.target = P(CP_TARGET, CF_TARGET); a.tstride = v[CV_TSTRIDE];
  a.coef = P(CP_COEF, CF_COEF); a.part = P(CP_PART, CF_PART); a.bpart = P(CP_BPART, CF_BPART);
  switch (op) {
    case COP_CONV:
      if (repack) rc = op_conv_repack_pad(cb, v[CV_CIN_RAW] > 0 ? v[CV_CIN_RAW] : ca, ca, wraw, wr, s);
      if (rc == DR_OK)
        rc = op_conv_nhwc_ex(n, ca, h, w, cb, in, wr, P(CP_BIAS, CF_BIAS), out, v[CV_NCHW], P(CP_PRE, CF_PRE), v[CV_EPI],
                             s, P(CP_CSUM, CF_CSUM));
      break;
    case COP_CONV_S3:
      if (repack) rc = op_conv_repack_split3(cb, ca, wraw, wr, s);
      if (rc == DR_OK)
        rc = op_conv_split3_ex(n, ca, h, w, cb, in, wr, P(CP_BIAS, CF_BIAS), out, v[CV_NCHW], P(CP_PRE, CF_PRE),
                               v[CV_EPI], s, v[CV_TERMS]);
      break;
    case COP_CONVT:
      if (repack) rc = op_convT_repack(ca, cb, wraw, wr, s);
      if (rc == DR_OK) rc = op_convT_nhwc(v[CV_EPI], a, s);
      break;
    case COP_CONVT_S3:
      if (repack) rc = op_convT_repack_split3(ca, cb, wraw, wr, s);
      if (rc == DR_OK) rc = op_convT_split3(v[CV_EPI], a, wr, s, v[CV_TERMS]);
      break;
    case COP_CONVT_OUT3:
      if (repack) rc = op_convT_out3_repack(ca, wraw, wr, s);
      if (rc == DR_OK) rc = op_convT_out3(a, s);
      break;
    case COP_WGRAD:
      rc = op_conv_wgrad(n, h, w, ca, cb, in, v[CV_LDA], v[CV_LO_SILU], P(CP_HI, 0), v[CV_LDB], out, v[CV_CBO], scale,
                         v[CV_ACC], P(CP_WS, CF_WS), ws_floats, s, P(CP_BIAS_OUT, CF_BIAS_OUT));
      break;
    case COP_WGRAD_S3:
      rc = op_wgrad_split3(n, h, w, ca, cb, in, v[CV_LDA], P(CP_HI, 0), v[CV_LDB], out, v[CV_CBO], scale, v[CV_ACC],
                           P(CP_WS, CF_WS), ws_floats, s, v[CV_TERMS]);
      break;
    case COP_CHAN_SUM:
      rc = op_chan_sum(n, ca, in, v[CV_LDA], out, v[CV_ACC], P(CP_WS, CF_WS), ws_floats, s);
      break;
    case COP_CHAN_SUM_FINAL:
      rc = op_chan_sum_final(n, ca, in, out, v[CV_ACC], s);
      break;
    default:
      dr_set_error("dr_internal_conv_run: unknown op %d", op);
      rc = DR_E_INVALID;
  }
  if (form && form_cap > 0 && dr_conv_form_last) snprintf(form, form_cap, "%s", dr_conv_form_last);
  if (rc != DR_OK && msg && msg_cap > 0) snprintf(msg, msg_cap, "%s", dr_last_error());
  return rc;
}

// Test hook of the grouped first Linear (tests/test_gpu_heads_fused.py): op_gemm_nt_split3_heads on caller-made
// operands.  need[0] / need[1]: the bytes of weight planes and the floats of partial sums the op asks for; with
// A == NULL nothing is launched and they alone are reported.  need[2]: op_s3_heads_splits(M, K).
extern "C" int dr_internal_s3_heads_run(int M, int K, const float* A, int lda, const float* A2, int lda2, int ksA,
                                        int nh, const int* widths, void* const* W, void* const* bias, void* const* Y,
                                        const int* ldy, void* wr, float* part, long long part_floats, long long* need,
                                        void* stream, char* msg, int msg_cap) {
  if (msg && msg_cap > 0) msg[0] = 0;
  if (nh < 1 || nh > DR_S3_HEADS || !widths) return DR_E_INVALID;
  if (need) {
    need[0] = (long long)op_nt_split3_heads_ws_bytes(widths, nh, K);
    need[1] = (long long)op_gemm_nt_split3_heads_part_floats(M, widths, nh, K);
    need[2] = op_s3_heads_splits(M, K);
  }
  if (!A) return DR_OK;
  S3Head h[DR_S3_HEADS];
  for (int i = 0; i < nh; ++i)
    h[i] = {(const float*)W[i], K, widths[i], bias ? (const float*)bias[i] : nullptr, (float*)Y[i], ldy[i]};
  const int rc = op_gemm_nt_split3_heads(M, K, A, lda, A2, lda2, ksA, h, nh, wr, part, (size_t)part_floats,
                                         (hipStream_t)stream);
  if (rc != DR_OK && msg && msg_cap > 0) snprintf(msg, msg_cap, "%s", dr_last_error());
  return rc;
}
