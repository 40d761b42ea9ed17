/*
 * libdreamer_hip -- C ABI of the MI355X (gfx950) Dreamer imagination engine.
 *
 * The reference (youngers2006/Dreamer) has no FFI: its hot path is a
 * composition of PyTorch ops inside Python classes.  Each entry point below
 * replaces one of those compositions and cites the reference code it
 * restates (file:line in /root/reference).  The Python package
 * ``dreamer_amd`` binds them with ctypes behind the reference's own class API
 * (Dreamer / WorldModel / Agent / Buffer ...).
 *
 * Conventions
 *  - every function returns 0 (DR_OK) or an error code; dr_last_error() gives
 *    a thread-local message.  Nothing throws across the ABI.
 *  - all pointers are device pointers owned by the caller (the PyTorch caching
 *    allocator); the library never allocates, frees, or keeps a pointer after
 *    returning.  Scratch comes from the caller's workspace (sizes from the
 *    *_bytes queries).
 *  - calls are asynchronous on the given hipStream_t; no implicit sync, so the
 *    whole train_Agent epoch can be captured into one hipGraph.
 *  - parameters are read in PyTorch's own layouts (Linear weight [out][in],
 *    GRUCell weight_ih [3H][in] gate order r,z,n, Conv2d [out][in][4][4]).
 *  - fp32 mode: the bias of a Conv2d / ConvTranspose2d layer whose shape runs on
 *    the split-conv kernels (32 / 64 / 128 / 256 input channels, a multiple of
 *    64 output channels -- 64 -> 32 for a transposed conv too) must be 16-byte
 *    aligned.  dr_encoder_features and the world-model training step return
 *    DR_E_INVALID, nothing launched, when it is not; dr_last_error() names the
 *    pointer.  (A tensor from the PyTorch allocator always is; a view at an
 *    offset that is no multiple of 4 floats is not.)
 *  - supported widths ("Supported widths"): hidden % 4 == 0;
 *    rows % 4 == 0, rows <= 32; cols divides 32; action <= 8; pixel
 *    encoders enc_f1, enc_f2 % 4 == 0 and img_h, img_w multiples of 2^depth,
 *    vector encoders obs_dim % 4 == 0.  The dr_imagine_*, dr_observe_*,
 *    dr_wm_train_*, dr_act_* entry points and dr_actor_act check the ones
 *    they depend on first and return DR_E_INVALID, nothing launched,
 *    outside them; dr_last_error() names the field, its value and the limit.
 *    The MLP widths and the bucket count are free.
 *  - arithmetic is fp32 (parity mode) unless dr_dims.precision selects bf16:
 *    fp32 GEMMs use the exact-f32 MFMA (v_mfma_f32_16x16x4_f32), elementwise
 *    code is built -ffp-contract=off; bf16 mode runs the encoder convolutions
 *    and feature projection on v_mfma_f32_16x16x32_bf16 (f32 accumulate).
 */
#ifndef DREAMER_HIP_H
#define DREAMER_HIP_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_OK 0
#define DR_E_INVALID 1001   /* bad dims / pointers */
#define DR_E_HIP 1002       /* a HIP launch failed */
#define DR_E_WORKSPACE 1003 /* workspace too small */
#define DR_E_UNSUPPORTED 1004 /* valid call outside what this entry point covers (dims / device):
                                 use the unfused entry points (dr_act_step) */

/* Linear (or LayerNorm) parameters: w [out][in] (LN: gamma [n]), b [out]. */
typedef struct { float* w; float* b; } dr_linear;

/* nn.Sequential(Linear, LayerNorm, SiLU, Linear, LayerNorm, SiLU, Linear)
 * indices 0,1,3,4,6 (DynamicsPredictors.py:15-23,52-60,85-93; Agent.py:219-227). */
typedef struct { dr_linear l0, n1, l3, n4, l6; } dr_mlp3;

/* Model widths (Dreamer.py:20-64 config keys). */
typedef struct {
  int hidden;          /* hidden_state_dims (600) */
  int rows, cols;      /* latent_state_dims (32, 32) */
  int action;          /* action_dims (3) */
  int img_h, img_w;    /* observation_dims (64, 64) */
  int enc_f1, enc_f2;  /* encoder_filter_num_1/2 (32, 64): conv channels f1, f2, 2*f2, 4*f2 */
  int enc_hidden;      /* encoder_hidden_layer_nodes (200) */
  int prior_h1, prior_h2, rew_h1, rew_h2, cont_h1, cont_h2;
  int actor_h1, actor_h2, critic_h1, critic_h2;
  int buckets;         /* critic_reward_buckets (255) */
  int dec_f1, dec_f2;  /* decoder_filter_num_1/2 (32, 64): convT channels 4*f2 -> 2*f2 -> f2 -> f1 -> 3 */
  int dec_hidden;      /* decoder_hidden_layer_nodes (200) */
  int precision;       /* DR_PREC_FP32 (parity mode, default) or DR_PREC_BF16 (perf mode: bf16 MFMA
                          operands, f32 accumulation; the extra `precision` config key) */
  int obs_dim;         /* 0: pixel observations img_h x img_w x 3 (the reference).  D > 0: proprioceptive
                          vector observations of D floats (BASELINE configs[4]; the reference has no such
                          encoder, VAE.py:33-42 is always convolutional).  The convolution slots then hold
                          an MLP: encoder conv[0] = Linear(D, 4*enc_f2), conv[1] =
                          Linear(4*enc_f2, 4*enc_f2), each + SiLU (F = 4*enc_f2 features, conv[2..3]
                          unused); decoder upscaler.3 -> 4*dec_f2, convt[0] = Linear(4*dec_f2, 4*dec_f2)
                          + SiLU, convt[1] = Linear(4*dec_f2, D) (no Tanh; convt[2..3] unused). */
  int enc_depth;       /* k4 s2 p1 convolutions of the encoder (and transposed convolutions of the decoder):
                          0 or 4 = the reference's VAE (VAE.py:33-42, 128-137); 5 = the "deeper VAE" of BASELINE
                          configs[3] (the extra config key encoder_depth; no reference definition -- one more
                          stride-2 layer each way, so 128x128 frames reach the same 4x4 grid 64x64 frames reach
                          in the reference): encoder channels 3, f1, f2, 2 f2, 4 f2, 4 f2 (conv[0..4]); decoder
                          4 d2 (H/32 x W/32) -> 4 d2 -> 2 d2 -> d2 -> d1 -> 3 (convt[0..4]). */
  int launch_form;     /* 0 (default): an entry point may run as ONE persistent launch where the shape and the
                          stream's CUs allow it (the warm start's posterior scan, scan.hip); 1: always the
                          launch sequence.  Set for work captured on one stream and replayed on a CU-masked
                          one (the pipelined epochs' warm start), and by DREAMER_PERSISTENT=0. */
  float* fault;        /* device float, may be NULL: the fault slot of the persistent launches (posterior
                          scan, imagination unroll, BPTT).  Their waits on other workgroups are bounded; if
                          one times out (a workgroup was not resident, e.g. held off by other work on the
                          CUs), the launch's outputs are written NaN and *fault = NaN.  Sticky: the library
                          never clears it.  The engine keeps it among the agent's loss slots, so the
                          non-finite skip (Agent.py:137-139) rejects that epoch's update on every rank.  Test
                          hook: DREAMER_PERSIST_FORCE=timeout (or scan / dream / bptt) makes every wait of
                          those launches time out, read at each call. */
  unsigned* fault_host; /* may be NULL: a word of pinned host memory (its device address,
                          dr_host_device_ptr) set to 1 on the same timeouts, so the host notices a fault
                          without a copy or a sync (dreamer_amd/engine.py check_faults raises).  Sticky. */
} dr_dims;
#define DR_MAX_DEPTH 5
#define DR_PREC_FP32 0
#define DR_PREC_BF16 1

/* WorldModel parameters (WorldModel.py:55-60). */
typedef struct {
  dr_linear conv[DR_MAX_DEPTH];   /* encoder.feature_extractor.{0,2,4,6(,8)} (dr_dims.enc_depth layers) */
  dr_linear map0, map1, map3;     /* encoder.latent_mapper.{0, 1 (LN), 3} */
  float *w_ih, *w_hh, *b_ih, *b_hh; /* sequence_model.GRU */
  dr_mlp3 prior;                  /* dynamics_predictor.logit_net */
  dr_mlp3 reward;                 /* reward_predictor.logit_net */
  dr_mlp3 cont;                   /* continue_predictor.logit_generator */
  float* buckets_rew;             /* reward_predictor.buckets_rew */
} dr_world_model;

/* Decoder parameters (VariationalAutoEncoder.py:118-137). */
typedef struct {
  dr_linear up0, up1, up3;        /* decoder.upscaler.{0, 1 (LN), 3} */
  dr_linear convt[DR_MAX_DEPTH];  /* decoder.image_builder.{0,2,4,6(,8)}: ConvTranspose2d w [in][out][4][4] */
} dr_decoder;

/* Actor (Agent.py:174-200): base_net.{0,1,3,4}, mu_head, log_sig_head. */
typedef struct { dr_linear l0, n1, l3, n4, mu, ls; } dr_actor;

/* Critic (Agent.py:212-241): value_net, buckets_crit. */
typedef struct { dr_mlp3 net; float* buckets; } dr_critic;

/* Randomness.  Explicit-noise mode reproduces the reference's draws
 * (parity); Philox mode generates them in-kernel keyed by
 * (seed, offset, stream, global row, element) so a data-parallel shard draws
 * exactly what the single-GPU run draws for the same global rows. */
typedef struct {
  const float* q;   /* Exp(1) variates [steps][rows*R][C] (Categorical sample), or NULL */
  const float* eps; /* N(0,1) variates [steps][rows][A] (actor rsample), or NULL */
  const unsigned long long* rng; /* device {seed, offset}; used where q/eps are NULL */
  int row0;         /* global index of local row 0 */
  int stream;       /* Philox stream id (distinct per call site) */
} dr_noise;

/* Source of observation frames for the encoder.  Frame f = t*B + b. */
typedef struct {
  const unsigned char* ring; /* u8 replay ring [cap][3][H][W] (Buffer.py:7), or NULL; with dr_dims.obs_dim
                                = D > 0 the ring holds f32 rows [cap][D] (pointer cast) */
  long long ring_cap;
  const long long* starts;   /* device [B] window starts (Buffer.py:36-50) */
  const float* obs;          /* f32 frames (when ring == NULL) */
  long long stride_b, stride_t; /* f32: element offset of frame (b,t) = b*stride_b + t*stride_t */
  int raw255;                /* 1: values are 0..255 -> x/255-0.5 (Dreamer.py:251); 0: already normalised */
  int t0;                    /* time offset: frame (b, t) is window step t0 + t (chunked encoding) */
} dr_frames;

const char* dr_last_error(void);
int dr_version(void);

/* A HIP stream whose kernels run only on the CUs set in mask (n_words 32-bit
 * words, bit i = CU i of the device's CU-mask order; hipExtStreamCreateWithCUMask).
 * The pipelined AC_epochs > 1 schedule (dreamer_amd/engine.py run_many) fences
 * the next epoch's warm start (conv encoder + posterior scan) off part of the
 * chip so that the latency-bound imagination / update chain keeps free CUs.
 * No Dreamer.py counterpart: a scheduling aid of this implementation. */
int dr_stream_create_cumask(int n_words, const unsigned* mask, hipStream_t* out);
int dr_stream_destroy(hipStream_t s);
/* the device's CU count (hipDeviceAttributeMultiprocessorCount) */
int dr_device_cus(int* out);
/* the device address of pinned host memory (hipHostGetDevicePointer): dr_dims.fault_host */
int dr_host_device_ptr(void* host, void** dev);

/* ---- a3  Encoder conv stack + latent_mapper.0 feature columns ---------------
 * feat[f][enc_hidden] = flatten(SiLU(conv4(...SiLU(conv1(frame f)))))
 *                       . map0.w[:, :F]^T + map0.b            (VAE.py:57-75)
 * for the n = B*T frames of `src` (time-major: f = t*B + b). */
size_t dr_encoder_workspace_bytes(const dr_dims* d, int n_frames);
int dr_encoder_features(const dr_dims* d, const dr_world_model* wm, const dr_frames* src, int B, int T,
                        float* feat, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---- a2/a5  posterior scan (warm_start_generator, Dreamer.py:244-262;
 *      observe_step, WorldModel.py:79-82; Encoder.encode, VAE.py:77-99) -----
 * If z_init == NULL, frame 0 is an encode from h_init (zeros if NULL) and
 * frame t>=1 runs GRU(z, actions[t-1], h) first.  If z_init != NULL every
 * frame t runs GRU(z, actions[t], h) first.  actions element (b,t,i) is at
 * actions[b*act_sb + t*act_st + i].  Writes the last frame's z, h (and
 * logits if non-NULL). */
size_t dr_observe_workspace_bytes(const dr_dims* d, int B);
int dr_observe_scan(const dr_dims* d, const dr_world_model* wm, int B, int T, const float* feat,
                    const float* actions, long long act_sb, long long act_st, const float* h_init,
                    const float* z_init, dr_noise noise, float* z_out, float* h_out, float* logits_out,
                    void* ws, size_t ws_bytes, hipStream_t stream);

/* ---- posterior trace: the same filter keeping EVERY step (the closed-loop
 *      diagnostic of Dreamer.closed_loop / WorldModel.observe_sequence) ---------
 * Arguments feat .. noise as dr_observe_scan (warm_start_generator's
 * convention, Dreamer.py:244-262, when z_init == NULL: h_0 = h_init or 0,
 * z_0 ~ posterior(h_0, x_0) with draw 0; observe_step, WorldModel.py:79-82, per
 * further frame, draw t).  Outputs, entry t from the state after frame t:
 *   latents      [B][T][R*C]     z_t (straight-through one-hot, VAE.py:88-98)
 *   hiddens      [B][T][hidden]  h_t (SequenceModel.py:19-24)
 *   post_logits  [B][T][R*C]     the encoder's raw logits (VAE.py:77-87), may be NULL
 *   prior_logits [B][T][R*C]     dynamics_predictor.logit_net(h_t)
 *                                (DynamicsPredictors.py:25-29), may be NULL
 *   rewards / continues [B][T]   symexp E[bucket] and sigmoid of the heads on
 *                                (h_t, z_t) (DynamicsPredictors.py:64-74, 95-105),
 *                                both or neither; entry 0 rides along
 *                                (unroll_model compares entry t >= 1 with the
 *                                targets of step t-1, WorldModel.py:113-123)
 * Always the launch sequence (dr_dims.launch_form is ignored; there is no
 * persistent form): per step dr_observe_scan's launch-form kernels -- the fused
 * one-hot GRU, the grouped latent_mapper.0 (+ the next hidden product at
 * B >= 128, on the same weight planes), the LN-SiLU sampler head, whose logits
 * store goes straight to post_logits -- and one strided copy of z_t, h_t into
 * the trace; then the prior MLP and the heads once over the B*T rows.  Honours
 * dr_dims.precision like dr_observe_scan.
 * Contract: entry t of latents / hiddens / post_logits is bit for bit what
 * dr_observe_scan returns in launch form (dr_dims.launch_form = 1) for the
 * prefix T' = t + 1 on the same inputs and noise.  (The scan's last step runs
 * latent_mapper.0 alone; at B >= 128 a step that is not the last runs it
 * grouped with the next hidden product on the weight planes and goes on from
 * that.  The trace does the same, and reports such a step a second time in the
 * last-step form: two more launches per step at B >= 128.)  A trace of T steps
 * equals a trace of T1 steps followed by a continuing call (h_init, z_init =
 * entry T1 - 1, actions / feat / noise advanced by T1 steps) of T - T1 steps,
 * as a time-chunked dr_observe_scan equals the whole scan: the next step reads
 * z_t's indices and straight-through values. */
size_t dr_observe_trace_workspace_bytes(const dr_dims* d, int B, int T);
int dr_observe_trace(const dr_dims* d, const dr_world_model* wm, int B, int T, const float* feat,
                     const float* actions, long long act_sb, long long act_st, const float* h_init,
                     const float* z_init, dr_noise noise, float* latents, float* hiddens, float* post_logits,
                     float* prior_logits, float* rewards, float* continues, void* ws, size_t ws_bytes,
                     hipStream_t stream);

/* ---- a7  imagination unroll (dream_episodes, Dreamer.py:143-175) -----------
 * Outputs use the reference's layouts: latents [B][H+1][R*C], hiddens
 * [B][H+1][hidden], actions/mus/sigmas [B][H][A], rewards/continues [B][H].
 * `tape` (dr_imagine_tape_bytes) keeps what dr_imagine_bwd needs. */
size_t dr_imagine_tape_bytes(const dr_dims* d, int B, int H);
size_t dr_imagine_workspace_bytes(const dr_dims* d, int B, int H);
int dr_imagine_fwd(const dr_dims* d, const dr_world_model* wm, const dr_actor* actor, int B, int H,
                   const float* z0, const float* h0, dr_noise noise, int deterministic, float* latents,
                   float* hiddens, float* actions, float* rewards, float* continues, float* mus,
                   float* sigmas, void* tape, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---- open-loop prediction: the same unroll under GIVEN actions (imagine_step
 *      with a recorded action, WorldModel.py:72-77, iterated as dream_episodes
 *      iterates it, Dreamer.py:158-164, without the actor) ---------------------
 * State 0 is (h0, z0) ([B][hidden], [B][R*C]); for k = 1..H
 *   h_k = GRU(z_{k-1}, a_{k-1}, h_{k-1})  (SequenceModel.py:19-24),
 *   z_k ~ prior(h_k), draw k-1             (DynamicsPredictors.py:25-39),
 *   r_k = symexp E[bucket], c_k = sigmoid  (DynamicsPredictors.py:64-74, 95-105)
 * on (h_k, z_k).  actions element (b, k, i) is at actions[b*act_sb + k*act_st
 * + i]; entry k drives the step k -> k+1.  Outputs in dr_imagine_fwd's
 * layouts: latents [B][H+1][R*C], hiddens [B][H+1][hidden], rewards /
 * continues [B][H] (entry k-1 holds r_k / c_k).  Noise: explicit q
 * [H][B*R][C] (draw k-1 at step index k-1) or Philox on `noise.stream`.  No
 * tape, no actor.  Always the launch sequence (per step: fused one-hot GRU;
 * one grouped launch of the products that read only h_{k+1} -- the prior's
 * first Linear and, at B >= 128, the next step's hidden product; the prior's
 * LN-SiLU layer; the sampler head), then the reward / continue heads once over
 * the B*(H+1) states, the kernels dr_imagine_fwd's launch form runs.  Honours
 * dr_dims.precision like dr_imagine_fwd. */
size_t dr_imagine_actions_workspace_bytes(const dr_dims* d, int B, int H);
int dr_imagine_actions(const dr_dims* d, const dr_world_model* wm, int B, int H, const float* z0, const float* h0,
                       const float* actions, long long act_sb, long long act_st, dr_noise noise, float* latents,
                       float* hiddens, float* rewards, float* continues, void* ws, size_t ws_bytes,
                       hipStream_t stream);

/* Backprop through the unroll for the actor (Agent.py:141-145 backward):
 * given dL/dmus, dL/dsigmas (and optionally dL/dactions, dL/dlatents,
 * dL/dhiddens; NULL = 0), writes dL/d(actor params) into `grad` (overwrite).
 * World-model weights receive no gradient (the reference's WM grads from this
 * path are discarded by WorldModel.training_step's zero_grad, WorldModel.py:195). */
int dr_imagine_bwd(const dr_dims* d, const dr_world_model* wm, const dr_actor* actor, int B, int H,
                   const float* latents, const float* hiddens, const float* actions, const float* g_mus,
                   const float* g_sigmas,
                   const float* g_actions, const float* g_latents, const float* g_hiddens,
                   const void* tape, const dr_actor* grad, void* ws, size_t ws_bytes, hipStream_t stream);
/* dr_imagine_bwd in two parts on the same workspace: _prep writes the upstream
 * state gradients (NULL = 0) and the transposed weights -- it needs neither
 * dL/dmus nor the tape, so it can run on a second stream while the returns and
 * losses are formed; _main runs the reverse loop and the weight gradients
 * (upstream_state: 1 if _prep was given dL/dlatents or dL/dhiddens). */
int dr_imagine_bwd_prep(const dr_dims* d, const dr_world_model* wm, const dr_actor* actor, int B, int H,
                        const float* g_actions, const float* g_latents, const float* g_hiddens, void* ws,
                        size_t ws_bytes, hipStream_t stream);
int dr_imagine_bwd_main(const dr_dims* d, const dr_world_model* wm, const dr_actor* actor, int B, int H,
                        const float* latents, const float* hiddens, const float* actions, const float* g_mus,
                        const float* g_sigmas, int upstream_state, const void* tape, const dr_actor* grad, void* ws,
                        size_t ws_bytes, hipStream_t stream);

/* ---- single steps (batch-1 acting path and per-block API) ------------------ */
/* imagine_step (WorldModel.py:72-77): h' = GRU(z,h,a); z' ~ prior(h'); r; c */
int dr_imagine_step(const dr_dims* d, const dr_world_model* wm, int B, const float* h, const float* z,
                    const float* a, dr_noise noise, float* h_out, float* z_out, float* r_out, float* c_out,
                    void* ws, size_t ws_bytes, hipStream_t stream);
/* Actor.act (Agent.py:202-210); workspace from dr_actor_act_workspace_bytes */
size_t dr_actor_act_workspace_bytes(const dr_dims* d, int B);
int dr_actor_act(const dr_dims* d, const dr_actor* actor, int B, const float* h, const float* z,
                 dr_noise noise, int deterministic, float* a_out, float* mu_out, float* sigma_out, void* ws,
                 size_t ws_bytes, hipStream_t stream);
/* Batch-1 acting step in ONE launch with in-kernel grid barriers (rollout_policy
 * / evaluate_agent / Run, Dreamer.py:177-226, 295-322, 374-401): if has_prev,
 * h' = GRU(z_prev, h, a_prev) (observe_step, WorldModel.py:79-82), else h' = 0
 * (episode start, Dreamer.py:186-187) and h, z_prev and a_prev are not read (h
 * must still be non-null; z_prev and a_prev may be NULL);
 * z' = Encoder.encode(h', frame) (VAE.py:57-99); a = Actor.act(h', z',
 * deterministic) (Agent.py:202-210).  It is dr_act_batch with one row, the
 * row's first flag (!has_prev) taken on the host: the same kernel, the same
 * bits, no extra launch or copy.
 * frame: the env observation [H][W][3] u8 on the device.  Noise: the sampler
 * draws stream `noise.stream`, the actor `noise.stream + 1` (explicit q [R*C],
 * eps [A] when given).  logits_out may be NULL.  Inputs and outputs may alias
 * (h / h_out, z_prev / z_out, a_prev / a_out).
 * dr_act_step_workspace_bytes(d) == dr_act_batch_workspace_bytes(d, 1); the
 * workspace starts with workgroup 0's stage clock (16 int64 of 100 MHz ticks:
 * words 0 ... 7 the stage ends, 15 the end of the kernel).
 * DR_E_INVALID: null pointers, obs_dim != 0 (vector observations: dr_act_vec).
 * Co-residency of the grid is checked once per device (occupancy query); the
 * call returns DR_E_UNSUPPORTED when the device cannot hold it, or for dims
 * outside the kernel's staging (callers then use the unfused entry points).
 * status (device int, may be NULL; the caller zeroes it): set to 1 if a grid
 * barrier timed out at run time; it is the authoritative signal -- all five
 * outputs then hold NaN and must not be used.
 * Test hook: the environment variable DREAMER_ACT_FORCE=timeout (every grid
 * barrier times out at once) or =nonresident (the co-residency check fails),
 * read at each call. */
size_t dr_act_step_workspace_bytes(const dr_dims* d);
int dr_act_step(const dr_dims* d, const dr_world_model* wm, const dr_actor* actor, const unsigned char* frame,
                int has_prev, const float* z_prev, const float* h, const float* a_prev, dr_noise noise,
                int deterministic, float* z_out, float* h_out, float* a_out, float* mu_out, float* sigma_out,
                float* logits_out, int* status, void* ws, size_t ws_bytes, hipStream_t stream);
/* The same step for n_env <= DR_ACT_MAX_ENVS environments in ONE launch
 * (vectorised rollout_policy / evaluate_agent; the reference drives one env,
 * Dreamer.py:177-226, 295-322).  Per row e, dr_act_step's semantics: if
 * first[e], h'_e = 0 (episode start, Dreamer.py:186-187, 222) and row e of
 * z_prev / h / a_prev is not read (it may be stale); otherwise h'_e =
 * GRU(z_prev_e, h_e, a_prev_e) (observe_step, WorldModel.py:79-82).  Then
 * z'_e = Encoder.encode(h'_e, frame_e) (VAE.py:57-99) and a_e = Actor.act(h'_e,
 * z'_e, deterministic) (Agent.py:202-210).
 * frames [n_env][H][W][3] u8 and first [n_env] u8 on the device; states and
 * outputs are row-major [n_env][...].  Noise: explicit q [n_env*R][C] and eps
 * [n_env][A]; Philox draws row e as dr_act_step would with row0 + e (sampler
 * stream `noise.stream`, actor `noise.stream + 1`).  Row e's outputs depend on
 * row e's inputs and noise alone and are the same bits for every n_env and row
 * position: the bits dr_act_step, its one-row call, gives on them.
 * h / h_out, z_prev / z_out and a_prev / a_out may alias.
 * DR_E_UNSUPPORTED: n_env > DR_ACT_MAX_ENVS, the dims dr_act_step rejects, or
 * a device that cannot hold the grid (checked per n_env with the dynamic LDS
 * that batch launches).  DR_E_INVALID: n_env < 1, null pointers.
 * status and DREAMER_ACT_FORCE as dr_act_step: after a barrier timeout status
 * is 1 and all five outputs of every row hold NaN. */
#define DR_ACT_MAX_ENVS 16
size_t dr_act_batch_workspace_bytes(const dr_dims* d, int n_env);
int dr_act_batch(const dr_dims* d, const dr_world_model* wm, const dr_actor* actor, int n_env,
                 const unsigned char* frames, const unsigned char* first, const float* z_prev, const float* h,
                 const float* a_prev, dr_noise noise, int deterministic, float* z_out, float* h_out, float* a_out,
                 float* mu_out, float* sigma_out, float* logits_out, int* status, void* ws, size_t ws_bytes,
                 hipStream_t stream);
/* dr_act_batch for vector observations (dr_dims.obs_dim = D > 0): the same step
 * for n_env = 1 ... DR_ACT_MAX_ENVS environments in ONE launch, the encoder's
 * convolutions replaced by the MLP of DESIGN.md 2c (conv[0] = Linear(D, F) +
 * SiLU, conv[1] = Linear(F, F) + SiLU, F = 4*enc_f2 features into
 * latent_mapper.0 on cat(features, h')).  Per row e: if first[e], h'_e = 0
 * (episode start, Dreamer.py:186-187, 222) and row e of z_prev / h / a_prev is
 * not read; otherwise h'_e = GRU(z_prev_e, h_e, a_prev_e) (observe_step,
 * WorldModel.py:79-82).  Then z'_e = Encoder.encode(h'_e, obs_e) (VAE.py:73-99
 * past the feature extractor) and a_e = Actor.act(h'_e, z'_e, deterministic)
 * (Agent.py:202-210).  obs [n_env][obs_dim] f32 and first [n_env] u8 on the
 * device.  Noise, aliasing, status and DREAMER_ACT_FORCE as dr_act_batch; row
 * e's outputs depend on row e's inputs and noise alone and are the same bits
 * for every n_env, row position and mix of first flags (n_env = 1 is the
 * batch-1 step).  The kernel shares everything but its encoder stages with
 * dr_act_batch's (act.hip).
 * DR_E_INVALID: n_env < 1, null pointers, obs_dim == 0 (pixel models use
 * dr_act_step / dr_act_batch).  DR_E_UNSUPPORTED: n_env > DR_ACT_MAX_ENVS,
 * obs_dim > DR_ACT_VEC_MAX_OBS, 4*enc_f2 > 256 or the other widths dr_act_step
 * bounds, or a device that cannot hold the grid. */
/* obs_dim < 1024; any D up to it is taken (no multiple-of-4 rule here, unlike dr_encoder_features) */
#define DR_ACT_VEC_MAX_OBS 1023
size_t dr_act_vec_workspace_bytes(const dr_dims* d, int n_env);
int dr_act_vec(const dr_dims* d, const dr_world_model* wm, const dr_actor* actor, int n_env, const float* obs,
               const unsigned char* first, const float* z_prev, const float* h, const float* a_prev, dr_noise noise,
               int deterministic, float* z_out, float* h_out, float* a_out, float* mu_out, float* sigma_out,
               float* logits_out, int* status, void* ws, size_t ws_bytes, hipStream_t stream);

/* GRU cell (SequenceModel.py:19-24) */
int dr_gru_cell(const dr_dims* d, const dr_world_model* wm, int B, const float* z, const float* h,
                const float* a, float* h_out, void* ws, size_t ws_bytes, hipStream_t stream);
/* Categorical sampler with unimix + straight-through value (VAE.py:88-98,
 * DynamicsPredictors.py:33-39): z = onehot(argmax(p_hat/q)) + p - p (value). */
int dr_categorical_sample(int M, int R, int C, const float* logits, dr_noise noise, float* z_out,
                          int* idx_out, float* soft_out, hipStream_t stream);
/* heads: prior logits, reward value (symexp E[bucket]), continue prob */
int dr_mlp3_fwd(const dr_mlp3* m, int M, int in_h, const float* h, long long ldh, int in_z, const float* z,
                long long ldz, int h1, int h2, int n_out, float* out, long long ldo, void* ws, size_t ws_bytes,
                hipStream_t stream);
size_t dr_step_workspace_bytes(const dr_dims* d, int B);
int dr_bucket_value(int M, int nb, const float* logits, const float* buckets, float* out, hipStream_t stream);

/* ---- a13-a16  actor-critic update pieces (Agent.py:78-172) ----------------- */
size_t dr_critic_tape_bytes(const dr_dims* d, int M);
size_t dr_critic_workspace_bytes(const dr_dims* d, int B, int H);
/* logits [M][nb] (optional), values [M] (optional); tape (optional) for bwd */
int dr_critic_fwd(const dr_dims* d, const dr_critic* c, int M, const float* h, long long ldh, const float* z,
                  long long ldz, float* logits, float* values, void* tape, void* ws, size_t ws_bytes,
                  hipStream_t stream);
/* The four heads that read the B*(H+1) imagined states in one pass: the reward
 * and continue heads (dr_imagine_fwd's, rewards / continues [B][H]) and the
 * target and online critics' values V_t, V_c [B][H+1] with the online critic's
 * tape (dr_critic_tape_bytes(d, B*(H+1))), from dr_imagine_fwd's latents /
 * hiddens.  The four first Linears over [h | z] run as one grouped product;
 * every output holds the bits that dr_imagine_fwd's heads and dr_critic_fwd
 * (target: values only, its workspace; online: values and tape) give on the
 * same inputs.  ws_im / ws_cr: the dr_imagine_fwd / dr_critic_fwd workspaces
 * (scratch of the tails), ws: dr_heads_workspace_bytes.  dr_imagine_fwd skips
 * its own heads when rewards and continues are both NULL.
 * dr_heads_supported: 1 in fp32 mode with B*(H+1) >= 1024 and head widths that
 * are multiples of 4 (<= 208 for the reward / continue heads); otherwise
 * dr_heads_fwd returns DR_E_UNSUPPORTED with nothing launched and nothing
 * written, and dr_heads_workspace_bytes returns 0. */
int dr_heads_supported(const dr_dims* d, int B, int H);
size_t dr_heads_workspace_bytes(const dr_dims* d, int B, int H);
int dr_heads_fwd(const dr_dims* d, const dr_world_model* wm, const dr_critic* target, const dr_critic* online,
                 int B, int H, const float* latents, const float* hiddens, float* rewards, float* continues,
                 float* V_t, float* V_c, void* ctape, void* ws_im, size_t ws_im_bytes, void* ws_cr,
                 size_t ws_cr_bytes, void* ws, size_t ws_bytes, hipStream_t stream);
/* lambda returns (Agent.py:156-172): V [B][H+1] target values */
int dr_lambda_returns(int B, int H, const float* r, const float* c, const float* V, float gamma, float lam,
                      float* R, hipStream_t stream);
/* update_S (Agent.py:78-88) over n returns; S is a device scalar updated in
 * place unless R holds NaN/Inf; norm_out = max(S, 1) (Agent.py:120). */
int dr_update_S(int n, const float* R, float* S, float* norm_out, void* ws, size_t ws_bytes,
                hipStream_t stream);
/* actor loss (Agent.py:105-125) and its gradient wrt mus/sigmas; loss_out
 * holds 1 + B*H floats: [0] = mean loss over the B*H local rows, the rest is
 * per-row scratch.  scale = dL/d(row loss) (1/(B*H) on one device). */
int dr_actor_loss_grad(int B, int H, int A, const float* mus, const float* sigmas, const float* actions,
                       const float* R, const float* V, const float* norm, float nu, float scale,
                       float* loss_out, float* g_mus, float* g_sigmas, hipStream_t stream);
/* critic two-hot cross-entropy (Agent.py:127-135) + backward into `grad`
 * (overwrite); rows are (b,t) with t<=H of hiddens/latents; row t=H is unused. */
int dr_critic_loss_bwd(const dr_dims* d, const dr_critic* c, int B, int H, const float* hiddens,
                       const float* latents, const float* R, const void* tape, float scale, float* loss_out,
                       const dr_critic* grad, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---- optimiser (torch.optim.AdamW + clip_grad_norm_ + soft target) -------- */
int dr_sqnorm(long long n, const float* g, float* acc, hipStream_t stream);
/* as dr_sqnorm, many workgroups (large buffers); scratch >= 512 floats */
int dr_sqnorm_multi(long long n, const float* g, float* acc, float* scratch, hipStream_t stream);
/* The agent's pre-update statistics in one launch (Agent.py:137-148):
 * sq[0] = |ga|^2 (actor grads), sq[1] = |gb|^2 (critic grads), *skip = any
 * non-finite value among loss[0..nloss).  Replaces the NaN check and the two
 * clip_grad_norm_ reductions.  scratch: DR_CLIP_SCRATCH_FLOATS floats,
 * zeroed once by the caller (holds the partials and an arrival ticket the
 * kernel re-arms); buffers 16-byte aligned.  Deterministic. */
#define DR_CLIP_SCRATCH_FLOATS 1024
int dr_clip_stats(long long na, const float* ga, long long nb, const float* gb, int nloss, const float* loss,
                  float* sq, int* skip, void* scratch, hipStream_t stream);
/* p <- AdamW(p, g*clip) (torch.optim.AdamW single-tensor op order) where
 * clip = min(1, max_norm/(sqrt(*sqnorm)+1e-6)) (sqnorm NULL: no clip).  The
 * step counter lives on the device: a prelude increments *step and writes
 * hyper[0] = lr/(1-b1^step), hyper[1] = sqrt(1-b2^step) (double math, like
 * torch's python scalars; the hyperparameters are doubles, like the python
 * floats torch.optim.AdamW computes 1 - beta etc. from).  g is scaled in place
 * by clip (as clip_grad_norm_ does).  Everything is skipped when *skip != 0. */
int dr_adamw(long long n, float* p, float* g, float* m, float* v, const float* sqnorm, float max_norm,
             double lr, double b1, double b2, double eps, double wd, int* step, float* hyper, const int* skip,
             hipStream_t stream);
int dr_ema(long long n, float* target, const float* src, float keep, float tau, const int* skip,
           hipStream_t stream);
/* Agent.train_step's whole optimiser tail in two launches (Agent.py:137-153):
 * dr_clip_stats over (actor, critic) grads with both AdamW preludes run by its
 * last workgroup, then dr_adamw(actor, clip by sq[0]), dr_adamw(critic, clip by
 * sq[1]) and dr_ema(target <- ema_keep * target + tau * critic) in one
 * elementwise pass.  Same per-element arithmetic (same bits) as those five
 * calls; scratch as dr_clip_stats. */
int dr_ac_optimiser_step(long long na, float* pa, float* ga, float* ma, float* va, int* step_a, float* hyper_a,
                         double lr_a, double b1_a, double b2_a, double eps_a, double wd_a, long long nc, float* pc,
                         float* gc, float* mc, float* vc, int* step_c, float* hyper_c, double lr_c, double b1_c,
                         double b2_c, double eps_c, double wd_c, float max_norm, float* target, float ema_keep,
                         float tau, int nloss, const float* loss, float* sq, int* skip, void* scratch,
                         hipStream_t stream);
/* non-finite flag: *flag = any(!isfinite(x[0..n))) (OR-accumulate) */
int dr_nonfinite(long long n, const float* x, int* flag, hipStream_t stream);

/* ---- a19/a20  world-model training step (WorldModel.training_step,
 *      WorldModel.py:148-198; unroll_model 84-146; Decoder.forward VAE.py:139-161)
 * Loss and gradients of one step over a window of T = horizon frames per row:
 * posterior scan (observe_step with the GRU run from zeros at t = 0), batched
 * prior / decoder / reward / continue heads on steps 1..T-1, the masked
 * reconstruction / reward / continue / KL losses with the max(1, KL) free-bit
 * clamps, and backprop through everything (decoder and encoder convolutions,
 * the posterior scan's GRU and straight-through samples) into `g_wm` /
 * `g_dec` (overwrite).  Arithmetic is fp32: the reference's fp16 autocast +
 * GradScaler is, in fp32, the plain backward (the scaler only skips steps with
 * non-finite gradients -- `skip` reports a non-finite loss; callers OR in a
 * gradient check).  losses (device, 4 floats): total, loss_pred, KL_dyn,
 * KL_rep (both KL means; the free-bit clamp is applied in `total`).
 * Frames: src frame (b, t) is window step t (time-major f = t*B + b).
 * Optional outputs (time-major [T][B][...]): posterior hiddens, latents, logits. */
typedef struct {
  const float* actions; long long act_sb, act_st;                     /* (b,t,i) at b*sb + t*st + i */
  const float* rewards; const float* continues; long long rc_sb, rc_st; /* (b,t) at b*sb + t*st */
} dr_wm_batch;
typedef struct { float beta_pred, beta_dyn, beta_rep; } dr_wm_loss_cfg;
size_t dr_wm_train_workspace_bytes(const dr_dims* d, int B, int T);
/* The same step in three phases for data parallelism (one shard of B rows per
 * rank, same workspace across the phases).  `stats` (device, 8 floats) carries
 * the loss sums that must be global: after DR_WM_PREP the caller all-reduces
 * (sum) stats[0] (mask.sum(), WorldModel.py:185), after DR_WM_FWD stats[1..4]
 * (masked squared-error, reward, continue and KL sums); DR_WM_BWD then forms
 * the global losses (rows_global = global B * (T-1) for the KL means,
 * 182-183) and gradients whose all-reduce SUM is the global gradient. */
#define DR_WM_PREP 1
#define DR_WM_FWD 2
#define DR_WM_BWD 4
/* DR_WM_BWD in three stages, called in this order with the same workspace;
 * each leaves one bucket of the gradient final, so a data-parallel caller can
 * all-reduce it while the next stage runs (WorldModel.py:195-200 backward +
 * SURVEY 8e "bucketed to overlap the backward"):
 *   HEADS: the loss grads, prior / reward / continue heads and the decoder
 *          (g_wm->prior, ->reward, ->cont, every g_dec field) final;
 *   SCAN:  the posterior scan: latent_mapper and GRU (->map0/1/3, ->w_ih,
 *          ->w_hh, ->b_ih, ->b_hh) final;
 *   ENC:   the encoder convolutions (->conv[0..3]) final. */
#define DR_WM_BWD_HEADS 8
#define DR_WM_BWD_SCAN 16
#define DR_WM_BWD_ENC 32
int dr_wm_train_phase(const dr_dims* d, const dr_world_model* wm, const dr_decoder* dec, int B, int T,
                      const dr_frames* src, const dr_wm_batch* batch, dr_noise noise, dr_wm_loss_cfg cfg, int phases,
                      float* stats, int rows_global, float* losses, int* skip, const dr_world_model* g_wm,
                      const dr_decoder* g_dec, float* hiddens_out, float* latents_out, float* post_logits_out,
                      void* ws, size_t ws_bytes, hipStream_t stream);
int dr_wm_train_grads(const dr_dims* d, const dr_world_model* wm, const dr_decoder* dec, int B, int T,
                      const dr_frames* src, const dr_wm_batch* batch, dr_noise noise, dr_wm_loss_cfg cfg,
                      float* losses, int* skip, const dr_world_model* g_wm, const dr_decoder* g_dec,
                      float* hiddens_out, float* latents_out, float* post_logits_out, void* ws, size_t ws_bytes,
                      hipStream_t stream);

/* Per-window loss of the last DR_WM_FWD on this workspace (prioritised replay,
 * below): scores_out[b], b < B, over the window's first T steps, from the
 * per-row loss terms the forward left in the workspace (the backward stages
 * write none of them, so the call may follow a whole dr_wm_train_phase).  Rows
 * are time-major, i = (t-1) B + b; m_{b,t} is the mask of WorldModel.py:170:
 *   pred_b = sum_t m (sqerr - rew_ll + cont_bce) / (sum_t m + 1e-5)
 *   kl_b   = 1/(T-1) sum_t m sum_g KL_{b,t,g}
 *   L_b    = beta_pred pred_b + (beta_dyn + beta_rep) kl_b
 * The free-bit clamp max(1, KL) is left out on purpose: it would give every
 * window the same KL term once the batch mean is under one nat.  (d, B, T) and
 * the workspace are those of the step. */
int dr_wm_window_scores(const dr_dims* d, int B, int T, dr_wm_loss_cfg cfg, void* ws, size_t ws_bytes,
                        float* scores_out, hipStream_t stream);

/* ---- a20  Decoder.forward (VAE.py:139-161), inference: mu [M][3][H][W] (NCHW)
 * from cat(h, flatten z) rows (h row stride ldh, z row stride ldz). */
size_t dr_decoder_workspace_bytes(const dr_dims* d, int M);
int dr_decoder_fwd(const dr_dims* d, const dr_decoder* dec, int M, const float* h, long long ldh, const float* z,
                   long long ldz, float* mu, void* ws, size_t ws_bytes, hipStream_t stream);

/* ---- frame metrics: decoded frames against the true ones (the squared error
 *      of the reconstruction term, WorldModel.py:129, and the u8 frames a
 *      prediction video shows) -------------------------------------------------
 * mu [B][T][3][H][W] (pixel models) or [B][T][obs_dim] (vector observations),
 * as dr_decoder_fwd writes rows m = b*T + t.  `truth` has dr_frames semantics
 * (t0 included): its frame (b, t) -- the u8 ring + starts, or the f32 form --
 * is compared with mu[b][t].  The true value is x = (float)u8 / 255.0f - 0.5f
 * (Dreamer.py:251) for the u8 ring and for f32 frames with raw255; f32 frames
 * without raw255, and vector rows, are used as stored.
 *   sqerr[b][t]   = sum over the frame of (mu - x)^2
 *   pred_u8[b][t] = (u8) min(255, max(0, rintf((mu + 0.5f) * 255.0f))), may be NULL
 *   true_u8[b][t] = the true frame as u8 (the ring's bytes; an f32 source is
 *                   quantised like pred_u8), may be NULL
 * Vector observations have no u8 form: pred_u8 and true_u8 must be NULL
 * (DR_E_INVALID otherwise), obs_dim <= 1023.
 * One 256-thread workgroup per frame, no atomics: each thread sums its
 * elements in ascending order, then a fixed wave reduction and the four wave
 * sums in wave order -- sqerr of a frame is the same bits at every B, T and
 * position, and from run to run. */
int dr_frame_metrics(const dr_dims* d, int B, int T, const float* mu, const dr_frames* truth, float* sqerr,
                     unsigned char* pred_u8, unsigned char* true_u8, hipStream_t stream);

/* ---- sampled futures on replay windows (Dreamer.sample_futures): SSIM of
 *      decoded frames, and the mean and spread of M decoded futures.  No
 *      reference counterpart: the definitions are these. ------------------------
 * dr_frame_ssim: mu, truth and the frame indexing (t0 included) as
 * dr_frame_metrics.  Pixel observations only (obs_dim > 0: DR_E_INVALID).
 *   p = min(0.5f, max(-0.5f, mu)) the clamped prediction, x the true value as
 *   dr_frame_metrics defines it; both centred on 0 (data range 1).
 *   Window: the 11-tap Gaussian with sigma = 1.5, g_k = exp(-(k - 5)^2 / 4.5),
 *   normalised to sum 1 in double and rounded to f32 once (constant data),
 *   applied separably -- along W first, then along H, taps in ascending order --
 *   at the (H - 10) x (W - 10) valid positions only.
 *   Per channel and position, on the centred values:
 *     m_p = sum w p, m_x = sum w x, v_p = sum w p^2 - m_p^2, v_x = sum w x^2 - m_x^2,
 *     c = sum w p x - m_p m_x;  u_p = m_p + 0.5, u_x = m_x + 0.5 (luminance means)
 *     map = ((2 u_p u_x + C1)(2 c + C2)) / ((u_p^2 + u_x^2 + C1)(v_p + v_x + C2)),
 *     C1 = 1e-4, C2 = 9e-4
 *   ssim_ch[b][t][ch] = mean of the map over the channel's valid positions (may be NULL)
 *   ssim[b][t]        = ((ch0 + ch1) + ch2) / 3
 * img_h < 11 or img_w < 11: DR_E_UNSUPPORTED, nothing launched; every size from
 * 11 x 11 up to img_w <= 163 (any img_h) is served (wider rows do not fit the
 * kernel's 64 KiB of LDS: DR_E_UNSUPPORTED).
 * One 256-thread workgroup per frame, no atomics, nothing shared between
 * workgroups.  A thread adds the map at its positions (row-major position tid,
 * tid + 256, ... of each strip of rows, strips in ascending order) in ascending
 * order per channel, then a fixed wave reduction and the four wave sums in wave
 * order: a frame's results are the same bits at every B, T and position, and
 * from run to run.  A prediction bit-equal to the (in-range) truth gives 1.0f. */
int dr_frame_ssim(const dr_dims* d, int B, int T, const float* mu, const dr_frames* truth, float* ssim,
                  float* ssim_ch, hipStream_t stream);

/* dr_ensemble_metrics: M decoded futures per window, mu [B][M][T][n] with row
 * (b*M + m)*T + t as dr_decoder_fwd writes it for rollout rows b*M + m; n =
 * 3*H*W, or obs_dim for vector observations.  truth (b, t) as dr_frame_metrics.
 * Per element i, in f32:  mean_i = (sum_m mu_m,i) / M  (m ascending),
 * var_i = (sum_m (mu_m,i - mean_i)^2) / M  (a second pass: the population variance).
 *   sqerr_mean[b][t] = sum_i (mean_i - x_i)^2      the ensemble mean's error
 *   spread[b][t]     = sum_i var_i
 *   mean_u8[b][t]    = the mean frame quantised as pred_u8 is (may be NULL)
 *   std_u8[b][t]     = (u8) min(255, rintf(255.0f * sqrtf(var_i))) (may be NULL)
 *   mean_f32[b][t][n] = the mean frame (may be NULL; dr_frame_ssim takes it as mu)
 * mean_u8 and std_u8 must be NULL for vector observations (DR_E_INVALID).
 * 1 <= M <= 64, else DR_E_INVALID.  M = 1: spread is exactly 0 and sqerr_mean
 * is dr_frame_metrics' sqerr bit for bit (buffers of the same alignment).
 * One 256-thread workgroup per (b, t), dr_frame_metrics' element order and
 * reduction, no atomics: the same bits at every B, T and position, and from
 * run to run.  Per-sample squared errors are dr_frame_metrics on B*M rows
 * with starts repeated M times. */
int dr_ensemble_metrics(const dr_dims* d, int B, int M, int T, const float* mu, const dr_frames* truth,
                        float* sqerr_mean, float* spread, unsigned char* mean_u8, unsigned char* std_u8,
                        float* mean_f32, hipStream_t stream);

/* ---- latent statistics on raw logits [M][R][C] (no unimix, no free bits, no
 *      mask: the terms of the KL losses, WorldModel.py:175-181, per row) --------
 *   kl[m]            = sum_r KL(Cat(logits = post[m][r]) || Cat(logits = prior[m][r]))
 *                      (torch's _kl_categorical_categorical: sum p (lp - lq), p = exp(lp))
 *   post_entropy[m]  = sum_r H(softmax post[m][r]);  prior_entropy[m] likewise
 *   kl_groups[m][r]  = the R terms of kl[m], may be NULL
 * prior_logits may be NULL: then only post_entropy is written, and kl,
 * prior_entropy (and kl_groups) must be NULL.  Domain as dr_categorical_sample:
 * 1 <= C <= 64, R >= 1, M >= 0, else DR_E_INVALID.  Max-subtracted
 * log-sum-exp; a class whose probability underflows to 0 adds exactly 0.  One
 * workgroup per row and a fixed reduction order, no atomics: a row has the same
 * bits at every M and position, and from run to run. */
int dr_latent_stats(int M, int R, int C, const float* post_logits, const float* prior_logits, float* kl,
                    float* post_entropy, float* prior_entropy, float* kl_groups, hipStream_t stream);

/* ---- agent trace on replay windows: what the actor and the critic make of
 *      real data (Dreamer.agent_trace).  Slot t of a window holds the frame x_t,
 *      the action a_t taken on seeing x_t and the symlog reward / continue flag
 *      of that transition (rollout_policy, Dreamer.py:212); state t + 1's heads
 *      are compared with slot t (unroll_model, WorldModel.py:113-123).
 *      Three one-shot kernels without atomics: a row (a window, for the
 *      returns) has the same bits at every batch size and position, and from
 *      run to run.  M = 0 rows is a no-op; bad dimensions and missing pointers
 *      give DR_E_INVALID before any launch. ---------------------------------- */
/* compute_batched_R_lambda_returns (Agent.py:156-172) with H = T - 1 on real
 * rewards and continues and the values V [B][T] of the T filtered states:
 *   R_lambda[b][t] = r_t + gamma c_t ((1 - lam) V_{t+1} + lam R_lambda[b][t+1]),
 *   R_lambda[b][T-2] = r_{T-2} + gamma c_{T-2} V_{T-1}
 *   R_mc[b][t]: the same at lam = 1, the discounted real return bootstrapped
 *               once at the window's end (may be NULL)
 *   td[b][t]  = (r_t + gamma c_t V_{t+1}) - V_t (may be NULL)
 * rewards / continues: window rows with strides rew_sb / cont_sb >= T - 1 (the
 * [B][S] arrays dr_replay_gather writes), entries 0 .. T-2 read; outputs
 * [B][T-1].  rewards_symlog != 0: the stored reward is in symlog space and goes
 * through symexp with its clamp (DreamerUtils.py:35-37) first.  c = 0 cuts the
 * recursion as in the reference.  One thread per window, dr_lambda_returns'
 * expressions in its order (1 - lam formed in double, rounded once): with
 * rewards_symlog = 0 R_lambda is bit for bit dr_lambda_returns(B, T - 1, ...),
 * and for finite V R_mc is bit for bit dr_lambda_returns(..., lam = 1).
 * B >= 0, T >= 2. */
int dr_replay_returns(int B, int T, const float* rewards, long long rew_sb, const float* continues,
                      long long cont_sb, int rewards_symlog, const float* V, float gamma, float lam,
                      float* R_lambda, float* R_mc, float* td, hipStream_t stream);
/* Per-row statistics of a bucket head's logits (Critic.forward, Agent.py:231-235):
 * rows m = b*T + t of `logits`, row stride ldl >= nb.
 *   entropy[b][t]    = H(softmax l)                              (may be NULL)
 *   std_symlog[b][t] = sqrt(sum p (bucket - sum p bucket)^2), in bucket (symlog)
 *                      units, in two passes                      (may be NULL)
 *   ce[b][t], t < Tt = -sum twohot(symlog(target[b][t])) log_softmax(l)
 *                      (Agent.py:127-135; to_twohot of DreamerUtils.py:39-50 with
 *                      its clamps and the 1e-8; symlog and the two weights are
 *                      formed in double, the log-probabilities in f32)
 * target (natural-space returns) and ce are [B][Tt], 0 <= Tt <= T: row (b, t) has
 * a target iff t < Tt (dr_critic_loss_bwd's row convention, so [B][T-1] returns
 * go in unpadded).  The two are both given (Tt > 0) or both NULL (Tt = 0); at
 * least one output is required.  2 <= nb <= 1024; buckets [nb] must be ascending
 * (not checked).  One wave per row: lane-strided terms in ascending order, then
 * a fixed wave tree; max-subtracted log-sum-exp, a class whose probability
 * underflows adds exactly 0. */
int dr_value_stats(int B, int T, int Tt, int nb, const float* logits, long long ldl, const float* buckets,
                   const float* target, float* entropy, float* std_symlog, float* ce, hipStream_t stream);
/* log-probability of recorded actions under a tanh-Normal policy (Agent.py:110-115):
 * mu, sigma [B][T][A] (Actor.forward, Agent.py:191-200); action element
 * (b, t, i) at actions[b*act_sb + t*act_st + i], as in dr_observe_trace.  Per
 * dimension, with y = clamp(a, -1 + 1e-6, 1 - 1e-6) in f32 and x = atanh(y):
 *   -(x - mu)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi) - 2 (log 2 - x - softplus(-2x))
 *   logp[b][t]         = the sum of the A terms, in ascending order from 0
 *   logp_dims[b][t][i] = the terms                                (may be NULL)
 *   base_entropy[b][t] = sum_i (1/2 + 1/2 log(2 pi) + log sigma_i) (may be NULL)
 * An action of exactly +-1 gives a finite value.  One thread per row.  A >= 1,
 * T >= 1, B >= 0. */
int dr_action_logprob(int B, int T, int A, const float* mu, const float* sigma, const float* actions,
                      long long act_sb, long long act_st, float* logp, float* logp_dims, float* base_entropy,
                      hipStream_t stream);

/* ---- dream trace: imagined rollouts under the actor from replay windows
 *      (Dreamer.dream_trace, dreamer_amd/dream_trace.py): what train_Agent learns
 *      from (Dreamer.py:143-175, Agent.py:96-135), per dream and per window.
 * N = B*M rows; row n = b*M + m is dream m of window b.  Inputs: rewards,
 * continues [N][H] as dr_imagine_fwd writes them (natural-space reward,
 * continue probability); V_target, V_online [N][H+1], dr_critic_fwd's values of
 * the H+1 states; mus, sigmas, actions [N][H][A]; norm: a device scalar holding
 * max(S, 1) (Agent.py:78-88), read and never written, NULL = 1.
 * Per dream (every output may be NULL; at least one output in all is required):
 *   R_lambda[n][t]  = r_t + gamma c_t ((1 - lam) Vt_{t+1} + lam R_lambda[n][t+1]),
 *                     R_lambda[n][H-1] = r_{H-1} + gamma c_{H-1} Vt_H (Agent.py:156-172):
 *                     bit for bit dr_lambda_returns(N, H, ...) -- its expressions
 *                     in its order, 1 - lam formed in double and rounded once
 *   R_mc[n][t]      = the same at lam = 1; for finite V bit for bit
 *                     dr_lambda_returns(..., lam = 1) (dr_replay_returns' convention)
 *   adv[n][t]       = R_lambda[n][t] - V_online[n][t];  adv_norm = adv / norm
 *                     (Agent.py:105-121)
 *   weight[n][t]    [N][H+1]: w_0 = 1, w_{t+1} = w_t * (gamma * c_t) in f32, t
 *                     ascending; entry H weighs the bootstrap value
 *   logp[n][t], base_entropy[n][t]: bit for bit dr_action_logprob's on the same
 *                     mus, sigmas and actions
 *   saturated[n][t] int32: the number of dimensions i with |a_i| >= sat
 * Per window over its M dreams, f32, m ascending from 0.0f; a mean is sum / M,
 * a std sqrt((sum_m (x_m - mean)^2) / M) in a second pass (population):
 *   reward_mean, reward_std [B][H]   of rewards
 *   ret_mean, ret_std       [B][H]   of R_lambda
 *   logp_mean, logp_std     [B][H]   of logp
 *   alive                   [B][H+1] the mean of weight
 *   action_spread           [B][H]   sqrt((sum_i var_m(a_i)) / A), i ascending
 *   best, worst, n_finite   [B] int32: the dream with the largest / smallest
 *                     R_mc[.][0] among those where it is finite, ties to the lower
 *                     m; n_finite counts those dreams, 0 of them: best = worst = 0
 * Non-finite inputs propagate into the per-dream outputs and into the means and
 * stds of their (b, t); they never make a dream best or worst.
 * One launch, one 256-thread workgroup per window, no atomics: a window's
 * outputs are the same bits at every B and position, with any subset of the
 * outputs asked for, and from run to run.  The window's R_lambda, logp and
 * weight rows sit in LDS: M <= DR_DREAM_STATS_MAX_DREAMS (dr_ensemble_metrics' 64) and
 *   (M | 1) * (3 H + 2) <= DR_DREAM_STATS_MAX_LDS_FLOATS   (M = 64: H <= 78)
 * else DR_E_UNSUPPORTED.  M, H, A >= 1, B >= 0 (B = 0 is a no-op); bad dimensions,
 * a missing input or no output: DR_E_INVALID before any launch. */
#define DR_DREAM_STATS_MAX_DREAMS 64
#define DR_DREAM_STATS_MAX_LDS_FLOATS 15360
typedef struct {
  float *R_lambda, *R_mc, *adv, *adv_norm, *weight, *logp, *base_entropy;
  int* saturated;
  float *reward_mean, *reward_std, *ret_mean, *ret_std, *logp_mean, *logp_std, *alive, *action_spread;
  int *best, *worst, *n_finite;
} dr_dream_outputs;
int dr_dream_stats(int B, int M, int H, int A, const float* rewards, const float* continues,
                   const float* V_target, const float* V_online, const float* mus, const float* sigmas,
                   const float* actions, float gamma, float lam, const float* norm, float sat,
                   const dr_dream_outputs* out, hipStream_t stream);
/* eps[s][row][i], s < steps, row < rows, i < A: the N(0,1) Philox variate of
 * (noise.stream + s, noise.row0 + row, i) -- what dr_imagine_fwd's actor draws at
 * step s -- written out, so that a call can pair them with explicit categorical
 * draws (dream_trace's sample=False). */
int dr_actor_draws(int steps, int rows, int A, dr_noise noise, float* eps, hipStream_t stream);

/* ---- perturbation saliency (Dreamer.saliency, dreamer_amd/saliency.py;
 *      Greydanus et al. 2018, "Visualizing and Understanding Atari Agents"):
 *      blend a blurred copy of the frame into one small region, run the agent
 *      again, score how far its outputs moved; repeated over a grid of regions.
 *      No reference counterpart: the definitions are these.  Pixel models only
 *      (obs_dim > 0: DR_E_UNSUPPORTED). ------------------------------------------
 * Grid: stride s with H % s == 0 and W % s == 0; Gy = H / s, Gx = W / s, G = Gy Gx
 * <= 1024.  Cell (i, j) has the integer centre cy = i s + s / 2, cx = j s + s / 2
 * (integer division).  Variant 0 of a frame is the frame itself, variant
 * 1 + i Gx + j is perturbed at cell (i, j).
 * Tables, made on the host in double, rounded to f32 and passed as device
 * arrays (the kernels call no expf):
 *   wb[0 .. 2 rb]            blur taps exp(-k^2 / (2 sigma_b^2)), k = -rb .. rb, normalised
 *                            to sum 1; rb = ceil(3 sigma_b) <= 15
 *   gm[0 .. max(H, W) - 1]   mask profile exp(-k^2 / (2 sigma_m^2))
 * Fill A, f32 per channel:
 *   fill = 0 (blur)  Hh[c][y][x] = sum_k wb[k + rb] I[c][y][clamp(x + k, 0, W - 1)], then the
 *                    same over y on Hh; each sum an explicit fmaf(w, v, acc) chain
 *                    from acc = 0.0f in ascending k
 *   fill = 1 (mean)  A[c] = (float)(exact integer sum of channel c) / (float)(H W)
 * Perturbed pixel: m = gm[|y - cy|] * gm[|x - cx|] (one f32 multiply),
 *   v = fmaf(m, A - I, I) with A - I one f32 subtraction,
 *   out = (u8) min(255, max(0, rintf(v))).
 *
 * dr_occlude_frames: src is a u8 ring source (dr_frames); frame f of the call is
 * src's frame (b = f, t = 0), t0 honoured -- a plain u8 array of N frames is a
 * ring with ring_cap = N and starts = 0 .. N-1.  out u8 [F][G+1][3][H][W].
 * Two stages: the fill into the workspace (blur: row strips through LDS; mean:
 * one workgroup per channel), then the blend -- a thread keeps I and A - I of
 * its 16 pixels in registers, loops over 32 variants of its frame and writes 16
 * bytes per store, so A is read once per workgroup; a width that is no multiple
 * of 16 (or a base that is not 16-byte aligned) takes a one-pixel-per-thread
 * path with the same arithmetic.
 * DR_E_INVALID, nothing launched: rb > 15, G > 1024, a stride that does not
 * divide the frame, a NULL table (wb is not read with fill = 1 and may be NULL
 * then).  DR_E_UNSUPPORTED, nothing launched: a src in f32 form, vector
 * observations, rows so wide that the blur's strip ((8 + 2 rb) rows of W floats)
 * does not fit 64 KiB of LDS.  F <= 65535.
 * Asynchronous, capturable, no atomics; a frame's variants are the same bits at
 * every F and position, and from run to run. */
size_t dr_occlude_workspace_bytes(const dr_dims* d, int F);
int dr_occlude_frames(const dr_dims* d, const dr_frames* src, int F, int s, int fill, const float* wb, int rb,
                      const float* gm, unsigned char* out, void* ws, size_t ws_bytes, hipStream_t stream);
/* Scores of variant g >= 1 of frame f against variant 0 of the same frame; rows
 * f (G + 1) + g of mu [.][A] (Actor.forward's mean), V [.] (critic.value), logits
 * and z [.][R*C] (the posterior's raw logits and its straight-through sample).
 * Outputs [F][G], entry g - 1, any of them may be NULL (then its input may be too):
 *   actor        = 1/2 sum_i (mu_g,i - mu_0,i)^2
 *   value_delta  = V_g - V_0 (one f32 subtraction);  value = 1/2 value_delta^2
 *   posterior_kl = sum_r KL(Cat(logits_0,r) || Cat(logits_g,r)) on raw logits as
 *                  dr_latent_stats defines kl: max-subtracted log-sum-exp,
 *                  lp = (x - max) - log(sum), a class whose p underflows adds 0
 *   latent_flips = the number of the R categoricals whose selected class (the
 *                  lowest index holding the maximum of z's group) differs, int32
 * One 256-thread workgroup per (f, g).  actor: a thread takes the elements tid,
 * tid + 256, ... in ascending order.  posterior_kl and latent_flips (C <= 64,
 * else DR_E_INVALID): a categorical takes W lanes, W the power of two >= C, one
 * class per lane and fixed trees inside the group as in dr_latent_stats; the
 * group's first lane adds its categoricals in ascending order.  Then
 * dr_frame_metrics' wave reduction and the four wave sums in wave order: the
 * same bits at every F and position and from run to run.  Identical rows give
 * exactly 0 everywhere. */
int dr_saliency_scores(int F, int G, int A, int R, int C, const float* mu, const float* V, const float* logits,
                       const float* z, float* actor, float* value, float* value_delta, float* posterior_kl,
                       int* latent_flips, hipStream_t stream);
/* Heat map of a score grid, scores [F][Gy][Gx], scale [F].  For pixel (y, x):
 *   fy = min(max(((float)(y - s/2)) / (float)s, 0), Gy - 1), i0 = floor(fy),
 *   i1 = min(i0 + 1, Gy - 1), wy = fy - i0; the same in x;
 *   map[f][y][x] = scale[f] * ((((1-wy)(1-wx)) S[i0][j0] + ((1-wy) wx) S[i0][j1])
 *                              + (wy (1-wx)) S[i1][j0]) + (wy wx) S[i1][j1])
 *   in f32, products and sums as written, no contraction: a cell's centre pixel
 *   gives scale[f] * S[i][j] exactly.
 * overlay u8 [F][3][H][W] (may be NULL; `frames`, a u8 ring source read as
 * dr_occlude_frames reads src, is needed only with it): heat = min(1, max(0, map)),
 * channel ch becomes (u8) rintf(fmaf(heat, 255 - I, I)), the others are copied.
 * One thread per pixel. */
int dr_saliency_map(const dr_dims* d, int F, int s, const float* scores, const float* scale,
                    const dr_frames* frames, int ch, float* map, unsigned char* overlay, hipStream_t stream);
/* q[row][c], row < rows, c < C: the Exp(1) Philox variate of (noise.stream,
 * noise.row0 + row, c), written out so that every variant of a frame can be
 * given its frame's draws as explicit noise (common random numbers). */
int dr_saliency_draws(int rows, int C, dr_noise noise, float* q, hipStream_t stream);

/* ---- latent planning: CEM / MPPI action search over world-model rollouts ----
 * (dreamer_amd/plan.py, Dreamer.plan; no reference counterpart: the reference's
 * only controller is the actor's forward pass, Dreamer.py:295-322.)
 *
 * E >= 1 environments, each with a belief state (h_e, z_e); horizon H >= 1; N
 * candidate action sequences per environment, the first N_pi >= 0 of them the
 * actor's; 1 <= K <= N elites; J >= 1 iterations.  Per environment the search
 * keeps mean[H][A] and std[H][A].  One iteration:
 *  1. sample   candidate (e, n): for n < N_pi the n-th actor sequence, else
 *              a[k][i] = clamp(mean[k][i] + std[k][i] * eps, -1, 1) in f32 (one
 *              multiply, one add, no contraction)                [dr_plan_sample]
 *  2. roll out the E*N rows from the replicated (h_e, z_e): r_k, c_k [E*N][H],
 *              entry k-1 on state k                          [dr_imagine_actions]
 *  3. bootstrap V_H = the critic's value of state H of every row, read with the
 *              row stride (H+1)*width from the rollout's arrays (or V_H = 0)
 *                                                                 [dr_critic_fwd]
 *  4. score    G = R_0, R_H = V_H, R_k = r_{k+1} + (gamma c_{k+1}) R_{k+1}:
 *              k_lambda_returns' expressions at lam = 1 in its order, the
 *              intermediate values it multiplies by 1 - lam = 0 taken as +0.  For
 *              finite V with column H = V_H, G is bit for bit column 0 of
 *              dr_lambda_returns(E*N, H, r, c, V, gamma, 1)
 *  5. rank     within an environment by score descending, ties by the lower
 *              candidate index.  A non-finite score (NaN, +-Inf) ranks after
 *              every finite one and is never an elite: K' = min(K, number of
 *              finite scores) elites
 *  6. weights  in rank order j = 0..K'-1: w_j = 1 when temperature = 0 (CEM),
 *              else w_j = exp((G_j - G_0) / temperature) (MPPI);  W = sum w_j,
 *              added in rank order from 0.0f
 *  7. refit    per element (k, i), sequentially in rank order, in f32:
 *              m = (sum w_j a_j) / W;  s = sqrt((sum w_j (a_j - m)^2) / W) in a
 *              second pass, then min(max(s, std_min), std_max);
 *              mean <- momentum * mean + (1 - momentum) * m  (1 - momentum formed
 *              in f32);  std <- s.  K' = 0: mean and std keep their bits.
 * Steps 4 to 7 are dr_plan_update.  After J iterations the action is the final
 * mean's first step.
 *
 * Both entry points are one-shot launches (nothing shared between workgroups,
 * no atomics, no waits); an environment's outputs are the same bits at every E
 * and position in the batch and from run to run.  E = 0 is a no-op.  Bad
 * dimensions or missing pointers: DR_E_INVALID before any launch; N >
 * DR_PLAN_MAX_CANDIDATES (one environment's scores, elite indices and weights
 * sit in LDS) or H * A > DR_PLAN_MAX_ELEMS: DR_E_UNSUPPORTED.
 *
 * dr_plan_sample: mean, std [E][H][A]; policy_actions [E][N_pi][H][A], NULL
 * exactly when N_pi = 0; actions [E][N][H][A] (out).  Explicit noise: noise.eps
 * [E][N][H*A], read only for n >= N_pi (noise.q is not used); otherwise Philox:
 * dr_normal on noise.stream, row (noise.row0 + e) * N + n, element k * A + i.
 * One thread per element.
 *
 * dr_plan_update: rewards, continues [E*N][H]; v_last [E*N] or NULL (V_H = 0);
 * actions [E][N][H][A]; mean, std [E][H][A] (in/out).  Outputs: scores [E][N]
 * (the raw value, non-finite included), elite_idx [E][K] in rank order (-1 past
 * K'), elite_w [E][K] (w_j / W, 0 past K'), n_elite [E] (K').  Needs
 * temperature >= 0, 0 <= momentum < 1, 0 <= std_min <= std_max.  One 256-thread
 * workgroup per environment; ranks by counting in LDS. */
#define DR_PLAN_MAX_CANDIDATES 2048
#define DR_PLAN_MAX_ELEMS 1024
int dr_plan_sample(int E, int N, int N_pi, int H, int A, const float* mean, const float* std,
                   const float* policy_actions, dr_noise noise, float* actions, hipStream_t stream);
int dr_plan_update(int E, int N, int H, int A, int K, const float* rewards, const float* continues,
                   const float* v_last, float gamma, float temperature, float momentum, float std_min,
                   float std_max, const float* actions, float* mean, float* std, float* scores, int* elite_idx,
                   float* elite_w, int* n_elite, hipStream_t stream);

/* ---- a1  replay gather (Buffer.sample_sequences, Buffer.py:49-61) --------- */
int dr_replay_gather(long long cap, int B, int S, int frame_elems, int A, const unsigned char* frames,
                     const float* actions, const float* rewards, const float* continues,
                     const long long* starts, float* obs_out, float* act_out, float* rew_out,
                     float* cont_out, hipStream_t stream);

/* ---- prioritised ("curious") replay: window sampling on the device ---------
 * (Curious Replay, Kauvar et al. 2023.)  One priority and one visit count per
 * ring slot; slot i stands for the window that starts at i.  priority is f32
 * [cap], visits i32 [cap], both on the device beside the ring mirror.
 *
 * Valid starts: validity is the reference's (Buffer.py:33-48) with the
 * straddle made exact instead of "one redraw".  Slot i is a valid start iff
 *   0 <= i < size - S + 1 (S = sequence_length), and
 *   not (size == cap and i < next_idx < i + S).
 * Weight: w_i = priority[i] if i is valid, else 0; a stored priority that is
 * non-finite or <= 0 counts as p_floor (= eps^alpha), so the total W is
 * positive whenever a valid start exists.
 * Draw: for a uniform u in [0, 1) the start is the least valid i with
 * C_i > u W, C_i the inclusive running sum of w in slot order; if rounding
 * leaves u W >= C_last, the last valid slot.  A draw never returns an invalid
 * slot.  prob[b] = w_i / W.  Sums are float64 in a fixed order (priorities
 * span 1e5 .. 4e-2 over up to 1e6 slots: an f32 running sum would make
 * low-priority windows unreachable), so the same inputs give the same bits.
 * Philox uniforms are 53-bit doubles from two words keyed (seed, offset,
 * stream_id, row b).
 * Priority update after a step on starts s_b with scores L_b:
 *   visits[s] += number of rows b with s_b = s
 *   priority[s] = c beta^visits[s] + (max_b |L_b| + eps)^alpha
 * (the maximum over the rows with s_b = s, visits[s] the updated count); a
 * non-finite score among them gives priority[s] = p_new.  The result does not
 * depend on the order of the rows and is bitwise repeatable (no float
 * atomics: the first row that holds a start writes its slot).  A start outside
 * [0, cap) is ignored.
 * Every call is asynchronous on `stream` and capturable; the caller owns the
 * memory.  priority must be 16-byte aligned; cap <= 2^30. */
size_t dr_replay_sample_workspace_bytes(long long cap);
/* u: the uniforms [B] (parity, tests) or NULL: Philox on rng = the device
 * {seed, offset} pair.  starts_out int64 [B]; prob_out f32 [B] or NULL.  Two
 * stages: the masked sums of 1024-slot chunks into ws (the whole ring is
 * re-summed on every call: the mask depends on size and next_idx), then one
 * workgroup per draw. */
int dr_replay_sample(long long cap, long long size, long long next_idx, int S, int B, const float* priority,
                     double p_floor, const double* u, const unsigned long long* rng, int stream_id,
                     long long* starts_out, float* prob_out, void* ws, size_t ws_bytes, hipStream_t stream);
/* prob_out[i] = w_i / W for every slot i < cap (the same first stage and W). */
int dr_replay_probabilities(long long cap, long long size, long long next_idx, int S, const float* priority,
                            double p_floor, float* prob_out, void* ws, size_t ws_bytes, hipStream_t stream);
int dr_replay_priority_update(long long cap, int B, const long long* starts, const float* scores, double c,
                              double beta, double alpha, double eps, double p_new, float* priority, int* visits,
                              hipStream_t stream);

/* ---- episode-aware replay: only windows inside one stream are drawn --------
 * (config key replay_episodes = "respect", DESIGN.md 5q.  No reference
 * definition: the reference's windows run across the end of an episode.)
 * Per-slot inputs, on the device beside the ring mirror: continues f32 [cap]
 * (what the ring stores) and first u8 [cap]; first[j] != 0 says that slot j
 * begins a new stream (a new episode, or a block of another environment).
 * Stops: slot j is a stop iff any of
 *   !(continues[j] >= 0.5f)              (a NaN is therefore a stop),
 *   j + 1 < cap and first[j + 1] != 0,
 *   j == cap - 1                         (windows never wrap the physical end),
 *   j is the newest written slot: size - 1 when size < cap, else
 *                                        (next_idx - 1 + cap) % cap.
 * Span: span[i] = 0 for i >= size; otherwise span[i] = j* - i + 1 with j* the
 * least stop >= i.  Slot i is a valid start iff span[i] >= S.  A window may
 * end on a terminal step (the continue head still sees terminals) and never
 * holds one before its last position.  Where the data has no break,
 * span[i] >= S is exactly the valid-start rule of prioritised replay above;
 * with breaks it is a subset of it.  span is an integer suffix minimum over
 * stop indices: no order of evaluation changes it.
 * dr_replay_spans writes span_out int32 [cap] and, if n_valid_out (a device
 * int64) is given, the number of slots with span >= S, a fixed-order integer
 * sum.  first may be NULL (all 0).  Three plain launches (the least stop of
 * each 1024-slot chunk; the suffix minimum over those and inside the chunk;
 * the count), capturable, no host sync, no allocation.  continues and
 * span_out must be 16-byte aligned, first 4-byte aligned; cap <= 2^30. */
size_t dr_replay_spans_workspace_bytes(long long cap);
int dr_replay_spans(long long cap, long long size, long long next_idx, const float* continues,
                    const unsigned char* first, int S, int* span_out, long long* n_valid_out, void* ws,
                    size_t ws_bytes, hipStream_t stream);
/* dr_replay_sample / dr_replay_probabilities with the valid starts taken from
 * span (int32 [cap], 16-byte aligned): w_i = priority[i] (floored as above) if
 * span[i] >= S, else 0.  priority may be NULL: every valid start weighs 1.0,
 * the float64 sums are then exact integers and the start is exactly the least
 * valid i with C_i > u n (n the number of valid starts), with no rounding
 * margin; prob = 1 / n.  A draw never returns a slot with span < S; where no
 * slot is valid the draw answers start 0, prob 0 (the host refuses first).
 * Same workspace as dr_replay_sample. */
int dr_replay_sample_spans(long long cap, long long size, long long next_idx, int S, int B, const float* priority,
                           double p_floor, const int* span, const double* u, const unsigned long long* rng,
                           int stream_id, long long* starts_out, float* prob_out, void* ws, size_t ws_bytes,
                           hipStream_t stream);
int dr_replay_probabilities_spans(long long cap, long long size, long long next_idx, int S, const float* priority,
                                  double p_floor, const int* span, float* prob_out, void* ws, size_t ws_bytes,
                                  hipStream_t stream);

/* ---- latent-disagreement ensemble (Plan2Explore, Sekar et al. 2020, in the
 *      form of DreamerV3's expl.Disag; config key explore = "disagreement",
 *      DESIGN.md 5o).  No reference definition: the reference learns from the
 *      environment's reward alone.
 * K members, each a dr_mlp3 Linear(Hd -> W) LN SiLU Linear(W -> W) LN SiLU
 * Linear(W -> L) on a hidden state h alone; L = rows * cols.  Always f32, in
 * both precision modes.  The members' l0 parameters are contiguous:
 *   m[k].l0.w = m[0].l0.w + k W Hd,  m[k].l0.b = m[0].l0.b + k W
 * (the first layer of all members is one product with N = K W); the same holds
 * for a gradient dr_ensemble.  Checked; DR_E_INVALID otherwise.
 * Predictions p_k = m[k](h) [M][L].  Disagreement of a row:
 *   mu_j = (1/K) sum_k p_kj,  d = (1/L) sum_j sqrt((1/K) sum_k (p_kj - mu_j)^2)
 * (population std over the members, mean over the columns).  The deviations are
 * taken from member 0 (dev_k = p_kj - p_0j, minus their mean), scaled by a
 * power of two before they are squared: d is exactly 0 where the members agree
 * (for every K, and for K = 1), never negative, does not lose small or large
 * magnitudes to the squares, and a NaN / Inf prediction makes its row's d
 * non-finite and no other row's.  One wave per row, columns lane-strided in
 * ascending order, a fixed wave tree: the same bits on every run.
 * Loss (training): loss_k = mean over rows and columns of (p_k - z)^2,
 * loss = mean_k loss_k; dL/dp_k = 2 (p_k - z) / (K M L) (exactly 0 where
 * p_k == z).  Sums in a fixed order, no float atomics. */
#define DR_DISAG_MAX_MEMBERS 16
typedef struct {
  int K, W;                          /* members (1 .. 16), width of both hidden layers */
  dr_mlp3 m[DR_DISAG_MAX_MEMBERS];   /* m[k], k < K */
} dr_ensemble;
/* train = 0: dr_disag_fwd's scratch; 1: dr_disag_train_grads'. */
size_t dr_disag_workspace_bytes(int K, int W, int Hd, int L, int M, int train);
/* h [M] rows of Hd floats, ldh apart.  pred_out [K][M][L] and disag_out [M]
 * may be NULL.  Reward update (rew may be NULL): for row m with b = m / rew_T,
 * t = m % rew_T and t >= rew_skip,
 *   rew[b rew_sb + (t - rew_skip) rew_st] = w_ext * rew[..] + w_int * d_m
 * in place (two products and one sum, each rounded); rew_T = 0: every row m
 * updates rew[m rew_st].  The engine passes its hiddens [B][H+1][Hd] with
 * rew_T = H + 1, rew_skip = 1 and its rewards [B][H]: rewards[b][t] is the
 * reward head's value on hiddens[b][t+1] (dr_imagine_fwd).  Plain launches on
 * `stream` (the shared first layer, 2 ceil(K / 4) grouped products, the row
 * kernel), capturable. */
int dr_disag_fwd(const dr_ensemble* e, int Hd, int L, int M, const float* h, long long ldh, float* pred_out,
                 float* disag_out, float* rew, int rew_T, int rew_skip, long long rew_sb, long long rew_st,
                 float w_ext, float w_int, void* ws, size_t ws_bytes, hipStream_t stream);
/* Forward on M rows of h, the loss against z (rows of L floats, ldz apart; the
 * posterior samples as 0/1 floats) and the gradient of every weight, bias and
 * LayerNorm parameter into g (overwritten; no input gradient exists).
 * losses [1 + K]: the total, then loss_k. */
int dr_disag_train_grads(const dr_ensemble* e, int Hd, int L, int M, const float* h, long long ldh, const float* z,
                         long long ldz, const dr_ensemble* g, float* losses, void* ws, size_t ws_bytes,
                         hipStream_t stream);

/* ---- k-nearest-neighbour search and the particle-entropy reward (APT, Liu &
 *      Abbeel 2021; config key explore = "entropy").  No
 *      reference definition.
 * Inputs.  Queries x_m: Mq rows of D floats, ldq apart.  Bank y_j: Nb rows,
 * ldb apart.  Optional int32 group ids qg[Mq], bg[Nb] (either may be NULL).
 * Eligibility.  Bank row j is eligible for query m iff every one of its D
 * values is finite, and it is not the case that both group arrays are given
 * and bg[j] == qg[m].  Groups are the only exclusion mechanism: self-exclusion
 * is "group = row index", excluding a whole dream is "group = row / (H + 1)".
 * Selection.  Per query the k eligible bank rows of smallest squared Euclidean
 * distance, in ascending (distance^2, index) order, into d2_out [Mq][k] (f32)
 * and idx_out [Mq][k] (int32); 1 <= k <= DR_KNN_MAX_K.  With fewer than k
 * eligible rows the remaining slots hold +inf and -1.  A query row with a
 * non-finite value gets NaN and -1 in all of its slots; no other row is
 * affected by it.
 * Two-stage precision.  The selection uses the Gram form |x|^2 + |y|^2 - 2 x.y,
 * clamped at 0, on the exact-f32 MFMA; the norms are the same k-ascending fmaf
 * chain as the dot product, so two bit-identical rows get exactly 0, and on
 * operands whose products and sums are exact in f32 the selection is the exact
 * one.  The reported d2_out values are recomputed for the k chosen indices in
 * the direct form sum (x - y)^2 (columns lane-strided in ascending order, a
 * fixed wave tree, no atomics): they carry the direct form's relative error,
 * not the Gram form's cancellation error, and the final order is by the
 * recomputed value, then the index.  The distance of a pair, in either form,
 * is a function of that pair's two rows and D only, not of Mq, Nb, the tile
 * position or the bank split: a query's output is the same bits whatever else
 * is in the batch, and on every run.  Rows whose squared norm overflows f32
 * are outside the contract.
 * Entropy reward.  d_m = (1 / k_m) sum_n sqrt(d2_out[m][n]) over the
 * k_m = min(k, eligible) filled slots, e_m = log1p(d_m) (APT's log(c + .) with
 * c = 1); k_m = 0 gives e_m = 0; a non-finite query row gives a non-finite e_m
 * for that row alone; e_m is exactly 0 when all of the row's neighbours are
 * bit-identical to it.
 * Launches: the tile kernel (grid = query tiles x bank splits; the split count
 * is a function of (Mq, Nb) alone), the merge / recompute kernel, and for the
 * reward the row kernel; plain launches on `stream`, capturable, no host
 * synchronisation, no allocation, no process-wide state. */
#define DR_KNN_MAX_K 32
size_t dr_knn_workspace_bytes(int Mq, int Nb, int D, int k);
int dr_knn(int D, int k, int Mq, const float* q, long long ldq, const int* qg, int Nb, const float* bank,
           long long ldb, const int* bg, float* d2_out, int* idx_out, void* ws, size_t ws_bytes, hipStream_t stream);
/* d2_out, idx_out, ent_out [Mq] and rew may be NULL (not all four).  The reward
 * update is dr_disag_fwd's with e_m in the place of d_m:
 *   rew[b rew_sb + (t - rew_skip) rew_st] = w_ext * rew[..] + w_int * e_m
 * for b = m / rew_T, t = m % rew_T >= rew_skip (two products and one sum, each
 * rounded); rew_T = 0: every row m updates rew[m rew_st].  Workspace:
 * dr_knn_workspace_bytes. */
int dr_state_entropy_fwd(int D, int k, int Mq, const float* q, long long ldq, const int* qg, int Nb, const float* bank,
                         long long ldb, const int* bg, float* d2_out, int* idx_out, float* ent_out, float* rew,
                         int rew_T, int rew_skip, long long rew_sb, long long rew_st, float w_ext, float w_int,
                         void* ws, size_t ws_bytes, hipStream_t stream);

/* Which parts of a train_Agent epoch (Dreamer.py:264-287) run as ONE persistent
 * launch for these dims and shapes (the stream's CU mask aside): bit 0 the warm
 * start's posterior scan over T steps (Dreamer.py:255-261), bit 1 the
 * imagination unroll (Dreamer.py:158-164), bit 2 its BPTT (Agent.py:141-145
 * backward).  0 when dims->launch_form is set. */
int dr_persistent_kernels(const dr_dims* d, int B, int T, int H);

/* Philox offset bump (keeps graph replays drawing fresh noise) */
int dr_rng_advance(unsigned long long* rng, unsigned long long delta, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
