/*
 * ganffn.h — C ABI of libganffn.so: the MI355X (gfx950) implementation of GAN-FFN's
 * tri-modal generator/discriminator training step.
 *
 * The reference has no FFI: its seam is the Python nn.Module API of model.py as
 * consumed by train_IEMOCAP.py.  Every entry point below states the
 * reference code it replaces (file:line under /root/reference).  The Python side
 * (gan_ffn_amd/model.py, gan_ffn_amd/engine.py) binds these with ctypes and keeps the
 * reference's class names, constructor/forward signatures and state_dict layout.
 *
 * Conventions
 *  - All tensors are fp32, row-major, DEVICE pointers (hipMalloc'ed by the caller — in
 *    practice torch's caching allocator).  Activations are [T x C] with T = S*B tokens,
 *    token t = s*B + b, i.e. exactly the memory of the reference's (S, B, C) tensors
 *    (train_IEMOCAP.py:142-147).
 *  - The caller owns EVERY buffer (inputs, outputs, saved-for-backward, workspace,
 *    parameter/gradient/optimizer-state slabs).  The library allocates nothing, creates no
 *    streams or events, and keeps no mutable state between calls except caches that do not
 *    affect results — the thread-local last-error string and, per (kernel, device, host thread),
 *    the facts that hipFuncSetAttribute has opted a kernel in to > 48 KiB of LDS and how many
 *    workgroups of the persistent short-K GEMM the device holds at once — and ONE debug switch,
 *    ganffn_debug_set_ffn_mode (default 0; bits 0..6 select the older launch sequences of the
 *    d_model-100 sub-chains for A/B measurement, bits 8..19 force the chunk counts of two kernels
 *    — same results to rounding; documented at its declaration).  The library exports nothing
 *    that is not declared here: in-kernel time stamps and their ganffn_lab_* setters exist only in
 *    the lab build (`make LAB=1`, a different .so), and the library reads no environment variable.
 *  - Results are bit-reproducible: no kernel accumulates with floating-point atomics (weight
 *    gradients, bias gradients, LayerNorm gradients and loss sums are owner-computed or reduced
 *    in a fixed order), so two runs from the same state and RNG offset give identical bits.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it and the call
 *    returns without synchronising (so calls are capturable in a hipGraph).
 *  - Return value: 0 ok; < 0 argument/shape/alignment error (message via
 *    ganffn_last_error, thread-local); > 0 a hipError_t from a launch.
 *  - Parameters of one encoder stack live in ONE slab: L consecutive layer blocks of
 *    ganffn_layer_param_count(E, F) floats, each laid out per ganffn_layer_param_offsets.
 *    Gradient and Adam-state slabs use the same layout.  gan_ffn_amd/model.py exposes the
 *    slab through nn.Parameter views named like the reference's state_dict keys
 *    (transformer_encoder.layers.N.self_attn.in_proj_weight ...).
 *  - Dropout uses the counter-based Philox4x32-10 contract of oracle/philox.py /
 *    gan_ffn_amd/csrc/common.h (philox4, drop_mult4).  `rng` points to TWO device uint64: {seed, offset}; kernels read them
 *    at run time, so a captured graph replays with fresh masks after ganffn_rng_advance.
 */
#ifndef GANFFN_H
#define GANFFN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GANFFN_VERSION 100 /* 0.1.0 */
#define GANFFN_MAX_SEQ 112 /* PositionalEncoding(max_len=110), model.py:1179, rounded up to 4 */

/* Encoder-stack configuration: PositionalEncoding + L post-LN nn.TransformerEncoderLayer
 * (model.py:1178-1197, 1210-1213).  p_* = 0 or train = 0 disables that dropout site.
 * Accepted: 1 <= S <= 110; E a multiple of 4, 4 <= E <= 640; H dividing E with an even head_dim E / H <= 64; F a multiple
 * of 4; 1 <= L <= 64.  Anything else is refused with a message.  Widths off the workload's (100, 512, 600, 300) run on the
 * generic kernels and are checked against the fp64 oracle by tests/test_hip_dispatch_range.py. */
typedef struct ganffn_enc_cfg {
    int32_t S, B;       /* sequence length (<= 110) and batch (dialogues) */
    int32_t E, H, F, L; /* d_model, heads, dim_feedforward (2048), layers (8) */
    float p_pe;         /* PositionalEncoding dropout, 0.2 (model.py:1179) */
    float p_enc;        /* TransformerEncoderLayer dropout, 0.1 (torch default; model.py:1210) */
    float ln_eps;       /* 1e-5 */
    int32_t train;      /* 1: dropout active (module.train()), 0: eval */
} ganffn_enc_cfg;

/* Head configuration (the layers after the encoder stack).
 *  kind 0 = generator  : gelu -> drop -> gelu(drop(fc1)) -> gelu(drop(fc2))            model.py:1223-1228
 *  kind 1 = discriminator: gelu -> gelu(drop(fc1)) -> gelu(drop(fc2)) -> sigmoid(drop(fc3)) model.py:1322-1326 */
typedef struct ganffn_head_cfg {
    int32_t T;          /* tokens = S*B */
    int32_t E;          /* input width (d_model) */
    int32_t D1, D2;     /* fc1 / fc2 output widths (gen: 512|1024, D_h; disc: 64, 16) */
    int32_t kind;
    float p;            /* module dropout (0.2) */
    int32_t train;
} ganffn_head_cfg;

/* ---- library info ------------------------------------------------------------------ */
int ganffn_version(void);
const char* ganffn_last_error(void);

/* ---- parameter slab layout --------------------------------------------------------- */
/* floats per encoder layer; offsets[12] in this order:
 * in_proj_weight[3E,E] in_proj_bias[3E] out_proj.weight[E,E] out_proj.bias[E]
 * linear1.weight[F,E] linear1.bias[F] linear2.weight[E,F] linear2.bias[E]
 * norm1.weight[E] norm1.bias[E] norm2.weight[E] norm2.bias[E] */
int64_t ganffn_layer_param_count(int E, int F);
int ganffn_layer_param_offsets(int E, int F, int64_t* offsets12);

/* ---- sizes the caller must allocate ------------------------------------------------ */
int64_t ganffn_encoder_saved_floats(const ganffn_enc_cfg* cfg);     /* saved-for-backward */
int64_t ganffn_encoder_workspace_floats(const ganffn_enc_cfg* cfg); /* scratch, fwd or bwd */
/* float offset, inside `saved`, of layer `layer`'s FFN hidden activation h = drop(relu(x1 W1^T + b1)) [T x F]
 * (inspection hook: tests read the ReLU pattern the forward pass actually took); -1 on a bad cfg / layer */
int64_t ganffn_encoder_saved_hidden_offset(const ganffn_enc_cfg* cfg, int layer);
int64_t ganffn_head_saved_floats(const ganffn_head_cfg* cfg);
int64_t ganffn_head_workspace_floats(const ganffn_head_cfg* cfg);

/* ---- RNG state --------------------------------------------------------------------- */
/* rng[0] = seed, rng[1] = offset (device memory).  offset += delta, on the stream. */
int ganffn_rng_advance(uint64_t* rng, uint64_t delta, void* stream);

/* ---- A1: PositionalEncoding table (model.py:1182-1188) ----------------------------- */
/* pe[max_len x E] on device, computed as the reference does (fp32 sin/cos of p*exp(-2i ln1e4/E)). */
int ganffn_pe_table(float* pe, int max_len, int E, void* stream);

/* ---- A1+A2: encoder stack = PE + L encoder layers (model.py:1196-1197, 1224) -------- */
/* x_in [T x E]; pe [>=S x E]; params: L layer blocks; out [T x E] (output of the last layer);
 * saved: ganffn_encoder_saved_floats floats (needed by _bwd; pass NULL for inference-only,
 * then workspace is used and nothing is kept); rng_offset_add is added to rng[1] for this call. */
int ganffn_encoder_fwd(const ganffn_enc_cfg* cfg, const float* x_in, const float* pe,
                       const float* params, float* out, float* saved, float* workspace,
                       const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* The eval-mode and the train-mode forward of ONE stack over the SAME input as one pass over two row segments (the GAN
 * schedule runs a generator in eval mode in a discriminator sub-step and in train mode, on the same batch with the same
 * parameters, in the sub-step after it).  cfg is the train-mode cfg; segment 0 runs it with train = 0 and keeps nothing
 * (out_eval), segment 1 runs it as given (out_train, saved_train: what ganffn_encoder_fwd would save).  Every launch covers
 * both segments; each output has the bits of the corresponding ganffn_encoder_fwd call (eval: saved = NULL; train: the same
 * rng_offset_add).  workspace: ganffn_encoder_fwd_pair_workspace_floats floats.  _supported: 1 when every kernel on the
 * stack's path has a two-segment form (today: every valid cfg, unless the debug mode word selects a lab variant of the
 * 2048 -> 100 product), else 0 — ganffn_encoder_fwd_pair then fails and the caller issues the two passes itself. */
int ganffn_encoder_fwd_pair_supported(const ganffn_enc_cfg* cfg);
int64_t ganffn_encoder_fwd_pair_workspace_floats(const ganffn_enc_cfg* cfg);
int ganffn_encoder_fwd_pair(const ganffn_enc_cfg* cfg, const float* x_in, const float* pe, const float* params,
                            float* out_eval, float* out_train, float* saved_train, float* workspace,
                            const uint64_t* rng, uint64_t rng_offset_add_train, void* stream);

/* Backward through layers [layer_lo, layer_hi) in reverse order.  dx [T x E] is in/out: on entry
 * dL/d(output of layer layer_hi-1), on exit dL/d(input of layer layer_lo); when layer_lo == 0 the
 * PE dropout backward is applied too, so dx is then dL/d(x_in).  grads (same layout as params)
 * is ACCUMULATED into (+=) when non-NULL; NULL skips every weight gradient (train_gen's pass
 * through the frozen discriminator, train_IEMOCAP.py:245-250: those grads are never used).
 * Splitting the range lets the caller start a layer's gradient all-reduce while earlier layers
 * are still in backward.
 * A sequence of range calls (top range first, the same dx and grads) computes what the whole-range
 * call computes, to rounding and NOT to the bit: the layer below a boundary reads dx from a plain
 * unsplit GEMM where the whole-range pass forms that product inside the next LayerNorm backward
 * (d_model 100) or as split-K slabs (other widths), and a smaller group of weight-gradient problems
 * may cut its token range into another number of chunks (from 512 tokens on).  Every call is
 * bit-reproducible in itself; the workspace carries nothing from one call to the next. */
int ganffn_encoder_bwd(const ganffn_enc_cfg* cfg, int layer_lo, int layer_hi, float* dx,
                       const float* params, float* grads, const float* saved, float* workspace,
                       const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* The same with need_dx_in = 0 when the stack's input needs no gradient (a network trained on data or on detached
 * fakes: train_disc / train_gen, train_IEMOCAP.py:200-252 — the networks' own inputs there are raw modalities or `.detach()`ed): with layer_lo == 0
 * the bottom layer's in-proj dgrad and the PE dropout backward are skipped, as autograd skips them for an input that does
 * not require grad, and dx is then left UNDEFINED on exit.  need_dx_in = 1 is ganffn_encoder_bwd. */
int ganffn_encoder_bwd2(const ganffn_enc_cfg* cfg, int layer_lo, int layer_hi, float* dx,
                        const float* params, float* grads, const float* saved, float* workspace,
                        const uint64_t* rng, uint64_t rng_offset_add, int need_dx_in, void* stream);

/* The whole-stack backward of a d_model-100 network with its weight gradients left UNREDUCED (round 5; the single-GPU step
 * runner): replaces `opt.zero_grad(); loss.backward()` + the gradient read of `opt.step()` of train_disc / train_gen
 * (train_IEMOCAP.py:216-226, 245-251) without the 14.5 MB zero-fill of the gradient slab and without the reduce launch.
 * The grouped weight-gradient launch cuts the token range into *n_parts chunks; chunk 0 WRITES (not +=) its partial
 * gradients into grads' encoder region, chunk z >= 1 into workspace + *part_offset + (z - 1) * *part_stride, a buffer shaped
 * like that region; the LayerNorm parameter gradients are written too.  So grads' encoder region [0, L * layer floats) need
 * NOT be zeroed by the caller (everything behind it — heads, `object` — still accumulates).  ganffn_adam_step_parts then adds
 * the chunks in order: exactly the sum, in exactly the association, that ganffn_encoder_bwd2's reduce launch forms — the
 * update is bit-identical (*n_parts is the chunk count the reduce launch chooses for the same pass, also where the
 * unreduced form alone would have room for more).  The workspace must stay untouched between the two calls.
 * ganffn_encoder_bwd_parts_supported(cfg): 1 when this form exists for cfg (d_model 100, default kernel paths), else 0;
 * ganffn_encoder_bwd_parts_covered(E, F): floats at the head of each layer block that the chunks cover (weights and biases of
 * in-proj, out-proj, linear1, linear2; the LayerNorm parameters behind them are not chunked). */
int ganffn_encoder_bwd_parts_supported(const ganffn_enc_cfg* cfg);
int64_t ganffn_encoder_bwd_parts_covered(int E, int F);
int ganffn_encoder_bwd_parts(const ganffn_enc_cfg* cfg, float* dx, const float* params, float* grads, const float* saved,
                             float* workspace, const uint64_t* rng, uint64_t rng_offset_add, int need_dx_in,
                             int64_t* part_offset, int64_t* part_stride, int* n_parts, void* stream);

/* ---- A3-A6: heads ------------------------------------------------------------------- */
/* x [T x E] = encoder output.  w1[D1,E] b1[D1] w2[D2,D1] b2[D2]; disc only: w3[1,D2] b3[1].
 * out: gen -> fusion [T x D2]; disc -> prob [T x 1]. */
int ganffn_head_fwd(const ganffn_head_cfg* cfg, const float* x, const float* w1, const float* b1,
                    const float* w2, const float* b2, const float* w3, const float* b3, float* out,
                    float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add,
                    void* stream);
/* d_out: gen [T x D2], disc [T x 1].  dx [T x E] written.  g* accumulated (+=) when non-NULL.
 * The gradient pointers come in pairs: a bias gradient without its weight gradient (gbK != NULL, gwK == NULL, K = 1, 2, 3)
 * is refused, and so is gw3 without gb3 (the fc3 reduce writes both); gw1 / gw2 without gb1 / gb2 are legal, and all NULL
 * computes dx alone (the pass through a frozen discriminator).  A refused call names the pair and writes nothing. */
int ganffn_head_bwd(const ganffn_head_cfg* cfg, const float* d_out, const float* x,
                    const float* w1, const float* w2, const float* w3, float* gw1, float* gb1,
                    float* gw2, float* gb2, float* gw3, float* gb3, float* dx, const float* saved,
                    float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* ---- plain Linear (VisualDiscriminator.object model.py:1355-1356; GAN_FFN.fc model.py:1448) */
int ganffn_linear_fwd(const float* x, const float* w, const float* b, float* y, int T, int K, int N,
                      void* stream);
/* dx may be NULL; gw/gb accumulated (+=) when non-NULL.  workspace (may be NULL; ganffn_linear_bwd_workspace_floats
 * floats, 16-byte aligned) lets the weight gradient split the token range over more workgroups; the partial results are
 * reduced in a fixed order, so the result is bit-reproducible with or without it. */
int64_t ganffn_linear_bwd_workspace_floats(int T, int K, int N);
int ganffn_linear_bwd(const float* dy, const float* x, const float* w, float* dx, float* gw,
                      float* gb, int T, int K, int N, float* workspace, int64_t workspace_floats, void* stream);

/* ---- A10: BCELoss(mean) (train_IEMOCAP.py:300,220-223,248) -------------------------- */
/* loss_out[0] (+)= scale * mean_i( -(y*max(log p,-100) + (1-y)*max(log(1-p),-100)) ), y = target.
 * accumulate != 0 adds to loss_out (the D loss is (real + fake)/2: two calls with scale 0.5). */
int ganffn_bce_fwd(const float* prob, float target, int n, float scale, float* loss_out,
                   int accumulate, void* stream);
/* dprob[i] = scale/n * (p - y) / max(p*(1-p), 1e-12)   (torch's binary_cross_entropy_backward) */
int ganffn_bce_bwd(const float* prob, float target, int n, float scale, float* dprob, void* stream);
/* Two-valued periodic target: y_i = (i % period) < split ? target_a : target_b.  train_disc's loss
 * (BCE(D(real),1) + BCE(D(fake),0)) / 2 (train_IEMOCAP.py:220-223) is ONE call on the batched
 * [real | fake] pass (batch axis 2B: period 2B, split B, target_a 1, target_b 0, scale 1). */
int ganffn_bce2_fwd(const float* prob, float target_a, float target_b, int period, int split, int n,
                    float scale, float* loss_out, int accumulate, void* stream);
int ganffn_bce2_bwd(const float* prob, float target_a, float target_b, int period, int split, int n,
                    float scale, float* dprob, void* stream);

/* ---- A10: Adam over a flat slab (train_IEMOCAP.py:292-297; phase 2 :661) ------------- */
/* step: device int32 counter, incremented by this call BEFORE use (t = ++*step).
 * g = grad + weight_decay*p (L2-coupled, not AdamW).  n floats. */
int ganffn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                     int32_t* step, int64_t n, float lr, float beta1, float beta2, float eps,
                     float weight_decay, float grad_scale, void* stream);
/* ganffn_adam_step over a slab whose encoder weight gradients ganffn_encoder_bwd_parts left unreduced: for element i of the
 * covered part of a layer block (i < enc_floats, i % layer_floats < covered_per_layer) the gradient is
 * grads[i] + parts[i] + parts[part_stride + i] + ... (n_parts - 1 extra chunks, in order); elsewhere grads[i].
 * n_parts == 1 is ganffn_adam_step. */
int ganffn_adam_step_parts(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int32_t* step, int64_t n,
                           float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                           const float* parts, int64_t part_stride, int n_parts, int64_t enc_floats, int64_t layer_floats,
                           int64_t covered_per_layer, void* stream);
/* The same update on a SLICE of the slabs with t = *step + 1 and the counter left alone, and the bump on its own:
 * data-parallel training applies Adam bucket by bucket, each as soon as its gradient all-reduce has finished
 * (ganffn_adam_update per bucket, then one ganffn_adam_bump) — identical to one ganffn_adam_step over the whole slab. */
int ganffn_adam_update(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                       const int32_t* step, int64_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, float grad_scale, void* stream);
int ganffn_adam_bump(int32_t* step, void* stream);

/* ---- A11: phase 2 (model.py:1441-1449, :74-81) --------------------------------------- */
/* fusion = a + b + c (elementwise, n floats) */
int ganffn_add3(const float* a, const float* b, const float* c, float* out, int64_t n, void* stream);
/* logits [T x C] (token t = s*B+b) -> log_prob [T x C]; loss_out[0] = masked weighted NLL:
 * -sum_t w[y_t] m_t lp[t,y_t] / sum_t w[y_t] m_t, labels/umask are batch-major [B x S] as the
 * reference's collate makes them (dataloader.py:55-58); class_w may be NULL (unweighted).
 * dlogits (may be NULL) receives dL/dlogits.  log_prob = (x - max) - log(sum exp(x - max)): a common shift of a token's
 * logits does not change it.  When every token is masked out (sum_t w[y_t] m_t = 0) the loss and dlogits are 0 (the
 * reference divides 0 by 0 there). */
int ganffn_logsoftmax_nll(const float* logits, const int64_t* labels, const float* umask,
                          const float* class_w, float* log_prob, float* loss_out, float* dlogits,
                          float* workspace2, int S, int B, int C, void* stream);

/* ---- N2 (config 5): masked "general2" matching attention, all time steps as queries ---- */
/* Replaces BiModel.forward's loop over MatchingAttention(att_type="general2") (model.py:1043-1049 -> :169-182,
 * :193).  x = transform(mem) [S x B x D] (caller's linear), mem [S x B x D], mask [B x S] (umask).  Outputs:
 * att [S x B x D] pooled memory per query step, alpha [B x S x S] (dialogue, query step, memory step) — the
 * reference's per-step alpha lists stacked —, tanh_s [B x S x S] saved for backward.  S <= 128, D <= 1024.
 * Also the attention of MELDLSTMModel.forward (model.py:547-552). */
int ganffn_general2_attention_fwd(const float* x, const float* mem, const float* mask, float* att,
                                  float* alpha, float* tanh_s, int S, int B, int D, void* stream);
/* d_att [S x B x D] -> dx, dmem [S x B x D] (dmem = pooling path + score path; the gradient through
 * x = transform(mem) is the caller's linear backward).  du_ws: workspace of B*S*S floats. */
int ganffn_general2_attention_bwd(const float* d_att, const float* x, const float* mem, const float* mask,
                                  const float* alpha, const float* tanh_s, float* du_ws, float* dx,
                                  float* dmem, int S, int B, int D, void* stream);

/* ---- N2 (config 5): the DialogueRNN recurrence ------------------------------------------ */
/* Replaces DialogueRNN.forward / DialogueRNNCell.forward (model.py:828-972) in the configuration
 * train_IEMOCAP_DialogueRNN.py runs: context_attention = "general" (:586), listener_state = False (:595), two parties
 * (listener state: ganffn_drnn_listener_*; the other attention types, with or without it: ganffn_drnn_att_* below; any
 * party count from 1 to GANFFN_DRNN_MAX_PARTIES, every attention type, with or without listener state:
 * ganffn_drnn_party_* at the end of this section, of which the two-party entry points are the parties = 2 case).
 * One call runs ndir (1 or 2) independent DialogueRNNs — BiModel's forward and reverse directions (model.py:1025-1033)
 * — through the same launches.  Per direction:
 *   U [S x B x D_m] (the reverse direction gets the reversed sequences, as BiModel._reverse_seq builds them),
 *   spk [S x B] int32 = argmax(qmask, party), mval [S x B] = qmask[s, b, spk] (0 on padded steps),
 *   e_out [S x B x D_e] emotion states (after dropout), alpha [B x S x S]: row t = attention weights of step t over the
 *   global history g_0 .. g_{t-1} (zero elsewhere; the reference's per-step alpha list is alpha[:, t, :t]).
 * Dropout (p = dropout_rec, train != 0) on g, the speaker's party state and e, Philox rows t*B + b, sites 8, 9, 10
 * (+ 4 for the second direction); the listener variant below adds site 11 (+ 4). */
typedef struct ganffn_drnn_cfg {
    int32_t S, B;        /* steps (<= 112), dialogues (<= 32) */
    int32_t Dm, H, He;   /* D_m, D_g = D_p, D_e  (100, 500, 100; multiples of 4) */
    float p;             /* dropout_rec */
    int32_t train;
} ganffn_drnn_cfg;
/* the 13 parameter tensors of one DialogueRNNCell (state_dict names under dialogue_cell.): g_cell / p_cell / e_cell
 * weight_ih [3H x (D_m+H)] | [3H x (D_m+H)] | [3He x H], weight_hh [3H x H] | [3H x H] | [3He x He], bias_ih, bias_hh,
 * attention.transform.weight [H x D_m] */
typedef struct ganffn_drnn_params {
    const float *g_wih, *g_whh, *g_bih, *g_bhh, *p_wih, *p_whh, *p_bih, *p_bhh, *e_wih, *e_whh, *e_bih, *e_bhh, *att_w;
} ganffn_drnn_params;
typedef struct ganffn_drnn_grads {   /* accumulated into (+=); all NULL = input gradient only */
    float *g_wih, *g_whh, *g_bih, *g_bhh, *p_wih, *p_whh, *p_bih, *p_bhh, *e_wih, *e_whh, *e_bih, *e_bhh, *att_w;
} ganffn_drnn_grads;
int64_t ganffn_drnn_saved_floats(const ganffn_drnn_cfg* cfg);      /* per direction */
int64_t ganffn_drnn_workspace_floats(const ganffn_drnn_cfg* cfg);  /* per direction; fwd and bwd */
/* (every ganffn_drnn_*_workspace_floats: with D_e > 128 the emotion cell runs per step and shares three step regions with the
 * g / p cells — pre-activations 2 x [B x 3 D] and the direct-path gradient [B x D] — which are sized for D = max(D_g, D_e);
 * for D_e > max(D_g, 128) that is 7 B (D_e - D_g) floats more than the D_g-sized regions.  D_e <= 128 or D_e <= D_g: D = D_g.) */
/* every array argument has ndir entries */
int ganffn_drnn_fwd(const ganffn_drnn_cfg* cfg, int ndir, const float* const* U, const int32_t* const* spk,
                    const float* const* mval, const ganffn_drnn_params* params, float* const* e_out,
                    float* const* alpha, float* const* saved, float* const* workspace, const uint64_t* rng,
                    uint64_t rng_offset_add, void* stream);
/* d_e [S x B x D_e] -> dU [S x B x D_m] (written), parameter gradients accumulated */
int ganffn_drnn_bwd(const ganffn_drnn_cfg* cfg, int ndir, const float* const* d_e, const float* const* U,
                    const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* params,
                    const ganffn_drnn_grads* grads, float* const* dU, const float* const* alpha,
                    const float* const* saved, float* const* workspace, const uint64_t* rng,
                    uint64_t rng_offset_add, void* stream);
/* The same recurrence with listener_state = True (model.py:899-921; train_IEMOCAP_DialogueRNN.py --active-listener): every
 * party row also takes a listener GRU step ql[p] = drop(l_cell([U_t, qs], q_{t-1}[p])), p = 0, 1, with qs the speaker's new
 * state after its dropout, and q_t[p] = (m != 0 && p == spk) ? qs : ql[p] — on padded steps (m = 0) both rows take ql.
 * Same cfg, same arguments plus the 4 l_cell tensors per direction: weight_ih [3H x (D_m+H)], weight_hh [3H x H], bias_ih,
 * bias_hh.  saved / workspace are sized by the _listener_ functions (per direction; larger than the listener-free sizes).
 * Listener dropout (train != 0): Philox site 11 + 4 * direction, row t*B + b, column p*H + u of a width-2H row, i.e. on the
 * CPU keep_mask(S*B, 2*H, p, 11 + 4*z, seed, offset).view(S, B, 2, H).  lgrads (ndir entries, accumulated into) may be
 * NULL, or have NULL members: no l_cell weight gradients. */
typedef struct ganffn_drnn_listener_params {
    const float *l_wih, *l_whh, *l_bih, *l_bhh;
} ganffn_drnn_listener_params;
typedef struct ganffn_drnn_listener_grads {
    float *l_wih, *l_whh, *l_bih, *l_bhh;
} ganffn_drnn_listener_grads;
int64_t ganffn_drnn_listener_saved_floats(const ganffn_drnn_cfg* cfg);      /* per direction */
int64_t ganffn_drnn_listener_workspace_floats(const ganffn_drnn_cfg* cfg);  /* per direction; fwd and bwd */
int ganffn_drnn_listener_fwd(const ganffn_drnn_cfg* cfg, int ndir, const float* const* U, const int32_t* const* spk,
                             const float* const* mval, const ganffn_drnn_params* params,
                             const ganffn_drnn_listener_params* lparams, float* const* e_out, float* const* alpha,
                             float* const* saved, float* const* workspace, const uint64_t* rng, uint64_t rng_offset_add,
                             void* stream);
int ganffn_drnn_listener_bwd(const ganffn_drnn_cfg* cfg, int ndir, const float* const* d_e, const float* const* U,
                             const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* params,
                             const ganffn_drnn_listener_params* lparams, const ganffn_drnn_grads* grads,
                             const ganffn_drnn_listener_grads* lgrads, float* const* dU, const float* const* alpha,
                             const float* const* saved, float* const* workspace, const uint64_t* rng,
                             uint64_t rng_offset_add, void* stream);

/* The other context attention types of DialogueRNNCell (model.py:856-859, MatchingAttention :134-194, SimpleAttention
 * :117-131; train_IEMOCAP_DialogueRNN.py --attention, :586): the same recurrence, the same launches per step (2 + 2
 * without listener state, 4 + 4 with it), one attention descriptor for both directions.  At step t >= 1 the memory is
 * g_0 .. g_{t-1} (after dropout), alpha = softmax_j(s_j), c_t = sum_j alpha_j g_j; s_j per type:
 *   general  <W U_t, g_j>                 w = transform.weight [D_g x D_m]
 *   simple   <w, g_j>                     w = scalar.weight [1 x D_g]
 *   dot      <U_t, g_j>                   no parameters; D_m == D_g
 *   general2 tanh(<W U_t + b, g_j>)       w = transform.weight [D_g x D_m], b = transform.bias [D_g] (the cell passes
 *                                         no mask: masking and re-normalisation are the identity)
 *   concat   v . tanh(W [g_j ; U_t])      w = transform.weight [D_a x (D_g + D_m)] (memory columns first),
 *                                         v = vector_prod.weight [1 x D_a]; D_a a multiple of 4, <= 512
 * params.att_w (and grads.att_w) are ignored: the attention's parameters are aparams (ndir entries; NULL for dot).
 * lparams == NULL: listener_state False, else the listener path above (lgrads as there).  saved / workspace are sized by
 * ganffn_drnn_att_saved_floats / _workspace_floats(cfg, att, listener) (per direction).  agrads (ndir entries or NULL;
 * members NULL = not wanted) are accumulated into.  No dropout of its own; deterministic (no atomics). */
enum { GANFFN_DRNN_ATT_GENERAL = 0, GANFFN_DRNN_ATT_SIMPLE = 1, GANFFN_DRNN_ATT_DOT = 2, GANFFN_DRNN_ATT_GENERAL2 = 3,
       GANFFN_DRNN_ATT_CONCAT = 4 };
typedef struct ganffn_drnn_att {
    int32_t type;        /* GANFFN_DRNN_ATT_* */
    int32_t Da;          /* concat: D_a (train_IEMOCAP_DialogueRNN.py:641: 100); ignored otherwise */
} ganffn_drnn_att;
typedef struct ganffn_drnn_att_params {
    const float *w, *b, *v;
} ganffn_drnn_att_params;
typedef struct ganffn_drnn_att_grads {
    float *w, *b, *v;
} ganffn_drnn_att_grads;
int64_t ganffn_drnn_att_saved_floats(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int listener);
int64_t ganffn_drnn_att_workspace_floats(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int listener);
int ganffn_drnn_att_fwd(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int ndir, const float* const* U,
                        const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* params,
                        const ganffn_drnn_listener_params* lparams, const ganffn_drnn_att_params* aparams,
                        float* const* e_out, float* const* alpha, float* const* saved, float* const* workspace,
                        const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_drnn_att_bwd(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int ndir, const float* const* d_e,
                        const float* const* U, const int32_t* const* spk, const float* const* mval,
                        const ganffn_drnn_params* params, const ganffn_drnn_listener_params* lparams,
                        const ganffn_drnn_att_params* aparams, const ganffn_drnn_grads* grads,
                        const ganffn_drnn_listener_grads* lgrads, const ganffn_drnn_att_grads* agrads, float* const* dU,
                        const float* const* alpha, const float* const* saved, float* const* workspace,
                        const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* Any number of parties (DialogueRNNCell with qmask [S x B x P], model.py:861-926; MELD's speaker one-hots are 9 wide):
 * ganffn_drnn_att_* with one more argument, parties = P, 1 <= P <= GANFFN_DRNN_MAX_PARTIES (anything else is an argument
 * error reported through ganffn_last_error).  spk (argmax over the P columns) must be < P, as it is < 2 above.  The party
 * states are [B x P x H]: the speaker's row takes the party cell's step, the other P - 1 rows keep their state (with
 * listener state every row takes the listener step, then the blend).  general attention goes through it like the
 * others: aparams[z].w = transform.weight.  saved / workspace are sized by ganffn_drnn_party_saved_floats /
 * _workspace_floats(cfg, att, listener, parties) (per direction); at parties = 2 they equal the _att_ sizes and every
 * call is the same launch sequence as ganffn_drnn_att_*, bit for bit.
 * Dropout: the party cell's site 9 (+ 4) mask is one row of width H per (t, b), shared by all party rows (only the
 * speaker's row is used); the listener's site 11 (+ 4) mask is row t*B + b, column p*H + u of a width-P*H row, i.e.
 * keep_mask(S*B, P*H, p, 11 + 4*z, seed, offset).view(S, B, P, H) — the two-party layout above at P = 2.
 * Launches per step: 2 + 2 without listener state for any P; 4 + 4 with it (the listener's products of a step are one
 * launch of 2 (1 + P) skinny problems: the bound on P is what that launch's argument block holds). */
#define GANFFN_DRNN_MAX_PARTIES 16
int64_t ganffn_drnn_party_saved_floats(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int listener, int parties);
int64_t ganffn_drnn_party_workspace_floats(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int listener, int parties);
int ganffn_drnn_party_fwd(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int parties, int ndir, const float* const* U,
                          const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* params,
                          const ganffn_drnn_listener_params* lparams, const ganffn_drnn_att_params* aparams,
                          float* const* e_out, float* const* alpha, float* const* saved, float* const* workspace,
                          const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_drnn_party_bwd(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int parties, int ndir, const float* const* d_e,
                          const float* const* U, const int32_t* const* spk, const float* const* mval,
                          const ganffn_drnn_params* params, const ganffn_drnn_listener_params* lparams,
                          const ganffn_drnn_att_params* aparams, const ganffn_drnn_grads* grads,
                          const ganffn_drnn_listener_grads* lgrads, const ganffn_drnn_att_grads* agrads, float* const* dU,
                          const float* const* alpha, const float* const* saved, float* const* workspace,
                          const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* Any batch size up to GANFFN_MAX_DIALOGUES (every reference trainer has --batch-size: train_IEMOCAP_DialogueRNN.py:580,
 * train_MELD.py:114; BASELINE.json configs[3] names a global batch of 256): ganffn_drnn_party_* with 1 <= cfg->B <=
 * GANFFN_MAX_DIALOGUES (anything else is an argument error reported through ganffn_last_error; the entry points above keep
 * their B <= 32).  The skinny products of a step take the dialogues in tiles of 32 on a grid axis, so a step is still 2 + 2
 * launches (4 + 4 with listener state) whatever B is, and every dialogue's sums are formed in the order of a 32-dialogue
 * call: in eval mode row b of the outputs does not depend on which other dialogues share the call.  Sizes, layouts
 * (functions of B as documented above) and arguments are those of ganffn_drnn_party_*; at B <= 32 every call is the same
 * launch sequence, bit for bit.  Dropout rows are t*B + b with B the whole batch of the call. */
#define GANFFN_MAX_DIALOGUES 256
int64_t ganffn_drnn_batch_saved_floats(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int listener, int parties);
int64_t ganffn_drnn_batch_workspace_floats(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int listener, int parties);
int ganffn_drnn_batch_fwd(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int parties, int ndir, const float* const* U,
                          const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* params,
                          const ganffn_drnn_listener_params* lparams, const ganffn_drnn_att_params* aparams,
                          float* const* e_out, float* const* alpha, float* const* saved, float* const* workspace,
                          const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_drnn_batch_bwd(const ganffn_drnn_cfg* cfg, const ganffn_drnn_att* att, int parties, int ndir, const float* const* d_e,
                          const float* const* U, const int32_t* const* spk, const float* const* mval,
                          const ganffn_drnn_params* params, const ganffn_drnn_listener_params* lparams,
                          const ganffn_drnn_att_params* aparams, const ganffn_drnn_grads* grads,
                          const ganffn_drnn_listener_grads* lgrads, const ganffn_drnn_att_grads* agrads, float* const* dU,
                          const float* const* alpha, const float* const* saved, float* const* workspace,
                          const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* Data movement of BiModel.forward around the recurrence (model.py:1008-1062), one launch each (csrc/drnn_head.hip):
 * ganffn_seq_reverse: out[s, b, :] (+)= s < lens[b] ? x[lens[b]-1-s, b, :] : 0 — BiModel._reverse_seq and, being its own
 *   transpose, its gradient (accumulate != 0 adds into out); x, out [S x B x D], D % 4 == 0.
 * ganffn_drnn_join_fwd: emotions [S x B x 2 D_e] = cat(dropout(e_f), dropout(reverse(e_b))) with p = dropout_rec + ...
 *   (BiModel.dropout_rec), two dropout sites; ganffn_drnn_join_bwd: the gradients of e_f and of e_b (in the reverse
 *   direction's own order) from d_emotions, same masks.  Mask layout: both halves are [S*B x D_e] Philox masks at the
 *   FORWARD-time token row t = s*B + b, column c < D_e, one (seed, offset + rng_offset_add); the first half at site_f, the
 *   second at site_b.  The second half's mask applies after the reversal: the element of e_b at reverse step len_b-1-s
 *   lands on row s*B + b and takes that row's mask, as the reference applies dropout_rec to reverse(e_b).
 * lens [B] (ganffn_seq_reverse, ganffn_drnn_join_*): 0 <= lens[b] <= S.  The kernels do not clamp it — a length outside that
 *   range indexes outside the buffers — so the range is the caller's contract.  Rows s >= lens[b] of a reversed tensor are
 *   exact zeros (accumulate: left as they are).
 * ganffn_mask_pos_inplace: d[i] = aux[i] > 0 ? d[i] * mscale : 0 — backward through dropout(relu(.)) from the saved output.
 *   The predicate is IEEE's: a positive subnormal passes, +0 and -0 mask; a masked element is +0. */
int ganffn_seq_reverse(const float* x, const int32_t* lens, float* out, int S, int B, int D, int accumulate, void* stream);
int ganffn_drnn_join_fwd(const float* e_f, const float* e_b, const int32_t* lens, float* emotions, int S, int B, int De,
                         float p, uint32_t site_f, uint32_t site_b, const uint64_t* rng, uint64_t rng_offset_add, int train,
                         void* stream);
int ganffn_drnn_join_bwd(const float* d_emotions, const int32_t* lens, float* d_e_f, float* d_e_b, int S, int B, int De,
                         float p, uint32_t site_f, uint32_t site_b, const uint64_t* rng, uint64_t rng_offset_add, int train,
                         void* stream);
int ganffn_mask_pos_inplace(float* d, const float* aux, float mscale, int64_t n, void* stream);

/* one launch of the recurrence's skinny product, `copies` (<= 8) independent problems sharing A: C_i[M x N] = A[M x K]
 * W_i^T (nn = 0, W_i [N x K]) or A W_i (nn = 1, W_i [K x N]); W / C hold the copies back to back; M <= 32 (unit tests and
 * the roofline leg of bench.py --config drnn) */
int ganffn_drnn_skinny(int nn, int copies, const float* A, const float* W, float* C, int M, int N, int K, void* stream);
/* the same with M <= GANFFN_MAX_DIALOGUES: above 32 rows the launch takes them in tiles of 32 on a grid axis (unit tests) */
int ganffn_drnn_skinny_batch(int nn, int copies, const float* A, const float* W, float* C, int M, int N, int K, void* stream);

/* ---- building blocks exported for unit tests ----------------------------------------- */
/* C[M x N] = A[M x K] * W[N x K]^T + bias (bias may be NULL) */
int ganffn_gemm_nt(const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                   void* stream);
/* C[M x N] = A[M x K] * B[K x N] */
int ganffn_gemm_nn(const float* A, const float* Bm, float* C, int M, int N, int K, void* stream);
/* C[M x N] += At[K x M]^T * B[K x N];  colsum[M] += sum_k At[k][m] when colsum != NULL */
int ganffn_gemm_tn_acc(const float* At, const float* Bm, float* C, float* colsum, int M, int N, int K,
                       void* stream);
/* h[T x F] = dropout_p(relu(x[T x E] * W1[F x E]^T + b1)): linear1 + activation + dropout of the encoder layer's
 * feed-forward block (torch TransformerEncoderLayer._ff_block; call site model.py:1210), one fused GEMM */
int ganffn_ffn_linear1_fwd(const float* x, const float* w1, const float* b1, float* h, int T, int E, int F,
                           float p, uint32_t site, const uint64_t* rng, uint64_t rng_offset_add, int train,
                           void* stream);
/* n (<= 40) independent problems C_i[M_i x N_i] += At_i[K_i x M_i]^T B_i[K_i x N_i] (+ column sums) in ONE launch: the
 * deferred weight-gradient GEMMs of all encoder layers of a backward pass (dense leading dimensions).  workspace
 * (ganffn_gemm_tn_grouped_workspace_floats() floats, or NULL): lets a group with few output tiles split the token range
 * over several workgroups per tile (partial slabs + one ordered reduce launch; deterministic).  NULL: one owner
 * workgroup per tile. */
int64_t ganffn_gemm_tn_grouped_workspace_floats(void);
int ganffn_gemm_tn_grouped(int n, const float* const* At, const float* const* Bm, float* const* C,
                           float* const* colsum, const int* M, const int* N, const int* K, float* workspace,
                           int64_t workspace_floats, void* stream);
/* Attention core of nn.MultiheadAttention (call sites model.py:1210,1244,1276,1307,1340,1377):
 * qkv [T x 3E] -> o [T x E]; site = dropout site id; p = 0 disables dropout.  lse [B*H x S] receives the log-sum-exp of
 * every score row (may be NULL when no backward follows).  The backward takes the forward's o and lse back: the 16-row
 * kernels (head_dim 10 and 30 at any S, 60 and 64 at S <= 48) use them instead of recomputing the softmax statistics;
 * every other case recomputes, writes no lse and ignores both (NULL allowed there).
 * Accepted: 1 <= S <= GANFFN_MAX_SEQ, H dividing E, head_dim E / H even and <= 64 (E need not be a multiple of 4),
 * B * H < 2^32 / 3584; anything else is refused with a message and nothing is written.  head_dim 10, 30, 60, 64 have
 * kernels of their own, every other one runs a kernel with a run-time head_dim. */
int ganffn_attention_fwd(const float* qkv, float* o, float* lse, int S, int B, int E, int H, float p,
                         uint32_t site, const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_attention_bwd(const float* qkv, const float* o, const float* lse, const float* d_o, float* d_qkv,
                         int S, int B, int E, int H, float p, uint32_t site, const uint64_t* rng,
                         uint64_t rng_offset_add, void* stream);
/* The same pair with the attention-dropout keep bits handed from the forward to the backward (what the encoder stack does
 * inside its saved-for-backward block): keep = ganffn_attention_keep_words(B, H) uint32, written by a forward with p > 0
 * and read by the backward INSTEAD of re-evaluating the Philox calls (head_dim <= 32; larger heads ignore it).  The
 * bits are the same, so both pairs give identical results; keep = NULL is exactly the pair above. */
int64_t ganffn_attention_keep_words(int B, int H);
int ganffn_attention_fwd_keep(const float* qkv, float* o, float* lse, uint32_t* keep, int S, int B, int E, int H,
                              float p, uint32_t site, const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_attention_bwd_keep(const float* qkv, const float* o, const float* lse, const float* d_o,
                              const uint32_t* keep, float* d_qkv, int S, int B, int E, int H, float p, uint32_t site,
                              const uint64_t* rng, uint64_t rng_offset_add, void* stream);
/* ---- key-length attention: padded utterances are not attended to -----------------------------------------------------------
 * An extension the reference does not have (its nn.TransformerEncoder calls pass no mask, so a generator's output for a real
 * utterance depends on how far the batch was padded): what nn.TransformerEncoder(..., src_key_padding_mask = mask) computes
 * when mask[b][j] = (j >= key_len[b]), on the same padded layout.  key_len is DEVICE int32 [B], never read by the host; a
 * kernel reads its dialogue's entry once per workgroup and clamps it to [1, S], so a bad length can neither empty a softmax
 * nor move a read out of range (the kernels behind the calls without lengths are instantiations of their own: they do not pay for
 * it).  With n = clamp(key_len[b], 1, S):
 *   forward   for every query row i < S (padded query rows are computed too) P[i][j] = softmax over j < n of q_i k_j / sqrt(hd)
 *             and 0 for j >= n; lse is over j < n; the dropout keep bits are those of the calls above (the Philox indexing
 *             does not depend on lengths); o_i = sum_j P~[i][j] v_j.
 *   backward  the gradient of that forward; keys j >= n get P = 0 explicitly in the recompute, and the k and v parts of d_qkv at
 *             rows n .. S-1 are WRITTEN as exact zeros.
 *   padding   finite values of k and v at rows >= n change no bit of any output (those rows are staged with a 0 factor).
 * keep may be NULL (as ganffn_attention_fwd / _bwd) or the keep words of ganffn_attention_fwd_keep.  key_len == NULL is exactly
 * the calls above, with the same bits, and so is key_len[b] >= S for every b.
 * ganffn_encoder_fwd_len / _bwd_len: ganffn_encoder_fwd / ganffn_encoder_bwd2 with the lengths handed to the attention core of
 * every layer — the only place of a layer where rows of a dialogue meet; everything else in a stack is row-wise.  Saved and
 * workspace sizes and layouts are those of ganffn_encoder_saved_floats / _workspace_floats, unchanged; the same launches.
 * The forward and the backward of one pass must be given the same lengths.
 * The GAN step has its forms too (GanEngine(mask_padding = True); the classifier step runners and the module path use the
 * entry points above when asked to):
 * ganffn_encoder_fwd_pair_len: ganffn_encoder_fwd_pair with the lengths handed to the attention of every layer in BOTH
 * segments (both are the same B dialogues, so one key_len[B] serves them).  The eval output has the bits of
 * ganffn_encoder_fwd_len(..., saved = NULL), the train output and the saved block those of ganffn_encoder_fwd_len with the same
 * rng_offset_add; key_len == NULL is ganffn_encoder_fwd_pair.  _pair_supported and _pair_workspace_floats are unchanged.
 * ganffn_encoder_bwd_parts_len: ganffn_encoder_bwd_parts with the lengths handed on; followed by ganffn_adam_step_parts the
 * update has the bits of ganffn_encoder_bwd_len + ganffn_adam_step.
 * ganffn_bce_len_fwd / _bwd: BCELoss over the real utterances only.  prob is [S x Bt] (row t = s * Bt + c); column c has target
 * target_a if c < split, else target_b, and n_c = clamp(key_len[c % n_len], 1, S) real rows (the attention clamp; a length of 0
 * or above S is clamped, not refused).  count = sum_c n_c, an integer summed on the device.
 *   forward   loss = scale * sum over s < n_c of l(s, c) / count, logs clamped at -100 as in ganffn_bce_fwd; one workgroup and a
 *             fixed-order tree, so the value is bit-reproducible.
 *   backward  dprob = scale / count * (p - y) / max(p (1 - p), 1e-12) where s < n_c; every other entry is written as +0.0f.
 * key_len == NULL, or every length >= S, gives the bits of ganffn_bce2_fwd / _bwd with period = Bt, n = S * Bt.  Refused:
 * Bt > 512, split outside [0, Bt], n_len outside [1, Bt].  Bt = 2B, split = B, n_len = B is the discriminator loss over
 * [real | fake] (both halves have the same lengths, so the one masked mean is (BCE(real, 1) + BCE(fake, 0)) / 2 over real
 * utterances); split = Bt is the generator loss. */
int ganffn_encoder_fwd_pair_len(const ganffn_enc_cfg* cfg, const int32_t* key_len, const float* x_in, const float* pe,
                                const float* params, float* out_eval, float* out_train, float* saved_train, float* workspace,
                                const uint64_t* rng, uint64_t rng_offset_add_train, void* stream);
int ganffn_encoder_bwd_parts_len(const ganffn_enc_cfg* cfg, const int32_t* key_len, float* dx, const float* params,
                                 float* grads, const float* saved, float* workspace, const uint64_t* rng,
                                 uint64_t rng_offset_add, int need_dx_in, int64_t* part_offset, int64_t* part_stride,
                                 int* n_parts, void* stream);
int ganffn_bce_len_fwd(const float* prob, const int32_t* key_len, int n_len, float target_a, float target_b, int S, int Bt,
                       int split, float scale, float* loss_out, int accumulate, void* stream);
int ganffn_bce_len_bwd(const float* prob, const int32_t* key_len, int n_len, float target_a, float target_b, int S, int Bt,
                       int split, float scale, float* dprob, void* stream);
int ganffn_attention_fwd_len(const float* qkv, float* o, float* lse, uint32_t* keep, const int32_t* key_len, int S, int B,
                             int E, int H, float p, uint32_t site, const uint64_t* rng, uint64_t rng_offset_add,
                             void* stream);
int ganffn_attention_bwd_len(const float* qkv, const float* o, const float* lse, const float* d_o, const uint32_t* keep,
                             const int32_t* key_len, float* d_qkv, int S, int B, int E, int H, float p, uint32_t site,
                             const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_encoder_fwd_len(const ganffn_enc_cfg* cfg, const int32_t* key_len, const float* x_in, const float* pe,
                           const float* params, float* out, float* saved, float* workspace, const uint64_t* rng,
                           uint64_t rng_offset_add, void* stream);
int ganffn_encoder_bwd_len(const ganffn_enc_cfg* cfg, const int32_t* key_len, int layer_lo, int layer_hi, float* dx,
                           const float* params, float* grads, const float* saved, float* workspace, const uint64_t* rng,
                           uint64_t rng_offset_add, int need_dx_in, void* stream);
/* ---- causal self-attention: a query never looks ahead -------------------------------------------------------------------------
 * The _len calls above with a flags word after key_len.  GANFFN_ATTN_CAUSAL: what nn.TransformerEncoder(src, mask = triu(-inf, 1),
 * src_key_padding_mask = pad) computes.  In every layer, query row i of dialogue b attends to keys j <= i and, when lengths are
 * given, j < clamp(key_len[b], 1, S): the key limit of a query is min(n, i + 1) >= 1, so no softmax is ever empty; lse is over
 * the allowed keys; the Philox indexing of the dropout is that of the calls above (it does not depend on the mask).  The
 * backward is the gradient of that forward, with P = 0 set explicitly for masked keys; the k and v parts of d_qkv at rows >= n
 * are written as exact zeros, as above.  Keep words at masked (query, key) positions are unspecified: nothing reads them.
 * Everything else of a stack is row-wise, so with the flag row t of the output of ganffn_encoder_fwd_mask is a function of input
 * rows 0 .. t alone, and finite values at later rows change no bit of it.
 * flags == 0 is exactly the _len call (same launches, same bits); key_len may be NULL with any flags; a bit other than
 * GANFFN_ATTN_CAUSAL is refused with a message and nothing is written.  Saved and workspace sizes and layouts are unchanged.  The
 * forward and the backward of one pass must be given the same flags (and lengths).  The causal kernels are instantiations of
 * their own; in the head_dim 10 / 30 family (and 60 / 64 at S <= 48) they also skip the key tiles above the diagonal.
 * The GAN step's forms (GanEngine(causal = True): generators under the mask, discriminators not):
 * ganffn_encoder_fwd_pair_mask: ganffn_encoder_fwd_pair_len with the flags word; GANFFN_ATTN_CAUSAL masks BOTH segments.  The eval
 * output has the bits of ganffn_encoder_fwd_mask(..., saved = NULL), the train output and the saved block those of
 * ganffn_encoder_fwd_mask with the same rng_offset_add and flags.
 * ganffn_encoder_bwd_parts_mask: ganffn_encoder_bwd_parts_len with the flags handed on; followed by ganffn_adam_step_parts the
 * update has the bits of ganffn_encoder_bwd_mask + ganffn_adam_step. */
#define GANFFN_ATTN_CAUSAL 1u
int ganffn_encoder_fwd_pair_mask(const ganffn_enc_cfg* cfg, const int32_t* key_len, uint32_t flags, const float* x_in,
                                 const float* pe, const float* params, float* out_eval, float* out_train, float* saved_train,
                                 float* workspace, const uint64_t* rng, uint64_t rng_offset_add_train, void* stream);
int ganffn_encoder_bwd_parts_mask(const ganffn_enc_cfg* cfg, const int32_t* key_len, uint32_t flags, float* dx,
                                  const float* params, float* grads, const float* saved, float* workspace, const uint64_t* rng,
                                  uint64_t rng_offset_add, int need_dx_in, int64_t* part_offset, int64_t* part_stride,
                                  int* n_parts, void* stream);
int ganffn_attention_fwd_mask(const float* qkv, float* o, float* lse, uint32_t* keep, const int32_t* key_len, uint32_t flags,
                              int S, int B, int E, int H, float p, uint32_t site, const uint64_t* rng,
                              uint64_t rng_offset_add, void* stream);
int ganffn_attention_bwd_mask(const float* qkv, const float* o, const float* lse, const float* d_o, const uint32_t* keep,
                              const int32_t* key_len, uint32_t flags, float* d_qkv, int S, int B, int E, int H, float p,
                              uint32_t site, const uint64_t* rng, uint64_t rng_offset_add, void* stream);
/* The general2 matching attention (N2 above) with a flags word after mask.  GANFFN_ATTN_CAUSAL: query step t attends to memory
 * steps j <= t only, a_tj = e^{s_tj} m_j [j <= t] / sum_{k <= t} e^{s_tk} m_k — MatchingAttention.forward(M[:t+1], M[t],
 * umask[:, :t+1]) for every t, the second attention of dialogue_rnn.UniModel.  alpha, tanh_s and du_ws are written completely on
 * every call, exact zeros at j > t (and alpha and du_ws at masked j); a query row at or past its dialogue's end attends over the
 * dialogue's real steps.  The causal kernels skip the work above the diagonal: a block of 16 query steps reads memory rows
 * j < min(S, t0 + 16) only, memory step j sums over t >= j only; every output element keeps a fixed summation order, no atomics.
 * flags == 0 is exactly the call above (same launches, same bits: the two entry points above forward here with 0); a bit other
 * than GANFFN_ATTN_CAUSAL, or a null pointer, is refused with a message before any launch.  The forward and the backward of one
 * pass must be given the same flags. */
int ganffn_general2_attention_fwd_mask(const float* x, const float* mem, const float* mask, uint32_t flags, float* att,
                                       float* alpha, float* tanh_s, int S, int B, int D, void* stream);
int ganffn_general2_attention_bwd_mask(const float* d_att, const float* x, const float* mem, const float* mask, uint32_t flags,
                                       const float* alpha, const float* tanh_s, float* du_ws, float* dx, float* dmem, int S,
                                       int B, int D, void* stream);
int ganffn_encoder_fwd_mask(const ganffn_enc_cfg* cfg, const int32_t* key_len, uint32_t flags, const float* x_in,
                            const float* pe, const float* params, float* out, float* saved, float* workspace,
                            const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_encoder_bwd_mask(const ganffn_enc_cfg* cfg, const int32_t* key_len, uint32_t flags, int layer_lo, int layer_hi,
                            float* dx, const float* params, float* grads, const float* saved, float* workspace,
                            const uint64_t* rng, uint64_t rng_offset_add, int need_dx_in, void* stream);
/* ---- streaming: a causal stack one utterance at a time, from per-layer K/V caches (csrc/stream.hip) ----------------------------
 * Under the causal mask the K and V of a past utterance never change and everything else of a stack is row-wise, so row t of a
 * dialogue needs only its own input row and the cached K / V of rows 0 .. t-1 in every layer.  A step takes n new rows, one per
 * active dialogue: row i belongs to cache slot slot[i] and is that dialogue's utterance number pos[slot[i]].
 * cfg here describes the CACHE: cfg->S = positions per slot (max_len, 1 .. 110), cfg->B = slots (capacity, 1 ..
 * GANFFN_MAX_DIALOGUES), cfg->train must be 0 (streaming is inference: no dropout, nothing saved), head_dim E / H even and <= 64.
 * Cache layout (the caller owns it; tests fill it directly): L layers, a4(capacity * 2 * max_len * E) floats apart (a4 = rounded
 * up to a multiple of 4), each layer [capacity][2 (K, V)][H][max_len][hd] floats with hd = E / H: the key (kv = 0) or value
 * (kv = 1) of slot s, head h, position j is the hd contiguous floats at (((s * 2 + kv) * H + h) * max_len + j) * hd.  Positions at
 * or above pos[s] are never read, so the cache needs no initialisation and a slot is reset by setting its position to 0.
 * slot [n] and pos [capacity] are int32 on the device; pos is READ ONLY here — advancing it (pos[slot[i]] += 1 after the last stack
 * of a step) is the caller's job, so several stacks can step from the same positions.  The slots of one call must be distinct.
 * A row whose slot is outside [0, capacity) or whose position is outside [0, max_len) is skipped by the attention step (its
 * attention output is a zero row, its positional-encoding sum a zero row, the cache is untouched) and nothing is accessed out of
 * range; its `out` row is then meaningless.
 * The step is the launch sequence of the forward at T = n rows with two launches swapped: the positional encoding is a gather by
 * position (plus layer 0's in-proj GEMM), the attention core is the single-query kernel.  Every rule that picks a summation
 * order (split-K factors, K chunks of the 2048 -> 100 product) is evaluated for T = n, so a step's values agree with the rows of
 * the full causal forward over the dialogue to rounding, NOT bit for bit.  The bits of a row depend on no other row of the call.
 * x, out [n x E]; pe [>= max_len x E]; workspace: the _workspace_floats of n_max >= n.  The attention call alone (a unit-test
 * hook) takes one layer's cache and this step's in-proj output qkv [n x 3E], and writes o [n x E]. */
int64_t ganffn_stream_cache_floats(const ganffn_enc_cfg* cfg);
int64_t ganffn_stream_workspace_floats(const ganffn_enc_cfg* cfg, int n_max);
int ganffn_encoder_stream_step(const ganffn_enc_cfg* cfg, int n, const int32_t* slot, const int32_t* pos, const float* x,
                               const float* pe, const float* params, float* cache, float* out, float* workspace, void* stream);
int ganffn_stream_attention(const float* qkv, float* cache_layer, const int32_t* slot, const int32_t* pos, float* o, int n,
                            int capacity, int max_len, int E, int H, void* stream);
/* ---- stream prefill: several new utterances per dialogue in one call (csrc/stream.hip) ---------------------------------------
 * The same caches, slots and positions as the step above, but chunk i of a call holds count[i] new rows of the dialogue in slot
 * slot[i], at positions t .. t + count[i] - 1 with t = pos[slot[i]]: a dialogue joined under way, caches rebuilt after the
 * weights changed, utterances that arrive in bursts.  x and out are [m][n][E], TIME-MAJOR (row j of chunk i is row j * n + i), so
 * a padded [S, B, E] batch passes straight in; m is the longest chunk's room, 1 <= m <= max_len, and count[i] <= m.
 * Row j < count[i] attends with its Q over the cached keys 0 .. t-1 and the chunk's own keys 0 .. j (scale 1 / sqrt(hd), softmax,
 * P V): what j + 1 consecutive steps compute.  The K and V of rows 0 .. count[i]-1 are written to every layer's cache at
 * t .. t + count[i] - 1 as bit copies; new keys and values are taken from the call's own rows, never read back from the cache.
 * slot, count [n] and pos [capacity] are int32 on the device; pos is READ ONLY — pos[slot[i]] += count[i] after the last stack of a
 * call is the caller's job.  The slots of one call must be distinct.
 * SKIP: a chunk whose slot is outside [0, capacity), whose position is negative, whose count is negative or above m, or with
 * pos + count > max_len is skipped WHOLE: the cache is untouched.  count = 0 writes nothing either.  For every chunk the attention
 * output and the positional-encoding sum of rows j >= count[i] (all m rows of a skipped chunk) are zero rows; their x rows are
 * read by no launch that could carry them into a valid row or into the cache, but they run through the row-wise launches
 * (LayerNorm, FFN), so x must be FINITE there and their `out` rows are meaningless.  Cache words at or above a position are never
 * read, and nothing is accessed out of range whatever slot / count / pos hold.
 * The call is the launch sequence of the forward at T = m * n rows with the same two launches swapped, so its values agree with
 * consecutive steps and with the full causal forward to rounding, NOT bit for bit.  The bits of a chunk's rows depend neither on
 * the other chunks of the call nor on the chunk's column i.  No atomics; every summation order is fixed.
 * Workspace: ganffn_stream_extend_workspace_floats(cfg, rows_max) serves every call with m * n <= rows_max (rows_max >= 1); a
 * call with more rows, or with workspace_floats below what its rows_max = m * n needs, is refused with a message that names the
 * number.  The attention call alone (a unit-test hook) takes one layer's cache, qkv [m][n][3E] and writes o [m][n][E]. */
int64_t ganffn_stream_extend_workspace_floats(const ganffn_enc_cfg* cfg, int rows_max);
int ganffn_encoder_stream_extend(const ganffn_enc_cfg* cfg, int n, int m, const int32_t* slot, const int32_t* count,
                                 const int32_t* pos, const float* x, const float* pe, const float* params, float* cache,
                                 float* out, float* workspace, int64_t workspace_floats, void* stream);
int ganffn_stream_attention_chunk(const float* qkv, float* cache_layer, const int32_t* slot, const int32_t* count,
                                  const int32_t* pos, float* o, int n, int m, int capacity, int max_len, int E, int H,
                                  void* stream);
/* ---- streaming: the causal DialogueRNN classifier head one utterance at a time (csrc/drnn_stream.hip) ---------------------------
 * The head of GAN_FFN_DialogueRNN(causal=True) (dialogue_rnn.UniModel) next to the streamed generators above: everything a
 * recurrence step needs from the past is the global history, the party states and the emotion history, kept as per-slot STATE.
 * slot [n], pos [capacity], count [n], spk int32 on the device, with the meaning they have above; pos is READ ONLY (the caller
 * advances it after the last consumer of a step); the slots of one call must be distinct.
 * State layout (the caller owns it; tests fill it directly): three regions back to back, each rounded up to a multiple of 4 floats:
 *   G [capacity][max_len][H]    global history: g_j of slot s is the H floats at (s * max_len + j) * H
 *   Q [capacity][parties][H]    party states
 *   E [capacity][max_len][He]   emotion history; E[s][t-1] is the emotion cell's recurrent state
 * Words of G and E at or above a slot's position are never read, and at position 0 the step takes g_prev, every party row and
 * e_prev as zeros WITHOUT reading the state: it needs no initialisation and a slot is reset by setting its position to 0.
 * ganffn_drnn_stream_step: row i (U [n x Dm], spk[i] in [0, parties)) is utterance t = pos[slot[i]] + off of the dialogue in slot
 * slot[i]; a plain step passes off = 0, count = NULL; with count given row i takes part only if off < count[i].  It computes
 * DialogueRNNCell.forward for one real utterance (m = 1) in eval mode — the g cell on [U, q[spk]] and g_{t-1}; the context
 * attention of the configured type over G[s][0 .. t-1] (c = 0 at t = 0); the party cell for the speaker's row; with `listener` the
 * listener cell for every party row, then the blend; the e cell — and writes G[s][t], all `parties` rows of Q[s], E[s][t] and
 * e_out[i] = e_t ([n x He]).  prm->att_w is ignored: the attention's parameters are aprm (ONE struct; NULL for dot), lprm is the
 * listener's (NULL without).  Inference only: no dropout, nothing saved, no atomics, every summation order fixed; the bits of a
 * row depend on no other row of the call.  7 launches (more product launches with listener state and more than 2 parties).
 * SKIP: a row whose slot is outside [0, capacity), whose position is negative, whose t is outside [0, max_len), whose spk is
 * outside [0, parties) or that count masks: the state is untouched and e_out[i] is a zero row; nothing is accessed out of range
 * whatever the index arrays hold.
 * Refused with a message before any launch: null or misaligned pointers, n outside [1, capacity], widths outside the limits, dot
 * with Dm != H, concat D_a outside its limits, missing attention or listener tensors.
 * ganffn_drnn_stream_extend: the step m times with off = 0 .. m-1 on time-major rows (spk [m][n], U [m][n][Dm], e_out [m][n][He]),
 * count [n] required, no host synchronisation: 7 launches per chunk step.
 * workspace: ganffn_drnn_stream_workspace_floats(cfg, n_max >= n), n_max <= capacity. */
typedef struct ganffn_drnn_stream_cfg {
    int32_t capacity, max_len;   /* slots (1 .. GANFFN_MAX_DIALOGUES), positions per slot (1 .. 110) */
    int32_t parties;             /* 1 .. GANFFN_DRNN_MAX_PARTIES */
    int32_t Dm, H, He;           /* as ganffn_drnn_cfg: multiples of 4, H <= 512 */
    int32_t listener;            /* 0 / 1 */
    ganffn_drnn_att att;         /* every GANFFN_DRNN_ATT_* type, under the rules of ganffn_drnn_att_* */
} ganffn_drnn_stream_cfg;
int64_t ganffn_drnn_stream_state_floats(const ganffn_drnn_stream_cfg* cfg);
int64_t ganffn_drnn_stream_workspace_floats(const ganffn_drnn_stream_cfg* cfg, int n_max);
int ganffn_drnn_stream_step(const ganffn_drnn_stream_cfg* cfg, int n, const int32_t* slot, const int32_t* pos, int off,
                            const int32_t* count, const int32_t* spk, const float* U, const ganffn_drnn_params* prm,
                            const ganffn_drnn_listener_params* lprm, const ganffn_drnn_att_params* aprm, float* state,
                            float* e_out, float* workspace, void* stream);
int ganffn_drnn_stream_extend(const ganffn_drnn_stream_cfg* cfg, int n, int m, const int32_t* slot, const int32_t* count,
                              const int32_t* pos, const int32_t* spk, const float* U, const ganffn_drnn_params* prm,
                              const ganffn_drnn_listener_params* lprm, const ganffn_drnn_att_params* aprm, float* state,
                              float* e_out, float* workspace, void* stream);
/* The second (general2) attention of new rows over a slot's emotion history.  x, att [m][n][D] time-major; x is the caller's
 * transform(e) of the new rows; e_hist is the state's E region, which ALREADY HOLDS the new rows.  Row (j, i) with j < count[i]
 * (count = NULL: 1 each) attends over E[s][0 .. pos[s] + j], s = slot[i]: alpha_k = softmax_k(tanh(<x, e_k>)), att = sum_k alpha_k
 * e_k — the causal row of ganffn_general2_attention_fwd_mask with an all-ones mask.  alpha [m][n][max_len] may be NULL; it is exact
 * zeros past the row's last memory step.  D a multiple of 4, <= 1024.  A row whose slot is outside [0, capacity), whose position is
 * negative, whose pos + j is at or above max_len, or with j >= count[i] is skipped: zero rows; nothing is read out of range. */
int ganffn_general2_stream_attention(const float* x, const float* e_hist, const int32_t* slot, const int32_t* count,
                                     const int32_t* pos, float* att, float* alpha, int n, int m, int capacity, int max_len, int D,
                                     void* stream);
/* ---- streaming: the causal MELD classifier's LSTM one utterance at a time (csrc/lstm_stream.hip) -------------------------------
 * nn.LSTM(In, H, num_layers = L, bidirectional = False) in eval mode (the recurrence of MELDLSTMModel(causal=True)): everything a
 * step needs from the past is (h, c) of every layer, kept as per-slot STATE next to the emotion history that
 * ganffn_general2_stream_attention reads.  slot [n], pos [capacity], count [n] int32 on the device, with the meaning they have
 * above; pos is READ ONLY (the caller advances it after the last consumer of a step); the slots of one call must be distinct.
 * State layout (the caller owns it; tests fill it directly): three regions back to back, each rounded up to a multiple of 4 floats:
 *   Hs [capacity][L][H]         h of every layer after the slot's last step: layer l of slot s at (s * L + l) * H
 *   Cs [capacity][L][H]         c of every layer
 *   E  [capacity][max_len][H]   emotion history: E[s][t] = the last layer's h_t (the same bits as Hs[s][L-1] after step t)
 * Words of E at or above a slot's position are never read, and at t = 0 every layer's h_prev and c_prev are taken as zeros WITHOUT
 * reading the state: it needs no initialisation and a slot is reset by setting its position to 0.
 * ganffn_stream_lstm_step: row i of x [n x In] is utterance t = pos[slot[i]] + off of the dialogue in slot slot[i]; a plain step
 * passes off = 0, count = NULL; with count given row i takes part only if off < count[i].  It computes torch's LSTM cell (gate
 * order i, f, g, o) for the L layers in turn with w_ih[l] [4H x In or H], w_hh[l] [4H x H], b_ih[l], b_hh[l] [4H] (host arrays of
 * L device pointers, weights 16-byte aligned) and writes Hs[s], Cs[s], E[s][t] and e_out[i] = the last layer's h_t ([n x H]).
 * Inference only: nothing saved, no atomics, every summation order fixed; the bits of a row depend on no other row of the call.
 * 2 L + 1 launches at L <= 7: gather, the L recurrent products and layer 0's input product in one launch, then per layer a gate
 * launch and (but for the last) the next layer's input product.
 * SKIP: a row whose slot is outside [0, capacity), whose position is negative, whose t is outside [0, max_len) or that count
 * masks: the state is untouched and e_out[i] is a zero row; nothing is accessed out of range whatever the index arrays hold.
 * Refused with a message before any launch (the size functions return a negative value): null or misaligned pointers, n outside
 * [1, capacity], m outside [1, max_len], capacity outside [1, GANFFN_MAX_DIALOGUES], max_len outside [1, 110], In or H not a
 * multiple of 4, H > 1024, L outside [1, 16], n_max > capacity.
 * ganffn_stream_lstm_extend: the step m times with off = 0 .. m-1 on time-major rows (x [m][n][In], e_out [m][n][H]), count [n]
 * required, no host synchronisation; the state it leaves is bit for bit that of the m step calls.
 * workspace: ganffn_stream_lstm_workspace_floats(cfg, n_max >= n), n_max <= capacity. */
typedef struct ganffn_stream_lstm_cfg {
    int32_t capacity, max_len;   /* slots (1 .. GANFFN_MAX_DIALOGUES), positions per slot (1 .. 110) */
    int32_t In, H, L;            /* input and hidden widths (multiples of 4, H <= 1024), layers (1 .. 16) */
} ganffn_stream_lstm_cfg;
int64_t ganffn_stream_lstm_state_floats(const ganffn_stream_lstm_cfg* cfg);
int64_t ganffn_stream_lstm_workspace_floats(const ganffn_stream_lstm_cfg* cfg, int n_max);
int ganffn_stream_lstm_step(const ganffn_stream_lstm_cfg* cfg, int n, const int32_t* slot, const int32_t* pos, int off,
                            const int32_t* count, const float* x, const float* const* w_ih, const float* const* w_hh,
                            const float* const* b_ih, const float* const* b_hh, float* state, float* e_out, float* workspace,
                            void* stream);
int ganffn_stream_lstm_extend(const ganffn_stream_lstm_cfg* cfg, int n, int m, const int32_t* slot, const int32_t* count,
                              const int32_t* pos, const float* x, const float* const* w_ih, const float* const* w_hh,
                              const float* const* b_ih, const float* const* b_hh, float* state, float* e_out, float* workspace,
                              void* stream);
/* z = x + drop(y); xhat = (z-mean)*rstd; out = xhat*w + b   (norm1/norm2 of the encoder layer).  Accepted: T >= 1 and
 * 1 <= E <= 640, a multiple of 4 or not; a wider row is refused with a message.  The variance is the two-pass one (mean
 * of the squared deviations), so a row mean far above the row's spread costs no more than fp32 rounding of z itself. */
int ganffn_add_dropout_layernorm_fwd(const float* x, const float* y, const float* w, const float* b,
                                     float* out, float* xhat, float* rstd, int T, int E, float eps,
                                     float p, uint32_t site, const uint64_t* rng,
                                     uint64_t rng_offset_add, void* stream);
/* d_out -> dz (residual branch) and dy = drop_bwd(dz); gw/gb accumulated when non-NULL */
int ganffn_add_dropout_layernorm_bwd(const float* d_out, const float* xhat, const float* rstd,
                                     const float* w, float* dz, float* dy, float* gw, float* gb, int T,
                                     int E, float p, uint32_t site, const uint64_t* rng,
                                     uint64_t rng_offset_add, void* stream);
/* out = keep ? x/(1-p) : 0 over a [R x C] tensor (Philox contract) — test hook for the mask layout */
int ganffn_dropout(const float* x, float* out, int R, int C, float p, uint32_t site,
                   const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* [T x K] x [K x 100] with a long K (linear2 forward / linear1 dgrad of the d_model-100 feed-forward block,
 * csrc/gemm_n100.hip): K is cut into *n_slabs (<= max_slabs <= 16) chunks, chunk z writes its partial product to
 * slabs + z * slab_stride ([T x 100], plain stores); the consumer adds the slabs in order (no atomics).  w_kmajor = 0:
 * W is [100 x K] (rows of K: out = A W^T), 1: W is [K x 100] (out = A W).  bias [100] (or NULL) is added by chunk 0.
 * K % 32 == 0, K >= 256. */
int ganffn_gemm_n100(const float* A, const float* W, int w_kmajor, const float* bias, float* slabs, int64_t slab_stride,
                     int T, int K, int max_slabs, int* n_slabs, void* stream);

/* Test / measurement hook: the generic 64 x 64-tile GEMM kernel exactly as the encoder stack launches it for the layers that
 * have no specialised kernel (the d_model-512 generator, nn.Linear call sites model.py:1244-1252 via torch's
 * TransformerEncoderLayer).  mode 0: C = A[M x K] W[N x K]^T, mode 1: C = A[M x K] W[K x N].  epi 0: + bias; 1: bias + ReLU +
 * dropout (linear1); 3: C = acc * (aux > 0 ? 1/(1-p) : 0) (dgrad through ReLU + dropout, aux = the saved activation [M x N]).
 * epi 0 with aux != NULL: C = A W + bias + aux, aux [M x N] — the fused residual / branch add that ganffn_encoder_bwd, the
 * LSTM and the DialogueRNN backward rely on.  epi 3 tests aux > 0 as IEEE does (a positive subnormal counts as positive, +0 and
 * -0 do not), the same predicate as the 1-bit pattern of ganffn_ffn_k100_hook, which is taken from the bits of the activation.
 * max_slabs > 1 with epi 0: K is split the way the encoder splits few-tile long-K products, slab z at C + z * slab_stride,
 * *n_slabs = slabs written (their sum is the product; bias and aux are added into slab 0 only; slabs at index *n_slabs and
 * above are not touched).  bench.py replays one iteration's launch mix through it. */
int ganffn_gemm_hook(int mode, int epi, const float* A, const float* W, const float* bias, const float* aux, float* C,
                     int64_t slab_stride, int M, int N, int K, float p, uint32_t site, const uint64_t* rng,
                     uint64_t rng_offset_add, int train, int max_slabs, int* n_slabs, void* stream);

/* ---- N4: one bidirectional LSTM layer (csrc/lstm.hip) -----------------------------------------------------------------
 * Replaces the recurrence of `nn.LSTM(input_size, hidden_size, num_layers = 4, bidirectional = True, dropout = p)` inside
 * MELDLSTMModel (/root/reference/model.py:520-562; built at /root/reference/train_MELD.py:147-151 with D_m = 600, D_e = 300),
 * one layer per call (the caller applies the inter-layer dropout and chains four calls).  x [S x B x In] padded, no mask (the
 * reference hands nn.LSTM the padded batch: model.py:546); out [S x B x 2H] = [h forward | h reverse]; torch's gate order
 * i, f, g, o: w_ih[d] [4H x In], w_hh[d] [4H x H], b_ih[d], b_hh[d] [4H], d = 0 forward, 1 reverse.  B <= 32 per call.
 * saved (ganffn_lstm_saved_floats): activated gates and cell states of every step, read by the backward;
 * workspace (ganffn_lstm_workspace_floats) is scratch.  The backward ACCUMULATES (+=) into gw_* / gb_* (any of them, or an
 * array, may be NULL) and writes dx [S x B x In] (NULL: not wanted).  Deterministic: no atomics. */
typedef struct ganffn_lstm_cfg {
    int32_t S, B, In, H;
} ganffn_lstm_cfg;
int64_t ganffn_lstm_saved_floats(const ganffn_lstm_cfg* cfg);
int64_t ganffn_lstm_workspace_floats(const ganffn_lstm_cfg* cfg);
int ganffn_lstm_layer_fwd(const ganffn_lstm_cfg* cfg, const float* x, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                          void* stream);
int ganffn_lstm_layer_bwd(const ganffn_lstm_cfg* cfg, const float* d_out, const float* x, const float* out,
                          const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                          float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                          float* workspace, void* stream);

/* ---- N4: the whole LSTM stack in one call (csrc/lstm.hip) ---------------------------------------------------------------
 * `nn.LSTM(In, H, num_layers = L, bidirectional = True, dropout = p)` of MELDLSTMModel (/root/reference/model.py:531,546; built
 * at /root/reference/train_MELD.py:147-151 with L = 4): the L per-layer bodies above chained, with the dropout nn.LSTM applies to
 * the output of every layer but the last (train != 0, p > 0) inside the library: Philox {seed, offset} contract, one call per
 * layer l with site 64 + l and offset rng_offset_add + l, rows = tokens, columns = 2H — the same launches, hence the same
 * bits, as ganffn_lstm_layer_* and ganffn_dropout issued one by one.  Weight and gradient pointers are arrays of [L][2]
 * (layer-major; d = 0 forward, 1 reverse): w_ih[2 l + d] is [4H x In] for l = 0 and [4H x 2H] above.  saved
 * (ganffn_lstm_stack_saved_floats) holds every layer's gates and cell states and the outputs between the layers; workspace
 * (ganffn_lstm_stack_workspace_floats) is scratch.  The backward regenerates the masks from the same {rng, rng_offset_add},
 * ACCUMULATES (+=) into gw_* / gb_* (arrays or entries may be NULL) and writes dx [S x B x In] (NULL: not wanted). */
typedef struct ganffn_lstm_stack_cfg {
    int32_t S, B, In, H, L;
    float p;
    int32_t train;
} ganffn_lstm_stack_cfg;
int64_t ganffn_lstm_stack_saved_floats(const ganffn_lstm_stack_cfg* cfg);
int64_t ganffn_lstm_stack_workspace_floats(const ganffn_lstm_stack_cfg* cfg);
int ganffn_lstm_stack_fwd(const ganffn_lstm_stack_cfg* cfg, const float* x, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                          const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_lstm_stack_bwd(const ganffn_lstm_stack_cfg* cfg, const float* d_out, const float* x, const float* out,
                          const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                          float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                          float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* ---- N4: the LSTM recurrence on up to GANFFN_MAX_DIALOGUES dialogues per call (csrc/lstm.hip) -------------------------------
 * The four ganffn_lstm_* and the four ganffn_lstm_stack_* entry points above (nn.LSTM of MELDLSTMModel, /root/reference/model.py:
 * 531,546, under train_MELD.py:114's --batch-size) with 1 <= cfg->B <= GANFFN_MAX_DIALOGUES instead of 32: same arguments, same
 * layouts and sizes as functions of B, still one product launch and one gate launch per step and direction pair.  At B <= 32
 * every call is the same launch sequence as its namesake above, bit for bit; B = 0 or B > GANFFN_MAX_DIALOGUES is an argument
 * error reported through ganffn_last_error (the size functions return a negative value). */
int64_t ganffn_lstm_batch_saved_floats(const ganffn_lstm_cfg* cfg);
int64_t ganffn_lstm_batch_workspace_floats(const ganffn_lstm_cfg* cfg);
int ganffn_lstm_batch_layer_fwd(const ganffn_lstm_cfg* cfg, const float* x, const float* const* w_ih, const float* const* w_hh,
                                const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                                void* stream);
int ganffn_lstm_batch_layer_bwd(const ganffn_lstm_cfg* cfg, const float* d_out, const float* x, const float* out,
                                const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                float* workspace, void* stream);
int64_t ganffn_lstm_stack_batch_saved_floats(const ganffn_lstm_stack_cfg* cfg);
int64_t ganffn_lstm_stack_batch_workspace_floats(const ganffn_lstm_stack_cfg* cfg);
int ganffn_lstm_stack_batch_fwd(const ganffn_lstm_stack_cfg* cfg, const float* x, const float* const* w_ih, const float* const* w_hh,
                                const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                                const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_lstm_stack_batch_bwd(const ganffn_lstm_stack_cfg* cfg, const float* d_out, const float* x, const float* out,
                                const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream);

/* ---- N4: the LSTM recurrence on packed sequences (csrc/lstm.hip) -------------------------------------------------------------
 * An extension the reference does not have (model.py:546 hands nn.LSTM the padded batch): what
 * pack_padded_sequence -> nn.LSTM -> pad_packed_sequence(total_length = S) computes, on the padded layout.  The arguments are
 * those of ganffn_lstm_batch_layer_* / ganffn_lstm_stack_batch_* with `lengths` after cfg: int32 [B] on the device, lengths[b] =
 * the number of real steps of dialogue b (<= 0: an empty dialogue; > S: taken as S).  It is only ever compared with a time index,
 * never used as an index, and never read by the host.  The rule, in BOTH directions, for dialogue b at time index tm >= lengths[b]:
 *   forward:  c_t = 0; h_t = 0, written into out[tm]; the saved activated gates are 0 — whatever the products computed for that
 *             row is discarded by a select;
 *   backward: dG = 0 for all four gates and the dc handed to the earlier step is 0, whatever dh / d_out hold there — a select,
 *             not a product with 0, so junk (NaN included) in d_out at padded positions cannot spread.
 * At tm < lengths[b] the arithmetic is that of the unpacked entry points.  So the reverse direction enters step lengths[b] - 1
 * with zero state, out is 0 past a dialogue's end, the inter-layer dropout of those rows is 0, the weight, bias and input
 * gradients see zero dG rows at padded tokens (dx is 0 there), and with every length >= S the results are the unpacked entry
 * points' bit for bit.  Contract on x: FINITE at padded positions (the project's collate and ganffn_batch_gather write zeros);
 * its values there change no result.  1 <= cfg->B <= GANFFN_MAX_DIALOGUES; sizes from ganffn_lstm_batch_*_floats /
 * ganffn_lstm_stack_batch_*_floats, layouts unchanged; the same launches per step as the unpacked calls.  A null `lengths` is an
 * argument error reported through ganffn_last_error. */
int ganffn_lstm_packed_layer_fwd(const ganffn_lstm_cfg* cfg, const int32_t* lengths, const float* x, const float* const* w_ih,
                                 const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                                 float* saved, float* workspace, void* stream);
int ganffn_lstm_packed_layer_bwd(const ganffn_lstm_cfg* cfg, const int32_t* lengths, const float* d_out, const float* x,
                                 const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                                 float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                                 const float* saved, float* workspace, void* stream);
int ganffn_lstm_stack_packed_fwd(const ganffn_lstm_stack_cfg* cfg, const int32_t* lengths, const float* x,
                                 const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                                 const float* const* b_hh, float* out, float* saved, float* workspace, const uint64_t* rng,
                                 uint64_t rng_offset_add, void* stream);
int ganffn_lstm_stack_packed_bwd(const ganffn_lstm_stack_cfg* cfg, const int32_t* lengths, const float* d_out, const float* x,
                                 const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                                 float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                                 const float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add,
                                 void* stream);

/* ---- N4: the LSTM recurrence with ONE direction (csrc/lstm.hip) ------------------------------------------------------------
 * An extension the reference does not have (its LSTM is bidirectional: model.py:531): `nn.LSTM(In, H, num_layers = L,
 * bidirectional = False, dropout = p)` — the forward direction alone, so out[t] depends on x[0 .. t] only; what the causal MELD
 * classifier (MELDLSTMModel(causal=True)) is built on.  The same drivers, kernels and layouts as the entry points above with a
 * direction count of 1 instead of 2: out / d_out [S x B x H], layer l > 0 reads an H-wide input, the inter-layer dropout draws
 * over [S B x H] (site 64 + l, offset rng_offset_add + l), the weight and gradient pointers are arrays of [1] (layer calls) or
 * [L][1] (stack calls: entry l = layer l), and a step stays one skinny product launch (one problem) + one gate launch in either
 * pass.  With the same forward-direction weights, out is bit for bit the forward half of the bidirectional layer's out.
 * ONE family for the padded and the packed run: `lengths` after cfg is int32 [B] on the device with the packed entry points'
 * rule (above) or NULL: every dialogue runs all S steps.  1 <= cfg->B <= GANFFN_MAX_DIALOGUES; the refusals are those of the
 * other families (In, H multiples of 4; L in 1 .. 16; p in [0, 1); no null pointer; 16-byte alignment; rng in train mode with
 * dropout).  saved / workspace sizes from the four *_floats functions below (-1 for a refused cfg). */
int64_t ganffn_unilstm_saved_floats(const ganffn_lstm_cfg* cfg);
int64_t ganffn_unilstm_workspace_floats(const ganffn_lstm_cfg* cfg);
int ganffn_unilstm_layer_fwd(const ganffn_lstm_cfg* cfg, const int32_t* lengths, const float* x, const float* const* w_ih,
                             const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                             float* saved, float* workspace, void* stream);
int ganffn_unilstm_layer_bwd(const ganffn_lstm_cfg* cfg, const int32_t* lengths, const float* d_out, const float* x,
                             const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                             float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                             const float* saved, float* workspace, void* stream);
int64_t ganffn_unilstm_stack_saved_floats(const ganffn_lstm_stack_cfg* cfg);
int64_t ganffn_unilstm_stack_workspace_floats(const ganffn_lstm_stack_cfg* cfg);
int ganffn_unilstm_stack_fwd(const ganffn_lstm_stack_cfg* cfg, const int32_t* lengths, const float* x, const float* const* w_ih,
                             const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                             float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream);
int ganffn_unilstm_stack_bwd(const ganffn_lstm_stack_cfg* cfg, const int32_t* lengths, const float* d_out, const float* x,
                             const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                             float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                             const float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add,
                             void* stream);

/* ---- N4: the MELD classifier's head (csrc/meld_head.hip) ------------------------------------------------------------------
 * Replaces `hidden = F.hardswish(emotions + F.hardswish(att_emotions))` and `self.smax_fc(hidden)` of MELDLSTMModel.forward
 * (/root/reference/model.py:553-560, the att2 branch /root/reference/train_MELD.py:71 runs) and autograd's backward of them.
 * emotions, att [T x D] (token t = s*B+b), w_fc [C x D], b_fc [C]; D a multiple of 4 and <= 1024, C <= 16.
 * fwd writes hidden [T x D] (the weight gradient reads it) and logits [T x C].
 * bwd: d_emotions = dlogits w_fc * hsw'(u) (the residual path alone: the attention's paths are the caller's), d_att = that *
 * hsw'(att), u recomputed from emotions and att; gw_fc / gb_fc are ACCUMULATED (+=) in a fixed order (gb_fc may be NULL).
 * hsw' as torch: 0 for x <= -3, 1 for x >= 3, x / 3 + 0.5 between.  One launch each; deterministic, no atomics. */
int ganffn_meld_head_fwd(const float* emotions, const float* att, const float* w_fc, const float* b_fc, float* hidden,
                         float* logits, int T, int D, int C, void* stream);
int ganffn_meld_head_bwd(const float* dlogits, const float* emotions, const float* att, const float* hidden, const float* w_fc,
                         float* d_emotions, float* d_att, float* gw_fc, float* gb_fc, int T, int D, int C, void* stream);

/* n floats of zeros, in stream order: the gradient slab of a step runner before a backward that accumulates into it (the
 * `optimizer.zero_grad()` of /root/reference/train_MELD.py:63 for engine.MeldEngine's slab). */
int ganffn_zero_floats(float* p, int64_t n, void* stream);

/* Measurement hook: the K = 100 -> 2048 products of the d_model-100 feed-forward block (csrc/gemm.hip gemm_wres_kernel) with the
 * arguments ganffn_encoder_fwd / _bwd give them (linear1 / linear2 of nn.TransformerEncoderLayer, call sites model.py:1210,1307).
 * which 0: out[T x 2048] = dropout_p(relu(a[T x 100] w[2048 x 100]^T + bias)); hmask != NULL: also the 1-bit [out > 0] pattern
 *          (ceil(T/32) * 2048 floats) a saved pass leaves for the backward.  Only the bits of rows < T are specified: when
 *          T % 32 != 0 the bits of rows >= T in the last row tile hold whatever the padded rows computed.
 * which 1: out[T x 2048] = (a[T x 100] w[100 x 2048]) * pattern / (1-p) — the linear2 dgrad; pattern from hmask when given,
 *          else from h_saved [T x 2048] > 0. */
int ganffn_ffn_k100_hook(int which, const float* a, const float* w, const float* bias, float* out, void* hmask,
                         const float* h_saved, int T, float p, uint32_t site, const uint64_t* rng, uint64_t rng_offset_add,
                         int train, void* stream);

/* A/B measurement hook (process-wide), a bit mask; 0 = the default path.  It is the library's ONLY mutable process state besides
 * the per-(kernel, device) "LDS opt-in done" masks: one 32-bit word held in a relaxed atomic (csrc/common.h `Mode`); every entry
 * point takes one snapshot of it per call, so a setter racing with a launch makes that launch take one path or the other, never
 * a mixture.  Bits 8..23 are lab knobs (forced tile / chunk counts), the others select an older or alternative launch
 * sequence that stays parity-tested. */
/*
 *   bits 0, 7, 22: reserved, ignored (until round 5 they selected the fused feed-forward kernels ffn.hip / ffn3.hip: measured
 *          slower in the step three times over and removed from the product; the kernels are in the history);
 *   bit 1: run the token-local chains around the LayerNorms of a d_model-100 layer (out-proj + LN1, LN2 + next in-proj and
 *          their backward mirrors, csrc/rowchain.hip) as separate GEMM + LayerNorm launches;
 *   bit 2: run the [T x 2048] x [2048 x 100] products on the generic 64 x 64 tiles instead of csrc/gemm_n100.hip;
 *   bit 3: run the grouped weight-gradient launch of a d_model-100 pass on the generic 64 x 64 tiles instead of
 *          csrc/gemm_tn100.hip;
 *   bit 4: csrc/gemm_tn100.hip adds its partial slabs in the kernel's last-arriving workgroup per tile instead of in a second
 *          launch (same bits; measured slower: the device-scope fences cost more than the launch);
 *   bit 5: run the discriminator head as separate GELU / GEMM / tail launches instead of csrc/disc_head.hip;
 *   bit 6: run the head of a d_model-100 encoder stack (positional encoding + dropout, layer 0's in-proj) as two launches
 *          instead of one (csrc/rowchain.hip);
 *   bits 8..15: forced K-chunk count of csrc/gemm_n100.hip (0 = choose; clamped to the caller's slab capacity);
 *   bits 16..19: forced token-chunk count of csrc/gemm_tn100.hip (0 = choose; clamped to 8 and to the workspace);
 *   bits 20..21: csrc/gemm_n100.hip with 4 (value 1) or 8 (value 2) waves per workgroup (0 = choose);
 *   bit 23: csrc/gemm_n100.hip and csrc/gemm_tn100.hip with rows 96..99 of the 100-wide dimension on a padded seventh 16-row
 *           MFMA tile (round 3's form) instead of v_mfma_f32_4x4x1_16B_f32 (measured: the step 34.4 -> 33.75 ms without it).
 *   bit 24: run the out-proj of the wide (d_model != 100) stacks unsplit instead of as two K halves summed by the LayerNorm kernel;
 *   bit 25: the linear2 dgrad takes its ReLU / dropout pattern from the saved hidden activation instead of the 1-bit copy that
 *           linear1's epilogue leaves beside it in the saved block (same predicate, same bits; 24.6 MB less to read per layer
 *           at the headline size).
 *   bit 28: ganffn_encoder_bwd_parts_supported() answers 0: weight gradients always go through the reduce launch (same bits).
 * Every combination is parity-tested; results agree to rounding.  The switch must not change between a forward pass and
 * the backward pass that consumes its saved block. */
int ganffn_debug_set_ffn_mode(int bits);

/* ---- the epoch loop with the corpus resident on the device (csrc/batch.hip) ---------------------------------------------------
 * The packed corpus of one split: per feature column (and the speaker one-hots) one fp32 matrix [n_rows x width], the
 * dialogues back to back; labels_src [n_rows] int64; row0 [n_dialogues + 1] int64, dialogue d owning rows row0[d] .. row0[d+1]-1.
 *
 * ganffn_batch_gather: ONE launch builds the padded batch of the dialogues idx[0 .. B-1] (int32, on the device), what
 *   dataloader.py:55-58's pad_sequence collate builds on the host: every column k seq-first cols[k].dst [S x B x width],
 *   umask [B x S] fp32 (1 on real utterances), label [B x S] int64.  Every output element is written: steps s >= the dialogue's
 *   length are zeros.  A dialogue longer than S gives its first S rows; an index outside [0, n_dialogues), or a row range of
 *   row0 outside [0, n_rows], is an empty dialogue — nothing outside the operands is read or written, whatever idx holds.
 *   `cols` is a HOST array of n_cols (1 .. GANFFN_BATCH_MAX_COLS) descriptors, copied into the launch; a column whose width is a
 *   multiple of 4 moves 16 bytes per lane and needs 16-byte aligned src and dst, any other width moves single floats.
 *   1 <= S <= 4096, 1 <= B <= GANFFN_MAX_DIALOGUES.
 * ganffn_epoch_record: ONE launch per step appends the step's results to the epoch buffers at `offset` (elements; offset +
 *   B S <= capacity): preds_out = argmax over the C (<= 16) classes of log_prob [S x B x C] in the batch-major flattening
 *   i = b S + s of train_IEMOCAP.py:154,158 (ties: the lowest class), labels_out / masks_out = label / umask [B x S] as they are;
 *   and loss_out[step] = loss[0], count_out[step] = the sum of umask (exact in any order: zeros and ones below 2^24; added in a
 *   fixed order, no atomics), 0 <= step < n_steps.  The host reads the five buffers once per epoch. */
#define GANFFN_BATCH_MAX_COLS 4
typedef struct ganffn_batch_col {
    const float* src;    /* [n_rows x width] */
    float* dst;          /* [S x B x width] */
    int32_t width;
} ganffn_batch_col;
int ganffn_batch_gather(const ganffn_batch_col* cols, int n_cols, const int64_t* labels_src, const int64_t* row0, int64_t n_rows,
                        const int32_t* idx, float* umask, int64_t* label, int S, int B, int n_dialogues, void* stream);
int ganffn_epoch_record(const float* log_prob, const int64_t* label, const float* umask, const float* loss, int S, int B, int C,
                        int64_t* preds_out, int64_t* labels_out, float* masks_out, int64_t offset, int64_t capacity,
                        float* loss_out, float* count_out, int step, int n_steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GANFFN_H */
