// lstm.hip — one BIDIRECTIONAL LSTM layer, forward and backward: the recurrence of
// `nn.LSTM(input_size, hidden_size, num_layers=4, bidirectional=True, dropout=p)` inside MELDLSTMModel
// (/root/reference/model.py:520-562, constructed at /root/reference/train_MELD.py:147-151 with D_m = 600, D_e = 300) on padded
// (seq_len, batch, features) tensors — the reference hands the LSTM the padded batch as it is (model.py:546: no packing, no
// mask), so every dialogue runs all S steps.
//
// torch's cell (gate rows of the weights in the order i, f, g, o):
//     G_t = x_t W_ih^T + b_ih + h_{t-1} W_hh^T + b_hh;   i, f, o = sigmoid(G_i, G_f, G_o),  g = tanh(G_g)
//     c_t = f c_{t-1} + i g;   h_t = o tanh(c_t);   the reverse direction runs t = S-1 .. 0; out[t] = [h_t fwd | h_t rev]
//
// Built from the pieces the DialogueRNN recurrence (dialogue_rnn.hip) already has, the same way and for the same reason — a
// step is a chain of tiny dependent products, so what counts is launches and round trips, not FLOPs:
//   * everything that depends on x alone is hoisted out of the chain: xg_d = x W_ih_d^T + b_ih_d for ALL steps is one GEMM per
//     direction (gemm.hip, fp32 MFMA);
//   * a step = ONE skinny MFMA product launch for BOTH directions (skinny_nt_kernel: [B x H] x [4H x H]^T + xg[t] + b_hh, the
//     dialogues on the n axis of v_mfma_f32_16x16x4_f32, K split over the waves and summed in wave order) + ONE gate launch for
//     both directions (sigmoid / tanh, the cell update, h_t straight into its half of out[t]): 2 launches per step;
//   * backward: per step one gate-gradient launch (dG_t and dc_{t-1} of both directions) and one skinny NN product
//     (dh_{t-1} = d_out[t-1] + dG_t W_hh, the weight read row-wise as stored); every weight gradient is DEFERRED: dG of all steps
//     is kept and four TN GEMMs after the loop compute dW_ih = dG^T x and dW_hh = dG^T h_prev over all tokens (owner-accumulated or
//     slab + ordered reduce: no atomics), the bias gradients are fixed-order column sums, dx = sum_d dG_d W_ih_d two NN GEMMs.
// Deterministic: no atomics anywhere.  B <= 32 per call behind ganffn_lstm_* / ganffn_lstm_stack_*; ganffn_lstm_batch_* /
// ganffn_lstm_stack_batch_* take up to GANFFN_MAX_DIALOGUES dialogues through the skinny kernels' dialogue-tile axis (still 2 + 2
// launches per step); the Python side chunks larger batches.
// ganffn_lstm_stack_fwd / _bwd (end of the file) chain the L layers of the stack in one call, with nn.LSTM's inter-layer dropout
// (Philox site 64 + l, offset base + l) between them: the same launches as L per-layer calls and L - 1 ganffn_dropout calls, so
// the same bits — what engine.MeldEngine runs instead of ops.lstm_forward's autograd chain.
//
// PACKED form (ganffn_lstm_packed_* / ganffn_lstm_stack_packed_*; an extension: the reference never packs): lengths[b] (int32, on
// the device, only ever compared with a time index) is the number of real steps of dialogue b.  At a time index tm >= lengths[b]
// the gate kernels SELECT zeros, in both directions: forward c_t = 0, h_t = 0 (into out[tm]) and zero saved gates, whatever the
// products computed for that row; backward dG = 0 for the four gates and a zero dc for the earlier step, whatever dh / d_out hold
// there.  That is pack_padded_sequence -> nn.LSTM -> pad_packed_sequence(total_length = S): the reverse direction enters step
// len - 1 with zero state (out[tm + 1] and c[tm + 1] are zero), the outputs past the end are zero, and the deferred GEMMs see
// zero dG rows at padded tokens, so nothing else changes — the same launches as the unpacked step, no host read of lengths.
#include "common.h"

namespace ganffn {

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

struct LstmGateDir {
    const float* G;        // [B x 4H] pre-activations of this step (everything added: xg, recurrent product, both biases)
    const float* c_prev;   // [B x H] (null at the first step: zeros)
    float* c;              // [B x H]
    float* h_out;          // h_t into out[t][:, d H .. (d + 1) H): leading dimension 2H
    float* gates;          // [B x 4H] activated i | f | g | o, kept for the backward
    int tm;                // this step's time index (read by the packed form only)
};
struct LstmGateArgs { LstmGateDir d[2]; int B, H; const int* lengths; };

// PACKED: dialogue b at a time index tm >= lengths[b] gets c = h = gates = 0 by a select (the row's products are discarded)
template <bool PACKED>
__global__ __launch_bounds__(256) void lstm_gate_fwd_kernel(LstmGateArgs a) {
    const LstmGateDir& q = a.d[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * a.H) return;
    const int b = idx / a.H, j = idx - b * a.H, H = a.H;
    const float* G = q.G + (size_t)b * 4 * H;
    const float i = sigmoidf_(G[j]), f = sigmoidf_(G[H + j]), g = tanhf(G[2 * H + j]), o = sigmoidf_(G[3 * H + j]);
    const float cp = q.c_prev ? q.c_prev[(size_t)b * H + j] : 0.f;
    const float c = f * cp + i * g;
    const float h = o * tanhf(c);
    float* S = q.gates + (size_t)b * 4 * H;
    if (PACKED) {
        const bool valid = q.tm < a.lengths[b];
        q.c[(size_t)b * H + j] = valid ? c : 0.f;
        q.h_out[(size_t)b * 2 * H + j] = valid ? h : 0.f;
        S[j] = valid ? i : 0.f; S[H + j] = valid ? f : 0.f; S[2 * H + j] = valid ? g : 0.f; S[3 * H + j] = valid ? o : 0.f;
    } else {
        q.c[(size_t)b * H + j] = c;
        q.h_out[(size_t)b * 2 * H + j] = h;
        S[j] = i; S[H + j] = f; S[2 * H + j] = g; S[3 * H + j] = o;
    }
}

struct LstmGateBwdDir {
    const float* dh; int ld_dh;   // gradient wrt h_t: d_out[t]'s half (ld 2H) at the first backward step, else the product's output (ld H)
    float* dc;                    // [B x H] in: dL/dc_t from the later step (zeros at the first backward step: dc_zero), out: dL/dc_{t-1}
    int dc_zero;
    const float* gates;           // activated i | f | g | o of this step
    const float* c; const float* c_prev;   // c_t, c_{t-1} (null: zeros)
    float* dG;                    // [B x 4H] gradient wrt the pre-activations of this step
    int tm;                       // this step's time index (read by the packed form only)
};
struct LstmGateBwdArgs { LstmGateBwdDir d[2]; int B, H; const int* lengths; };

// PACKED: dialogue b at a time index tm >= lengths[b] gets dG = 0 and hands dc = 0 to the earlier step, by a select and not a
// product with 0: whatever d_out / dh hold at a padded position (NaN included) cannot spread
template <bool PACKED>
__global__ __launch_bounds__(256) void lstm_gate_bwd_kernel(LstmGateBwdArgs a) {
    const LstmGateBwdDir& q = a.d[blockIdx.y];
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.B * a.H) return;
    const int b = idx / a.H, j = idx - b * a.H, H = a.H;
    const float* S = q.gates + (size_t)b * 4 * H;
    const float i = S[j], f = S[H + j], g = S[2 * H + j], o = S[3 * H + j];
    const float tc = tanhf(q.c[(size_t)b * H + j]);
    const float cp = q.c_prev ? q.c_prev[(size_t)b * H + j] : 0.f;
    const float dh = q.dh[(size_t)b * q.ld_dh + j];
    const float dc = dh * o * (1.f - tc * tc) + (q.dc_zero ? 0.f : q.dc[(size_t)b * H + j]);
    float* dG = q.dG + (size_t)b * 4 * H;
    const float di = dc * g * i * (1.f - i), df = dc * cp * f * (1.f - f), dg = dc * i * (1.f - g * g), dO = dh * tc * o * (1.f - o);
    const float dcp = dc * f;
    if (PACKED) {
        const bool valid = q.tm < a.lengths[b];
        dG[j] = valid ? di : 0.f; dG[H + j] = valid ? df : 0.f; dG[2 * H + j] = valid ? dg : 0.f; dG[3 * H + j] = valid ? dO : 0.f;
        q.dc[(size_t)b * H + j] = valid ? dcp : 0.f;
    } else {
        dG[j] = di; dG[H + j] = df; dG[2 * H + j] = dg; dG[3 * H + j] = dO;
        q.dc[(size_t)b * H + j] = dcp;
    }
}

// out[n] += sum over rows of X[row][n], rows in order (the two bias gradients of a direction are this same sum)
__global__ __launch_bounds__(256) void lstm_colsum2_kernel(const float* __restrict__ X, int rows, int N, float* __restrict__ o1, float* __restrict__ o2) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s[4] = {0.f, 0.f, 0.f, 0.f};                 // four interleaved chains, joined in a fixed order
    int r = 0;
    for (; r + 4 <= rows; r += 4) {
        s[0] += X[(size_t)r * N + n]; s[1] += X[(size_t)(r + 1) * N + n]; s[2] += X[(size_t)(r + 2) * N + n]; s[3] += X[(size_t)(r + 3) * N + n];
    }
    for (; r < rows; ++r) s[0] += X[(size_t)r * N + n];
    const float t = (s[0] + s[1]) + (s[2] + s[3]);
    if (o1) o1[n] += t;
    if (o2) o2[n] += t;
}

struct LstmOff { int64_t gates, c, total; };             // saved: gates [2][T x 4H] | c [2][T x H]
LstmOff lstm_saved(const ganffn_lstm_cfg* c) {
    const int64_t T = (int64_t)c->S * c->B, H = c->H;
    LstmOff o;
    o.gates = 0; o.c = 2 * T * 4 * H; o.total = o.c + 2 * T * H;
    return o;
}
// workspace: forward xg [2][T x 4H] | G [2][B x 4H];  backward dG [2][T x 4H] | dh [2][B x H] | dc [2][B x H] | TN partial slabs
int64_t lstm_ws(const ganffn_lstm_cfg* c) {
    const int64_t T = (int64_t)c->S * c->B, H = c->H, B = c->B;
    const int64_t fwd = 2 * T * 4 * H + 2 * B * 4 * H;
    const int64_t part = gemm_tn_part_floats(4 * c->H, c->In > c->H ? c->In : c->H, (int)T);
    const int64_t bwd = 2 * T * 4 * H + 4 * B * H + part + 64;
    return (fwd > bwd ? fwd : bwd) + 64;
}

// ---- the whole stack (ganffn_lstm_stack_*): L layers chained, nn.LSTM's inter-layer dropout between them
constexpr uint32_t SITE_LSTM0 = 64;                      // + layer (ops.SITE_LSTM): the dropout behind every layer but the last

inline ganffn_lstm_cfg stack_layer_cfg(const ganffn_lstm_stack_cfg* c, int l) {
    return ganffn_lstm_cfg{c->S, c->B, l == 0 ? c->In : 2 * c->H, c->H};
}
// saved: per layer the layer's own block (gates | c: 10 T H floats whatever its input width), then per layer but the last
// its output [T x 2H] and the dropped output [T x 2H] the next layer reads (unused when no dropout is active)
struct LstmStackOff { int64_t layer_stride, outs, total; };
LstmStackOff lstm_stack_saved(const ganffn_lstm_stack_cfg* c) {
    const int64_t T = (int64_t)c->S * c->B, H = c->H;
    LstmStackOff o;
    o.layer_stride = 10 * T * H;
    o.outs = c->L * o.layer_stride;
    o.total = o.outs + (int64_t)(c->L - 1) * 2 * T * 2 * H;
    return o;
}
// workspace: the widest layer's own workspace (16-byte rounded) | two [T x 2H] gradient buffers the backward alternates between
int64_t lstm_stack_layer_ws(const ganffn_lstm_stack_cfg* c) {
    int64_t m = 0;
    for (int l = 0; l < c->L; ++l) {
        const ganffn_lstm_cfg lc = stack_layer_cfg(c, l);
        const int64_t w = lstm_ws(&lc);
        m = w > m ? w : m;
    }
    return (m + 3) & ~(int64_t)3;
}

int check_lstm(const ganffn_lstm_cfg* c, int maxB = 32) {
    GF_CHECK_ARG(c, "null lstm cfg");
    GF_CHECK_ARG(c->S >= 1 && c->B >= 1 && c->B <= maxB, "lstm: S=%d B=%d (B <= %d per call)", c->S, c->B, maxB);
    GF_CHECK_ARG(c->In >= 4 && (c->In & 3) == 0 && c->H >= 4 && (c->H & 3) == 0, "lstm: In=%d H=%d must be multiples of 4", c->In, c->H);
    return 0;
}

int check_lstm_stack(const ganffn_lstm_stack_cfg* c, int maxB = 32) {
    GF_CHECK_ARG(c, "null lstm stack cfg");
    GF_CHECK_ARG(c->L >= 1 && c->L <= 16, "lstm stack: L=%d (1 .. 16 layers)", c->L);
    GF_CHECK_ARG(c->p >= 0.f && c->p < 1.f, "lstm stack: dropout p=%g must be in [0, 1)", (double)c->p);
    const ganffn_lstm_cfg l0 = stack_layer_cfg(c, 0);
    return check_lstm(&l0, maxB);
}

}  // namespace
}  // namespace ganffn

using namespace ganffn;

extern "C" int64_t ganffn_lstm_saved_floats(const ganffn_lstm_cfg* c) { return check_lstm(c) ? -1 : lstm_saved(c).total; }
extern "C" int64_t ganffn_lstm_workspace_floats(const ganffn_lstm_cfg* c) { return check_lstm(c) ? -1 : lstm_ws(c); }

// maxB: 32 behind the entry points that always had that limit, GANFFN_MAX_DIALOGUES behind the _batch_ and _packed_ ones;
// lengths: null behind every entry point but the _packed_ ones (which refuse a null one themselves)
static int lstm_layer_fwd(const ganffn_lstm_cfg* c, const float* x, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                          void* stream, int maxB, const int* lengths = nullptr) {
    GF_TRY(check_lstm(c, maxB));
    GF_CHECK_ARG(x && w_ih && w_hh && b_ih && b_hh && out && saved && workspace, "lstm_layer_fwd: null pointer");
    GF_CHECK_ARG(aligned16(x) && aligned16(out) && aligned16(saved) && aligned16(workspace), "lstm_layer_fwd: buffers must be 16-byte aligned");
    for (int d = 0; d < 2; ++d)
        GF_CHECK_ARG(w_ih[d] && w_hh[d] && b_ih[d] && b_hh[d] && aligned16(w_ih[d]) && aligned16(w_hh[d]), "lstm_layer_fwd: direction %d: null / unaligned weights", d);
    hipStream_t st = (hipStream_t)stream;
    const int S = c->S, B = c->B, In = c->In, H = c->H;
    const int64_t T = (int64_t)S * B;
    const LstmOff so = lstm_saved(c);
    float* xg = workspace;                          // [2][T x 4H]
    float* G = xg + 2 * T * 4 * H;                  // [2][B x 4H]
    for (int d = 0; d < 2; ++d) {
        EpiArgs e;
        e.bias = b_ih[d];
        GF_TRY(launch_gemm_nt(x, In, w_ih[d], In, xg + d * T * 4 * H, 4 * H, (int)T, 4 * H, In, EPI_NONE, e, st));
    }
    const dim3 ggrid((B * H + 255) / 256, 2);
    for (int t = 0; t < S; ++t) {
        SkinnyGroup sg;
        LstmGateArgs ga;
        ga.B = B; ga.H = H; ga.lengths = lengths;
        for (int d = 0; d < 2; ++d) {
            const int64_t tm = d == 0 ? t : S - 1 - t, tp = d == 0 ? tm - 1 : tm + 1;      // this step's / the previous step's time index
            float* Gd = G + (int64_t)d * B * 4 * H;
            float* cS = saved + so.c + d * T * H;
            float* gS = saved + so.gates + d * T * 4 * H;
            const float* xgt = xg + d * T * 4 * H + tm * B * 4 * H;
            // (first step: h_{-1} = 0 — the product runs on this step's own, still unwritten, c slot, zeroed below)
            sg.p[d] = SkinnyProb{t == 0 ? cS + tm * B * H : out + tp * B * 2 * H + d * H, t == 0 ? H : 2 * H, w_hh[d], H, xgt, 4 * H, nullptr,
                                 b_hh[d], Gd, 4 * H, B, 4 * H, H};
            ga.d[d] = LstmGateDir{Gd, t == 0 ? nullptr : cS + tp * B * H, cS + tm * B * H, out + tm * B * 2 * H + d * H, gS + tm * B * 4 * H, (int)tm};
        }
        if (t == 0) {
            // the first step's h_prev operand: this step's own (not yet written) c slot, zeroed — h_{-1} = 0 without a special kernel
            for (int d = 0; d < 2; ++d) {
                const int64_t tm = d == 0 ? 0 : S - 1;
                GF_HIP(hipMemsetAsync(saved + so.c + d * T * H + tm * B * H, 0, (size_t)B * H * sizeof(float), st));
            }
        }
        GF_TRY(launch_skinny(sg, 2, false, st));
        if (lengths) hipLaunchKernelGGL(lstm_gate_fwd_kernel<true>, ggrid, dim3(256), 0, st, ga);
        else hipLaunchKernelGGL(lstm_gate_fwd_kernel<false>, ggrid, dim3(256), 0, st, ga);
        GF_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int ganffn_lstm_layer_fwd(const ganffn_lstm_cfg* c, const float* x, const float* const* w_ih, const float* const* w_hh,
                                     const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                                     void* stream) {
    return lstm_layer_fwd(c, x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace, stream, 32);
}

static int lstm_layer_bwd(const ganffn_lstm_cfg* c, const float* d_out, const float* x, const float* out,
                          const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                          float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                          float* workspace, void* stream, int maxB, const int* lengths = nullptr) {
    GF_TRY(check_lstm(c, maxB));
    GF_CHECK_ARG(d_out && x && out && w_ih && w_hh && saved && workspace, "lstm_layer_bwd: null pointer");
    GF_CHECK_ARG(aligned16(d_out) && aligned16(x) && aligned16(out) && aligned16(saved) && aligned16(workspace) && (!dx || aligned16(dx)),
                 "lstm_layer_bwd: buffers must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int S = c->S, B = c->B, In = c->In, H = c->H;
    const int64_t T = (int64_t)S * B;
    const LstmOff so = lstm_saved(c);
    float* dG = workspace;                          // [2][T x 4H]
    float* dh = dG + 2 * T * 4 * H;                 // [2][B x H]
    float* dc = dh + 2 * B * H;                     // [2][B x H]
    float* part = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(dc + 2 * B * H) + 15) & ~(uintptr_t)15);
    const long part_floats = gemm_tn_part_floats(4 * H, In > H ? In : H, (int)T);
    const dim3 ggrid((B * H + 255) / 256, 2);
    for (int t = S - 1; t >= 0; --t) {              // step index of the forward loop, walked backwards
        LstmGateBwdArgs gb;
        gb.B = B; gb.H = H; gb.lengths = lengths;
        for (int d = 0; d < 2; ++d) {
            const int64_t tm = d == 0 ? t : S - 1 - t, tp = d == 0 ? tm - 1 : tm + 1;
            const float* cS = saved + so.c + d * T * H;
            const float* gS = saved + so.gates + d * T * 4 * H;
            const bool first = t == S - 1;          // first backward step: no later step feeds dh / dc
            gb.d[d] = LstmGateBwdDir{first ? d_out + tm * B * 2 * H + d * H : dh + (int64_t)d * B * H, first ? 2 * H : H, dc + (int64_t)d * B * H,
                                     first ? 1 : 0, gS + tm * B * 4 * H, cS + tm * B * H, t == 0 ? nullptr : cS + tp * B * H,
                                     dG + d * T * 4 * H + tm * B * 4 * H, (int)tm};
        }
        if (lengths) hipLaunchKernelGGL(lstm_gate_bwd_kernel<true>, ggrid, dim3(256), 0, st, gb);
        else hipLaunchKernelGGL(lstm_gate_bwd_kernel<false>, ggrid, dim3(256), 0, st, gb);
        GF_LAUNCH_CHECK();
        if (t > 0) {
            // dh_{t-1} = d_out[t-1]'s half + dG_t W_hh   ([B x 4H] x [4H x H], the weight row-wise as stored)
            SkinnyGroup sg;
            for (int d = 0; d < 2; ++d) {
                const int64_t tm = d == 0 ? t : S - 1 - t, tp = d == 0 ? tm - 1 : tm + 1;
                sg.p[d] = SkinnyProb{dG + d * T * 4 * H + tm * B * 4 * H, 4 * H, w_hh[d], H, d_out + tp * B * 2 * H + d * H, 2 * H, nullptr, nullptr,
                                     dh + (int64_t)d * B * H, H, B, H, 4 * H};
            }
            GF_TRY(launch_skinny(sg, 2, true, st));
        }
    }
    // deferred weight gradients over all tokens (accumulated: the caller zeroes), bias gradients, input gradient
    for (int d = 0; d < 2; ++d) {
        const float* dGd = dG + d * T * 4 * H;
        if (gw_ih && gw_ih[d]) GF_TRY(launch_gemm_tn_acc(dGd, 4 * H, x, In, gw_ih[d], In, nullptr, 4 * H, In, (int)T, st, part, part_floats));
        if (gw_hh && gw_hh[d] && S > 1) {
            // h_prev of time tm: forward direction out[tm - 1], reverse direction out[tm + 1] (zero at the direction's first step)
            const float* dGs = d == 0 ? dGd + (int64_t)B * 4 * H : dGd;
            const float* hp = d == 0 ? out + d * H : out + (int64_t)B * 2 * H + d * H;
            GF_TRY(launch_gemm_tn_acc(dGs, 4 * H, hp, 2 * H, gw_hh[d], H, nullptr, 4 * H, H, (int)(T - B), st, part, part_floats));
        }
        float* b1 = gb_ih ? gb_ih[d] : nullptr;
        float* b2 = gb_hh ? gb_hh[d] : nullptr;
        if (b1 || b2) {
            hipLaunchKernelGGL(lstm_colsum2_kernel, dim3((4 * H + 255) / 256), dim3(256), 0, st, dGd, (int)T, 4 * H, b1, b2);
            GF_LAUNCH_CHECK();
        }
    }
    if (dx) {
        EpiArgs e0;
        GF_TRY(launch_gemm_nn(dG, 4 * H, w_ih[0], In, dx, In, (int)T, In, 4 * H, EPI_NONE, e0, st));
        EpiArgs e1;
        e1.aux_in = dx;                              // + the reverse direction's share (each element read and written by one thread)
        GF_TRY(launch_gemm_nn(dG + T * 4 * H, 4 * H, w_ih[1], In, dx, In, (int)T, In, 4 * H, EPI_NONE, e1, st));
    }
    return 0;
}

extern "C" int ganffn_lstm_layer_bwd(const ganffn_lstm_cfg* c, const float* d_out, const float* x, const float* out,
                                     const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                     float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                     float* workspace, void* stream) {
    return lstm_layer_bwd(c, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace, stream, 32);
}

// ---- L layers in one call -------------------------------------------------------------------------------------------
extern "C" int64_t ganffn_lstm_stack_saved_floats(const ganffn_lstm_stack_cfg* c) { return check_lstm_stack(c) ? -1 : lstm_stack_saved(c).total; }
extern "C" int64_t ganffn_lstm_stack_workspace_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c) ? -1 : lstm_stack_layer_ws(c) + 2 * (int64_t)c->S * c->B * 2 * c->H;
}

// The per-layer entry points above, chained (same launches, same bits), with nn.LSTM(dropout = p)'s dropout on the output of every
// layer but the last: site SITE_LSTM0 + l, offset rng_offset_add + l — what ops.lstm_forward issues as separate calls.
static int lstm_stack_fwd(const ganffn_lstm_stack_cfg* c, const float* x, const float* const* w_ih, const float* const* w_hh,
                          const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                          const uint64_t* rng, uint64_t rng_offset_add, void* stream, int maxB, const int* lengths = nullptr) {
    GF_TRY(check_lstm_stack(c, maxB));
    GF_CHECK_ARG(x && w_ih && w_hh && b_ih && b_hh && out && saved && workspace, "lstm_stack_fwd: null pointer");
    const bool drop = c->train && c->p > 0.f && c->L > 1;
    GF_CHECK_ARG(!drop || rng, "lstm_stack_fwd: rng required in train mode");
    const int64_t T = (int64_t)c->S * c->B, H = c->H;
    const LstmStackOff so = lstm_stack_saved(c);
    const float* in = x;
    for (int l = 0; l < c->L; ++l) {
        const ganffn_lstm_cfg lc = stack_layer_cfg(c, l);
        const bool last = l + 1 == c->L;
        float* o = last ? out : saved + so.outs + (int64_t)l * 2 * T * 2 * H;
        GF_TRY(lstm_layer_fwd(&lc, in, w_ih + 2 * l, w_hh + 2 * l, b_ih + 2 * l, b_hh + 2 * l, o, saved + l * so.layer_stride,
                              workspace, stream, maxB, lengths));
        in = o;
        if (!last && drop) {
            float* dr = o + T * 2 * H;
            GF_TRY(launch_dropout(o, dr, (int)T, 2 * (int)H, c->p, SITE_LSTM0 + l, rng, rng_offset_add + l, 1, (hipStream_t)stream));
            in = dr;
        }
    }
    return 0;
}

extern "C" int ganffn_lstm_stack_fwd(const ganffn_lstm_stack_cfg* c, const float* x, const float* const* w_ih, const float* const* w_hh,
                                     const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                                     const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_fwd(c, x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace, rng, rng_offset_add, stream, 32);
}

// x, out: the forward's; gw_* / gb_*: arrays of [L][2] pointers, ACCUMULATED into like the per-layer backward (NULL arrays or
// entries: not wanted); dx [S x B x In] may be NULL.  The dropout masks are regenerated from {rng, rng_offset_add}.
static int lstm_stack_bwd(const ganffn_lstm_stack_cfg* c, const float* d_out, const float* x, const float* out,
                          const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                          float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                          float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream, int maxB,
                          const int* lengths = nullptr) {
    GF_TRY(check_lstm_stack(c, maxB));
    GF_CHECK_ARG(d_out && x && out && w_ih && w_hh && saved && workspace, "lstm_stack_bwd: null pointer");
    const bool drop = c->train && c->p > 0.f && c->L > 1;
    GF_CHECK_ARG(!drop || rng, "lstm_stack_bwd: rng required in train mode");
    const int64_t T = (int64_t)c->S * c->B, H = c->H;
    const LstmStackOff so = lstm_stack_saved(c);
    float* dbuf = workspace + lstm_stack_layer_ws(c);          // [2][T x 2H]
    const float* d = d_out;
    for (int l = c->L - 1; l >= 0; --l) {
        const ganffn_lstm_cfg lc = stack_layer_cfg(c, l);
        const float* o = l + 1 == c->L ? out : saved + so.outs + (int64_t)l * 2 * T * 2 * H;
        const float* prev = l == 0 ? nullptr : saved + so.outs + (int64_t)(l - 1) * 2 * T * 2 * H;
        const float* in = l == 0 ? x : drop ? prev + T * 2 * H : prev;
        float* dxl = l == 0 ? dx : dbuf + (int64_t)(l & 1) * T * 2 * H;
        GF_TRY(lstm_layer_bwd(&lc, d, in, o, w_ih + 2 * l, w_hh + 2 * l, dxl, gw_ih ? gw_ih + 2 * l : nullptr,
                              gw_hh ? gw_hh + 2 * l : nullptr, gb_ih ? gb_ih + 2 * l : nullptr, gb_hh ? gb_hh + 2 * l : nullptr,
                              saved + l * so.layer_stride, workspace, stream, maxB, lengths));
        if (l > 0 && drop)
            GF_TRY(launch_dropout(dxl, dxl, (int)T, 2 * (int)H, c->p, SITE_LSTM0 + (l - 1), rng, rng_offset_add + (l - 1), 1, (hipStream_t)stream));
        d = dxl;
    }
    return 0;
}
extern "C" int ganffn_lstm_stack_bwd(const ganffn_lstm_stack_cfg* c, const float* d_out, const float* x, const float* out,
                                     const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                     float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                     float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_bwd(c, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace, rng, rng_offset_add, stream, 32);
}

// ---- 1 <= B <= GANFFN_MAX_DIALOGUES dialogues per call ---------------------------------------------------------------------
// The bodies above with the skinny products' dialogue-tile axis (dialogue_rnn.hip): the same layouts and sizes as functions of
// B, the same launches per step; B <= 32 is the launch sequence of the entry points above, bit for bit.
extern "C" int64_t ganffn_lstm_batch_saved_floats(const ganffn_lstm_cfg* c) { return check_lstm(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_saved(c).total; }
extern "C" int64_t ganffn_lstm_batch_workspace_floats(const ganffn_lstm_cfg* c) { return check_lstm(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_ws(c); }
extern "C" int ganffn_lstm_batch_layer_fwd(const ganffn_lstm_cfg* c, const float* x, const float* const* w_ih, const float* const* w_hh,
                                           const float* const* b_ih, const float* const* b_hh, float* out, float* saved,
                                           float* workspace, void* stream) {
    return lstm_layer_fwd(c, x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace, stream, GANFFN_MAX_DIALOGUES);
}
extern "C" int ganffn_lstm_batch_layer_bwd(const ganffn_lstm_cfg* c, const float* d_out, const float* x, const float* out,
                                           const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                           float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                           float* workspace, void* stream) {
    return lstm_layer_bwd(c, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace, stream, GANFFN_MAX_DIALOGUES);
}
extern "C" int64_t ganffn_lstm_stack_batch_saved_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_stack_saved(c).total;
}
extern "C" int64_t ganffn_lstm_stack_batch_workspace_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_stack_layer_ws(c) + 2 * (int64_t)c->S * c->B * 2 * c->H;
}
extern "C" int ganffn_lstm_stack_batch_fwd(const ganffn_lstm_stack_cfg* c, const float* x, const float* const* w_ih,
                                           const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                                           float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_fwd(c, x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace, rng, rng_offset_add, stream, GANFFN_MAX_DIALOGUES);
}
extern "C" int ganffn_lstm_stack_batch_bwd(const ganffn_lstm_stack_cfg* c, const float* d_out, const float* x, const float* out,
                                           const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                           float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                           float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_bwd(c, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace, rng, rng_offset_add, stream,
                          GANFFN_MAX_DIALOGUES);
}

// ---- packed sequences: lengths[b] real steps per dialogue ------------------------------------------------------------------
// The _batch_ bodies with the length-aware gate kernels (the rule: top of the file): same layouts, sizes (ganffn_lstm_batch_*_floats /
// ganffn_lstm_stack_batch_*_floats) and launches.  lengths: int32 [B] on the device, never read by the host.
extern "C" int ganffn_lstm_packed_layer_fwd(const ganffn_lstm_cfg* c, const int32_t* lengths, const float* x, const float* const* w_ih,
                                            const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                                            float* saved, float* workspace, void* stream) {
    GF_CHECK_ARG(lengths, "lstm_packed_layer_fwd: null lengths");
    return lstm_layer_fwd(c, x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace, stream, GANFFN_MAX_DIALOGUES, lengths);
}
extern "C" int ganffn_lstm_packed_layer_bwd(const ganffn_lstm_cfg* c, const int32_t* lengths, const float* d_out, const float* x,
                                            const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                                            float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                                            const float* saved, float* workspace, void* stream) {
    GF_CHECK_ARG(lengths, "lstm_packed_layer_bwd: null lengths");
    return lstm_layer_bwd(c, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace, stream, GANFFN_MAX_DIALOGUES,
                          lengths);
}
extern "C" int ganffn_lstm_stack_packed_fwd(const ganffn_lstm_stack_cfg* c, const int32_t* lengths, const float* x,
                                            const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                                            const float* const* b_hh, float* out, float* saved, float* workspace, const uint64_t* rng,
                                            uint64_t rng_offset_add, void* stream) {
    GF_CHECK_ARG(lengths, "lstm_stack_packed_fwd: null lengths");
    return lstm_stack_fwd(c, x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace, rng, rng_offset_add, stream, GANFFN_MAX_DIALOGUES, lengths);
}
extern "C" int ganffn_lstm_stack_packed_bwd(const ganffn_lstm_stack_cfg* c, const int32_t* lengths, const float* d_out, const float* x,
                                            const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                                            float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                                            const float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add,
                                            void* stream) {
    GF_CHECK_ARG(lengths, "lstm_stack_packed_bwd: null lengths");
    return lstm_stack_bwd(c, d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace, rng, rng_offset_add, stream,
                          GANFFN_MAX_DIALOGUES, lengths);
}
