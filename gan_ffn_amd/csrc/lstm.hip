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
//
// ONE direction (ganffn_unilstm_* at the end of the file; an extension: the reference's LSTM is bidirectional): the direction
// count ndir, 2 or 1, is a property of the call (LstmCall::ndir).  The layouts take it — every region [ndir][...], h_at's leading
// dimension ndir H, layer l > 0's input ndir H wide, the stack's blocks [T x ndir H]; with ndir = 2 every offset and size is what
// it was —, the gate kernels read the leading dimension of h from their arguments (LstmGateArgs::ldh) and run grid.y = ndir,
// the skinny launches carry ndir problems, and the hoisted, deferred and dx GEMMs loop d < ndir (one direction: dx is the single
// NN product, no residual pass).  nn.LSTM(bidirectional=False): out[t] is a function of x[0 .. t]; a step stays 2 + 2 launches,
// and with the same weights out is bit for bit the forward half of the two-direction layer's (the same products, the same K split).
#include "common.h"

namespace ganffn {

namespace {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

struct LstmGateDir {
    const float* G;        // [B x 4H] pre-activations of this step (everything added: xg, recurrent product, both biases)
    const float* c_prev;   // [B x H] (null at the first step: zeros)
    float* c;              // [B x H]
    float* h_out;          // h_t into out[t][:, d H .. (d + 1) H): leading dimension ldh = ndir H
    float* gates;          // [B x 4H] activated i | f | g | o, kept for the backward
    int tm;                // this step's time index (read by the packed form only)
};
struct LstmGateArgs { LstmGateDir d[2]; int B, H, ldh; const int* lengths; };      // d[0 .. ndir): the launch's grid.y

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
        q.h_out[(size_t)b * a.ldh + j] = valid ? h : 0.f;
        S[j] = valid ? i : 0.f; S[H + j] = valid ? f : 0.f; S[2 * H + j] = valid ? g : 0.f; S[3 * H + j] = valid ? o : 0.f;
    } else {
        q.c[(size_t)b * H + j] = c;
        q.h_out[(size_t)b * a.ldh + j] = h;
        S[j] = i; S[H + j] = f; S[2 * H + j] = g; S[3 * H + j] = o;
    }
}

struct LstmGateBwdDir {
    const float* dh; int ld_dh;   // gradient wrt h_t: d_out[t]'s part (ld ndir H) at the first backward step, else the product's output (ld H)
    float* dc;                    // [B x H] in: dL/dc_t from the later step (zeros at the first backward step: dc_zero), out: dL/dc_{t-1}
    int dc_zero;
    const float* gates;           // activated i | f | g | o of this step
    const float* c; const float* c_prev;   // c_t, c_{t-1} (null: zeros)
    float* dG;                    // [B x 4H] gradient wrt the pre-activations of this step
    int tm;                       // this step's time index (read by the packed form only)
};
struct LstmGateBwdArgs { LstmGateBwdDir d[2]; int B, H, ldh; const int* lengths; };   // (ldh: unread — dh carries its own ld_dh)

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

// ------------------------------------------------------------------------------------------
// Host half.  THE layouts: every region of every buffer is laid out here, once, in floats from the start of its buffer; the
// eight size functions return the totals and the four drivers take every pointer from the offsets.
// ------------------------------------------------------------------------------------------
// Slack terms of a layer's workspace size, in floats.  PART_SLACK follows the TN partial slabs: it paid for re-aligning their
// start, which is a rounded offset that rounds nothing now (lstm_layout).  TAIL_SLACK ends the workspace: no region reaches into
// it.  Both are kept only so that no reported size changes.
constexpr int64_t PART_SLACK = 64, TAIL_SLACK = 64;

// One layer of ndir directions (2: nn.LSTM(bidirectional=True), 1: forward only — ganffn_unilstm_*).  [ndir]: the forward
// direction's block, then (ndir == 2) the reverse direction's; T = S B tokens, a time index tm owns B rows.
struct LstmLayout {
    int64_t T, B, H, ndir;
    int64_t gates, c, saved_total;                   // saved: gates [ndir][T x 4H] (activated i | f | g | o) | c [ndir][T x H]
    int64_t xg, G;                                   // workspace, forward: xg [ndir][T x 4H] | G [ndir][B x 4H] (this step's pre-activations)
    int64_t dG, dh, dc, part, part_floats;           // workspace, backward: dG [ndir][T x 4H] | dh [ndir][B x H] | dc [ndir][B x H] | TN partial slabs
    int64_t ws_total;                                // the larger pass + the slack
    // direction d's rows of time index tm in the per-token regions, direction d's block of the per-step ones
    int64_t gates_at(int d, int64_t tm) const { return gates + (d * T + tm * B) * 4 * H; }
    int64_t c_at(int d, int64_t tm) const { return c + (d * T + tm * B) * H; }
    int64_t xg_at(int d, int64_t tm) const { return xg + (d * T + tm * B) * 4 * H; }
    int64_t dG_at(int d, int64_t tm) const { return dG + (d * T + tm * B) * 4 * H; }
    int64_t G_of(int d) const { return G + d * B * 4 * H; }
    int64_t dh_of(int d) const { return dh + d * B * H; }
    int64_t dc_of(int d) const { return dc + d * B * H; }
    // ... and in out / d_out [T x ndir H]: direction d's part of time index tm's rows (leading dimension ldh)
    int64_t ldh() const { return ndir * H; }
    int64_t h_at(int d, int64_t tm) const { return (tm * B * ndir + d) * H; }
};
LstmLayout lstm_layout(const ganffn_lstm_cfg* c, int ndir) {
    LstmLayout L;
    const int64_t T = L.T = (int64_t)c->S * c->B, B = L.B = c->B, H = L.H = c->H, D = L.ndir = ndir;
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t r = p; p += n; return r; };
    L.gates = take(D * T * 4 * H); L.c = take(D * T * H);
    L.saved_total = p;
    p = 0;
    L.xg = take(D * T * 4 * H); L.G = take(D * B * 4 * H);
    const int64_t fwd = p;
    p = 0;
    L.dG = take(D * T * 4 * H); L.dh = take(D * B * H); L.dc = take(D * B * H);
    // the slabs start 16-byte aligned (gemm.hip's launcher refuses them otherwise): H % 4 == 0 (check_lstm) makes every region
    // above a multiple of 4 floats and the drivers refuse a workspace that is not 16-byte aligned, so this rounds nothing
    p = (p + 3) & ~(int64_t)3;
    // one slab region serves both deferred weight-gradient products, [4H x In] and [4H x H]: sized for the wider; the launcher
    // splits no further than the floats it is given
    L.part_floats = gemm_tn_part_floats(4 * c->H, c->In > c->H ? c->In : c->H, (int)T);
    L.part = take(L.part_floats);
    const int64_t bwd = p + PART_SLACK;
    L.ws_total = (fwd > bwd ? fwd : bwd) + TAIL_SLACK;
    return L;
}

// ---- the whole stack (ganffn_lstm_stack_*): L layers chained, nn.LSTM's inter-layer dropout between them
constexpr uint32_t SITE_LSTM0 = 64;                      // + layer (ops.SITE_LSTM): the dropout behind every layer but the last

inline ganffn_lstm_cfg stack_layer_cfg(const ganffn_lstm_stack_cfg* c, int l, int ndir) {
    return ganffn_lstm_cfg{c->S, c->B, l == 0 ? c->In : ndir * c->H, c->H};
}
struct LstmStackLayout {
    int64_t TD;                                      // floats of one [T x ndir H] block
    // saved: per layer the layer's own saved block (5 ndir T H floats whatever its input width), then per layer but the last its
    // output [T x ndir H] and the dropped output [T x ndir H] the next layer reads (unused when no dropout is active)
    int64_t layer_stride, between, saved_total;
    // workspace: the widest layer's own workspace (rounded to 16 bytes) | two [T x ndir H] gradient buffers: layer l's input gradient
    // goes to buffer l & 1, where layer l - 1 reads it as its d_out
    int64_t layer_ws, dbuf, ws_total;
    int64_t out(int l) const { return between + l * 2 * TD; }
    int64_t dropped(int l) const { return out(l) + TD; }
    int64_t d_in(int l) const { return dbuf + (l & 1) * TD; }
};
LstmStackLayout lstm_stack_layout(const ganffn_lstm_stack_cfg* c, int ndir) {
    LstmStackLayout L;
    L.TD = (int64_t)c->S * c->B * ndir * c->H;
    L.layer_ws = 0;
    for (int l = 0; l < c->L; ++l) {
        const ganffn_lstm_cfg lc = stack_layer_cfg(c, l, ndir);
        const LstmLayout ll = lstm_layout(&lc, ndir);
        L.layer_stride = ll.saved_total;                // (the same for every layer: no term of it holds In)
        L.layer_ws = ll.ws_total > L.layer_ws ? ll.ws_total : L.layer_ws;
    }
    L.layer_ws = (L.layer_ws + 3) & ~(int64_t)3;
    L.between = c->L * L.layer_stride;
    L.saved_total = L.out(c->L - 1);                    // (the last layer has no block there: its output is the call's)
    L.dbuf = L.layer_ws;
    L.ws_total = L.dbuf + 2 * L.TD;
    return L;
}

// maxB: 32 behind the entry points that always had that limit, GANFFN_MAX_DIALOGUES behind the _batch_ and _packed_ ones
int check_lstm(const ganffn_lstm_cfg* c, int maxB) {
    GF_CHECK_ARG(c, "null lstm cfg");
    GF_CHECK_ARG(c->S >= 1 && c->B >= 1 && c->B <= maxB, "lstm: S=%d B=%d (B <= %d per call)", c->S, c->B, maxB);
    GF_CHECK_ARG(c->In >= 4 && (c->In & 3) == 0 && c->H >= 4 && (c->H & 3) == 0, "lstm: In=%d H=%d must be multiples of 4", c->In, c->H);
    return 0;
}

int check_lstm_stack(const ganffn_lstm_stack_cfg* c, int maxB) {
    GF_CHECK_ARG(c, "null lstm stack cfg");
    GF_CHECK_ARG(c->L >= 1 && c->L <= 16, "lstm stack: L=%d (1 .. 16 layers)", c->L);
    GF_CHECK_ARG(c->p >= 0.f && c->p < 1.f, "lstm stack: dropout p=%g must be in [0, 1)", (double)c->p);
    const ganffn_lstm_cfg l0 = stack_layer_cfg(c, 0, 2);     // (layer 0's cfg holds no direction count)
    return check_lstm(&l0, maxB);
}

// What a forward or a backward call needs; the entry-point families differ only in ndir, maxB and lengths.  The weight and
// gradient arrays have one entry per direction ([L][ndir] in a stack call); a member its pass does not take stays null.
struct LstmCall {
    const ganffn_lstm_cfg* c;                  // (a stack call: null here, the stack's beside it in LstmStackCall)
    int ndir;                                  // directions: 2 (forward | reverse) or 1 (forward only)
    int maxB; const int* lengths;              // dialogue limit; real steps per dialogue (int32 [B] on the device) or null: all S
    hipStream_t st;
    const float* x; float* out; float* saved; float* workspace;                  // (the backward only reads out and saved)
    const float* const* w_ih; const float* const* w_hh; const float* const* b_ih; const float* const* b_hh;
    const float* d_out; float* dx;                                               // backward; dx may be null
    float* const* gw_ih; float* const* gw_hh; float* const* gb_ih; float* const* gb_hh;      // accumulated into; null arrays / entries: not wanted
    LstmCall& forward(const float* x_, const float* const* wi, const float* const* wh, const float* const* bi, const float* const* bh,
                      float* out_, float* saved_, float* ws) {
        x = x_; w_ih = wi; w_hh = wh; b_ih = bi; b_hh = bh; out = out_; saved = saved_; workspace = ws;
        return *this;
    }
    LstmCall& backward(const float* d_out_, const float* x_, const float* out_, const float* const* wi, const float* const* wh, float* dx_,
                       float* const* gwi, float* const* gwh, float* const* gbi, float* const* gbh, const float* saved_, float* ws) {
        d_out = d_out_; x = x_; out = const_cast<float*>(out_); w_ih = wi; w_hh = wh; dx = dx_;
        gw_ih = gwi; gw_hh = gwh; gb_ih = gbi; gb_hh = gbh; saved = const_cast<float*>(saved_); workspace = ws;
        return *this;
    }
};
inline LstmCall lstm_call(const ganffn_lstm_cfg* c, int maxB, const int* lengths, void* stream, int ndir = 2) {
    LstmCall k{};
    k.c = c; k.ndir = ndir; k.maxB = maxB; k.lengths = lengths; k.st = (hipStream_t)stream;
    return k;
}
struct LstmStackCall {
    const ganffn_lstm_stack_cfg* c; const uint64_t* rng; uint64_t add;     // add = rng_offset_add: layer l's dropout draws offset add + l
    LstmCall k;
    bool drop() const { return c->train && c->p > 0.f && c->L > 1; }
    // layer l's call: its cfg, its entries of the [L][ndir] arrays, its saved block; the driver sets x / out / d_out / dx
    LstmCall layer(const ganffn_lstm_cfg* lc, int l, const LstmStackLayout& L) const {
        LstmCall q = k;
        q.c = lc; q.saved = k.saved + l * L.layer_stride;
        q.w_ih = k.w_ih + k.ndir * l; q.w_hh = k.w_hh + k.ndir * l;
        if (k.b_ih) { q.b_ih = k.b_ih + k.ndir * l; q.b_hh = k.b_hh + k.ndir * l; }
        if (k.gw_ih) q.gw_ih = k.gw_ih + k.ndir * l;
        if (k.gw_hh) q.gw_hh = k.gw_hh + k.ndir * l;
        if (k.gb_ih) q.gb_ih = k.gb_ih + k.ndir * l;
        if (k.gb_hh) q.gb_hh = k.gb_hh + k.ndir * l;
        return q;
    }
};

// What a driver refuses before its first launch.  A stack driver (s given) checks the stack's cfg, the call's pointers and the
// rng; the layer drivers it then runs check each layer's buffers and weights themselves, as every layer call does.
int check_pass(const LstmCall& k, bool bwd, const LstmStackCall* s) {
    const char* of = s ? "stack" : "layer";
    GF_CHECK_ARG(k.ndir == 1 || k.ndir == 2, "lstm: %d directions", k.ndir);
    const char* pass = bwd ? "bwd" : "fwd";
    GF_TRY(s ? check_lstm_stack(s->c, k.maxB) : check_lstm(k.c, k.maxB));
    GF_CHECK_ARG(k.x && k.out && k.saved && k.workspace && k.w_ih && k.w_hh && (bwd ? k.d_out != nullptr : k.b_ih && k.b_hh),
                 "lstm_%s_%s: null pointer", of, pass);
    if (s) {
        GF_CHECK_ARG(!s->drop() || s->rng, "lstm_stack_%s: rng required in train mode", pass);
        return 0;
    }
    // (d_out and dx are null in a forward call, dx may be in a backward one: null counts as aligned)
    GF_CHECK_ARG(aligned16(k.d_out) && aligned16(k.x) && aligned16(k.out) && aligned16(k.saved) && aligned16(k.workspace) && aligned16(k.dx),
                 "lstm_layer_%s: buffers must be 16-byte aligned", pass);
    for (int d = 0; d < k.ndir; ++d)
        GF_CHECK_ARG(k.w_ih[d] && k.w_hh[d] && (bwd || (k.b_ih[d] && k.b_hh[d])) && aligned16(k.w_ih[d]) && aligned16(k.w_hh[d]),
                     "lstm_layer_%s: direction %d: null / unaligned weights", pass, d);
    return 0;
}

// The gate launch of a step, all ndir directions on grid.y: THE choice of its kernel, for both passes — the length-aware instantiation
// behind the _packed_ entry points (the call has lengths), the plain one behind all others.
template <class Args> void launch_gates(void (*packed)(Args), void (*plain)(Args), const LstmCall& k, Args& a) {
    a.B = k.c->B; a.H = k.c->H; a.ldh = k.ndir * k.c->H; a.lengths = k.lengths;
    hipLaunchKernelGGL(k.lengths ? packed : plain, dim3((a.B * a.H + 255) / 256, k.ndir), dim3(256), 0, k.st, a);
}

}  // namespace
}  // namespace ganffn

using namespace ganffn;

static int lstm_layer_fwd(const LstmCall& k) {
    GF_TRY(check_pass(k, false, nullptr));
    const int S = k.c->S, B = k.c->B, In = k.c->In, H = k.c->H, ND = k.ndir;
    const LstmLayout L = lstm_layout(k.c, ND);
    const int T = (int)L.T, ldh = (int)L.ldh();
    float* out = k.out; float* saved = k.saved; float* ws = k.workspace;
    for (int d = 0; d < ND; ++d) {
        GF_TRY(gemm(gemm_nt(k.x, k.w_ih[d], ws + L.xg_at(d, 0), T, 4 * H, In).bias(k.b_ih[d]).on(k.st)));
    }
    for (int t = 0; t < S; ++t) {
        SkinnyGroup sg;
        LstmGateArgs ga{};
        for (int d = 0; d < ND; ++d) {
            const int64_t tm = d == 0 ? t : S - 1 - t, tp = d == 0 ? tm - 1 : tm + 1;      // this step's / the previous step's time index
            float* c_t = saved + L.c_at(d, tm);
            float* Gd = ws + L.G_of(d);
            // first step: h_{-1} = 0 without a special kernel — the product runs on this step's own, not yet written, c slot, zeroed here
            if (t == 0) GF_HIP(hipMemsetAsync(c_t, 0, (size_t)B * H * sizeof(float), k.st));
            sg.p[d] = SkinnyProb{t == 0 ? c_t : out + L.h_at(d, tp), t == 0 ? H : ldh, k.w_hh[d], H, ws + L.xg_at(d, tm), 4 * H, nullptr,
                                 k.b_hh[d], Gd, 4 * H, B, 4 * H, H};
            ga.d[d] = LstmGateDir{Gd, t == 0 ? nullptr : saved + L.c_at(d, tp), c_t, out + L.h_at(d, tm), saved + L.gates_at(d, tm), (int)tm};
        }
        GF_TRY(launch_skinny(sg, ND, false, k.st));
        launch_gates(lstm_gate_fwd_kernel<true>, lstm_gate_fwd_kernel<false>, k, ga);
        GF_LAUNCH_CHECK();
    }
    return 0;
}

static int lstm_layer_bwd(const LstmCall& k) {
    GF_TRY(check_pass(k, true, nullptr));
    const int S = k.c->S, B = k.c->B, In = k.c->In, H = k.c->H, ND = k.ndir;
    const LstmLayout L = lstm_layout(k.c, ND);
    const int T = (int)L.T, ldh = (int)L.ldh();
    const float* d_out = k.d_out; const float* out = k.out; const float* saved = k.saved; float* ws = k.workspace;
    for (int t = S - 1; t >= 0; --t) {              // step index of the forward loop, walked backwards
        const bool first = t == S - 1;              // first backward step: no later step feeds dh / dc
        LstmGateBwdArgs gb{};
        SkinnyGroup sg;
        for (int d = 0; d < ND; ++d) {
            const int64_t tm = d == 0 ? t : S - 1 - t, tp = d == 0 ? tm - 1 : tm + 1;
            float* dG_t = ws + L.dG_at(d, tm);
            float* dh = ws + L.dh_of(d);
            gb.d[d] = LstmGateBwdDir{first ? d_out + L.h_at(d, tm) : dh, first ? ldh : H, ws + L.dc_of(d), first ? 1 : 0,
                                     saved + L.gates_at(d, tm), saved + L.c_at(d, tm), t == 0 ? nullptr : saved + L.c_at(d, tp), dG_t, (int)tm};
            // dh_{t-1} = d_out[t-1]'s part + dG_t W_hh   ([B x 4H] x [4H x H], the weight row-wise as stored)
            if (t > 0) sg.p[d] = SkinnyProb{dG_t, 4 * H, k.w_hh[d], H, d_out + L.h_at(d, tp), ldh, nullptr, nullptr, dh, H, B, H, 4 * H};
        }
        launch_gates(lstm_gate_bwd_kernel<true>, lstm_gate_bwd_kernel<false>, k, gb);
        GF_LAUNCH_CHECK();
        if (t > 0) GF_TRY(launch_skinny(sg, ND, true, k.st));
    }
    // deferred weight gradients over all tokens (accumulated: the caller zeroes), bias gradients, input gradient
    float* part = ws + L.part;
    for (int d = 0; d < ND; ++d) {
        const float* dGd = ws + L.dG_at(d, 0);
        if (k.gw_ih && k.gw_ih[d]) GF_TRY(gemm(gemm_tn(dGd, k.x, k.gw_ih[d], 4 * H, In, T).tn_workspace(part, L.part_floats).on(k.st)));
        if (k.gw_hh && k.gw_hh[d] && S > 1) {
            // h_prev of time tm: forward direction out[tm - 1], reverse direction out[tm + 1] (zero at the direction's first step):
            // the forward direction pairs dG of times 1 .. S-1 with out of 0 .. S-2, the reverse one dG of 0 .. S-2 with out of 1 .. S-1
            const int from = d == 0 ? 1 : 0;
            GF_TRY(gemm(gemm_tn(ws + L.dG_at(d, from), out + L.h_at(d, 1 - from), k.gw_hh[d], 4 * H, H, T - B).ld(4 * H, ldh, H)
                            .tn_workspace(part, L.part_floats).on(k.st)));
        }
        float* b1 = k.gb_ih ? k.gb_ih[d] : nullptr;
        float* b2 = k.gb_hh ? k.gb_hh[d] : nullptr;
        if (b1 || b2) {
            hipLaunchKernelGGL(lstm_colsum2_kernel, dim3((4 * H + 255) / 256), dim3(256), 0, k.st, dGd, T, 4 * H, b1, b2);
            GF_LAUNCH_CHECK();
        }
    }
    if (k.dx) {
        GF_TRY(gemm(gemm_nn(ws + L.dG_at(0, 0), k.w_ih[0], k.dx, T, In, 4 * H).on(k.st)));
        // + the reverse direction's share (each element read and written by one thread); one direction: no residual pass
        if (ND == 2) GF_TRY(gemm(gemm_nn(ws + L.dG_at(1, 0), k.w_ih[1], k.dx, T, In, 4 * H).residual(k.dx).on(k.st)));
    }
    return 0;
}

// The layer driver L times (same launches, same bits as L per-layer calls), with nn.LSTM(dropout = p)'s dropout on the output of
// every layer but the last: site SITE_LSTM0 + l, offset add + l — what ops.lstm_forward issues as separate calls.
static int lstm_stack_fwd(const LstmStackCall& s) {
    GF_TRY(check_pass(s.k, false, &s));
    const ganffn_lstm_stack_cfg* c = s.c;
    const int ND = s.k.ndir;
    const LstmStackLayout L = lstm_stack_layout(c, ND);
    const int T = c->S * c->B;
    const float* in = s.k.x;
    for (int l = 0; l < c->L; ++l) {
        const ganffn_lstm_cfg lc = stack_layer_cfg(c, l, ND);
        const bool last = l + 1 == c->L;
        LstmCall q = s.layer(&lc, l, L);
        q.x = in; q.out = last ? s.k.out : s.k.saved + L.out(l);
        GF_TRY(lstm_layer_fwd(q));
        in = q.out;
        if (!last && s.drop()) {
            float* dr = s.k.saved + L.dropped(l);
            GF_TRY(launch_dropout(q.out, dr, T, ND * c->H, c->p, SITE_LSTM0 + l, s.rng, s.add + l, 1, s.k.st));
            in = dr;
        }
    }
    return 0;
}

// x, out: the forward's; the dropout masks are regenerated from {rng, add}
static int lstm_stack_bwd(const LstmStackCall& s) {
    GF_TRY(check_pass(s.k, true, &s));
    const ganffn_lstm_stack_cfg* c = s.c;
    const int ND = s.k.ndir;
    const LstmStackLayout L = lstm_stack_layout(c, ND);
    const int T = c->S * c->B;
    const float* d = s.k.d_out;
    for (int l = c->L - 1; l >= 0; --l) {
        const ganffn_lstm_cfg lc = stack_layer_cfg(c, l, ND);
        LstmCall q = s.layer(&lc, l, L);
        q.d_out = d;
        q.x = l == 0 ? s.k.x : s.k.saved + (s.drop() ? L.dropped(l - 1) : L.out(l - 1));
        q.out = l + 1 == c->L ? s.k.out : s.k.saved + L.out(l);
        q.dx = l == 0 ? s.k.dx : s.k.workspace + L.d_in(l);
        GF_TRY(lstm_layer_bwd(q));
        if (l > 0 && s.drop())
            GF_TRY(launch_dropout(q.dx, q.dx, T, ND * c->H, c->p, SITE_LSTM0 + (l - 1), s.rng, s.add + (l - 1), 1, s.k.st));
        d = q.dx;
    }
    return 0;
}

// ---- the entry points: each states its family — the dialogue limit and whether it takes lengths — fills one call and runs a driver
constexpr int PLAIN_MAX_DIALOGUES = 32;       // ganffn_lstm_* / ganffn_lstm_stack_*: the limit they always had (they keep refusing 33)

extern "C" int64_t ganffn_lstm_saved_floats(const ganffn_lstm_cfg* c) { return check_lstm(c, PLAIN_MAX_DIALOGUES) ? -1 : lstm_layout(c, 2).saved_total; }
extern "C" int64_t ganffn_lstm_workspace_floats(const ganffn_lstm_cfg* c) { return check_lstm(c, PLAIN_MAX_DIALOGUES) ? -1 : lstm_layout(c, 2).ws_total; }
extern "C" int ganffn_lstm_layer_fwd(const ganffn_lstm_cfg* c, const float* x, const float* const* w_ih, const float* const* w_hh,
                                     const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                                     void* stream) {
    return lstm_layer_fwd(lstm_call(c, PLAIN_MAX_DIALOGUES, nullptr, stream).forward(x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace));
}
extern "C" int ganffn_lstm_layer_bwd(const ganffn_lstm_cfg* c, const float* d_out, const float* x, const float* out,
                                     const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                     float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                     float* workspace, void* stream) {
    return lstm_layer_bwd(lstm_call(c, PLAIN_MAX_DIALOGUES, nullptr, stream)
                              .backward(d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace));
}

// L layers in one call.  gw_* / gb_*: arrays of [L][2] pointers, ACCUMULATED into like the per-layer backward (NULL arrays or
// entries: not wanted); dx [S x B x In] may be NULL.
extern "C" int64_t ganffn_lstm_stack_saved_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c, PLAIN_MAX_DIALOGUES) ? -1 : lstm_stack_layout(c, 2).saved_total;
}
extern "C" int64_t ganffn_lstm_stack_workspace_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c, PLAIN_MAX_DIALOGUES) ? -1 : lstm_stack_layout(c, 2).ws_total;
}
extern "C" int ganffn_lstm_stack_fwd(const ganffn_lstm_stack_cfg* c, const float* x, const float* const* w_ih, const float* const* w_hh,
                                     const float* const* b_ih, const float* const* b_hh, float* out, float* saved, float* workspace,
                                     const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_fwd({c, rng, rng_offset_add,
                           lstm_call(nullptr, PLAIN_MAX_DIALOGUES, nullptr, stream).forward(x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace)});
}
extern "C" int ganffn_lstm_stack_bwd(const ganffn_lstm_stack_cfg* c, const float* d_out, const float* x, const float* out,
                                     const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                     float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                     float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_bwd({c, rng, rng_offset_add, lstm_call(nullptr, PLAIN_MAX_DIALOGUES, nullptr, stream)
                                                       .backward(d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace)});
}

// ---- 1 <= B <= GANFFN_MAX_DIALOGUES dialogues per call ---------------------------------------------------------------------
// The same drivers with the skinny products' dialogue-tile axis (dialogue_rnn.hip): the same layouts and sizes as functions of
// B, the same launches per step; B <= 32 is the launch sequence of the entry points above, bit for bit.
extern "C" int64_t ganffn_lstm_batch_saved_floats(const ganffn_lstm_cfg* c) { return check_lstm(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_layout(c, 2).saved_total; }
extern "C" int64_t ganffn_lstm_batch_workspace_floats(const ganffn_lstm_cfg* c) { return check_lstm(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_layout(c, 2).ws_total; }
extern "C" int ganffn_lstm_batch_layer_fwd(const ganffn_lstm_cfg* c, const float* x, const float* const* w_ih, const float* const* w_hh,
                                           const float* const* b_ih, const float* const* b_hh, float* out, float* saved,
                                           float* workspace, void* stream) {
    return lstm_layer_fwd(lstm_call(c, GANFFN_MAX_DIALOGUES, nullptr, stream).forward(x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace));
}
extern "C" int ganffn_lstm_batch_layer_bwd(const ganffn_lstm_cfg* c, const float* d_out, const float* x, const float* out,
                                           const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                           float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                           float* workspace, void* stream) {
    return lstm_layer_bwd(lstm_call(c, GANFFN_MAX_DIALOGUES, nullptr, stream)
                              .backward(d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace));
}
extern "C" int64_t ganffn_lstm_stack_batch_saved_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_stack_layout(c, 2).saved_total;
}
extern "C" int64_t ganffn_lstm_stack_batch_workspace_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_stack_layout(c, 2).ws_total;
}
extern "C" int ganffn_lstm_stack_batch_fwd(const ganffn_lstm_stack_cfg* c, const float* x, const float* const* w_ih,
                                           const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                                           float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_fwd({c, rng, rng_offset_add,
                           lstm_call(nullptr, GANFFN_MAX_DIALOGUES, nullptr, stream).forward(x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace)});
}
extern "C" int ganffn_lstm_stack_batch_bwd(const ganffn_lstm_stack_cfg* c, const float* d_out, const float* x, const float* out,
                                           const float* const* w_ih, const float* const* w_hh, float* dx, float* const* gw_ih,
                                           float* const* gw_hh, float* const* gb_ih, float* const* gb_hh, const float* saved,
                                           float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_bwd({c, rng, rng_offset_add, lstm_call(nullptr, GANFFN_MAX_DIALOGUES, nullptr, stream)
                                                       .backward(d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace)});
}

// ---- packed sequences: lengths[b] real steps per dialogue ------------------------------------------------------------------
// The _batch_ calls with lengths, so with the length-aware gate kernels (the rule: top of the file): same layouts, sizes
// (ganffn_lstm_batch_*_floats / ganffn_lstm_stack_batch_*_floats) and launches.  lengths: int32 [B] on the device, never read by
// the host; a null one is refused here, before anything else: behind these entry points it would select the other kernels.
extern "C" int ganffn_lstm_packed_layer_fwd(const ganffn_lstm_cfg* c, const int32_t* lengths, const float* x, const float* const* w_ih,
                                            const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                                            float* saved, float* workspace, void* stream) {
    GF_CHECK_ARG(lengths, "lstm_packed_layer_fwd: null lengths");
    return lstm_layer_fwd(lstm_call(c, GANFFN_MAX_DIALOGUES, lengths, stream).forward(x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace));
}
extern "C" int ganffn_lstm_packed_layer_bwd(const ganffn_lstm_cfg* c, const int32_t* lengths, const float* d_out, const float* x,
                                            const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                                            float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                                            const float* saved, float* workspace, void* stream) {
    GF_CHECK_ARG(lengths, "lstm_packed_layer_bwd: null lengths");
    return lstm_layer_bwd(lstm_call(c, GANFFN_MAX_DIALOGUES, lengths, stream)
                              .backward(d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace));
}
extern "C" int ganffn_lstm_stack_packed_fwd(const ganffn_lstm_stack_cfg* c, const int32_t* lengths, const float* x,
                                            const float* const* w_ih, const float* const* w_hh, const float* const* b_ih,
                                            const float* const* b_hh, float* out, float* saved, float* workspace, const uint64_t* rng,
                                            uint64_t rng_offset_add, void* stream) {
    GF_CHECK_ARG(lengths, "lstm_stack_packed_fwd: null lengths");
    return lstm_stack_fwd({c, rng, rng_offset_add,
                           lstm_call(nullptr, GANFFN_MAX_DIALOGUES, lengths, stream).forward(x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace)});
}
extern "C" int ganffn_lstm_stack_packed_bwd(const ganffn_lstm_stack_cfg* c, const int32_t* lengths, const float* d_out, const float* x,
                                            const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                                            float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                                            const float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add,
                                            void* stream) {
    GF_CHECK_ARG(lengths, "lstm_stack_packed_bwd: null lengths");
    return lstm_stack_bwd({c, rng, rng_offset_add, lstm_call(nullptr, GANFFN_MAX_DIALOGUES, lengths, stream)
                                                       .backward(d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace)});
}

// ---- one direction: nn.LSTM(bidirectional=False) ----------------------------------------------------------------------------
// The same drivers with ndir = 1 (an extension: the reference's LSTM is bidirectional): every region [1][...], out / d_out
// [S x B x H], layer l > 0's input H wide, weight and gradient arrays [L][1]; one problem per skinny launch, one hoisted input
// product, one dx product — still 2 launches per step, forward and backward.  ONE family for the padded and the packed run:
// lengths (int32 [B] on the device) may be NULL = every dialogue runs all S steps; 1 <= B <= GANFFN_MAX_DIALOGUES.
constexpr int UNI = 1;

extern "C" int64_t ganffn_unilstm_saved_floats(const ganffn_lstm_cfg* c) { return check_lstm(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_layout(c, UNI).saved_total; }
extern "C" int64_t ganffn_unilstm_workspace_floats(const ganffn_lstm_cfg* c) { return check_lstm(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_layout(c, UNI).ws_total; }
extern "C" int ganffn_unilstm_layer_fwd(const ganffn_lstm_cfg* c, const int32_t* lengths, const float* x, const float* const* w_ih,
                                        const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                                        float* saved, float* workspace, void* stream) {
    return lstm_layer_fwd(lstm_call(c, GANFFN_MAX_DIALOGUES, lengths, stream, UNI).forward(x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace));
}
extern "C" int ganffn_unilstm_layer_bwd(const ganffn_lstm_cfg* c, const int32_t* lengths, const float* d_out, const float* x,
                                        const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                                        float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                                        const float* saved, float* workspace, void* stream) {
    return lstm_layer_bwd(lstm_call(c, GANFFN_MAX_DIALOGUES, lengths, stream, UNI)
                              .backward(d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace));
}
extern "C" int64_t ganffn_unilstm_stack_saved_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_stack_layout(c, UNI).saved_total;
}
extern "C" int64_t ganffn_unilstm_stack_workspace_floats(const ganffn_lstm_stack_cfg* c) {
    return check_lstm_stack(c, GANFFN_MAX_DIALOGUES) ? -1 : lstm_stack_layout(c, UNI).ws_total;
}
extern "C" int ganffn_unilstm_stack_fwd(const ganffn_lstm_stack_cfg* c, const int32_t* lengths, const float* x, const float* const* w_ih,
                                        const float* const* w_hh, const float* const* b_ih, const float* const* b_hh, float* out,
                                        float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add, void* stream) {
    return lstm_stack_fwd({c, rng, rng_offset_add, lstm_call(nullptr, GANFFN_MAX_DIALOGUES, lengths, stream, UNI)
                                                       .forward(x, w_ih, w_hh, b_ih, b_hh, out, saved, workspace)});
}
extern "C" int ganffn_unilstm_stack_bwd(const ganffn_lstm_stack_cfg* c, const int32_t* lengths, const float* d_out, const float* x,
                                        const float* out, const float* const* w_ih, const float* const* w_hh, float* dx,
                                        float* const* gw_ih, float* const* gw_hh, float* const* gb_ih, float* const* gb_hh,
                                        const float* saved, float* workspace, const uint64_t* rng, uint64_t rng_offset_add,
                                        void* stream) {
    return lstm_stack_bwd({c, rng, rng_offset_add, lstm_call(nullptr, GANFFN_MAX_DIALOGUES, lengths, stream, UNI)
                                                       .backward(d_out, x, out, w_ih, w_hh, dx, gw_ih, gw_hh, gb_ih, gb_hh, saved, workspace)});
}
