// lstm_stream.hip — the streaming form of nn.LSTM(In, H, num_layers = L, bidirectional = False) in eval mode (the recurrence of
// dialogue_rnn.MELDLSTMModel(causal=True)): ONE step of the L layers per new utterance against per-slot device state.  The index
// arrays (slot [n], pos [capacity] read only, count [n], off) and the SKIP rule are those of drnn_stream.hip.
//
// State (the caller owns it; include/ganffn.h states the same), three regions, each rounded up to a multiple of 4 floats:
//     Hs [capacity][L][H]         h of every layer after the slot's last step
//     Cs [capacity][L][H]         c of every layer
//     E  [capacity][max_len][H]   emotion history: E[s][t] = the last layer's h_t (the bits of Hs[s][L-1] after step t)
// Words of E at or above a slot's position are never read (E is the memory of ganffn_general2_stream_attention; the step itself
// only writes it), and at t = 0 every layer's h_prev and c_prev are taken as zeros WITHOUT reading the state: it needs no
// initialisation and a slot is reset by setting its position to 0.
//
// A step (row i: slot s = slot[i], t = pos[s] + off) is torch's LSTM cell (gate order i, f, g, o) for the L layers in turn.  Its
// cost is the weight read and its launch count, so the weight products go through launch_skinny (every row's sums in an order that
// does not depend on the other rows) and everything that does not depend on this step's new h shares the first product launch:
//   1. gather      dense operand rows by slot: x, every layer's h_prev and c_prev (zeros at t = 0 and for skipped rows).  Everything
//                  read from the state is copied here, so the in-place state writes below cannot race with a read.
//   2. products    the L recurrent products h_prev_l W_hh_l^T + b_hh_l and layer 0's input product x W_ih_0^T + b_ih_0
//                  (L + 1 problems, groups of 8 per launch)
//   3. per layer l gate: one thread per (row, column) -> Hs[s][l], Cs[s][l], a dense h_l row; the last layer also E[s][t], e_out[i]
//                  product (l < L-1): h_l W_ih_{l+1}^T + b_ih_{l+1} + (layer l+1's recurrent product)
// 2L + 1 launches at L <= 7.  A skipped row (slot outside [0, capacity), position negative, t outside [0, max_len), or masked by
// count) writes nothing to the state and a zero e_out row; nothing is accessed out of range whatever the index arrays hold.
// Inference only: nothing saved, no atomics, every summation order fixed; the bits of a row depend on no other row of the call.
#include "common.h"

namespace ganffn {

namespace {

constexpr int LS_MAXLEN = 110;
constexpr int LS_MAXH = 1024;
constexpr int LS_MAXL = 16;

static inline int64_t a4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// the index arrays of a call and the limits they are checked against
struct RowIdx {
    const int32_t* slot; const int32_t* pos; const int32_t* count;
    int off, capacity, max_len;
};
// whether row i takes part; s and t are valid only then
__device__ __forceinline__ bool row_live(const RowIdx& r, int i, int& s, int& t) {
    s = r.slot[i];
    if (s < 0 || s >= r.capacity) return false;
    const int p0 = r.pos[s];
    if (p0 < 0 || p0 >= r.max_len) return false;
    t = p0 + r.off;                       // (off < max_len: no overflow)
    if (t >= r.max_len) return false;
    return !(r.count && r.off >= r.count[i]);
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + __expf(-x)); }

// the dense buffers of a call (workspace) and the state regions
struct StepBufs {
    float *X, *Hp, *Cp;            // gathered: [n x In], [n x L x H], [n x L x H]
    float *GH;                     // recurrent products, layer-major: [L][n x 4H]
    float *GI;                     // the current layer's input product (l > 0: with its recurrent product added) [n x 4H]
    float *Hrow;                   // the current layer's new h [n x H]
    float *Hs, *Cs, *E;            // state regions
};

// ---- 1. gather ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lstm_stream_gather_kernel(RowIdx r, StepBufs b, const float* __restrict__ x, int In4, int LH4) {
    const int i = blockIdx.x;
    int s = 0, t = 0;
    const bool live = row_live(r, i, s, t);
    const bool past = live && t > 0;                 // the state is read only behind a position
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4* xi = reinterpret_cast<const float4*>(x) + (size_t)i * In4;
    float4* xo = reinterpret_cast<float4*>(b.X) + (size_t)i * In4;
    for (int k = threadIdx.x; k < In4; k += 256) {    // (workgroup-uniform branches: a select between a load and `zero` spills it)
        float4 v = zero;
        if (live) v = xi[k];
        xo[k] = v;
    }
    const float4* hs = reinterpret_cast<const float4*>(b.Hs) + (size_t)(past ? s : 0) * LH4;
    const float4* cs = reinterpret_cast<const float4*>(b.Cs) + (size_t)(past ? s : 0) * LH4;
    float4* ho = reinterpret_cast<float4*>(b.Hp) + (size_t)i * LH4;
    float4* co = reinterpret_cast<float4*>(b.Cp) + (size_t)i * LH4;
    for (int k = threadIdx.x; k < LH4; k += 256) {
        float4 h = zero, c = zero;
        if (past) {
            h = hs[k];
            c = cs[k];
        }
        ho[k] = h;
        co[k] = c;
    }
}

// ---- 3. gate of layer l ---------------------------------------------------------------------------------------------------------
// One thread per (row, column); the activation math of lstm.hip's lstm_gate_fwd_kernel.  Ga (+ Gb when given): the pre-activations
// [n x 4H], everything added.  LAST: the layer's h is the step's emotion row.
template <bool LAST>
__global__ __launch_bounds__(256) void lstm_stream_gate_kernel(RowIdx r, StepBufs b, const float* __restrict__ Ga, const float* __restrict__ Gb,
                                                               float* __restrict__ e_out, int n, int H, int L, int l) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * H) return;
    const int i = idx / H, j = idx - i * H;
    int s = 0, t = 0;
    if (!row_live(r, i, s, t)) {                      // the next product gets a finite row; the state is left alone
        b.Hrow[(size_t)i * H + j] = 0.f;
        if (LAST) e_out[(size_t)i * H + j] = 0.f;
        return;
    }
    const float* ga = Ga + (size_t)i * 4 * H + j;
    float pi = ga[0], pf = ga[H], pg = ga[2 * H], po = ga[3 * H];
    if (Gb) {
        const float* gb = Gb + (size_t)i * 4 * H + j;
        pi += gb[0]; pf += gb[H]; pg += gb[2 * H]; po += gb[3 * H];
    }
    const float ig = sigm(pi), fg = sigm(pf), gg = tanhf(pg), og = sigm(po);
    const float c = fg * b.Cp[((size_t)i * L + l) * H + j] + ig * gg;
    const float h = og * tanhf(c);
    b.Hs[((size_t)s * L + l) * H + j] = h;
    b.Cs[((size_t)s * L + l) * H + j] = c;
    b.Hrow[(size_t)i * H + j] = h;
    if (LAST) {
        b.E[((size_t)s * r.max_len + t) * H + j] = h;
        e_out[(size_t)i * H + j] = h;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static int check_cfg(const ganffn_stream_lstm_cfg* c) {
    GF_CHECK_ARG(c, "lstm_stream: null cfg");
    GF_CHECK_ARG(c->capacity >= 1 && c->capacity <= GANFFN_MAX_DIALOGUES, "lstm_stream: capacity=%d out of range [1,%d]", c->capacity,
                 GANFFN_MAX_DIALOGUES);
    GF_CHECK_ARG(c->max_len >= 1 && c->max_len <= LS_MAXLEN, "lstm_stream: max_len=%d out of range [1,%d]", c->max_len, LS_MAXLEN);
    GF_CHECK_ARG(c->In >= 4 && (c->In & 3) == 0 && c->H >= 4 && (c->H & 3) == 0, "lstm_stream: In=%d, H=%d must be multiples of 4", c->In,
                 c->H);
    GF_CHECK_ARG(c->H <= LS_MAXH, "lstm_stream: H = %d > %d (the emotion history is the memory of the general2 stream attention)", c->H,
                 LS_MAXH);
    GF_CHECK_ARG(c->L >= 1 && c->L <= LS_MAXL, "lstm_stream: L=%d out of range [1,%d]", c->L, LS_MAXL);
    return 0;
}

struct StateLayout { int64_t Hs, Cs, E, total; };
static StateLayout state_layout(const ganffn_stream_lstm_cfg* c) {
    StateLayout S;
    const int64_t hc = a4((int64_t)c->capacity * c->L * c->H);
    S.Hs = 0;
    S.Cs = S.Hs + hc;
    S.E = S.Cs + hc;
    S.total = S.E + a4((int64_t)c->capacity * c->max_len * c->H);
    return S;
}
// carve the workspace of n rows; returns its size in floats (ws may be null: size only)
static int64_t carve(const ganffn_stream_lstm_cfg* c, int n, float* ws, StepBufs& b) {
    int64_t o = 0;
    const int64_t H = c->H, In = c->In, L = c->L;
    auto take = [&](int64_t floats) { float* p = ws ? ws + o : nullptr; o += a4(floats); return p; };
    b.X = take(n * In); b.Hp = take(n * L * H); b.Cp = take(n * L * H);
    b.GH = take(L * n * 4 * H); b.GI = take(n * 4 * H); b.Hrow = take(n * H);
    return o;
}

static inline SkinnyProb prob(const float* A, int lda, const float* W, int ldw, const float* cin, const float* bias, float* C, int ldc, int M,
                              int N, int K) {
    SkinnyProb q{};
    q.A = A; q.lda = lda; q.W = W; q.ldw = ldw; q.Cin = cin; q.ldcin = ldc; q.Cin2 = nullptr; q.bias = bias; q.C = C; q.ldc = ldc;
    q.M = M; q.N = N; q.K = K;
    return q;
}
static int launch_probs(const SkinnyProb* pr, int np, hipStream_t st) {
    for (int lo = 0; lo < np; lo += 8) {
        SkinnyGroup sg;
        const int cnt = np - lo < 8 ? np - lo : 8;
        for (int i = 0; i < cnt; ++i) sg.p[i] = pr[lo + i];
        GF_TRY(launch_skinny(sg, cnt, false, st));
    }
    return 0;
}

struct StepCall {
    const ganffn_stream_lstm_cfg* c; int n;
    const int32_t *slot, *pos, *count;
    const float* const* w_ih; const float* const* w_hh; const float* const* b_ih; const float* const* b_hh;
    float *state, *workspace; hipStream_t st;
};
// every refusal of a step or an extend, before any launch
static int check_step(const StepCall& k, const char* what, const float* x, const float* e_out) {
    GF_TRY(check_cfg(k.c));
    GF_CHECK_ARG(k.n >= 1 && k.n <= k.c->capacity, "%s: n=%d out of range [1, capacity=%d]", what, k.n, k.c->capacity);
    GF_CHECK_ARG(k.slot && k.pos && x && k.w_ih && k.w_hh && k.b_ih && k.b_hh && k.state && e_out && k.workspace, "%s: null pointer", what);
    GF_CHECK_ARG(aligned16(x) && aligned16(k.state) && aligned16(e_out) && aligned16(k.workspace), "%s: buffers must be 16-byte aligned", what);
    for (int l = 0; l < k.c->L; ++l) {
        GF_CHECK_ARG(k.w_ih[l] && k.w_hh[l] && k.b_ih[l] && k.b_hh[l], "%s: null LSTM parameter of layer %d", what, l);
        GF_CHECK_ARG(aligned16(k.w_ih[l]) && aligned16(k.w_hh[l]), "%s: LSTM weights of layer %d must be 16-byte aligned", what, l);
    }
    return 0;
}

// the launches of one step over rows that check_step has accepted
static int step_launches(const StepCall& k, int off, const float* x, float* e_out) {
    const ganffn_stream_lstm_cfg* c = k.c;
    const int n = k.n, H = c->H, In = c->In, L = c->L, H4 = 4 * H;
    StepBufs b;
    carve(c, n, k.workspace, b);
    const StateLayout S = state_layout(c);
    b.Hs = k.state + S.Hs; b.Cs = k.state + S.Cs; b.E = k.state + S.E;
    const RowIdx r{k.slot, k.pos, k.count, off, c->capacity, c->max_len};
    const size_t gstride = (size_t)n * H4;           // a layer's block of GH

    hipLaunchKernelGGL(lstm_stream_gather_kernel, dim3(n), dim3(256), 0, k.st, r, b, x, In / 4, L * H / 4);
    GF_LAUNCH_CHECK();

    // everything that does not depend on this step's new h
    SkinnyProb pr[LS_MAXL + 1];
    int np = 0;
    for (int l = 0; l < L; ++l)                                                                       // h_prev_l W_hh_l^T + b_hh_l
        pr[np++] = prob(b.Hp + (size_t)l * H, L * H, k.w_hh[l], H, nullptr, k.b_hh[l], b.GH + l * gstride, H4, n, H4, H);
    pr[np++] = prob(b.X, In, k.w_ih[0], In, nullptr, k.b_ih[0], b.GI, H4, n, H4, In);                // x W_ih_0^T + b_ih_0
    GF_TRY(launch_probs(pr, np, k.st));

    const dim3 ggrid((unsigned)(((size_t)n * H + 255) / 256));
    for (int l = 0; l < L; ++l) {
        const float* gb = l == 0 ? b.GH : nullptr;          // layer 0's two products share a launch; later ones arrive added (Cin)
        if (l == L - 1) hipLaunchKernelGGL(lstm_stream_gate_kernel<true>, ggrid, dim3(256), 0, k.st, r, b, b.GI, gb, e_out, n, H, L, l);
        else hipLaunchKernelGGL(lstm_stream_gate_kernel<false>, ggrid, dim3(256), 0, k.st, r, b, b.GI, gb, e_out, n, H, L, l);
        GF_LAUNCH_CHECK();
        if (l + 1 < L) {                                                                              // h_l W_ih_{l+1}^T + b_ih_{l+1} + GH_{l+1}
            pr[0] = prob(b.Hrow, H, k.w_ih[l + 1], H, b.GH + (l + 1) * gstride, k.b_ih[l + 1], b.GI, H4, n, H4, H);
            GF_TRY(launch_probs(pr, 1, k.st));
        }
    }
    return 0;
}

}  // namespace

extern "C" int64_t ganffn_stream_lstm_state_floats(const ganffn_stream_lstm_cfg* c) {
    return check_cfg(c) ? -1 : state_layout(c).total;
}
extern "C" int64_t ganffn_stream_lstm_workspace_floats(const ganffn_stream_lstm_cfg* c, int n_max) {
    if (check_cfg(c)) return -1;
    if (n_max < 1 || n_max > c->capacity) return fail(-1, "lstm_stream: n_max=%d out of range [1, capacity=%d]", n_max, c->capacity);
    StepBufs b;
    return carve(c, n_max, nullptr, b);
}

extern "C" int ganffn_stream_lstm_step(const ganffn_stream_lstm_cfg* cfg, int n, const int32_t* slot, const int32_t* pos, int off,
                                       const int32_t* count, const float* x, const float* const* w_ih, const float* const* w_hh,
                                       const float* const* b_ih, const float* const* b_hh, float* state, float* e_out, float* workspace,
                                       void* stream) {
    const StepCall k{cfg, n, slot, pos, count, w_ih, w_hh, b_ih, b_hh, state, workspace, (hipStream_t)stream};
    GF_TRY(check_step(k, "lstm_stream_step", x, e_out));
    GF_CHECK_ARG(off >= 0 && off < cfg->max_len, "lstm_stream_step: off=%d out of range [0, max_len=%d)", off, cfg->max_len);
    return step_launches(k, off, x, e_out);
}

extern "C" int ganffn_stream_lstm_extend(const ganffn_stream_lstm_cfg* cfg, int n, int m, const int32_t* slot, const int32_t* count,
                                         const int32_t* pos, const float* x, const float* const* w_ih, const float* const* w_hh,
                                         const float* const* b_ih, const float* const* b_hh, float* state, float* e_out, float* workspace,
                                         void* stream) {
    const StepCall k{cfg, n, slot, pos, count, w_ih, w_hh, b_ih, b_hh, state, workspace, (hipStream_t)stream};
    GF_TRY(check_step(k, "lstm_stream_extend", x, e_out));
    GF_CHECK_ARG(count, "lstm_stream_extend: null pointer (count)");
    GF_CHECK_ARG(m >= 1 && m <= cfg->max_len, "lstm_stream_extend: m=%d out of range [1, max_len=%d]", m, cfg->max_len);
    // the recurrence is serial in t: the step, m times, on the rows of chunk step j (time-major), no host synchronisation
    for (int j = 0; j < m; ++j) GF_TRY(step_launches(k, j, x + (size_t)j * n * cfg->In, e_out + (size_t)j * n * cfg->H));
    return 0;
}

}  // namespace ganffn
