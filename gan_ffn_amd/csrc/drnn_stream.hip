// drnn_stream.hip — the streaming form of the causal DialogueRNN classifier head (dialogue_rnn.UniModel): ONE recurrence step per
// new utterance against per-slot device state, and the second (general2) attention of the new rows over the slot's emotion history.
// The generators' side of a streamed step is stream.hip; this file is the head's.
//
// State (the caller owns it; include/ganffn.h states the same), three regions, each rounded up to a multiple of 4 floats:
//     G [capacity][max_len][H]    global history g_0 .. g_{t-1} of the dialogue in slot s
//     Q [capacity][parties][H]    party states
//     E [capacity][max_len][He]   emotion history; E[s][t-1] is the emotion cell's recurrent state
// Words of G and E at or above a slot's position are never read, and at position 0 g_prev, every party row and e_prev are taken
// as zeros WITHOUT reading the state: it needs no initialisation and a slot is reset by setting its position to 0.
//
// A step (row i: slot s = slot[i], t = pos[s] + off, speaker spk[i]) is DialogueRNNCell.forward for one real utterance in eval
// mode.  It is one link of a latency chain whose cost is the weight read, so the weight products go through launch_skinny (up to
// 256 rows in tiles of 32, every row's sums in an order that does not depend on the other rows) and everything that does not depend
// on this step's g_t, c_t or qs shares the first product launch:
//   1. gather        dense operand rows by slot and position: [U | q[spk]], g_{t-1}, e_{t-1}, all party rows (zeros at t = 0)
//   2. products      g cell (input and recurrent), party cell recurrent, party cell U part, attention query, e cell recurrent,
//                    listener U part and the listener's recurrent product per party row (groups of 8 problems per launch)
//   3. gate + attn   one workgroup per row: g_t -> G[s][t], then the context attention over G[s][0 .. t-1] -> c_t
//   4. product       party cell context part: c_t W_ih_p[:, Dm:]^T + (U part)
//   5. party gate    qs; without listener state it writes Q[s]
//   6. products      e cell input qs W_ih_e^T (and the listener's qs part)
//   7. e gate        e_t -> E[s][t], e_out; with listener state the listener gates of every party row and the blend -> Q[s]
// A skipped row (slot outside [0, capacity), position negative, t outside [0, max_len), speaker outside [0, parties), or masked by
// count) leaves the state untouched and gives a zero e_out row; nothing is accessed out of range whatever the index arrays hold.
// Inference only: no dropout, nothing saved, no atomics, every summation order fixed; the bits of a row depend on no other row.
#include "common.h"

namespace ganffn {

namespace {

enum : int { ATT_GENERAL = GANFFN_DRNN_ATT_GENERAL, ATT_SIMPLE = GANFFN_DRNN_ATT_SIMPLE, ATT_DOT = GANFFN_DRNN_ATT_DOT,
             ATT_GENERAL2 = GANFFN_DRNN_ATT_GENERAL2, ATT_CONCAT = GANFFN_DRNN_ATT_CONCAT };
constexpr int DS_NT = 512;            // threads of a row's workgroup: one state column per thread (H <= 512)
constexpr int DS_WAVES = DS_NT / 64;
constexpr int DS_MAXLEN = 110;
constexpr int DS_MAXDA = 512;

static inline int64_t a4(int64_t n) { return (n + 3) & ~(int64_t)3; }

// the index arrays of a call and the limits they are checked against
struct RowIdx {
    const int32_t* slot; const int32_t* pos; const int32_t* count; const int32_t* spk;
    int off, capacity, max_len, parties;
};
// whether row i takes part; s, t, sp are valid only then
__device__ __forceinline__ bool row_live(const RowIdx& r, int i, int& s, int& t, int& sp) {
    s = r.slot[i];
    if (s < 0 || s >= r.capacity) return false;
    const int p0 = r.pos[s];
    if (p0 < 0 || p0 >= r.max_len) return false;
    t = p0 + r.off;                       // (off < max_len: no overflow)
    if (t >= r.max_len) return false;
    if (r.count && r.off >= r.count[i]) return false;
    sp = r.spk[i];
    return sp >= 0 && sp < r.parties;
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + __expf(-x)); }
// torch.nn.GRUCell, column u of a width-W cell: r, z, n row blocks of the pre-activations (biases included)
__device__ __forceinline__ float gru_col(const float* __restrict__ gi, const float* __restrict__ gh, int W, int u, float h) {
    const float r = sigm(gi[u] + gh[u]);
    const float z = sigm(gi[W + u] + gh[W + u]);
    const float n = tanhf(gi[2 * W + u] + r * gh[2 * W + u]);
    return (1.0f - z) * n + z * h;
}

// the dense buffers of a call (workspace) and the state regions
struct StepBufs {
    float *Acat, *Gp, *Ep, *Qg;                 // gathered: [n x (Dm+H)], [n x H], [n x He], [n x P x H]
    float *GIg, *GHg, *GHp, *XP, *GIp;          // [n x 3H]
    float *XA;                                  // attention query [n x H] (concat: X = W_u U [n x Da])
    float *CT, *QS;                             // context, speaker's new party state [n x H]
    float *GIe, *GHe;                           // [n x 3He]
    float *XL, *GIl, *GHl;                      // listener: [n x 3H], [n x 3H], [n x P x 3H]
    float *G, *Q, *E;                           // state regions
};

// ---- 1. gather ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void drnn_stream_gather_kernel(RowIdx r, StepBufs b, const float* __restrict__ U, int Dm, int H, int He) {
    const int i = blockIdx.x, P = r.parties;
    int s = 0, t = 0, sp = 0;
    const bool live = row_live(r, i, s, t, sp);
    const bool past = live && t > 0;                 // the state is read only behind a position
    float* acat = b.Acat + (size_t)i * (Dm + H);
    const float* u = U + (size_t)i * Dm;
    for (int k = threadIdx.x; k < Dm; k += 256) acat[k] = live ? u[k] : 0.f;
    const float* q = b.Q + (size_t)(past ? s : 0) * P * H;
    const float* g = b.G + ((size_t)(past ? s : 0) * r.max_len + (past ? t - 1 : 0)) * H;
    for (int k = threadIdx.x; k < H; k += 256) {
        acat[Dm + k] = past ? q[(size_t)sp * H + k] : 0.f;
        b.Gp[(size_t)i * H + k] = past ? g[k] : 0.f;
    }
    for (int k = threadIdx.x; k < P * H; k += 256) b.Qg[(size_t)i * P * H + k] = past ? q[k] : 0.f;
    const float* e = b.E + ((size_t)(past ? s : 0) * r.max_len + (past ? t - 1 : 0)) * He;
    for (int k = threadIdx.x; k < He; k += 256) b.Ep[(size_t)i * He + k] = past ? e[k] : 0.f;
}

// ---- 3. g gate + context attention --------------------------------------------------------------------------------------------
struct AttnPrm {
    const float* q_const;     // simple: scalar.weight [H]
    const float* Wg;          // concat: transform.weight (memory columns first), leading dimension ldw
    const float* v;           // concat: vector_prod.weight [Da]
    int ldw, Da;
};

// scores s_j = <q, g_j>, j < t: wave w takes history rows w, w + 16, ... two at a time (16 row loads in flight per lane)
__device__ __forceinline__ void stream_scores(const float* __restrict__ q, const float* __restrict__ Gs, int H, int t, float* __restrict__ out,
                                              int lane, int w) {
    float qr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) qr[i] = lane + 64 * i < H ? q[lane + 64 * i] : 0.f;
    for (int j0 = w; j0 < t; j0 += 2 * DS_WAVES) {
        const int j1 = min(j0 + DS_WAVES, t - 1);
        const float* g0 = Gs + (size_t)j0 * H;
        const float* g1 = Gs + (size_t)j1 * H;
        float v0[8], v1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = min(lane + 64 * i, H - 1);
            v0[i] = g0[k];
            v1[i] = g1[k];
        }
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { s0 += qr[i] * v0[i]; s1 += qr[i] * v1[i]; }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) {
            out[j0] = s0;
            if (j0 + DS_WAVES < t) out[j0 + DS_WAVES] = s1;
        }
    }
}
// concat: s_j = sum_a v_a tanh(<Wg[a], g_j> + X[a]).  The state keeps no projected history, so W_g g_j is formed here: a wave holds
// two history rows in registers and walks the D_a weight rows (shared by every wave and row of the launch: they stay in cache)
__device__ __forceinline__ void stream_concat_scores(const AttnPrm& ap, const float* __restrict__ X, const float* __restrict__ Gs, int H, int t,
                                                     float* __restrict__ out, int lane, int w) {
    for (int j0 = w; j0 < t; j0 += 2 * DS_WAVES) {
        const int j1 = min(j0 + DS_WAVES, t - 1);
        const float* g0 = Gs + (size_t)j0 * H;
        const float* g1 = Gs + (size_t)j1 * H;
        float v0[8], v1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = lane + 64 * i;
            v0[i] = k < H ? g0[k] : 0.f;
            v1[i] = k < H ? g1[k] : 0.f;
        }
        float s0 = 0.f, s1 = 0.f;
        for (int a = 0; a < ap.Da; ++a) {
            const float* wr = ap.Wg + (size_t)a * ap.ldw;
            float wv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) wv[i] = wr[min(lane + 64 * i, H - 1)];
            float d0 = 0.f, d1 = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) { d0 += wv[i] * v0[i]; d1 += wv[i] * v1[i]; }
            d0 = wave_sum(d0);
            d1 = wave_sum(d1);
            const float va = ap.v[a], xa = X[a];
            s0 += va * tanhf(d0 + xa);
            s1 += va * tanhf(d1 + xa);
        }
        if (lane == 0) {
            out[j0] = s0;
            if (j0 + DS_WAVES < t) out[j0 + DS_WAVES] = s1;
        }
    }
}

template <int ATT>
__global__ __launch_bounds__(DS_NT) void drnn_stream_gate_attn_kernel(RowIdx r, StepBufs b, AttnPrm ap, const float* __restrict__ U, int Dm, int H) {
    __shared__ float sc[128];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int s = 0, t = 0, sp = 0;
    if (!row_live(r, i, s, t, sp)) {                  // (workgroup-uniform) the product that reads CT gets a finite row
        if (tid < H) b.CT[(size_t)i * H + tid] = 0.f;
        return;
    }
    float* const Gs = b.G + (size_t)s * r.max_len * H;          // the slot's history; row t is this step's
    if (tid < H)
        Gs[(size_t)t * H + tid] = gru_col(b.GIg + (size_t)i * 3 * H, b.GHg + (size_t)i * 3 * H, H, tid, b.Gp[(size_t)i * H + tid]);
    if (t == 0) {                                     // no history: c = 0
        if (tid < H) b.CT[(size_t)i * H + tid] = 0.f;
        return;
    }
    // scores over g_0 .. g_{t-1} (row t, written above, is not among them)
    if constexpr (ATT == ATT_CONCAT) stream_concat_scores(ap, b.XA + (size_t)i * ap.Da, Gs, H, t, sc, lane, w);
    else if constexpr (ATT == ATT_SIMPLE) stream_scores(ap.q_const, Gs, H, t, sc, lane, w);
    else if constexpr (ATT == ATT_DOT) stream_scores(U + (size_t)i * Dm, Gs, H, t, sc, lane, w);
    else stream_scores(b.XA + (size_t)i * H, Gs, H, t, sc, lane, w);
    __syncthreads();
    // softmax over t <= 110 scores: every wave forms the same maximum and sum from the same words in the same order
    float v0 = lane < t ? sc[lane] : -INFINITY, v1 = lane + 64 < t ? sc[lane + 64] : -INFINITY;
    if (ATT == ATT_GENERAL2) {
        v0 = lane < t ? tanhf(v0) : -INFINITY;
        v1 = lane + 64 < t ? tanhf(v1) : -INFINITY;
    }
    const float m = wave_max(fmaxf(v0, v1));
    const float e0 = lane < t ? __expf(v0 - m) : 0.f, e1 = lane + 64 < t ? __expf(v1 - m) : 0.f;
    const float inv = 1.0f / wave_sum(e0 + e1);
    __syncthreads();
    if (w == 0) {
        sc[lane] = e0 * inv;
        sc[lane + 64] = e1 * inv;
    }
    __syncthreads();
    // context: c_k = sum_j alpha_j g_j[k], one column per thread, 8 history rows in flight
    if (tid < H) {
        const float* gk = Gs + tid;
        float c = 0.f;
        for (int j = 0; j < t; j += 8) {
            float g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) g[u] = gk[(size_t)min(j + u, t - 1) * H];
#pragma unroll
            for (int u = 0; u < 8; ++u) c += (j + u < t ? sc[j + u] : 0.f) * g[u];
        }
        b.CT[(size_t)i * H + tid] = c;
    }
}

// ---- 5. party gate ----------------------------------------------------------------------------------------------------------
template <bool LISTENER>
__global__ __launch_bounds__(DS_NT) void drnn_stream_party_kernel(RowIdx r, StepBufs b, int Dm, int H) {
    const int i = blockIdx.x, k = threadIdx.x, P = r.parties;
    int s = 0, t = 0, sp = 0;
    const bool live = row_live(r, i, s, t, sp);
    if (k >= H) return;
    if (!live) {
        b.QS[(size_t)i * H + k] = 0.f;
        return;
    }
    const float qs = gru_col(b.GIp + (size_t)i * 3 * H, b.GHp + (size_t)i * 3 * H, H, k, b.Acat[(size_t)i * (Dm + H) + Dm + k]);
    b.QS[(size_t)i * H + k] = qs;
    if (!LISTENER) {                                  // the speaker's row takes qs, the others keep their state (zeros at t = 0)
        float* q = b.Q + (size_t)s * P * H + k;
        const float* qg = b.Qg + (size_t)i * P * H + k;
        for (int pa = 0; pa < P; ++pa) q[(size_t)pa * H] = pa == sp ? qs : qg[(size_t)pa * H];
    }
}

// ---- 7. emotion gate (+ listener gates and the blend) ----------------------------------------------------------------------------
template <bool LISTENER>
__global__ __launch_bounds__(DS_NT) void drnn_stream_emotion_kernel(RowIdx r, StepBufs b, float* __restrict__ e_out, int H, int He) {
    const int i = blockIdx.x, P = r.parties;
    int s = 0, t = 0, sp = 0;
    const bool live = row_live(r, i, s, t, sp);
    float* const eo = e_out + (size_t)i * He;
    if (!live) {
        for (int k = threadIdx.x; k < He; k += DS_NT) eo[k] = 0.f;
        return;
    }
    float* const es = b.E + ((size_t)s * r.max_len + t) * He;
    for (int k = threadIdx.x; k < He; k += DS_NT) {
        const float e = gru_col(b.GIe + (size_t)i * 3 * He, b.GHe + (size_t)i * 3 * He, He, k, b.Ep[(size_t)i * He + k]);
        es[k] = e;
        eo[k] = e;
    }
    if (LISTENER) {            // every party row takes a listener step from its old state; the speaker's row takes qs instead
        for (int idx = threadIdx.x; idx < P * H; idx += DS_NT) {
            const int pa = idx / H, u = idx - pa * H;
            const float ql = gru_col(b.GIl + (size_t)i * 3 * H, b.GHl + ((size_t)i * P + pa) * 3 * H, H, u, b.Qg[(size_t)i * P * H + idx]);
            b.Q[(size_t)s * P * H + idx] = pa == sp ? b.QS[(size_t)i * H + u] : ql;
        }
    }
}

// ---- the second attention of new rows: single-query general2 over a slot's emotion history ---------------------------------
// One workgroup per (row i, chunk step j): keys E[s][0 .. pos[s] + j].  Scores: wave w takes keys w, w + 32, ... two at a time (sixteen waves: three passes at 94 keys), lanes
// split D in float4 words (8 loads in flight); alpha_k = e^{tanh(s_k)} / sum (tanh bounds the scores: no maximum needed); pooling:
// one float4 column word per thread, 8 key rows in flight.
constexpr int G2_NT = 1024;
constexpr int G2_WAVES = G2_NT / 64;
__global__ __launch_bounds__(G2_NT) void general2_stream_kernel(const float* __restrict__ x, const float* __restrict__ e_hist,
                                                                const int32_t* __restrict__ slot, const int32_t* __restrict__ count,
                                                                const int32_t* __restrict__ pos, float* __restrict__ att,
                                                                float* __restrict__ alpha, int n, int m, int capacity, int max_len, int D) {
    __shared__ float sc[128];
    const int i = blockIdx.x, j = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t row = (size_t)j * n + i;
    const int D4 = D >> 2;
    float4* const arow = reinterpret_cast<float4*>(att + row * D);
    float* const al = alpha ? alpha + row * max_len : nullptr;
    const int s = slot[i];
    int p0 = -1;
    if (s >= 0 && s < capacity) p0 = pos[s];
    const int c = count ? count[i] : 1;
    const bool live = p0 >= 0 && p0 < max_len && j < c && j < max_len - p0;
    if (!live) {
        if (tid < D4) arow[tid] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (al) for (int k = tid; k < max_len; k += G2_NT) al[k] = 0.f;
        return;
    }
    const int nk = p0 + j + 1;                         // 1 .. max_len keys
    const float* const Es = e_hist + (size_t)s * max_len * D;
    const float4* const x4 = reinterpret_cast<const float4*>(x + row * D);
    float4 xr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xr[u] = lane + 64 * u < D4 ? x4[lane + 64 * u] : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k0 = w; k0 < nk; k0 += 2 * G2_WAVES) {
        const int k1 = min(k0 + G2_WAVES, nk - 1);
        const float4* e0 = reinterpret_cast<const float4*>(Es + (size_t)k0 * D);
        const float4* e1 = reinterpret_cast<const float4*>(Es + (size_t)k1 * D);
        float4 a[4], bq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = min(lane + 64 * u, D4 - 1);
            a[u] = e0[q];
            bq[u] = e1[q];
        }
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            s0 += xr[u].x * a[u].x + xr[u].y * a[u].y + xr[u].z * a[u].z + xr[u].w * a[u].w;
            s1 += xr[u].x * bq[u].x + xr[u].y * bq[u].y + xr[u].z * bq[u].z + xr[u].w * bq[u].w;
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) {
            sc[k0] = s0;
            if (k0 + G2_WAVES < nk) sc[k0 + G2_WAVES] = s1;
        }
    }
    __syncthreads();
    const float e0 = lane < nk ? expf(tanhf(sc[lane])) : 0.f, e1 = lane + 64 < nk ? expf(tanhf(sc[lane + 64])) : 0.f;
    const float inv = 1.0f / wave_sum(e0 + e1);        // (every wave: the same words in the same order)
    __syncthreads();
    if (w == 0) {
        sc[lane] = e0 * inv;
        sc[lane + 64] = e1 * inv;
    }
    __syncthreads();
    if (al) for (int k = tid; k < max_len; k += G2_NT) al[k] = k < nk ? sc[k] : 0.f;
    if (tid < D4) {
        const float4* ek = reinterpret_cast<const float4*>(Es) + tid;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int k = 0; k < nk; k += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ek[(size_t)min(k + u, nk - 1) * D4];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float p = k + u < nk ? sc[k + u] : 0.f;
                acc.x += p * v[u].x;
                acc.y += p * v[u].y;
                acc.z += p * v[u].z;
                acc.w += p * v[u].w;
            }
        }
        arow[tid] = acc;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
static int check_cfg(const ganffn_drnn_stream_cfg* c) {
    GF_CHECK_ARG(c, "drnn_stream: null cfg");
    GF_CHECK_ARG(c->capacity >= 1 && c->capacity <= GANFFN_MAX_DIALOGUES, "drnn_stream: capacity=%d out of range [1,%d]", c->capacity,
                 GANFFN_MAX_DIALOGUES);
    GF_CHECK_ARG(c->max_len >= 1 && c->max_len <= DS_MAXLEN, "drnn_stream: max_len=%d out of range [1,%d]", c->max_len, DS_MAXLEN);
    GF_CHECK_ARG(c->parties >= 1 && c->parties <= GANFFN_DRNN_MAX_PARTIES, "drnn_stream: parties=%d outside [1, %d] (GANFFN_DRNN_MAX_PARTIES)",
                 c->parties, GANFFN_DRNN_MAX_PARTIES);
    GF_CHECK_ARG(c->Dm >= 4 && (c->Dm & 3) == 0 && c->H >= 4 && (c->H & 3) == 0 && c->He >= 4 && (c->He & 3) == 0,
                 "drnn_stream: D_m=%d, D_g=D_p=%d, D_e=%d must be multiples of 4", c->Dm, c->H, c->He);
    GF_CHECK_ARG(c->H <= 512, "drnn_stream: D_g = D_p = %d > 512 (the step kernels hold one column per thread)", c->H);
    GF_CHECK_ARG(c->listener == 0 || c->listener == 1, "drnn_stream: listener=%d (0 / 1)", c->listener);
    // the attention descriptor, under the rules of the recurrence (check_att in dialogue_rnn.hip)
    const ganffn_drnn_att& at = c->att;
    GF_CHECK_ARG(at.type >= GANFFN_DRNN_ATT_GENERAL && at.type <= GANFFN_DRNN_ATT_CONCAT,
                 "drnn_stream: unknown attention type %d (0 general, 1 simple, 2 dot, 3 general2, 4 concat)", at.type);
    GF_CHECK_ARG(at.type != GANFFN_DRNN_ATT_CONCAT || (at.Da >= 4 && at.Da <= DS_MAXDA && (at.Da & 3) == 0),
                 "drnn_stream: concat needs D_a a multiple of 4 in [4, %d], got D_a=%d", DS_MAXDA, at.Da);
    GF_CHECK_ARG(at.type != GANFFN_DRNN_ATT_DOT || c->Dm == c->H, "drnn_stream: dot attention needs D_m == D_g, got D_m=%d D_g=%d", c->Dm,
                 c->H);
    return 0;
}

struct StateLayout { int64_t G, Q, E, total; };
static StateLayout state_layout(const ganffn_drnn_stream_cfg* c) {
    StateLayout L;
    L.G = 0;
    L.Q = L.G + a4((int64_t)c->capacity * c->max_len * c->H);
    L.E = L.Q + a4((int64_t)c->capacity * c->parties * c->H);
    L.total = L.E + a4((int64_t)c->capacity * c->max_len * c->He);
    return L;
}
// carve the workspace of n rows; returns its size in floats (ws may be null: size only)
static int64_t carve(const ganffn_drnn_stream_cfg* c, int n, float* ws, StepBufs& b) {
    int64_t o = 0;
    const int64_t H = c->H, Dm = c->Dm, He = c->He, P = c->parties;
    auto take = [&](int64_t floats) { float* p = ws ? ws + o : nullptr; o += a4(floats); return p; };
    b.Acat = take(n * (Dm + H)); b.Gp = take(n * H); b.Ep = take(n * He); b.Qg = take(n * P * H);
    b.GIg = take(n * 3 * H); b.GHg = take(n * 3 * H); b.GHp = take(n * 3 * H); b.XP = take(n * 3 * H); b.GIp = take(n * 3 * H);
    b.XA = take(n * (c->att.type == ATT_CONCAT ? (int64_t)c->att.Da : H));
    b.CT = take(n * H); b.QS = take(n * H);
    b.GIe = take(n * 3 * He); b.GHe = take(n * 3 * He);
    b.XL = b.GIl = b.GHl = nullptr;
    if (c->listener) { b.XL = take(n * 3 * H); b.GIl = take(n * 3 * H); b.GHl = take(n * P * 3 * H); }
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
    const ganffn_drnn_stream_cfg* c; int n;
    const int32_t *slot, *pos, *count, *spk;
    const ganffn_drnn_params* prm; const ganffn_drnn_listener_params* lprm; const ganffn_drnn_att_params* aprm;
    float *state, *workspace; hipStream_t st;
};
// every refusal of a step or an extend, before any launch
static int check_step(const StepCall& k, const char* what, const float* U, const float* e_out) {
    GF_TRY(check_cfg(k.c));
    GF_CHECK_ARG(k.n >= 1 && k.n <= k.c->capacity, "%s: n=%d out of range [1, capacity=%d]", what, k.n, k.c->capacity);
    GF_CHECK_ARG(k.slot && k.pos && k.spk && U && k.prm && k.state && e_out && k.workspace, "%s: null pointer", what);
    GF_CHECK_ARG(aligned16(U) && aligned16(k.state) && aligned16(e_out) && aligned16(k.workspace), "%s: buffers must be 16-byte aligned", what);
    const ganffn_drnn_params& p = *k.prm;
    GF_CHECK_ARG(p.g_wih && p.g_whh && p.g_bih && p.g_bhh && p.p_wih && p.p_whh && p.p_bih && p.p_bhh && p.e_wih && p.e_whh && p.e_bih && p.e_bhh,
                 "%s: null cell parameter", what);
    GF_CHECK_ARG(aligned16(p.g_wih) && aligned16(p.g_whh) && aligned16(p.p_wih) && aligned16(p.p_whh) && aligned16(p.e_wih) && aligned16(p.e_whh),
                 "%s: cell weights must be 16-byte aligned", what);
    if (k.c->listener) {
        GF_CHECK_ARG(k.lprm && k.lprm->l_wih && k.lprm->l_whh && k.lprm->l_bih && k.lprm->l_bhh, "%s: listener state needs the l_cell tensors", what);
        GF_CHECK_ARG(aligned16(k.lprm->l_wih) && aligned16(k.lprm->l_whh), "%s: listener weights must be 16-byte aligned", what);
    }
    const int at = k.c->att.type;
    if (at != ATT_DOT) {
        GF_CHECK_ARG(k.aprm && k.aprm->w && aligned16(k.aprm->w), "%s: null or misaligned attention weight", what);
        GF_CHECK_ARG(at != ATT_GENERAL2 || k.aprm->b, "%s: general2 attention needs transform.bias", what);
        GF_CHECK_ARG(at != ATT_CONCAT || k.aprm->v, "%s: concat attention needs vector_prod.weight", what);
    }
    return 0;
}

// the launches of one step over rows that check_step has accepted
static int step_launches(const StepCall& k, int off, const float* U, const int32_t* spk, float* e_out) {
    const ganffn_drnn_stream_cfg* c = k.c;
    const int n = k.n, H = c->H, Dm = c->Dm, He = c->He, P = c->parties, at = c->att.type, H3 = 3 * H, ldi = Dm + H;
    StepBufs b;
    carve(c, n, k.workspace, b);
    const StateLayout L = state_layout(c);
    b.G = k.state + L.G; b.Q = k.state + L.Q; b.E = k.state + L.E;
    const RowIdx r{k.slot, k.pos, k.count, spk, off, c->capacity, c->max_len, P};
    const ganffn_drnn_params& p = *k.prm;

    hipLaunchKernelGGL(drnn_stream_gather_kernel, dim3(n), dim3(256), 0, k.st, r, b, U, Dm, H, He);
    GF_LAUNCH_CHECK();

    // everything that depends on neither g_t, c_t nor qs
    SkinnyProb pr[8 + GANFFN_DRNN_MAX_PARTIES];
    int np = 0;
    pr[np++] = prob(b.Acat, ldi, p.g_wih, ldi, nullptr, p.g_bih, b.GIg, H3, n, H3, ldi);              // g cell: [U, q[spk]] W_ih^T
    pr[np++] = prob(b.Gp, H, p.g_whh, H, nullptr, p.g_bhh, b.GHg, H3, n, H3, H);                      // g cell: g_{t-1} W_hh^T
    pr[np++] = prob(b.Acat + Dm, ldi, p.p_whh, H, nullptr, p.p_bhh, b.GHp, H3, n, H3, H);             // party cell: q[spk] W_hh^T
    pr[np++] = prob(b.Acat, ldi, p.p_wih, ldi, nullptr, p.p_bih, b.XP, H3, n, H3, Dm);                // party cell: U part
    pr[np++] = prob(b.Ep, He, p.e_whh, He, nullptr, p.e_bhh, b.GHe, 3 * He, n, 3 * He, He);           // e cell: e_{t-1} W_hh^T
    if (at == ATT_GENERAL || at == ATT_GENERAL2)
        pr[np++] = prob(b.Acat, ldi, k.aprm->w, Dm, nullptr, at == ATT_GENERAL2 ? k.aprm->b : nullptr, b.XA, H, n, H, Dm);
    else if (at == ATT_CONCAT)                                                                        // X = U W_u^T, W_u = w[:, H:]
        pr[np++] = prob(b.Acat, ldi, k.aprm->w + H, H + Dm, nullptr, nullptr, b.XA, c->att.Da, n, c->att.Da, Dm);
    if (c->listener) {
        pr[np++] = prob(b.Acat, ldi, k.lprm->l_wih, ldi, nullptr, k.lprm->l_bih, b.XL, H3, n, H3, Dm); // listener: U part
        for (int pa = 0; pa < P; ++pa)                                                                // listener: q[pa] W_hh^T
            pr[np++] = prob(b.Qg + (size_t)pa * H, P * H, k.lprm->l_whh, H, nullptr, k.lprm->l_bhh, b.GHl + (size_t)pa * H3, P * H3, n, H3, H);
    }
    GF_TRY(launch_probs(pr, np, k.st));

    AttnPrm ap{};
    if (at == ATT_SIMPLE) ap.q_const = k.aprm->w;
    if (at == ATT_CONCAT) { ap.Wg = k.aprm->w; ap.v = k.aprm->v; ap.ldw = H + Dm; ap.Da = c->att.Da; }
#define GF_DS_GATE_ATTN(ATT_) hipLaunchKernelGGL(drnn_stream_gate_attn_kernel<ATT_>, dim3(n), dim3(DS_NT), 0, k.st, r, b, ap, U, Dm, H)
    switch (at) {
        case ATT_GENERAL: GF_DS_GATE_ATTN(ATT_GENERAL); break;
        case ATT_SIMPLE: GF_DS_GATE_ATTN(ATT_SIMPLE); break;
        case ATT_DOT: GF_DS_GATE_ATTN(ATT_DOT); break;
        case ATT_GENERAL2: GF_DS_GATE_ATTN(ATT_GENERAL2); break;
        default: GF_DS_GATE_ATTN(ATT_CONCAT); break;
    }
#undef GF_DS_GATE_ATTN
    GF_LAUNCH_CHECK();

    pr[0] = prob(b.CT, H, p.p_wih + Dm, ldi, b.XP, nullptr, b.GIp, H3, n, H3, H);                     // party cell: c_t part + U part
    GF_TRY(launch_probs(pr, 1, k.st));
    if (c->listener) hipLaunchKernelGGL(drnn_stream_party_kernel<true>, dim3(n), dim3(DS_NT), 0, k.st, r, b, Dm, H);
    else hipLaunchKernelGGL(drnn_stream_party_kernel<false>, dim3(n), dim3(DS_NT), 0, k.st, r, b, Dm, H);
    GF_LAUNCH_CHECK();

    np = 0;
    pr[np++] = prob(b.QS, H, p.e_wih, H, nullptr, p.e_bih, b.GIe, 3 * He, n, 3 * He, H);              // e cell: qs W_ih^T
    if (c->listener) pr[np++] = prob(b.QS, H, k.lprm->l_wih + Dm, ldi, b.XL, nullptr, b.GIl, H3, n, H3, H);   // listener: qs part + U part
    GF_TRY(launch_probs(pr, np, k.st));
    if (c->listener) hipLaunchKernelGGL(drnn_stream_emotion_kernel<true>, dim3(n), dim3(DS_NT), 0, k.st, r, b, e_out, H, He);
    else hipLaunchKernelGGL(drnn_stream_emotion_kernel<false>, dim3(n), dim3(DS_NT), 0, k.st, r, b, e_out, H, He);
    GF_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int64_t ganffn_drnn_stream_state_floats(const ganffn_drnn_stream_cfg* c) {
    return check_cfg(c) ? -1 : state_layout(c).total;
}
extern "C" int64_t ganffn_drnn_stream_workspace_floats(const ganffn_drnn_stream_cfg* c, int n_max) {
    if (check_cfg(c)) return -1;
    if (n_max < 1 || n_max > c->capacity) return fail(-1, "drnn_stream: n_max=%d out of range [1, capacity=%d]", n_max, c->capacity);
    StepBufs b;
    return carve(c, n_max, nullptr, b);
}

extern "C" int ganffn_drnn_stream_step(const ganffn_drnn_stream_cfg* cfg, int n, const int32_t* slot, const int32_t* pos, int off,
                                       const int32_t* count, const int32_t* spk, const float* U, const ganffn_drnn_params* prm,
                                       const ganffn_drnn_listener_params* lprm, const ganffn_drnn_att_params* aprm, float* state,
                                       float* e_out, float* workspace, void* stream) {
    const StepCall k{cfg, n, slot, pos, count, spk, prm, lprm, aprm, state, workspace, (hipStream_t)stream};
    GF_TRY(check_step(k, "drnn_stream_step", U, e_out));
    GF_CHECK_ARG(off >= 0 && off < cfg->max_len, "drnn_stream_step: off=%d out of range [0, max_len=%d)", off, cfg->max_len);
    return step_launches(k, off, U, spk, e_out);
}

extern "C" int ganffn_drnn_stream_extend(const ganffn_drnn_stream_cfg* cfg, int n, int m, const int32_t* slot, const int32_t* count,
                                         const int32_t* pos, const int32_t* spk, const float* U, const ganffn_drnn_params* prm,
                                         const ganffn_drnn_listener_params* lprm, const ganffn_drnn_att_params* aprm, float* state,
                                         float* e_out, float* workspace, void* stream) {
    const StepCall k{cfg, n, slot, pos, count, spk, prm, lprm, aprm, state, workspace, (hipStream_t)stream};
    GF_TRY(check_step(k, "drnn_stream_extend", U, e_out));
    GF_CHECK_ARG(count, "drnn_stream_extend: null pointer (count)");
    GF_CHECK_ARG(m >= 1 && m <= cfg->max_len, "drnn_stream_extend: m=%d out of range [1, max_len=%d]", m, cfg->max_len);
    // the recurrence is serial in t: the step, m times, on the rows of chunk step j (time-major), no host synchronisation
    for (int j = 0; j < m; ++j)
        GF_TRY(step_launches(k, j, U + (size_t)j * n * cfg->Dm, spk + (size_t)j * n, e_out + (size_t)j * n * cfg->He));
    return 0;
}

extern "C" int ganffn_general2_stream_attention(const float* x, const float* e_hist, const int32_t* slot, const int32_t* count,
                                                const int32_t* pos, float* att, float* alpha, int n, int m, int capacity, int max_len,
                                                int D, void* stream) {
    GF_CHECK_ARG(x && e_hist && slot && pos && att, "general2_stream_attention: null pointer");
    GF_CHECK_ARG(capacity >= 1 && capacity <= GANFFN_MAX_DIALOGUES && n >= 1 && n <= capacity,
                 "general2_stream_attention: n=%d capacity=%d (1 <= n <= capacity <= %d)", n, capacity, GANFFN_MAX_DIALOGUES);
    GF_CHECK_ARG(max_len >= 1 && max_len <= DS_MAXLEN, "general2_stream_attention: max_len=%d out of range [1,%d]", max_len, DS_MAXLEN);
    GF_CHECK_ARG(m >= 1 && m <= max_len, "general2_stream_attention: m=%d out of range [1,max_len=%d]", m, max_len);
    GF_CHECK_ARG(D >= 4 && (D & 3) == 0 && D <= 1024, "general2_stream_attention: D=%d must be a multiple of 4 in [4, 1024]", D);
    GF_CHECK_ARG(aligned16(x) && aligned16(e_hist) && aligned16(att), "general2_stream_attention: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(general2_stream_kernel, dim3(n, m), dim3(G2_NT), 0, (hipStream_t)stream, x, e_hist, slot, count, pos, att, alpha, n,
                       m, capacity, max_len, D);
    GF_LAUNCH_CHECK();
    return 0;
}

}  // namespace ganffn
