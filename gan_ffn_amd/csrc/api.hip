// api.hip — C ABI of libganffn.so (declared in include/ganffn.h): argument checking and the launch
// sequences of the encoder stack, the heads and the plain linears.  No allocation, no synchronisation.
#include "common.h"

#include <string.h>
#include <algorithm>

namespace ganffn {

static thread_local char g_err[512] = "";
char* err_buf() { return g_err; }
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// from elementwise.hip
int launch_gelu_bwd_drop(const float* d, const float* u, float* out, int R, int C, float p, uint32_t site,
                         const uint64_t* rng, uint64_t add, int train, hipStream_t st);
int launch_disc_tail_fwd(const float* a2, const float* w3, const float* b3, float* prob, int T, int D2, float p,
                         const uint64_t* rng, uint64_t add, int train, hipStream_t st);
int launch_disc_tail_bwd(const float* dprob, const float* prob, const float* a2, const float* u2, const float* w3,
                         float* d_pre2, float* gw3, float* gb3, int T, int D2, float p, const uint64_t* rng, uint64_t add,
                         int train, hipStream_t st, float* gpart);
int launch_disc_tail_reduce(const float* gpart, int nblk_, int D2, float* gw3, float* gb3, hipStream_t st);
// disc_head.hip: the d_model-100 discriminator head (100 -> 64 -> 16 -> 1) as one kernel per direction
bool disc_head_fused_supported(int E, int D1, int D2);
int disc_head_blocks(int T);
int launch_disc_head_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                         const float* b3, float* g0, float* u1, float* a1, float* u2, float* a2, float* prob, float* out, int T,
                         float p, const uint64_t* rng, uint64_t add, int train, hipStream_t st);
int launch_disc_head_bwd(const float* dprob, const float* x, const float* w1, const float* w2, const float* w3, const float* u1,
                         const float* u2, const float* a2, const float* prob, float* dx, float* d_pre1, float* d_pre2, float* gpart,
                         int T, float p, const uint64_t* rng, uint64_t add, int train, hipStream_t st);
int launch_small_linear_fwd(const float* x, const float* w, const float* b, float* y, int T, int K, int N, hipStream_t st);
int launch_small_linear_bwd(const float* dy, const float* x, const float* w, float* dx, float* gw, float* gb, int T, int K,
                            int N, hipStream_t st);

// ------------------------------------------------------------------------------------------
// parameter slab layout of one encoder layer
// ------------------------------------------------------------------------------------------
struct LayerOff {
    int64_t in_w, in_b, out_w, out_b, w1, b1, w2, b2, n1w, n1b, n2w, n2b, total;
};
static LayerOff layer_off(int E, int F) {
    LayerOff o;
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t r = p; p += (n + 3) & ~int64_t(3); return r; };
    o.in_w = take((int64_t)3 * E * E);
    o.in_b = take(3 * E);
    o.out_w = take((int64_t)E * E);
    o.out_b = take(E);
    o.w1 = take((int64_t)F * E);
    o.b1 = take(F);
    o.w2 = take((int64_t)E * F);
    o.b2 = take(E);
    o.n1w = take(E);
    o.n1b = take(E);
    o.n2w = take(E);
    o.n2b = take(E);
    o.total = p;
    return o;
}

// ------------------------------------------------------------------------------------------
// saved-for-backward layout of one encoder stack
//   X[0..L]      (L+1) * T*E     X[0] = PE output, X[l+1] = output of layer l
//   per layer:   qkv 3TE | attn_o TE | x1 TE | xhat1 TE | xhat2 TE | h TF | rstd1 T4 | rstd2 T4 | lse (T H)4 | keep B H 448
// ------------------------------------------------------------------------------------------
struct SavedOff {
    int64_t X, layers, per_layer, qkv, attn_o, x1, xhat1, xhat2, h, rstd1, rstd2, lse, keep, hmask, total;
};
static SavedOff saved_off(const ganffn_enc_cfg* c) {
    SavedOff s;
    const int64_t T = (int64_t)c->S * c->B, TE = T * c->E, TF = T * c->F, T4 = (T + 3) & ~int64_t(3);
    s.X = 0;
    s.layers = (int64_t)(c->L + 1) * TE;
    int64_t p = 0;
    s.qkv = p; p += 3 * TE;
    s.attn_o = p; p += TE;
    s.x1 = p; p += TE;
    s.xhat1 = p; p += TE;
    s.xhat2 = p; p += TE;
    s.h = p; p += TF;
    s.rstd1 = p; p += T4;
    s.rstd2 = p; p += T4;
    s.lse = p; p += (T * c->H + 3) & ~int64_t(3);     // attention log-sum-exp [B*H x S]
    s.keep = p; p += (int64_t)c->B * c->H * ATTN_KEEP_WORDS;   // attention-dropout keep words (uint32) of a train-mode pass
    s.hmask = p; p += (epi_mask_words(T, c->F) / 2 + 3) & ~int64_t(3);   // [h > 0] of the hidden activation, 1 bit each (uint16 words)
    s.per_layer = p;
    s.total = s.layers + (int64_t)c->L * s.per_layer;
    return s;
}

static int check_cfg(const ganffn_enc_cfg* c) {
    GF_CHECK_ARG(c, "null cfg");
    GF_CHECK_ARG(c->S >= 1 && c->S <= 110, "S=%d out of range [1,110] (PositionalEncoding max_len, model.py:1179)", c->S);
    GF_CHECK_ARG(c->B >= 1, "B=%d", c->B);
    GF_CHECK_ARG(c->E >= 4 && (c->E & 3) == 0 && c->E <= 640, "E=%d must be a multiple of 4 and <= 640", c->E);
    GF_CHECK_ARG(c->H >= 1 && c->E % c->H == 0, "E=%d not divisible by H=%d", c->E, c->H);
    GF_CHECK_ARG(c->F >= 4 && (c->F & 3) == 0, "F=%d must be a multiple of 4", c->F);
    GF_CHECK_ARG(c->L >= 1 && c->L <= 64, "L=%d", c->L);
    GF_CHECK_ARG(c->p_pe >= 0.f && c->p_pe < 1.f && c->p_enc >= 0.f && c->p_enc < 1.f, "dropout p out of [0,1)");
    return 0;
}

// A/B switches: one atomic word (common.h `Mode`); what each bit selects and what was measured is in include/ganffn.h and
// DESIGN.md section 6.
std::atomic<uint32_t> g_mode_word{0};
GF_LAB_ONLY(extern unsigned long long* g_n100_stamps; extern unsigned long long* g_wres_stamps;)
constexpr int MAX_SPLITS = 16;  // partial-output slabs: K chunks of gemm_n100 (<= 16) / split-K GEMMs (<= 8)
static_assert(MAX_SPLITS <= LN_MAXSLAB, "the LayerNorm kernels sum every slab a split rule may write");

static int64_t a4(int64_t n) { return (n + 3) & ~int64_t(3); }

// per LayerNorm backward launch: per-block partial sums of the weight / bias gradient
static int64_t ln_part_floats(const ganffn_enc_cfg* c) {
    const int T = c->S * c->B;
    return (int64_t)row_blocks_any_plan(T) * 2 * c->E;
}

// Slack terms of the size functions, in floats.  REGION_SLACK follows the grouped-wgrad parts and the rowchain weight pack: it paid
// for re-aligning the next region by address; every offset of BwdLayout is a multiple of 4 floats (E and F are), so it pays for
// nothing and is kept only so that the sizes do not change.  TAIL_SLACK ends every encoder and head workspace: no region of a
// layout reaches into it, and it too is kept only so that the sizes do not change.
constexpr int64_t REGION_SLACK = 8, TAIL_SLACK = 64;

// workspace of a forward segment that keeps nothing, over the T = S B rows of c (a streaming pass: S = 1, B = rows):
//   X ping-pong [2][T x E] | layer: one layer's saved set (SavedOff), reused by every layer | tmp: slabs [MAX_SPLITS][T x E]
// slabs: the float count of tmp, and of the second segment's slabs that a two-segment pass keeps behind `total`
struct UnsavedLayout { int64_t TE, X, layer, tmp, slabs, total; };
static UnsavedLayout unsaved_layout(const ganffn_enc_cfg* c) {
    UnsavedLayout u;
    u.TE = (int64_t)c->S * c->B * c->E;
    u.X = 0; u.layer = 2 * u.TE; u.tmp = u.layer + saved_off(c).per_layer; u.slabs = MAX_SPLITS * u.TE; u.total = u.tmp + u.slabs;
    return u;
}

// workspace of the backward over a layer range; i = l - layer_lo counts the range's layers from its bottom:
//   L sets of dh [T x F] | dyA [T x E] | dyB [T x E] | d_qkv [T x 3E], what layer i's four weight-gradient GEMMs read |
//   dz2 | dz1 | d_attn [T x E] each | tmp [MAX_SPLITS][T x E] | lnp: LayerNorm partial-sum blocks [L][2 (LN2, LN1)][LNP] |
//   tnp: partial slabs of the grouped weight-gradient launch | rcw [L][RCW]: transposed {in-proj, out-proj} weights (d_model 100)
struct BwdLayout {
    int64_t TE, TF, SET, LNP, RCW, dz2, dz1, d_attn, tmp, lnp, tnp, rcw, total;
    int64_t dh(int i) const { return i * SET; }
    int64_t dyA(int i) const { return dh(i) + TF; }
    int64_t dyB(int i) const { return dyA(i) + TE; }
    int64_t d_qkv(int i) const { return dyB(i) + TE; }
    int64_t d_qkv_above(int i) const { return d_qkv(i + 1); }   // the rowchain LN2 backward runs the in-proj dgrad of the layer above
    int64_t lnp2(int i) const { return lnp + 2 * i * LNP; }
    int64_t lnp1(int i) const { return lnp2(i) + LNP; }
    int64_t rcw_layer(int i) const { return rcw + i * RCW; }
};
static BwdLayout bwd_layout(const ganffn_enc_cfg* c) {
    BwdLayout b;
    const int64_t T = (int64_t)c->S * c->B, L = c->L;
    b.TE = T * c->E; b.TF = T * c->F; b.SET = b.TF + 5 * b.TE; b.LNP = ln_part_floats(c); b.RCW = rc_pack_floats();
    b.dz2 = L * b.SET; b.dz1 = b.dz2 + b.TE; b.d_attn = b.dz1 + b.TE; b.tmp = b.d_attn + b.TE; b.lnp = b.tmp + MAX_SPLITS * b.TE;
    b.tnp = a4(b.lnp + L * 2 * b.LNP);
    b.rcw = a4(b.tnp + gemm_tn_grouped_part_floats());
    b.total = b.rcw + REGION_SLACK + (rc_supported(c->E) ? L * b.RCW + REGION_SLACK : 0);
    return b;
}
// one workspace serves a backward range or a forward that keeps nothing
static int64_t enc_ws_floats(const ganffn_enc_cfg* c) { return std::max(bwd_layout(c).total, unsaved_layout(c).total) + TAIL_SLACK; }

}  // namespace ganffn

using namespace ganffn;

extern "C" int ganffn_version(void) { return GANFFN_VERSION; }
extern "C" const char* ganffn_last_error(void) { return err_buf(); }

extern "C" int64_t ganffn_layer_param_count(int E, int F) { return layer_off(E, F).total; }
extern "C" int ganffn_layer_param_offsets(int E, int F, int64_t* o) {
    GF_CHECK_ARG(o, "null offsets");
    const LayerOff l = layer_off(E, F);
    const int64_t v[12] = {l.in_w, l.in_b, l.out_w, l.out_b, l.w1, l.b1, l.w2, l.b2, l.n1w, l.n1b, l.n2w, l.n2b};
    memcpy(o, v, sizeof(v));
    return 0;
}

extern "C" int64_t ganffn_encoder_saved_floats(const ganffn_enc_cfg* c) { return check_cfg(c) != 0 ? -1 : saved_off(c).total; }
extern "C" int64_t ganffn_encoder_saved_hidden_offset(const ganffn_enc_cfg* c, int layer) {
    if (check_cfg(c) != 0 || layer < 0 || layer >= c->L) return -1;
    const SavedOff so = saved_off(c);
    return so.layers + (int64_t)layer * so.per_layer + so.h;
}
extern "C" int64_t ganffn_encoder_workspace_floats(const ganffn_enc_cfg* c) { return check_cfg(c) != 0 ? -1 : enc_ws_floats(c); }

// ------------------------------------------------------------------------------------------
// encoder stack forward
// ------------------------------------------------------------------------------------------
// One row segment of a forward pass: T = S B rows that go through the stack with their own buffers and train flag.  A pass
// has one segment or two (the second over the same input, in the same launches: every forward kernel has a two-segment form).
struct FwdSeg {
    float* X;          // the running activation: X[0] = PE output, X[l + 1] = output of layer l (the last one goes to `out`)
    float* layers;     // layer l's saved set (SavedOff: qkv, attn_o, x1, xhat1, xhat2, h, rstd1, rstd2, lse, keep, hmask)
    float* tmp;        // [MAX_SPLITS][T x E] GEMM output (partial slabs) before residual + LayerNorm
    float* out;        // the stack's output
    int64_t TE, per_layer;
    int L, train;
    bool keeps;        // a backward will follow: every X[l] and layer set has its own place, keep words and hmask are written
    float* x(int l) const { return l == L ? out : X + (keeps ? l : (l & 1)) * TE; }
    float* layer(int l) const { return layers + (keeps ? l : 0) * per_layer; }
};
// nothing kept: the segment lives in the workspace (UnsavedLayout)
static FwdSeg unsaved_seg(const ganffn_enc_cfg* c, float* workspace, float* out, int train) {
    const UnsavedLayout u = unsaved_layout(c);
    return FwdSeg{workspace + u.X, workspace + u.layer, workspace + u.tmp, out, u.TE, saved_off(c).per_layer, c->L, train, false};
}
// everything kept in `saved` (SavedOff); the slabs are the caller's
static FwdSeg saved_seg(const ganffn_enc_cfg* c, float* saved, float* tmp, float* out, int train) {
    const SavedOff so = saved_off(c);
    return FwdSeg{saved + so.X, saved + so.layers, tmp, out, (int64_t)c->S * c->B * c->E, so.per_layer, c->L, train, true};
}

// One encoder pass.  Every encoder entry point fills one and runs encoder_fwd, encoder_fwd_pair or encoder_bwd on it (the
// streaming ones: encoder_fwd_walk); what an entry point does not take stays null / 0.
struct EncCall {
    const ganffn_enc_cfg* c; const uint64_t* rng; uint64_t add; hipStream_t st;
    const int32_t* key_len; uint32_t flags;            // the attention core's per-dialogue key lengths (or null), GANFFN_ATTN_* bits
    const float* x_in; const float* pe; const float* params; float* workspace;
    float* out; float* saved; float* out_train;        // forward; saved null: nothing kept.  Pair: out is the eval segment's, out_train
                                                       // and saved are the train segment's.  (The backward only reads saved.)
    int layer_lo, layer_hi, need_dx_in; float* dx; float* grads;       // backward over layers [layer_lo, layer_hi)
    TnSlabs* slabs;                                    // (or null) leave the weight gradients unreduced: ganffn_encoder_bwd_parts*
    EncCall& forward(const float* x, const float* pe_, const float* P, float* o, float* sv, float* ws) { x_in = x; pe = pe_; params = P; out = o; saved = sv; workspace = ws; return *this; }
    EncCall& pair(float* o_train) { out_train = o_train; return *this; }
    EncCall& backward(int lo, int hi, float* dx_, const float* P, float* G, const float* sv, float* ws, int need) {
        layer_lo = lo; layer_hi = hi; dx = dx_; params = P; grads = G; saved = const_cast<float*>(sv); workspace = ws; need_dx_in = need;
        return *this;
    }
};
static inline EncCall enc_call(const ganffn_enc_cfg* c, const int32_t* key_len, uint32_t flags, const uint64_t* rng, uint64_t add, void* stream) {
    EncCall k{};
    k.c = c; k.key_len = key_len; k.flags = flags; k.rng = rng; k.add = add; k.st = (hipStream_t)stream;
    return k;
}

// The launch sequence of the stack, once.  s1 (or null): the second segment; every launcher takes it as its optional trailing
// operand set, built here from s1 and null without one.  Every rule that picks a summation order (split-K factors, K chunks of
// gemm_n100) is evaluated for T = S B, one segment's rows, so a segment has the bits of a pass of its own.
// key_len (or null): per-dialogue key lengths of the attention core, the one place of a layer where rows of a dialogue meet;
// both segments are the same B dialogues, so one [B] array serves both
// flags: GANFFN_ATTN_* bits for the same place (0 = none), for both segments alike
// sa (or null): the pass is a streaming step (ganffn_encoder_stream_step) — c is S = 1, B = n, eval; the positional encoding is
// the gather by per-dialogue position followed by layer 0's in-proj GEMM, and the attention core is the single-query step over
// layer l's K/V cache (stream.hip).  Every other launch is the one a pass over T = n rows issues; null changes no call.
// With sa->count (ganffn_encoder_stream_extend) the T = m * n rows are n chunks of up to m rows, time-major, and the two launches
// are the chunk forms of the same file; without it they are the step's, as before.
static int encoder_fwd_walk(const EncCall& k, const Mode md, const FwdSeg& s0, const FwdSeg* s1, const StreamArgs* sa) {
    const ganffn_enc_cfg* c = k.c; const int32_t* key_len = k.key_len; const uint32_t flags = k.flags;
    const float* pe = k.pe; const float* x_in = k.x_in; const float* params = k.params;
    const uint64_t* rng = k.rng; const uint64_t add = k.add; hipStream_t st = k.st;
    GF_CHECK_ARG(!sa || (!s1 && !key_len && flags == 0 && !s0.train), "encoder_stream_step: one eval segment, no lengths, no flags");
    const int S = c->S, B = c->B, E = c->E, H = c->H, F = c->F, L = c->L, T = S * B;
    const int64_t TE = (int64_t)T * E;
    const LayerOff lo = layer_off(E, F);
    const SavedOff so = saved_off(c);
    // t1's addresses are only handed on where s1 is: without a second segment the adapters below (nt, run) leave it out of the call
    const FwdSeg& t1 = s1 ? *s1 : s0;
    const int train0 = s0.train, train1 = s1 ? s1->train : 0;
    auto keep_words = [&](const FwdSeg& s, float* sv) { return s.keeps ? reinterpret_cast<uint32_t*>(sv + so.keep) : nullptr; };
    // [T x K] x W[N x K]^T of both segments in one launch; slab_cap (or 0): at most so many K slabs TE apart, summed by the
    // LayerNorm kernel, *splits of them written (gemm_plan picks the kernel and the count)
    auto nt = [&](const float* A0, const float* A1, int K, const float* W, float* C0, float* C1, int N, int epi, const EpiArgs& ea,
                  uint16_t* mask1 = nullptr, int slab_cap = 0, int* splits = nullptr) {
        GemmCall g = gemm_nt(A0, W, C0, T, N, K).epilogue(epi, ea).on(st);
        if (slab_cap) g.slabs(slab_cap, TE, splits);
        if (s1) g.pair(GemmSeg1{A1, C1, mask1, train1});
        return gemm(g);
    };
    // A row stage (common.h RowCall) over both segments.  d_model 100: the stage with its GEMMs is one kernel (rowchain.hip) — out-proj
    // + residual + dropout + LN1, LN2 + the NEXT layer's in-proj, and the positional encoding + dropout at the head of the stack with
    // layer 0's; every other width, or the mode word: the same launches one by one.  row_plan says which, row_fwd does it.
    const RowPlan rp = row_plan(E, md, sa != nullptr);
    // (a RowCall is filled where it stands and each segment built once: some 600 stages a step are issued from one host thread)
    auto stage = [&](RowKind kind, float p, uint32_t site) {
        RowCall r = row_call(kind, T, B, E, c->ln_eps, p, site, rng, add, st);
        r.plan = rp;
        return r;
    };
    // seg(s, v): the stage's operands for segment s, whose saved set of the layer is v
    auto run = [&](RowCall& r, float* v0, float* v1, auto&& seg) {
        r.forward(seg(s0, v0));
        if (s1) r.pair(seg(*s1, v1));
        return row_fwd(r);
    };

    // X[0] = dropout(x_in + pe), then qkv of layer 0 = X[0] W_in^T + b_in
    if (sa) {
        if (sa->count)
            GF_TRY(launch_stream_pe_chunk(x_in, pe, sa->slot, sa->count, sa->pos, s0.x(0), T / sa->m, sa->m, sa->capacity, sa->max_len,
                                          E, st));
        else
            GF_TRY(launch_stream_pe(x_in, pe, sa->slot, sa->pos, s0.x(0), T, sa->capacity, sa->max_len, E, st));
        EpiArgs e0;
        e0.bias = params + lo.in_b;
        GF_TRY(nt(s0.x(0), t1.x(0), E, params + lo.in_w, s0.layer(0) + so.qkv, t1.layer(0) + so.qkv, 3 * E, EPI_NONE, e0));
    } else {
        RowCall r = stage(ROW_PE, c->p_pe, SITE_PE);
        r.inproj(params + lo.in_w, params + lo.in_b);
        GF_TRY(run(r, nullptr, nullptr, [&](const FwdSeg& s, float*) { return pe_seg(x_in, pe, s.x(0), s.layer(0) + so.qkv, s.train); }));
    }

    for (int l = 0; l < L; ++l) {
        const float* P = params + (int64_t)l * lo.total;
        const float* Pn = (l + 1 < L) ? P + lo.total : nullptr;      // the next layer's parameters
        float* const v0 = s0.layer(l);
        float* const v1 = t1.layer(l);
        const uint32_t site = SITE_LAYER0 + 4 * l;
        // attention core (keep words only when a backward will follow)
        if (sa && sa->count) {
            GF_TRY(launch_stream_attention_chunk(v0 + so.qkv, sa->cache + (int64_t)l * sa->layer_stride, sa->slot, sa->count, sa->pos,
                                                 v0 + so.attn_o, T / sa->m, sa->m, sa->capacity, sa->max_len, E, H, st));
        } else if (sa) {
            GF_TRY(launch_stream_attention(v0 + so.qkv, sa->cache + (int64_t)l * sa->layer_stride, sa->slot, sa->pos, v0 + so.attn_o, T,
                                           sa->capacity, sa->max_len, E, H, st));
        } else {
            AttnCall a = attn_call(S, B, E, H, c->p_enc, site + 0, rng, add, st).mask(key_len, flags);
            a.forward(AttnSeg{v0 + so.qkv, v0 + so.attn_o, v0 + so.lse, keep_words(s0, v0), train0});
            if (s1) a.pair(AttnSeg{v1 + so.qkv, v1 + so.attn_o, v1 + so.lse, keep_words(t1, v1), train1});
            GF_TRY(attention_fwd(a));
        }
        // stage A: out-proj, residual + dropout + LN1
        // (as separate launches the 512-wide out-proj is 376 output tiles on 256 CUs: K in two halves, summed by the LayerNorm kernel)
        {
            RowCall r = stage(ROW_LN, c->p_enc, site + 1);
            r.norm(P + lo.n1w, P + lo.n1b).front(P + lo.out_w, P + lo.out_b, md.outproj_nosplit() ? 1 : MAX_SPLITS, TE);
            GF_TRY(run(r, v0, v1, [&](const FwdSeg& s, float* v) {
                return ln_front_seg(v + so.attn_o, s.tmp, s.x(l), v + so.x1, v + so.xhat1, v + so.rstd1, s.train);
            }));
        }
        // FFN: h = drop(relu(x1 W1^T + b1)); y = h W2^T + b2
        int splits = 1;
        {
            EpiArgs e1, e2;
            e1.bias = P + lo.b1; e1.p = c->p_enc; e1.site = site + 2; e1.rng = rng; e1.rng_add = add; e1.train = train0;
            // hmask: the pattern the linear2 dgrad will ask for
            if (s0.keeps) e1.mask_out = reinterpret_cast<uint16_t*>(v0 + so.hmask);
            uint16_t* const mask1 = t1.keeps ? reinterpret_cast<uint16_t*>(v1 + so.hmask) : nullptr;
            GF_TRY(nt(v0 + so.x1, v1 + so.x1, E, P + lo.w1, v0 + so.h, v1 + so.h, F, EPI_RELU_DROP, e1, mask1));
            // few output tiles, K = 2048: K chunks = output slabs, summed by the LayerNorm kernel (gemm_n100.hip at d_model 100)
            e2.bias = P + lo.b2;
            GF_TRY(nt(v0 + so.h, v1 + so.h, F, P + lo.w2, s0.tmp, t1.tmp, E, EPI_NONE, e2, nullptr, MAX_SPLITS, &splits));
        }
        // stage B: the slabs, residual + dropout + LN2, then (all but the last layer) qkv of layer l + 1 from the fresh rows
        {
            RowCall r = stage(ROW_LN, c->p_enc, site + 3);
            r.norm(P + lo.n2w, P + lo.n2b).slabs(splits, TE);
            if (Pn) r.inproj(Pn + lo.in_w, Pn + lo.in_b);
            GF_TRY(run(r, v0, v1, [&](const FwdSeg& s, float* v) {
                return ln_slab_seg(s.tmp, v + so.x1, s.x(l + 1), v + so.xhat2, v + so.rstd2, Pn ? s.layer(l + 1) + so.qkv : nullptr, s.train);
            }));
        }
    }
    return 0;
}

// what every pass refuses before its first launch, in this order; pass = "fwd" | "fwd_pair" | "bwd" (the one with a dx)
static int check_pass(const EncCall& k, const char* pass, bool pointers_given, bool all_aligned) {
    GF_TRY(check_cfg(k.c));
    GF_CHECK_ARG((k.flags & ~GANFFN_ATTN_CAUSAL) == 0, "encoder_%s: unknown flag bits 0x%x", pass, k.flags & ~GANFFN_ATTN_CAUSAL);
    GF_CHECK_ARG(pointers_given, "encoder_%s: null pointer", pass);
    GF_CHECK_ARG(!k.dx || (0 <= k.layer_lo && k.layer_lo < k.layer_hi && k.layer_hi <= k.c->L), "encoder_bwd: bad layer range [%d,%d)",
                 k.layer_lo, k.layer_hi);
    GF_CHECK_ARG(all_aligned, "encoder_%s: buffers must be 16-byte aligned", pass);
    GF_CHECK_ARG(!(k.c->train && (k.c->p_pe > 0.f || k.c->p_enc > 0.f)) || k.rng, "encoder_%s: rng required in train mode", pass);
    return 0;
}
static int encoder_fwd(const EncCall& k) {
    const Mode md = mode();
    GF_TRY(check_pass(k, "fwd", k.x_in && k.pe && k.params && k.out && k.workspace,
                      aligned16(k.x_in) && aligned16(k.params) && aligned16(k.out) && aligned16(k.workspace) && aligned16(k.saved)));
    const FwdSeg s0 = k.saved ? saved_seg(k.c, k.saved, k.workspace, k.out, k.c->train) : unsaved_seg(k.c, k.workspace, k.out, k.c->train);
    return encoder_fwd_walk(k, md, s0, nullptr, nullptr);
}
extern "C" int ganffn_encoder_fwd(const ganffn_enc_cfg* c, const float* x_in, const float* pe, const float* params,
                                  float* out, float* saved, float* workspace, const uint64_t* rng, uint64_t add,
                                  void* stream) {
    return encoder_fwd(enc_call(c, nullptr, 0, rng, add, stream).forward(x_in, pe, params, out, saved, workspace));
}
extern "C" int ganffn_encoder_fwd_len(const ganffn_enc_cfg* c, const int32_t* key_len, const float* x_in, const float* pe,
                                      const float* params, float* out, float* saved, float* workspace, const uint64_t* rng,
                                      uint64_t add, void* stream) {
    return encoder_fwd(enc_call(c, key_len, 0, rng, add, stream).forward(x_in, pe, params, out, saved, workspace));
}
extern "C" int ganffn_encoder_fwd_mask(const ganffn_enc_cfg* c, const int32_t* key_len, uint32_t flags, const float* x_in,
                                       const float* pe, const float* params, float* out, float* saved, float* workspace,
                                       const uint64_t* rng, uint64_t add, void* stream) {
    return encoder_fwd(enc_call(c, key_len, flags, rng, add, stream).forward(x_in, pe, params, out, saved, workspace));
}

// ------------------------------------------------------------------------------------------
// streaming step: n new rows, one per active dialogue, through the whole stack against per-layer K/V caches
//   cache: L layers, stream_layer_floats apart, each [capacity][2 (K, V)][H][max_len][E / H]   (c->B = capacity, c->S = max_len)
//   workspace: the unsaved segment of a forward over T = n_max rows
// ------------------------------------------------------------------------------------------
static int check_stream_cfg(const ganffn_enc_cfg* c) {
    GF_TRY(check_cfg(c));
    GF_CHECK_ARG(c->B <= GANFFN_MAX_DIALOGUES, "stream: capacity B=%d out of range [1,%d]", c->B, GANFFN_MAX_DIALOGUES);
    GF_CHECK_ARG(c->train == 0, "stream: train=%d (streaming is inference: train must be 0)", c->train);
    GF_CHECK_ARG(((c->E / c->H) & 1) == 0 && c->E / c->H <= 64, "stream: head_dim %d must be even and <= 64", c->E / c->H);
    return 0;
}
static int64_t stream_layer_floats(const ganffn_enc_cfg* c) { return a4((int64_t)c->B * 2 * c->S * c->E); }
static ganffn_enc_cfg stream_rows_cfg(const ganffn_enc_cfg* c, int n) {
    ganffn_enc_cfg r = *c;
    r.S = 1; r.B = n; r.train = 0;
    return r;
}
extern "C" int64_t ganffn_stream_cache_floats(const ganffn_enc_cfg* c) { return check_stream_cfg(c) != 0 ? -1 : c->L * stream_layer_floats(c); }
extern "C" int64_t ganffn_stream_workspace_floats(const ganffn_enc_cfg* c, int n_max) {
    if (check_stream_cfg(c) != 0) return -1;
    if (n_max < 1 || n_max > c->B) return fail(-1, "stream_workspace_floats: n_max=%d out of range [1,%d]", n_max, c->B);
    const ganffn_enc_cfg r = stream_rows_cfg(c, n_max);
    return enc_ws_floats(&r);
}
extern "C" int ganffn_encoder_stream_step(const ganffn_enc_cfg* c, int n, const int32_t* slot, const int32_t* pos, const float* x,
                                          const float* pe, const float* params, float* cache, float* out, float* workspace,
                                          void* stream) {
    const Mode md = mode();
    GF_TRY(check_stream_cfg(c));
    GF_CHECK_ARG(n >= 1 && n <= c->B, "encoder_stream_step: n=%d out of range [1,%d]", n, c->B);
    GF_CHECK_ARG(slot && pos && x && pe && params && cache && out && workspace, "encoder_stream_step: null pointer");
    GF_CHECK_ARG(aligned16(x) && aligned16(pe) && aligned16(params) && aligned16(cache) && aligned16(out) && aligned16(workspace),
                 "encoder_stream_step: buffers must be 16-byte aligned");
    const ganffn_enc_cfg r = stream_rows_cfg(c, n);
    const FwdSeg s0 = unsaved_seg(&r, workspace, out, 0);
    const StreamArgs sa{slot, pos, cache, stream_layer_floats(c), c->B, c->S};
    return encoder_fwd_walk(enc_call(&r, nullptr, 0, nullptr, 0, stream).forward(x, pe, params, out, nullptr, workspace), md, s0, nullptr, &sa);
}

// ------------------------------------------------------------------------------------------
// stream prefill: n chunks of up to m new rows each (time-major [m][n][E]) through the whole stack against the same caches
//   workspace: the unsaved segment of a forward over T = rows_max rows (nothing of a backward: streaming is inference)
// ------------------------------------------------------------------------------------------
static int64_t stream_extend_ws(const ganffn_enc_cfg* c, int rows) {
    const ganffn_enc_cfg r = stream_rows_cfg(c, rows);
    return unsaved_layout(&r).total + TAIL_SLACK;
}
extern "C" int64_t ganffn_stream_extend_workspace_floats(const ganffn_enc_cfg* c, int rows_max) {
    if (check_stream_cfg(c) != 0) return -1;
    if (rows_max < 1 || rows_max > c->S * c->B)
        return fail(-1, "stream_extend_workspace_floats: rows_max=%d out of range [1,%d] (max_len * capacity)", rows_max, c->S * c->B);
    return stream_extend_ws(c, rows_max);
}
extern "C" int ganffn_encoder_stream_extend(const ganffn_enc_cfg* c, int n, int m, const int32_t* slot, const int32_t* count,
                                            const int32_t* pos, const float* x, const float* pe, const float* params, float* cache,
                                            float* out, float* workspace, int64_t workspace_floats, void* stream) {
    const Mode md = mode();
    GF_TRY(check_stream_cfg(c));
    GF_CHECK_ARG(n >= 1 && n <= c->B, "encoder_stream_extend: n=%d out of range [1,%d]", n, c->B);
    GF_CHECK_ARG(m >= 1 && m <= c->S, "encoder_stream_extend: m=%d out of range [1,%d]", m, c->S);
    GF_CHECK_ARG(slot && count && pos && x && pe && params && cache && out && workspace, "encoder_stream_extend: null pointer");
    GF_CHECK_ARG(aligned16(x) && aligned16(pe) && aligned16(params) && aligned16(cache) && aligned16(out) && aligned16(workspace),
                 "encoder_stream_extend: buffers must be 16-byte aligned");
    const int rows = m * n;
    GF_CHECK_ARG(workspace_floats >= stream_extend_ws(c, rows),
                 "encoder_stream_extend: m*n=%d rows need a workspace of %lld floats (rows_max >= %d), got %lld", rows,
                 (long long)stream_extend_ws(c, rows), rows, (long long)workspace_floats);
    const ganffn_enc_cfg r = stream_rows_cfg(c, rows);
    const FwdSeg s0 = unsaved_seg(&r, workspace, out, 0);
    StreamArgs sa{slot, pos, cache, stream_layer_floats(c), c->B, c->S};
    sa.count = count;
    sa.m = m;
    return encoder_fwd_walk(enc_call(&r, nullptr, 0, nullptr, 0, stream).forward(x, pe, params, out, nullptr, workspace), md, s0, nullptr, &sa);
}
extern "C" int ganffn_stream_attention_chunk(const float* qkv, float* cache_layer, const int32_t* slot, const int32_t* count,
                                             const int32_t* pos, float* o, int n, int m, int capacity, int max_len, int E, int H,
                                             void* stream) {
    return launch_stream_attention_chunk(qkv, cache_layer, slot, count, pos, o, n, m, capacity, max_len, E, H, (hipStream_t)stream);
}
extern "C" int ganffn_stream_attention(const float* qkv, float* cache_layer, const int32_t* slot, const int32_t* pos, float* o, int n,
                                       int capacity, int max_len, int E, int H, void* stream) {
    return launch_stream_attention(qkv, cache_layer, slot, pos, o, n, capacity, max_len, E, H, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// encoder stack forward over two row segments: the eval-mode pass (nothing kept) and the train-mode pass (saved for the
// backward) of ONE stack over the SAME input.  In the GAN schedule every discriminator sub-step runs its partner generator
// in eval mode and the next sub-step runs that generator in train mode on the same batch with the same parameters; here the
// two passes are the two segments of one encoder_fwd_walk.  Segment 0 is the unsaved segment of ganffn_encoder_fwd at the
// head of the workspace with train = 0, segment 1 the saved segment over saved_train with its slabs behind segment 0's
// workspace.  In a two-segment kernel a workgroup picks its segment from its index and then does what a workgroup of the
// single-segment launch does, so each output has the bits ganffn_encoder_fwd gives it.
// ------------------------------------------------------------------------------------------
static bool pair_supported(const ganffn_enc_cfg* c, const Mode md) {
    // every width has its segment forms; of gemm_n100's variants only the product one (eight waves, 4x4x1 tail), not the lab ones
    return !(n100_supported(c->E, c->F) && !md.n100_off() && (md.n100_pad7() || md.n100_force_kw() == 1));
}
extern "C" int ganffn_encoder_fwd_pair_supported(const ganffn_enc_cfg* c) {
    if (check_cfg(c) != 0) return 0;
    return pair_supported(c, mode()) ? 1 : 0;
}
extern "C" int64_t ganffn_encoder_fwd_pair_workspace_floats(const ganffn_enc_cfg* c) {
    if (check_cfg(c) != 0) return -1;
    const UnsavedLayout u = unsaved_layout(c);      // segment 0's part of the workspace; then segment 1's slabs
    return u.total + u.slabs + TAIL_SLACK;
}
static int encoder_fwd_pair(const EncCall& k) {
    const Mode md = mode();
    const ganffn_enc_cfg* c = k.c;
    GF_TRY(check_cfg(c));
    GF_CHECK_ARG(pair_supported(c, md), "encoder_fwd_pair: no two-segment form for E=%d H=%d F=%d S=%d (ganffn_encoder_fwd_pair_supported)",
                 c->E, c->H, c->F, c->S);
    GF_TRY(check_pass(k, "fwd_pair", k.x_in && k.pe && k.params && k.out && k.out_train && k.saved && k.workspace,
                      aligned16(k.x_in) && aligned16(k.params) && aligned16(k.out) && aligned16(k.out_train) && aligned16(k.saved) &&
                          aligned16(k.workspace)));
    const FwdSeg s0 = unsaved_seg(c, k.workspace, k.out, 0);
    const FwdSeg s1 = saved_seg(c, k.saved, k.workspace + unsaved_layout(c).total, k.out_train, c->train);
    return encoder_fwd_walk(k, md, s0, &s1, nullptr);
}
extern "C" int ganffn_encoder_fwd_pair(const ganffn_enc_cfg* c, const float* x_in, const float* pe, const float* params,
                                       float* out_eval, float* out_train, float* saved_train, float* workspace,
                                       const uint64_t* rng, uint64_t add_train, void* stream) {
    return encoder_fwd_pair(enc_call(c, nullptr, 0, rng, add_train, stream).forward(x_in, pe, params, out_eval, saved_train, workspace).pair(out_train));
}
extern "C" int ganffn_encoder_fwd_pair_len(const ganffn_enc_cfg* c, const int32_t* key_len, const float* x_in, const float* pe,
                                           const float* params, float* out_eval, float* out_train, float* saved_train,
                                           float* workspace, const uint64_t* rng, uint64_t add_train, void* stream) {
    return encoder_fwd_pair(enc_call(c, key_len, 0, rng, add_train, stream).forward(x_in, pe, params, out_eval, saved_train, workspace).pair(out_train));
}
// the same with a flags word: GANFFN_ATTN_CAUSAL puts BOTH segments under the causal mask (0 = the call above; an unknown bit is
// refused by check_pass before any launch)
extern "C" int ganffn_encoder_fwd_pair_mask(const ganffn_enc_cfg* c, const int32_t* key_len, uint32_t flags, const float* x_in,
                                            const float* pe, const float* params, float* out_eval, float* out_train,
                                            float* saved_train, float* workspace, const uint64_t* rng, uint64_t add_train,
                                            void* stream) {
    return encoder_fwd_pair(enc_call(c, key_len, flags, rng, add_train, stream).forward(x_in, pe, params, out_eval, saved_train, workspace).pair(out_train));
}

// ------------------------------------------------------------------------------------------
// encoder stack backward over layers [lo_l, hi_l)
// ------------------------------------------------------------------------------------------
static int encoder_bwd(const EncCall& k) {
    const Mode md = mode();
    const ganffn_enc_cfg* c = k.c;
    const int layer_lo = k.layer_lo, layer_hi = k.layer_hi, need_dx_in = k.need_dx_in;
    TnSlabs* const slabs = k.slabs;
    float* const dx = k.dx; float* const grads = k.grads; float* const workspace = k.workspace;
    const float* params = k.params; const float* saved = k.saved;
    const uint64_t* rng = k.rng; const uint64_t add = k.add; hipStream_t st = k.st;
    GF_TRY(check_pass(k, "bwd", dx && params && saved && workspace,
                      aligned16(dx) && aligned16(params) && aligned16(saved) && aligned16(workspace) && aligned16(grads)));
    const int S = c->S, B = c->B, E = c->E, H = c->H, F = c->F, T = S * B;
    const int64_t TE = (int64_t)T * E;
    const LayerOff lo = layer_off(E, F);
    const SavedOff so = saved_off(c);
    const BwdLayout w = bwd_layout(c);
    const int train = c->train;

    // Weight gradients are DEFERRED: every layer keeps what its 4 wgrad GEMMs read (dh, dyA, dyB, d_qkv) in its own
    // buffer set, and one grouped launch at the end of the range computes all of them (4 x layers problems).  The
    // LayerNorm weight / bias gradients are reduced the same way: per-block partial sums now, one ordered reduce
    // launch for the whole range at the end.  Nothing in here uses atomics: gradients are bit-reproducible.
    float* dz2 = workspace + w.dz2;        // [T x E] LN2 input gradient (residual branch into x1)
    float* dz1 = workspace + w.dz1;        // [T x E] LN1 input gradient (residual branch into X[l])
    float* d_attn = workspace + w.d_attn;  // [T x E]
    float* tmp = workspace + w.tmp;        // [MAX_SPLITS][T x E] partial slabs of dh W1
    // The two LayerNorm backward stages are row stages (common.h RowCall).  Under the rowchain plan (d_model 100) the in-proj dgrad of
    // the layer above runs inside the LN2 stage and the out-proj dgrad inside the LN1 stage, on transposed weights packed here;
    // otherwise both are GEMMs of this walk.  rcw, per layer: in_w^T [E x 3E] | out_w^T [E x E]
    const RowPlan rp = row_plan(E, md);
    if (rp.rowchain) GF_TRY(launch_rc_pack(params + (int64_t)layer_lo * lo.total, lo.total, lo.in_w, lo.out_w, workspace + w.rcw, layer_hi - layer_lo, st));
    auto stage = [&](uint32_t site) {
        RowCall r = row_call(ROW_LN, T, B, E, c->ln_eps, c->p_enc, site, rng, add, st);
        r.plan = rp;
        return r;
    };
    TnDesc tn[40]; int ntn = 0;
    LnRedList red;

    const float* dxin = dx;       // gradient wrt the current layer's output: the caller's dx, then in-proj dgrad slabs
    int dxin_slabs = 1;
    int64_t dxin_stride = rp.rowchain ? 0 : TE;   // of one tensor no kernel reads it; each plan keeps the value its launches always got
    for (int l = layer_hi - 1; l >= layer_lo; --l) {
        const float* P = params + (int64_t)l * lo.total;
        float* G = grads ? grads + (int64_t)l * lo.total : nullptr;
        const float* sv = saved + so.layers + (int64_t)l * so.per_layer;
        const float* Xl = saved + so.X + (int64_t)l * TE;
        const uint32_t site = SITE_LAYER0 + 4 * l;
        const int i = l - layer_lo;
        float* dh = workspace + w.dh(i);         // [T x F]
        float* dyA = workspace + w.dyA(i);       // [T x E] d(FFN output)
        float* dyB = workspace + w.dyB(i);       // [T x E] d(attention block output)
        float* d_qkv = workspace + w.d_qkv(i);   // [T x 3E]
        float* lnp2 = workspace + w.lnp2(i);
        float* lnp1 = workspace + w.lnp1(i);
        // LN2 backward: dL/dX[l+1] -> dz2 (to x1), dyA (to FFN output).  dL/dX[l+1] is the caller's dx for the top layer
        // of the range and otherwise the in-proj dgrad of the layer above: split-K partial slabs in `tmp`, summed here
        {
            RowCall r = stage(site + 3);
            r.backward(sv + so.xhat2, sv + so.rstd2, P + lo.n2w, dz2, dyA, train);
            // rowchain, below the top layer of the range: the in-proj dgrad of the layer above (its d_qkv is still in that layer's
            // buffer set, its residual-branch gradient in dz1) runs inside this kernel
            if (rp.rowchain && l < layer_hi - 1) r.from_inproj(workspace + w.d_qkv_above(i), workspace + w.rcw_layer(i + 1), dz1);
            else r.from(dxin, dxin_slabs, dxin_stride, nullptr);
            if (G) r.param_grads(G + lo.n2w, G + lo.n2b, lnp2, &red);
            GF_TRY(row_bwd(r));
        }
        // linear2 wgrad: gW2[E,F] += dyA^T h ; gb2 += colsum(dyA)
        if (G) tn[ntn++] = TnDesc{dyA, E, sv + so.h, F, G + lo.w2, F, G + lo.b2, E, F, T};
        const float pdrop = train ? c->p_enc : 0.f, mscale = (pdrop > 0.f) ? 1.0f / (1.0f - pdrop) : 1.0f;
        int splits = 1;
        {
            EpiArgs em;
            em.aux_in = sv + so.h;
            em.mscale = mscale;
            if (!md.mask_float()) em.mask_in = reinterpret_cast<const uint16_t*>(sv + so.hmask);     // linear1's epilogue left the pattern as bits
            GF_TRY(gemm(gemm_nn(dyA, P + lo.w2, dh, T, F, E).epilogue(EPI_MASK_POS, em).on(st)));
        }
        // linear1 wgrad: gW1[F,E] += dh^T x1 ; gb1 += colsum(dh)
        if (G) tn[ntn++] = TnDesc{dh, F, sv + so.x1, E, G + lo.w1, E, G + lo.b1, F, E, T};
        {
            // d x1 = dh W1 (split-K slabs) + dz2, consumed directly by the LN1 backward
            GF_TRY(gemm(gemm_nn(dh, P + lo.w1, tmp, T, E, F).slabs(MAX_SPLITS, TE, &splits).on(st)));
        }
        {
            // LN1 backward; rowchain: + the out-proj dgrad (d_attn = dyB W_o) on the rows while they are in the workgroup
            RowCall r = stage(site + 1);
            r.backward(sv + so.xhat1, sv + so.rstd1, P + lo.n1w, dz1, dyB, train).from(tmp, splits, TE, dz2);
            if (rp.rowchain) r.outproj_dgrad(workspace + w.rcw_layer(i) + 3 * (int64_t)E * E, d_attn);
            if (G) r.param_grads(G + lo.n1w, G + lo.n1b, lnp1, &red);
            GF_TRY(row_bwd(r));
        }
        // out-proj wgrad + dgrad
        if (G) tn[ntn++] = TnDesc{dyB, E, sv + so.attn_o, E, G + lo.out_w, E, G + lo.out_b, E, E, T};
        if (!rp.rowchain) GF_TRY(gemm(gemm_nn(dyB, P + lo.out_w, d_attn, T, E, E).on(st)));
        // attention core backward
        GF_TRY(attention_bwd(attn_call(S, B, E, H, c->p_enc, site + 0, rng, add, st).mask(k.key_len, k.flags)
                                 .backward(sv + so.qkv, sv + so.attn_o, sv + so.lse, reinterpret_cast<const uint32_t*>(sv + so.keep), d_attn, d_qkv, train)));
        // in-proj wgrad + dgrad; dX[l] = d_qkv W_in + dz1
        if (G) tn[ntn++] = TnDesc{d_qkv, 3 * E, Xl, E, G + lo.in_w, E, G + lo.in_b, 3 * E, E, T};
        if (ntn == 40 || (l == layer_lo && ntn > 0)) {
            GF_TRY(launch_gemm_tn_grouped(tn, ntn, st, workspace + w.tnp, gemm_tn_grouped_part_floats(), slabs));
            ntn = 0;
        }
        // dX[l] = d_qkv W_in + dz1 (.residual: added by split 0 in the GEMM epilogue)
        if (l > layer_lo && rp.rowchain) {
            // (the in-proj dgrad of this layer runs inside the LN2 backward kernel of layer l - 1)
        } else if (l > layer_lo) {
            // few output tiles (T/64 x E/64): split K into slabs that the next layer's LN2 backward sums on the fly
            // (`tmp` is free here: its previous content, this layer's dh W1 slabs, went into the LN1 backward above)
            int sp = 1;
            GF_TRY(gemm(gemm_nn(d_qkv, P + lo.in_w, tmp, T, E, 3 * E).residual(dz1).slabs(MAX_SPLITS, TE, &sp, SLABS_INPROJ_DGRAD).on(st)));
            dxin = tmp;
            dxin_slabs = sp;
            dxin_stride = TE;
        } else if (layer_lo > 0 || need_dx_in) {
            GF_TRY(gemm(gemm_nn(d_qkv, P + lo.in_w, dx, T, E, 3 * E).residual(dz1).on(st)));
        }   // (else: the stack's input needs no gradient — autograd would not compute this product either)
    }
    // (unreduced mode: nobody zeroed the gradient slab's encoder region — the LayerNorm parameter gradients are WRITTEN too)
    if (red.n > 0) GF_TRY(launch_ln_param_reduce(red, E, st, slabs != nullptr));
    if (layer_lo == 0 && need_dx_in) GF_TRY(launch_dropout_bwd_inplace(dx, T, E, c->p_pe, SITE_PE, rng, add, train, st));
    return 0;
}
extern "C" int ganffn_encoder_bwd2(const ganffn_enc_cfg* c, int layer_lo, int layer_hi, float* dx, const float* params,
                                   float* grads, const float* saved, float* workspace, const uint64_t* rng, uint64_t add,
                                   int need_dx_in, void* stream) {
    return encoder_bwd(enc_call(c, nullptr, 0, rng, add, stream).backward(layer_lo, layer_hi, dx, params, grads, saved, workspace, need_dx_in));
}
extern "C" int ganffn_encoder_bwd(const ganffn_enc_cfg* c, int layer_lo, int layer_hi, float* dx, const float* params,
                                  float* grads, const float* saved, float* workspace, const uint64_t* rng, uint64_t add,
                                  void* stream) {
    return ganffn_encoder_bwd2(c, layer_lo, layer_hi, dx, params, grads, saved, workspace, rng, add, 1, stream);
}
extern "C" int ganffn_encoder_bwd_len(const ganffn_enc_cfg* c, const int32_t* key_len, int layer_lo, int layer_hi, float* dx,
                                      const float* params, float* grads, const float* saved, float* workspace, const uint64_t* rng,
                                      uint64_t add, int need_dx_in, void* stream) {
    return encoder_bwd(enc_call(c, key_len, 0, rng, add, stream).backward(layer_lo, layer_hi, dx, params, grads, saved, workspace, need_dx_in));
}
extern "C" int ganffn_encoder_bwd_mask(const ganffn_enc_cfg* c, const int32_t* key_len, uint32_t flags, int layer_lo, int layer_hi,
                                       float* dx, const float* params, float* grads, const float* saved, float* workspace,
                                       const uint64_t* rng, uint64_t add, int need_dx_in, void* stream) {
    return encoder_bwd(enc_call(c, key_len, flags, rng, add, stream).backward(layer_lo, layer_hi, dx, params, grads, saved, workspace, need_dx_in));
}
// does ganffn_encoder_bwd_parts leave the weight gradients of this stack unreduced?  (d_model 100 on the rowchain / tn100 kernels,
// at most 10 layers: one grouped weight-gradient launch for the whole pass)
static bool bwd_parts_supported(const ganffn_enc_cfg* c, const Mode md) {
    return row_plan(c->E, md).rowchain && !md.tn100_off() && !md.tn100_in_kernel_sum() && !md.adam_slabs_off() && c->F == 2048 &&
           4 * c->L <= 40;
}
extern "C" int ganffn_encoder_bwd_parts_supported(const ganffn_enc_cfg* c) {
    if (check_cfg(c) != 0) return -1;
    return bwd_parts_supported(c, mode()) ? 1 : 0;
}
extern "C" int64_t ganffn_encoder_bwd_parts_covered(int E, int F) { return layer_off(E, F).n1w; }
extern "C" int ganffn_encoder_bwd_parts_mask(const ganffn_enc_cfg* c, const int32_t* key_len, uint32_t flags, float* dx,
                                             const float* params, float* grads, const float* saved, float* workspace,
                                             const uint64_t* rng, uint64_t add, int need_dx_in, int64_t* part_offset,
                                             int64_t* part_stride, int* n_parts, void* stream) {
    GF_TRY(check_cfg(c));
    GF_CHECK_ARG(grads && part_offset && part_stride && n_parts, "encoder_bwd_parts: null pointer");
    GF_CHECK_ARG(bwd_parts_supported(c, mode()), "encoder_bwd_parts: this stack's weight gradients are reduced in the launch (ask ganffn_encoder_bwd_parts_supported)");
    TnSlabs sl{grads, (long)c->L * layer_off(c->E, c->F).total, 1, nullptr, 0};
    EncCall k = enc_call(c, key_len, flags, rng, add, stream).backward(0, c->L, dx, params, grads, saved, workspace, need_dx_in);
    k.slabs = &sl;
    GF_TRY(encoder_bwd(k));
    *n_parts = sl.n_parts;
    *part_offset = sl.part ? sl.part - workspace : 0;
    *part_stride = sl.part_stride;
    return 0;
}
extern "C" int ganffn_encoder_bwd_parts_len(const ganffn_enc_cfg* c, const int32_t* key_len, float* dx, const float* params,
                                            float* grads, const float* saved, float* workspace, const uint64_t* rng, uint64_t add,
                                            int need_dx_in, int64_t* part_offset, int64_t* part_stride, int* n_parts, void* stream) {
    return ganffn_encoder_bwd_parts_mask(c, key_len, 0, dx, params, grads, saved, workspace, rng, add, need_dx_in, part_offset,
                                         part_stride, n_parts, stream);
}
extern "C" int ganffn_encoder_bwd_parts(const ganffn_enc_cfg* c, float* dx, const float* params, float* grads, const float* saved,
                                        float* workspace, const uint64_t* rng, uint64_t add, int need_dx_in, int64_t* part_offset,
                                        int64_t* part_stride, int* n_parts, void* stream) {
    return ganffn_encoder_bwd_parts_len(c, nullptr, dx, params, grads, saved, workspace, rng, add, need_dx_in, part_offset, part_stride,
                                        n_parts, stream);
}

// ------------------------------------------------------------------------------------------
// heads
// saved layout: gen : t0 [T,E] | u1 [T,D1] | a1 [T,D1] | u2 [T,D2]
//               disc: g0 [T,E] | u1 [T,D1] | a1 [T,D1] | u2 [T,D2] | a2 [T,D2] | prob [T4]
// ------------------------------------------------------------------------------------------
static int check_head(const ganffn_head_cfg* c) {
    GF_CHECK_ARG(c, "null head cfg");
    GF_CHECK_ARG(c->T >= 1 && c->E >= 4 && (c->E & 3) == 0, "head: bad T=%d E=%d", c->T, c->E);
    GF_CHECK_ARG(c->D1 >= 4 && (c->D1 & 3) == 0 && c->D2 >= 4 && (c->D2 & 3) == 0, "head: D1=%d D2=%d must be multiples of 4", c->D1, c->D2);
    GF_CHECK_ARG(c->kind == 0 || c->kind == 1, "head: kind=%d", c->kind);
    GF_CHECK_ARG(c->kind == 0 || c->D2 <= 32, "disc head: D2=%d > 32", c->D2);
    GF_CHECK_ARG(c->p >= 0.f && c->p < 1.f, "head: p=%g out of [0,1)", (double)c->p);
    return 0;
}
// the saved layout above (a2 and prob: kind 1 only) and the workspace of the head backward: d_pre1 [T x D1] | d_pre2 [T x D2] |
// part2, part1: split-K partial slabs of the gw2 / gw1 weight-gradient GEMMs (part2_floats, part1_floats) | tailp: per-block
// partial sums of the discriminator tail (36 floats a block, of the fused kernel's blocks or the tail kernel's)
struct HeadLayout {
    int64_t s0, u1, a1, u2, a2, prob, saved_total;
    int64_t d_pre1, d_pre2, part2, part1, tailp, ws_total, part2_floats, part1_floats;
};
static HeadLayout head_layout(const ganffn_head_cfg* c) {
    const int64_t T = c->T, TD1 = T * c->D1, TD2 = T * c->D2;
    HeadLayout h;
    h.s0 = 0; h.u1 = T * c->E; h.a1 = h.u1 + TD1; h.u2 = h.a1 + TD1; h.a2 = h.u2 + TD2; h.prob = h.a2 + TD2;
    h.saved_total = c->kind == 1 ? h.prob + a4(T) : h.a2;
    h.part2_floats = a4(gemm_tn_part_floats(c->D2, c->D1, c->T)); h.part1_floats = a4(gemm_tn_part_floats(c->D1, c->E, c->T));
    h.d_pre1 = 0; h.d_pre2 = a4(TD1); h.part2 = h.d_pre2 + a4(TD2); h.part1 = h.part2 + h.part2_floats; h.tailp = h.part1 + h.part1_floats;
    const int64_t tail_blocks = disc_head_blocks((int)T) > (T + 255) / 256 ? disc_head_blocks((int)T) : (T + 255) / 256;
    h.ws_total = h.tailp + tail_blocks * 36 + TAIL_SLACK;
    return h;
}
extern "C" int64_t ganffn_head_saved_floats(const ganffn_head_cfg* c) { return check_head(c) != 0 ? -1 : head_layout(c).saved_total; }
extern "C" int64_t ganffn_head_workspace_floats(const ganffn_head_cfg* c) { return check_head(c) != 0 ? -1 : head_layout(c).ws_total; }

extern "C" int ganffn_head_fwd(const ganffn_head_cfg* c, const float* x, const float* w1, const float* b1, const float* w2,
                               const float* b2, const float* w3, const float* b3, float* out, float* saved, float* workspace,
                               const uint64_t* rng, uint64_t add, void* stream) {
    GF_TRY(check_head(c));
    const Mode md = mode();
    GF_CHECK_ARG(x && w1 && b1 && w2 && b2 && out && saved, "head_fwd: null pointer");
    GF_CHECK_ARG(c->kind == 0 || (w3 && b3), "head_fwd: disc needs fc3");
    GF_CHECK_ARG(!(c->train && c->p > 0.f) || rng, "head_fwd: rng required in train mode");
    hipStream_t st = (hipStream_t)stream;
    const int T = c->T, E = c->E, D1 = c->D1, D2 = c->D2, train = c->train;
    const HeadLayout h = head_layout(c);
    float *s0 = saved + h.s0, *u1 = saved + h.u1, *a1 = saved + h.a1, *u2 = saved + h.u2;     // s0: t0 / g0
    float *a2 = saved + h.a2, *prob = saved + h.prob;                                         // (kind 1)
    if (c->kind == 1 && disc_head_fused_supported(E, D1, D2) && !md.dhead_off())
        return launch_disc_head_fwd(x, w1, b1, w2, b2, w3, b3, s0, u1, a1, u2, a2, prob, out, T, c->p, rng, add, train, st);
    // the generator head drops its input and ends after fc2; the discriminator's gets gelu only (model.py:1322) and fc2 goes on to the tail
    const bool gen = c->kind == 0;
    GF_TRY(launch_gelu_drop_fwd(x, s0, T, E, gen ? c->p : 0.f, SITE_HEAD0, rng, add, gen ? train : 0, st));
    EpiArgs e;
    e.p = c->p; e.rng = rng; e.rng_add = add; e.train = train;
    e.bias = b1; e.site = SITE_HEAD1; e.aux_out = u1;
    GF_TRY(gemm(gemm_nt(s0, w1, a1, T, D1, E).epilogue(EPI_DROP_GELU, e).on(st)));
    e.bias = b2; e.site = SITE_HEAD2; e.aux_out = u2;
    GF_TRY(gemm(gemm_nt(a1, w2, gen ? out : a2, T, D2, D1).epilogue(EPI_DROP_GELU, e).on(st)));
    if (gen) return 0;
    GF_TRY(launch_disc_tail_fwd(a2, w3, b3, prob, T, D2, c->p, rng, add, train, st));
    hipError_t er = hipMemcpyAsync(out, prob, (size_t)T * sizeof(float), hipMemcpyDeviceToDevice, st);
    return er == hipSuccess ? 0 : fail((int)er, "head_fwd: memcpy failed");
}

extern "C" int ganffn_head_bwd(const ganffn_head_cfg* c, const float* d_out, const float* x, const float* w1, const float* w2,
                               const float* w3, float* gw1, float* gb1, float* gw2, float* gb2, float* gw3, float* gb3,
                               float* dx, const float* saved, float* workspace, const uint64_t* rng, uint64_t add,
                               void* stream) {
    GF_TRY(check_head(c));
    const Mode md = mode();
    GF_CHECK_ARG(d_out && x && w1 && w2 && dx && saved && workspace, "head_bwd: null pointer");
    GF_CHECK_ARG(aligned16(workspace), "head_bwd: workspace must be 16-byte aligned");
    GF_CHECK_ARG(c->kind == 0 || w3, "head_bwd: disc needs fc3");
    GF_CHECK_ARG(!(c->train && c->p > 0.f) || rng, "head_bwd: rng required in train mode");
    // gradient pointers come in pairs: the bias gradient is the column sum of the weight-gradient launch, and the fc3 reduce
    // writes both — refused here, before the first launch, so that nothing is written
    GF_CHECK_ARG(gw1 || !gb1, "head_bwd: gb1 given without gw1 (a bias gradient needs its weight gradient)");
    GF_CHECK_ARG(gw2 || !gb2, "head_bwd: gb2 given without gw2 (a bias gradient needs its weight gradient)");
    GF_CHECK_ARG(gw3 || !gb3, "head_bwd: gb3 given without gw3 (a bias gradient needs its weight gradient)");
    GF_CHECK_ARG(!gw3 || gb3, "head_bwd: gw3 given without gb3 (the fc3 gradients are reduced together)");
    hipStream_t st = (hipStream_t)stream;
    const int T = c->T, E = c->E, D1 = c->D1, D2 = c->D2, train = c->train;
    const HeadLayout h = head_layout(c);
    const float *s0 = saved + h.s0, *u1 = saved + h.u1, *a1 = saved + h.a1, *u2 = saved + h.u2;
    const float *a2 = saved + h.a2, *prob = saved + h.prob;                                    // (kind 1)
    float *d_pre1 = workspace + h.d_pre1, *d_pre2 = workspace + h.d_pre2;                      // [T x D1], [T x D2]
    float *part2 = workspace + h.part2, *part1 = workspace + h.part1, *tailp = workspace + h.tailp;
    const bool fused = c->kind == 1 && disc_head_fused_supported(E, D1, D2) && !md.dhead_off();
    if (fused) {
        // one kernel: dprob -> d_pre3 -> d_pre2 -> d_pre1 -> dx; the fc1 / fc2 weight gradients (token reductions) stay GEMMs
        GF_TRY(launch_disc_head_bwd(d_out, x, w1, w2, w3, u1, u2, a2, prob, dx, gw1 ? d_pre1 : nullptr, gw2 ? d_pre2 : nullptr,
                                    gw3 ? tailp : nullptr, T, c->p, rng, add, train, st));
        if (gw3) GF_TRY(launch_disc_tail_reduce(tailp, disc_head_blocks(T), D2, gw3, gb3, st));
    } else if (c->kind == 0) {
        GF_TRY(launch_gelu_bwd_drop(d_out, u2, d_pre2, T, D2, c->p, SITE_HEAD2, rng, add, train, st));   // d_pre2 = d_out * gelu'(u2) * m2
    } else {
        GF_TRY(launch_disc_tail_bwd(d_out, prob, a2, u2, w3, d_pre2, gw3, gb3, T, D2, c->p, rng, add, train, st, tailp));
    }
    if (gw2) GF_TRY(gemm(gemm_tn(d_pre2, a1, gw2, D2, D1, T).sums(gb2).tn_workspace(part2, h.part2_floats).on(st)));
    EpiArgs e;
    e.p = c->p; e.rng = rng; e.rng_add = add; e.train = train;
    e.aux_in = u1; e.site = SITE_HEAD1;
    if (!fused) GF_TRY(gemm(gemm_nn(d_pre2, w2, d_pre1, T, D1, D2).epilogue(EPI_GELU_BWD_DROP, e).on(st)));
    if (gw1) GF_TRY(gemm(gemm_tn(d_pre1, s0, gw1, D1, E, T).sums(gb1).tn_workspace(part1, h.part1_floats).on(st)));
    if (fused) return 0;
    e.aux_in = x;
    if (c->kind == 0) {
        e.site = SITE_HEAD0;
        GF_TRY(gemm(gemm_nn(d_pre1, w1, dx, T, E, D1).epilogue(EPI_GELU_BWD_DROP, e).on(st)));
    } else {
        GF_TRY(gemm(gemm_nn(d_pre1, w1, dx, T, E, D1).epilogue(EPI_GELU_BWD, e).on(st)));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// plain linear
// ------------------------------------------------------------------------------------------
static bool mfma_ok(int K, int N) { return (K & 3) == 0 && (N & 3) == 0; }

extern "C" int ganffn_linear_fwd(const float* x, const float* w, const float* b, float* y, int T, int K, int N, void* stream) {
    GF_CHECK_ARG(x && w && y && T > 0 && K > 0 && N > 0, "linear_fwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if ((K & 3) == 0 && aligned16(x) && aligned16(w)) {
        return gemm(gemm_nt(x, w, y, T, N, K).bias(b).on(st));
    }
    return launch_small_linear_fwd(x, w, b, y, T, K, N, st);
}

extern "C" int64_t ganffn_linear_bwd_workspace_floats(int T, int K, int N) {
    return mfma_ok(K, N) ? a4(gemm_tn_part_floats(N, K, T)) : 0;
}

extern "C" int ganffn_linear_bwd(const float* dy, const float* x, const float* w, float* dx, float* gw, float* gb, int T,
                                 int K, int N, float* workspace, int64_t workspace_floats, void* stream) {
    GF_CHECK_ARG(dy && x && w && T > 0 && K > 0 && N > 0, "linear_bwd: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (mfma_ok(K, N) && aligned16(dy) && aligned16(x) && aligned16(w)) {
        if (dx) GF_TRY(gemm(gemm_nn(dy, w, dx, T, K, N).on(st)));
        // weight gradient: split over tokens into partial slabs when the caller lends a workspace (deterministic
        // ordered reduce), one workgroup per tile over the whole token range otherwise
        const bool ws_ok = workspace != nullptr && aligned16(workspace);
        if (gw) GF_TRY(gemm(gemm_tn(dy, x, gw, N, K, T).sums(gb).tn_workspace(ws_ok ? workspace : nullptr, ws_ok ? (long)workspace_floats : 0).on(st)));
        return 0;
    }
    return launch_small_linear_bwd(dy, x, w, dx, gw, gb, T, K, N, st);
}

// ------------------------------------------------------------------------------------------
// building blocks for unit tests
// ------------------------------------------------------------------------------------------
extern "C" int ganffn_gemm_nt(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, void* stream) {
    return gemm(gemm_nt(A, W, C, M, N, K).bias(bias).on((hipStream_t)stream));
}
extern "C" int ganffn_gemm_nn(const float* A, const float* Bm, float* C, int M, int N, int K, void* stream) {
    return gemm(gemm_nn(A, Bm, C, M, N, K).on((hipStream_t)stream));
}
extern "C" int ganffn_gemm_tn_acc(const float* At, const float* Bm, float* C, float* colsum, int M, int N, int K, void* stream) {
    return gemm(gemm_tn(At, Bm, C, M, N, K).sums(colsum).on((hipStream_t)stream));
}
extern "C" int ganffn_ffn_linear1_fwd(const float* x, const float* w1, const float* b1, float* h, int T, int E, int F, float p,
                                      uint32_t site, const uint64_t* rng, uint64_t add, int train, void* stream) {
    GF_CHECK_ARG(x && w1 && b1 && h && T > 0 && E > 0 && F > 0, "ffn_linear1_fwd: bad arguments");
    GF_CHECK_ARG(!(train && p > 0.f) || rng, "ffn_linear1_fwd: rng required when dropout is active");
    EpiArgs e;
    e.bias = b1; e.p = p; e.site = site; e.rng = rng; e.rng_add = add; e.train = train;
    return gemm(gemm_nt(x, w1, h, T, F, E).epilogue(EPI_RELU_DROP, e).on((hipStream_t)stream));
}
// test / measurement hook: the generic 64 x 64 GEMM kernel as the encoder stack launches it (bench.py replays the d_model-512
// generator's launch mix through this)
extern "C" int ganffn_gemm_hook(int mode, int epi, const float* A, const float* W, const float* bias, const float* aux, float* C,
                                int64_t slab_stride, int M, int N, int K, float p, uint32_t site, const uint64_t* rng, uint64_t add,
                                int train, int max_slabs, int* n_slabs, void* stream) {
    GF_CHECK_ARG((mode == 0 || mode == 1) && (epi == EPI_NONE || epi == EPI_RELU_DROP || epi == EPI_MASK_POS),
                 "gemm_hook: mode %d / epilogue %d not offered by the hook", mode, epi);
    GF_CHECK_ARG(epi != EPI_MASK_POS || aux, "gemm_hook: the mask epilogue needs the saved activation");
    GF_CHECK_ARG(!(epi == EPI_RELU_DROP && train && p > 0.f) || rng, "gemm_hook: rng required when dropout is active");
    EpiArgs e;
    e.bias = bias; e.aux_in = aux; e.mscale = (train && p > 0.f && epi == EPI_MASK_POS) ? 1.f / (1.f - p) : 1.f;
    e.p = p; e.site = site; e.rng = rng; e.rng_add = add; e.train = train;
    int splits = 1;
    GemmCall g = (mode == 0 ? gemm_nt(A, W, C, M, N, K) : gemm_nn(A, W, C, M, N, K)).epilogue(epi, e).on((hipStream_t)stream);
    if (max_slabs > 1 && epi == EPI_NONE) g.slabs(max_slabs, (long)slab_stride, &splits, SLABS_GENERIC);
    GF_TRY(gemm(g));
    if (n_slabs) *n_slabs = splits;
    return 0;
}
// measurement hook: the K = 100 -> 2048 products of the d_model-100 feed-forward block with the arguments the encoder stack
// gives them (bench.py --replay-family ffn_k100, tools/family_pmc.sh)
extern "C" int ganffn_ffn_k100_hook(int which, const float* a, const float* w, const float* bias, float* out, void* hmask,
                                    const float* h_saved, int T, float p, uint32_t site, const uint64_t* rng, uint64_t add, int train,
                                    void* stream) {
    GF_CHECK_ARG((which == 0 || which == 1) && a && w && out && T > 0, "ffn_k100_hook: bad arguments");
    const int E = 100, F = 2048;
    EpiArgs e;
    if (which == 0) {
        GF_CHECK_ARG(bias, "ffn_k100_hook: linear1 needs its bias");
        GF_CHECK_ARG(!(train && p > 0.f) || rng, "ffn_k100_hook: rng required when dropout is active");
        e.bias = bias; e.p = p; e.site = site; e.rng = rng; e.rng_add = add; e.train = train;
        e.mask_out = reinterpret_cast<uint16_t*>(hmask);
        return gemm(gemm_nt(a, w, out, T, F, E).epilogue(EPI_RELU_DROP, e).on((hipStream_t)stream));
    }
    GF_CHECK_ARG(hmask || h_saved, "ffn_k100_hook: the linear2 dgrad needs the pattern bits or the saved activation");
    e.aux_in = h_saved;
    e.mask_in = reinterpret_cast<const uint16_t*>(hmask);
    e.mscale = (train && p > 0.f) ? 1.f / (1.f - p) : 1.f;
    return gemm(gemm_nn(a, w, out, T, F, E).epilogue(EPI_MASK_POS, e).on((hipStream_t)stream));
}
extern "C" int ganffn_gemm_n100(const float* A, const float* W, int w_kmajor, const float* bias, float* slabs, int64_t slab_stride,
                                int T, int K, int max_slabs, int* n_slabs, void* stream) {
    GF_CHECK_ARG(n_slabs && max_slabs >= 1 && max_slabs <= MAX_SPLITS, "gemm_n100: max_slabs=%d out of [1,%d]", max_slabs, MAX_SPLITS);
    GF_CHECK_ARG(n100_supported(100, K), "gemm_n100: K=%d must be a multiple of 32, >= 256", K);
    return gemm((w_kmajor ? gemm_nn(A, W, slabs, T, 100, K) : gemm_nt(A, W, slabs, T, 100, K))
                    .bias(bias).slabs(max_slabs, (long)slab_stride, n_slabs, SLABS_N100).on((hipStream_t)stream));
}
#ifdef GANFFN_LAB
// lab builds only (make LAB=1 -> lib/libganffn_lab.so; never in the product library, not declared in include/ganffn.h):
// in-kernel time stamps of gemm_n100 (5 x uint64 per workgroup) and gemm_wres (4 x uint64)
extern "C" int ganffn_lab_set_n100_stamps(void* dev_buf) { g_n100_stamps = (unsigned long long*)dev_buf; return 0; }
extern "C" int ganffn_lab_set_wres_stamps(void* dev_buf) { g_wres_stamps = (unsigned long long*)dev_buf; return 0; }
#endif
extern "C" int ganffn_debug_set_ffn_mode(int bits) {
    g_mode_word.store((uint32_t)bits, std::memory_order_relaxed);
    return 0;
}
extern "C" int64_t ganffn_gemm_tn_grouped_workspace_floats(void) { return gemm_tn_grouped_part_floats(); }
extern "C" int ganffn_gemm_tn_grouped(int n, const float* const* At, const float* const* Bm, float* const* C, float* const* colsum,
                                      const int* M, const int* N, const int* K, float* workspace, int64_t workspace_floats,
                                      void* stream) {
    GF_CHECK_ARG(n >= 1 && n <= 40 && At && Bm && C && M && N && K, "gemm_tn_grouped: bad arguments");
    TnDesc d[40];
    for (int i = 0; i < n; ++i) d[i] = TnDesc{At[i], M[i], Bm[i], N[i], C[i], N[i], colsum ? colsum[i] : nullptr, M[i], N[i], K[i]};
    return launch_gemm_tn_grouped(d, n, (hipStream_t)stream, workspace, (long)workspace_floats);
}
extern "C" int ganffn_attention_fwd(const float* qkv, float* o, float* lse, int S, int B, int E, int H, float p, uint32_t site,
                                    const uint64_t* rng, uint64_t add, void* stream) {
    return attention_fwd(attn_call(S, B, E, H, p, site, rng, add, (hipStream_t)stream).forward(AttnSeg{qkv, o, lse, nullptr, 1}));
}
extern "C" int64_t ganffn_attention_keep_words(int B, int H) { return (int64_t)B * H * ATTN_KEEP_WORDS; }
extern "C" int ganffn_attention_fwd_keep(const float* qkv, float* o, float* lse, uint32_t* keep, int S, int B, int E, int H, float p,
                                         uint32_t site, const uint64_t* rng, uint64_t add, void* stream) {
    return attention_fwd(attn_call(S, B, E, H, p, site, rng, add, (hipStream_t)stream).forward(AttnSeg{qkv, o, lse, keep, 1}));
}
extern "C" int ganffn_attention_bwd_keep(const float* qkv, const float* o, const float* lse, const float* d_o, const uint32_t* keep,
                                         float* d_qkv, int S, int B, int E, int H, float p, uint32_t site, const uint64_t* rng,
                                         uint64_t add, void* stream) {
    return attention_bwd(attn_call(S, B, E, H, p, site, rng, add, (hipStream_t)stream).backward(qkv, o, lse, keep, d_o, d_qkv, 1));
}
extern "C" int ganffn_attention_bwd(const float* qkv, const float* o, const float* lse, const float* d_o, float* d_qkv, int S,
                                    int B, int E, int H, float p, uint32_t site, const uint64_t* rng, uint64_t add,
                                    void* stream) {
    return attention_bwd(attn_call(S, B, E, H, p, site, rng, add, (hipStream_t)stream).backward(qkv, o, lse, nullptr, d_o, d_qkv, 1));
}
// the attention pair with per-dialogue key lengths (keep may be NULL; key_len NULL = the pairs above)
extern "C" int ganffn_attention_fwd_len(const float* qkv, float* o, float* lse, uint32_t* keep, const int32_t* key_len, int S, int B,
                                        int E, int H, float p, uint32_t site, const uint64_t* rng, uint64_t add, void* stream) {
    return attention_fwd(attn_call(S, B, E, H, p, site, rng, add, (hipStream_t)stream).mask(key_len, 0).forward(AttnSeg{qkv, o, lse, keep, 1}));
}
extern "C" int ganffn_attention_bwd_len(const float* qkv, const float* o, const float* lse, const float* d_o, const uint32_t* keep,
                                        const int32_t* key_len, float* d_qkv, int S, int B, int E, int H, float p, uint32_t site,
                                        const uint64_t* rng, uint64_t add, void* stream) {
    return attention_bwd(attn_call(S, B, E, H, p, site, rng, add, (hipStream_t)stream).mask(key_len, 0).backward(qkv, o, lse, keep, d_o, d_qkv, 1));
}
// the same pair with a flags word (GANFFN_ATTN_CAUSAL; 0 = the _len pair, an unknown bit is refused before any launch)
extern "C" int ganffn_attention_fwd_mask(const float* qkv, float* o, float* lse, uint32_t* keep, const int32_t* key_len, uint32_t flags,
                                         int S, int B, int E, int H, float p, uint32_t site, const uint64_t* rng, uint64_t add,
                                         void* stream) {
    return attention_fwd(attn_call(S, B, E, H, p, site, rng, add, (hipStream_t)stream).mask(key_len, flags).forward(AttnSeg{qkv, o, lse, keep, 1}));
}
extern "C" int ganffn_attention_bwd_mask(const float* qkv, const float* o, const float* lse, const float* d_o, const uint32_t* keep,
                                         const int32_t* key_len, uint32_t flags, float* d_qkv, int S, int B, int E, int H, float p,
                                         uint32_t site, const uint64_t* rng, uint64_t add, void* stream) {
    return attention_bwd(attn_call(S, B, E, H, p, site, rng, add, (hipStream_t)stream).mask(key_len, flags).backward(qkv, o, lse, keep, d_o, d_qkv, 1));
}
