// attention16.hip — self-attention core for SMALL heads (head_dim <= 32: the d_model = 100 / 10-head networks, i.e. five of
// the six networks of the GAN step, and the 300-d MELD-dimension stack), forward and backward, on
// v_mfma_f32_16x16x4_f32 (exact fp32).
//
// Replaces the attention core of torch's nn.MultiheadAttention inside nn.TransformerEncoderLayer
// (/root/reference/model.py:1210,1276,1307,1340,1377): P = softmax(q k^T / sqrt(hd)) over keys, NO masks (unless the caller gives key
// lengths: keys at or past a dialogue's length then get probability 0 — an extension, see ganffn_attention_fwd_len), dropout(0.1)
// on P in train mode, O = P v.
//
// Why a second kernel family (attention.hip keeps head_dim 60/64): with hd = 10 a 32x32x2 MFMA product that has the head
// dimension on its M axis uses 10 of 32 output rows, and one wave per 32 queries leaves one wave per SIMD with every
// latency (LDS, Philox, exp) exposed.  Here a wave owns 16 queries (forward) or 16 keys (backward): 16x16x4 tiles waste
// 10/16 instead of 10/32, a (dialogue, head) problem is 6-7 waves instead of 3, so a CU holds 2-3 waves per SIMD and one
// wave's VALU work (softmax, Philox) runs under another's MFMAs.
//
// Forward (query on the lane): S^T = K Q^T leaves a lane's query with all its keys in that lane's registers (softmax
// max/sum = in-lane + two cross-group shuffles), and the probability tile is directly the B operand of O^T = V^T P^T
// (an accumulator tile feeds the next MFMA; k index = key, permuted consistently on the LDS side).  The forward also
// writes the log-sum-exp of every (dialogue, head, query) row.
// Backward (KEY on the lane): S = Q K^T and dP = dO V^T have the key on the lane and 4 consecutive queries in the 4
// accumulator registers, so
//   * P = exp(S - LSE) needs no reduction (LSE saved by the forward; D_i = sum_d dO_id O_id from the saved output);
//   * the Philox contract (one call = 4 consecutive queries at one key) is exactly one call per accumulator tile per
//     lane — no mask exchange between lanes;
//   * the tiles are directly the B operands of dV^T = dO^T P~ and dK^T = Q^T dS (a wave owns its 16 keys' dK, dV:
//     no reduction across waves, no atomics);  only dS crosses LDS once, for dQ = dS K.
// Layout: qkv [T x 3E] packed q|k|v per token (t = s*B + b), head h = columns h*hd .. h*hd+hd-1; lse [B*H x S].
#include "common.h"

namespace ganffn {

typedef float floatx4 __attribute__((ext_vector_type(4)));

namespace {

template <int HD>
struct A16 {
    static constexpr int KS = (HD + 3) / 4;                 // k-steps of 4 over the head dimension
    static constexpr int NTD = (HD + 15) / 16;              // 16-row output tiles over the head dimension
    // row stride of the [*, hd] LDS matrices: >= 4 KS, and = 4 (mod 8) so that rows 4 apart sit 16 banks apart
    // (the "4 consecutive keys x 16 head-dim columns" operand reads of both half-waves are then conflict-free)
    static constexpr int LD = (KS & 1) ? 4 * KS : 4 * KS + 4;
    static constexpr int TAIL = 16 * NTD;                   // floats readable past the last row (discarded outputs)
};
static_assert(A16<10>::LD == 12 && A16<30>::LD == 36 && A16<16>::LD == 20 && A16<12>::LD == 12, "LD rule");

struct HeadSrc16 {
    float* dst;
    const float* src;
    int ld_src;
    float scale;
    int key;       // 1: a k or v matrix, staged up to the dialogue's key length; 0: q or dO, staged up to S (the rest zero)
};

// Stage NM [S x HD] head slices into LDS images [16 NT rows][LD] (rows >= S and columns >= HD zero), in two phases so that
// the caller can put data-independent work (the Philox calls) between issuing the global loads and waiting for them.
// load(): every global load of all matrices, UNCONDITIONAL, from clamped addresses, nothing else — no use of a loaded
// value before store().  (Round 4: the first version wrote `ok ? q * scale : 0` in load(); hipcc turned each such select
// into a load under an exec-mask branch and, where the scale multiply followed, put an `s_waitcnt vmcnt(0)` right behind
// it: the forward of a d_model-100 pass paid FIVE dependent global round trips before its first LDS write, the backward
// three.  Out-of-range elements are now zeroed by a 0 / scale FACTOR at store time — a multiply cannot be folded into
// "do not load" — and a sched_barrier keeps the loads together.)
template <int HD, int NT, int NM, int NW = NT>   // NW: waves of the workgroup doing the staging
struct HeadStage {
    static constexpr int LD = A16<HD>::LD, PR = LD / 2, ROWS = 16 * NT, PER = ROWS * PR, NTH = 64 * NW;
    static constexpr int U = (PER + NTH - 1) / NTH;
    float2 v[NM][U];
    __device__ __forceinline__ void load(const HeadSrc16 (&m)[NM], int S, int B, int b, int tid) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = min(tid + u * NTH, PER - 1);
            const int s = i / PR, j = i - s * PR;
            const size_t row = (size_t)(min(s, S - 1) * B + b);
            const int col = min(2 * j, HD - 2);
#pragma unroll
            for (int mi = 0; mi < NM; ++mi) v[mi][u] = *reinterpret_cast<const float2*>(m[mi].src + row * m[mi].ld_src + col);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ __forceinline__ void store(const HeadSrc16 (&m)[NM], int S, int n, int tid) const {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = tid + u * NTH;
            if (PER % NTH == 0 || i < PER) {
                const int s = i / PR, j = i - s * PR;
                const float in = (s < S && 2 * j < HD) ? 1.f : 0.f;
                const float ink = (s < n && 2 * j < HD) ? 1.f : 0.f;      // (without lengths n is S: the same value)
#pragma unroll
                for (int mi = 0; mi < NM; ++mi) {
                    const float f = (m[mi].key ? ink : in) * m[mi].scale;
                    *reinterpret_cast<float2*>(m[mi].dst + s * LD + 2 * j) = make_float2(v[mi][u].x * f, v[mi][u].y * f);
                }
            }
        }
#pragma unroll
        for (int mi = 0; mi < NM; ++mi)
            if (tid < A16<HD>::TAIL) m[mi].dst[ROWS * LD + tid] = 0.f;
    }
};

// acc[t] (+)= X_t Y^T over the head dimension: A = rows 16t + c of Xm (one tile per t), B = row `yrow` of Ym for this lane.
// D[m][n]: m = row of X inside tile t (4g + reg), n = this lane's Y row.
template <int HD, int NT>
__device__ __forceinline__ void dot_tiles(floatx4 (&acc)[NT], const float* __restrict__ Xm, const float* __restrict__ yb,
                                          int c, int g) {
    constexpr int LD = A16<HD>::LD, KS = A16<HD>::KS;
    constexpr int BT = KS <= 4 ? KS : (KS % 4 == 0 ? 4 : (KS % 3 == 0 ? 3 : (KS % 5 == 0 ? 5 : 1)));
    const float* pa = Xm + c * LD + g;
#pragma unroll
    for (int k0 = 0; k0 < KS; k0 += BT) {
        float av[BT][NT], bv[BT];
#pragma unroll
        for (int j = 0; j < BT; ++j) {
            bv[j] = yb[4 * (k0 + j)];
#pragma unroll
            for (int t = 0; t < NT; ++t) av[j][t] = pa[t * 16 * LD + 4 * (k0 + j)];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < BT; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j][t], bv[j], acc[t], 0, 0, 0);
    }
}

// out[dt] (rows d = 16 dt + 4g + reg, column = this lane's n) += sum over rows x = 16t + 4g' + reg of Mm[x][d] * P[t][reg]
// (P = accumulator tiles used as the B operand; k index = g').  Two interleaved accumulator chains per output tile.
template <int HD, int NT>
__device__ __forceinline__ void apply_tiles(floatx4 (&out)[A16<HD>::NTD], const floatx4 (&P)[NT], const float* __restrict__ Mm,
                                            int c, int g) {
    constexpr int LD = A16<HD>::LD, NTD = A16<HD>::NTD;
    floatx4 alt[NTD];
#pragma unroll
    for (int dt = 0; dt < NTD; ++dt) alt[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float* pa = Mm + 4 * g * LD + c;
    float av[2][4][NTD];
    auto fetch = [&](int t, float (&dst)[4][NTD]) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int dt = 0; dt < NTD; ++dt) dst[r][dt] = pa[(16 * t + r) * LD + 16 * dt];
    };
    fetch(0, av[0]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t + 1 < NT) fetch(t + 1, av[(t + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int dt = 0; dt < NTD; ++dt) {
                if (r & 1) alt[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t & 1][r][dt], P[t][r], alt[dt], 0, 0, 0);
                else out[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t & 1][r][dt], P[t][r], out[dt], 0, 0, 0);
            }
    }
#pragma unroll
    for (int dt = 0; dt < NTD; ++dt) out[dt] += alt[dt];
}

// Causal forms: a wave needs only the tiles on its side of the diagonal.  The number of live tiles is wave-uniform (w is taken
// through readfirstlane: an SGPR), and tile_dispatch turns it into a COMPILE-TIME count once: a chain of scalar compares calls
// f(integral_constant<I>) for I == w, and the body behind each arm is straight-line code over exactly its live tiles, with the
// batched operand loads of dot_tiles / apply_tiles.  (The first version guarded every tile of every loop with `if (t <= w)`:
// correct, but hipcc copied the accumulator tiles at each of the ~40 merges — 327 v_mov against 32 and 147 VGPRs against 65 in
// the 7-tile forward.)
// -DGANFFN_CAUSAL_MASK_ONLY builds the causal kernels with the mask alone (every tile computed): the other side of the measurement
// in profiles/attention_causal_ab.txt, not a product configuration.
#ifdef GANFFN_CAUSAL_MASK_ONLY
constexpr bool CAUSAL_SKIP = false;
#else
constexpr bool CAUSAL_SKIP = true;
#endif

template <int NT, int I = 0, class F>
__device__ __forceinline__ void tile_dispatch(int w, F&& f) {
    if constexpr (I + 1 >= NT) {
        f(std::integral_constant<int, I>{});
    } else {
        if (w == I) f(std::integral_constant<int, I>{});
        else tile_dispatch<NT, I + 1>(w, f);
    }
}

// value of lane r of this lane's quad (DPP quad_perm broadcast)
template <int R>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, R * 0x55, 0xF, 0xF, true);
}

// store 4 consecutive head-dim values d0 .. d0+3 (this lane's accumulator registers) of one token row
template <int HD>
__device__ __forceinline__ void store4(float* __restrict__ row, int d0, const floatx4& v, float mul) {
    if (d0 + 1 < HD) *reinterpret_cast<float2*>(row + d0) = make_float2(v[0] * mul, v[1] * mul);
    if (d0 + 3 < HD) *reinterpret_cast<float2*>(row + d0 + 2) = make_float2(v[2] * mul, v[3] * mul);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// forward: one workgroup per (dialogue, head, block of WPB query tiles); a wave owns 16 queries.  WPB < NT cuts a
// (dialogue, head) problem into NT / WPB workgroups that each stage the head's K and V again (a few KB out of L2) — the
// 320 problems of a d_model-100 pass are 1.25 per CU as whole workgroups (64 CUs hold two), finer workgroups spread evenly
// ------------------------------------------------------------------------------------------
// PAIR: two batches of the same shape in one launch (the eval-mode and the train-mode pass of one generator): workgroups
// 0 .. nb0 - 1 are the first batch's, the rest the second's with its own qkv / o / lse / keep words and train flag (s1).  The
// choice is wave-uniform and made once; (dialogue, head) indices and with them the Philox row groups are local to the batch,
// so each batch gets the bits of its own launch.
struct Attn16Seg1 {
    const float* qkv; float* o; float* lse; uint32_t* keepw; int train;
};
// LEN: per-dialogue key lengths (key_len, device int32 [B]; with PAIR both batches are the same B dialogues and b is already
// local to the batch, so key_len[b] serves both).  A template flag and not a test of the
// pointer: the instantiations without lengths (every launch of the GAN step) keep the instructions they had — no scalar load, no
// uniform branch (the listings compared: profiles/attention_key_len_ab.txt).
// CAUSAL (only with LEN; a null key_len reads as S): query i attends to keys j <= i, i.e. the lane's key limit is
// min(n, query + 1).  Wave w owns query tile w, so key tiles t > w are dead: the wave runs the tail of the kernel compiled for
// w + 1 key tiles (tile_dispatch) — no score MFMAs, exp / sum work or P V products for the rest, and no Philox calls.
// PAIR && CAUSAL (both segments of a generator's two-segment pass under the mask): the segment choice comes first and changes
// pointers and the train flag only, so everything after it is the single-batch causal kernel — w through readfirstlane, the
// dispatch over key tiles 0 .. w in both segments, dead tiles skipped in the keep-bit loop, keep words stored by the train
// segment alone (dc.on) — and each segment has the bits of its own causal launch.
template <int HD, int NT, int WPB, bool PAIR = false, bool LEN = false, bool CAUSAL = false>
__global__ __launch_bounds__(64 * WPB) void attn16_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ o,
                                                             float* __restrict__ lse, uint32_t* __restrict__ keepw, int S, int B,
                                                             int E, int H, float p, uint32_t site,
                                                             const uint64_t* __restrict__ rng, uint64_t add, int train,
                                                             Attn16Seg1 s1, int nb0,
                                                             const int32_t* __restrict__ key_len) {
    unsigned bid = blockIdx.x;
    if constexpr (PAIR) {
        if (bid >= (unsigned)nb0) {
            bid -= (unsigned)nb0;
            qkv = s1.qkv; o = s1.o; lse = s1.lse; keepw = s1.keepw; train = s1.train;
        }
    }
    constexpr int LD = A16<HD>::LD, NTD = A16<HD>::NTD, MAT = 16 * NT * LD + A16<HD>::TAIL;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    static_assert(NT % WPB == 0, "query tiles per workgroup must divide the tile count");
    constexpr int NQB = NT / WPB;
    const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
    static_assert(!CAUSAL || LEN, "the causal instantiations are those with lengths");
    const int bh = bid / NQB;
    const int w0 = (bid - bh * NQB) * WPB + (tid >> 6);
    const int w = CAUSAL ? __builtin_amdgcn_readfirstlane(w0) : w0;      // w: query tile of this wave
    const int b = bh / H, head = bh - b * H;
    const int n = LEN ? attn_key_len(key_len, b, S) : S;      // keys < n take part (workgroup-uniform)
    float* Qs = smem;
    float* Ks = Qs + MAT;
    float* Vs = Ks + MAT;
    const int ld3 = 3 * E;
    const DropCtx dc = make_drop(rng, add, site, p, train);
    uint32_t mine = 0;
    {
        const HeadSrc16 m3[3] = {{Qs, qkv + head * HD, ld3, rsqrtf((float)HD), 0}, {Ks, qkv + E + head * HD, ld3, 1.f, 1},
                                 {Vs, qkv + 2 * E + head * HD, ld3, 1.f, 1}};
        HeadStage<HD, NT, 3, WPB> stg;
        stg.load(m3, S, B, b, tid);
        if (dc.on) {
            // Dropout keep-bits, computed while the global loads are in flight (they depend on indices only).  One Philox
            // call = 4 consecutive queries (the 4 lanes of a quad) at one key.  Lane ql of a quad evaluates the calls of
            // register r == ql (keys 16t + 4g + ql); bit 4t + qq of `mine` = keep(query 4Q + qq, that key).
            const int ql = c & 3;
            const uint32_t rowgroup = (uint32_t)(bh * 28 + 4 * w + (c >> 2));
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (CAUSAL && CAUSAL_SKIP && t > w) continue;      // dead key tile: its keep bits are never read
                uint32_t wd[4];
                philox4(rowgroup * 128u + (uint32_t)(16 * t + 4 * g + ql), dc.site, dc.o0, dc.o1, dc.k0, dc.k1, wd);
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) mine |= (wd[qq] >= dc.thr ? 1u : 0u) << (4 * t + qq);
            }
            // keep words for the backward (A16_KEEP_WORDS per (dialogue, head)): word [query group Q = 4w + c/4][4g + ql],
            // nibble t = the four queries of the group at key 16t + 4g + ql — one coalesced dword store per lane; the
            // backward then needs no Philox call at all (its lane (key 16w' + c', group g') reads word [4t + g'][c'])
            if (keepw != nullptr) keepw[(size_t)rowgroup * 16 + 4 * g + ql] = mine;
        }
        stg.store(m3, S, n, tid);
    }
    __syncthreads();

    // CAUSAL: the rest of the kernel over the first NL = w + 1 key tiles, then return.  (One algorithm written twice: the code below
    // is that of the kernels without the flag, left where and as it was so that they keep their instructions — sharing one body
    // with the causal form, or only moving it into a block of its own, changed their listings.)
    if constexpr (CAUSAL) {
        auto tail = [&](auto nl_) {
            constexpr int NL = decltype(nl_)::value + 1;
            // S^T tiles: pr[t][reg] = score(key 16t + 4g + reg, query 16w + c)
            floatx4 pr[NL];
#pragma unroll
            for (int t = 0; t < NL; ++t) pr[t] = floatx4{0.f, 0.f, 0.f, 0.f};
            dot_tiles<HD, NL>(pr, Ks, Qs + (16 * w + c) * LD + g, c, g);

            const int lim = min(n, 16 * w + c + 1);     // this lane's query sees keys < lim (>= 1, ghost queries too)
            float m = -INFINITY;
#pragma unroll
            for (int t = 0; t < NL; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (16 * t + 4 * g + r >= lim) pr[t][r] = -INFINITY;
                    m = fmaxf(m, pr[t][r]);
                }
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < NL; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = __expf(pr[t][r] - m);     // exp(-inf) = 0 for padded keys
                    pr[t][r] = e;
                    sum += e;
                }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            const float inv = 1.0f / sum;
            const int qi = 16 * w + c;
            if (lse != nullptr && g == 0 && qi < S) lse[(size_t)bh * S + qi] = m + __logf(sum);

            if (dc.on) {
                const int ql = c & 3;
                const uint32_t mq[4] = {quad_bcast<0>(mine), quad_bcast<1>(mine), quad_bcast<2>(mine), quad_bcast<3>(mine)};
                const float ps = inv * dc.scale;
#pragma unroll
                for (int t = 0; t < NL; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pr[t][r] = ((mq[r] >> (4 * t + ql)) & 1u) ? pr[t][r] * ps : 0.f;
            } else {
#pragma unroll
                for (int t = 0; t < NL; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) pr[t][r] *= inv;
            }

            // O^T[d][query] = sum_key V[key][d] P~^T[key][query]
            floatx4 oacc[NTD];
#pragma unroll
            for (int dt = 0; dt < NTD; ++dt) oacc[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
            apply_tiles<HD, NL>(oacc, pr, Vs, c, g);
            if (qi < S) {
                float* orow = o + (size_t)(qi * B + b) * E + head * HD;
#pragma unroll
                for (int dt = 0; dt < NTD; ++dt) store4<HD>(orow, 16 * dt + 4 * g, oacc[dt], 1.f);
            }
        };
        if constexpr (CAUSAL_SKIP) tile_dispatch<NT>(w, tail);      // key tiles 0 .. w
        else tail(std::integral_constant<int, NT - 1>{});
        return;
    }
    // S^T tiles: pr[t][reg] = score(key 16t + 4g + reg, query 16w + c)
    floatx4 pr[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) pr[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    dot_tiles<HD, NT>(pr, Ks, Qs + (16 * w + c) * LD + g, c, g);

    float m = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (16 * t + 4 * g + r >= n) pr[t][r] = -INFINITY;
            m = fmaxf(m, pr[t][r]);
        }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = __expf(pr[t][r] - m);     // exp(-inf) = 0 for padded keys
            pr[t][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    const int qi = 16 * w + c;
    if (lse != nullptr && g == 0 && qi < S) lse[(size_t)bh * S + qi] = m + __logf(sum);

    if (dc.on) {
        const int ql = c & 3;
        const uint32_t mq[4] = {quad_bcast<0>(mine), quad_bcast<1>(mine), quad_bcast<2>(mine), quad_bcast<3>(mine)};
        const float ps = inv * dc.scale;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[t][r] = ((mq[r] >> (4 * t + ql)) & 1u) ? pr[t][r] * ps : 0.f;
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[t][r] *= inv;
    }

    // O^T[d][query] = sum_key V[key][d] P~^T[key][query]
    floatx4 oacc[NTD];
#pragma unroll
    for (int dt = 0; dt < NTD; ++dt) oacc[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    apply_tiles<HD, NT>(oacc, pr, Vs, c, g);
    if (qi < S) {
        float* orow = o + (size_t)(qi * B + b) * E + head * HD;
#pragma unroll
        for (int dt = 0; dt < NTD; ++dt) store4<HD>(orow, 16 * dt + 4 * g, oacc[dt], 1.f);
    }
}

// ------------------------------------------------------------------------------------------
// backward: wave w owns keys 16w .. 16w+15 (dK, dV) and, after the dS hand-over, queries 16w .. 16w+15 (dQ)
// ------------------------------------------------------------------------------------------
// SAVED: the dropout keep bits come from the words the forward stored (keepw) instead of Philox calls — the same bits, so
// both forms give identical results (tests/test_hip_ops.py::test_attention_fwd_bwd compares them with torch.equal)
// CAUSAL (only with LEN): P = 0 for keys past the query, set explicitly (exp(s - lse) is not 0 there).  Wave w owns keys
// 16w .. 16w+15 and needs query tiles t >= w only: it runs the products compiled for NT - w query tiles (tile_dispatch) — no score /
// dP MFMAs, Philox calls (or keep-word unpacking), exp work or dV / dK products for tiles t < w — and their dS is neither
// written to LDS nor read: the dQ product of query tile w reads key tiles t <= w, which are exactly the ones key-wave t wrote
// for query tile w >= t.  Every wave reaches both barriers: they stand outside the dispatched parts.
template <int HD, int NT, bool SAVED, bool LEN = false, bool CAUSAL = false>
__global__ __launch_bounds__(64 * NT) void attn16_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                             const float* __restrict__ lse, const float* __restrict__ d_o,
                                                             const uint32_t* __restrict__ keepw, float* __restrict__ d_qkv,
                                                             int S, int B, int E, int H, float p, uint32_t site,
                                                             const uint64_t* __restrict__ rng, uint64_t add, int train,
                                                             const int32_t* __restrict__ key_len) {
    constexpr int LD = A16<HD>::LD, NTD = A16<HD>::NTD, KS = A16<HD>::KS, ROWS = 16 * NT, MAT = ROWS * LD + A16<HD>::TAIL;
    constexpr int LDS_S = ROWS + 4;                      // dS image [query][key]: rows 4 apart sit 16 banks apart
    extern __shared__ __attribute__((aligned(16))) float smem[];
    static_assert(!CAUSAL || LEN, "the causal instantiations are those with lengths");
    const int tid = threadIdx.x, lane = tid & 63, w0 = tid >> 6, c = lane & 15, g = lane >> 4;
    const int w = CAUSAL ? __builtin_amdgcn_readfirstlane(w0) : w0;      // causal: an SGPR, so the tile skips are scalar branches
    const int bh = blockIdx.x, b = bh / H, head = bh - b * H;
    const int n = LEN ? attn_key_len(key_len, b, S) : S;      // keys < n take part (workgroup-uniform)
    // K, LSE and D live for the whole kernel; scaled q, V and dO are dead once dV / dK are accumulated, and the dS image
    // takes their place (one more barrier) — at S = 94 that is 43 KB instead of 57 KB a workgroup: three per CU, not two
    float* Ks = smem;
    float* Ls = Ks + MAT;        // [ROWS] log-sum-exp per query (+big for padded rows)
    float* Ds = Ls + ROWS;       // [ROWS] D_i = sum_d dO_id O_id
    uint32_t* Wk = reinterpret_cast<uint32_t*>(Ds + ROWS);    // [NT][64] keep words (saved-mask form)
    float* Qs = Ds + ROWS + 64 * NT;       // scaled q
    float* Vs = Qs + MAT;
    float* Os = Vs + MAT;        // dO
    float* SS = Qs;              // [ROWS][LDS_S] dS, over q / V / dO
    const int ld3 = 3 * E;
    const float scale = rsqrtf((float)HD);
    const DropCtx dc = make_drop(rng, add, site, p, train);
    uint32_t wdt[NT][4];                 // Philox words of this lane's (key, 4-query group) pairs (saved masks: all-ones / zero)
    uint32_t kw1 = 0;                    // saved masks: keep word [4w + g][c] — wave w fetches word row w for the whole workgroup
#pragma unroll
    for (int t = 0; t < NT; ++t) wdt[t][0] = wdt[t][1] = wdt[t][2] = wdt[t][3] = 0xFFFFFFFFu;
    {
        const HeadSrc16 m4[4] = {{Qs, qkv + head * HD, ld3, scale, 0}, {Ks, qkv + E + head * HD, ld3, 1.f, 1},
                                 {Vs, qkv + 2 * E + head * HD, ld3, 1.f, 1}, {Os, d_o + head * HD, E, 1.f, 0}};
        // D and LSE of this wave's 16 query rows, straight from global memory (issued with the staging loads)
        const int qi = 16 * w + c;
        const size_t rowo = (size_t)(min(qi, S - 1) * B + b) * E + head * HD;
        float part = 0.f;
        float ov[KS], dv[KS];
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const int d = min(4 * kk + g, HD - 1);
            ov[kk] = o[rowo + d];
            dv[kk] = d_o[rowo + d];
        }
        const float lv = lse[(size_t)bh * S + min(qi, S - 1)];
        HeadStage<HD, NT, 4> stg;
        stg.load(m4, S, B, b, tid);
        if (SAVED) {
            // every wave needs a nibble of ALL 4 NT keep words of its (c, g) column: each wave fetches one word row (one
            // coalesced dword per lane) and the rows meet in LDS (all six words per lane straight from memory measured
            // slower than the Philox calls at 640 problems: 25.9 against 23.9 us)
            kw1 = keepw[((size_t)bh * 28 + 4 * w + g) * 16 + c];
            __builtin_amdgcn_sched_barrier(0);
        }
        if (!SAVED && dc.on) {
            // the keep words of this lane's (key, 4-query group) pairs: exactly one Philox call per accumulator tile, and
            // data-independent — evaluated while the global loads are in flight
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (CAUSAL && CAUSAL_SKIP && t < w) continue;      // dead query tile
                philox4((uint32_t)(bh * 28 + 4 * t + g) * 128u + (uint32_t)(16 * w + c), dc.site, dc.o0, dc.o1, dc.k0, dc.k1, wdt[t]);
            }
        }
        stg.store(m4, S, n, tid);
        if (SAVED) Wk[tid] = kw1;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) part += (4 * kk + g < HD && qi < S) ? ov[kk] * dv[kk] : 0.f;
        part += __shfl_xor(part, 16, 64);
        part += __shfl_xor(part, 32, 64);
        if (g == 0) {
            Ds[qi] = part;
            Ls[qi] = qi < S ? lv : 1e30f;
        }
    }
    __syncthreads();
    // CAUSAL: the rest of the kernel over the live tiles only, then return (the code below is the kernels' without the flag: see
    // the forward)
    if constexpr (CAUSAL) {
        const int kj = 16 * w + c;                     // this lane's key
        floatx4 ds[NT];                                // dS of this lane's key, query tiles F .. NT-1 (handed to LDS below)
        // scores, P~, dS and the dV / dK products over the query tiles F .. NT-1 (F = the wave's own tile w, a compile-time value)
        auto products = [&](auto f_) {
            constexpr int F = decltype(f_)::value, NL = NT - F;
            if (SAVED) {
                // the same registers the Philox form fills: all-ones (kept) or zero (dropped: 0 < thr) — the rest of the kernel is
                // one code path (a separate bit-test path compiled to 82 VGPRs and ran SLOWER than the Philox calls at 640 problems)
#pragma unroll
                for (int t = F; t < NT; ++t) {
                    const uint32_t nib = Wk[64 * t + lane] >> (4 * w);
#pragma unroll
                    for (int r = 0; r < 4; ++r) wdt[t][r] = ((nib >> r) & 1u) ? 0xFFFFFFFFu : 0u;
                }
            }

            floatx4 ps[NL], dp[NL];
            // initial accumulators: -LSE[query] for the scores (P = exp(acc) needs no subtraction), 0 for dP
#pragma unroll
            for (int t = 0; t < NL; ++t) {
                const float4 l4 = *reinterpret_cast<const float4*>(Ls + 16 * (F + t) + 4 * g);
                ps[t] = floatx4{-l4.x, -l4.y, -l4.z, -l4.w};
                dp[t] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
            dot_tiles<HD, NL>(ps, Qs + F * 16 * LD, Ks + kj * LD + g, c, g);      // S[query 16t+4g+reg][key kj] - LSE
            dot_tiles<HD, NL>(dp, Os + F * 16 * LD, Vs + kj * LD + g, c, g);      // dP~[query][key] = dO . V

            // a key past the dialogue's length has P = 0 (and with it dS = 0): its dK and dV rows are written as zeros
            const bool keyok = kj < n;
#pragma unroll
            for (int t = 0; t < NL; ++t) {
                const float4 d4 = *reinterpret_cast<const float4*>(Ds + 16 * (F + t) + 4 * g);
                const float dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = keyok && kj <= 16 * (F + t) + 4 * g + r;      // the key is not past the query
                    const float pv = ok ? __expf(ps[t][r]) : 0.f;                // probability (pre-dropout)
                    const bool keep = !dc.on || wdt[F + t][r] >= dc.thr;
                    const float dpk = keep ? dp[t][r] * dc.scale : 0.f;          // dP = keep * scale * dP~
                    ps[t][r] = keep ? pv * dc.scale : 0.f;                       // P~
                    dp[t][r] = pv * (dpk - dd[r]);                               // dS
                }
            }

            // dV^T[d][key] = sum_q dO[q][d] P~[q][key];  dK^T[d][key] = sum_q (scale Q)[q][d] dS[q][key]
            floatx4 av[NTD], ak[NTD];
#pragma unroll
            for (int dt = 0; dt < NTD; ++dt) { av[dt] = floatx4{0.f, 0.f, 0.f, 0.f}; ak[dt] = floatx4{0.f, 0.f, 0.f, 0.f}; }
            const float* pv_ = Os + (F * 16 + 4 * g) * LD + c;
            const float* pk_ = Qs + (F * 16 + 4 * g) * LD + c;
            float a1[2][4][NTD], a2[2][4][NTD];
            auto fetch = [&](int t, float (&d1)[4][NTD], float (&d2)[4][NTD]) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int dt = 0; dt < NTD; ++dt) {
                        d1[r][dt] = pv_[(16 * t + r) * LD + 16 * dt];
                        d2[r][dt] = pk_[(16 * t + r) * LD + 16 * dt];
                    }
            };
            fetch(0, a1[0], a2[0]);
#pragma unroll
            for (int t = 0; t < NL; ++t) {
                if (t + 1 < NL) fetch(t + 1, a1[(t + 1) & 1], a2[(t + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int dt = 0; dt < NTD; ++dt) {
                        av[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t & 1][r][dt], ps[t][r], av[dt], 0, 0, 0);
                        ak[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[t & 1][r][dt], dp[t][r], ak[dt], 0, 0, 0);
                    }
            }
            if (kj < S) {
                float* row = d_qkv + (size_t)(kj * B + b) * ld3 + head * HD;
#pragma unroll
                for (int dt = 0; dt < NTD; ++dt) {
                    store4<HD>(row + 2 * E, 16 * dt + 4 * g, av[dt], 1.f);
                    store4<HD>(row + E, 16 * dt + 4 * g, ak[dt], 1.f);
                }
            }
#pragma unroll
            for (int t = 0; t < NL; ++t) ds[F + t] = dp[t];
        };
        if constexpr (CAUSAL_SKIP) tile_dispatch<NT>(w, products);      // query tiles w .. NT-1
        else products(std::integral_constant<int, 0>{});
        // dS -> LDS [query][key], over the operands every wave has finished reading
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (CAUSAL_SKIP && t < w) continue;      // never computed, never read: query tile t takes key tiles <= t only
#pragma unroll
            for (int r = 0; r < 4; ++r) SS[(16 * t + 4 * g + r) * LDS_S + kj] = ds[t][r];
        }
        __syncthreads();

        // dQ^T[d][query 16w + c] = scale * sum_key K[key][d] dS[query][key], over the key tiles 0 .. w
        auto dq = [&](auto nl_) {
            constexpr int NL = decltype(nl_)::value + 1;
            floatx4 pq[NL];
            const float* ss = SS + (16 * w + c) * LDS_S + 4 * g;
#pragma unroll
            for (int t = 0; t < NL; ++t) {
                const float4 q4 = *reinterpret_cast<const float4*>(ss + 16 * t);
                pq[t] = floatx4{q4.x, q4.y, q4.z, q4.w};
            }
            floatx4 aq[NTD];
#pragma unroll
            for (int dt = 0; dt < NTD; ++dt) aq[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
            apply_tiles<HD, NL>(aq, pq, Ks, c, g);
            const int qi = 16 * w + c;
            if (qi < S) {
                float* row = d_qkv + (size_t)(qi * B + b) * ld3 + head * HD;
#pragma unroll
                for (int dt = 0; dt < NTD; ++dt) store4<HD>(row, 16 * dt + 4 * g, aq[dt], scale);
            }
        };
        if constexpr (CAUSAL_SKIP) tile_dispatch<NT>(w, dq);
        else dq(std::integral_constant<int, NT - 1>{});
        return;
    }
    if (SAVED) {
        // the same registers the Philox form fills: all-ones (kept) or zero (dropped: 0 < thr) — the rest of the kernel is
        // one code path (a separate bit-test path compiled to 82 VGPRs and ran SLOWER than the Philox calls at 640 problems)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const uint32_t nib = Wk[64 * t + lane] >> (4 * w);
#pragma unroll
            for (int r = 0; r < 4; ++r) wdt[t][r] = ((nib >> r) & 1u) ? 0xFFFFFFFFu : 0u;
        }
    }

    const int kj = 16 * w + c;                     // this lane's key
    floatx4 ps[NT], dp[NT];
    // initial accumulators: -LSE[query] for the scores (P = exp(acc) needs no subtraction), 0 for dP
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float4 l4 = *reinterpret_cast<const float4*>(Ls + 16 * t + 4 * g);
        ps[t] = floatx4{-l4.x, -l4.y, -l4.z, -l4.w};
        dp[t] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    dot_tiles<HD, NT>(ps, Qs, Ks + kj * LD + g, c, g);      // S[query 16t+4g+reg][key kj] - LSE
    dot_tiles<HD, NT>(dp, Os, Vs + kj * LD + g, c, g);      // dP~[query][key] = dO . V

    // a key past the dialogue's length has P = 0 (and with it dS = 0): its dK and dV rows are written as zeros
    const bool keyok = kj < n;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float4 d4 = *reinterpret_cast<const float4*>(Ds + 16 * t + 4 * g);
        const float dd[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pv = keyok ? __expf(ps[t][r]) : 0.f;             // probability (pre-dropout)
            const bool keep = !dc.on || wdt[t][r] >= dc.thr;
            const float dpk = keep ? dp[t][r] * dc.scale : 0.f;          // dP = keep * scale * dP~
            ps[t][r] = keep ? pv * dc.scale : 0.f;                       // P~
            dp[t][r] = pv * (dpk - dd[r]);                               // dS
        }
    }

    // dV^T[d][key] = sum_q dO[q][d] P~[q][key];  dK^T[d][key] = sum_q (scale Q)[q][d] dS[q][key]
    {
        floatx4 av[NTD], ak[NTD];
#pragma unroll
        for (int dt = 0; dt < NTD; ++dt) { av[dt] = floatx4{0.f, 0.f, 0.f, 0.f}; ak[dt] = floatx4{0.f, 0.f, 0.f, 0.f}; }
        const float* pv_ = Os + 4 * g * LD + c;
        const float* pk_ = Qs + 4 * g * LD + c;
        float a1[2][4][NTD], a2[2][4][NTD];
        auto fetch = [&](int t, float (&d1)[4][NTD], float (&d2)[4][NTD]) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int dt = 0; dt < NTD; ++dt) {
                    d1[r][dt] = pv_[(16 * t + r) * LD + 16 * dt];
                    d2[r][dt] = pk_[(16 * t + r) * LD + 16 * dt];
                }
        };
        fetch(0, a1[0], a2[0]);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t + 1 < NT) fetch(t + 1, a1[(t + 1) & 1], a2[(t + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int dt = 0; dt < NTD; ++dt) {
                    av[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[t & 1][r][dt], ps[t][r], av[dt], 0, 0, 0);
                    ak[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[t & 1][r][dt], dp[t][r], ak[dt], 0, 0, 0);
                }
        }
        if (kj < S) {
            float* row = d_qkv + (size_t)(kj * B + b) * ld3 + head * HD;
#pragma unroll
            for (int dt = 0; dt < NTD; ++dt) {
                store4<HD>(row + 2 * E, 16 * dt + 4 * g, av[dt], 1.f);
                store4<HD>(row + E, 16 * dt + 4 * g, ak[dt], 1.f);
            }
        }
    }
    // dS -> LDS [query][key], over the operands every wave has finished reading
    __syncthreads();
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) SS[(16 * t + 4 * g + r) * LDS_S + kj] = dp[t][r];
    __syncthreads();

    // dQ^T[d][query 16w + c] = scale * sum_key K[key][d] dS[query][key]
    {
        floatx4 pq[NT];
        const float* ss = SS + (16 * w + c) * LDS_S + 4 * g;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float4 q4 = *reinterpret_cast<const float4*>(ss + 16 * t);
            pq[t] = floatx4{q4.x, q4.y, q4.z, q4.w};
        }
        floatx4 aq[NTD];
#pragma unroll
        for (int dt = 0; dt < NTD; ++dt) aq[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
        apply_tiles<HD, NT>(aq, pq, Ks, c, g);
        const int qi = 16 * w + c;
        if (qi < S) {
            float* row = d_qkv + (size_t)(qi * B + b) * ld3 + head * HD;
#pragma unroll
            for (int dt = 0; dt < NTD; ++dt) store4<HD>(row, 16 * dt + 4 * g, aq[dt], scale);
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side: the launches for a call that attention.hip has checked (check_attn) and attn16_supported() accepts
// ------------------------------------------------------------------------------------------
// head_dim 10 / 30: always.  head_dim 60 / 64: short sequences only — measured against attention.hip (tools/lab/attn_big.py,
// B = 32): S = 33, hd 60: forward 17.1 -> 9.6 us, backward 30.4 -> 19.4 us; S = 94, hd 64: forward 17.2 -> 36.9 us
// (16 k-steps per score tile on 16-wide tiles), backward 34.1 -> 32.2 us.
#ifndef GANFFN_A16_CAUSAL_TU
bool attn16_supported(int E, int H, int S) {
    const int hd = H > 0 ? E / H : 0;
    if (!(H > 0 && E % H == 0)) return false;
    if (hd == 10 || hd == 30) return true;
    return (hd == 60 || hd == 64) && S <= 48;
}
#endif
// The CAUSAL instantiations live in a translation unit of their own: attention16_causal.hip is this file compiled with
// GANFFN_A16_CAUSAL_TU, which keeps the causal launches (attn16_fwd<true> / attn16_bwd<true>) and nothing else, and this
// file without it keeps everything else.  Measured, not a matter of taste: with both in one module 52 of the 176 kernels without
// the flag (the head_dim 10 backward among them) came out of hipcc with another schedule and register assignment than the
// parent's, although their source had not changed; apart, all 176 are the parent's instruction for instruction.
#ifdef GANFFN_A16_CAUSAL_TU
constexpr bool A16_CAUSAL = true;
#else
constexpr bool A16_CAUSAL = false;
#endif
// The LEN flag of this unit's kernels: f(LEN).  The causal instantiations are LEN ones (a null key_len reads as S in the kernel).
template <class F>
static int with_len(const AttnCall& k, F&& f) {
    if constexpr (A16_CAUSAL) return f(std::true_type{});
    else return with_flag(k.key_len != nullptr, f);
}

// Hand the dropout keep bits from the forward to the backward (instead of re-evaluating the Philox calls there) only while
// the launch leaves most CUs with ONE backward workgroup: measured (tools/lab/attn_ab.py, S = 94, head_dim 10, p = 0.1)
// 16.7 -> 15.2 us at 320 problems, but 24.0 -> 25.1 us at 640 — there the Philox calls run in the shadow of the staging
// loads, while unpacking the saved words sits behind the barrier on the critical path of co-resident workgroups.
static bool attn16_use_keep(int B, int H) { return (long)B * H <= 384; }

template <int HD>
static size_t fwd_lds(int nt) { return (size_t)3 * (16 * nt * A16<HD>::LD + A16<HD>::TAIL) * sizeof(float); }
template <int HD>
static size_t bwd_lds(int nt) {
    const size_t mat = (size_t)16 * nt * A16<HD>::LD + A16<HD>::TAIL, img = (size_t)16 * nt * (16 * nt + 4);
    return (mat + 2 * 16 * nt + 64 * nt + (img > 3 * mat ? img : 3 * mat)) * sizeof(float);
}

template <int HD, int NT>
static int launch16_fwd(const AttnCall& k) {
    const size_t lds = fwd_lds<HD>(NT);
    // the workgroup cut and the keep-word rule are those of ONE batch of B dialogues: what a single launch would choose
    const bool keep = attn16_use_keep(k.B, k.H);
    // query tiles per workgroup: measured at hd = 10, S = 94 (tools/lab/attn_wpb.py, lab build): 320 problems 11.1 us as
    // whole workgroups, 10.1 / 9.9 / 11.5 us cut in 2 / 3 / 6; 640 problems 15.0 us whole, 16.4 / 17.9 / 21.5 us cut —
    // the cut pays while the problems do not fill the chip, then the repeated K / V staging costs more than the balance gains
    constexpr bool CUTTABLE = NT % 2 == 0 && NT > 2;
    const bool cut = (long)k.B * k.H < 512 && CUTTABLE;
    auto launch = [&](auto wpb, auto pair, auto len) -> int {
        constexpr int WPB = decltype(wpb)::value;
        constexpr bool PAIR = decltype(pair)::value, LEN = decltype(len)::value;
        const AttnSeg &s0 = k.seg[0], &t1 = k.seg[1];      // without a second segment t1 is null / 0
        const Attn16Seg1 s1{t1.qkv, t1.o, t1.lse, keep ? t1.keep : nullptr, t1.train};
        const int nb0 = k.B * k.H * (NT / WPB);            // workgroups of one batch
        GF_TRY((lds_optin<attn16_fwd_kernel<HD, NT, WPB, PAIR, LEN, A16_CAUSAL>>(lds, "attention_fwd")));
        hipLaunchKernelGGL((attn16_fwd_kernel<HD, NT, WPB, PAIR, LEN, A16_CAUSAL>), dim3((PAIR ? 2 : 1) * nb0), dim3(64 * WPB), lds, k.st,
                           s0.qkv, s0.o, s0.lse, keep ? s0.keep : nullptr, k.S, k.B, k.E, k.H, k.p, k.site, k.rng, k.add, s0.train, s1,
                           PAIR ? nb0 : 0, k.key_len);
        GF_LAUNCH_CHECK();
        return 0;
    };
    return with_flag(k.nseg == 2, [&](auto pair) {
        return with_len(k, [&](auto len) {
            if constexpr (CUTTABLE)
                if (cut) return launch(std::integral_constant<int, 2>{}, pair, len);
            return launch(std::integral_constant<int, NT>{}, pair, len);
        });
    });
}
template <int HD, int NT>
static int launch16_bwd(const AttnCall& k) {
    const size_t lds = bwd_lds<HD>(NT);
    const bool saved = k.keep != nullptr && k.train && k.p > 0.f && attn16_use_keep(k.B, k.H);      // the forward of this pass stored its keep words
    return with_flag(saved, [&](auto sv) {
        return with_len(k, [&](auto len) -> int {
            constexpr bool SAVED = decltype(sv)::value, LEN = decltype(len)::value;
            GF_TRY((lds_optin<attn16_bwd_kernel<HD, NT, SAVED, LEN, A16_CAUSAL>>(lds, "attention_bwd")));
            hipLaunchKernelGGL((attn16_bwd_kernel<HD, NT, SAVED, LEN, A16_CAUSAL>), dim3(k.B * k.H), dim3(64 * NT), lds, k.st, k.qkv, k.o, k.lse,
                               k.d_o, k.keep, k.d_qkv, k.S, k.B, k.E, k.H, k.p, k.site, k.rng, k.add, k.train, k.key_len);
            GF_LAUNCH_CHECK();
            return 0;
        });
    });
}

#define NT16_SWITCH3(FN, HD, ...)                           \
    switch ((k.S + 15) / 16) {                              \
        case 1: return FN<HD, 1>(__VA_ARGS__);              \
        case 2: return FN<HD, 2>(__VA_ARGS__);              \
        default: return FN<HD, 3>(__VA_ARGS__);             \
    }
#define NT16_SWITCH(FN, HD, ...)                            \
    switch ((k.S + 15) / 16) {                              \
        case 1: return FN<HD, 1>(__VA_ARGS__);              \
        case 2: return FN<HD, 2>(__VA_ARGS__);              \
        case 3: return FN<HD, 3>(__VA_ARGS__);              \
        case 4: return FN<HD, 4>(__VA_ARGS__);              \
        case 5: return FN<HD, 5>(__VA_ARGS__);              \
        case 6: return FN<HD, 6>(__VA_ARGS__);              \
        default: return FN<HD, 7>(__VA_ARGS__);             \
    }

template <bool CAUSAL>
int attn16_fwd(const AttnCall& k) {
    static_assert(CAUSAL == A16_CAUSAL, "each unit launches its own kernels only");
    if (k.E / k.H == 64) { NT16_SWITCH3(launch16_fwd, 64, k) }
    if (k.E / k.H == 60) { NT16_SWITCH3(launch16_fwd, 60, k) }
    if (k.E / k.H == 10) { NT16_SWITCH(launch16_fwd, 10, k) }
    NT16_SWITCH(launch16_fwd, 30, k)
}
template <bool CAUSAL>
int attn16_bwd(const AttnCall& k) {
    static_assert(CAUSAL == A16_CAUSAL, "each unit launches its own kernels only");
    if (k.E / k.H == 64) { NT16_SWITCH3(launch16_bwd, 64, k) }
    if (k.E / k.H == 60) { NT16_SWITCH3(launch16_bwd, 60, k) }
    if (k.E / k.H == 10) { NT16_SWITCH(launch16_bwd, 10, k) }
    NT16_SWITCH(launch16_bwd, 30, k)
}
template int attn16_fwd<A16_CAUSAL>(const AttnCall& k);
template int attn16_bwd<A16_CAUSAL>(const AttnCall& k);

}  // namespace ganffn
