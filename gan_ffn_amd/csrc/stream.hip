// stream.hip — the streaming (one new utterance per dialogue) form of causal self-attention: per-layer K/V caches and a
// single-query attention step, and the positional-encoding gather by per-dialogue position that heads a streamed stack
// (ganffn_encoder_stream_step in api.hip; ganffn_stream_attention is the kernel alone).
//
// Cache layout of ONE layer (include/ganffn.h states the same): [capacity][2 (K, V)][H][max_len][hd] floats, hd = E / H — the
// key (value) of slot s, head h, position j is the hd contiguous floats at (((s * 2 + kv) * H + h) * max_len + j) * hd.
//
// stream_attention_kernel, per (row i, head h), s = slot[i], t = pos[s]: writes the row's K and V head slices into the cache at
// position t, attends with the row's Q over the cached keys 0 .. t-1 and the new key, scale 1 / sqrt(hd), softmax, P V, and
// writes o[i] in the layout the out-proj reads.  The new key and value come from the qkv row itself: no address written in a
// launch is read in it.  This is a decode step: bound by the K/V read and by latency, so plain vector ALU, no MFMA.  One wave per
// (row, head), four per workgroup: lanes over keys for the scores (at most two keys per lane: max_len <= 128), wave shuffles for
// the maximum and the sum, then lanes over (key group, d) for P V — 64 / hd groups take every (64 / hd)-th key each, with V rows
// read as consecutive floats, 8 loads in flight per lane (one at a time, a head_dim 64 problem at position 109 is 110 dependent
// round trips: profiles/stream_step_ab.txt), and the groups' partial sums are added in group order.  Every order is fixed and no lane of a wave
// looks at another wave's data: the bits of a row do not depend on the other rows of the launch.  No atomics, no dropout.
// A row whose slot is outside [0, capacity) or whose position is outside [0, max_len) is skipped: its o row is zeros and the
// cache is untouched; nothing is read or written out of range whatever slot / pos hold.  pos is read only.
// Slots of one launch must be distinct (two rows of one slot would write the same cache position).
#include "common.h"

namespace ganffn {

namespace {

constexpr int STREAM_WAVES = 4;

// HD: compile-time head_dim (10, 30, 60, 64) or 0 = the run-time value hd_rt (even, <= 64)
template <int HD>
__global__ __launch_bounds__(64 * STREAM_WAVES) void stream_attention_kernel(const float* __restrict__ qkv, float* __restrict__ cache,
                                                                              const int32_t* __restrict__ slot,
                                                                              const int32_t* __restrict__ pos, float* __restrict__ o,
                                                                              int n, int capacity, int max_len, int E, int H, int hd_rt,
                                                                              float scale) {
    const int hd = HD ? HD : hd_rt;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(blockIdx.x * STREAM_WAVES + (threadIdx.x >> 6));   // (row, head) problem
    if (w >= n * H) return;
    const int i = w / H, h = w - i * H;
    float* const orow = o + (size_t)i * E + h * hd;
    const int s = slot[i];
    int t = -1;
    if (s >= 0 && s < capacity) t = pos[s];
    if (t < 0 || t >= max_len) {             // (wave-uniform) skipped row: zeros, the cache is not touched
        if (lane < hd) orow[lane] = 0.f;
        return;
    }
    const float* const qrow = qkv + (size_t)i * 3 * E + h * hd;
    const float* const knew = qrow + E;
    const float* const vnew = qrow + 2 * E;
    float* const kc = cache + ((size_t)(s * 2) * H + h) * max_len * hd;            // [max_len][hd] keys of (s, h)
    float* const vc = cache + ((size_t)(s * 2 + 1) * H + h) * max_len * hd;        // [max_len][hd] values
    const int nk = t + 1;                    // keys 0 .. t-1 from the cache, key t from the row

    // lane d holds q[d]; the score loops read it lane by lane
    const float qv = lane < hd ? qrow[lane] : 0.f;
    // append (the new K / V are taken from the row below, never from here)
    if (lane < hd) {
        kc[(size_t)t * hd + lane] = knew[lane];
        vc[(size_t)t * hd + lane] = vnew[lane];
    }

    // scores: key j = lane and j = lane + 64
    float sc[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int j = lane + 64 * r;
        const bool live = j < nk;
        const float* kp = (j == t) ? knew : kc + (size_t)(live ? j : 0) * hd;
        float acc = 0.f;
        if constexpr (HD != 0 && HD % 4 == 0) {
#pragma unroll
            for (int d = 0; d < HD; d += 4) {
                float4 k4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (live) k4 = *reinterpret_cast<const float4*>(kp + d);
                acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), d + 0)), k4.x, acc);
                acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), d + 1)), k4.y, acc);
                acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), d + 2)), k4.z, acc);
                acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), d + 3)), k4.w, acc);
            }
        } else if constexpr (HD != 0) {
#pragma unroll
            for (int d = 0; d < HD; d += 2) {
                float2 k2 = make_float2(0.f, 0.f);
                if (live) k2 = *reinterpret_cast<const float2*>(kp + d);
                acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), d + 0)), k2.x, acc);
                acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), d + 1)), k2.y, acc);
            }
        } else {
            for (int d = 0; d < hd; d += 2) {
                float2 k2 = make_float2(0.f, 0.f);
                if (live) k2 = *reinterpret_cast<const float2*>(kp + d);
                acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), d + 0)), k2.x, acc);
                acc = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(qv), d + 1)), k2.y, acc);
            }
        }
        sc[r] = live ? acc * scale : -INFINITY;
    }
    // softmax over the nk keys (key 0 is always live: the maximum is finite)
    const float m = wave_max(fmaxf(sc[0], sc[1]));
    const float p0 = (lane < nk) ? expf(sc[0] - m) : 0.f;
    const float p1 = (lane + 64 < nk) ? expf(sc[1] - m) : 0.f;
    const float inv = 1.0f / wave_sum(p0 + p1);

    // P V: group g of hd lanes takes keys g, g + G, ...; lane (g, d) accumulates p_j V[j][d]
    const int G = 64 / hd;
    const int g = lane / hd, d = lane - g * hd;
    const bool ingrp = g < G;
    float acc = 0.f;
    constexpr int PV_BATCH = 8;              // V loads in flight per lane: the loop is latency-bound, not bandwidth-bound
    for (int j0 = 0; j0 < nk; j0 += PV_BATCH * G) {     // (uniform bound: every lane takes part in the shuffles)
        float vv[PV_BATCH];
#pragma unroll
        for (int u = 0; u < PV_BATCH; ++u) {
            const int j = j0 + u * G + g;
            const float* vp = (j == t) ? vnew : vc + (size_t)j * hd;
            vv[u] = (ingrp && j < nk) ? vp[d] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PV_BATCH; ++u) {
            const int j = j0 + u * G + g;
            const float pa = __shfl(p0, j & 63, 64);
            const float pb = __shfl(p1, j & 63, 64);
            const float pj = (ingrp && j < nk) ? (j < 64 ? pa : pb) : 0.f;      // (p is 0 at and past nk, V is not read there)
            acc = fmaf(pj, vv[u], acc);
        }
    }
    // the groups' partial sums, in group order
    float tot = 0.f;
    for (int gg = 0; gg < G; ++gg) tot += __shfl(acc, gg * hd + d, 64);
    if (lane < hd) orow[lane] = tot * inv;
}

// x0[i] = x[i] + pe[pos[slot[i]]] (eval mode: no dropout); a skipped row gives a zero row
__global__ __launch_bounds__(256) void stream_pe_kernel(const float* __restrict__ x, const float* __restrict__ pe,
                                                        const int32_t* __restrict__ slot, const int32_t* __restrict__ pos,
                                                        float* __restrict__ x0, int capacity, int max_len, int E) {
    const int i = blockIdx.x;
    const int s = slot[i];
    int t = -1;
    if (s >= 0 && s < capacity) t = pos[s];
    const bool live = t >= 0 && t < max_len;
    const float4* x4 = reinterpret_cast<const float4*>(x + (size_t)i * E);
    const float4* p4 = reinterpret_cast<const float4*>(pe + (size_t)(live ? t : 0) * E);
    float4* o4 = reinterpret_cast<float4*>(x0 + (size_t)i * E);
    for (int e = threadIdx.x; e < (E >> 2); e += blockDim.x) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            const float4 a = x4[e], b = p4[e];
            v = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
        o4[e] = v;
    }
}

}  // namespace

int launch_stream_attention(const float* qkv, float* cache_layer, const int32_t* slot, const int32_t* pos, float* o, int n,
                            int capacity, int max_len, int E, int H, hipStream_t st) {
    GF_CHECK_ARG(qkv && cache_layer && slot && pos && o, "stream_attention: null pointer");
    GF_CHECK_ARG(n >= 1 && capacity >= 1 && capacity <= GANFFN_MAX_DIALOGUES && n <= capacity,
                 "stream_attention: n=%d capacity=%d (1 <= n <= capacity <= %d)", n, capacity, GANFFN_MAX_DIALOGUES);
    GF_CHECK_ARG(max_len >= 1 && max_len <= 110, "stream_attention: max_len=%d out of range [1,110]", max_len);
    GF_CHECK_ARG(E >= 4 && (E & 3) == 0 && E <= 640 && H >= 1 && E % H == 0, "stream_attention: E=%d H=%d", E, H);
    const int hd = E / H;
    GF_CHECK_ARG((hd & 1) == 0 && hd <= 64, "stream_attention: head_dim %d must be even and <= 64", hd);
    GF_CHECK_ARG(aligned16(qkv) && aligned16(cache_layer) && aligned16(o), "stream_attention: buffers must be 16-byte aligned");
    const float scale = 1.0f / sqrtf((float)hd);
    const dim3 grid((n * H + STREAM_WAVES - 1) / STREAM_WAVES), block(64 * STREAM_WAVES);
#define GF_STREAM_LAUNCH(HD_)                                                                                                    \
    hipLaunchKernelGGL(stream_attention_kernel<HD_>, grid, block, 0, st, qkv, cache_layer, slot, pos, o, n, capacity, max_len, E, H, \
                       hd, scale)
    switch (hd) {
        case 10: GF_STREAM_LAUNCH(10); break;
        case 30: GF_STREAM_LAUNCH(30); break;
        case 60: GF_STREAM_LAUNCH(60); break;
        case 64: GF_STREAM_LAUNCH(64); break;
        default: GF_STREAM_LAUNCH(0); break;
    }
#undef GF_STREAM_LAUNCH
    GF_LAUNCH_CHECK();
    return 0;
}

int launch_stream_pe(const float* x, const float* pe, const int32_t* slot, const int32_t* pos, float* x0, int n, int capacity,
                     int max_len, int E, hipStream_t st) {
    GF_CHECK_ARG(x && pe && slot && pos && x0, "stream_pe: null pointer");
    GF_CHECK_ARG(n >= 1 && capacity >= 1 && max_len >= 1 && E >= 4 && (E & 3) == 0, "stream_pe: n=%d capacity=%d max_len=%d E=%d", n,
                 capacity, max_len, E);
    GF_CHECK_ARG(aligned16(x) && aligned16(pe) && aligned16(x0), "stream_pe: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(stream_pe_kernel, dim3(n), dim3(256), 0, st, x, pe, slot, pos, x0, capacity, max_len, E);
    GF_LAUNCH_CHECK();
    return 0;
}

}  // namespace ganffn
