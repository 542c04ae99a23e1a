// stream.hip — the streaming (one new utterance per dialogue) form of causal self-attention: per-layer K/V caches and a
// single-query attention step, and the positional-encoding gather by per-dialogue position that heads a streamed stack
// (ganffn_encoder_stream_step in api.hip; ganffn_stream_attention is the kernel alone).  Below them the chunk forms of both, for
// several new utterances per dialogue in one call (ganffn_encoder_stream_extend, ganffn_stream_attention_chunk).
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

// ---------------------------------------------------------------------------------------------------------------------------
// The chunk form (stream prefill): chunk i of a launch holds c = count[i] new rows of slot s = slot[i] at positions t .. t+c-1,
// t = pos[s]; qkv is [m][n][3E] and o [m][n][E], time-major.  Row j < c attends over the cached keys 0 .. t-1 and the chunk's own
// keys 0 .. j — what j + 1 consecutive launches of the kernel above compute — and the K / V head slices of rows 0 .. c-1 go to
// the cache at t .. t+c-1 as bit copies of the qkv words.
// One workgroup (sixteen waves) per (head, chunk, query split).  It reads the K and V of its (slot, head) from global memory ONCE —
// rows 0 .. t-1 from the cache, rows t .. t+c-1 from qkv, never from the cache: no address written in a launch is read in it —
// into LDS, [t + c][hd + 1] floats each.  The odd row stride hd + 1 is what the two access patterns below want: in the scores a
// lane owns a key and walks d, so the lanes read one column of consecutive rows; a 4-byte LDS read banks each 32-lane half over
// 32 dwords, so an odd stride gives 32 distinct banks (the plain strides 10, 30, 60, 64 would be 2-, 2-, 4- and 32-way
// conflicts); in P V a lane group reads hd consecutive floats of one row.  Split 0 also writes the cache and the zero rows.  Then wave w of split z takes the query pairs 2 ((r * nsplit + z) * 16 + w)
// and + 1, r = 0, 1, ...: interleaved, because under the causal rule query j costs t + j + 1 keys, and two at a time, so that one
// K / V read from LDS serves both and their dependent chains overlap.  Per query: q[d] is wave-uniform and
// comes through scalar loads, lanes over keys for the scores (two keys per lane, the second half only when there are more than
// 64 keys), wave shuffles for maximum and sum, p to the wave's 2 x 128 floats of LDS, then lanes over (key group, d) for P V: 64 / hd
// groups, group g takes the key blocks g, g + G, ... of 4 consecutive keys, p as one 16-byte broadcast read per block, and the
// groups' partial sums are added in group order.  Plain vector ALU, no MFMA: profiles/stream_extend_ab.txt has the times beside the
// full-sequence MFMA kernel's.  Every order is fixed by (t, j, hd) alone, no wave looks at another chunk's data and which
// workgroup or wave takes a query changes no operation of it: the bits of a chunk's rows depend neither on the other chunks of
// the launch nor on the chunk's column.  No atomics.
// Skip rule: s outside [0, capacity), t < 0, c < 0, c > m or t + c > max_len skips the chunk whole (cache untouched); o rows
// j >= c (all m of a skipped chunk) are written as zeros, qkv rows j >= c and cache words at or above t are never read.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int CHUNK_WAVES = 16;             // waves of a workgroup: they share the K / V in LDS and hide each other's latencies
constexpr int CHUNK_PBUF = 128;              // p of one query: max_len <= 110 keys, zero-filled up to the P V loop's bound

template <int HD>
__global__ __launch_bounds__(64 * CHUNK_WAVES) void stream_attention_chunk_kernel(
    const float* __restrict__ qkv, float* __restrict__ cache, const int32_t* __restrict__ slot, const int32_t* __restrict__ count,
    const int32_t* __restrict__ pos, float* __restrict__ o, int n, int m, int capacity, int max_len, int E, int H, int hd_rt,
    float scale) {
    extern __shared__ __attribute__((aligned(16))) float chunk_lds[];
    const int hd = HD ? HD : hd_rt;
    const int ldk = hd + 1;
    const int h = blockIdx.x, i = blockIdx.y, z = blockIdx.z, nsplit = gridDim.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s = slot[i];
    int c = count[i];
    int t = -1;
    if (s >= 0 && s < capacity) t = pos[s];
    if (t < 0 || c < 0 || c > m || t > max_len - c) c = 0;      // skipped chunk (workgroup-uniform): zeros, nothing else
    const size_t row3 = (size_t)n * 3 * E, rowo = (size_t)n * E;             // time-major: row j of chunk i is row j * n + i
    const float* const qbase = qkv + (size_t)i * 3 * E + h * hd;
    float* const obase = o + (size_t)i * E + h * hd;
    if (z == 0) {                            // o rows c .. m-1 of this head: exact zeros
        for (int idx = tid; idx < (m - c) * hd; idx += 64 * CHUNK_WAVES) {
            const int j = c + idx / hd, d = idx - (idx / hd) * hd;
            obase[(size_t)j * rowo + d] = 0.f;
        }
    }
    if (c == 0) return;
    const int nk = t + c;                    // 1 .. max_len
    float* const Ks = chunk_lds;
    float* const Vs = Ks + (size_t)max_len * ldk;
    float* const Ps = Ks + ((2 * max_len * ldk + 3) & ~3) + wave * 2 * CHUNK_PBUF;   // (16-byte aligned; two queries' p)
    float* const kc = cache + ((size_t)(s * 2) * H + h) * max_len * hd;
    float* const vc = cache + ((size_t)(s * 2 + 1) * H + h) * max_len * hd;
    // the (slot, head)'s K and V, once: float2 words (hd is even, every base is 8-byte aligned)
    const int hw = hd >> 1;
    for (int idx = tid; idx < nk * hw; idx += 64 * CHUNK_WAVES) {
        const int j = idx / hw, d = (idx - j * hw) * 2;
        float2 k2, v2;
        if (j < t) {
            k2 = *reinterpret_cast<const float2*>(kc + (size_t)j * hd + d);
            v2 = *reinterpret_cast<const float2*>(vc + (size_t)j * hd + d);
        } else {
            const float* r = qbase + (size_t)(j - t) * row3 + d;
            k2 = *reinterpret_cast<const float2*>(r + E);
            v2 = *reinterpret_cast<const float2*>(r + 2 * E);
            if (z == 0) {                    // append: bit copies
                *reinterpret_cast<float2*>(kc + (size_t)j * hd + d) = k2;
                *reinterpret_cast<float2*>(vc + (size_t)j * hd + d) = v2;
            }
        }
        Ks[j * ldk + d] = k2.x;
        Ks[j * ldk + d + 1] = k2.y;
        Vs[j * ldk + d] = v2.x;
        Vs[j * ldk + d + 1] = v2.y;
    }
    __syncthreads();

    const int G = 64 / hd;
    const int g = lane / hd, dd = lane - g * hd;
    const bool ingrp = g < G;
    // two consecutive queries ja, ja + 1 per pass: one K / V read from LDS serves both, and their two dependent chains (scalar
    // loads, shuffles, LDS round trips) overlap.  An odd last query runs as its own partner and is stored once.
    for (int ja = 2 * (z * CHUNK_WAVES + wave); ja < c; ja += 2 * nsplit * CHUNK_WAVES) {       // (wave-uniform)
        const bool two = ja + 1 < c;
        const int jb = two ? ja + 1 : ja;
        const int nka = t + ja + 1, nkb = t + jb + 1;          // the queries' keys: nka <= nkb <= nk
        const float* __restrict__ const qa = qbase + (size_t)ja * row3;           // wave-uniform addresses: scalar loads
        const float* __restrict__ const qb = qbase + (size_t)jb * row3;
        // scores: key lane and key lane + 64
        const int k0 = lane < nkb ? lane : 0, k1 = lane + 64 < nkb ? lane + 64 : 0;
        float a0 = 0.f, a1 = 0.f, b0 = 0.f, b1 = 0.f;
        if (nkb > 64) {
            if constexpr (HD != 0) {
#pragma unroll
                for (int d = 0; d < HD; ++d) {
                    const float x0 = Ks[k0 * ldk + d], x1 = Ks[k1 * ldk + d];
                    a0 = fmaf(qa[d], x0, a0);
                    a1 = fmaf(qa[d], x1, a1);
                    b0 = fmaf(qb[d], x0, b0);
                    b1 = fmaf(qb[d], x1, b1);
                }
            } else {
                for (int d = 0; d < hd; ++d) {
                    const float x0 = Ks[k0 * ldk + d], x1 = Ks[k1 * ldk + d];
                    a0 = fmaf(qa[d], x0, a0);
                    a1 = fmaf(qa[d], x1, a1);
                    b0 = fmaf(qb[d], x0, b0);
                    b1 = fmaf(qb[d], x1, b1);
                }
            }
        } else {
            if constexpr (HD != 0) {
#pragma unroll
                for (int d = 0; d < HD; ++d) {
                    const float x0 = Ks[k0 * ldk + d];
                    a0 = fmaf(qa[d], x0, a0);
                    b0 = fmaf(qb[d], x0, b0);
                }
            } else {
                for (int d = 0; d < hd; ++d) {
                    const float x0 = Ks[k0 * ldk + d];
                    a0 = fmaf(qa[d], x0, a0);
                    b0 = fmaf(qb[d], x0, b0);
                }
            }
        }
        // softmax over each query's keys (key 0 is always live: the maxima are finite); query a does not see key nka
        const float sa0 = lane < nka ? a0 * scale : -INFINITY, sa1 = lane + 64 < nka ? a1 * scale : -INFINITY;
        const float sb0 = lane < nkb ? b0 * scale : -INFINITY, sb1 = lane + 64 < nkb ? b1 * scale : -INFINITY;
        const float ma = wave_max(fmaxf(sa0, sa1)), mb = wave_max(fmaxf(sb0, sb1));
        const float pa0 = lane < nka ? expf(sa0 - ma) : 0.f, pa1 = lane + 64 < nka ? expf(sa1 - ma) : 0.f;
        const float pb0 = lane < nkb ? expf(sb0 - mb) : 0.f, pb1 = lane + 64 < nkb ? expf(sb1 - mb) : 0.f;
        const float inva = 1.0f / wave_sum(pa0 + pa1), invb = 1.0f / wave_sum(pb0 + pb1);
        Ps[lane] = pa0;
        Ps[lane + 64] = pa1;
        Ps[CHUNK_PBUF + lane] = pb0;
        Ps[CHUNK_PBUF + lane + 64] = pb1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // P V: lane (g, dd) takes the key blocks g, g + G, ... (4 keys each) and accumulates p_j V[j][dd] for both queries
        float acca = 0.f, accb = 0.f;
        if (ingrp) {
#pragma unroll 2
            for (int kb = g; kb * 4 < nkb; kb += G) {
                const float4 pa4 = *reinterpret_cast<const float4*>(Ps + kb * 4);
                const float4 pb4 = *reinterpret_cast<const float4*>(Ps + CHUNK_PBUF + kb * 4);
                const int j0 = kb * 4;
                // (a key at or past nkb has p = 0 and is given the V row of query b's own key nkb - 1 instead of its own, which may be
                // a later row of the chunk or lie past what this workgroup loaded; query a takes a zero for key nka, query b's row)
                const float v0 = Vs[j0 * ldk + dd];
                const float v1 = Vs[min(j0 + 1, nkb - 1) * ldk + dd];
                const float v2 = Vs[min(j0 + 2, nkb - 1) * ldk + dd];
                const float v3 = Vs[min(j0 + 3, nkb - 1) * ldk + dd];
                accb = fmaf(pb4.x, v0, accb);
                accb = fmaf(pb4.y, v1, accb);
                accb = fmaf(pb4.z, v2, accb);
                accb = fmaf(pb4.w, v3, accb);
                acca = fmaf(pa4.x, j0 < nka ? v0 : 0.f, acca);
                acca = fmaf(pa4.y, j0 + 1 < nka ? v1 : 0.f, acca);
                acca = fmaf(pa4.z, j0 + 2 < nka ? v2 : 0.f, acca);
                acca = fmaf(pa4.w, j0 + 3 < nka ? v3 : 0.f, acca);
            }
        }
        // the groups' partial sums, in group order
        float tota = 0.f, totb = 0.f;
        for (int gg = 0; gg < G; ++gg) {
            tota += __shfl(acca, gg * hd + dd, 64);
            totb += __shfl(accb, gg * hd + dd, 64);
        }
        if (lane < hd) {
            obase[(size_t)ja * rowo + lane] = tota * inva;
            if (two) obase[(size_t)jb * rowo + lane] = totb * invb;
        }
        // (the next pass's p must not land before this pass's reads: LDS operations of a wave complete in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// x0[j, i] = x[j, i] + pe[pos[slot[i]] + j] for the rows j < count[i] of a chunk that is not skipped; every other row is zeros
__global__ __launch_bounds__(128) void stream_pe_chunk_kernel(const float* __restrict__ x, const float* __restrict__ pe,
                                                              const int32_t* __restrict__ slot, const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ pos, float* __restrict__ x0, int n, int m,
                                                              int capacity, int max_len, int E) {
    const int i = blockIdx.x, j = blockIdx.y;
    const int s = slot[i];
    int c = count[i];
    int t = -1;
    if (s >= 0 && s < capacity) t = pos[s];
    if (t < 0 || c < 0 || c > m || t > max_len - c) c = 0;
    const bool live = j < c;
    const size_t row = (size_t)j * n + i;
    const float4* x4 = reinterpret_cast<const float4*>(x + row * E);
    const float4* p4 = reinterpret_cast<const float4*>(pe + (size_t)(live ? t + j : 0) * E);
    float4* o4 = reinterpret_cast<float4*>(x0 + row * E);
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

int launch_stream_attention_chunk(const float* qkv, float* cache_layer, const int32_t* slot, const int32_t* count,
                                  const int32_t* pos, float* o, int n, int m, int capacity, int max_len, int E, int H,
                                  hipStream_t st) {
    GF_CHECK_ARG(qkv && cache_layer && slot && count && pos && o, "stream_attention_chunk: null pointer");
    GF_CHECK_ARG(n >= 1 && capacity >= 1 && capacity <= GANFFN_MAX_DIALOGUES && n <= capacity,
                 "stream_attention_chunk: n=%d capacity=%d (1 <= n <= capacity <= %d)", n, capacity, GANFFN_MAX_DIALOGUES);
    GF_CHECK_ARG(max_len >= 1 && max_len <= 110, "stream_attention_chunk: max_len=%d out of range [1,110]", max_len);
    GF_CHECK_ARG(m >= 1 && m <= max_len, "stream_attention_chunk: m=%d out of range [1,max_len=%d]", m, max_len);
    GF_CHECK_ARG(E >= 4 && (E & 3) == 0 && E <= 640 && H >= 1 && E % H == 0, "stream_attention_chunk: E=%d H=%d", E, H);
    const int hd = E / H;
    GF_CHECK_ARG((hd & 1) == 0 && hd <= 64, "stream_attention_chunk: head_dim %d must be even and <= 64", hd);
    GF_CHECK_ARG(aligned16(qkv) && aligned16(cache_layer) && aligned16(o), "stream_attention_chunk: buffers must be 16-byte aligned");
    const float scale = 1.0f / sqrtf((float)hd);
    // K and V of one (slot, head) at row stride hd + 1, and two p buffers per wave (16-byte aligned: both terms are multiples of 4)
    const size_t lds = ((size_t)((2 * max_len * (hd + 1) + 3) & ~3) + CHUNK_WAVES * 2 * CHUNK_PBUF) * sizeof(float);
    // few chunks: split a chunk's queries over up to 4 workgroups (each reads the K / V again; split 0 writes the cache)
    int nsplit = 256 / (n * H);
    nsplit = nsplit < 1 ? 1 : (nsplit > 4 ? 4 : nsplit);
    if (nsplit > (m + 2 * CHUNK_WAVES - 1) / (2 * CHUNK_WAVES)) nsplit = (m + 2 * CHUNK_WAVES - 1) / (2 * CHUNK_WAVES);
    const dim3 grid(H, n, nsplit), block(64 * CHUNK_WAVES);
#define GF_CHUNK_LAUNCH(HD_)                                                                                                     \
    do {                                                                                                                         \
        GF_TRY(lds_optin<stream_attention_chunk_kernel<HD_>>(lds, "stream_attention_chunk"));                                    \
        hipLaunchKernelGGL(stream_attention_chunk_kernel<HD_>, grid, block, lds, st, qkv, cache_layer, slot, count, pos, o, n, m, \
                           capacity, max_len, E, H, hd, scale);                                                                  \
    } while (0)
    switch (hd) {
        case 10: GF_CHUNK_LAUNCH(10); break;
        case 30: GF_CHUNK_LAUNCH(30); break;
        case 60: GF_CHUNK_LAUNCH(60); break;
        case 64: GF_CHUNK_LAUNCH(64); break;
        default: GF_CHUNK_LAUNCH(0); break;
    }
#undef GF_CHUNK_LAUNCH
    GF_LAUNCH_CHECK();
    return 0;
}

int launch_stream_pe_chunk(const float* x, const float* pe, const int32_t* slot, const int32_t* count, const int32_t* pos,
                           float* x0, int n, int m, int capacity, int max_len, int E, hipStream_t st) {
    GF_CHECK_ARG(x && pe && slot && count && pos && x0, "stream_pe_chunk: null pointer");
    GF_CHECK_ARG(n >= 1 && m >= 1 && m <= max_len && capacity >= 1 && max_len >= 1 && E >= 4 && (E & 3) == 0,
                 "stream_pe_chunk: n=%d m=%d capacity=%d max_len=%d E=%d", n, m, capacity, max_len, E);
    GF_CHECK_ARG(aligned16(x) && aligned16(pe) && aligned16(x0), "stream_pe_chunk: buffers must be 16-byte aligned");
    hipLaunchKernelGGL(stream_pe_chunk_kernel, dim3(n, m), dim3(128), 0, st, x, pe, slot, count, pos, x0, n, m, capacity, max_len, E);
    GF_LAUNCH_CHECK();
    return 0;
}

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
