// meld_head.hip — the head of the MELD classifier (MELDLSTMModel.forward, /root/reference/model.py:553-560, the att2 branch
// train_MELD.py:71 runs) behind the LSTM stack and the matching attention, as ONE launch forward and ONE launch backward for
// the step runner (engine.MeldEngine):
//     u = emotions + hardswish(att);   hidden = hardswish(u);   logits = hidden W_fc^T + b_fc          (C <= 16 classes)
// and from dlogits: d_hidden = dlogits W_fc, d_u = d_hidden hsw'(u), d_emotions = d_u, d_att = d_u hsw'(att) (u recomputed from
// emotions and att: nothing but `hidden` is kept, for the weight gradient), plus the smax_fc weight and bias gradients.
// A bandwidth-sized kernel (T D floats per tensor, a few FLOPs each): what it saves is launches — five elementwise / BLAS
// launches forward and autograd's mirror of them backward.  The C x D weight block sits in LDS (16.8 KB at 7 x 600), a token row
// is one wave's work, float4 along D, the class sums are butterfly reductions in a fixed order.  No atomics: every output
// element has one writer, the weight gradient adds 16 token-group sums in group order (small_linear_dw_kernel's scheme,
// elementwise.hip).
#include "common.h"

namespace ganffn {

namespace {

constexpr int MELD_MAX_C = 16;

// torch's hardswish and its derivative (0 for x <= -3, 1 for x >= 3, x / 3 + 0.5 strictly between)
__device__ __forceinline__ float hsw_f(float x) { return x * fminf(fmaxf(x + 3.f, 0.f), 6.f) * (1.f / 6.f); }
__device__ __forceinline__ float hsw_grad_f(float x) { return x <= -3.f ? 0.f : x >= 3.f ? 1.f : x * (1.f / 3.f) + 0.5f; }

__device__ __forceinline__ float4 hsw4(const float4 v) { return make_float4(hsw_f(v.x), hsw_f(v.y), hsw_f(v.z), hsw_f(v.w)); }
__device__ __forceinline__ float4 hsw_grad4(const float4 v) {
    return make_float4(hsw_grad_f(v.x), hsw_grad_f(v.y), hsw_grad_f(v.z), hsw_grad_f(v.w));
}

// the weight block [C x D] into LDS, float4 at a time, by the whole workgroup
__device__ __forceinline__ void load_w_lds(const float* __restrict__ w, float4* __restrict__ w_s, int n4) {
    for (int i = threadIdx.x; i < n4; i += blockDim.x) w_s[i] = reinterpret_cast<const float4*>(w)[i];
    __syncthreads();
}

// one wave per token row; rows t = blockIdx.x * waves + wave, strided by the grid
__global__ __launch_bounds__(256) void meld_head_fwd_kernel(const float* __restrict__ e, const float* __restrict__ att,
                                                            const float* __restrict__ w, const float* __restrict__ b,
                                                            float* __restrict__ hidden, float* __restrict__ logits, int T, int D4, int C) {
    extern __shared__ float4 w_s[];
    load_w_lds(w, w_s, C * D4);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (int t = blockIdx.x * waves + wave; t < T; t += gridDim.x * waves) {
        const float4* e4 = reinterpret_cast<const float4*>(e) + (size_t)t * D4;
        const float4* a4 = reinterpret_cast<const float4*>(att) + (size_t)t * D4;
        float4* h4 = reinterpret_cast<float4*>(hidden) + (size_t)t * D4;
        float acc[MELD_MAX_C];
#pragma unroll
        for (int c = 0; c < MELD_MAX_C; ++c) acc[c] = 0.f;
        for (int d = lane; d < D4; d += 64) {
            const float4 ev = e4[d], av = hsw4(a4[d]);
            const float4 h = hsw4(make_float4(ev.x + av.x, ev.y + av.y, ev.z + av.z, ev.w + av.w));
            h4[d] = h;
#pragma unroll
            for (int c = 0; c < MELD_MAX_C; ++c) {
                if (c < C) {
                    const float4 wv = w_s[c * D4 + d];
                    acc[c] += (h.x * wv.x + h.y * wv.y) + (h.z * wv.z + h.w * wv.w);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < MELD_MAX_C; ++c) {
            if (c < C) {
                const float s = wave_sum(acc[c]);
                if (lane == 0) logits[(size_t)t * C + c] = s + b[c];
            }
        }
    }
}

// blocks [0, n_dx): the data gradients, one wave per token row (16 rows per block pass, strided by n_dx);
// blocks [n_dx, n_dx + C * ceil(D / 64)): gw[c, 64 columns] and gb[c], 16 token groups x 64 columns, group sums added in order
__global__ __launch_bounds__(1024) void meld_head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ e,
                                                             const float* __restrict__ att, const float* __restrict__ hidden,
                                                             const float* __restrict__ w, float* __restrict__ d_e, float* __restrict__ d_att,
                                                             float* __restrict__ gw, float* __restrict__ gb, int T, int D4, int C, int n_dx) {
    extern __shared__ float4 w_s[];
    if ((int)blockIdx.x < n_dx) {
        load_w_lds(w, w_s, C * D4);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int t = blockIdx.x * 16 + wave; t < T; t += n_dx * 16) {
            float dl[MELD_MAX_C];
#pragma unroll
            for (int c = 0; c < MELD_MAX_C; ++c) dl[c] = c < C ? dlogits[(size_t)t * C + c] : 0.f;
            const float4* e4 = reinterpret_cast<const float4*>(e) + (size_t)t * D4;
            const float4* a4 = reinterpret_cast<const float4*>(att) + (size_t)t * D4;
            float4* de4 = reinterpret_cast<float4*>(d_e) + (size_t)t * D4;
            float4* da4 = reinterpret_cast<float4*>(d_att) + (size_t)t * D4;
            for (int d = lane; d < D4; d += 64) {
                float4 dh = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int c = 0; c < MELD_MAX_C; ++c) {
                    if (c < C) {
                        const float4 wv = w_s[c * D4 + d];
                        dh.x += dl[c] * wv.x; dh.y += dl[c] * wv.y; dh.z += dl[c] * wv.z; dh.w += dl[c] * wv.w;
                    }
                }
                const float4 ev = e4[d], av = a4[d], ha = hsw4(av);
                const float4 gu = hsw_grad4(make_float4(ev.x + ha.x, ev.y + ha.y, ev.z + ha.z, ev.w + ha.w));
                const float4 du = make_float4(dh.x * gu.x, dh.y * gu.y, dh.z * gu.z, dh.w * gu.w);
                const float4 ga = hsw_grad4(av);
                de4[d] = du;
                da4[d] = make_float4(du.x * ga.x, du.y * ga.y, du.z * ga.z, du.w * ga.w);
            }
        }
        return;
    }
    // ---- smax_fc weight / bias gradient: gw[c, k] += sum_t dlogits[t, c] hidden[t, k];  gb[c] += sum_t dlogits[t, c]
    float (*red)[65] = reinterpret_cast<float (*)[65]>(w_s);
    const int D = D4 * 4, nk = (D + 63) / 64;
    const int job = (int)blockIdx.x - n_dx, c = job / nk, kb = job - c * nk;
    const int kl = threadIdx.x & 63, g = threadIdx.x >> 6, k = kb * 64 + kl;
    const int kc = min(k, D - 1);
    float acc = 0.f, accb = 0.f;
    for (int t0 = g; t0 < T; t0 += 16 * 8) {
        float a[8], h[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int t = min(t0 + 16 * u, T - 1);
            a[u] = dlogits[(size_t)t * C + c];
            h[u] = hidden[(size_t)t * D + kc];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float m = (t0 + 16 * u < T) ? 1.f : 0.f;
            acc += m * a[u] * h[u];
            accb += m * a[u];
        }
    }
    red[g][kl] = acc;
    if (kl == 0) red[g][64] = accb;
    __syncthreads();
    if (g == 0) {
        float sw = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) sw += red[i][kl];
        if (k < D) gw[(size_t)c * D + k] += sw;
        if (gb && kl == 0 && kb == 0) {
            float sb = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) sb += red[i][64];
            gb[c] += sb;
        }
    }
}

int check_meld_head(int T, int D, int C, const char* what) {
    GF_CHECK_ARG(T >= 1 && D >= 4 && (D & 3) == 0 && D <= 1024 && C >= 1 && C <= MELD_MAX_C,
                 "%s: T=%d D=%d C=%d (D a multiple of 4 and <= 1024, 1 <= C <= %d)", what, T, D, C, MELD_MAX_C);
    return 0;
}

}  // namespace
}  // namespace ganffn

using namespace ganffn;

extern "C" int ganffn_meld_head_fwd(const float* emotions, const float* att, const float* w_fc, const float* b_fc, float* hidden,
                                    float* logits, int T, int D, int C, void* stream) {
    GF_TRY(check_meld_head(T, D, C, "meld_head_fwd"));
    GF_CHECK_ARG(emotions && att && w_fc && b_fc && hidden && logits, "meld_head_fwd: null pointer");
    GF_CHECK_ARG(aligned16(emotions) && aligned16(att) && aligned16(w_fc) && aligned16(hidden), "meld_head_fwd: buffers must be 16-byte aligned");
    const size_t lds = (size_t)C * D * sizeof(float);
    GF_TRY(lds_optin<meld_head_fwd_kernel>(lds, "meld_head_fwd"));
    const int blocks = (T + 3) / 4 < 512 ? (T + 3) / 4 : 512;
    hipLaunchKernelGGL(meld_head_fwd_kernel, dim3(blocks), dim3(256), lds, (hipStream_t)stream, emotions, att, w_fc, b_fc, hidden, logits,
                       T, D / 4, C);
    GF_LAUNCH_CHECK();
    return 0;
}

extern "C" int ganffn_meld_head_bwd(const float* dlogits, const float* emotions, const float* att, const float* hidden,
                                    const float* w_fc, float* d_emotions, float* d_att, float* gw_fc, float* gb_fc, int T, int D, int C,
                                    void* stream) {
    GF_TRY(check_meld_head(T, D, C, "meld_head_bwd"));
    GF_CHECK_ARG(dlogits && emotions && att && hidden && w_fc && d_emotions && d_att && gw_fc, "meld_head_bwd: null pointer");
    GF_CHECK_ARG(aligned16(emotions) && aligned16(att) && aligned16(w_fc) && aligned16(d_emotions) && aligned16(d_att),
                 "meld_head_bwd: buffers must be 16-byte aligned");
    const size_t red = 16 * 65 * sizeof(float), wb = (size_t)C * D * sizeof(float);
    const size_t lds = wb > red ? wb : red;
    GF_TRY(lds_optin<meld_head_bwd_kernel>(lds, "meld_head_bwd"));
    const int n_dx = (T + 15) / 16 < 256 ? (T + 15) / 16 : 256;
    const int n_dw = C * ((D + 63) / 64);
    hipLaunchKernelGGL(meld_head_bwd_kernel, dim3(n_dx + n_dw), dim3(1024), lds, (hipStream_t)stream, dlogits, emotions, att, hidden, w_fc,
                       d_emotions, d_att, gw_fc, gb_fc, T, D / 4, C, n_dx);
    GF_LAUNCH_CHECK();
    return 0;
}

// n floats of zeros on the stream (a gradient slab before a backward that accumulates into it)
extern "C" int ganffn_zero_floats(float* p, int64_t n, void* stream) {
    GF_CHECK_ARG(p && n > 0, "zero_floats: bad arguments");
    GF_HIP(hipMemsetAsync(p, 0, (size_t)n * sizeof(float), (hipStream_t)stream));
    return 0;
}
