// dialogue_rnn.hip — the DialogueRNN recurrence of BASELINE.json configs[4] (GAN_FFN_DialogueRNN head) on gfx950.
//
// Replaces DialogueRNNCell.forward / DialogueRNN.forward (/root/reference/model.py:828-972) in the configuration
// train_IEMOCAP_DialogueRNN.py runs (:586 --attention general, :595 listener off; dims :634-642: D_m = 100,
// D_g = D_p = 500, D_e = 100): per utterance step t and dialogue b
//     g_t  = drop(GRU_g([U_t, q_{t-1}[spk]], g_{t-1}))                    global state
//     c_t  = sum_j softmax_j(<W_a U_t, g_j>) g_j,  j < t                   "general" attention over the global history
//     q_t[spk] = m ? drop(GRU_p([U_t, c_t], q_{t-1}[spk])) : q_{t-1}[spk]  speaker's party state (listener unchanged)
//     e_t  = drop(GRU_e(q_t[spk], e_{t-1}))                                emotion state
// (m = qmask[t,b,spk]: 0 on padded steps, where the reference's blend keeps both party states.)
//
// Why not one kernel per dialogue: a step needs every cell's full weight matrix (12.7 MB per direction); one workgroup
// per dialogue would stream that through ONE CU 94 times.  Instead the dialogues are the N axis (<= 32 per tile) of
// skinny matrix products that spread a cell's weight rows over ~100-200 workgroups, and the S steps are a chain of small
// launches (2 per step forward, 2 backward, both directions of BiModel in the same launches; independent pieces of a step
// share a launch: within step t the global and the party cell do not depend on each other — the party cell reads the
// context over g_0 .. g_{t-1}, not g_t — so their four products are one launch and their gate kernels another, with the
// context attention of the next step behind the global cell's gate math in the workgroup that owns the dialogue; round 2
// ran the cells one after the other, 4 + 4 launches per step):
//   * everything that depends on U alone is hoisted out of the recurrence into three ordinary GEMMs over all steps
//     (x-parts of the g / p cells incl. b_ih, and the attention query W_a U_t);
//   * skinny_nt / skinny_nn: C[B x N] = A[B x K] W^T resp. A W on v_mfma_f32_16x16x4_f32 (exact fp32): a workgroup owns
//     16 weight rows (columns) and all dialogues, its waves split K and are summed through LDS in a fixed order;
//   * gate kernels (elementwise GRU math + Philox dropout + party select/update), attention kernels (one workgroup
//     per dialogue, history in L2);
//   * the emotion cell feeds nothing back into the recurrence: its input product for all steps is one GEMM after the
//     main loop and its own recurrence (independent per dialogue, 300 x 100 weight) runs as one persistent workgroup per
//     (dialogue, direction) — drnn_echain_fwd / bwd_kernel;
//   * backward mirrors it step by step in reverse; all weight gradients are deferred: the per-step gate gradients are
//     kept and ONE grouped TN GEMM launch (gemm.hip, owner-accumulated, no atomics) computes the 9 products at the end.
// Everything is deterministic (no atomics).  Dropout follows the Philox contract of common.h with rows t*B + b.
// listener_state = True (model.py:899-921, --active-listener) is a variant of the same driver (ganffn_drnn_listener_fwd /
// _bwd): 4 launches per step each way instead of 2 — see "Listener state" below.
// The other context attention types (--attention simple / dot / general2 / concat, model.py:117-194) run through
// ganffn_drnn_att_fwd / _bwd with the same launches per step: their extra work sits in the gate + attention launches (see
// "Other context attention types" below).
#include "common.h"

namespace ganffn {

typedef float floatx4 __attribute__((ext_vector_type(4)));

enum : uint32_t { SITE_DRNN_G = 8, SITE_DRNN_P = 9, SITE_DRNN_E = 10, SITE_DRNN_L = 11 };   // + 4 for the second direction

// ------------------------------------------------------------------------------------------
// skinny products: M <= 32 rows of A (dialogues) against a weight matrix; up to GANFFN_MAX_DIALOGUES rows in tiles of 32
// ("Dialogue-tile axis" below)
// ------------------------------------------------------------------------------------------
// (SkinnyProb / SkinnyGroup: common.h — lstm.hip runs its recurrent products through the same kernels)

// NT: C[b][n] = sum_k A[b][k] W[n][k] (+ Cin[b][n] + bias[n]).  Workgroup = 16 weight rows x 32 dialogues, NW waves split K
// (4 for the K = 500 products of the forward step, 12 for the K = 1500 ones of the backward step: 125 -> 128 k each).
// MFMA tile D[m = weight row][n' = dialogue]: A-operand = W rows, B-operand = A rows; both are float4 loads along k
// (k block of 16 per 4 MFMAs: step i contracts k = kb + 4g + i, identically on both operands).
// A launch is one link of a serial chain, so what counts is its latency: every load of a chunk of SK_NT k-blocks (a
// wave's whole K range in both uses) is issued before the first MFMA — one memory round trip (10.9 -> 9.9 us in-step).
// (Round 4: two weight tiles per workgroup — 4 loads per 4 MFMA groups instead of 3 per 2, half the workgroups, a third
// less L2 traffic — measured SLOWER: configuration 5 15.07 against 14.80 ms, three interleaved runs each.  The launch is not
// L2-bandwidth-sized; fewer, fatter waves lengthen the one round trip it consists of.)
constexpr int SK_NT = 8;
template <int NW>
__device__ __forceinline__ void skinny_nt_body(const SkinnyProb& q) {
    __shared__ __attribute__((aligned(16))) float red[NW][2][4][64];
    const int n0 = blockIdx.x * 16;
    if (n0 >= q.N) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int KQ = (((q.K + NW - 1) / NW) + 15) / 16 * 16;     // k range per wave, multiple of 16
    const int kbeg = w * KQ, kend = min(q.K, kbeg + KQ);
    const float* wrow = q.W + (size_t)min(n0 + c, q.N - 1) * q.ldw;
    const float* a0 = q.A + (size_t)min(c, q.M - 1) * q.lda;
    const float* a1 = q.A + (size_t)min(16 + c, q.M - 1) * q.lda;
    // the epilogue's addends (waves 0 and 1 write the tile) are fetched with the operands, not after the reduction
    float e_cin[4] = {0.f, 0.f, 0.f, 0.f}, e_cin2[4] = {0.f, 0.f, 0.f, 0.f}, e_bias[4] = {0.f, 0.f, 0.f, 0.f};
    if (threadIdx.x < 128) {
        const int eb = min(16 * (int)(threadIdx.x >> 6) + c, q.M - 1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int en = min(n0 + 4 * g + r, q.N - 1);
            if (q.Cin) e_cin[r] = q.Cin[(size_t)eb * q.ldcin + en];
            if (q.Cin2) e_cin2[r] = q.Cin2[(size_t)eb * q.ldc + en];
            if (q.bias) e_bias[r] = q.bias[en];
        }
    }
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kb = kbeg; kb < kend; kb += 16 * SK_NT) {
        float4 wv[SK_NT], x0[SK_NT], x1[SK_NT];
        float f[SK_NT];
#pragma unroll
        for (int u = 0; u < SK_NT; ++u) {
            const int k = kb + 16 * u + 4 * g;             // K % 4 == 0: a float4 never straddles the end
            f[u] = k < kend ? 1.f : 0.f;
            const int kc = max(min(k, q.K - 4), 0);
            wv[u] = *reinterpret_cast<const float4*>(wrow + kc);
            x0[u] = *reinterpret_cast<const float4*>(a0 + kc);
            x1[u] = *reinterpret_cast<const float4*>(a1 + kc);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < SK_NT; ++u) {
            const float wx = wv[u].x * f[u], wy = wv[u].y * f[u], wz = wv[u].z * f[u], ww = wv[u].w * f[u];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wx, x0[u].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wx, x1[u].x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wy, x0[u].y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wy, x1[u].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wz, x0[u].z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wz, x1[u].z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ww, x0[u].w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ww, x1[u].w, acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        red[w][0][r][lane] = acc0[r];
        red[w][1][r][lane] = acc1[r];
    }
    __syncthreads();
    // thread -> (dialogue tile mt, lane): sums the waves in order; lane holds C[b = 16 mt + c][n0 + 4g .. 4g+3]
    if (threadIdx.x < 128) {
        const int mt = threadIdx.x >> 6;
        const int b = 16 * mt + c, n = n0 + 4 * g;
        if (b < q.M && n < q.N) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = red[0][mt][r][lane];
#pragma unroll
                for (int ww = 1; ww < NW; ++ww) v[r] += red[ww][mt][r][lane];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (n + r < q.N) {
                    float o = v[r];
                    if (q.Cin) o += e_cin[r];
                    if (q.Cin2) o += e_cin2[r];
                    if (q.bias) o += e_bias[r];
                    q.C[(size_t)b * q.ldc + n + r] = o;
                }
            }
        }
    }
}
template <int NW>
__global__ __launch_bounds__(64 * NW) void skinny_nt_kernel(SkinnyGroup grp) { skinny_nt_body<NW>(grp.p[blockIdx.z]); }

// More than 8 NT problems in one launch: the listener's products of one step with P > 3 parties (one input-side product and
// one hidden-side product per party row, per direction: 2 (1 + P)).  A separate kernel, so that the 8-problem launches of
// the two-party recurrence and of lstm.hip keep their kernel and argument block.
constexpr int DR_MAXP = GANFFN_DRNN_MAX_PARTIES;
struct SkinnyGroupWide {
    SkinnyProb p[2 * (1 + DR_MAXP)];
};
static_assert(sizeof(SkinnyGroupWide) <= 4096, "the wide skinny group is passed as a kernel argument (4 KB at most)");
template <int NW>
__global__ __launch_bounds__(64 * NW) void skinny_nt_wide_kernel(SkinnyGroupWide grp) { skinny_nt_body<NW>(grp.p[blockIdx.z]); }

// out[c][r] = in[r][c] for up to 8 matrices [rows x cols] (leading dimension ld_in) -> [cols x rows]: the recurrent
// weights in the orientation the backward step's products read row-wise (once per backward call)
struct TrGroup { const float* in[8]; float* out[8]; int ld_in[8]; int rows, cols; };
__global__ __launch_bounds__(256) void drnn_transpose_kernel(TrGroup t) {
    __shared__ float tile[32][33];
    const int z = blockIdx.z, c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 8 * i, c = c0 + tx;
        tile[ty + 8 * i][tx] = (r < t.rows && c < t.cols) ? t.in[z][(size_t)r * t.ld_in[z] + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i, r = r0 + tx;
        if (r < t.rows && c < t.cols) t.out[z][(size_t)c * t.rows + r] = tile[tx][ty + 8 * i];
    }
}

// NN: C[b][n] = sum_k A[b][k] W[k][n] (+ Cin).  Workgroup = 16 output columns x 32 dialogues, 8 waves split K.
// MFMA tile D[m = dialogue][n' = column]: A-operand = A rows (float4 along k), B-operand = W[k][n0 + n'] (one dword per
// step: 16 consecutive columns of a row = 64 contiguous bytes).
__device__ __forceinline__ void skinny_nn_body(const SkinnyProb& q) {
    __shared__ __attribute__((aligned(16))) float red[8][2][4][64];
    const int n0 = blockIdx.x * 16;
    if (n0 >= q.N) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int KQ = (((q.K + 7) / 8) + 15) / 16 * 16;
    const int kbeg = w * KQ, kend = min(q.K, kbeg + KQ);
    const float* a0 = q.A + (size_t)min(c, q.M - 1) * q.lda;
    const float* a1 = q.A + (size_t)min(16 + c, q.M - 1) * q.lda;
    const float* wcol = q.W + min(n0 + c, q.N - 1);
    floatx4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kb = kbeg; kb < kend; kb += 16) {
        const int k = kb + 4 * g;
        const float f = k < kend ? 1.f : 0.f;
        const int kc = max(min(k, q.K - 4), 0);
        const float4 x0 = *reinterpret_cast<const float4*>(a0 + kc);
        const float4 x1 = *reinterpret_cast<const float4*>(a1 + kc);
        float wv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) wv[i] = wcol[(size_t)(kc + i) * q.ldw] * f;
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.x, wv[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.x, wv[0], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.y, wv[1], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.y, wv[1], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.z, wv[2], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.z, wv[2], acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0.w, wv[3], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1.w, wv[3], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        red[w][0][r][lane] = acc0[r];
        red[w][1][r][lane] = acc1[r];
    }
    __syncthreads();
    // accumulator register r of tile mt at lane (c, g) = C[b = 16 mt + 4g + r][n0 + c]
    if (threadIdx.x < 128) {
        const int mt = threadIdx.x >> 6;
        const int n = n0 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = 16 * mt + 4 * g + r;
            if (b < q.M && n < q.N) {
                float o = 0.f;
#pragma unroll
                for (int ww = 0; ww < 8; ++ww) o += red[ww][mt][r][lane];
                if (q.Cin) o += q.Cin[(size_t)b * q.ldcin + n];
                if (q.Cin2) o += q.Cin2[(size_t)b * q.ldc + n];
                q.C[(size_t)b * q.ldc + n] = o;
            }
        }
    }
}
__global__ __launch_bounds__(512) void skinny_nn_kernel(SkinnyGroup grp) { skinny_nn_body(grp.p[blockIdx.z]); }

// Dialogue-tile axis: 32 < M <= GANFFN_MAX_DIALOGUES.  blockIdx.y = y is a tile of 32 dialogues: the workgroup is exactly the
// workgroup of the kernels above on rows 32 y .. 32 y + 31 of A, Cin, Cin2 and C (M clipped to the rows left), so with the K
// split unchanged every row's sum is formed in the order the one-tile launch forms it: row b of an M-row product has the bits
// of the same row in any other product over the same W, whatever tile it falls in.  The weight rows are re-read per tile
// (from L2 / MALL after the first); a launch stays one memory round trip + one LDS reduction long, which is what a link of
// the chain costs — the alternative, a loop over the tiles inside the workgroup with wv[] kept in registers, makes each of
// the workgroup's waves M / 32 times as long and was not kept (DESIGN.md "Dialogue tiles").  Separate kernels, so that launches
// with M <= 32 keep their kernel, grid and argument block.
__device__ __forceinline__ SkinnyProb skinny_tile(const SkinnyProb& q) {
    SkinnyProb t = q;
    const int m0 = 32 * (int)blockIdx.y;
    t.A = q.A + (size_t)m0 * q.lda;
    t.Cin = q.Cin ? q.Cin + (size_t)m0 * q.ldcin : nullptr;
    t.Cin2 = q.Cin2 ? q.Cin2 + (size_t)m0 * q.ldc : nullptr;
    t.C = q.C + (size_t)m0 * q.ldc;
    t.M = min(32, q.M - m0);
    return t;
}
template <int NW>
__global__ __launch_bounds__(64 * NW) void skinny_nt_tiled_kernel(SkinnyGroup grp) {
    if (32 * (int)blockIdx.y >= grp.p[blockIdx.z].M) return;
    skinny_nt_body<NW>(skinny_tile(grp.p[blockIdx.z]));
}
template <int NW>
__global__ __launch_bounds__(64 * NW) void skinny_nt_wide_tiled_kernel(SkinnyGroupWide grp) {
    if (32 * (int)blockIdx.y >= grp.p[blockIdx.z].M) return;
    skinny_nt_body<NW>(skinny_tile(grp.p[blockIdx.z]));
}
__global__ __launch_bounds__(512) void skinny_nn_tiled_kernel(SkinnyGroup grp) {
    if (32 * (int)blockIdx.y >= grp.p[blockIdx.z].M) return;
    skinny_nn_body(skinny_tile(grp.p[blockIdx.z]));
}

int launch_skinny(const SkinnyGroup& grp, int nprob, bool nn, hipStream_t st) {
    int maxN = 0, maxK = 0, maxM = 0;
    for (int i = 0; i < nprob; ++i) {
        const SkinnyProb& q = grp.p[i];
        GF_CHECK_ARG(q.M >= 1 && q.M <= GANFFN_MAX_DIALOGUES && (q.K & 3) == 0 && (q.lda & 3) == 0 && aligned16(q.A) && (nn || ((q.ldw & 3) == 0 && aligned16(q.W))),
                     "drnn skinny product: M=%d K=%d lda=%d ldw=%d unsupported", q.M, q.K, q.lda, q.ldw);
        maxN = q.N > maxN ? q.N : maxN;
        maxK = q.K > maxK ? q.K : maxK;
        maxM = q.M > maxM ? q.M : maxM;
    }
    if (maxM > 32) {          // dialogue tiles on grid.y: the same launch count, (maxM + 31) / 32 times the workgroups
        const dim3 grid((maxN + 15) / 16, (maxM + 31) / 32, nprob);
        if (nn) hipLaunchKernelGGL(skinny_nn_tiled_kernel, grid, dim3(512), 0, st, grp);
        else if (maxK > 4 * 16 * SK_NT) hipLaunchKernelGGL(skinny_nt_tiled_kernel<12>, grid, dim3(768), 0, st, grp);
        else hipLaunchKernelGGL(skinny_nt_tiled_kernel<4>, grid, dim3(256), 0, st, grp);
        GF_LAUNCH_CHECK();
        return 0;
    }
    if (nn) hipLaunchKernelGGL(skinny_nn_kernel, dim3((maxN + 15) / 16, 1, nprob), dim3(512), 0, st, grp);
    else if (maxK > 4 * 16 * SK_NT) hipLaunchKernelGGL(skinny_nt_kernel<12>, dim3((maxN + 15) / 16, 1, nprob), dim3(768), 0, st, grp);
    else hipLaunchKernelGGL(skinny_nt_kernel<4>, dim3((maxN + 15) / 16, 1, nprob), dim3(256), 0, st, grp);
    GF_LAUNCH_CHECK();
    return 0;
}
// n NT problems in one launch: up to 8 through launch_skinny (the same launch as before parties were general), more through
// the wide group
static int launch_skinny_nt(const SkinnyProb* pr, int n, hipStream_t st) {
    if (n <= 8) {
        SkinnyGroup sg;
        for (int i = 0; i < n; ++i) sg.p[i] = pr[i];
        return launch_skinny(sg, n, false, st);
    }
    GF_CHECK_ARG(n <= 2 * (1 + DR_MAXP), "drnn skinny product: %d problems in one launch (<= %d)", n, 2 * (1 + DR_MAXP));
    SkinnyGroupWide wg;
    int maxN = 0, maxK = 0, maxM = 0;
    for (int i = 0; i < n; ++i) {
        const SkinnyProb& q = pr[i];
        GF_CHECK_ARG(q.M >= 1 && q.M <= GANFFN_MAX_DIALOGUES && (q.K & 3) == 0 && (q.lda & 3) == 0 && aligned16(q.A) && (q.ldw & 3) == 0 && aligned16(q.W),
                     "drnn skinny product: M=%d K=%d lda=%d ldw=%d unsupported", q.M, q.K, q.lda, q.ldw);
        wg.p[i] = q;
        maxN = q.N > maxN ? q.N : maxN;
        maxK = q.K > maxK ? q.K : maxK;
        maxM = q.M > maxM ? q.M : maxM;
    }
    if (maxM > 32) {
        const dim3 grid((maxN + 15) / 16, (maxM + 31) / 32, n);
        if (maxK > 4 * 16 * SK_NT) hipLaunchKernelGGL(skinny_nt_wide_tiled_kernel<12>, grid, dim3(768), 0, st, wg);
        else hipLaunchKernelGGL(skinny_nt_wide_tiled_kernel<4>, grid, dim3(256), 0, st, wg);
        GF_LAUNCH_CHECK();
        return 0;
    }
    if (maxK > 4 * 16 * SK_NT) hipLaunchKernelGGL(skinny_nt_wide_kernel<12>, dim3((maxN + 15) / 16, 1, n), dim3(768), 0, st, wg);
    else hipLaunchKernelGGL(skinny_nt_wide_kernel<4>, dim3((maxN + 15) / 16, 1, n), dim3(256), 0, st, wg);
    GF_LAUNCH_CHECK();
    return 0;
}

// ------------------------------------------------------------------------------------------
// GRU gate math (torch.nn.GRUCell: r, z, n row blocks; n = tanh(i_n + r * h_n); h' = (1 - z) n + z h)
// ------------------------------------------------------------------------------------------
struct GateDir {
    const float* GI; const float* GH;     // [B x 3H] pre-activations (biases included)
    const float* hprev;                   // [B x H]
    float* R; float* Z; float* N; float* HN;   // saved gates of this step [B x H]
    float* hout;                          // g / e cells: state after dropout [B x H]
    // party cell only:
    const int* spk; const int* spk_next;  // [B] speaker of this / the next step (spk_next NULL on the last step)
    const float* mval;                    // [B] 1 on valid steps, 0 on padding
    const float* Qprev; float* Qnext;     // [B x P x H] party states before / after this step
    float* QN; float* QSnext;             // [B x H] q_t[spk_t]; q_t[spk_{t+1}] (next step's g / p cell input)
    uint32_t site;
};
struct GateArgs {
    GateDir d[2];
    int B, H, row0;        // row0 = t * B: dropout row of dialogue 0
    float p; int train;
    int P;                 // parties (party cell; 1 <= P <= DR_MAXP)
    const uint64_t* rng; uint64_t add;
};

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + __expf(-x)); }

template <int PARTY>
__device__ __forceinline__ void gru_gate_fwd_body(const GateArgs& a, const GateDir& d, const int idx) {
    if (idx >= a.B * a.H) return;
    const int b = idx / a.H, u = idx - b * a.H, H3 = 3 * a.H;
    const float* gi = d.GI + (size_t)b * H3;
    const float* gh = d.GH + (size_t)b * H3;
    const float h = d.hprev[idx];
    const float r = sigm(gi[u] + gh[u]);
    const float z = sigm(gi[a.H + u] + gh[a.H + u]);
    const float hn = gh[2 * a.H + u];
    const float n = tanhf(gi[2 * a.H + u] + r * hn);
    float hnew = (1.0f - z) * n + z * h;
    d.R[idx] = r; d.Z[idx] = z; d.N[idx] = n; d.HN[idx] = hn;
    const DropCtx dc = make_drop(a.rng, a.add, d.site, a.p, a.train);
    hnew *= drop_mult1(dc, (uint32_t)(a.row0 + b), (uint32_t)a.H, (uint32_t)u);
    if (PARTY == 0) {
        d.hout[idx] = hnew;
    } else if (PARTY == 2) {
        d.QN[idx] = hnew;     // listener path: qs after its dropout (QSP[t]); drnn_listener_fwd_kernel blends and writes Q
    } else {
        // q_t[spk] = m ? qs : q_{t-1}[spk]; the other P - 1 parties keep their state (listener_state False, model.py:888-893)
        const int s = d.spk[b];
        const float m = d.mval[b];
        const float qs = m != 0.f ? hnew : h;
        const size_t q0 = (size_t)b * a.P * a.H + u;
        for (int pa = 0; pa < a.P; ++pa) d.Qnext[q0 + (size_t)pa * a.H] = pa == s ? qs : d.Qprev[q0 + (size_t)pa * a.H];
        d.QN[idx] = qs;
        if (d.spk_next) {
            const int sn = d.spk_next[b];
            d.QSnext[idx] = sn == s ? qs : d.Qprev[q0 + (size_t)sn * a.H];
        }
    }
}
template <int PARTY>
__global__ __launch_bounds__(256) void gru_gate_fwd_kernel(GateArgs a) {
    gru_gate_fwd_body<PARTY>(a, a.d[blockIdx.z], blockIdx.x * 256 + threadIdx.x);
}
struct GateBwdDir {
    const float* dh;        // [B x H] gradient wrt the cell output AFTER dropout (g / e cells) or wrt Q[t+1][spk] (party cell)
    const float* dh2;       // optional second addend (e cell: upstream dE_out[t])
    const float* R; const float* Z; const float* N; const float* HN;
    const float* hprev;
    float* dGI; float* dGH; // [B x 3H] gate gradients (kept for the weight-gradient GEMMs)
    float* dhdir;           // [B x H] direct path to hprev: dh' * z (+ (1 - m) dq for the party cell)
    const float* mval;      // party cell: [B]
    const int* spk;         // party cell: [B]; dh is then the [B x P x H] gradient wrt Q[t+1], read at party spk[b]
    uint32_t site;
    // party cell, optional: the previous (later-in-time) step's party-gradient assembly done here instead of in its own
    // launch — dQ[t+1][b][p] = p == spk_{t+1}[b] ? dQSp + dQSg : dQ[t+2][b][p]; written to pg_out (= dh) and used directly
    const float* pg_dQ = nullptr; const float* pg_dQSp = nullptr; const float* pg_dQSg = nullptr; const int* pg_spk = nullptr;
    float* pg_out = nullptr;
};
struct GateBwdArgs {
    GateBwdDir d[2];
    int B, H, row0;
    float p; int train;
    int P;                 // parties (party cell)
    const uint64_t* rng; uint64_t add;
};

template <int PARTY>
__device__ __forceinline__ void gru_gate_bwd_body(const GateBwdArgs& a, const GateBwdDir& d, const int idx) {
    if (idx >= a.B * a.H) return;
    const int b = idx / a.H, u = idx - b * a.H, H3 = 3 * a.H;
    float dout;
    if (PARTY == 1 && d.pg_out != nullptr) {
        const int sn = d.pg_spk[b], s = d.spk[b];
        const size_t o0 = (size_t)b * a.P * a.H + u;
        const float own = d.pg_dQSp[idx] + d.pg_dQSg[idx];
        dout = 0.f;
        for (int pa = 0; pa < a.P; ++pa) {
            const size_t o = o0 + (size_t)pa * a.H;
            const float v = pa == sn ? own : d.pg_dQ[o];
            d.pg_out[o] = v;
            if (pa == s) dout = v;
        }
    } else {
        dout = PARTY == 1 ? d.dh[((size_t)b * a.P + d.spk[b]) * a.H + u] : d.dh[idx];   // (PARTY 2, listener: dh = d qs [B x H])
    }
    if (d.dh2) dout += d.dh2[idx];
    float pass = 0.f;
    if (PARTY == 1) {
        const float m = d.mval[b];
        pass = m != 0.f ? 0.f : dout;      // padded step: q_t[spk] = q_{t-1}[spk]
        dout = m != 0.f ? dout : 0.f;
    }
    const DropCtx dc = make_drop(a.rng, a.add, d.site, a.p, a.train);
    const float dhn = dout * drop_mult1(dc, (uint32_t)(a.row0 + b), (uint32_t)a.H, (uint32_t)u);   // grad wrt h' (pre-dropout)
    const float r = d.R[idx], z = d.Z[idx], n = d.N[idx], hn = d.HN[idx], h = d.hprev[idx];
    const float dn = dhn * (1.0f - z);
    const float dz = dhn * (h - n);
    const float dnp = dn * (1.0f - n * n);
    const float drp = dnp * hn * r * (1.0f - r);
    const float dzp = dz * z * (1.0f - z);
    float* gi = d.dGI + (size_t)b * H3;
    float* gh = d.dGH + (size_t)b * H3;
    gi[u] = drp; gi[a.H + u] = dzp; gi[2 * a.H + u] = dnp;
    gh[u] = drp; gh[a.H + u] = dzp; gh[2 * a.H + u] = dnp * r;
    d.dhdir[idx] = dhn * z + pass;
}
template <int PARTY>
__global__ __launch_bounds__(256) void gru_gate_bwd_kernel(GateBwdArgs a) {
    gru_gate_bwd_body<PARTY>(a, a.d[blockIdx.z], blockIdx.x * 256 + threadIdx.x);
}
// ------------------------------------------------------------------------------------------
// "general" context attention of step t over the global history g_0 .. g_{t-1} (model.py:161-164,193)
// one workgroup per (dialogue, direction); G rows are (S+1) blocks of B: block j+1 = g_j
// ------------------------------------------------------------------------------------------
constexpr int DR_MAXS = 112;
struct AttnDir {
    const float* XA;     // [B x H] query W_a U_t of this step
    const float* G;      // [(S+1) B x H]
    float* CT;           // [B x H] context
    float* alpha;        // [B x S x S], row t
};
struct AttnArgs { AttnDir d[2]; int B, H, S, t; };

// 1024 threads per (dialogue, direction).  The work is tiny (t x H multiply-adds) and latency-bound, so every phase keeps
// many independent loads in flight: 16 waves take 2 history steps each per pass for the scores, and the pooling splits
// the history in two halves per column with 8 loads in flight per thread.
constexpr int DR_AT = 1024;
__device__ __forceinline__ void drnn_scores(const float* __restrict__ q, const float* __restrict__ G, int B, int H, int b, int t,
                                            float* __restrict__ out, int lane, int w) {
    float qr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) qr[i] = lane + 64 * i < H ? q[lane + 64 * i] : 0.f;
    for (int j0 = w; j0 < t; j0 += 32) {
        const int j1 = min(j0 + 16, t - 1);
        const float* g0 = G + ((size_t)(j0 + 1) * B + b) * H;
        const float* g1 = G + ((size_t)(j1 + 1) * B + b) * H;
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
            if (j0 + 16 < t) out[j0 + 16] = s1;
        }
    }
}

// Other context attention types (ganffn_drnn_att_*; model.py:134-194).  "simple" and "dot" are general attention with
// another hoisted query (the constant w, resp. U_t itself), so they run the bodies above as they are; "general2" takes a
// tanh on the scores, "concat" scores s_j = v . tanh(W_g g_j + W_u U_t) from P_j = W_g g_j, computed right after g_j in
// the workgroup that owns the dialogue, and X_t = U_t W_u^T (hoisted).
enum : int { ATT_GENERAL = GANFFN_DRNN_ATT_GENERAL, ATT_SIMPLE = GANFFN_DRNN_ATT_SIMPLE, ATT_DOT = GANFFN_DRNN_ATT_DOT,
             ATT_GENERAL2 = GANFFN_DRNN_ATT_GENERAL2, ATT_CONCAT = GANFFN_DRNN_ATT_CONCAT };
constexpr int DR_MAXDA = 512;
struct AttnXDir {
    float* TS;           // general2: [B x S x S] tanh scores, row t (saved for backward)
    float* P;            // concat: [S B x D_a] P_j = W_g g_j, row j B + b
    const float* XC;     // concat: [S B x D_a] X_t = W_u U_t, row t B + b
    const float* Wg;     // concat: W_g = transform.weight[:, :D_g], leading dimension ldw = D_g + D_m
    const float* v;      // concat: vector_prod.weight [D_a]
    float* dP;           // concat, backward: [S B x D_a] accumulated gradient wrt P_j
    float* dXC;          // concat, backward: [S B x D_a] gradient wrt X_t
    float* dVp;          // concat, backward: [S B x D_a] per-step partials of the gradient wrt v (reduced after the loop)
};
struct AttnX { AttnXDir d[2]; int ldw, Da; };

// concat: P_j[b] = W_g g_j[b] (g_j = G block j + 1); wave w takes rows w, w + 16, ... two at a time, lanes split D_g
__device__ __forceinline__ void drnn_concat_project(const AttnX& x, const AttnXDir& xd, const float* __restrict__ G, int B, int H,
                                                    int b, int j, int lane, int w) {
    const float* g = G + ((size_t)(j + 1) * B + b) * H;
    float gr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) gr[i] = lane + 64 * i < H ? g[lane + 64 * i] : 0.f;
    for (int a0 = w; a0 < x.Da; a0 += 32) {
        const int a1 = min(a0 + 16, x.Da - 1);
        const float* w0 = xd.Wg + (size_t)a0 * x.ldw;
        const float* w1 = xd.Wg + (size_t)a1 * x.ldw;
        float v0[8], v1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = min(lane + 64 * i, H - 1);
            v0[i] = w0[k];
            v1[i] = w1[k];
        }
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { s0 += gr[i] * v0[i]; s1 += gr[i] * v1[i]; }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) {
            xd.P[((size_t)j * B + b) * x.Da + a0] = s0;
            if (a0 + 16 < x.Da) xd.P[((size_t)j * B + b) * x.Da + a0 + 16] = s1;
        }
    }
}

// concat scores of step t: s_j = sum_a v_a tanh(P_j[a] + X_t[a]), j < t; wave per history step (two at a time), lanes split D_a
__device__ __forceinline__ void drnn_concat_scores(const AttnX& x, const AttnXDir& xd, int B, int b, int t, float* __restrict__ out,
                                                   int lane, int w) {
    const float* X = xd.XC + ((size_t)t * B + b) * x.Da;
    float xr[8], vr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int a = lane + 64 * i;
        xr[i] = a < x.Da ? X[a] : 0.f;
        vr[i] = a < x.Da ? xd.v[a] : 0.f;
    }
    for (int j0 = w; j0 < t; j0 += 32) {
        const int j1 = min(j0 + 16, t - 1);
        const float* p0 = xd.P + ((size_t)j0 * B + b) * x.Da;
        const float* p1 = xd.P + ((size_t)j1 * B + b) * x.Da;
        float v0[8], v1[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int a = min(lane + 64 * i, x.Da - 1);
            v0[i] = p0[a];
            v1[i] = p1[a];
        }
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { s0 += vr[i] * tanhf(v0[i] + xr[i]); s1 += vr[i] * tanhf(v1[i] + xr[i]); }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        if (lane == 0) {
            out[j0] = s0;
            if (j0 + 16 < t) out[j0 + 16] = s1;
        }
    }
}

template <int ATT>
__device__ __forceinline__ void drnn_attn_fwd_body(const AttnArgs& a, const AttnDir& d, const int b, const AttnX* x = nullptr) {
    __shared__ float sc[DR_MAXS + 16];
    __shared__ float red[2];
    __shared__ float part[512];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, t = a.t;
    if constexpr (ATT == ATT_CONCAT) drnn_concat_scores(*x, x->d[blockIdx.z], a.B, b, t, sc, lane, w);     // D_a <= 512 (host)
    else drnn_scores(d.XA + (size_t)b * a.H, d.G, a.B, a.H, b, t, sc, lane, w);     // H <= 512 (checked on the host)
    __syncthreads();
    // softmax over t <= 112 scores: the first two waves
    float v = tid < t ? sc[tid] : -INFINITY;
    if (ATT == ATT_GENERAL2 && tid < t) {         // s_j = tanh(<W U_t + b, g_j>) (model.py:169-182 with an all-ones mask)
        v = tanhf(v);
        x->d[blockIdx.z].TS[((size_t)b * a.S + t) * a.S + tid] = v;
    }
    float m = wave_max(v);
    if (tid < 128 && lane == 0) red[w] = m;
    __syncthreads();
    m = fmaxf(red[0], red[1]);
    __syncthreads();
    float e = tid < t ? __expf(v - m) : 0.f;
    const float es = wave_sum(e);
    if (tid < 128 && lane == 0) red[w] = es;
    __syncthreads();
    const float inv = 1.0f / (red[0] + red[1]);
    if (tid < t) {
        const float al = e * inv;
        sc[tid] = al;
        d.alpha[((size_t)b * a.S + t) * a.S + tid] = al;
    }
    __syncthreads();
    // context: c_k = sum_j alpha_j g_j[k]; thread (k, half) sums its half of the history, 8 loads in flight
    const int k = tid & 511, half = tid >> 9, jmid = (t + 1) >> 1;
    const int jb = half ? jmid : 0, je = half ? t : jmid;
    float c = 0.f;
    if (k < a.H) {
        const float* gk = d.G + ((size_t)a.B + b) * a.H + k;          // g_0[k]; step j adds j * B * H
        const size_t st = (size_t)a.B * a.H;
        for (int j = jb; j < je; j += 8) {
            float g[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) g[u] = gk[(size_t)min(j + u, je - 1) * st];
#pragma unroll
            for (int u = 0; u < 8; ++u) c += (j + u < je ? sc[j + u] : 0.f) * g[u];
        }
    }
    if (half) part[k] = c;
    __syncthreads();
    if (!half && k < a.H) d.CT[(size_t)b * a.H + k] = c + part[k];
}
__global__ __launch_bounds__(DR_AT) void drnn_attn_fwd_kernel(AttnArgs a) { drnn_attn_fwd_body<ATT_GENERAL>(a, a.d[blockIdx.z], blockIdx.x); }

// Second launch of a forward step: both cells' gate math and, behind the global cell's, the context attention of the NEXT
// step.  Blocks [0, party_blocks) run the party gate body (1024 elements each); block party_blocks + b owns dialogue b:
// its first H threads produce g_t[b], then the whole workgroup pools g_0 .. g_t[b] for step t + 1 (the newest history row
// was written by this very workgroup: a workgroup-scope fence + barrier orders it).
// (PARTY = 2: the listener path's party gate, which leaves the blend to drnn_listener_fwd_kernel)
struct GateAttnArgs { GateArgs g, p; AttnArgs at; int party_blocks, has_attn; };
template <int PARTY, int ATT = ATT_GENERAL>
__device__ __forceinline__ void drnn_gates_attn_fwd_body(const GateAttnArgs& a, const AttnX* x = nullptr) {
    if ((int)blockIdx.x < a.party_blocks) {
        gru_gate_fwd_body<PARTY>(a.p, a.p.d[blockIdx.z], blockIdx.x * DR_AT + threadIdx.x);
        return;
    }
    const int b = blockIdx.x - a.party_blocks;
    if ((int)threadIdx.x < a.g.H) gru_gate_fwd_body<0>(a.g, a.g.d[blockIdx.z], b * a.g.H + threadIdx.x);
    if (!a.has_attn) return;
    __threadfence_block();
    __syncthreads();
    if constexpr (ATT == ATT_CONCAT) {      // P_{t-1} = W_g g_{t-1} of the row just written, before the scores of step t read it
        drnn_concat_project(*x, x->d[blockIdx.z], a.at.d[blockIdx.z].G, a.at.B, a.at.H, b, a.at.t - 1, threadIdx.x & 63, threadIdx.x >> 6);
        __threadfence_block();
        __syncthreads();
    }
    drnn_attn_fwd_body<ATT>(a.at, a.at.d[blockIdx.z], b, x);
}
__global__ __launch_bounds__(DR_AT) void drnn_gates_attn_fwd_kernel(GateAttnArgs a) { drnn_gates_attn_fwd_body<1>(a); }
__global__ __launch_bounds__(DR_AT) void drnn_gates_attn_lfwd_kernel(GateAttnArgs a) { drnn_gates_attn_fwd_body<2>(a); }
// general2 / concat: the same launch with the attention type's own arguments (PARTY 1: listener-free, 2: listener)
struct GateAttnXArgs { GateAttnArgs a; AttnX x; };
template <int PARTY, int ATT>
__global__ __launch_bounds__(DR_AT) void drnn_gates_attnx_fwd_kernel(GateAttnXArgs a) { drnn_gates_attn_fwd_body<PARTY, ATT>(a.a, &a.x); }

struct AttnBwdDir {
    const float* dCT;    // [B x H]
    const float* XA;     // [B x H]
    const float* G;      // [(S+1) B x H]
    const float* alpha;  // [B x S x S]
    float* dG;           // [(S+1) B x H] accumulated gradient wrt g_j (block j+1)
    float* dXA;          // [B x H]
};
struct AttnBwdArgs { AttnBwdDir d[2]; int B, H, S, t; };

template <int ATT>
__device__ __forceinline__ void drnn_attn_bwd_body(const AttnBwdArgs& a, const AttnBwdDir& d, const int b, const AttnX* x = nullptr) {
    __shared__ float da[DR_MAXS + 16];
    __shared__ float al[DR_MAXS + 16];
    __shared__ float red[2];
    __shared__ float part[512];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, t = a.t;
    const float* dc = d.dCT + (size_t)b * a.H;
    drnn_scores(dc, d.G, a.B, a.H, b, t, da, lane, w);                 // d alpha_j = <dc, g_j>
    if (tid < t) al[tid] = d.alpha[((size_t)b * a.S + t) * a.S + tid];
    float ts = 0.f;
    if (ATT == ATT_GENERAL2 && tid < t) ts = x->d[blockIdx.z].TS[((size_t)b * a.S + t) * a.S + tid];
    __syncthreads();
    float dot = tid < t ? al[tid] * da[tid] : 0.f;
    dot = wave_sum(dot);
    if (tid < 128 && lane == 0) red[w] = dot;
    __syncthreads();
    const float tot = red[0] + red[1];
    __syncthreads();
    if (tid < t) {
        if (ATT == ATT_GENERAL2) da[tid] = al[tid] * (da[tid] - tot) * (1.0f - ts * ts);      // through the tanh
        else da[tid] = al[tid] * (da[tid] - tot);                      // d score_j
    }
    __syncthreads();
    // dXA_k = sum_j dscore_j g_j[k];  dG[j][k] += alpha_j dc_k + dscore_j x_k.  Thread (k, half) owns column k of its half of
    // the history: no other thread touches those dG elements (no race, no atomics).  (concat: the score path goes through P)
    const int k = tid & 511, half = tid >> 9, jmid = (t + 1) >> 1;
    const int jb = half ? jmid : 0, je = half ? t : jmid;
    float dx = 0.f;
    if (k < a.H) {
        const float dck = dc[k], xk = ATT == ATT_CONCAT ? 0.f : d.XA[(size_t)b * a.H + k];
        const size_t st = (size_t)a.B * a.H, base = ((size_t)a.B + b) * a.H + k;
        for (int j = jb; j < je; j += 8) {
            float g[8], og[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const size_t o = base + (size_t)min(j + u, je - 1) * st;
                if (ATT != ATT_CONCAT) g[u] = d.G[o];
                og[u] = d.dG[o];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (j + u < je) {
                    if (ATT == ATT_CONCAT) {
                        d.dG[base + (size_t)(j + u) * st] = og[u] + al[j + u] * dck;
                    } else {
                        dx += da[j + u] * g[u];
                        d.dG[base + (size_t)(j + u) * st] = og[u] + al[j + u] * dck + da[j + u] * xk;
                    }
                }
            }
        }
    }
    if constexpr (ATT != ATT_CONCAT) {
        if (half) part[k] = dx;
        __syncthreads();
        if (!half && k < a.H) d.dXA[(size_t)b * a.H + k] = dx + part[k];
    } else {
        // concat: thread (k, half) owns column k of the D_a-wide rows and its half of the history.
        //   dz_{j,k} = dscore_j v_k (1 - tanh^2),  dX_t[k] = sum_j dz_{j,k},  dP_j[k] += dz_{j,k},  dv partial[k] = sum_j dscore_j tanh
        __shared__ float dpt[DR_MAXDA];
        __shared__ float partv[DR_MAXDA];
        const AttnXDir& xd = x->d[blockIdx.z];
        const int Da = x->Da;
        float dv = 0.f;
        if (k < Da) {
            const float xc = xd.XC[((size_t)t * a.B + b) * Da + k], vc = xd.v[k];
            const size_t st = (size_t)a.B * Da, base = (size_t)b * Da + k;
            for (int j = jb; j < je; j += 8) {
                float pv[8], op[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const size_t o = base + (size_t)min(j + u, je - 1) * st;
                    pv[u] = xd.P[o];
                    op[u] = xd.dP[o];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (j + u < je) {
                        const float th = tanhf(pv[u] + xc);
                        const float dz = da[j + u] * vc * (1.0f - th * th);
                        dx += dz;
                        dv += da[j + u] * th;
                        const float np = op[u] + dz;
                        xd.dP[base + (size_t)(j + u) * st] = np;
                        if (j + u == t - 1) dpt[k] = np;               // dP_{t-1} is complete: step t is the last reader of g_{t-1}
                    }
                }
            }
        }
        if (half && k < Da) { part[k] = dx; partv[k] = dv; }
        __threadfence_block();
        __syncthreads();
        if (!half && k < Da) {
            xd.dXC[((size_t)t * a.B + b) * Da + k] = dx + part[k];
            xd.dVp[((size_t)t * a.B + b) * Da + k] = dv + partv[k];
        }
        __syncthreads();
        // dG[g_{t-1}] += W_g^T dP_{t-1} (before the global gate gradient of step t - 1 reads it): thread (k, half) sums its half
        // of the D_a rows, the halves are added in a fixed order
        const int amid = (Da + 1) >> 1, ab = half ? amid : 0, ae = half ? Da : amid;
        float s = 0.f;
        if (k < a.H) {
            const float* wk = xd.Wg + k;
            for (int c = ab; c < ae; c += 8) {
                float wv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) wv[u] = wk[(size_t)min(c + u, ae - 1) * x->ldw];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += c + u < ae ? wv[u] * dpt[c + u] : 0.f;
            }
        }
        if (half && k < a.H) part[k] = s;
        __syncthreads();
        if (!half && k < a.H) {
            float* dg = d.dG + ((size_t)t * a.B + b) * a.H + k;
            *dg = *dg + (s + part[k]);
        }
    }
}
__global__ __launch_bounds__(DR_AT) void drnn_attn_bwd_kernel(AttnBwdArgs a) { drnn_attn_bwd_body<ATT_GENERAL>(a, a.d[blockIdx.z], blockIdx.x); }

// First launch of a backward step t: the attention backward of step t + 1 (it completes dG row t + 1 of its dialogue),
// then the global cell's gate gradient of step t on that row, in the workgroup that owns the dialogue; the party cell's
// gate gradient (independent of both) in blocks [0, party_blocks).
// (PARTY = 2: the listener path's party gate — dh = d qs assembled by drnn_listener_bwd_kernel, dh2 = d ss)
struct GateAttnBwdArgs { GateBwdArgs g, p; AttnBwdArgs at; int party_blocks, has_attn; };
template <int PARTY, int ATT = ATT_GENERAL>
__device__ __forceinline__ void drnn_gates_attn_bwd_body(const GateAttnBwdArgs& a, const AttnX* x = nullptr) {
    if ((int)blockIdx.x < a.party_blocks) {
        gru_gate_bwd_body<PARTY>(a.p, a.p.d[blockIdx.z], blockIdx.x * DR_AT + threadIdx.x);
        return;
    }
    const int b = blockIdx.x - a.party_blocks;
    if (a.has_attn) {
        drnn_attn_bwd_body<ATT>(a.at, a.at.d[blockIdx.z], b, x);
        __threadfence_block();
        __syncthreads();
    }
    if ((int)threadIdx.x < a.g.H) gru_gate_bwd_body<0>(a.g, a.g.d[blockIdx.z], b * a.g.H + threadIdx.x);
}
__global__ __launch_bounds__(DR_AT) void drnn_gates_attn_bwd_kernel(GateAttnBwdArgs a) { drnn_gates_attn_bwd_body<1>(a); }
__global__ __launch_bounds__(DR_AT) void drnn_gates_attn_lbwd_kernel(GateAttnBwdArgs a) { drnn_gates_attn_bwd_body<2>(a); }
struct GateAttnXBwdArgs { GateAttnBwdArgs a; AttnX x; };
template <int PARTY, int ATT>
__global__ __launch_bounds__(DR_AT) void drnn_gates_attnx_bwd_kernel(GateAttnXBwdArgs a) { drnn_gates_attn_bwd_body<PARTY, ATT>(a.a, &a.x); }

// small helpers of the other attention types (once per call, outside the step chain)
// simple: the constant query w in every row of XA
__global__ __launch_bounds__(256) void drnn_bcast_row_kernel(const float* __restrict__ w, float* __restrict__ out, int64_t rows, int cols) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < rows * cols) out[i] = w[i % cols];
}
// dot: dU += dXA (the query is U_t itself)
__global__ __launch_bounds__(256) void drnn_add_kernel(float* __restrict__ dst, const float* __restrict__ src, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += src[i];
}
// out[c] += sum_r A[r][c] in a fixed order (16 waves take rows w, w + 16, ...; the waves are added in order): simple's dw,
// concat's dv
__global__ __launch_bounds__(1024) void drnn_colsum_kernel(const float* __restrict__ A, int rows, int cols, float* __restrict__ out) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (c < cols)
        for (int r = w; r < rows; r += 16) s += A[(size_t)r * cols + c];
    part[w][lane] = s;
    __syncthreads();
    if (w == 0 && c < cols) {
        float o = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) o += part[i][lane];
        out[c] += o;
    }
}

// ------------------------------------------------------------------------------------------
// Listener state (listener_state = True, model.py:899-921): every party row also takes a listener GRU step
//     ql[p] = drop_L(GRU_l([U_t, qs], q_{t-1}[p]))      p = 0 .. P-1; qs = the speaker's new state after its dropout
//     q_t[p] = (m != 0 && p == spk) ? qs : ql[p]
// The input side [U_t, qs] is the same for every party row: its U part is one GEMM over all steps (XL, b_ih included), its
// qs part one skinny product per step; the hidden side is one skinny product per party row (Q's [B x P x H] rows, lda PH),
// all of them in one launch (launch_skinny_nt: the wide group beyond 8 problems, i.e. P > 3 with both directions).
// drnn_listener_fwd_kernel: the listener gates of every party row + the blend (writes Q[t+1], QN[t], QS[t+1] — what the
// party gate writes without the listener).  Dropout site SITE_DRNN_L (+4 per direction), row t*B + b, column p*H + u of
// a width-PH row.
// ------------------------------------------------------------------------------------------
struct LGateDir {
    const float* GI;          // [B x 3H] input pre-activations, shared by every party row: XL[t] + QSP[t] W_ih_l[:, Dm:]^T
    const float* GH;          // [B x P x 3H] hidden pre-activations per party row (b_hh included)
    const float* Qprev;       // [B x P x H] Q[t]
    const float* QSP;         // [B x H] qs of this step (after its dropout)
    float* R; float* Z; float* N; float* HN;      // [B x P x H] saved listener gates of this step
    const int* spk; const int* spk_next;          // spk_next NULL on the last step
    const float* mval;
    float* Qnext; float* QN; float* QSnext;       // as GateDir
    uint32_t site;
};
struct LGateArgs {
    LGateDir d[2];
    int B, H, row0;
    float p; int train;
    int P;
    const uint64_t* rng; uint64_t add;
};
__global__ __launch_bounds__(256) void drnn_listener_fwd_kernel(LGateArgs a) {
    const LGateDir& d = a.d[blockIdx.z];
    const int idx = blockIdx.x * 256 + threadIdx.x, H = a.H, HP = a.P * a.H;
    if (idx >= a.B * HP) return;
    const int b = idx / HP, j = idx - b * HP, pa = j / H, u = j - pa * H;
    const float* gi = d.GI + (size_t)b * 3 * H;
    const float* gh = d.GH + ((size_t)b * a.P + pa) * 3 * H;
    const float h = d.Qprev[idx];
    const float r = sigm(gi[u] + gh[u]);
    const float z = sigm(gi[H + u] + gh[H + u]);
    const float hn = gh[2 * H + u];
    const float n = tanhf(gi[2 * H + u] + r * hn);
    float hnew = (1.0f - z) * n + z * h;
    d.R[idx] = r; d.Z[idx] = z; d.N[idx] = n; d.HN[idx] = hn;
    const DropCtx dc = make_drop(a.rng, a.add, d.site, a.p, a.train);
    hnew *= drop_mult1(dc, (uint32_t)(a.row0 + b), (uint32_t)HP, (uint32_t)j);
    const int s = d.spk[b];
    const float q = (d.mval[b] != 0.f && pa == s) ? d.QSP[(size_t)b * H + u] : hnew;
    d.Qnext[idx] = q;
    if (pa == s) d.QN[(size_t)b * H + u] = q;
    if (d.spk_next && pa == d.spk_next[b]) d.QSnext[(size_t)b * H + u] = q;
}

// Backward of the listener and the blend at step t, one thread per (dialogue, column) covering every party row (so the
// party sum of the input-side gate gradient is formed in a fixed order, p = 0 .. P-1, without atomics).  Gradient wrt Q[t+1][p]:
//     dq[p] = dQl[p] + (p == spk_{t+1} ? dQSp + dQSg : 0) + (p == spk_t ? dQN[t] : 0)
// (dQl = dGH_l[p] W_hh_l + dh' z of step t+1: the listener's hidden path; dQSp / dQSg: QS[t+1] = Q[t+1][spk_{t+1}] as the
// party cell's hidden state and the global cell's input of step t+1; dQN: QN[t] = Q[t+1][spk_t] into the emotion cell).
// The row the blend took from qs passes dq to d qs and its listener gets zero.
struct LGateBwdDir {
    const float* dQl;         // [B x P x H] NULL on the last step
    const float* dQSp; const float* dQSg; const int* spk_next;
    const float* dQN;         // [B x H]
    const int* spk; const float* mval;
    const float* R; const float* Z; const float* N; const float* HN;   // [B x P x H]
    const float* Qprev;       // [B x P x H] Q[t]
    float* dGI;               // [B x 3H] input-side gate gradient, summed over the party rows
    float* dGH;               // [B x P x 3H]
    float* dhdir;             // [B x P x H] direct path to Q[t]: dh' z
    float* dqs;               // [B x H] gradient wrt qs through the blend
    uint32_t site;
};
struct LGateBwdArgs {
    LGateBwdDir d[2];
    int B, H, row0;
    float p; int train;
    int P;
    const uint64_t* rng; uint64_t add;
};
__global__ __launch_bounds__(256) void drnn_listener_bwd_kernel(LGateBwdArgs a) {
    const LGateBwdDir& d = a.d[blockIdx.z];
    const int idx = blockIdx.x * 256 + threadIdx.x, H = a.H, H3 = 3 * a.H;
    if (idx >= a.B * H) return;
    const int b = idx / H, u = idx - b * H;
    const int s = d.spk[b], sn = d.dQl ? d.spk_next[b] : -1;
    const bool took_qs = d.mval[b] != 0.f;
    const DropCtx dc = make_drop(a.rng, a.add, d.site, a.p, a.train);
    float sr = 0.f, sz = 0.f, sn_ = 0.f, dqs = 0.f;
    for (int pa = 0; pa < a.P; ++pa) {
        const size_t o = ((size_t)b * a.P + pa) * H + u;
        float dq = 0.f;
        if (d.dQl) {
            dq = d.dQl[o];
            if (pa == sn) dq += d.dQSp[idx] + d.dQSg[idx];
        }
        if (pa == s) dq += d.dQN[idx];
        if (took_qs && pa == s) { dqs = dq; dq = 0.f; }
        const float dhn = dq * drop_mult1(dc, (uint32_t)(a.row0 + b), (uint32_t)(a.P * H), (uint32_t)(pa * H + u));
        const float r = d.R[o], z = d.Z[o], n = d.N[o], hn = d.HN[o], h = d.Qprev[o];
        const float dn = dhn * (1.0f - z);
        const float dz = dhn * (h - n);
        const float dnp = dn * (1.0f - n * n);
        const float drp = dnp * hn * r * (1.0f - r);
        const float dzp = dz * z * (1.0f - z);
        float* gh = d.dGH + ((size_t)b * a.P + pa) * H3;
        gh[u] = drp; gh[H + u] = dzp; gh[2 * H + u] = dnp * r;
        sr += drp; sz += dzp; sn_ += dnp;
        d.dhdir[o] = dhn * z;
    }
    float* gi = d.dGI + (size_t)b * H3;
    gi[u] = sr; gi[H + u] = sz; gi[2 * H + u] = sn_;
    d.dqs[idx] = dqs;
}

// ------------------------------------------------------------------------------------------
// Emotion cell as ONE chain per dialogue (round 2).  e_t = drop(GRU_e(q_t[spk], e_{t-1})) takes q_t from the party cell
// but feeds nothing back into the recurrence, so: (1) its input product GI_e = QN W_ih^T + b_ih for ALL steps is one
// ordinary GEMM after the main loop; (2) what remains is a recurrence over e alone, independent per dialogue, with a
// 300 x 100 recurrent weight — one 512-thread workgroup per (dialogue, direction) runs all S steps with that weight in
// registers and no grid-level synchronisation.  The backward mirrors it (e chain first, then dQN for all steps as one
// GEMM).  Replaces 4 launches per step (2 skinny products, 2 gate kernels) by 4 launches per call.  D_e <= 128.
// ------------------------------------------------------------------------------------------
constexpr int EC_MAXHE = 128;
constexpr int EC_NT = 512;
struct EchainDir {
    const float* GI;          // [T x 3He] input pre-activations of all steps (b_ih included)
    const float* whh;         // [3He x He]
    const float* bhh;         // [3He]
    float* E;                 // [(S+1) B x He], block 0 = zeros
    float* R; float* Z; float* N; float* HN;      // [T x He] saved gates
    uint32_t site;
};
struct EchainArgs {
    EchainDir d[2];
    int S, B, He;
    float p; int train;
    const uint64_t* rng; uint64_t add;
};

__global__ __launch_bounds__(EC_NT) void drnn_echain_fwd_kernel(EchainArgs a) {
    const EchainDir& d = a.d[blockIdx.z];
    const int b = blockIdx.x, tid = threadIdx.x, He = a.He, H3 = 3 * He;
    __shared__ __attribute__((aligned(16))) float e_s[EC_MAXHE];
    __shared__ float gh_s[3 * EC_MAXHE];
    float w[EC_MAXHE];
    float bj = 0.f;
    if (tid < H3) {
        bj = d.bhh[tid];
#pragma unroll
        for (int k = 0; k < EC_MAXHE; ++k) w[k] = k < He ? d.whh[(size_t)tid * He + k] : 0.f;
    } else {
#pragma unroll
        for (int k = 0; k < EC_MAXHE; ++k) w[k] = 0.f;
    }
    if (tid < EC_MAXHE) e_s[tid] = 0.f;
    const DropCtx dc = make_drop(a.rng, a.add, d.site, a.p, a.train);
    // input pre-activations of the next 4 steps are always in flight (a step is ~1 us, an L2 / HBM round trip up to 2)
    constexpr int PF = 4;
    float gq[PF][3];
    const int uu = min(tid, He - 1);
    auto fetch = [&](int t, float (&g)[3]) __attribute__((always_inline)) {
        const float* gi = d.GI + ((size_t)min(t, a.S - 1) * a.B + b) * H3;
        g[0] = gi[uu]; g[1] = gi[He + uu]; g[2] = gi[2 * He + uu];
    };
#pragma unroll
    for (int i = 0; i < PF; ++i) fetch(i, gq[i]);
    for (int t = 0; t < a.S; ++t) {
        const size_t row = (size_t)t * a.B + b;
        const float gi0 = gq[0][0], gi1 = gq[0][1], gi2 = gq[0][2];
#pragma unroll
        for (int i = 0; i + 1 < PF; ++i) { gq[i][0] = gq[i + 1][0]; gq[i][1] = gq[i + 1][1]; gq[i][2] = gq[i + 1][2]; }
        fetch(t + PF, gq[PF - 1]);
        __syncthreads();                                   // e_s holds e_{t-1}
        {
            float acc = bj;
#pragma unroll
            for (int k4 = 0; k4 < EC_MAXHE / 4; ++k4) {
                if (4 * k4 < He) {                         // uniform
                    const float4 e4 = *reinterpret_cast<const float4*>(e_s + 4 * k4);
                    acc += e4.x * w[4 * k4] + e4.y * w[4 * k4 + 1] + e4.z * w[4 * k4 + 2] + e4.w * w[4 * k4 + 3];
                }
            }
            if (tid < H3) gh_s[tid] = acc;
        }
        __syncthreads();
        if (tid < He) {
            const float h = e_s[tid];
            const float r = sigm(gi0 + gh_s[tid]);
            const float z = sigm(gi1 + gh_s[He + tid]);
            const float hn = gh_s[2 * He + tid];
            const float n = tanhf(gi2 + r * hn);
            float hnew = (1.0f - z) * n + z * h;
            const size_t o = row * He + tid;
            d.R[o] = r; d.Z[o] = z; d.N[o] = n; d.HN[o] = hn;
            hnew *= drop_mult1(dc, (uint32_t)row, (uint32_t)He, (uint32_t)tid);
            d.E[((size_t)(t + 1) * a.B + b) * He + tid] = hnew;
            // (written after every thread has read e_s for this step's matvec: second barrier above)
            e_s[tid] = hnew;
        }
    }
}

struct EchainBwdDir {
    const float* d_e;         // [T x He] upstream gradient wrt every e_t
    const float* whh;         // [3He x He]
    const float* E;           // [(S+1) B x He]
    const float* R; const float* Z; const float* N; const float* HN;
    float* dGI; float* dGH;   // [T x 3He] gate gradients of all steps (kept for dQN and the weight gradients)
    uint32_t site;
};
struct EchainBwdArgs {
    EchainBwdDir d[2];
    int S, B, He;
    float p; int train;
    const uint64_t* rng; uint64_t add;
};

__global__ __launch_bounds__(EC_NT) void drnn_echain_bwd_kernel(EchainBwdArgs a) {
    const EchainBwdDir& d = a.d[blockIdx.z];
    const int b = blockIdx.x, tid = threadIdx.x, He = a.He, H3 = 3 * He;
    __shared__ float carry_s[EC_MAXHE];                   // gradient wrt e_t arriving from step t+1
    __shared__ float dgh_s[3 * EC_MAXHE];
    __shared__ float dir_s[EC_MAXHE];
    __shared__ float part_s[4][EC_MAXHE];
    // thread (k, part): column k of W_hh restricted to a quarter of its 3He rows
    const int k = tid & (EC_MAXHE - 1), part = tid >> 7, jper = (H3 + 3) / 4, j0 = part * jper;
    float wT[(3 * EC_MAXHE + 3) / 4];
#pragma unroll
    for (int i = 0; i < (3 * EC_MAXHE + 3) / 4; ++i) wT[i] = (k < He && i < jper && j0 + i < H3) ? d.whh[(size_t)(j0 + i) * He + k] : 0.f;
    if (tid < EC_MAXHE) carry_s[tid] = 0.f;
    const DropCtx dc = make_drop(a.rng, a.add, d.site, a.p, a.train);
    // the saved gates / states / upstream gradients of the next 4 steps are always in flight
    constexpr int PF = 4;
    float sq[PF][6];
    const int uu = min(tid, He - 1);
    auto fetch = [&](int t, float (&v)[6]) __attribute__((always_inline)) {
        const size_t o = ((size_t)max(t, 0) * a.B + b) * He + uu;
        v[0] = d.R[o]; v[1] = d.Z[o]; v[2] = d.N[o]; v[3] = d.HN[o]; v[4] = d.E[o]; v[5] = d.d_e[o];
    };
#pragma unroll
    for (int i = 0; i < PF; ++i) fetch(a.S - 1 - i, sq[i]);
    for (int t = a.S - 1; t >= 0; --t) {
        const size_t row = (size_t)t * a.B + b;
        const float r = sq[0][0], z = sq[0][1], n = sq[0][2], hn = sq[0][3], h = sq[0][4], de = sq[0][5];
#pragma unroll
        for (int i = 0; i + 1 < PF; ++i)
#pragma unroll
            for (int q = 0; q < 6; ++q) sq[i][q] = sq[i + 1][q];
        fetch(t - PF, sq[PF - 1]);
        __syncthreads();                                   // carry_s complete
        if (tid < He) {
            const float dout = carry_s[tid] + de;
            const float dhn = dout * drop_mult1(dc, (uint32_t)row, (uint32_t)He, (uint32_t)tid);
            const float dn = dhn * (1.0f - z);
            const float dz = dhn * (h - n);
            const float dnp = dn * (1.0f - n * n);
            const float drp = dnp * hn * r * (1.0f - r);
            const float dzp = dz * z * (1.0f - z);
            float* gi = d.dGI + row * H3;
            float* gh = d.dGH + row * H3;
            gi[tid] = drp; gi[He + tid] = dzp; gi[2 * He + tid] = dnp;
            gh[tid] = drp; gh[He + tid] = dzp; gh[2 * He + tid] = dnp * r;
            dgh_s[tid] = drp; dgh_s[He + tid] = dzp; dgh_s[2 * He + tid] = dnp * r;
            dir_s[tid] = dhn * z;
        }
        __syncthreads();
        {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < (3 * EC_MAXHE + 3) / 4; ++i)
                if (i < jper) acc += dgh_s[min(j0 + i, H3 - 1)] * wT[i];     // (rows beyond H3 carry zero weights)
            part_s[part][k] = acc;
        }
        __syncthreads();
        if (tid < He) carry_s[tid] = dir_s[tid] + ((part_s[0][tid] + part_s[1][tid]) + (part_s[2][tid] + part_s[3][tid]));
    }
}

// ------------------------------------------------------------------------------------------
// Host side.  Every entry point of the recurrence fills one DrnnCall and runs drnn_fwd / drnn_bwd on it; one DrnnLayout per
// call says where every region of the saved-for-backward block and of the workspace lies.
// Layout (floats; every region 16-byte aligned): a function of (cfg, attention, listener, parties).  P = parties: the party
// states Q, their gradients dQ and the listener's per-party-row regions are [.. x P x ..]; P = 2 gives the sizes and offsets
// the two-party entry points always had.  The listener's regions lie behind the listener-free ones and general2's / concat's
// behind those, so a region's offset does not depend on what follows it; a region the configuration does not use is -1.
// ------------------------------------------------------------------------------------------
struct DrnnLayout {
    // saved: U-only products, states ((S + 1) blocks of B rows; block 0 = zeros), per-step inputs, gates of the g / p / e cells
    int64_t XG, XP, XA, G, Q, E, QS, CT, QN, Rg, Zg, Ng, HNg, Rp, Zp, Np, HNp, Re, Ze, Ne, HNe;
    int64_t XL = -1, QSP = -1, Rl = -1, Zl = -1, Nl = -1, HNl = -1;        // listener
    int64_t TS = -1, XC = -1, PC = -1;         // general2: tanh scores; concat: X_t = W_u U_t, P_j = W_g g_j
    int64_t saved_total;
    // workspace: pre-activations of a step, gate gradients of all steps, recurrent gradients (a / b: ping-pong)
    int64_t GI, GH, GIp, GHp, dGIg, dGHg, dGIp, dGHp, dGIe, dGHe, dXA, dCT, dG, dQa, dQb, dEa, dEb, dQsel, dQSp, dQSg, dhdir, dhdirG, dQN;
    int64_t GIe, dQNall, WT;      // emotion chain: input pre-activations / dQN of all steps; transposed recurrent weights (backward): 4 x [H x 3H]
    int64_t GIl = -1, GHl = -1, dGIl = -1, dGHl = -1, dss = -1, dqs = -1, dQl = -1, dhdirl = -1, WTl = -1;     // listener (WTl: transposed l_wih[:, Dm:], l_whh)
    int64_t dXC = -1, dP = -1, dVp = -1;       // concat
    int64_t ws_total;
};
static DrnnLayout drnn_layout(const ganffn_drnn_cfg* c, const ganffn_drnn_att& at, bool listener, int P) {
    DrnnLayout L;
    const int64_t T = (int64_t)c->S * c->B, T1 = (int64_t)(c->S + 1) * c->B, B = c->B, H = c->H, He = c->He, Da = at.Da;
    int64_t p = 0;
    auto take = [&](int64_t n) { int64_t r = p; p += (n + 3) & ~int64_t(3); return r; };
    L.XG = take(T * 3 * H); L.XP = take(T * 3 * H); L.XA = take(T * H);
    L.G = take(T1 * H); L.Q = take(T1 * P * H); L.E = take(T1 * He);
    L.QS = take(T1 * H); L.CT = take(T * H); L.QN = take(T * H);
    L.Rg = take(T * H); L.Zg = take(T * H); L.Ng = take(T * H); L.HNg = take(T * H);
    L.Rp = take(T * H); L.Zp = take(T * H); L.Np = take(T * H); L.HNp = take(T * H);
    L.Re = take(T * He); L.Ze = take(T * He); L.Ne = take(T * He); L.HNe = take(T * He);
    if (listener) { L.XL = take(T * 3 * H); L.QSP = take(T * H); L.Rl = take(T * P * H); L.Zl = take(T * P * H); L.Nl = take(T * P * H); L.HNl = take(T * P * H); }
    if (at.type == ATT_GENERAL2) L.TS = take(B * c->S * c->S);
    if (at.type == ATT_CONCAT) { L.XC = take(T * Da); L.PC = take(T * Da); }
    L.saved_total = p;

    p = 0;
    // D_e > EC_MAXHE: the emotion cell runs per step and borrows GI, GH ([B x 3 He]) and dhdir ([B x He]) from the global and
    // party cells, so those three hold the wider of the two cells (Hs); every other configuration keeps B*3*H / B*H
    const int64_t Hs = He > EC_MAXHE && He > H ? He : H;
    L.GI = take(B * 3 * Hs); L.GH = take(B * 3 * Hs); L.GIp = take(B * 3 * H); L.GHp = take(B * 3 * H);
    L.dGIg = take(T * 3 * H); L.dGHg = take(T * 3 * H); L.dGIp = take(T * 3 * H); L.dGHp = take(T * 3 * H);
    L.dGIe = take(T * 3 * He); L.dGHe = take(T * 3 * He);
    L.dXA = take(T * H); L.dCT = take(B * H); L.dG = take(T1 * H);
    L.dQa = take(B * P * H); L.dQb = take(B * P * H); L.dEa = take(B * He); L.dEb = take(B * He);
    L.dQsel = take(B * H); L.dQSp = take(B * H); L.dQSg = take(B * H); L.dhdir = take(B * Hs); L.dhdirG = take(B * H); L.dQN = take(B * H);
    L.GIe = take(T * 3 * He); L.dQNall = take(T * H);
    L.WT = take(4 * H * 3 * H);
    if (listener) {
        L.GIl = take(B * 3 * H); L.GHl = take(B * P * 3 * H); L.dGIl = take(T * 3 * H); L.dGHl = take(T * P * 3 * H);
        L.dss = take(B * H); L.dqs = take(B * H); L.dQl = take(B * P * H); L.dhdirl = take(B * P * H); L.WTl = take(2 * H * 3 * H);
    }
    if (at.type == ATT_CONCAT) { L.dXC = take(T * Da); L.dP = take(T * Da); L.dVp = take(T * Da); }
    L.ws_total = p;
    return L;
}

// maxB: 32 behind the entry points that always had that limit (they keep refusing 33 dialogues), GANFFN_MAX_DIALOGUES behind
// ganffn_drnn_batch_*
static int check_drnn(const ganffn_drnn_cfg* c, int ndir, int maxB = 32) {
    GF_CHECK_ARG(c, "null drnn cfg");
    GF_CHECK_ARG(ndir == 1 || ndir == 2, "drnn: ndir=%d", ndir);
    GF_CHECK_ARG(c->S >= 1 && c->S <= DR_MAXS && c->B >= 1 && c->B <= maxB, "drnn: S=%d (<= %d), B=%d (<= %d)", c->S, DR_MAXS, c->B, maxB);
    GF_CHECK_ARG(c->Dm >= 4 && (c->Dm & 3) == 0 && c->H >= 4 && (c->H & 3) == 0 && c->He >= 4 && (c->He & 3) == 0,
                 "drnn: D_m=%d, D_g=D_p=%d, D_e=%d must be multiples of 4", c->Dm, c->H, c->He);
    GF_CHECK_ARG(c->H <= 512, "drnn: D_g = D_p = %d > 512 (attention kernels hold one column per thread)", c->H);
    GF_CHECK_ARG(c->p >= 0.f && c->p < 1.f, "drnn: dropout p out of [0,1)");
    return 0;
}

static int check_att(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at) {
    GF_CHECK_ARG(at, "drnn_att: null attention descriptor");
    GF_CHECK_ARG(at->type >= GANFFN_DRNN_ATT_GENERAL && at->type <= GANFFN_DRNN_ATT_CONCAT,
                 "drnn_att: unknown attention type %d (0 general, 1 simple, 2 dot, 3 general2, 4 concat)", at->type);
    GF_CHECK_ARG(at->type != GANFFN_DRNN_ATT_CONCAT || (at->Da >= 4 && at->Da <= DR_MAXDA && (at->Da & 3) == 0),
                 "drnn_att: concat needs D_a a multiple of 4 in [4, %d], got D_a=%d", DR_MAXDA, at->Da);
    GF_CHECK_ARG(at->type != GANFFN_DRNN_ATT_DOT || c->Dm == c->H, "drnn_att: dot attention needs D_m == D_g, got D_m=%d D_g=%d",
                 c->Dm, c->H);
    return 0;
}
static int check_att_params(const ganffn_drnn_att* at, const ganffn_drnn_att_params* ap, int ndir) {
    GF_CHECK_ARG(ap || at->type == GANFFN_DRNN_ATT_DOT, "drnn_att: null attention parameters");
    for (int z = 0; z < ndir && at->type != GANFFN_DRNN_ATT_DOT; ++z) {
        GF_CHECK_ARG(ap[z].w && aligned16(ap[z].w), "drnn_att: direction %d: null or misaligned attention weight", z);
        GF_CHECK_ARG(at->type != GANFFN_DRNN_ATT_GENERAL2 || ap[z].b, "drnn_att: direction %d: general2 needs transform.bias", z);
        GF_CHECK_ARG(at->type != GANFFN_DRNN_ATT_CONCAT || ap[z].v, "drnn_att: direction %d: concat needs vector_prod.weight", z);
    }
    return 0;
}

static int check_parties(int P) {
    GF_CHECK_ARG(P >= 1 && P <= DR_MAXP, "drnn_party: parties=%d outside [1, %d] (GANFFN_DRNN_MAX_PARTIES)", P, DR_MAXP);
    return 0;
}

static int memset_f(float* p, int64_t n, hipStream_t st) {
    hipError_t e = hipMemsetAsync(p, 0, (size_t)n * sizeof(float), st);
    if (e != hipSuccess) return fail((int)e, "drnn: memset failed: %s", hipGetErrorString(e));
    return 0;
}

// What a forward or a backward call needs; the entry-point families differ only in what they put here.  Arrays have ndir entries.
struct DrnnCall {
    const ganffn_drnn_cfg* c; int ndir;
    const float* const* U; const int32_t* const* spk; const float* const* mval;
    const ganffn_drnn_params* prm; const ganffn_drnn_listener_params* lp;        // lp NULL: listener_state False
    float* const* alpha; float* const* saved; float* const* workspace;           // (the backward only reads alpha and saved)
    float* const* e_out;                                                         // forward
    const float* const* d_e; float* const* dU; const ganffn_drnn_grads* grd; const ganffn_drnn_listener_grads* lg;   // backward; lg may be NULL
    // context attention: always a descriptor and, per direction, its parameters and gradient pointers (a NULL member: the type
    // has no such tensor / that gradient is not wanted).  ap[z].w and ag[z].w are THE attention weight and its gradient.
    ganffn_drnn_att att; ganffn_drnn_att_params ap[2]; ganffn_drnn_att_grads ag[2];
    bool general_dw[2];                         // general attention: ag[z].w is produced (each entry point has its rule)
    int P = 2, maxB = 32;                       // parties; dialogue limit (GANFFN_MAX_DIALOGUES behind ganffn_drnn_batch_*)
    const uint64_t* rng; uint64_t add; hipStream_t st;
    // how the entry points fill it: one group of their arguments per setter
    DrnnCall& inputs(const float* const* U_, const int32_t* const* spk_, const float* const* mval_) { U = U_; spk = spk_; mval = mval_; return *this; }
    DrnnCall& cells(const ganffn_drnn_params* prm_, const ganffn_drnn_listener_params* lp_) { prm = prm_; lp = lp_; return *this; }
    DrnnCall& grads(const ganffn_drnn_grads* grd_, const ganffn_drnn_listener_grads* lg_) { grd = grd_; lg = lg_; return *this; }
    DrnnCall& limits(int parties, int max_dialogues) { P = parties; maxB = max_dialogues; return *this; }
    DrnnCall& forward(float* const* e, float* const* al, float* const* sv, float* const* ws) { e_out = e; alpha = al; saved = sv; workspace = ws; return *this; }
    DrnnCall& backward(const float* const* de, float* const* du, const float* const* al, const float* const* sv, float* const* ws) {
        d_e = de; dU = du; alpha = const_cast<float* const*>(al); saved = const_cast<float* const*>(sv); workspace = ws;
        return *this;
    }
};
static inline DrnnCall drnn_call(const ganffn_drnn_cfg* c, int ndir, const uint64_t* rng, uint64_t add, void* stream) {
    DrnnCall k{};
    k.c = c; k.ndir = ndir; k.rng = rng; k.add = add; k.st = (hipStream_t)stream;
    return k;
}
static int check_call(const DrnnCall& k) { return check_drnn(k.c, k.ndir, k.maxB) || check_parties(k.P) ? -1 : 0; }
// what both drivers refuse before their first launch; pass = "fwd" | "bwd", arrays_given: none of the pass's arguments is NULL
static int check_pass(const DrnnCall& k, const char* pass, bool arrays_given) {
    GF_TRY(check_call(k));
    GF_CHECK_ARG(arrays_given, "drnn_%s: null pointer", pass);
    GF_CHECK_ARG(!(k.c->train && k.c->p > 0.f) || k.rng, "drnn_%s: rng required in train mode", pass);
    for (int z = 0; k.lp && z < k.ndir; ++z)
        GF_CHECK_ARG(k.lp[z].l_wih && k.lp[z].l_whh && k.lp[z].l_bih && k.lp[z].l_bhh, "drnn_listener_%s: direction %d: null listener parameter", pass, z);
    return 0;
}
// the attention of the entry points without a descriptor (ganffn_drnn_fwd / _bwd, _listener_*): general, on the 13th cell tensor
static inline void att_of_cell(DrnnCall& k) {
    k.att = ganffn_drnn_att{ATT_GENERAL, 0};
    for (int z = 0; z < 2 && z < k.ndir; ++z) {             // (nothing is checked yet: the driver refuses a null prm / grd)
        if (k.prm) k.ap[z].w = k.prm[z].att_w;
        if (k.grd) { k.ag[z].w = k.grd[z].att_w; k.general_dw[z] = k.grd[z].g_wih != nullptr; }      // produced iff g_wih's is given
    }
}
// ... and of those with one (ganffn_drnn_att_* / _party_* / _batch_*): checked here, behind the call's own limits (the driver sees copies)
static int att_of_descriptor(DrnnCall& k, const ganffn_drnn_att* at, const ganffn_drnn_att_params* ap, const ganffn_drnn_att_grads* ag) {
    GF_TRY(check_call(k));
    GF_TRY(check_att(k.c, at));
    GF_TRY(check_att_params(at, ap, k.ndir));
    k.att = *at;
    for (int z = 0; z < k.ndir; ++z) {
        if (ap) k.ap[z] = ap[z];
        if (ag) { k.ag[z] = ag[z]; k.general_dw[z] = ag[z].w != nullptr; }      // produced iff agrads[z].w is given
    }
    return 0;
}

// One skinny product by name: out[M x N] = A[M x K] . W^T (NT launches, W [N x K]; NN launches: A . W, W [K x N])
// (+ addend[M x N]) (+ bias[N]); out_acc: added into out (the second addend is the output block itself)
struct Prod : SkinnyProb {
    Prod& a(const float* p, int ld) { A = p; lda = ld; return *this; }
    Prod& w(const float* p, int ld) { W = p; ldw = ld; return *this; }
    Prod& plus(const float* p, int ld) { Cin = p; ldcin = ld; return *this; }
    Prod& plus_bias(const float* b) { bias = b; return *this; }
    Prod& out(float* p, int ld) { C = p; ldc = ld; return *this; }
    Prod& out_acc(float* p, int ld) { Cin2 = p; return out(p, ld); }
};
static inline Prod prod(int M, int N, int K) { Prod q{}; q.M = M; q.N = N; q.K = K; return q; }

// what every gate kernel's argument block starts with: Hc = the cell's width, r0 = t * B
template <class Args> static inline void step_header(Args& a, const DrnnCall& k, int Hc, int64_t r0) {
    a.B = k.c->B; a.H = Hc; a.row0 = (int)r0; a.p = k.c->p; a.train = k.c->train; a.P = k.P; a.rng = k.rng; a.add = k.add;
}
// ... and what the attention half of the gate + attention launch of step t starts with (the attention is that of step t + 1)
template <class Args> static inline void attn_header(Args& a, const ganffn_drnn_cfg* c, int t) {
    a.party_blocks = (c->B * c->H + DR_AT - 1) / DR_AT;
    a.has_attn = t + 1 < c->S;
    a.at.B = c->B; a.at.H = c->H; a.at.S = c->S; a.at.t = t + 1;
}

// The gate + attention launch of a step: THE choice of its kernel <PARTY, ATT>, for both passes.  PARTY = 2 with listener state
// (the listener kernel then writes Q / QN / QS); general, simple and dot score <query, g_j> and run the plain kernels, general2
// and concat the x kernels with their own arguments (AttnX) behind the plain ones.  (PARTY = 1 and general2 are named first: the kernels
// lie in the code object in the order they are instantiated in.)
struct StepFwd {
    typedef GateAttnArgs Args; typedef GateAttnXArgs XArgs; static constexpr bool bwd = false;
    static auto plain(bool listener) { return !listener ? drnn_gates_attn_fwd_kernel : drnn_gates_attn_lfwd_kernel; }
    template <int ATT> static auto extra(bool listener) { return !listener ? drnn_gates_attnx_fwd_kernel<1, ATT> : drnn_gates_attnx_fwd_kernel<2, ATT>; }
};
struct StepBwd {
    typedef GateAttnBwdArgs Args; typedef GateAttnXBwdArgs XArgs; static constexpr bool bwd = true;
    static auto plain(bool listener) { return !listener ? drnn_gates_attn_bwd_kernel : drnn_gates_attn_lbwd_kernel; }
    template <int ATT> static auto extra(bool listener) { return !listener ? drnn_gates_attnx_bwd_kernel<1, ATT> : drnn_gates_attnx_bwd_kernel<2, ATT>; }
};
template <class Step> static inline void launch_gates_attn(const typename Step::Args& a, const DrnnCall& k, const DrnnLayout& L) {
    const bool listener = k.lp != nullptr, cc = k.att.type == ATT_CONCAT;
    const dim3 grid(a.party_blocks + a.at.B, 1, k.ndir);
    if (k.att.type == ATT_GENERAL2 || cc) {
        typename Step::XArgs gx;
        gx.a = a;
        gx.x.ldw = k.c->H + k.c->Dm; gx.x.Da = k.att.Da;
        for (int z = 0; z < k.ndir; ++z) {
            float* sv = k.saved[z]; float* ws = k.workspace[z];
            gx.x.d[z] = AttnXDir{cc ? nullptr : sv + L.TS, cc ? sv + L.PC : nullptr, cc ? sv + L.XC : nullptr, k.ap[z].w, k.ap[z].v,
                                 cc && Step::bwd ? ws + L.dP : nullptr, cc && Step::bwd ? ws + L.dXC : nullptr, cc && Step::bwd ? ws + L.dVp : nullptr};
        }
        auto kern = k.att.type == ATT_GENERAL2 ? Step::template extra<ATT_GENERAL2>(listener) : Step::template extra<ATT_CONCAT>(listener);
        hipLaunchKernelGGL(kern, grid, dim3(DR_AT), 0, k.st, gx);
    } else {
        auto kern = Step::plain(listener);
        hipLaunchKernelGGL(kern, grid, dim3(DR_AT), 0, k.st, a);
    }
}

}  // namespace ganffn

using namespace ganffn;

static int skinny_copies(bool nn, int copies, const SkinnyProb& q, hipStream_t st) {      // copy i: weight i, output i
    SkinnyGroup sg;
    for (int i = 0; i < copies; ++i) sg.p[i] = Prod{q}.w(q.W + (size_t)i * q.N * q.K, q.ldw).out(q.C + (size_t)i * q.M * q.N, q.ldc);
    return launch_skinny(sg, copies, nn, st);
}
// test / measurement hook: one skinny product C[M x N] = A[M x K] W^T (nn = 0, W [N x K]) or A W (nn = 1, W [K x N]),
// replicated `copies` (<= 8) times in one launch like a step of the recurrence (2 directions x 2 cells x 2 products)
extern "C" int ganffn_drnn_skinny(int nn, int copies, const float* A, const float* W, float* C, int M, int N, int K, void* stream) {
    GF_CHECK_ARG(M >= 1 && M <= 32, "drnn_skinny: M=%d (1 .. 32; ganffn_drnn_skinny_batch takes more)", M);
    GF_CHECK_ARG(A && W && C && copies >= 1 && copies <= 8, "drnn_skinny: bad arguments");
    return skinny_copies(nn != 0, copies, prod(M, N, K).a(A, K).w(W, nn ? N : K).out(C, N), (hipStream_t)stream);
}

// the same with the dialogue-tile axis: M <= GANFFN_MAX_DIALOGUES (M <= 32 is the launch above)
extern "C" int ganffn_drnn_skinny_batch(int nn, int copies, const float* A, const float* W, float* C, int M, int N, int K, void* stream) {
    GF_CHECK_ARG(A && W && C && copies >= 1 && copies <= 8, "drnn_skinny_batch: bad arguments");
    GF_CHECK_ARG(M >= 1 && M <= GANFFN_MAX_DIALOGUES && N >= 1 && K >= 4, "drnn_skinny_batch: M=%d (1 .. %d) N=%d K=%d", M, GANFFN_MAX_DIALOGUES, N, K);
    return skinny_copies(nn != 0, copies, prod(M, N, K).a(A, K).w(W, nn ? N : K).out(C, N), (hipStream_t)stream);
}

// sizes per direction: the layout's two totals (no descriptor: general attention; no party count: two parties)
static const ganffn_drnn_att ATT_OF_CELL{ATT_GENERAL, 0};
extern "C" int64_t ganffn_drnn_saved_floats(const ganffn_drnn_cfg* c) { return check_drnn(c, 1) ? -1 : drnn_layout(c, ATT_OF_CELL, false, 2).saved_total; }
extern "C" int64_t ganffn_drnn_workspace_floats(const ganffn_drnn_cfg* c) { return check_drnn(c, 1) ? -1 : drnn_layout(c, ATT_OF_CELL, false, 2).ws_total; }
extern "C" int64_t ganffn_drnn_listener_saved_floats(const ganffn_drnn_cfg* c) { return check_drnn(c, 1) ? -1 : drnn_layout(c, ATT_OF_CELL, true, 2).saved_total; }
extern "C" int64_t ganffn_drnn_listener_workspace_floats(const ganffn_drnn_cfg* c) { return check_drnn(c, 1) ? -1 : drnn_layout(c, ATT_OF_CELL, true, 2).ws_total; }
extern "C" int64_t ganffn_drnn_att_saved_floats(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int listener) {
    return check_drnn(c, 1) || check_att(c, at) ? -1 : drnn_layout(c, *at, listener != 0, 2).saved_total;
}
extern "C" int64_t ganffn_drnn_att_workspace_floats(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int listener) {
    return check_drnn(c, 1) || check_att(c, at) ? -1 : drnn_layout(c, *at, listener != 0, 2).ws_total;
}
extern "C" int64_t ganffn_drnn_party_saved_floats(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int listener, int parties) {
    return check_drnn(c, 1) || check_att(c, at) || check_parties(parties) ? -1 : drnn_layout(c, *at, listener != 0, parties).saved_total;
}
extern "C" int64_t ganffn_drnn_party_workspace_floats(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int listener, int parties) {
    return check_drnn(c, 1) || check_att(c, at) || check_parties(parties) ? -1 : drnn_layout(c, *at, listener != 0, parties).ws_total;
}
// 1 <= B <= GANFFN_MAX_DIALOGUES dialogues (ganffn_drnn_batch_*): the same functions of B
extern "C" int64_t ganffn_drnn_batch_saved_floats(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int listener, int parties) {
    return check_drnn(c, 1, GANFFN_MAX_DIALOGUES) || check_att(c, at) || check_parties(parties) ? -1 : drnn_layout(c, *at, listener != 0, parties).saved_total;
}
extern "C" int64_t ganffn_drnn_batch_workspace_floats(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int listener, int parties) {
    return check_drnn(c, 1, GANFFN_MAX_DIALOGUES) || check_att(c, at) || check_parties(parties) ? -1 : drnn_layout(c, *at, listener != 0, parties).ws_total;
}

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
static int drnn_fwd(const DrnnCall& k) {
    const ganffn_drnn_cfg* c = k.c;
    const ganffn_drnn_params* prm = k.prm;
    const ganffn_drnn_listener_params* lp = k.lp;
    const float* const* U = k.U; const int32_t* const* spk = k.spk; const float* const* mval = k.mval;
    float* const* alpha = k.alpha; float* const* saved = k.saved; float* const* workspace = k.workspace;
    GF_TRY(check_pass(k, "fwd", U && spk && mval && prm && k.e_out && alpha && saved && workspace));
    const int ndir = k.ndir, P = k.P, att = k.att.type, Da = k.att.Da, S = c->S, B = c->B, Dm = c->Dm, H = c->H, He = c->He, T = S * B;
    const DrnnLayout L = drnn_layout(c, k.att, lp != nullptr, P);
    hipStream_t st = k.st;
    for (int z = 0; z < ndir; ++z) {
        GF_CHECK_ARG(U[z] && spk[z] && mval[z] && k.e_out[z] && alpha[z] && saved[z] && workspace[z] && aligned16(U[z]) &&
                     aligned16(saved[z]) && aligned16(workspace[z]), "drnn_fwd: direction %d: null or misaligned buffer", z);
        float* sv = saved[z];
        const float* aw = k.ap[z].w;
        // U-only terms for all steps, out[T x N] = U W[:, :Dm]^T (+ bias): XG (with bih_g), XP likewise, XA = the attention's query
        auto u_term = [&](const float* W, int ldw, const float* bias, float* out, int N) {
            return gemm(gemm_nt(U[z], W, out, T, N, Dm).ld(Dm, ldw, N).bias(bias).on(st));
        };
        GF_TRY(u_term(prm[z].g_wih, Dm + H, prm[z].g_bih, sv + L.XG, 3 * H));
        GF_TRY(u_term(prm[z].p_wih, Dm + H, prm[z].p_bih, sv + L.XP, 3 * H));
        if (att == ATT_GENERAL || att == ATT_GENERAL2) {      // query W U_t, general2: + b
            GF_TRY(u_term(aw, Dm, att == ATT_GENERAL2 ? k.ap[z].b : nullptr, sv + L.XA, H));
        } else if (att == ATT_DOT) {               // query U_t itself (D_m == D_g)
            hipError_t er = hipMemcpyAsync(sv + L.XA, U[z], (size_t)T * H * sizeof(float), hipMemcpyDeviceToDevice, st);
            if (er != hipSuccess) return fail((int)er, "drnn_fwd: memcpy failed: %s", hipGetErrorString(er));
        } else if (att == ATT_SIMPLE) {            // constant query w
            hipLaunchKernelGGL(drnn_bcast_row_kernel, dim3((unsigned)(((int64_t)T * H + 255) / 256)), dim3(256), 0, st, aw, sv + L.XA, (int64_t)T, H);
            GF_LAUNCH_CHECK();
        } else {                                   // concat: X = U W_u^T, W_u = transform.weight[:, D_g:]
            GF_TRY(u_term(aw + H, H + Dm, nullptr, sv + L.XC, Da));
        }
        if (lp) GF_TRY(u_term(lp[z].l_wih, Dm + H, lp[z].l_bih, sv + L.XL, 3 * H));      // listener: XL, with bih_l
        // zero initial states: G[0], Q[0], E[0], QS[0], CT[0]; alpha (entries j >= t stay zero)
        GF_TRY(memset_f(sv + L.G, (int64_t)B * H, st));
        GF_TRY(memset_f(sv + L.Q, (int64_t)B * P * H, st));
        GF_TRY(memset_f(sv + L.E, (int64_t)B * He, st));
        GF_TRY(memset_f(sv + L.QS, (int64_t)B * H, st));
        GF_TRY(memset_f(sv + L.CT, (int64_t)B * H, st));
        GF_TRY(memset_f(alpha[z], (int64_t)B * S * S, st));
    }
    const dim3 gHe((B * He + 255) / 256, 1, ndir);
    const bool echain = He <= EC_MAXHE;          // emotion cell as one chain per dialogue after the main loop
    // A step is two launches: the four products of the global and the party cell (the party cell needs c_t but not g_t, the
    // global cell neither: they are independent within a step), then both cells' gate math with the context attention of
    // step t + 1 behind the global cell's (c_0 = 0: step 0 needs none).
    for (int t = 0; t < S; ++t) {
        const int64_t r0 = (int64_t)t * B, r1 = (int64_t)(t + 1) * B;
        SkinnyGroup sg;
        for (int z = 0; z < ndir; ++z) {
            float* sv = saved[z]; float* ws = workspace[z];
            // ---- global cell: GI = QS[t] Wih_g[:, Dm:]^T + XG[t] ; GH = G[t] Whh_g^T + bhh_g
            sg.p[4 * z] = prod(B, 3 * H, H).a(sv + L.QS + r0 * H, H).w(prm[z].g_wih + Dm, Dm + H).plus(sv + L.XG + r0 * 3 * H, 3 * H).out(ws + L.GI, 3 * H);
            sg.p[4 * z + 1] = prod(B, 3 * H, H).a(sv + L.G + r0 * H, H).w(prm[z].g_whh, H).plus_bias(prm[z].g_bhh).out(ws + L.GH, 3 * H);
            // ---- party cell (speaker): GI = CT[t] Wih_p[:, Dm:]^T + XP[t] ; GH = QS[t] Whh_p^T + bhh_p
            sg.p[4 * z + 2] = prod(B, 3 * H, H).a(sv + L.CT + r0 * H, H).w(prm[z].p_wih + Dm, Dm + H).plus(sv + L.XP + r0 * 3 * H, 3 * H).out(ws + L.GIp, 3 * H);
            sg.p[4 * z + 3] = prod(B, 3 * H, H).a(sv + L.QS + r0 * H, H).w(prm[z].p_whh, H).plus_bias(prm[z].p_bhh).out(ws + L.GHp, 3 * H);
        }
        GF_TRY(launch_skinny(sg, 4 * ndir, false, st));
        GateAttnArgs gaa;
        GateArgs &ga = gaa.g, &gp = gaa.p;
        step_header(ga, k, H, r0);
        step_header(gp, k, H, r0);
        attn_header(gaa, c, t);
        for (int z = 0; z < ndir; ++z) {
            float* sv = saved[z]; float* ws = workspace[z];
            ga.d[z] = GateDir{ws + L.GI, ws + L.GH, sv + L.G + r0 * H, sv + L.Rg + r0 * H, sv + L.Zg + r0 * H, sv + L.Ng + r0 * H,
                              sv + L.HNg + r0 * H, sv + L.G + r1 * H, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              SITE_DRNN_G + 4u * z};
            gp.d[z] = GateDir{ws + L.GIp, ws + L.GHp, sv + L.QS + r0 * H, sv + L.Rp + r0 * H, sv + L.Zp + r0 * H, sv + L.Np + r0 * H,
                              sv + L.HNp + r0 * H, nullptr, spk[z] + r0, t + 1 < S ? spk[z] + r1 : nullptr, mval[z] + r0,
                              sv + L.Q + r0 * P * H, sv + L.Q + r1 * P * H, sv + L.QN + r0 * H, sv + L.QS + r1 * H,
                              SITE_DRNN_P + 4u * z};
            if (lp) gp.d[z].QN = sv + L.QSP + r0 * H;       // qs only; the listener kernel below writes Q / QN / QS
            gaa.at.d[z] = AttnDir{sv + L.XA + r1 * H, sv + L.G, sv + L.CT + r1 * H, alpha[z]};
        }
        launch_gates_attn<StepFwd>(gaa, k, L);
        GF_LAUNCH_CHECK();
        if (lp) {
            // ---- listener: GI_l = QSP[t] Wih_l[:, Dm:]^T + XL[t] ; GH_l[p] = Q[t][p] Whh_l^T + bhh_l (p = 0 .. P-1)
            SkinnyProb lpr[2 * (1 + DR_MAXP)];
            LGateArgs la;
            step_header(la, k, H, r0);
            for (int z = 0; z < ndir; ++z) {
                float* sv = saved[z]; float* ws = workspace[z];
                lpr[(1 + P) * z] = prod(B, 3 * H, H).a(sv + L.QSP + r0 * H, H).w(lp[z].l_wih + Dm, Dm + H).plus(sv + L.XL + r0 * 3 * H, 3 * H).out(ws + L.GIl, 3 * H);
                for (int pa = 0; pa < P; ++pa)
                    lpr[(1 + P) * z + 1 + pa] = prod(B, 3 * H, H).a(sv + L.Q + r0 * P * H + pa * H, P * H).w(lp[z].l_whh, H).plus_bias(lp[z].l_bhh)
                                                    .out(ws + L.GHl + pa * 3 * H, P * 3 * H);
                la.d[z] = LGateDir{ws + L.GIl, ws + L.GHl, sv + L.Q + r0 * P * H, sv + L.QSP + r0 * H, sv + L.Rl + r0 * P * H,
                                   sv + L.Zl + r0 * P * H, sv + L.Nl + r0 * P * H, sv + L.HNl + r0 * P * H, spk[z] + r0,
                                   t + 1 < S ? spk[z] + r1 : nullptr, mval[z] + r0, sv + L.Q + r1 * P * H, sv + L.QN + r0 * H,
                                   sv + L.QS + r1 * H, SITE_DRNN_L + 4u * z};
            }
            GF_TRY(launch_skinny_nt(lpr, (1 + P) * ndir, st));
            hipLaunchKernelGGL(drnn_listener_fwd_kernel, dim3((B * P * H + 255) / 256, 1, ndir), dim3(256), 0, st, la);
            GF_LAUNCH_CHECK();
        }
        if (echain) continue;
        // ---- emotion cell: GI = QN[t] Wih_e^T + bih_e ; GH = E[t] Whh_e^T + bhh_e
        GateArgs ge;
        step_header(ge, k, He, r0);
        for (int z = 0; z < ndir; ++z) {
            float* sv = saved[z]; float* ws = workspace[z];
            sg.p[2 * z] = prod(B, 3 * He, H).a(sv + L.QN + r0 * H, H).w(prm[z].e_wih, H).plus_bias(prm[z].e_bih).out(ws + L.GI, 3 * He);
            sg.p[2 * z + 1] = prod(B, 3 * He, He).a(sv + L.E + r0 * He, He).w(prm[z].e_whh, He).plus_bias(prm[z].e_bhh).out(ws + L.GH, 3 * He);
            ge.d[z] = GateDir{ws + L.GI, ws + L.GH, sv + L.E + r0 * He, sv + L.Re + r0 * He, sv + L.Ze + r0 * He, sv + L.Ne + r0 * He,
                              sv + L.HNe + r0 * He, sv + L.E + r1 * He, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              SITE_DRNN_E + 4u * z};
        }
        GF_TRY(launch_skinny(sg, 2 * ndir, false, st));
        hipLaunchKernelGGL(gru_gate_fwd_kernel<0>, gHe, dim3(256), 0, st, ge);
        GF_LAUNCH_CHECK();
    }
    if (echain) {
        EchainArgs ea;
        ea.S = S; ea.B = B; ea.He = He; ea.p = c->p; ea.train = c->train; ea.rng = k.rng; ea.add = k.add;
        for (int z = 0; z < ndir; ++z) {
            float* sv = saved[z]; float* ws = workspace[z];
            // GI_e of every step: one GEMM over all T rows of q_t[spk]
            GF_TRY(gemm(gemm_nt(sv + L.QN, prm[z].e_wih, ws + L.GIe, T, 3 * He, H).bias(prm[z].e_bih).on(st)));
            ea.d[z] = EchainDir{ws + L.GIe, prm[z].e_whh, prm[z].e_bhh, sv + L.E, sv + L.Re, sv + L.Ze, sv + L.Ne, sv + L.HNe,
                                SITE_DRNN_E + 4u * z};
        }
        hipLaunchKernelGGL(drnn_echain_fwd_kernel, dim3(B, 1, ndir), dim3(EC_NT), 0, st, ea);
        GF_LAUNCH_CHECK();
    }
    for (int z = 0; z < ndir; ++z) {
        hipError_t er = hipMemcpyAsync(k.e_out[z], saved[z] + L.E + (int64_t)B * He, (size_t)T * He * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (er != hipSuccess) return fail((int)er, "drnn_fwd: memcpy failed: %s", hipGetErrorString(er));
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------
static int drnn_bwd(const DrnnCall& k) {
    const ganffn_drnn_cfg* c = k.c;
    const ganffn_drnn_params* prm = k.prm;
    const ganffn_drnn_listener_params* lp = k.lp;
    const float* const* d_e = k.d_e; const float* const* U = k.U; const int32_t* const* spk = k.spk; const float* const* mval = k.mval;
    float* const* dU = k.dU; const float* const* alpha = k.alpha; const float* const* saved = k.saved; float* const* workspace = k.workspace;
    GF_TRY(check_pass(k, "bwd", d_e && U && spk && mval && prm && k.grd && dU && alpha && saved && workspace));
    const int ndir = k.ndir, P = k.P, att = k.att.type, Da = k.att.Da, S = c->S, B = c->B, Dm = c->Dm, H = c->H, He = c->He, T = S * B;
    const DrnnLayout L = drnn_layout(c, k.att, lp != nullptr, P);
    hipStream_t st = k.st;
    for (int z = 0; z < ndir; ++z) {
        GF_CHECK_ARG(d_e[z] && U[z] && dU[z] && saved[z] && workspace[z] && alpha[z], "drnn_bwd: direction %d: null buffer", z);
        float* ws = workspace[z];
        GF_TRY(memset_f(ws + L.dG, (int64_t)(S + 1) * B * H, st));
        GF_TRY(memset_f(ws + L.dQa, (int64_t)B * P * H, st));
        GF_TRY(memset_f(ws + L.dEa, (int64_t)B * He, st));
        GF_TRY(memset_f(ws + L.dXA, (int64_t)B * H, st));          // step 0 has no attention: dXA[0] = 0
        if (att == ATT_CONCAT) {            // dX (row block 0 stays zero), dP (accumulated), v partials (row block 0 stays zero)
            GF_TRY(memset_f(ws + L.dXC, (int64_t)T * Da, st));
            GF_TRY(memset_f(ws + L.dP, (int64_t)T * Da, st));
            GF_TRY(memset_f(ws + L.dVp, (int64_t)T * Da, st));
        }
    }
    const dim3 gHe((B * He + 255) / 256, 1, ndir);
    const bool echain = He <= EC_MAXHE;
    // the step products contract over the 3H gate rows: transposed copies [H x 3H] make them row-wise reads (the NT
    // kernel, 16.6 -> see DESIGN.md) — order per direction: p_wih[:, Dm:], p_whh, g_wih[:, Dm:], g_whh
    const int64_t WM = (int64_t)H * 3 * H;
    TrGroup tr;
    tr.rows = 3 * H; tr.cols = H;
    auto transposed = [&](int i, const float* src, int ld, float* out) { tr.in[i] = src; tr.ld_in[i] = ld; tr.out[i] = out; };
    for (int z = 0; z < ndir; ++z) {
        float* wt = workspace[z] + L.WT;
        transposed(4 * z, prm[z].p_wih + Dm, Dm + H, wt); transposed(4 * z + 1, prm[z].p_whh, H, wt + WM);
        transposed(4 * z + 2, prm[z].g_wih + Dm, Dm + H, wt + 2 * WM); transposed(4 * z + 3, prm[z].g_whh, H, wt + 3 * WM);
    }
    hipLaunchKernelGGL(drnn_transpose_kernel, dim3((H + 31) / 32, (3 * H + 31) / 32, 4 * ndir), dim3(256), 0, st, tr);
    GF_LAUNCH_CHECK();
    if (lp) {      // listener: l_wih[:, Dm:], l_whh
        for (int z = 0; z < ndir; ++z) {
            transposed(2 * z, lp[z].l_wih + Dm, Dm + H, workspace[z] + L.WTl); transposed(2 * z + 1, lp[z].l_whh, H, workspace[z] + L.WTl + WM);
        }
        hipLaunchKernelGGL(drnn_transpose_kernel, dim3((H + 31) / 32, (3 * H + 31) / 32, 2 * ndir), dim3(256), 0, st, tr);
        GF_LAUNCH_CHECK();
    }
    if (echain) {
        // emotion chain first (it depends on nothing else): gate gradients of all steps, then dQN of all steps in one GEMM
        EchainBwdArgs eb;
        eb.S = S; eb.B = B; eb.He = He; eb.p = c->p; eb.train = c->train; eb.rng = k.rng; eb.add = k.add;
        for (int z = 0; z < ndir; ++z) {
            const float* sv = saved[z]; float* ws = workspace[z];
            eb.d[z] = EchainBwdDir{d_e[z], prm[z].e_whh, sv + L.E, sv + L.Re, sv + L.Ze, sv + L.Ne, sv + L.HNe, ws + L.dGIe,
                                   ws + L.dGHe, SITE_DRNN_E + 4u * z};
        }
        hipLaunchKernelGGL(drnn_echain_bwd_kernel, dim3(B, 1, ndir), dim3(EC_NT), 0, st, eb);
        GF_LAUNCH_CHECK();
        for (int z = 0; z < ndir; ++z)
            GF_TRY(gemm(gemm_nn(workspace[z] + L.dGIe, prm[z].e_wih, workspace[z] + L.dQNall, T, H, 3 * He).on(st)));
    }
    for (int t = S - 1; t >= 0; --t) {
        const int64_t r0 = (int64_t)t * B, r1 = (int64_t)(t + 1) * B;
        const bool even = ((S - 1 - t) & 1) == 0;            // ping-pong of the recurrent gradients
        const int64_t dQin = even ? L.dQa : L.dQb;        // gradient wrt Q[t+1] (assembled by the party gate kernel below)
        const int64_t dEin = even ? L.dEa : L.dEb, dEout = even ? L.dEb : L.dEa;
        const int64_t dQNt = echain ? L.dQNall + r0 * H : L.dQN;      // dQN[t]: a row block of the chain's GEMM, or this step's product
        SkinnyGroup sg;
        // ---- emotion cell (per step only when the chain kernels do not apply)
        if (!echain) {
            GateBwdArgs ge;
            step_header(ge, k, He, r0);
            for (int z = 0; z < ndir; ++z) {
                const float* sv = saved[z]; float* ws = workspace[z];
                ge.d[z] = GateBwdDir{ws + dEin, d_e[z] + r0 * He, sv + L.Re + r0 * He, sv + L.Ze + r0 * He, sv + L.Ne + r0 * He,
                                     sv + L.HNe + r0 * He, sv + L.E + r0 * He, ws + L.dGIe + r0 * 3 * He, ws + L.dGHe + r0 * 3 * He,
                                     ws + L.dhdir, nullptr, nullptr, SITE_DRNN_E + 4u * z};
                // dQN[t] = dGI_e Wih_e ; dE_rec = dGH_e Whh_e + dhdir
                sg.p[2 * z] = prod(B, H, 3 * He).a(ws + L.dGIe + r0 * 3 * He, 3 * He).w(prm[z].e_wih, H).out(ws + L.dQN, H);
                sg.p[2 * z + 1] = prod(B, He, 3 * He).a(ws + L.dGHe + r0 * 3 * He, 3 * He).w(prm[z].e_whh, He).plus(ws + L.dhdir, He).out(ws + dEout, He);
            }
            hipLaunchKernelGGL(gru_gate_bwd_kernel<0>, gHe, dim3(256), 0, st, ge);
            GF_LAUNCH_CHECK();
            GF_TRY(launch_skinny(sg, 2 * ndir, true, st));
        }
        if (lp) {
            // ---- listener + blend backward: dGI_l (party sum), dGH_l, dh' z of both party rows, d qs through the blend
            // ---- then d ss = dGI_l Wih_l[:, Dm:] ; dQl[p] = dGH_l[p] Whh_l + dh' z (gradient wrt Q[t] through the listener)
            LGateBwdArgs lb;
            step_header(lb, k, H, r0);
            SkinnyProb lpr[2 * (1 + DR_MAXP)];
            for (int z = 0; z < ndir; ++z) {
                const float* sv = saved[z]; float* ws = workspace[z];
                const bool last = t == S - 1;
                lb.d[z] = LGateBwdDir{last ? nullptr : ws + L.dQl, ws + L.dQSp, ws + L.dQSg, last ? nullptr : spk[z] + r1,
                                      ws + dQNt, spk[z] + r0, mval[z] + r0,
                                      sv + L.Rl + r0 * P * H, sv + L.Zl + r0 * P * H, sv + L.Nl + r0 * P * H, sv + L.HNl + r0 * P * H,
                                      sv + L.Q + r0 * P * H, ws + L.dGIl + r0 * 3 * H, ws + L.dGHl + r0 * P * 3 * H, ws + L.dhdirl,
                                      ws + L.dqs, SITE_DRNN_L + 4u * z};
                const float* wt = ws + L.WTl;
                lpr[(1 + P) * z] = prod(B, H, 3 * H).a(ws + L.dGIl + r0 * 3 * H, 3 * H).w(wt, 3 * H).out(ws + L.dss, H);
                for (int pa = 0; pa < P; ++pa)
                    lpr[(1 + P) * z + 1 + pa] = prod(B, H, 3 * H).a(ws + L.dGHl + r0 * P * 3 * H + pa * 3 * H, P * 3 * H).w(wt + WM, 3 * H)
                                                    .plus(ws + L.dhdirl + pa * H, P * H).out(ws + L.dQl + pa * H, P * H);
            }
            hipLaunchKernelGGL(drnn_listener_bwd_kernel, dim3((B * H + 255) / 256, 1, ndir), dim3(256), 0, st, lb);
            GF_LAUNCH_CHECK();
            GF_TRY(launch_skinny_nt(lpr, (1 + P) * ndir, st));
        }
        // ---- gate gradients of both cells in one launch.  Party cell: gradient wrt Q[t+1][spk] = dQ[t+1][spk] + dQN (selected
        // inside the kernel).  Global cell: dg_t = dG[t+1] — the attention uses of g_t at later steps and the recurrent path
        // were all added by the steps already done.
        GateAttnBwdArgs gab;
        GateBwdArgs &gg = gab.g, &gb = gab.p;
        step_header(gg, k, H, r0);
        step_header(gb, k, H, r0);
        attn_header(gab, c, t);             // attention backward of step t + 1: needs its dCT (the products of step t + 1)
        for (int z = 0; z < ndir; ++z) {
            const float* sv = saved[z]; float* ws = workspace[z];
            gb.d[z] = GateBwdDir{ws + dQin, ws + dQNt, sv + L.Rp + r0 * H, sv + L.Zp + r0 * H, sv + L.Np + r0 * H, sv + L.HNp + r0 * H,
                                 sv + L.QS + r0 * H, ws + L.dGIp + r0 * 3 * H, ws + L.dGHp + r0 * 3 * H, ws + L.dhdir, mval[z] + r0,
                                 spk[z] + r0, SITE_DRNN_P + 4u * z};
            if (t < S - 1) {      // assemble dQ[t+1] here (the previous iteration's party-gradient launch is gone)
                const bool even1 = ((S - 2 - t) & 1) == 0;
                gb.d[z].pg_dQ = ws + (even1 ? L.dQa : L.dQb);
                gb.d[z].pg_out = ws + dQin;
                gb.d[z].pg_dQSp = ws + L.dQSp; gb.d[z].pg_dQSg = ws + L.dQSg; gb.d[z].pg_spk = spk[z] + r1;
            }
            if (lp) {             // listener: the party cell's output qs gets d qs (blend) + d ss (listener input); no pass-through
                gb.d[z].dh = ws + L.dqs; gb.d[z].dh2 = ws + L.dss;
                gb.d[z].pg_out = nullptr;
            }
            gg.d[z] = GateBwdDir{ws + L.dG + r1 * H, nullptr, sv + L.Rg + r0 * H, sv + L.Zg + r0 * H, sv + L.Ng + r0 * H, sv + L.HNg + r0 * H,
                                 sv + L.G + r0 * H, ws + L.dGIg + r0 * 3 * H, ws + L.dGHg + r0 * 3 * H, ws + L.dhdirG, nullptr,
                                 nullptr, SITE_DRNN_G + 4u * z};
            gab.at.d[z] = AttnBwdDir{ws + L.dCT, sv + L.XA + r1 * H, sv + L.G, alpha[z], ws + L.dG, ws + L.dXA + r1 * H};
        }
        launch_gates_attn<StepBwd>(gab, k, L);
        GF_LAUNCH_CHECK();
        // ---- the four dgrad products of the step in one launch
        for (int z = 0; z < ndir; ++z) {
            float* ws = workspace[z];
            const float* wt = ws + L.WT;
            // dCT[t] = dGI_p Wih_p[:, Dm:] ; dQS_p = dGH_p Whh_p + dhdir
            sg.p[4 * z] = prod(B, H, 3 * H).a(ws + L.dGIp + r0 * 3 * H, 3 * H).w(wt, 3 * H).out(ws + L.dCT, H);
            sg.p[4 * z + 1] = prod(B, H, 3 * H).a(ws + L.dGHp + r0 * 3 * H, 3 * H).w(wt + WM, 3 * H).plus(ws + L.dhdir, H).out(ws + L.dQSp, H);
            // dQS_g = dGI_g Wih_g[:, Dm:] ; dG[t] += dGH_g Whh_g + dhdir
            sg.p[4 * z + 2] = prod(B, H, 3 * H).a(ws + L.dGIg + r0 * 3 * H, 3 * H).w(wt + 2 * WM, 3 * H).out(ws + L.dQSg, H);
            sg.p[4 * z + 3] = prod(B, H, 3 * H).a(ws + L.dGHg + r0 * 3 * H, 3 * H).w(wt + 3 * WM, 3 * H).plus(ws + L.dhdirG, H).out_acc(ws + L.dG + r0 * H, H);
        }
        GF_TRY(launch_skinny(sg, 4 * ndir, false, st));
    }
    // ---- dU and the deferred weight gradients (all steps at once)
    for (int z = 0; z < ndir; ++z) {
        const float* sv = saved[z]; float* ws = workspace[z];
        const ganffn_drnn_grads& g = k.grd[z];
        const float* aw = k.ap[z].w;
        float* agw = k.ag[z].w;
        // dU = the first product, += every later one (.residual(dU): each element read and written by one thread)
        GF_TRY(gemm(gemm_nn(ws + L.dGIg, prm[z].g_wih, dU[z], T, Dm, 3 * H).ld(3 * H, Dm + H, Dm).on(st)));
        GF_TRY(gemm(gemm_nn(ws + L.dGIp, prm[z].p_wih, dU[z], T, Dm, 3 * H).ld(3 * H, Dm + H, Dm).residual(dU[z]).on(st)));
        if (att == ATT_GENERAL || att == ATT_GENERAL2) {
            GF_TRY(gemm(gemm_nn(ws + L.dXA, aw, dU[z], T, Dm, H).residual(dU[z]).on(st)));
        } else if (att == ATT_DOT) {
            hipLaunchKernelGGL(drnn_add_kernel, dim3((unsigned)(((int64_t)T * Dm + 255) / 256)), dim3(256), 0, st, dU[z], ws + L.dXA, (int64_t)T * Dm);
            GF_LAUNCH_CHECK();
        } else if (att == ATT_CONCAT) {         // dU += dX W_u
            GF_TRY(gemm(gemm_nn(ws + L.dXC, aw + H, dU[z], T, Dm, Da).ld(Da, H + Dm, Dm).residual(dU[z]).on(st)));
        }
        if (lp) GF_TRY(gemm(gemm_nn(ws + L.dGIl, lp[z].l_wih, dU[z], T, Dm, 3 * H).ld(3 * H, Dm + H, Dm).residual(dU[z]).on(st)));
        if (agw && att == ATT_SIMPLE) {         // dw = column sum of dXA (the constant query)
            hipLaunchKernelGGL(drnn_colsum_kernel, dim3((H + 63) / 64), dim3(1024), 0, st, ws + L.dXA, T, H, agw);
            GF_LAUNCH_CHECK();
        }
        if (k.ag[z].v && att == ATT_CONCAT) {   // dv: the per-step partials in a fixed order
            hipLaunchKernelGGL(drnn_colsum_kernel, dim3((Da + 63) / 64), dim3(1024), 0, st, ws + L.dVp, T, Da, k.ag[z].v);
            GF_LAUNCH_CHECK();
        }
        if (g.g_wih || agw) {
            TnDesc tn[16];
            int n = 0;
            if (g.g_wih) {
                tn[n++] = TnDesc{ws + L.dGIg, 3 * H, U[z], Dm, g.g_wih, Dm + H, g.g_bih, 3 * H, Dm, T};
                tn[n++] = TnDesc{ws + L.dGIg, 3 * H, sv + L.QS, H, g.g_wih + Dm, Dm + H, nullptr, 3 * H, H, T};
                tn[n++] = TnDesc{ws + L.dGHg, 3 * H, sv + L.G, H, g.g_whh, H, g.g_bhh, 3 * H, H, T};
                tn[n++] = TnDesc{ws + L.dGIp, 3 * H, U[z], Dm, g.p_wih, Dm + H, g.p_bih, 3 * H, Dm, T};
                tn[n++] = TnDesc{ws + L.dGIp, 3 * H, sv + L.CT, H, g.p_wih + Dm, Dm + H, nullptr, 3 * H, H, T};
                tn[n++] = TnDesc{ws + L.dGHp, 3 * H, sv + L.QS, H, g.p_whh, H, g.p_bhh, 3 * H, H, T};
                tn[n++] = TnDesc{ws + L.dGIe, 3 * He, sv + L.QN, H, g.e_wih, H, g.e_bih, 3 * He, H, T};
                tn[n++] = TnDesc{ws + L.dGHe, 3 * He, sv + L.E, He, g.e_whh, He, g.e_bhh, 3 * He, He, T};
            }
            if (att == ATT_GENERAL && k.general_dw[z])
                tn[n++] = TnDesc{ws + L.dXA, H, U[z], Dm, agw, Dm, nullptr, H, Dm, T};
            if (att == ATT_GENERAL2 && agw)             // transform.bias: the column sum of dXA
                tn[n++] = TnDesc{ws + L.dXA, H, U[z], Dm, agw, Dm, k.ag[z].b, H, Dm, T};
            if (att == ATT_CONCAT && agw) {            // dW_g = sum dP^T g, dW_u = sum dX^T U: the two column blocks of transform.weight
                tn[n++] = TnDesc{ws + L.dP, Da, sv + L.G + (int64_t)B * H, H, agw, H + Dm, nullptr, Da, H, T};
                tn[n++] = TnDesc{ws + L.dXC, Da, U[z], Dm, agw + H, H + Dm, nullptr, Da, Dm, T};
            }
            if (g.g_wih && lp && k.lg && k.lg[z].l_wih) {
                // listener: input side against [U, qs] (party-summed dGI_l), hidden side against Q[t][p] (P T rows)
                const ganffn_drnn_listener_grads& l = k.lg[z];
                tn[n++] = TnDesc{ws + L.dGIl, 3 * H, U[z], Dm, l.l_wih, Dm + H, l.l_bih, 3 * H, Dm, T};
                tn[n++] = TnDesc{ws + L.dGIl, 3 * H, sv + L.QSP, H, l.l_wih + Dm, Dm + H, nullptr, 3 * H, H, T};
                tn[n++] = TnDesc{ws + L.dGHl, 3 * H, sv + L.Q, H, l.l_whh, H, l.l_bhh, 3 * H, H, P * T};
            }
            if (n) GF_TRY(launch_gemm_tn_grouped(tn, n, st));
        }
    }
    return 0;
}

// ------------------------------------------------------------------------------------------
// entry points: five families, one DrnnCall each way.  ganffn_drnn_* and ganffn_drnn_listener_* (lprm given): general
// attention on the 13th cell tensor, two parties; ganffn_drnn_att_*: an attention descriptor, with (lprm != NULL) or without
// listener state; ganffn_drnn_party_*: and any party count 1 .. GANFFN_DRNN_MAX_PARTIES (att is its parties = 2 case);
// ganffn_drnn_batch_*: and 1 <= B <= GANFFN_MAX_DIALOGUES dialogues through the skinny products' dialogue-tile axis (B <= 32
// is the launch sequence of ganffn_drnn_party_*, bit for bit; above it the same number of launches per step).
// ------------------------------------------------------------------------------------------
extern "C" int ganffn_drnn_fwd(const ganffn_drnn_cfg* c, int ndir, const float* const* U, const int32_t* const* spk,
                               const float* const* mval, const ganffn_drnn_params* prm, float* const* e_out,
                               float* const* alpha, float* const* saved, float* const* workspace, const uint64_t* rng,
                               uint64_t add, void* stream) {
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, nullptr).forward(e_out, alpha, saved, workspace);
    att_of_cell(k);
    return drnn_fwd(k);
}
extern "C" int ganffn_drnn_listener_fwd(const ganffn_drnn_cfg* c, int ndir, const float* const* U, const int32_t* const* spk,
                                        const float* const* mval, const ganffn_drnn_params* prm,
                                        const ganffn_drnn_listener_params* lprm, float* const* e_out, float* const* alpha,
                                        float* const* saved, float* const* workspace, const uint64_t* rng, uint64_t add,
                                        void* stream) {
    GF_CHECK_ARG(lprm, "drnn_listener_fwd: null listener parameters");
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, lprm).forward(e_out, alpha, saved, workspace);
    att_of_cell(k);
    return drnn_fwd(k);
}
extern "C" int ganffn_drnn_bwd(const ganffn_drnn_cfg* c, int ndir, const float* const* d_e, const float* const* U,
                               const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* prm,
                               const ganffn_drnn_grads* grd, float* const* dU, const float* const* alpha,
                               const float* const* saved, float* const* workspace, const uint64_t* rng, uint64_t add,
                               void* stream) {
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, nullptr).grads(grd, nullptr).backward(d_e, dU, alpha, saved, workspace);
    att_of_cell(k);
    return drnn_bwd(k);
}
extern "C" int ganffn_drnn_listener_bwd(const ganffn_drnn_cfg* c, int ndir, const float* const* d_e, const float* const* U,
                                        const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* prm,
                                        const ganffn_drnn_listener_params* lprm, const ganffn_drnn_grads* grd,
                                        const ganffn_drnn_listener_grads* lgrd, float* const* dU, const float* const* alpha,
                                        const float* const* saved, float* const* workspace, const uint64_t* rng, uint64_t add,
                                        void* stream) {
    GF_CHECK_ARG(lprm, "drnn_listener_bwd: null listener parameters");
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, lprm).grads(grd, lgrd).backward(d_e, dU, alpha, saved, workspace);
    att_of_cell(k);
    return drnn_bwd(k);
}
extern "C" int ganffn_drnn_att_fwd(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int ndir, const float* const* U,
                                   const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* prm,
                                   const ganffn_drnn_listener_params* lprm, const ganffn_drnn_att_params* aprm,
                                   float* const* e_out, float* const* alpha, float* const* saved, float* const* workspace,
                                   const uint64_t* rng, uint64_t add, void* stream) {
    GF_CHECK_ARG(at, "drnn_att_fwd: null attention descriptor");
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, lprm).forward(e_out, alpha, saved, workspace);
    GF_TRY(att_of_descriptor(k, at, aprm, nullptr));
    return drnn_fwd(k);
}
extern "C" int ganffn_drnn_att_bwd(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int ndir, const float* const* d_e,
                                   const float* const* U, const int32_t* const* spk, const float* const* mval,
                                   const ganffn_drnn_params* prm, const ganffn_drnn_listener_params* lprm,
                                   const ganffn_drnn_att_params* aprm, const ganffn_drnn_grads* grd,
                                   const ganffn_drnn_listener_grads* lgrd, const ganffn_drnn_att_grads* agrd, float* const* dU,
                                   const float* const* alpha, const float* const* saved, float* const* workspace,
                                   const uint64_t* rng, uint64_t add, void* stream) {
    GF_CHECK_ARG(at, "drnn_att_bwd: null attention descriptor");
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, lprm).grads(grd, lgrd).backward(d_e, dU, alpha, saved, workspace);
    GF_TRY(att_of_descriptor(k, at, aprm, agrd));
    return drnn_bwd(k);
}
extern "C" int ganffn_drnn_party_fwd(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int parties, int ndir, const float* const* U,
                                     const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* prm,
                                     const ganffn_drnn_listener_params* lprm, const ganffn_drnn_att_params* aprm,
                                     float* const* e_out, float* const* alpha, float* const* saved, float* const* workspace,
                                     const uint64_t* rng, uint64_t add, void* stream) {
    GF_CHECK_ARG(at, "drnn_party_fwd: null attention descriptor");
    GF_TRY(check_parties(parties));
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, lprm).forward(e_out, alpha, saved, workspace).limits(parties, 32);
    GF_TRY(att_of_descriptor(k, at, aprm, nullptr));
    return drnn_fwd(k);
}
extern "C" int ganffn_drnn_party_bwd(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int parties, int ndir, const float* const* d_e,
                                     const float* const* U, const int32_t* const* spk, const float* const* mval,
                                     const ganffn_drnn_params* prm, const ganffn_drnn_listener_params* lprm,
                                     const ganffn_drnn_att_params* aprm, const ganffn_drnn_grads* grd,
                                     const ganffn_drnn_listener_grads* lgrd, const ganffn_drnn_att_grads* agrd, float* const* dU,
                                     const float* const* alpha, const float* const* saved, float* const* workspace,
                                     const uint64_t* rng, uint64_t add, void* stream) {
    GF_CHECK_ARG(at, "drnn_party_bwd: null attention descriptor");
    GF_TRY(check_parties(parties));
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, lprm).grads(grd, lgrd)
                     .backward(d_e, dU, alpha, saved, workspace).limits(parties, 32);
    GF_TRY(att_of_descriptor(k, at, aprm, agrd));
    return drnn_bwd(k);
}
extern "C" int ganffn_drnn_batch_fwd(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int parties, int ndir, const float* const* U,
                                     const int32_t* const* spk, const float* const* mval, const ganffn_drnn_params* prm,
                                     const ganffn_drnn_listener_params* lprm, const ganffn_drnn_att_params* aprm,
                                     float* const* e_out, float* const* alpha, float* const* saved, float* const* workspace,
                                     const uint64_t* rng, uint64_t add, void* stream) {
    GF_CHECK_ARG(at, "drnn_batch_fwd: null attention descriptor");
    GF_TRY(check_parties(parties));
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, lprm).forward(e_out, alpha, saved, workspace)
                     .limits(parties, GANFFN_MAX_DIALOGUES);
    GF_TRY(att_of_descriptor(k, at, aprm, nullptr));
    return drnn_fwd(k);
}
extern "C" int ganffn_drnn_batch_bwd(const ganffn_drnn_cfg* c, const ganffn_drnn_att* at, int parties, int ndir, const float* const* d_e,
                                     const float* const* U, const int32_t* const* spk, const float* const* mval,
                                     const ganffn_drnn_params* prm, const ganffn_drnn_listener_params* lprm,
                                     const ganffn_drnn_att_params* aprm, const ganffn_drnn_grads* grd,
                                     const ganffn_drnn_listener_grads* lgrd, const ganffn_drnn_att_grads* agrd, float* const* dU,
                                     const float* const* alpha, const float* const* saved, float* const* workspace,
                                     const uint64_t* rng, uint64_t add, void* stream) {
    GF_CHECK_ARG(at, "drnn_batch_bwd: null attention descriptor");
    GF_TRY(check_parties(parties));
    DrnnCall k = drnn_call(c, ndir, rng, add, stream).inputs(U, spk, mval).cells(prm, lprm).grads(grd, lgrd)
                     .backward(d_e, dU, alpha, saved, workspace).limits(parties, GANFFN_MAX_DIALOGUES);
    GF_TRY(att_of_descriptor(k, at, aprm, agrd));
    return drnn_bwd(k);
}
