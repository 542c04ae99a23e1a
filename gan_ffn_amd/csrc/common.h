// common.h — shared device/host helpers for libganffn (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>
#include <type_traits>

#include "../../include/ganffn.h"

// Lab instrumentation (in-kernel time stamps and their setters) exists only in lab builds (`make LAB=1` ->
// lib/libganffn_lab.so, selected by tools/lab scripts through GANFFN_LIB); the product library compiles none of it.
#ifdef GANFFN_LAB
#define GF_LAB_ONLY(...) __VA_ARGS__
#else
#define GF_LAB_ONLY(...)
#endif

namespace ganffn {

// The library's only mutable process state besides the per-(kernel, device) "LDS opt-in done" masks: ONE word, the A/B mode
// mask of ganffn_debug_set_ffn_mode (include/ganffn.h lists the bits; default 0 = the product path).  It is a relaxed atomic —
// a setter racing with a launch makes that launch take either path, never a torn mixture of switches — and every entry
// point / launcher takes ONE snapshot (`const Mode md = mode();`) and decides from it.
struct Mode {
    uint32_t bits;
    // (bits 0, 7 and 22 selected the fused feed-forward kernels ffn.hip / ffn3.hip until round 5: measured slower in the step three
    //  times over, removed from the product — history + DESIGN.md section 3; the bits are reserved and ignored)
    bool rc_off() const { return bits & 2u; }                       // bit 1: separate GEMM + LayerNorm launches instead of rowchain.hip
    bool n100_off() const { return bits & 4u; }                     // bit 2: generic tiles instead of gemm_n100.hip
    bool tn100_off() const { return bits & 8u; }                    // bit 3: generic tiles instead of gemm_tn100.hip
    bool tn100_in_kernel_sum() const { return bits & 16u; }         // bit 4: last-arriver slab sum (measured slower)
    bool dhead_off() const { return bits & 32u; }                   // bit 5: discriminator head as separate launches
    bool pe_off() const { return bits & 64u; }                      // bit 6: positional encoding and layer 0's in-proj as two launches
    int n100_force_splits() const { return (int)((bits >> 8) & 0xFFu); }     // bits 8..15 (lab): K-chunk count of gemm_n100
    int tn100_force_splits() const { return (int)((bits >> 16) & 0xFu); }    // bits 16..19 (lab): token-chunk count of tn100
    int n100_force_kw() const { const int k = (int)((bits >> 20) & 3u); return k == 3 ? 2 : k; }   // bits 20..21 (lab)
    bool n100_pad7() const { return bits & (1u << 23); }            // bit 23: padded seventh tile instead of the 4x4x1 tail
    bool outproj_nosplit() const { return bits & (1u << 24); }      // bit 24: the wide out-proj unsplit
    bool mask_float() const { return bits & (1u << 25); }           // bit 25: linear2 dgrad reads the saved activation, not the bits
    bool adam_slabs_off() const { return bits & (1u << 28); }       // bit 28: tn100 slabs through the reduce launch (round 4's form)
};
extern std::atomic<uint32_t> g_mode_word;
inline Mode mode() { return Mode{g_mode_word.load(std::memory_order_relaxed)}; }

// ---------------------------------------------------------------------------------------
// error reporting (thread-local message, int return codes; no exceptions across the ABI)
// ---------------------------------------------------------------------------------------
char* err_buf();
int fail(int code, const char* fmt, ...);

#define GF_CHECK_ARG(cond, ...)                         \
    do {                                                \
        if (!(cond)) return ::ganffn::fail(-1, __VA_ARGS__); \
    } while (0)

#define GF_LAUNCH_CHECK()                                                              \
    do {                                                                               \
        hipError_t e__ = hipGetLastError();                                            \
        if (e__ != hipSuccess)                                                         \
            return ::ganffn::fail((int)e__, "%s:%d launch failed: %s", __FILE__, __LINE__, \
                                  hipGetErrorString(e__));                             \
    } while (0)

#define GF_HIP(expr)                                                                                \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return ::ganffn::fail((int)e__, "%s:%d %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
    } while (0)

#define GF_TRY(expr)              \
    do {                          \
        int r__ = (expr);         \
        if (r__ != 0) return r__; \
    } while (0)

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// Opt a kernel in to more than 48 KiB of dynamic LDS: once per (kernel, device, host thread), not on every launch.
// KERN is the kernel itself (a non-type template argument), so every instantiation has its own flag word.
template <auto KERN>
static inline int lds_optin(size_t lds, const char* what) {
    if (lds <= 48 * 1024) return 0;
    static thread_local uint64_t done_mask = 0;       // one bit per device ordinal
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return ::ganffn::fail((int)e, "%s: hipGetDevice failed: %s", what, hipGetErrorString(e));
    if (dev < 64 && ((done_mask >> dev) & 1u)) return 0;
    e = hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return ::ganffn::fail((int)e, "%s: hipFuncSetAttribute failed: %s", what, hipGetErrorString(e));
    if (dev < 64) done_mask |= uint64_t(1) << dev;
    return 0;
}

// ---------------------------------------------------------------------------------------
// buffer loads / stores: a 128-bit descriptor in scalar registers + a 32-bit byte offset per lane + a scalar byte offset —
// no 64-bit per-lane address arithmetic (fp32 MFMAs share the vector ALU: every VALU instruction next to them costs MFMA time,
// and hipcc's 64-bit address temporaries alias load destinations and bring low s_waitcnt vmcnt to the top of K-loop steps:
// DESIGN.md section 0d rows 2c / 2d).  The hardware range check covers the LANE offset only (not the scalar one); callers
// that pass bytes = 0xFFFFFFFF clamp their offsets into the operand themselves, and the launchers refuse operands >= 4 GiB.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 buf_load_f4(__amdgpu_buffer_rsrc_t rs, uint32_t voff_bytes, uint32_t soff_bytes) {
    typedef unsigned int u32x4_ __attribute__((ext_vector_type(4)));
    const u32x4_ v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff_bytes, (int)soff_bytes, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ void buf_store_u32(__amdgpu_buffer_rsrc_t rs, uint32_t voff_bytes, uint32_t soff_bytes, uint32_t v) {
    __builtin_amdgcn_raw_buffer_store_b32(v, rs, (int)voff_bytes, (int)soff_bytes, 0);
}

// ---------------------------------------------------------------------------------------
// dropout sites (mirror of oracle/ganffn_oracle.py SITE_*)
// ---------------------------------------------------------------------------------------
enum : uint32_t {
    SITE_PE = 0,
    SITE_HEAD0 = 1,
    SITE_HEAD1 = 2,
    SITE_HEAD2 = 3,
    SITE_HEAD3 = 4,
    SITE_LAYER0 = 16,  // + 4*layer + {0 attn-prob, 1 post-attn, 2 ffn-mid, 3 post-ffn}
};

// ---------------------------------------------------------------------------------------
// Philox4x32-10 (contract: oracle/philox.py)
// ---------------------------------------------------------------------------------------
struct DropCtx {
    uint32_t k0, k1;   // seed lo/hi
    uint32_t o0, o1;   // offset lo/hi
    uint32_t site;
    uint32_t thr;      // drop iff word < thr
    float scale;       // 1/(1-p)
    int on;
};

__host__ __device__ inline uint32_t drop_threshold(float p) {
    if (p <= 0.f) return 0u;
    double t = (double)p * 4294967296.0;
    if (t >= 4294967295.0) return 0xFFFFFFFFu;
    return (uint32_t)t;  // floor
}

__device__ __forceinline__ DropCtx make_drop(const uint64_t* rng, uint64_t add, uint32_t site, float p, int on) {
    DropCtx d;
    d.on = on && (p > 0.f);
    d.site = site;
    d.thr = drop_threshold(p);
    d.scale = d.on ? 1.0f / (1.0f - p) : 1.0f;
    uint64_t seed = 0, off = 0;
    if (d.on) {
        seed = rng[0];
        off = rng[1] + add;
    }
    d.k0 = (uint32_t)seed;
    d.k1 = (uint32_t)(seed >> 32);
    d.o0 = (uint32_t)off;
    d.o1 = (uint32_t)(off >> 32);
    return d;
}

// k0 / k1 (the seed halves) MUST be wave-uniform: they are scalar operands of the round's xor (every caller takes them from
// make_drop, which reads the generator state through scalar loads); the counter words c0..c3 are per lane.
__device__ __forceinline__ void philox4(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                        uint32_t k1, uint32_t (&out)[4]) {
    // one v_mad_u64_u32 per 32x32->64 product (hipcc would emit v_mul_hi_u32 + v_mul_lo_u32, both quarter-rate)
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        uint64_t p0, p1, cy0, cy1;
        asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(p0), "=s"(cy0) : "s"(M0), "v"(c0));
        asm("v_mad_u64_u32 %0, %1, %2, %3, 0" : "=v"(p1), "=s"(cy1) : "s"(M1), "v"(c2));
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
        const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        // hi ^ c ^ k in ONE instruction: gfx950's v_bitop3_b32 with the truth table of a 3-input xor (0x96); hipcc emits two
        // v_xor_b32 (gfx9 has no v_xor3) — 40 instead of 20 per call, and every one of them is paid in MFMA time in the GEMM
        // epilogues.  The round key is wave-uniform (make_drop reads it through scalar loads): the one scalar operand allowed.
        uint32_t n0, n2;
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n0) : "v"(hi1), "v"(c1), "s"(k0));
        asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(n2) : "v"(hi0), "v"(c3), "s"(k1));
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// keep-multipliers (0 or 1/(1-p)) for the 4 consecutive rows 4*rg .. 4*rg+3 of column c in a [R x C] tensor
__device__ __forceinline__ void drop_mult4(const DropCtx& d, uint32_t rowgroup, uint32_t C, uint32_t c, float (&m)[4]) {
    if (!d.on) {
        m[0] = m[1] = m[2] = m[3] = 1.f;
        return;
    }
    uint32_t w[4];
    philox4(rowgroup * C + c, d.site, d.o0, d.o1, d.k0, d.k1, w);
#pragma unroll
    for (int i = 0; i < 4; ++i) m[i] = (w[i] >= d.thr) ? d.scale : 0.f;
}

// single element (row r, col c) — used by row-wise kernels; 4x the Philox work of drop_mult4
__device__ __forceinline__ float drop_mult1(const DropCtx& d, uint32_t r, uint32_t C, uint32_t c) {
    if (!d.on) return 1.f;
    uint32_t w[4];
    philox4((r >> 2) * C + c, d.site, d.o0, d.o1, d.k0, d.k1, w);
    const uint32_t x = (r & 3) == 0 ? w[0] : (r & 3) == 1 ? w[1] : (r & 3) == 2 ? w[2] : w[3];
    return (x >= d.thr) ? d.scale : 0.f;
}

// ---------------------------------------------------------------------------------------
// math
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_f(float x) {  // nn.GELU() exact (erf) form
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}
__device__ __forceinline__ float gelu_grad_f(float x) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * __expf(-0.5f * x * x);
    return cdf + x * pdf;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------------------
// internal launchers shared between translation units
// ---------------------------------------------------------------------------------------
enum Epilogue : int {
    EPI_NONE = 0,          // C = acc (+bias)
    EPI_RELU_DROP = 1,     // C = drop(relu(acc+bias))                       (FFN linear1)
    EPI_DROP_GELU = 2,     // aux = drop(acc+bias); C = gelu(aux)            (head fc1/fc2)
    EPI_MASK_POS = 3,      // C = acc * (aux > 0 ? mscale : 0)               (FFN dgrad through relu+dropout)
    EPI_GELU_BWD_DROP = 4, // C = drop_bwd(acc) * gelu'(aux)  i.e. d(pre-dropout) of u=drop(v), a=gelu(u) chain
    EPI_GELU_BWD = 5,      // C = acc * gelu'(aux)
    EPI_GELU_BWD_DROP0 = 6 // C = acc * dropmult * gelu'(aux): aux = pre-gelu x, out=drop(gelu(x)) (gen head site 0)
};

struct EpiArgs {
    const float* bias = nullptr;  // [N]
    float* aux_out = nullptr;     // [M x N] (EPI_DROP_GELU)
    const float* aux_in = nullptr;// [M x N]
    float mscale = 1.f;           // EPI_MASK_POS
    // 1-bit form of the ReLU / dropout pattern of a [M x N] activation: EPI_RELU_DROP writes it (when non-null) beside the
    // activation, EPI_MASK_POS reads it INSTEAD of aux_in (when non-null).  Word ((m / 32) * N + n) * 2 + h, h = (m / 4) & 1,
    // holds rows 32 (m / 32) + 4 h + (i & 3) + 8 (i >> 2) of column n in bit i — one lane's 16 accumulator registers of a
    // 32 x 32 MFMA tile; epi_mask_words(M, N) uint16 words.
    uint16_t* mask_out = nullptr;
    const uint16_t* mask_in = nullptr;
    float p = 0.f;                // dropout prob
    uint32_t site = 0;
    const uint64_t* rng = nullptr;
    uint64_t rng_add = 0;
    int train = 0;
};

inline long epi_mask_words(long M, long N) { return ((M + 31) / 32) * N * 2; }

// second row segment of a two-segment NT product (EPI_NONE, also split-K, or EPI_RELU_DROP): its input rows, output (slabs
// at the same stride), pattern words (may be null) and train flag.  The n100 kernel reads A and C only.
struct GemmSeg1 {
    const float* A; float* C; uint16_t* mask_out; int train;
};
//   NT  C[MxN]  = A[MxK] * W[NxK]^T   NN  C[MxN] = A[MxK] * B[KxN]   TN  C[MxN] += At[KxM]^T * B[KxN], colsum[M] += sum_k At[k][m]
enum GemmLayout : int { GEMM_NT = 0, GEMM_NN = 1, GEMM_TN = 2 };
// who decides how many K slabs an EPI_NONE product writes (gemm.hip, "split policies"); the caller gives the cap and the stride
enum GemmSlabRule : int {
    SLABS_AUTO = 0,      // the [T x K] x [K x 100] kernel (gemm_n100.hip) with its own chunk rule where it takes the shape and
                         // Mode::n100_off() is clear, else the generic kernel split by gemm_splitk_factor
    SLABS_GENERIC,       // the generic kernel split by gemm_splitk_factor, whatever the shape (ganffn_gemm_hook)
    SLABS_INPROJ_DGRAD,  // the generic kernel split by gemm_inproj_dgrad_splits
    SLABS_N100,          // gemm_n100.hip whatever the mode word says; a shape it does not take is refused (ganffn_gemm_n100)
};
// One dense product.  Every caller fills one and runs gemm() on it; what a caller does not have stays null / 0.  The struct lives
// on the caller's stack.  Deterministic in every form: split products write slabs that the consumer (NT / NN) or an ordered
// reduce launch (TN) adds in split order; no atomics.
struct GemmCall {
    GemmLayout layout;
    const float* A; int lda;       // NT / NN: [M x K];  TN: At [K x M]
    const float* B; int ldb;       // NT: W [N x K];  NN / TN: [K x N]
    float* C; int ldc;
    int M, N, K;
    int epi; EpiArgs ea;           // NT / NN
    hipStream_t st;
    // K slabs (EPI_NONE, NT / NN): slab z = the partial product of K chunk z at C + z * slab_stride, at most slab_cap of them, the
    // count written goes to *n_slabs.  slab_cap 0 = not asked for: one product at C.
    GemmSlabRule slab_rule; int slab_cap; long slab_stride; int* n_slabs;
    bool has_seg1; GemmSeg1 seg1;  // NT: the same product for a second segment of M rows in the same launch
    float* colsum; float* part_ws; long part_floats;   // TN: column sums of At (or null), partial-slab workspace (or null)
    GemmCall& ld(int lda_, int ldb_, int ldc_) { lda = lda_; ldb = ldb_; ldc = ldc_; return *this; }
    GemmCall& epilogue(int epi_, const EpiArgs& ea_) { epi = epi_; ea = ea_; return *this; }
    // EPI_NONE's two operands, for the callers that have nothing else to say about the epilogue: C = acc + bias[N] + residual[M x N]
    GemmCall& bias(const float* b) { ea.bias = b; return *this; }
    GemmCall& residual(const float* r) { ea.aux_in = r; return *this; }         // leading dimension ldc; may be C itself
    GemmCall& slabs(int cap, long stride, int* n, GemmSlabRule rule = SLABS_AUTO) {
        slab_cap = cap; slab_stride = stride; n_slabs = n; slab_rule = rule;
        return *this;
    }
    GemmCall& pair(const GemmSeg1& s) { seg1 = s; has_seg1 = true; return *this; }
    GemmCall& sums(float* colsum_) { colsum = colsum_; return *this; }
    GemmCall& tn_workspace(float* ws, long floats) { part_ws = ws; part_floats = floats; return *this; }
    GemmCall& on(hipStream_t st_) { st = st_; return *this; }
};
// the three layouts with the dense leading dimensions almost every caller has; .ld() for the rest
static inline GemmCall gemm_call(GemmLayout layout, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K) {
    GemmCall k{};
    k.layout = layout; k.A = A; k.lda = lda; k.B = B; k.ldb = ldb; k.C = C; k.ldc = ldc; k.M = M; k.N = N; k.K = K; k.epi = EPI_NONE;
    return k;
}
static inline GemmCall gemm_nt(const float* A, const float* W, float* C, int M, int N, int K) { return gemm_call(GEMM_NT, A, K, W, K, C, N, M, N, K); }
static inline GemmCall gemm_nn(const float* A, const float* B, float* C, int M, int N, int K) { return gemm_call(GEMM_NN, A, K, B, N, C, N, M, N, K); }
static inline GemmCall gemm_tn(const float* At, const float* B, float* C, int M, int N, int K) { return gemm_call(GEMM_TN, At, M, B, N, C, N, M, N, K); }
// What gemm_plan (gemm.hip) decides for a call: a pure host function of the call and the mode word, no HIP call inside.
enum GemmFamily : int {
    GEMM_GENERIC = 0,    // gemm_kernel / gemm_pair_kernel, 64 x 64 x 16 tiles
    GEMM_SHORTK,         // the same code under its K <= 128 symbol
    GEMM_WRES,           // gemm_wres_kernel / gemm_wres_pair_kernel: K = 100, N >= 1024, weight fragments resident in registers
    GEMM_N100,           // gemm_n100.hip
    GEMM_TN_ACC,         // gemm_kernel<MODE_TN>: owner-adds-in-place, or (splits > 1) partial slabs + tn_reduce_kernel
};
enum N100Variant : int { N100_KW2_TAIL4 = 0, N100_KW2_PAD7, N100_KW1_PAD7 };   // waves per token group along K; features 96..99
constexpr int N100_BM = 64, N100_BK = 32;       // gemm_n100.hip's token tile and K tile
struct GemmPlan {
    GemmFamily family; bool pair;
    int epi;             // the kernel's epilogue (EPI_GELU_BWD_DROP0 runs EPI_GELU_BWD_DROP's code)
    int splits, kchunk;  // K chunks (= slabs written) and the chunk length; 1 and K when not split
    long slab_stride;    // what the kernel gets: the call's when split, 0 when not;  TN: floats per partial slab
    dim3 grid;           // GEMM_WRES: (column panels, token tiles of all segments); its launcher cuts the tiles down to what is resident
    N100Variant n100;
};
// gemm.hip: check the call (every refusal of the dense paths, before any launch), plan it (kernel family and variant, K split,
// grid), launch
int gemm(const GemmCall& k);
// floats of partial-slab workspace a split TN product of this shape can use (0: it will not split)
long gemm_tn_part_floats(int M, int N, int K);

// skinny products (dialogue_rnn.hip): M <= 32 rows of A (dialogues) against a weight matrix, up to 8 problems per launch — one
// link of a recurrence's launch chain (DialogueRNN cells, lstm.hip's recurrent products)
struct SkinnyProb {
    const float* A; int lda;      // [M x K]
    const float* W; int ldw;      // NT: [N x K];  NN: [K x N]
    const float* Cin; int ldcin;  // optional addend [M x N]
    const float* Cin2;            // optional second addend [M x N], leading dimension ldc (may be C itself: in-place +=)
    const float* bias;            // optional [N]
    float* C; int ldc;            // [M x N]
    int M, N, K;
};
struct SkinnyGroup {
    SkinnyProb p[8];
};
// nn = false: C = A W^T (+ Cin + Cin2 + bias), W [N x K];  nn = true: C = A W (+ Cin + Cin2), W [K x N]
int launch_skinny(const SkinnyGroup& grp, int nprob, bool nn, hipStream_t st);

// grouped wgrad: n independent TN problems in one launch
struct TnDesc {
    const float* At; int lda;
    const float* B; int ldb;
    float* C; int ldc;
    float* colsum;
    int M, N, K;
};
// part_ws (optional, gemm_tn_grouped_part_floats() floats): when the group has too few output tiles to load every CU
// evenly, the token range is split over 2..8 workgroups per tile; each writes its partial tile to the workspace and one
// grouped reduce launch adds the partials in split order (deterministic).  Without a workspace: one owner per tile.
// Unreduced weight gradients of a d_model-100 pass (round 5; single-GPU step): in  — grad_base / range_floats: the gradient
// slab region every problem's C and colsum lie in (densely, ldc == N); out — n_parts token chunks were computed: chunk 0 WROTE
// (not added) its partial gradients into the slab region itself, chunk z >= 1 into part + (z - 1) * part_stride, shaped like the
// region.  ganffn_adam_step_parts adds them in chunk order: the sum the reduce launch would have formed, bit for bit.
struct TnSlabs {
    float* grad_base; long range_floats;
    int n_parts; float* part; long part_stride;
};
int launch_gemm_tn_grouped(const TnDesc* d, int n, hipStream_t st, float* part_ws = nullptr, long part_floats = 0, TnSlabs* slabs = nullptr);
// gemm_tn100.hip: the same for groups whose every problem has a 100-wide dimension (d_model-100 encoder passes), on
// 112-wide 16x16x4 tiles; needs the partial-slab workspace
bool tn100_supported(const TnDesc* d, int n);
int launch_gemm_tn100_grouped(const TnDesc* d, int n, hipStream_t st, float* part_ws, long part_floats, TnSlabs* slabs = nullptr);
long gemm_tn_grouped_part_floats();

// lse [B*H x S]: log-sum-exp of every score row, written by the forward (may be NULL: not kept) and, together with the
// forward's output o, read by the backward of the small-head kernels (attention16.hip); the head_dim 60/64 kernels
// (attention.hip) recompute the softmax statistics and ignore both.
// keep [B*H x ATTN_KEEP_WORDS] (or NULL): the dropout keep bits of the probability matrix, written by a train-mode
// small-head forward and read back by its backward instead of recomputing the Philox calls (attention16.hip; the
// head_dim 60/64 kernels ignore it).  Same bits either way.
constexpr int ATTN_KEEP_WORDS = 28 * 16;
// one batch of a forward pass: its buffers and train flag
struct AttnSeg {
    const float* qkv; float* o; float* lse; uint32_t* keep; int train;
};
// One call of the attention core.  Every caller (the ganffn_attention_* entry points, encoder_fwd_walk and encoder_bwd in api.hip)
// fills one and runs attention_fwd or attention_bwd on it; what a caller does not have stays null / 0.
// key_len (optional, device int32 [B]): dialogue b attends over keys j < clamp(key_len[b], 1, S) only (probability 0 past it,
// dK and dV rows written as zeros); null = all S keys, today's bits.  With a second segment the lengths serve both batches (the
// same B dialogues).
// flags: GANFFN_ATTN_CAUSAL = query i attends to keys j <= i as well (key limit min(n, i + 1)); kernels of their own, instantiated
// only in the form with lengths (a null key_len reads as S there), for one segment and for two.  0 = the launches and bits without it.
struct AttnCall {
    int S, B, E, H; float p; uint32_t site; const uint64_t* rng; uint64_t add; hipStream_t st;
    const int32_t* key_len; uint32_t flags;
    AttnSeg seg[2]; int nseg;                          // forward; nseg 2: a second batch of the same shape in the same launch
    const float* qkv; const float* o; const float* lse; const uint32_t* keep; const float* d_o; float* d_qkv; int train;   // backward
    bool causal() const { return (flags & GANFFN_ATTN_CAUSAL) != 0; }
    AttnCall& mask(const int32_t* key_len_, uint32_t flags_) { key_len = key_len_; flags = flags_; return *this; }
    AttnCall& forward(const AttnSeg& s) { seg[0] = s; nseg = 1; return *this; }
    AttnCall& pair(const AttnSeg& s) { seg[1] = s; nseg = 2; return *this; }
    AttnCall& backward(const float* qkv_, const float* o_, const float* lse_, const uint32_t* keep_, const float* d_o_, float* d_qkv_, int train_) {
        qkv = qkv_; o = o_; lse = lse_; keep = keep_; d_o = d_o_; d_qkv = d_qkv_; train = train_;
        return *this;
    }
};
static inline AttnCall attn_call(int S, int B, int E, int H, float p, uint32_t site, const uint64_t* rng, uint64_t add, hipStream_t st) {
    AttnCall k{};
    k.S = S; k.B = B; k.E = E; k.H = H; k.p = p; k.site = site; k.rng = rng; k.add = add; k.st = st;
    return k;
}
// attention.hip: check the call (every refusal of the family is there, before any launch), then the 16-row kernels where
// attn16_supported() says so, else the 32-row ones
int attention_fwd(const AttnCall& k);
int attention_bwd(const AttnCall& k);
// f(std::true_type{}) or f(std::false_type{}): a run-time fact as a template flag of the kernel that f launches
template <class F>
static inline int with_flag(bool on, F&& f) { return on ? f(std::true_type{}) : f(std::false_type{}); }
// the key length of dialogue b inside a kernel instantiated for lengths: one scalar load per workgroup (b is workgroup-uniform),
// clamped here so that a bad length can neither empty a softmax nor move a read out of range
__device__ __forceinline__ int attn_key_len(const int32_t* __restrict__ key_len, int b, int S) {
    return key_len ? min(max(key_len[b], 1), S) : S;
}
// attention16.hip: which shapes the 16-row kernels take, and their launches for a call that attention_fwd / attention_bwd has
// checked and attn16_supported() accepts: CAUSAL = k.causal(), defined in attention16_causal.hip for true and in attention16.hip
// for false
bool attn16_supported(int E, int H, int S);
template <bool CAUSAL> int attn16_fwd(const AttnCall& k);
template <bool CAUSAL> int attn16_bwd(const AttnCall& k);

// stream.hip — streaming causal attention over per-layer K/V caches (layout: include/ganffn.h, "streaming"): per row i, slot
// s = slot[i] at position t = pos[s], append the row's K / V at t and attend with its Q over keys 0 .. t; a row with s outside
// [0, capacity) or t outside [0, max_len) gives a zero row and touches nothing
int launch_stream_attention(const float* qkv, float* cache_layer, const int32_t* slot, const int32_t* pos, float* o, int n,
                            int capacity, int max_len, int E, int H, hipStream_t st);
// x0[i] = x[i] + pe[pos[slot[i]]] (eval mode); a skipped row gives a zero row
int launch_stream_pe(const float* x, const float* pe, const int32_t* slot, const int32_t* pos, float* x0, int n, int capacity,
                     int max_len, int E, hipStream_t st);
// the chunk form (ganffn_stream_attention_chunk): qkv [m][n][3E] and o [m][n][E] time-major; chunk i holds c = count[i] new rows
// of slot s = slot[i] at positions t .. t+c-1, t = pos[s]; row j < c attends over cached keys 0 .. t-1 and the chunk's keys
// 0 .. j, and the rows' K / V go to the cache at t .. t+c-1.  A chunk with s outside [0, capacity), t < 0, c < 0, c > m or
// t + c > max_len is skipped whole (cache untouched); o rows j >= c are zeros for every chunk, qkv rows j >= c are never read
int launch_stream_attention_chunk(const float* qkv, float* cache_layer, const int32_t* slot, const int32_t* count,
                                  const int32_t* pos, float* o, int n, int m, int capacity, int max_len, int E, int H,
                                  hipStream_t st);
// x0[j, i] = x[j, i] + pe[pos[slot[i]] + j] for j < count[i] of a chunk that is not skipped; every other row is a zero row
int launch_stream_pe_chunk(const float* x, const float* pe, const int32_t* slot, const int32_t* count, const int32_t* pos,
                           float* x0, int n, int m, int capacity, int max_len, int E, hipStream_t st);
// what encoder_fwd_walk (api.hip) needs to run a stack as a streaming step: layer l's cache is cache + l * layer_stride.
// count (or null = the one-row step) and m: the chunk form over m * n time-major rows (ganffn_encoder_stream_extend)
struct StreamArgs {
    const int32_t* slot; const int32_t* pos; float* cache; int64_t layer_stride; int capacity, max_len;
    const int32_t* count = nullptr; int m = 1;
};

int launch_dropout_bwd_inplace(float* dx, int R, int C, float p, uint32_t site, const uint64_t* rng, uint64_t add,
                               int train, hipStream_t st);
int launch_dropout(const float* x, float* out, int R, int C, float p, uint32_t site, const uint64_t* rng,
                   uint64_t add, int train, hipStream_t st);
// kernel argument of the two-segment LayerNorm forward (elementwise.hip): the second row segment's operands and train flag
struct LnFwdSeg1 {
    const float* x; const float* y; float* out; float* xhat; float* rstd; int train;
};
int launch_add_inplace(float* a, const float* b, int64_t n, hipStream_t st);

// gemm_n100.hip — [T x K] x [K x 100] with a long K on 16x16x4 MFMAs (112-wide feature tile), K cut into output slabs.  Reached
// through gemm(): gemm.hip's check and plan decide (its chunk rule, n100_splits, stands there beside the other split rules),
// launch_gemm_n100 launches what the plan says.
bool n100_supported(int N, int K);
int launch_gemm_n100(const GemmCall& k, const GemmPlan& p);

// rowchain.hip — d_model 100: out-proj + residual + dropout + LayerNorm1, LayerNorm2 + the next layer's in-proj, and the
// mirror-image backward chains, one kernel each (16 token rows per workgroup)
bool rc_supported(int E);
long rc_pack_floats();          // floats of one layer's transposed {in-proj, out-proj} weights (backward)
int rc_blocks(int T);           // workgroups = partial rows of the LayerNorm parameter gradients per launch
int launch_rc_pack(const float* params, long layer_stride, long off_in, long off_out, float* wt, int nl, hipStream_t st);
// kernel argument of the two-segment rowchain forward: the second row segment's operands (named as in the kernel: pre_a = attn_o,
// y = slabs / PE table, x = residual, post_out = qkv) and train flag
struct RcFwdSeg1 {
    const float* pre_a; const float* y; const float* x;
    float* out; float* xhat; float* rstd; float* post_out;
    int train;
};
int ln_bwd_blocks(int T);       // the same for the plain LayerNorm backward (elementwise.hip)

// ---------------------------------------------------------------------------------------
// Row stages: the token-local steps of an encoder pass around the two LayerNorms and the positional encoding.
//   forward   [front GEMM: y = attn_o . pre_w^T + pre_b]  ->  ROW_LN: out = LayerNorm(x + dropout(y)) | ROW_PE: out = dropout(x + pe[s])
//             ->  [trailing in-proj: post_out = out . post_w^T + post_b]
//   backward  (ROW_LN) d = (sum of the slabs of d_out | d_qkv . w_in_t^T) + addend  ->  dz, dy = dz * dropout multiplier, the parameter
//             gradients  ->  [d_attn = dy . wo_t^T]
// Every caller fills a RowCall and runs row_fwd or row_bwd on it (elementwise.hip); what a caller does not have stays null / 0.
// ---------------------------------------------------------------------------------------
// Which kernels run a stage: a pure function of the width and the mode word.
struct RowPlan {
    bool rowchain;       // the stage with its GEMMs is one rowchain.hip kernel (d_model 100) instead of separate launches
    bool head_fused;     // ... and so is the ROW_PE stage at the head of a stack
    // partial-sum blocks (rows of gpart, 2 E floats each) a backward launch writes
    int blocks(int T) const { return rowchain ? rc_blocks(T) : ln_bwd_blocks(T); }
};
// streaming: the head of the stack is the streaming step's own gather (stream.hip), never a row stage
static inline RowPlan row_plan(int E, const Mode md, bool streaming = false) {
    const bool rc = rc_supported(E) && !md.rc_off();
    return RowPlan{rc, rc && !md.pe_off() && !streaming};
}
// what a workspace must hold per backward launch, whichever mode word the pass will run under
static inline int row_blocks_any_plan(int T) {
    const int a = RowPlan{false, false}.blocks(T), b = RowPlan{true, true}.blocks(T);
    return a > b ? a : b;
}
enum RowKind : int { ROW_LN = 0, ROW_PE = 1 };
constexpr int LN_MAXSLAB = 16;   // slabs a LayerNorm kernel sums on the fly: the cap of every split rule that feeds one (api.hip MAX_SPLITS)
// one row segment of a forward stage: T rows with their own buffers and train flag
struct RowSeg {
    const float* attn_o;                      // the front GEMM's input rows [T x E]
    const float* y;                           // ROW_LN without a front GEMM: the slabs;  ROW_PE: the positional-encoding table
    const float* x;                           // residual input [T x E] (ROW_PE: the stack's input)
    float* out; float* xhat; float* rstd;     // xhat / rstd may be null (nothing kept for a backward)
    float* post_out;                          // the trailing in-proj's output [T x 3E]
    float* tmp;                               // slab scratch: where the separate-launch plan writes the front GEMM's slabs
    int train;
};
// the three forms a forward segment takes; what a form does not have stays null
static inline RowSeg pe_seg(const float* x_in, const float* pe, float* out, float* qkv, int train) {
    RowSeg s{};
    s.x = x_in; s.y = pe; s.out = out; s.post_out = qkv; s.train = train;
    return s;
}
static inline RowSeg ln_front_seg(const float* attn_o, float* tmp, const float* x, float* out, float* xhat, float* rstd, int train) {
    RowSeg s{};
    s.attn_o = attn_o; s.tmp = tmp; s.x = x; s.out = out; s.xhat = xhat; s.rstd = rstd; s.train = train;
    return s;
}
static inline RowSeg ln_slab_seg(const float* y, const float* x, float* out, float* xhat, float* rstd, float* qkv, int train) {
    RowSeg s{};
    s.y = y; s.x = x; s.out = out; s.xhat = xhat; s.rstd = rstd; s.post_out = qkv; s.train = train;
    return s;
}
// the LayerNorm parameter gradients still to be summed from per-block partial rows: row_bwd appends, launch_ln_param_reduce adds
struct LnRedRec { float* gw; float* gb; const float* part; int nblk; };
struct LnRedList { LnRedRec r[2 * 64]; int n = 0; };
struct RowCall {
    RowKind kind; int T, B, E; float eps, p; uint32_t site; const uint64_t* rng; uint64_t add; hipStream_t st;
    RowPlan plan;                                               // default: separate launches
    const float* gamma; const float* beta;                      // ROW_LN
    const float* pre_w; const float* pre_b; int pre_slab_cap;   // front GEMM (or null): W [E x E], bias, at most so many K slabs
    int nslab; long slab_stride;                                // slabs of y / d_out, summed on the fly (a front GEMM reports its own count)
    const float* post_w; const float* post_b;                   // trailing in-proj (or null): W [3E x E], bias
    RowSeg seg[2]; int nseg;                                    // forward; nseg 2: a second segment of T rows in the same launches
    // backward
    const float* d_out; const float* addend; const float* xhat; const float* rstd; float* dz; float* dy; int train;
    float* gw; float* gb; float* gpart; LnRedList* red;         // gpart null: one workgroup adds its sums to gw / gb itself
    const float* d_qkv; const float* w_in_t;                    // rowchain only: d_out is d_qkv . w_in_t^T (in-proj weight packed by rc_pack)
    const float* wo_t; float* d_attn;                           // rowchain only: d_attn = dy . wo_t^T (out-proj weight packed by rc_pack)
    RowCall& under(const RowPlan& p_) { plan = p_; return *this; }
    RowCall& norm(const float* gamma_, const float* beta_) { gamma = gamma_; beta = beta_; return *this; }
    RowCall& front(const float* w, const float* b, int slab_cap, long stride) { pre_w = w; pre_b = b; pre_slab_cap = slab_cap; slab_stride = stride; return *this; }
    RowCall& slabs(int n, long stride) { nslab = n; slab_stride = stride; return *this; }
    RowCall& inproj(const float* w, const float* b) { post_w = w; post_b = b; return *this; }
    RowCall& forward(const RowSeg& s) { seg[0] = s; nseg = 1; return *this; }
    RowCall& pair(const RowSeg& s) { seg[1] = s; nseg = 2; return *this; }
    RowCall& backward(const float* xhat_, const float* rstd_, const float* gamma_, float* dz_, float* dy_, int train_) {
        xhat = xhat_; rstd = rstd_; gamma = gamma_; dz = dz_; dy = dy_; train = train_;
        return *this;
    }
    RowCall& from(const float* d_out_, int n, long stride, const float* addend_) { d_out = d_out_; nslab = n; slab_stride = stride; addend = addend_; return *this; }
    RowCall& from_inproj(const float* d_qkv_, const float* w_in_t_, const float* addend_) { d_qkv = d_qkv_; w_in_t = w_in_t_; addend = addend_; d_out = nullptr; nslab = 0; return *this; }
    RowCall& outproj_dgrad(const float* wo_t_, float* d_attn_) { wo_t = wo_t_; d_attn = d_attn_; return *this; }
    RowCall& param_grads(float* gw_, float* gb_, float* gpart_, LnRedList* red_) { gw = gw_; gb = gb_; gpart = gpart_; red = red_; return *this; }
};
static inline RowCall row_call(RowKind kind, int T, int B, int E, float eps, float p, uint32_t site, const uint64_t* rng, uint64_t add, hipStream_t st) {
    RowCall k{};
    k.kind = kind; k.T = T; k.B = B; k.E = E; k.eps = eps; k.p = p; k.site = site; k.rng = rng; k.add = add; k.st = st; k.nslab = 1;
    return k;
}
// elementwise.hip: check the call (check_row_fwd / check_row_bwd: every refusal of the family, before any launch), then what the plan says — one
// rowchain launch (launch_rc_fwd / launch_rc_bwd, rowchain.hip), or the separate launches: gemm() into the segment's slab scratch,
// the LayerNorm or PE kernel over the slab count gemm() reported, gemm() for the in-proj.  row_bwd composes no GEMM: the products
// around a backward stage read other buffers and sit elsewhere in the launch order under the two plans (api.hip encoder_bwd).
int row_fwd(const RowCall& k);
int row_bwd(const RowCall& k);
int launch_rc_fwd(const RowCall& k);
int launch_rc_bwd(const RowCall& k);
// gw / gb += (overwrite: =, the caller did not zero them) the sums of every record's partial rows, in block order
int launch_ln_param_reduce(const LnRedList& list, int E, hipStream_t st, bool overwrite = false);
int launch_gelu_drop_fwd(const float* x, float* out, int R, int C, float p, uint32_t site, const uint64_t* rng,
                         uint64_t add, int train, hipStream_t st);

}  // namespace ganffn
