// batch.hip — the epoch loop's data movement with the corpus resident on the device (data.DeviceCorpus / data.DeviceLoader,
// artifacts.train_or_eval_model's device path):
//   ganffn_batch_gather : one launch builds a whole padded batch — every feature column and the speaker one-hots seq-first
//                         (S, B, width), umask (B, S) and label (B, S) — from the packed corpus ([N_utt x width] matrices,
//                         dialogues back to back, row0 = prefix offsets) and a device-side list of dialogue indices.
//   ganffn_epoch_record : one launch per step appends the step's predictions (argmax over classes, batch-major), labels and
//                         masks to the epoch buffers and stores the step's loss and its count of real utterances, so that the
//                         host reads an epoch's results once, after the last step.
// Both are bandwidth-sized copies: one workgroup per (step, dialogue) cell moves that cell's row of every column, 16 bytes per
// lane where the column width is a multiple of 4 (100, 512, 600, 300 — rows are then 16-byte aligned), one float per lane
// otherwise (the speaker one-hots: P = 2, 9).  Every output element is written exactly once (padding as zeros); no atomics.
// Whatever the index list or row0 hold, no lane reads or writes outside the operands: an index outside [0, n_dialogues) or a
// row range outside [0, n_rows] is an empty dialogue, a dialogue longer than S gives its first S rows.
#include "common.h"

namespace ganffn {

namespace {

constexpr int BATCH_MAX_S = 4096;

struct BatchCols {
    ganffn_batch_col c[GANFFN_BATCH_MAX_COLS];
};

__global__ __launch_bounds__(256) void batch_gather_kernel(const BatchCols cols, int n_cols, const int64_t* __restrict__ labels_src,
                                                           const int64_t* __restrict__ row0, int64_t n_rows,
                                                           const int32_t* __restrict__ idx, float* __restrict__ umask,
                                                           int64_t* __restrict__ label, int S, int B, int n_dialogues) {
    const int cell = blockIdx.x;                 // s * B + b: the row of every seq-first output
    const int s = cell / B, b = cell - s * B;
    const int d = idx[b];
    int64_t r0 = 0, len = 0;
    if (d >= 0 && d < n_dialogues) {
        const int64_t a = row0[d], e = row0[d + 1];
        if (a >= 0 && e >= a && e <= n_rows) {
            r0 = a;
            len = e - a;
        }
    }
    const bool real = (int64_t)s < len;          // (len > S: the rows past S are never asked for)
    const int64_t r = r0 + s;
    if (threadIdx.x == 0) {
        umask[(size_t)b * S + s] = real ? 1.f : 0.f;
        label[(size_t)b * S + s] = real ? labels_src[r] : 0;
    }
#pragma unroll
    for (int k = 0; k < GANFFN_BATCH_MAX_COLS; ++k) {
        if (k < n_cols) {
            const int w = cols.c[k].width;
            const float* src = cols.c[k].src + (size_t)r * w;
            float* dst = cols.c[k].dst + (size_t)cell * w;
            if ((w & 3) == 0) {
                float4* dst4 = reinterpret_cast<float4*>(dst);
                if (real) {              // (workgroup-uniform: src is only ever dereferenced for a real row)
                    const float4* src4 = reinterpret_cast<const float4*>(src);
                    for (int i = threadIdx.x; i < (w >> 2); i += blockDim.x) dst4[i] = src4[i];
                } else {
                    for (int i = threadIdx.x; i < (w >> 2); i += blockDim.x) dst4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else if (real) {
                for (int i = threadIdx.x; i < w; i += blockDim.x) dst[i] = src[i];
            } else {
                for (int i = threadIdx.x; i < w; i += blockDim.x) dst[i] = 0.f;
            }
        }
    }
}

// element i = b * S + s of the step, i in [0, B S): pred = the lowest class with the largest log-probability of token (s, b).
// Workgroup 0 also adds the step's masks — in a fixed order, and exactly whatever the order (zeros and ones below 2^24).
__global__ __launch_bounds__(256) void epoch_record_kernel(const float* __restrict__ log_prob, const int64_t* __restrict__ label,
                                                           const float* __restrict__ umask, const float* __restrict__ loss,
                                                           int64_t* __restrict__ preds_out, int64_t* __restrict__ labels_out,
                                                           float* __restrict__ masks_out, float* __restrict__ loss_out,
                                                           float* __restrict__ count_out, int S, int B, int C) {
    const int n = S * B;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int b = i / S, s = i - b * S;
        const float* lp = log_prob + ((size_t)s * B + b) * C;
        float best = lp[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = lp[c];
            if (v > best) {
                best = v;
                arg = c;
            }
        }
        preds_out[i] = arg;
        labels_out[i] = label[i];
        masks_out[i] = umask[i];
    }
    if (blockIdx.x == 0) {
        __shared__ float red[256];
        float acc = 0.f;
        for (int j = threadIdx.x; j < n; j += 256) acc += umask[j];
        red[threadIdx.x] = acc;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            count_out[0] = red[0];
            loss_out[0] = loss[0];
        }
    }
}

}  // namespace
}  // namespace ganffn

using namespace ganffn;

extern "C" int ganffn_batch_gather(const ganffn_batch_col* cols, int n_cols, const int64_t* labels_src, const int64_t* row0,
                                   int64_t n_rows, const int32_t* idx, float* umask, int64_t* label, int S, int B, int n_dialogues,
                                   void* stream) {
    GF_CHECK_ARG(n_cols >= 1 && n_cols <= GANFFN_BATCH_MAX_COLS, "batch_gather: n_cols=%d (1 .. %d columns)", n_cols,
                 GANFFN_BATCH_MAX_COLS);
    GF_CHECK_ARG(S >= 1 && S <= BATCH_MAX_S && B >= 1 && B <= GANFFN_MAX_DIALOGUES && n_dialogues >= 1 && n_rows >= 1,
                 "batch_gather: S=%d B=%d n_dialogues=%d n_rows=%lld (1 <= S <= %d, 1 <= B <= %d, at least one dialogue and one row)", S,
                 B, n_dialogues, (long long)n_rows, BATCH_MAX_S, GANFFN_MAX_DIALOGUES);
    GF_CHECK_ARG(cols && labels_src && row0 && idx && umask && label, "batch_gather: null pointer");
    BatchCols bc = {};
    for (int k = 0; k < n_cols; ++k) {
        GF_CHECK_ARG(cols[k].src && cols[k].dst, "batch_gather: column %d: null pointer", k);
        GF_CHECK_ARG(cols[k].width >= 1 && cols[k].width <= 65536, "batch_gather: column %d: width=%d (1 .. 65536)", k, cols[k].width);
        GF_CHECK_ARG((cols[k].width & 3) != 0 || (aligned16(cols[k].src) && aligned16(cols[k].dst)),
                     "batch_gather: column %d: a width that is a multiple of 4 needs 16-byte aligned buffers", k);
        bc.c[k] = cols[k];
    }
    hipLaunchKernelGGL(batch_gather_kernel, dim3(S * B), dim3(256), 0, (hipStream_t)stream, bc, n_cols, labels_src, row0, n_rows, idx,
                       umask, label, S, B, n_dialogues);
    GF_LAUNCH_CHECK();
    return 0;
}

extern "C" int ganffn_epoch_record(const float* log_prob, const int64_t* label, const float* umask, const float* loss, int S, int B,
                                   int C, int64_t* preds_out, int64_t* labels_out, float* masks_out, int64_t offset, int64_t capacity,
                                   float* loss_out, float* count_out, int step, int n_steps, void* stream) {
    GF_CHECK_ARG(S >= 1 && S <= BATCH_MAX_S && B >= 1 && B <= GANFFN_MAX_DIALOGUES && C >= 1 && C <= 16,
                 "epoch_record: S=%d B=%d C=%d (1 <= S <= %d, 1 <= B <= %d, 1 <= C <= 16)", S, B, C, BATCH_MAX_S, GANFFN_MAX_DIALOGUES);
    GF_CHECK_ARG(log_prob && label && umask && loss && preds_out && labels_out && masks_out && loss_out && count_out,
                 "epoch_record: null pointer");
    const int64_t n = (int64_t)S * B;
    GF_CHECK_ARG(offset >= 0 && capacity >= n && offset <= capacity - n && step >= 0 && step < n_steps,
                 "epoch_record: offset=%lld + %lld elements outside the epoch buffers of %lld, or step=%d outside [0, %d)",
                 (long long)offset, (long long)n, (long long)capacity, step, n_steps);
    hipLaunchKernelGGL(epoch_record_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, log_prob, label, umask,
                       loss, preds_out + offset, labels_out + offset, masks_out + offset, loss_out + step, count_out + step, S, B, C);
    GF_LAUNCH_CHECK();
    return 0;
}
