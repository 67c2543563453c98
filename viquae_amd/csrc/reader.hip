// reader.hip -- the answer-extraction head of MultiPassageBERT on gfx950 (the evaluation path of the reference's Reader,
// meerqat/train/trainee.py:742-824).  C ABI: include/meerqat_hip.h.
//
//   qa_head_kernel       logits = h . W^T + b for W [2, H] (BertForQuestionAnswering.qa_outputs), one wave per token row,
//                        the rows spread over the whole GPU: the head reads N*M*L*H*4 bytes (151 MB for 8 questions at
//                        L = 256) and is a pure stream; start and end logits are written as two planes
//   log_softmax_kernel   one workgroup per (question, start | end): nn.LogSoftmax over the question's M*L positions
//                        (meerqat/train/optim.py:42-87): logp = fl(fl(x - max) - logf(S)), S = sum expf(x - max) in fp32,
//                        per-thread partial sums of a few terms then a tree over the workgroup; p = expf(logp)
//   best_spans_kernel    one workgroup per question: get_best_spans (meerqat/models/qa.py:18-77) by brute force over the
//                        M*L*L candidates P[m,i,j] = fl(fl(s_i e_j) w_m) (i <= j; row 0 zeroed when cannot_be_first_token)
//
// Span selection is exact: a candidate is the 64-bit key (value bits << 32) | ~(m L^2 + i L + j).  For non-negative floats
// the bit pattern orders like the value (denormals included: nothing is flushed), so the largest key is the largest value
// with, among equal values, the lowest (passage, flat index) -- the reference's "first passage whose maximum is the largest,
// then the first flat argmax inside it".  Candidates below the diagonal and in the zeroed row are 0 and are not visited:
// candidate 0 of passage 0 (value 0, the lowest index of all) seeds every thread, which stands for all of them at once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/meerqat_hip.h"
#include "device_common.h"
#include "host_check.h"

namespace {

using namespace mq_dev;

constexpr int HEAD_WAVES = 4;  // token rows per head workgroup (one per wave)
constexpr int RT = 1024;       // threads of a log-softmax / span workgroup
constexpr int RW = RT / 64;

__global__ __launch_bounds__(HEAD_WAVES * 64) void qa_head_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                                  const float* __restrict__ b, float* __restrict__ start,
                                                                  float* __restrict__ end, int64_t rows, int H) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * HEAD_WAVES;
    const float b0 = b ? b[0] : 0.f, b1 = b ? b[1] : 0.f;
    for (int64_t r = (int64_t)blockIdx.x * HEAD_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
        const float* x = h + r * H;
        float a0 = 0.f, a1 = 0.f;
        for (int k = lane * 4; k < H; k += 256) {
            const float4 v = *reinterpret_cast<const float4*>(x + k);
            const float4 u0 = *reinterpret_cast<const float4*>(w + k);
            const float4 u1 = *reinterpret_cast<const float4*>(w + H + k);
            a0 = fmaf(v.x, u0.x, a0); a0 = fmaf(v.y, u0.y, a0); a0 = fmaf(v.z, u0.z, a0); a0 = fmaf(v.w, u0.w, a0);
            a1 = fmaf(v.x, u1.x, a1); a1 = fmaf(v.y, u1.y, a1); a1 = fmaf(v.z, u1.z, a1); a1 = fmaf(v.w, u1.w, a1);
        }
        a0 = wave_sum(a0);
        a1 = wave_sum(a1);
        if (lane == 0) {
            start[r] = a0 + b0;
            end[r] = a1 + b1;
        }
    }
}

// value of the whole workgroup (every thread gets it); `red` holds RW slots
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (threadIdx.x & 63) < RW ? red[threadIdx.x & 63] : -INFINITY;
    v = wave_max(v);
    __syncthreads();
    return v;
}

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);  // butterfly: a tree over the wave's 64 partial sums
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = (threadIdx.x & 63) < RW ? red[threadIdx.x & 63] : 0.f;
    v = wave_sum(v);  // and over the RW wave sums
    __syncthreads();
    return v;
}

__global__ __launch_bounds__(RT) void log_softmax_kernel(const float* __restrict__ xs, const float* __restrict__ xe, int64_t n,
                                                         float* __restrict__ ls, float* __restrict__ le, float* __restrict__ ps,
                                                         float* __restrict__ pe) {
    __shared__ float red[RW];
    const int64_t off = (int64_t)blockIdx.x * n;
    const bool is_end = blockIdx.y != 0;
    const float* x = (is_end ? xe : xs) + off;
    float* lp = (is_end ? le : ls) + off;
    float* p = (is_end ? pe : ps) + off;
    float mx = -INFINITY;
    for (int64_t k = threadIdx.x; k < n; k += RT) mx = fmaxf(mx, x[k]);
    mx = block_max(mx, red);
    float s = 0.f;
    for (int64_t k = threadIdx.x; k < n; k += RT) s += expf(x[k] - mx);
    s = block_sum(s, red);
    const float lse = logf(s);
    for (int64_t k = threadIdx.x; k < n; k += RT) {
        const float v = (x[k] - mx) - lse;
        lp[k] = v;
        p[k] = expf(v);
    }
}

__global__ __launch_bounds__(RT) void best_spans_kernel(const float* __restrict__ sp, const float* __restrict__ ep,
                                                        const float* __restrict__ weights, int M, int L, int cbf,
                                                        int64_t* __restrict__ out_p, int64_t* __restrict__ out_s,
                                                        int64_t* __restrict__ out_e) {
    __shared__ uint64_t red[RW];
    const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t LL = (uint32_t)L * (uint32_t)L;
    uint64_t best = 0xFFFFFFFFull;  // candidate 0 of passage 0, value 0
    for (int m = 0; m < M; ++m) {
        const int64_t row = ((int64_t)q * M + m) * L;
        const float* s = sp + row;
        const float* e = ep + row;
        const float wm = weights ? weights[(int64_t)q * M + m] : 1.f;
        const uint32_t base = (uint32_t)m * LL;
        for (int i = (cbf ? 1 : 0) + wave; i < L; i += RW) {
            const float si = s[i];
            const uint32_t rbase = base + (uint32_t)i * (uint32_t)L;
            for (int j = i + lane; j < L; j += 64) {
                float v = si * e[j];
                if (weights) v = v * wm;
                const uint64_t key = ((uint64_t)(__float_as_uint(v) & 0x7FFFFFFFu) << 32) | (0xFFFFFFFFu - (rbase + (uint32_t)j));
                best = key > best ? key : best;
            }
        }
    }
    best = wave_max_u64(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (wave == 0) {
        best = lane < RW ? red[lane] : 0ull;
        best = wave_max_u64(best);
        if (lane == 0) {
            const uint32_t g = 0xFFFFFFFFu - (uint32_t)best;
            const uint32_t f = g % LL;
            out_p[q] = g / LL;
            out_s[q] = f / (uint32_t)L;
            out_e[q] = f % (uint32_t)L + 1;
        }
    }
}

}  // namespace

extern "C" {

int mq_reader_qa_head_f32(const float* h_dev, const float* w_dev, const float* b_dev, float* start_dev, float* end_dev,
                          int64_t rows, int H, void* stream) {
    if (rows < 0 || H <= 0 || (H % 4) != 0) return MQ_EINVAL;
    if (rows == 0) return MQ_OK;
    if (!h_dev || !w_dev || !start_dev || !end_dev) return MQ_EINVAL;
    if (((uintptr_t)h_dev | (uintptr_t)w_dev) & 15) return MQ_EINVAL;
    const int64_t blocks = (rows + HEAD_WAVES - 1) / HEAD_WAVES;
    const unsigned grid = (unsigned)(blocks < (1 << 20) ? blocks : (1 << 20));
    hipLaunchKernelGGL(qa_head_kernel, dim3(grid), dim3(HEAD_WAVES * 64), 0, (hipStream_t)stream, h_dev, w_dev, b_dev, start_dev,
                       end_dev, rows, H);
    return mq_launch_status();
}

int mq_reader_log_softmax_f32(const float* start_logits_dev, const float* end_logits_dev, int N, int M, int L,
                              float* start_logp_dev, float* end_logp_dev, float* start_p_dev, float* end_p_dev, void* stream) {
    if (N < 0 || M < 0 || L < 0) return MQ_EINVAL;
    if (N == 0 || M == 0 || L == 0) return MQ_OK;
    if (!start_logits_dev || !end_logits_dev || !start_logp_dev || !end_logp_dev || !start_p_dev || !end_p_dev) return MQ_EINVAL;
    hipLaunchKernelGGL(log_softmax_kernel, dim3((unsigned)N, 2), dim3(RT), 0, (hipStream_t)stream, start_logits_dev,
                       end_logits_dev, (int64_t)M * L, start_logp_dev, end_logp_dev, start_p_dev, end_p_dev);
    return mq_launch_status();
}

int mq_reader_best_spans_f32(const float* start_p_dev, const float* end_p_dev, const float* weights_dev, int N, int M, int L,
                             int cannot_be_first_token, int64_t* passage_dev, int64_t* start_dev, int64_t* end_dev,
                             void* stream) {
    if (N < 0 || M <= 0 || L <= 0) return MQ_EINVAL;
    if ((int64_t)M * L * L > (int64_t)0xFFFFFFFF) return MQ_EINVAL;  // candidate indices are 32-bit
    if (N == 0) return MQ_OK;
    if (!start_p_dev || !end_p_dev || !passage_dev || !start_dev || !end_dev) return MQ_EINVAL;
    hipLaunchKernelGGL(best_spans_kernel, dim3((unsigned)N), dim3(RT), 0, (hipStream_t)stream, start_p_dev, end_p_dev, weights_dev,
                       M, L, cannot_be_first_token ? 1 : 0, passage_dev, start_dev, end_dev);
    return mq_launch_status();
}

}  // extern "C"
