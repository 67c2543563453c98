// clip_resnet.hip -- what openai-clip's ModifiedResNet (the `clip-RN50` column) needs beyond conv.hip and resnet.hip, for gfx950.  Same
// conventions: NHWC, an activation that only feeds convolutions is a split-bf16 (hi, lo) pair in PAIR LAYOUT (device_common.h, with
// the split, the join and the wave reductions), BatchNorms folded on the host.  All four kernels run on the vector ALU and are bound by
// memory traffic, not arithmetic.
//   stem3x3s2_kernel      conv 3 x 3 / 2 (3 -> 32, pad 1) + folded bn1 + ReLU: fp32 NCHW pixels -> the pair.  K = 27 has no matrix-pipe shape.
//   avgpool2x2_kernel     AvgPool2d(2) on a pair -> pair (the stem's pool, the pool in front of a strided block's conv3, the shortcut's).
//   attn_tokens_kernel    AttentionPool2d's token matrix: [mean over HW | the HW pixels] + positional embedding -> pair, and the mean
//                         token's rows once more as their own pair (q_proj's operand).
//   attn_single_query_kernel   softmax(q . k_t * scale) . v for ONE query per (image, head): a wave per (image, head), lane = dimension.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/meerqat_hip.h"
#include "device_common.h"
#include "host_check.h"

namespace {

using namespace mq_dev;

// ---- the stem's first convolution: 3 x 3, stride 2, padding 1, 3 -> 32 channels, + bias (bn1 folded), ReLU --------------------------
// A thread = 8 output channels x 4 adjacent output pixels of one row: per (kh, c) it reads the 9 input pixels 2 ow0 - 1 ... 2 ow0 + 7 of
// one input row and makes 3 x 4 x 8 fused multiply-adds; every output is the chain bias -> (kh, c, kw) in that order.  The four threads of
// a pixel group (32 channels) are adjacent lanes: their input reads are one request, their 16-byte stores fill the pixel's 64-byte row
// of the pair.  Weights [27, 32] (3.4 KiB) sit in LDS.
constexpr int STEM_N = 32, STEM_PX = 4;

__global__ __launch_bounds__(256) void stem3x3s2_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, unsigned short* __restrict__ Ph,
                                                        unsigned short* __restrict__ Pl, int B, int H, int W) {
    __shared__ __attribute__((aligned(16))) float ws[27 * STEM_N];
    for (int e = threadIdx.x; e < 27 * STEM_N; e += 256) ws[e] = wt[e];
    __syncthreads();
    const int Ho = H >> 1, Wo = W >> 1;
    const unsigned gpr = (unsigned)(Wo + STEM_PX - 1) / STEM_PX;          // pixel groups per output row
    const unsigned long long unit = (unsigned long long)blockIdx.x * 64u + (threadIdx.x >> 2);
    if (unit >= (unsigned long long)B * Ho * gpr) return;
    const int ch0 = (threadIdx.x & 3) * 8;
    const unsigned g = (unsigned)(unit % gpr);
    const unsigned long long rowid = unit / gpr;                          // b * Ho + oh
    const int oh = (int)(rowid % (unsigned)Ho);
    const size_t b = (size_t)(rowid / (unsigned)Ho);
    const int ow0 = (int)g * STEM_PX;
    const size_t plane = (size_t)H * W;
    const float* xb = x + b * 3 * plane;
    float acc[STEM_PX][8];
#pragma unroll
    for (int p = 0; p < STEM_PX; ++p)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[p][j] = bias[ch0 + j];
#pragma unroll 1
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = 2 * oh - 1 + kh;
        const bool rok = ih >= 0 && ih < H;
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
            const float* xr = xb + (size_t)c * plane + (size_t)(rok ? ih : 0) * W;
            float in[2 * STEM_PX + 1];
#pragma unroll
            for (int k = 0; k < 2 * STEM_PX + 1; ++k) {
                const int iw = 2 * ow0 - 1 + k;
                in[k] = (rok && iw >= 0 && iw < W) ? xr[iw] : 0.f;
            }
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const float* wp = ws + ((kh * 3 + kw) * 3 + c) * STEM_N + ch0;
                const float4 w0 = *reinterpret_cast<const float4*>(wp), w1 = *reinterpret_cast<const float4*>(wp + 4);
                const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                for (int p = 0; p < STEM_PX; ++p)
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[p][j] = __builtin_fmaf(in[2 * p + kw], wv[j], acc[p][j]);
            }
        }
    }
    const size_t m0 = (size_t)rowid * Wo + ow0;
#pragma unroll
    for (int p = 0; p < STEM_PX; ++p) {
        if (ow0 + p < Wo) {
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) t[j] = __builtin_fmaxf(acc[p][j], 0.f);
            bf16x8_t h8, l8;
            split8(t, h8, l8);
            const size_t at = pair_index(m0 + p, ch0, STEM_N);
            *reinterpret_cast<bf16x8_t*>(Ph + at) = h8;
            *reinterpret_cast<bf16x8_t*>(Pl + at) = l8;
        }
    }
}

// ---- AvgPool2d(2) on a pair ---------------------------------------------------------------------------------------------------------
// out(b, ho, wo, c) = split((((x00 + x01) + x10) + x11) * 0.25), x_ij = hi + lo of input pixel (2 ho + i, 2 wo + j), every operation one
// fp32 rounding.  A thread = 8 channels of one output pixel (eight 16-byte loads, two 16-byte stores); threads are numbered in the memory
// order of the OUTPUT pair, so a wave stores 1 KiB contiguous in each array and the two output pixels of adjacent lane groups read four
// adjacent input pixels (256 contiguous bytes per array and input row).
__global__ __launch_bounds__(256) void avgpool2x2_kernel(const unsigned short* __restrict__ Xh, const unsigned short* __restrict__ Xl,
                                                         unsigned short* __restrict__ Ph, unsigned short* __restrict__ Pl, int H, int W,
                                                         int C, unsigned M) {
    const int CB = C >> 5, Ho = H >> 1, Wo = W >> 1;
    const unsigned long long q = (unsigned long long)blockIdx.x * 256u + threadIdx.x;   // 16-byte chunk of the output arrays
    const unsigned long long per_rb = (unsigned long long)CB * 1024u;
    const unsigned rb = (unsigned)(q / per_rb);
    const unsigned rem = (unsigned)(q - (unsigned long long)rb * per_rb);
    const unsigned cb = rem >> 10, r = (rem >> 2) & 255u, o = rem & 3u;
    const unsigned m = rb * 256u + r;
    if (m >= M) return;
    const unsigned hw = (unsigned)(Ho * Wo);
    const unsigned b = m / hw, pix = m - b * hw;
    const unsigned ho = pix / (unsigned)Wo, wo = pix - ho * (unsigned)Wo;
    const unsigned p00 = (b * (unsigned)H + 2u * ho) * (unsigned)W + 2u * wo;            // < B * H * W < 2^31 (checked by the caller)
    const int col = (int)(cb * 32u + o * 8u);
    float v[4][8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const size_t at = pair_index((size_t)p00 + (size_t)((k >> 1) * W + (k & 1)), col, C);
        join8(*reinterpret_cast<const bf16x8_t*>(Xh + at), *reinterpret_cast<const bf16x8_t*>(Xl + at), v[k]);
    }
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (((v[0][e] + v[1][e]) + v[2][e]) + v[3][e]) * 0.25f;
    bf16x8_t h8, l8;
    split8(t, h8, l8);
    const size_t at = pair_index((size_t)m, col, C);
    *reinterpret_cast<bf16x8_t*>(Ph + at) = h8;
    *reinterpret_cast<bf16x8_t*>(Pl + at) = l8;
}

// ---- AttentionPool2d's tokens ---------------------------------------------------------------------------------------------------------
// Y fp32 [B HW, C] -> the pair over [B (HW + 1), C]: row b (HW + 1) = mean_b + pos[0], rows + 1 + p = Y[b HW + p] + pos[1 + p];  mean_b =
// (the fp32 sum in the order p = 0 ... HW - 1, one rounding per pixel) / HW, mq_pool_hw_f32's mean.  The mean token is also written as row
// b of a pair over [B, C] (q_proj's operand).  A thread = 8 channels of one image, walking its pixels.
__global__ __launch_bounds__(64) void attn_tokens_kernel(const float* __restrict__ Y, const float* __restrict__ pos,
                                                         unsigned short* __restrict__ Th, unsigned short* __restrict__ Tl,
                                                         unsigned short* __restrict__ Qh, unsigned short* __restrict__ Ql, int B, int HW,
                                                         int C) {
    const unsigned long long u = (unsigned long long)blockIdx.x * 64u + threadIdx.x;
    const unsigned octs = (unsigned)C >> 3;
    if (u >= (unsigned long long)B * octs) return;
    const size_t b = (size_t)(u / octs);
    const int col = (int)(u % octs) * 8;
    const size_t T = (size_t)HW + 1;
    float sum[8];
    auto load8 = [](const float* p, float (&t)[8]) __attribute__((always_inline)) {
        const float4 a = *reinterpret_cast<const float4*>(p), c = *reinterpret_cast<const float4*>(p + 4);
        t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w; t[4] = c.x; t[5] = c.y; t[6] = c.z; t[7] = c.w;
    };
    auto store = [&](unsigned short* Oh, unsigned short* Ol, size_t row, const float (&t)[8]) __attribute__((always_inline)) {
        bf16x8_t h8, l8;
        split8(t, h8, l8);
        const size_t at = pair_index(row, col, C);
        *reinterpret_cast<bf16x8_t*>(Oh + at) = h8;
        *reinterpret_cast<bf16x8_t*>(Ol + at) = l8;
    };
    for (int p = 0; p < HW; ++p) {
        float y[8], e[8], t[8];
        load8(Y + (b * HW + p) * (size_t)C + col, y);
        load8(pos + (size_t)(p + 1) * C + col, e);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sum[j] = p ? sum[j] + y[j] : y[j];
            t[j] = y[j] + e[j];
        }
        store(Th, Tl, b * T + 1 + p, t);
    }
    float e[8], t[8];
    load8(pos + col, e);
#pragma unroll
    for (int j = 0; j < 8; ++j) t[j] = sum[j] / (float)HW + e[j];
    store(Th, Tl, b * T, t);
    store(Qh, Ql, b, t);
}

// ---- attention with ONE query per (image, head) ---------------------------------------------------------------------------------------
// A 64-lane workgroup per (image b, head h); lane d = dimension d of the head (head size 64).
//   s_t = (sum over d of q[d] k_t[d]) * scale: the 64 products summed by a butterfly (lane ^ 32, 16, 8, 4, 2, 1), kept in LDS;
//   m = max s_t;  p_t = expf(s_t - m);  l = sum p_t (each lane sums its t = lane, lane + 64, ... in that order, then the butterfly);
//   o[d] = (sum over t = 0 ... T - 1, in that order, of p_t v_t[d]) / l  -> split pair over [B, C].
// A wave reads 256 contiguous bytes of K, then of V, per key.
__global__ __launch_bounds__(64) void attn_single_query_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                               unsigned short* __restrict__ Oh, unsigned short* __restrict__ Ol, int T,
                                                               int heads, float scale) {
    extern __shared__ __attribute__((aligned(16))) float sc[];   // T scores, then probabilities
    const int lane = (int)threadIdx.x;
    const size_t b = blockIdx.x / (unsigned)heads;
    const int h = (int)(blockIdx.x % (unsigned)heads);
    const int C = heads * 64;
    const float qd = q[b * C + h * 64 + lane];
    const float* k0 = kv + b * T * (size_t)(2 * C) + h * 64 + lane;
    const float* v0 = k0 + C;
    for (int t = 0; t < T; ++t) {
        const float s = wave_sum(qd * k0[(size_t)t * (2 * C)]) * scale;
        if (lane == 0) sc[t] = s;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int t = lane; t < T; t += 64) m = __builtin_fmaxf(m, sc[t]);
    m = wave_max(m);
    float l = 0.f;
    for (int t = lane; t < T; t += 64) {
        const float p = expf(sc[t] - m);
        sc[t] = p;
        l += p;
    }
    l = wave_sum(l);
    __syncthreads();
    float o = 0.f;
    for (int t = 0; t < T; ++t) o += sc[t] * v0[(size_t)t * (2 * C)];
    o /= l;
    __bf16 hi, lo;
    split1(o, hi, lo);
    const size_t at = pair_index(b, h * 64 + lane, C);
    Oh[at] = __builtin_bit_cast(unsigned short, hi);
    Ol[at] = __builtin_bit_cast(unsigned short, lo);
}

}  // namespace

extern "C" {

int mq_clip_stem_conv3x3s2_f32(const float* x_dev, int B, int H, int W, const float* wt_dev, const float* bias_dev, int N,
                               uint16_t* Ph_dev, uint16_t* Pl_dev, void* stream) {
    if (B == 0) return MQ_OK;
    if (!x_dev || !wt_dev || !bias_dev || !Ph_dev || !Pl_dev || B < 0 || H <= 0 || W <= 0 || N <= 0) return MQ_EINVAL;
    if (N != STEM_N || (H & 1) || (W & 1)) return MQ_EUNSUPPORTED;
    if ((size_t)B * 3 * H * W >= 0x7FFFFFFFull * 4) return MQ_EUNSUPPORTED;
    const size_t units = (size_t)B * (size_t)(H / 2) * (size_t)((W / 2 + STEM_PX - 1) / STEM_PX);
    if ((units + 63) / 64 > 0x7FFFFFFFull) return MQ_EUNSUPPORTED;
    hipLaunchKernelGGL(stem3x3s2_kernel, dim3((unsigned)((units + 63) / 64)), dim3(256), 0, (hipStream_t)stream, x_dev, wt_dev, bias_dev,
                       (unsigned short*)Ph_dev, (unsigned short*)Pl_dev, B, H, W);
    return mq_launch_status();
}

int mq_avgpool2x2_pair_f32(const uint16_t* Xh_dev, const uint16_t* Xl_dev, int B, int H, int W, int C, uint16_t* Ph_dev, uint16_t* Pl_dev,
                           void* stream) {
    if (B == 0) return MQ_OK;
    if (!Xh_dev || !Xl_dev || !Ph_dev || !Pl_dev || B < 0 || H <= 0 || W <= 0 || C <= 0 || C % 32) return MQ_EINVAL;
    if ((H & 1) || (W & 1)) return MQ_EINVAL;
    if (((uintptr_t)Xh_dev | (uintptr_t)Xl_dev | (uintptr_t)Ph_dev | (uintptr_t)Pl_dev) & 15) return MQ_EINVAL;
    const size_t P = (size_t)B * H * W, M = P / 4;
    if (P >= 0x7FFFFFFFull) return MQ_EUNSUPPORTED;
    const size_t chunks = ((M + 255) / 256) * (size_t)(C / 32) * 1024;
    if (chunks / 256 > 0x7FFFFFFFull) return MQ_EUNSUPPORTED;
    hipLaunchKernelGGL(avgpool2x2_kernel, dim3((unsigned)(chunks / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned short*)Xh_dev, (const unsigned short*)Xl_dev, (unsigned short*)Ph_dev, (unsigned short*)Pl_dev, H, W,
                       C, (unsigned)M);
    return mq_launch_status();
}

int mq_attnpool_tokens_f32(const float* Y_dev, int B, int HW, int C, const float* pos_dev, uint16_t* Th_dev, uint16_t* Tl_dev,
                           uint16_t* Qh_dev, uint16_t* Ql_dev, void* stream) {
    if (B == 0) return MQ_OK;
    if (!Y_dev || !pos_dev || !Th_dev || !Tl_dev || !Qh_dev || !Ql_dev || B < 0 || HW <= 0 || C <= 0 || C % 32) return MQ_EINVAL;
    if (((uintptr_t)Y_dev | (uintptr_t)pos_dev | (uintptr_t)Th_dev | (uintptr_t)Tl_dev | (uintptr_t)Qh_dev | (uintptr_t)Ql_dev) & 15)
        return MQ_EINVAL;
    if ((size_t)B * ((size_t)HW + 1) >= 0x7FFFFFFFull) return MQ_EUNSUPPORTED;
    const size_t threads = (size_t)B * (size_t)(C / 8);
    if ((threads + 63) / 64 > 0x7FFFFFFFull) return MQ_EUNSUPPORTED;
    hipLaunchKernelGGL(attn_tokens_kernel, dim3((unsigned)((threads + 63) / 64)), dim3(64), 0, (hipStream_t)stream, Y_dev, pos_dev,
                       (unsigned short*)Th_dev, (unsigned short*)Tl_dev, (unsigned short*)Qh_dev, (unsigned short*)Ql_dev, B, HW, C);
    return mq_launch_status();
}

int mq_attention_single_query_f32(const float* q_dev, const float* kv_dev, int B, int T, int heads, int head_dim, float scale,
                                  uint16_t* Oh_dev, uint16_t* Ol_dev, void* stream) {
    if (B == 0) return MQ_OK;
    if (!q_dev || !kv_dev || !Oh_dev || !Ol_dev || B < 0 || T <= 0 || heads <= 0 || head_dim <= 0) return MQ_EINVAL;
    if (head_dim != 64 || T > 8192) return MQ_EUNSUPPORTED;   // a lane per dimension; the scores of one head in 32 KiB of LDS
    if ((size_t)B * heads > 0x7FFFFFFFull || (size_t)B * T >= 0x7FFFFFFFull) return MQ_EUNSUPPORTED;
    hipLaunchKernelGGL(attn_single_query_kernel, dim3((unsigned)((size_t)B * heads)), dim3(64), (size_t)T * sizeof(float),
                       (hipStream_t)stream, q_dev, kv_dev, (unsigned short*)Oh_dev, (unsigned short*)Ol_dev, T, heads, scale);
    return mq_launch_status();
}

}  // extern "C"
