// resnet.hip -- what a torchvision bottleneck ResNet (meerqat/image/embedding.py: `resnet50` cut before avgpool + AdaptiveMaxPool2d(1),
// the `imagenet-RN50` column) needs beyond the ArcFace kernels of conv.hip, for gfx950.  Same conventions: NHWC, an activation that only
// feeds convolutions is a split-bf16 (hi, lo) pair in PAIR LAYOUT (device_common.h), the BatchNorm behind a convolution
// is folded into its weights and bias on the host, elementwise work rides on the epilogue of the kernel that PRODUCES a tensor.
//   stem7x7_pool_kernel   conv 7 x 7 / 2 (3 -> 64, pad 3) + folded bn1 + ReLU + max-pool 3 x 3 / 2 (pad 1) in one pass on the vector
//                         ALU: reads fp32 NCHW pixels, writes the POOLED tensor as a pair -- the un-pooled 112 x 112 x 64 tensor (3.2 MB
//                         per image in fp32, the largest of the network) never exists in memory.
//   conv1x1_x3s_kernel    a 1 x 1 convolution (stride 1 or 2, no padding) on a pair as an implicit GEMM: conv3x3_x3s_kernel's
//                         machinery (conv.hip) with ONE tap -- the LDS-DMA gathers each output pixel's 64-byte channel blocks from the
//                         input pair (stride 2 = every other pixel, for free), three bf16 MFMA products per fp32 product -- and the
//                         bottleneck's epilogues: relu(acc + bias) -> pair;  acc + bias -> fp32 (the downsample shortcut);
//                         relu(acc + bias + shortcut) -> fp32 (the next shortcut / the pooled head's input) and -> pair (the next conv1).
//   pool_hw_kernel        global max / mean over the H W pixels of the last fp32 [B H W, C] tensor -> [B, C].
// The 3 x 3 convolutions of the bottlenecks are mq_conv3x3_pair_f32 (conv.hip) unchanged, with a zero PReLU slope = ReLU.
// The tile -> XCD mapping and the three-product K step that conv1x1_x3s_kernel shares with conv3x3_x3s_kernel are x3_tile.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/meerqat_hip.h"
#include "host_check.h"
#include "x3_tile.h"

namespace {

using namespace mq_dev;

// ---- 1 x 1 convolution on a pair ---------------------------------------------------------------------------------------------------
// C[M = B Ho Wo, N] = A[M, C] . W[N, C]^T, A row m = input pixel (b, ho s, wo s) of the input pair: K step cb of an output pixel is the 64
// contiguous bytes [pixel][channels 32 cb ...] of the pair, fetched by a per-lane LDS-DMA address (a page of zeros for the rows past M).
// Tiles: 16 waves, each 64 rows x WN columns, RG row groups x 16 / RG column groups (256 x 256, 256 x 128, 512 x 64); two LDS stages;
// per 16 k the products lo.hi, hi.lo, hi.hi on v_mfma_f32_32x32x16_bf16 -- the order of gemm_nt_x3s_kernel and conv3x3_x3s_kernel.
// Epilogue, per element: v = acc + bias;  v += R (if given);  v = max(v, 0) (if relu);  Y = v (if given);  P = split(v) (if given).
struct C1Args {
    const unsigned short *Xh, *Xl;  // input pair, PAIR LAYOUT over [B * H * W, C]
    const unsigned short *Wh, *Wl;  // weights, tile layout [ceil(N / 256)][C / 32][256][32] (mq_split_bf16_tiled_f32)
    const float* bias;              // [N]
    const float* R;                 // fp32 [M, N] or null
    float* Y;                       // fp32 [M, N] or null
    unsigned short *Ph, *Pl;        // pair output, PAIR LAYOUT over [M, N], or null
    const void* zeros;              // >= 16 bytes of zeros
    int H, W, C, N, stride, Ho, Wo, M, ntm, ntn, relu;
};

template <int RG, int WN>
__global__ __launch_bounds__(1024) void conv1x1_x3s_kernel(const C1Args a) {
    constexpr int CG = 16 / RG, MT = 64 * RG, NT = WN * CG, NF = WN / 32, AP = MT / 256;
    constexpr int A_BYTES = MT * 64, W_BYTES = NT * 64, STAGE = 2 * A_BYTES + 2 * W_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w / CG, wc = w % CG;
    int mt, nt;
    if (!xcd_tile((int)blockIdx.x, a.ntm, a.ntn, &mt, &nt)) return;
    const int m0 = mt * MT, n0 = nt * NT;
    const int CB = a.C >> 5;

    // ---- the gather: wave w fills rows [16 (w + 16 j), + 16) of the A stage, lane = (row, 16-byte slot)
    const unsigned slot = (unsigned)(lane & 3);
    const char* asrc_h[AP];
    const char* asrc_l[AP];
    size_t astep[AP];
#pragma unroll
    for (int j = 0; j < AP; ++j) {
        const int r = 16 * (w + 16 * j) + (lane >> 2);
        const int m = m0 + r;
        const unsigned hw = (unsigned)(a.Ho * a.Wo);
        const unsigned mm = m < a.M ? (unsigned)m : 0u;
        const unsigned bi = mm / hw, pix = mm - bi * hw;
        const unsigned ho = pix / (unsigned)a.Wo, wo = pix - ho * (unsigned)a.Wo;
        const unsigned p = (bi * (unsigned)a.H + ho * (unsigned)a.stride) * (unsigned)a.W + wo * (unsigned)a.stride;
        const size_t off = (size_t)(p >> 8) * (size_t)CB * 16384 + (size_t)((p & 255u) * 64u + (slot ^ (unsigned)((r >> 2) & 3)) * 16u);
        const bool ok = m < a.M;
        asrc_h[j] = ok ? reinterpret_cast<const char*>(a.Xh) + off : reinterpret_cast<const char*>(a.zeros);
        asrc_l[j] = ok ? reinterpret_cast<const char*>(a.Xl) + off : reinterpret_cast<const char*>(a.zeros);
        astep[j] = ok ? (size_t)16384 : (size_t)0;
    }
    const unsigned lds0 = __builtin_amdgcn_readfirstlane(lds_addr_of(smem));
    // weights: piece w of NT / 16 (16 rows x 64 B), rows n0 % 256 + 16 w ... of the K step's 16-KiB block
    const int rW = 16 * w + (lane >> 2);
    const unsigned w_voff = (unsigned)(((n0 & 255) + rW) * 64) + (slot ^ (unsigned)((rW >> 2) & 3)) * 16u;
    const char* wh0 = reinterpret_cast<const char*>(a.Wh) + (size_t)(n0 >> 8) * (size_t)CB * 16384;
    const char* wl0 = reinterpret_cast<const char*>(a.Wl) + (size_t)(n0 >> 8) * (size_t)CB * 16384;

    auto issue = [&](int cb, int stg) __attribute__((always_inline)) {
        const unsigned so = lds0 + (unsigned)(stg * STAGE);
#pragma unroll
        for (int j = 0; j < AP; ++j) {
            const unsigned dst = so + (unsigned)(16 * (w + 16 * j) * 64);
            dma16v(asrc_h[j] + (size_t)cb * astep[j], dst);
            dma16v(asrc_l[j] + (size_t)cb * astep[j], dst + A_BYTES);
        }
        if (w < NT / 16) {
            const unsigned dst = so + 2 * A_BYTES + (unsigned)(16 * w * 64);
            const size_t kw_ = (size_t)__builtin_amdgcn_readfirstlane(cb) * 16384;
            dma16s(wh0 + kw_, w_voff, dst);
            dma16s(wl0 + kw_, w_voff, dst + W_BYTES);
        }
    };

    const int i = lane & 31, kg = lane >> 5;
    const int sww = (i >> 2) & 3;
    const char* ard = smem + (64 * wr + i) * 64;               // Ah rows of this wave; Al at + A_BYTES
    const char* wrd = smem + 2 * A_BYTES + (WN * wc + i) * 64;  // Wh rows of this wave; Wl at + W_BYTES
    f32x16 acc[2][NF];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < NF; ++y) acc[x][y] = (f32x16){0};

    issue(0, 0);
    int stage = 0;
    for (int kb = 0; kb < CB; ++kb) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (kb + 1 < CB) issue(kb + 1, stage ^ 1);
        x3_step<NF>(ard + stage * STAGE, wrd + stage * STAGE, A_BYTES, W_BYTES, kg, sww, acc);
        stage ^= 1;
    }

    // ---- epilogue: one 32 x 32 accumulator at a time through LDS (4 KiB per wave), so that a lane ends up with eight consecutive
    // columns of one row: 16-byte loads and stores.
    // The walk is spelled out in each kernel that has it (here, conv.hip, resnet.hip, encoder.hip): shared as one function that takes
    // the per-element operations as functors, it changes the kernels' assembly.
    __syncthreads();  // every wave has read its last operands
    float* Ot = reinterpret_cast<float*>(smem) + w * 1024;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < NF; ++y) {
            const float bs = a.bias[n0 + WN * wc + 32 * y + i];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = (reg & 3) + 8 * (reg >> 2) + 4 * kg;
                Ot[row * 32 + ((((i >> 3) ^ (row & 3)) << 3) | (i & 7))] = acc[x][y][reg] + bs;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int row = 16 * it + (lane >> 2), g = lane & 3;
                const float* src = Ot + row * 32 + ((g ^ (row & 3)) << 3);
                const float4 u = *reinterpret_cast<const float4*>(src), v = *reinterpret_cast<const float4*>(src + 4);
                const int gm = m0 + 64 * wr + 32 * x + row, gn = n0 + WN * wc + 32 * y + 8 * g;
                if (gm < a.M) {
                    float t[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
                    const size_t at = (size_t)gm * a.N + gn;
                    if (a.R) {
                        const float4 ru = *reinterpret_cast<const float4*>(a.R + at), rv = *reinterpret_cast<const float4*>(a.R + at + 4);
                        t[0] += ru.x; t[1] += ru.y; t[2] += ru.z; t[3] += ru.w;
                        t[4] += rv.x; t[5] += rv.y; t[6] += rv.z; t[7] += rv.w;
                    }
                    if (a.relu) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) t[e] = t[e] > 0.f ? t[e] : 0.f;
                    }
                    if (a.Y) {
                        *reinterpret_cast<float4*>(a.Y + at) = make_float4(t[0], t[1], t[2], t[3]);
                        *reinterpret_cast<float4*>(a.Y + at + 4) = make_float4(t[4], t[5], t[6], t[7]);
                    }
                    if (a.Ph) {
                        bf16x8_t h8, l8;
                        split8(t, h8, l8);
                        const size_t pt = pair_index((size_t)gm, gn, a.N);
                        *reinterpret_cast<bf16x8_t*>(a.Ph + pt) = h8;
                        *reinterpret_cast<bf16x8_t*>(a.Pl + pt) = l8;
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next accumulator overwrites the scratch
        }
}

template <int RG, int WN>
int launch_conv1x1(C1Args a, hipStream_t st) {
    constexpr int CG = 16 / RG, MT = 64 * RG, NT = WN * CG;
    constexpr int STAGES = 2 * (2 * MT * 64 + 2 * NT * 64);
    constexpr int LDS = STAGES > 16 * 4096 ? STAGES : 16 * 4096;  // the epilogue's scratch: 4 KiB per wave
    if (a.N % NT) return MQ_EINVAL;
    a.ntm = (a.M + MT - 1) / MT;
    a.ntn = a.N / NT;
    const int ntiles = ((a.ntm + 7) >> 3) * 8 * a.ntn;
    MQ_DYNAMIC_LDS(LDS, conv1x1_x3s_kernel<RG, WN>);
    hipLaunchKernelGGL((conv1x1_x3s_kernel<RG, WN>), dim3((unsigned)ntiles), dim3(1024), LDS, st, a);
    return mq_launch_status();
}

// ---- the stem: conv 7 x 7 / 2 pad 3 (3 -> 64) + bias (bn1 folded) + ReLU + max-pool 3 x 3 / 2 pad 1 ---------------------------------
// Pooled pixel (ph, pw) = max of the conv pixels (2 ph - 1 + dh, 2 pw - 1 + dw), dh, dw in 0..2; the ReLU output is >= 0 and every window
// holds a real pixel, so a conv pixel outside the image simply counts as 0.  A thread = 8 output channels x a strip of 4 pooled rows x 2
// pooled columns: it walks the strip's 9 conv rows top to bottom, computes 5 adjacent conv pixels of each (columns 4 q - 1 ... 4 q + 3:
// both pooled columns' windows) as direct fp32 fused multiply-adds in (kh, c, kw) order from the NCHW pixels, reduces them to the two
// horizontal maxima and keeps a running vertical maximum -- nothing is exchanged between threads and no conv pixel is stored.  The
// price: 5 / 4 x 9 / 8 = 1.41 x the convolution's multiply-adds (the stem is 3 % of the network's).  The 147 x 64 weights sit in LDS
// (37 KiB), one 32-byte read per tap serves 5 x 8 multiply-adds.
constexpr int STEM_PH = 4;

__global__ __launch_bounds__(256) void stem7x7_pool_kernel(const float* __restrict__ x, const float* __restrict__ wt,
                                                           const float* __restrict__ bias, unsigned short* __restrict__ Ph,
                                                           unsigned short* __restrict__ Pl, int B, int H, int W) {
    __shared__ __attribute__((aligned(16))) float ws[147 * 64];
    for (int e = threadIdx.x; e < 147 * 64; e += 256) ws[e] = wt[e];
    __syncthreads();
    const int Hc = H >> 1, Wc = W >> 1, Hp = Hc >> 1, Wp = Wc >> 1;   // conv and pooled sizes (H, W multiples of 4)
    const int ch0 = (threadIdx.x & 7) * 8;
    const unsigned qpr = (unsigned)Wc >> 2, strips = (unsigned)(Hp + STEM_PH - 1) / STEM_PH, upi = qpr * strips;  // units per image
    const unsigned u = blockIdx.x * 32u + (threadIdx.x >> 3);
    if (u >= (unsigned)B * upi) return;
    const unsigned b = u / upi, rem = u - b * upi;
    const int strip = (int)(rem / qpr), q = (int)(rem - (unsigned)strip * qpr);
    const int ph0 = strip * STEM_PH, oc0 = 4 * q - 1;      // first pooled row; first conv column
    const float* xb = x + (size_t)b * 3 * H * W;
    const size_t plane = (size_t)H * W;
    float bs[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bs[j] = bias[ch0 + j];
    float runA[8], runB[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) runA[j] = runB[j] = 0.f;
#pragma unroll 1
    for (int t = 0; t <= 2 * STEM_PH; ++t) {
        const int oh = 2 * ph0 - 1 + t;                   // conv row
        float rowA[8], rowB[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) rowA[j] = rowB[j] = 0.f;
        if (oh >= 0 && oh < Hc) {
            float acc[5][8];
#pragma unroll
            for (int p = 0; p < 5; ++p)
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[p][j] = bs[j];
#pragma unroll 1
            for (int kh = 0; kh < 7; ++kh) {
                const int ih = 2 * oh - 3 + kh;
                const bool rok = ih >= 0 && ih < H;
#pragma unroll 1
                for (int c = 0; c < 3; ++c) {
                    float in[15];
                    const float* xr = xb + (size_t)c * plane + (size_t)(rok ? ih : 0) * W;
#pragma unroll
                    for (int k = 0; k < 15; ++k) {
                        const int iw = 2 * oc0 - 3 + k;
                        in[k] = (rok && iw >= 0 && iw < W) ? xr[iw] : 0.f;
                    }
#pragma unroll
                    for (int kw = 0; kw < 7; ++kw) {
                        const float* wp = ws + ((kh * 7 + kw) * 3 + c) * 64 + ch0;
                        const float4 w0 = *reinterpret_cast<const float4*>(wp), w1 = *reinterpret_cast<const float4*>(wp + 4);
                        const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                        for (int p = 0; p < 5; ++p)
#pragma unroll
                            for (int j = 0; j < 8; ++j) acc[p][j] = __builtin_fmaf(in[2 * p + kw], wv[j], acc[p][j]);
                    }
                }
            }
            // ReLU and the horizontal maxima; conv column -1 (q = 0) is outside the image
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v0 = oc0 >= 0 ? __builtin_fmaxf(acc[0][j], 0.f) : 0.f;
                const float v1 = __builtin_fmaxf(acc[1][j], 0.f), v2 = __builtin_fmaxf(acc[2][j], 0.f);
                const float v3 = __builtin_fmaxf(acc[3][j], 0.f), v4 = __builtin_fmaxf(acc[4][j], 0.f);
                rowA[j] = __builtin_fmaxf(__builtin_fmaxf(v0, v1), v2);
                rowB[j] = __builtin_fmaxf(__builtin_fmaxf(v2, v3), v4);
            }
        }
        // conv row t of the strip closes pooled row t / 2 - 1 and opens pooled row t / 2 when t is even
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            runA[j] = __builtin_fmaxf(runA[j], rowA[j]);
            runB[j] = __builtin_fmaxf(runB[j], rowB[j]);
        }
        if (t >= 2 && !(t & 1)) {
            const int ph = ph0 + (t >> 1) - 1;
            if (ph < Hp) {
                bf16x8_t h8, l8;
                const size_t m = ((size_t)b * Hp + ph) * Wp + 2 * q;
                split8(runA, h8, l8);
                size_t at = pair_index(m, ch0, 64);
                *reinterpret_cast<bf16x8_t*>(Ph + at) = h8;
                *reinterpret_cast<bf16x8_t*>(Pl + at) = l8;
                split8(runB, h8, l8);
                at = pair_index(m + 1, ch0, 64);
                *reinterpret_cast<bf16x8_t*>(Ph + at) = h8;
                *reinterpret_cast<bf16x8_t*>(Pl + at) = l8;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { runA[j] = rowA[j]; runB[j] = rowB[j]; }
        }
    }
}

// ---- the pooled head: out[b, c] = max or mean over the HW pixels of X[b HW + p, c].  One thread per (b, c), pixels in the order p = 0
// ... HW - 1: the mean is that fp32 sum (one rounding per pixel) divided once by HW.  A wave reads 256 contiguous bytes per pixel.
__global__ __launch_bounds__(256) void pool_hw_kernel(const float* __restrict__ X, int HW, int C, int mean, float* __restrict__ out) {
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x, b = (int)blockIdx.y;
    if (c >= C) return;
    const float* p = X + (size_t)b * HW * C + c;
    float r = p[0];
    for (int k = 1; k < HW; ++k) {
        const float v = p[(size_t)k * C];
        r = mean ? r + v : __builtin_fmaxf(r, v);
    }
    out[(size_t)b * C + c] = mean ? r / (float)HW : r;
}

}  // namespace

extern "C" {

int mq_conv1x1_pair_f32(const uint16_t* Xh_dev, const uint16_t* Xl_dev, int B, int H, int W, int C, int stride, const uint16_t* Wh_dev,
                        const uint16_t* Wl_dev, int N, const float* bias_dev, const float* residual_dev, int relu, float* Y_dev,
                        uint16_t* Ph_dev, uint16_t* Pl_dev, const void* zeros_dev, int tile, void* stream) {
    if (B == 0) return MQ_OK;
    if (!Xh_dev || !Xl_dev || !Wh_dev || !Wl_dev || !bias_dev || !zeros_dev || B < 0 || H <= 0 || W <= 0) return MQ_EINVAL;
    if (C <= 0 || C % 32 || N <= 0 || N % 64 || (stride != 1 && stride != 2)) return MQ_EINVAL;
    if ((Ph_dev == nullptr) != (Pl_dev == nullptr) || (!Y_dev && !Ph_dev)) return MQ_EINVAL;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    const size_t M = (size_t)B * Ho * Wo, P = (size_t)B * H * W;
    if (M >= 0x7FFFFFFFull || P >= 0x7FFFFFFFull) return MQ_EUNSUPPORTED;
    C1Args a = {};
    a.Xh = Xh_dev; a.Xl = Xl_dev; a.Wh = Wh_dev; a.Wl = Wl_dev; a.bias = bias_dev; a.R = residual_dev; a.Y = Y_dev;
    a.Ph = Ph_dev; a.Pl = Pl_dev; a.zeros = zeros_dev;
    a.H = H; a.W = W; a.C = C; a.N = N; a.stride = stride; a.Ho = Ho; a.Wo = Wo; a.M = (int)M; a.relu = relu ? 1 : 0;
    if (tile == MQ_CONV_TILE_AUTO) {
        // the widest tile the channel count fills while it still gives most CUs a workgroup (the rule of mq_conv3x3_pair_f32)
        if (N % 256 == 0 && ((M + 255) / 256) * (size_t)(N / 256) >= 192) tile = MQ_CONV_TILE_256x256;
        else if (N % 128 == 0) tile = MQ_CONV_TILE_256x128;
        else tile = MQ_CONV_TILE_512x64;
    }
    switch (tile) {
        case MQ_CONV_TILE_256x256: return launch_conv1x1<4, 64>(a, (hipStream_t)stream);
        case MQ_CONV_TILE_256x128: return launch_conv1x1<4, 32>(a, (hipStream_t)stream);
        case MQ_CONV_TILE_512x64: return launch_conv1x1<8, 32>(a, (hipStream_t)stream);
    }
    return MQ_EINVAL;
}

int mq_stem_conv7x7_pool_f32(const float* x_dev, int B, int H, int W, const float* wt_dev, const float* bias_dev, uint16_t* Ph_dev,
                             uint16_t* Pl_dev, void* stream) {
    if (B == 0) return MQ_OK;
    if (!x_dev || !wt_dev || !bias_dev || !Ph_dev || !Pl_dev || B < 0 || H <= 0 || W <= 0) return MQ_EINVAL;
    if ((H & 3) || (W & 7)) return MQ_EUNSUPPORTED;
    const size_t units = (size_t)B * (size_t)((H / 4 + STEM_PH - 1) / STEM_PH) * (size_t)(W / 8);
    if ((size_t)B * 3 * H * W >= 0x7FFFFFFFull * 4 || (units + 31) / 32 > 0x7FFFFFFFull) return MQ_EUNSUPPORTED;
    hipLaunchKernelGGL(stem7x7_pool_kernel, dim3((unsigned)((units + 31) / 32)), dim3(256), 0, (hipStream_t)stream, x_dev, wt_dev,
                       bias_dev, (unsigned short*)Ph_dev, (unsigned short*)Pl_dev, B, H, W);
    return mq_launch_status();
}

int mq_pool_hw_f32(const float* X_dev, int B, int HW, int C, int mode, float* out_dev, void* stream) {
    if (B == 0) return MQ_OK;
    if (!X_dev || !out_dev || B < 0 || B > 65535 || HW <= 0 || C <= 0) return MQ_EINVAL;
    if (mode != MQ_POOL_MAX && mode != MQ_POOL_MEAN) return MQ_EINVAL;
    hipLaunchKernelGGL(pool_hw_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, X_dev, HW, C,
                       mode == MQ_POOL_MEAN, out_dev);
    return mq_launch_status();
}

}  // extern "C"
