// mtcnn.hip -- MTCNN face detection on gfx950 (facenet_pytorch's detect_face as restated in tests/mtcnn_restatement.py; what the
// reference runs through meerqat/image/face_detection.py).  C ABI: include/meerqat_hip.h.  All network arithmetic is fp32 FMA with
// fp32 accumulation (3 to 128 channels, a few GFLOP per image: no MFMA); box geometry uses separate multiplies and adds, like the
// elementwise tensor operations it restates, so that integer decisions (floor, trunc, clip, NMS) compare bit for bit.
//
//   resample_kernel   every pyramid level of every image, or every crop of a stage, in one launch: adaptive average pooling
//                     ("area": windows [floor(i in / out), ceil((i + 1) in / out))) of a rectangle of a packed uint8 RGB image,
//                     zero outside the image, then (x - 127.5) * 0.0078125, planar CHW fp32.  Window sums are integers (exact).
//   pnet_kernel       one workgroup per (level, 16 x 16 tile of output cells): the 42 x 42 x 3 input patch, the pooled conv1 map
//                     (conv1 + PReLU + ceil-mode 2/2 max-pool fused) and the conv2 map live in LDS (57 KiB); conv3, the two 1 x 1
//                     heads, the softmax, the threshold and the box generation run in registers.  Only passing cells leave: each is
//                     appended to its image's candidate list through an atomic counter (the maps are stored only for the tests).
//   nms_kernel        one workgroup per segment (image): ranks the eligible boxes by (score descending, key ascending) -- so the
//                     result never depends on the order of the appends -- then greedy suppression over the sorted list, IoU or
//                     "Min" overlap with the +1 area convention, optionally only inside equal sub-groups (the pyramid level).
//   refine_kernel     box regression, rerec, trunc + pad, crop-skip rule and the crop jobs of the next stage, compacting the
//                     per-image lists into one.
//   rnet_kernel       one workgroup per 24 x 24 crop, every map in LDS (68 KiB).
//   onet_kernel       one workgroup per 48 x 48 crop (126 KiB of LDS): conv1 and conv2 walk their output channels in groups whose
//                     maps are pooled before the next group overwrites them (the 46 x 46 x 32 map never exists).
//   onet_post_kernel  landmarks to pixels and the last box regression.
// Dense weights are packed [input in LDS order (c, y, x)][output]: the published flatten order (w, h, c) is folded into the row order
// on the host (viquae_amd/image/face_detection.py), and neighbouring threads read neighbouring weights.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/meerqat_hip.h"
#include "host_check.h"

namespace {

// ---- packed weights (floats): per layer weight, bias[, PReLU slope], in network order
constexpr int P_W1 = 0, P_B1 = P_W1 + 270, P_A1 = P_B1 + 10, P_W2 = P_A1 + 10, P_B2 = P_W2 + 1440, P_A2 = P_B2 + 16,
              P_W3 = P_A2 + 16, P_B3 = P_W3 + 4608, P_A3 = P_B3 + 32, P_W41 = P_A3 + 32, P_B41 = P_W41 + 64, P_W42 = P_B41 + 2,
              P_B42 = P_W42 + 128, P_TOTAL = P_B42 + 4;
constexpr int R_W1 = 0, R_B1 = R_W1 + 756, R_A1 = R_B1 + 28, R_W2 = R_A1 + 28, R_B2 = R_W2 + 12096, R_A2 = R_B2 + 48,
              R_W3 = R_A2 + 48, R_B3 = R_W3 + 12288, R_A3 = R_B3 + 64, R_W4 = R_A3 + 64, R_B4 = R_W4 + 73728, R_A4 = R_B4 + 128,
              R_W51 = R_A4 + 128, R_B51 = R_W51 + 256, R_W52 = R_B51 + 2, R_B52 = R_W52 + 512, R_TOTAL = R_B52 + 4;
constexpr int O_W1 = 0, O_B1 = O_W1 + 864, O_A1 = O_B1 + 32, O_W2 = O_A1 + 32, O_B2 = O_W2 + 18432, O_A2 = O_B2 + 64,
              O_W3 = O_A2 + 64, O_B3 = O_W3 + 36864, O_A3 = O_B3 + 64, O_W4 = O_A3 + 64, O_B4 = O_W4 + 32768, O_A4 = O_B4 + 128,
              O_W5 = O_A4 + 128, O_B5 = O_W5 + 294912, O_A5 = O_B5 + 256, O_W61 = O_A5 + 256, O_B61 = O_W61 + 512,
              O_W62 = O_B61 + 2, O_B62 = O_W62 + 1024, O_W63 = O_B62 + 4, O_B63 = O_W63 + 2560, O_TOTAL = O_B63 + 10;

constexpr int REC = MQ_MTCNN_REC;  // floats of a box record: x1, y1, x2, y2, score, reg 0..3

__device__ __forceinline__ float prelu(float v, float a) { return v > 0.f ? v : a * v; }
__device__ __forceinline__ float softmax1(float a0, float a1) {
    const float m = fmaxf(a0, a1);
    const float e0 = expf(a0 - m), e1 = expf(a1 - m);
    return e1 / (e0 + e1);
}

// ------------------------------------------------------------------------------------------------ resampling
__global__ __launch_bounds__(256) void resample_kernel(const uint8_t* __restrict__ images, const int64_t* __restrict__ offsets,
                                                       const int32_t* __restrict__ hw, int n_images,
                                                       const int64_t* __restrict__ jobs, float* __restrict__ out, int64_t out_floats,
                                                       int32_t* __restrict__ overflow) {
    const int64_t* j = jobs + (int64_t)blockIdx.x * MQ_MTCNN_JOB;
    const int64_t img = j[0], x0 = j[1], y0 = j[2], cw = j[3], ch = j[4], ow = j[5], oh = j[6], off = j[7];
    if (img < 0 || img >= n_images || ow <= 0 || oh <= 0) return;
    const int64_t n = ow * oh;
    if (off < 0 || off + 3 * n > out_floats) {
        if (threadIdx.x == 0 && blockIdx.y == 0) *overflow = 1;
        return;
    }
    const int H = hw[2 * img], W = hw[2 * img + 1];
    const uint8_t* src = images + offsets[img];
    for (int64_t p = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; p < n; p += (int64_t)gridDim.y * blockDim.x) {
        float v[3] = {0.f, 0.f, 0.f};
        if (cw > 0 && ch > 0) {
            const int64_t oy = p / ow, ox = p - oy * ow;
            const int64_t ys = (oy * ch) / oh, ye = ((oy + 1) * ch + oh - 1) / oh;
            const int64_t xs = (ox * cw) / ow, xe = ((ox + 1) * cw + ow - 1) / ow;
            uint64_t s[3] = {0, 0, 0};
            for (int64_t yy = ys; yy < ye; ++yy) {
                const int64_t gy = y0 + yy;
                if (gy < 0 || gy >= H) continue;
                for (int64_t xx = xs; xx < xe; ++xx) {
                    const int64_t gx = x0 + xx;
                    if (gx < 0 || gx >= W) continue;
                    const uint8_t* px = src + (gy * W + gx) * 3;
                    s[0] += px[0]; s[1] += px[1]; s[2] += px[2];
                }
            }
            const float cnt = (float)((ye - ys) * (xe - xs));
            for (int c = 0; c < 3; ++c) v[c] = ((float)s[c] / cnt - 127.5f) * 0.0078125f;
        }
        for (int c = 0; c < 3; ++c) out[off + c * n + p] = v[c];
    }
}

// ------------------------------------------------------------------------------------------------ P-Net
constexpr int PT = 16;                 // output cells per tile side
constexpr int PPL = PT + 4;            // pooled conv1 map the tile needs (conv2 and conv3 each take 2)
constexpr int PIN = 2 * PPL + 2;       // input patch side
constexpr int PC2 = PT + 2;

__device__ __forceinline__ int pnet_pooled(int h) { return (h - 3) / 2 + 1; }  // ceil((h - 2 - 2) / 2) + 1, h >= 12

__global__ __launch_bounds__(256) void pnet_kernel(const float* __restrict__ in, int64_t in_floats, const int64_t* __restrict__ levels,
                                                   const float* __restrict__ level_scale, const float* __restrict__ wt, float thr,
                                                   int n_images, int cap, float* __restrict__ rec, int32_t* __restrict__ cidx,
                                                   int32_t* __restrict__ csub, int32_t* __restrict__ count,
                                                   int32_t* __restrict__ overflow, float* __restrict__ maps, int64_t maps_floats) {
    __shared__ float s_in[3 * PIN * PIN];
    __shared__ float s_pl[10 * PPL * PPL];
    __shared__ float s_c2[16 * PC2 * PC2];
    __shared__ float s_w3[P_TOTAL - P_W3];  // conv3 and the heads: 32 + 6 accumulators per thread leave no scalar registers for them
    const int64_t* lv = levels + (int64_t)blockIdx.y * MQ_MTCNN_LEVEL;
    const int64_t in_off = lv[0];
    const int H = (int)lv[1], W = (int)lv[2], img = (int)lv[3];
    if (lv[1] < 12 || lv[2] < 12 || lv[1] > 0x3fffffff || lv[2] > 0x3fffffff || img < 0 || img >= n_images) return;
    const int Hp = pnet_pooled(H), Wp = pnet_pooled(W), Ho = Hp - 4, Wo = Wp - 4;
    // a level table that points outside the buffers it describes is refused, never followed
    if (in_off < 0 || in_off > in_floats || 3 * (int64_t)H * W > in_floats - in_off ||
        (maps && (lv[6] < 0 || lv[6] > maps_floats || 5 * (int64_t)Ho * Wo > maps_floats - lv[6]))) {
        if (threadIdx.x == 0) *overflow = 1;
        return;
    }
    const int tiles_x = (Wo + PT - 1) / PT, tiles_y = (Ho + PT - 1) / PT;
    if ((int)blockIdx.x >= tiles_x * tiles_y) return;
    const int oy0 = ((int)blockIdx.x / tiles_x) * PT, ox0 = ((int)blockIdx.x % tiles_x) * PT;
    const int iy0 = 2 * oy0, ix0 = 2 * ox0;
    const int tid = threadIdx.x;
    const float* src = in + in_off;
    for (int i = tid; i < P_TOTAL - P_W3; i += 256) s_w3[i] = wt[P_W3 + i];
    for (int i = tid; i < 3 * PIN * PIN; i += 256) {
        const int c = i / (PIN * PIN), r = i % (PIN * PIN), y = iy0 + r / PIN, x = ix0 + r % PIN;
        s_in[i] = (y < H && x < W) ? src[((int64_t)c * H + y) * W + x] : 0.f;
    }
    __syncthreads();
    // conv1 + PReLU + 2/2 ceil-mode max-pool: one pooled position per thread, all ten channels
    for (int p = tid; p < PPL * PPL; p += 256) {
        const int py = p / PPL, px = p % PPL;
        float best[10];
#pragma unroll
        for (int co = 0; co < 10; ++co) best[co] = -INFINITY;
        for (int d = 0; d < 4; ++d) {
            const int r = 2 * py + (d >> 1), c = 2 * px + (d & 1);
            if (iy0 + r >= H - 2 || ix0 + c >= W - 2) continue;  // the partial window at the map's edge
            float acc[10];
#pragma unroll
            for (int co = 0; co < 10; ++co) acc[co] = wt[P_B1 + co];
            for (int ci = 0; ci < 3; ++ci)
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll 1
                    for (int kx = 0; kx < 3; ++kx) {
                        const float x = s_in[(ci * PIN + r + ky) * PIN + c + kx];
#pragma unroll
                        for (int co = 0; co < 10; ++co) acc[co] = fmaf(wt[P_W1 + ((co * 3 + ci) * 3 + ky) * 3 + kx], x, acc[co]);
                    }
#pragma unroll
            for (int co = 0; co < 10; ++co) best[co] = fmaxf(best[co], prelu(acc[co], wt[P_A1 + co]));
        }
        const bool inside = oy0 + py < Hp && ox0 + px < Wp;
#pragma unroll
        for (int co = 0; co < 10; ++co) s_pl[(co * PPL + py) * PPL + px] = inside ? best[co] : 0.f;
    }
    __syncthreads();
    for (int p = tid; p < PC2 * PC2; p += 256) {
        const int y = p / PC2, x = p % PC2;
        float acc[16];
#pragma unroll
        for (int co = 0; co < 16; ++co) acc[co] = wt[P_B2 + co];
        for (int ci = 0; ci < 10; ++ci)
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll 1
                for (int kx = 0; kx < 3; ++kx) {
                    const float v = s_pl[(ci * PPL + y + ky) * PPL + x + kx];
#pragma unroll
                    for (int co = 0; co < 16; ++co) acc[co] = fmaf(wt[P_W2 + ((co * 10 + ci) * 3 + ky) * 3 + kx], v, acc[co]);
                }
#pragma unroll
        for (int co = 0; co < 16; ++co) s_c2[(co * PC2 + y) * PC2 + x] = prelu(acc[co], wt[P_A2 + co]);
    }
    __syncthreads();
    const int y = tid / PT, x = tid % PT, oy = oy0 + y, ox = ox0 + x;
    float acc[32];
#pragma unroll
    for (int co = 0; co < 32; ++co) acc[co] = s_w3[P_B3 - P_W3 + co];
    for (int ci = 0; ci < 16; ++ci)
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll 1
            for (int kx = 0; kx < 3; ++kx) {
                const float v = s_c2[(ci * PC2 + y + ky) * PC2 + x + kx];
#pragma unroll
                for (int co = 0; co < 32; ++co) acc[co] = fmaf(s_w3[P_W3 - P_W3 + ((co * 16 + ci) * 3 + ky) * 3 + kx], v, acc[co]);
            }
    float a0 = s_w3[P_B41 - P_W3], a1 = s_w3[P_B41 - P_W3 + 1], r[4] = {s_w3[P_B42 - P_W3], s_w3[P_B42 - P_W3 + 1], s_w3[P_B42 - P_W3 + 2], s_w3[P_B42 - P_W3 + 3]};
#pragma unroll
    for (int co = 0; co < 32; ++co) {
        const float h = prelu(acc[co], s_w3[P_A3 - P_W3 + co]);
        a0 = fmaf(s_w3[P_W41 - P_W3 + co], h, a0);
        a1 = fmaf(s_w3[P_W41 - P_W3 + 32 + co], h, a1);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = fmaf(s_w3[P_W42 - P_W3 + k * 32 + co], h, r[k]);
    }
    if (oy >= Ho || ox >= Wo) return;
    const float prob = softmax1(a0, a1);
    const int64_t cell = (int64_t)oy * Wo + ox;
    if (maps) {
        float* m = maps + lv[6];
        const int64_t plane = (int64_t)Ho * Wo;
        m[cell] = prob;
        for (int k = 0; k < 4; ++k) m[(k + 1) * plane + cell] = r[k];
    }
    if (!(prob >= thr)) return;
    const int pos = atomicAdd(&count[img], 1);
    if (pos >= cap) { *overflow = 1; return; }
    const float s = level_scale[blockIdx.y];
    const int64_t b = (int64_t)img * cap + pos;
    float* o = rec + b * REC;
    o[0] = floorf((2.f * (float)ox + 1.f) / s);
    o[1] = floorf((2.f * (float)oy + 1.f) / s);
    o[2] = floorf((2.f * (float)ox + 12.f) / s);
    o[3] = floorf((2.f * (float)oy + 12.f) / s);
    o[4] = prob;
    for (int k = 0; k < 4; ++k) o[5 + k] = r[k];
    cidx[b] = (int32_t)(lv[5] + cell);
    csub[b] = (int32_t)lv[4];
}

// ------------------------------------------------------------------------------------------------ NMS
constexpr int NT = 512;

__global__ __launch_bounds__(NT) void nms_kernel(const float* __restrict__ rec, int64_t n_total, const int64_t* __restrict__ seg_start,
                                                 const int32_t* __restrict__ seg_count, int64_t seg_cap, const int32_t* __restrict__ key,
                                                 const int32_t* __restrict__ sub, float score_gt, float thr, int mode_min,
                                                 float* __restrict__ out_rec, int32_t* __restrict__ out_key,
                                                 int32_t* __restrict__ out_sub, int32_t* __restrict__ out_src,
                                                 int32_t* __restrict__ out_count, float* ws_f, int32_t* ws_i) {
    __shared__ int s_m, s_kept;
    const int g = blockIdx.x, tid = threadIdx.x;
    const int64_t s0 = seg_start[g];
    int64_t n64 = seg_count[g];
    if (s0 < 0 || s0 > n_total) n64 = 0;
    if (n64 > n_total - s0) n64 = n_total - s0;   // a counter that ran past its capacity: only what was stored
    if (seg_cap > 0 && n64 > seg_cap) n64 = seg_cap;
    const int n = n64 < 0 ? 0 : (int)n64;
    float* w_score = ws_f + s0;                    // [n_total] each: score / x1 / y1 / x2 / y2 of the sorted list
    float* w_x1 = ws_f + n_total + s0;
    float* w_y1 = ws_f + 2 * n_total + s0;
    float* w_x2 = ws_f + 3 * n_total + s0;
    float* w_y2 = ws_f + 4 * n_total + s0;
    int32_t* w_key = ws_i + s0;                    // [n_total] each: key / sorted order / sub of the sorted list / suppressed
    int32_t* w_order = ws_i + n_total + s0;
    int32_t* w_sub = ws_i + 2 * n_total + s0;
    volatile int32_t* w_dead = ws_i + 3 * n_total + s0;
    if (tid == 0) { s_m = 0; s_kept = 0; }
    for (int i = tid; i < n; i += NT) {
        w_score[i] = rec[(s0 + i) * REC + 4];
        w_key[i] = key ? key[s0 + i] : i;
    }
    __syncthreads();
    // rank among the eligible boxes: score descending, equal scores by ascending key (keys are distinct inside a segment)
    for (int i = tid; i < n; i += NT) {
        const float si = w_score[i];
        if (!(si > score_gt)) continue;
        const int ki = w_key[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) {
            const float sj = w_score[j];
            if (!(sj > score_gt)) continue;
            rank += (sj > si || (sj == si && w_key[j] < ki)) ? 1 : 0;
        }
        w_order[rank] = i;
        atomicAdd(&s_m, 1);
    }
    __syncthreads();
    const int m = s_m;
    for (int r = tid; r < m; r += NT) {
        const int64_t i = s0 + w_order[r];
        w_x1[r] = rec[i * REC]; w_y1[r] = rec[i * REC + 1]; w_x2[r] = rec[i * REC + 2]; w_y2[r] = rec[i * REC + 3];
        w_sub[r] = sub ? sub[i] : 0;
        w_dead[r] = 0;
    }
    __syncthreads();
    for (int r = 0; r < m; ++r) {
        if (!w_dead[r]) {
            const float x1 = w_x1[r], y1 = w_y1[r], x2 = w_x2[r], y2 = w_y2[r];
            const float area = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
            const int sr = w_sub[r];
            for (int j = r + 1 + tid; j < m; j += NT) {
                if (w_dead[j] || w_sub[j] != sr) continue;
                const float a1 = w_x1[j], b1 = w_y1[j], a2 = w_x2[j], b2 = w_y2[j];
                const float aj = (a2 - a1 + 1.f) * (b2 - b1 + 1.f);
                const float iw = fmaxf(0.f, fminf(x2, a2) - fmaxf(x1, a1) + 1.f);
                const float ih = fmaxf(0.f, fminf(y2, b2) - fmaxf(y1, b1) + 1.f);
                const float inter = iw * ih;
                const float o = mode_min ? inter / fminf(area, aj) : inter / (area + aj - inter);
                if (o > thr) w_dead[j] = 1;
            }
            if (tid == 0) {
                const int i = w_order[r];
                const int64_t d = s0 + s_kept;
                for (int c = 0; c < REC; ++c) out_rec[d * REC + c] = rec[(s0 + i) * REC + c];
                if (out_key) out_key[d] = w_key[i];
                if (out_sub) out_sub[d] = sr;
                if (out_src) out_src[d] = i;
                s_kept++;
            }
        }
        __syncthreads();
    }
    if (tid == 0) out_count[g] = s_kept;
}

// ------------------------------------------------------------------------------------------------ box refinement
__global__ __launch_bounds__(256) void refine_kernel(const float* __restrict__ in_rec, const int64_t* __restrict__ seg_start,
                                                     const int64_t* __restrict__ dst_start, int n_seg,
                                                     const int32_t* __restrict__ hw, int flags, int crop, int64_t out_cap,
                                                     float* __restrict__ out_rec, int32_t* __restrict__ out_img,
                                                     int32_t* __restrict__ out_pad, int64_t* __restrict__ jobs,
                                                     int32_t* __restrict__ valid, int32_t* __restrict__ overflow) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = dst_start[n_seg];
    if (k >= total) return;
    if (k >= out_cap) { *overflow = 1; return; }
    int lo = 0, hi = n_seg;  // the segment g with dst_start[g] <= k < dst_start[g + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (dst_start[mid] <= k) lo = mid; else hi = mid;
    }
    const int g = lo;
    const float* b = in_rec + (seg_start[g] + (k - dst_start[g])) * REC;
    float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    const float one = (flags & MQ_MTCNN_REFINE_PLUS_ONE) ? 1.f : 0.f;
    const float w = x2 - x1 + one, h = y2 - y1 + one;
    x1 = x1 + b[5] * w; y1 = y1 + b[6] * h; x2 = x2 + b[7] * w; y2 = y2 + b[8] * h;
    if (flags & MQ_MTCNN_REFINE_REREC) {
        const float hh = y2 - y1, ww = x2 - x1, side = fmaxf(ww, hh);
        x1 = x1 + ww * 0.5f - side * 0.5f;
        y1 = y1 + hh * 0.5f - side * 0.5f;
        x2 = x1 + side;
        y2 = y1 + side;
    }
    float* o = out_rec + k * REC;
    o[0] = x1; o[1] = y1; o[2] = x2; o[3] = y2; o[4] = b[4];
    o[5] = 0.f; o[6] = 0.f; o[7] = 0.f; o[8] = 0.f;
    out_img[k] = g;
    const int H = hw[2 * g], W = hw[2 * g + 1];
    int x = __float2int_rz(x1), y = __float2int_rz(y1), ex = __float2int_rz(x2), ey = __float2int_rz(y2);
    if (x < 1) x = 1;
    if (y < 1) y = 1;
    if (ex > W) ex = W;
    if (ey > H) ey = H;
    out_pad[4 * k] = y; out_pad[4 * k + 1] = ey; out_pad[4 * k + 2] = x; out_pad[4 * k + 3] = ex;
    const bool ok = ey > y - 1 && ex > x - 1;
    valid[k] = ok ? 1 : 0;
    int64_t* j = jobs + k * MQ_MTCNN_JOB;
    j[0] = g; j[1] = x - 1; j[2] = y - 1; j[3] = ok ? ex - (x - 1) : 0; j[4] = ok ? ey - (y - 1) : 0;
    j[5] = crop; j[6] = crop; j[7] = k * 3 * (int64_t)crop * crop;
}

// ------------------------------------------------------------------------------------------------ R-Net / O-Net
// the K x K taps of one input channel added to acc, in (ky, kx) order
template <int K>
__device__ __forceinline__ float taps(const float* __restrict__ wp, const float* ip, int W, float acc) {
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) acc = fmaf(wp[ky * K + kx], ip[ky * W + kx], acc);
    return acc;
}

// valid convolution of stride 1 + bias + PReLU of the output channels [co0, co0 + nco): LDS [Cin][H][W] -> LDS [nco][H-K+1][W-K+1].
// Four accumulators take the input channels ci = 0, 1, 2, 3 (mod 4) -- four independent FMA chains, each a quarter as long -- and are
// summed as (a0 + a1) + (a2 + a3), the bias in a0.
template <int K>
__device__ __forceinline__ void conv_prelu(const float* in, int Cin, int H, int W, const float* __restrict__ w,
                                           const float* __restrict__ bias, const float* __restrict__ slope, int co0, int nco,
                                           float* out, int tid, int nt) {
    const int Ho = H - K + 1, Wo = W - K + 1, plane = Ho * Wo;
    for (int o = tid; o < nco * plane; o += nt) {
        const int c = o / plane, r = o - c * plane, y = r / Wo, x = r - y * Wo, co = co0 + c;
        const float* wp = w + (int64_t)co * Cin * K * K;
        const float* ip = in + y * W + x;
        float a0 = bias[co], a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int ci = 0;
#pragma unroll 1
        for (; ci + 3 < Cin; ci += 4) {
            a0 = taps<K>(wp + ci * K * K, ip + ci * H * W, W, a0);
            a1 = taps<K>(wp + (ci + 1) * K * K, ip + (ci + 1) * H * W, W, a1);
            a2 = taps<K>(wp + (ci + 2) * K * K, ip + (ci + 2) * H * W, W, a2);
            a3 = taps<K>(wp + (ci + 3) * K * K, ip + (ci + 3) * H * W, W, a3);
        }
#pragma unroll 1
        for (; ci < Cin; ++ci) a0 = taps<K>(wp + ci * K * K, ip + ci * H * W, W, a0);
        out[o] = prelu((a0 + a1) + (a2 + a3), slope[co]);
    }
}

__host__ __device__ constexpr int pooled(int h, int k, int s) { return (h - k + s - 1) / s + 1; }  // ceil mode, no padding

// ceil-mode max-pool: LDS [C][H][W] -> LDS [C][pooled(H)][pooled(W)]; windows are clipped at the map's edge
__device__ __forceinline__ void maxpool(const float* in, int C, int H, int W, int k, int s, float* out, int tid, int nt) {
    const int Hp = pooled(H, k, s), Wp = pooled(W, k, s);
    for (int o = tid; o < C * Hp * Wp; o += nt) {
        const int c = o / (Hp * Wp), r = o - c * Hp * Wp, py = r / Wp, px = r - py * Wp;
        float best = -INFINITY;
        for (int y = py * s; y < min(py * s + k, H); ++y)
            for (int x = px * s; x < min(px * s + k, W); ++x) best = fmaxf(best, in[(c * H + y) * W + x]);
        out[o] = best;
    }
}

// dense + bias + PReLU: LDS in[n_in] -> LDS out[n_out]; w packed [n_in][n_out]; n_in is a multiple of 4.  Four accumulators take
// the inputs i = 0, 1, 2, 3 (mod 4), summed as (a0 + a1) + (a2 + a3), the bias in a0.
__device__ __forceinline__ void dense_prelu(const float* in, int n_in, int n_out, const float* __restrict__ w,
                                            const float* __restrict__ bias, const float* __restrict__ slope, float* out, int tid, int nt) {
    for (int j = tid; j < n_out; j += nt) {
        float a0 = bias[j], a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 2
        for (int i = 0; i < n_in; i += 4) {
            a0 = fmaf(w[(int64_t)i * n_out + j], in[i], a0);
            a1 = fmaf(w[(int64_t)(i + 1) * n_out + j], in[i + 1], a1);
            a2 = fmaf(w[(int64_t)(i + 2) * n_out + j], in[i + 2], a2);
            a3 = fmaf(w[(int64_t)(i + 3) * n_out + j], in[i + 3], a3);
        }
        out[j] = prelu((a0 + a1) + (a2 + a3), slope[j]);
    }
}

// one head output: w [n_out][n_in] as published
__device__ __forceinline__ float head(const float* in, int n_in, const float* __restrict__ w, float bias) {
    float acc = bias;
    for (int i = 0; i < n_in; ++i) acc = fmaf(w[i], in[i], acc);
    return acc;
}

constexpr int RT = 256;
constexpr int R_A = 28 * 22 * 22, R_B = 48 * 9 * 9;

__global__ __launch_bounds__(RT) void rnet_kernel(const float* __restrict__ crops, const float* __restrict__ wt,
                                                  const int32_t* __restrict__ valid, float* __restrict__ rec) {
    __shared__ float A[R_A];
    __shared__ float B[R_B];
    const int64_t k = blockIdx.x;
    const int tid = threadIdx.x;
    float* o = rec + k * REC;
    if (valid && !valid[k]) {  // no crop: the box can never pass
        if (tid == 0) { o[4] = -INFINITY; o[5] = 0.f; o[6] = 0.f; o[7] = 0.f; o[8] = 0.f; }
        return;
    }
    for (int i = tid; i < 3 * 24 * 24; i += RT) B[i] = crops[k * (3 * 24 * 24) + i];
    __syncthreads();
    conv_prelu<3>(B, 3, 24, 24, wt + R_W1, wt + R_B1, wt + R_A1, 0, 28, A, tid, RT);   // 28 x 22 x 22
    __syncthreads();
    maxpool(A, 28, 22, 22, 3, 2, B, tid, RT);                                            // 28 x 11 x 11
    __syncthreads();
    conv_prelu<3>(B, 28, 11, 11, wt + R_W2, wt + R_B2, wt + R_A2, 0, 48, A, tid, RT);  // 48 x 9 x 9
    __syncthreads();
    maxpool(A, 48, 9, 9, 3, 2, B, tid, RT);                                              // 48 x 4 x 4
    __syncthreads();
    conv_prelu<2>(B, 48, 4, 4, wt + R_W3, wt + R_B3, wt + R_A3, 0, 64, A, tid, RT);    // 64 x 3 x 3
    __syncthreads();
    dense_prelu(A, 576, 128, wt + R_W4, wt + R_B4, wt + R_A4, B, tid, RT);
    __syncthreads();
    if (tid < 6) {
        const float v = tid < 2 ? head(B, 128, wt + R_W51 + tid * 128, wt[R_B51 + tid])
                                : head(B, 128, wt + R_W52 + (tid - 2) * 128, wt[R_B52 + tid - 2]);
        A[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        o[4] = softmax1(A[0], A[1]);
        for (int c = 0; c < 4; ++c) o[5 + c] = A[2 + c];
    }
}

constexpr int OT = 512;
constexpr int O_R0 = 32 * 23 * 23;                       // pool1; later conv3 / pool3 / conv4 / dense5
constexpr int O_IN = 3 * 48 * 48, O_T1 = 4 * 46 * 46;    // input + one group of conv1
constexpr int O_T2 = 16 * 21 * 21, O_P2 = 64 * 10 * 10;  // one group of conv2 + pool2 (reuse the input's region)
constexpr int O_R1 = O_IN + O_T1;
static_assert(O_T2 + O_P2 <= O_R1, "conv2's group and pool2 reuse the input region");
static_assert((O_R0 + O_R1) * 4 <= 160 * 1024, "LDS budget");

__global__ __launch_bounds__(OT) void onet_kernel(const float* __restrict__ crops, const float* __restrict__ wt,
                                                  const int32_t* __restrict__ valid, float* __restrict__ rec,
                                                  float* __restrict__ pts) {
    __shared__ float R0[O_R0];
    __shared__ float R1[O_R1];
    const int64_t k = blockIdx.x;
    const int tid = threadIdx.x;
    float* o = rec + k * REC;
    if (valid && !valid[k]) {
        if (tid == 0) { o[4] = -INFINITY; o[5] = 0.f; o[6] = 0.f; o[7] = 0.f; o[8] = 0.f; }
        if (tid < 10) pts[k * 10 + tid] = 0.f;
        return;
    }
    float* in = R1;
    float* t1 = R1 + O_IN;
    for (int i = tid; i < O_IN; i += OT) in[i] = crops[k * O_IN + i];
    __syncthreads();
    for (int co0 = 0; co0 < 32; co0 += 4) {  // conv1 (46 x 46) four channels at a time, pooled 3/2 into 23 x 23
        conv_prelu<3>(in, 3, 48, 48, wt + O_W1, wt + O_B1, wt + O_A1, co0, 4, t1, tid, OT);
        __syncthreads();
        maxpool(t1, 4, 46, 46, 3, 2, R0 + co0 * 23 * 23, tid, OT);
        __syncthreads();
    }
    float* t2 = R1;
    float* p2 = R1 + O_T2;
    for (int co0 = 0; co0 < 64; co0 += 16) {  // conv2 (21 x 21) sixteen channels at a time, pooled 3/2 into 10 x 10
        conv_prelu<3>(R0, 32, 23, 23, wt + O_W2, wt + O_B2, wt + O_A2, co0, 16, t2, tid, OT);
        __syncthreads();
        maxpool(t2, 16, 21, 21, 3, 2, p2 + co0 * 100, tid, OT);
        __syncthreads();
    }
    float* c3 = R0;
    float* p3 = R0 + 64 * 8 * 8;
    float* c4 = p3 + 64 * 4 * 4;
    float* d5 = c4 + 128 * 3 * 3;
    float* hd = d5 + 256;
    conv_prelu<3>(p2, 64, 10, 10, wt + O_W3, wt + O_B3, wt + O_A3, 0, 64, c3, tid, OT);   // 64 x 8 x 8
    __syncthreads();
    maxpool(c3, 64, 8, 8, 2, 2, p3, tid, OT);                                               // 64 x 4 x 4
    __syncthreads();
    conv_prelu<2>(p3, 64, 4, 4, wt + O_W4, wt + O_B4, wt + O_A4, 0, 128, c4, tid, OT);    // 128 x 3 x 3
    __syncthreads();
    dense_prelu(c4, 1152, 256, wt + O_W5, wt + O_B5, wt + O_A5, d5, tid, OT);
    __syncthreads();
    if (tid < 16) {
        float v;
        if (tid < 2) v = head(d5, 256, wt + O_W61 + tid * 256, wt[O_B61 + tid]);
        else if (tid < 6) v = head(d5, 256, wt + O_W62 + (tid - 2) * 256, wt[O_B62 + tid - 2]);
        else v = head(d5, 256, wt + O_W63 + (tid - 6) * 256, wt[O_B63 + tid - 6]);
        hd[tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        o[4] = softmax1(hd[0], hd[1]);
        for (int c = 0; c < 4; ++c) o[5 + c] = hd[2 + c];
    }
    if (tid < 10) pts[k * 10 + tid] = hd[6 + tid];
}

// landmarks to pixels from the box the crop was cut for, then the last box regression (in place)
__global__ __launch_bounds__(256) void onet_post_kernel(float* __restrict__ rec, float* __restrict__ pts, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float* b = rec + k * REC;
    const float x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
    const float w = x2 - x1 + 1.f, h = y2 - y1 + 1.f;
    for (int i = 0; i < 5; ++i) {
        pts[k * 10 + i] = w * pts[k * 10 + i] + x1 - 1.f;
        pts[k * 10 + 5 + i] = h * pts[k * 10 + 5 + i] + y1 - 1.f;
    }
    b[0] = x1 + b[5] * w; b[1] = y1 + b[6] * h; b[2] = x2 + b[7] * w; b[3] = y2 + b[8] * h;
}

}  // namespace

extern "C" {

int mq_mtcnn_weight_floats(int net) {
    return net == MQ_MTCNN_PNET ? P_TOTAL : net == MQ_MTCNN_RNET ? R_TOTAL : net == MQ_MTCNN_ONET ? O_TOTAL : 0;
}

int mq_mtcnn_resample_u8_f32(const uint8_t* images_dev, const int64_t* offsets_dev, const int32_t* hw_dev, int n_images,
                             const int64_t* jobs_dev, int64_t n_jobs, int64_t max_out_pixels, float* out_dev, int64_t out_floats,
                             int32_t* overflow_dev, void* stream) {
    if (n_jobs == 0) return MQ_OK;
    if (!images_dev || !offsets_dev || !hw_dev || !jobs_dev || !out_dev || !overflow_dev || n_images <= 0 || n_jobs < 0 ||
        n_jobs > 0x7fffffff || max_out_pixels <= 0 || out_floats <= 0)
        return MQ_EINVAL;
    int64_t by = (max_out_pixels + 255) / 256;
    if (by > 64) by = 64;
    resample_kernel<<<dim3((unsigned)n_jobs, (unsigned)by), 256, 0, (hipStream_t)stream>>>(images_dev, offsets_dev, hw_dev, n_images,
                                                                                           jobs_dev, out_dev, out_floats, overflow_dev);
    return mq_launch_status();
}

int mq_mtcnn_pnet_f32(const float* in_dev, int64_t in_floats, const int64_t* levels_dev, const float* level_scale_dev, int n_levels,
                      int max_tiles, const float* weights_dev, float threshold, int n_images, int cap, float* rec_dev, int32_t* idx_dev,
                      int32_t* sub_dev, int32_t* count_dev, int32_t* overflow_dev, float* maps_dev, int64_t maps_floats, void* stream) {
    if (!count_dev || !overflow_dev || n_images <= 0 || n_levels < 0) return MQ_EINVAL;
    MQ_HIP(hipMemsetAsync(count_dev, 0, sizeof(int32_t) * (size_t)n_images, (hipStream_t)stream));
    MQ_HIP(hipMemsetAsync(overflow_dev, 0, sizeof(int32_t), (hipStream_t)stream));
    if (n_levels == 0) return MQ_OK;
    if (!in_dev || !levels_dev || !level_scale_dev || !weights_dev || !rec_dev || !idx_dev || !sub_dev || cap <= 0 || max_tiles <= 0 ||
        n_levels > 65535 || in_floats <= 0 || (maps_dev && maps_floats <= 0))
        return MQ_EINVAL;
    pnet_kernel<<<dim3((unsigned)max_tiles, (unsigned)n_levels), 256, 0, (hipStream_t)stream>>>(
        in_dev, in_floats, levels_dev, level_scale_dev, weights_dev, threshold, n_images, cap, rec_dev, idx_dev, sub_dev, count_dev,
        overflow_dev, maps_dev, maps_floats);
    return mq_launch_status();
}

size_t mq_mtcnn_nms_workspace_bytes(int64_t n_total) { return n_total > 0 ? (size_t)n_total * 9 * 4 : 0; }

int mq_mtcnn_nms_f32(const float* rec_dev, int64_t n_total, const int64_t* seg_start_dev, const int32_t* seg_count_dev, int n_seg,
                     int64_t seg_cap,
                     const int32_t* key_dev, const int32_t* sub_dev, float score_gt, float threshold, int mode, float* out_rec_dev,
                     int32_t* out_key_dev, int32_t* out_sub_dev, int32_t* out_src_dev, int32_t* out_count_dev, void* ws_dev,
                     size_t ws_bytes, void* stream) {
    if (n_seg == 0) return MQ_OK;
    if (!seg_start_dev || !seg_count_dev || !out_count_dev || n_seg < 0 || n_total < 0 || seg_cap < 0 || (mode != MQ_MTCNN_NMS_UNION && mode != MQ_MTCNN_NMS_MIN))
        return MQ_EINVAL;
    if (n_total > 0 && (!rec_dev || !out_rec_dev || !ws_dev)) return MQ_EINVAL;
    if (ws_bytes < mq_mtcnn_nms_workspace_bytes(n_total)) return MQ_EWORKSPACE;
    float* ws_f = (float*)ws_dev;
    int32_t* ws_i = (int32_t*)ws_dev + 5 * n_total;
    nms_kernel<<<(unsigned)n_seg, NT, 0, (hipStream_t)stream>>>(rec_dev, n_total, seg_start_dev, seg_count_dev, seg_cap, key_dev, sub_dev, score_gt,
                                                               threshold, mode == MQ_MTCNN_NMS_MIN, out_rec_dev, out_key_dev,
                                                               out_sub_dev, out_src_dev, out_count_dev, ws_f, ws_i);
    return mq_launch_status();
}

int mq_mtcnn_refine_f32(const float* in_rec_dev, const int64_t* seg_start_dev, const int64_t* dst_start_dev, int n_seg, int64_t total,
                        const int32_t* hw_dev, int flags, int crop_size, int64_t out_cap, float* out_rec_dev, int32_t* out_img_dev,
                        int32_t* out_pad_dev, int64_t* jobs_dev, int32_t* valid_dev, int32_t* overflow_dev, void* stream) {
    if (total == 0) return MQ_OK;
    if (!in_rec_dev || !seg_start_dev || !dst_start_dev || !hw_dev || !out_rec_dev || !out_img_dev || !out_pad_dev || !jobs_dev ||
        !valid_dev || !overflow_dev || n_seg <= 0 || total < 0 || crop_size <= 0 || out_cap <= 0)
        return MQ_EINVAL;
    refine_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(in_rec_dev, seg_start_dev, dst_start_dev, n_seg, hw_dev,
                                                                                  flags, crop_size, out_cap, out_rec_dev, out_img_dev,
                                                                                  out_pad_dev, jobs_dev, valid_dev, overflow_dev);
    return mq_launch_status();
}

int mq_mtcnn_rnet_f32(const float* crops_dev, int64_t n, const float* weights_dev, const int32_t* valid_dev, float* rec_dev,
                      void* stream) {
    if (n == 0) return MQ_OK;
    if (!crops_dev || !weights_dev || !rec_dev || n < 0 || n > 0x7fffffff) return MQ_EINVAL;
    rnet_kernel<<<(unsigned)n, RT, 0, (hipStream_t)stream>>>(crops_dev, weights_dev, valid_dev, rec_dev);
    return mq_launch_status();
}

int mq_mtcnn_onet_f32(const float* crops_dev, int64_t n, const float* weights_dev, const int32_t* valid_dev, float* rec_dev,
                      float* points_dev, int flags, void* stream) {
    if (n == 0) return MQ_OK;
    if (!crops_dev || !weights_dev || !rec_dev || !points_dev || n < 0 || n > 0x7fffffff) return MQ_EINVAL;
    onet_kernel<<<(unsigned)n, OT, 0, (hipStream_t)stream>>>(crops_dev, weights_dev, valid_dev, rec_dev, points_dev);
    MQ_HIP(hipGetLastError());
    if (flags & MQ_MTCNN_ONET_POST) {
        onet_post_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(rec_dev, points_dev, n);
        MQ_HIP(hipGetLastError());
    }
    return MQ_OK;
}

}  // extern "C"
