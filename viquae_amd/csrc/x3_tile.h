// The pieces that the split-bf16 convolution tile kernels share: conv3x3_x3s_kernel and conv3x3_patch_kernel (conv.hip) and
// conv1x1_x3s_kernel (resnet.hip).  The kernels themselves stay apart.
#pragma once
#include "device_common.h"

namespace mq_dev {

// Workgroup b runs on XCD b & 7.  Each XCD takes a CONTIGUOUS range of row blocks (per = ceil(ntm / 8) of them) and all column tiles
// of a row block: the tiles its CUs hold at one time are neighbours in the image, so the halo rows two row blocks share (2 of a
// 512-pixel tile's 4.6 image rows at 112 x 112) and a row block's A rows are fetched into that XCD's L2 once.  The grid is padded to
// 8 * per * ntn workgroups; false = this one has no tile.
__device__ __forceinline__ bool xcd_tile(int b, int ntm, int ntn, int* mt, int* nt) {
    const int per = (ntm + 7) >> 3;
    *mt = __builtin_amdgcn_readfirstlane((b & 7) * per + (b >> 3) / ntn);
    *nt = __builtin_amdgcn_readfirstlane((b >> 3) % ntn);
    return !((b >> 3) / ntn >= per || *mt >= ntm);
}

// One K step (32 k) of a wave's 64 x 32 NF tile from an LDS stage of 64-byte rows whose 16-byte chunks are XOR-swizzled by (row >> 2) & 3.
// as / ws: this lane's row (lane & 31) of the hi arrays of A and W, the lo arrays A_BYTES / W_BYTES further; kg = lane >> 5, sww = the
// lane's swizzle key.  Per 16 k the fragment reads, then the products lo.hi, hi.lo, hi.hi on v_mfma_f32_32x32x16_bf16 for every
// accumulator -- the order of gemm_nt_x3s_kernel, so the implicit and the explicit convolutions give the same bits.
template <int NF>
__device__ __forceinline__ void x3_step(const char* as, const char* ws, int A_BYTES, int W_BYTES, int kg, int sww, f32x16 (&acc)[2][NF]) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int o = ((2 * m + kg) ^ sww) * 16;
        bf16x8_t ah[2], al[2], wh[NF], wl[NF];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            ah[x] = *reinterpret_cast<const bf16x8_t*>(as + x * 32 * 64 + o);
            al[x] = *reinterpret_cast<const bf16x8_t*>(as + A_BYTES + x * 32 * 64 + o);
        }
#pragma unroll
        for (int y = 0; y < NF; ++y) {
            wh[y] = *reinterpret_cast<const bf16x8_t*>(ws + y * 32 * 64 + o);
            wl[y] = *reinterpret_cast<const bf16x8_t*>(ws + W_BYTES + y * 32 * 64 + o);
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < NF; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[x], wh[y], acc[x][y], 0, 0, 0);
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < NF; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[x], wl[y], acc[x][y], 0, 0, 0);
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < NF; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[x], wh[y], acc[x][y], 0, 0, 0);
    }
}

}  // namespace mq_dev
