// Device helpers shared by the .hip translation units of libmeerqat_hip.so: the vector types, the LDS-DMA pieces, the PAIR LAYOUT,
// the split-bf16 arithmetic and the wave reductions.  These are contracts between producers and consumers in different files, so
// each is stated here once.  Everything is __device__ __forceinline__; a translation unit says `using namespace mq_dev;` and keeps
// its kernels in its own anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mq_dev {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) char lds_char;

// ---- LDS-DMA ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned lds_addr_of(const void* p) { return (unsigned)(unsigned long)(lds_char*)p; }
// one 1-KiB LDS-DMA piece, LDS destination lds_dst (wave-uniform) + lane * 16.  Issued from inline asm so hipcc does not drain it in
// front of the next ds_read.  Source: a wave-uniform 64-bit base (SGPR pair) + a per-lane 32-bit byte offset (the per-step address
// update is scalar arithmetic only) ...
__device__ __forceinline__ void dma16s(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// ... or a 64-bit source address per lane (the gather)
__device__ __forceinline__ void dma16v(const void* lane_ptr, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(lane_ptr), "s"(lds_dst) : "memory");
}
// dma16s with the non-temporal cache policy (streamed-once operands; measured per kernel)
__device__ __forceinline__ void dma16s_nt(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// dma16s with the sc1 policy: the aux pieces of the streaming screening scan
__device__ __forceinline__ void dma16s_sc1(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 sc1\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}
// a 4-byte-per-lane LDS-DMA piece (256 bytes per full wave; inactive lanes move nothing): LDS destination = lds_dst + lane * 4
__device__ __forceinline__ void dma4s(const void* sbase, unsigned voff, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(voff), "s"(sbase), "s"(lds_dst) : "memory");
}

// ---- PAIR LAYOUT -----------------------------------------------------------------------------------------------------------------
// The (hi, lo) arrays of a split activation [M, K] (K a multiple of 32) are stored tile by tile, exactly like the weights of
// split_bf16_tiled_kernel (encoder.hip): element (row, col) lives at pair_index(row, col, K) = [row / 256][col / 32][row % 256][col % 32],
// and the arrays hold ceil(M / 256) * 256 * K elements (rows beyond M are never written, and never read: the GEMM's A stream
// re-reads row M - 1 instead).  The A operand of one K step of a GEMM tile is then one contiguous 16-KiB block; 8 consecutive
// columns of a row (what the producers store at once) stay 16 contiguous bytes.
__device__ __forceinline__ size_t pair_index(size_t row, int col, int K) {
    return ((row >> 8) * (size_t)(K >> 5) + (size_t)(col >> 5)) * (256 * 32) + ((row & 255) << 5) + (size_t)(col & 31);
}

// ---- the split: hi = bf16(x), lo = bf16(x - hi) ------------------------------------------------------------------------------------
// Every producer of a split operand computes exactly this, so every consumer sees the same bits whichever kernel wrote them.
__device__ __forceinline__ void split1(float x, __bf16& h, __bf16& l) {
    h = (__bf16)x;
    l = (__bf16)(x - (float)h);
}
// split8 / split4 spell split1's two lines in their own loops: routed through split1 the compiler orders the vector inserts
// differently and several kernels come out with another instruction schedule.
__device__ __forceinline__ void split8(const float (&t)[8], bf16x8_t& h8, bf16x8_t& l8) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 h = (__bf16)t[e];
        h8[e] = h;
        l8[e] = (__bf16)(t[e] - (float)h);
    }
}
__device__ __forceinline__ void split8(const float4& u, const float4& v, bf16x8_t& hi, bf16x8_t& lo) {
    const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
    split8(x, hi, lo);
}
// four values -> their packed (hi, lo) bf16 quadruples (8 bytes each)
__device__ __forceinline__ void split4(const float x0, const float x1, const float x2, const float x3, uint2& hi, uint2& lo) {
    const float x[4] = {x0, x1, x2, x3};
    bf16x4_t h4, l4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const __bf16 h = (__bf16)x[e];
        h4[e] = h;
        l4[e] = (__bf16)(x[e] - (float)h);
    }
    hi = __builtin_bit_cast(uint2, h4);
    lo = __builtin_bit_cast(uint2, l4);
}
// one value -> hi in the low half-word, lo in the high one
__device__ __forceinline__ unsigned split_bits(float x) {
    __bf16 h, l;
    split1(x, h, l);
    return (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, l) << 16);
}
__device__ __forceinline__ void join8(const bf16x8_t& h8, const bf16x8_t& l8, float (&t)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (float)h8[e] + (float)l8[e];   // exact in fp32: |lo| <= ulp(hi) / 2, 8 + 8 significant bits
}
// Lanes l and l^1 of a wave hold ADJACENT columns (even column in the even lane); after one DPP exchange the even lane stores the
// packed hi pair, the odd lane the packed lo pair -- one 4-byte store per lane.
__device__ __forceinline__ void store_split_pair(float x, bool valid, unsigned short* __restrict__ hi, unsigned short* __restrict__ lo,
                                                 size_t even_col_index, int lane) {
    const unsigned mine = split_bits(x);
    const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(0, (int)mine, 0xB1, 0xF, 0xF, false);  // lane ^ 1
    const bool odd = lane & 1;
    const unsigned ev = odd ? other : mine, od = odd ? mine : other;  // the pair's even / odd column
    const unsigned word = odd ? ((ev >> 16) | (od & 0xFFFF0000u)) : ((ev & 0xFFFFu) | (od << 16));
    if (valid) *reinterpret_cast<unsigned*>((odd ? lo : hi) + even_col_index) = word;
}

// ---- wave reductions: a butterfly over the 64 lanes (lane ^ 32, 16, 8, 4, 2, 1), every lane ends with the result ----------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
        const uint64_t w = ((uint64_t)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

}  // namespace mq_dev
