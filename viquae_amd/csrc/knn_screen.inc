// knn_screen.inc -- bf16 screening + exact fp32 re-scoring (included by knn.hip inside its namespace).
//
// The exact scan (knn_scan_kernel) is bound by the fp32 matrix pipe (157 TFLOP/s).  This path gets the
// SAME bit-exact result faster:
//   1. screen_scan_kernel / screen_scan16_kernel: S~ = bf16(X) . bf16(Q)^T on v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16
//      (16x the fp32 MFMA rate; the second is the default: same cycles, the chip holds a higher clock under it)
//      over a bf16 copy of the KB, with a pooled selection under a RELAXED threshold: a row is kept while
//      S~ >= tau - margin_q, where tau is ANY lower bound of the final k-th best S~ (the k-th largest of the
//      query's stripe maxima across all slabs, or a slab pool's own k-th best) and margin_q = 2*eps_q bounds
//      |S~ - S| from above (eps_q below).  Every row whose EXACT score can reach the exact top-k is therefore
//      kept.  Pools: 8 single-writer slices per (query, slab), left as they are at the end of the slab
//      (POOL_LAYOUT_SLICES; the two-waves streaming scan of one query tile, knn_small8.inc, fills two halves per pool
//      front to back: POOL_LAYOUT_HALVES, recorded in the workspace word behind the tile's overflow flag).
//   2. cand_select_kernel<walk>: per query, union of the slab pools (three walks: slices of few slabs entry by entry,
//      halves / slices of many slabs line by line), global k-th best S~ (radix selection), same relaxed filter
//      -> a few hundred candidate rows.
//   3. rescore_kernel: the exact score of each candidate = the k-ordered fp32 fma chain over the fp32
//      row (bit-identical to what the exact scan's MFMA accumulates).
//   4. final_select_kernel: exact top-k by (score desc, id asc) of the re-scored candidates -> D, I.
//   Anything that does not fit the bounded buffers (pathological ties / clustered data) raises a per-
//   query-tile overflow flag and that tile is recomputed by the exact scan: the result is exact always.
//
// Error bound.  With x~ = bf16(x), q~ = bf16(q) (round to nearest even):  q.x - q~.x~ = q.(x - x~) + (q - q~).x~, so
//   |q.x - q~.x~| <= ||q|| ||x - x~|| + ||q - q~|| ||x~||           (Cauchy-Schwarz; MEASURED rounding errors, about
//                                                                    half of the worst case 2^-8 ||q|| ||x||)
// products of bf16 values are exact in fp32; both accumulations (the bf16 MFMA's and the exact chain's) are fp32
// sums of dp terms: + dp (2^-22 + 2^-24) ||q|| ||x|| (the MFMA accumulation term is taken 4x the textbook bound).
//   eps_q = ||q|| max_x ||x - x~|| + ||q - q~|| max_x ||x~|| + dp 2.98e-7 ||q|| max_x ||x||
// with the maxima over the shard kept by mq_knn_screen_prepare (row_err_stats_kernel) and the query norms taken
// per call (screen_margin_kernel); margin_q = 2 eps_q, every factor rounded up for the fp32 evaluation of the bound.
//
// Centred screen (inner product).  For a fixed query, q.(x - c) = q.x - q.c ranks the rows exactly like q.x, whatever
// the vector c.  Dense-retrieval embeddings share a large common component (DPR, CLIP: the mean of the rows is a large
// part of every row), so the index rounds xc = x - c to bf16 instead of x, with c the mean of the first rows it was
// given: S~ = q~ . xc~, the two rounding terms of eps_q then carry max ||xc - xc~|| and max ||xc~|| -- the norms of the
// SMALL vectors -- and the thresholds, pools and candidate filter all live on the shifted scores.  Only the
// accumulation term keeps max(||x||, ||xc||): it also covers the fp32 chain of the exact scores, which runs on the
// uncentred rows.  fl(x - c) differs from x - c by 2^-24 relative per component: far inside that term.  The re-scoring
// reads the original fp32 rows, so D and I are unchanged.  The L2 screen centres the same way: it ranks by
// q.x - ||x||^2/2 = q.xc - ||x||^2/2 + q.c, its two extra columns keep -||x||^2/2 of the STORED rows, and the terms of
// its bound that carry ||x||^2 keep the uncentred maximum.

#define MQ_SMFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int SPOOL = 1024;                   // screening pool per (query, slab): k + (margin x local score density) rows fit
constexpr int SPR = SPOOL / 64;
constexpr int SBK = 64;                       // bf16 k-depth of one LDS stage (128-byte tile rows)
constexpr int S_OP_BYTES = TQ * SBK * 2;      // one operand tile, one stage = 32 KiB
constexpr int S_LDS_X = 0;                    // [2][256][64] bf16
constexpr int S_LDS_Q = 2 * S_OP_BYTES;       // [2][256][64] bf16
constexpr int NSL = 8;                        // pool slices per query: one per (row-panel wave, lane half) that feeds it
constexpr int SLCAP = SPOOL / NSL;            // 128 slots per slice
constexpr int S_LDS_CNT = 4 * S_OP_BYTES;     // scnt[256][8] int, thr[256] f32, marg[256] f32, wgflag
constexpr int S_LDS_TOTAL = S_LDS_CNT + (NSL + 2) * TQ * 4 + 16;
static_assert(S_LDS_TOTAL <= 160 * 1024, "LDS budget");
static_assert(SPOOL / 2 / NSL <= SLCAP - 64, "a compacted slice must stay below the compaction trigger");
constexpr int SMAX_SLOTS = 256;               // stripe maxima consulted per query (any subset of the stripes is a valid bound)
#ifndef RESCORE_COLS
#define RESCORE_COLS 32
#endif
constexpr int RMAX = 1024;                    // candidate rows per query handed to the exact re-scoring
constexpr int POOL_LAYOUT_SLICES = 0;         // a pool = NSL slices of SLCAP slots, slice z holding pcount[z] keys from its start
constexpr int POOL_LAYOUT_HALVES = 1;         // ... two halves of SPOOL / 2 slots filled front to back (pcount: the same fill as slices)
constexpr int CSEL_WALK_SLICES = 0;           // cand_select_kernel's pool walks: slices, few slabs with long pools (S < 64)
constexpr int CSEL_WALK_HALVES = 1;           // ... halves, line by line
constexpr int CSEL_WALK_SLICE_LINES = 2;      // ... slices, many slabs (S >= 64), line by line
constexpr int CSEL_WORK = 1024;               // cand_select: listed pool entries behind the slices' first keys (S >= 64)
constexpr int CSEL_PER = 16;                  // cand_select: pool keys per thread (256 threads -> 4096 per query)

constexpr unsigned short S16_ONE = 0x3F80;
__device__ __forceinline__ float s16_to_f32(unsigned short u) { return __uint_as_float((unsigned)u << 16); }
__device__ __forceinline__ unsigned short f32_to_bf16_rne(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7F800000u) == 0x7F800000u) return (unsigned short)((u >> 16) | ((u & 0xFFFFu) ? 0x40u : 0u));  // inf / nan
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// fp32 row-major [n, d] -> bf16 row-major [n, dp] (dp = d rounded up to 64, zero padded)
// aug (see "L2 through two extra columns" and "Inner product with centred queries" below): 0 = none; 1 = KB rows: columns d,
// d+1 = the bf16 pair (h, l) of -sqn[r] / 2; 2 = query rows: columns d, d+1 = 1, 1.  (KB rows of the centred-query screen --
// (h, l) of c . (x - c), the k-ordered fp32 fma chain over the row -- are to_bf16_rows_centred_kernel's.)
// center (may be NULL): a fixed vector c subtracted before the rounding -- q.(x - c) ranks the rows of one query exactly like
// q.x, and for embeddings that share a large common component the rounding error then scales with ||x - c|| (see
// "Centred screen" in the header of this file).
// dst is the WHOLE bf16 copy (KB or queries) in TILE layout: row R = tile_row0 + r, column k live at xb_tile_index(R, k, dp) =
// [R / 256][k / 64][R % 256][k % 64], i.e. the [256 rows][64 columns] operand tile of one K step of the screening scan is one
// contiguous 32-KiB block (src, sqn start at row tile_row0).
__device__ __forceinline__ size_t xb_tile_index(int64_t R, int k, int dp) {
    return (((size_t)(R / TN) * (size_t)(dp / SBK) + (size_t)(k / SBK)) * TN + (size_t)(R % TN)) * SBK + (size_t)(k % SBK);
}
__global__ void to_bf16_rows_kernel(const float* __restrict__ src, int64_t n, int d, int dp, unsigned short* __restrict__ dst,
                                    int aug, const float* __restrict__ sqn, const float* __restrict__ center, int64_t tile_row0) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // one thread per 4 output elements
    const int per_row = dp / 4;
    if (e >= n * per_row) return;
    const int64_t r = e / per_row;
    const int k = (int)(e - r * per_row) * 4;
    float xv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // (addresses inside the row, the tests afterwards: the four loads travel together)
        const int cc = k + j < d ? k + j : d - 1;
        xv[j] = src[r * d + cc];
    }
    if (center) {
        float cv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) cv[j] = center[k + j < d ? k + j : d - 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] -= cv[j];
    }
    unsigned short o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = k + j;
        o[j] = (c < d) ? f32_to_bf16_rne(xv[j]) : (unsigned short)0;
        if (aug == 2 && (c == d || c == d + 1)) o[j] = S16_ONE;  // 1.0
        if (aug == 1 && (c == d || c == d + 1)) {
            const float v = -0.5f * sqn[r];
            const unsigned short h = f32_to_bf16_rne(v);
            o[j] = (c == d) ? h : f32_to_bf16_rne(v - s16_to_f32(h));
        }
    }
    unsigned short* at = dst + xb_tile_index(tile_row0 + r, k, dp);
    *reinterpret_cast<uint2*>(at) = make_uint2((unsigned)o[0] | ((unsigned)o[1] << 16), (unsigned)o[2] | ((unsigned)o[3] << 16));
}

// to_bf16_rows_kernel with aug = 3 for KB rows (the centred-query screen), 64 rows per workgroup: there the one thread of a row
// that owns columns d, d + 1 walks the whole row for c . (x - c) on its own, element by element from global memory -- 2.9 ms per
// 65,536 x 2048 rows, 14 x what the copy itself needs (rocprofv3, round 5: the 2048-d index of the fusion config).  Here the
// workgroup passes [64 rows][64 columns] tiles of x - c through LDS: every thread rounds and stores its elements, thread r < 64
// continues row r's chain over the tile -- the same k-ordered fp32 fma chain on the same differences, the same bits.
__global__ __launch_bounds__(256) void to_bf16_rows_centred_kernel(const float* __restrict__ src, int64_t n, int d, int dp,
                                                                   unsigned short* __restrict__ dst,
                                                                   const float* __restrict__ center, int64_t tile_row0) {
    __shared__ float tile[64][65];
    __shared__ float cs[64];
    const int t = threadIdx.x, c = t & 63, rb = t >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    float v = 0.f;
    for (int kc = 0; kc < dp; kc += 64) {
        const int col = kc + c;
        const float cen = center[col < d ? col : d - 1];
        float x[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {  // addresses inside the matrix whatever the row / column: no load under a test
            const int64_t row = row0 + rb + 4 * j;
            x[j] = src[(row < n ? row : n - 1) * (int64_t)d + (col < d ? col : d - 1)];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int r = rb + 4 * j;
            const float xc = x[j] - cen;
            tile[r][c] = xc;
            if (row0 + r < n && col != d && col != d + 1)  // (the pair's columns have ONE writer: thread r, below)
                dst[xb_tile_index(tile_row0 + row0 + r, col, dp)] = col < d ? f32_to_bf16_rne(xc) : (unsigned short)0;
        }
        if (t < 64) cs[t] = cen;
        __syncthreads();
        if (t < 64) {
            const int kn = d - kc < 64 ? d - kc : 64;
            for (int k = 0; k < kn; ++k) v = fmaf(cs[k], tile[t][k], v);
        }
        __syncthreads();
    }
    if (t < 64 && row0 + t < n) {
        const unsigned short h = f32_to_bf16_rne(v);
        dst[xb_tile_index(tile_row0 + row0 + t, d, dp)] = h;
        dst[xb_tile_index(tile_row0 + row0 + t, d + 1, dp)] = f32_to_bf16_rne(v - s16_to_f32(h));
    }
}

// Shard statistics of the error bound, updated by every mq_knn_screen_prepare call (atomic max on the bit patterns
// of non-negative floats): stats[0] = max ||x||^2, stats[1] = max ||x - bf16(x)||^2.  x - bf16(x) is exact in fp32;
// the fp32 sums carry a relative error <= (dp + 1) 2^-24, covered by the slack factors of screen_margin_kernel.
// A row with an inf / NaN element is skipped: its scores are non-finite on every path, or never enter a result.  A row of finite
// elements whose sums overflow is NOT harmless: with the inner product its scores stay finite against small queries (x ~ 2^64,
// q ~ 2^-64), so it records +inf in every statistic -- the margin turns infinite and the tiles fall back to the exact scan.  L2
// (l2 = 1) skips such a row when ||x||^2 itself overflows: its distance is then infinite on every path.  Sums that UNDERflow
// are covered in screen_margin_kernel (an absolute floor of d 2^-148 under every squared sum).
// stats[2] = max ||x - c||^2 (= stats[0] without a centre); stats[1] is then max ||(x - c) - bf16(x - c)||^2;
// stats[3] = max |c . (x - c)| (0 without a centre): the row term of the centred-query screen.
// xb = the whole bf16 copy (tile layout), rm = the row-major rows from row `row0` on.
__global__ __launch_bounds__(256) void row_err_stats_kernel(const float* __restrict__ rm, const unsigned short* __restrict__ xb,
                                                            int64_t n, int d, int dp, unsigned* __restrict__ stats,
                                                            const float* __restrict__ center, int64_t row0, int l2) {
    const int lane = threadIdx.x & 63;
    float ms2 = 0.f, me2 = 0.f, mc2 = 0.f, mv = 0.f;  // this wave's running maxima: one set of atomics per wave, not per row
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
        float s2 = 0.f, e2 = 0.f, c2 = 0.f, v = 0.f;
        int nf = 0;  // inf / NaN elements of the row
        for (int k = lane; k < d; k += 64) {
            const float x = rm[r * d + k];
            const float xc = center ? x - center[k] : x;
            const float e = xc - s16_to_f32(xb[xb_tile_index(row0 + r, k, dp)]);
            nf += !(fabsf(x) < INFINITY);
            s2 += x * x;
            e2 += e * e;
            c2 += xc * xc;
            if (center) v += center[k] * xc;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            s2 += __shfl_xor(s2, o); e2 += __shfl_xor(e2, o); c2 += __shfl_xor(c2, o); v += __shfl_xor(v, o); nf += __shfl_xor(nf, o);
        }
        if (s2 < INFINITY && e2 < INFINITY && c2 < INFINITY) {  // false for NaN as well
            ms2 = fmaxf(ms2, s2);
            me2 = fmaxf(me2, e2);
            mc2 = fmaxf(mc2, c2);
            mv = fmaxf(mv, fabsf(v) < INFINITY ? fabsf(v) : (nf == 0 ? INFINITY : 0.f));
        } else if (nf == 0 && !(l2 && !(s2 < INFINITY))) {  // finite elements, overflowing sums: see above
            ms2 = me2 = mc2 = mv = INFINITY;
        }
    }
    if (lane == 0) {
        atomicMax(stats, __float_as_uint(ms2));
        atomicMax(stats + 1, __float_as_uint(me2));
        atomicMax(stats + 2, __float_as_uint(mc2));
        atomicMax(stats + 3, __float_as_uint(mv));
    }
}

// margin[q] = 2 eps_q with (header, "Error bound")
//   eps_q = ||q|| max||x - x~|| + ||q - q~|| max||x~|| + dp 2.98e-7 ||q|| max||x||,
// every factor rounded up by a slack that covers the fp32 evaluation of the norms themselves.
// L2 through two extra columns.  The exact path ranks by g = -max(0, d_f), d_f = fl(fl(qn + xn) - 2 S_f) (S_f the fp32
// chain, qn / xn the chain norms).  The screen scans x' = [x~, h, l], q' = [q~, 1, 1] with (h, l) the bf16 pair of -xn/2, so
// S~' ~= q.x - xn/2 = (qn - d)/2: the same ranking for one query.  Against G = (qn - d_f)/2 the screen is off by at most
//   eps' = ||q|| max||x - x~|| + ||q - q~|| max||x~|| + (dp' 2^-22 + d 2^-24) ||q|| max||x||      (as for IP)
//        + (dp' 2^-23 + 2^-17) max||x||^2      (MFMA accumulation over the two extra terms, residual of the (h, l) pair)
//        + 1.51 2^-24 (||q||^2 + max||x||^2)   (roundings inside d_f)
// and the clamp at d_f <= 0 ties rows whose G may differ by up to Gpos = (1.01 d + 1.51) 2^-24 (||q||^2 + max||x||^2):
// margin' = 2 eps' + Gpos keeps every row of the exact answer, clamped ties included (DESIGN.md).
// Inner product with centred queries (mode 2, round 5).  With c the centre of the bf16 copy, qc = q - c and xc = x - c:
//   q.x = qc.xc + c.xc + q.c,
// and q.c is one constant per query: the rows of a query rank by qc.xc + v, v = c.xc -- a per-ROW term, carried like the L2
// metric's -xn/2 as the bf16 pair (h, l) in two extra columns against (1, 1) in the query.  The roundings then live on qc and
// xc BOTH: embeddings that share a large common component (image features: non-negative, far from centred) keep a margin
// that follows the spread of the scores; with q uncentred it followed ||q||, and at d = 2048 a shared component twice the
// isotropic part sent every query tile to the exact scan (profiles/r05_notes.md).  Against the fp32 chain S_f of q.x:
//   eps'' = ||qc|| max||xc - xc~|| + ||qc - qc~|| max||xc~||                       (the two roundings)
//         + dp' 2^-22 (||qc|| max||xc|| + max|v|)                                  (fp32 accumulation in the MFMA, 4x the textbook bound)
//         + d 2^-24 ||q|| max||x||                                                 (the chain S_f itself)
//         + (2^-17 + d 2^-24 (1 + ||c|| max||xc|| / max|v|)) max|v|                (residual of the (h, l) pair, the chain of v)
//         + 2^-23 (||q|| + ||qc||) max||xc||                                       (qc and xc are themselves fp32 differences)
__global__ __launch_bounds__(256) void screen_margin_kernel(const float* __restrict__ q_rm, const unsigned short* __restrict__ Qb,
                                                            const float* __restrict__ xstats, int nq, int nqpad, int d, int dp,
                                                            float* __restrict__ margin, int mode, const float* __restrict__ center,
                                                            unsigned* __restrict__ zero, size_t zero_words) {
    // the call's overflow flags, shared thresholds and stripe maxima start from zero: cleared here, ahead of the scan like the
    // margins, rather than by a launch of their own (one query tile: every launch of the call is ~0.5 % of it)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < zero_words; i += (size_t)gridDim.x * 256) zero[i] = 0u;
    const int l2 = mode == 1;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per query
    const int lane = threadIdx.x & 63;
    if (q >= nqpad) return;
    if (q >= nq) { if (lane == 0) margin[q] = -1.f; return; }  // padding query of the last tile: never selects anything
    float q2 = 0.f, dq2 = 0.f, qu2 = 0.f, c2 = 0.f;
    // four strides of the lane per step, their loads in flight together (one query tile: a round trip per stride was most of
    // this kernel); the sums run in the same order as one stride at a time
    for (int k0 = lane; k0 < d; k0 += 256) {
        float u4[4], c4[4];
        unsigned short b4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k0 + 64 * j < d ? k0 + 64 * j : d - 1;
            u4[j] = q_rm[(size_t)q * d + kk];
            c4[j] = (mode == 2) ? center[kk] : 0.f;
            b4[j] = Qb[xb_tile_index(q, kk, dp)];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k0 + 64 * j < d) {
                const float u = u4[j], cv = c4[j];
                const float v = u - cv;  // what to_bf16_rows_kernel rounded
                const float e = v - s16_to_f32(b4[j]);
                q2 += v * v;
                dq2 += e * e;
                qu2 += u * u;
                c2 += cv * cv;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { q2 += __shfl_xor(q2, o); dq2 += __shfl_xor(dq2, o); qu2 += __shfl_xor(qu2, o); c2 += __shfl_xor(c2, o); }
    // Underflow: a square or a sum below 2^-126 is rounded with an ABSOLUTE error of at most 2^-150, so each of these sums of d
    // squares (and the chain of c . xc) can fall short by at most d 2^-150 -- even to 0 for a non-zero row (x ~ 2^-66: the
    // rounding errors squared vanish while the scores, against queries ~ 2^66, stay ordinary numbers).  uf = d 2^-148 added
    // under every sum keeps each factor an upper bound; at ordinary scales it is far below the sums' last bit.
    const float uf = (float)d * 0x1p-148f;
    const float qn = sqrtf(q2 + uf) * 1.001f, dqn = sqrtf(dq2 + uf) * 1.001f;
    // xstats: max ||x||^2, max ||xc - xc~||^2, max ||xc||^2 with xc = x - c the rows the screen actually rounds (c = 0
    // unless the index centred its bf16 copy).  The two rounding terms live on the centred rows; the accumulation
    // slack covers the bf16 MFMA on (q~, xc~) AND the fp32 chain of the exact scores on (q, x): it takes the larger norm.
    const float xun = sqrtf(xstats[0] + uf) * 1.001f, dxn = sqrtf(xstats[1] + uf) * 1.001f, xcn = sqrtf(xstats[2] + uf) * 1.001f;
    const float xn = fmaxf(xun, xcn);
    // A factor that overflowed (+inf) times one that underflowed (0) would make the margin NaN, and a NaN margin reads as a
    // padding query (margin >= 0 false) to every kernel behind this one: any margin that is not a number >= 0 becomes +inf,
    // which keeps every row and sends the tile to the exact scan.
    if (mode == 2) {
        const float qun = sqrtf(qu2 + uf) * 1.001f, cn = sqrtf(c2 + uf) * 1.001f, vmax = (xstats[3] + uf) * 1.001f;
        const float u = 5.9604645e-8f;  // 2^-24
        float eps = qn * dxn + dqn * xcn * 1.002f;
        eps += (float)dp * 2.3842e-7f * 1.004f * (qn * xcn + vmax);
        eps += (float)d * u * 1.004f * qun * xun;
        eps += 7.63e-6f * vmax + (float)d * u * 1.004f * (vmax + cn * xcn);
        eps += 2.0f * u * (qun + qn) * xcn;
        const float m = (2.0f * eps) * 1.001f + 1e-30f;
        if (lane == 0) margin[q] = m >= 0.f ? m : INFINITY;
        return;
    }
    // dp * (2^-22 for the bf16 MFMA's fp32 accumulation, taken 4x the textbook bound because its internal summation
    // order/rounding is not documented, + 2^-24 for the exact chain), on ||q~|| ||x~|| <= 1.004 ||q|| ||x||
    const float acc = (float)dp * 2.98e-7f * 1.004f;
    float eps = qn * dxn + dqn * xcn * 1.002f + acc * qn * xn;
    float extra = 0.f;
    if (l2) {
        const float x2 = xn * xn, q2u = qn * qn, u = 5.9604645e-8f;  // 2^-24
        eps += ((float)dp * 1.2e-7f + 7.63e-6f) * x2 + 1.51f * u * (q2u + x2);
        extra = (1.01f * (float)d + 1.51f) * u * (q2u + x2);
    }
    const float m = (2.0f * eps + extra) * 1.001f + 1e-30f;
    if (lane == 0) margin[q] = m >= 0.f ? m : INFINITY;
}

struct ScreenArgs {
    const unsigned short* Xb;  // KB, bf16, tile layout [rows / 256][dp / 64][256][64] (xb_tile_index)
    const unsigned short* Qb;  // queries, bf16, tile layout like Xb ([nqpad / 256][dp / 64][256][64])
    const float* margin;       // [nqpad]
    u64* pools;                // [nqt][S][256][SPOOL] unsorted keys (score = S~)
    int* pcount;               // [nqt][S][256][NSL] entries per pool slice at the end of the slab
    int* ovf;                  // [nqt] overflow flags (tile must be recomputed by the exact scan)
    unsigned long long* dbg;   // MQ_TIMING builds only
    unsigned* gthr;            // [nqpad] shared across slabs: max over slabs of the slab's k-th best S~ (orderable bits, 0 = none)
    unsigned* smax;            // [nqpad][ms] stripe maxima (orderable score words, 0 = none), see screen_scan_kernel
    int ms;                    // stripe slots per query (<= SMAX_SLOTS)
    int sps;                   // stripe slots per slab: a slab's 16 stripes fold into sps slots (atomic max)
    long long N;
    int dp, nqt, S, k, qpx;
    long long nchunks;
};

template <int R>
__device__ __forceinline__ u64 wave_kth_largest_n(const u64 (&v)[R], int k) {
    unsigned Th = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = Th | (1u << bit);
        int c = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64((unsigned)(v[r] >> 32) >= cand));
        if (c >= k) Th = cand;
    }
    int cgt = 0, ceq = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        cgt += __builtin_popcountll(__builtin_amdgcn_ballot_w64((unsigned)(v[r] >> 32) > Th));
        ceq += __builtin_popcountll(__builtin_amdgcn_ballot_w64((unsigned)(v[r] >> 32) == Th));
    }
    if (cgt + ceq == k) return (u64)Th << 32;
    const int need = k - cgt;
    unsigned Tl = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = Tl | (1u << bit);
        int c = 0;
#pragma unroll
        for (int r = 0; r < R; ++r)
            c += __builtin_popcountll(__builtin_amdgcn_ballot_w64((unsigned)(v[r] >> 32) == Th && (unsigned)v[r] >= cand));
        if (c >= need) Tl = cand;
    }
    return ((u64)Th << 32) | Tl;
}

// all-to-all reductions inside a 16-lane DPP row: xor 1, xor 2 (quad_perm), 7-i (row_half_mirror), 15-i (row_mirror)
__device__ __forceinline__ int row16_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);
    return v;
}
__device__ __forceinline__ unsigned row16_umin(unsigned v) {
    unsigned o;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false); v = o < v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false); v = o < v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false); v = o < v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false); v = o < v ? o : v;
    return v;
}
__device__ __forceinline__ unsigned row16_umax(unsigned v) {
    unsigned o;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false); v = o > v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false); v = o > v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false); v = o > v ? o : v;
    o = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false); v = o > v ? o : v;
    return v;
}

// Relaxed compaction of one query's pool by one wave.  The pool is 8 slices of 128 slots; slice s is
// appended to by exactly one lane (private counter, no atomics).  Keeps every key whose score is
// >= (k-th best score) - margin and refreshes the query's relaxed threshold.  Survivors are dealt
// round-robin back to the slices.
// Returns the survivor count, negated when they exceed SURV_MAX (the caller flags the tile; only the
// exact top-k are kept then).
constexpr int SURV_MAX = SPOOL / 2;  // leaves >= 64 free slots per slice = two more chunks of appends
template <int NSL_ = NSL>  // slices per pool (SPOOL / NSL_ slots each)
__device__ __forceinline__ int compact_pool_relaxed(u64* __restrict__ P, int* __restrict__ scnt_q, int k, float margin,
                                                    float* thr_q, unsigned* gthr_q, int lane) {
    constexpr int SLCAP_ = SPOOL / NSL_, GPS = SLCAP_ / 64;  // 64-slot groups per slice
    u64 v[SPR];
    int g = 0;
#pragma unroll
    for (int r = 0; r < SPR; ++r) {
        const int cs = scnt_q[r / GPS];  // slice r/GPS holds slots [SLCAP_*(r/GPS), +SLCAP_); this lane: slot 64*(r%GPS)+lane
        const bool valid = ((r % GPS) * 64 + lane) < cs;
        v[r] = valid ? __hip_atomic_load(P + r * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
        if ((r % GPS) == 0) g += cs;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every slot is in registers before any slot is rewritten
    u64 cut = 1ull;  // g <= k: keep everything
    bool fits = true;
    if (g > k) {
        // A LOWER bound of the k-th best score suffices (the relaxed rule then keeps a superset): bisect the
        // orderable score word between the pool's min and max for a fixed number of steps instead of resolving
        // all 64 key bits -- ~3x cheaper than the exact selection, precision ~2^-14 of the score range.
        unsigned mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
        for (int r = 0; r < SPR; ++r) {
            const unsigned h = (unsigned)(v[r] >> 32);
            if (v[r] != 0ull) { mn = h < mn ? h : mn; mx = h > mx ? h : mx; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned a = (unsigned)__shfl_xor((int)mn, o), b = (unsigned)__shfl_xor((int)mx, o);
            mn = a < mn ? a : mn;
            mx = b > mx ? b : mx;
        }
        unsigned lo = mn, hi = mx + 1u;  // count(>= lo) = g >= k; count(>= hi) = 0 < k
        for (int it = 0; it < 14 && hi - lo > 1u; ++it) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            int c = 0;
#pragma unroll
            for (int r = 0; r < SPR; ++r) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64((unsigned)(v[r] >> 32) >= mid));
            if (c >= k) lo = mid; else hi = mid;
        }
        const u64 T = (u64)lo << 32;  // at least k keys are >= T
        if (lane == 0) atomicMax(gthr_q, lo);  // telemetry / future cross-slab pruning
        const float thr = fmaxf(key_score(T) - margin, *thr_q);  // the stripe-maxima bound may already be tighter
        const u64 Kthr = make_key(thr, 0xFFFFFFFFu);  // smallest key with score >= thr
        int c = 0;
#pragma unroll
        for (int r = 0; r < SPR; ++r) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(v[r] >= Kthr));
        fits = c <= SURV_MAX;
        cut = fits ? Kthr : wave_kth_largest_n<SPR>(v, k);
        if (lane == 0) *thr_q = thr;
    }
    int base = 0;
    const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < SPR; ++r) {
        const bool keep = v[r] != 0ull && v[r] >= cut;
        const u64 m = __builtin_amdgcn_ballot_w64(keep);
        if (keep) {
            const int sidx = base + __builtin_popcountll(m & lt);
            P[(sidx % NSL_) * SLCAP_ + (sidx / NSL_)] = v[r];
        }
        base += __builtin_popcountll(m);
    }
    if (lane < NSL_) scnt_q[lane] = (base + NSL_ - 1 - lane) / NSL_;
    return fits ? base : -base;
}


// SHAPE selects the matrix instruction of the K loop and, with it, the accumulator layout the selection epilogue walks:
//   SCAN_MFMA_32  v_mfma_f32_32x32x16_bf16, four f32x16 accumulators per wave (2 x 2 sub-tiles of 32 x 32)
//   SCAN_MFMA_16  v_mfma_f32_16x16x32_bf16, sixteen f32x4 accumulators per wave (4 x 4 sub-tiles of 16 x 16)
// Same waves, wave tile, stages, LDS image, DMA and barrier; the same pools, counters, stripes and thresholds come out, so
// nothing behind the scan can tell the two apart (MQ_KNN_OPT_SCAN_MFMA picks the instance per launch).
constexpr int SCAN_MFMA_32 = 0, SCAN_MFMA_16 = 1;
template <int SHAPE>
__device__ __forceinline__ void screen_scan_body(const ScreenArgs& a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int* scnt = reinterpret_cast<int*>(smem + S_LDS_CNT);  // [256][8]
    float* thr = reinterpret_cast<float*>(scnt + TQ * NSL);
    float* marg = thr + TQ;
    int* wgflag = reinterpret_cast<int*>(marg + TQ);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w >> 2, wc = w & 3;

    int qt, slab;
    {
        const int b = blockIdx.x;
        if (a.qpx > 0) {
            const int ngroups = a.nqt / a.qpx, xpg = 8 / ngroups, spx = a.S / xpg;
            const int xcd = b & 7, j = b >> 3;
            qt = (xcd / xpg) * a.qpx + (j % a.qpx);
            slab = (xcd % xpg) * spx + j / a.qpx;
        } else {
            slab = b / a.nqt;
            qt = b % a.nqt;
        }
    }
    qt = __builtin_amdgcn_readfirstlane(qt);
    slab = __builtin_amdgcn_readfirstlane(slab);
    const int c0 = __builtin_amdgcn_readfirstlane((int)((a.nchunks * slab) / a.S));
    const int c1 = __builtin_amdgcn_readfirstlane((int)((a.nchunks * (slab + 1)) / a.S));
    const int k = a.k;
    u64* mypools = a.pools + ((size_t)qt * a.S + slab) * (size_t)TQ * SPOOL;

    if (tid < TQ) {
        for (int z = 0; z < NSL; ++z) scnt[tid * NSL + z] = 0;
        marg[tid] = a.margin[qt * TQ + tid];
        thr[tid] = marg[tid] < 0.f ? INFINITY : -INFINITY;
    }
    if (tid == 0) wgflag[0] = wgflag[1] = wgflag[2] = 0;

    // DMA: an operand tile stage is [256 rows][128 B]; one wave instruction moves 8 rows; wave w moves rows
    // [16w, 16w+16) of both operands.  16-byte chunk c of row r is stored at chunk c ^ ((r>>1)&7) so that the
    // fragment ds_read_b128 below are bank-conflict free; the swizzle is applied to the per-lane SOURCE chunk.
    const int nkb = a.dp / SBK;
    const int r8 = lane >> 3, ch = lane & 7;
    // Both bf16 operands are stored tile by tile (xb_tile_index): the operand of one K step is ONE contiguous 32-KiB block.
    // Row-major, a step's 256 pieces of 128 bytes sat 2 dp bytes apart -- at dp = 768 that is 12 cache lines, so the pieces of
    // a tile fell on a quarter of the L2 channels (and on 256 different DRAM pages when they came from HBM).  Measured, whole
    // search at 1.5M x 768, same box, same kernel otherwise: 4096 queries 8.65 -> 8.40 ms, 1024 queries 2.43 -> 2.35 ms,
    // 256 queries 0.91 -> 0.88 ms (profiles/r03_notes.md section 14).
    unsigned voff[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int r = 16 * w + 8 * u + r8;
        voff[u] = (unsigned)((r * SBK + (ch ^ ((r >> 1) & 7)) * 8) * 2);
    }
    const size_t chunk_bytes = (size_t)TN * a.dp * 2;  // = nkb tiles of S_OP_BYTES
    const char* const xbase0 = reinterpret_cast<const char*>(a.Xb);
    const char* const qbase0 = reinterpret_cast<const char*>(a.Qb) + (size_t)qt * chunk_bytes;
    const unsigned lds_x = __builtin_amdgcn_readfirstlane(lds_addr_of(smem + S_LDS_X + 16 * w * 128));
    const unsigned lds_q = __builtin_amdgcn_readfirstlane(lds_addr_of(smem + S_LDS_Q + 16 * w * 128));
    auto issue = [&](int c, int kb, int stage) __attribute__((always_inline)) {
        const char* xb = xbase0 + (size_t)c * chunk_bytes + (size_t)kb * S_OP_BYTES;
        const char* qb = qbase0 + (size_t)kb * S_OP_BYTES;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            dma16s(xb, voff[u], lds_x + stage * S_OP_BYTES + u * 1024);
            dma16s(qb, voff[u], lds_q + stage * S_OP_BYTES + u * 1024);
        }
    };

    // MFMA 32x32x16 bf16 operands: lane (i = lane&31, kg = lane>>5) holds k = 8*kg .. 8*kg+7 of row i
    // MFMA 16x16x32 bf16 operands: lane (i = lane&15, kg = lane>>4) holds k = 8*kg .. 8*kg+7 of row i; the sub-tiles' rows are
    // 16 apart, so (row >> 1) & 7 = (i >> 1) & 7 stays the swizzle term
    const int i = SHAPE == SCAN_MFMA_16 ? lane & 15 : lane & 31, kg = SHAPE == SCAN_MFMA_16 ? lane >> 4 : lane >> 5;
    const int sw = (i >> 1) & 7;
    const char* xrd = smem + S_LDS_X + (64 * wr + i) * 128;
    const char* qrd = smem + S_LDS_Q + (64 * wc + i) * 128;

    // Stripe maxima.  Each (lane, 32-row sub-tile) sees a fixed stripe of the slab's rows for its query: 16 rows of
    // every chunk.  The stripes of one query over all lanes / sub-tiles / slabs are DISJOINT row sets, so the j-th
    // largest of their running maxima is <= the j-th best S~ of the whole shard: a valid (and, with 16 S stripes,
    // tight: ~0.3 sigma under the true k-th best) lower bound of the global k-th best long before any pool holds k
    // good rows -- the per-slab pools alone only know the slab's own k-th best.  Maxima only grow, so stale reads
    // by other workgroups are still valid bounds.
    // 16x16x32: a stripe belongs to a (lane, query column) instead -- rows 16 a + 4 kg + reg (a = 0 .. 3) of the wave's 64,
    // again 16 rows of every chunk, stripe wr * 4 + kg of the query; that arm calls the four maxima rmc0 .. rmc3.
    float rm00 = -INFINITY, rm10 = -INFINITY, rm01 = -INFINITY, rm11 = -INFINITY;
    // When there are more than 16 slabs, a slab's 16 stripes fold into sps = 256 / S slots (atomic max): a slot then
    // holds the maximum over a union of stripes -- still disjoint row sets.
    const int ms = a.ms, sps = a.sps;
    const bool publish = slab * sps + sps <= ms;
    // stripe -> slot offsets of this wave's two lane halves (kg = 0 / 1), as scalars: sps need not be a power of two
    // 16x16x32: the same four values are the slots of the wave's four lane quarters kg = 0, 1, 2, 3 (a0, a1, b0, b1).
    const int so_a0 = __builtin_amdgcn_readfirstlane((wr * 4) % sps), so_a1 = __builtin_amdgcn_readfirstlane((wr * 4 + 1) % sps);
    const int so_b0 = __builtin_amdgcn_readfirstlane((wr * 4 + 2) % sps), so_b1 = __builtin_amdgcn_readfirstlane((wr * 4 + 3) % sps);
    // Everything else the selection epilogue needs per lane (its two queries, their stripe slots, pool slices) is
    // re-derived from the thread id at the start of each epilogue -- through an opaque copy, so that the compiler cannot
    // hoist those values out of the chunk loop and keep ~25 VGPRs of them alive across the K loop, where they pushed the
    // loop's own LDS addresses into scratch (a scratch reload inside the loop costs a vmcnt(0), i.e. a drained DMA).
    int etid = tid, elane = lane;

    // Threshold refresh from the stripe maxima, SHARED by the slabs of a query tile: the workgroup of slab s bounds the
    // queries q = s + S o of the tile (every query has one owner; recomputing all 256 in each of the S workgroups made
    // them read the same 256 KB of slots at the same moment, 12-30 us per refresh), publishes the bound with an atomic
    // max into gthr[q] -- the same word the pool compactions and cand_select use: any lower bound of the global k-th
    // best S~ may go there -- and everybody picks the thresholds up from gthr (consume_bounds).  Slot o of the tile is
    // handled by wave o % 16, 16 lanes per query, 16 stripe slots per lane (slot e * 16 + sub: one load = 64 contiguous
    // bytes per query); the k-th largest of a query's <= 256 maxima is bracketed by 12 bisection steps whose counts are
    // reduced inside the 16-lane DPP row.  The warm-up round is the exception:
    // `all`: bound every query of the tile here and now (the warm-up round: nobody can wait for everybody twice).
    auto refresh_thresholds = [&](const bool all) __attribute__((always_inline)) {
        const int sub = elane & 15;
        const int q_first = all ? 0 : slab, q_step = all ? 1 : a.S;
        unsigned svall[TQ / NWAVES / 4][16];
#pragma unroll
        for (int b4 = 0; b4 < TQ / NWAVES / 4; ++b4) {
            const int q = q_first + q_step * (w + NWAVES * (4 * b4 + (elane >> 4)));
            const unsigned* pb = a.smax + (size_t)(qt * TQ + (q < TQ ? q : 0)) * ms + sub;
#pragma unroll
            for (int e = 0; e < 16; ++e)
                svall[b4][e] = (q < TQ && e * 16 + sub < ms) ? __hip_atomic_load(pb + e * 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        }
#pragma unroll
        for (int b4 = 0; b4 < TQ / NWAVES / 4; ++b4) {
            if (q_first + q_step * (w + NWAVES * 4 * b4) >= TQ) break;  // wave-uniform: no owned query in this or later batches
            const int q = q_first + q_step * (w + NWAVES * (4 * b4 + (elane >> 4)));
            const unsigned (&sv)[16] = svall[b4];
            unsigned mn = 0xFFFFFFFFu, mx = 0u;
            int nz = 0;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                nz += sv[e] != 0u;
                mn = (sv[e] != 0u && sv[e] < mn) ? sv[e] : mn;
                mx = sv[e] > mx ? sv[e] : mx;
            }
            nz = row16_sum(nz);
            mn = row16_umin(mn);
            mx = row16_umax(mx);
            unsigned lo = mn, hi = mx == 0xFFFFFFFFu ? mx : mx + 1u;  // count(>= lo) = nz; count(>= hi) = 0
            for (int it = 0; it < 12; ++it) {  // 2^-12 of the maxima's spread: ~1e-3 sigma
                const unsigned mid = lo + ((hi - lo) >> 1);
                int cnt = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e) cnt += sv[e] >= mid;
                cnt = row16_sum(cnt);
                if (cnt >= k) lo = mid; else hi = mid;
            }
            // >= k stripes, i.e. >= k distinct rows, score >= lo (zeros = unpublished slots never count: lo > 0)
            if (sub == 0 && q < TQ && nz >= k && marg[q] >= 0.f) {
                if (all) {
                    const float nt = key_score((u64)lo << 32) - marg[q];
                    if (nt > thr[q]) thr[q] = nt;
                } else {
                    atomicMax(a.gthr + qt * TQ + q, lo);
                }
            }
        }
    };
    // thr[q] = (best published lower bound of the global k-th best S~) - margin; waves 0-3, one query per lane.
    // `wait`: give the other slabs' owners a few microseconds to publish their first bound (after the warm-up pass).
    auto consume_bounds = [&](const bool wait) __attribute__((always_inline)) {
        if (etid >= TQ) return;
        const bool real = marg[etid] >= 0.f;
        unsigned gb = 0u;
        for (int attempt = 0; attempt < (wait ? 16 : 1); ++attempt) {
            gb = __hip_atomic_load(a.gthr + qt * TQ + etid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_ballot_w64(real && gb == 0u) == 0ull) break;
            __builtin_amdgcn_s_sleep(16);
        }
        if (real && gb != 0u) {
            const float nt = key_score((u64)gb << 32) - marg[etid];
            if (nt > thr[etid]) thr[etid] = nt;
        }
    };

    // The slab's first chunk is scored TWICE.  The first pass only feeds the stripe maxima; every workgroup then
    // derives thresholds from everybody's maxima before anything is appended, so no pool ever receives the flood of
    // a threshold-less first chunk (256 keys per query and slab, which cand_select would have to wade through).
    int ci = c0, kbi = 0, replay = 1;
    auto issue_next = [&](int stg) __attribute__((always_inline)) {
        if (ci < c1) {
            issue(ci, kbi, stg);
            if (++kbi == nkb) {
                kbi = 0;
                if (replay) replay = 0; else ++ci;
            }
        }
    };
    // K loop.  LDS holds two stages of (X tile, Q tile) = 2 x 64 KiB.  Global step s reads stage s % 2; ONE barrier per step,
    // placed before the step's last two MFMAs (default) instead of at its top (the round-1 loop; tools/ablate/):
    //
    //   step s:   MFMA m=0 (operands prefetched) | reads+MFMA m=1,2 | reads m=3, MFMA acc00/acc01 (m=3)
    //             lgkmcnt(0): this wave's reads of stage s%2 have returned      vmcnt(0): its pieces of DMA(s+1) have landed
    //             s_barrier  => every wave is done reading stage s%2 AND the whole of stage (s+1)%2 is in LDS
    //             MFMA acc10/acc11 (m=3) | prefetch the m=0 operands of step s+1 | issue DMA(s+2) into stage s%2
    //
    // Waves reach the barrier with two MFMAs still to issue and leave it with six MFMAs' worth of operands in registers,
    // so the matrix pipe neither drains at the barrier nor waits for the first LDS reads of the next step, and the ~550
    // issue cycles of the four LDS-DMA pieces hide behind those MFMAs instead of standing between the barrier and the first
    // read.  At a chunk boundary DMA(s+2) is already in flight while the selection epilogue runs.
    issue_next(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    issue_next(1);
    int stage = 0;
#ifdef MQ_CLOCK
    // diagnostic build (tools/scan_clock.py, tools/scan_compactions.py; three words per workgroup, 4096 workgroups): the clock the chip holds while this kernel runs = shader-clock ticks per 100 MHz
    // wall-clock tick, one stamp pair around the whole chunk loop; the stamps go to a.dbg, which nothing else reads
    const unsigned long long ck_s0_ = __builtin_amdgcn_s_memtime(), ck_r0_ = __builtin_amdgcn_s_memrealtime();
    unsigned long long ck_rounds_ = 0;  // compaction rounds of this workgroup (tools/scan_compactions.py)
#endif
#ifdef MQ_TIMING
    unsigned long long tacc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast_ = __builtin_amdgcn_s_memtime();
#define MQ_TS(i) MQ_T(i)
#define MQ_TS_DUMP if (lane == 0) { for (int i_ = 0; i_ < 8; ++i_) a.dbg[((size_t)blockIdx.x * NWAVES + w) * 8 + i_] = tacc_[i_]; }
#else
#define MQ_TS(i)
#define MQ_TS_DUMP
#endif

    for (int pass = (c0 < c1 ? -1 : 0); pass < c1 - c0; ++pass) {
        const bool warm = pass < 0;
        const int c = c0 + (warm ? 0 : pass);
        f32x16 acc00 = {0}, acc01 = {0}, acc10 = {0}, acc11 = {0};  // SCAN_MFMA_32
        // SCAN_MFMA_16: c<a><b> = rows 16 a .. of the wave's 64 x queries 16 b ..; sixteen named values (an array indexed by
        // loop variables invites the compiler to keep it in scratch)
        f32x4_t c00 = {0}, c10 = {0}, c20 = {0}, c30 = {0}, c01 = {0}, c11 = {0}, c21 = {0}, c31 = {0};
        f32x4_t c02 = {0}, c12 = {0}, c22 = {0}, c32 = {0}, c03 = {0}, c13 = {0}, c23 = {0}, c33 = {0};
#define MQ_LDF(p) (*reinterpret_cast<const bf16x8_t*>(p))
        if constexpr (SHAPE == SCAN_MFMA_32) {
            // m = 0 operands of the chunk's first step (its stage landed before the barrier of the previous step)
            const int off0 = ((0 + kg) ^ sw) * 16;
            bf16x8_t pxa0 = MQ_LDF(xrd + stage * S_OP_BYTES + off0), pxa1 = MQ_LDF(xrd + stage * S_OP_BYTES + 32 * 128 + off0);
            bf16x8_t pqb0 = MQ_LDF(qrd + stage * S_OP_BYTES + off0), pqb1 = MQ_LDF(qrd + stage * S_OP_BYTES + 32 * 128 + off0);
            for (int kb = 0; kb < nkb; ++kb) {
                const char* xs = xrd + stage * S_OP_BYTES;
                const char* qs = qrd + stage * S_OP_BYTES;
                if (kb == 0) {
                    // the chunk's first MFMAs take the constant 0 as their C operand: no 64 v_mov per wave and chunk to clear the
                    // accumulators while the matrix pipe sits idle between two chunks
                    const f32x16 zero16 = {0};
                    acc00 = MQ_SMFMA(pxa0, pqb0, zero16, 0, 0, 0);
                    acc01 = MQ_SMFMA(pxa0, pqb1, zero16, 0, 0, 0);
                    acc10 = MQ_SMFMA(pxa1, pqb0, zero16, 0, 0, 0);
                    acc11 = MQ_SMFMA(pxa1, pqb1, zero16, 0, 0, 0);
                } else {
                    acc00 = MQ_SMFMA(pxa0, pqb0, acc00, 0, 0, 0);
                    acc01 = MQ_SMFMA(pxa0, pqb1, acc01, 0, 0, 0);
                    acc10 = MQ_SMFMA(pxa1, pqb0, acc10, 0, 0, 0);
                    acc11 = MQ_SMFMA(pxa1, pqb1, acc11, 0, 0, 0);
                }
#pragma unroll
                for (int m = 1; m < SBK / 16 - 1; ++m) {
                    const int off = ((2 * m + kg) ^ sw) * 16;
                    const bf16x8_t xa0 = MQ_LDF(xs + off), xa1 = MQ_LDF(xs + 32 * 128 + off);
                    const bf16x8_t qb0 = MQ_LDF(qs + off), qb1 = MQ_LDF(qs + 32 * 128 + off);
                    acc00 = MQ_SMFMA(xa0, qb0, acc00, 0, 0, 0);
                    acc01 = MQ_SMFMA(xa0, qb1, acc01, 0, 0, 0);
                    acc10 = MQ_SMFMA(xa1, qb0, acc10, 0, 0, 0);
                    acc11 = MQ_SMFMA(xa1, qb1, acc11, 0, 0, 0);
                }
                {
                    const int off = ((2 * (SBK / 16 - 1) + kg) ^ sw) * 16;
                    const bf16x8_t xa0 = MQ_LDF(xs + off), xa1 = MQ_LDF(xs + 32 * 128 + off);
                    const bf16x8_t qb0 = MQ_LDF(qs + off), qb1 = MQ_LDF(qs + 32 * 128 + off);
                    acc00 = MQ_SMFMA(xa0, qb0, acc00, 0, 0, 0);
                    acc01 = MQ_SMFMA(xa0, qb1, acc01, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    // every LDS read of this wave from the current stage has returned; its DMA pieces of the next stage have landed
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    acc10 = MQ_SMFMA(xa1, qb0, acc10, 0, 0, 0);
                    acc11 = MQ_SMFMA(xa1, qb1, acc11, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const int freed = stage;
                stage ^= 1;
                if (kb + 1 < nkb) {  // the next step's first operands, from the stage that has just been declared complete
                    pxa0 = MQ_LDF(xrd + stage * S_OP_BYTES + off0); pxa1 = MQ_LDF(xrd + stage * S_OP_BYTES + 32 * 128 + off0);
                    pqb0 = MQ_LDF(qrd + stage * S_OP_BYTES + off0); pqb1 = MQ_LDF(qrd + stage * S_OP_BYTES + 32 * 128 + off0);
                }
                __builtin_amdgcn_sched_barrier(0);
                issue_next(freed);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            // 16x16x32: a K step is two 32-deep half-steps h; in half-step h the lane reads chunk (4 h + kg) ^ sw of rows
            // 16 a + i (X: the A fragment of row block a) and 16 b + i (Q: the B fragment of column b).  A half-step is walked
            // column by column: its four A fragments stay live, the B fragments alternate between qe and qo, read one column
            // ahead.  Registers: 64 accumulators + 16 (A) + 8 (B) + 8 that let the NEXT half-step's fragments arrive in time --
            // 96, what the 32x32x16 loop holds behind its barrier.  Half-step 0 keeps its A fragments in x0 .. x3 and reads
            // e0, e1 = A0, A1 of half-step 1 meanwhile; its last column issues rows 0, 1 first and reads A2, A3 of half-step 1
            // into the x0, x1 they leave.  Half-step 1 runs on (e0, e1, x0, x1); behind the barrier -- as above, before the
            // step's last four MFMAs -- x2, x3 and the first B fragment of the next step are read, then x0, x1 once the
            // last column's rows 2, 3 have issued, and the next step's first column takes rows 2, 3 first.
#define MQ_M16 __builtin_amdgcn_mfma_f32_16x16x32_bf16
#define MQ_ACC(x) x
#define MQ_ZERO(x) zero4
#define MQ_FR(base, r, off) MQ_LDF((base) + (r) * 16 * 128 + (off))
#define MQ_MM(a_, b_, A, B, C) c##a_##b_ = MQ_M16(A, B, C(c##a_##b_), 0, 0, 0);
#define MQ_PIN __builtin_amdgcn_sched_barrier(0);  // the order below IS the register plan: nothing moves across a column
#define MQ_HALF0(C)                                                                               \
    qo = MQ_FR(qs, 1, off0); e0 = MQ_FR(xs, 0, off1); e1 = MQ_FR(xs, 1, off1);                    \
    MQ_MM(2, 0, x2, qe, C) MQ_MM(3, 0, x3, qe, C) MQ_MM(0, 0, x0, qe, C) MQ_MM(1, 0, x1, qe, C)   \
    MQ_PIN qe = MQ_FR(qs, 2, off0);                                                               \
    MQ_MM(0, 1, x0, qo, C) MQ_MM(1, 1, x1, qo, C) MQ_MM(2, 1, x2, qo, C) MQ_MM(3, 1, x3, qo, C)   \
    MQ_PIN qo = MQ_FR(qs, 3, off0);                                                               \
    MQ_MM(0, 2, x0, qe, C) MQ_MM(1, 2, x1, qe, C) MQ_MM(2, 2, x2, qe, C) MQ_MM(3, 2, x3, qe, C)   \
    MQ_PIN qe = MQ_FR(qs, 0, off1);                                                               \
    MQ_MM(0, 3, x0, qo, C) MQ_MM(1, 3, x1, qo, C)                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    x0 = MQ_FR(xs, 2, off1); x1 = MQ_FR(xs, 3, off1);                                             \
    MQ_MM(2, 3, x2, qo, C) MQ_MM(3, 3, x3, qo, C)                                                 \
    __builtin_amdgcn_sched_barrier(0);
            const int offk = (kg ^ sw) * 16;  // chunk (0 + kg) ^ sw; half-step 1 reads chunk (4 + kg) ^ sw, 64 bytes to the side
            const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
            bf16x8_t x0, x1, x2, x3, e0, e1, qe, qo;
            {
                const int off0 = offk;
                const char* xs = xrd + stage * S_OP_BYTES;
                x2 = MQ_FR(xs, 2, off0); x3 = MQ_FR(xs, 3, off0); qe = MQ_FR(qrd + stage * S_OP_BYTES, 0, off0);
                x0 = MQ_FR(xs, 0, off0); x1 = MQ_FR(xs, 1, off0);
            }
            for (int kb = 0; kb < nkb; ++kb) {
                const char* xs = xrd + stage * S_OP_BYTES;
                const char* qs = qrd + stage * S_OP_BYTES;
                // (an opaque copy per step: hoisted out of the loop, the second offset and the sums it enters are registers
                // the loop does not have)
                int off0 = offk;
                asm volatile("" : "+v"(off0));
                const int off1 = off0 ^ 64;
                if (kb == 0) {  // C = the constant 0, as above
                    MQ_HALF0(MQ_ZERO)
                } else {
                    MQ_HALF0(MQ_ACC)
                }
                qo = MQ_FR(qs, 1, off1);
                MQ_MM(0, 0, e0, qe, MQ_ACC) MQ_MM(1, 0, e1, qe, MQ_ACC) MQ_MM(2, 0, x0, qe, MQ_ACC) MQ_MM(3, 0, x1, qe, MQ_ACC)
                MQ_PIN qe = MQ_FR(qs, 2, off1);
                MQ_MM(0, 1, e0, qo, MQ_ACC) MQ_MM(1, 1, e1, qo, MQ_ACC) MQ_MM(2, 1, x0, qo, MQ_ACC) MQ_MM(3, 1, x1, qo, MQ_ACC)
                MQ_PIN qo = MQ_FR(qs, 3, off1);
                MQ_MM(0, 2, e0, qe, MQ_ACC) MQ_MM(1, 2, e1, qe, MQ_ACC) MQ_MM(2, 2, x0, qe, MQ_ACC) MQ_MM(3, 2, x1, qe, MQ_ACC)
                __builtin_amdgcn_sched_barrier(0);
                // every LDS read of this wave from the current stage has returned; its DMA pieces of the next stage have landed
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                const int freed = stage;
                stage ^= 1;
                // the next step's first fragments, from the stage that has just been declared complete (after the chunk's last
                // step these are the next chunk's, read again at its top: five reads per chunk for a loop without a branch;
                // after the slab's LAST chunk no DMA has filled that stage -- the reads are inside LDS and their values dead)
                x2 = MQ_FR(xrd + stage * S_OP_BYTES, 2, off0); x3 = MQ_FR(xrd + stage * S_OP_BYTES, 3, off0);
                qe = MQ_FR(qrd + stage * S_OP_BYTES, 0, off0);
                MQ_MM(2, 3, x0, qo, MQ_ACC) MQ_MM(3, 3, x1, qo, MQ_ACC)
                __builtin_amdgcn_sched_barrier(0);
                x0 = MQ_FR(xrd + stage * S_OP_BYTES, 0, off0); x1 = MQ_FR(xrd + stage * S_OP_BYTES, 1, off0);
                MQ_MM(0, 3, e0, qo, MQ_ACC) MQ_MM(1, 3, e1, qo, MQ_ACC)
                __builtin_amdgcn_sched_barrier(0);
                issue_next(freed);
                __builtin_amdgcn_sched_barrier(0);
            }
#undef MQ_HALF0
#undef MQ_PIN
#undef MQ_MM
#undef MQ_FR
#undef MQ_ZERO
#undef MQ_ACC
#undef MQ_M16
        }
#undef MQ_LDF

        // relaxed selection: C/D map col j = lane&31 -> query q0 (b=0) / q1 (b=1);
        // row i' = (reg&3) + 8*(reg>>2) + 4*kg -> KB row 64*wr + 32*a + i'
        {
            unsigned t_ = threadIdx.x;
            asm volatile("" : "+v"(t_));
            etid = (int)t_;
            elane = etid & 63;
        }
        const int ekg = SHAPE == SCAN_MFMA_16 ? elane >> 4 : elane >> 5;
        const unsigned rowbase = (unsigned)c * TN + wr * 64 + 4 * ekg;
        const unsigned nrows = (unsigned)a.N;
        const int rc0 = warm ? 0 : pass;  // chunk ordinal inside the slab
        const bool ragged = ((long long)c + 1) * TN > a.N;
        MQ_TS(0)
#ifdef MQ_TIMING
        if constexpr (SHAPE == SCAN_MFMA_32) asm volatile("" ::"v"(acc00[0]), "v"(acc01[0]), "v"(acc10[0]), "v"(acc11[15]));  // bucket 1 = wait for the last MFMAs
        else asm volatile("" ::"v"(c00[0]), "v"(c13[0]), "v"(c23[0]), "v"(c33[3]));
#endif
        MQ_TS(1)
        if constexpr (SHAPE == SCAN_MFMA_32) {
            const int q0 = wc * 64 + (elane & 31), q1 = q0 + 32;  // this lane's two queries (tile-local)
            // this lane's stripes: (wr * 2 + ekg) * 2 (sub-tile 0) and the next one (sub-tile 1)
            unsigned* const sm0 = a.smax + (size_t)(qt * TQ + q0) * ms + slab * sps;
            unsigned* const sm1 = a.smax + (size_t)(qt * TQ + q1) * ms + slab * sps;
            const int so0 = ekg ? so_b0 : so_a0, so1 = ekg ? so_b1 : so_a1;
            // this lane's private slices of its two queries' pools: no atomics, the slot counters live in
            // registers during the scan
            const int sl = wr * 2 + ekg;
            const float t0 = thr[q0], t1 = thr[q1];
            int n0 = scnt[q0 * NSL + sl], n1 = scnt[q1 * NSL + sl];
            u64* P0 = mypools + (size_t)q0 * SPOOL + sl * SLCAP;
            u64* P1 = mypools + (size_t)q1 * SPOOL + sl * SLCAP;
            // One 32x32 sub-tile (16 scores per lane) at a time: v_max3 tree -> stripe maximum (published when it grows)
            // -> the sub-tile is skipped when no lane of the wave reaches its threshold, else its register triples are
            // tested the same way before the per-score appends.  Hits are rare (~1e-3 of the scores), so most of the
            // 16 compare-and-branch sites of a sub-tile never execute.
            // `rag` (compile-time): the chunk reaches past the last row (the last chunk of the shard only) -- its own copy of
            // the code, so that the ordinary path carries none of the row-bound tests
            // `wm` (compile-time): the warm-up pass, which only feeds the stripe maxima.
            auto subtile = [&](auto rag, auto wm, auto pb, const f32x16& v, const float t, u64* __restrict__ P, int& n, float& rmax,
                               unsigned* slot, const unsigned rb) __attribute__((always_inline)) {
                constexpr bool ragged = decltype(rag)::value, warm = decltype(wm)::value, publish = decltype(pb)::value;
                const float m0 = fmaxf(fmaxf(v[0], v[1]), v[2]), m1 = fmaxf(fmaxf(v[3], v[4]), v[5]);
                const float m2 = fmaxf(fmaxf(v[6], v[7]), v[8]), m3 = fmaxf(fmaxf(v[9], v[10]), v[11]);
                const float m4 = fmaxf(fmaxf(v[12], v[13]), v[14]);
                const float gm = fmaxf(fmaxf(fmaxf(m0, m1), m2), fmaxf(fmaxf(m3, m4), v[15]));
                if (!ragged) {
                    if (gm > rmax) {
                        rmax = gm;
                        if (publish) __hip_atomic_fetch_max(slot, (unsigned)(make_key(gm, 0u) >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (__builtin_amdgcn_ballot_w64(gm >= t) == 0ull) return;
                }
                if (warm) return;
                auto site = [&](const int reg) __attribute__((always_inline)) {
                    const unsigned r = rb + (reg & 3) + 8 * (reg >> 2);
                    if ((!ragged || r < nrows) && v[reg] >= t) P[n++] = make_key(v[reg], r);
                };
                if (ragged || __builtin_amdgcn_ballot_w64(m0 >= t) != 0ull) { site(0); site(1); site(2); }
                if (ragged || __builtin_amdgcn_ballot_w64(m1 >= t) != 0ull) { site(3); site(4); site(5); }
                if (ragged || __builtin_amdgcn_ballot_w64(m2 >= t) != 0ull) { site(6); site(7); site(8); }
                if (ragged || __builtin_amdgcn_ballot_w64(m3 >= t) != 0ull) { site(9); site(10); site(11); }
                if (ragged || __builtin_amdgcn_ballot_w64(m4 >= t) != 0ull) { site(12); site(13); site(14); }
                site(15);
            };
#define MQ_SUBTILES(RAG, WM, PB)                                                          \
    subtile(RAG{}, WM{}, PB{}, acc00, t0, P0, n0, rm00, sm0 + so0, rowbase);              \
    subtile(RAG{}, WM{}, PB{}, acc10, t0, P0, n0, rm10, sm0 + so1, rowbase + 32);         \
    subtile(RAG{}, WM{}, PB{}, acc01, t1, P1, n1, rm01, sm1 + so0, rowbase);              \
    subtile(RAG{}, WM{}, PB{}, acc11, t1, P1, n1, rm11, sm1 + so1, rowbase + 32);
            using T_ = std::true_type;
            using F_ = std::false_type;
            if (ragged) {  // the stripe maxima are not fed from a ragged chunk
                if (warm) { MQ_SUBTILES(T_, T_, F_) } else { MQ_SUBTILES(T_, F_, F_) }
            } else if (warm) {
                if (publish) { MQ_SUBTILES(F_, T_, T_) } else { MQ_SUBTILES(F_, T_, F_) }
            } else if (publish) {
                MQ_SUBTILES(F_, F_, T_)
            } else {
                MQ_SUBTILES(F_, F_, F_)
            }
#undef MQ_SUBTILES
            MQ_TS(3)
            scnt[q0 * NSL + sl] = n0;
            scnt[q1 * NSL + sl] = n1;
            if (n0 > SLCAP - 64 || n1 > SLCAP - 64) wgflag[rc0 % 3] = 1;
            if (etid == 0) wgflag[(rc0 + 1) % 3] = 0;
        } else {
            // 16x16 C/D map: col = lane & 15 -> query wc * 64 + 16 b + (lane & 15) of column b; row = 4 kg + reg -> KB row
            // 64 wr + 16 a + 4 kg + reg.  A lane owns four queries and 16 rows of the chunk for each: the column's four
            // accumulators c0b .. c3b are the 16 scores the 32 x 32 sub-tile rule above walks -- the same v_max3 tree, the
            // same ballot-gated triples.  One column at a time, so that what a column needs (threshold, counter, pool and
            // slot addresses) is live for that column only.
            // Slice wr * 2 + (kg >> 1) of a query has TWO writer lanes here, lane and lane ^ 16 (kg even / odd): both hold the
            // slice's counter n.  Per group of sites that passed its ballot the lanes swap their hit counts (one ds_swizzle);
            // the even lane appends at n, the odd one behind the even one's hits, both advance n by the sum -- so both write
            // the same value back to scnt.  A slice still takes at most 2 x 16 keys per chunk and query.
            float &rmc0 = rm00, &rmc1 = rm10, &rmc2 = rm01, &rmc3 = rm11;  // running maxima of this lane's query columns 0 .. 3
            const int qc = wc * 64 + (elane & 15);
            const int sl = wr * 2 + (ekg >> 1);
            const bool odd = (ekg & 1) != 0;
            const int so = ekg == 0 ? so_a0 : ekg == 1 ? so_a1 : ekg == 2 ? so_b0 : so_b1;
            bool full = false;
            auto column = [&](auto rag, auto wm, auto pb, const int b, const f32x4_t& v0, const f32x4_t& v1, const f32x4_t& v2,
                              const f32x4_t& v3, float& rmax) __attribute__((always_inline)) {
                constexpr bool ragged = decltype(rag)::value, warm = decltype(wm)::value, publish = decltype(pb)::value;
                const int q = qc + 16 * b;
                const float t = thr[q];
                const float m0 = fmaxf(fmaxf(v0[0], v0[1]), v0[2]), m1 = fmaxf(fmaxf(v0[3], v1[0]), v1[1]);
                const float m2 = fmaxf(fmaxf(v1[2], v1[3]), v2[0]), m3 = fmaxf(fmaxf(v2[1], v2[2]), v2[3]);
                const float m4 = fmaxf(fmaxf(v3[0], v3[1]), v3[2]);
                const float gm = fmaxf(fmaxf(fmaxf(m0, m1), m2), fmaxf(fmaxf(m3, m4), v3[3]));
                if (!ragged) {
                    if (gm > rmax) {
                        rmax = gm;
                        if (publish)
                            __hip_atomic_fetch_max(a.smax + (size_t)(qt * TQ + q) * ms + slab * sps + so, (unsigned)(make_key(gm, 0u) >> 32),
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (__builtin_amdgcn_ballot_w64(gm >= t) == 0ull) return;
                }
                if (warm) return;
                int n = scnt[q * NSL + sl];
                u64* __restrict__ P = mypools + (size_t)q * SPOOL + sl * SLCAP;
                // sites (x, a, reg): score x of row rowbase + 16 a + reg; every lane of the wave gets here together
                auto sites = [&](const float x0, const unsigned r0, const bool two, const float x1, const unsigned r1, const float x2,
                                 const unsigned r2) __attribute__((always_inline)) {
                    const bool h0 = (!ragged || rowbase + r0 < nrows) && x0 >= t;
                    const bool h1 = two && (!ragged || rowbase + r1 < nrows) && x1 >= t;
                    const bool h2 = two && (!ragged || rowbase + r2 < nrows) && x2 >= t;
                    const int mine = (int)h0 + (int)h1 + (int)h2;
                    const int theirs = __builtin_amdgcn_ds_swizzle(mine, 0x401F);  // lane ^ 16
                    int at = n + (odd ? theirs : 0);
                    if (h0) P[at++] = make_key(x0, rowbase + r0);
                    if (h1) P[at++] = make_key(x1, rowbase + r1);
                    if (h2) P[at++] = make_key(x2, rowbase + r2);
                    n += mine + theirs;
                };
                if (ragged || __builtin_amdgcn_ballot_w64(m0 >= t) != 0ull) sites(v0[0], 0, true, v0[1], 1, v0[2], 2);
                if (ragged || __builtin_amdgcn_ballot_w64(m1 >= t) != 0ull) sites(v0[3], 3, true, v1[0], 16, v1[1], 17);
                if (ragged || __builtin_amdgcn_ballot_w64(m2 >= t) != 0ull) sites(v1[2], 18, true, v1[3], 19, v2[0], 32);
                if (ragged || __builtin_amdgcn_ballot_w64(m3 >= t) != 0ull) sites(v2[1], 33, true, v2[2], 34, v2[3], 35);
                if (ragged || __builtin_amdgcn_ballot_w64(m4 >= t) != 0ull) sites(v3[0], 48, true, v3[1], 49, v3[2], 50);
                if (ragged || __builtin_amdgcn_ballot_w64(v3[3] >= t) != 0ull) sites(v3[3], 51, false, 0.f, 0u, 0.f, 0u);
                scnt[q * NSL + sl] = n;
                full |= n > SLCAP - 64;
            };
#define MQ_COLUMNS(RAG, WM, PB)                                      \
    column(RAG{}, WM{}, PB{}, 0, c00, c10, c20, c30, rmc0);          \
    column(RAG{}, WM{}, PB{}, 1, c01, c11, c21, c31, rmc1);          \
    column(RAG{}, WM{}, PB{}, 2, c02, c12, c22, c32, rmc2);          \
    column(RAG{}, WM{}, PB{}, 3, c03, c13, c23, c33, rmc3);
            using T_ = std::true_type;
            using F_ = std::false_type;
            if (ragged) {
                if (warm) { MQ_COLUMNS(T_, T_, F_) } else { MQ_COLUMNS(T_, F_, F_) }
            } else if (warm) {
                if (publish) { MQ_COLUMNS(F_, T_, T_) } else { MQ_COLUMNS(F_, T_, F_) }
            } else if (publish) {
                MQ_COLUMNS(F_, F_, T_)
            } else {
                MQ_COLUMNS(F_, F_, F_)
            }
#undef MQ_COLUMNS
            MQ_TS(3)
            if (full) wgflag[rc0 % 3] = 1;
            if (etid == 0) wgflag[(rc0 + 1) % 3] = 0;
        }
        MQ_TS(5)
        if (warm) {
            // Every slab publishes its warm-up maxima at about the same moment; give the stragglers a few microseconds
            // (bounded: a slab that is not resident yet simply leaves this one with looser thresholds).
            if (ms >= k) {
                const unsigned* pb = a.smax + (size_t)(qt * TQ + w) * ms;  // poll one query's slots: 4 per lane
                for (int attempt = 0; attempt < 12; ++attempt) {
                    int nzp = 0;
#pragma unroll
                    for (int e = 0; e < SMAX_SLOTS / 64; ++e) {
                        const unsigned sv = (e * 64 + elane < ms) ? __hip_atomic_load(pb + e * 64 + elane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                        nzp += __builtin_popcountll(__builtin_amdgcn_ballot_w64(sv != 0u));
                    }
                    if (nzp >= ms - ms / 8) break;  // (nearly) every slab is in
                    __builtin_amdgcn_s_sleep(32);
                }
                // shared from the start; owners that publish late are caught by the pick-ups of the first three chunks
                refresh_thresholds(false);
                consume_bounds(true);
            }
            MQ_TS(7)
            continue;
        }
        if (ms >= k) {
            // own share after 4, 8, 16 ... chunks (the warm-up covers 1 and 2); thresholds are picked up right away
            // (earlier rounds, fast owners), once more a chunk later (this round's stragglers), and in each of the first
            // three chunks (stragglers of the warm-up round)
#ifndef MQ_ROUND_BITS
#define MQ_ROUND_BITS 0
#endif
            // a round when rc0 + 1 has at most 1 + MQ_ROUND_BITS significant bits (MQ_ROUND_BITS = 0: powers of two)
            auto is_round = [](const int r) {
                const unsigned x = (unsigned)(r + 1);
                const int drop = 31 - __builtin_clz(x) - MQ_ROUND_BITS;  // bits below the leading 1 + MQ_ROUND_BITS
                return r > 1 && (drop <= 0 || (x & ((1u << drop) - 1u)) == 0u);
            };
            const bool round = is_round(rc0);
            if (round) refresh_thresholds(false);
            if (round || (rc0 > 2 && is_round(rc0 - 1)) || rc0 < 3) consume_bounds(false);
        }
        MQ_TS(2)
        MQ_TS(4)
        // Compaction is decided one chunk late, which takes every barrier out of the ordinary epilogue: a lane raised
        // flag[(c - 1) % 3] during the PREVIOUS chunk's appends when one of its slices passed half its capacity
        // (<= 96 of 128 slots then, <= 128 now); the K-loop barriers in between make the flag uniform.  This chunk
        // raises flag[c % 3]; flag[(c + 1) % 3] is cleared for the next one.
        if (wgflag[(rc0 + 2) % 3]) {
#ifdef MQ_CLOCK
            ++ck_rounds_;
#endif
            __syncthreads();  // vmcnt(0) of every wave + barrier: all appended keys are in L2
            for (int j = 0; j < TQ / NWAVES; ++j) {
                const int q = w + NWAVES * j;
                int* sc = scnt + q * NSL;
                // every pool of the tile is compacted in the same round: pools of one tile fill at about the same
                // rate, and a round costs the slowest wave -- 16 balanced compactions per wave beat a trickle of
                // single ones that each stall the other 15 waves
                if (compact_pool_relaxed<NSL>(mypools + (size_t)q * SPOOL, sc, k, marg[q], &thr[q], a.gthr + qt * TQ + q, elane) < 0 &&
                    elane == 0)
                    a.ovf[qt] = 1;
            }
            __syncthreads();
            if (etid == 0) wgflag[rc0 % 3] = 0;  // slices are at most half full again
        }
        MQ_TS(6)
    }
    MQ_TS_DUMP
#ifdef MQ_CLOCK
    if (a.dbg && tid == 0 && blockIdx.x < 4096) {
        a.dbg[3 * blockIdx.x] = __builtin_amdgcn_s_memtime() - ck_s0_;
        a.dbg[3 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - ck_r0_;
        a.dbg[3 * blockIdx.x + 2] = ck_rounds_;
    }
#endif
    // The pools stay in their sliced layout (no end-of-slab compaction): cand_select reads slice z of a pool at
    // [z * SLCAP, z * SLCAP + count z).
    __syncthreads();
    if (tid < TQ) {
        int4* dst = reinterpret_cast<int4*>(a.pcount + (((size_t)qt * a.S + slab) * TQ + tid) * NSL);
        const int4* src = reinterpret_cast<const int4*>(scnt + tid * NSL);
        dst[0] = src[0];
        dst[1] = src[1];
    }
}
__global__ __launch_bounds__(1024) void screen_scan_kernel(const ScreenArgs a) { screen_scan_body<SCAN_MFMA_32>(a); }
__global__ __launch_bounds__(1024) void screen_scan16_kernel(const ScreenArgs a) { screen_scan_body<SCAN_MFMA_16>(a); }

// ------------------------------------------------------------------------------------------------
// candidate selection, exact re-scoring, final selection
// ------------------------------------------------------------------------------------------------

// ONE wave, R words per lane (0 = absent): the largest T with |{w >= T}| >= k (0 if there is none) -- the k-th largest word
template <int R>
__device__ __forceinline__ unsigned wave_kth_word(const unsigned (&w)[R], int k) {
    unsigned T = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const unsigned cand = T | (1u << bit);
        int c = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(w[r] >= cand));
        if (c >= k) T = cand;
    }
    return T;
}

// block-wide (256 threads) count of set predicates; `slot` rotates over 3 LDS counters so that one
// __syncthreads() per call suffices
__device__ __forceinline__ int block_count(const bool (&p)[CSEL_PER], int* ctr, int& slot, int lane) {
    int c = 0;
#pragma unroll
    for (int r = 0; r < CSEL_PER; ++r) c += __builtin_popcountll(__builtin_amdgcn_ballot_w64(p[r]));
    const int nxt = slot == 2 ? 0 : slot + 1;
    if (threadIdx.x == 0) ctr[nxt] = 0;
    if (lane == 0 && c) atomicAdd(&ctr[slot], c);
    __syncthreads();
    const int total = ctr[slot];
    slot = nxt;
    return total;
}

#ifdef MQ_TIMING
// tools/cand_select_timing.py: 100 MHz wall-clock stamps of thread 0, eight per query of ONE query tile, behind the scan kernels'
// own slots (32768 words: 256 workgroups x 16 waves x 8); the tools' buffers hold CS_DBG_AT + 256 * 8 words
__device__ unsigned long long* g_cs_dbg;
#define CS_DBG_AT 32768
#define CS_TS(i) if (threadIdx.x == 0 && g_cs_dbg && gridDim.x <= 256) g_cs_dbg[CS_DBG_AT + blockIdx.x * 8 + (i)] = wall_clock64();
#else
#define CS_TS(i)
#endif
template <int WALK>  // how the pools are read (CSEL_WALK_*; one instance each: the line walks cost 35 registers = a resident block at 4096 queries)
__global__ __launch_bounds__(256) void cand_select_kernel(const u64* __restrict__ pools, const int* __restrict__ pcount,
                                                          const float* __restrict__ margin, const unsigned* __restrict__ gthr,
                                                          const unsigned* __restrict__ smax, int ms,
                                                          int* __restrict__ ovf, int nq, int S, int k,
                                                          unsigned* __restrict__ cand_rows, int* __restrict__ ccount,
                                                          const int* __restrict__ layout_word) {
    constexpr int CAP = 256 * CSEL_PER;
    __shared__ u64 buf[CAP];
    __shared__ int ctr[3];
    __shared__ int nbuf, nout, state, nwork;
    __shared__ unsigned bcast[2];
    __shared__ unsigned work[CSEL_WORK];
    const int q = blockIdx.x, qt = q / TQ, ql = q % TQ, t = threadIdx.x, lane = t & 63;
    constexpr int LAYOUT = WALK == CSEL_WALK_HALVES ? POOL_LAYOUT_HALVES : POOL_LAYOUT_SLICES;  // what the host expects
    CS_TS(0)
    if (t == 0) {
        ctr[0] = ctr[1] = ctr[2] = 0; nbuf = 0; nout = 0;
        // which scan filled the pools: the word behind a lone tile's overflow flag, zeroed with it, set by screen_small8_kernel.
        // Not what the host launched this instance for (an option changed between the two phases of a split call): the tile
        // goes to the exact scan.
        const int filled = layout_word ? *layout_word : POOL_LAYOUT_SLICES;
        if (filled != LAYOUT) ovf[qt] = 1;
        // an infinite margin (screen_margin_kernel: a factor of the bound overflowed) bounds nothing, and the bf16 scores of such
        // data may be inf / NaN themselves (the centred screen's row term c . (x - c) at x ~ 2^100) and never reach a pool:
        // the tile goes to the exact scan whatever the pools hold
        if (!(margin[q] < INFINITY)) ovf[qt] = 1;
        state = (filled != LAYOUT || ovf[qt]) ? -1 : 0;
    }
    __syncthreads();
    if (state < 0) {  // one reader: the decision must be block-uniform
        if (t == 0) ccount[q] = 0;
        return;
    }
    // Pools of this query: S slabs x up to SPOOL keys (L2-resident).  First bound: the best threshold any slab
    // published (gthr = max over slabs of a lower bound of the slab's k-th best S~ <= global k-th best S~).
    unsigned gb = gthr[q];
    const float mg = margin[q];
    // second bound: the k-th largest of the query's final stripe maxima (disjoint row sets, see screen_scan_kernel):
    // at least k rows score that much, so it is <= the global k-th best S~.  ms <= 256 words: wave 0 bisects them from
    // registers with ballots alone (32 block-wide rounds of counter + barrier took 7 of the kernel's 42 us per query).
    {
        if (t < 64) {
            unsigned w4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // (clamped address, then the test: four loads in flight, not four round trips)
                const unsigned wv = smax[(size_t)q * ms + (t + 64 * r < ms ? t + 64 * r : ms - 1)];
                w4[r] = (t + 64 * r < ms) ? wv : 0u;
            }
            const unsigned Tw = wave_kth_word<4>(w4, k);
            if (t == 0) bcast[0] = Tw;
        }
        __syncthreads();
        const unsigned Tq = bcast[0];
        if (Tq > gb) gb = Tq;  // Tq = 0 when fewer than k stripes exist (S * 16 < k): gthr alone then
    }
    u64 K0 = gb ? make_key(key_score((u64)gb << 32) - mg, 0xFFFFFFFFu) : 1ull;
    int slot = 0;
    CS_TS(1)
    // Pool walk.  Few slabs (long pools): thread t looks at slice t / 32 of every slab, entries t % 32, + 32, ... (one
    // count load and one key load per thread and slab).  Many slabs (S >= 64: short pools of a few keys each), or pool halves:
    // line by line, below.
    const int zsl = t >> 5, esub = t & 31;
    auto for_each_key = [&](auto&& fn) __attribute__((always_inline)) {
        if (WALK != CSEL_WALK_SLICES) {
            // Pools read line by line.  A "unit" is a run of pool slots one writer fills front to back, its count known:
            //   CSEL_WALK_HALVES  screen_small8_kernel's pools -- two writers per (query, slab), each filling its half of the pool,
            //     so a half's usual 1 - 8 keys are ONE 64-byte line (dealt over four slices they were four lines: the walk fetched
            //     2150 lines per query for 310 survivors and ran at the memory system's line rate, 25 of the kernel's 42 us);
            //   CSEL_WALK_SLICE_LINES  the slices layout with many slabs (S >= 64: a one-tile search the tile kernel serves, wide
            //     columns) -- a unit is a slice; its keys beyond the first used to follow one dependent load at a time.
            // Thread t takes units t and t + 256 of every 512: the count (a half: its four slice counts in one load), then the
            // first line; what a unit holds beyond eight keys is listed line by line and fetched by all threads afterwards.
            constexpr int UPP = WALK == CSEL_WALK_HALVES ? 2 : NSL, USL = SPOOL / UPP;
            if (t == 0) nwork = 0;
            __syncthreads();
            for (int u0 = t; u0 < S * UPP; u0 += 512) {
                int n2[2];
                u64 k16[2][8];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int ui = u0 + 256 * u, sl = ui / UPP, uu = ui % UPP;
                    // (an address inside the array whatever sl: a load under a test is a branch and a round trip of its own)
                    const int* pc = pcount + (((size_t)qt * S + (sl < S ? sl : S - 1)) * TQ + ql) * NSL;
                    if (WALK == CSEL_WALK_HALVES) {
                        const int4 c = *reinterpret_cast<const int4*>(pc + 4 * uu);
                        n2[u] = c.x + c.y + c.z + c.w;
                    } else {
                        n2[u] = pc[uu];
                    }
                    if (sl >= S) n2[u] = 0;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int ui = u0 + 256 * u, sl = ui / UPP, uu = ui % UPP;
                    // the first line of the unit whatever its count (nearly every unit holds a key; slots beyond the count are
                    // ignored below): eight loads in flight behind the two counts, no test in between
                    const ulonglong2* P2 = reinterpret_cast<const ulonglong2*>(
                        pools + (((size_t)qt * S + (sl < S ? sl : S - 1)) * TQ + ql) * SPOOL + uu * USL);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const ulonglong2 x = P2[e];
                        k16[u][2 * e] = x.x;
                        k16[u][2 * e + 1] = x.y;
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (n2[u] > 8) {
                        const int ui = u0 + 256 * u, sl = ui / UPP, uu = ui % UPP;
                        const int lines = (n2[u] - 1) >> 3;  // lines 1 .. lines of the unit
                        const int w0 = atomicAdd(&nwork, lines) - 1;
                        const unsigned base = ((unsigned)sl << 19) | ((unsigned)uu << 16) | (unsigned)n2[u];
                        const u64* P = pools + (((size_t)qt * S + sl) * TQ + ql) * SPOOL + uu * USL;
                        for (int l = 1; l <= lines; ++l) {
                            if (w0 + l < CSEL_WORK) work[w0 + l] = base | ((unsigned)l << 10);
                            else
                                for (int e = 8 * l; e < 8 * l + 8 && e < n2[u]; ++e) fn(P[e]);  // list full: the slow way
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e < n2[u]) fn(k16[u][e]);
                }
            }
            __syncthreads();
            const int nw = nwork < CSEL_WORK ? nwork : CSEL_WORK;
            for (int i = t; i < nw; i += 256) {
                const unsigned e = work[i];
                const int n = (int)(e & 1023u), l = (int)((e >> 10) & 63u);
                const ulonglong2* P2 = reinterpret_cast<const ulonglong2*>(
                    pools + (((size_t)qt * S + (e >> 19)) * TQ + ql) * SPOOL + ((e >> 16) & 7u) * USL + 8 * l);
                ulonglong2 x[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[j] = ulonglong2{0ull, 0ull};
                    if (8 * l + 2 * j < n) x[j] = P2[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (8 * l + 2 * j < n) fn(x[j].x);
                    if (8 * l + 2 * j + 1 < n) fn(x[j].y);
                }
            }
        } else {
            // four slabs at a time: their four slice counts, then their <= 4 x 4 keys per thread (a slice has SLCAP = 128
            // slots = 4 per thread), are requested together instead of one dependent count -> key round trip per slab
            static_assert(SLCAP == 4 * 32, "four key slots per thread and slice");
            for (int s0 = 0; s0 < S; s0 += 4) {
                int n4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const size_t pi = ((size_t)qt * S + (s0 + u < S ? s0 + u : s0)) * TQ + ql;
                    n4[u] = s0 + u < S ? pcount[pi * NSL + zsl] : 0;
                }
                u64 x16[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const size_t pi = ((size_t)qt * S + (s0 + u < S ? s0 + u : s0)) * TQ + ql;
                    const u64* P = pools + pi * SPOOL + zsl * SLCAP;
#pragma unroll
                    for (int r = 0; r < 4; ++r) x16[u][r] = (esub + 32 * r < n4[u]) ? P[esub + 32 * r] : 0ull;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (esub + 32 * r < n4[u]) fn(x16[u][r]);
                }
            }
        }
    };
    // survivors of `key` into LDS; returns how many there are (may exceed CAP: then only the count is meaningful)
    auto collect = [&](u64 key) {
        if (t == 0) nbuf = 0;
        __syncthreads();
        for_each_key([&](u64 x) {
            if (x >= key) {
                const int sl_ = atomicAdd(&nbuf, 1);
                if (sl_ < CAP) buf[sl_] = x;
            }
        });
        __syncthreads();
        return nbuf;
    };
    // block-wide count of pool keys >= key (streams every pool), and the largest score word seen
    auto stream_count = [&](u64 key, unsigned* mxw) {
        int c = 0;
        unsigned mx = 0u;
        for_each_key([&](u64 x) {
            c += x >= key;
            const unsigned h = (unsigned)(x >> 32);
            mx = h > mx ? h : mx;
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            c += __shfl_xor(c, o);
            const unsigned m2 = (unsigned)__shfl_xor((int)mx, o);
            mx = m2 > mx ? m2 : mx;
        }
        const int nxt = slot == 2 ? 0 : slot + 1;
        if (t == 0) ctr[nxt] = 0;
        if (lane == 0) { if (c) atomicAdd(&ctr[slot], c); if (mxw) atomicMax(reinterpret_cast<unsigned*>(&state), mx); }
        __syncthreads();
        const int total_ = ctr[slot];
        slot = nxt;
        if (mxw) *mxw = (unsigned)state;
        return total_;
    };
    int total = collect(K0);
    CS_TS(2)
    if (total > CAP) {
        // many small slabs, or no stripe bound: bisect the score word (streaming counts) for a lower bound of the
        // global k-th best S~, apply the margin, collect again.
        unsigned mxw = 0u;
        stream_count(K0, &mxw);
        unsigned lo = (unsigned)(K0 >> 32), hi = mxw + 1u;  // count(>= lo) > CAP > k; count(>= hi) = 0
        for (int it = 0; it < 18 && hi - lo > 1u; ++it) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            if (stream_count((u64)mid << 32, nullptr) >= k) lo = mid; else hi = mid;
        }
        K0 = make_key(key_score((u64)lo << 32) - mg, 0xFFFFFFFFu);
        total = collect(K0);
    }
    if (total > CAP) {
        if (t == 0) { ccount[q] = 0; ovf[qt] = 1; }
        return;
    }
    CS_TS(3)
    u64 v[CSEL_PER];
#pragma unroll
    for (int r = 0; r < CSEL_PER; ++r) v[r] = (t + 256 * r < total) ? buf[t + 256 * r] : 0ull;
    u64 Kthr = 1ull;  // total <= k: every entry is a candidate
    if (total > k) {
        // k-th largest score word of the block: most-significant-digit-first radix selection, four rounds of a 256-bin
        // histogram (LDS atomics) and a suffix sum over the bins.  (32 rounds of bisection cost 9 - 10 us per query whether
        // block-wide over a counter and a barrier per bit or by one wave with ballots alone: a third of the kernel.)
        unsigned Th = 0u;
        {
            int* hist = reinterpret_cast<int*>(work);  // 256 bins + 4 wave totals: the pool walk's list is done with
            static_assert(CSEL_WORK >= 260, "the histogram lives in the walk's list");
            int kk = k;  // the kk-th largest of the keys whose higher digits equal Th's is looked for
            const int wv = t >> 6;
#pragma unroll 1
            for (int shift = 24; shift >= 0; shift -= 8) {
                hist[t] = 0;
                __syncthreads();
#pragma unroll
                for (int r = 0; r < CSEL_PER; ++r) {
                    const unsigned wd = (unsigned)(v[r] >> 32);
                    const unsigned hi = shift == 24 ? 0u : wd >> ((shift + 8) & 31);
                    if (t + 256 * r < total && hi == Th) atomicAdd(&hist[(wd >> shift) & 255u], 1);
                }
                __syncthreads();
                const int h = hist[t];
                int sfx = h;  // matching keys whose digit is >= t
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int up = __shfl_down(sfx, o);
                    if (lane + o < 64) sfx += up;
                }
                if (lane == 0) hist[256 + wv] = sfx;
                __syncthreads();
                for (int ww = wv + 1; ww < 4; ++ww) sfx += hist[256 + ww];
                if (sfx >= kk && sfx - h < kk) {  // one thread: its bin holds the kk-th largest
                    bcast[0] = (unsigned)t;
                    bcast[1] = (unsigned)(kk - (sfx - h));
                }
                __syncthreads();
                Th = (Th << 8) | bcast[0];
                kk = (int)bcast[1];
            }
        }
        // every key whose score is >= (k-th best score) - margin; ties in the k-th score are all inside
        const float thr = key_score((u64)Th << 32) - mg;
        Kthr = make_key(thr, 0xFFFFFFFFu);
    }
    CS_TS(4)
    bool keep[CSEL_PER];
#pragma unroll
    for (int r = 0; r < CSEL_PER; ++r) keep[r] = v[r] != 0ull && v[r] >= Kthr;
    const int cc = block_count(keep, ctr, slot, lane);
    if (cc > RMAX) {
        if (t == 0) { ccount[q] = 0; ovf[qt] = 1; }
        return;
    }
#pragma unroll
    for (int r = 0; r < CSEL_PER; ++r)
        if (keep[r]) cand_rows[(size_t)q * RMAX + atomicAdd(&nout, 1)] = key_row(v[r]);
    if (t == 0) ccount[q] = cc;
    CS_TS(5)
#ifdef MQ_TIMING
    if (t == 0 && g_cs_dbg && gridDim.x <= 256) g_cs_dbg[CS_DBG_AT + blockIdx.x * 8 + 6] = (unsigned long long)total;
#endif
}

// Exact score of 64 candidate rows of one query.  256 threads: all four waves stage [64 rows][RC k] tiles of the
// fp32 row-major KB copy into LDS with 16-byte loads (4 rows x 256 B per wave instruction, rows fully coalesced);
// wave 0 then walks the k-ordered fp32 fma chain of one candidate per lane -- bit-identical to what
// v_mfma_f32_32x32x2_f32 accumulates in the exact scan.
__global__ __launch_bounds__(256) void rescore_kernel(const float* __restrict__ Xrm, const float* __restrict__ Q, int d,
                                                      const unsigned* __restrict__ cand_rows, const int* __restrict__ ccount,
                                                      u64* __restrict__ ckeys, const float* __restrict__ qn,
                                                      const float* __restrict__ xn, unsigned flip) {
    // One block = 64 candidates of one query.  All four waves stage RC columns of the 64 rows through LDS (16-byte
    // pieces, two stages); wave 0 runs the 64 sequential chains, one lane per candidate.  RC = 32 measured best
    // (0.80 ms at 4096 x 252 candidates; 64 columns 1.08, 128 columns 1.59; one private tile per wave 1.57+): the
    // kernel runs at the rate the memory system gathers 3-KB rows at (5.5 TB/s at 4096 queries, 3.7 TB/s at 256), so more
    // resident blocks beat longer pieces.  A deeper ring does not help either (whole step, same box: 2 stages 9.35 ms; 3 stages
    // 9.61-9.65; 16 columns x 3 / 4 stages 9.73 / 9.79), nor do 64 columns at ONE query tile, where four blocks per CU are
    // resident whatever their size (54.3 us against 54.0; with the requests ahead of the chain: tail 100 against 92 us), nor do
    // 32-candidate blocks there (eight in flight per CU: tail 106 against 92 us at d = 768, 74 against 78 at d = 512).
    // Twelve of a query's sixteen blocks usually find nothing to do and leave: four blocks per query walking their groups
    // instead change nothing at 4096 queries (526 us) and cost a one-tile search its tail (a query with 5 groups makes one
    // block do two: 92 -> 110 us).
    // The pieces of the next stage are requested before wave 0 walks the current one and written to LDS after it.
    constexpr int RC = RESCORE_COLS;
    constexpr int NB = 2, U = 64 * RC / 4 / 256;
    static_assert(64 * RC / 4 % 256 == 0 && RC <= 256, "whole 16-byte pieces per thread; one query value per thread");
    __shared__ float tile[NB][64][RC + 4];
    __shared__ float qs[NB][RC];
    __shared__ unsigned rows[64];
    const int q = blockIdx.x, g0 = blockIdx.y * 64, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int cc = ccount[q];
    if (g0 >= cc) return;
    if (t < 64) rows[t] = cand_rows[(size_t)q * RMAX + (g0 + t < cc ? g0 + t : g0)];
    __syncthreads();
    const bool vec_ok = (d & 3) == 0;
    float4 pv[U];
    float pq = 0.f;
    // `vec` (compile-time): d is a multiple of 4, every piece is one aligned 16-byte load.  Kept apart from the element-wise
    // variant: merged, the compiler turns BOTH into four predicated 4-byte loads per piece (4x the gather instructions)
    auto request_as = [&](auto vec, int kc) __attribute__((always_inline)) {
        constexpr bool VEC = decltype(vec)::value;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int f = t + 256 * u, rr = f / (RC / 4), k4 = (f % (RC / 4)) * 4;
            const float* src = Xrm + (size_t)rows[rr] * d + kc + k4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (VEC) {
                if (kc + k4 < d) v = *reinterpret_cast<const float4*>(src);
            } else {
                if (kc + k4 + 0 < d) v.x = src[0];
                if (kc + k4 + 1 < d) v.y = src[1];
                if (kc + k4 + 2 < d) v.z = src[2];
                if (kc + k4 + 3 < d) v.w = src[3];
            }
            pv[u] = v;
        }
        if (t < RC) pq = (kc + t < d) ? Q[(size_t)q * d + kc + t] : 0.f;
    };
    auto request = [&](int kc) __attribute__((always_inline)) {
        if (vec_ok) request_as(std::true_type{}, kc); else request_as(std::false_type{}, kc);
    };
    auto deposit = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int f = t + 256 * u, rr = f / (RC / 4), k4 = (f % (RC / 4)) * 4;
            *reinterpret_cast<float4*>(&tile[buf][rr][k4]) = pv[u];
        }
        if (t < RC) qs[buf][t] = pq;
    };
    float acc = 0.f;
    request(0);
    deposit(0);
    int buf = 0;
    for (int kc = 0; kc < d; kc += RC) {
        __syncthreads();  // stage `buf` is whole; wave 0 is done with the other one
        const bool more = kc + RC < d;
        if (more) request(kc + RC);
        if (w == 0) {
#pragma unroll 16
            for (int kk = 0; kk < RC; ++kk) acc = fmaf(tile[buf][lane][kk], qs[buf][kk], acc);
        }
        if (more) deposit(buf ^ 1);
        buf ^= 1;
    }
    if (w == 0 && qn) {  // L2: the exact scan's own expression, g = -max(0, (qn + xn) - 2 S)
        const float dd = (qn[q] + xn[rows[lane]]) - 2.0f * acc;
        acc = -(dd < 0.f ? 0.f : dd);
    }
    // strict FAISS rule: a score must beat the heap neutral value -FLT_MAX to enter (NaN, -inf never do)
    if (w == 0) ckeys[(size_t)q * RMAX + g0 + lane] = (g0 + lane < cc && acc > -FLT_MAX) ? make_key(acc, rows[lane] ^ flip) : 0ull;
}

// exact top-k (score desc, then the tie order `flip` encodes) of a query's re-scored candidates -> D, I; one wave per query
// KS = 128 (k <= 128) or 256: the number of keys the final sort handles
template <int KS>
__global__ __launch_bounds__(64) void final_select_kernel(const u64* __restrict__ ckeys, const int* __restrict__ ccount,
                                                          const int* __restrict__ ovf, int k, long long id_offset,
                                                          float* __restrict__ D, long long* __restrict__ I, int l2, unsigned flip) {
    constexpr int R = RMAX / 64;
    __shared__ u64 packed[KS];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (ovf[q / TQ]) return;  // recomputed by the exact scan
    const int cc = ccount[q];
    u64 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = (r * 64 + lane < cc) ? ckeys[(size_t)q * RMAX + r * 64 + lane] : 0ull;
    int nz = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) nz += __builtin_popcountll(__builtin_amdgcn_ballot_w64(v[r] != 0ull));
    // (the bisection costs a fixed ~35 cycles per ballot of a lone wave: only the registers that can hold keys take part)
    u64 T = 1ull;
    if (nz > k) {
        if (cc <= 256) T = wave_kth_largest_n<4>(reinterpret_cast<const u64(&)[4]>(v), k);
        else if (cc <= 512) T = wave_kth_largest_n<8>(reinterpret_cast<const u64(&)[8]>(v), k);
        else T = wave_kth_largest_n<R>(v, k);
    }
#pragma unroll
    for (int r = 0; r < KS / 64; ++r) packed[lane + 64 * r] = 0ull;
    __syncthreads();
    int base = 0;
    const u64 lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool keep = v[r] != 0ull && v[r] >= T;
        const u64 m = __builtin_amdgcn_ballot_w64(keep);
        if (keep) packed[base + __builtin_popcountll(m & lt)] = v[r];
        base += __builtin_popcountll(m);
    }
    __syncthreads();
    u64 s2[KS / 64];
#pragma unroll
    for (int r = 0; r < KS / 64; ++r) s2[r] = packed[lane + 64 * r];
    if (KS == 128) sort128_desc(reinterpret_cast<u64(&)[2]>(s2), lane); else sort_desc_n<KS / 64>(s2, lane);
#pragma unroll
    for (int r = 0; r < KS / 64; ++r) {
        const int idx = r * 64 + lane;
        if (idx < k) {
            const u64 key = s2[r];
            const float sc = key ? key_score(key) : -FLT_MAX;
            D[(size_t)q * k + idx] = (l2 ? -sc : sc) + 0.0f;  // L2: keys carry -distance; unfilled slots report FAISS's neutral value (+-FLT_MAX)
            I[(size_t)q * k + idx] = key ? (long long)(key_row(key) ^ flip) + id_offset : -1;
        }
    }
}
