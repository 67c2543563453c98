// bm25.hip -- exhaustive BM25 passage search on gfx950 (Lucene 8 BM25Similarity arithmetic over a CSR inverted index; what the
// reference delegates to Elasticsearch, meerqat/ir/search.py:81-205).  C ABI: include/meerqat_hip.h.
//
//   bm25_impact_kernel   elementwise over the postings: impact[p] = float(tf / (tf + cache[code[doc[p]]])), the division in
//                        double; cache is the 256-entry table k1 * ((1 - b) + b * len / avgdl) of the one-byte length codes
//   bm25_score_kernel    one workgroup per (document block of MQ_BM25_BLOCK_ROWS rows, query): the block's fp32 accumulators live
//                        in LDS (64 KiB, two workgroups per CU); clauses are taken in clause order, each one's postings inside the
//                        block found by two binary searches on the sorted document ids, then acc[doc] = acc[doc] + weight * impact
//                        as a plain LDS read-modify-write (a term lists a document once: no two lanes meet), a barrier between
//                        clauses.  The sum of a document is the sequential fp32 sum in clause order: no float atomic anywhere, bit
//                        for bit reproducible.  The block is then stored coalesced into the dense [queries, N] score matrix.
//   topk_* kernels       exact top-k of every row of a dense non-negative fp32 matrix (mq_topk_rows_f32): radix select on the 64-bit
//                        key (score bits << 32) | (id_asc ? ~id : id) -- non-negative floats order like their bit patterns, all
//                        keys are distinct, so exactly k keys lie at or above the k-th.  Up to six histogram passes of 11 / 11 /
//                        10 / 11 / 11 / 10 bits (integer atomics only; a pass whose bucket holds exactly the rows still wanted ends
//                        the selection, so distinct scores take three), a gather of the winners, a bitonic sort in LDS.  Rows of
//                        score 0 matched no clause and never enter; unfilled slots are (-inf, -1).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "../../include/meerqat_hip.h"
#include "host_check.h"

namespace {

constexpr int R = MQ_BM25_BLOCK_ROWS;  // documents per scoring workgroup: 16,384 fp32 accumulators = 64 KiB of LDS
constexpr int ST = 512;                // threads of a scoring workgroup
constexpr int CB = ST / 2;             // clauses whose posting ranges are searched at once (two bounds each)

constexpr int TT = 1024;               // threads of a selection workgroup
constexpr int NB = 2048;               // histogram bins (11 bits)
constexpr int PASSES = 6;
constexpr int ROWS_PER_WG = TT * 16;   // least share of a row worth a workgroup of its own
constexpr int MAX_SPLIT = 64;

__host__ __device__ __forceinline__ int pass_shift(int p) { return p == 0 ? 53 : p == 1 ? 42 : p == 2 ? 32 : p == 3 ? 21 : p == 4 ? 10 : 0; }
__host__ __device__ __forceinline__ int pass_bits(int p) { return (p == 2 || p == 5) ? 10 : 11; }

__global__ __launch_bounds__(256) void bm25_impact_kernel(const int32_t* __restrict__ doc, const int32_t* __restrict__ tf,
                                                          const uint8_t* __restrict__ code, const float* __restrict__ cache,
                                                          float* __restrict__ impact, int64_t nnz) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += stride) {
        const double f = (double)tf[p];
        impact[p] = (float)(f / (f + (double)cache[code[doc[p]]]));
    }
}

// first position in [lo, hi) whose document id is >= target
__device__ __forceinline__ int64_t lower_bound(const int32_t* __restrict__ doc, int64_t lo, int64_t hi, int64_t target) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)doc[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(ST) void bm25_score_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ doc,
                                                        const float* __restrict__ impact, int64_t N, int64_t n_terms,
                                                        const int32_t* __restrict__ qptr, const int32_t* __restrict__ cterm,
                                                        const float* __restrict__ cweight, float* __restrict__ scores) {
    __shared__ float acc[R];
    __shared__ int64_t bound[2 * CB];
    const int tid = threadIdx.x;
    const int q = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * R;
    for (int i = tid; i < R; i += ST) acc[i] = 0.f;
    const int cbeg = qptr[q], cend = qptr[q + 1];
    for (int c0 = cbeg; c0 < cend; c0 += CB) {
        const int nc = min(CB, cend - c0);
        __syncthreads();  // the accumulators are zeroed / the previous batch's bounds are no longer read
        if (tid < 2 * nc) {
            const int t = cterm[c0 + (tid >> 1)];
            // (a term id outside the vocabulary gets an empty range: nothing is read through it)
            bound[tid] = (t < 0 || t >= n_terms) ? 0 : lower_bound(doc, ptr[t], ptr[t + 1], base + (int64_t)(tid & 1) * R);
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const int64_t lo = bound[2 * c], hi = bound[2 * c + 1];
            if (lo == hi) continue;  // uniform over the workgroup
            const float w = cweight[c0 + c];
            for (int64_t p = lo + tid; p < hi; p += ST) {
                const int d = (int)((int64_t)doc[p] - base);
                if ((unsigned)d < (unsigned)R) acc[d] = __fadd_rn(acc[d], __fmul_rn(w, impact[p]));  // (always, for sorted postings)
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int rows = (int)min((int64_t)R, N - base);
    float* out = scores + (int64_t)q * N + base;
    for (int i = tid; i < rows; i += ST) out[i] = acc[i];
}

// Parameter grid: GT settings of (k1, b) scored in ONE sweep of the postings.  What a setting changes is the 256-entry norm cache
// alone, so a workgroup keeps GT accumulators per document (RG = R / GT documents: the same 64 KiB) and the tile's caches in LDS,
// both with the setting as the fast index -- a lane's posting then reads and writes GT consecutive floats (128-bit LDS accesses).
// Per posting and setting the arithmetic is bm25_impact_kernel's followed by bm25_score_kernel's, in that order: the double
// division, its rounding to float, the float product with the clause weight, the float sum in clause order.  `gt` <= GT settings
// are live (a last, partial tile); the others compute on a zero cache and are not stored.  scores: [gt, n, N], n = gridDim.y.
template <int GT>
struct GridShape {
    static constexpr int RG = R / GT;
    static constexpr bool STAGE_CODES = GT >= 2;  // the block's length codes in LDS (at GT = 1 they would cost a workgroup per CU)
    static constexpr int CODE_BYTES = STAGE_CODES ? RG : 16;
};

template <int GT>
__device__ __forceinline__ void load_row(float (&v)[GT], const float* __restrict__ p) {
    if constexpr (GT % 4 == 0) {
#pragma unroll
        for (int j = 0; j < GT / 4; ++j) {
            const float4 x = reinterpret_cast<const float4*>(p)[j];
            v[4 * j] = x.x; v[4 * j + 1] = x.y; v[4 * j + 2] = x.z; v[4 * j + 3] = x.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < GT; ++j) v[j] = p[j];
    }
}

template <int GT>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&v)[GT]) {
    if constexpr (GT % 4 == 0) {
#pragma unroll
        for (int j = 0; j < GT / 4; ++j) reinterpret_cast<float4*>(p)[j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < GT; ++j) p[j] = v[j];
    }
}

template <int GT>
__global__ __launch_bounds__(ST) void bm25_score_grid_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ doc,
                                                             const int32_t* __restrict__ tf, const uint8_t* __restrict__ code,
                                                             const float* __restrict__ caches, int gt, int64_t N, int64_t n_terms,
                                                             const int32_t* __restrict__ qptr, const int32_t* __restrict__ cterm,
                                                             const float* __restrict__ cweight, float* __restrict__ scores) {
    constexpr int RG = GridShape<GT>::RG;
    __shared__ __attribute__((aligned(16))) float acc[RG * GT];     // [document][setting]
    __shared__ __attribute__((aligned(16))) float norm[256 * GT];   // [length code][setting]
    __shared__ uint8_t lcode[GridShape<GT>::CODE_BYTES];
    __shared__ int64_t bound[2 * CB];
    const int tid = threadIdx.x;
    const int q = blockIdx.y;
    const int64_t base = (int64_t)blockIdx.x * RG;
    const int rows = (int)min((int64_t)RG, N - base);
    for (int i = tid; i < RG * GT; i += ST) acc[i] = 0.f;
    for (int i = tid; i < 256 * GT; i += ST) {
        const int c = i / GT, g = i % GT;
        norm[i] = g < gt ? caches[g * 256 + c] : 0.f;
    }
    if constexpr (GridShape<GT>::STAGE_CODES)
        for (int i = tid; i < RG; i += ST) lcode[i] = i < rows ? code[base + i] : (uint8_t)0;
    const int cbeg = qptr[q], cend = qptr[q + 1];
    for (int c0 = cbeg; c0 < cend; c0 += CB) {
        const int nc = min(CB, cend - c0);
        __syncthreads();  // LDS is initialised / the previous batch's bounds are no longer read
        if (tid < 2 * nc) {
            const int t = cterm[c0 + (tid >> 1)];
            bound[tid] = (t < 0 || t >= n_terms) ? 0 : lower_bound(doc, ptr[t], ptr[t + 1], base + (int64_t)(tid & 1) * RG);
        }
        __syncthreads();
        for (int c = 0; c < nc; ++c) {
            const int64_t lo = bound[2 * c], hi = bound[2 * c + 1];
            if (lo == hi) continue;  // uniform over the workgroup
            const float w = cweight[c0 + c];
            for (int64_t p = lo + tid; p < hi; p += ST) {
                const int d = (int)((int64_t)doc[p] - base);
                if ((unsigned)d >= (unsigned)rows) continue;  // (never, for sorted postings of documents below N)
                const double f = (double)tf[p];
                int lc;
                if constexpr (GridShape<GT>::STAGE_CODES) lc = lcode[d]; else lc = code[base + d];
                float a[GT], nv[GT];
                load_row<GT>(a, acc + d * GT);
                load_row<GT>(nv, norm + lc * GT);
#pragma unroll
                for (int g = 0; g < GT; ++g) {
                    const float impact = (float)(f / (f + (double)nv[g]));
                    a[g] = __fadd_rn(a[g], __fmul_rn(w, impact));
                }
                store_row<GT>(acc + d * GT, a);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int64_t n = gridDim.y;
    for (int i = tid; i < rows; i += ST) {
        float a[GT];
        load_row<GT>(a, acc + i * GT);
#pragma unroll
        for (int g = 0; g < GT; ++g)
            if (g < gt) scores[((int64_t)g * n + q) * N + base + i] = a[g];
    }
}

// ---------------------------------------------------------------------------------------------------------------- top-k
struct Select {
    uint64_t prefix;  // the decided high bits of the k-th key, the undecided ones zero
    uint32_t want;    // rows still to take from the bucket `prefix` names
    int decided;      // passes whose digit is decided
    bool done;        // the bucket holds exactly `want` rows (or the row has no more than k hits): take key >= prefix
};

__device__ __forceinline__ uint64_t make_key(float s, int64_t id, int id_desc) {
    const uint32_t low = id_desc ? (uint32_t)id : ~(uint32_t)id;
    return ((uint64_t)__float_as_uint(s) << 32) | low;
}

// Replays the histograms of the passes already run (hist [PASSES][NB] of this row) and returns what they decide.  Every thread of
// the workgroup calls it and gets the same answer; sfx / slot are LDS scratch of NB + 1 and 2 words.
__device__ Select replay(const uint32_t* __restrict__ hist, int passes_run, int k, uint32_t* sfx, uint32_t* slot) {
    Select s;
    s.prefix = 0; s.want = (uint32_t)k; s.decided = 0; s.done = false;
    const int tid = threadIdx.x;
    for (int p = 0; p < passes_run && !s.done; ++p) {
        const uint32_t* h = hist + p * NB;
        __syncthreads();
        // suffix sums over the bins, sfx[d] = rows of this pass in bins >= d: every thread owns the bin pair (2 tid, 2 tid + 1), the
        // pair sums sit in the even entries and are scanned there (Hillis-Steele), the odd entries follow from them
        const uint32_t h0 = h[2 * tid], h1 = h[2 * tid + 1];
        sfx[2 * tid] = h0 + h1;
        if (tid == 0) { sfx[NB] = 0; slot[0] = 0; slot[1] = 0; }
        __syncthreads();
        for (int o = 1; o < TT; o <<= 1) {
            const uint32_t add = (tid + o < TT) ? sfx[2 * (tid + o)] : 0u;
            __syncthreads();
            sfx[2 * tid] += add;
            __syncthreads();
        }
        sfx[2 * tid + 1] = sfx[2 * tid] - h0;
        __syncthreads();
        if (p == 0 && sfx[0] <= s.want) {  // no more hits than k: every hit is taken
            s.done = true;
            s.want = sfx[0];
            break;
        }
        for (int d = tid; d < NB; d += TT)
            if (sfx[d] >= s.want && sfx[d + 1] < s.want) { slot[0] = (uint32_t)d; slot[1] = sfx[d + 1]; }
        __syncthreads();
        const uint32_t d = slot[0], above = slot[1];
        s.prefix |= (uint64_t)d << pass_shift(p);
        s.want -= above;
        s.decided = p + 1;
        if (h[d] == s.want) s.done = true;
    }
    __syncthreads();
    return s;
}

struct TopkArgs {
    const float* scores;  // [rows, N]
    int64_t N;
    int k, id_desc, split;
    uint32_t* hist;       // [rows][PASSES][NB]
    uint32_t* count;      // [rows]
    uint64_t* cand;       // [rows][kpad]
    int kpad;
    float* D;
    int64_t* I;
    int64_t id_offset;
};

__global__ __launch_bounds__(TT) void topk_hist_kernel(TopkArgs a, int pass) {
    __shared__ uint32_t sfx[NB + 1];
    __shared__ uint32_t slot[2];
    __shared__ uint32_t bins[NB];
    const int row = blockIdx.y, tid = threadIdx.x;
    uint32_t* hist = a.hist + (size_t)row * PASSES * NB;
    const Select s = replay(hist, pass, a.k, sfx, slot);
    if (s.done) return;
    for (int d = tid; d < NB; d += TT) bins[d] = 0;
    __syncthreads();
    const int shift = pass_shift(pass), bits = pass_bits(pass);
    const int top = shift + bits;  // key bits [top, 64) are decided
    const uint64_t hi_prefix = top < 64 ? (s.prefix >> top) : 0;
    const float* x = a.scores + (int64_t)row * a.N;
    const int64_t per = (a.N + a.split - 1) / a.split;
    const int64_t beg = (int64_t)blockIdx.x * per, end = min(a.N, beg + per);
    for (int64_t i = beg + tid; i < end; i += TT) {
        const float v = x[i];
        if (__float_as_uint(v) == 0u) continue;  // matched no clause: not a hit
        const uint64_t key = make_key(v, i, a.id_desc);
        if (top < 64 && (key >> top) != hi_prefix) continue;
        atomicAdd(&bins[(uint32_t)(key >> shift) & ((1u << bits) - 1u)], 1u);
    }
    __syncthreads();
    for (int d = tid; d < NB; d += TT)
        if (bins[d]) atomicAdd(&hist[pass * NB + d], bins[d]);
}

__global__ __launch_bounds__(TT) void topk_gather_kernel(TopkArgs a) {
    __shared__ uint32_t sfx[NB + 1];
    __shared__ uint32_t slot[2];
    const int row = blockIdx.y, tid = threadIdx.x;
    const Select s = replay(a.hist + (size_t)row * PASSES * NB, PASSES, a.k, sfx, slot);
    const float* x = a.scores + (int64_t)row * a.N;
    const int64_t per = (a.N + a.split - 1) / a.split;
    const int64_t beg = (int64_t)blockIdx.x * per, end = min(a.N, beg + per);
    uint64_t* cand = a.cand + (size_t)row * a.kpad;
    for (int64_t i = beg + tid; i < end; i += TT) {
        const float v = x[i];
        if (__float_as_uint(v) == 0u) continue;
        const uint64_t key = make_key(v, i, a.id_desc);
        if (key < s.prefix) continue;
        const uint32_t at = atomicAdd(&a.count[row], 1u);
        if (at < (uint32_t)a.kpad) cand[at] = key;  // exactly min(k, hits) keys pass: the bound only guards the buffer
    }
}

__global__ __launch_bounds__(TT) void topk_sort_kernel(TopkArgs a) {
    __shared__ uint64_t keys[MQ_KNN_MAX_K];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int n = (int)min(a.count[row], (uint32_t)a.k);
    const uint64_t* cand = a.cand + (size_t)row * a.kpad;
    for (int i = tid; i < a.kpad; i += TT) keys[i] = i < n ? cand[i] : 0ull;  // 0 is below every hit's key (score bits > 0)
    __syncthreads();
    // bitonic sort, descending, of kpad (a power of two) keys
    for (int size = 2; size <= a.kpad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < a.kpad / 2; i += TT) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t u = keys[lo], v = keys[hi];
                if ((u < v) == desc) { keys[lo] = v; keys[hi] = u; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < a.k; i += TT) {
        const uint64_t key = keys[i];
        const uint32_t low = (uint32_t)key;
        a.D[(int64_t)row * a.k + i] = i < n ? __uint_as_float((uint32_t)(key >> 32)) : -INFINITY;
        a.I[(int64_t)row * a.k + i] = i < n ? (int64_t)(a.id_desc ? low : ~low) + a.id_offset : -1;
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline int kpad_of(int k) {
    int p = 2;
    while (p < k) p <<= 1;
    return p;
}

struct TopkLayout {
    size_t hist, count, cand, total;
};

inline TopkLayout topk_layout(int rows, int k) {
    TopkLayout l;
    l.hist = 0;
    l.count = align256((size_t)rows * PASSES * NB * sizeof(uint32_t));
    l.cand = l.count + align256((size_t)rows * sizeof(uint32_t));
    l.total = l.cand + align256((size_t)rows * kpad_of(k) * sizeof(uint64_t));
    return l;
}

// workgroups that share one row of N elements when `rows` rows are selected at once
inline int topk_split(int rows, int64_t N) {
    int64_t split = (N + ROWS_PER_WG - 1) / ROWS_PER_WG;
    const int64_t fill = (2048 + rows - 1) / rows;  // enough workgroups for every CU, not more
    if (split > fill) split = fill;
    if (split > MAX_SPLIT) split = MAX_SPLIT;
    if (split < 1) split = 1;
    return (int)split;
}

int topk_rows(const float* scores, int rows, int64_t N, int k, int flags, int64_t id_offset, float* D, int64_t* I, char* ws,
              hipStream_t st) {
    const TopkLayout l = topk_layout(rows, k);
    TopkArgs a;
    a.scores = scores; a.N = N; a.k = k; a.id_desc = (flags & MQ_KNN_FLAG_TIE_ID_DESC) ? 1 : 0;
    a.split = topk_split(rows, N);
    a.hist = reinterpret_cast<uint32_t*>(ws + l.hist);
    a.count = reinterpret_cast<uint32_t*>(ws + l.count);
    a.cand = reinterpret_cast<uint64_t*>(ws + l.cand);
    a.kpad = kpad_of(k);
    a.D = D; a.I = I; a.id_offset = id_offset;
    MQ_HIP(hipMemsetAsync(ws, 0, l.cand, st));  // histograms and counters
    const dim3 grid(a.split, rows);
    for (int p = 0; p < PASSES; ++p) hipLaunchKernelGGL(topk_hist_kernel, grid, dim3(TT), 0, st, a, p);
    hipLaunchKernelGGL(topk_gather_kernel, grid, dim3(TT), 0, st, a);
    hipLaunchKernelGGL(topk_sort_kernel, dim3(rows), dim3(TT), 0, st, a);
    return mq_launch_status();
}

constexpr int MAX_ROWS_PER_CALL = 65535;  // gridDim.y

constexpr int GRID_TILE = 8;  // settings per sweep: 2,048 documents x 8 accumulators, 78 KiB of LDS, two workgroups per CU

// the instantiated tile width that holds g settings: the next power of two
inline int grid_width(int g) {
    int w = 1;
    while (w < g) w <<= 1;
    return w;
}

struct GridArgs {
    const int64_t* ptr; const int32_t* doc; const int32_t* tf; const uint8_t* code;
    int64_t N, n_terms;
    const int32_t* qptr; const int32_t* cterm; const float* cweight;
};

template <int GT>
void launch_grid(const GridArgs& a, const float* caches, int gt, int q0, int n, float* scores, hipStream_t st) {
    const unsigned blocks = (unsigned)((a.N + GridShape<GT>::RG - 1) / GridShape<GT>::RG);
    hipLaunchKernelGGL(bm25_score_grid_kernel<GT>, dim3(blocks, n), dim3(ST), 0, st, a.ptr, a.doc, a.tf, a.code, caches, gt, a.N,
                       a.n_terms, a.qptr + q0, a.cterm, a.cweight, scores);
}

}  // namespace

extern "C" {

int mq_bm25_block_rows(void) { return R; }

int mq_bm25_clause_batch(void) { return CB; }

int mq_bm25_impacts_f32(const int32_t* doc_dev, const int32_t* tf_dev, const uint8_t* code_dev, const float* cache_dev,
                        int64_t nnz, float* impact_dev, void* stream) {
    if (nnz < 0) return MQ_EINVAL;
    if (nnz == 0) return MQ_OK;
    if (!doc_dev || !tf_dev || !code_dev || !cache_dev || !impact_dev) return MQ_EINVAL;
    const int64_t blocks = (nnz + 255) / 256;
    hipLaunchKernelGGL(bm25_impact_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, (hipStream_t)stream,
                       doc_dev, tf_dev, code_dev, cache_dev, impact_dev, nnz);
    return mq_launch_status();
}

size_t mq_topk_rows_workspace_bytes(int rows, int k) {
    if (rows < 1 || rows > MAX_ROWS_PER_CALL || k < 1 || k > MQ_KNN_MAX_K) return 0;
    return topk_layout(rows, k).total;
}

int mq_topk_rows_launch_info(int rows, int64_t N, int64_t out[8]) {
    if (!out || rows < 1 || rows > MAX_ROWS_PER_CALL || N < 1 || N > 0x7fffffffLL) return MQ_EINVAL;
    out[0] = topk_split(rows, N);
    out[1] = PASSES;
    for (int p = 0; p < PASSES; ++p) out[2 + p] = pass_shift(p);
    return MQ_OK;
}

int mq_topk_rows_f32(const float* scores_dev, int rows, int64_t N, int k, int flags, int64_t id_offset, float* D_dev,
                     int64_t* I_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    if (!scores_dev || !D_dev || !I_dev || !ws_dev || rows < 1 || rows > MAX_ROWS_PER_CALL || N < 1 || N > 0x7fffffffLL || k < 1)
        return MQ_EINVAL;
    if (flags & ~MQ_KNN_FLAG_TIE_ID_DESC) return MQ_EINVAL;
    if (k > MQ_KNN_MAX_K) return MQ_EUNSUPPORTED;
    if (ws_bytes < topk_layout(rows, k).total) return MQ_EWORKSPACE;
    return topk_rows(scores_dev, rows, N, k, flags, id_offset, D_dev, I_dev, static_cast<char*>(ws_dev), (hipStream_t)stream);
}

int mq_bm25_chunk_queries(int64_t N, int nq, size_t budget_bytes) {
    if (N < 1 || nq < 1) return 0;
    int64_t c = (int64_t)(budget_bytes / ((size_t)N * sizeof(float)));
    if (c < 1) c = 1;
    if (c > nq) c = nq;
    if (c > MAX_ROWS_PER_CALL) c = MAX_ROWS_PER_CALL;
    const int64_t grid_cap = ((int64_t)1 << 31) / ST / ((N + R - 1) / R);  // threads of one scoring launch stay below 2^31
    if (c > grid_cap) c = grid_cap < 1 ? 1 : grid_cap;
    return (int)c;
}

size_t mq_bm25_workspace_bytes(int64_t N, int nq, int k, size_t budget_bytes) {
    const int c = mq_bm25_chunk_queries(N, nq, budget_bytes);
    if (c < 1 || k < 1 || k > MQ_KNN_MAX_K) return 0;
    return align256((size_t)c * (size_t)N * sizeof(float)) + topk_layout(c, k).total;
}

int mq_bm25_search_f32(const int64_t* ptr_dev, const int32_t* doc_dev, const float* impact_dev, int64_t N, int64_t n_terms,
                       const int32_t* qptr_dev, const int32_t* cterm_dev, const float* cweight_dev, int nq, int k, int flags,
                       int64_t id_offset, float* D_dev, int64_t* I_dev, void* ws_dev, size_t ws_bytes, size_t budget_bytes,
                       void* stream) {
    // doc / impact / cterm / cweight may be NULL only when there is nothing behind them (an index without postings, a batch without
    // clauses): qptr then lists empty ranges and no kernel reads them
    if (!ptr_dev || !qptr_dev || !D_dev || !I_dev || !ws_dev || N < 1 || N > 0x7fffffffLL || n_terms < 0 || nq < 1 || k < 1)
        return MQ_EINVAL;
    if (flags & ~MQ_KNN_FLAG_TIE_ID_DESC) return MQ_EINVAL;
    if (k > MQ_KNN_MAX_K) return MQ_EUNSUPPORTED;
    const int chunk = mq_bm25_chunk_queries(N, nq, budget_bytes);
    if (ws_bytes < mq_bm25_workspace_bytes(N, nq, k, budget_bytes)) return MQ_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* scores = static_cast<float*>(ws_dev);
    char* sel = static_cast<char*>(ws_dev) + align256((size_t)chunk * (size_t)N * sizeof(float));
    const unsigned blocks = (unsigned)((N + R - 1) / R);
    for (int q0 = 0; q0 < nq; q0 += chunk) {
        const int n = nq - q0 < chunk ? nq - q0 : chunk;
        hipLaunchKernelGGL(bm25_score_kernel, dim3(blocks, n), dim3(ST), 0, st, ptr_dev, doc_dev, impact_dev, N, n_terms,
                           qptr_dev + q0, cterm_dev, cweight_dev, scores);
        MQ_HIP(hipGetLastError());
        const int rc = topk_rows(scores, n, N, k, flags, id_offset, D_dev + (int64_t)q0 * k, I_dev + (int64_t)q0 * k, sel, st);
        if (rc != MQ_OK) return rc;
    }
    return MQ_OK;
}

int mq_bm25_grid_tile(void) { return GRID_TILE; }

int mq_bm25_grid_block_rows(int g) {
    if (g < 1 || g > GRID_TILE) return 0;
    return R / grid_width(g);
}

int mq_bm25_grid_chunk_queries(int64_t N, int nq, int g, size_t budget_bytes) {
    if (N < 1 || nq < 1 || g < 1 || g > GRID_TILE) return 0;
    int64_t c = (int64_t)(budget_bytes / ((size_t)g * (size_t)N * sizeof(float)));
    if (c > nq) c = nq;
    if (c > MAX_ROWS_PER_CALL / g) c = MAX_ROWS_PER_CALL / g;  // one selection launch takes the tile's g * c rows
    const int64_t rg = R / grid_width(g);
    const int64_t grid_cap = ((int64_t)1 << 31) / ST / ((N + rg - 1) / rg);  // threads of one scoring launch stay below 2^31
    if (c > grid_cap) c = grid_cap;
    if (c < 1) c = 1;
    return (int)c;
}

size_t mq_bm25_grid_workspace_bytes(int64_t N, int nq, int g, int k, size_t budget_bytes) {
    const int c = mq_bm25_grid_chunk_queries(N, nq, g, budget_bytes);
    if (c < 1 || k < 1 || k > MQ_KNN_MAX_K) return 0;
    // the score matrix, the selection's scratch, and the tile's [g * c, k] results before they go to their slices of D / I
    return align256((size_t)g * (size_t)c * (size_t)N * sizeof(float)) + topk_layout(g * c, k).total +
           align256((size_t)g * c * k * sizeof(float)) + align256((size_t)g * c * k * sizeof(int64_t));
}

int mq_bm25_search_grid_f32(const int64_t* ptr_dev, const int32_t* doc_dev, const int32_t* tf_dev, const uint8_t* code_dev,
                            const float* caches_dev, int G, int64_t N, int64_t n_terms, const int32_t* qptr_dev,
                            const int32_t* cterm_dev, const float* cweight_dev, int nq, int k, int flags, int64_t id_offset,
                            float* D_dev, int64_t* I_dev, void* ws_dev, size_t ws_bytes, size_t budget_bytes, void* stream) {
    // doc / tf / cterm / cweight may be NULL only when there is nothing behind them, as for mq_bm25_search_f32
    if (!ptr_dev || !code_dev || !caches_dev || !qptr_dev || !D_dev || !I_dev || !ws_dev || G < 1 || N < 1 || N > 0x7fffffffLL ||
        n_terms < 0 || nq < 1 || k < 1)
        return MQ_EINVAL;
    if (flags & ~MQ_KNN_FLAG_TIE_ID_DESC) return MQ_EINVAL;
    if (k > MQ_KNN_MAX_K) return MQ_EUNSUPPORTED;
    const int tile = G < GRID_TILE ? G : GRID_TILE;
    const int chunk = mq_bm25_grid_chunk_queries(N, nq, tile, budget_bytes);
    if (ws_bytes < mq_bm25_grid_workspace_bytes(N, nq, tile, k, budget_bytes)) return MQ_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* scores = static_cast<float*>(ws_dev);
    char* sel = static_cast<char*>(ws_dev) + align256((size_t)tile * (size_t)chunk * (size_t)N * sizeof(float));
    float* stage_D = reinterpret_cast<float*>(sel + topk_layout(tile * chunk, k).total);
    int64_t* stage_I = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(stage_D) + align256((size_t)tile * chunk * k * sizeof(float)));
    GridArgs a;
    a.ptr = ptr_dev; a.doc = doc_dev; a.tf = tf_dev; a.code = code_dev; a.N = N; a.n_terms = n_terms;
    a.qptr = qptr_dev; a.cterm = cterm_dev; a.cweight = cweight_dev;
    for (int g0 = 0; g0 < G; g0 += GRID_TILE) {
        const int gt = G - g0 < GRID_TILE ? G - g0 : GRID_TILE;
        const float* caches = caches_dev + (size_t)g0 * 256;
        for (int q0 = 0; q0 < nq; q0 += chunk) {
            const int n = nq - q0 < chunk ? nq - q0 : chunk;
            switch (grid_width(gt)) {
                case 1: launch_grid<1>(a, caches, gt, q0, n, scores, st); break;
                case 2: launch_grid<2>(a, caches, gt, q0, n, scores, st); break;
                case 4: launch_grid<4>(a, caches, gt, q0, n, scores, st); break;
                default: launch_grid<8>(a, caches, gt, q0, n, scores, st); break;
            }
            MQ_HIP(hipGetLastError());
            if (n == nq) {  // the tile's rows (setting, query) are consecutive rows of D / I: one selection over all of them
                const int rc = topk_rows(scores, gt * n, N, k, flags, id_offset, D_dev + (int64_t)g0 * nq * k,
                                         I_dev + (int64_t)g0 * nq * k, sel, st);
                if (rc != MQ_OK) return rc;
                continue;
            }
            // a query chunk: the tile's rows are selected at once into the staging tables, then each setting's n rows are copied
            // into its own slice of D / I (one strided copy per table)
            const int rc = topk_rows(scores, gt * n, N, k, flags, id_offset, stage_D, stage_I, sel, st);
            if (rc != MQ_OK) return rc;
            const int64_t at = ((int64_t)g0 * nq + q0) * k;
            MQ_HIP(hipMemcpy2DAsync(D_dev + at, (size_t)nq * k * sizeof(float), stage_D, (size_t)n * k * sizeof(float),
                                      (size_t)n * k * sizeof(float), gt, hipMemcpyDeviceToDevice, st));
            MQ_HIP(hipMemcpy2DAsync(I_dev + at, (size_t)nq * k * sizeof(int64_t), stage_I, (size_t)n * k * sizeof(int64_t),
                                      (size_t)n * k * sizeof(int64_t), gt, hipMemcpyDeviceToDevice, st));
        }
    }
    return MQ_OK;
}

}  // extern "C"
