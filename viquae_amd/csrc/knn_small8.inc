// knn_small8.inc -- the streaming screening scan for ONE query tile (<= 256 queries), included by knn.hip after knn_screen.inc.
//
// The reference searches in `Dataset.map` batches of 256 questions (experiments/ir/viquae/dpr/search/config.json:25 ->
// meerqat/ir/search.py:146): one query tile.  screen_scan_kernel then streams the bf16 copy of the shard exactly once, and
// the work is balanced between HBM (2.3 GB at 1.5M x 768) and the matrix pipe (0.59 TFLOP): it has to be a STREAMING kernel.
// The 256 x 256 tile kernel is not: it re-fetches the query tile every K step through the same LDS-DMA queue as the rows
// (as many L2 -> LDS bytes as HBM -> LDS bytes) and its two 64-KiB stages leave one step of lookahead for an HBM round
// trip (0.73-0.755 ms = 3.1 TB/s).  This kernel turns the roles around:
//
//   * the QUERIES live in registers for the whole launch: eight waves per workgroup, two per SIMD; wave w owns queries
//     [32 w, 32 w + 32) as the B operands of v_mfma_f32_32x32x16_bf16 for every k (register budget below) and does 4 NKB
//     MFMAs per item = one 32-row tile into ONE 32 x 32 accumulator;
//   * the whole LDS (160 KiB) is a ring of NST row tiles of [32 rows][dp] bf16 (48 KiB at dp = 768, NST = 3), filled by
//     LDS-DMA two tiles ahead (tools/probes/dma_stream_bench.hip: this ring alone streams 6.3 TB/s), no query traffic
//     at all, ONE barrier per item;
//   * 256 workgroups = 256 slabs of consecutive row tiles, one workgroup per CU, each row read from HBM exactly once.
//
// Why two waves per SIMD: a wave issues in order, and whatever stands between two of its MFMAs beyond 2-3 instructions (the
// selection's appends, the bookkeeping, barrier skew) is idle matrix pipe when it is alone on its SIMD.  With two, while one wave
// selects, appends, publishes or waits at the barrier, the other one's MFMAs keep the matrix pipe busy -- the ordinary latency
// hiding the 16-wave tile kernel has, without its query traffic.  No hand-placed riders: the selection is plain code after the
// item's MFMAs.  (Round 4's one-wave-per-SIMD kernel and its cycle accounting: DESIGN_HISTORY.md, profiles/r04_notes.md.)
//
// Selection is the tile kernel's, re-mapped: a lane column of the 32 x 32 accumulator is one query, so thresholds are
// lane-local; every (lane half, slab) is one stripe of disjoint rows whose running maximum is published into the
// query's slot of the slab (atomic max); the workgroup of slab s owns query s of the tile: it turns the 256 slot maxima
// of that query into a lower bound of the global k-th best S~ (k-th largest slot) and publishes it in gthr[s].
// Inside the streaming loop nothing is read from global memory by an instruction the compiler would wait for (a
// compiler-issued load waits with vmcnt(0) = a drained DMA ring; so does the reload of a spilled register, which is why
// every per-lane offset of a rare path is re-derived from the thread id there): the slot row of the owned query and the
// 256 gthr words arrive through the same LDS-DMA queue as the rows, one 1-KiB aux piece each per tile (waves 1 and 0), with
// the sc1 policy, and are consumed one ring turn later.  The first items of a slab are a warm-up: scored for the stripe
// maxima only (threshold +inf), and scored again at the END of the slab.
// Appends go to the lane's own half of the (query, slab) pool (512 slots = slices 4 kg .. 4 kg + 3 of the pool layout
// cand_select_kernel reads), filled front to back: POOL_LAYOUT_HALVES, recorded in the workspace word behind the tile's
// overflow flag.  A half that fills up flags the tile for the exact scan (tie-heavy data only: a slab pool receives ~10 keys).
//
// Same keys, same pools, same cand_select / rescore / final_select behind it: the search result is bit-identical to
// the tile kernel's and to the exact scan's (tests/test_small_scan_gpu.py).
//
// Register budget: 512 per SIMD lane / 2 waves = 256 per wave = 16 NKB accumulation registers (queries, named as MFMA B operands
// in asm: "a" constraints -- the unified register file of gfx950 lets A / B operands be accumulation registers; the compiler on
// its own copies them to VGPRs first) + at most 256 - 16 NKB VGPRs: 64 at NKB = 12 (accumulator 16, ring of four A fragments 16,
// fragment addresses 4, selection state) -- the kernel must not spill: a scratch reload inside the streaming loop is a vmcnt(0),
// a drained ring.
//
// The L2 metric -- and the centred inner product -- at d = 768 (round 6; round 5's attempts: tools/probes/small8_l2_rowterm.patch).  Its row term -||x||^2 / 2 sits in
// two extra bf16 columns = a 13th K block, one more than the registers hold.  When those two columns are ALONE in their block (d a
// multiple of 64) this kernel's ROWTERM instance does not stream that block and takes the term as fp32: -||x||^2 / 2 of a tile's
// 32 rows reaches the tile's ring slot one item before the tile is consumed (ordinary loads + one LDS store by a late wave, see
// rt_fetch / rt_deposit), and becomes the START of the accumulation chain: the accumulator is loaded from it (four 16-byte LDS
// reads) and the item's first MFMA adds to it instead of to 0.  The fp32 term is what the (h, l) pair of the two columns
// approximates to 2^-17, entering at the beginning of the chain instead of its end: covered by the margin of the two-column
// screen.  No LDS-DMA piece, no adds behind the MFMAs, the accumulator re-DEFINED as a whole vector: the instance keeps its
// registers (round 5's five formulations and this round's first eight spilled query fragments into the streaming loop).
//
// LDS-DMA: all NKB pieces of a tile ([32 rows][128 B] each) are issued by the four waves of group 0 (w < 4; group = w >> 2), eight
// rows each, one instruction per piece and wave; the late waves 4-7 issue nothing (issue_all).  The aux pieces (gthr words, the
// owned query's stripe slots) stay with waves 0 and 1.

constexpr int SM_ROWS = 32;                  // KB rows per ring tile
constexpr int SM_PIECE = SM_ROWS * SBK * 2;  // [32 rows][64 k] bf16 = 4 KiB: one contiguous piece of the tiled bf16 copy
constexpr int SM_MAX_NKB = 12;               // dp <= 768: 12 K blocks x 16 = 192 of a wave's 256 registers per lane hold its queries
constexpr int SM_AUX = 1024;                 // one aux piece (256 words) per ring slot and kind
constexpr int SM_MIN_TILES_PER_SLAB = 8;     // below that the tile kernel serves the search
constexpr int SM_HALF = SPOOL / 2;           // pool slots of one lane half
// ring depth: NST x (tile + two aux pieces) + thr / marg / scratch (3 KiB) within 160 KiB, at most 6
constexpr int sm_nst(int nkb) { return (157 * 1024) / (nkb * SM_PIECE + 2 * SM_AUX) > 6 ? 6 : (157 * 1024) / (nkb * SM_PIECE + 2 * SM_AUX); }

struct SmallArgs {
    ScreenArgs s;
    long long ntiles;   // 32-row tiles of the shard
    const float* sqn;   // screen_small8_kernel<12, true> only: ||x||^2 per row (L2: the row term -||x||^2 / 2 travels as fp32), or NULL with
                        // `rowterm` set: the term is read as the (h, l) pair of the copy's 13th K block (centred inner product)
    int rowterm;        // 0: the plain instance; 1: the ROWTERM instance
    int nkb_copy;       // K blocks of the stored bf16 copy per 256-row block (= the kernel's NKB, + 1 with the fp32 row term)
};

template <int N>
__device__ __forceinline__ void sm_wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}

// D = A(x rows) . B(queries) + C on the bf16 matrix pipe with the B operand in an accumulation register / a VGPR.
// `s_nop 1`: the A operand may have been written by a VALU move the compiler placed right in front of the statement.
// The accumulator lives in VGPRs: the selection reads it as ordinary VALU operands (in accumulation registers every score
// would cost a v_accvgpr_read first).
#define SM_MFMA_A(acc, xa, qb) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(xa), "a"(qb))
#define SM_MFMA_V(acc, xa, qb) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(xa), "v"(qb))
#define SM_MFMA_A0(acc, xa, qb) asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(xa), "a"(qb))

#ifdef MQ_TIMING
// cycle accounting per wave (tools/small_scan_timing.py; the slots are listed in the kernel)
#define SM_T(i) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); tacc_[i] += now_ - tlast_; tlast_ = now_; }
#else
#define SM_T(i)
#endif

#ifndef SM8_NXF
#define SM8_NXF(nkb) ((nkb) > 8 ? 4 : 6)
#endif

template <int NKB, bool ROWTERM = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void screen_small8_kernel(const SmallArgs sa) {
    constexpr int NST = sm_nst(NKB);
    constexpr int STAGE = NKB * SM_PIECE;
    constexpr int NM = 4 * NKB;  // MFMAs per item and wave
    constexpr int NXF = SM8_NXF(NKB);  // A fragments in flight (NKB > 8: up to 64 of the 128 VGPRs hold queries)
    static_assert(NST >= 3, "the ring needs two tiles of lookahead");
    constexpr int L_AUXG = NST * STAGE;            // [NST][256] u32: gthr words (wave 0's aux piece)
    constexpr int L_AUXS = L_AUXG + NST * SM_AUX;  // [NST][256] u32: the owned query's stripe slots (wave 1's aux piece)
    constexpr int L_THR = L_AUXS + NST * SM_AUX;   // thr[256] f32, marg[256] f32
    constexpr int L_SCR = L_THR + 2 * TQ * 4;      // [256] u32 scratch (end of the warm-up)
    static_assert(L_SCR + SM_AUX <= 160 * 1024, "LDS budget");
    constexpr int L_ROW = L_SCR + SM_AUX;  // ROWTERM: [NST][256] f32, ||x||^2 of the ring tiles' 32 rows, eight copies (one 1-KiB piece like the others)
    static_assert(!ROWTERM || L_ROW + NST * SM_AUX <= 160 * 1024, "LDS budget with the row terms");
    const ScreenArgs& a = sa.s;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* thr = reinterpret_cast<float*>(smem + L_THR);
    float* marg = thr + TQ;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0 .. 7
    const int grp = w >> 2, wr = w & 3;                      // DMA group, row quarter of a piece
    const int i = lane & 31, kg = lane >> 5;                 // MFMA operand row / column, k half
    const int slab = blockIdx.x;
    const int qt = 0;
    const int k = a.k;
    const long long tl0 = (sa.ntiles * slab) / a.S, tl1 = (sa.ntiles * (slab + 1)) / a.S;
    const int nt = (int)(tl1 - tl0);
    // item j: tile tl0 + (j < nt ? j : j - nt).  The first `warm_end` items feed the stripe maxima only (threshold +inf) and are
    // replayed at the end of the slab.  round 4 fixed warm_end = 2 and then WAITED (bounded polls of global memory, two
    // __syncthreads) for the other slabs' maxima and the owners' bounds: 35-55 us of a 600-us launch with the ring stalled.  Here
    // the warm-up simply goes on -- tiles keep streaming, maxima keep growing -- until the gthr copy that travels with every item
    // shows a bound for every real query of the tile (or SM8_WARM_CAP items have passed: whatever is there then is used, like
    // after round 4's last poll); the decision is workgroup-uniform through a double-buffered LDS flag word per early wave.
#ifndef SM8_OWNER_EVERY
#define SM8_OWNER_EVERY 127
#endif
#ifndef SM8_OWNER_AFTER
#define SM8_OWNER_AFTER(j) ((((j) + 1) & (j)) == 0 || ((j) & SM8_OWNER_EVERY) == 0)
#endif
#ifndef SM8_WARM_CAP
#define SM8_WARM_CAP 24
#endif
    const int wcap = nt / 2 < SM8_WARM_CAP ? (nt / 2 > 1 ? nt / 2 : 1) : SM8_WARM_CAP;
    int warm_end = -1;  // unknown yet
    unsigned* const wflag = reinterpret_cast<unsigned*>(smem + L_SCR);  // [2][4]: "a real query of early wave w has no bound yet", by item parity
    u64* mypools = a.pools + ((size_t)qt * a.S + slab) * (size_t)TQ * SPOOL;

    if (tid < TQ) {
        marg[tid] = a.margin[qt * TQ + tid];
        thr[tid] = marg[tid] < 0.f ? INFINITY : -INFINITY;
    }
    if (tid < 8) wflag[tid] = 1u;

    // ---- LDS-DMA: ring slot of item j = j % NST.  Early wave wr moves rows [8 wr, 8 wr + 8) of every piece, one instruction per
    // piece -- the 16-byte chunk c of row r is stored at chunk c ^ ((r >> 1) & 7) (the fragment reads below are then bank-conflict
    // free); the swizzle is applied to the SOURCE chunk.
    const int r8 = lane >> 3, ch = lane & 7;
    const unsigned voff = (unsigned)((8 * wr + r8) * 128 + ((ch ^ (((8 * wr + r8) >> 1) & 7)) * 16));
    const unsigned lds_ring = __builtin_amdgcn_readfirstlane(lds_addr_of(smem)) + (unsigned)(wr * 1024);
    const unsigned lds_auxg = __builtin_amdgcn_readfirstlane(lds_addr_of(smem + L_AUXG));
    const unsigned lds_auxs = __builtin_amdgcn_readfirstlane(lds_addr_of(smem + L_AUXS));
    const char* const xbase0 = reinterpret_cast<const char*>(a.Xb);
    const size_t blk_bytes = (size_t)(ROWTERM ? sa.nkb_copy : NKB) * S_OP_BYTES;  // (the stored copy keeps its 13th K block: the tile kernel reads it)
    const unsigned lds_row = __builtin_amdgcn_readfirstlane(lds_addr_of(smem + L_ROW));
    const void* const gthr_src = a.gthr + qt * TQ;
    const void* const smax_src = a.smax + (size_t)(qt * TQ + (slab < TQ ? slab : 0)) * a.ms;
    auto tile_of = [&](const int j) { return tl0 + (j < nt ? j : j - nt); };
    auto src_of = [&](const long long tile) { return xbase0 + (size_t)(tile >> 3) * blk_bytes + (size_t)(tile & 7) * SM_PIECE; };
    auto issue_all = [&](const char* src, const int slot) __attribute__((always_inline)) {  // this wave's share of one item, at once
        if (grp != 0) return;  // the late waves issue nothing (below)
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) dma16s(src + (size_t)kb * S_OP_BYTES, voff, lds_ring + slot * STAGE + kb * SM_PIECE);
        if (w == 0) dma16s_sc1(gthr_src, (unsigned)lane * 16u, lds_auxg + slot * SM_AUX);
        if (w == 1) dma16s_sc1(smax_src, (unsigned)lane * 16u, lds_auxs + slot * SM_AUX);
    };
    // this wave's pieces of item j have landed: NST - 2 younger items are in flight behind it (past the end of the slab the loop
    // keeps requesting its last item, so the count never changes)
    auto wait_item = [&]() __attribute__((always_inline)) {
        if (w < 2) sm_wait_vm<(NKB + 1) * (NST - 2)>();
        else if (w < 4) sm_wait_vm<NKB * (NST - 2)>();
    };

    // ROWTERM: the row terms travel by ORDINARY loads of one late wave (w == 4: the late waves issue no LDS-DMA, so a vmcnt(0) of
    // theirs waits for nothing but this load and the rare pool appends): during item j it requests ||x||^2 of the 32 rows of the tile
    // the early waves request for slot (j + NST - 1) % NST, and deposits -||x||^2 / 2 there during item j + 1 -- one barrier before
    // the tile is consumed.  ONE register lives across an item.  (Any LDS-DMA piece added to issue_all -- a norms array, the first
    // bytes of the copy's 13th K block, on wave 0, 1, 2 or all four -- pushed this instance over its 128 VGPRs: 56-88 bytes of
    // scratch, three query fragments reloaded inside the streaming loop; round 6, eight builds.)
    // Two sources: the L2 metric has ||x||^2 per row in fp32 (sa.sqn; the term is -1/2 of it); the centred inner product keeps its
    // row term c.(x - c) only as the (h, l) bf16 pair at the start of each row of the copy's 13th K block: h + l, exact in fp32, is
    // what those two columns contribute against the query's (1, 1).
    float rt_next = 0.f;
    auto rt_fetch = [&](const long long tile_) __attribute__((always_inline)) {
        if (sa.sqn) {
            long long r = tile_ * SM_ROWS + (lane & 31);
            if (r > a.N - 1) r = a.N - 1;  // past the shard: any value (those rows never enter a pool)
            rt_next = -0.5f * sa.sqn[r];
        } else {
            const unsigned v = *reinterpret_cast<const unsigned*>(src_of(tile_) + (size_t)NKB * S_OP_BYTES + (size_t)(lane & 31) * 128);
            rt_next = __uint_as_float(v << 16) + __uint_as_float(v & 0xFFFF0000u);
        }
    };
    auto rt_deposit = [&](const int slot_) __attribute__((always_inline)) {
        sm_wait_vm<0>();
        reinterpret_cast<float*>(smem + L_ROW + slot_ * SM_AUX)[lane & 31] = rt_next;
    };

    // A fragments: row i of the tile, 16-byte chunk (2 m + kg) ^ sw of its 128-byte K-block row (LDS byte addresses of the
    // CURRENT ring slot, advanced by one slot per item)
    const int sw = (i >> 1) & 7;
    unsigned xs[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) xs[m] = (unsigned)(i * 128 + (((2 * m + kg) ^ sw) * 16));

    // ---- selection state of this lane: its query is q = 32 w + (lane & 31), its rows of a tile 4 kg + (reg & 3) + 8 (reg >> 2)
    int n = 0;
    float rm = -INFINITY, pm = -INFINITY;  // stripe maximum of this lane half: running / as last published
    const bool publish = slab * a.sps + a.sps <= a.ms;
    const unsigned nrows = (unsigned)a.N;
    const int q = 32 * w + i;
    const bool live = __builtin_amdgcn_ballot_w64(a.margin[qt * TQ + q] >= 0.f) != 0ull;  // (marg[q] is another wave's write: not yet visible)

    unsigned owner_lo = 0u;  // wave 1: the bound published last (wave-uniform)
    auto publish_bound = [&](const unsigned* sl, const int lane_) __attribute__((always_inline)) {
        const uint4 v4 = *reinterpret_cast<const uint4*>(sl + lane_ * 4);
        const unsigned sv[4] = {v4.x, v4.y, v4.z, v4.w};
        unsigned mn = 0xFFFFFFFFu, mx = 0u;
        int nz = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            nz += sv[e] != 0u;
            mn = (sv[e] != 0u && sv[e] < mn) ? sv[e] : mn;
            mx = sv[e] > mx ? sv[e] : mx;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            nz += __shfl_xor(nz, o);
            const unsigned a_ = (unsigned)__shfl_xor((int)mn, o), b_ = (unsigned)__shfl_xor((int)mx, o);
            mn = a_ < mn ? a_ : mn;
            mx = b_ > mx ? b_ : mx;
        }
        if (nz < k) return false;
        // count(>= lo) >= k and count(>= hi) < k throughout.  The slots only grow, so the bound published last time is still a valid
        // lower end: later calls bisect a short interval and stop once it is within 2^-10 of the slots' spread (the first call:
        // ten steps; round 4 always did twelve -- ~3500 cycles of ONE wave with the other seven waiting at the next barrier)
        unsigned lo = owner_lo > mn ? owner_lo : mn, hi = mx == 0xFFFFFFFFu ? mx : mx + 1u;
        const unsigned tol = ((mx - mn) >> 10) + 1u;
        for (int it = 0; it < 12 && hi - lo > tol; ++it) {
            const unsigned mid = lo + ((hi - lo) >> 1);
            int cnt = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(sv[e] >= mid));
            if (cnt >= k) lo = mid; else hi = mid;
        }
        owner_lo = lo;
        if (lane_ == 0) __hip_atomic_fetch_max(a.gthr + qt * TQ + slab, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return true;
    };

    // ---- prologue: the first NST - 1 items, then the query registers; ONE wait for all of it
#pragma unroll
    for (int j = 0; j < NST - 1; ++j)
        if (j < nt + 1) issue_all(src_of(tile_of(j)), j % NST);
    if (ROWTERM && w == 4) {
#pragma unroll
        for (int j = 0; j < NST - 1; ++j)
            if (j < nt + 1) { rt_fetch(tile_of(j)); rt_deposit(j % NST); }
    }
    // the wave's queries -> accumulation registers (B operands: lane (col = lane & 31, kg) holds k = 16 m + 8 kg .. + 7 of query col)
    // (the compiler splits a 256-register budget 128 / 128 between VGPRs and accumulation registers once a function names the
    // latter: K blocks [0, 8) in accumulation registers, the rest in VGPRs)
    constexpr int QA = NKB < 8 ? NKB : 8, QV = NKB - QA;
    bf16x8_t qa[QA * 4], qv[QV * 4 > 0 ? QV * 4 : 1];
    {
        const char* qb = reinterpret_cast<const char*>(a.Qb) + (size_t)qt * TQ * a.dp * 2;
        const char* q0p = qb + (size_t)q * 128 + kg * 16;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const bf16x8_t v = *reinterpret_cast<const bf16x8_t*>(q0p + (size_t)kb * S_OP_BYTES + m * 32);
                if (kb < QA) qa[kb * 4 + m] = v; else qv[(kb - QA) * 4 + m] = v;
            }
    }
    // vmcnt(0): the explicit wait also tells the compiler that its own loads (the queries) have returned -- without it, it waits
    // for them at their first use INSIDE the loop, with counts that ignore the LDS-DMA pieces in flight: a drained ring every tile
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();                     // thr / marg

    // pool / slot offsets of the lane are re-derived from an opaque thread id where a rare path needs them: a loop invariant that
    // does not fit the registers is spilled, and a scratch reload inside the streaming loop drains the LDS-DMA ring
    auto lane_q = [&]() __attribute__((always_inline)) {
        unsigned t_ = threadIdx.x;
        asm volatile("" : "+v"(t_));
        return (int)(t_ >> 6) * 32 + (int)(t_ & 31);
    };
    auto lane_kg4 = [&]() __attribute__((always_inline)) {
        unsigned t_ = threadIdx.x;
        asm volatile("" : "+v"(t_));
        return 4u * ((t_ >> 5) & 1u);
    };
    auto pofs_of = [&]() __attribute__((always_inline)) { return (unsigned)(lane_q() * SPOOL) + lane_kg4() * (unsigned)(SM_HALF / 4); };
    auto sofs_of = [&]() __attribute__((always_inline)) { return (unsigned)((qt * TQ + lane_q()) * a.ms + slab * a.sps); };
    // a lane's pool half fills front to back (POOL_LAYOUT_HALVES: the usual handful of keys of a half share one line for cand_select)
    auto half_slot = [](const int n_) { return (unsigned)n_; };

    f32x16 acc = {0};
    // ---- selection of the accumulator of item js (screen_scan_kernel's sub-tile rule): v_max3 tree -> stripe maximum -> nothing
    // more when no lane of the wave reaches its threshold, else the register triples are tested the same way before the per-score
    // appends.  +inf while the item is a warm-up tile; a pool half that could not take 16 more scores stops taking any (flagged
    // at the end of the kernel).
    auto select = [&](const int js) __attribute__((always_inline)) {
        const long long tile_s = tile_of(js);
        const unsigned rbs = (unsigned)(tile_s * SM_ROWS) + lane_kg4();
        const float t = (warm_end < 0 || js < warm_end || n > SM_HALF - 16) ? INFINITY : thr[lane_q()];
        if ((tile_s + 1) * SM_ROWS > a.N) {  // the ragged last tile of the shard: row bounds, no maxima
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const unsigned r = rbs + (reg & 3) + 8 * (reg >> 2);
                if (r < nrows && acc[reg] >= t && n < SM_HALF) { mypools[pofs_of() + half_slot(n)] = make_key(acc[reg], r); ++n; }
            }
            return;
        }
        const float m0 = fmaxf(fmaxf(acc[0], acc[1]), acc[2]), m1 = fmaxf(fmaxf(acc[3], acc[4]), acc[5]);
        const float m2 = fmaxf(fmaxf(acc[6], acc[7]), acc[8]), m3 = fmaxf(fmaxf(acc[9], acc[10]), acc[11]);
        const float m4 = fmaxf(fmaxf(acc[12], acc[13]), acc[14]);
        const float gm = fmaxf(fmaxf(fmaxf(m0, m1), m2), fmaxf(fmaxf(m3, m4), acc[15]));
        rm = fmaxf(rm, gm);
        if (__builtin_amdgcn_ballot_w64(gm >= t) != 0ull) {
            u64* const P = mypools + pofs_of();
            auto site = [&](const int reg) __attribute__((always_inline)) {
                if (acc[reg] >= t) { P[half_slot(n)] = make_key(acc[reg], rbs + (reg & 3) + 8 * (reg >> 2)); ++n; }
            };
            if (__builtin_amdgcn_ballot_w64(m0 >= t) != 0ull) { site(0); site(1); site(2); }
            if (__builtin_amdgcn_ballot_w64(m1 >= t) != 0ull) { site(3); site(4); site(5); }
            if (__builtin_amdgcn_ballot_w64(m2 >= t) != 0ull) { site(6); site(7); site(8); }
            if (__builtin_amdgcn_ballot_w64(m3 >= t) != 0ull) { site(9); site(10); site(11); }
            if (__builtin_amdgcn_ballot_w64(m4 >= t) != 0ull) { site(12); site(13); site(14); }
            site(15);
        }
    };
#ifdef MQ_TIMING
    // cycle accounting per wave (tools/small_scan_timing.py): [0] wait for the item, [1] barrier, [2] bounds / publish / owner duty,
    // [3] selection, [4] the early waves' LDS-DMA issue, [5] the MFMAs, [6] s_memrealtime ticks of the kernel, [7] warm-up items
    unsigned long long tacc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast_ = __builtin_amdgcn_s_memtime();
    const unsigned long long rt0_ = __builtin_amdgcn_s_memrealtime();
#endif
    bool owner_done = false;  // wave 1: the owned query has had its first bound
    int j = 0;
    for (; j < nt + (warm_end < 0 ? wcap : warm_end); ++j) {
        const int slot = j % NST;
        wait_item();
        SM_T(0)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS stores of the last item (thr, wflag) are done
        __builtin_amdgcn_s_barrier();  // item j is in LDS for every wave; every wave is done reading item j - 1
        asm volatile("" ::: "memory");
        SM_T(1)
        if (warm_end < 0) {  // (workgroup-uniform: every wave reads the flag words the early waves wrote during item j - 1)
            const uint4 f = *reinterpret_cast<const uint4*>(wflag + 4 * ((j + 1) & 1));
            if (__builtin_amdgcn_readfirstlane((int)(f.x | f.y | f.z | f.w)) == 0 || j >= wcap) warm_end = j;
        }
        const int last = nt + (warm_end < 0 ? wcap : warm_end) - 1;
        const int dj = j + NST - 1 < last ? j + NST - 1 : last, dslot = (j + NST - 1) % NST;
        const char* const dsrc = src_of(tile_of(dj));
        if (ROWTERM && w == 4) {
            if (j > 0) rt_deposit((j + NST - 2) % NST);  // requested during item j - 1 for slot (j - 1 + NST - 1) % NST
            rt_fetch(tile_of(dj));
        }

        // Bookkeeping of the item: thresholds from the gthr copy that travelled with it, stripe maxima that grew, owner duty -- after the
        // wave's MFMAs: the matrix pipe starts right behind the barrier (early waves) / the selection starts there (late waves).
        auto bookkeeping = [&]() __attribute__((always_inline)) {
            // thresholds from the gthr copy that travelled with this item (issued NST - 1 items ago)
            if (tid < TQ) {
                const unsigned gb = reinterpret_cast<const unsigned*>(smem + L_AUXG + slot * SM_AUX)[tid];
                const float mg = marg[tid], cur = thr[tid];
                const float nt_ = key_score((u64)gb << 32) - mg;
                const float nv = (gb != 0u && mg >= 0.f && nt_ > cur) ? nt_ : cur;
                thr[tid] = nv;
                if (warm_end < 0) {
                    const bool unknown = __builtin_amdgcn_ballot_w64(mg >= 0.f && nv == -INFINITY) != 0ull;
                    if (lane == 0) wflag[4 * (j & 1) + w] = unknown ? 1u : 0u;
                }
            }
            // stripe maxima that grew during the last item
            if (publish && __builtin_amdgcn_ballot_w64(rm > pm) != 0ull) {
                if (rm > pm) { pm = rm; __hip_atomic_fetch_max(a.smax + sofs_of(), (unsigned)(make_key(rm, 0u) >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
            }
            // owner duty: during the warm-up every item until the owned query has its first bound (k of its slots are there), then after
            // 2, 4, 8 ... tiles and once per 128 tiles (every 32: 2.8 % slower, every call holds eight waves at the next barrier) -- from the slot copy of this item
            if (w == 1 && slab < TQ && j > 0 && (owner_done ? SM8_OWNER_AFTER(j) : true))
                owner_done = publish_bound(reinterpret_cast<const unsigned*>(smem + L_AUXS + slot * SM_AUX), lane) || owner_done;
        };
        SM_T(2)
        SM_T(4)
        if (!live) {  // a wave whose 32 queries are all padding only moves its share of the rows
            bookkeeping();
            issue_all(dsrc, dslot);
        } else {
            auto mfmas = [&]() __attribute__((always_inline)) {
                bf16x8_t xf[NXF];
#pragma unroll
                for (int g = 0; g < NXF && g < NM; ++g) xf[g] = *reinterpret_cast<const bf16x8_t*>(smem + xs[g & 3] + (g >> 2) * SM_PIECE);
                if (ROWTERM) {  // the chain starts from -||x||^2 / 2 of the lane's rows 4 kg + 8 jj .. + 3 (= registers 4 jj .. 4 jj + 3)
                    const float* rp = reinterpret_cast<const float*>(smem + L_ROW + slot * SM_AUX) + lane_kg4();
                    const float4 t0 = *reinterpret_cast<const float4*>(rp), t1 = *reinterpret_cast<const float4*>(rp + 8);
                    const float4 t2 = *reinterpret_cast<const float4*>(rp + 16), t3 = *reinterpret_cast<const float4*>(rp + 24);
                    // ONE definition of the whole vector: element-wise stores into `acc` keep the previous item's value alive up to
                    // here (sixteen registers across bookkeeping, DMA issue and barrier)
                    acc = (f32x16){t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w, t2.x, t2.y, t2.z, t2.w, t3.x, t3.y, t3.z, t3.w};
                }
#pragma unroll
                for (int g = 0; g < NM; ++g) {
                    if (g < 4 * QA) { if (g == 0 && !ROWTERM) SM_MFMA_A0(acc, xf[0], qa[0]); else SM_MFMA_A(acc, xf[g % NXF], qa[g]); }
                    else SM_MFMA_V(acc, xf[g % NXF], qv[g - 4 * QA]);
                    if (g + NXF < NM) xf[g % NXF] = *reinterpret_cast<const bf16x8_t*>(smem + xs[(g + NXF) & 3] + ((g + NXF) >> 2) * SM_PIECE);
                }
            };
            // The two waves of a SIMD (w and w + 4) run half an item out of phase: wave w does the MFMAs of item j and then
            // examines them; wave w + 4 first examines item j - 1 (its accumulator has waited through the barrier) and then does its
            // MFMAs -- each wave's selection, appends and bookkeeping overlap the other one's MFMAs instead of coinciding with its own
            // twin's (both waves leave the barrier together: in step, the matrix pipe idled through both selections)
            if (grp == 0) {
                mfmas();
                // the accumulator is read by VALU instructions next: 16-pass MFMA -> 18 wait states
                asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc));
                SM_T(5)
                bookkeeping();
                SM_T(2)
                select(j);
                SM_T(3)
                // ALL of the workgroup's LDS-DMA pieces of the item two tiles ahead are issued here, by the early waves, after their
                // selection: the CU's memory pipeline takes a 1-KiB piece every ~88 cycles at the HBM-bound rate, so whoever issues
                // blocks on its queue -- these waves would otherwise idle at the next barrier (~1200 cycles per item, measured),
                // while a piece issued among the late waves' MFMAs stalls the critical path (their 48 MFMAs took 2750 cycles)
                issue_all(dsrc, dslot);
                SM_T(4)
            } else {
                if (j > 0) select(j - 1);
                SM_T(3)
                mfmas();
                SM_T(5)
                bookkeeping();
                SM_T(2)
            }
        }
        SM_T(3)
        // the fragment addresses follow the ring
        {
            const unsigned step = slot + 1 == NST ? (unsigned)(-(NST - 1) * STAGE) : (unsigned)STAGE;
#pragma unroll
            for (int m = 0; m < 4; ++m) xs[m] += step;
        }
    }
    if (live && grp == 1) {  // the late waves' last item
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc));
        select(j - 1);
    }
    if (live && publish && rm > pm)  // (of no use to this launch any more; keeps the slots equal to what the lanes saw)
        __hip_atomic_fetch_max(a.smax + sofs_of(), (unsigned)(make_key(rm, 0u) >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sm_wait_vm<0>();  // no LDS-DMA piece may land after the workgroup has given its LDS back
#ifdef MQ_TIMING
    tacc_[6] = __builtin_amdgcn_s_memrealtime() - rt0_;
    tacc_[7] = (unsigned long long)warm_end;
    if (lane == 0 && a.dbg) { for (int i_ = 0; i_ < 8; ++i_) a.dbg[((size_t)blockIdx.x * 8 + w) * 8 + i_] = tacc_[i_]; }
#endif

    // ---- slice counts of the pool layout cand_select_kernel reads: this lane half dealt its entries over slices 4 kg .. 4 kg + 3
    {
        int* pc = a.pcount + (((size_t)qt * a.S + slab) * TQ + lane_q()) * NSL + (int)lane_kg4();
#pragma unroll
        for (int z = 0; z < 4; ++z) {  // the half's four slices fill one after the other
            const int left = n - z * SLCAP;
            pc[z] = left < 0 ? 0 : (left > SLCAP ? SLCAP : left);
        }
        if (n > SM_HALF - 16) a.ovf[qt] = 1;  // a half that filled up may have dropped keys: exact scan for the tile
        if (blockIdx.x == 0 && threadIdx.x == 0) a.ovf[1] = POOL_LAYOUT_HALVES;  // one query tile: the spare word behind its flag
    }
}
