"""Cases, row builders and a second reference for the direct tests of mq_topk_rows_f32 (tests/test_topk_rows_gpu.py); numpy only,
imports without a GPU and without torch.

The selection (csrc/bm25.hip: topk_hist_kernel / topk_gather_kernel / topk_sort_kernel) is a radix select on the 64-bit key
(score bits << 32) | (id_asc ? ~id : id): up to six histogram passes over the key's digits, `split` workgroups per row (each reads
one chunk of per = ceil(N / split) elements with a thread stride of TT), a gather of the winners, a bitonic sort of kpad keys.

Row FAMILIES (each a uint32 bit pattern viewed as float32, seeded, non-negative and finite):
  distinct      uniform values + 1e-3: the score digits decide, three passes
  levels50      50 levels: long tied runs, score and id digits decide
  all_equal     one value everywhere: only the id passes decide
  two_ulp       `upper` elements hold the successor of the float the others hold: the lowest score digit decides, then the ids
  extremes      denormals, the smallest normal, 1.0 and its successor, FLT_MAX and its predecessor, non-hits
  sparse        `hits` hits at random positions that always include 0 and N - 1 (as far as `hits` allows), zeros elsewhere
  chunk_edges   zeros but for plants at 0, N - 1 and both sides of every workgroup boundary (c * per - 1, c * per), the two sides of
                a boundary EQUAL, and lower fillers elsewhere so that there are more than k plants: winners are the first and last
                element a workgroup reads, and ties cross workgroups

`schedule` restates the pass decisions (histogram, suffix sums, bucket choice) in numpy without sorting anything: a second
reference, independent of bm25_restatement.topk.  tests/test_topk_rows_cases_cpu.py checks on these restatements alone that every
case reaches the regime it is listed for."""
import collections
import ctypes

import numpy as np

TT = 1024          # the kernel's TT: threads (and thread stride) of a selection workgroup; no getter reports it
MAX_ROWS = 65535   # the kernel's MAX_ROWS_PER_CALL
MAX_K = 2048       # MQ_KNN_MAX_K
TIE_ORDERS = ("id_asc", "id_desc")
K_SWEEP = (1, 2, 3, 100, 300, 1024, 1025, 2047, 2048)
K_EDGES = (1, 300, 2048)
K_PADS = (5, 9, 17, 33, 200)       # kpad 8, 16, 32, 64, 256: with the sweep, every size of the final sort from 2 to 2048
BIG_OFFSET = 2 ** 40 + 7
EXTREME_BITS = (1, 2, 3, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3F800001, 0x7F7FFFFE, 0x7F7FFFFF, 0)
ONE = 0x3F800000   # bits of 1.0f; two_ulp rows hold it and its successor

Row = collections.namedtuple("Row", "family arg")          # arg: hits (sparse), upper (two_ulp), else None
Case = collections.namedtuple("Case", "name N rows ks tie_orders id_offset purpose")


# ---------------------------------------------------------------------------------------------------------------- the library's geometry
def launch_info(lib, rows, N):
    """(split, [shift of every pass]) from mq_topk_rows_launch_info; raises on a refused (rows, N)."""
    out = (ctypes.c_int64 * 8)()
    rc = lib.mq_topk_rows_launch_info(int(rows), int(N), out)
    if rc != 0:
        raise ValueError(f"mq_topk_rows_launch_info({rows}, {N}) = {rc}")
    return int(out[0]), [int(out[2 + p]) for p in range(int(out[1]))]


def split_of(lib, rows, N):
    return launch_info(lib, rows, N)[0]


def shifts_of(lib):
    return launch_info(lib, 1, 1)[1]


def rows_per_wg(lib):
    """The kernel's ROWS_PER_WG: the largest N one workgroup takes alone when a single row is selected (bisection on the getter)."""
    lo, hi = 1, 1 << 30   # split(lo) == 1 < split(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if split_of(lib, 1, mid) == 1:
            lo = mid
        else:
            hi = mid
    return lo


def max_split(lib):
    """The kernel's MAX_SPLIT: the workgroups one row of the largest N gets."""
    return split_of(lib, 1, 2 ** 31 - 1)


def kpad_of(k):
    p = 2
    while p < k:
        p <<= 1
    return p


# ---------------------------------------------------------------------------------------------------------------- rows
def _positions(rng, N, hits):
    """`hits` distinct positions in [0, N), 0 and N - 1 among them as far as `hits` allows."""
    fixed = [0, N - 1][:hits] if N > 1 else [0][:hits]
    inner = rng.choice(max(N - 2, 0), hits - len(fixed), replace=False) + 1 if hits > len(fixed) else []
    return np.concatenate([np.array(fixed, dtype=np.int64), np.asarray(inner, dtype=np.int64)])


def boundaries(N, split):
    """First elements of the second and later workgroups' chunks."""
    per = (N + split - 1) // split
    return [c * per for c in range(1, split) if c * per < N]


def make_row(row, N, split, seed):
    """One row of N float32 (see the module docstring).  `split` is only read by chunk_edges."""
    rng = np.random.default_rng(seed)
    bits = np.zeros(N, dtype=np.uint32)
    if row.family == "distinct":
        bits = (rng.random(N).astype(np.float32) + np.float32(1e-3)).view(np.uint32)
    elif row.family == "levels50":
        bits = (rng.integers(0, 50, N).astype(np.float32) / np.float32(7)).view(np.uint32)
    elif row.family == "all_equal":
        bits[:] = np.float32(0.625).view(np.uint32)
    elif row.family == "two_ulp":
        bits[:] = ONE
        bits[rng.choice(N, min(row.arg, N), replace=False)] = ONE + 1
    elif row.family == "extremes":
        bits = np.array(EXTREME_BITS, dtype=np.uint32)[rng.integers(0, len(EXTREME_BITS), N)]
    elif row.family == "sparse":
        at = _positions(rng, N, row.arg)
        bits[at] = (rng.random(len(at)).astype(np.float32) + np.float32(0.1)).view(np.uint32)
    elif row.family == "chunk_edges":
        edges = boundaries(N, split)
        free = np.ones(N, dtype=bool)
        free[[0, N - 1] + edges + [e - 1 for e in edges]] = False
        free = np.flatnonzero(free)
        fill = rng.choice(free, min(MAX_K + 50, len(free) // 2), replace=False)
        bits[fill] = (rng.random(len(fill)).astype(np.float32) * np.float32(0.5) + np.float32(0.25)).view(np.uint32)   # below 1
        for c, e in enumerate(edges):   # the two sides of boundary c hold the same value, another one per boundary
            bits[e - 1] = bits[e] = np.float32(2 + c).view(np.uint32)
        bits[0] = np.float32(1000).view(np.uint32)
        bits[N - 1] = np.float32(1001).view(np.uint32)
    else:
        raise ValueError(row.family)
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    values = bits.view(np.float32)
    assert np.isfinite(values).all() and not (bits >> 31).any()
    return values


def matrix(case, split):
    """The case's [rows, N] float32 matrix; `split` = split_of(lib, len(case.rows), case.N)."""
    X = np.zeros((len(case.rows), case.N), dtype=np.float32)
    for r, row in enumerate(case.rows):
        X[r] = make_row(row, case.N, split, seed=1000 * r + case.N % 997)
    return X


# ---------------------------------------------------------------------------------------------------------------- the second reference
def keys_of(row, tie_order):
    """The 64-bit keys of the row's hits (elements whose bits are not zero), in id order."""
    bits = np.ascontiguousarray(row).view(np.uint32)
    ids = np.flatnonzero(bits).astype(np.uint64)
    low = ids if tie_order == "id_desc" else (~ids & np.uint64(0xFFFFFFFF))
    return (bits[ids.astype(np.int64)].astype(np.uint64) << np.uint64(32)) | low


Pass = collections.namedtuple("Pass", "shift nonempty bucket want above")   # bucket: size of the chosen one; want: AFTER the pass
Schedule = collections.namedtuple("Schedule", "passes per_pass keys")       # passes: an int, or "all" when hits <= k


def schedule(row, k, tie_order, shifts):
    """The pass decisions of the radix select, restated: per pass the histogram of the digit at `shift` over the keys that match the
    digits decided so far, the bucket d with (keys in buckets >= d) >= want > (keys in buckets > d), want -= above; the selection
    is done once the chosen bucket holds exactly `want` keys.  Returns the passes needed ("all": no more hits than k, every hit is
    taken after the first histogram), the per-pass figures, and the selected keys in no particular order.  Nothing is sorted."""
    cur = keys_of(row, tie_order)
    if len(cur) <= k:
        return Schedule("all", [], cur)
    want, taken, per_pass, top = k, [], [], 64
    for p, shift in enumerate(shifts):
        width = top - shift
        digit = ((cur >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64)
        hist = np.bincount(digit, minlength=1 << width)
        sfx = np.concatenate([np.cumsum(hist[::-1])[::-1], [0]])           # sfx[d] = keys in buckets >= d
        d = int(np.flatnonzero((sfx[:-1] >= want) & (sfx[1:] < want))[0])
        above = int(sfx[d + 1])
        taken.append(cur[digit > d])
        want -= above
        cur = cur[digit == d]
        per_pass.append(Pass(shift, int(np.count_nonzero(hist)), int(hist[d]), want, above))
        top = shift
        if hist[d] == want:
            taken.append(cur)
            return Schedule(p + 1, per_pass, np.concatenate(taken))
    raise AssertionError("distinct keys: the last pass always ends the selection")


def split_keys(keys, tie_order):
    """(score bits uint32, ids int64) of keys."""
    low = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return (keys >> np.uint64(32)).astype(np.uint32), (low if tie_order == "id_desc" else ~low).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- the case list
FAMILIES = ("distinct", "levels50", "all_equal", "two_ulp", "extremes", "sparse", "chunk_edges")
TWO_ULP_UPPER = 650                  # between the swept k 300 and 1024: one k below and one above the count of the larger value
SPARSE_HITS = (0, 1, 2, 299, 300, 301, 2047, 2048, 2049)   # k - 1, k, k + 1 hits for k = 1, 300, 2048 of the sweep, and none / one


def _sparse_rows(n, N, k, seed):
    """n sparse rows of at most 10 % hits; the first five have 0, 1, k - 1, k, k + 1."""
    rng = np.random.default_rng(seed)
    hits = [0, 1, k - 1, k, k + 1] + rng.integers(0, N // 10 + 1, n - 5).tolist()
    return tuple(Row("sparse", int(h)) for h in hits)


def cases(lib):
    """The list both test files run: (name, N, rows, k values, tie orders, id_offset, purpose)."""
    W, S = rows_per_wg(lib), max_split(lib)     # 16,384 and 64
    out = []

    def add(name, N, rows, ks, purpose, id_offset=0):
        out.append(Case(name, int(N), tuple(rows), tuple(ks), TIE_ORDERS, id_offset, purpose))

    for N in (1, 2):
        for row in (Row("distinct", None), Row("all_equal", None), Row("two_ulp", 1), Row("sparse", 0), Row("sparse", 1)):
            add(f"N{N}-{row.family}{'' if row.arg is None else row.arg}", N, [row], (1, 2, 3), "smallest rows; kpad 2 and 4")
    for N in (TT - 1, TT, TT + 1):
        add(f"N{N}-stride", N, [Row("distinct", None), Row("all_equal", None), Row("chunk_edges", None)], K_EDGES,
            "the workgroup's thread stride")
    for N in (W, W + 1):
        add(f"N{N}-split", N, [Row("all_equal", None), Row("chunk_edges", None)], K_EDGES,
            "split 1 -> 2; the second workgroup ends on a short chunk")
    mixed = ([Row("distinct", None), Row("levels50", None), Row("all_equal", None), Row("two_ulp", TWO_ULP_UPPER), Row("extremes", None)]
             + [Row("sparse", h) for h in SPARSE_HITS] + [Row("chunk_edges", None)])
    add("N70001-mixed", 70_001, mixed, K_SWEEP, "the k sweep; rows that finish after different passes in one launch", BIG_OFFSET)
    for row in mixed:
        if row.family != "sparse" or row.arg in (0, 1, 299, 300, 301):
            add(f"N70001-{row.family}{'' if row.arg is None else row.arg}", 70_001, [row], K_SWEEP, "the k sweep, one family alone")
    add("N70001-kpads", 70_001, [Row("levels50", None), Row("distinct", None)], K_PADS, "the sizes of the final sort the sweep leaves out")
    add("N50001-rows700", 50_001, _sparse_rows(700, 50_001, 100, 7), (100,), "fill caps the split below ceil(N / ROWS_PER_WG)")
    add("N17000-rows2048", 17_000, _sparse_rows(2048, 17_000, 100, 8), (100,), "fill = 1")
    add("cap-first", (S - 1) * W + 1, [Row("chunk_edges", None)], (300,), "first N at the cap of MAX_SPLIT workgroups")
    add("N2^21+100", 2 ** 21 + 100, [Row("all_equal", None), Row("chunk_edges", None)], K_EDGES,
        "the shift-21 id pass separates rows; the cap of MAX_SPLIT")
    return out
