"""Cases, input builders, references and tolerances of the attention kernel tests (tests/test_attention_gpu.py); imports without a GPU.

The two kernels (csrc/encoder.hip: attention_mfma_kernel, fp32 MFMAs; attention_x3_kernel, split-bf16 MFMAs) compute
softmax(q k^T * scale + mask) v per (sequence, head).  A BATCH here is a token matrix qkv [T, 3 * heads * 64] with the row span of
every sequence: a dense batch has spans (b * L, L) and a mask [B, L], a packed batch has spans of different lengths and no mask.

References (all on the CPU, per (sequence, head)):
  ref     float64 torch.  Padding: (1 - mask) * finfo(float32).min added in float64 (the BERT form; a sequence with no live key gets
          L equal logits, hence uniform attention).  Causal exclusion: -inf.
  f32     the same formula in float32; e32 = max |f32 - ref| is the fp32 error of THIS computation on THESE inputs.
  ref_x3  float64 attention whose logits are the restated split: hi = bf16(x), lo = bf16(x - hi) (round to nearest even, as split_bits
          in csrc/encoder.hip), s = scale * sum_d (qh kh + qh kl + ql kh); softmax and P V exact.
Bounds: fp32 kernel |out - ref| <= 4 e32 (summation orders differ, as in test_single_query_attention_kernel); split-bf16 kernel
|out - ref_x3| <= 4 e32 + 2^-16 max |v| (the P V products drop lo lo and round each lo: 3 * 2^-18 relative per product, sum p = 1).
tests/test_attention_cases_cpu.py checks by arithmetic that every case has the property it is listed for."""
import collections
import functools

import torch

DH = 64
SCALE = 0.125
F32_MIN = torch.finfo(torch.float32).min

Batch = collections.namedtuple("Batch", "name qkv spans heads masks nonbinary")  # masks: None or a list of int64 [len] / None


# ---------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------
def split_pair(x):
    """the restated split of a float32 tensor: (hi, lo) bfloat16 tensors"""
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def _heads_first(x, heads):
    return x.reshape(x.shape[0], heads, DH).transpose(0, 1)   # [heads, len, 64]


def attend(batch, causal=False, dtype=torch.float64, split=False):
    """softmax(q k^T * SCALE + mask) v of every sequence of the batch -> [T, heads * 64] in `dtype`"""
    H = batch.heads * DH
    out = torch.zeros((batch.qkv.shape[0], H), dtype=dtype)
    for n, (r0, ln) in enumerate(batch.spans):
        rows = batch.qkv[r0:r0 + ln]
        q32, k32 = _heads_first(rows[:, :H], batch.heads), _heads_first(rows[:, H:2 * H], batch.heads)
        v = _heads_first(rows[:, 2 * H:], batch.heads).to(dtype)
        if split:
            (qh, ql), (kh, kl) = split_pair(q32), split_pair(k32)
            qh, ql, kh, kl = [t.to(dtype) for t in (qh, ql, kh, kl)]
            s = (qh @ kh.transpose(1, 2) + qh @ kl.transpose(1, 2) + ql @ kh.transpose(1, 2)) * SCALE
        else:
            s = (q32.to(dtype) @ k32.to(dtype).transpose(1, 2)) * SCALE
        m = batch.masks[n] if batch.masks is not None else None
        if m is not None:
            dead = (m == 0).to(dtype) if batch.nonbinary else 1.0 - m.to(dtype)   # the kernels test != 0
            s = s + (dead * F32_MIN)[None, None, :]
        if causal:
            s = s.masked_fill(torch.ones((ln, ln), dtype=torch.bool).triu(1)[None], float("-inf"))
        out[r0:r0 + ln] = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(ln, H)
    return out


Refs = collections.namedtuple("Refs", "ref ref_x3 e32 vmax bound_f32 bound_x3")
_REFS = {}


def refs(batch, causal=False):
    """the float64 references of a batch and the bounds derived from them (computed once per (batch, causal), never modified)"""
    key = (batch.name, bool(causal))
    if key not in _REFS:
        ref = attend(batch, causal)
        e32 = float((attend(batch, causal, dtype=torch.float32).double() - ref).abs().max())
        H = batch.heads * DH
        vmax = float(torch.cat([batch.qkv[r0:r0 + ln, 2 * H:] for r0, ln in batch.spans]).abs().max())
        _REFS[key] = Refs(ref, attend(batch, causal, split=True), e32, vmax, 4 * e32, 4 * e32 + 2.0 ** -16 * vmax)
    return _REFS[key]


def probabilities(batch, n, dtype=torch.float64):
    """[heads, len, len] attention probabilities of sequence n (no mask, not causal): what the CPU conditions look at"""
    H = batch.heads * DH
    r0, ln = batch.spans[n]
    rows = batch.qkv[r0:r0 + ln].to(dtype)
    s = _heads_first(rows[:, :H], batch.heads) @ _heads_first(rows[:, H:2 * H], batch.heads).transpose(1, 2) * SCALE
    return s, torch.softmax(s, -1)


# ---------------------------------------------------------------------------------------------------
# dispatch rule of mq_attention_packed_f32 / mq_attention_split_f32, restated
# ---------------------------------------------------------------------------------------------------
Launch = collections.namedtuple("Launch", "nkt multi wide waves grid_y qpb")   # qpb: queries per workgroup


def dispatch(L, bf16x3, packed):
    """the instantiation a launch with max_len (packed) or L (dense) = `L` takes"""
    nkt = 2 if L <= 64 else 4 if L <= 128 else 8
    wide = bool(packed and bf16x3 and 128 < L <= 256)
    waves = (L + 31) // 32 if wide else (4 if L >= 97 else (L + 31) // 32)
    return Launch(nkt, L > 256, wide, waves, 1 if wide else (L + 127) // 128, 32 * waves if wide else 128)


def nt_live(ln, launch):
    """key tiles the split-bf16 kernel stages for a sequence of ln tokens"""
    return launch.nkt if launch.multi else min((ln + 31) // 32, launch.nkt)


def idle_waves(ln, launch):
    """waves without a query, over the workgroups of a sequence of ln tokens that do not return early"""
    return sum(1 for y in range(launch.grid_y) if y * launch.qpb < ln
               for w in range(launch.waves) if y * launch.qpb + 32 * w >= ln)


def early_returns(ln, launch):
    return sum(1 for y in range(launch.grid_y) if y * launch.qpb >= ln)


# ---------------------------------------------------------------------------------------------------
# A. packed launches
# ---------------------------------------------------------------------------------------------------
def _randn(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def packed_batch(name, lengths, heads, seed, qkv=None):
    cu = [0]
    for ln in lengths:
        cu.append(cu[-1] + ln)
    if qkv is None:
        qkv = _randn(seed, cu[-1], 3 * heads * DH)
    return Batch(name, qkv, [(cu[i], ln) for i, ln in enumerate(lengths)], heads, None, False)


PackedCase = collections.namedtuple("PackedCase", "name lengths heads launches")   # launches: [(lengths launched, max_len)]

# the packed order is unsorted and every matrix holds one sequence of another class, which no launch of the case owns
PACKED_CASES = [
    PackedCase("upto64", [33, 1, 70, 64, 31, 2, 32], 2, [([1, 31, 32, 33, 64, 2], 64), ([1, 31, 32, 33, 2], 33), ([1, 31, 2], 31)]),
    PackedCase("upto128", [97, 65, 20, 128, 96, 100], 3, [([65, 96, 97, 128, 100], 128), ([65, 96], 96)]),
    PackedCase("upto256", [160, 129, 40, 256, 130, 255, 200], 2, [([129, 160, 255, 256, 130, 200], 256), ([129, 160, 130], 160)]),
    PackedCase("over256", [300, 50, 513, 257], 2, [([257, 300, 513], 513)]),
]
PACKED_LAUNCHES = [(c.name, i) for c in PACKED_CASES for i in range(len(c.launches))]
# all four classes in one matrix, classes from encoders.pack_plan_from_lengths (MIXED_L: the padded length the planner is told;
# 1341 real tokens of 8 * 600 is far below its 90 % bar, so the plan is not declined)
MIXED = PackedCase("mixed", [33, 300, 100, 513, 2, 200, 64, 129], 2, None)
MIXED_L = 600


def packed_case(name):
    return MIXED if name == "mixed" else next(c for c in PACKED_CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def packed_case_batch(name):
    c = packed_case(name)
    return packed_batch("packed-" + name, c.lengths, c.heads, seed=1000 + len(c.lengths) * 7 + c.lengths[0])


def seq_ids_of(case, launched):
    """sequence numbers (positions in the packed matrix) of the launched lengths, in the order the launch lists them"""
    return [case.lengths.index(ln) for ln in launched]


# ---------------------------------------------------------------------------------------------------
# B. dense launches with production's masks and the block edges
# ---------------------------------------------------------------------------------------------------
MaskRow = collections.namedtuple("MaskRow", "name mask dead live")   # dead: [lo, hi) ranges with no live key; live: keys that are live


def _mask(L, ones=(), zeros=()):
    m = torch.zeros(L, dtype=torch.int64)
    for lo, hi in ones:
        m[lo:hi] = 1
    for lo, hi in zeros:
        m[lo:hi] = 0
    return m


def _eca(L, n_text):
    """ECA's joint mask: text, padding up to 256, face slots (1, 1, 0, 0[, 0]: two faces found), one image"""
    m = _mask(L, ones=[(0, n_text), (256, 258), (L - 1, L)])
    dead = ([(n_text, 256)] if n_text < 256 else []) + [(258, L - 1)]
    return MaskRow(f"eca{L}_text{n_text}", m, dead, [0, n_text - 1, 256, 257, L - 1])


def _block_rows(L):
    rows = [MaskRow("first_block_dead", _mask(L, ones=[(256, L)]), [(0, 256)], [256, L - 1]),
            MaskRow("only_255", _mask(L, ones=[(255, 256)]), [(0, 255), (256, L)], [255]),
            MaskRow("only_256", _mask(L, ones=[(256, 257)]), [(0, 256), (257, L)], [256]),
            MaskRow("edge_pair_dead", _mask(L, ones=[(0, L)], zeros=[(255, 257)]), [(255, 257)], [0, 254, 257, L - 1])]
    if L > 512:   # block 1 = keys 256 .. 511 is followed by a live block
        rows.insert(1, MaskRow("later_block_dead", _mask(L, ones=[(0, 256), (512, L)]), [(256, 512)], [0, 255, 512]))
    else:         # block 1 = keys 256 .. L - 1 is the last one
        rows.insert(1, MaskRow("later_block_dead", _mask(L, ones=[(0, 256)]), [(256, L)], [0, 255]))
    return rows


def _nonbinary(m, seed):
    """some of the 1s replaced by 2 or 7"""
    r = torch.rand(m.shape, generator=torch.Generator().manual_seed(seed))
    return torch.where((m != 0) & (r < 0.3), torch.full_like(m, 2), torch.where((m != 0) & (r > 0.7), torch.full_like(m, 7), m))


MASK_ROWS = {
    261: [_eca(261, n) for n in (256, 140, 17)],
    262: [_eca(262, n) for n in (256, 140, 17)],
    200: [MaskRow("tile_64_95_dead", _mask(200, ones=[(0, 200)], zeros=[(64, 96)]), [(64, 96)], [0, 63, 96, 199]),
          MaskRow("tile_0_31_dead", _mask(200, ones=[(32, 200)]), [(0, 32)], [32, 199]),
          MaskRow("only_last", _mask(200, ones=[(199, 200)]), [(0, 199)], [199]),
          MaskRow("prefix_150", _mask(200, ones=[(0, 150)]), [(150, 200)], [0, 149])],
    300: _block_rows(300),
    513: _block_rows(513),
}
MASK_HEADS = {261: 3, 262: 2, 200: 2, 300: 2, 513: 2}
# the != 0 case: ECA's holes and a dead tile, with 2s and 7s among the live keys (non-causal only; the reference uses mask != 0)
NONBINARY_L = 261
NONBINARY_ROWS = [MaskRow(r.name + "_2s_and_7s", _nonbinary(r.mask, 5 + i), r.dead, r.live) for i, r in enumerate(MASK_ROWS[261])]


def dense_batch(name, qkv, L, heads, masks=None, nonbinary=False):
    B = qkv.shape[0] // L
    return Batch(name, qkv, [(b * L, L) for b in range(B)], heads, masks, nonbinary)


def causal_ok(row):
    """every query keeps a live key at or before itself <=> key 0 is live"""
    return bool(row.mask[0] != 0)


def mask_rows(L, causal, nonbinary=False):
    rows = NONBINARY_ROWS if nonbinary else MASK_ROWS[L]
    return [r for r in rows if causal_ok(r)] if causal else rows


@functools.lru_cache(maxsize=None)
def mask_batch(L, causal, nonbinary=False):
    rows, heads = mask_rows(L, causal, nonbinary), MASK_HEADS[L]
    qkv = _randn(2000 + L, len(MASK_ROWS[L]) * L, 3 * heads * DH)[:len(rows) * L]
    return dense_batch(f"mask-{L}-{int(causal)}-{int(nonbinary)}", qkv, L, heads, [r.mask for r in rows], nonbinary)


MASK_CASES = [(L, c, False) for L in MASK_ROWS for c in (False, True)] + [(NONBINARY_L, False, True)]

# ---------------------------------------------------------------------------------------------------
# C. a sequence with no live key (row 1 of 3; its neighbours are ordinary prefix masks)
# ---------------------------------------------------------------------------------------------------
EMPTY_L = {37: 3, 200: 2, 300: 2}   # L -> heads
EMPTY_ROW = 1


@functools.lru_cache(maxsize=None)
def empty_batch(L, filled=False):
    """filled: the same batch with the empty row's mask all ones in its place (the oracle of the neighbours' bits)"""
    heads = EMPTY_L[L]
    masks = [_mask(L, ones=[(0, L)]), _mask(L, ones=[(0, L)] if filled else []), _mask(L, ones=[(0, L // 2 + 1)])]
    return dense_batch(f"empty-{L}-{int(filled)}", _randn(3000 + L, 3 * L, 3 * heads * DH), L, heads, masks)


# ---------------------------------------------------------------------------------------------------
# D. logits of checkpoint size
# ---------------------------------------------------------------------------------------------------
BIG_KINDS = ("rising", "falling", "spike", "wide")
BIG_L = {100: 2, 200: 3, 300: 2, 513: 2}   # L -> heads
BIG_PACKED = [513, 300]
STEP_MIN, SPIKE_GAP, SPIKE_P = 8.0, 60.0, 0.999
NOISE = 0.05
BLOCK_STEP = 9.5


def spike_positions(L):
    return sorted({p for p in (0, 255, 256, L - 1) if p < L})


def _big_sequence(kind, L, heads, seed, spike_at=0):
    """one sequence [L, 3 * heads * 64].  Per head u is a direction with |u|^2 = 64, so SCALE * (c u) . (g u) = 8 c g; queries are
    q_i = c_i u with c_i in [0.9, 1] (every row differs), keys k_j = g_j u, both plus NOISE * N(0, 1).
      rising   8 g_j = -40 + R j / L + 9.5 (j // 256), R = 80 - 9.5 ((L - 1) // 256): logits from -40 to about 40, and every 256-key
               block starts 9.5 above the end of the previous one (so does the one-key last block of L = 513)
      falling  the negative of that: block 0 holds the maximum
      spike    g = 10 at one key, 0 elsewhere: that key sits 72 .. 80 above the rest
      wide     q, k = 3 N(0, 1)"""
    g = torch.Generator().manual_seed(seed)
    H = heads * DH
    qkv = torch.randn((L, 3 * H), generator=g)
    if kind == "wide":
        qkv[:, :2 * H] *= 3.0
        return qkv
    j = torch.arange(L, dtype=torch.float32)
    if kind == "spike":
        gj = torch.zeros(L)
        gj[spike_at] = 10.0
    else:
        gj = (-40.0 + (80.0 - BLOCK_STEP * ((L - 1) // 256)) * j / L + BLOCK_STEP * (j // 256)) / 8.0
        if kind == "falling":
            gj = -gj
    c = 0.9 + 0.1 * torch.rand(L, generator=g)
    for h in range(heads):
        u = torch.randn(DH, generator=g)
        u = u * (8.0 / u.norm())
        qkv[:, h * DH:(h + 1) * DH] = c[:, None] * u[None] + NOISE * qkv[:, h * DH:(h + 1) * DH]
        qkv[:, H + h * DH:H + (h + 1) * DH] = gj[:, None] * u[None] + NOISE * qkv[:, H + h * DH:H + (h + 1) * DH]
    return qkv


@functools.lru_cache(maxsize=None)
def big_batch(kind, L):
    heads = BIG_L[L]
    spikes = spike_positions(L) if kind == "spike" else [0, 0]
    seqs = [_big_sequence(kind, L, heads, 4000 + 10 * L + n, p) for n, p in enumerate(spikes)]
    return dense_batch(f"big-{kind}-{L}", torch.cat(seqs), L, heads)


BIG_PACKED_SPIKES = {513: 256, 300: 255}


@functools.lru_cache(maxsize=None)
def big_packed_batch(kind):
    seqs = [_big_sequence(kind, ln, 2, 5000 + ln, BIG_PACKED_SPIKES[ln]) for ln in BIG_PACKED]
    return packed_batch(f"bigpacked-{kind}", BIG_PACKED, 2, 0, qkv=torch.cat(seqs))


def spike_of(batch, n):
    """the spike position of sequence n of a spike batch"""
    if batch.name.startswith("bigpacked"):
        return BIG_PACKED_SPIKES[batch.spans[n][1]]
    return spike_positions(batch.spans[n][1])[n]
