"""The two attention kernels (csrc/encoder.hip: attention_mfma_kernel, attention_x3_kernel) called through the C ABI on buffers the
tests own: packed launches row by row (A), dense launches with the masks production builds and masks on the 256-key block edges (B),
a sequence with no live key (C), logits of checkpoint size through the online softmax (D).

Cases, references and bounds: tests/attention_cases.py (conditions checked on the CPU by tests/test_attention_cases_cpu.py).
Nothing is tuned against the kernels: ref is float64 torch, e32 the error of the same formula in float32 torch on the CPU;
fp32 kernel |out - ref| <= 4 e32, split-bf16 kernel |out - ref_x3| <= 4 e32 + 2^-16 max |v| with ref_x3's logits from the restated
split.  On N(0, 1) inputs the project's flat bars (1e-5, causal 2e-5, split-bf16 5e-5 against ref) hold as well.  Pair outputs
are the split of the fp32 output of the same launch, bit for bit.  Every test prints its measured error next to its bound."""
import pytest
import torch

from tests import attention_cases as A

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -4   # include/meerqat_hip.h
SENTINEL = -1                   # every bit set: a NaN as float32 and as bfloat16, which no kernel output is


def _lib():
    from viquae_amd import _lib
    return _lib, _lib.load()


def _stream(t):
    from viquae_amd.encoders import _stream
    return _stream(t)


class Buffers:
    """fp32 output [T, H] and pair output (PAIR LAYOUT over [T, H], rows padded to 256), every word preset to SENTINEL"""

    def __init__(self, T, H):
        from viquae_amd.encoders import SplitAct
        self.T, self.H = T, H
        self.out = torch.full((T, H), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
        self.sp = SplitAct.empty(T, H, "cuda")
        self.sp.hi.fill_(SENTINEL)
        self.sp.lo.fill_(SENTINEL)

    def bits(self):
        return self.out.view(torch.int32)

    def same_bits(self, other):
        return (torch.equal(self.bits(), other.bits()) and torch.equal(self.sp.hi, other.sp.hi)
                and torch.equal(self.sp.lo, other.sp.lo))


def _pair_of(x):
    hi, lo = A.split_pair(x)
    return hi.view(torch.int16), lo.view(torch.int16)


def _expect_pair(buf, owned_rows):
    """the pair arrays a launch must leave: the split of the fp32 output on the rows it owns, SENTINEL on every other word (the rows
    of other sequences and the padding rows of the layout)"""
    from viquae_amd.encoders import _tile
    Mp = (buf.T + 255) // 256 * 256
    hi = torch.full((Mp, buf.H), SENTINEL, dtype=torch.int16, device="cuda")
    lo = hi.clone()
    h, l = _pair_of(buf.out[owned_rows])
    hi[owned_rows], lo[owned_rows] = h, l
    return _tile(hi), _tile(lo)


def dense(qkv, mask, B, L, heads, causal, x3, buf=None, row0=0):
    """mq_attention_split_f32 over rows [row0, row0 + B L) of qkv: one launch with the fp32 output, one with the pair output"""
    lib_mod, lib = _lib()
    H = heads * A.DH
    buf = buf or Buffers(B * L, H)
    q = qkv.data_ptr() + row0 * 3 * H * 4
    m = mask.data_ptr() if mask is not None else None
    for out, hi, lo in ((buf.out.data_ptr(), None, None), (None, buf.sp.hi.data_ptr(), buf.sp.lo.data_ptr())):
        lib_mod.check(lib.mq_attention_split_f32(q, m, out, hi, lo, B, L, heads, A.DH, A.SCALE, int(causal), int(x3), _stream(qkv)),
                      "mq_attention_split_f32")
    return buf


def packed(qkv, cu, ids, max_len, heads, causal, x3, buf):
    """mq_attention_packed_f32 of the sequences `ids`: one launch with the fp32 output, one with the pair output"""
    lib_mod, lib = _lib()
    for out, hi, lo in ((buf.out.data_ptr(), None, None), (None, buf.sp.hi.data_ptr(), buf.sp.lo.data_ptr())):
        lib_mod.check(lib.mq_attention_packed_f32(qkv.data_ptr(), cu.data_ptr(), ids.data_ptr(), ids.numel(), int(max_len), out, hi, lo,
                                                  heads, A.DH, A.SCALE, int(causal), int(x3), _stream(qkv)), "mq_attention_packed_f32")
    return buf


def _rows(batch, seqs):
    return torch.cat([torch.arange(batch.spans[n][0], batch.spans[n][0] + batch.spans[n][1]) for n in seqs]).cuda()


def _within(label, out, rows, r, causal, x3, unit_variance):
    """tolerance assertions on the rows `rows` of the fp32 output `out`; returns err / bound"""
    got = out[rows].double().cpu()
    rows = rows.cpu()
    assert torch.isfinite(got).all(), f"{label}: non-finite output"
    want, bound = (r.ref_x3[rows], r.bound_x3) if x3 else (r.ref[rows], r.bound_f32)
    err, flat = float((got - want).abs().max()), float((got - r.ref[rows]).abs().max())
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print(f"attention {label} causal={int(causal)} x3={int(x3)}: max err {err:.3e} against {'ref_x3' if x3 else 'ref'}; bound {bound:.3e} "
          f"(fp32 torch-CPU err {r.e32:.3e}); ratio {ratio:.3f}; against ref {flat:.3e}")
    assert err <= bound, f"{label}: {err:.3e} > {bound:.3e}"
    if unit_variance:
        assert flat < (5e-5 if x3 else 2e-5 if causal else 1e-5), f"{label}: {flat:.3e} misses the project's flat bar"
    return ratio


def _pair_is_split_of_out(buf, rows):
    hi, lo = _expect_pair(buf, rows)
    return torch.equal(buf.sp.hi, hi) and torch.equal(buf.sp.lo, lo)


# ---------------------------------------------------------------------------------------------------
def test_restated_split_equals_the_library_split_bit_for_bit():
    from viquae_amd import encoders as E
    g = torch.Generator().manual_seed(11)
    x = torch.randn(4096, generator=g) * torch.exp2(torch.randint(-20, 21, (4096,), generator=g).float())
    x[:8] = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -17, 3.0e38, 1e-30])
    hi, lo = E.split_bf16(x.cuda())
    wh, wl = _pair_of(x)
    assert torch.equal(hi.cpu(), wh) and torch.equal(lo.cpu(), wl)


# ---------------------------------------------------------------------------------------------------
# A. packed launches
# ---------------------------------------------------------------------------------------------------
def _packed_inputs(case):
    batch = A.packed_case_batch(case.name)
    cu = torch.tensor([r0 for r0, _ in batch.spans] + [batch.qkv.shape[0]], dtype=torch.int32, device="cuda")
    return batch, batch.qkv.cuda(), cu


def _check_packed_launch(label, batch, qkv, cu, seqs, max_len, causal, x3, buf, owned_before=()):
    """one launch over the sequences `seqs` into `buf` (whose rows of `owned_before` earlier launches wrote)"""
    H = batch.heads * A.DH
    ids = torch.tensor(seqs, dtype=torch.int32, device="cuda")
    before = buf.bits().clone()
    packed(qkv, cu, ids, max_len, batch.heads, causal, x3, buf)
    rows, owned = _rows(batch, seqs), _rows(batch, list(owned_before) + list(seqs))
    # 1. every row of every launched sequence against the float64 references
    ratio = _within(label, buf.out, rows, A.refs(batch, causal), causal, x3, unit_variance=True)
    # 2. ... and bit-identical to a dense launch of that sequence alone
    for n in seqs:
        r0, ln = batch.spans[n]
        alone = dense(qkv, None, 1, ln, batch.heads, causal, x3, row0=r0)
        assert torch.equal(buf.bits()[r0:r0 + ln], alone.bits()), f"{label}: sequence {n} ({ln} tokens) differs from its dense launch"
        assert _pair_is_split_of_out(alone, torch.arange(ln, device="cuda"))
    # 3. nothing else is written: fp32 rows of other sequences keep their words, the pair arrays are the split of the owned rows
    #    and SENTINEL everywhere else
    other = torch.ones(buf.T, dtype=torch.bool, device="cuda")
    other[rows] = False
    assert torch.equal(buf.bits()[other], before[other]), f"{label}: wrote rows of a sequence outside seq_ids"
    not_owned = torch.ones(buf.T, dtype=torch.bool, device="cuda")
    not_owned[owned] = False
    assert bool((buf.bits()[not_owned] == SENTINEL).all())
    assert _pair_is_split_of_out(buf, owned), f"{label}: pair output is not the split of the fp32 output / wrote outside the launch"
    # 4. the order of seq_ids changes no bit
    if len(seqs) > 1 and not owned_before:
        again = packed(qkv, cu, torch.tensor(seqs[::-1], dtype=torch.int32, device="cuda"), max_len, batch.heads, causal, x3,
                       Buffers(buf.T, H))
        assert buf.same_bits(again), f"{label}: permuting seq_ids changed the output"
    return ratio


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("name,launch", A.PACKED_LAUNCHES)
def test_packed_launch_rows_bits_and_untouched_neighbours(name, launch, causal, x3):
    case = A.packed_case(name)
    batch, qkv, cu = _packed_inputs(case)
    launched, max_len = case.launches[launch]
    buf = Buffers(qkv.shape[0], batch.heads * A.DH)
    _check_packed_launch(f"A packed {name} max_len={max_len}", batch, qkv, cu, A.seq_ids_of(case, launched), max_len, causal, x3, buf)


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("causal", [0, 1])
def test_packed_launches_of_the_production_planner_fill_the_matrix_class_by_class(causal, x3):
    import numpy as np
    from viquae_amd import encoders as E
    batch, qkv, cu = _packed_inputs(A.MIXED)
    plan = E.pack_plan_from_lengths(np.array(A.MIXED.lengths), A.MIXED_L, "cuda")
    assert plan is not None and torch.equal(plan[2], cu) and len(plan[3]) == 4
    buf, done = Buffers(qkv.shape[0], batch.heads * A.DH), []
    for ids, max_len in plan[3]:
        seqs = ids.tolist()
        _check_packed_launch(f"A packed mixed max_len={max_len}", batch, qkv, cu, seqs, max_len, causal, x3, buf, owned_before=done)
        done += seqs
    assert sorted(done) == list(range(len(A.MIXED.lengths))) and not bool((buf.bits() == SENTINEL).any())


def test_packed_argument_checks():
    _, lib = _lib()
    case = A.packed_case("upto64")
    batch, qkv, cu = _packed_inputs(case)
    ids = torch.tensor([1, 5], dtype=torch.int32, device="cuda")
    buf = Buffers(qkv.shape[0], batch.heads * A.DH)
    q, c, i, o, h, l = qkv.data_ptr(), cu.data_ptr(), ids.data_ptr(), buf.out.data_ptr(), buf.sp.hi.data_ptr(), buf.sp.lo.data_ptr()

    def call(q=q, c=c, i=i, n=2, ml=2, o=o, h=h, l=l, heads=2, dh=64, x3=0):
        return lib.mq_attention_packed_f32(q, c, i, n, ml, o, h, l, heads, dh, A.SCALE, 0, x3, None)
    assert call(n=0) == 0 and call(ml=0) == 0
    for x3 in (0, 1):
        assert call(q=None, x3=x3) == EINVAL and call(c=None, x3=x3) == EINVAL and call(i=None, x3=x3) == EINVAL
        assert call(o=None, h=None, l=None, x3=x3) == EINVAL
        assert call(l=None, x3=x3) == EINVAL and call(h=None, x3=x3) == EINVAL      # half a pair
        assert call(heads=0, x3=x3) == EINVAL and call(heads=-2, x3=x3) == EINVAL and call(n=-1, x3=x3) == EINVAL
        assert call(dh=32, x3=x3) == EUNSUPPORTED and call(dh=128, x3=x3) == EUNSUPPORTED
    assert call(q=q + 4, x3=1) == EINVAL                                           # 16-byte query loads
    torch.cuda.synchronize()
    fresh = Buffers(qkv.shape[0], batch.heads * A.DH)
    assert buf.same_bits(fresh), "a refused or empty launch wrote to its outputs"


# ---------------------------------------------------------------------------------------------------
# B. dense launches: ECA's holes, dead tiles, the 255 / 256 block edge
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("L,causal,nonbinary", A.MASK_CASES)
def test_dense_masks_with_holes_dead_tiles_and_block_edges(L, causal, nonbinary, x3):
    batch = A.mask_batch(L, causal, nonbinary)
    B = len(batch.spans)
    qkv, mask = batch.qkv.cuda(), torch.stack(batch.masks).cuda()
    buf = dense(qkv, mask, B, L, batch.heads, causal, x3)
    names = ",".join(r.name for r in A.mask_rows(L, causal, nonbinary))
    _within(f"B masks L={L} [{names}]", buf.out, torch.arange(B * L, device="cuda"), A.refs(batch, causal), causal, x3, unit_variance=True)
    assert _pair_is_split_of_out(buf, torch.arange(B * L, device="cuda"))
    if nonbinary:   # only mask != 0 counts
        ones = dense(qkv, (mask != 0).to(torch.int64), B, L, batch.heads, causal, x3)
        assert buf.same_bits(ones)


# ---------------------------------------------------------------------------------------------------
# C. a sequence with no live key attends uniformly to its L keys
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("L", list(A.EMPTY_L))
def test_sequence_without_a_live_key_attends_uniformly(L, x3):
    """Without attention_no_live_key (csrc/encoder.hip) both kernels compute den = 0, inv = inf and 0 * inf = NaN for every element
    of that sequence; with it the sequence's context rows are the mean of its value rows."""
    batch, filled = A.empty_batch(L), A.empty_batch(L, filled=True)
    qkv = batch.qkv.cuda()
    buf = dense(qkv, torch.stack(batch.masks).cuda(), 3, L, batch.heads, 0, x3)
    empty = torch.arange(A.EMPTY_ROW * L, (A.EMPTY_ROW + 1) * L, device="cuda")
    nans = int(torch.isnan(buf.out[empty]).sum())
    print(f"attention C empty L={L} x3={x3}: {nans} NaN of {empty.numel() * buf.H} elements in the sequence without a live key")
    _within(f"C empty L={L} (all rows)", buf.out, torch.arange(3 * L, device="cuda"), A.refs(batch), 0, x3, unit_variance=True)
    _within(f"C empty L={L} (the empty sequence)", buf.out, empty, A.refs(batch), 0, x3, unit_variance=True)
    assert _pair_is_split_of_out(buf, torch.arange(3 * L, device="cuda"))
    # nothing leaks between sequences: the neighbours have the bits of the same batch with that mask row all ones
    ref = dense(qkv, torch.stack(filled.masks).cuda(), 3, L, batch.heads, 0, x3)
    others = torch.cat([torch.arange(0, L), torch.arange(2 * L, 3 * L)]).cuda()
    assert torch.equal(buf.bits()[others], ref.bits()[others])
    hi, lo = buf.sp.rowmajor()
    rhi, rlo = ref.sp.rowmajor()
    assert torch.equal(hi[others], rhi[others]) and torch.equal(lo[others], rlo[others])


# ---------------------------------------------------------------------------------------------------
# D. logits of checkpoint size: the online softmax over key blocks
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("L", list(A.BIG_L))
@pytest.mark.parametrize("kind", A.BIG_KINDS)
def test_dense_attention_at_checkpoint_sized_logits(kind, L, x3):
    batch = A.big_batch(kind, L)
    B = len(batch.spans)
    buf = dense(batch.qkv.cuda(), None, B, L, batch.heads, 0, x3)
    _within(f"D {kind} L={L}", buf.out, torch.arange(B * L, device="cuda"), A.refs(batch), 0, x3, unit_variance=False)
    assert _pair_is_split_of_out(buf, torch.arange(B * L, device="cuda"))


@pytest.mark.parametrize("x3", [0, 1])
@pytest.mark.parametrize("kind", A.BIG_KINDS)
def test_packed_attention_at_checkpoint_sized_logits(kind, x3):
    batch = A.big_packed_batch(kind)
    qkv = batch.qkv.cuda()
    cu = torch.tensor([0, A.BIG_PACKED[0], sum(A.BIG_PACKED)], dtype=torch.int32, device="cuda")
    buf = packed(qkv, cu, torch.tensor([1, 0], dtype=torch.int32, device="cuda"), max(A.BIG_PACKED), batch.heads, 0, x3,
                 Buffers(qkv.shape[0], batch.heads * A.DH))
    rows = torch.arange(qkv.shape[0], device="cuda")
    _within(f"D packed {kind} {A.BIG_PACKED}", buf.out, rows, A.refs(batch), 0, x3, unit_variance=False)
    assert _pair_is_split_of_out(buf, rows)
