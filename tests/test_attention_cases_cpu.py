"""The conditions the attention kernel tests rely on (tests/attention_cases.py), checked by arithmetic without a GPU: every case has
the property it is listed for, every derived bound is small against the reference, and the restated split does work."""
import math

import pytest
import torch

from tests import attention_cases as A

CAP = 1e-3   # every derived bound is at most CAP * max |ref|


def _all_batches():
    out = []
    for c in A.PACKED_CASES + [A.MIXED]:
        out += [(A.packed_case_batch(c.name), causal) for causal in (False, True)]
    out += [(A.mask_batch(L, causal, nb), causal) for L, causal, nb in A.MASK_CASES]
    out += [(A.empty_batch(L), False) for L in A.EMPTY_L]
    out += [(A.big_batch(kind, L), False) for kind in A.BIG_KINDS for L in A.BIG_L]
    out += [(A.big_packed_batch(kind), False) for kind in A.BIG_KINDS]
    return out


def test_shapes_stay_inside_the_agreed_limits():
    for b, _ in _all_batches():
        assert len(b.spans) <= 8 and max(ln for _, ln in b.spans) <= 513 and b.heads in (2, 3), b.name
        assert b.qkv.dtype == torch.float32 and b.qkv.shape[1] == 3 * b.heads * A.DH
    groups = {"A": [c.heads for c in A.PACKED_CASES], "B": list(A.MASK_HEADS.values()), "C": list(A.EMPTY_L.values()),
              "D": list(A.BIG_L.values())}
    assert all(3 in h and 2 in h for h in groups.values()), groups


# ---------------------------------------------------------------------------------------------------
# A. packed launches land in the instantiations they are listed for
# ---------------------------------------------------------------------------------------------------
EXPECT = {   # (case, launch) -> fp32 / split-bf16 instantiation: (NKT, MULTI, WIDE, waves, grid y)
    ("upto64", 0): ((2, False, False, 2, 1), (2, False, False, 2, 1)),
    ("upto64", 1): ((2, False, False, 2, 1), (2, False, False, 2, 1)),
    ("upto64", 2): ((2, False, False, 1, 1), (2, False, False, 1, 1)),
    ("upto128", 0): ((4, False, False, 4, 1), (4, False, False, 4, 1)),
    ("upto128", 1): ((4, False, False, 3, 1), (4, False, False, 3, 1)),
    ("upto256", 0): ((8, False, False, 4, 2), (8, False, True, 8, 1)),
    ("upto256", 1): ((8, False, False, 4, 2), (8, False, True, 5, 1)),
    ("over256", 0): ((8, True, False, 4, 5), (8, True, False, 4, 5)),
}


def test_packed_launch_lists_take_the_listed_instantiations():
    assert set(EXPECT) == set(A.PACKED_LAUNCHES)
    for (name, i), want in EXPECT.items():
        case = A.packed_case(name)
        launched, max_len = case.launches[i]
        assert max(launched) == max_len and set(launched) <= set(case.lengths) and len(set(case.lengths)) == len(case.lengths)
        assert set(launched) < set(case.lengths), "every matrix keeps a sequence that no launch owns"
        for x3 in (0, 1):
            d = A.dispatch(max_len, x3, packed=True)
            assert (d.nkt, d.multi, d.wide, d.waves, d.grid_y) == want[x3], (name, i, x3, d)
            # every launched length belongs to the class: the same key-tile count as its own dense launch, queries covered
            for ln in launched:
                assert A.dispatch(ln, x3, packed=False).nkt == d.nkt and A.dispatch(ln, x3, packed=False).multi == d.multi
                assert d.grid_y * d.qpb >= ln
    assert case.lengths != sorted(case.lengths)


def test_packed_launches_cover_the_paths_only_the_packed_kernels_have():
    seen = set()
    for name, i in A.PACKED_LAUNCHES:
        launched, max_len = A.packed_case(name).launches[i]
        for x3 in (0, 1):
            d = A.dispatch(max_len, x3, packed=True)
            if d.waves == 1:
                seen.add("one wave")
            for ln in launched:
                if A.idle_waves(ln, d):
                    seen.add("idle waves" + (" wide" if d.wide else ""))
                if x3 and A.nt_live(ln, d) < d.nkt:
                    seen.add("nt_live < NKT" + (" wide" if d.wide else ""))
                    if A.nt_live(ln, d) % 2:
                        seen.add("nt_live odd" + (" wide" if d.wide else ""))
                if d.grid_y > 1 and A.early_returns(ln, d):
                    seen.add("early return" + (" multi" if d.multi else ""))
    assert seen >= {"one wave", "idle waves", "idle waves wide", "nt_live < NKT", "nt_live < NKT wide", "nt_live odd",
                    "nt_live odd wide", "early return multi"}, seen
    assert "early return" not in seen   # below 257 tokens a class has two blocks in y only when all its sequences have more than 128
    # the figures the issue names: 160 tokens = 5 live tiles of 8, 130 tokens leave waves 5 to 7 idle, five blocks in y for 513
    wide = A.dispatch(256, 1, True)
    assert A.nt_live(160, wide) == 5 and A.idle_waves(130, wide) == 3 and A.dispatch(513, 1, True).grid_y == 5
    assert A.early_returns(300, A.dispatch(513, 0, True)) == 2


def test_the_mixed_case_is_planned_into_all_four_classes():
    import numpy as np
    from viquae_amd import encoders as E
    plan = E.pack_plan_from_lengths(np.array(A.MIXED.lengths), A.MIXED_L, "cpu")
    assert plan is not None
    classes = [(ids.tolist(), ml) for ids, ml in plan[3]]
    assert [ml for _, ml in classes] == [64, 100, 200, 513] and sorted(i for ids, _ in classes for i in ids) == list(range(8))
    assert plan[2].tolist() == [0] + [sum(A.MIXED.lengths[:i + 1]) for i in range(8)]


# ---------------------------------------------------------------------------------------------------
# B, C. masks
# ---------------------------------------------------------------------------------------------------
def test_masks_have_the_dead_ranges_they_are_listed_for():
    for L, rows in list(A.MASK_ROWS.items()) + [(A.NONBINARY_L, A.NONBINARY_ROWS)]:
        for r in rows:
            assert r.mask.shape == (L,) and r.dead and r.live, r.name
            for lo, hi in r.dead:
                assert 0 <= lo < hi <= L and not r.mask[lo:hi].any(), (r.name, lo, hi)
            assert all(r.mask[k] != 0 for k in r.live), r.name
            assert r.mask.any(), "outside group C every sequence has a live key"
    names = {L: {r.name: r for r in rows} for L, rows in A.MASK_ROWS.items()}
    for L in (300, 513):
        assert (0, 256) in names[L]["first_block_dead"].dead                       # m_run is still -inf when block 1 arrives
        lo, hi = names[L]["later_block_dead"].dead[0]
        assert lo == 256 and hi == min(L, 512) and hi - lo >= 32                   # every key of block 1
        assert int(names[L]["only_255"].mask.sum()) == 1 and int(names[L]["only_256"].mask.sum()) == 1
        assert int((names[L]["edge_pair_dead"].mask == 0).sum()) == 2
    assert (64, 96) in names[200]["tile_64_95_dead"].dead and (0, 32) in names[200]["tile_0_31_dead"].dead
    assert int(names[200]["only_last"].mask.sum()) == 1
    for L in (261, 262):   # holes: text, padding, two faces, empty face slots, image
        for r in A.MASK_ROWS[L]:
            assert r.mask[256:].tolist() == [1, 1] + [0] * (L - 259) + [1]
    assert any(r.mask[:256].all() for r in A.MASK_ROWS[261]) and any(not r.mask[17:256].any() for r in A.MASK_ROWS[261])
    for r in A.NONBINARY_ROWS:
        assert {2, 7} <= set(r.mask.tolist()) <= {0, 1, 2, 7}
    for r, p in zip(A.NONBINARY_ROWS, A.MASK_ROWS[A.NONBINARY_L]):
        assert torch.equal(r.mask != 0, p.mask != 0)


def test_causal_runs_keep_a_live_key_at_or_before_every_query():
    some = 0
    for L, causal, nb in A.MASK_CASES:
        b = A.mask_batch(L, causal, nb)
        assert len(b.spans) == len(A.mask_rows(L, causal, nb)) >= 2
        for m in b.masks:
            live = (m != 0)
            assert live.any()
            if causal:
                assert bool((torch.cumsum(live.long(), 0) > 0).all())
                some += 1
    assert some >= 10
    for L, rows in A.MASK_ROWS.items():   # exactly the rows with a dead key 0 are left out
        assert [r.name for r in rows if not A.causal_ok(r)] == [r.name for r in rows if r.mask[0] == 0]


def test_the_empty_row_is_the_only_one_without_a_live_key():
    for L in A.EMPTY_L:
        b, f = A.empty_batch(L), A.empty_batch(L, filled=True)
        assert [bool(m.any()) for m in b.masks] == [True, False, True] and A.EMPTY_ROW == 1
        assert torch.equal(b.qkv, f.qkv) and torch.equal(b.masks[0], f.masks[0]) and torch.equal(b.masks[2], f.masks[2])
        assert bool(f.masks[1].all())
        # the reference of the empty row is the mean of its L value rows
        H = b.heads * A.DH
        r0, ln = b.spans[A.EMPTY_ROW]
        mean = b.qkv[r0:r0 + ln, 2 * H:].double().mean(0)
        assert (A.refs(b).ref[r0:r0 + ln] - mean[None]).abs().max() < 1e-14
        assert (A.refs(b).ref_x3[r0:r0 + ln] - mean[None]).abs().max() < 1e-14


# ---------------------------------------------------------------------------------------------------
# D. the online softmax is stressed the way each kind says
# ---------------------------------------------------------------------------------------------------
def _big_batches(kind):
    return [A.big_batch(kind, L) for L in A.BIG_L] + [A.big_packed_batch(kind)]


@pytest.mark.parametrize("kind,sign", [("rising", 1.0), ("falling", -1.0)])
def test_block_maxima_move_by_eight_at_every_block_boundary(kind, sign):
    boundaries = 0
    for b in _big_batches(kind):
        for n, (_, ln) in enumerate(b.spans):
            s, _ = A.probabilities(b, n)
            assert 30 < float(s.max()) < 60 and -60 < float(s.min()) < -30, (b.name, float(s.min()), float(s.max()))
            bm = torch.stack([s[:, :, k0:k0 + 256].max(-1).values for k0 in range(0, ln, 256)], -1)   # [heads, query, block]
            if bm.shape[-1] > 1:
                step = sign * (bm[..., 1:] - bm[..., :-1])
                assert float(step.min()) >= A.STEP_MIN, (b.name, float(step.min()))    # alpha (or the new block's weight) <= e^-8
                boundaries += bm.shape[-1] - 1
    assert boundaries >= 2 * (1 + 2) + (1 + 2)


def test_spike_rows_put_their_weight_on_one_key():
    places = set()
    for b in _big_batches("spike"):
        for n, (_, ln) in enumerate(b.spans):
            at = A.spike_of(b, n)
            s, p = A.probabilities(b, n)
            rest = torch.cat([s[..., :at], s[..., at + 1:]], -1)
            if ln > 1:
                assert float((s[..., at] - rest.max(-1).values).min()) >= A.SPIKE_GAP, b.name
            assert float(p.max(-1).values.min()) >= A.SPIKE_P and bool((p.argmax(-1) == at).all())
            places.add((ln, at))
    assert {(300, 0), (300, 255), (300, 256), (300, 299), (513, 0), (513, 255), (513, 256), (513, 512), (100, 99), (200, 199)} <= places


def test_wide_logits_are_wide():
    for b in _big_batches("wide"):
        s, _ = A.probabilities(b, 0)
        assert 7.0 < float(s.std()) < 11.0 and float(s.abs().max()) > 25.0


# ---------------------------------------------------------------------------------------------------
# tolerances
# ---------------------------------------------------------------------------------------------------
def test_every_derived_bound_is_small_against_the_reference():
    """e32 > 0 everywhere but on the spike batches: there every other key is e^-60 below the spike, less than half an ulp of
    float64 relative to it, so ref, the float32 evaluation and (bit for bit) the spike's value row coincide and e32 is exactly 0 --
    the fp32 kernel is then held to equality and the split-bf16 kernel to 2^-16 max |v| alone."""
    for b, causal in _all_batches():
        r = A.refs(b, causal)
        top = float(r.ref.abs().max())
        print(f"{b.name} causal={int(causal)}: e32 {r.e32:.3e} bound fp32 {r.bound_f32:.3e} x3 {r.bound_x3:.3e} max|ref| {top:.3f} "
              f"|ref_x3 - ref| {float((r.ref_x3 - r.ref).abs().max()):.3e}")
        assert torch.isfinite(r.ref).all() and torch.isfinite(r.ref_x3).all()
        if "spike" in b.name:
            assert r.e32 == 0.0
        else:
            assert r.e32 > 0.0, b.name
        assert r.bound_f32 <= CAP * top and r.bound_x3 <= CAP * top, b.name
        assert math.isclose(r.bound_x3 - r.bound_f32, 2.0 ** -16 * r.vmax, rel_tol=1e-9)


def test_the_restated_split_does_work_on_the_wide_case():
    for b in _big_batches("wide"):
        r = A.refs(b)
        assert float((r.ref_x3 - r.ref).abs().max()) > r.bound_x3, b.name


def test_restated_split_is_round_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 3.0e38, 1e-40])
    hi, lo = A.split_pair(x)
    assert hi[:4].float().tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -1.0]          # ties go to the even mantissa
    assert lo[:4].float().tolist() == [0.0, 2.0 ** -8, -(2.0 ** -8), -(2.0 ** -8)]
    y = torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 5
    hi, lo = A.split_pair(y)
    assert float((hi.float() + lo.float() - y).abs().max()) <= 2.0 ** -17 * float(y.abs().max())
