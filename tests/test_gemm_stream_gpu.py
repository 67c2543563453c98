"""The persistent tile stream of the split-bf16 GEMMs (csrc/gemm_x3w.inc, gemm_nt_x3s_kernel) and the batches production runs.

gemm_x3s_launch starts at most CU-count (rounded down to 8) workgroups; a product with more 256 x 256 tile slots is walked as
a stream of tiles per workgroup: the LDS-DMA cursor runs two K steps ahead across tile boundaries, one tile's C stores overlap
the next tile's MFMAs, padded slots are skipped inside the stream.  Output (m, n) depends only on row m of A and row n of W,
with the same products in the same order whatever the launch, so

* operator level: a launch that streams == the same rows computed in launches of 8 row blocks (one tile per workgroup), word
  for word, every element; and == fp64 within the project's GEMM bound 3e-5 * max(|a| @ |w|^T);
* workgroup counts: MQ_GEMM_WGS = 8, 16, 0 in child processes == the default count in this process, word for word;
* model level: an item's vector is the same bits alone and inside a production-size batch (DPR dense and packed, CLIP vision
  and text, the reader), and within TOL = 1e-3 of the Hugging Face goldens.

Shapes and slot arithmetic: tests/gemm_stream_shapes.py (its conditions are checked without a GPU by
tests/test_gemm_stream_shapes_cpu.py and again here against the device's CU count)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import gemm_stream_shapes as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-3  # north_star: "encoder outputs must match the reference within 1e-3 fp32"


def _limit():
    return S.limit_of(torch.cuda.get_device_properties(0).multi_processor_count)


def _assert_streams(M, N):
    """the conditions of a stream test: the big launch streams, a group of 8 row blocks does not"""
    limit = _limit()
    ntm, ntn = (M + 255) // 256, (N + 255) // 256
    slots = ((ntm + 7) & ~7) * ntn
    assert slots > limit, f"[{M}, {N}]: {slots} tile slots do not exceed the {limit} persistent workgroups: nothing streams"
    assert 8 * ntn <= limit, f"[{M}, {N}]: a group of 8 row blocks has {8 * ntn} slots > {limit}: the oracle would stream too"


def _no_sentinel(ws):
    """no output word of rows < M is still the 0xFF.. it was allocated with (never a finite result: fp32 / bf16 NaN patterns)"""
    return all(not bool((t == -1).any()) for t in ws)


def _same_words(xs, ys):
    return len(xs) == len(ys) and all(x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y) for x, y in zip(xs, ys))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------
# 1. operator level
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.stream_cases(), ids=S.case_id)
def test_stream_is_bit_identical_to_one_tile_per_workgroup_launches(hip_lib, case):
    """Oracle A.  Three launches of the streaming product into sentinel-filled outputs: identical words, no sentinel left;
    and every element equals the same call on each group of 8 row blocks alone."""
    from tests import gemm_stream_child as C
    from viquae_amd import _lib
    s, v, wide = case
    _assert_streams(s.M, s.N)
    ops = C.operands(s.M, s.N, s.K, v, s.M * 7 + s.N * 3 + s.K)
    with _lib.gemm_option(_lib.GEMM_OPT_WIDE, wide):
        first = None
        for rep in range(3):
            c = C.launch(ops, v, sentinel=True)
            torch.cuda.synchronize()
            ws = C.words(c)    # every launch has a fresh output
            del c
            assert _no_sentinel(ws), f"launch {rep}: an output element was never written"
            if first is None:
                first = ws
            else:
                assert _same_words(ws, first), f"launch {rep} differs from launch 0"
            del ws
        for lo in range(0, s.M, S.GROUP_ROWS):
            hi = min(lo + S.GROUP_ROWS, s.M)
            g = C.words(C.launch(ops, v, lo, hi, sentinel=True))
            assert _same_words(g, tuple(t[lo:hi] for t in first)), f"rows [{lo}, {hi}) differ from their one-tile-per-workgroup launch"


def _fp64_check(out, ops, M, chunk=16384):
    """out [M, N] fp32 against a.double() @ w.double().T + b within 3e-5 * max(|a| @ |w|^T), in row chunks to bound memory;
    prints and returns (err, scale)"""
    w64, b64 = ops.w_f32.double(), ops.bias.double() if ops.bias is not None else None
    wabs = w64.abs()
    err = scale = 0.0
    for lo in range(0, M, chunk):
        a64 = ops.a_f32[lo:lo + chunk].double()
        ref = a64 @ w64.T
        if b64 is not None:
            ref += b64
        err = max(err, (out[lo:lo + chunk].double() - ref).abs().max().item())
        scale = max(scale, (a64.abs() @ wabs.T).max().item())
    return err, scale


@pytest.mark.parametrize("shape", S.STREAM_SHAPES, ids=S.shape_id)
def test_stream_against_fp64(hip_lib, shape):
    """Oracle B: what a sliced launch would share with the big one.  EPI_BIAS, fp32 output, every element."""
    from tests import gemm_stream_child as C
    from viquae_amd import _lib
    _assert_streams(shape.M, shape.N)
    v = S.BIAS_F32
    ops = C.operands(shape.M, shape.N, shape.K, v, shape.M * 7 + shape.N * 3 + shape.K)
    for wide in shape.wides:
        with _lib.gemm_option(_lib.GEMM_OPT_WIDE, wide):
            out = C.launch(ops, v, sentinel=True)
        err, scale = _fp64_check(out, ops, shape.M)
        print(f"{S.shape_id(shape)} wide={wide}: max |HIP - fp64| = {err:.3e}, bound {3e-5 * scale:.3e}")
        assert err < 3e-5 * scale, (err, scale)


@pytest.mark.parametrize("v", [S.BIAS_F32, S.Variant(S.EPI_BIAS_GELU, None, True, True)], ids=S.variant_id)
def test_stagger_does_not_change_a_bit(hip_lib, v):
    """MQ_GEMM_OPT_STAGGER delays the workgroups' starts: another interleaving of the streams, the same words."""
    from tests import gemm_stream_child as C
    from viquae_amd import _lib
    M, N, K = S.STAGGER_SHAPE
    _assert_streams(M, N)
    assert ((M + 255) // 256 + 7) // 8 * 8 * ((N + 255) // 256) >= 4 * _limit()   # a "many times" shape
    ops = C.operands(M, N, K, v, 99)
    before = hip_lib.mq_gemm_set_option(_lib.GEMM_OPT_STAGGER, 0)
    hip_lib.mq_gemm_set_option(_lib.GEMM_OPT_STAGGER, before)
    outs = []
    for stagger in (0, 1, 16):
        with _lib.gemm_option(_lib.GEMM_OPT_STAGGER, stagger):
            c = C.launch(ops, v, sentinel=True)
            torch.cuda.synchronize()
        outs.append(C.words(c))
        assert _no_sentinel(outs[-1])
    assert _same_words(outs[1], outs[0]) and _same_words(outs[2], outs[0])
    assert hip_lib.mq_gemm_set_option(_lib.GEMM_OPT_STAGGER, before) == before   # the blocks restored it


def _splitk(hip_lib, a, ws, bias, M, N, K, tiled, nsplit):
    from viquae_amd import _lib
    from viquae_amd.encoders import _stream
    out = torch.full((M, N), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    part = torch.empty((nsplit, M, N), dtype=torch.float32, device="cuda")
    _lib.check(hip_lib.mq_gemm_nt_bf16x3s_splitk_f32(a.hi.data_ptr(), a.lo.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(), bias.data_ptr(),
                                                     out.data_ptr(), M, N, K, int(tiled), nsplit, part.data_ptr(), _stream(out)),
               "mq_gemm_nt_bf16x3s_splitk_f32")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("nsplit", S.SPLITK_NSPLIT)
@pytest.mark.parametrize("M,N,K", S.SPLITK_SHAPES)
def test_split_k_stream(hip_lib, M, N, K, nsplit, wide):
    """mq_gemm_nt_bf16x3s_splitk_f32 on a product that streams (the ArcFace head never does; the ABI allows it): every split walks
    its K range per tile of the stream.  The per-split sum order does not depend on the launch: == the same call on groups of 8
    row blocks, word for word; and fp64 at the GEMM bound."""
    from tests import gemm_stream_child as C
    from viquae_amd import _lib
    _assert_streams(M, N)
    nk = K // 32
    per = -(-nk // nsplit)
    assert -(-nk // per) == nsplit   # the library keeps this split count (no empty split)
    ops = C.operands(M, N, K, S.BIAS_F32, M + N + K + nsplit)
    with _lib.gemm_option(_lib.GEMM_OPT_WIDE, wide):
        big = _splitk(hip_lib, ops.a, ops.w, ops.bias, M, N, K, True, nsplit)
        assert _no_sentinel((big.view(torch.int32),))
        for lo in range(0, M, S.GROUP_ROWS):
            hi = min(lo + S.GROUP_ROWS, M)
            g = _splitk(hip_lib, C.slice_rows(ops.a, lo, hi), ops.w, ops.bias, hi - lo, N, K, True, nsplit)
            assert torch.equal(g.view(torch.int32), big[lo:hi].view(torch.int32)), f"rows [{lo}, {hi})"
    err, scale = _fp64_check(big, ops, M)
    print(f"split-K {M}x{N}x{K} / {nsplit} wide={wide}: max |HIP - fp64| = {err:.3e}, bound {3e-5 * scale:.3e}")
    assert err < 3e-5 * scale, (err, scale)


# ---------------------------------------------------------------------------------------------------
# 2. other workgroup counts, each in a fresh child process (MQ_GEMM_WGS is read once per process)
# ---------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_workgroup_count(hip_lib, tmp_path):
    """MQ_GEMM_WGS = 8 (each workgroup walks 4 to 36 tile slots of these shapes), 16 and 0 (one workgroup per slot) against the
    default count in this process: identical words; and 8 workgroups once more with the sixteen-wave kernel (MQ_GEMM_WIDE=0).
    One child at a time, each under its own time limit."""
    from tests import gemm_stream_child as C
    from viquae_amd import _lib
    assert "MQ_GEMM_WGS" not in os.environ, "this process must run at the default workgroup count"
    for M, N, K, _ in S.CHILD_CASES:
        assert 4 <= S.slots(M, N) // 8 <= 36
    here = {}
    for wide in (1, 0):
        with _lib.gemm_option(_lib.GEMM_OPT_WIDE, wide):
            here[wide] = C.child_outputs()
        assert len(here[wide]) == sum(2 if v.osp else 1 for *_, v in S.CHILD_CASES)
        for name, arr in here[wide].items():
            assert not (arr == -1).any(), name
    for wgs, wide in [(wgs, 1) for wgs in S.CHILD_WGS] + [(8, 0)]:
        out_dir = tmp_path / f"wgs{wgs}_wide{wide}"
        out_dir.mkdir()
        env = dict(os.environ, MQ_GEMM_WGS=str(wgs), MQ_GEMM_WIDE=str(wide), PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        res = subprocess.run([sys.executable, "-m", "tests.gemm_stream_child", str(out_dir)], cwd=ROOT, env=env,
                             capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, (wgs, wide, res.stderr[-3000:])
        z = np.load(out_dir / "outputs.npz")
        assert str(z["wgs"]) == str(wgs)
        assert sorted(k for k in z.files if k != "wgs") == sorted(here[wide])
        for name, arr in here[wide].items():
            got = z[name]
            assert got.dtype == arr.dtype and got.shape == arr.shape and np.array_equal(got, arr), (wgs, wide, name)


# ---------------------------------------------------------------------------------------------------
# 3. model level: a vector does not depend on its batch
# ---------------------------------------------------------------------------------------------------
def _spy(monkeypatch, obj, name, calls):
    real = getattr(obj, name)
    monkeypatch.setattr(obj, name, lambda *a, **k: (calls.append(name), real(*a, **k))[1])


def _dpr_base(seed):
    from oracle import encoders as oe
    from viquae_amd.encoders import DPRContextEncoder
    cfg = oe.BERT_BASE
    state = oe.seeded_state(oe.bert_param_shapes(cfg), seed)
    return cfg, DPRContextEncoder.from_state_dict(cfg, state).to("cuda").eval()


def _golden_positions(rng, B, avoid=()):
    """positions 0, 1, 255, 256, 1023, 2046, 2047 and one seeded position of a batch of 2048"""
    fixed = [0, 1, 255, 256, 1023, 2046, 2047]
    while True:
        p = int(rng.integers(2, B - 2))
        if p not in fixed and p not in avoid:
            return np.array(fixed + [p])


@pytest.mark.parametrize("gemm", ["split_bf16", "f32"])
def test_dpr_vector_is_the_same_alone_and_inside_the_benchmarked_batch(hip_lib, gemm, monkeypatch):
    """bert-base, the 8 golden passages (100 tokens) inside 2048 x 100 seeded passages: the DENSE forward over 204,800 rows
    (800 row blocks; row blocks cut across passages; 2,400 to 9,600 tiles per GEMM).  pooler_output at their positions ==
    the forward of the 8 alone, bit for bit, and within TOL of Hugging Face."""
    from viquae_amd import encoders
    monkeypatch.setenv("MQ_ENC_GEMM", gemm)
    z = np.load(os.path.join(GOLDEN, "dpr_base_8x100.npz"))
    cfg, model = _dpr_base(int(z["seed"]))
    B, L = 2048, 100
    rng = np.random.default_rng(2048)
    at = _golden_positions(rng, B)
    ids = rng.integers(1000, cfg["vocab_size"], (B, L)).astype(np.int64)
    mask = np.ones((B, L), np.int64)                      # full-length fillers: < 10 % padding, the pack plan declines
    ids[at], mask[at] = z["input_ids"], z["attention_mask"]
    assert encoders._pack_plan(_cuda(mask)) is None and encoders._pack_plan(_cuda(z["attention_mask"])) is None
    calls = []
    _spy(monkeypatch, model.bert_model, "_layers", calls)
    _spy(monkeypatch, model.bert_model, "packed_layers", calls)
    alone = model(input_ids=_cuda(z["input_ids"]), attention_mask=_cuda(z["attention_mask"]))["pooler_output"]
    big = model(input_ids=_cuda(ids), attention_mask=_cuda(mask))["pooler_output"]
    assert calls == ["_layers", "_layers"], "both forwards must be the dense one"
    assert big.shape == (B, cfg["hidden_size"])
    if gemm == "split_bf16":
        _assert_streams(B * L, 3 * cfg["hidden_size"])
    err = np.abs(alone.cpu().numpy() - z["pooler_output"]).max()
    print(f"DPR 8 alone [{gemm}]: max |HIP - HF| = {err:.3e}")
    assert err < TOL
    assert np.abs(big[_cuda(at)].cpu().numpy() - z["pooler_output"]).max() < TOL
    assert torch.equal(big[_cuda(at)].view(torch.int32), alone.view(torch.int32))


def test_dpr_packed_forward_at_the_benchmarked_batch(hip_lib, monkeypatch):
    """2048 passages padded to 256 with real lengths drawn like _padded_batch (and lengths 1 and 2): the PACKED forward.  The 8
    golden passages inside it == the 8 alone (padded to 256), bit for bit; the length-1 and length-2 passages == their dense
    forward in a small batch."""
    from viquae_amd import encoders
    z = np.load(os.path.join(GOLDEN, "dpr_base_8x100.npz"))
    cfg, model = _dpr_base(int(z["seed"]))
    B, L = 2048, 256
    rng = np.random.default_rng(256)
    short = np.array([4, 5, 700, 1500, 2044, 2045])
    at = _golden_positions(rng, B, avoid=(2, 3, 6) + tuple(short))
    lens = np.clip(rng.normal(0.5 * L, 0.15 * L, B).astype(int), 3, L)
    lens[2], lens[3] = L, 3                         # the longest and _padded_batch's shortest, and below it:
    lens[[4, 700, 2045]] = 1                        # length 1
    lens[[5, 1500, 2044]] = 2                       # length 2
    ids = rng.integers(1000, cfg["vocab_size"], (B, L)).astype(np.int64)
    g_ids = np.zeros((8, L), np.int64)
    g_mask = np.zeros((8, L), np.int64)
    g_ids[:, :100], g_mask[:, :100] = z["input_ids"], z["attention_mask"]
    lens[at] = g_mask.sum(1)
    ids[at] = g_ids
    mask = (np.arange(L)[None] < lens[:, None]).astype(np.int64)
    ids[mask == 0] = 0
    assert (mask[at] == g_mask).all()
    calls = []
    _spy(monkeypatch, model.bert_model, "_layers", calls)
    _spy(monkeypatch, model.bert_model, "packed_layers", calls)
    big = model(input_ids=_cuda(ids), attention_mask=_cuda(mask))["pooler_output"]
    alone = model(input_ids=_cuda(g_ids), attention_mask=_cuda(g_mask))["pooler_output"]
    assert calls == ["packed_layers", "packed_layers"], "both forwards must be the packed one"
    _assert_streams(int(lens.sum()), 3 * cfg["hidden_size"])
    assert torch.equal(big[_cuda(at)].view(torch.int32), alone.view(torch.int32))
    assert np.abs(alone.cpu().numpy() - z["pooler_output"]).max() < TOL
    # lengths 1 and 2: the dense forward of a small batch (the six short passages and two long neighbours)
    small = np.concatenate([short, [2, 6]])
    monkeypatch.setattr(encoders, "_pack_plan", lambda m: None)
    dense = model(input_ids=_cuda(ids[small]), attention_mask=_cuda(mask[small]))["pooler_output"]
    assert calls[2:] == ["_layers"]
    assert sorted(lens[short]) == [1, 1, 1, 2, 2, 2]
    assert torch.isfinite(dense).all()
    assert torch.equal(big[_cuda(small)].view(torch.int32), dense.view(torch.int32))


def test_clip_vision_vector_is_the_same_alone_and_inside_1024_images(hip_lib):
    """ViT-B/32: the 4 golden images inside a seeded batch of 1024 (51,200 token rows: 1,800 QKV tiles)."""
    from oracle import encoders as oe
    from viquae_amd.encoders import CLIPModel
    z = np.load(os.path.join(GOLDEN, "clip_vitb32_4.npz"))
    cfg = oe.CLIP_VITB32
    state = oe.seeded_state(oe.clip_vision_param_shapes(cfg), int(z["seed"]))
    model = CLIPModel.from_state_dict({"vision_config": cfg}, state).to("cuda").eval()
    B = 1024
    rng = np.random.default_rng(1024)
    at = np.array([0, 511, 1023, int(rng.integers(1, 511))])
    g = torch.Generator(device="cuda").manual_seed(1024)
    px = torch.randn((B,) + z["pixel_values"].shape[1:], generator=g, device="cuda")
    golden_px = _cuda(z["pixel_values"].astype(np.float32))
    px[_cuda(at)] = golden_px
    tokens = (cfg["image_size"] // cfg["patch_size"]) ** 2 + 1
    _assert_streams(B * tokens, 3 * cfg["hidden_size"])
    alone = model.get_image_features(pixel_values=golden_px)
    big = model.get_image_features(pixel_values=px)
    assert big.shape == (B, z["image_features"].shape[1])
    err = np.abs(alone.cpu().numpy() - z["image_features"]).max()
    print(f"CLIP vision 4 alone: max |HIP - HF| = {err:.3e}")
    assert err < TOL
    assert np.abs(big[_cuda(at)].cpu().numpy() - z["image_features"]).max() < TOL
    assert torch.equal(big[_cuda(at)].view(torch.int32), alone.view(torch.int32))


def test_clip_text_vector_is_the_same_alone_and_inside_2048_titles(hip_lib, monkeypatch):
    """ViT-B/32's text tower: the 4 golden titles inside 2048 seeded titles padded to 77 (the packed forward, the default)."""
    from oracle import encoders as oe
    from viquae_amd.encoders import CLIPModel
    z = np.load(os.path.join(GOLDEN, "clip_text_vitb32_4.npz"))
    cfg = dict(oe.CLIP_TEXT_VITB32, eos_token_id=2)
    state = oe.seeded_state(oe.clip_text_param_shapes(cfg), int(z["seed"]))
    model = CLIPModel.from_state_dict({"text_config": dict(cfg, hidden_act="quick_gelu")}, state).to("cuda").eval()
    B, L = 2048, 77
    rng = np.random.default_rng(77)
    at = np.array([0, 1023, 2047, int(rng.integers(1, 1023))])
    bos, eot = cfg["vocab_size"] - 2, cfg["vocab_size"] - 1
    lens = np.clip(rng.normal(24, 12, B).astype(int), 3, L)
    ids = rng.integers(3, cfg["vocab_size"] - 2, (B, L)).astype(np.int64)
    ids[:, 0] = bos
    for b, n in enumerate(lens):
        ids[b, n - 1:] = eot          # end of text, then padding with the same id (CLIPTokenizer's pad token)
    mask = (np.arange(L)[None] < lens[:, None]).astype(np.int64)
    ids[at], mask[at] = z["input_ids"], z["attention_mask"]
    calls = []
    _spy(monkeypatch, model, "_text_features_packed", calls)
    _spy(monkeypatch, model, "_text_features_dense", calls)
    alone = model.get_text_features(input_ids=_cuda(z["input_ids"]), attention_mask=_cuda(z["attention_mask"]))
    big = model.get_text_features(input_ids=_cuda(ids), attention_mask=_cuda(mask))
    assert calls == ["_text_features_packed", "_text_features_packed"]
    _assert_streams(int(mask.sum()), 3 * cfg["hidden_size"])
    err = np.abs(alone.cpu().numpy() - z["text_features"]).max()
    print(f"CLIP text 4 alone: max |HIP - HF| = {err:.3e}")
    assert err < TOL
    assert np.abs(big[_cuda(at)].cpu().numpy() - z["text_features"]).max() < TOL
    assert torch.equal(big[_cuda(at)].view(torch.int32), alone.view(torch.int32))


def test_reader_logits_are_the_same_192_at_a_time_and_8_at_a_time(hip_lib, monkeypatch):
    """The reader golden's 192 x 256 tokens (49,152 rows: the stream) against the same sequences run 8 at a time (2,048 rows,
    at most 96 slots: one tile per workgroup): identical logits.  The golden itself stays with test_logits_against_hf."""
    from tests import reader_restatement as rr
    from viquae_amd.encoders import MultiPassageBERT
    monkeypatch.setenv("MQ_ENC_GEMM", "split_bf16")
    golden = rr.load_golden()
    g = golden["sizes"]["base2"]
    d = np.load(os.path.join(rr.GOLDEN, "reader_base2.npz"))
    vocab = len(golden["world"]["vocab"])
    config = rr.hf_config(g["config"], vocab)
    model = MultiPassageBERT.from_state_dict(config, rr.reader_state(g["config"], vocab, g["seed"])).cuda().eval()
    for bi in range(len(g["batches"])):
        inputs = {k: torch.from_numpy(d[f"b{bi}_{k}"].astype(np.int64)).cuda() for k in ("input_ids", "token_type_ids", "attention_mask")}
        B, L = inputs["input_ids"].shape
        assert B % 8 == 0 and 8 * L == S.GROUP_ROWS
        _assert_streams(B * L, 3 * int(config["hidden_size"]))
        assert S.group_slots(int(config["intermediate_size"])) <= _limit()
        out = model(**inputs)
        for lo in range(0, B, 8):
            part = model(**{k: v[lo:lo + 8] for k, v in inputs.items()})
            for k in ("start_logits", "end_logits"):
                assert torch.equal(part[k].view(torch.int32), out[k][lo:lo + 8].contiguous().view(torch.int32)), (bi, lo, k)
