"""GPU suite of the CLIP ResNet encoder: each new kernel (csrc/clip_resnet.hip) against float64 torch on the values it reads, the
forward against the float64 golden of tests/clip_resnet_restatement.py and against the restatement on a second layout at two
resolutions, batch invariance, the device-side transform with CLIP's constants bit for bit against its restatement, and the
pipelined image job against the serial one."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import clip_resnet_restatement as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PAIR_TOL = 2e-5   # hi + lo keeps 16 mantissa bits (the ArcFace and ResNet kernel tests' figure), times max |reference|
EINVAL, EUNSUPPORTED = -1, -4


def _pair(x2d):
    """fp32 [rows, C] on the GPU -> its split pair"""
    from viquae_amd.encoders import SplitAct, split_bf16
    return SplitAct(*split_bf16(x2d.contiguous()))


def _split_bits(t):
    """fp32 tensor -> the (hi, lo) bf16 tensors of its split"""
    hi = t.bfloat16()
    return hi, (t - hi.float()).bfloat16()


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (3, 224, 224), (5, 64, 96), (2, 36, 40), (7, 2, 2), (3, 10, 14), (1, 6, 2)])
def test_stem_kernel_against_float64(B, H, W):
    """conv 3 x 3 / 2 (3 -> 32) + bias + ReLU: odd batches, output rows that are not multiples of the 4-pixel groups, 1 x 1 maps"""
    from viquae_amd import _lib
    from viquae_amd.encoders import SplitAct, _stream
    g = torch.Generator().manual_seed(B * 1000 + H)
    x = torch.randn((B, 3, H, W), generator=g)
    w = torch.randn((32, 3, 3, 3), generator=g) * 0.3
    b = torch.randn(32, generator=g) * 0.5
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)).permute(0, 2, 3, 1).reshape(-1, 32)
    xd, wt, bd = x.cuda(), w.permute(2, 3, 1, 0).reshape(27, 32).contiguous().cuda(), b.cuda()
    P = SplitAct.empty(B * (H // 2) * (W // 2), 32, xd.device)
    _lib.check(_lib.load().mq_clip_stem_conv3x3s2_f32(xd.data_ptr(), B, H, W, wt.data_ptr(), bd.data_ptr(), 32, P.hi.data_ptr(),
                                                      P.lo.data_ptr(), _stream(xd)), "stem")
    got = P.float().double().cpu()
    assert got.shape == ref.shape
    err, tol = float((got - ref).abs().max()), PAIR_TOL * float(ref.abs().max())
    print(f"clip stem {B}x{H}x{W}: max err {err:.3e} tol {tol:.3e}")
    assert err <= tol


def test_stem_argument_checks():
    from viquae_amd import _lib
    lib = _lib.load()
    z = torch.zeros(1 << 14, device="cuda")
    p = z.data_ptr()
    assert lib.mq_clip_stem_conv3x3s2_f32(p, 1, 8, 8, p, p, 32, p, p, None) == 0
    assert lib.mq_clip_stem_conv3x3s2_f32(p, 0, 8, 8, p, p, 32, p, p, None) == 0
    assert lib.mq_clip_stem_conv3x3s2_f32(p, 1, 8, 8, p, p, 64, p, p, None) == EUNSUPPORTED
    assert lib.mq_clip_stem_conv3x3s2_f32(p, 1, 7, 8, p, p, 32, p, p, None) == EUNSUPPORTED
    assert lib.mq_clip_stem_conv3x3s2_f32(p, 1, 8, 9, p, p, 32, p, p, None) == EUNSUPPORTED
    assert lib.mq_clip_stem_conv3x3s2_f32(None, 1, 8, 8, p, p, 32, p, p, None) == EINVAL
    assert lib.mq_clip_stem_conv3x3s2_f32(p, 1, 8, 8, p, p, 32, p, None, None) == EINVAL
    assert lib.mq_clip_stem_conv3x3s2_f32(p, -1, 8, 8, p, p, 32, p, p, None) == EINVAL
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 32), (3, 112, 112, 64), (5, 14, 14, 256), (2, 6, 10, 96), (7, 8, 8, 2048), (1, 56, 56, 128),
                                     (3, 28, 28, 512), (9, 2, 2, 64)])
def test_avgpool_kernel(B, H, W, C):
    """AvgPool2d(2) on a pair: bit for bit the documented fp32 order on the pair's values, and within the pair tolerance of float64;
    odd batches, row counts off the 256-row tiles, 1 x 1 outputs"""
    from viquae_amd import _lib
    from viquae_amd.encoders import SplitAct, _stream
    g = torch.Generator().manual_seed(H * 100 + C)
    X = _pair(torch.randn((B * H * W, C), generator=g).cuda() * 3)
    a = X.float().view(B, H, W, C)                                # what the kernel reads: hi + lo, exact in fp32
    P = SplitAct.empty(B * (H // 2) * (W // 2), C, a.device)
    _lib.check(_lib.load().mq_avgpool2x2_pair_f32(X.hi.data_ptr(), X.lo.data_ptr(), B, H, W, C, P.hi.data_ptr(), P.lo.data_ptr(),
                                                  _stream(a)), "mq_avgpool2x2_pair_f32")
    t = (((a[:, 0::2, 0::2] + a[:, 0::2, 1::2]) + a[:, 1::2, 0::2]) + a[:, 1::2, 1::2]) * 0.25   # the documented order, fp32
    hi, lo = _split_bits(t.reshape(-1, C))
    ghi, glo = P.rowmajor()
    assert torch.equal(ghi.view(torch.bfloat16), hi) and torch.equal(glo.view(torch.bfloat16), lo)
    ref = F.avg_pool2d(a.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(-1, C)
    err, tol = float((P.float().double() - ref).abs().max()), PAIR_TOL * float(ref.abs().max())
    print(f"avgpool {(B, H, W, C)}: max err {err:.3e} tol {tol:.3e}")
    assert err <= tol


def test_avgpool_argument_checks():
    from viquae_amd import _lib
    lib = _lib.load()
    z = torch.zeros(1 << 14, device="cuda")
    p = z.data_ptr()
    assert lib.mq_avgpool2x2_pair_f32(p, p, 1, 4, 4, 32, p, p, None) == 0 and lib.mq_avgpool2x2_pair_f32(p, p, 0, 4, 4, 32, p, p, None) == 0
    assert lib.mq_avgpool2x2_pair_f32(p, p, 1, 3, 4, 32, p, p, None) == EINVAL
    assert lib.mq_avgpool2x2_pair_f32(p, p, 1, 4, 6 + 1, 32, p, p, None) == EINVAL
    assert lib.mq_avgpool2x2_pair_f32(p, p, 1, 4, 4, 48, p, p, None) == EINVAL
    assert lib.mq_avgpool2x2_pair_f32(p, None, 1, 4, 4, 32, p, p, None) == EINVAL
    assert lib.mq_avgpool2x2_pair_f32(p, p, 1, 4, 4, 32, p + 2, p, None) == EINVAL   # 16-byte accesses
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,HW,C", [(3, 49, 2048), (1, 1, 64), (5, 4, 96), (2, 144, 256), (7, 9, 32), (300, 4, 64)])
def test_tokens_kernel(B, HW, C):
    """[mean | pixels] + positional embedding -> pair: within the pair tolerance of float64; the mean token bit for bit the
    documented order (fp32 sum over p = 0 ... HW - 1, one division, + pos[0]); the mean tokens' own pair equals those rows"""
    from viquae_amd import _lib
    from viquae_amd.encoders import SplitAct, _stream
    g = torch.Generator().manual_seed(HW * 10 + C)
    y = (torch.randn((B * HW, C), generator=g) * 2).relu().cuda()
    pos = torch.randn((HW + 1, C), generator=g).cuda()
    T = HW + 1
    tok, mean = SplitAct.empty(B * T, C, y.device), SplitAct.empty(B, C, y.device)
    _lib.check(_lib.load().mq_attnpool_tokens_f32(y.data_ptr(), B, HW, C, pos.data_ptr(), tok.hi.data_ptr(), tok.lo.data_ptr(),
                                                  mean.hi.data_ptr(), mean.lo.data_ptr(), _stream(y)), "mq_attnpool_tokens_f32")
    y3 = y.view(B, HW, C)
    ref = torch.cat([y3.double().mean(1, keepdim=True), y3.double()], dim=1) + pos.double()[None]
    got = tok.float().view(B, T, C)
    err, tol = float((got.double() - ref).abs().max()), PAIR_TOL * float(ref.abs().max())
    print(f"tokens {(B, HW, C)}: max err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    seq = y3[:, 0].clone()
    for k in range(1, HW):
        seq += y3[:, k]
    m = torch.from_numpy(seq.cpu().numpy() / np.float32(HW)).cuda() + pos[0]        # an IEEE division, on the host
    hi, lo = _split_bits(m)
    thi, tlo = tok.rowmajor()
    assert torch.equal(thi.view(B, T, C)[:, 0].view(torch.bfloat16), hi) and torch.equal(tlo.view(B, T, C)[:, 0].view(torch.bfloat16), lo)
    mhi, mlo = mean.rowmajor()
    assert torch.equal(mhi.view(torch.bfloat16), hi) and torch.equal(mlo.view(torch.bfloat16), lo)
    # the pixel rows: the split of the very fp32 sum
    hi, lo = _split_bits(y3 + pos[1:][None])
    assert torch.equal(thi.view(B, T, C)[:, 1:].view(torch.bfloat16), hi) and torch.equal(tlo.view(B, T, C)[:, 1:].view(torch.bfloat16), lo)


def test_tokens_argument_checks():
    from viquae_amd import _lib
    lib = _lib.load()
    z = torch.zeros(1 << 14, device="cuda")
    p = z.data_ptr()
    assert lib.mq_attnpool_tokens_f32(p, 1, 4, 32, p, p, p, p, p, None) == 0 and lib.mq_attnpool_tokens_f32(p, 0, 4, 32, p, p, p, p, p, None) == 0
    assert lib.mq_attnpool_tokens_f32(p, 1, 4, 40, p, p, p, p, p, None) == EINVAL
    assert lib.mq_attnpool_tokens_f32(p, 1, 0, 32, p, p, p, p, p, None) == EINVAL
    assert lib.mq_attnpool_tokens_f32(p, 1, 4, 32, None, p, p, p, p, None) == EINVAL
    assert lib.mq_attnpool_tokens_f32(p, 1, 4, 32, p, p, p, p, None, None) == EINVAL
    assert lib.mq_attnpool_tokens_f32(p + 4, 1, 4, 32, p, p, p, p, p, None) == EINVAL   # 16-byte accesses
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,T,heads", [(3, 50, 32), (1, 2, 4), (5, 5, 8), (2, 145, 32), (7, 1, 2), (261, 50, 1)])
def test_single_query_attention_kernel(B, T, heads):
    """softmax(q . k_t / 8) . v per (image, head), fp32 in, pair out.  The same arithmetic in fp32 torch on the CPU gives the fp32
    error of this computation; the kernel's summation orders (a butterfly over the 64 lanes, t = 0 ... T - 1) differ from torch's,
    hence the factor 4: bound = max(PAIR_TOL max |ref|, 4 x that fp32 error)."""
    from viquae_amd import _lib
    from viquae_amd.encoders import SplitAct, _stream
    C = heads * 64
    g = torch.Generator().manual_seed(T * 100 + heads)
    q = torch.randn((B, C), generator=g) * 1.5
    kv = torch.randn((B * T, 2 * C), generator=g) * 1.5

    def attend(q, kv):
        qh = q.view(B, heads, 1, 64)
        k = kv[:, :C].reshape(B, T, heads, 64).transpose(1, 2)
        v = kv[:, C:].reshape(B, T, heads, 64).transpose(1, 2)
        p = torch.softmax((qh @ k.transpose(2, 3)) * 0.125, dim=-1)
        return (p @ v).transpose(1, 2).reshape(B, C), p
    ref, p = attend(q.double(), kv.double())
    cpu32, _ = attend(q, kv)
    qd, kvd = q.cuda(), kv.cuda()
    O = SplitAct.empty(B, C, qd.device)
    _lib.check(_lib.load().mq_attention_single_query_f32(qd.data_ptr(), kvd.data_ptr(), B, T, heads, 64, 0.125, O.hi.data_ptr(),
                                                         O.lo.data_ptr(), _stream(qd)), "mq_attention_single_query_f32")
    got = O.float().double().cpu()
    err, e32 = float((got - ref).abs().max()), float((cpu32.double() - ref).abs().max())
    tol = max(PAIR_TOL * float(ref.abs().max()), 4 * e32)
    print(f"single-query attention {(B, T, heads)}: max err {err:.3e}; fp32 torch-CPU err {e32:.3e}; pair bound "
          f"{PAIR_TOL * float(ref.abs().max()):.3e}; largest probability {float(p.max()):.3f}")
    assert err <= tol


def test_single_query_attention_argument_checks():
    from viquae_amd import _lib
    lib = _lib.load()
    z = torch.zeros(1 << 14, device="cuda")
    p = z.data_ptr()
    assert lib.mq_attention_single_query_f32(p, p, 1, 3, 2, 64, 0.125, p, p, None) == 0
    assert lib.mq_attention_single_query_f32(p, p, 0, 3, 2, 64, 0.125, p, p, None) == 0
    assert lib.mq_attention_single_query_f32(p, p, 1, 3, 2, 32, 0.125, p, p, None) == EUNSUPPORTED
    assert lib.mq_attention_single_query_f32(p, p, 1, 3, 2, 128, 0.125, p, p, None) == EUNSUPPORTED
    assert lib.mq_attention_single_query_f32(p, p, 1, 8193, 2, 64, 0.125, p, p, None) == EUNSUPPORTED
    assert lib.mq_attention_single_query_f32(p, p, 1, 0, 2, 64, 0.125, p, p, None) == EINVAL
    assert lib.mq_attention_single_query_f32(p, p, 1, 3, 0, 64, 0.125, p, p, None) == EINVAL
    assert lib.mq_attention_single_query_f32(None, p, 1, 3, 2, 64, 0.125, p, p, None) == EINVAL
    assert lib.mq_attention_single_query_f32(p, p, 1, 3, 2, 64, 0.125, None, p, None) == EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "clip_rn50_8.npz"))


@pytest.fixture(scope="module")
def golden_state(golden):
    return R.seeded_state(int(golden["state_seed"]), tuple(golden["layers"]))


def test_forward_matches_the_float64_golden(golden, golden_state):
    from viquae_amd.clip_resnet import CLIPModifiedResNet
    model = CLIPModifiedResNet.from_state_dict({"visual." + k: v for k, v in golden_state.items()}).cuda()
    x = torch.from_numpy(R.normalize_u8(golden["images_u8"], R.MEAN, R.STD)).cuda()
    with torch.no_grad():
        out = model(x)                      # the reference's positional call
        again = model(pixel_values=x)       # the pipeline's keyword call
    assert out.shape == (8, 1024) and out.dtype == torch.float32 and torch.equal(out, again)
    err = np.abs(out.cpu().numpy().astype(np.float64) - golden["out_f64"]).max()
    print(f"clip RN50: max |HIP - float64| = {err:.3e} (fp32 torch-CPU: {np.abs(golden['out_f32'] - golden['out_f64']).max():.3e}); "
          f"max |feature| = {np.abs(golden['out_f64']).max():.3f}")
    assert err <= 1e-3


@pytest.mark.parametrize("size,B", [(64, 5), (96, 3)])
def test_another_stage_layout_and_resolution(size, B):
    """layers = (1, 2, 1, 1) with a 2 x 2 and a 3 x 3 attention pool against the restatement run here on the CPU in float64"""
    from viquae_amd.clip_resnet import CLIPModifiedResNet
    layers = (1, 2, 1, 1)
    state = R.seeded_state(21 + size, layers, size)
    x = torch.randn((B, 3, size, size), generator=torch.Generator().manual_seed(4))
    ref = R.forward(state, x.numpy(), layers).numpy()
    ref32 = R.forward(state, x.numpy(), layers, dtype=torch.float32).numpy()
    model = CLIPModifiedResNet.from_state_dict(state, layers=layers).cuda()
    assert model.input_resolution == size and model.spacial_dim == size // 32
    with torch.no_grad():
        got = model(x.cuda()).cpu().numpy()
    assert got.shape == ref.shape == (B, 1024)
    err = np.abs(got - ref).max()
    print(f"layers {layers} at {size}: max err {err:.3e} (fp32 torch-CPU: {np.abs(ref32 - ref).max():.3e}), max |feature| {np.abs(ref).max():.3f}")
    assert err <= 1e-3
    for bad in ((1, 3, size + 32, size + 32), (1, 3, size, size + 32), (1, 3, 224, 200), (1, 1, size, size), (3, size, size)):
        with pytest.raises(ValueError, match=f"{size}, {size}"):
            model(torch.zeros(bad, device="cuda"))
    with pytest.raises(Exception, match="MI355X only"):
        model(torch.zeros((1, 3, size, size)))


def test_batch_invariance(golden, golden_state):
    """one forward of 8 images equals the concatenation of forwards over chunks of 3 and a model built with chunk=3, bit for bit"""
    from viquae_amd.clip_resnet import CLIPModifiedResNet
    x = torch.from_numpy(R.normalize_u8(golden["images_u8"], R.MEAN, R.STD)).cuda()
    whole = CLIPModifiedResNet.from_state_dict(golden_state).cuda()
    chunked = CLIPModifiedResNet.from_state_dict(golden_state, chunk=3).cuda()
    with torch.no_grad():
        a, b = whole(x), chunked(x)
        c = torch.cat([whole(x[s:s + 3]) for s in range(0, 8, 3)])
    assert a.shape == (8, 1024) and torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------------- transform, job
TRANSFORM = {"resize_kwargs": {"size": 224, "interpolation": "bicubic"}, "mean": list(R.MEAN), "std": list(R.STD)}


def _synthetic_images():
    """30 PIL images: mixed sizes (the ones where the two crop rules differ among them, up- and down-scaling) and modes"""
    from PIL import Image
    rng = np.random.default_rng(17)
    sizes = [(224, 231), (448, 462), (231, 224), (224, 224), (500, 375), (375, 500), (100, 150), (97, 60), (1024, 683), (227, 227),
             (300, 229), (229, 300), (640, 480), (235, 600), (900, 231), (462, 448), (224, 235), (51, 51), (333, 500), (2000, 1500)]
    out = []
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([128 + 100 * np.sin(xx / (3 + c + i % 5)) * np.cos(yy / (4 + c)) + rng.normal(0, 12, (h, w)) for c in range(3)], axis=2)
        out.append(Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)))
    base = out[4]
    out += [base.convert("L"), base.convert("RGBA"), base.convert("P"), out[0].convert("L"), out[1].convert("P"),
            out[6].convert("RGBA"), out[7].convert("L"), out[13].convert("P"), out[2].convert("RGBA"), out[11].convert("L")]
    return out


def test_transform_is_bit_identical_to_the_restatement():
    """clip.load's _transform(224) -- Resize(224, BICUBIC), CenterCrop(224), RGB, ToTensor, Normalize with CLIP's constants -- on the
    device (the documented config's transform_kwargs) against its restatement on PIL images"""
    from viquae_amd.image.preprocess import TorchvisionTransformHIP
    images = _synthetic_images()
    assert len(images) == 30
    got = TorchvisionTransformHIP(**TRANSFORM)(images, return_tensors="pt")["pixel_values"].cpu().numpy()
    want = np.stack([R.transform(im) for im in images])
    assert got.shape == want.shape == (30, 3, 224, 224) and got.dtype == np.float32
    bad = [i for i in range(30) if not np.array_equal(got[i], want[i])]
    assert not bad, [(i, images[i].size, images[i].mode, float(np.abs(got[i] - want[i]).max())) for i in bad]


def test_pipelined_job_equals_the_serial_embed_and_the_restatement(tmp_path, monkeypatch, golden_state):
    """python -m viquae_amd.image.embedding's dataset_embed with the documented config: PNG, baseline and progressive JPEG files, one
    that does not decode and one that is missing; pipelined (decode workers, JPEG on the device, the transform on a side stream)
    against the serial embed: the same None rows, the same bits; every vector within 1e-3 of the restatement of the whole path."""
    import shutil
    import datasets
    from PIL import Image
    from viquae_amd.data import loading
    from viquae_amd.image import embedding as IE
    datasets.disable_progress_bars()
    rng = np.random.default_rng(9)
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    monkeypatch.setattr(loading, "IMAGE_PATH", img_dir)
    names = []
    for i in range(22):
        h, w = (224 + 7 * (i % 5), 231 + 40 * (i % 4)) if i % 3 else (300 + 31 * i, 260 + 3 * i)
        yy, xx = np.mgrid[0:h, 0:w]
        a = np.stack([128 + 90 * np.sin(xx / (7 + c + i)) * np.cos(yy / (5 + c)) + rng.normal(0, 10, xx.shape) for c in range(3)], axis=2)
        ext, kw = (("jpg", dict(quality=88)), ("jpg", dict(quality=70, progressive=True)), ("png", {}), ("jpg", dict(subsampling=0)))[i % 4]
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(img_dir / f"f{i}.{ext}", **kw)
        names.append(f"f{i}.{ext}")
    data = open(img_dir / "f4.jpg", "rb").read()
    (img_dir / "cut.jpg").write_bytes(data[: len(data) // 2])     # opens, does not decode
    names[9], names[13] = "cut.jpg", "missing.jpg"
    datasets.Dataset.from_dict({"image": names, "id": list(range(len(names)))}).save_to_disk(str(tmp_path / "ds"))
    weights = tmp_path / "clip_RN50_state_dict.pth"
    torch.save({"visual." + k: torch.from_numpy(np.asarray(v)) for k, v in golden_state.items()}, weights)
    config = {"map_kwargs": {"batch_size": 256},
              "model_kwargs": {"type": "transformers", "class_name": "CLIPModifiedResNet", "pretrained_model_name_or_path": str(weights)},
              "transform_kwargs": dict({"class_name": "TorchvisionTransformHIP", "pretrained_model_name_or_path": None}, **TRANSFORM),
              "save_as": "clip-RN50"}
    outs = []
    # serial embed | the pipeline at one batch | the pipeline over batches of 8 with three decode processes
    for flag, bs, processes in (("0", 256, None), ("1", 256, None), ("1", 8, 3)):
        monkeypatch.setenv("MQ_EMBED_PIPELINE", flag)
        cfg = dict(config, map_kwargs={"batch_size": bs})
        work = tmp_path / f"ds{len(outs)}"    # its own copy: a second run on the same directory is served from the map cache
        shutil.copytree(tmp_path / "ds", work)
        with pytest.warns(UserWarning):
            ds = IE.dataset_embed(str(work), output_path=str(tmp_path / f"out{len(outs)}"), processes=processes, **cfg)
        st = IE.dataset_embed.last_pipeline_stats
        assert (st is not None) == (flag == "1") and (st is None or st["batches"] == -(-len(names) // bs))
        outs.append(ds["clip-RN50"])
    serial = outs[0]
    assert [i for i, v in enumerate(serial) if v is None] == [9, 13]
    a = np.asarray([v for v in serial if v is not None], dtype=np.float32)
    assert a.shape == (20, 1024)
    for o in outs[1:]:
        assert [v is None for v in o] == [v is None for v in serial]
        assert np.array_equal(a, np.asarray([v for v in o if v is not None], dtype=np.float32))
    kept = [n for i, n in enumerate(names) if i not in (9, 13)]
    x = np.stack([R.transform(Image.open(img_dir / n)) for n in kept])
    want = R.forward(golden_state, x).numpy()
    err = np.abs(a - want).max()
    print(f"job: max |vector - restatement| = {err:.3e}, max |feature| = {np.abs(want).max():.3f}")
    assert err <= 1e-3
