"""GPU suite of the torchvision ResNet encoder: each new kernel (csrc/resnet.hip) against float64 torch, the forward against the
float64 golden of tests/resnet_restatement.py, batch invariance, the device-side torchvision transform bit for bit against its
restatement, and the pipelined image job against the serial one."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resnet_restatement as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
POOL = {"Class_name": "AdaptiveMaxPool2d", "output_size": 1}
PAIR_TOL = 2e-5   # hi + lo keeps 16 mantissa bits (the ArcFace kernel tests' figure), times max |reference|


def _pair(x2d):
    """fp32 [rows, C] on the GPU -> its split pair"""
    from viquae_amd.encoders import SplitAct, split_bf16
    return SplitAct(*split_bf16(x2d.contiguous()))


@pytest.mark.parametrize("B,H,W", [(1, 32, 32), (3, 224, 224), (5, 64, 96), (2, 36, 40), (7, 4, 8)])
def test_stem_kernel_against_float64(B, H, W):
    """conv 7 x 7 / 2 + bias + ReLU + max-pool 3 x 3 / 2: odd batches, partial strips of pooled rows, images that are all border"""
    from viquae_amd import _lib
    from viquae_amd.encoders import SplitAct, _stream
    g = torch.Generator().manual_seed(B * 1000 + H)
    x = torch.randn((B, 3, H, W), generator=g)
    w = torch.randn((64, 3, 7, 7), generator=g) * 0.1
    b = torch.randn(64, generator=g) * 0.5
    ref = F.max_pool2d(F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=3)), 3, 2, 1)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, 64)
    xd, wt, bd = x.cuda(), w.permute(2, 3, 1, 0).reshape(147, 64).contiguous().cuda(), b.cuda()
    P = SplitAct.empty(B * (H // 4) * (W // 4), 64, xd.device)
    _lib.check(_lib.load().mq_stem_conv7x7_pool_f32(xd.data_ptr(), B, H, W, wt.data_ptr(), bd.data_ptr(), P.hi.data_ptr(), P.lo.data_ptr(),
                                                    _stream(xd)), "stem")
    got = P.float().double().cpu()
    assert got.shape == ref.shape
    err, tol = float((got - ref).abs().max()), PAIR_TOL * float(ref.abs().max())
    print(f"stem {B}x{H}x{W}: max err {err:.3e} tol {tol:.3e}")
    assert err <= tol


def test_stem_refuses_sizes_it_cannot_tile():
    from viquae_amd import _lib
    lib = _lib.load()
    z = torch.zeros(16, device="cuda")
    assert lib.mq_stem_conv7x7_pool_f32(z.data_ptr(), 1, 30, 32, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None) == -4
    assert lib.mq_stem_conv7x7_pool_f32(z.data_ptr(), 1, 32, 36, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None) == -4
    assert lib.mq_stem_conv7x7_pool_f32(None, 1, 32, 32, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None) == -1


# (B, H, W, C, N, stride, tile): tile 0 = AUTO, 1 = 256 x 256, 3 = 256 x 128, 4 = 512 x 64
CONV1X1 = [(2, 9, 7, 64, 64, 1, 0), (2, 9, 7, 64, 256, 1, 1), (3, 7, 5, 256, 128, 2, 3), (1, 23, 17, 96, 64, 2, 4),
           (5, 14, 14, 256, 512, 2, 0), (2, 28, 28, 128, 512, 1, 1), (1, 1, 1, 32, 64, 1, 0), (3, 16, 16, 512, 256, 1, 3),
           (4, 8, 8, 2048, 512, 1, 0), (1, 56, 56, 64, 256, 1, 4)]


@pytest.mark.parametrize("B,H,W,C,N,stride,tile", CONV1X1)
def test_conv1x1_kernel_against_float64(B, H, W, C, N, stride, tile):
    """both epilogues of the bottleneck (relu -> pair; + shortcut, relu -> fp32 and pair) and the downsample's (-> fp32), at stride
    1 and 2, with row counts that are not multiples of the 256-row tiles"""
    from viquae_amd import _lib
    from viquae_amd.encoders import SplitAct, _stream, split_bf16_tiled
    lib = _lib.load()
    g = torch.Generator().manual_seed(C + N + H)
    x = torch.randn((B * H * W, C), generator=g).cuda()
    w = (torch.randn((N, C), generator=g) / C ** 0.5).cuda()
    bias = torch.randn(N, generator=g).cuda()
    X = _pair(x)
    wh, wl = split_bf16_tiled(w)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    M = B * Ho * Wo
    res = torch.randn((M, N), generator=g).cuda()
    zeros = torch.zeros(64, dtype=torch.uint8, device="cuda")
    a = X.float().double().view(B, H, W, C)[:, ::stride, ::stride].reshape(M, C)   # what the kernel reads: the pair's values
    lin = a @ w.double().T + bias.double()

    def run(residual, relu, want_y, want_p):
        Y = torch.full((M, N), float("nan"), device="cuda") if want_y else None
        P = SplitAct.empty(M, N, x.device) if want_p else None
        p = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        _lib.check(lib.mq_conv1x1_pair_f32(X.hi.data_ptr(), X.lo.data_ptr(), B, H, W, C, stride, wh.data_ptr(), wl.data_ptr(), N,
                                           bias.data_ptr(), p(residual), relu, p(Y), P.hi.data_ptr() if P else None,
                                           P.lo.data_ptr() if P else None, zeros.data_ptr(), tile, _stream(x)), "mq_conv1x1_pair_f32")
        return Y, P
    cases = {"relu -> pair": (None, 1, False, True), "plain -> fp32": (None, 0, True, False),
             "shortcut, relu -> fp32 + pair": (res, 1, True, True), "shortcut, relu -> fp32": (res, 1, True, False)}
    for what, (residual, relu, want_y, want_p) in cases.items():
        ref = lin + (residual.double() if residual is not None else 0)
        ref = ref.clamp_min(0) if relu else ref
        tol = PAIR_TOL * float(ref.abs().max())
        Y, P = run(residual, relu, want_y, want_p)
        for name, got in (("Y", Y), ("P", P.float() if P is not None else None)):
            if got is not None:
                err = float((got.double() - ref).abs().max())
                print(f"conv1x1 {(B, H, W, C, N, stride, tile)} {what} {name}: max err {err:.3e} tol {tol:.3e}")
                assert err <= tol, (what, name)
        if Y is not None and P is not None:   # the pair is the split of the very fp32 value
            hi, lo = P.rowmajor()
            assert torch.equal(hi.view(torch.bfloat16), Y.bfloat16())
            assert torch.equal(lo.view(torch.bfloat16), (Y - Y.bfloat16().float()).bfloat16())


def test_conv1x1_argument_checks():
    from viquae_amd import _lib
    lib = _lib.load()
    z = torch.zeros(1 << 16, device="cuda")
    p = z.data_ptr()
    ok = dict(B=1, H=4, W=4, C=32, stride=1, N=64, tile=0)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.mq_conv1x1_pair_f32(p, p, a["B"], a["H"], a["W"], a["C"], a["stride"], p, p, a["N"], p, None, 1, a.get("Y", p),
                                       a.get("Ph", p), a.get("Pl", p), p, a["tile"], None)
    assert call() == 0 and call(B=0) == 0
    assert call(C=48) == -1 and call(N=96) == -1 and call(stride=3) == -1 and call(tile=2) == -1 and call(tile=1) == -1
    assert call(Y=None, Ph=None, Pl=None) == -1 and call(Pl=None) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("B,HW,C", [(8, 49, 2048), (3, 1, 100), (5, 6, 300), (1, 196, 64)])
def test_pool_kernel(B, HW, C):
    from viquae_amd import _lib
    from viquae_amd.encoders import _stream
    x = torch.randn((B * HW, C), generator=torch.Generator().manual_seed(HW)).cuda()
    for mode, ref in ((0, x.view(B, HW, C).amax(1)), (1, x.double().view(B, HW, C).mean(1))):
        out = torch.empty((B, C), device="cuda")
        _lib.check(_lib.load().mq_pool_hw_f32(x.data_ptr(), B, HW, C, mode, out.data_ptr(), _stream(x)), "mq_pool_hw_f32")
        if mode == 0:
            assert torch.equal(out, ref)
        else:
            seq = x.view(B, HW, C)[:, 0].clone()   # the documented order: p = 0 ... HW - 1 in fp32, then one division
            for k in range(1, HW):
                seq += x.view(B, HW, C)[:, k]
            assert np.array_equal(out.cpu().numpy(), seq.cpu().numpy() / np.float32(HW))   # an IEEE division, on the host
            assert float((out.double() - ref).abs().max()) <= PAIR_TOL * float(x.abs().max())
    assert _lib.load().mq_pool_hw_f32(x.data_ptr(), B, HW, C, 2, x.data_ptr(), None) == -1


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "resnet50_8.npz"))


@pytest.fixture(scope="module")
def golden_state(golden):
    return R.seeded_state(int(golden["state_seed"]), tuple(golden["layers"]))


@pytest.mark.parametrize("key,pool", [("max", "AdaptiveMaxPool2d"), ("mean", "AdaptiveAvgPool2d")])
def test_forward_matches_the_float64_golden(golden, golden_state, key, pool):
    from viquae_amd.resnet import TorchvisionResNet
    model = TorchvisionResNet.from_state_dict(golden_state, pool_kwargs={"Class_name": pool, "output_size": 1}).cuda()
    x = torch.from_numpy(R.normalize_u8(golden["images_u8"])).cuda()
    with torch.no_grad():
        out = model(x)                      # the reference's positional call
        again = model(pixel_values=x)       # the pipeline's keyword call
    assert out.shape == (8, 2048, 1, 1) and out.dtype == torch.float32 and torch.equal(out, again)
    got = out.squeeze().cpu().numpy().astype(np.float64)
    err = np.abs(got - golden[key + "_f64"]).max()
    print(f"resnet50 {key}-pool: max |HIP - float64| = {err:.3e} (fp32 torch-CPU: {np.abs(golden[key + '_f32'] - golden[key + '_f64']).max():.3e}); "
          f"max |feature| = {np.abs(golden[key + '_f64']).max():.3f}")
    assert err <= 1e-3


def test_another_stage_layout_and_size():
    """layers = (1, 2, 1, 1) at 64 x 96 against the restatement run here on the CPU in float64"""
    from viquae_amd.resnet import TorchvisionResNet
    layers = (1, 2, 1, 1)
    state = R.seeded_state(21, layers)
    x = torch.randn((5, 3, 64, 96), generator=torch.Generator().manual_seed(4))
    for pool in ("AdaptiveMaxPool2d", "AdaptiveAvgPool2d"):
        ref = R.forward(state, x.numpy(), layers, pool=pool).numpy()
        model = TorchvisionResNet.from_state_dict(state, layers=layers, pool_kwargs={"Class_name": pool, "output_size": [1, 1]}).cuda()
        with torch.no_grad():
            got = model(x.cuda()).cpu().numpy()
        assert got.shape == ref.shape == (5, 2048, 1, 1)
        err = np.abs(got - ref).max()
        print(f"layers {layers} {pool}: max err {err:.3e}, max |feature| {np.abs(ref).max():.3f}")
        assert err <= 1e-3
    with pytest.raises(ValueError, match="multiples of 32"):
        model(torch.zeros((1, 3, 224, 200), device="cuda"))
    with pytest.raises(Exception, match="MI355X only"):
        model(torch.zeros((1, 3, 64, 64)))


def test_batch_invariance(golden, golden_state):
    """one forward of 8 images equals the concatenation of forwards over chunks of 3, bit for bit"""
    from viquae_amd.resnet import TorchvisionResNet
    x = torch.from_numpy(R.normalize_u8(golden["images_u8"])).cuda()
    whole = TorchvisionResNet.from_state_dict(golden_state, pool_kwargs=POOL).cuda()
    chunked = TorchvisionResNet.from_state_dict(golden_state, pool_kwargs=POOL, chunk=3).cuda()
    with torch.no_grad():
        a, b = whole(x), chunked(x)
        c = torch.cat([whole(x[s:s + 3]) for s in range(0, 8, 3)])
    assert torch.equal(a, b) and torch.equal(a, c)


def _synthetic_images():
    """~30 PIL images: mixed sizes (the ones where the two crop rules differ among them, up- and down-scaling) and modes"""
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


@pytest.mark.parametrize("kwargs", [{}, {"resize_kwargs": {"size": 224, "interpolation": "bicubic"}},
                                    {"resize_kwargs": {"size": 256}, "crop_size": 224},
                                    {"resize_kwargs": {"size": [240, 300], "interpolation": 3}, "crop_size": 224},
                                    {"resize_kwargs": {"size": 231, "interpolation": 2}, "crop_size": 224}])
def test_transform_is_bit_identical_to_the_restatement(kwargs):
    from viquae_amd.image.preprocess import TorchvisionTransformHIP
    images = _synthetic_images()
    assert len(images) == 30
    t = TorchvisionTransformHIP(**kwargs)
    got = t(images, return_tensors="pt")["pixel_values"].cpu().numpy()
    rk = kwargs.get("resize_kwargs", {"size": 224})
    want = np.stack([R.transform_restatement(im, size=rk["size"], crop_size=kwargs.get("crop_size", 224),
                                             interpolation=rk.get("interpolation", "bilinear")) for im in images])
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
    weights = tmp_path / "resnet50_state_dict.pth"
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in golden_state.items()}, weights)
    config = {"map_kwargs": {"batch_size": 256},
              "model_kwargs": {"type": "transformers", "class_name": "TorchvisionResNet", "pretrained_model_name_or_path": str(weights),
                               "pool_kwargs": {"Class_name": "AdaptiveMaxPool2d", "output_size": 1}},
              "transform_kwargs": {"class_name": "TorchvisionTransformHIP", "pretrained_model_name_or_path": None},
              "save_as": "imagenet-RN50"}
    outs = []
    # serial embed | the pipeline at the config's batch (one batch) | the pipeline over batches of 8 with three decode processes
    for flag, bs, processes in (("0", 256, None), ("1", 256, None), ("1", 8, 3)):
        monkeypatch.setenv("MQ_EMBED_PIPELINE", flag)
        cfg = dict(config, map_kwargs={"batch_size": bs})
        work = tmp_path / f"ds{len(outs)}"    # its own copy: a second run on the same directory is served from the map cache
        shutil.copytree(tmp_path / "ds", work)
        with pytest.warns(UserWarning):
            ds = IE.dataset_embed(str(work), output_path=str(tmp_path / f"out{len(outs)}"), processes=processes, **cfg)
        st = IE.dataset_embed.last_pipeline_stats
        assert (st is not None) == (flag == "1") and (st is None or st["batches"] == -(-len(names) // bs))
        outs.append(ds["imagenet-RN50"])
    serial = outs[0]
    assert [i for i, v in enumerate(serial) if v is None] == [9, 13]
    a = np.asarray([v for v in serial if v is not None], dtype=np.float32)
    assert a.shape == (20, 2048)
    for o in outs[1:]:
        assert [v is None for v in o] == [v is None for v in serial]
        assert np.array_equal(a, np.asarray([v for v in o if v is not None], dtype=np.float32))
    kept = [n for i, n in enumerate(names) if i not in (9, 13)]
    x = np.stack([R.transform_restatement(Image.open(img_dir / n)) for n in kept])
    want = R.forward(golden_state, x, pool="AdaptiveMaxPool2d").reshape(len(kept), -1).numpy()
    err = np.abs(a - want).max()
    print(f"job: max |vector - restatement| = {err:.3e}")
    assert err <= 1e-3
