"""CPU suite of the torchvision ResNet encoder (viquae_amd/resnet.py) and its transform: the restatement and its golden, the crop
rule of the image plan, the configuration surface, the refusals and the BatchNorm folding.  No GPU: the model is only constructed."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from tests import resnet_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
POOL = {"Class_name": "AdaptiveMaxPool2d", "output_size": 1}
# the shipped experiments/image_embedding/imagenet/config.json with model_kwargs.type / class_name added and a transform_kwargs
CONFIG = {"map_kwargs": {"batch_size": 256},
          "model_kwargs": {"type": "transformers", "class_name": "TorchvisionResNet",
                           "pretrained_model_name_or_path": "resnet50_state_dict.pth", "pool_kwargs": POOL},
          "transform_kwargs": {"class_name": "TorchvisionTransformHIP", "pretrained_model_name_or_path": None},
          "save_as": "imagenet-RN50"}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "resnet50_8.npz"))


def _torch_state(state):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}


def test_restatement_reproduces_the_golden(golden):
    state = R.seeded_state(int(golden["state_seed"]), tuple(golden["layers"]))
    assert np.array_equal(R.golden_images(int(golden["image_seed"])), golden["images_u8"])
    x = R.normalize_u8(golden["images_u8"])
    for key, pool in (("max", "AdaptiveMaxPool2d"), ("mean", "AdaptiveAvgPool2d")):
        got = R.forward(state, x, pool=pool, dtype=torch.float32).reshape(8, -1).numpy()
        ref = golden[key + "_f32"]
        assert got.shape == ref.shape == (8, 2048)
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()
        assert np.abs(ref - golden[key + "_f64"]).max() <= 1e-4   # the fp32 reference itself, against float64


def test_golden_scale_and_liveness(golden):
    """the 1e-3 absolute tolerance of the GPU test is at most 1e-3 of the largest feature, and no image's features are mostly dead"""
    for key in ("max_f64", "mean_f64"):
        f = golden[key]
        assert 1.0 <= np.abs(f).max() <= 30.0, key
        assert ((f != 0).sum(axis=1) > 1024).all(), key


SIZES = [(224, 231), (448, 462), (231, 224), (224, 224), (500, 375), (375, 500), (227, 227), (300, 229), (1000, 700), (235, 600)]


def test_image_plan_crop_rules(hip_lib):
    """mq_image_plan: the torchvision rule is int(round((size - crop) / 2.0)); the default stays (size - crop) // 2"""
    sizes = np.asarray(SIZES, dtype=np.int64)

    def plan(mode):
        geom, totals = np.zeros((len(SIZES), 12), np.int64), np.zeros(5, np.int64)
        assert hip_lib.mq_image_plan(sizes.ctypes.data, len(SIZES), mode, 224, 0, 224, 224, 2, geom.ctypes.data, totals.ctypes.data) == 0
        return geom
    default, tv = plan(1), plan(1 | 0x100)   # MQ_IMAGE_RESIZE_SHORTEST, | MQ_IMAGE_CROP_TORCHVISION
    outs = [R.resize_output_size(h, w, 224) for h, w in SIZES]
    G_OUTH, G_OUTW, G_TOP, G_LEFT = 3, 4, 5, 6   # the geometry table's fields (csrc/image.hip)
    differ = 0
    for row, (oh, ow) in enumerate(outs):
        assert tuple(default[row, G_OUTH:G_OUTW + 1]) == tuple(tv[row, G_OUTH:G_OUTW + 1]) == (oh, ow)
        assert tuple(default[row, G_TOP:G_LEFT + 1]) == ((oh - 224) // 2, (ow - 224) // 2), SIZES[row]
        assert tuple(tv[row, G_TOP:G_LEFT + 1]) == (R.crop_origin(oh, 224), R.crop_origin(ow, 224)), SIZES[row]
        other = [c for c in range(12) if c not in (G_TOP, G_LEFT)]
        assert np.array_equal(default[row, other], tv[row, other])
        differ += not np.array_equal(default[row], tv[row])
    assert outs[0] == (224, 231) and outs[1] == (224, 231) and outs[2] == (231, 224)
    assert R.crop_origin(231, 224) == 4 and (231 - 224) // 2 == 3 and differ >= 3
    # the transform classes ask for their own rule
    from viquae_amd.image.preprocess import CLIPImageProcessorHIP, TorchvisionTransformHIP
    g_tv, _ = TorchvisionTransformHIP().plan(sizes)
    g_clip, _ = CLIPImageProcessorHIP(size=224, resample=2).plan(sizes)
    assert np.array_equal(g_tv, tv) and np.array_equal(g_clip, default)


def test_rescale_table_is_torchvisions_rule():
    """float32(float64(u8) * (1 / 255)) == float32(u8) / float32(255) for all 256 bytes, so (x - mean) / std agree too"""
    u = np.arange(256)
    table = (u.astype(np.float64) * (1 / 255)).astype(np.float32)
    tv = u.astype(np.float32) / np.float32(255)
    assert np.array_equal(table, tv)
    for m, s in zip(R.MEAN, R.STD):
        assert np.array_equal((table - np.float32(m)) / np.float32(s), (tv - np.float32(m)) / np.float32(s))


def test_classes_resolve_and_the_config_binds(tmp_path):
    from viquae_amd import encoders
    from viquae_amd.data.loading import get_class_from_name, get_pretrained
    from viquae_amd.image import embedding as IE
    from viquae_amd.image.preprocess import TorchvisionTransformHIP
    from viquae_amd.resnet import TorchvisionResNet
    assert get_class_from_name("TorchvisionResNet") is TorchvisionResNet is encoders.HIP_CLASSES["TorchvisionResNet"]
    assert get_class_from_name("TorchvisionTransformHIP") is TorchvisionTransformHIP
    config = json.loads(json.dumps(CONFIG))
    job = inspect.signature(IE.dataset_embed).bind("some/dataset", **config)
    inspect.signature(IE.embed).bind({"image": []}, model=object(), transform=object(), **job.arguments["fn_kwargs"])
    assert job.arguments["fn_kwargs"] == {"save_as": "imagenet-RN50"}
    # ... and loads: a (1, 1, 1, 1) state on disk, `layers` beside the other model keywords
    path = tmp_path / "resnet_state_dict.pth"
    torch.save(_torch_state(R.seeded_state(3, (1, 1, 1, 1))), path)
    config["model_kwargs"].update(pretrained_model_name_or_path=str(path), layers=[1, 1, 1, 1])
    got = IE.get_model_and_transform(model_kwargs=config["model_kwargs"], transform_kwargs=config["transform_kwargs"])
    model, transform = got["model"], got["transform"]
    assert isinstance(model, TorchvisionResNet) and model.layers == (1, 1, 1, 1) and not model.training and model.num_features == 2048
    assert isinstance(transform, TorchvisionTransformHIP) and transform.on_device and (transform.crop_h, transform.crop_w) == (224, 224)
    assert transform.resample == 2 and transform.size_mode == "shortest" and transform.size_h == 224
    with pytest.raises(NotImplementedError):
        model.train(True)
    # the encoders still refuse a random initialisation
    with pytest.raises(ValueError, match="random initialisation"):
        get_pretrained("TorchvisionResNet", None, pool_kwargs=POOL)


def test_transform_keywords():
    from viquae_amd.image.preprocess import TorchvisionTransformHIP as T
    t = T(resize_kwargs={"size": [256, 300], "interpolation": "bicubic"}, crop_size=224)
    assert (t.size_mode, t.size_h, t.size_w, t.resample) == ("exact", 256, 300, 3)
    assert T(resize_kwargs={"size": 256, "interpolation": 3}).resample == 3 and T.from_pretrained(None, crop_size=192).crop_h == 192
    with pytest.raises(NotImplementedError):
        T(resize_kwargs={"size": 224, "max_size": 300})
    with pytest.raises(NotImplementedError):
        T(resize_kwargs={"size": 224, "interpolation": "nearest"})
    with pytest.raises(NotImplementedError, match="pads"):
        T(resize_kwargs={"size": [100, 300]}).plan(np.asarray([[50, 60]]))


def test_type_torchvision_is_still_declined():
    from viquae_amd.image import embedding as IE
    with pytest.raises(NotImplementedError, match="outside the MI355X build"):
        IE.get_model_and_transform({"type": "torchvision", "pool_kwargs": POOL})
    for other in ("clip", "torchscript"):
        with pytest.raises(NotImplementedError, match="outside the MI355X build"):
            IE.get_model_and_transform({"type": other})


def test_missing_weight_file(tmp_path):
    from viquae_amd.resnet import TorchvisionResNet
    missing = tmp_path / "nowhere" / "resnet50_state_dict.pth"
    with pytest.raises(FileNotFoundError, match="resnet50_state_dict.pth"):
        TorchvisionResNet.from_pretrained(missing, pool_kwargs=POOL)


def test_refusals():
    from viquae_amd.resnet import TorchvisionResNet as M
    state = R.seeded_state(3, (1, 1, 1, 1))
    basic = {k: v for k, v in state.items() if ".conv3." not in k and ".bn3." not in k}
    with pytest.raises(NotImplementedError, match="BasicBlock"):
        M.from_state_dict(basic, layers=(1, 1, 1, 1), pool_kwargs=POOL)
    grouped = dict(state)
    grouped["layer1.0.conv2.weight"] = state["layer1.0.conv2.weight"][:, :2]   # groups = 32
    with pytest.raises(NotImplementedError, match="grouped"):
        M.from_state_dict(grouped, layers=(1, 1, 1, 1), pool_kwargs=POOL)
    with pytest.raises(NotImplementedError):
        M.from_state_dict(state, layers=(1, 1, 1, 1), pool_kwargs=POOL, replace_stride_with_dilation=[False, True, True])
    for bad in ({"Class_name": "AdaptiveMaxPool2d", "output_size": 2}, {"Class_name": "MaxPool2d", "kernel_size": 7},
                {"Class_name": "AdaptiveAvgPool2d", "output_size": [7, 7]}):
        with pytest.raises(NotImplementedError):
            M.from_state_dict(state, layers=(1, 1, 1, 1), pool_kwargs=bad)
    with pytest.raises(TypeError):
        M.from_state_dict(state, layers=(1, 1, 1, 1))
    with pytest.raises(ValueError, match="layers"):
        M.from_state_dict(state, pool_kwargs=POOL)   # resnet50's depths on a (1, 1, 1, 1) state
    for ok in ({"Class_name": "AdaptiveAvgPool2d", "output_size": (1, 1)}, {"Class_name": "AdaptiveMaxPool2d", "output_size": [1, 1]}):
        M.from_state_dict({"module." + k: v for k, v in state.items()}, layers=(1, 1, 1, 1), pool_kwargs=ok)


def test_folding_is_exact_in_float64():
    """conv(x, W') + b == bn(conv(x, W)) to 1e-12, for the three kernel sizes of the network"""
    from viquae_amd.arcface import _affine
    from viquae_amd.resnet import fold_conv_bn
    rng = np.random.default_rng(11)
    for cout, cin, k, stride, pad in ((16, 3, 7, 2, 3), (24, 8, 3, 2, 1), (32, 16, 1, 1, 0)):
        state = {"c.weight": rng.standard_normal((cout, cin, k, k)), "b.weight": rng.uniform(0.5, 1.5, cout),
                 "b.bias": rng.standard_normal(cout), "b.running_mean": rng.standard_normal(cout),
                 "b.running_var": rng.uniform(0.5, 2.0, cout)}
        x = torch.from_numpy(rng.standard_normal((2, cin, 13, 11)))
        t = {n: torch.from_numpy(v) for n, v in state.items()}
        ref = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, t["c.weight"], stride=stride, padding=pad),
                                             t["b.running_mean"], t["b.running_var"], t["b.weight"], t["b.bias"], training=False, eps=1e-5)
        w, b = fold_conv_bn(state["c.weight"], _affine(state, "b"))
        assert w.dtype == np.float64 and b.dtype == np.float64
        got = torch.nn.functional.conv2d(x, torch.from_numpy(w), torch.from_numpy(b), stride=stride, padding=pad)
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_loaded_weights_are_the_folded_ones():
    """the registered fp32 weights: (kh, kw, c) columns of the float64 fold; the stem's [147, 64] transpose"""
    from viquae_amd.arcface import _affine
    from viquae_amd.resnet import TorchvisionResNet, fold_conv_bn
    state = R.seeded_state(5, (1, 1, 1, 1))
    m = TorchvisionResNet.from_state_dict(state, layers=(1, 1, 1, 1), pool_kwargs=POOL)
    for name, bn in (("conv1", "bn1"), ("layer2.0.conv2", "layer2.0.bn2"), ("layer3.0.downsample.0", "layer3.0.downsample.1")):
        w, b = fold_conv_bn(state[name + ".weight"], _affine(state, bn))
        assert np.array_equal(m._b(name + ".w2").numpy(), w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1).astype(np.float32))
        assert np.array_equal(m._b(name + ".b").numpy(), b.astype(np.float32))
    assert np.array_equal(m.conv1_wt.numpy(), m.conv1_w2.numpy().T) and m.conv1_wt.shape == (147, 64)
    assert m._geom["layer2.0.conv2"] == (128, 128, 3, 2) and m._geom["layer2.0.downsample.0"] == (512, 256, 1, 2)
    assert m._geom["layer1.0.downsample.0"] == (256, 64, 1, 1)
