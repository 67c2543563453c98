"""CPU suite of the CLIP ResNet encoder (viquae_amd/clip_resnet.py): the restatement and its golden, the BatchNorm folding and the
padded stem weights, the loader (prefixes, fp16 storage, a full CLIP state dict, TorchScript archives), the refusals and the
configuration surface.  No GPU: the model is only constructed."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import clip_resnet_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SMALL = (1, 1, 1, 1)
# INTEGRATION.md's stand-in for experiments/image_embedding/clip/config.json
CONFIG = {"map_kwargs": {"batch_size": 2048},
          "model_kwargs": {"type": "transformers", "class_name": "CLIPModifiedResNet",
                           "pretrained_model_name_or_path": "clip_RN50_state_dict.pth"},
          "transform_kwargs": {"class_name": "TorchvisionTransformHIP", "pretrained_model_name_or_path": None,
                               "resize_kwargs": {"size": 224, "interpolation": "bicubic"},
                               "mean": [0.48145466, 0.4578275, 0.40821073], "std": [0.26862954, 0.26130258, 0.27577711]},
          "save_as": "clip-RN50"}
NEW_SYMBOLS = ("mq_clip_stem_conv3x3s2_f32", "mq_avgpool2x2_pair_f32", "mq_attnpool_tokens_f32", "mq_attention_single_query_f32")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "clip_rn50_8.npz"))


def _torch_state(state, prefix=""):
    return {prefix + k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}


def test_restatement_reproduces_the_golden(golden):
    state = R.seeded_state(int(golden["state_seed"]), tuple(golden["layers"]))
    assert np.array_equal(R.golden_images(int(golden["image_seed"])), golden["images_u8"])
    x = R.normalize_u8(golden["images_u8"], R.MEAN, R.STD)
    got = R.forward(state, x, dtype=torch.float32).numpy()
    ref = golden["out_f32"]
    assert got.shape == ref.shape == (8, 1024) and golden["out_f64"].dtype == np.float64
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


def test_golden_scale_and_the_fp32_reference(golden):
    """the encoder gate (1e-3 absolute) means something: the features are of order 1 and fp32 torch itself is far inside the gate;
    were either to fail, the seeded state would be wrong, not the gate"""
    f64, f32 = golden["out_f64"], golden["out_f32"]
    err = np.abs(f32 - f64).max()
    print(f"max |golden| = {np.abs(f64).max():.3f}, max |fp32 torch-CPU - float64| = {err:.3e}")
    assert np.abs(f64).max() >= 1.0
    assert err <= 1e-3


def test_seeded_state_is_stored_like_the_checkpoint_and_attends():
    """convolution / linear tensors fp16, BatchNorm and the positional embedding fp32; on a small state the attention is neither
    uniform nor one-hot"""
    state = R.seeded_state(5, SMALL, 64)
    for k, v in state.items():
        if k.endswith("num_batches_tracked"):
            continue
        conv_or_linear = re.search(r"(conv\d|downsample\.0|_proj)\.(weight|bias)$", k) is not None
        assert v.dtype == (np.float16 if conv_or_linear else np.float32), k
    assert state["attnpool.positional_embedding"].shape == (5, 2048) and "layer2.0.downsample.0.weight" in state
    x = np.random.default_rng(0).standard_normal((3, 3, 64, 64)).astype(np.float32)
    out, p = R.forward(state, x, SMALL, return_attention=True)
    assert out.shape == (3, 1024) and p.shape == (3, 32, 5)
    assert torch.allclose(p.sum(-1), torch.ones(3, 32, dtype=torch.float64))
    entropy = -(p * p.log()).sum(-1)
    assert 0.1 < float(entropy.min()) and float(entropy.max()) < np.log(5) - 1e-3


def test_attention_pool_restatement_is_multi_head_attention():
    """the written-out pool against torch's own F.multi_head_attention_forward, the call AttentionPool2d makes"""
    state = R.seeded_state(9, SMALL, 96)
    f = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 2048, 3, 3))).relu()
    t = lambda k: torch.from_numpy(state["attnpool." + k].astype(np.float64))  # noqa: E731
    x = f.flatten(2).permute(2, 0, 1)
    x = torch.cat([x.mean(dim=0, keepdim=True), x], dim=0) + t("positional_embedding")[:, None, :]
    ref, _ = torch.nn.functional.multi_head_attention_forward(
        query=x[:1], key=x, value=x, embed_dim_to_check=2048, num_heads=32, q_proj_weight=t("q_proj.weight"),
        k_proj_weight=t("k_proj.weight"), v_proj_weight=t("v_proj.weight"), in_proj_weight=None,
        in_proj_bias=torch.cat([t("q_proj.bias"), t("k_proj.bias"), t("v_proj.bias")]), bias_k=None, bias_v=None, add_zero_attn=False,
        dropout_p=0.0, out_proj_weight=t("c_proj.weight"), out_proj_bias=t("c_proj.bias"), use_separate_proj_weight=True,
        training=False, need_weights=False)
    got = R.attention_pool(state, f)
    assert got.shape == ref.squeeze(0).shape == (2, 1024)
    assert float((got - ref.squeeze(0)).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_folding_is_exact_in_float64():
    """conv(x, W') + b == bn(conv(x, W)) to 1e-12 for the stem's strided 3 x 3 and a block's convolutions, from fp16-stored weights"""
    from viquae_amd.arcface import _affine
    from viquae_amd.resnet import fold_conv_bn
    rng = np.random.default_rng(11)
    for cout, cin, k, stride, pad in ((32, 3, 3, 2, 1), (24, 8, 3, 1, 1), (32, 16, 1, 1, 0)):
        state = {"c.weight": rng.standard_normal((cout, cin, k, k)).astype(np.float16), "b.weight": rng.uniform(0.5, 1.5, cout),
                 "b.bias": rng.standard_normal(cout), "b.running_mean": rng.standard_normal(cout),
                 "b.running_var": rng.uniform(0.5, 2.0, cout)}
        x = torch.from_numpy(rng.standard_normal((2, cin, 14, 10)))
        t = {n: torch.from_numpy(np.asarray(v, np.float64)) for n, v in state.items()}
        ref = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, t["c.weight"], stride=stride, padding=pad),
                                             t["b.running_mean"], t["b.running_var"], t["b.weight"], t["b.bias"], training=False, eps=1e-5)
        w, b = fold_conv_bn(state["c.weight"], _affine(state, "b"))
        assert w.dtype == np.float64 and b.dtype == np.float64
        got = torch.nn.functional.conv2d(x, torch.from_numpy(w), torch.from_numpy(b), stride=stride, padding=pad)
        assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_loaded_weights_are_the_folded_ones():
    """the registered fp32 tensors: the float64 fold with (kh, kw, c) columns; the stem's [27, 32] transpose; conv2's 32 output
    channels and conv3's 32 input channels of zeros; every block convolution at stride 1 and the pooled blocks; the head"""
    from viquae_amd.arcface import _affine
    from viquae_amd.clip_resnet import CLIPModifiedResNet
    from viquae_amd.resnet import fold_conv_bn
    state = R.seeded_state(5, SMALL, 64)
    m = CLIPModifiedResNet.from_state_dict(state, layers=SMALL)
    for name, bn in (("conv1", "bn1"), ("layer2.0.conv2", "layer2.0.bn2"), ("layer3.0.downsample.0", "layer3.0.downsample.1")):
        w, b = fold_conv_bn(state[name + ".weight"], _affine(state, bn))
        assert np.array_equal(m._b(name + ".w2").numpy(), w.transpose(0, 2, 3, 1).reshape(w.shape[0], -1).astype(np.float32))
        assert np.array_equal(m._b(name + ".b").numpy(), b.astype(np.float32))
    assert np.array_equal(m.conv1_wt.numpy(), m.conv1_w2.numpy().T) and m.conv1_wt.shape == (27, 32)
    w2, b2 = fold_conv_bn(state["conv2.weight"], _affine(state, "bn2"))
    got = m.conv2_w2.numpy().reshape(64, 3, 3, 32)
    assert np.array_equal(got[:32], w2.transpose(0, 2, 3, 1).astype(np.float32)) and not got[32:].any()
    assert np.array_equal(m.conv2_b.numpy()[:32], b2.astype(np.float32)) and not m.conv2_b.numpy()[32:].any()
    w3, _ = fold_conv_bn(state["conv3.weight"], _affine(state, "bn3"))
    got = m.conv3_w2.numpy().reshape(64, 3, 3, 64)
    assert np.array_equal(got[..., :32], w3.transpose(0, 2, 3, 1).astype(np.float32)) and not got[..., 32:].any()
    assert m._geom["conv1"] == (32, 3, 3, 2) and m._geom["conv2"] == (64, 32, 3, 1) and m._geom["conv3"] == (64, 64, 3, 1)
    assert m._geom["layer2.0.conv2"] == (128, 128, 3, 1) and m._geom["layer2.0.downsample.0"] == (512, 256, 1, 1)
    assert m._avgpooled == {"layer2.0", "layer3.0", "layer4.0"} and "layer1.0.downsample.0" in m._geom
    assert (m.spacial_dim, m.input_resolution, m.heads, m.output_dim, m.num_features) == (2, 64, 32, 1024, 2048)
    assert np.array_equal(m.kv_w.numpy(), np.concatenate([state["attnpool.k_proj.weight"], state["attnpool.v_proj.weight"]]).astype(np.float32))
    assert np.array_equal(m.kv_b.numpy(), np.concatenate([state["attnpool.k_proj.bias"], state["attnpool.v_proj.bias"]]).astype(np.float32))
    assert np.array_equal(m.pos.numpy(), state["attnpool.positional_embedding"]) and m.c_w.shape == (1024, 2048)
    # the torchvision walk has no pooled block
    from viquae_amd.resnet import TorchvisionResNet
    assert TorchvisionResNet._avgpooled == frozenset()


def _same_buffers(a, b):
    sa, sb = dict(a.named_buffers()), dict(b.named_buffers())
    return sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_loader_prefixes_fp16_and_a_full_clip_state_dict(tmp_path):
    from viquae_amd.clip_resnet import CLIPModifiedResNet as M
    state = R.seeded_state(6, SMALL, 64)
    bare = M.from_state_dict(state, layers=SMALL)
    assert bare.q_w.dtype == torch.float32 and np.array_equal(bare.q_w.numpy(), state["attnpool.q_proj.weight"].astype(np.float32))
    for prefix in ("visual.", "module.", "module.visual."):
        assert _same_buffers(bare, M.from_state_dict(_torch_state(state, prefix), layers=SMALL)), prefix
    # the same weights stored in fp32 load to the same buffers: the fp16 upcast is exact
    assert _same_buffers(bare, M.from_state_dict({k: np.asarray(v, np.float32) if v.dtype == np.float16 else v for k, v in state.items()},
                                                 layers=SMALL))
    # a full CLIP state dict: the text tower's keys, one of them NAMED like the pool's positional embedding, are ignored
    full = _torch_state(state, "visual.")
    full.update({"positional_embedding": torch.zeros(77, 512), "text_projection": torch.zeros(512, 1024), "logit_scale": torch.tensor(4.6),
                 "token_embedding.weight": torch.zeros(10, 512), "ln_final.weight": torch.ones(512), "ln_final.bias": torch.zeros(512),
                 "transformer.resblocks.0.attn.in_proj_weight": torch.zeros(1536, 512).half(), "input_resolution": torch.tensor(64),
                 "context_length": torch.tensor(77), "vocab_size": torch.tensor(10)})
    assert _same_buffers(bare, M.from_state_dict(full, layers=SMALL))
    path = tmp_path / "clip_state_dict.pth"
    torch.save(full, path)
    loaded = M.from_pretrained(path, layers=[1, 1, 1, 1])
    assert _same_buffers(bare, loaded) and loaded.layers == SMALL and not loaded.training


def test_missing_weight_file(tmp_path):
    from viquae_amd.clip_resnet import CLIPModifiedResNet
    missing = tmp_path / "nowhere" / "clip_RN50_state_dict.pth"
    with pytest.raises(FileNotFoundError, match="clip_RN50_state_dict.pth"):
        CLIPModifiedResNet.from_pretrained(missing)


class _Node(torch.nn.Module):
    pass


class _Archive(torch.nn.Module):
    """what the original RN50.pt is to the loader: a scripted module whose state dict carries the weights under CLIP's dotted names
    (a tree of forward-less containers; its own forward is never run)"""

    def __init__(self, state):
        super().__init__()
        for key, value in state.items():
            *path, leaf = key.split(".")
            module = self
            for name in path:
                if name not in module._modules:
                    module.add_module(name, _Node())
                module = module._modules[name]
            module.register_buffer(leaf, value)

    def forward(self, x):
        return x


def test_torchscript_archive_fallback(tmp_path, monkeypatch):
    """a TorchScript archive (a scripted container made here, saved with torch.jit.save) is refused by torch.load(weights_only=True);
    the loader then reads torch.jit.load(path, map_location="cpu").state_dict().  torch.jit.load is only wrapped to record the call."""
    from viquae_amd.clip_resnet import CLIPModifiedResNet as M
    state = _torch_state(R.seeded_state(8, SMALL, 64), "visual.")
    state["logit_scale"] = torch.tensor(4.6)
    path = tmp_path / "RN50.pt"
    torch.jit.script(_Archive(state)).save(str(path))
    with pytest.raises(Exception), pytest.warns(UserWarning):
        torch.load(path, map_location="cpu", weights_only=True)
    real_load, calls = torch.jit.load, []

    def jit_load(f, map_location=None, **kw):
        calls.append((os.fspath(f), map_location))
        return real_load(f, map_location=map_location, **kw)
    monkeypatch.setattr(torch.jit, "load", jit_load)
    m = M.from_pretrained(path, layers=SMALL)
    assert calls == [(str(path), "cpu")]
    assert _same_buffers(m, M.from_state_dict(state, layers=SMALL)) and m.q_w.dtype == torch.float32
    # a plain state-dict file never reaches torch.jit.load
    plain = tmp_path / "plain.pth"
    torch.save(state, plain)
    assert _same_buffers(m, M.from_pretrained(plain, layers=SMALL)) and len(calls) == 1
    # a file that is neither: the first loader's error is the one reported
    junk = tmp_path / "junk.pth"
    junk.write_bytes(b"not a checkpoint")
    with pytest.raises(Exception) as e:
        M.from_pretrained(junk)
    assert not isinstance(e.value, FileNotFoundError) and "junk" not in type(e.value).__name__


def test_refusals():
    from viquae_amd.clip_resnet import CLIPModifiedResNet as M
    state = R.seeded_state(3, SMALL, 64)
    # RN50x4 (width 80) and RN50x64 (width 128)
    for width in (80, 128):
        wide = R.seeded_state(3, SMALL, 64, width=width)
        with pytest.raises(NotImplementedError, match="width"):
            M.from_state_dict(wide, layers=SMALL)
    with pytest.raises(NotImplementedError, match="head size"):
        M.from_state_dict(state, layers=SMALL, heads=16)
    vit = {"visual.class_embedding": np.zeros(768, np.float16), "visual.conv1.weight": np.zeros((768, 3, 32, 32), np.float16),
           "visual.positional_embedding": np.zeros((50, 768), np.float16), "visual.proj": np.zeros((768, 512), np.float16)}
    with pytest.raises(NotImplementedError, match="attnpool"):
        M.from_state_dict(vit)
    with pytest.raises(ValueError, match="layers"):
        M.from_state_dict(state)                      # RN50's depths on a (1, 1, 1, 1) state
    with pytest.raises(ValueError, match="layers"):
        M.from_state_dict(state, layers=(1, 1, 1))
    m = M.from_state_dict(state, layers=SMALL)
    with pytest.raises(NotImplementedError, match="eval mode"):
        m.train(True)
    assert m.train(False) is m and m.eval() is m and not m.training
    bad = dict(state)
    bad["attnpool.positional_embedding"] = state["attnpool.positional_embedding"][:4]
    with pytest.raises(ValueError, match="positional_embedding"):
        M.from_state_dict(bad, layers=SMALL)


def test_class_resolves_and_the_documented_config_binds(tmp_path):
    from viquae_amd import encoders
    from viquae_amd.clip_resnet import CLIPModifiedResNet
    from viquae_amd.data.loading import get_class_from_name, get_pretrained
    from viquae_amd.image import embedding as IE
    from viquae_amd.image.preprocess import TorchvisionTransformHIP
    assert get_class_from_name("CLIPModifiedResNet") is CLIPModifiedResNet is encoders.HIP_CLASSES["CLIPModifiedResNet"]
    config = json.loads(json.dumps(CONFIG))
    job = inspect.signature(IE.dataset_embed).bind("some/dataset", **config)
    inspect.signature(IE.embed).bind({"image": []}, model=object(), transform=object(), **job.arguments["fn_kwargs"])
    assert job.arguments["fn_kwargs"] == {"save_as": "clip-RN50"}
    # ... and loads: a (1, 1, 1, 1) state for 64 x 64 on disk, `layers` beside the other model keywords
    path = tmp_path / "clip_state_dict.pth"
    torch.save(_torch_state(R.seeded_state(3, SMALL, 64), "visual."), path)
    config["model_kwargs"].update(pretrained_model_name_or_path=str(path), layers=[1, 1, 1, 1])
    got = IE.get_model_and_transform(model_kwargs=config["model_kwargs"], transform_kwargs=config["transform_kwargs"])
    model, transform = got["model"], got["transform"]
    assert isinstance(model, CLIPModifiedResNet) and model.layers == SMALL and not model.training and model.output_dim == 1024
    assert isinstance(transform, TorchvisionTransformHIP) and transform.on_device and (transform.crop_h, transform.crop_w) == (224, 224)
    assert transform.resample == 3 and transform.size_mode == "shortest" and transform.size_h == 224
    with pytest.raises(ValueError, match="random initialisation"):
        get_pretrained("CLIPModifiedResNet", None)
    # the documented config is the one in INTEGRATION.md
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert '"class_name": "CLIPModifiedResNet"' in text and '"save_as": "clip-RN50"' in text and "0.48145466" in text


def test_type_clip_is_still_declined_and_points_to_the_config():
    from viquae_amd.image import embedding as IE
    with pytest.raises(NotImplementedError, match="outside the MI355X build") as e:
        IE.get_model_and_transform({"type": "clip", "name": "RN50"})
    assert "CLIPModifiedResNet" in str(e.value)


def test_new_symbols_in_header_table_and_library(hip_lib):
    from viquae_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "meerqat_hip.h")).read()
    assert "clip_resnet.hip" in build.SOURCES
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and hasattr(hip_lib, name), name
