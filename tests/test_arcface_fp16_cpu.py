"""CPU suite for the opt-in fp16 face encoder (ArcFaceR50(precision="fp16")): ABI declared / exported / bound, the precision
switch's validation, the new kernels free of scratch, and the torch statement of the autocast schedule (tests/autocast_schedule.py)
against the golden file's ``embeddings_fp16_autocast``."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import autocast_schedule as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mq_conv3x3_f16", "mq_stem_conv3x3_f16", "mq_conv1x1_f16", "mq_head_prep_f16")


def test_fp16_entries_are_declared_exported_and_bound(hip_lib):
    from viquae_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "meerqat_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(rf"\b{n}\s*\(", header), n
        assert hasattr(hip_lib, n), n
        assert n in _lib.SIGNATURES, n


def test_fp16_entries_check_their_arguments(hip_lib):
    """argument checks happen before any HIP call: MQ_EINVAL (-1) on a bad channel count, stride or epilogue, bad tile"""
    p = 16  # any non-null pointer value: nothing is dereferenced on these paths
    conv = hip_lib.mq_conv3x3_f16
    assert conv(p, 1, 8, 8, 48, 1, p, 64, p, p, p, None, None, None, None, p, p, 0, None) == -1        # C % 32
    assert conv(p, 1, 8, 8, 64, 3, p, 64, p, p, p, None, None, None, None, p, p, 0, None) == -1        # stride
    assert conv(p, 1, 8, 8, 64, 1, p, 96, p, p, p, None, None, None, None, p, p, 0, None) == -1        # N % 64
    assert conv(p, 1, 8, 8, 64, 1, p, 64, p, p, p, p, None, None, None, p, p, 0, None) == -1           # PReLU with a residual
    assert conv(p, 1, 8, 8, 64, 1, p, 64, p, p, None, None, None, None, p, p, p, 0, None) == -1        # residual epilogue without R
    assert conv(p, 1, 8, 8, 64, 1, p, 64, p, p, p, None, None, None, None, p, p, 9, None) == -1        # unknown tile
    assert conv(p, 1, 8, 8, 64, 1, p, 64, p, p, p, None, None, None, None, p, p, 1, None) == -1        # 256 columns, N = 64
    assert conv(p, 1, 8, 8, 64, 2, p, 64, p, p, p, None, None, None, None, p, p, 0x105, None) == -1    # the patch tile at stride 2
    assert conv(p, 1, 8, 8, 64, 1, p, 64, p, p, p, None, None, None, None, p, p, 5, None) == -1        # patch needs channel-major K
    assert conv(p, 0, 8, 8, 64, 1, p, 64, p, p, p, None, None, None, None, p, p, 0, None) == 0         # B = 0: nothing to do
    assert hip_lib.mq_conv1x1_f16(p, 1, 8, 8, 40, 2, p, 64, p, p, p, None) == -1
    assert hip_lib.mq_conv1x1_f16(p, 1, 8, 8, 64, 3, p, 64, p, p, p, None) == -1
    assert hip_lib.mq_stem_conv3x3_f16(p, 1, 8, 6, p, p, p, p, p, p, p, p, None) == -4               # W % 4: MQ_EUNSUPPORTED
    assert hip_lib.mq_stem_conv3x3_f16(p, 1, 8, 8, p, None, p, p, p, p, p, p, None) == -1
    assert hip_lib.mq_head_prep_f16(p, 1, 49, 500, p, p, p, p, None) == -1


def test_precision_is_validated(monkeypatch):
    from oracle import arcface as oa
    from viquae_amd.arcface import ArcFaceR50
    from viquae_amd.image import face_recognition as fr
    state = oa.seeded_state(0)
    assert ArcFaceR50(state).precision == "fp32"
    m = ArcFaceR50.from_state_dict(state, precision="fp16")
    assert m.precision == "fp16" and m.layer3_13_conv2_w16.dtype == torch.int16
    w = np.asarray(state["layer1.0.conv1.weight"], np.float32)
    want = torch.from_numpy(w.transpose(0, 2, 3, 1).reshape(64, -1).astype(np.float16))
    from viquae_amd.encoders import _untile
    assert torch.equal(_untile(m.layer1_0_conv1_w16, 64, 576).view(torch.float16), want)  # unfolded: bn2 is not in the weights
    # an fp16 model holds the weights of its own precision only: of the folded fp32 weights and biases, only the shared head's
    assert {n for n, _ in m.named_buffers() if n.endswith(("_w2", "_b"))} == {"fc_w2", "fc_b"}
    for bad in ("bf16", "FP16", None, 16):
        with pytest.raises(ValueError):
            ArcFaceR50(state, precision=bad)
    # from_pretrained: argument, then MQ_ARCFACE_PRECISION, then fp32; fp16 precision needs the reference's fp16 switch
    seen = []
    monkeypatch.setattr(ArcFaceR50, "from_pretrained", classmethod(lambda cls, path, **kw: seen.append(kw["precision"]) or torch.nn.Module()))
    monkeypatch.delenv("MQ_ARCFACE_PRECISION", raising=False)
    fr.from_pretrained()
    fr.from_pretrained(precision="fp16")
    monkeypatch.setenv("MQ_ARCFACE_PRECISION", "fp16")
    fr.from_pretrained()
    fr.from_pretrained(precision="fp32")
    assert seen == ["fp32", "fp16", "fp16", "fp32"]
    with pytest.raises(ValueError):
        fr.from_pretrained(fp16=False)                       # fp16 from the environment, autocast switched off
    monkeypatch.setenv("MQ_ARCFACE_PRECISION", "half")
    with pytest.raises(ValueError):
        fr.from_pretrained()
    monkeypatch.delenv("MQ_ARCFACE_PRECISION")
    with pytest.raises(ValueError):
        fr.from_pretrained(fp16=False, precision="fp16")
    assert fr.from_pretrained(fp16=False) is not None and seen[-1] == "fp32"


def test_fp16_kernels_do_not_spill():
    """hipcc's kernel-resource remarks for every instance of the fp16 kernels (a spill inside the K loop would drain the LDS-DMA
    ring)."""
    src = os.path.join(ROOT, "viquae_amd", "csrc", "conv.hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off",
           "-Wno-unused-result", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    cur, seen = None, {}
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            seen[cur] = int(m.group(1))
    expected = {f"_ZN12_GLOBAL__N_118conv3x3_x3s_kernelILi{rg}ELi{wn}ELi{ep}ELb1EEEvNS_8ConvArgsE"
                for rg, wn in ((4, 64), (8, 64), (4, 32), (8, 32)) for ep in (0, 1)}
    expected |= {f"_ZN12_GLOBAL__N_120conv3x3_patch_kernelILi{ep}ELb1EEEvNS_8ConvArgsE" for ep in (0, 1)}
    expected |= {"_ZN12_GLOBAL__N_120stem_conv_f16_kernelEPKfS1_S1_S1_S1_S1_S1_PtS2_iii",
                 "_ZN12_GLOBAL__N_118conv1x1_f16_kernelEPKtiiiiiiiS1_iPKfS3_Pt",
                 "_ZN12_GLOBAL__N_120head_prep_f16_kernelEPKtiiiPKfS3_PtS4_"}
    assert expected <= set(seen), sorted(expected - set(seen))
    # the raster instances keep the 12 bytes of stack their fp32 twins have always had (the K-walk counters the DMA lambda
    # updates), no more; every other fp16 kernel has none
    twins = {k: k.replace("ELb1E", "ELb0E") for k in expected if "x3s" in k}
    assert all(seen[k] <= seen[t] <= 12 for k, t in twins.items()), {k: (seen[k], seen[t]) for k, t in twins.items()}
    assert all(seen[k] == 0 for k in expected - set(twins)), {k: seen[k] for k in expected if seen[k]}


def test_schedule_reproduces_the_golden_fp16_autocast_embeddings():
    """tests/autocast_schedule.py, in fp32 between the roundings, against tools/make_golden_arcface.py's fp16 statement"""
    from oracle import arcface as oa
    g = np.load(os.path.join(ROOT, "tests", "golden", "arcface_r50_8.npz"))
    state = {k: torch.from_numpy(v) for k, v in oa.seeded_state(int(g["seed_weights"])).items()}
    x = (torch.from_numpy(g["faces_u8"]).permute(0, 3, 1, 2).to(torch.float32).div(255.0) - 0.5) / 0.5
    with torch.no_grad():
        y = ac.forward(state, x).numpy()
    assert np.abs(y - g["embeddings_fp16_autocast"]).max() <= 1e-5
    assert np.abs(y - g["embeddings"]).max() > 1e-3   # and it is not the fp32 forward
