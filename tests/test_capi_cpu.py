"""CPU suite: libmeerqat_hip.so builds for gfx950, loads without a GPU, and exports every symbol that
include/meerqat_hip.h declares (no compute calls here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "meerqat_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mq_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported(hip_lib):
    names = _declared()
    assert len(names) >= 12
    for n in names:
        assert hasattr(hip_lib, n), f"{n} declared in include/meerqat_hip.h but not exported"


def test_binding_table_covers_header(hip_lib):
    from viquae_amd import _lib
    assert sorted(_lib.SIGNATURES) == _declared()


def test_host_only_entries(hip_lib):
    assert b"gfx950" in hip_lib.mq_version()
    assert hip_lib.mq_padded_rows(1) == 256 and hip_lib.mq_padded_rows(257) == 512
    assert hip_lib.mq_padded_dim(768) == 768 and hip_lib.mq_padded_dim(100) == 112
    assert hip_lib.mq_packed_bytes(1_500_000, 768) == 1_500_160 * 768 * 4
    assert hip_lib.mq_strerror(-2) == b"workspace too small"
    # argument validation happens before any HIP call
    assert hip_lib.mq_knn_search_f32(None, None, 10, 8, None, 1, 5, 0, 0, 0, None, None, None, 0, None) == -1
    assert hip_lib.mq_knn_workspace_bytes(1000, 64, 10, 4096) == 0  # k above MQ_KNN_MAX_K


def test_code_object_is_gfx950():
    from viquae_amd import build
    data = open(build.SO, "rb").read()
    assert b"gfx950" in data and b"knn_scan_kernel" in data


def test_product_does_not_import_oracle():
    """The product path must never route through the oracle (or any CPU fallback)."""
    pkg = os.path.join(ROOT, "viquae_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports the oracle"


def test_search_path_switches_are_set_through_the_abi(hip_lib):
    """the A/B switches are process-wide atomics behind mq_knn_set_option / mq_knn_get_option (first values from the
    environment, read once) -- not getenv() on the search path."""
    from viquae_amd import _lib
    assert hip_lib.mq_knn_get_option(_lib.KNN_OPT_SMALL_SCAN) in (0, 1)
    before = hip_lib.mq_knn_get_option(_lib.KNN_OPT_PARTITIONS)
    with _lib.knn_option(_lib.KNN_OPT_PARTITIONS, 0) as o:
        assert o.previous == before and hip_lib.mq_knn_get_option(_lib.KNN_OPT_PARTITIONS) == 0
        # the planner follows the switch at once: k = 300 over 1.5M rows is served over row ranges, or by exact rounds
        assert hip_lib.mq_knn_screen_scan_kind(1_500_000, 768, 4096, 300, 0) == 0
    assert hip_lib.mq_knn_get_option(_lib.KNN_OPT_PARTITIONS) == before
    if before:
        assert hip_lib.mq_knn_screen_scan_kind(1_500_000, 768, 4096, 300, 0) == 1
    assert hip_lib.mq_knn_set_option(99, 1) == -1 and hip_lib.mq_knn_set_option(0, -5) == -1 and hip_lib.mq_knn_get_option(-1) == -1


def test_streaming_kernels_do_not_spill():
    """The streaming scans keep queries in registers and an LDS-DMA ring in flight: a spilled register is a scratch reload inside
    the loop, whose `s_waitcnt vmcnt(0)` drains the ring every item.  The 12-K-block instances sit at the
    register limit (two waves per SIMD: 128 + 128), so the invariant is checked at build time: hipcc's kernel-resource remarks must
    report no scratch for every instance of the streaming kernel and for the 256 x 256 tile kernel."""
    import subprocess
    src = os.path.join(ROOT, "viquae_amd", "csrc", "knn.hip")
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
    # every streaming instance ("screen_small" matches no kernel but screen_small8_kernel: round 4's one-wave kernel is retired)
    watched = {k: v for k, v in seen.items() if "screen_small" in k or "screen_scan_kernel" in k}
    expected = {"_ZN12_GLOBAL__N_118screen_scan_kernelENS_10ScreenArgsE"}
    expected |= {f"_ZN12_GLOBAL__N_120screen_small8_kernelILi{nkb}ELb0EEEvNS_9SmallArgsE" for nkb in range(1, 13)}
    expected.add("_ZN12_GLOBAL__N_120screen_small8_kernelILi12ELb1EEEvNS_9SmallArgsE")  # the ROWTERM instance
    assert set(watched) == expected and len(expected) == 14, sorted(watched)
    assert all(v == 0 for v in watched.values()), {k: v for k, v in watched.items() if v}


_FAILING_LAUNCHES = r"""
import ctypes, json
from viquae_amd import _lib
lib = _lib.load()
buf = ctypes.create_string_buffer(4096)
p = (ctypes.addressof(buf) + 15) & ~15          # a non-null, 16-byte-aligned placeholder: without a device nothing reads it
calls = {
    # conv.hip: a plain launch, and one that raises the kernel's dynamic LDS first
    "mq_head_prep_f16": lambda: lib.mq_head_prep_f16(p, 1, 1, 32, p, p, p, p, None),
    "mq_conv3x3_pair_f32": lambda: lib.mq_conv3x3_pair_f32(p, p, 1, 2, 2, 32, 1, p, p, 64, p, p, None, None, None, None, p, p, p, 0, None),
    # resnet.hip: likewise
    "mq_pool_hw_f32": lambda: lib.mq_pool_hw_f32(p, 1, 4, 8, 0, p, None),
    "mq_conv1x1_pair_f32": lambda: lib.mq_conv1x1_pair_f32(p, p, 1, 2, 2, 32, 1, p, p, 64, p, None, 0, p, None, None, p, 0, None),
    # clip_resnet.hip, diag.hip
    "mq_avgpool2x2_pair_f32": lambda: lib.mq_avgpool2x2_pair_f32(p, p, 1, 2, 2, 32, p, p, None),
    "mq_diag_mfma_bf16_dot": lambda: lib.mq_diag_mfma_bf16_dot(p, p, 16, p, None),
}
out = {"initial": lib.mq_last_hip_error()}
for name, call in calls.items():
    lib.mq_internal_set_hip_error(0)
    out[name] = [call(), lib.mq_last_hip_error()]
print(json.dumps(out))
"""


def test_hip_failures_are_recorded():
    """MQ_EHIP promises "see mq_last_hip_error()": every entry reports a failing HIP call through MQ_HIP / mq_launch_status
    (csrc/host_check.h), which record the error.  Without a device every launch fails, so entries of conv.hip, resnet.hip,
    clip_resnet.hip and diag.hip -- whose bare `hipGetLastError() == hipSuccess ? ...` returns recorded nothing -- are called with
    arguments that clear validation, in a child process (the error is thread-local and starts at 0)."""
    import json
    import subprocess
    import sys
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU: there every launch fails")
    from viquae_amd import build
    build.build()
    res = subprocess.run([sys.executable, "-c", _FAILING_LAUNCHES], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out.pop("initial") == 0
    assert len(out) == 6
    for name, (code, err) in out.items():
        assert code == -3 and err != 0, (name, code, err)   # MQ_EHIP, and the hipError_t behind it


def test_shared_helpers_are_defined_once():
    """The device helpers that define the library's data layout (csrc/device_common.h, csrc/x3_tile.h) and the HIP error path
    (csrc/host_check.h) have one definition: no translation unit grows its own copy again."""
    csrc = os.path.join(ROOT, "viquae_amd", "csrc")
    names = "pair_index|split1|split8|split4|split_bits|join8|store_split_pair|lds_addr_of|dma16s|dma16v|wave_sum|wave_min|wave_max"
    units = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".inc")))
    assert len(units) >= 16
    for f in units:
        src = open(os.path.join(csrc, f)).read()
        m = re.search(r"^[ \t]*(?:template\s*<[^>]*>\s*)?(?:static\s+|inline\s+|__device__\s+|__host__\s+|__forceinline__\s+)+"
                      r"[\w:<>\*&\s]+?\b(" + names + r")\s*\([^;{]*\)\s*\{", src, flags=re.M)
        assert not m, f"{f} defines {m.group(1)}: it belongs to the shared headers"
        assert not re.search(r"typedef[^;]*\b(bf16x8_t|bf16x4_t|f32x16|lds_char)\s*(__attribute__[^;]*)?;", src), f"{f}: a shared typedef"
        assert not re.search(r"#\s*define\s+\w+_HIP\(call\)", src), f"{f} defines its own HIP check macro"
        assert "hipGetLastError() == hipSuccess" not in src, f"{f} returns a launch status without recording the error"
        assert "mq_internal_set_hip_error(int" not in src or f == "knn.hip", f"{f} re-declares mq_internal_set_hip_error"
