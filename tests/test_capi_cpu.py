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
