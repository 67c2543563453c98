"""The 16x16x32 instance of the screened search's tile kernel (csrc/knn_screen.inc) holds 64 accumulators, 16 + 8 operand
registers and 8 more for the next half-step's fragments against a budget of 128: a spilled register is a scratch reload inside the
K loop, whose wait drains the LDS-DMA.  hipcc's kernel-resource remarks must report no scratch, no spilled VGPR and four waves per
SIMD (tests/test_capi_cpu.py checks the 32x32x16 instance and the streaming kernels the same way)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan16_kernel_does_not_spill():
    src = os.path.join(ROOT, "viquae_amd", "csrc", "knn.hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off",
           "-Wno-unused-result", "--offload-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    cur, seen = None, {}
    for line in out.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]|VGPRs): (\d+)", line)
        if m and cur:
            seen.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    mine = [v for name, v in seen.items() if "screen_scan16_kernel" in name]
    assert len(mine) == 1, sorted(seen)
    assert mine[0]["ScratchSize [bytes/lane]"] == 0 and mine[0]["VGPRs Spill"] == 0, mine[0]
    assert mine[0]["Occupancy [waves/SIMD]"] == 4 and mine[0]["VGPRs"] <= 128, mine[0]
