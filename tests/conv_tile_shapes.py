"""Tiles of the two matrix-pipe convolution kernels (conv3x3_x3s_kernel / conv3x3_patch_kernel in csrc/conv.hip, conv1x1_x3s_kernel in
csrc/resnet.hip): the MQ_CONV_TILE_AUTO rules restated, the tile geometry, a walker over the launches of the three convolutional
encoders at a batch B, and the shapes of tests/test_conv_tiles_gpu.py; imports without a GPU.

The rules are restated from include/meerqat_hip.h, run_conv3x3 (conv.hip) and mq_conv1x1_pair_f32 (resnet.hip), with M = B * Ho * Wo
output rows and N output channels:

    3 x 3   N == 64, stride 1, channel-major K, 2 W + 2 <= 256  ->  the patch kernel (256 x 64)
            N % 256 == 0 and ceil(M / 256) * (N / 256) >= 192   ->  256 x 256
            N % 128 == 0                                        ->  512 x 128 if ceil(M / 512) * (N / 128) >= 192 else 256 x 128
            otherwise                                           ->  512 x 64
    1 x 1   N % 256 == 0 and ceil(M / 256) * (N / 256) >= 192   ->  256 x 256
            N % 128 == 0                                        ->  256 x 128
            otherwise                                           ->  512 x 64

A launch has ntm = ceil(M / MT) row blocks and ntn = N / NT column tiles in 8 * per * ntn workgroups, per = ceil(ntm / 8): workgroup b
runs on XCD b & 7, row block (b & 7) * per + (b >> 3) / ntn, column tile (b >> 3) % ntn; the workgroups whose row block is >= ntm (the
padded slots) return at once.

This restatement can drift from the C rules without any test noticing: nothing here reads the library.  That is accepted: what shows
that the shapes below reach the kernels they name is a mutation of one tile instantiation at a time (its lo.hi product skipped), under
which the GPU tests of exactly those shapes fail, and a kernel trace of one model-level test (profiles/conv_tiles_trace.md)."""
import collections

AUTO, T256x256, T512x128, T256x128, T512x64, PATCH = 0, 1, 2, 3, 4, 5   # MQ_CONV_TILE_* (include/meerqat_hip.h)
K_CHANNEL_MAJOR = 0x100                                                 # MQ_CONV_K_CHANNEL_MAJOR
TILE_DIMS = {T256x256: (256, 256), T512x128: (512, 128), T256x128: (256, 128), T512x64: (512, 64), PATCH: (256, 64)}  # rows MT, columns NT
TILE_NAMES = {T256x256: "256x256", T512x128: "512x128", T256x128: "256x128", T512x64: "512x64", PATCH: "patch256x64"}
WIDE_TILES = (T256x256, T512x128)      # what no forward of 8 images launches
PATCH_MAX_W = 127                      # 256 + 2 W + 2 rows fill the patch kernel's 512-row LDS buffer exactly
FULL = 192                             # workgroups that "give every CU a workgroup" in the rules


def out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


def rows(B, H, W, stride):
    Ho, Wo = out_hw(H, W, stride)
    return B * Ho * Wo


def _cdiv(a, b):
    return -(-a // b)


def auto3x3(M, N, stride, W, cmajor=True):
    """what MQ_CONV_TILE_AUTO resolves to in mq_conv3x3_pair_f32 / mq_conv3x3_f16"""
    if N == 64 and stride == 1 and cmajor and W <= PATCH_MAX_W:
        return PATCH
    if N % 256 == 0 and _cdiv(M, 256) * (N // 256) >= FULL:
        return T256x256
    if N % 128 == 0:
        return T512x128 if _cdiv(M, 512) * (N // 128) >= FULL else T256x128
    return T512x64


def auto1x1(M, N):
    """what MQ_CONV_TILE_AUTO resolves to in mq_conv1x1_pair_f32"""
    if N % 256 == 0 and _cdiv(M, 256) * (N // 256) >= FULL:
        return T256x256
    if N % 128 == 0:
        return T256x128
    return T512x64


Geometry = collections.namedtuple("Geometry", "MT NT ntm ntn per padded")


def geometry(tile, M, N):
    """MT, NT, row blocks, column tiles, row blocks per XCD, workgroups launched on padded slots"""
    MT, NT = TILE_DIMS[tile]
    ntm, ntn = _cdiv(M, MT), N // NT
    per = _cdiv(ntm, 8)
    return Geometry(MT, NT, ntm, ntn, per, (8 * per - ntm) * ntn)


def decode(b, g):
    """workgroup b of a launch with geometry g -> (row block, column tile, runs)"""
    mt, nt = (b & 7) * g.per + (b >> 3) // g.ntn, (b >> 3) % g.ntn
    return mt, nt, mt < g.ntm


# ---- the launches of a network at batch B ---------------------------------------------------------------------------------------------
# kernel "conv3x3" | "conv3x3_patch" | "conv1x1";  epilogue of conv3x3: "prelu_pair" | "residual_affine" | "residual";  of conv1x1:
# "relu_pair" | "plain_f32" | "shortcut_f32_pair" | "shortcut_f32" | "shortcut_pair";  tile, input H (= W), N, stride
Launch = collections.namedtuple("Launch", "kernel epilogue tile H N stride")

RESNET_LAYERS = (3, 4, 6, 3)
ARCFACE_LAYERS = (3, 4, 14, 3)
NETWORKS = ("arcface", "resnet", "clip")
DEFAULT_CHUNK = {"arcface": 656, "resnet": 328, "clip": 328}   # the classes' default `chunk`
SHIPPED_BATCH = {"resnet": 256}                                # the shipped imagenet-RN50 config's batch_size


def _l3(B, H, N, stride, epilogue):
    tile = auto3x3(rows(B, H, H, stride), N, stride, H)
    return Launch("conv3x3_patch" if tile == PATCH else "conv3x3", epilogue, tile, H, N, stride)


def _l1(B, H, N, stride, epilogue):
    return Launch("conv1x1", epilogue, auto1x1(rows(B, H, H, stride), N), H, N, stride)


def arcface_launches(B, layers=ARCFACE_LAYERS, size=112):
    """viquae_amd.arcface.ArcFaceR50._forward (both precisions: run_conv3x3<F16> is one function): per IBasicBlock conv1 (PReLU -> pair)
    and conv2 (stride 2 in a stage's first block; + shortcut -> fp32 and the next block's bn1 -> pair).  The strided 1 x 1 downsamples
    and the head are the encoder GEMM's, not these kernels'."""
    out, H = [], size
    blocks = [(64 << s, i) for s, n in enumerate(layers) for i in range(n)]
    for bi, (planes, i) in enumerate(blocks):
        out.append(_l3(B, H, planes, 1, "prelu_pair"))
        stride = 2 if i == 0 else 1
        out.append(_l3(B, H, planes, stride, "residual_affine" if bi + 1 < len(blocks) else "residual"))
        H = out_hw(H, H, stride)[0]
    return out


def _bottlenecks(B, H, layers, clip):
    """viquae_amd.resnet.TorchvisionResNet._stages; clip: the strided blocks keep stride 1 and pool 2 x 2 in front of conv3 / the shortcut"""
    out = []
    blocks = [(s, i) for s, n in enumerate(layers) for i in range(n)]
    for bi, (s, i) in enumerate(blocks):
        width, strided, last = 64 << s, i == 0 and s > 0, bi + 1 == len(blocks)
        next_has_downsample = not last and blocks[bi + 1][1] == 0
        out.append(_l1(B, H, width, 1, "relu_pair"))
        out.append(_l3(B, H, width, 1 if clip or not strided else 2, "prelu_pair"))
        Ho = H // 2 if strided else H
        if i == 0:
            out.append(_l1(B, Ho if clip else H, 4 * width, 1 if clip or not strided else 2, "plain_f32"))
        epi = "shortcut_f32" if last else "shortcut_pair" if next_has_downsample else "shortcut_f32_pair"
        out.append(_l1(B, Ho, 4 * width, 1, epi))
        H = Ho
    return out


def resnet_launches(B, layers=RESNET_LAYERS, size=224):
    return _bottlenecks(B, size // 4, layers, clip=False)


def clip_launches(B, layers=RESNET_LAYERS, size=224):
    """viquae_amd.clip_resnet.CLIPModifiedResNet: the stem's conv2 (32 -> 32 loaded as 32 -> 64) and conv3 (64 -> 64) at size / 2, then the
    bottlenecks"""
    H = size // 2
    return [_l3(B, H, 64, 1, "prelu_pair"), _l3(B, H, 64, 1, "prelu_pair")] + _bottlenecks(B, size // 4, layers, clip=True)


LAUNCHES = {"arcface": arcface_launches, "resnet": resnet_launches, "clip": clip_launches}


def launch_set(net, B):
    return frozenset(LAUNCHES[net](B))


def production_batches(net):
    """the batches whose launch sets a model-level test must reproduce: the class's default chunk and the shipped config's batch"""
    return (DEFAULT_CHUNK[net],) + ((SHIPPED_BATCH[net],) if net in SHIPPED_BATCH else ())


def smallest_production_batch(net):
    """the smallest batch whose launch set is that of every production batch of `net` (None if they differ among themselves)"""
    want = {launch_set(net, B) for B in production_batches(net)}
    if len(want) != 1:
        return None
    want = want.pop()
    return next(B for B in range(1, min(production_batches(net)) + 1) if launch_set(net, B) == want)


# ---- operator-level shapes (tests/test_conv_tiles_gpu.py) --------------------------------------------------------------------------------
# (B, H, W, C, N, stride) and the tile AUTO must resolve to
Conv = collections.namedtuple("Conv", "B H W C N stride tile")

CONV3X3 = [
    Conv(4, 111, 111, 32, 256, 1, T256x256),   # M = 49,284: ntm 193, per 25
    Conv(4, 110, 110, 32, 256, 1, T256x128),   # just below: 190 tiles of either wide kind
    Conv(2, 111, 111, 64, 512, 1, T256x256),   # M = 24,642: ntm 97, per 13, ntn 2
    Conv(2, 221, 221, 64, 512, 2, T256x256),   # the same M at stride 2
    Conv(8, 111, 111, 32, 128, 1, T512x128),   # M = 98,568: ntm 193, per 25
    Conv(8, 221, 221, 32, 128, 2, T512x128),
    Conv(3, 113, 113, 64, 64, 2, T512x64),     # M = 9747: ntm 20
]
CONV3X3_JUST_BELOW = {CONV3X3[1]: CONV3X3[0]}  # shape -> the neighbour one tile count above it
CONV3X3_PATCH = [
    Conv(2, 112, 112, 32, 64, 1, PATCH),       # CLIP's stem conv2: one channel block, 98 row tiles
    Conv(1, 112, 112, 64, 64, 1, PATCH),
    Conv(1, 9, 127, 32, 64, 1, PATCH),         # W = 127: the widest patch
    Conv(1, 9, 128, 32, 64, 1, T512x64),       # W = 128: falls through
]
CONV3X3_F16 = [s for s in CONV3X3 if s.tile in WIDE_TILES and s.stride == 1]   # the three shapes AUTO sends to 256 x 256 and 512 x 128

CONV1X1 = [
    Conv(2, 111, 111, 64, 512, 1, T256x256),   # ntm 97, per 13, ntn 2
    Conv(2, 110, 110, 64, 512, 1, T256x128),   # just below
    Conv(2, 221, 221, 64, 512, 2, T256x256),
    Conv(1, 111, 111, 256, 1024, 1, T256x256),  # ntm 49, per 7, ntn 4
    Conv(1, 77, 77, 512, 2048, 1, T256x256),   # ntm 24, per 3, ntn 8
    Conv(3, 57, 57, 64, 64, 1, T512x64),       # M = 9747: ntm 20
]
CONV1X1_JUST_BELOW = {CONV1X1[1]: CONV1X1[0]}

# mq_im2col_split_f32 past the blockIdx.z carry: 64 rows per workgroup, gridDim.y <= 65535
IM2COL_CARRY = dict(B=1, H=2049, W=2048, C=8, k=1, stride=1, pad=0, kpad=32)
IM2COL_ROWS_PER_BLOCK, GRID_Y_MAX = 64, 65535


def conv_id(s):
    return f"{s.B}x{s.H}x{s.W}x{s.C}-N{s.N}-s{s.stride}"


def conv_rows(s):
    return rows(s.B, s.H, s.W, s.stride)
