"""The conditions of the convolution tile tests (tests/test_conv_tiles_gpu.py), checked by arithmetic before anything reaches a GPU:
every operator shape lands in the branch of the AUTO rule it is listed for, the set covers the XCD decode's cases, no forward of 8 images
launches a wide tile, and the batch of the model-level tests is the smallest one with the production launch set."""
import pytest

from tests import conv_tile_shapes as S


def _auto(kernel, s):
    M = S.conv_rows(s)
    return S.auto3x3(M, s.N, s.stride, s.W) if kernel == "3x3" else S.auto1x1(M, s.N)


def test_every_operator_shape_lands_in_its_branch():
    for kernel, shapes in (("3x3", S.CONV3X3 + S.CONV3X3_PATCH), ("1x1", S.CONV1X1)):
        for s in shapes:
            assert s.C % 32 == 0 and s.N % 64 == 0 and s.stride in (1, 2), s
            assert _auto(kernel, s) == s.tile, (kernel, s, S.TILE_NAMES[_auto(kernel, s)])
            assert s.N % S.TILE_DIMS[s.tile][1] == 0, s
    # a "just below" partner: the same N, C and stride, fewer rows, the neighbouring branch -- and one tile count short of FULL
    for kernel, partners in (("3x3", S.CONV3X3_JUST_BELOW), ("1x1", S.CONV1X1_JUST_BELOW)):
        assert partners
        for below, above in partners.items():
            assert (below.C, below.N, below.stride) == (above.C, above.N, above.stride) and S.conv_rows(below) < S.conv_rows(above)
            assert above.tile == S.T256x256 and below.tile == S.T256x128 and _auto(kernel, below) == S.T256x128
            full = lambda s: -(-S.conv_rows(s) // 256) * (s.N // 256)  # noqa: E731
            assert S.FULL - 8 <= full(below) < S.FULL <= full(above) < S.FULL + 8
    # the 512 x 128 branch has the same threshold; its neighbour below is 256 x 128 as well
    assert S.auto3x3(S.rows(8, 110, 110, 1), 128, 1, 110) == S.T256x128
    # stride 2 and stride 1 partners have the same rows, so the same geometry
    assert S.conv_rows(S.CONV3X3[3]) == S.conv_rows(S.CONV3X3[2]) and S.conv_rows(S.CONV3X3[5]) == S.conv_rows(S.CONV3X3[4])
    assert S.conv_rows(S.CONV1X1[2]) == S.conv_rows(S.CONV1X1[0])
    # the patch kernel: the rule's W limit fills the 512-row buffer exactly, and one more pixel falls through
    assert 256 + 2 * S.PATCH_MAX_W + 2 == 512
    assert {s.W for s in S.CONV3X3_PATCH if s.tile == S.PATCH} >= {112, S.PATCH_MAX_W}
    assert [s.tile for s in S.CONV3X3_PATCH if s.W == S.PATCH_MAX_W + 1] == [S.T512x64]
    assert S.auto3x3(1000, 64, 1, 56, cmajor=False) == S.T512x64 and S.auto3x3(1000, 64, 2, 56) == S.T512x64
    # the fp16 kernel takes the three stride-1 shapes of the wide tiles
    assert sorted(s.tile for s in S.CONV3X3_F16) == [S.T256x256, S.T256x256, S.T512x128]
    assert len({S.conv_id(s) for s in S.CONV3X3 + S.CONV3X3_PATCH}) == len(S.CONV3X3 + S.CONV3X3_PATCH)
    assert len({S.conv_id(s) for s in S.CONV1X1}) == len(S.CONV1X1)


def test_the_shape_set_covers_the_decode():
    geo = {}
    for kernel, shapes in (("3x3", S.CONV3X3 + S.CONV3X3_PATCH), ("1x1", S.CONV1X1)):
        for s in shapes:
            geo.setdefault((kernel, s.tile), []).append((S.conv_rows(s), S.geometry(s.tile, S.conv_rows(s), s.N)))
    everything = [g for v in geo.values() for g in v]
    assert {g.ntn for _, g in everything} >= {1, 2, 4, 8}
    # each wide tile of each kernel: several row blocks per XCD, a row-block count that is no multiple of 8 (padded slots that must
    # return), a ragged last row block
    for key in (("3x3", S.T256x256), ("3x3", S.T512x128), ("1x1", S.T256x256)):
        assert any(g.per > 1 and g.ntm % 8 != 0 and g.padded > 0 and M % g.MT != 0 for M, g in geo[key]), key
    assert {g.ntn for _, g in geo[("3x3", S.T256x256)]} >= {1, 2}
    assert {g.ntn for _, g in geo[("1x1", S.T256x256)]} >= {2, 4, 8}
    assert any(g.ntm % 8 == 0 and g.per > 1 for _, g in geo[("1x1", S.T256x256)])       # and one with no padded slot
    # the figures the shape lists quote
    assert S.geometry(S.T256x256, S.conv_rows(S.CONV3X3[0]), 256)[2:5] == (193, 1, 25)
    assert S.geometry(S.T256x256, S.conv_rows(S.CONV3X3[2]), 512)[2:5] == (97, 2, 13)
    assert S.geometry(S.T512x128, S.conv_rows(S.CONV3X3[4]), 128)[2:5] == (193, 1, 25)
    assert S.geometry(S.T512x64, S.conv_rows(S.CONV3X3[6]), 64).ntm == 20
    assert S.geometry(S.PATCH, S.conv_rows(S.CONV3X3_PATCH[0]), 64).ntm == 98
    assert S.geometry(S.T256x256, S.conv_rows(S.CONV1X1[3]), 1024)[2:5] == (49, 4, 7)
    assert S.geometry(S.T256x256, S.conv_rows(S.CONV1X1[4]), 2048)[2:5] == (24, 8, 3)
    assert S.geometry(S.T512x64, S.conv_rows(S.CONV1X1[5]), 64).ntm == 20
    # the decode: every (row block, column tile) exactly once, the padded slots and nothing else skipped
    for M, g in everything:
        seen = [S.decode(b, g) for b in range(8 * g.per * g.ntn)]
        run = [(mt, nt) for mt, nt, ok in seen if ok]
        assert sorted(run) == [(mt, nt) for mt in range(g.ntm) for nt in range(g.ntn)] and len(seen) - len(run) == g.padded, (M, g)
    # the im2col carry: more row blocks than one grid dimension holds
    c = S.IM2COL_CARRY
    M = S.rows(c["B"], c["H"] + 2 * c["pad"] - c["k"] + 1, c["W"] + 2 * c["pad"] - c["k"] + 1, c["stride"])
    assert -(-M // S.IM2COL_ROWS_PER_BLOCK) > S.GRID_Y_MAX and c["kpad"] % 32 == 0 and c["k"] ** 2 * c["C"] <= c["kpad"]


@pytest.mark.parametrize("net", S.NETWORKS)
def test_eight_images_launch_no_wide_tile_and_production_batches_do(net):
    for B in range(1, 9):
        assert not {l.tile for l in S.LAUNCHES[net](B)} & set(S.WIDE_TILES), (net, B)
    for B in S.production_batches(net):
        tiles = {(l.kernel, l.tile) for l in S.LAUNCHES[net](B)}
        assert ("conv3x3", S.T256x256) in tiles and ("conv3x3", S.T512x128) in tiles, (net, B)
        assert (("conv1x1", S.T256x256) in tiles) == (net != "arcface"), (net, B)
        assert any(l.kernel == "conv3x3_patch" for l in S.LAUNCHES[net](B))      # the 64-channel stage of all three
    # the walkers list what the networks have: 24 IBasicBlocks of two 3 x 3s; 16 bottlenecks of three convolutions + 4 downsamples
    assert len(S.arcface_launches(8)) == 48 and len(S.resnet_launches(8)) == 52 and len(S.clip_launches(8)) == 54
    assert {l.stride for l in S.clip_launches(8)} == {1} and {l.stride for l in S.resnet_launches(8)} == {1, 2}
    # 1 x 1 launches of the two ResNets at a production batch: 15 of the 19 distinct (epilogue, H, N, stride) on 256 x 256, every
    # epilogue form among them; at 8 images all 19 run 256 x 128 or 512 x 64
    if net != "arcface":
        one = {l for l in S.LAUNCHES[net](S.DEFAULT_CHUNK[net]) if l.kernel == "conv1x1"}
        wide = {l for l in one if l.tile == S.T256x256}
        assert len(one) == 19 and len(wide) == 15, (net, sorted(one))
        assert {l.epilogue for l in wide} == {"relu_pair", "plain_f32", "shortcut_f32_pair", "shortcut_f32", "shortcut_pair"}


@pytest.mark.parametrize("net", S.NETWORKS)
def test_the_model_level_batch_is_the_smallest_with_the_production_launch_set(net):
    B = S.smallest_production_batch(net)
    assert B is not None, "the production batches of one network launch different sets"
    want = S.launch_set(net, S.DEFAULT_CHUNK[net])
    assert S.launch_set(net, B) == want and S.launch_set(net, B - 1) != want
    for P in S.production_batches(net):
        assert S.launch_set(net, P) == want and B <= P
    # the rules are monotonic in the rows: nothing changes between that batch and the largest chunk
    assert all(S.launch_set(net, b) == want for b in range(B, S.DEFAULT_CHUNK[net] + 1))
    # small enough for a test: a fraction of a chunk more than the launch set needs would only cost time
    assert B < S.DEFAULT_CHUNK[net]
