"""GPU: the tiles of conv3x3_x3s_kernel / conv3x3_patch_kernel (csrc/conv.hip) and conv1x1_x3s_kernel (csrc/resnet.hip) that the
production batches launch and no forward of 8 images does -- 256 x 256 and 512 x 128, with several row blocks per XCD, row-block counts
that are no multiple of 8, 1 to 8 column tiles and ragged last row blocks (tests/conv_tile_shapes.py; its conditions are checked on the
CPU by tests/test_conv_tile_shapes_cpu.py).

Operator level: each shape under MQ_CONV_TILE_AUTO and under the tile AUTO must pick, in the K order the models use
(MQ_CONV_K_CHANNEL_MAJOR), against float64 torch on the values the kernel reads (nine shifted matrix products), every epilogue form,
within PAIR_TOL = 2e-5 x max |reference| (three fp32-accumulated bf16 products and the 16-bit output pair emulated on a CPU against
float64 at K = 288, 2048, 4608 stay at 4.7e-6 ... 6.2e-6 x max |reference|: the reference alone is a factor 3 inside).  Outputs are
filled with NaN bit patterns before the launch: every element of the rows < M must be written.

Model level: one forward at the smallest batch with the production launch set equals, bit for bit, the forwards over chunks of 8 images
(the tiles the golden tests pin): every tile walks an output's K range in the same order and the heads' split counts are fixed."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import autocast_schedule as ac
from tests import conv_tile_shapes as S
from tests.test_arcface_fp16_gpu import _check, _dev16, _f32, _host16, _pre, _rng_params

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PAIR_TOL = 2e-5      # tests/test_resnet_gpu.py's: hi + lo keeps 16 mantissa bits, times max |reference|
K_ORDER_TOL = 1e-5   # tests/test_arcface_gpu.py's: the two K orders sum the same products


def _pair(x2d):
    from viquae_amd.encoders import SplitAct, split_bf16
    return SplitAct(*split_bf16(x2d.contiguous()))


def _nan_pair(M, N):
    """a pair output whose every bf16 is 0xFFFF, a NaN"""
    from viquae_amd.encoders import SplitAct
    P = SplitAct.empty(M, N, "cuda")
    P.hi.fill_(-1), P.lo.fill_(-1)
    return P


def _nan_f32(M, N):
    return torch.full((M, N), float("nan"), device="cuda")


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _bf16_values(t):
    """fp32 values that are bf16 values: with such a scale and shift, Y * scale + shift is exact in float64, so its rounding to fp32 is
    the kernel's fused multiply-add"""
    return t.bfloat16().float()


def _split(v):
    """the (hi, lo) bf16 pair of fp32 v, as the kernels make it"""
    hi = v.bfloat16()
    return hi, (v - hi.float()).bfloat16()


def _assert_close(got, ref, what):
    """every element written (no NaN left) and within PAIR_TOL x max |ref| of the float64 reference"""
    assert got.shape == ref.shape, what
    assert not torch.isnan(got).any(), f"{what}: elements of the rows < M were not written"
    err, tol = float((got.double() - ref).abs().max()), PAIR_TOL * float(ref.abs().max())
    print(f"{what}: max err {err:.3e} tol {tol:.3e}")
    assert err <= tol, what


def _assert_same_pair(a, b, what):
    for x, y in zip(a.rowmajor(), b.rowmajor()):
        assert torch.equal(x, y), what


def _conv3x3_f64(xv, w2, bias, stride):
    """float64 3 x 3 convolution, padding 1, as nine shifted matrix products: xv [B, H, W, C] float64, w2 fp32 [N, 9 C] with column
    (kh * 3 + kw) * C + c -> [B * Ho * Wo, N]"""
    B, H, W, C = xv.shape
    Ho, Wo = S.out_hw(H, W, stride)
    xp = F.pad(xv, (0, 0, 1, 1, 1, 1))
    out = bias.double().expand(B * Ho * Wo, -1).clone()
    for t in range(9):
        kh, kw = divmod(t, 3)
        a = xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride].reshape(B * Ho * Wo, C)
        out += a @ w2[:, t * C:(t + 1) * C].double().T
    return out


@pytest.mark.parametrize("s", S.CONV3X3 + S.CONV3X3_PATCH, ids=S.conv_id)
def test_conv3x3_pair_tiles_against_float64(s):
    """mq_conv3x3_pair_f32, channel-major K: PReLU -> pair (real slopes; zero slopes = the ResNets' ReLU), residual -> Y and pair =
    split(Y * scale + shift), residual -> Y alone; AUTO and the explicit tile give the same bits; the pair is the split of the very Y"""
    from viquae_amd import _lib
    from viquae_amd.encoders import split_bf16_tiled
    lib = _lib.load()
    B, H, W, C, N, stride = s[:6]
    M = S.conv_rows(s)
    g = torch.Generator(device="cuda").manual_seed(H * 1000 + C + N + stride)
    X = _pair(torch.randn((B * H * W, C), generator=g, device="cuda"))
    w2 = torch.randn((N, 9 * C), generator=g, device="cuda") * 0.05
    bias = torch.randn(N, generator=g, device="cuda")
    slope = torch.rand(N, generator=g, device="cuda") * 0.4
    relu = torch.zeros(N, device="cuda")
    scale = _bf16_values(torch.rand(N, generator=g, device="cuda") + 0.5)
    shift = _bf16_values(torch.randn(N, generator=g, device="cuda"))
    res = torch.randn((M, N), generator=g, device="cuda")
    ws = split_bf16_tiled(w2)
    zeros = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    lin = _conv3x3_f64(X.float().double().view(B, H, W, C), w2, bias, stride)   # the pair's values: what the kernel reads
    assert lin.shape == (M, N)

    def run(tile, slope=None, res=None, scale=None, shift=None):
        Y = _nan_f32(M, N) if slope is None else None
        P = _nan_pair(M, N) if slope is not None or scale is not None else None
        _lib.check(lib.mq_conv3x3_pair_f32(X.hi.data_ptr(), X.lo.data_ptr(), B, H, W, C, stride, ws[0].data_ptr(), ws[1].data_ptr(), N,
                                           bias.data_ptr(), _ptr(slope), _ptr(res), _ptr(scale), _ptr(shift), _ptr(Y),
                                           P.hi.data_ptr() if P else None, P.lo.data_ptr() if P else None, zeros.data_ptr(), tile, st),
                   "mq_conv3x3_pair_f32")
        return Y, P
    forms = {"prelu": dict(slope=slope), "relu": dict(slope=relu), "residual + affine": dict(res=res, scale=scale, shift=shift),
             "residual": dict(res=res)}
    tag = f"conv3x3 {S.conv_id(s)} {S.TILE_NAMES[s.tile]}"
    auto = {k: run(S.AUTO | S.K_CHANNEL_MAJOR, **kw) for k, kw in forms.items()}
    _assert_close(auto["prelu"][1].float(), torch.where(lin >= 0, lin, lin * slope.double()), tag + " prelu P")
    _assert_close(auto["relu"][1].float(), lin.clamp_min(0), tag + " relu P")
    ref_y = lin + res.double()
    Y, P = auto["residual + affine"]
    _assert_close(Y, ref_y, tag + " residual Y")
    _assert_close(P.float(), ref_y * scale.double() + shift.double(), tag + " residual P")
    _assert_close(auto["residual"][0], ref_y, tag + " residual Y alone")
    assert torch.equal(auto["residual"][0], Y), tag                 # the shortcut does not depend on the pair output
    # the pair is split(fma(Y, scale, shift)) of the very fp32 Y (exact in float64, see _bf16_values: one rounding, to fp32)
    hi, lo = _split((Y.double() * scale.double() + shift.double()).float())
    ph, pl = P.rowmajor()
    assert torch.equal(ph.view(torch.bfloat16), hi) and torch.equal(pl.view(torch.bfloat16), lo), tag
    del lin, ref_y, hi, lo, ph, pl
    # AUTO picked the tile the branch names: the same bits as with that tile asked for
    for k, kw in forms.items():
        Ye, Pe = run(s.tile | S.K_CHANNEL_MAJOR, **kw)
        if Ye is not None:
            assert torch.equal(Ye, auto[k][0]), (tag, k)
        if Pe is not None:
            _assert_same_pair(Pe, auto[k][1], (tag, k))
    if s.tile == S.PATCH:   # the patch kernel gives the bits of the channel-major gather
        for k in ("prelu", "residual + affine"):
            Yg, Pg = run(S.T512x64 | S.K_CHANNEL_MAJOR, **forms[k])
            assert Yg is None or torch.equal(Yg, auto[k][0]), (tag, k)
            _assert_same_pair(Pg, auto[k][1], (tag, k, "gather"))
    # the two K orders: the same products summed in another order
    Yt, _ = run(S.T512x64 if s.tile == S.PATCH else s.tile, res=res)
    assert not torch.isnan(Yt).any()
    assert float((Yt - Y).abs().max()) <= K_ORDER_TOL * float(Y.abs().max()), tag


@pytest.mark.parametrize("s", S.CONV3X3_F16, ids=S.conv_id)
def test_conv3x3_f16_tiles_follow_the_autocast_schedule(s):
    """mq_conv3x3_f16 on the shapes AUTO sends to 256 x 256 and 512 x 128: tests/test_arcface_fp16_gpu.py's reference and per-element ulp
    tolerances, unchanged; AUTO and the explicit tile give the same bits.

    Inputs and weights are normal deviates rounded to multiples of 2^-8: every product is a multiple of 2^-16 and every partial sum
    stays below 2^8 (asserted), 24 bits, so fp32 accumulation is exact in any order and grouping.  The trade-off: a wrong, missing or
    doubled product anywhere in these row blocks shows undiluted, but these row counts see no full-mantissa data at operator level;
    the wide tiles get that at up to 6272 rows in tests/test_arcface_fp16_gpu.py and at 497 faces in the model-level test below.
    The 0.005 % of outputs that still differ are affine results within half an fp32 ulp of an fp16 tie: torch converts float64 to
    fp16 through fp32 and so rounds the reference twice there.

    Why not that file's inputs: its tolerance allows one fp16 ulp of r(acc), and fp32 accumulation keeps a sum within about
    2^-24 x sum |x w| of the exact one, which is more than an fp16 ulp of a sum that cancelled below 2^-13.  A hundred times more
    outputs than that file's (12.6 M per shape) meet such sums.  Correctly rounded fp32 accumulation of the full-mantissa inputs,
    emulated on a CPU with one rounding per 4 products and per product (a plain FMA chain), leaves r(acc) more than one ulp from
    r(float64 sum) on 380 ... 745 and 989 ... 1619 outputs of the three shapes.  Without any 3e4 channel the worst |error| / tolerance
    of "conv1+bn2+prelu" is then 0.998 ... 0.999 and 0.999 ... 1.066: no margin, one miss.  With the two 3e4 channels (they put +-inf
    into the outputs, which must land where the reference's does) (8, 111, 111, 32 -> 128) misses on two and three outputs."""
    from viquae_amd import _lib
    from viquae_amd.encoders import _tile, _untile
    lib = _lib.load()
    B, H, W, C, N, stride = s[:6]
    M = S.conv_rows(s)
    rng = np.random.default_rng(H * 7 + C + N)
    grid = lambda a: (np.rint(a * 256) / 256).astype(np.float16).astype(np.float64)  # noqa: E731
    x = grid(rng.standard_normal((B, H, W, C)))
    w = grid(rng.standard_normal((N, C, 3, 3)) / np.sqrt(9 * C))
    assert np.array_equal(np.rint(x * 256), x * 256) and np.array_equal(np.rint(w * 256), w * 256)   # fp16 kept the grid
    assert np.abs(x).max() * np.abs(w).reshape(N, -1).sum(axis=1).max() < 256, "a partial sum could need more than 24 bits"
    pre = _pre(x, w, stride, 1).reshape(M, N)
    ps, pb = _rng_params(rng, N, big=(3, N - 2))
    slope = rng.uniform(-0.3, 0.4, N).astype(np.float32).astype(np.float16).astype(np.float64)
    ns, nb = _rng_params(rng, N)
    ident = rng.standard_normal((M, N)).astype(np.float16).astype(np.float64)
    T = lambda a: torch.from_numpy(a)  # noqa: E731
    t = ac.affine(T(pre), T(ps), T(pb)).numpy()
    want1 = ac.prelu(T(t), T(slope)).numpy()
    wantY = ac.r(T(t) + T(ident)).numpy()
    wantP = ac.affine(T(wantY), T(ns), T(nb)).numpy()
    u = ac.ulp16
    tol_t = u(pre) * np.abs(ps) + u(t)
    tol1 = tol_t * np.maximum(np.abs(slope), 1) + u(want1)
    tolY = tol_t + u(wantY)
    tolP = tolY * np.abs(ns) + u(wantP)
    wt = _tile(torch.from_numpy(w.transpose(0, 2, 3, 1).reshape(N, -1).astype(np.float16)).view(torch.int16)).cuda()
    X, R = _dev16(x.reshape(-1, C)), _dev16(ident)
    zeros = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_ps, d_pb, d_sl, d_ns, d_nb = _f32(ps), _f32(pb), _f32(slope), _f32(ns), _f32(nb)
    nrow = ((M + 255) // 256) * 256 * N
    out = {}
    for tile in (S.AUTO, s.tile):
        P1, Y, P2 = (torch.full((nrow,), -1, dtype=torch.int16, device="cuda") for _ in range(3))   # 0xFFFF: an fp16 NaN
        flag = tile | S.K_CHANNEL_MAJOR
        _lib.check(lib.mq_conv3x3_f16(X.data_ptr(), B, H, W, C, stride, wt.data_ptr(), N, d_ps.data_ptr(), d_pb.data_ptr(), d_sl.data_ptr(),
                                      None, None, None, None, P1.data_ptr(), zeros.data_ptr(), flag, None), "prelu")
        _lib.check(lib.mq_conv3x3_f16(X.data_ptr(), B, H, W, C, stride, wt.data_ptr(), N, d_ps.data_ptr(), d_pb.data_ptr(), None,
                                      R.data_ptr(), d_ns.data_ptr(), d_nb.data_ptr(), Y.data_ptr(), P2.data_ptr(), zeros.data_ptr(), flag, None),
                   "residual + bn1")
        torch.cuda.synchronize()
        out[tile] = (P1, Y, P2)
    tag = f"conv3x3 f16 {S.conv_id(s)} {S.TILE_NAMES[s.tile]}"
    for a, b in zip(out[S.AUTO], out[s.tile]):
        assert torch.equal(_untile(a, M, N), _untile(b, M, N)), tag
    P1, Y, P2 = out[S.AUTO]
    missed = []
    for got, want, tol, what in ((P1, want1, tol1, " conv1+bn2+prelu"), (Y, wantY, tolY, " conv2+bn3+residual"), (P2, wantP, tolP, " next bn1")):
        try:
            _check(_host16(got, M, N), want, tol, tag + what)     # refuses NaN: every element was written
        except AssertionError as e:   # all three outputs are checked before the test fails
            missed.append(str(e))
    assert not missed, missed


@pytest.mark.parametrize("s", S.CONV1X1, ids=S.conv_id)
def test_conv1x1_pair_tiles_against_float64(s):
    """mq_conv1x1_pair_f32: the four epilogue cases of tests/test_resnet_gpu.py's float64 test and the one a block in front of a
    downsample runs (shortcut, relu -> pair alone), under AUTO and the explicit tile"""
    from viquae_amd import _lib
    from viquae_amd.encoders import split_bf16_tiled
    lib = _lib.load()
    B, H, W, C, N, stride = s[:6]
    M = S.conv_rows(s)
    g = torch.Generator(device="cuda").manual_seed(H * 1000 + C + N + stride)
    X = _pair(torch.randn((B * H * W, C), generator=g, device="cuda"))
    w = torch.randn((N, C), generator=g, device="cuda") / C ** 0.5
    bias = torch.randn(N, generator=g, device="cuda")
    res = torch.randn((M, N), generator=g, device="cuda")
    wh, wl = split_bf16_tiled(w)
    zeros = torch.zeros(64, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    a = X.float().double().view(B, H, W, C)[:, ::stride, ::stride].reshape(M, C)   # what the kernel reads: the pair's values
    lin = a @ w.double().T + bias.double()

    def run(tile, residual, relu, want_y, want_p):
        Y = _nan_f32(M, N) if want_y else None
        P = _nan_pair(M, N) if want_p else None
        _lib.check(lib.mq_conv1x1_pair_f32(X.hi.data_ptr(), X.lo.data_ptr(), B, H, W, C, stride, wh.data_ptr(), wl.data_ptr(), N,
                                           bias.data_ptr(), _ptr(residual), relu, _ptr(Y), P.hi.data_ptr() if P else None,
                                           P.lo.data_ptr() if P else None, zeros.data_ptr(), tile, st), "mq_conv1x1_pair_f32")
        return Y, P
    cases = {"relu -> pair": (None, 1, False, True), "plain -> fp32": (None, 0, True, False),
             "shortcut, relu -> fp32 + pair": (res, 1, True, True), "shortcut, relu -> fp32": (res, 1, True, False),
             "shortcut, relu -> pair": (res, 1, False, True)}
    tag = f"conv1x1 {S.conv_id(s)} {S.TILE_NAMES[s.tile]}"
    for what, case in cases.items():
        residual, relu = case[:2]
        ref = lin + (residual.double() if residual is not None else 0)
        ref = ref.clamp_min(0) if relu else ref
        Y, P = run(S.AUTO, *case)
        if Y is not None:
            _assert_close(Y, ref, f"{tag} {what} Y")
        if P is not None:
            _assert_close(P.float(), ref, f"{tag} {what} P")
        if Y is not None and P is not None:   # the pair is the split of the very fp32 value
            hi, lo = _split(Y)
            ph, pl = P.rowmajor()
            assert torch.equal(ph.view(torch.bfloat16), hi) and torch.equal(pl.view(torch.bfloat16), lo), (tag, what)
        Ye, Pe = run(s.tile, *case)
        if Y is not None:
            assert torch.equal(Ye, Y), (tag, what)
        if P is not None:
            _assert_same_pair(Pe, P, (tag, what))


def test_im2col_rows_past_the_grid_dimension_carry():
    """mq_im2col_split_f32 with more 64-row tiles than gridDim.y holds (65535): the rest rides on blockIdx.z.  Every row against the
    statement of tests/test_arcface_gpu.py's im2col test (k = 1: the pre-operations on the pixel's channels, zeros up to Kpad)."""
    from viquae_amd import _lib
    c = S.IM2COL_CARRY
    B, H, W, C, kpad = c["B"], c["H"], c["W"], c["C"], c["kpad"]
    M = B * H * W
    assert M > S.GRID_Y_MAX * S.IM2COL_ROWS_PER_BLOCK
    g = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((B, H, W, C), generator=g, device="cuda")
    slope = torch.rand(C, generator=g, device="cuda") * 0.3 + 0.1
    scale = torch.rand(C, generator=g, device="cuda") + 0.5
    shift = torch.randn(C, generator=g, device="cuda")
    A = _nan_pair(M, kpad)   # the launch must write every row
    _lib.check(_lib.load().mq_im2col_split_f32(x.data_ptr(), B, H, W, C, 0, c["k"], c["k"], c["stride"], c["pad"], slope.data_ptr(),
                                               scale.data_ptr(), shift.data_ptr(), A.hi.data_ptr(), A.lo.data_ptr(), kpad,
                                               torch.cuda.current_stream().cuda_stream), "mq_im2col_split_f32")
    got = A.float()
    assert got.shape == (M, kpad) and not torch.isnan(got).any()
    xd = x.double().view(M, C)
    want = torch.where(xd >= 0, xd, xd * slope.double()) * scale.double() + shift.double()
    for lo_, hi_ in ((0, 4096), (S.GRID_Y_MAX * S.IM2COL_ROWS_PER_BLOCK - 4096, M), (0, M)):   # the two ends named, then everything
        d = (got[lo_:hi_, :C].double() - want[lo_:hi_]).abs()
        assert bool((d <= 2e-5 * want[lo_:hi_].abs() + 1e-6).all()), (lo_, hi_, float(d.max()))   # hi + lo keeps 16 bits
    assert not got[:, C:].any()


# ---- model level: the production launch set, pinned through batch invariance ------------------------------------------------------------

@pytest.fixture(scope="module")
def arcface_golden():
    from oracle import arcface as oa
    g = np.load(os.path.join(HERE, "golden", "arcface_r50_8.npz"))
    return g, oa.seeded_state(int(g["seed_weights"]))


@pytest.fixture(scope="module")
def resnet_golden():
    from tests import resnet_restatement as R
    g = np.load(os.path.join(HERE, "golden", "resnet50_8.npz"))
    return g, R.seeded_state(int(g["state_seed"]), tuple(g["layers"]))


@pytest.fixture(scope="module")
def clip_golden():
    from tests import clip_resnet_restatement as R
    g = np.load(os.path.join(HERE, "golden", "clip_rn50_8.npz"))
    return g, R.seeded_state(int(g["state_seed"]), tuple(g["layers"]))


@pytest.fixture
def release():
    """hands the forward's buffers back before the next model runs"""
    yield
    torch.cuda.empty_cache()


def _batch(golden8, B, seed, low=None):
    """[B, 3, S, S]: the golden's first four images, seeded random ones, the golden's last four"""
    assert golden8.shape[0] == 8 and B >= 16
    g = torch.Generator().manual_seed(seed)
    shape = (B - 8,) + tuple(golden8.shape[1:])
    mid = torch.rand(shape, generator=g) * 2 - 1 if low is not None else torch.randn(shape, generator=g)
    return torch.cat([golden8[:4], mid, golden8[4:]]).cuda()


def _whole_and_chunks(model, x, net):
    """(a): the whole batch in one forward (the production launch set) == the forwards over chunks of 8 (the tiles of the golden tests)"""
    B = x.shape[0]
    assert B == S.smallest_production_batch(net) and model.chunk >= B
    with torch.no_grad():
        whole = model(x).reshape(B, -1)
        parts = torch.cat([model(x[i:i + 8]).reshape(min(8, B - i), -1) for i in range(0, B, 8)])
    assert torch.isfinite(whole).all()
    bad = (whole != parts).any(dim=1).nonzero().flatten().tolist()
    assert not bad, f"{net}: rows {bad[:8]} ... of the batch of {B} differ from the chunked forward by {float((whole - parts).abs().max()):.3e}"
    return torch.cat([whole[:4], whole[-4:]]).cpu().numpy()


def test_arcface_production_launch_set_is_batch_invariant(arcface_golden, release):
    from oracle import arcface as oa
    from viquae_amd.arcface import ArcFaceR50
    g, state = arcface_golden
    B = S.smallest_production_batch("arcface")
    x8 = torch.from_numpy(np.stack([oa.preprocess(f) for f in g["faces_u8"]]))
    model = ArcFaceR50.from_state_dict(state, chunk=max(B, S.DEFAULT_CHUNK["arcface"])).cuda()
    got = _whole_and_chunks(model, _batch(x8, B, 11, low=-1), "arcface")
    err = np.abs(got - g["embeddings_f64"]).max()
    print(f"arcface fp32, batch {B}: golden rows max |HIP - float64| = {err:.3e}")
    assert err <= 1e-3


def test_arcface_fp16_production_launch_set_is_batch_invariant(arcface_golden, release):
    from viquae_amd.arcface import ArcFaceR50
    g, state = arcface_golden
    B = S.smallest_production_batch("arcface")
    x8 = (torch.from_numpy(g["faces_u8"]).permute(0, 3, 1, 2).to(torch.float32).div(255.0) - 0.5) / 0.5   # as its golden test
    model = ArcFaceR50.from_state_dict(state, chunk=max(B, S.DEFAULT_CHUNK["arcface"]), precision="fp16").cuda()
    y = _whole_and_chunks(model, _batch(x8, B, 12, low=-1), "arcface")
    ref = g["embeddings_fp16_autocast"]
    d = y - ref
    mx, rms = float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))
    cos = min(float(a @ b / np.linalg.norm(a) / np.linalg.norm(b)) for a, b in zip(y, ref))
    print(f"arcface fp16, batch {B}: golden rows vs embeddings_fp16_autocast: max {mx:.3e}, rms {rms:.3e}, min cosine {cos:.7f}")
    # the bound of test_fp16_forward_matches_the_golden_autocast_embeddings
    assert mx <= 2 * float(g["fp16_autocast_max_abs_dev"]) and rms <= 2 * 1.7e-3, (mx, rms)
    assert cos >= 1 - 1e-5, cos


def test_resnet_production_launch_set_is_batch_invariant(resnet_golden, release):
    from tests import resnet_restatement as R
    from viquae_amd.resnet import TorchvisionResNet
    g, state = resnet_golden
    B = S.smallest_production_batch("resnet")
    x8 = torch.from_numpy(R.normalize_u8(g["images_u8"]))
    model = TorchvisionResNet.from_state_dict(state, pool_kwargs={"Class_name": "AdaptiveMaxPool2d", "output_size": 1},
                                              chunk=max(B, S.DEFAULT_CHUNK["resnet"])).cuda()
    got = _whole_and_chunks(model, _batch(x8, B, 13), "resnet")
    err = np.abs(got.astype(np.float64) - g["max_f64"]).max()
    print(f"resnet50, batch {B}: golden rows max |HIP - float64| = {err:.3e}")
    assert err <= 1e-3


def test_clip_resnet_production_launch_set_is_batch_invariant(clip_golden, release):
    from tests import clip_resnet_restatement as R
    from viquae_amd.clip_resnet import CLIPModifiedResNet
    g, state = clip_golden
    B = S.smallest_production_batch("clip")
    x8 = torch.from_numpy(R.normalize_u8(g["images_u8"], R.MEAN, R.STD))
    model = CLIPModifiedResNet.from_state_dict(state, chunk=max(B, S.DEFAULT_CHUNK["clip"])).cuda()
    got = _whole_and_chunks(model, _batch(x8, B, 14), "clip")
    err = np.abs(got.astype(np.float64) - g["out_f64"]).max()
    print(f"clip RN50, batch {B}: golden rows max |HIP - float64| = {err:.3e}")
    assert err <= 1e-3
