"""GPU: the opt-in fp16 face encoder (ArcFaceR50(precision="fp16"), csrc/conv.hip's fp16 kernels) against
tests/autocast_schedule.py, the torch statement of arcface_torch's fp16 autocast rounding points.  Per kernel the inputs are fp16
tensors from torch and the reference puts float64 arithmetic between the same roundings: >= 99.5 % of the outputs must be bit-identical
and every other one within one fp16 ulp of its pre-affine value (scaled through what follows) -- one-ulp flips of r(acc) are all that
fp32 accumulation may change.  End to end the same flips cascade through 50 layers, so the full forward is held to a noise band."""
import numpy as np
import pytest
import torch

from tests import autocast_schedule as ac

pytestmark = pytest.mark.gpu


def _dev16(a):
    """float array [M, C] (fp16 values) -> fp16 activation in PAIR LAYOUT (flat int16) on the GPU"""
    from viquae_amd.encoders import _tile
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float16)).view(np.int16))
    return _tile(t).cuda()


def _host16(flat, M, C):
    from viquae_amd.encoders import _untile
    return _untile(flat.cpu(), M, C).view(torch.float16).to(torch.float64).numpy()


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _check(got, want, tol, what):
    """bit-identical rate >= 99.5 %; the rest within tol; +-inf exactly where the reference has it"""
    assert got.shape == want.shape, what
    inf_g, inf_w = np.isinf(got), np.isinf(want)
    assert np.array_equal(inf_g, inf_w) and np.array_equal(got[inf_w], want[inf_w]), (what, int(inf_g.sum()), int(inf_w.sum()))
    assert not np.isnan(got).any() and not np.isnan(want).any(), what
    same = (got == want)
    rate = float(same.mean())
    print(f"{what}: {100 * rate:.3f} % bit-identical")
    assert rate >= 0.995, (what, rate)
    fin = ~inf_w
    bad = fin & (np.abs(got - want) > tol)
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(got - want)[bad].max()))


def _rng_params(rng, N, big=()):
    a = rng.uniform(0.5, 1.5, N) * rng.choice([-1.0, 1.0], N, p=[0.1, 0.9])
    a[list(big)] = 3.0e4       # these channels overflow fp16 after the affine: +-inf must land where the reference's does
    b = rng.normal(0, 0.5, N)
    return a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)


def _pre(x16, w, stride, pad):
    """float64 r(conv) of fp16 x [B, H, W, C] with fp16 weights"""
    return ac.conv_nhwc(torch.from_numpy(x16), torch.from_numpy(w), stride, pad).numpy()


SHAPES = [  # (B, H, C, N, stride, tiles)
    (2, 56, 64, 64, 1, (4, 5, 0)),
    (2, 56, 64, 64, 2, (4, 0)),
    (2, 56, 128, 128, 2, (2, 3, 4, 0)),
    (2, 28, 128, 128, 1, (2, 3, 4, 5, 0)),
    (2, 28, 256, 256, 2, (1, 2, 3, 4, 0)),
    (2, 14, 256, 256, 1, (1, 2, 3, 4, 5, 0)),
    (2, 14, 512, 512, 2, (1, 2, 3, 4, 0)),
    (2, 7, 512, 512, 1, (1, 2, 3, 4, 5, 0)),
]


@pytest.mark.parametrize("B,H,C,N,stride,tiles", SHAPES)
def test_conv3x3_f16_kernels_follow_the_autocast_schedule(B, H, C, N, stride, tiles):
    """conv1 + bn2 + PReLU, conv2 + bn3 + residual (+ the next bn1 and without it), every tile variant, 56 / 28 / 14 / 7, stride 1 / 2"""
    from viquae_amd import _lib
    from viquae_amd.encoders import _tile
    lib = _lib.load()
    rng = np.random.default_rng(H * 7 + C + stride)
    W = H
    x = rng.standard_normal((B, H, W, C)).astype(np.float16).astype(np.float64)
    w = (rng.standard_normal((N, C, 3, 3)) / np.sqrt(9 * C)).astype(np.float16).astype(np.float64)
    Ho = (H - 1) // stride + 1
    M = B * Ho * Ho
    pre = _pre(x, w, stride, 1).reshape(M, N)                                 # r(acc), float64 accumulation
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
    for tile in tiles:
        P1, Y, P2, Y3 = (torch.full((nrow,), -1, dtype=torch.int16, device="cuda") for _ in range(4))
        flag = tile | 0x100
        _lib.check(lib.mq_conv3x3_f16(X.data_ptr(), B, H, W, C, stride, wt.data_ptr(), N, d_ps.data_ptr(), d_pb.data_ptr(), d_sl.data_ptr(),
                                      None, None, None, None, P1.data_ptr(), zeros.data_ptr(), flag, None), "prelu")
        _lib.check(lib.mq_conv3x3_f16(X.data_ptr(), B, H, W, C, stride, wt.data_ptr(), N, d_ps.data_ptr(), d_pb.data_ptr(), None,
                                      R.data_ptr(), d_ns.data_ptr(), d_nb.data_ptr(), Y.data_ptr(), P2.data_ptr(), zeros.data_ptr(), flag, None),
                   "residual + bn1")
        _lib.check(lib.mq_conv3x3_f16(X.data_ptr(), B, H, W, C, stride, wt.data_ptr(), N, d_ps.data_ptr(), d_pb.data_ptr(), None,
                                      R.data_ptr(), None, None, Y3.data_ptr(), None, zeros.data_ptr(), flag, None), "residual")
        torch.cuda.synchronize()
        tag = f"conv3x3 {H}x{H}x{C}->{N} s{stride} tile {tile}"
        _check(_host16(P1, M, N), want1, tol1, tag + " conv1+bn2+prelu")
        _check(_host16(Y, M, N), wantY, tolY, tag + " conv2+bn3+residual")
        _check(_host16(P2, M, N), wantP, tolP, tag + " next bn1")
        assert torch.equal(Y3, Y), tag                                        # the shortcut does not depend on the next bn1
    if stride == 1:  # the tile with too few columns is refused, not run
        assert lib.mq_conv3x3_f16(X.data_ptr(), B, H, W, C, stride, wt.data_ptr(), N, d_ps.data_ptr(), d_pb.data_ptr(), d_sl.data_ptr(),
                                  None, None, None, None, P1.data_ptr(), zeros.data_ptr(), 1 if N < 256 else 9, None) == -1


@pytest.mark.parametrize("B,H,W", [(2, 112, 112), (3, 12, 8)])
def test_stem_f16_follows_the_autocast_schedule(B, H, W):
    from viquae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(B * H)
    x = rng.uniform(-1, 1, (B, 3, H, W)).astype(np.float32)
    w = (rng.standard_normal((64, 3, 3, 3)) / 5.0).astype(np.float32)
    w16 = w.astype(np.float16).astype(np.float64)
    ps, pb = _rng_params(rng, 64, big=(5,))
    slope = rng.uniform(-0.3, 0.4, 64).astype(np.float16).astype(np.float64)
    ns, nb = _rng_params(rng, 64)
    T = lambda a: torch.from_numpy(a)  # noqa: E731
    xr = ac.r(T(x.astype(np.float64))).permute(0, 2, 3, 1).contiguous().numpy()
    pre = _pre(xr, w16, 1, 1)
    t = ac.affine(T(pre), T(ps), T(pb)).numpy()
    v = ac.prelu(T(t), T(slope)).numpy()
    P = ac.affine(T(v), T(ns), T(nb)).numpy()
    u = ac.ulp16
    tolv = (u(pre) * np.abs(ps) + u(t)) * np.maximum(np.abs(slope), 1) + u(v)
    tolP = tolv * np.abs(ns) + u(P)
    wt = w16.transpose(2, 3, 1, 0).reshape(27, 64)
    dP = torch.empty(((B * H * W + 255) // 256) * 256 * 64, dtype=torch.int16, device="cuda")
    Md = B * (H // 2) * (W // 2)
    dD = torch.empty(((Md + 255) // 256) * 256 * 64, dtype=torch.int16, device="cuda")
    args = [_f32(a) for a in (x, wt, ps, pb, slope, ns, nb)]     # held: a freed temporary's block would be reused by the next upload
    dx, dwt, dps, dpb, dsl, dns, dnb = (a.data_ptr() for a in args)
    _lib.check(lib.mq_stem_conv3x3_f16(dx, B, H, W, dwt, dps, dpb, dsl, dns, dnb, dP.data_ptr(), dD.data_ptr(), None), "stem")
    torch.cuda.synchronize()
    _check(_host16(dP, B * H * W, 64), P.reshape(-1, 64), tolP.reshape(-1, 64), f"stem {H}x{W} P")
    _check(_host16(dD, Md, 64), v[:, ::2, ::2].reshape(-1, 64), tolv[:, ::2, ::2].reshape(-1, 64), f"stem {H}x{W} D")


@pytest.mark.parametrize("B,H,C,N,stride", [(2, 56, 64, 64, 1), (2, 56, 64, 128, 2), (2, 28, 128, 256, 2), (2, 14, 256, 512, 2), (3, 7, 512, 512, 1)])
def test_downsample_f16_follows_the_autocast_schedule(B, H, C, N, stride):
    from viquae_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(H + N)
    x = rng.standard_normal((B, H, H, C)).astype(np.float16).astype(np.float64)
    w = (rng.standard_normal((N, C, 1, 1)) / np.sqrt(C)).astype(np.float16).astype(np.float64)
    ps, pb = _rng_params(rng, N, big=(1,))
    Ho = (H - 1) // stride + 1
    M = B * Ho * Ho
    pre = _pre(x, w, stride, 0).reshape(M, N)
    want = ac.affine(torch.from_numpy(pre), torch.from_numpy(ps), torch.from_numpy(pb)).numpy()
    Y = torch.empty(((M + 255) // 256) * 256 * N, dtype=torch.int16, device="cuda")
    wt = torch.from_numpy(w.reshape(N, C).astype(np.float16)).view(torch.int16).cuda()
    X, d_ps, d_pb = _dev16(x.reshape(-1, C)), _f32(ps), _f32(pb)
    _lib.check(lib.mq_conv1x1_f16(X.data_ptr(), B, H, H, C, stride, wt.data_ptr(), N, d_ps.data_ptr(), d_pb.data_ptr(), Y.data_ptr(), None),
               "downsample")
    torch.cuda.synchronize()
    _check(_host16(Y, M, N), want, ac.ulp16(pre) * np.abs(ps) + ac.ulp16(want), f"downsample {H}x{H}x{C}->{N} s{stride}")


def test_head_prep_f16_is_bn2_flatten_float():
    from viquae_amd import _lib
    from viquae_amd.encoders import SplitAct
    lib = _lib.load()
    rng = np.random.default_rng(5)
    B, HW, C = 37, 49, 512
    t = (rng.standard_normal((B * HW, C)) * 4).astype(np.float16).astype(np.float64)
    a, b = _rng_params(rng, C, big=(7,))
    want = ac.affine(torch.from_numpy(t), torch.from_numpy(a), torch.from_numpy(b)).numpy()
    want = want.reshape(B, HW * C)                                   # NHWC flatten: column pixel * C + c
    A = SplitAct.empty(B, HW * C, "cuda")
    X, d_a, d_b = _dev16(t), _f32(a), _f32(b)
    _lib.check(lib.mq_head_prep_f16(X.data_ptr(), B, HW, C, d_a.data_ptr(), d_b.data_ptr(), A.hi.data_ptr(), A.lo.data_ptr(), None),
               "head prep")
    hi, lo = A.rowmajor()
    got = (hi.view(torch.bfloat16).double() + lo.view(torch.bfloat16).double()).cpu().numpy()
    _check(got, want, ac.ulp16(want), "head prep")
    assert np.array_equal(got[np.isfinite(got)].astype(np.float16).astype(np.float64), got[np.isfinite(got)])   # hi + lo is an fp16 value


def _golden_model(**kw):
    from oracle import arcface as oa
    from viquae_amd.arcface import ArcFaceR50
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arcface_r50_8.npz"))
    x = (torch.from_numpy(g["faces_u8"]).permute(0, 3, 1, 2).to(torch.float32).div(255.0) - 0.5) / 0.5
    return g, x, ArcFaceR50.from_state_dict(oa.seeded_state(int(g["seed_weights"])), **kw).cuda()


def test_fp16_forward_matches_the_golden_autocast_embeddings():
    g, x, model = _golden_model(precision="fp16")
    with torch.no_grad():
        y = model(x.cuda()).cpu().numpy()
        y2 = model(x.cuda()).cpu().numpy()
    assert y.shape == (8, 512) and y.dtype == np.float32
    assert np.array_equal(y, y2)                                          # deterministic
    ref = g["embeddings_fp16_autocast"]
    d = y - ref
    mx, rms = float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))
    cos = min(float(a @ b / np.linalg.norm(a) / np.linalg.norm(b)) for a, b in zip(y, ref))
    print(f"fp16 forward vs embeddings_fp16_autocast: max {mx:.3e}, rms {rms:.3e}, min cosine {cos:.7f}")
    assert mx <= 2 * float(g["fp16_autocast_max_abs_dev"]) and rms <= 2 * 1.7e-3, (mx, rms)
    # torch-CPU's own fp32 operators instead of correctly rounded fp32 between the golden's roundings already move the embeddings
    # by 8.4e-3 max / 1.7e-3 rms (|y| ~ 6.8, rms ~ 1):
    # cosine 1 - 1e-5 is ~ 3x that noise in squared-error terms
    assert cos >= 1 - 1e-5, cos


def test_fp16_chunks_and_default_precision():
    g, x, m16 = _golden_model(precision="fp16", chunk=3)
    _, _, m32 = _golden_model()
    _, _, m32b = _golden_model(precision="fp32")
    xc = x.cuda()
    with torch.no_grad():
        whole = m16(xc)                                                   # 8 faces in chunks of 3
        parts = torch.cat([m16(xc[s:s + 3]) for s in range(0, 8, 3)])
        assert torch.equal(whole, parts)
        y32 = m32(xc)
        assert torch.equal(y32, m32b(xc))                                # precision unset = the fp32 path, bit for bit
        assert not torch.equal(y32, whole)


def test_pipelined_fp16_face_job_equals_the_serial_one(tmp_path, monkeypatch):
    """the face job at MQ_ARCFACE_PRECISION=fp16 (from_pretrained reads it), software-pipelined and serial: the same bits"""
    import datasets
    import shutil
    from PIL import Image
    from oracle import arcface as oa
    from viquae_amd.arcface import ArcFaceR50
    from viquae_amd.data import loading
    from viquae_amd.image import face_recognition as fr
    datasets.disable_progress_bars()
    rng = np.random.default_rng(11)
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    monkeypatch.setattr(loading, "IMAGE_PATH", img_dir)
    yy, xx = np.mgrid[0:240, 0:300]
    names, lms = [], []
    for i in range(17):
        a = np.stack([128 + 90 * np.sin(xx / (6 + c + i)) * np.cos(yy / (5 + c)) + rng.normal(0, 10, xx.shape) for c in range(3)], axis=2)
        Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)[: 200 + 3 * (i % 7), : 260 + 5 * (i % 5)]).save(img_dir / f"f{i}.jpg", quality=85)
        names.append(f"f{i}.jpg")
        n_faces = (1, 0, 3, 2, 5, 1)[i % 6]
        lms.append(None if n_faces == 0 else [((oa.SRC * (0.7 + 0.2 * f)) + np.array([30.0 + 25 * f, 20.0 + 3 * i], np.float32)).tolist() for f in range(n_faces)])
    ds_path = tmp_path / "ds"
    datasets.Dataset.from_dict({"image": names, "face_landmarks": lms}).save_to_disk(str(ds_path))
    state = oa.seeded_state(3)
    made = []

    def fake_from_pretrained(model_name="r50", fp16=True, train=False, precision=None):
        import os
        made.append(precision or os.environ.get("MQ_ARCFACE_PRECISION", "fp32"))
        return ArcFaceR50.from_state_dict(state, precision=made[-1]).cuda()

    monkeypatch.setattr(fr, "from_pretrained", fake_from_pretrained)
    monkeypatch.setenv("MQ_ARCFACE_PRECISION", "fp16")
    got = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("MQ_EMBED_PIPELINE", flag)
        work = tmp_path / f"ds{flag}"
        shutil.copytree(ds_path, work)
        out = fr.dataset_compute_face_embedding(str(work), map_kwargs={"max_n_faces": 2, "batch_size": 5})
        got[flag] = out["face_embedding"]
    assert made == ["fp16", "fp16"]
    n = 0
    for i, (a, b) in enumerate(zip(got["1"], got["0"])):
        if lms[i] is None:
            assert a is None and b is None, i
        else:
            a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
            assert a.shape == (min(2, len(lms[i])), 512) and np.array_equal(a, b), i
            n += 1
    assert n > 10
