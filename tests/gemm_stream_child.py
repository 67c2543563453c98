"""Operands and launches of the tile stream tests (tests/test_gemm_stream_gpu.py), and the child process of their workgroup
count leg: MQ_GEMM_WGS is read once per process, so another count needs a fresh process.

    python -m tests.gemm_stream_child OUT_DIR

runs gemm_stream_shapes.CHILD_CASES under the environment it was given and writes the raw output words to
OUT_DIR/outputs.npz (c<case>_<array>: one int32 array for an fp32 output, the int16 (hi, lo) arrays of a pair output)."""
import collections
import contextlib
import os
import sys

import numpy as np
import torch

from tests import gemm_stream_shapes as S

Operands = collections.namedtuple("Operands", "a_f32 a w_f32 w bias res_f32 res")


def operands(M, N, K, v, seed):
    """Seeded operands of one product: a [M, K] as a SplitAct, w [N, K] split (tiled or row-major per the variant), bias [N],
    the residual [M, N] in the variant's form (None, fp32, SplitAct)."""
    from viquae_amd import encoders as E
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn((M, K), generator=g, device="cuda") * 0.7
    w = torch.randn((N, K), generator=g, device="cuda") * 0.05
    b = torch.randn((N,), generator=g, device="cuda")
    r32 = r = None
    if v.res is not None:
        r32 = r = torch.randn((M, N), generator=g, device="cuda")
        if v.res == "pair":
            r = E.SplitAct(*E.split_bf16(r32))
    asp = E.SplitAct(*E.split_bf16(a))
    wsp = E.split_bf16_tiled(w) if v.tiled else E.split_bf16(w)
    return Operands(a, asp, w, wsp, b, r32, r)


def slice_rows(x, lo, hi):
    """Rows [lo, hi) of an fp32 matrix or of a SplitAct (lo a multiple of 256: a contiguous piece of the pair layout)."""
    from viquae_amd import encoders as E
    if x is None:
        return None
    if not isinstance(x, E.SplitAct):
        return x[lo:hi]
    assert lo % S.GT == 0 and 0 <= lo < hi <= x.shape[0]
    F = x.shape[1]
    end = (hi + S.GT - 1) // S.GT * S.GT
    return E.SplitAct(x.hi[lo * F:end * F], x.lo[lo * F:end * F], shape=(hi - lo, F))


@contextlib.contextmanager
def sentinel_pairs():
    """Pair outputs allocated inside the block start as 0xFF bytes."""
    from viquae_amd import encoders as E
    real = E.SplitAct.__dict__["empty"]

    def filled(rows, features, device):
        sp = real.__func__(E.SplitAct, rows, features, device)
        sp.hi.fill_(-1)
        sp.lo.fill_(-1)
        return sp
    E.SplitAct.empty = staticmethod(filled)
    try:
        yield
    finally:
        E.SplitAct.empty = real


def launch(ops, v, lo=0, hi=None, sentinel=False):
    """One gemm_nt call of the variant on rows [lo, hi) of the operands -> the output (fp32 tensor or SplitAct).
    ``sentinel``: the output buffer is filled with 0xFF bytes first."""
    from viquae_amd import encoders as E
    M, N = ops.a.shape[0], ops.w_f32.shape[0]
    hi = M if hi is None else hi
    a, r = ops.a, ops.res
    if (lo, hi) != (0, M):
        a, r = slice_rows(a, lo, hi), slice_rows(r, lo, hi)
    out = None
    if sentinel and not v.osp:
        out = torch.full((hi - lo, N), -1, dtype=torch.int32, device="cuda").view(torch.float32)
    with (sentinel_pairs() if sentinel and v.osp else contextlib.nullcontext()):
        return E.gemm_nt(a, ops.w_f32, ops.bias if v.epi != E.EPI_NONE else None, r, v.epi, out=out, wsplit=ops.w, out_split=v.osp)


def words(c):
    """The raw words of every element of an output: (int32 [M, N],) or the int16 (hi, lo) [M, N] of a pair's real rows."""
    from viquae_amd import encoders as E
    if isinstance(c, E.SplitAct):
        return tuple(c.rowmajor())
    return (c.view(torch.int32),)


def child_outputs():
    """{c<case>_<array>: numpy words} of CHILD_CASES at this process's workgroup count"""
    out = {}
    for i, (M, N, K, v) in enumerate(S.CHILD_CASES):
        ops = operands(M, N, K, v, 4000 + i)
        c = launch(ops, v, sentinel=True)
        torch.cuda.synchronize()
        for j, t in enumerate(words(c)):
            out[f"c{i}_{j}"] = t.cpu().numpy()
    return out


def main(argv):
    out_dir = argv[1]
    np.savez(os.path.join(out_dir, "outputs.npz"), wgs=np.array(os.environ.get("MQ_GEMM_WGS", "")), **child_outputs())
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
