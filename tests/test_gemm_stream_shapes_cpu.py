"""The conditions of the tile stream tests (tests/test_gemm_stream_gpu.py), checked for an MI355X's 256 CUs before anything
reaches a GPU: every stream shape streams, every group of 8 row blocks does not, every class of shape is there."""
from tests import gemm_stream_shapes as S

CU = 256


def _by_class(c):
    return [s for s in S.STREAM_SHAPES if c in s.classes]


def test_stream_shapes_stream_and_their_slices_do_not():
    limit = S.limit_of(CU)
    assert limit == 256
    for s in S.STREAM_SHAPES:
        assert S.slots(s.M, s.N) > limit, s
        assert S.group_slots(s.N) <= limit and S.group_slots(s.N) <= 96, s
        assert S.slots(min(s.M, S.GROUP_ROWS), s.N) == S.group_slots(s.N)
        assert s.K % 32 == 0 and set(s.classes) <= set(S.CLASSES) and s.variants and set(s.wides) <= {0, 1} and 1 in s.wides
        assert all(not v.osp and v.res != "pair" for v in s.variants) or s.N % 32 == 0, s   # pair layout: 32-column tiles
    for c in S.CLASSES:
        assert _by_class(c), f"no shape of class {c}"
    # slots just above the limit: some workgroups run two tiles, the others one; many times: at least four tiles each
    for s in _by_class("just_above"):
        assert limit < S.slots(s.M, s.N) < 2 * limit, s
        assert {len([x for x in S.walk(wg, s.M, s.N, limit) if x[3]]) for wg in range(limit)} >= {1, 2} or "pad_skip" in s.classes, s
    for s in _by_class("many"):
        assert S.slots(s.M, s.N) >= 4 * limit, s
    assert any((s.M, s.N, s.K) == (204800, 2304, 768) for s in _by_class("production"))
    assert all(s.K == 3072 for s in _by_class("k3072"))
    assert {s.K for s in _by_class("short_k")} >= {32, 64}
    # padded slots skipped inside the stream: at some workgroup's second or later visit
    for s in _by_class("pad_skip"):
        assert S.tiles(s.M, s.N)[0] % 8 != 0, s
        assert any(it >= 1 and not inside for wg in range(limit) for it, _, _, inside in S.walk(wg, s.M, s.N, limit)), s
    # the ragged last row block is some workgroup's second or later tile
    for s in _by_class("ragged_m"):
        assert s.M % S.GT != 0, s
        last = S.tiles(s.M, s.N)[0] - 1
        assert any(it >= 1 and mt == last for wg in range(limit) for it, mt, _, _ in S.walk(wg, s.M, s.N, limit)), s
    assert {s.N for s in _by_class("ragged_n")} >= {320, 33 * 32}
    assert {s.N for s in _by_class("n_mod_32")} >= {515, 516}
    # N = 33 * 32: full and partial column tiles alternate inside one workgroup's stream, in both orders
    for s in (s for s in _by_class("ragged_n") if s.N == 33 * 32):
        ntn = S.tiles(s.M, s.N)[1]
        orders = set()
        for wg in range(limit):
            partial = [nt == ntn - 1 for _, _, nt, inside in S.walk(wg, s.M, s.N, limit) if inside]
            orders |= set(zip(partial, partial[1:]))
        assert {(False, True), (True, False)} <= orders, s
    # N ragged: fp32 and pair outputs, with and without a residual
    for s in (s for s in _by_class("ragged_n") if s.N % 32 == 0):
        assert {(v.osp, v.res is not None) for v in s.variants} == {(False, False), (True, False), (False, True), (True, True)}, s


def test_every_epilogue_output_form_and_kernel_is_on_a_just_above_and_a_many_times_shape():
    wanted = {(v.epi, v.res) for v in S.ALL_VARIANTS}
    assert {e for e, _ in wanted} == {S.EPI_NONE, S.EPI_BIAS, S.EPI_BIAS_GELU, S.EPI_BIAS_QUICKGELU, S.EPI_BIAS_RESIDUAL}
    assert {r for e, r in wanted if e == S.EPI_BIAS_RESIDUAL} == {"f32", "pair"}
    for c in ("just_above", "many"):
        cases = [(s, v, w) for s, v, w in S.stream_cases() if c in s.classes]
        assert {(v.epi, v.res) for _, v, _ in cases} >= wanted, c
        assert {v.osp for _, v, _ in cases} == {False, True} and {v.tiled for _, v, _ in cases} == {False, True}, c
        assert {w for _, _, w in cases} == {0, 1}, c
    for s in S.STREAM_SHAPES:
        assert S.BIAS_F32 in s.variants, s       # the variant the fp64 leg runs on
    assert len({S.case_id(c) for c in S.stream_cases()}) == len(S.stream_cases())


def test_stagger_split_k_and_child_shapes():
    limit = S.limit_of(CU)
    M, N, _ = S.STAGGER_SHAPE
    assert S.slots(M, N) >= 4 * limit
    for M, N, K in S.SPLITK_SHAPES:
        assert S.slots(M, N) > limit and S.group_slots(N) <= limit
        for n in S.SPLITK_NSPLIT:
            per = -(-(K // 32) // n)
            assert -(-(K // 32) // per) == n
    # with 8 workgroups each walks 4 to 36 tile slots; at the default count none of these products streams
    for M, N, K, v in S.CHILD_CASES:
        assert 4 <= S.slots(M, N) // 8 <= 36 and S.slots(M, N) <= 2 * limit and K % 32 == 0
    assert S.CHILD_WGS == (8, 16, 0)
