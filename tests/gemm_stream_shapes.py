"""Shapes and slot arithmetic of the persistent tile stream tests (tests/test_gemm_stream_gpu.py); imports without a GPU.

The split-bf16 GEMMs (csrc/gemm_x3w.inc, gemm_nt_x3s_kernel) start at most `limit` = CU count rounded down to 8 workgroups.
A product with more 256 x 256 tile slots than that is walked as a stream of tiles per workgroup; one with at most `limit`
slots runs one tile per workgroup.  Slot b -> row block ((b >> 3) / ntn) * 8 + (b & 7), column tile (b >> 3) % ntn: the row
blocks are padded to a multiple of 8 and the padded slots are skipped.

A "stream" shape has slots > limit.  Its oracle is the same call on groups of 8 row blocks (GROUP_ROWS rows): 8 * ntn slots,
one tile per workgroup."""
import collections

GT = 256                 # tile edge (csrc/encoder.hip)
GROUP_ROWS = 8 * GT      # one group of 8 row blocks

EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_QUICKGELU, EPI_BIAS_RESIDUAL = 0, 1, 2, 3, 4  # viquae_amd.encoders.EPI_*


def tiles(M, N):
    return (M + GT - 1) // GT, (N + GT - 1) // GT


def slots(M, N):
    ntm, ntn = tiles(M, N)
    return ((ntm + 7) & ~7) * ntn


def group_slots(N):
    return 8 * tiles(1, N)[1]


def limit_of(cu):
    return cu // 8 * 8


def walk(wg, M, N, wgs):
    """The slots workgroup `wg` of `wgs` visits, as (visit number, row block, column tile, inside the matrix)."""
    ntm, ntn = tiles(M, N)
    out = []
    for it, b in enumerate(range(wg, slots(M, N), wgs)):
        mt, nt = ((b >> 3) // ntn) * 8 + (b & 7), (b >> 3) % ntn
        out.append((it, mt, nt, mt < ntm))
    return out


Variant = collections.namedtuple("Variant", "epi res osp tiled")   # res: None | "f32" | "pair"; osp: pair output; tiled weights

# the set test_wide_wave_gemm_is_bit_identical_to_the_sixteen_wave_gemm lists
ALL_VARIANTS = [Variant(EPI_NONE, None, False, True), Variant(EPI_BIAS, None, False, True), Variant(EPI_BIAS, None, True, False),
                Variant(EPI_BIAS_GELU, None, True, True), Variant(EPI_BIAS_QUICKGELU, None, False, True),
                Variant(EPI_BIAS_RESIDUAL, "f32", False, True), Variant(EPI_BIAS_RESIDUAL, "pair", False, True),
                Variant(EPI_BIAS_RESIDUAL, "pair", True, True), Variant(EPI_BIAS_RESIDUAL, "f32", True, False)]
BIAS_F32 = Variant(EPI_BIAS, None, False, True)                      # the variant oracle B (fp64) runs on
ENCODER_VARIANTS = [BIAS_F32, Variant(EPI_BIAS_GELU, None, True, True), Variant(EPI_BIAS_RESIDUAL, "pair", True, True)]
# N ragged against 256: fp32 and pair outputs, with and without a residual
RAGGED_N_VARIANTS = [BIAS_F32, Variant(EPI_BIAS, None, True, True), Variant(EPI_BIAS_RESIDUAL, "f32", False, True),
                     Variant(EPI_BIAS_RESIDUAL, "pair", True, False)]
# N % 32 != 0: fp32 output only (the pair layout is made of 32-column tiles)
F32_ONLY_VARIANTS = [Variant(EPI_NONE, None, False, True), BIAS_F32, Variant(EPI_BIAS_GELU, None, False, False),
                     Variant(EPI_BIAS_RESIDUAL, "f32", False, True)]

Shape = collections.namedtuple("Shape", "M N K classes variants wides")

# classes:  just_above  slots in (limit, 2 limit): some workgroups run two tiles, the others one
#           many        slots >= 4 limit
#           production  the benchmarked DPR 2048 x 100 QKV product
#           k3072       the FFN2 depth
#           pad_skip    ntm % 8 != 0: padded slots are skipped inside the stream (at a workgroup's second or later visit)
#           ragged_m    M % 256 != 0: the ragged last row block is reached late in a stream
#           ragged_n    N % 256 != 0 (N = 320, 33 * 32): full and partial tiles in one launch
#           n_mod_32    N % 32 != 0 (516: the wide kernel; 515: the sixteen-wave kernel whatever GEMM_OPT_WIDE says)
#           short_k     K = 32, 64: one and two K steps per tile
STREAM_SHAPES = [
    Shape(6144, 3072, 768, ("just_above",), ALL_VARIANTS, (1, 0)),                      # 24 x 12 = 288 slots (FFN1)
    Shape(22528, 768, 3072, ("just_above", "k3072"), ENCODER_VARIANTS, (1, 0)),         # 88 x 3 = 264 (FFN2)
    Shape(51200, 2304, 768, ("many",), ALL_VARIANTS, (1, 0)),                           # 200 x 9 = 1800 (CLIP ViT-B/32 x 1024, QKV)
    Shape(204800, 2304, 768, ("many", "production"), [BIAS_F32, Variant(EPI_BIAS, None, True, True)], (1, 0)),  # 800 x 9 = 7200
    Shape(102400, 768, 3072, ("many", "k3072"), ENCODER_VARIANTS, (1, 0)),              # 400 x 3 = 1200 (FFN2)
    Shape(8960, 2304, 768, ("pad_skip", "just_above"), ENCODER_VARIANTS, (1, 0)),       # ntm = 35 -> 40 x 9 = 360
    Shape(29000, 768, 768, ("pad_skip", "ragged_m", "just_above"), ENCODER_VARIANTS, (1, 0)),   # ntm = 114 -> 120 x 3 = 360
    Shape(70001, 1024, 256, ("pad_skip", "ragged_m", "many"), ENCODER_VARIANTS, (1, 0)),        # ntm = 274 -> 280 x 4 = 1120
    Shape(35000, 320, 96, ("ragged_n", "ragged_m", "pad_skip", "just_above"), RAGGED_N_VARIANTS, (1, 0)),  # 144 x 2 = 288
    Shape(131072, 320, 96, ("ragged_n", "many"), RAGGED_N_VARIANTS, (1, 0)),            # 512 x 2 = 1024
    Shape(20480, 33 * 32, 128, ("ragged_n", "just_above"), RAGGED_N_VARIANTS, (1, 0)),  # 80 x 5 = 400: column tiles 0 2 4 1 3 per workgroup
    Shape(100000, 33 * 32, 128, ("ragged_n", "ragged_m", "pad_skip", "many"), RAGGED_N_VARIANTS, (1, 0)),  # 392 x 5 = 1960
    Shape(30000, 516, 64, ("n_mod_32", "ragged_n", "short_k", "just_above"), F32_ONLY_VARIANTS, (1, 0)),   # 120 x 3 = 360
    Shape(30000, 515, 64, ("n_mod_32", "ragged_n", "short_k", "just_above"), F32_ONLY_VARIANTS, (1,)),     # sixteen-wave by the (N & 3) rule
    Shape(120000, 516, 96, ("n_mod_32", "ragged_n", "many"), F32_ONLY_VARIANTS, (1,)),  # 472 x 3 = 1416
    Shape(120000, 515, 96, ("n_mod_32", "ragged_n", "many"), F32_ONLY_VARIANTS, (1,)),
    Shape(40960, 768, 32, ("short_k", "just_above"), ENCODER_VARIANTS, (1, 0)),         # 160 x 3 = 480, one K step per tile
    Shape(40000, 768, 64, ("short_k", "ragged_m", "pad_skip", "just_above"), ENCODER_VARIANTS, (1, 0)),  # ntm = 157 -> 160 x 3, two K steps
    Shape(140000, 1024, 32, ("short_k", "ragged_m", "pad_skip", "many"), ENCODER_VARIANTS, (1, 0)),      # ntm = 547 -> 552 x 4 = 2208
]
CLASSES = ("just_above", "many", "production", "k3072", "pad_skip", "ragged_m", "ragged_n", "n_mod_32", "short_k")

STAGGER_SHAPE = (51200, 2304, 768)            # a "many" shape, repeated with MQ_GEMM_OPT_STAGGER = 0, 1, 16
SPLITK_SHAPES = [(6144, 3072, 768), (29000, 768, 768)]
SPLITK_NSPLIT = (2, 3)

# section 2 (tests/gemm_stream_child.py): moderate shapes run under MQ_GEMM_WGS = 8, 16, 0 in child processes
CHILD_WGS = (8, 16, 0)
CHILD_CASES = [(5000, 768, 768, Variant(EPI_BIAS, None, False, True)),
               (5000, 3072, 768, Variant(EPI_BIAS_GELU, None, True, True)),
               (4100, 768, 3072, Variant(EPI_BIAS_RESIDUAL, "pair", True, True)),
               (2049, 320, 96, Variant(EPI_BIAS_RESIDUAL, "f32", False, False))]


def shape_id(s):
    return f"{s.M}x{s.N}x{s.K}"


def variant_id(v):
    return f"epi{v.epi}-{v.res or 'nores'}-{'pair' if v.osp else 'f32'}-{'tiled' if v.tiled else 'rowmajor'}"


def stream_cases():
    """(shape, variant, wide) of oracle A"""
    return [(s, v, wide) for s in STREAM_SHAPES for v in s.variants for wide in s.wides]


def case_id(case):
    s, v, wide = case
    return f"{shape_id(s)}-{variant_id(v)}-wide{wide}"
