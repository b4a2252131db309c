"""Which layer loop an encoder forward runs (csrc/encoder_plan.h), walked on the CPU through om_debug_encoder_plan, and
what the two host-side questions that share the plan answer: om_encoder_workspace_bytes[_packed] and om_encoder_packed_supported.

Every expected value of the decision table is written out by hand from the rules.  The byte counts and the packed-supported answers
are those of the library before encoder_plan.h existed (commit 00a3882, built and asked on the CPU): moving the decision into one
function changes none of them."""
import ctypes as C
import contextlib

from openmatch_amd import native as N

F32, BF16, F16 = N.OM_F32, N.OM_BF16, N.OM_F16
FUSED, PENDING, FEW32, PLAIN, MODERN, T5_FUSED, T5_PLAIN = (N.ENC_PATH[k] for k in (
    "bert_fused", "bert_pending_ln", "bert_few32", "bert_plain", "modernbert", "t5_fused", "t5_plain"))
FEW, TWO, LO8 = 1 << 8, 1 << 9, 1 << 10
REFUSED = -1
# include/openmatch_hip.h: OM_OPT_*
OPT_FUSED_LN, OPT_ATTENTION_FAST, OPT_TWO_PLANE, OPT_GEMM_VARIANT, OPT_SKINNY_M, OPT_FEW_ROWS_LN_FUSE = 0, 2, 11, 12, 19, 21

# tests/test_distilbert_mpnet.py: the widths of BIAS_PATHS
SMALL = dict(hidden=256, n_heads=4, head_dim=64, ffn=1024)
D32 = dict(hidden=128, n_heads=4, head_dim=32, ffn=512)
D32W = dict(hidden=256, n_heads=8, head_dim=32, ffn=1024)
BASE = dict(hidden=768, n_heads=12, head_dim=64, ffn=3072)
ODD = dict(hidden=320, n_heads=5, head_dim=64, ffn=1280)          # rows of whole 128 bytes, no multiple of 256


def bert(dtype, shape=BASE, **kw):
    return dict(dict(arch=N.ARCH_BERT, dtype=dtype, n_layers=12, vocab=30522, max_pos=512, type_vocab=2, act=N.ACT_GELU_ERF, ln_eps=1e-12,
                     pooling=N.POOL_FIRST, **shape), **kw)


def mpnet(dtype, shape):
    return bert(dtype, shape, n_layers=2, type_vocab=0, max_pos=516, rel_buckets=32, rel_max_dist=128, pooling=N.POOL_MEAN)


def t5(dtype, **kw):
    return dict(dict(arch=N.ARCH_T5, dtype=dtype, hidden=512, n_heads=8, head_dim=64, ffn=2048, n_layers=6, vocab=32128, act=N.ACT_RELU,
                     ln_eps=1e-6, rel_buckets=32, rel_max_dist=128, pooling=N.POOL_MEAN), **kw)


def modernbert(dtype, **kw):
    return dict(dict(arch=N.ARCH_MODERNBERT, dtype=dtype, n_layers=22, vocab=50368, max_pos=8192, act=N.ACT_GELU_ERF, ln_eps=1e-5,
                     pooling=N.POOL_FIRST, rope_theta_global=160000.0, rope_theta_local=10000.0, half_window=64, sliding_layers=0x36db6d,
                     **dict(BASE, ffn=1152)), **kw)


def plan(cfg, B, L, packed=0, gated=0, rel=None, hidden=0):
    """om_debug_encoder_plan; rel defaults to what the configuration asks for (T5: always; BERT family: rel_buckets > 0)"""
    c = N.OmEncoderConfig(**cfg)
    if rel is None:
        rel = cfg["arch"] == N.ARCH_T5 or cfg.get("rel_buckets", 0) > 0
    return N.lib().om_debug_encoder_plan(C.byref(c), int(gated), int(rel), B, L, packed, int(hidden))


@contextlib.contextmanager
def switched(opt, value):
    lib = N.lib()
    before = lib.om_debug_option_value(opt)
    N.check(lib.om_debug_option(opt, value))
    try:
        yield
    finally:
        N.check(lib.om_debug_option(opt, before))


# (name, configuration, B, L, keyword arguments of plan(), expected word) at the default switches:
# OM_OPT_ENCODER_FUSED_LN 1, OM_OPT_ENCODER_TWO_PLANE 3, OM_OPT_GEMM_SKINNY_M 1 024, OM_OPT_FEW_ROWS_LN_FUSE 64, OM_OPT_GEMM_VARIANT 0
TABLE = [
    # ---- the 13 rows of tests/test_distilbert_mpnet.py BIAS_PATHS (packed: a legal bound of that batch)
    ("plain_f32", mpnet(F32, SMALL), 6, 128, {}, PLAIN),                        # float32: nothing fuses, no few-rows kernel
    ("plain_f16", mpnet(F16, D32), 12, 128, {}, PLAIN),                         # 1 536 rows > 1 024; hidden 128 is no multiple of 256
    ("few_rows_ln_folded", mpnet(F16, SMALL), 2, 30, {}, PENDING | FEW),        # 60 rows <= 64
    ("few_rows", mpnet(F16, SMALL), 6, 128, {}, FEW32 | FEW),                   # 64 < 768 rows <= 1 024
    ("fused", mpnet(F16, SMALL), 12, 128, {}, FUSED | TWO),                     # 1 536 rows, widths of 256; bit 1 of the two-plane switch
    ("fused_bf16", mpnet(BF16, SMALL), 12, 128, {}, FUSED | TWO),               # ... bit 0
    ("packed", mpnet(BF16, SMALL), 24, 128, dict(packed=1536), FUSED | TWO),
    ("long", mpnet(F16, SMALL), 4, 384, {}, FUSED | TWO),
    ("long_packed", mpnet(F16, SMALL), 8, 384, dict(packed=2048), FUSED | TWO),
    ("long_f32", mpnet(F32, SMALL), 2, 300, {}, PLAIN),
    ("d32", mpnet(F32, D32), 6, 128, {}, PLAIN),
    ("d32_long", mpnet(F16, D32), 3, 300, {}, FEW32 | FEW),                     # 900 rows
    ("d32_packed", mpnet(F16, D32W), 24, 128, dict(packed=1536), FUSED | TWO),
    # ---- T5
    ("t5_fused", t5(BF16), 16, 128, {}, T5_FUSED),
    ("t5_fused_f16_tanh", t5(F16, act=N.ACT_GELU_TANH), 16, 128, {}, T5_FUSED),
    ("t5_f32", t5(F32), 16, 128, {}, T5_PLAIN),
    ("t5_few_rows", t5(F16), 4, 128, {}, T5_PLAIN | FEW),                       # 512 rows <= 1 024: the exception of rule 4 is BERT's
    ("t5_few_rows_bf16", t5(BF16), 4, 128, {}, T5_PLAIN | FEW),
    ("t5_gated", t5(BF16, act=N.ACT_GELU_TANH), 16, 128, dict(gated=1), T5_PLAIN),
    ("t5_packed", t5(BF16), 16, 128, dict(packed=1024), T5_FUSED),
    ("t5_packed_gated", t5(BF16, act=N.ACT_GELU_TANH), 16, 128, dict(packed=1024, gated=1), REFUSED),
    ("t5_no_table", t5(BF16), 16, 128, dict(rel=0), REFUSED),
    # ---- ModernBERT
    ("modernbert", modernbert(F16), 16, 128, {}, MODERN),
    ("modernbert_f32", modernbert(F32), 16, 128, {}, MODERN),
    ("modernbert_few_rows", modernbert(BF16), 4, 32, {}, MODERN | FEW),         # its contractions still run on the few-rows kernel
    ("modernbert_packed", modernbert(F16), 16, 128, dict(packed=1024), REFUSED),
    # ---- rule edges, bert-base widths
    ("rows_64", bert(F16), 2, 32, {}, PENDING | FEW),                           # OM_OPT_FEW_ROWS_LN_FUSE
    ("rows_65", bert(F16), 5, 13, {}, FEW32 | FEW),
    ("rows_64_bf16", bert(BF16), 2, 32, {}, PENDING | FEW),
    ("rows_1024", bert(F16), 8, 128, {}, FEW32 | FEW),                          # OM_OPT_GEMM_SKINNY_M
    ("rows_1025", bert(F16), 25, 41, {}, FUSED | TWO),                          # contractions over 1 280 rows: whole tiles
    ("bf16_511", bert(BF16), 7, 73, {}, FEW32 | FEW),
    ("bf16_512", bert(BF16), 4, 128, {}, FUSED | TWO),                          # few rows give way to the two-plane fused path
    ("bf16_1024", bert(BF16), 8, 128, {}, FUSED | TWO),
    ("f16_511", bert(F16), 7, 73, {}, FEW32 | FEW),
    ("f16_512", bert(F16), 4, 128, {}, FEW32 | FEW),                            # float16 keeps the few-rows path up to 1 024 rows
    ("hidden_not_256", bert(F16, ODD), 12, 128, {}, PLAIN),
    ("hidden_not_256_few", bert(F16, ODD), 2, 30, {}, FEW32 | FEW),             # K = 320: the pending-LayerNorm epilogues take K % 128 == 0
    ("relu_bert_bf16", bert(BF16, act=N.ACT_RELU), 12, 128, {}, PLAIN),         # the fused epilogues are erf-GELU's
    ("no_layers", bert(F16, n_layers=0), 12, 128, {}, PLAIN),
    ("no_layers_few", bert(F16, n_layers=0), 2, 32, {}, PLAIN | FEW),
    ("hidden_states_too", bert(F16), 12, 128, dict(hidden=1), FUSED | TWO),
    ("empty_batch", bert(F16), 0, 128, {}, 0),
    # ---- refusals
    ("bad_heads", bert(F16, head_dim=48), 12, 128, {}, REFUSED),
    ("f16_relu_bert", bert(F16, act=N.ACT_RELU), 12, 128, {}, REFUSED),
    ("L_1025", bert(F16, max_pos=2048), 2, 1025, {}, REFUSED),
    ("L_beyond_table", bert(F16), 2, 513, {}, REFUSED),
    ("table_without_buckets", bert(F16), 12, 128, dict(rel=1), REFUSED),
    ("buckets_without_table", mpnet(F16, SMALL), 12, 128, dict(rel=0), REFUSED),
    ("packed_f32", bert(F32), 12, 128, dict(packed=1024), REFUSED),
    ("packed_hidden_states", bert(F16), 12, 128, dict(packed=1024, hidden=1), REFUSED),
    ("packed_no_pooling", bert(F16, pooling=N.POOL_NONE), 12, 128, dict(packed=1024), REFUSED),
    ("packed_300_rows", bert(F16), 12, 128, dict(packed=300), REFUSED),
    ("packed_256_rows", bert(F16), 12, 128, dict(packed=256), REFUSED),
    ("packed_beyond_batch", bert(F16), 12, 128, dict(packed=1792), REFUSED),    # > 1 536 + 255
    ("packed_whole_batch", bert(F16), 12, 128, dict(packed=1536), FUSED | TWO),
    ("packed_hidden_not_256", bert(F16, ODD), 12, 128, dict(packed=1024), REFUSED),
]

# (switch, value, rows of the same form) -- what moves when a switch does
SWITCHED = [
    (OPT_FUSED_LN, 0, [("fused", bert(F16), 12, 128, {}, PLAIN), ("t5", t5(BF16), 16, 128, {}, T5_PLAIN),
                       ("packed", bert(F16), 12, 128, dict(packed=1024), REFUSED), ("few", bert(F16), 2, 32, {}, PENDING | FEW)]),
    (OPT_GEMM_VARIANT, 2, [("fused", bert(F16), 12, 128, {}, PLAIN), ("t5", t5(BF16), 16, 128, {}, T5_PLAIN),
                           ("packed", bert(BF16), 12, 128, dict(packed=1024), REFUSED)]),
    (OPT_TWO_PLANE, 0, [("fused", bert(F16), 12, 128, {}, FUSED), ("fused_bf16", bert(BF16), 12, 128, {}, FUSED),
                        ("few", bert(F16), 6, 128, {}, PLAIN | FEW), ("query", bert(F16), 2, 32, {}, PLAIN | FEW),
                        ("bf16_512", bert(BF16), 4, 128, {}, PLAIN | FEW)]),      # no second plane to stay on the fused path for
    (OPT_TWO_PLANE, 3, [("fused", bert(F16), 12, 128, {}, FUSED | TWO), ("fused_bf16", bert(BF16), 12, 128, {}, FUSED | TWO)]),
    (OPT_TWO_PLANE, 7, [("fused", bert(F16), 12, 128, {}, FUSED | TWO | LO8), ("fused_bf16", bert(BF16), 12, 128, {}, FUSED | TWO),
                        ("few", bert(F16), 6, 128, {}, FEW32 | FEW)]),
    (OPT_SKINNY_M, 0, [("query", bert(F16), 2, 32, {}, PLAIN), ("rows_512", bert(F16), 4, 128, {}, FUSED | TWO)]),
    (OPT_FEW_ROWS_LN_FUSE, 0, [("query", bert(F16), 2, 32, {}, FEW32 | FEW)]),
]


def _walk(rows):
    wrong = []
    for name, cfg, B, L, kw, want in rows:
        got = plan(cfg, B, L, **kw)
        if got != want:
            wrong.append((name, got, want))
    return wrong


def test_encoder_plan_without_a_gpu():
    lib = N.lib()
    assert len({r[0] for r in TABLE}) == len(TABLE)
    assert not _walk(TABLE)
    assert plan(bert(F16, ODD), 12, 128, packed=1024) == REFUSED and b"fused 16-bit path" in lib.om_last_error()
    assert plan(modernbert(F16), 16, 128, packed=1024) == REFUSED and b"not for ModernBERT" in lib.om_last_error()
    assert plan(bert(F16, head_dim=48), 12, 128) == REFUSED and b"head_dim must be 32 or 64" in lib.om_last_error()
    for opt, value, rows in SWITCHED:
        with switched(opt, value):
            assert not _walk(rows), (opt, value)
    assert not _walk(TABLE)          # every switch is back


# ---- what the library answered before the plan existed: rows of B x L tokens, bert-base / t5-base / ModernBERT-base widths
SHAPES = {32: (1, 32), 64: (2, 32), 65: (5, 13), 512: (4, 128), 1024: (8, 128), 1280: (10, 128), 8192: (64, 128)}
WORKSPACE = {      # (arch, dtype, packed_rows) -> bytes per SHAPES entry
    (0, 0, 0): [1084928, 2169344, 2212352, 17314304, 34628096, 43284992, 277021184],
    (0, 1, 0): [5691392, 6639104, 6687232, 19833344, 34923008, 30671360, 170680832],
    (0, 1, 512): [None, None, None, 15117312, 15141888, 15154176, 15486208],
    (0, 1, 4096): [None, None, None, None, None, None, 87926016],
    (0, 2, 0): [5691392, 6639104, 6687232, 19833344, 34923008, 30671360, 170680832],
    (0, 2, 512): [None, None, None, 15117312, 15141888, 15154176, 15486208],
    (0, 2, 4096): [None, None, None, None, None, None, 87926016],
    (1, 0, 0): [1527552, 3005184, 3019520, 24393216, 47998464, 59801088, 378471936],
    (1, 1, 0): [5544192, 6295296, 6296320, 17475072, 29419008, 35390976, 196634112],
    (1, 1, 512): [None, None, None, 17477632, 17502208, 17514496, 17846528],
    (1, 1, 4096): [None, None, None, None, None, None, 101296384],
    (1, 2, 0): [5544192, 6295296, 6296320, 17475072, 29419008, 35390976, 196634112],
    (1, 2, 512): [None, None, None, 17477632, 17502208, 17514496, 17846528],
    (1, 2, 4096): [None, None, None, None, None, None, 101296384],
    (2, 0, 0): [1478144, 2955776, 3011072, 23605760, 47211008, 59013632, 377684480],
    (2, 1, 0): [743936, 1487360, 1528832, 11821568, 23642624, 29553152, 189137408],
    (2, 1, 512): [None, None, None, 11824128, 11848704, 11860992, 12193024],
    (2, 1, 4096): [None, None, None, None, None, None, 94782720],
    (2, 2, 0): [743936, 1487360, 1528832, 11821568, 23642624, 29553152, 189137408],
    (2, 2, 512): [None, None, None, 11824128, 11848704, 11860992, 12193024],
    (2, 2, 4096): [None, None, None, None, None, None, 94782720],
}
MPNET_MEAN_HEAD = ([5836288, 6879744, 6882304, 22183168, 38835456, 35365120, 196470016], 101132288)


def _sized(arch, dtype, **kw):
    base = dict(arch=arch, dtype=dtype, hidden=768, n_layers=12, n_heads=12, head_dim=64, ffn=3072, vocab=30522, max_pos=512, type_vocab=2,
                act=N.ACT_GELU_ERF, ln_eps=1e-12, pooling=N.POOL_FIRST)
    if arch == N.ARCH_T5:
        base.update(act=N.ACT_RELU, rel_buckets=32, rel_max_dist=128, type_vocab=0)
    if arch == N.ARCH_MODERNBERT:
        base.update(rope_theta_global=160000.0, rope_theta_local=10000.0, half_window=64, sliding_layers=0xdb6, type_vocab=0)
    base.update(kw)
    return N.OmEncoderConfig(**base)


def test_workspace_bytes_are_those_of_the_library_before_the_plan():
    lib = N.lib()
    for (arch, dtype, rows), want in WORKSPACE.items():
        c = _sized(arch, dtype)
        for (m, (B, L)), bytes_ in zip(SHAPES.items(), want):
            if bytes_ is None:
                continue
            got = lib.om_encoder_workspace_bytes_packed(C.byref(c), B, L, rows) if rows else lib.om_encoder_workspace_bytes(C.byref(c), B, L)
            assert got == bytes_, (arch, dtype, rows, m, got, bytes_)
    c = _sized(N.ARCH_BERT, F16, pooling=N.POOL_MEAN, rel_buckets=32, rel_max_dist=128, head_in=768, head_out=128)      # mean pooling, a bias table, a head
    assert [lib.om_encoder_workspace_bytes(C.byref(c), *SHAPES[m]) for m in SHAPES] == MPNET_MEAN_HEAD[0]
    assert lib.om_encoder_workspace_bytes_packed(C.byref(c), 64, 128, 4096) == MPNET_MEAN_HEAD[1]
    # the f32-stream buffers follow OM_OPT_GEMM_SKINNY_M alone: the two-plane switch moves no byte
    c = _sized(N.ARCH_BERT, BF16)
    with switched(OPT_TWO_PLANE, 0):
        assert lib.om_encoder_workspace_bytes(C.byref(c), 4, 128) == WORKSPACE[(0, 1, 0)][3]


_T5 = dict(arch=N.ARCH_T5, act=N.ACT_RELU)
PACKED_SUPPORTED = [      # (what differs from tests/test_host_logic.py's partial bert-base float16 configuration at 64 x 128, 4 096 rows; the answer)
    ({}, 1), (dict(dtype=F32), 0), (dict(dtype=BF16), 1), (dict(hidden=128), 0), (dict(act=N.ACT_RELU), 0),
    (dict(_T5, dtype=BF16), 1), (dict(_T5), 1), (dict(_T5, gated=1), 0),
    (dict(_T5, act=N.ACT_GELU_TANH), 0),                       # float16 T5 with tanh-GELU: the forward takes it, this answer does not
    (dict(_T5, dtype=BF16, act=N.ACT_GELU_TANH), 1), (dict(arch=N.ARCH_MODERNBERT), 0),
    (dict(rows=256), 0), (dict(rows=4100), 0), (dict(rows=8192), 1), (dict(rows=7936), 1), (dict(rows=8448), 0),
    (dict(L=512), 1), (dict(L=1100), 0),
    (dict(B=8, L=128, rows=512), 0),                           # the padded form is few rows
    (dict(B=9, L=128, rows=512), 1),
    (dict(n_layers=0), 0), (dict(hidden=772), 0), (dict(ffn=3200), 0), (dict(B=0), 0),
    (dict(n_heads=12, head_dim=64, pooling=N.POOL_MEAN), 1), (dict(hidden=256, ffn=1024, n_heads=8, head_dim=32), 1),
]
# (switch, value) -> answers for [bert float16, bert bfloat16, t5 bfloat16]
PACKED_SUPPORTED_SWITCHED = {(OPT_FUSED_LN, 0): [0, 0, 0], (OPT_GEMM_VARIANT, 2): [0, 0, 0], (OPT_ATTENTION_FAST, 0): [1, 0, 0],
                             (OPT_SKINNY_M, 8192): [0, 0, 0]}


def _supported(gated=0, B=64, L=128, rows=4096, **kw):
    cfg = dict(arch=N.ARCH_BERT, dtype=F16, act=N.ACT_GELU_ERF, hidden=768, ffn=3072, n_layers=12)      # no heads, pooling, position table
    cfg.update(kw)
    return N.lib().om_encoder_packed_supported(C.byref(N.OmEncoderConfig(**cfg)), gated, B, L, rows)


def test_packed_supported_answers_are_those_of_the_library_before_the_plan():
    wrong = [(kw, _supported(**kw), want) for kw, want in PACKED_SUPPORTED if _supported(**kw) != want]
    assert not wrong, wrong
    for (opt, value), want in PACKED_SUPPORTED_SWITCHED.items():
        with switched(opt, value):
            assert [_supported(), _supported(dtype=BF16), _supported(**dict(_T5, dtype=BF16))] == want, (opt, value)
    assert _supported() == 1
