"""What a training step runs (csrc/train_plan.h), walked on the CPU through om_debug_train_plan, and what the host-side
questions that share the plan answer: the four *_bytes entries, om_encoder_train_packed_supported and the refusals of the step's entries.

Every expected word of the decision and switch tables is written out by hand from the rules.  The byte counts, the packed-supported
answers and the refusal texts of the entries are those of the library before train_plan.h existed (commit e010628, built and asked on
the CPU): moving the decisions into one function changes none of them."""
import ctypes as C
import contextlib

from openmatch_amd import native as N

F32, BF16, F16 = N.OM_F32, N.OM_BF16, N.OM_F16
# om_debug_train_plan's word (include/openmatch_hip.h)
HIDDEN, PLAIN, CLS, MEAN = 0, 1, 2, 3
T5, GATED, REL, PACKED, BERT16, RES32, PRE, KEEP, EARLY, LANE, ATOM = (1 << b for b in range(2, 13))
REFUSED = -1
# include/openmatch_hip.h: OM_OPT_*
OPT_ATTENTION_FAST, OPT_WGRAD_STREAM, OPT_WGRAD_BATCH, OPT_TAPE_GRAD, OPT_RES32 = 2, 8, 14, 17, 18


def WB(n):
    return n << 16


SMALL = dict(hidden=256, n_heads=4, head_dim=64, ffn=1024)
D32 = dict(hidden=128, n_heads=4, head_dim=32, ffn=512)
D32W = dict(hidden=256, n_heads=8, head_dim=32, ffn=1024)
D128 = dict(hidden=128, n_heads=2, head_dim=64, ffn=512)
BASE = dict(hidden=768, n_heads=12, head_dim=64, ffn=3072)
ODD = dict(hidden=320, n_heads=5, head_dim=64, ffn=1280)          # rows of whole 128 bytes, no multiple of 128 elements
NARROW = dict(hidden=256, n_heads=4, head_dim=64, ffn=256)        # ffn < 2 * hidden: not bert16


def bert(dtype, shape=BASE, **kw):
    return dict(dict(arch=N.ARCH_BERT, dtype=dtype, n_layers=12, vocab=30522, max_pos=512, type_vocab=2, act=N.ACT_GELU_ERF, ln_eps=1e-12,
                     pooling=N.POOL_FIRST, **shape), **kw)


def small(dtype, shape=SMALL, **kw):
    return bert(dtype, shape, **dict(dict(n_layers=2), **kw))


def mpnet(dtype, shape=SMALL):
    return bert(dtype, shape, n_layers=2, type_vocab=0, max_pos=516, rel_buckets=32, rel_max_dist=128, pooling=N.POOL_MEAN)


def t5(dtype, **kw):
    return dict(dict(arch=N.ARCH_T5, dtype=dtype, hidden=512, n_heads=8, head_dim=64, ffn=2048, n_layers=6, vocab=32128, act=N.ACT_RELU,
                     ln_eps=1e-6, rel_buckets=32, rel_max_dist=128, pooling=N.POOL_MEAN), **kw)


def plan(cfg, B, L, packed=0, hidden=0, rel=None, backward=0, flags=-1):
    """om_debug_train_plan; rel defaults to what the configuration asks for (T5: always; BERT family: rel_buckets > 0)"""
    c = N.OmEncoderConfig(**cfg)
    if rel is None:
        rel = cfg["arch"] == N.ARCH_T5 or cfg.get("rel_buckets", 0) > 0
    return N.lib().om_debug_train_plan(C.byref(c), B, L, packed, int(hidden), int(rel), int(backward), flags)


@contextlib.contextmanager
def switched(opt, value):
    lib = N.lib()
    before = lib.om_debug_option_value(opt)
    N.check(lib.om_debug_option(opt, value))
    try:
        yield
    finally:
        N.check(lib.om_debug_option(opt, before))


# what a 16-bit BERT step with ffn >= 2 * hidden carries at the default switches, and what its backward adds
B16 = BERT16 | RES32 | PRE
BWD = LANE | WB(4)
# (name, configuration, B, L, keyword arguments of plan(), the forward's word, the backward's word) at the default switches:
# OM_OPT_TRAIN_RES32 1, OM_OPT_TRAIN_TAPE_GRAD 1, OM_OPT_TRAIN_WGRAD_STREAM 1, OM_OPT_TRAIN_WGRAD_BATCH 4, OM_OPT_ATTENTION_FAST 1
TABLE = [
    # ---- bert-base at the training batch: 9 216 rows
    ("base_f16", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | BWD),
    ("base_bf16", bert(BF16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | BWD),
    ("base_f32", bert(F32), 72, 128, {}, PLAIN, PLAIN),                          # float32: no tape flags, no keep slices, no direct kernel
    ("base_bf16_mean", bert(BF16, pooling=N.POOL_MEAN), 72, 128, {}, MEAN | B16 | KEEP, MEAN | B16 | KEEP | BWD),
    ("base_f16_hidden", bert(F16), 72, 128, dict(hidden=1), HIDDEN | B16 | KEEP, HIDDEN | B16 | KEEP | BWD),
    # ---- hidden 256 / ffn 1 024
    ("small_f16", small(F16), 12, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | BWD),
    ("small_f16_16_rows", small(F16), 1, 16, {}, CLS | B16, CLS | B16 | LANE),   # M < 32: no keep slices, so no batch
    ("small_bf16_32_rows", small(BF16), 2, 16, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | BWD),
    ("small_f32", small(F32), 12, 128, {}, PLAIN, PLAIN),
    ("small_f16_no_layers", small(F16, n_layers=0), 12, 128, {}, PLAIN | B16 | KEEP, CLS | B16 | KEEP | BWD),      # the forward's tail asks for layers
    # ---- widths the direct weight-gradient kernels do not take
    ("odd_f16", small(F16, ODD), 12, 128, {}, CLS | B16, CLS | B16),             # 320 % 128: no lane; % 256: no keep
    ("odd_f32", small(F32, ODD), 12, 128, {}, PLAIN, PLAIN),
    ("d32_f16", small(F16, D32), 12, 128, {}, CLS | B16, CLS | B16 | LANE),      # widths of 128: the lane, no batch
    ("d32_f32", small(F32, D32), 6, 128, {}, PLAIN, PLAIN),
    ("d32w_bf16", small(BF16, D32W), 12, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | BWD),
    # ---- ffn < 2 * hidden in 16 bits: not bert16 -- no res32; the forward's tail is f32 for pooling "first" alone, the backward's never
    ("narrow_f16_first", small(F16, NARROW), 12, 128, {}, CLS | PRE | KEEP, PLAIN | PRE | KEEP | BWD),
    ("narrow_f16_mean", small(F16, NARROW, pooling=N.POOL_MEAN), 12, 128, {}, PLAIN | PRE | KEEP, PLAIN | PRE | KEEP | BWD),
    # ---- MPNet: a bucket table
    ("mpnet_f16", mpnet(F16), 12, 128, {}, MEAN | REL | B16 | KEEP, MEAN | REL | B16 | KEEP | BWD),
    ("mpnet_f32", mpnet(F32), 6, 128, {}, PLAIN | REL, PLAIN | REL),
    # ---- T5: no lane, no batch, no keep slices; 16-bit runs still carry the pre_grad flag (nothing of a T5 step reads it)
    ("t5_relu_bf16", t5(BF16), 16, 128, {}, PLAIN | T5 | PRE, PLAIN | T5 | PRE),
    ("t5_gated_f16", t5(F16, act=N.ACT_GELU_TANH), 16, 128, {}, PLAIN | T5 | GATED | PRE, PLAIN | T5 | GATED | PRE),
    ("t5_relu_f32", t5(F32), 16, 128, {}, PLAIN | T5, PLAIN | T5),
    ("t5_gated_f32", t5(F32, act=N.ACT_GELU_TANH), 16, 128, {}, PLAIN | T5 | GATED, PLAIN | T5 | GATED),
    ("t5_hidden", t5(BF16), 16, 128, dict(hidden=1), HIDDEN | T5 | PRE, HIDDEN | T5 | PRE),
    ("t5_no_table", t5(BF16), 16, 128, dict(rel=0), PLAIN | T5 | PRE, PLAIN | T5 | PRE),      # (refused where final_ln_g is looked at: train.hip)
    # ---- packed rows: 24 x 128 ragged in 1 536 rows
    ("packed_f16", small(F16), 24, 128, dict(packed=1536), CLS | PACKED | B16 | KEEP, CLS | PACKED | B16 | KEEP | BWD),
    ("packed_bf16_mean", small(BF16, pooling=N.POOL_MEAN), 24, 128, dict(packed=1536), MEAN | PACKED | B16 | KEEP, MEAN | PACKED | B16 | KEEP | BWD),
    ("packed_mpnet", mpnet(BF16), 24, 128, dict(packed=1536), MEAN | REL | PACKED | B16 | KEEP, MEAN | REL | PACKED | B16 | KEEP | BWD),
    ("packed_t5", t5(BF16), 24, 128, dict(packed=1536), PLAIN | T5 | PACKED | PRE, PLAIN | T5 | PACKED | PRE),
    ("packed_t5_gated", t5(F16, act=N.ACT_GELU_TANH), 24, 128, dict(packed=1536), PLAIN | T5 | GATED | PACKED | PRE, PLAIN | T5 | GATED | PACKED | PRE),
    # ---- an empty batch: nothing runs, nothing is refused (the packed bound is never looked at)
    ("empty", small(F16), 0, 128, {}, 0, 0),
    ("empty_packed", small(F16), 0, 128, dict(packed=300), 0, 0),
    # ---- refusals
    ("packed_300", small(F16), 24, 128, dict(packed=300), REFUSED, REFUSED),
    ("packed_hidden", small(F16), 24, 128, dict(packed=1536, hidden=1), REFUSED, REFUSED),
    ("packed_narrow", small(F16, NARROW), 24, 128, dict(packed=1536), REFUSED, REFUSED),
    ("table_without_buckets", small(F16), 12, 128, dict(rel=1), REFUSED, REFUSED),
    ("buckets_without_table", mpnet(F16), 12, 128, dict(rel=0), REFUSED, REFUSED),
]

# a backward reads the tape as its forward wrote it (flags: 1 res32, 2 pre_grad), not as the switches say now
TAPE_FLAGS = [
    ("base_f16", bert(F16), 72, 128, [CLS | BERT16 | KEEP | BWD, CLS | BERT16 | RES32 | KEEP | BWD, CLS | BERT16 | PRE | KEEP | BWD, CLS | B16 | KEEP | BWD]),
    ("base_f32", bert(F32), 72, 128, [PLAIN, PLAIN | RES32, PLAIN | PRE, PLAIN | RES32 | PRE]),      # taken as given (the map is keyed by address)
    ("t5_bf16", t5(BF16), 16, 128, [PLAIN | T5, PLAIN | T5 | RES32, PLAIN | T5 | PRE, PLAIN | T5 | RES32 | PRE]),
]

# (switch, value, rows of TABLE's form) -- what moves when a switch does
SWITCHED = [
    (OPT_RES32, 0, [("base", bert(F16), 72, 128, {}, CLS | BERT16 | PRE | KEEP, CLS | BERT16 | PRE | KEEP | BWD),
                    ("flags_3", bert(F16), 72, 128, dict(flags=3), CLS | B16 | KEEP, CLS | B16 | KEEP | BWD),      # the tape's flags, not the switch
                    ("t5", t5(BF16), 16, 128, {}, PLAIN | T5 | PRE, PLAIN | T5 | PRE)]),
    (OPT_TAPE_GRAD, 0, [("base", bert(F16), 72, 128, {}, CLS | BERT16 | RES32 | KEEP, CLS | BERT16 | RES32 | KEEP | BWD),
                        ("t5", t5(BF16), 16, 128, {}, PLAIN | T5, PLAIN | T5)]),
    (OPT_WGRAD_STREAM, 0, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | WB(4))]),
    # bit 1: early transposes -- the forward's needs 16 bits and layers, the backward's reuse the bit alone; any non-zero word: the lane
    (OPT_WGRAD_STREAM, 2, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP | EARLY, CLS | B16 | KEEP | EARLY | BWD),
                           ("f32", bert(F32), 72, 128, {}, PLAIN, PLAIN | EARLY),
                           ("no_layers", small(F16, n_layers=0), 12, 128, {}, PLAIN | B16 | KEEP, CLS | B16 | KEEP | EARLY | BWD),
                           ("t5", t5(BF16), 16, 128, {}, PLAIN | T5 | PRE, PLAIN | T5 | PRE)]),
    (OPT_WGRAD_STREAM, 4, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | ATOM | BWD),
                           ("odd", small(F16, ODD), 12, 128, {}, CLS | B16, CLS | B16 | ATOM)]),
    (OPT_WGRAD_STREAM, 8, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | BWD)]),      # bit 3 is the row kernel's own
    (OPT_WGRAD_STREAM, 3, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP | EARLY, CLS | B16 | KEEP | EARLY | BWD)]),
    # layers per launch: clamped to 0 .. 12; the keep slices stay whatever it says
    (OPT_WGRAD_BATCH, -1, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | LANE)]),
    (OPT_WGRAD_BATCH, 0, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | LANE)]),
    (OPT_WGRAD_BATCH, 2, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | LANE | WB(2))]),
    (OPT_WGRAD_BATCH, 12, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | LANE | WB(12)),
                           ("d32", small(F16, D32), 12, 128, {}, CLS | B16, CLS | B16 | LANE)]),
    (OPT_WGRAD_BATCH, 99, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | LANE | WB(12))]),
    (OPT_ATTENTION_FAST, 0, [("base", bert(F16), 72, 128, {}, CLS | B16 | KEEP, CLS | B16 | KEEP | BWD),
                             ("packed", small(F16), 24, 128, dict(packed=1536), REFUSED, REFUSED),
                             ("packed_t5", t5(BF16), 24, 128, dict(packed=1536), REFUSED, REFUSED)]),
]


def _walk(rows):
    wrong = []
    for name, cfg, B, L, kw, fwd, bwd in rows:
        got = (plan(cfg, B, L, **kw), plan(cfg, B, L, backward=1, **kw))
        if got != (fwd, bwd):
            wrong.append((name, got, (fwd, bwd)))
    return wrong


def test_train_plan_without_a_gpu():
    assert len({r[0] for r in TABLE}) == len(TABLE)
    assert not _walk(TABLE)
    for name, cfg, B, L, words in TAPE_FLAGS:
        assert [plan(cfg, B, L, backward=1, flags=f) for f in range(4)] == words, name


def test_train_plan_switches():
    for opt, value, rows in SWITCHED:
        with switched(opt, value):
            assert not _walk(rows), (opt, value)
    assert not _walk(TABLE)          # every switch is back


# ---- refusals: (name, configuration, B, L, keyword arguments, the text) -- every text of rule 1 and of the packed-rows rules; the
# rows that break two rules at once pin the order
_S = small(F16)
LONG = ("packed rows in training: 16-bit BERT-family or T5 encoder, widths of 256, L <= 256, rows a multiple of 256 in [512, B * L) "
        "(om_encoder_train_packed_supported)")
SHORT = "packed rows in training: not for this configuration (om_encoder_train_packed_supported)"
TOGETHER = "relative position bias: rel_bias and rel_buckets must be set together"
REFUSALS = [
    ("arch", dict(_S, arch=N.ARCH_MODERNBERT), 12, 128, {}, "unknown arch"),
    ("dtype", dict(_S, dtype=7), 12, 128, {}, "dtype must be OM_F32, OM_BF16 or OM_F16"),
    ("arch+dtype", dict(_S, arch=N.ARCH_MODERNBERT, dtype=7), 12, 128, {}, "unknown arch"),
    ("t5_d_kv", t5(BF16, head_dim=32, n_heads=16), 16, 128, {}, "T5 training: only d_kv 64 with n_heads*64 == d_model"),
    ("head_dim", dict(_S, head_dim=48), 12, 128, {}, "head_dim must be 32 or 64 with n_heads*head_dim == hidden"),
    ("head_dim+L", dict(_S, head_dim=48), 12, 513, {}, "head_dim must be 32 or 64 with n_heads*head_dim == hidden"),
    ("L_513", _S, 2, 513, {}, "training supports sequence lengths up to 512"),
    ("L_0", _S, 2, 0, {}, "training supports sequence lengths up to 512"),
    ("L_513+f32", small(F32), 2, 513, {}, "training supports sequence lengths up to 512"),
    ("d32_L_300", small(F16, D32), 2, 300, {}, "training with head_dim 32 supports sequence lengths up to 256"),
    ("d32_L_300+f32", small(F32, D32), 2, 300, {}, "training with head_dim 32 supports sequence lengths up to 256"),
    ("f32_L_200", small(F32), 2, 200, {}, "float32 training supports sequence lengths up to 192 (16-bit formats: 512)"),
    ("bert_relu", dict(_S, act=N.ACT_RELU), 12, 128, {}, "BERT training supports the erf-GELU FFN"),
    ("t5_erf", t5(BF16, act=N.ACT_GELU_ERF), 16, 128, {}, "T5 training supports relu and gated gelu_new feed-forward layers"),
    ("row_bytes", small(F16, dict(hidden=96, n_heads=3, head_dim=32, ffn=384)), 12, 128, {}, "hidden/ffn rows must be multiples of 128 bytes"),
    ("row_bytes_f32", small(F32, dict(hidden=32, n_heads=1, head_dim=32, ffn=144)), 12, 128, {}, "hidden/ffn rows must be multiples of 128 bytes"),
    ("pooling", dict(_S, pooling=N.POOL_NONE), 12, 128, {}, "pooling must be first or mean"),
    ("pooling+packed", dict(_S, pooling=N.POOL_NONE), 24, 128, dict(packed=300), "pooling must be first or mean"),
    ("pooling+empty", dict(_S, pooling=N.POOL_NONE), 0, 128, {}, "pooling must be first or mean"),
    ("packed_300", _S, 24, 128, dict(packed=300), LONG),
    ("packed_300_backward", _S, 24, 128, dict(packed=300, backward=1), SHORT),
    ("packed_hidden", _S, 24, 128, dict(packed=1536, hidden=1), LONG),
    ("packed_hidden_backward", _S, 24, 128, dict(packed=1536, hidden=1, backward=1), SHORT),
    ("packed_f32", small(F32), 24, 128, dict(packed=1536), LONG),
    ("packed+table", _S, 24, 128, dict(packed=300, rel=1), LONG),
    ("packed+table_backward", _S, 24, 128, dict(packed=300, rel=1, backward=1), SHORT),
    ("table_without_buckets", _S, 12, 128, dict(rel=1), TOGETHER),
    ("table_without_buckets_backward", _S, 12, 128, dict(rel=1, backward=1), TOGETHER),
    ("table_without_buckets_hidden", _S, 12, 128, dict(rel=1, hidden=1), TOGETHER),
    ("buckets_without_table", mpnet(F16), 12, 128, dict(rel=0), TOGETHER),
    ("packed_ok+table", _S, 24, 128, dict(packed=1536, rel=1), TOGETHER),
]


def test_train_plan_refusals():
    lib = N.lib()
    assert plan(_S, 12, 128) >= 0
    for name, cfg, B, L, kw, text in REFUSALS:
        assert plan(cfg, B, L, **kw) == REFUSED, name
        assert lib.om_last_error().decode() == "om_debug_train_plan: " + text, name
    assert lib.om_debug_train_plan(None, 12, 128, 0, 0, 0, 0, -1) == REFUSED


# ---- the entries themselves, asked on the CPU with addresses that are never read: every refusal here comes before the first HIP call.
# The weight- and buffer-dependent checks stay in train.hip, between the plan's refusals: these rows pin where.
_A = 0x10000


def _forward(cfg, B, L, packed=0, hidden=0, rel=0, type_emb=1, tape_bytes=1 << 40, align=0):
    lib = N.lib()
    layers = (N.OmLayerWeights * 1)()
    c = N.OmEncoderConfig(**cfg)
    w = N.OmEncoderWeights(layers_host=layers, rel_bias=_A if rel else None, type_emb=_A if type_emb else None)
    tail = (0.1, 0.1, 1, _A + align, tape_bytes, _A, _A, 1 << 40, None)
    if packed:
        rc = lib.om_encoder_train_forward_packed(C.byref(c), C.byref(w), _A, _A, _A, B, L, packed, *tail)
    elif hidden:
        rc = lib.om_encoder_train_forward_hidden(C.byref(c), C.byref(w), _A, _A, _A, B, L, *tail)
    else:
        rc = lib.om_encoder_train_forward(C.byref(c), C.byref(w), _A, _A, _A, B, L, *tail)
    return lib.om_last_error().decode() if rc else ""


def _backward(cfg, B, L, packed=0, rel=0):
    """a workspace of 0 bytes: "workspace too small" ends every call that passes the packed-rows rule"""
    lib = N.lib()
    layers, glayers = (N.OmLayerWeights * 1)(), (N.OmLayerGrads * 1)()
    c = N.OmEncoderConfig(**cfg)
    w = N.OmEncoderWeights(layers_host=layers, rel_bias=_A if rel else None)
    g = N.OmEncoderGrads(layers_host=glayers)
    tail = (0.1, 0.1, 1, _A, _A, C.byref(g), _A, 0, None)
    if packed:
        rc = lib.om_encoder_train_backward_packed(C.byref(c), C.byref(w), _A, _A, _A, B, L, packed, *tail)
    else:
        rc = lib.om_encoder_train_backward(C.byref(c), C.byref(w), _A, _A, _A, B, L, *tail)
    return lib.om_last_error().decode() if rc else ""


def test_entry_refusals_are_those_of_the_library_before_the_plan():
    cfg_, fwd_, bwd_ = "check_train_cfg: ", "train_forward_impl: ", "train_backward_impl: "
    assert _forward(dict(_S, arch=N.ARCH_MODERNBERT), 12, 128) == cfg_ + "unknown arch"
    assert _forward(dict(_S, pooling=N.POOL_NONE), 24, 128, packed=300) == cfg_ + "pooling must be first or mean"
    assert _forward(dict(_S, pooling=N.POOL_NONE), 0, 128) == cfg_ + "pooling must be first or mean"
    assert _forward(_S, 0, 128, packed=300) == ""
    assert _forward(_S, 24, 128, packed=300, align=8) == fwd_ + "tape/workspace must be 256-byte aligned"
    assert _forward(_S, 24, 128, packed=300) == fwd_ + LONG
    assert _forward(_S, 24, 128, packed=300, rel=1) == fwd_ + LONG
    assert _forward(_S, 24, 128, packed=300, tape_bytes=0) == fwd_ + LONG
    assert _forward(_S, 24, 128, packed=1536, tape_bytes=0) == fwd_ + "tape or workspace too small"
    assert _forward(_S, 12, 128, rel=1, tape_bytes=0) == fwd_ + "tape or workspace too small"
    assert _forward(dict(_S, max_pos=64), 12, 128, rel=1) == fwd_ + "sequence longer than the position table"
    assert _forward(_S, 12, 128, rel=1) == fwd_ + TOGETHER
    assert _forward(_S, 12, 128, rel=1, hidden=1) == fwd_ + TOGETHER
    assert _forward(mpnet(F16), 12, 128, rel=0) == fwd_ + TOGETHER
    assert _forward(dict(_S, type_vocab=0), 12, 128, rel=1) == fwd_ + TOGETHER
    assert _forward(dict(_S, type_vocab=0), 12, 128) == fwd_ + "token types: a type_emb table needs type_vocab > 0"
    assert _forward(t5(BF16), 16, 128, rel=0) == "t5_bias_setup: T5 needs rel_bias and final_ln_g"
    assert _backward(dict(_S, arch=N.ARCH_MODERNBERT), 12, 128) == cfg_ + "unknown arch"
    assert _backward(dict(_S, pooling=N.POOL_NONE), 24, 128, packed=300) == cfg_ + "pooling must be first or mean"
    assert _backward(_S, 0, 128, packed=300) == ""
    assert _backward(_S, 24, 128, packed=300) == bwd_ + SHORT
    assert _backward(_S, 24, 128, packed=300, rel=1) == bwd_ + SHORT
    assert _backward(_S, 24, 128, packed=1536) == bwd_ + "workspace too small"
    assert _backward(_S, 12, 128, rel=1) == bwd_ + "workspace too small"
    with switched(OPT_ATTENTION_FAST, 0):
        assert _forward(_S, 24, 128, packed=1536) == fwd_ + LONG
        assert _backward(_S, 24, 128, packed=1536) == bwd_ + SHORT


# ---- byte counts: name -> (configuration, B, L, om_encoder_tape_bytes, om_encoder_train_workspace_bytes)
BYTES = {
    "base_f16": (bert(F16), 72, 128, 3072245760, 2176303104),
    "base_bf16": (bert(BF16), 72, 128, 3072245760, 2176303104),
    "base_f32": (bert(F32), 72, 128, 5464571904, 1095155712),
    "base_bf16_mean_head": (bert(BF16, pooling=N.POOL_MEAN, head_in=768, head_out=128), 72, 128, 3072061440, 2176118784),
    "small_f16": (small(F16), 12, 128, 29122560, 43835392),
    "small_f16_16_rows": (small(F16), 1, 16, 305152, 7792640),
    "odd_f16": (small(F16, ODD), 12, 128, 36403200, 38082560),
    "odd_f32": (small(F32, ODD), 12, 128, 64911360, 62289920),
    "d32_f16": (small(F16, D32), 12, 128, 14561280, 14200832),
    "d128_f16": (small(F16, D128), 24, 128, 29122560, 25223168),
    "narrow_f16": (small(F16, NARROW), 12, 128, 16539648, 28106752),
    "long_bf16": (small(BF16), 4, 512, 38805504, 55681024),
    "mpnet_f16": (mpnet(F16), 12, 128, 29122560, 44102656),
    "mpnet_f32": (mpnet(F32), 12, 128, 51929088, 48526336),
    "t5_relu_bf16": (t5(BF16), 16, 128, 127991808, 91563008),
    "t5_gated_bf16": (t5(BF16, act=N.ACT_GELU_TANH), 16, 128, 178323456, 112534528),
    "t5_relu_f32": (t5(F32), 16, 128, 255918080, 180954112),
    "t5_gated_f32": (t5(F32, act=N.ACT_GELU_TANH), 16, 128, 356581376, 222897152),
}
# packed rows: the bounds asked, and per configuration [supported, tape bytes, workspace bytes] of each.  24 x 128 = 3 072 tokens
# (base: 72 x 128): 256 is below 512, 1 500 no multiple of 256, 3 072 = B * L and 3 328 beyond it
ROWS = [1536, 1024, 512, 256, 1500, 3072, 2816, 3328, 2560]
_NO = [0, 0, 0]
_REFUSED = [_NO] * 9
PACKED_BYTES = {
    "small_f16": (small(F16), 24, 128, [[1, 29147136, 44161792], [1, 19447808, 32101120], [1, 9748480, 20040448], _NO, _NO, _NO,
                                        [1, 53395456, 74313472], _NO, [1, 48545792, 68283136]]),
    "small_bf16_mean": (small(BF16, pooling=N.POOL_MEAN), 24, 128, [[1, 29147136, 44161792], [1, 19447808, 32101120], [1, 9748480, 20040448], _NO, _NO,
                                                                  _NO, [1, 53395456, 74313472], _NO, [1, 48545792, 68283136]]),
    "d32w_f16": (small(F16, D32W), 24, 128, [[1, 29147136, 44751616], [1, 19447808, 32690944], [1, 9748480, 20630272], _NO, _NO, _NO,
                                             [1, 53395456, 74903296], _NO, [1, 48545792, 68872960]]),
    "mpnet_bf16": (mpnet(BF16), 24, 128, [[1, 29147136, 44429056], [1, 19447808, 32368384], [1, 9748480, 20307712], _NO, _NO, _NO,
                                          [1, 53395456, 74580736], _NO, [1, 48545792, 68550400]]),
    "t5_relu_bf16": (t5(BF16), 24, 128, [[1, 96043008, 78888704], [1, 64061440, 65779456], [1, 32079872, 52670208], _NO, _NO, _NO,
                                         [1, 175996928, 111661824], _NO, [1, 160006144, 105107200]]),
    "t5_gated_f16": (t5(F16, act=N.ACT_GELU_TANH), 24, 128, [[1, 133791744, 97763072], [1, 89227264, 82556672], [1, 44662784, 67350272], _NO, _NO, _NO,
                                                             [1, 245202944, 135779072], _NO, [1, 222920704, 128175872]]),
    "base_bf16": (bert(BF16), 72, 128, [[1, 512409600, 571989504], [1, 341753856, 465032704], [1, 171098112, 358075904], _NO, _NO,
                                        [1, 1024376832, 892859904], [1, 939048960, 839381504], [1, 1109704704, 946338304], [1, 853721088, 785903104]]),
    "narrow_f16": (small(F16, NARROW), 24, 128, _REFUSED),                 # BERT with ffn < 2 * hidden
    "d128_f16": (small(F16, D128), 24, 128, _REFUSED),                     # widths of 128
    "small_f32": (small(F32), 24, 128, _REFUSED),
    "small_f16_L_257": (small(F16), 12, 257, _REFUSED),
    "small_f16_no_layers": (small(F16, n_layers=0), 24, 128, _REFUSED),
    "small_f16_no_pooling": (small(F16, pooling=N.POOL_NONE), 24, 128, _REFUSED),
}
# (switch, value) -> [tape, workspace] of base_f16, base_f32, t5_relu_bf16, then the 1 536-row answers of small_f16 and t5_relu_bf16:
# the f32 sums of res32 move the BERT tape; no other switch moves a byte (the keep slices and x32a / x32b stay reserved)
_DEFAULT = [[3072245760, 2176303104], [5464571904, 1095155712], [127991808, 91563008], [1, 29147136, 44161792], [1, 96043008, 78888704]]
BYTES_SWITCHED = {
    (OPT_RES32, 0): [[2732507136, 2176303104], [5464571904, 1095155712], [127991808, 91563008], [1, 26001408, 44161792], [1, 96043008, 78888704]],
    (OPT_TAPE_GRAD, 0): _DEFAULT, (OPT_WGRAD_STREAM, 0): _DEFAULT, (OPT_WGRAD_STREAM, 2): _DEFAULT, (OPT_WGRAD_BATCH, 0): _DEFAULT,
    (OPT_WGRAD_BATCH, 12): _DEFAULT,
    (OPT_ATTENTION_FAST, 0): _DEFAULT[:3] + [_NO, _NO],
}


def _bytes(cfg, B, L):
    c = N.OmEncoderConfig(**cfg)
    return [N.lib().om_encoder_tape_bytes(C.byref(c), B, L), N.lib().om_encoder_train_workspace_bytes(C.byref(c), B, L)]


def _packed(cfg, B, L, rows):
    lib, c = N.lib(), N.OmEncoderConfig(**cfg)
    return [lib.om_encoder_train_packed_supported(C.byref(c), B, L, rows), lib.om_encoder_tape_bytes_packed(C.byref(c), B, L, rows),
            lib.om_encoder_train_workspace_bytes_packed(C.byref(c), B, L, rows)]


def test_bytes_and_packed_supported_are_those_of_the_library_before_the_plan():
    for name, (cfg, B, L, tape, ws) in BYTES.items():
        assert _bytes(cfg, B, L) == [tape, ws], name
    for name, (cfg, B, L, want) in PACKED_BYTES.items():
        assert [_packed(cfg, B, L, r) for r in ROWS] == want, name
    for (opt, value), want in BYTES_SWITCHED.items():
        with switched(opt, value):
            got = [_bytes(*BYTES[k][:3]) for k in ("base_f16", "base_f32", "t5_relu_bf16")] + [
                _packed(*PACKED_BYTES[k][:3], 1536) for k in ("small_f16", "t5_relu_bf16")]
            assert got == want, (opt, value)
    lib = N.lib()
    assert lib.om_encoder_tape_bytes(None, 12, 128) == 0 and lib.om_encoder_train_workspace_bytes(C.byref(N.OmEncoderConfig(**_S)), 0, 128) == 0
    assert lib.om_encoder_train_packed_supported(None, 24, 128, 1536) == 0
