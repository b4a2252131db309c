"""Two lanes: a large padded fused-BERT batch runs as two half-batches on two streams over two views of one workspace.

  CPU   the rule (csrc/encoder_plan.h encoder_lanes) through om_debug_encoder_lanes, a table written out by hand; the plan word and the
        workspace size do not know about it
  CPU   the two views through om_debug_encoder_lane_ranges: inside the workspace, disjoint, as large as a carve of the lane's own shape
  CPU   the fused-epilogue contractions plan the whole's GEMM family at a lane's height
  GPU   the forward: representations with OM_OPT_ENCODER_LANES at 2 048 and at 0 are the same bits; the fork counter says which ran
  GPU   ordering against the caller's stream; the packed entry; what declines at fork time (timing mode, a capturing stream)"""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.helpers import NS, synth_tokens
from tests.test_encoder_plan import BASE, BF16, F16, F32, FUSED, OPT_FUSED_LN, SMALL, TWO, bert, modernbert, plan, switched, t5

DEV = "cuda:0"
OPT_SKIP_PAD, OPT_LANES = 22, 24                    # include/openmatch_hip.h: OM_OPT_ENCODER_SKIP_PAD, OM_OPT_ENCODER_LANES
LOW = 2048                                          # the switch as the GPU tests set it
FIELDS = ["x", "y", "x1", "qkv", "ctx", "ff", "ff2", "pooled", "headout", "kmax", "final32", "stats", "slots", "y_lo", "x1_lo"]


# ------------------------------------------------------------------------------------------------------------- CPU
def lanes(cfg, B, L, packed=0, gated=0, rel=None, hidden=0):
    """(om_debug_encoder_lanes, B0 or None)"""
    c = N.OmEncoderConfig(**cfg)
    if rel is None:
        rel = cfg["arch"] == N.ARCH_T5 or cfg.get("rel_buckets", 0) > 0
    b0 = C.c_int64(-1)
    rc = N.lib().om_debug_encoder_lanes(C.byref(c), int(gated), int(rel), B, L, packed, int(hidden), C.byref(b0))
    return rc, (b0.value if rc == 1 else None)


SMALL2 = dict(n_layers=2, vocab=600, max_pos=160)              # with SMALL's widths: the GPU tests' models

# (name, configuration, B, L, keyword arguments of lanes(), expected (answer, B0)) at the default switch, 65 536
DEFAULT_TABLE = [
    ("headline_f16", bert(F16), 1024, 128, {}, (1, 512)),
    ("headline_bf16", bert(BF16), 1024, 128, {}, (1, 512)),
    ("lane_rows_65024", bert(F16), 1024, 127, {}, (0, None)),            # B0 = 512 (whole tiles): 512 * 127 < 65 536
    ("b_2048_l_64", bert(F16), 2048, 64, {}, (1, 1024)),
    ("b_2044_l_128", bert(F16), 2044, 128, {}, (1, 1022)),                # two lanes of 130 816 padded rows
    ("b_2048_l_128", bert(F16), 2048, 128, {}, (0, None)),               # lanes of 131 072 rows: measured slower forked
    ("packed", bert(F16), 1024, 128, dict(packed=73728), (0, None)),
    ("want_hidden", bert(F16), 1024, 128, dict(hidden=1), (0, None)),
    ("rel_bias", bert(F16, rel_buckets=32, rel_max_dist=128), 1024, 128, {}, (0, None)),
    ("float32", bert(F32), 1024, 128, {}, (0, None)),
    ("t5", t5(BF16, pooling=N.POOL_FIRST), 1024, 128, {}, (0, None)),
    ("modernbert", modernbert(F16), 1024, 128, {}, (0, None)),
    ("small_batch", bert(F16), 512, 128, {}, (0, None)),                  # 32 768 rows per lane
]
# the same at the GPU tests' switch, 2 048
LOW_TABLE = [
    ("b_1024", bert(F16, SMALL, **SMALL2), 1024, 16, {}, (1, 512)),
    ("b_1027", bert(F16, SMALL, **SMALL2), 1027, 16, {}, (1, 512)),                # 513 rounded down to whole tiles (16 sequences each)
    ("b_1023", bert(F16, SMALL, **SMALL2), 1023, 16, {}, (0, None)),               # B0 = 496 < 512: the whole takes the [CLS] tail, lane 0 would not
    ("mean_256", bert(F16, SMALL, **SMALL2, pooling=N.POOL_MEAN), 256, 16, {}, (1, 128)),      # no tail involved: 2 048 rows per lane
    ("mean_255", bert(F16, SMALL, **SMALL2, pooling=N.POOL_MEAN), 255, 16, {}, (0, None)),     # B0 = 112: 1 792 rows
    ("bf16_1027", bert(BF16, SMALL, **SMALL2), 1027, 16, {}, (1, 512)),
]


def test_lanes_rule_without_a_gpu():
    lib = N.lib()
    assert lib.om_debug_option_value(OPT_LANES) == 65536                              # the default
    wrong = [(name, lanes(cfg, B, L, **kw), want) for name, cfg, B, L, kw, want in DEFAULT_TABLE if lanes(cfg, B, L, **kw) != want]
    assert not wrong, wrong
    with switched(OPT_LANES, LOW):
        wrong = [(name, lanes(cfg, B, L, **kw), want) for name, cfg, B, L, kw, want in LOW_TABLE if lanes(cfg, B, L, **kw) != want]
        assert not wrong, wrong
    for opt, value in ((OPT_LANES, 0), (OPT_FUSED_LN, 0)):
        with switched(opt, value):
            assert lanes(bert(F16), 1024, 128) == (0, None), (opt, value)
    assert lanes(bert(F16), 1024, 128) == (1, 512)                                    # every switch is back
    assert lib.om_debug_encoder_lanes(None, 0, 0, 1024, 128, 0, 0, None) == -1
    c = N.OmEncoderConfig(**bert(F16))
    assert lib.om_debug_encoder_lanes(C.byref(c), 0, 0, 1024, 128, 0, 0, None) == 1   # B0 may be NULL
    # neither the plan word nor the workspace size knows about it
    with switched(OPT_LANES, 0):
        off = plan(bert(F16), 1024, 128), lib.om_encoder_workspace_bytes(C.byref(c), 1024, 128)
    on = plan(bert(F16), 1024, 128), lib.om_encoder_workspace_bytes(C.byref(c), 1024, 128)
    assert off == on and on[0] == FUSED | TWO and on[1] > 0


def _ranges(cfg, B, L, lane):
    c = N.OmEncoderConfig(**cfg)
    out = (C.c_int64 * 30)()
    n = N.lib().om_debug_encoder_lane_ranges(C.byref(c), 0, 0, B, L, lane, out, 30)
    assert n == len(FIELDS), N.lib().om_last_error()
    return {f: (out[2 * i], out[2 * i + 1]) for i, f in enumerate(FIELDS)}


def _own_carve(cfg, Bh, L):
    """bytes of each field in a workspace carved for the call (Bh, L) alone (csrc/encoder.hip carve: 16-bit BERT, fused path)"""
    H, F, layers = cfg["hidden"], cfg["ffn"], cfg["n_layers"]
    M = Bh * L
    Mp = (M + 255) // 256 * 256
    return dict(x=Mp * H * 2, y=Mp * H * 2, x1=Mp * H * 2, qkv=Mp * 3 * H * 2, ctx=Mp * H * 2, ff=Mp * F * 2, ff2=0, pooled=Bh * H * 4,
                headout=Bh * 4, kmax=Bh * 4, final32=(Bh if cfg["pooling"] == N.POOL_FIRST else M) * H * 4, stats=2 * layers * Mp * 8,
                slots=2 * ((H + 255) // 256) * Mp * 8, y_lo=Mp * H * 2, x1_lo=Mp * H * 2)


@pytest.mark.parametrize("name,cfg,B,L,switch", [("headline", bert(F16), 1024, 128, 65536), ("b_1027", bert(F16, SMALL, **SMALL2), 1027, 16, LOW),
                                                 ("mean_1027", bert(BF16, SMALL, **SMALL2, pooling=N.POOL_MEAN), 1027, 16, LOW)],
                         ids=["headline", "b-1027", "mean-1027"])
def test_lane_views_are_disjoint_and_inside_the_workspace(name, cfg, B, L, switch):
    c = N.OmEncoderConfig(**cfg)
    with switched(OPT_LANES, switch):
        rc, B0 = lanes(cfg, B, L)
        assert rc == 1
        total = N.lib().om_encoder_workspace_bytes(C.byref(c), B, L)
        views = [_ranges(cfg, B, L, h) for h in (0, 1)]
        assert N.lib().om_debug_encoder_lane_ranges(C.byref(c), 0, 0, B, L, 2, (C.c_int64 * 30)(), 30) == -1
    with switched(OPT_LANES, 0):                                     # a call that does not fork has no views
        assert N.lib().om_debug_encoder_lane_ranges(C.byref(c), 0, 0, B, L, 0, (C.c_int64 * 30)(), 30) == -1
    for h, Bh in ((0, B0), (1, B - B0)):
        own = _own_carve(cfg, Bh, L)
        for f, (off, nbytes) in views[h].items():
            assert nbytes == own[f], (h, f, nbytes, own[f])
            assert 0 <= off and off + nbytes <= total, (h, f, off, nbytes, total)
            assert off % 4 == 0 and (f in ("kmax", "pooled", "headout", "final32") or off % 256 == 0), (h, f, off)
    live = [[(off, off + nb, f) for f, (off, nb) in v.items() if nb] for v in views]
    for a0, a1, fa in live[0]:
        for b0, b1, fb in live[1]:
            assert a1 <= b0 or b1 <= a0, (fa, fb)
    for v in live:                                                   # and inside one lane no field overlaps another
        spans = sorted(v)
        assert all(p[1] <= q[0] for p, q in zip(spans, spans[1:])), spans


@pytest.mark.parametrize("two", [False, True], ids=["one-plane", "two-planes"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_lane_heights_plan_the_whole_family(dt, two):
    """om_debug_gemm_plan_ex (no GPU), bert-base widths, default switches: the folded QKV, out-proj, FFN1 and FFN2 plan the same
    generation-7 family at M = 65 536 as at M = 131 072, and so does the first layer's plain QKV"""
    from tests.test_gemm_epilogues import EPS, fake_ep
    from tests.test_gemm_epilogues import plan as gemm_plan
    from tests.test_gemm_kernels import FAM
    H, Fw = BASE["hidden"], BASE["ffn"]
    out_side = dict(bias=1, resid=1, ldr=H, rln_stats=1, rln_g=1, rln_b=1, stats_out=1, ln_inv_h=1.0 / H, ln_eps=EPS)
    if two:
        out_side.update(out_lo=1, resid_lo=1)
    folded = dict(bias=1, ln_stats=1, ln_colsum=1, ln_inv_h=1.0 / H, ln_eps=EPS)
    g7 = {FAM[k] for k in ("g7", "g7_one_tile", "7c16", "7r16")}
    for name, spec, Nn, K in (("qkv0", dict(bias=1), 3 * H, H), ("qkv", folded, 3 * H, H), ("out-proj", out_side, H, H),
                              ("ffn1", dict(folded, act=N.ACT_GELU_ERF), Fw, H), ("ffn2", out_side, H, Fw)):
        full = gemm_plan(dt, dt, 131072, Nn, K, fake_ep(spec))
        assert full in g7, (name, full)
        assert gemm_plan(dt, dt, 65536, Nn, K, fake_ep(spec)) == full, name


# ------------------------------------------------------------------------------------------------------------- GPU
FL = 16
SIZES = (1024, 1027)


def _masks(B):
    """name -> (ids, mask) on the host, L = 16: a full row, a one-token row, a fully masked row and holes in EACH lane"""
    rng = np.random.default_rng(5)
    ids, ragged = synth_tokens(rng, B, FL, vocab=600, lo_len=5, lo_id=300)
    for at in (0, 512):                                # lane 0 starts at sequence 0, lane 1 at 512 (B0 of both sizes)
        ragged[at, :] = 1                              # a full-length row
        ragged[at + 1, :] = 0; ragged[at + 1, 0] = 1   # a row of one token
        ragged[at + 2, :] = 0                          # a fully masked row
        ragged[at + 3, :] = 0; ragged[at + 3, ::3] = 1 # holes: the extent is the last unmasked token's
    ragged[511, :] = 0; ragged[511, :2] = 1            # the last sequence of lane 0 ...
    ragged[B - 1, :] = 0; ragged[B - 1, :3] = 1        # ... and of lane 1: the [CLS] rows the compact pad rows replicate
    ids = rng.integers(1, 600, (B, FL))
    return {"ragged": (ids, ragged), "ones": (ids, np.ones_like(ragged))}


@pytest.fixture(scope="module")
def env():
    from tests.test_pad_skip import _models
    masks = {B: {k: tuple(torch.from_numpy(a).to(DEV) for a in v) for k, v in _masks(B).items()} for B in SIZES}
    return _models(), masks, {}


def _model(env, name, pooling, dtype):
    from openmatch.modeling import DRModelForInference
    models, _, built = env
    key = (name, pooling, dtype)
    if key not in built:
        built[key] = DRModelForInference(lm_q=models[name], lm_p=models[name], pooling=pooling,
                                         model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()
    return built[key]


def _encode(model, ids, mask, pooling, packed_rows=None):
    from openmatch_amd.encoder import compute_dtype_code, hip_encode
    code = compute_dtype_code(model.model_args)
    return hip_encode(model.lm_p, {"input_ids": ids, "attention_mask": mask}, pooling, None, False, code, want_hidden=False,
                      packed_rows=packed_rows)[1]


def _forks():
    return N.lib().om_debug_encoder_lane_forks()


def _cfg(name, dtype, pooling):
    heads, hd = (8, 32) if name == "bert-8x32" else (4, 64)
    return N.OmEncoderConfig(arch=N.ARCH_BERT, dtype=F16 if dtype == "float16" else BF16, hidden=256, n_layers=2, n_heads=heads, head_dim=hd,
                             ffn=1024, vocab=600, max_pos=160, type_vocab=2, act=N.ACT_GELU_ERF, ln_eps=1e-12,
                             pooling=N.POOL_FIRST if pooling == "first" else N.POOL_MEAN)


@pytest.mark.gpu
@pytest.mark.parametrize("pooling", ["first", "mean"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", ["bert-4x64", "bert-8x32"])
def test_forward_keeps_its_bits(env, name, dtype, pooling):
    """the representations with the switch at 2 048 and at 0: torch.equal, at B = 1 024 and 1 027 (lane 1's height rounded up), for ragged
    lengths and all ones, with pad-skip at 1 and at 0; the counter rises by exactly 1 per forked forward and by 0 with the switch at 0"""
    _, masks, _ = env
    model = _model(env, name, pooling, dtype)
    lib = N.lib()
    for B in SIZES:
        with switched(OPT_LANES, LOW):
            assert lib.om_debug_encoder_lanes(C.byref(_cfg(name, dtype, pooling)), 0, 0, B, FL, 0, 0, None) == 1      # the case runs what it names
        for mname, (ids, mask) in masks[B].items():
            for skip_pad in (1, 0):
                label = (name, dtype, pooling, B, mname, skip_pad)
                with switched(OPT_SKIP_PAD, skip_pad):
                    n0 = _forks()
                    with switched(OPT_LANES, 0):
                        want = _encode(model, ids, mask, pooling)
                    n1 = _forks()
                    with switched(OPT_LANES, LOW):
                        got = _encode(model, ids, mask, pooling)
                    n2 = _forks()
                torch.cuda.synchronize()
                assert (n1 - n0, n2 - n1) == (0, 1), label
                assert torch.isfinite(want).all(), label
                assert torch.equal(got, want), (label, (got - want).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["side-stream", "default-stream"])
def test_results_are_ordered_on_the_callers_stream(env, where):
    """two different batches back to back through the same workspace, each result consumed by a torch op on the caller's stream with
    nothing between: every consumer sees its switch-0 result (a missing join shows lane 1's rows unfinished, a missing fork lane 1
    reading inputs that are not there yet)"""
    _, masks, _ = env
    model = _model(env, "bert-4x64", "first", "float16")
    (ids_a, mask_a), (ids_b, mask_b) = masks[1024]["ragged"], masks[1024]["ones"]
    ids_b = ids_b.flip(0).contiguous()
    with switched(OPT_LANES, 0):
        want = [_encode(model, ids_a, mask_a, "first").clone(), _encode(model, ids_b, mask_b, "first").clone()]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV) if where == "side-stream" else torch.cuda.default_stream(DEV)
    n0 = _forks()
    with switched(OPT_LANES, LOW), torch.cuda.stream(stream):
        for rnd in range(2):
            got = []
            for ids, mask in ((ids_a, mask_a), (ids_b, mask_b)):
                ids_now, mask_now = ids + 0, mask * 1            # the inputs are produced on the caller's stream just before
                got.append(_encode(model, ids_now, mask_now, "first") * 1.0)
            stream.synchronize()
            for g, w in zip(got, want):
                assert torch.equal(g, w), (where, rnd)
    torch.cuda.synchronize()
    assert _forks() - n0 == 4


@pytest.mark.gpu
@pytest.mark.parametrize("B", SIZES)
def test_packed_entry_does_not_fork(env, B):
    from openmatch_amd import encoder as enc_mod
    from openmatch_amd.encoder import packed_rows_bound
    _, masks, _ = env
    model = _model(env, "bert-4x64", "first", "float16")
    ids, mask = masks[B]["ragged"]
    rows = packed_rows_bound(mask.cpu())
    with switched(OPT_LANES, 0):
        want = _encode(model, ids, mask, "first", packed_rows=rows)
    assert enc_mod.LAST_CALL["packed"]
    n0 = _forks()
    with switched(OPT_LANES, LOW):
        got = _encode(model, ids, mask, "first", packed_rows=rows)
    torch.cuda.synchronize()
    assert enc_mod.LAST_CALL["packed"] and _forks() == n0
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_timing_mode_declines(env):
    """under om_kernel_timing_enable(1) the forward stays one chain: the counter does not move, launches and flops are the switch-0 run's"""
    _, masks, _ = env
    model = _model(env, "bert-4x64", "first", "float16")
    ids, mask = masks[1024]["ragged"]
    lib = N.lib()
    ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
    with switched(OPT_LANES, 0):
        _encode(model, ids, mask, "first")               # weights packed and folded, buffers allocated
    got = {}
    n0 = _forks()
    for sw in (0, LOW):
        with switched(OPT_LANES, sw):
            torch.cuda.synchronize()
            assert lib.om_kernel_timing_enable(1) == 0
            try:
                assert lib.om_kernel_timing_read(0, C.byref(ms), C.byref(n), C.byref(fl)) == 0      # class 0: 16-bit GEMMs; empties it
                _encode(model, ids, mask, "first")
                torch.cuda.synchronize()
                assert lib.om_kernel_timing_read(0, C.byref(ms), C.byref(n), C.byref(fl)) == 0
            finally:
                lib.om_kernel_timing_enable(0)
            got[sw] = (n.value, fl.value)
    assert _forks() == n0
    assert got[LOW] == got[0] and got[0][0] == 8, got


@pytest.mark.gpu
def test_a_capturing_stream_declines(env):
    """one forward captured with torch.cuda.graph after an eager warm call on the same stream: the counter does not move, and the
    replay equals the eager result"""
    _, masks, _ = env
    model = _model(env, "bert-4x64", "first", "float16")
    ids, mask = masks[1024]["ragged"]
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        with switched(OPT_LANES, 0):
            want = _encode(model, ids, mask, "first").clone()      # the warm call: workspace and pad-skip buffer of this stream exist
        n0 = _forks()
        with switched(OPT_LANES, LOW):
            eager = _encode(model, ids, mask, "first").clone()
    stream.synchronize()
    assert _forks() - n0 == 1 and torch.equal(eager, want)
    graph = torch.cuda.CUDAGraph()
    n0 = _forks()
    with switched(OPT_LANES, LOW):
        with torch.cuda.graph(graph, stream=stream):
            out = _encode(model, ids, mask, "first")
    assert _forks() == n0
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
