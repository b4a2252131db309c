"""Pad rows skipped on the device ("pad rows"): a padded 16-bit om_encoder_forward that returns representations only packs
its rows on the device and its generation-7 contractions read the token count from device memory (GemmEpilogue::rows_dev).

  CPU   the rule (csrc/encoder_plan.h encoder_skip_pad) through om_debug_encoder_skip_pad, a table written out by hand
  GPU   one kernel at a time through om_debug_gemm_ex: rows below roundup256(clamp(count, 0, M)) carry the bits of the call without a
        count, rows from there on keep the sentinel they held; the count is a hint other families ignore; timing mode prices the rows run
  GPU   the forward: the representations with OM_OPT_ENCODER_SKIP_PAD at 1 and at 0 are the same bits, on one stream and on two"""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.helpers import NS, synth_tokens
from tests.test_encoder_plan import BASE, BF16, D32, F16, F32, OPT_FUSED_LN, OPT_GEMM_VARIANT, SMALL, bert, modernbert, switched, t5

DEV = "cuda:0"
OPT_SKIP_PAD = 22                                   # include/openmatch_hip.h: OM_OPT_ENCODER_SKIP_PAD


# ------------------------------------------------------------------------------------------------------------- CPU
def skip(cfg, B, L, gated=0, rel=None, hidden=0):
    c = N.OmEncoderConfig(**cfg)
    if rel is None:
        rel = cfg["arch"] == N.ARCH_T5 or cfg.get("rel_buckets", 0) > 0
    return N.lib().om_debug_encoder_skip_pad(C.byref(c), int(gated), int(rel), B, L, int(hidden))


# (name, configuration, B, L, keyword arguments of skip(), expected) at the default switches
SKIP_TABLE = [
    ("base_f16", bert(F16), 1024, 128, {}, 1),                                    # the headline batch
    ("base_bf16", bert(BF16), 1024, 128, {}, 1),
    ("base_f16_mean", bert(F16, pooling=N.POOL_MEAN), 1024, 128, {}, 1),
    ("small_24x128", bert(F16, SMALL, n_layers=2), 24, 128, {}, 1),
    ("rows_1025", bert(F16), 25, 41, {}, 1),                                      # 1 025 rows: the bound is 1 280
    ("t5_fused", t5(BF16), 16, 128, {}, 1),
    ("t5_fused_f16_relu", t5(F16), 16, 128, {}, 1),
    ("want_hidden", bert(F16), 1024, 128, dict(hidden=1), 0),
    ("no_pooling", bert(F16, pooling=N.POOL_NONE), 1024, 128, {}, 0),
    ("float32", bert(F32), 1024, 128, {}, 0),
    ("modernbert", modernbert(F16), 1024, 128, {}, 0),
    ("few_rows_8x128", bert(F16), 8, 128, {}, 0),                                 # 1 024 rows: the few-rows kernels
    ("few_rows_bf16_8x128", bert(BF16), 8, 128, {}, 0),                           # fused (two planes), but the packed entry sends few rows back
    ("hidden_128", bert(F16, D32), 1024, 128, {}, 0),                             # widths off 256: nothing fuses
    ("t5_gated", t5(BF16, act=N.ACT_GELU_TANH), 16, 128, dict(gated=1), 0),
    ("t5_f16_tanh", t5(F16, act=N.ACT_GELU_TANH), 16, 128, {}, 0),                # the packed entry's float16 T5 is ReLU only
    ("t5_f32", t5(F32), 16, 128, {}, 0),
    ("relu_bert", bert(BF16, act=N.ACT_RELU), 1024, 128, {}, 0),
    ("refused_heads", bert(F16, head_dim=48), 1024, 128, {}, 0),                  # a call the forward refuses
    ("refused_length", bert(F16), 2, 513, {}, 0),
    ("empty_batch", bert(F16), 0, 128, {}, 0),
]


def test_skip_rule_without_a_gpu():
    lib = N.lib()
    wrong = [(name, skip(cfg, B, L, **kw), want) for name, cfg, B, L, kw, want in SKIP_TABLE if skip(cfg, B, L, **kw) != want]
    assert not wrong, wrong
    assert lib.om_debug_option_value(OPT_SKIP_PAD) == 1                           # the default
    for opt, value in ((OPT_SKIP_PAD, 0), (OPT_FUSED_LN, 0), (OPT_GEMM_VARIANT, 2)):
        with switched(opt, value):
            for dt in (F16, BF16):
                assert skip(bert(dt), 1024, 128) == 0, (opt, value, dt)
            assert skip(t5(BF16), 16, 128) == 0, (opt, value)
    assert skip(bert(F16), 1024, 128) == 1 and skip(bert(BF16), 1024, 128) == 1    # every switch is back
    assert lib.om_debug_encoder_skip_pad(None, 0, 0, 1024, 128, 0) == -1
    # the plan word does not know about it
    from tests.test_encoder_plan import FUSED, TWO, plan
    with switched(OPT_SKIP_PAD, 0):
        off = plan(bert(F16), 1024, 128)
    assert off == plan(bert(F16), 1024, 128) == FUSED | TWO


def test_debug_epilogue_mirrors_the_field():
    names = [f for f, _ in N.OmDebugGemmEpilogue._fields_]
    assert names[-1] == "rows_dev" and names[-2] == "reverse"
    assert C.sizeof(N.OmDebugGemmEpilogue) == 232 and N.OmDebugGemmEpilogue.rows_dev.offset == 224      # include/openmatch_hip.h


# ------------------------------------------------------------------------------------------------------------- GPU, one kernel
GM, GN, GK = 1024, 512, 256
COUNTS = [0, 1, 256, 257, 1000, 1024, 5000, -3]
G_WALKS = [(None, 0), (None, 1), (8, 0), (8, 1)]                                   # (OM_OPT_GEMM_MAX_GRID, reverse)


def rows_of(count):
    return (min(max(count, 0), GM) + 255) // 256 * 256


def _epilogue_cases():
    """(id, dtype, OM_OPT_GEMM_CONT, family, epilogue name) -- every generation-7 epilogue tests/test_gemm_epilogues.py reaches"""
    from tests.test_gemm_epilogues import CONT, RESTART
    cases = []
    for dt, name in ((BF16, "bf16"), (F16, "f16")):
        ring_two = CONT | 512 if dt == BF16 else CONT               # bit 9: bfloat16's two-plane variant on the ring
        rest_two = CONT if dt == BF16 else CONT & ~256              # bit 8 cleared: float16's on the restart-per-tile kernel
        cases += [(f"{name}-7c16-plain", dt, 511 if dt == BF16 else CONT & ~128, "7c16", "plain"),      # tests/test_gemm_kernels.py FAMILIES
                  (f"{name}-7c16-ln-gelu", dt, CONT, "7c16", "ln_gelu"),
                  (f"{name}-7r16-one-plane", dt, CONT, "7r16", "lnf2"),
                  (f"{name}-7r16-two-planes", dt, ring_two, "7r16", "lnf3"),
                  (f"{name}-restart-ln-gelu", dt, RESTART, "g7", "ln_gelu"),
                  (f"{name}-restart-one-plane", dt, RESTART, "g7", "lnf2"),
                  (f"{name}-restart-two-planes", dt, rest_two, "g7", "lnf3")]
    cases.append(("f16-7r16-16+8", F16, CONT, "7r16", "lnf4"))
    return [pytest.param(*c[1:], id=c[0]) for c in cases]


def test_kernel_cases_plan_the_family_they_name():
    """om_debug_gemm_plan_ex (no GPU): every case of test_g7_row_count reaches its family, with a row count or without"""
    from tests.test_gemm_epilogues import EPS, fake_ep, plan
    from tests.test_gemm_kernels import FAM, gemm_options
    specs = {"plain": dict(bias=1), "ln_gelu": dict(act=N.ACT_GELU_ERF, bias=1, ln_stats=1, ln_colsum=1, ln_inv_h=1.0 / GK, ln_eps=EPS)}
    out_side = dict(bias=1, resid=1, ldr=GN, rln_stats=1, rln_g=1, rln_b=1, stats_out=1, ln_inv_h=1.0 / GN, ln_eps=EPS)
    specs.update(lnf2=out_side, lnf3=dict(out_side, out_lo=1, resid_lo=1), lnf4=dict(out_side, out_lo=1, lo8=1))
    for case in _epilogue_cases():
        dt, cont, family, epi = case.values
        with gemm_options(cont=cont, skinny_m=0):
            for count in (0, 7 << 32):
                ep = fake_ep(specs[epi])
                ep.rows_dev = count
                assert plan(dt, dt, GM, GN, GK, ep) == FAM[family], (case.id, count)


class G7Call:
    """one epilogue at M = 1024, N = 512, K = 256: fresh sentinel-filled outputs per launch, the count in device memory"""

    def __init__(self, dt, epi):
        from tests.test_gemm_epilogues import EPS, ln_inputs, row_stats
        self.dt, self.epi = dt, epi
        d = ln_inputs(dt, GM, GN, GK, 31, DEV)
        self.d = d
        self.a_stats = row_stats(d["A"]).to(DEV)
        self.r_stats = (d["r_stats"] if epi == "lnf3" else d["r1_stats"]).to(DEV)
        self.eps = EPS
        self.count = torch.zeros(1, dtype=torch.int32, device=DEV)

    def launch(self, count, rev):
        """count None: no rows_dev.  Returns (rc, family, {name: (rows-major 2-D view of the output, rows per M row)})"""
        from tests.test_gemm_epilogues import ERF, NONE, gemm_ex, make_ep, out_buf
        from tests.test_gemm_kernels import F32 as GF32
        d, dt = self.d, self.dt
        C_ = out_buf(dt, GM, GN, GN + 64)
        outs = {"C": C_}
        if self.epi == "plain":
            kw = dict(act=NONE, bias=d["bias"])
        elif self.epi == "ln_gelu":
            kw = dict(act=ERF, bias=d["bias"], ln_stats=self.a_stats, ln_colsum=d["colsum"], ln_inv_h=1.0 / GK, ln_eps=self.eps)
        else:
            nslots = GN // 128
            S = out_buf(GF32, nslots * GM, 2)
            outs["S"] = S
            kw = dict(act=NONE, bias=d["bias"], resid=d["R"], ldr=GN, rln_stats=self.r_stats, rln_g=d["g"], rln_b=d["b"], stats_out=S,
                      ln_inv_h=1.0 / GN, ln_eps=self.eps)
            if self.epi == "lnf3":
                LO = out_buf(dt, GM, GN, GN + 64)
                outs["LO"] = LO
                kw.update(out_lo=LO, resid_lo=d["R_lo"])
            if self.epi == "lnf4":
                LO = out_buf(F16, 1, GM * GN // 2)                   # M N bytes, tile by tile in row-tile order (omk_lo8_offset)
                outs["LO8"] = LO
                kw.update(out_lo=LO, lo8=1)
        ep = make_ep(reverse=rev, **kw)
        if count is not None:
            self.count.fill_(count)
            ep.rows_dev = self.count.data_ptr()
        snaps = {k: b.snapshot() for k, b in outs.items()}
        rc, fam = gemm_ex(dt, dt, d["A"], d["B"], C_, GM, GN, GK, ep)
        for k, b in outs.items():
            assert b.outside_changed(snaps[k]) == 0, f"{self.epi}: written outside the window of {k}"
        views = {}
        for k, b in outs.items():
            w = b.window.clone()
            if k == "S":                      # [slots][M] pairs -> [M, slots * 2]
                w = w.view(GN // 128, GM, 2).permute(1, 0, 2).reshape(GM, -1).contiguous()
            if k == "LO8":                    # one row tile = 256 * N bytes
                w = w.view(torch.uint8).view(GM // 256, -1).repeat_interleave(256, 0).contiguous()
            views[k] = w
        return rc, fam, views


def _bits(t):
    """[rows, bytes]"""
    return t.contiguous().view(torch.uint8)


FILL = 0x5A      # every byte of a fresh Buf, in all three formats (tests/test_gemm_kernels.py SENTINEL: 0x5A5A, 0x5A5A5A5A)


@pytest.mark.gpu
@pytest.mark.parametrize("dt,cont,family,epi", _epilogue_cases())
def test_g7_row_count(dt, cont, family, epi):
    """rows below roundup256(clamp(count)) of C, out_lo and stats_out: the bits of the call without rows_dev; rows from there on keep
    the sentinel -- eight counts, both walk directions, the default grid and one of 8 workgroups"""
    from tests.test_gemm_kernels import FAM, gemm_options
    call = G7Call(dt, epi)
    with gemm_options(cont=cont, skinny_m=0):
        rc, fam, full = call.launch(None, 0)
        assert rc == 0 and fam == FAM[family], (rc, fam, N.lib().om_last_error())
        for k in full:
            assert not bool((_bits(full[k]) == FILL).all(1).any()), f"{k}: the full call left a row of the fill pattern"
        for cap, rev in G_WALKS:
            with gemm_options(**({} if cap is None else dict(max_grid=cap))):
                for count in COUNTS:
                    rc, fam, got = call.launch(count, rev)
                    assert rc == 0 and fam == FAM[family], (count, cap, rev, rc, fam, N.lib().om_last_error())
                    R = rows_of(count)
                    for k in full:
                        label = f"{epi} {k} count={count} max_grid={cap} reverse={rev}"
                        assert torch.equal(_bits(got[k][:R]), _bits(full[k][:R])), f"{label}: rows below {R} differ from the full call"
                        assert bool((_bits(got[k][R:]) == FILL).all()), f"{label}: rows from {R} on were written"


@pytest.mark.gpu
def test_count_is_a_hint_other_families_ignore():
    """a float32 call and a 16-bit call of M < 512 (no generation-7 shape) return what they return without the count"""
    from tests.test_gemm_epilogues import gemm_ex, make_ep, out_buf
    from tests.test_gemm_kernels import FAM
    gen = torch.Generator(device=DEV).manual_seed(5)
    count = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    for dt, td, M in ((F32, torch.float32, 1024), (BF16, torch.bfloat16, 256), (F16, torch.float16, 384)):
        A = torch.randn(M, GK, generator=gen, device=DEV).to(td)
        B = (torch.randn(GN, GK, generator=gen, device=DEV) / 16).to(td)
        bias = torch.randn(GN, generator=gen, device=DEV)
        got = []
        for with_count in (False, True):
            C_ = out_buf(dt, M, GN)
            ep = make_ep(bias=bias)
            if with_count:
                ep.rows_dev = count.data_ptr()
            rc, fam = gemm_ex(dt, dt, A, B, C_, M, GN, GK, ep)
            assert rc == 0 and fam not in (FAM["g7"], FAM["g7_one_tile"], FAM["7c16"], FAM["7r16"]), (rc, fam)
            got.append((fam, C_.window.clone()))
        assert got[0][0] == got[1][0]
        assert torch.equal(_bits(got[0][1]), _bits(got[1][1])), (dt, M)
        assert torch.isfinite(got[1][1].float()).all()               # every row computed


@pytest.mark.gpu
def test_timing_mode_prices_the_rows_run():
    """om_kernel_timing_enable(1): the flops read back are 2 rows256 N K of the calls made"""
    from tests.test_gemm_epilogues import CONT
    from tests.test_gemm_kernels import gemm_options
    lib = N.lib()
    call = G7Call(F16, "lnf2")
    plain = G7Call(F16, "ln_gelu")
    ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
    with gemm_options(cont=CONT, skinny_m=0):
        assert lib.om_kernel_timing_enable(1) == 0
        try:
            assert lib.om_kernel_timing_read(0, C.byref(ms), C.byref(n), C.byref(fl)) == 0      # class 0: 16-bit GEMMs; empties it
            want = 0.0
            for c_, count in ((call, 257), (plain, 1000), (call, 0), (plain, None), (call, 5000), (plain, -3)):
                rc, _, _ = c_.launch(count, 0)
                assert rc == 0
                want += 2.0 * (GM if count is None else rows_of(count)) * GN * GK
            assert lib.om_kernel_timing_read(0, C.byref(ms), C.byref(n), C.byref(fl)) == 0
        finally:
            lib.om_kernel_timing_enable(0)
    assert n.value == 6 and fl.value == want, (n.value, fl.value, want)


# ------------------------------------------------------------------------------------------------------------- GPU, the forward
FB, FL = 24, 128


def _models():
    """name -> (HF module, float16 allowed): a 2-layer BERT of hidden 256 / ffn 1024 with 4 x 64 heads, the same with 8 x 32, a fused T5"""
    from transformers import BertConfig, BertModel, T5Config, T5EncoderModel
    from tests.test_head_dim32 import _perturb
    torch.manual_seed(11)
    kw = dict(num_hidden_layers=2, vocab_size=600, max_position_embeddings=160, hidden_size=256, intermediate_size=1024)
    t5cfg = T5Config(d_model=256, d_ff=1024, num_layers=2, num_heads=4, d_kv=64, vocab_size=600, feed_forward_proj="relu")
    return {"bert-4x64": _perturb(BertModel(BertConfig(num_attention_heads=4, **kw)).eval()),
            "bert-8x32": _perturb(BertModel(BertConfig(num_attention_heads=8, **kw)).eval()),
            "t5": T5EncoderModel(t5cfg).eval()}


def _masks():
    """name -> (ids, mask) on the host, B = 24, L = 128"""
    rng = np.random.default_rng(3)
    ids, ragged = synth_tokens(rng, FB, FL, vocab=600, lo_len=5, lo_id=300)
    ragged[0, :] = 1                                   # a full-length row
    ragged[1, :] = 0; ragged[1, 0] = 1                 # a row of one token
    ragged[2, :] = 0                                   # a fully masked row
    ragged[3, :] = 0; ragged[3, ::3] = 1               # holes: the extent is the last unmasked token's
    ids = rng.integers(1, 600, (FB, FL))
    few = np.zeros_like(ragged); few[:, :7] = 1        # 168 tokens: one row tile
    few[5, :3] = 1; few[5, 3:] = 0
    return {"ragged": (ids, ragged), "ones": (ids, np.ones_like(ragged)), "under-256": (ids, few)}


@pytest.fixture(scope="module")
def forward_env():
    return _models(), _masks()


def _tokens(mask):
    """what omk_mask_extent counts: per sequence 1 + its last unmasked token, L for a fully masked one"""
    L = mask.shape[1]
    last = np.where(mask.any(1), L - np.argmax(mask[:, ::-1] != 0, 1), L)
    return int(last.sum())


def _encode(lm, ids, mask, pooling, dtype):
    from openmatch.modeling import DRModelForInference
    from openmatch_amd import encoder as enc_mod
    from openmatch_amd.encoder import compute_dtype_code, hip_encode
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling=pooling, model_args=NS(encoder_only=hasattr(lm, "encoder") and not hasattr(lm, "embeddings"), dtype=dtype)).to(DEV).eval()
    code = compute_dtype_code(model.model_args)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    reps = hip_encode(model.lm_p, items, pooling, None, False, code, want_hidden=False)[1]
    assert enc_mod.LAST_CALL == {"rows": ids.shape[0] * ids.shape[1], "packed": False}
    return reps


@pytest.mark.gpu
@pytest.mark.parametrize("pooling", ["first", "mean"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", ["bert-4x64", "bert-8x32", "t5"])
def test_forward_keeps_its_bits(forward_env, name, dtype, pooling):
    """the representations with the switch at 1 and at 0: torch.equal, for ragged lengths (a one-token row, a fully masked row, a
    full-length row, holes), all ones, and a batch of fewer than 256 tokens; the Python side sees a padded call either way"""
    models, masks = forward_env
    lm = models[name]
    arch = N.ARCH_T5 if name == "t5" else N.ARCH_BERT
    heads, hd = (8, 32) if name == "bert-8x32" else (4, 64)
    cfg = N.OmEncoderConfig(arch=arch, dtype=F16 if dtype == "float16" else BF16, hidden=256, n_layers=2, n_heads=heads, head_dim=hd,
                            ffn=1024, vocab=600, max_pos=160, type_vocab=0 if name == "t5" else 2,
                            act=N.ACT_RELU if name == "t5" else N.ACT_GELU_ERF, ln_eps=1e-12, pooling=N.POOL_FIRST,
                            rel_buckets=32 if name == "t5" else 0, rel_max_dist=128 if name == "t5" else 0)
    assert N.lib().om_debug_encoder_skip_pad(C.byref(cfg), 0, int(name == "t5"), FB, FL, 0) == 1      # the case runs what it names
    for mname, (ids, mask) in masks.items():
        got = _encode(lm, ids, mask, pooling, dtype)
        with switched(OPT_SKIP_PAD, 0):
            want = _encode(lm, ids, mask, pooling, dtype)
        torch.cuda.synchronize()
        assert torch.isfinite(want).all(), (name, mname)
        assert torch.equal(got, want), (name, dtype, pooling, mname, (got - want).abs().max().item())


@pytest.mark.gpu
def test_two_streams(forward_env, monkeypatch):
    """two different batches on two streams with nothing between them: each equals its sequential result (one side buffer per stream)"""
    models, masks = forward_env
    lm = models["bert-4x64"]
    orig_get = N.Workspace.get.__func__

    def get(cls, dev, nbytes, tag="default"):      # hip_encode's workspace is one per device: here one per stream
        return orig_get(cls, dev, nbytes, tag + ":" + str(torch.cuda.current_stream(dev).cuda_stream))
    monkeypatch.setattr(N.Workspace, "get", classmethod(get))
    batches = [masks["ragged"], masks["under-256"]]
    want = [_encode(lm, ids, mask, "first", "float16").clone() for ids, mask in batches]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV) for _ in batches]
    for rnd in range(2):                              # the second round reuses both side buffers
        got = []
        for s, (ids, mask) in zip(streams, batches):
            with torch.cuda.stream(s):
                got.append(_encode(lm, ids, mask, "first", "float16"))
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert torch.equal(g, w), rnd


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bert-4x64", "t5"])
def test_forward_contractions_stop_at_the_token_count(forward_env, name):
    """the forward's contractions did receive the count: under om_kernel_timing_enable(1) the 16-bit GEMM flops of one forward are those
    of roundup256(tokens) rows -- four contractions per layer, 2 R (4 H^2 + 2 F H), but for a contraction planned onto another family
    than generation 7 -- and of all B L rows with the switch at 0"""
    models, masks = forward_env
    lib = N.lib()
    H, F, layers = 256, 1024, 2
    per_row = layers * 2.0 * (4 * H * H + 2 * F * H)
    ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
    # The count is a hint to generation 7 alone.  Seven of the eight contractions carry a fused-norm epilogue, which only generation 7
    # implements; the first layer's QKV is a plain contraction (bias, or nothing for T5) that the planner may send to another family
    # at this small shape, and that family computes all B L rows.  om_debug_gemm_plan says which, without a launch.
    fam = lib.om_debug_gemm_plan(F16, 1 << 32, H, 2 << 32, H, F16, 3 << 32, 3 * H, FB * FL, 3 * H, H, None if name == "t5" else 4 << 32,
                                 None, 0, N.ACT_NONE)
    assert fam > 0
    qkv0_all_rows = 0 if fam in (N.GEMM_FAMILY["g7"], N.GEMM_FAMILY["7c16"], N.GEMM_FAMILY["7r16"], N.GEMM_FAMILY["g7_one_tile"]) else 1
    for mname, (ids, mask) in masks.items():
        R = (_tokens(mask) + 255) // 256 * 256
        _encode(models[name], ids, mask, "first", "float16")          # weights packed and folded, buffers allocated
        got = {}
        for sw in (1, 0):
            with switched(OPT_SKIP_PAD, sw):
                torch.cuda.synchronize()
                assert lib.om_kernel_timing_enable(1) == 0
                try:
                    assert lib.om_kernel_timing_read(0, C.byref(ms), C.byref(n), C.byref(fl)) == 0      # empties the class
                    _encode(models[name], ids, mask, "first", "float16")
                    torch.cuda.synchronize()
                    assert lib.om_kernel_timing_read(0, C.byref(ms), C.byref(n), C.byref(fl)) == 0
                finally:
                    lib.om_kernel_timing_enable(0)
                got[sw] = (n.value, fl.value)
        assert got[0] == (4 * layers, per_row * FB * FL), (name, mname, got)
        assert got[1] == (4 * layers, per_row * R + qkv0_all_rows * 2.0 * 3 * H * H * (FB * FL - R)), (name, mname, R, got)
    assert (_tokens(masks["ragged"][1]) + 255) // 256 * 256 < FB * FL and _tokens(masks["under-256"][1]) < 256
