"""[CLS] rows of the last layer: with pooling "first" the fused BERT forward runs what follows its last layer's attention
-- out-proj, FFN1, FFN2 and their row statistics -- over the B [CLS] rows, gathered into roundup256(B) compact rows, not over every token.

  CPU   the rule (csrc/encoder_plan.h encoder_cls_tail) through om_debug_encoder_cls_tail, a table written out by hand; the plan word and
        the workspace size do not know about it
  CPU   the three last-layer epilogues plan the same GEMM family at the compact heights as at the full height
  GPU   the gather kernel alone through om_debug_gather_rows: bytes, replicated pad rows, nothing outside the windows
  GPU   the forward: representations with OM_OPT_ENCODER_CLS_TAIL at 1 and at 0 are the same bits through all three entry forms
  GPU   the rule really ran: the 16-bit GEMM flops of one forward price the last layer's three contractions at the compact height"""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.helpers import NS, synth_tokens
from tests.test_encoder_plan import (BASE, BF16, D32, F16, F32, FUSED, OPT_FUSED_LN, OPT_TWO_PLANE, TWO, bert, modernbert, plan, switched,
                                     t5)

DEV = "cuda:0"
OPT_SKIP_PAD, OPT_CLS_TAIL = 22, 23                 # include/openmatch_hip.h: OM_OPT_ENCODER_SKIP_PAD, OM_OPT_ENCODER_CLS_TAIL


# ------------------------------------------------------------------------------------------------------------- CPU
def tail(cfg, B, L, packed=0, gated=0, rel=None, hidden=0):
    c = N.OmEncoderConfig(**cfg)
    if rel is None:
        rel = cfg["arch"] == N.ARCH_T5 or cfg.get("rel_buckets", 0) > 0
    return N.lib().om_debug_encoder_cls_tail(C.byref(c), int(gated), int(rel), B, L, packed, int(hidden))


# (name, configuration, B, L, keyword arguments of tail(), expected) at the default switches
TAIL_TABLE = [
    ("headline_f16", bert(F16), 1024, 128, {}, 1),
    ("headline_bf16", bert(BF16), 1024, 128, {}, 1),
    ("headline_packed", bert(F16), 1024, 128, dict(packed=73728), 1),
    ("b_512", bert(F16), 512, 128, {}, 1),
    ("b_511", bert(F16), 511, 128, {}, 0),
    ("b_24", bert(F16), 24, 128, {}, 0),                     # the shape tests/test_pad_skip.py counts flops on
    ("size_clause_l3", bert(F16), 1024, 3, {}, 0),           # 3 072 rows < 4 * 1 024
    ("size_clause_l4", bert(F16), 1024, 4, {}, 1),
    ("mean_pooling", bert(F16, pooling=N.POOL_MEAN), 1024, 128, {}, 0),
    ("no_pooling", bert(F16, pooling=N.POOL_NONE), 1024, 128, {}, 0),
    ("want_hidden", bert(F16), 1024, 128, dict(hidden=1), 0),
    ("float32", bert(F32), 1024, 128, {}, 0),
    ("one_layer", bert(F16, n_layers=1), 1024, 128, {}, 0),
    ("t5", t5(BF16, pooling=N.POOL_FIRST), 1024, 128, {}, 0),
    ("modernbert", modernbert(F16), 1024, 128, {}, 0),
    ("hidden_128", bert(F16, D32), 1024, 128, {}, 0),
]


def test_tail_rule_without_a_gpu():
    lib = N.lib()
    wrong = [(name, tail(cfg, B, L, **kw), want) for name, cfg, B, L, kw, want in TAIL_TABLE if tail(cfg, B, L, **kw) != want]
    assert not wrong, wrong
    assert lib.om_debug_option_value(OPT_CLS_TAIL) == 1                            # the default
    for opt, value in ((OPT_TWO_PLANE, 7), (OPT_FUSED_LN, 0), (OPT_CLS_TAIL, 0)):  # 7: float16's second plane in eight bits
        with switched(opt, value):
            assert tail(bert(F16), 1024, 128) == 0, (opt, value)
    assert tail(bert(F16), 1024, 128) == 1                                         # every switch is back
    assert lib.om_debug_encoder_cls_tail(None, 0, 0, 1024, 128, 0, 0) == -1
    # neither the plan word nor the workspace size knows about it
    c = N.OmEncoderConfig(**bert(F16))
    with switched(OPT_CLS_TAIL, 0):
        off = plan(bert(F16), 1024, 128), lib.om_encoder_workspace_bytes(C.byref(c), 1024, 128)
    on = plan(bert(F16), 1024, 128), lib.om_encoder_workspace_bytes(C.byref(c), 1024, 128)
    assert off == on and on[0] == FUSED | TWO and on[1] > 0


@pytest.mark.parametrize("two", [False, True], ids=["one-plane", "two-planes"])
@pytest.mark.parametrize("dt", [F16, BF16], ids=["f16", "bf16"])
def test_compact_heights_plan_the_full_height_family(dt, two):
    """om_debug_gemm_plan_ex (no GPU), bert-base widths, default switches: out-proj, FFN1 and FFN2 of the last layer plan the same
    generation-7 family at M = 512, 768 and 1 024 as at M = 131 072"""
    from tests.test_gemm_epilogues import EPS, fake_ep
    from tests.test_gemm_epilogues import plan as gemm_plan
    from tests.test_gemm_kernels import FAM
    H, Fw = BASE["hidden"], BASE["ffn"]
    out_side = dict(bias=1, resid=1, ldr=H, rln_stats=1, rln_g=1, rln_b=1, stats_out=1, ln_inv_h=1.0 / H, ln_eps=EPS)
    if two:
        out_side.update(out_lo=1, resid_lo=1)
    ffn1 = dict(bias=1, act=N.ACT_GELU_ERF, ln_stats=1, ln_colsum=1, ln_inv_h=1.0 / H, ln_eps=EPS)
    g7 = {FAM[k] for k in ("g7", "g7_one_tile", "7c16", "7r16")}
    for name, spec, Nn, K in (("out-proj", out_side, H, H), ("ffn1", ffn1, Fw, H), ("ffn2", out_side, H, Fw)):
        full = gemm_plan(dt, dt, 131072, Nn, K, fake_ep(spec))
        assert full in g7, (name, full)
        for M in (512, 768, 1024):
            assert gemm_plan(dt, dt, M, Nn, K, fake_ep(spec)) == full, (name, M)


# ------------------------------------------------------------------------------------------------------------- GPU, the gather
@pytest.mark.gpu
@pytest.mark.parametrize("rows,L", [([7, 7, 0, 39, 12], 1), (None, 8)], ids=["row-list", "pitch-8"])
def test_gather_rows(rows, L):
    """three 16-bit planes [40, 256] and a statistics array [40, 2] into sentinel-filled destinations of 512 rows, B = 5: rows 0-4 are
    their sources byte for byte, rows 5-511 are row 4, nothing is written outside the windows"""
    from tests.test_gemm_kernels import Buf
    S, H, B, Mc = 40, 256, 5, 512
    gen = torch.Generator(device=DEV).manual_seed(9)
    src = [torch.randn(S, H, generator=gen, device=DEV).to(torch.float16) for _ in range(3)]
    st_src = torch.randn(S, 2, generator=gen, device=DEV)
    dst = [Buf(F16, Mc, H, H) for _ in range(3)]
    st_dst = Buf(F32, Mc, 2, 2, pre=2)                      # (two guard rows: a 16-byte aligned window)
    snaps = [b.snapshot() for b in dst + [st_dst]]
    idx = torch.tensor(rows, dtype=torch.int32, device=DEV) if rows is not None else None
    with torch.cuda.device(DEV):
        rc = N.lib().om_debug_gather_rows(N.ptr(src[0]), dst[0].ptr(), N.ptr(src[1]), dst[1].ptr(), N.ptr(src[2]), dst[2].ptr(), N.ptr(st_src),
                                          st_dst.ptr(), N.ptr(idx), B, L, Mc, H, N.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0, N.lib().om_last_error()
    from_ = rows if rows is not None else [b * L for b in range(B)]
    take = torch.tensor(from_ + [from_[-1]] * (Mc - B), device=DEV)
    for s, d in zip(src + [st_src], dst + [st_dst]):
        assert torch.equal(d.window.contiguous().view(torch.uint8), s[take].contiguous().view(torch.uint8))
    for b, snap in zip(dst + [st_dst], snaps):
        assert b.outside_changed(snap) == 0


# ------------------------------------------------------------------------------------------------------------- GPU, the forward
FL = 16
LAYERS, FH, FF = 2, 256, 1024


def _masks(B):
    """name -> (ids, mask) on the host, L = 16"""
    rng = np.random.default_rng(3)
    ids, ragged = synth_tokens(rng, B, FL, vocab=600, lo_len=5, lo_id=300)
    ragged[0, :] = 1                                   # a full-length row
    ragged[1, :] = 0; ragged[1, 0] = 1                 # a row of one token
    ragged[2, :] = 0                                   # a fully masked row
    ragged[3, :] = 0; ragged[3, ::3] = 1               # holes: the extent is the last unmasked token's
    ragged[B - 1, :] = 0; ragged[B - 1, :2] = 1        # the sequence whose [CLS] row the compact pad rows replicate
    ids = rng.integers(1, 600, (B, FL))
    return {"ragged": (ids, ragged), "ones": (ids, np.ones_like(ragged))}


@pytest.fixture(scope="module")
def forward_env():
    from tests.test_pad_skip import _models
    return _models(), {B: _masks(B) for B in (512, 513)}


def _encode(lm, ids, mask, dtype, packed):
    from openmatch.modeling import DRModelForInference
    from openmatch_amd import encoder as enc_mod
    from openmatch_amd.encoder import compute_dtype_code, hip_encode, packed_rows_bound
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling="first", model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()
    code = compute_dtype_code(model.model_args)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    rows = packed_rows_bound(torch.from_numpy(mask)) if packed else None
    reps = hip_encode(model.lm_p, items, "first", None, False, code, want_hidden=False, packed_rows=rows)[1]
    return reps, dict(enc_mod.LAST_CALL)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", ["bert-4x64", "bert-8x32"])
def test_forward_keeps_its_bits(forward_env, name, dtype):
    """the representations with the switch at 1 and at 0: torch.equal, at B = 512 (Mc = 512) and B = 513 (Mc = 768: replicated pad
    rows), for ragged lengths (a one-token row, a fully masked row, holes, a full-length row) and all ones, through the padded entry,
    the padded entry without pad-skip, and the packed entry"""
    models, masks = forward_env
    lm = models[name]
    heads, hd = (8, 32) if name == "bert-8x32" else (4, 64)
    cfg = N.OmEncoderConfig(arch=N.ARCH_BERT, dtype=F16 if dtype == "float16" else BF16, hidden=FH, n_layers=LAYERS, n_heads=heads, head_dim=hd,
                            ffn=FF, vocab=600, max_pos=160, type_vocab=2, act=N.ACT_GELU_ERF, ln_eps=1e-12, pooling=N.POOL_FIRST)
    lib = N.lib()
    for B in (512, 513):
        for mname, (ids, mask) in masks[B].items():
            for entry, skip_pad, packed in (("padded", 1, False), ("padded-all-rows", 0, False), ("packed", 1, True)):
                label = (name, dtype, B, mname, entry)
                with switched(OPT_SKIP_PAD, skip_pad):
                    got, call = _encode(lm, ids, mask, dtype, packed)
                    with switched(OPT_CLS_TAIL, 0):
                        want, call0 = _encode(lm, ids, mask, dtype, packed)
                torch.cuda.synchronize()
                assert call == call0 and call["packed"] == (packed and mname == "ragged"), label      # (all ones: nothing to pack)
                # the case runs what it names
                assert lib.om_debug_encoder_cls_tail(C.byref(cfg), 0, 0, B, FL, call["rows"] if call["packed"] else 0, 0) == 1, label
                assert torch.isfinite(want).all(), label
                assert torch.equal(got, want), (label, (got - want).abs().max().item())


@pytest.mark.gpu
def test_last_layer_contractions_run_the_compact_rows(forward_env):
    """under om_kernel_timing_enable(1), one B = 512, L = 16 forward without pad-skip (every row count is the host's): 4 launches per
    layer either way; all M rows with the switch at 0, the last layer's out-proj, FFN1 and FFN2 at Mc = 512 rows with it at 1"""
    models, masks = forward_env
    lib = N.lib()
    B, Mc = 512, 512
    M = B * FL
    ids, mask = masks[B]["ragged"]
    ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
    got = {}
    with switched(OPT_SKIP_PAD, 0):
        _encode(models["bert-4x64"], ids, mask, "float16", False)      # weights packed and folded, buffers allocated
        for sw in (0, 1):
            with switched(OPT_CLS_TAIL, sw):
                torch.cuda.synchronize()
                assert lib.om_kernel_timing_enable(1) == 0
                try:
                    assert lib.om_kernel_timing_read(0, C.byref(ms), C.byref(n), C.byref(fl)) == 0      # class 0: 16-bit GEMMs; empties it
                    _encode(models["bert-4x64"], ids, mask, "float16", False)
                    torch.cuda.synchronize()
                    assert lib.om_kernel_timing_read(0, C.byref(ms), C.byref(n), C.byref(fl)) == 0
                finally:
                    lib.om_kernel_timing_enable(0)
                got[sw] = (n.value, fl.value)
    full = LAYERS * 2.0 * M * (4 * FH * FH + 2 * FF * FH)
    assert got[0] == (4 * LAYERS, full), got
    assert got[1] == (4 * LAYERS, full - 2.0 * (M - Mc) * (FH * FH + 2 * FF * FH)), got
