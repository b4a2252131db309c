"""Packed rows for the decoder-only stack (om_causal_encoder_forward_packed; csrc/encoder_causal.hip, csrc/attention_causal.hip): each
sequence's rows up to its last unmasked token, back to back.  The kernels alone against their padded forms bit for bit (the same
bodies and the same chunk walk, only the base pointers differ) and against the float64 reference under the bound of
tests/test_attention_kernels.py; the entry end to end against HF fp32 at the bars of tests/test_causal_lm.py and against the padded
entry bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from openmatch_amd import encoder as E
from openmatch_amd import native as N
from tests.helpers import NS
from tests.test_attention_causal import D, GROUPS, LENGTHS, ROPES, SCALE, _hf_rotary, grouped_inputs, padding_masks, run_case
from tests.test_attention_kernels import (BF16, BITS_DT, DEV, F16, F32, NAME, TORCH_DT, bits, mask_extent, new_ctx, pack_rows, rows_of,
                                          untouched, violations)
from tests.test_causal_lm import LLAMA3, QWEN05, SMALL, _check, _hf_reps, _left, _lm, _model, _ragged, _rel

DTYPES = ("float32", "float16", "bfloat16")
# (shape, layers, sequences, length, shortest row, seed of the lengths): ragged right-padded batches whose row bound saves at least one
# 256-row tile (test_reference_batches_save_a_tile checks that on the CPU).  The Qwen2-0.5B width runs at 16 x 128: 8 x 128 is 1 024
# padded rows, AT the few-rows threshold where om_causal_encoder_packed_supported answers 0 by its contract -- that batch is asserted
# to stay on the padded entry instead (test_batch_at_the_few_rows_threshold_stays_padded).
BATCHES = {"small-16x128": (SMALL, 3, 16, 128, 40, 1), "small-8x320": (SMALL, 3, 8, 320, 100, 2), "small-4x1024": (SMALL, 3, 4, 1024, 300, 3),
           "qwen05-16x128": (QWEN05, 2, 16, 128, 30, 4)}


def _batch(key):
    shape, layers, n, L, lo, seed = BATCHES[key]
    ids, mask = _ragged(np.random.default_rng(seed), n, L, lo)
    return shape, layers, ids, mask


def _causal_cfg(shape=SMALL, dtype=N.OM_F16, pooling=N.POOL_LAST, layers=1):
    f = dict(arch=N.ARCH_CAUSAL, dtype=dtype, hidden=shape["hidden_size"], n_layers=layers, n_heads=shape["num_attention_heads"], head_dim=64,
             ffn=shape["intermediate_size"], vocab=600, act=N.ACT_SILU, ln_eps=1e-6, pooling=pooling)
    return N.OmCausalConfig(base=N.OmEncoderConfig(**f), n_kv_heads=shape["num_key_value_heads"], rope_attention_scaling=1.0,
                            inv_freq=(C.c_float * 32)(*([0.5] * 32)))


# ------------------------------------------------------------------------------------------------------------- CPU
def test_symbols_resolve_and_the_abi_version_stays():
    lib = N.lib()
    for name in ("om_causal_encoder_packed_supported", "om_causal_encoder_workspace_bytes_packed", "om_causal_encoder_forward_packed",
                 "om_debug_attention_causal_packed", "om_debug_rope_gqa_rows"):
        assert hasattr(lib, name) and name in N.exported_symbols(), name
    assert lib.om_abi_version() == 6 == N.ABI_VERSION
    assert C.sizeof(N.OmCausalConfig) == 232


def test_supported_truth_table():
    lib = N.lib()
    ok = lambda cc, B=16, L=128, rows=1024: lib.om_causal_encoder_packed_supported(C.byref(cc), B, L, rows)      # noqa: E731
    for shape in (SMALL, QWEN05):
        for dtype in (N.OM_F32, N.OM_F16, N.OM_BF16):
            assert ok(_causal_cfg(shape, dtype)) == 1, (shape, dtype)
    cc = _causal_cfg()
    assert ok(cc, rows=1000) == 0 and ok(cc, rows=1025) == 0              # not whole 256-row tiles
    assert ok(cc, rows=256) == 0 and ok(cc, rows=0) == 0                  # below 512
    assert ok(cc, rows=2048) == 1 and ok(cc, rows=2304) == 0              # at most B * L + 255
    assert ok(cc, B=17, L=127, rows=2304) == 1 and ok(cc, B=17, L=127, rows=2560) == 0      # (2 159 tokens: 2 414 is the limit)
    assert ok(cc, L=1025, rows=1024) == 0
    skinny = lib.om_debug_option_value(N.OPT_GEMM_SKINNY_M)
    assert skinny == 1024
    assert ok(cc, B=8, L=128, rows=512) == 0 and ok(cc, B=8, L=128, rows=768) == 0          # B * L AT the few-rows threshold
    assert ok(cc, B=9, L=128, rows=768) == 1
    cc.base.head_dim = 128
    assert ok(cc) == 0
    cc.base.head_dim = 64
    cc.base.arch = N.ARCH_BERT
    assert ok(cc) == 0
    cc.base.arch = N.ARCH_CAUSAL
    cc.n_kv_heads = 3
    assert ok(cc) == 0
    cc.n_kv_heads = 2
    assert ok(cc) == 1
    assert lib.om_causal_encoder_packed_supported(None, 16, 128, 1024) == 0


def test_workspace_bytes_of_packed_rows():
    lib = N.lib()
    for shape in (SMALL, QWEN05):
        for dtype in (N.OM_F32, N.OM_F16, N.OM_BF16):
            for pooling in (N.POOL_LAST, N.POOL_MEAN, N.POOL_FIRST):
                cc = _causal_cfg(shape, dtype, pooling)
                for B, L in ((16, 128), (8, 320), (4, 1024), (7, 100)):
                    padded = lib.om_causal_encoder_workspace_bytes(C.byref(cc), B, L)
                    sizes = [lib.om_causal_encoder_workspace_bytes_packed(C.byref(cc), B, L, rows) for rows in range(512, B * L + 256, 256)]
                    assert all(s > 0 for s in sizes)
                    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes                    # non-decreasing in rows
                    for rows, s in zip(range(512, B * L + 256, 256), sizes):
                        if rows < B * L:
                            assert s < padded, (B, L, rows, s, padded)
    assert lib.om_causal_encoder_workspace_bytes_packed(None, 16, 128, 1024) == 0
    assert lib.om_causal_encoder_workspace_bytes_packed(C.byref(cc), 16, 128, 0) == 0


# (dtype, pooling, B, L, packed_rows or 0, bytes) for _causal_cfg's shape: what the library built from the commit BEFORE csrc/prenorm_stack.h
# answered -- under 512 rows, 600 and 800 rows (16-bit: whole 256-row tiles), and packed
WORKSPACE_BYTES = ((N.OM_BF16, N.POOL_LAST, 3, 40, 0, 556800), (N.OM_F16, N.POOL_FIRST, 5, 120, 0, 3544832), (N.OM_F32, N.POOL_MEAN, 5, 120, 0, 5535488),
                   (N.OM_BF16, N.POOL_MEAN, 4, 200, 0, 5542656), (N.OM_F16, N.POOL_LAST, 16, 128, 1024, 4740352),
                   (N.OM_BF16, N.POOL_MEAN, 4, 1024, 1280, 7219456), (N.OM_F32, N.POOL_FIRST, 16, 128, 1536, 12606720))


def test_workspace_bytes_are_what_they_were():
    lib = N.lib()
    for dtype, pooling, B, L, rows, want in WORKSPACE_BYTES:
        cc = _causal_cfg(dtype=dtype, pooling=pooling)
        got = lib.om_causal_encoder_workspace_bytes_packed(C.byref(cc), B, L, rows) if rows else lib.om_causal_encoder_workspace_bytes(C.byref(cc), B, L)
        assert got == want, (dtype, pooling, B, L, rows)


def test_a_null_layer_pointer_is_refused_before_the_first_launch():
    """o_w of layer 1 of 3 is null: the refusal comes back on a machine without a GPU, so nothing was launched for layer 0 (fake
    non-null pointers, no stream: the call shape of tests/test_gemma3_host.py::test_every_refusal_comes_back_through_the_c_entry)"""
    lib = N.lib()
    layers = (N.OmLayerWeights * 3)()
    for i in range(3):
        for name in ("qkv_w", "o_w", "ln1_g", "ln2_g", "ffn1_w", "ffn1g_w", "ffn2_w"):
            setattr(layers[i], name, 256)
    layers[1].o_w = None
    w = N.OmEncoderWeights(word_emb=256, final_ln_g=256, layers_host=C.cast(layers, C.POINTER(N.OmLayerWeights)))
    cc = _causal_cfg(layers=3)
    assert lib.om_causal_encoder_forward(C.byref(cc), C.byref(w), 16, 16, 1, 8, None, 16, 256, 1 << 40, None) != 0
    assert b"Llama / Qwen2 layers need qkv_w, o_w" in lib.om_last_error()
    assert lib.om_causal_encoder_forward_packed(C.byref(cc), C.byref(w), 16, 16, 16, 128, 1024, 16, 256, 1 << 40, None) != 0
    assert b"Llama / Qwen2 layers need qkv_w, o_w" in lib.om_last_error()


def test_forward_refuses_on_the_host():
    """the call shape of test_abi_is_unchanged_and_the_causal_struct_embeds_the_config: nothing is launched"""
    lib = N.lib()
    w = N.OmEncoderWeights()

    def refused(cfg, B=16, L=128, rows=1024, ids=16, mask=16, weights=w):
        return lib.om_causal_encoder_forward_packed(C.byref(cfg) if cfg is not None else None, C.byref(weights) if weights is not None else None,
                                                    ids, mask, B, L, rows, 16, 256, 1 << 30, None)
    cc = _causal_cfg()
    for kw in (dict(ids=None), dict(mask=None), dict(weights=None)):
        assert refused(cc, **kw) != 0 and b"null argument" in lib.om_last_error()
    assert refused(None) != 0 and b"null argument" in lib.om_last_error()
    none = _causal_cfg(pooling=N.POOL_NONE)
    assert refused(none) != 0 and b"representations only" in lib.om_last_error()
    for rows in (1000, 256, 2304):
        assert refused(cc, rows=rows) != 0 and b"multiple of 256 in [512, B * L + 255]" in lib.om_last_error(), rows
    assert refused(cc, rows=0) != 0 and b"positive" in lib.om_last_error()
    assert refused(cc, L=1025) != 0 and b"1024" in lib.om_last_error()
    cc.base.head_dim = 128
    assert refused(cc) != 0 and b"head_dim 64" in lib.om_last_error()


def test_host_rule(monkeypatch):
    cc = _causal_cfg()
    ok = lambda rows=1024, B=16, L=128, want_hidden=False, pooling="last": E.causal_packed_rows_apply(cc, B, L, rows, want_hidden, pooling)      # noqa: E731
    assert ok() and ok(rows=512) and ok(rows=1792)
    assert not ok(rows=2048) and not ok(rows=256) and not ok(rows=1000)         # no tile saved; below 512; not whole tiles
    assert not ok(want_hidden=True) and not ok(pooling=None)
    assert not ok(B=8, rows=512)                                                 # the library's few-rows rule
    ids, mask = _ragged(np.random.default_rng(1), 16, 128, 40)
    assert ok(rows=E.packed_rows_bound(torch.from_numpy(mask)))
    left = torch.from_numpy(_left(ids, mask)[1])
    assert E.packed_rows_bound(left) == 2048 == E.rows_bound_of(E.token_rows_of(left))      # every row ends at the last column
    assert not ok(rows=E.packed_rows_bound(left))
    monkeypatch.setenv("OM_ENCODER_PACKED", "0")
    assert not ok()


def test_reference_batches_save_a_tile():
    for key, (shape, layers, n, L, lo, seed) in BATCHES.items():
        _, _, ids, mask = _batch(key)
        rows = E.packed_rows_bound(torch.from_numpy(mask))
        assert mask[0].all() and rows is not None and 512 <= rows <= (n * L) // 256 * 256 - 256, (key, rows)
        assert E.causal_packed_rows_apply(_causal_cfg(shape), n, L, rows, False, "last"), key
        half = _mixed(ids, mask)[1]
        rows = E.packed_rows_bound(torch.from_numpy(half))
        if key == "small-16x128":
            assert rows <= (n * L) // 256 * 256 - 256, rows


# ------------------------------------------------------------------------------------------------------------- GPU, kernels alone
def _packed_launch(dtype, qp, ctx, mask, cu, B, L, heads, kv):
    rc = N.lib().om_debug_attention_causal_packed(dtype, N.ptr(qp), N.ptr(ctx), N.ptr(mask), N.ptr(cu), B, L, heads, kv, SCALE, N.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
@pytest.mark.parametrize("heads,kv", GROUPS)
@pytest.mark.parametrize("L", LENGTHS)
def test_packed_attention_is_the_padded_kernel_row_for_row(L, heads, kv, dtype):
    """Every query below its sequence's extent: the bits of om_debug_attention_causal's row b * L + q, hence within the bound of the
    float64 reference where the query is in contract; rows of ctx at and beyond the token count keep the sentinel."""
    B = 5 if L <= 512 else 4
    mask = padding_masks(B, L)
    padded, ref, bound, contract = run_case(dtype, B, L, heads, kv, mask)
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=77 + 13 * L + heads + kv)
    mask = mask.to(DEV)
    kmax = mask_extent(mask)
    total = int(kmax.sum())
    rows = total + 7
    cu, _, row_map = pack_rows(kmax, L, rows)
    assert int(cu[B]) == total and int(cu[B + 1]) == total
    src = row_map[:total].long()
    qp = torch.zeros(rows, qkv.shape[1], dtype=TORCH_DT[dtype], device=DEV)
    qp[:total] = qkv[src]
    qp0 = qp.clone()
    ctx = new_ctx(rows, heads * D, dtype)
    assert _packed_launch(dtype, qp, ctx, mask, cu, B, L, heads, kv) == 0, N.lib().om_last_error()
    assert torch.equal(bits(qp, dtype), bits(qp0, dtype))
    flat = padded.reshape(B * L, heads * D)
    assert torch.equal(bits(ctx[:total].contiguous(), dtype), bits(flat[src].contiguous(), dtype))
    assert untouched(ctx[total:], dtype), "rows at and beyond the token count were written"
    got = torch.zeros(B * L, heads * D, dtype=TORCH_DT[dtype], device=DEV)
    got[src] = ctx[:total]
    inside = torch.zeros(B * L, dtype=torch.bool, device=DEV)
    inside[src] = True
    inside = inside.view(B, L) & contract
    bad = violations(got.view(B, L, heads * D), ref, bound, inside)
    ratio = ((got.view(B, L, -1).double() - ref).abs() / bound)[rows_of(inside, heads * D)]
    print(f"packed causal {NAME[dtype]} L={L} heads={heads} kv={kv}: max err/bound {ratio.max().item():.3f}, rows {total} of {B * L}")
    assert not bad.any(), (int(bad.sum()), ratio.max().item())
    assert torch.equal(inside, contract)                   # every query in contract lies inside its sequence's extent


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_packed_attention_under_a_row_bound_that_is_too_small(dtype):
    """The bound ends ten rows into the third sequence: the fourth and fifth hold no rows.  The first two carry the padded bits; the
    ten rows of the third are finite (it is left-padded: they are masked queries without a visible key, outside the contract, which
    average the keys their chunk holds -- ten here, 128 in the padded call); nothing past the bound is written."""
    B, L, heads, kv = 5, 320, 4, 2
    mask = padding_masks(B, L)
    padded, _, _, _ = run_case(dtype, B, L, heads, kv, mask)
    qkv = grouped_inputs(dtype, B, L, heads, kv, seed=77 + 13 * L + heads + kv)
    mask = mask.to(DEV)
    kmax = mask_extent(mask)
    rows = int(kmax[:2].sum()) + 10
    cu, _, row_map = pack_rows(kmax, L, rows)
    assert cu.tolist()[2:] == [rows - 10, rows, rows, rows, int(kmax.sum())]
    src = row_map.long()
    assert int(src.min()) >= 0
    extra = 64
    qp = torch.zeros(rows + extra, qkv.shape[1], dtype=TORCH_DT[dtype], device=DEV)
    qp[:rows] = qkv[src]
    ctx = new_ctx(rows + extra, heads * D, dtype)
    assert _packed_launch(dtype, qp, ctx, mask, cu, B, L, heads, kv) == 0, N.lib().om_last_error()
    flat = padded.reshape(B * L, heads * D)
    whole = rows - 10
    assert int(mask[2, :10].sum()) == 0
    assert torch.equal(bits(ctx[:whole].contiguous(), dtype), bits(flat[src[:whole]].contiguous(), dtype))
    assert torch.isfinite(ctx[whole:rows].double()).all()
    assert untouched(ctx[rows:], dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["default", "llama3"])
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=lambda d: NAME[d])
def test_packed_rope_is_the_padded_pass_gathered(dtype, kind):
    B, L, heads, kv = 4, 257, 4, 2
    rot, _, _ = _hf_rotary(ROPES[kind], L)
    inv = (C.c_float * 32)(*[float(v) for v in rot.inv_freq])
    scaling = float(rot.attention_scaling)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[1, 100:] = 0
    mask[2, :200] = 0                                       # left-padded: its rows keep their columns
    mask[3, 1:] = 0
    mask = mask.to(DEV)
    x = torch.randn(B * L, (heads + 2 * kv) * D, generator=torch.Generator().manual_seed(5)).to(TORCH_DT[dtype]).to(DEV)
    padded = x.clone()
    N.check(N.lib().om_debug_rope_gqa(dtype, N.ptr(padded), B * L, L, heads, kv, inv, scaling, N.stream_ptr()))
    kmax = mask_extent(mask)
    total = int(kmax.sum())
    assert total == L + 100 + L + 1
    rows = total + 9
    _, _, row_map = pack_rows(kmax, L, rows)
    assert (row_map[total:] == -1).all()
    src = row_map[:total].long()
    xp = torch.randn(rows, x.shape[1], generator=torch.Generator().manual_seed(6)).to(TORCH_DT[dtype]).to(DEV)
    xp[:total] = x[src]
    xp0 = xp.clone()
    N.check(N.lib().om_debug_rope_gqa_rows(dtype, N.ptr(xp), rows, L, heads, kv, inv, scaling, N.ptr(row_map), N.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(bits(xp[:total].contiguous(), dtype), bits(padded[src].contiguous(), dtype))
    assert torch.equal(bits(xp[total:].contiguous(), dtype), bits(xp0[total:].contiguous(), dtype))          # the -1 rows
    vcol = (heads + kv) * D
    assert torch.equal(bits(xp[:, vcol:].contiguous(), dtype), bits(xp0[:, vcol:].contiguous(), dtype))      # the v heads
    assert not torch.equal(bits(xp[:total, :vcol].contiguous(), dtype), bits(xp0[:total, :vcol].contiguous(), dtype))
    lib = N.lib()
    assert lib.om_debug_rope_gqa_rows(dtype, N.ptr(xp), rows, L, heads, kv, inv, scaling, None, N.stream_ptr()) != 0
    assert lib.om_debug_rope_gqa_rows(dtype, N.ptr(xp), rows, 1025, heads, kv, inv, scaling, N.ptr(row_map), N.stream_ptr()) != 0


# ------------------------------------------------------------------------------------------------------------- GPU, end to end
def _mixed(ids, mask):
    """every second row left-padded: leading pad tokens inside a packed extent"""
    li, lm_ = _left(ids, mask)
    ids2, mask2 = ids.copy(), mask.copy()
    ids2[1::2], mask2[1::2] = li[1::2], lm_[1::2]
    return ids2, mask2


def _encode(lm, ids, mask, pooling, dtype, head=None, normalize=False, packed=True):
    """DRModelForInference.encode_passage on device tensors; packed: with the token counts of the mask as the HOST holds it
    (encoder.token_rows_of), from which the model computes the row bound.  Returns (reps, LAST_CALL)."""
    model = _model(lm, pooling, dtype, head, normalize)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    if packed:
        items[E.TOKEN_ROWS_KEY] = E.token_rows_of(torch.from_numpy(mask))
    with torch.no_grad():
        hidden, r = model.encode_passage(items, want_hidden=False)
    assert hidden is None
    call = dict(E.LAST_CALL)
    lm.to("cpu")
    if head is not None:
        head.to("cpu")
    return r.double().cpu(), call


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(BATCHES))
def test_packed_encode_matches_hf_and_the_padded_entry(key):
    """`last` bare, `mean` + LinearHead + normalize, `first`: HF fp32 at the bars of tests/test_causal_lm.py::_check, and the bits of
    the padded entry on the same batch in every format."""
    from openmatch.modeling import LinearHead
    shape, layers, ids, mask = _batch(key)
    n, L = ids.shape
    H = shape["hidden_size"]
    lm = _lm("qwen2" if shape is QWEN05 or L == 320 else "llama", shape, layers=layers, seed=200 + L)
    torch.manual_seed(300 + L)
    head = LinearHead(H, 256)
    want_rows = E.packed_rows_bound(torch.from_numpy(mask))
    for pooling, hd, norm in (("last", None, False), ("mean", head, True), ("first", None, False)):
        lin = hd.linear if hd is not None else None
        want = _hf_reps(lm, ids, mask, pooling, lin, norm)
        for dtype in DTYPES:
            got, call = _encode(lm, ids, mask, pooling, dtype, hd, norm)
            assert call == {"rows": want_rows, "packed": True} and call["rows"] < n * L, (call, dtype, pooling)
            _check(got, want, dtype, f"causal packed {key} {pooling}", (lm, ids, mask, pooling, lin, norm))
            padded, call = _encode(lm, ids, mask, pooling, dtype, hd, norm, packed=False)
            assert call == {"rows": n * L, "packed": False}
            assert torch.equal(got, padded), (key, pooling, dtype, (got - padded).abs().max().item())


@pytest.mark.gpu
def test_leading_pad_tokens_inside_a_packed_extent():
    """half of the rows left-padded: their extent is the whole row, the right-padded half still saves tiles"""
    shape, layers, ids, mask = _batch("small-16x128")
    ids, mask = _mixed(ids, mask)
    lm = _lm("llama", seed=401)
    for pooling in ("last", "mean"):
        want = _hf_reps(lm, ids, mask, pooling)
        for dtype in DTYPES:
            got, call = _encode(lm, ids, mask, pooling, dtype)
            assert call["packed"] is True and call["rows"] < ids.size, call
            _check(got, want, dtype, f"causal packed mixed padding {pooling}", (lm, ids, mask, pooling, None, False))
            padded, _ = _encode(lm, ids, mask, pooling, dtype, packed=False)
            assert torch.equal(got, padded), (pooling, dtype)


@pytest.mark.gpu
def test_left_padded_batch_stays_on_the_padded_entry():
    shape, layers, ids, mask = _batch("small-16x128")
    ids, mask = _left(ids, mask)
    lm = _lm("qwen2", seed=402)
    want = _hf_reps(lm, ids, mask, "last")
    for dtype in DTYPES:
        got, call = _encode(lm, ids, mask, "last", dtype)
        assert call == {"rows": ids.size, "packed": False}
        _check(got, want, dtype, "causal left-padded, bound given", (lm, ids, mask, "last", None, False))
        padded, _ = _encode(lm, ids, mask, "last", dtype, packed=False)
        assert torch.equal(got, padded)


@pytest.mark.gpu
def test_batch_at_the_few_rows_threshold_stays_padded():
    """Qwen2-0.5B width at 8 x 128: 1 024 padded rows, where the padded entry's contractions take the few-rows kernels"""
    lm = _lm("qwen2", QWEN05, layers=2, seed=403)
    ids, mask = _ragged(np.random.default_rng(5), 8, 128, 16)
    assert E.packed_rows_bound(torch.from_numpy(mask)) in (512, 768)
    want = _hf_reps(lm, ids, mask, "last")
    for dtype in DTYPES:
        got, call = _encode(lm, ids, mask, "last", dtype)
        assert call == {"rows": 1024, "packed": False}
        _check(got, want, dtype, "qwen2-0.5B width 8 x 128, bound given", (lm, ids, mask, "last", None, False))


@pytest.mark.gpu
def test_llama3_rope_positions_survive_packing():
    """the case of tests/test_causal_lm.py::test_llama3_rope through the packed entry"""
    lm = _lm("llama", seed=51, sharp=6.0, rope_parameters=LLAMA3)
    plain = _lm("llama", seed=51)
    plain.load_state_dict(lm.state_dict())
    ids, mask = _ragged(np.random.default_rng(51), 3, 512, 300)
    want = _hf_reps(lm, ids, mask, "last")
    assert _rel(_hf_reps(plain, ids, mask, "last"), want) > 0.05
    for dtype in DTYPES:
        got, call = _encode(lm, ids, mask, "last", dtype)
        assert call["packed"] is True and call["rows"] < 3 * 512, call
        _check(got, want, dtype, "llama3 rope L=512 packed", (lm, ids, mask, "last", None, False))


@pytest.mark.gpu
@pytest.mark.parametrize("pooling", ["last", "mean", "first"])
def test_a_bound_that_is_too_small_poisons_the_batch(pooling):
    shape, layers, ids, mask = _batch("small-16x128")
    lm = _lm("llama", seed=404)
    model = _model(lm, pooling, "float16")
    code = E.compute_dtype_code(model.model_args)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    rows = E.packed_rows_bound(torch.from_numpy(mask))
    assert rows - 256 >= 512 and int(E.token_rows_of(torch.from_numpy(mask)).sum()) > rows - 256
    with torch.no_grad():
        small = E.hip_encode(model.lm_p, items, pooling, None, False, code, want_hidden=False, packed_rows=rows - 256)[1]
        assert E.LAST_CALL == {"rows": rows - 256, "packed": True}
        assert not torch.isfinite(small).any()
        good = E.hip_encode(model.lm_p, items, pooling, None, False, code, want_hidden=False, packed_rows=rows)[1]
        assert E.LAST_CALL == {"rows": rows, "packed": True}
        padded = E.hip_encode(model.lm_p, items, pooling, None, False, code, want_hidden=False)[1]
    assert torch.isfinite(good).all() and torch.equal(good, padded)
    lm.to("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_encoder_over_qwen2_takes_packed_rows(dtype):
    """RRModel on the collator's compact batch (host-side lengths): the scores of the padded call, bit for bit"""
    from openmatch.modeling import LinearHead, RRModel
    from openmatch_amd.feed import pack_token_batch, token_rows_bound
    lm = _lm("qwen2", seed=71)
    torch.manual_seed(72)
    head = LinearHead(256, 1)
    ids, mask = _ragged(np.random.default_rng(7), 12, 160, 40)
    batch = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask)}
    compact = pack_token_batch(dict(batch))
    rows = token_rows_bound(compact)
    assert rows is not None and 512 <= rows <= (12 * 160) // 256 * 256 - 256
    model = RRModel(lm=lm, head=head, pooling="last", model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()
    with torch.no_grad():
        padded = model.encode({k: v.to(DEV) for k, v in batch.items()})
        assert E.LAST_CALL == {"rows": 12 * 160, "packed": False}
        packed = model.encode(compact)
        assert E.LAST_CALL == {"rows": rows, "packed": True}
    assert packed.shape == (12, 1) and torch.isfinite(packed).all()
    assert torch.equal(packed, padded)
    if dtype == "float32":
        want = _hf_reps(lm.to("cpu"), ids, mask, "last", head.to("cpu").linear)
        assert (packed.double().cpu() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())
