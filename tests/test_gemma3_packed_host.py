"""Packed rows for EmbeddingGemma on the host (no GPU): the three om_gemma3_encoder_*_packed entries and the two kernel hooks resolve,
the library's rule and the host's rule answer as include/openmatch_hip.h states them, the reference batches of
tests/test_gemma3_packed_encode.py save a tile and plan the GEMM families their assertions rest on (om_debug_gemm_plan: the planner
picks a tile family from the row count, so "packed bits == padded bits" holds only where both row counts plan alike), and the packed
entry refuses before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import encoder as E
from openmatch_amd import native as N
from tests.test_causal_lm import _left
from tests.test_gemma3_host import TINY, _c_config
from tests.test_modernbert import _ragged

EG = dict(hidden_size=768, num_attention_heads=3, num_key_value_heads=1, head_dim=256, intermediate_size=1152)
CODES = (N.OM_F32, N.OM_F16, N.OM_BF16)
# (shape, sequences, length, shortest row, seed of the lengths): ragged right-padded batches.  "same": every contraction plans the same
# family for B * L rows and for the bound (bit-equality is asserted on the GPU); "differ": at least one does not (held to HF alone).
BATCHES = {"tiny-16x128": (TINY, 16, 128, 42, 1, "same"), "tiny-8x320": (TINY, 8, 320, 80, 1, "same"), "tiny-4x1024": (TINY, 4, 1024, 256, 1, "same"),
           "eg-16x128": (EG, 16, 128, 42, 3, "same"), "eg-5x640": (EG, 5, 640, 160, 1, "same"), "eg-64x128": (EG, 64, 128, 32, 1, "differ")}


def batch(key):
    shape, n, L, lo, seed, _ = BATCHES[key]
    return _ragged(np.random.default_rng(seed), n, L, lo)


def short_batch():
    """16 x 128 with 128 + 15 x 50 = 878 tokens: a bound of 1 024 rows, AT the few-rows threshold"""
    rng = np.random.default_rng(9)
    ids, mask = np.zeros((16, 128), np.int64), np.zeros((16, 128), np.int64)
    for i in range(16):
        n = 128 if i == 0 else 50
        ids[i, :n] = rng.integers(3, 600, n)
        mask[i, :n] = 1
    return ids, mask


def planned_families(code, shape, rows):
    """om_debug_gemm_plan for the five contractions of a layer (csrc/encoder_gemma3.hip) over `rows` rows: qkv, o_proj, up_proj,
    gate_proj with the tanh-GELU x up epilogue, down_proj.  Every buffer gets a made-up base address of its own, 512-byte aligned as the
    device allocator's are (tests/test_gemm_kernels.py::planned_family)."""
    H, F = shape["hidden_size"], shape["intermediate_size"]
    A = shape["num_attention_heads"] * 256
    P = A + 2 * shape["num_key_value_heads"] * 256
    bases = iter(range(1 << 30, 1 << 40, 1 << 30))
    y, qkv, ctx, ff, ff2 = (next(bases) for _ in range(5))

    def plan(a, lda, c, ldc, Nn, K, r=None, ldr=0, act=N.ACT_NONE):
        return N.lib().om_debug_gemm_plan(code, a, lda, next(bases), K, code, c, ldc, rows, Nn, K, None, r, ldr, act)
    return (plan(y, H, qkv, P, P, H), plan(ctx, A, y, H, H, A), plan(y, H, ff2, F, F, H),
            plan(y, H, ff, F, F, H, ff2, F, N.ACT_GELU_TANH | N.ACT_MUL_RESID), plan(ff, F, y, H, H, F))


def _cfg(shape=EG, **over):
    return _c_config(hidden=shape["hidden_size"], n_heads=shape["num_attention_heads"], n_kv_heads=shape["num_key_value_heads"],
                     ffn=shape["intermediate_size"], **over)


def test_symbols_resolve_and_the_abi_version_stays():
    lib = N.lib()
    for name in ("om_gemma3_encoder_packed_supported", "om_gemma3_encoder_workspace_bytes_packed", "om_gemma3_encoder_forward_packed",
                 "om_debug_attention_gqa_d256_packed", "om_debug_qknorm_rope_d256_rows"):
        assert hasattr(lib, name) and name in N.exported_symbols(), name
    assert lib.om_abi_version() == 6 == N.ABI_VERSION
    assert C.sizeof(N.OmGemma3Config) == 1288 and C.sizeof(N.OmCausalConfig) == 232 and C.sizeof(N.OmGemma3Norms) == 32


def test_supported_truth_table():
    lib = N.lib()
    ok = lambda gc, B=16, L=128, rows=1536: lib.om_gemma3_encoder_packed_supported(C.byref(gc), B, L, rows)      # noqa: E731
    assert lib.om_debug_option_value(N.OPT_GEMM_SKINNY_M) == 1024
    for shape in (TINY, EG):
        for code in CODES:
            for rows in (1280, 1536, 1792):
                assert ok(_cfg(shape, dtype=code), rows=rows) == 1, (shape, code, rows)
    gc = _cfg()
    assert ok(gc, rows=1000) == 0 and ok(gc, rows=1025) == 0              # not whole 256-row tiles
    assert ok(gc, rows=512) == 0 and ok(gc, rows=1024) == 0               # the few-rows clause: packed_rows itself at or below the threshold
    assert ok(gc, rows=0) == 0 and ok(gc, rows=-256) == 0
    assert ok(gc, rows=2048) == 1 and ok(gc, rows=2304) == 0              # at most B * L + 255
    assert ok(gc, B=8, L=128, rows=1280) == 0                             # B * L = 1 024: the padded form AT the threshold
    assert ok(gc, B=9, L=128, rows=1280) == 1
    assert ok(gc, L=1025, rows=1536) == 0
    assert ok(_cfg(head_dim=128)) == 0
    assert ok(_cfg(pooling=N.POOL_LAST)) == 0
    assert ok(_cfg(bidirectional=0)) == 0                                 # the causal flag
    assert ok(_cfg(pooling=N.POOL_FIRST)) == 1 and ok(_cfg(pooling=N.POOL_MEAN)) == 1
    assert lib.om_gemma3_encoder_packed_supported(None, 16, 128, 1536) == 0


def test_host_rule(monkeypatch):
    gc = _cfg()
    ok = lambda rows=1536, B=16, L=128, want_hidden=False, pooling="mean": E.gemma3_packed_rows_apply(gc, B, L, rows, want_hidden, pooling)      # noqa: E731
    assert ok() and ok(rows=1280) and ok(rows=1792) and ok(pooling="first")
    assert not ok(rows=2048) and not ok(rows=2304)                        # no tile saved
    assert not ok(rows=1024) and not ok(rows=512) and not ok(rows=1000)   # the few-rows threshold; not whole tiles
    assert not ok(want_hidden=True) and not ok(pooling=None)
    assert not ok(B=8, rows=768) and not ok(B=9, rows=1280)               # (9 x 128 = 1 152 rows: 1 280 saves nothing)
    assert ok(B=64, rows=5376)
    ids, mask = batch("eg-16x128")
    assert ok(rows=E.packed_rows_bound(torch.from_numpy(mask)))
    left = torch.from_numpy(_left(ids, mask)[1])
    assert E.packed_rows_bound(left) == 2048 == E.rows_bound_of(E.token_rows_of(left))      # every row ends at the last column
    assert not ok(rows=E.packed_rows_bound(left))
    assert not ok(rows=E.packed_rows_bound(torch.from_numpy(short_batch()[1])))
    monkeypatch.setenv("OM_ENCODER_PACKED", "0")
    assert not ok()
    monkeypatch.setenv("OM_ENCODER_PACKED", "1")
    assert ok()
    assert not E.gemma3_packed_rows_apply(_cfg(head_dim=128), 16, 128, 1536, False, "mean")      # the library's own answer


def test_workspace_bytes_of_packed_rows():
    lib = N.lib()
    for shape in (TINY, EG):
        for code in CODES:
            for pooling in (N.POOL_MEAN, N.POOL_FIRST):
                gc = _cfg(shape, dtype=code, pooling=pooling)
                for B, L in ((16, 128), (8, 320), (4, 1024), (7, 200)):
                    padded = lib.om_gemma3_encoder_workspace_bytes(C.byref(gc), B, L)
                    assert padded > 0
                    sizes = [lib.om_gemma3_encoder_workspace_bytes_packed(C.byref(gc), B, L, rows) for rows in range(1280, B * L + 256, 256)]
                    assert all(s > 0 for s in sizes)
                    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes                    # non-decreasing in rows
                    for rows, s in zip(range(1280, B * L + 256, 256), sizes):
                        if rows < B * L:
                            assert s < padded, (B, L, rows, s, padded)
    gc = _cfg()
    assert lib.om_gemma3_encoder_workspace_bytes_packed(None, 16, 128, 1536) == 0
    assert lib.om_gemma3_encoder_workspace_bytes_packed(C.byref(gc), 16, 128, 0) == 0
    for bad in (_cfg(head_dim=128), _cfg(bidirectional=0), _cfg(pooling=N.POOL_LAST)):            # a refused config
        assert lib.om_gemma3_encoder_workspace_bytes_packed(C.byref(bad), 16, 128, 1536) == 0
    # the padded entry's bytes are what they were: x f32 | y | qkv | ctx | ff | ff2 over 1 024 rows + the mean-pooling rows + the small ones
    floor = 1024 * (768 * 4 + (768 + 5 * 256 + 3 * 256 + 2 * 1152) * 2) + 4 * 200 * 768 * 4
    got = lib.om_gemma3_encoder_workspace_bytes(C.byref(_cfg()), 4, 200)
    assert floor <= got <= floor + 16 * 256 + 2 * 4 * 768 * 4


# (dtype, pooling, B, L, packed_rows or 0, bytes) for _c_config's shape: what the library built from the commit BEFORE csrc/prenorm_stack.h
# answered -- under 512 rows, 600 and 800 rows (16-bit: whole 256-row tiles), and packed
WORKSPACE_BYTES = ((N.OM_BF16, N.POOL_FIRST, 3, 40, 0, 1607168), (N.OM_F16, N.POOL_FIRST, 5, 120, 0, 10239488), (N.OM_F32, N.POOL_MEAN, 5, 120, 0, 15990272),
                   (N.OM_BF16, N.POOL_MEAN, 4, 200, 0, 16101888), (N.OM_F16, N.POOL_FIRST, 16, 128, 1024, 13685760),
                   (N.OM_BF16, N.POOL_MEAN, 4, 1024, 1280, 20989952), (N.OM_F32, N.POOL_FIRST, 16, 128, 1536, 36232192))


def test_workspace_bytes_are_what_they_were():
    lib = N.lib()
    for dtype, pooling, B, L, rows, want in WORKSPACE_BYTES:
        gc = _c_config(dtype=dtype, pooling=pooling)
        got = lib.om_gemma3_encoder_workspace_bytes_packed(C.byref(gc), B, L, rows) if rows else lib.om_gemma3_encoder_workspace_bytes(C.byref(gc), B, L)
        assert got == want, (dtype, pooling, B, L, rows)


@pytest.mark.parametrize("key", list(BATCHES))
def test_reference_batches_save_a_tile_and_plan_as_their_assertions_need(key):
    shape, n, L, lo, seed, kind = BATCHES[key]
    ids, mask = batch(key)
    rows = E.packed_rows_bound(torch.from_numpy(mask))
    assert mask[0].all() and rows is not None and rows % 256 == 0 and 1024 < rows <= (n * L) // 256 * 256 - 256, (key, rows)
    for code in CODES:
        for pooling in ("mean", "first"):
            assert E.gemma3_packed_rows_apply(_cfg(shape, dtype=code, pooling=N.POOL_MEAN if pooling == "mean" else N.POOL_FIRST), n, L, rows, False, pooling)
        padded, packed = planned_families(code, shape, n * L), planned_families(code, shape, rows)
        assert all(f > 0 for f in padded + packed), (key, code, padded, packed)
        if kind == "same":
            assert padded == packed, (key, code, n * L, padded, rows, packed)
        else:
            assert any(a != b for a, b in zip(padded, packed)), (key, code, padded, packed)


def test_where_the_planned_families_part():
    """What DESIGN.md section 8 records, as the library reports it at the default switches: over whole-tile row counts from 1 280 up every
    contraction plans one family until 6 656 rows at EmbeddingGemma's widths (8 448 at the tiny model's), where the qkv projection moves"""
    for code in CODES:
        for shape, first in ((EG, 6656), (TINY, 8448)):
            base = planned_families(code, shape, 1280)
            changes = [rows for rows in range(1536, 16640, 256) if planned_families(code, shape, rows) != planned_families(code, shape, rows - 256)]
            assert changes[0] == first, (code, shape, changes)
            assert planned_families(code, shape, first - 256) == base
            assert planned_families(code, shape, first)[0] != base[0] and planned_families(code, shape, first)[1:] == base[1:]
    assert planned_families(N.OM_F16, EG, 1024) != planned_families(N.OM_F16, EG, 1280)      # why packed_rows must lie above the threshold


def test_forward_packed_refuses_on_the_host():
    """the call shape of test_gemma3_host.py::test_every_refusal_comes_back_through_the_c_entry: nothing is launched"""
    lib = N.lib()
    layers = (N.OmLayerWeights * 3)()
    norms = (N.OmGemma3Norms * 3)()
    for i in range(3):
        for name in ("qkv_w", "o_w", "ln1_g", "ln2_g", "ffn1_w", "ffn1g_w", "ffn2_w"):
            setattr(layers[i], name, 256)
        for name, _ in N.OmGemma3Norms._fields_:
            setattr(norms[i], name, 256)
    w = N.OmEncoderWeights(word_emb=256, final_ln_g=256, layers_host=C.cast(layers, C.POINTER(N.OmLayerWeights)))

    def refused(cfg, B=16, L=128, rows=1536, ids=16, mask=16, weights=w, reps=16, ws=256, nbytes=1 << 40):
        rc = lib.om_gemma3_encoder_forward_packed(C.byref(cfg) if cfg is not None else None, C.byref(weights) if weights is not None else None,
                                                  norms, ids, mask, B, L, rows, reps, ws, nbytes, None)
        return lib.om_last_error() if rc != 0 else None
    gc = _cfg()
    for kw in (dict(ids=None), dict(mask=None), dict(weights=None)):
        assert b"null argument" in refused(gc, **kw), kw
    assert b"null argument" in refused(None)
    assert b"positive" in refused(gc, rows=0)
    for rows in (1000, 1025, 2304):
        assert b"multiple of 256" in refused(gc, rows=rows), rows
    assert b"representations only" in refused(_cfg(pooling=N.POOL_NONE))
    assert b"workspace too small" in refused(gc, nbytes=lib.om_gemma3_encoder_workspace_bytes_packed(C.byref(gc), 16, 128, 1536) - 1)
    assert b"256-byte aligned" in refused(gc, ws=None)
    assert b"out_reps" in refused(gc, reps=None)
    assert b"1024" in refused(gc, L=1025)
    assert b"head_dim 256" in refused(_cfg(head_dim=128))
    assert b"last" in refused(_cfg(pooling=N.POOL_LAST))
    norms[2].k_norm_g = None
    assert b"k_norm_g" in refused(gc)
    norms[2].k_norm_g = 256
    # the hooks check their arguments on the host
    inv = (C.c_float * 128)(*([0.5] * 128))
    assert lib.om_debug_attention_gqa_d256_packed(N.OM_F32, 256, 256, 256, None, 1, 8, 3, 1, 0.0625, 0, None) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_attention_gqa_d256_packed(N.OM_F32, 256, 256, 256, 256, 1, 1025, 3, 1, 0.0625, 0, None) != 0 and b"1024" in lib.om_last_error()
    assert lib.om_debug_attention_gqa_d256_packed(N.OM_F32, 256, 256, 256, 256, 1, 8, 3, 2, 0.0625, 0, None) != 0 and b"divide" in lib.om_last_error()
    assert lib.om_debug_attention_gqa_d256_packed(7, 256, 256, 256, 256, 1, 8, 3, 1, 0.0625, 0, None) != 0 and b"dtype" in lib.om_last_error()
    assert lib.om_debug_qknorm_rope_d256_rows(N.OM_F32, 256, 8, 8, 3, 1, 256, 256, 1e-6, inv, 1.0, None, None) != 0 and b"null" in lib.om_last_error()
    assert lib.om_debug_qknorm_rope_d256_rows(N.OM_F32, 256, 8, 1025, 3, 1, 256, 256, 1e-6, inv, 1.0, 256, None) != 0 and b"1024" in lib.om_last_error()
