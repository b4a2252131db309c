"""EmbeddingGemma encoded from PACKED rows (om_gemma3_encoder_forward_packed; csrc/encoder_gemma3.hip, csrc/attention_d256.hip) through
DRModelForInference.encode_passage, the mask's token counts held on the host so that the model computes the row bound.  The reference
is HF's bidirectional Gemma3TextModel in fp32, eager, on the CPU (tests/test_gemma3_encode.py) at the bars of test_causal_lm._check;
where the planner picks the same GEMM family for both row counts (asserted on the CPU in tests/test_gemma3_packed_host.py) the packed
representations are also the padded entry's byte for byte."""
import numpy as np
import pytest
import torch

from openmatch_amd import encoder as E
from tests.test_causal_lm import DEV, _check, _hf_reps, _left, _model
from tests.test_gemma3_encode import EG_TYPES
from tests.test_gemma3_host import TINY, TYPES3, gemma_lm
from tests.test_gemma3_packed_host import BATCHES, batch, short_batch

DTYPES = ("float32", "float16", "bfloat16")


def _lm_of(key):
    shape, n, L, _, seed, _ = BATCHES[key]
    if shape is TINY:
        return gemma_lm(TINY, TYPES3, 8, seed=500 + L), 128
    return gemma_lm(shape, EG_TYPES, 512, seed=600 + L), 768


def _encode(lm, ids, mask, pooling, dtype, head=None, normalize=False, packed=True, want_hidden=False):
    """DRModelForInference.encode_passage on device tensors; packed: with the token counts of the mask as the HOST holds it
    (encoder.token_rows_of), from which the model computes the row bound.  Returns (reps, LAST_CALL)."""
    model = _model(lm, pooling, dtype, head, normalize)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    if packed:
        items[E.TOKEN_ROWS_KEY] = E.token_rows_of(torch.from_numpy(mask))
    with torch.no_grad():
        hidden, r = model.encode_passage(items, want_hidden=want_hidden)
    assert (hidden is not None) == want_hidden
    call = dict(E.LAST_CALL)
    lm.to("cpu")
    if head is not None:
        head.to("cpu")
    return r.double().cpu(), call


def _modes(hidden):
    from openmatch.modeling import LinearHead
    torch.manual_seed(700 + hidden)
    head = LinearHead(hidden, hidden)
    return (("mean", head, True), ("mean", None, False), ("first", None, False))


@pytest.mark.gpu
@pytest.mark.parametrize("key", [k for k, v in BATCHES.items() if v[-1] == "same"])
def test_packed_encode_matches_hf_and_the_padded_entry(key):
    """`mean` with and without LinearHead + normalize, `first`: the call runs on the bound's rows, meets HF fp32 at _check's bars and
    carries the bits of the padded entry on the same batch in every format"""
    ids, mask = batch(key)
    n, L = ids.shape
    lm, hidden = _lm_of(key)
    want_rows = E.packed_rows_bound(torch.from_numpy(mask))
    for pooling, hd, norm in _modes(hidden):
        lin = hd.linear if hd is not None else None
        want = _hf_reps(lm, ids, mask, pooling, lin, norm)
        for dtype in DTYPES:
            got, call = _encode(lm, ids, mask, pooling, dtype, hd, norm)
            assert call["packed"] is True and call["rows"] == want_rows < n * L, (call, dtype, pooling)
            _check(got, want, dtype, f"gemma3 packed {key} {pooling}{' head norm' if hd else ''}", (lm, ids, mask, pooling, lin, norm))
            padded, call = _encode(lm, ids, mask, pooling, dtype, hd, norm, packed=False)
            assert call == {"rows": n * L, "packed": False}
            assert torch.equal(got, padded), (key, pooling, dtype, (got - padded).abs().max().item())


@pytest.mark.gpu
def test_large_batch_where_the_gemm_families_part_matches_hf():
    """64 x 128 at EmbeddingGemma's width: 8 192 padded rows plan other tile families than the bound's (test_gemma3_packed_host.py), so no
    bit claim -- the packed entry is held to the padded entry's own bar against HF fp32"""
    key = "eg-64x128"
    ids, mask = batch(key)
    lm, hidden = _lm_of(key)
    want_rows = E.packed_rows_bound(torch.from_numpy(mask))
    want = _hf_reps(lm, ids, mask, "mean")
    for dtype in DTYPES:
        got, call = _encode(lm, ids, mask, "mean", dtype)
        assert call["packed"] is True and call["rows"] == want_rows < ids.size, (call, dtype)
        _check(got, want, dtype, f"gemma3 packed {key} mean", (lm, ids, mask, "mean", None, False))


@pytest.mark.gpu
def test_batches_the_rule_sends_back_stay_on_the_padded_entry(monkeypatch):
    """A left-padded batch (its bound is B * L), a call that asks for hidden states, a 16 x 128 batch whose bound is 1 024 rows (at the
    few-rows threshold) and OM_ENCODER_PACKED=0: the padded entry runs, and gives the padded results"""
    ids, mask = batch("tiny-16x128")
    lm, _ = _lm_of("tiny-16x128")
    li, lmask = _left(ids, mask)
    si, smask = short_batch()
    assert E.packed_rows_bound(torch.from_numpy(smask)) == 1024
    for tag, (i_, m_), kw in (("left-padded", (li, lmask), {}), ("want_hidden", (ids, mask), dict(want_hidden=True)), ("bound 1024", (si, smask), {})):
        want = _hf_reps(lm, i_, m_, "mean")
        for dtype in DTYPES:
            got, call = _encode(lm, i_, m_, "mean", dtype, **kw)
            assert call["packed"] is False and call["rows"] == i_.size, (tag, call)
            _check(got, want, dtype, f"gemma3 {tag}, bound given", (lm, i_, m_, "mean", None, False))
            padded, _ = _encode(lm, i_, m_, "mean", dtype, packed=False)
            assert torch.equal(got, padded), (tag, dtype)
    packed, call = _encode(lm, ids, mask, "mean", "float16")
    assert call["packed"] is True
    monkeypatch.setenv("OM_ENCODER_PACKED", "0")
    off, call = _encode(lm, ids, mask, "mean", "float16")
    assert call == {"rows": ids.size, "packed": False}
    assert torch.equal(off, packed)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_padded_call_after_a_packed_call_keeps_the_padded_bits(dtype):
    """padded, packed, padded through one model and one workspace: nothing the packed call leaves behind (cu, row_map, the cleared ctx
    rows) reaches the next padded call"""
    ids, mask = batch("eg-16x128")
    lm, _ = _lm_of("eg-16x128")
    model = _model(lm, "mean", dtype)
    code = E.compute_dtype_code(model.model_args)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    rows = E.packed_rows_bound(torch.from_numpy(mask))
    with torch.no_grad():
        before = E.hip_encode(model.lm_p, items, "mean", None, False, code, want_hidden=False)[1].clone()
        assert E.LAST_CALL == {"rows": ids.size, "packed": False}
        packed = E.hip_encode(model.lm_p, items, "mean", None, False, code, want_hidden=False, packed_rows=rows)[1].clone()
        assert E.LAST_CALL == {"rows": rows, "packed": True}
        after = E.hip_encode(model.lm_p, items, "mean", None, False, code, want_hidden=False)[1].clone()
        assert E.LAST_CALL == {"rows": ids.size, "packed": False}
    assert torch.isfinite(before).all() and torch.equal(before, after) and torch.equal(before, packed)
    lm.to("cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("pooling", ["mean", "first"])
def test_a_bound_that_is_too_small_poisons_the_batch(pooling):
    ids, mask = batch("tiny-16x128")
    lm, _ = _lm_of("tiny-16x128")
    model = _model(lm, pooling, "float16")
    code = E.compute_dtype_code(model.model_args)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    rows = E.packed_rows_bound(torch.from_numpy(mask))
    assert rows - 256 > 1024 and int(E.token_rows_of(torch.from_numpy(mask)).sum()) > rows - 256
    with torch.no_grad():
        small = E.hip_encode(model.lm_p, items, pooling, None, False, code, want_hidden=False, packed_rows=rows - 256)[1]
        assert E.LAST_CALL == {"rows": rows - 256, "packed": True}
        assert not torch.isfinite(small).any()
        good = E.hip_encode(model.lm_p, items, pooling, None, False, code, want_hidden=False, packed_rows=rows)[1]
        assert E.LAST_CALL == {"rows": rows, "packed": True}
        padded = E.hip_encode(model.lm_p, items, pooling, None, False, code, want_hidden=False)[1]
    assert torch.isfinite(good).all() and torch.equal(good, padded)
    lm.to("cpu")
