"""Qwen3 embedders (HF Qwen3Model: heads of 128 columns, an attention width that is not the hidden size, q / k norms) encoded through
the HIP path (om_causal2_encoder_forward / _packed), against the HF module built at test time in fp32 on the CPU, at the bars of
tests/test_causal_lm.py::_check."""
import numpy as np
import pytest
import torch

from openmatch_amd import encoder as E
from tests.helpers import NS
from tests.test_causal_lm import DEV, _check, _hf_reps, _hip, _left, _model, _ragged, _rel
from tests.test_qwen3_host import EMB06, TINY, _lm3

DTYPES = ("float32", "float16", "bfloat16")


@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(24, 6), (129, 5), (320, 4), (1024, 2)])
def test_encode_matches_hf_tiny(L, n):
    """3 layers at hidden 256, 4 heads of 128 over 2 K / V heads (attention width 512), q / k norm weights perturbed away from 1: `last`
    bare and `mean` + LinearHead + normalize, right- and left-padded, three formats"""
    from openmatch.modeling import LinearHead
    lm = _lm3(seed=L, **({"attention_bias": True} if L == 129 else {}))
    torch.manual_seed(100 + L)
    head = LinearHead(256, 256)
    ids, mask = _ragged(np.random.default_rng(L), n, L, max(2, L // 3))
    for side, (i_, m_) in (("right", (ids, mask)), ("left", _left(ids, mask))):
        for pooling, hd, norm in (("last", None, False), ("mean", head, True)):
            lin = hd.linear if hd is not None else None
            want = _hf_reps(lm, i_, m_, pooling, lin, norm)
            for dtype in DTYPES:
                _check(_hip(lm, i_, m_, pooling, dtype, hd, norm), want, dtype, f"qwen3 tiny L={L} {side} {pooling}", (lm, i_, m_, pooling, lin, norm))


@pytest.mark.gpu
@pytest.mark.parametrize("n_kv", [4, 1])
def test_mha_and_mqa(n_kv):
    lm = _lm3(dict(TINY, num_key_value_heads=n_kv), seed=20 + n_kv, sharp=4.0)
    ids, mask = _ragged(np.random.default_rng(n_kv), 5, 200, 60)
    want = _hf_reps(lm, ids, mask, "last")
    for dtype in DTYPES:
        _check(_hip(lm, ids, mask, "last", dtype), want, dtype, f"qwen3 n_kv={n_kv}", (lm, ids, mask, "last", None, False))


@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(128, 4), (512, 2)])
def test_encode_matches_hf_embedding_06b_width(L, n):
    """Qwen3-Embedding-0.6B width (1024 / 16 heads of 128 / 8 K / V heads / 3072), 2 layers"""
    lm = _lm3(EMB06, layers=2, seed=7 + L)
    ids, mask = _ragged(np.random.default_rng(L + 1), n, L, L // 4)
    want = _hf_reps(lm, ids, mask, "last")
    for dtype in DTYPES:
        _check(_hip(lm, ids, mask, "last", dtype), want, dtype, f"qwen3-0.6B width L={L}", (lm, ids, mask, "last", None, False))


@pytest.mark.gpu
def test_head_dim_64():
    """heads of 64 columns through the new entries: the 64-wide attention kernels behind the q / k norm + rotation pass"""
    lm = _lm3(dict(TINY, head_dim=64), seed=33)
    ids, mask = _ragged(np.random.default_rng(33), 5, 200, 60)
    want = _hf_reps(lm, ids, mask, "last")
    for dtype in DTYPES:
        _check(_hip(lm, ids, mask, "last", dtype), want, dtype, "qwen3 head_dim 64", (lm, ids, mask, "last", None, False))


@pytest.mark.gpu
def test_the_qk_norm_matters():
    """HF with q_norm / k_norm replaced by the identity is more than 5 % away from HF; the HIP result matches the real one"""
    import copy
    lm = _lm3(seed=41, sharp=2.0)
    ids, mask = _ragged(np.random.default_rng(41), 3, 200, 100)
    want = _hf_reps(lm, ids, mask, "mean")
    other = copy.deepcopy(lm)
    for layer in other.layers:
        layer.self_attn.q_norm = torch.nn.Identity()
        layer.self_attn.k_norm = torch.nn.Identity()
    assert _rel(_hf_reps(other, ids, mask, "mean"), want) > 0.05
    got = _hip(lm, ids, mask, "mean", "float32")
    assert _rel(got, want) < 1e-4, _rel(got, want)


@pytest.mark.gpu
def test_causality_bit_for_bit():
    lm = _lm3(seed=31)
    L = 320
    rng = np.random.default_rng(31)
    ids = rng.integers(3, 600, (3, L)).astype(np.int64)
    mask = np.ones_like(ids)
    for dtype in DTYPES:
        h0, r0 = _hip(lm, ids, mask, "last", dtype, hidden=True)
        for t in (1, 127, 128, 300):
            ids2 = ids.copy()
            ids2[:, t + 1:] = rng.integers(3, 600, (3, L - t - 1))
            ids2[:, L - 1] = (ids[:, L - 1] - 3 + 1) % 597 + 3          # the last token certainly changes
            h1, r1 = _hip(lm, ids2, mask, "last", dtype, hidden=True)
            bits = torch.int32 if dtype == "float32" else torch.int16
            assert torch.equal(h0[:, :t + 1].contiguous().view(bits), h1[:, :t + 1].contiguous().view(bits)), (dtype, t)
            assert not torch.equal(h0[:, t + 1:], h1[:, t + 1:])
            assert (r0 - r1).abs().max().item() > 1e-3


def _encode(lm, ids, mask, pooling, dtype, head=None, normalize=False, packed=True):
    """tests/test_causal_packed.py::_encode: encode_passage with (packed) or without the host's token counts; (reps, LAST_CALL)"""
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


PACKED = {"tiny-16x128": (TINY, 3, 16, 128), "tiny-4x1024": (TINY, 3, 4, 1024), "0.6B-16x128": (EMB06, 2, 16, 128)}


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(PACKED))
def test_packed_entry_equals_the_padded_entry(key):
    """ragged right-padded batches of more than 1 024 padded rows: the packed entry's representations carry the padded entry's bits
    in every format, for `last`, `first` and `mean` + LinearHead + normalize; `last` also at the HF bars"""
    from openmatch.modeling import LinearHead
    shape, layers, n, L = PACKED[key]
    lm = _lm3(shape, layers=layers, seed=200 + L)
    torch.manual_seed(300 + L)
    head = LinearHead(shape["hidden_size"], 256)
    ids, mask = _ragged(np.random.default_rng(L + n), n, L, L // 8)
    want_rows = E.packed_rows_bound(torch.from_numpy(mask))
    assert want_rows <= n * L - 256
    for pooling, hd, norm in (("last", None, False), ("mean", head, True), ("first", None, False)):
        lin = hd.linear if hd is not None else None
        want = _hf_reps(lm, ids, mask, pooling, lin, norm) if pooling == "last" else None
        for dtype in DTYPES:
            got, call = _encode(lm, ids, mask, pooling, dtype, hd, norm)
            assert call == {"rows": want_rows, "packed": True}, (call, dtype, pooling)
            if want is not None:
                _check(got, want, dtype, f"qwen3 packed {key} {pooling}", (lm, ids, mask, pooling, lin, norm))
            padded, call = _encode(lm, ids, mask, pooling, dtype, hd, norm, packed=False)
            assert call == {"rows": n * L, "packed": False}
            assert torch.equal(got, padded), (key, pooling, dtype, (got - padded).abs().max().item())


@pytest.mark.gpu
def test_a_bound_that_is_too_small_poisons_the_batch_and_left_padding_stays_padded():
    lm = _lm3(seed=404)
    ids, mask = _ragged(np.random.default_rng(144), 16, 128, 16)
    model = _model(lm, "last", "float16")
    code = E.compute_dtype_code(model.model_args)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    rows = E.packed_rows_bound(torch.from_numpy(mask))
    assert rows - 256 >= 512 and int(E.token_rows_of(torch.from_numpy(mask)).sum()) > rows - 256
    with torch.no_grad():
        small = E.hip_encode(model.lm_p, items, "last", None, False, code, want_hidden=False, packed_rows=rows - 256)[1]
        assert E.LAST_CALL == {"rows": rows - 256, "packed": True}
        assert not torch.isfinite(small).any()
        good = E.hip_encode(model.lm_p, items, "last", None, False, code, want_hidden=False, packed_rows=rows)[1]
        padded = E.hip_encode(model.lm_p, items, "last", None, False, code, want_hidden=False)[1]
    assert torch.isfinite(good).all() and torch.equal(good, padded)
    lm.to("cpu")
    li, lmask = _left(ids, mask)
    got, call = _encode(lm, li, lmask, "last", "float16")
    assert call == {"rows": ids.size, "packed": False}
    _check(got, _hf_reps(lm, li, lmask, "last"), "float16", "qwen3 left-padded, bound given", (lm, li, lmask, "last", None, False))


@pytest.mark.gpu
def test_refusals_on_the_device():
    """Training raises naming the family; 1 025 tokens are refused; the next valid call succeeds."""
    from openmatch.modeling import DRModel
    lm = _lm3(seed=91)
    model = DRModel(lm_q=lm, lm_p=lm, pooling="last", model_args=NS(encoder_only=False, dtype="bfloat16")).to(DEV)
    items = {"input_ids": torch.ones(2, 16, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(2, 16, dtype=torch.int64, device=DEV)}
    model.train()
    with pytest.raises(NotImplementedError, match="Qwen3 training"):
        model.encode_passage(items)
    model.eval()
    long = {"input_ids": torch.ones(1, 1025, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(1, 1025, dtype=torch.int64, device=DEV)}
    with torch.no_grad(), pytest.raises(Exception, match="1024|1 024|length"):
        model.encode_passage(long)
    with torch.no_grad():
        reps = model.encode_passage(items)[1]
    assert reps.shape == (2, 256) and torch.isfinite(reps).all()
