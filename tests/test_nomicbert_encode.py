"""NomicBERT (HF NomicBertModel: nomic-embed-text-v1 / v1.5) encoded through the HIP path -- the post-LayerNorm BERT loops without
biases, Q / K rotated before attention, SwiGLU over one [gate; up] contraction (csrc/encoder.hip, csrc/encoder_plan.h) -- against the
HF module built at test time (random init, norms / biases / embeddings perturbed so that no norm weight is 1, eager attention) in fp32
on the CPU.  Gates: tests/test_causal_lm.py::_check."""
import numpy as np
import pytest
import torch

from openmatch_amd import encoder as E
from tests.helpers import NS
from tests.test_causal_lm import _check, _hip, _left, _model, _pool
from tests.test_modernbert import _ragged, _rel
from tests.test_nomicbert_host import ODD, _nomic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = ("float32", "float16", "bfloat16")
EMBED = dict(hidden_size=768, num_attention_heads=12, intermediate_size=3072)          # nomic-embed-text-v1 / v1.5


def _sharp(lm, k):
    """q / k weights scaled: peaked attention, so that what the rotation does to the scores moves the output far"""
    with torch.no_grad():
        for layer in lm.layers:
            layer.self_attn.q_proj.weight.mul_(k)
            layer.self_attn.k_proj.weight.mul_(k)
    return lm


def _hf_reps(lm, ids, mask, pooling, head=None, normalize=False, tti=None):
    with torch.no_grad():
        h = lm(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask),
               token_type_ids=torch.from_numpy(tti) if tti is not None else None).last_hidden_state
    return _pool(h, mask, pooling, head, normalize)


def _all_formats(lm, ids, mask, pooling, tag, head=None, normalize=False):
    lin = head.linear if head is not None else None
    want = _hf_reps(lm, ids, mask, pooling, lin, normalize)
    for dtype in DTYPES:
        _check(_hip(lm, ids, mask, pooling, dtype, head, normalize), want, dtype, tag, (lm, ids, mask, pooling, lin, normalize))


@pytest.mark.parametrize("n,L", [(1, 16), (5, 24), (16, 128), (8, 320), (2, 1024)])
def test_encode_matches_hf(n, L):
    """hidden 256 / 4 heads / ffn 512 / 3 layers; `first` pooling bare and `mean` pooling with a LinearHead and normalize, on a ragged
    right-padded batch and on the same rows left-padded (positions are columns: HF's arange).  16-bit: 16 rows run the pending-LayerNorm
    loop, 120 the f32-stream few-rows loop, 2 048 and more the fused loop (attention up to 256 keys at 128, chunked beyond); float32
    the plain loop."""
    from openmatch.modeling import LinearHead
    lm = _nomic(seed=L)
    torch.manual_seed(100 + L)
    head = LinearHead(256, 256)
    ids, mask = _ragged(np.random.default_rng(L), n, L, max(2, L // 3))
    for side, (i_, m_) in (("right", (ids, mask)), ("left", _left(ids, mask))):
        for pooling, hd, norm in (("first", None, False), ("mean", head, True)):
            _all_formats(lm, i_, m_, pooling, f"nomic {n}x{L} {side} {pooling}", hd, norm)


def test_unfusable_widths():
    """hidden 192 / 3 heads / ffn 320: no width is a multiple of 256, every format takes the plain loop"""
    lm = _nomic(ODD, seed=5)
    ids, mask = _ragged(np.random.default_rng(5), 16, 128, 30)
    for pooling in ("first", "mean"):
        _all_formats(lm, ids, mask, pooling, f"nomic 192/320 16x128 {pooling}")


class _WithTypes:
    """the module called with fixed token_type_ids: what _check's autocast oracle calls"""
    def __init__(self, lm, tti):
        self.lm, self.tti = lm, torch.from_numpy(tti)

    def to(self, device):
        self.lm.to(device)
        return self

    def __call__(self, input_ids, attention_mask):
        return self.lm(input_ids=input_ids, attention_mask=attention_mask, token_type_ids=self.tti.to(input_ids.device))


def test_token_types():
    """4 x 32 whose second half carries token type 1: HF with the same ids, and not what all-zero ids give"""
    lm = _nomic(seed=6)
    ids, mask = _ragged(np.random.default_rng(6), 4, 32, 12)
    tti = np.zeros_like(ids)
    tti[:, 16:] = 1
    want = _hf_reps(lm, ids, mask, "mean", tti=tti)
    assert _rel(_hf_reps(lm, ids, mask, "mean"), want) > 1e-3
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    for dtype in DTYPES:
        model = _model(lm, "mean", dtype)
        with torch.no_grad():
            got = model.encode_passage(dict(items, token_type_ids=torch.from_numpy(tti).to(DEV)))[1].double().cpu()
            zero = model.encode_passage(items)[1].double().cpu()
        lm.to("cpu")
        _check(got, want, dtype, "nomic token types", (_WithTypes(lm, tti), ids, mask, "mean", None, False))
        assert _rel(zero, got) > 1e-3, _rel(zero, got)


def test_rotation_matters():
    """HF with apply_rotary_pos_emb replaced by the identity is more than 5 % away from real HF; the HIP result is within 1e-4 of real HF"""
    import transformers.models.nomic_bert.modeling_nomic_bert as M
    lm = _sharp(_nomic(seed=7), 8.0)
    ids, mask = _ragged(np.random.default_rng(7), 3, 200, 100)
    want = _hf_reps(lm, ids, mask, "mean")
    orig = M.apply_rotary_pos_emb
    M.apply_rotary_pos_emb = lambda q, k, cos, sin, unsqueeze_dim=1: (q, k)
    try:
        unrotated = _hf_reps(lm, ids, mask, "mean")
    finally:
        M.apply_rotary_pos_emb = orig
    assert torch.equal(_hf_reps(lm, ids, mask, "mean"), want)
    assert _rel(unrotated, want) > 0.05, _rel(unrotated, want)
    got = _hip(lm, ids, mask, "mean", "float32")
    assert _rel(got, want) < 1e-4, _rel(got, want)


@pytest.mark.parametrize("n,L", [(16, 128), (2, 512)])
def test_nomic_embed_width(n, L):
    """768 / 12 heads / 3072 (nomic-embed-text-v1.5), 2 layers, `mean` pooling: 2 048 rows on the fused loop in 16 bits, 1 024 rows on
    the few-rows loop in float16 and (bfloat16 from 512 rows: the two-plane stream) the fused loop"""
    lm = _nomic(EMBED, layers=2, seed=8 + L)
    ids, mask = _ragged(np.random.default_rng(8 + L), n, L, L // 4)
    _all_formats(lm, ids, mask, "mean", f"nomic-embed width {n}x{L}")


def _encode(lm, ids, mask, pooling, dtype, packed=True, want_hidden=False):
    """DRModelForInference.encode_passage on device tensors; packed: with the token counts of the mask as the HOST holds it, from which
    the model computes the row bound.  Returns (reps, LAST_CALL)."""
    model = _model(lm, pooling, dtype)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    if packed:
        items[E.TOKEN_ROWS_KEY] = E.token_rows_of(torch.from_numpy(mask))
    with torch.no_grad():
        hidden, r = model.encode_passage(items, want_hidden=want_hidden)
    assert (hidden is not None) == want_hidden
    call = dict(E.LAST_CALL)
    lm.to("cpu")
    return r.double().cpu(), call


def _packed_batch():
    ids, mask = _ragged(np.random.default_rng(9), 16, 128, 20)
    rows = E.packed_rows_bound(torch.from_numpy(mask))
    assert int(mask.sum()) <= 16 * 128 - 256 and 512 <= rows <= 16 * 128 - 256
    return ids, mask, rows


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_packed_rows(dtype, monkeypatch):
    """A ragged right-padded 16 x 128 batch runs over its packed rows: HF at the bars of _check, and the bits of the padded entry"""
    lm = _nomic(seed=9)
    ids, mask, rows = _packed_batch()
    for pooling in ("first", "mean"):
        want = _hf_reps(lm, ids, mask, pooling)
        got, call = _encode(lm, ids, mask, pooling, dtype)
        assert call == {"rows": rows, "packed": True}, call
        _check(got, want, dtype, f"nomic packed 16x128 {pooling}", (lm, ids, mask, pooling, None, False))
        monkeypatch.setenv("OM_ENCODER_PACKED", "0")
        padded, call = _encode(lm, ids, mask, pooling, dtype)
        monkeypatch.delenv("OM_ENCODER_PACKED")
        assert call == {"rows": 16 * 128, "packed": False}, call
        assert torch.equal(got, padded), (pooling, (got - padded).abs().max().item())


def test_packed_rows_bound_too_small_and_what_stays_padded():
    lm = _nomic(seed=10)
    ids, mask, rows = _packed_batch()
    assert rows - 256 >= 512 and int(E.token_rows_of(torch.from_numpy(mask)).sum()) > rows - 256
    model = _model(lm, "mean", "float16")
    code = E.compute_dtype_code(model.model_args)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    with torch.no_grad():
        small = E.hip_encode(model.lm_p, items, "mean", None, False, code, want_hidden=False, packed_rows=rows - 256)[1]
        assert E.LAST_CALL == {"rows": rows - 256, "packed": True}
        assert not torch.isfinite(small).any()
        good = E.hip_encode(model.lm_p, items, "mean", None, False, code, want_hidden=False, packed_rows=rows)[1]
        assert E.LAST_CALL == {"rows": rows, "packed": True}
        padded = E.hip_encode(model.lm_p, items, "mean", None, False, code, want_hidden=False)[1]
    assert torch.isfinite(good).all() and torch.equal(good, padded)
    lm.to("cpu")
    _, call = _encode(lm, ids, mask, "mean", "float32")
    assert call == {"rows": 16 * 128, "packed": False}, call
    _, call = _encode(lm, ids, mask, "mean", "float16", want_hidden=True)
    assert call == {"rows": 16 * 128, "packed": False}, call


def test_cross_encoder():
    """RRModel: pooling "first" and a 1-logit head over 6 pairs of 40 tokens, the second segment with token type 1"""
    from openmatch.modeling import LinearHead, RRModel
    lm = _nomic(seed=11)
    torch.manual_seed(12)
    head = LinearHead(256, 1)
    ids, mask = _ragged(np.random.default_rng(11), 6, 40, 25)
    tti = np.zeros_like(ids)
    tti[:, 12:] = 1
    want = _hf_reps(lm, ids, mask, "first", head.linear, tti=tti)
    model = RRModel(lm=lm, head=head, pooling="first", model_args=NS(encoder_only=False, dtype="float32")).to(DEV).eval()
    with torch.no_grad():
        got = model.encode({"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV),
                            "token_type_ids": torch.from_numpy(tti).to(DEV)})
    assert got.shape == (6, 1)
    assert (got.double().cpu() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


def test_refusals_on_the_device():
    """Training raises naming the family; 1 025 tokens are refused; the next valid call succeeds."""
    from openmatch.modeling import DRModel
    lm = _nomic(seed=13)
    model = DRModel(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=False, dtype="bfloat16")).to(DEV)
    items = {"input_ids": torch.ones(2, 16, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(2, 16, dtype=torch.int64, device=DEV)}
    model.train()
    with pytest.raises(NotImplementedError, match="NomicBERT training"):
        model.encode_passage(items)
    model.eval()
    long = {"input_ids": torch.ones(1, 1025, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(1, 1025, dtype=torch.int64, device=DEV)}
    with torch.no_grad(), pytest.raises(Exception, match="1024|1 024|length"):
        model.encode_passage(long)
    with torch.no_grad():
        reps = model.encode_passage(items)[1]
    assert reps.shape == (2, 256) and torch.isfinite(reps).all()
