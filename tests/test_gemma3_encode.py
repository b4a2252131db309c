"""EmbeddingGemma encoded through the HIP path (csrc/encoder_gemma3.hip, csrc/attention_d256.hip): a bidirectional HF Gemma3TextModel
built at test time (random weights, perturbed norm weights and embeddings, eager attention) in fp32 on the CPU is the reference,
through DRModelForInference.encode_passage -- the tiny model [sliding, sliding, full] with a window of 8 -> 4 and EmbeddingGemma's
width (768 / 3 heads over 1 K / V head of 256 columns / 1152) with a window of 512 -> 256."""
import copy

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.helpers import NS
from tests.test_causal_lm import DEV, _check, _hf_reps, _hip, _left
from tests.test_gemma3_host import TINY, TYPES3, gemma_lm
from tests.test_modernbert import _ragged, _rel

EG = dict(hidden_size=768, num_attention_heads=3, num_key_value_heads=1, head_dim=256, intermediate_size=1152)
EG_TYPES = ["sliding_attention", "full_attention", "sliding_attention"]
DTYPES = ("float32", "float16", "bfloat16")


def _cases(lm, hidden, L, n, seed, tag):
    """ragged right- and left-padded batches; `mean` with a LinearHead and normalize and bare, `first` bare (right-padded: under left
    padding position 0 is a pad token, whose hidden state no contract describes)"""
    from openmatch.modeling import LinearHead
    torch.manual_seed(100 + L)
    head = LinearHead(hidden, hidden)
    ids, mask = _ragged(np.random.default_rng(seed), n, L, max(2, L // 3))
    for side, (i_, m_) in (("right", (ids, mask)), ("left", _left(ids, mask))):
        modes = [("mean", head, True), ("mean", None, False)] + ([("first", None, False), ("first", head, True)] if side == "right" else [])
        for pooling, hd, norm in modes:
            lin = hd.linear if hd is not None else None
            want = _hf_reps(lm, i_, m_, pooling, lin, norm)
            for dtype in DTYPES:
                _check(_hip(lm, i_, m_, pooling, dtype, hd, norm), want, dtype, f"{tag} L={L} {side} {pooling}{' head norm' if hd else ''}",
                       (lm, i_, m_, pooling, lin, norm))


@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(8, 6), (128, 5), (640, 3)])
def test_encode_matches_hf_tiny(L, n):
    """hidden 128, 2 heads over 1 K / V head, ffn 192, [sliding, sliding, full], window 8 -> 4: the band cuts at every length"""
    _cases(gemma_lm(TINY, TYPES3, 8, seed=L), 128, L, n, L, "gemma3 tiny")


@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(8, 6), (128, 4), (640, 3)])
def test_encode_matches_hf_embeddinggemma_width(L, n):
    """768 / 3 / 1 / 256 / 1152, [sliding, full, sliding], window 512 -> 256: 640 tokens exercise the band at the real width"""
    _cases(gemma_lm(EG, EG_TYPES, 512, seed=7 + L), 768, L, n, L + 1, "gemma3 768")


@pytest.mark.gpu
def test_hidden_states_match_hf():
    lm = gemma_lm(TINY, TYPES3, 8, seed=3)
    ids, mask = _ragged(np.random.default_rng(3), 4, 96, 30)
    with torch.no_grad():
        want = lm(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state.double()
    h, _ = _hip(lm, ids, mask, "mean", "float32", hidden=True)
    m = torch.from_numpy(mask).bool()
    assert ((h.double() - want)[m].abs().max() / want[m].abs().max()).item() < 1e-4


@pytest.mark.gpu
def test_the_window_matters():
    """The same weights with the window widened past the sequence differ by more than 0.1 relative at 640 tokens; the HIP path follows
    each model's own window"""
    lm = gemma_lm(EG, EG_TYPES, 512, seed=21)
    wide = copy.deepcopy(lm)                        # (never through to_dict(): the constructor would halve the window again)
    wide.config.sliding_window = 2048
    for layer in wide.layers:
        if hasattr(layer.self_attn, "sliding_window") and layer.self_attn.sliding_window is not None:
            layer.self_attn.sliding_window = 2048
    ids, mask = _ragged(np.random.default_rng(21), 2, 640, 600)
    want, other = _hf_reps(lm, ids, mask, "mean"), _hf_reps(wide, ids, mask, "mean")
    assert _rel(other, want) > 0.1, _rel(other, want)
    for dtype in DTYPES:
        _check(_hip(lm, ids, mask, "mean", dtype), want, dtype, "gemma3 window 256", (lm, ids, mask, "mean", None, False))
    assert _rel(_hip(wide, ids, mask, "mean", "float32"), other) < 1e-4


@pytest.mark.gpu
def test_one_plus_w_matters():
    """Norm weights taken as g = w instead of 1 + w, or dropped (g = 1), are far from the model"""
    lm = gemma_lm(TINY, TYPES3, 8, seed=31)
    ids, mask = _ragged(np.random.default_rng(31), 4, 64, 20)
    want = _hf_reps(lm, ids, mask, "mean")
    plain = copy.deepcopy(lm)
    minus = copy.deepcopy(lm)
    with torch.no_grad():
        for name, p in plain.named_parameters():
            if "norm" in name:
                p.zero_()                            # g = 1
        for name, p in minus.named_parameters():
            if "norm" in name:
                p.sub_(1.0)                          # g = w
    assert _rel(_hf_reps(plain, ids, mask, "mean"), want) > 0.1 and _rel(_hf_reps(minus, ids, mask, "mean"), want) > 0.1
    assert _rel(_hip(lm, ids, mask, "mean", "float32"), want) < 1e-4


@pytest.mark.gpu
def test_query_pre_attn_scalar_is_honoured():
    """query_pre_attn_scalar 64 at head_dim 256: a score scale of 1 / 8, twice head_dim ** -0.5 (scores of standard deviation about 2)"""
    lm = gemma_lm(TINY, TYPES3, 8, seed=41, query_pre_attn_scalar=64)
    same = gemma_lm(TINY, TYPES3, 8, seed=41, query_pre_attn_scalar=256)
    same.load_state_dict(lm.state_dict())
    ids, mask = _ragged(np.random.default_rng(41), 4, 200, 100)
    want = _hf_reps(lm, ids, mask, "mean")
    assert _rel(_hf_reps(same, ids, mask, "mean"), want) > 0.05
    for dtype in DTYPES:
        _check(_hip(lm, ids, mask, "mean", dtype), want, dtype, "gemma3 query_pre_attn_scalar 64", (lm, ids, mask, "mean", None, False))


@pytest.mark.gpu
def test_refusals_on_the_device():
    """Training raises naming the family; 1 025 tokens and `last` pooling are refused; the next valid call succeeds."""
    from openmatch.modeling import DRModel
    lm = gemma_lm(TINY, TYPES3, 8, seed=51)
    model = DRModel(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=False, dtype="bfloat16")).to(DEV)
    items = {"input_ids": torch.ones(2, 16, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(2, 16, dtype=torch.int64, device=DEV)}
    model.train()
    with pytest.raises(NotImplementedError, match="Gemma3 training"):
        model.encode_passage(items)
    model.eval()
    long = {"input_ids": torch.ones(1, 1025, dtype=torch.int64, device=DEV), "attention_mask": torch.ones(1, 1025, dtype=torch.int64, device=DEV)}
    with torch.no_grad(), pytest.raises(N.NativeError, match="1024"):
        model.encode_passage(long)
    last = DRModel(lm_q=lm, lm_p=lm, pooling="last", model_args=NS(encoder_only=False, dtype="bfloat16")).to(DEV).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="pooling='last'"):
        last.encode_passage(items)
    with torch.no_grad():
        reps = model.encode_passage(items)[1]
    assert reps.shape == (2, 128) and torch.isfinite(reps).all()
