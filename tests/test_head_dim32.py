"""Head dimension 32 (attention_d32.hip): MiniLM-shaped BERT encoders -- all-MiniLM-L6-v2, e5-small-v2, bge-small-en-v1.5,
gte-small, the MS MARCO MiniLM cross-encoders: hidden 384, 12 heads of 32 -- encoded and trained through the HIP path, against the
HF module in fp32 on the CPU.  The 64-wide kernels are covered by the other test files and do not change."""
import ctypes as C

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.helpers import NS, synth_tokens

DEV = "cuda:0"
MINILM = dict(hidden_size=384, num_attention_heads=12, intermediate_size=1536)
SMALL = dict(hidden_size=256, num_attention_heads=8, intermediate_size=1024)


def _perturb(lm):
    """Trained-checkpoint-like LayerNorm affines and biases, not the 1 / 0 of an init."""
    with torch.no_grad():
        for name, p in lm.named_parameters():
            if "LayerNorm.weight" in name:
                p.copy_(1.0 + 0.3 * torch.randn_like(p))
            elif "bias" in name:
                p.copy_(0.1 * torch.randn_like(p))
    return lm


def _bert(shape, layers, max_pos, **kw):
    from transformers import BertConfig, BertModel
    return _perturb(BertModel(BertConfig(num_hidden_layers=layers, vocab_size=600, max_position_embeddings=max_pos, **shape, **kw)).eval())


def _ragged(rng, n, L, lo_len):
    ids, mask = synth_tokens(rng, n, L, vocab=600, lo_len=lo_len, lo_id=300)
    ids[0, :], mask[0, :] = rng.integers(300, 600, L), 1            # one full-length row
    return ids, mask


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a, b, dim=1).min().item()


# ------------------------------------------------------------------------------------------------------------- CPU
def test_train_packed_supported_accepts_32_wide_heads():
    """om_encoder_train_packed_supported (host-only): 8 heads of 32 at hidden 256 take the packed training entry; 16 heads of 48
    at hidden 768 are refused, where the head width is the only reason."""
    lib = N.lib()
    cfg = N.OmEncoderConfig(arch=N.ARCH_BERT, dtype=N.OM_BF16, hidden=256, n_layers=2, n_heads=8, head_dim=32, ffn=1024, vocab=600,
                            max_pos=512, type_vocab=2, act=N.ACT_GELU_ERF, ln_eps=1e-12, pooling=N.POOL_MEAN)
    assert lib.om_encoder_train_packed_supported(C.byref(cfg), 8, 128, 768) == 1
    wide = N.OmEncoderConfig(arch=N.ARCH_BERT, dtype=N.OM_BF16, hidden=768, n_layers=2, n_heads=16, head_dim=48, ffn=3072, vocab=600,
                             max_pos=512, type_vocab=2, act=N.ACT_GELU_ERF, ln_eps=1e-12, pooling=N.POOL_MEAN)
    assert lib.om_encoder_train_packed_supported(C.byref(wide), 8, 128, 768) == 0
    wide.n_heads, wide.head_dim = 12, 64                             # the same shape with 64-wide heads: accepted
    assert lib.om_encoder_train_packed_supported(C.byref(wide), 8, 128, 768) == 1


# ------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("L,n", [(24, 8), (128, 6), (200, 5), (256, 4), (384, 3), (1024, 2)])
def test_minilm_encode_matches_hf(L, n):
    """MiniLM shape (384 / 12 heads / 1536, 3 layers), mean pooling + normalise, ragged batches: f32 within 1e-4 of HF fp32; float16
    against the f32 HIP path at the bars of test_f16_fused_path_tracks_f32_path_across_lengths, and closer than bfloat16.  From 257
    tokens on the attention walks its keys in chunks with the online softmax."""
    from openmatch.modeling import DRModelForInference
    torch.manual_seed(3 + L)
    lm = _bert(MINILM, 3, 1024)
    rng = np.random.default_rng(L)
    ids, mask = _ragged(rng, n, L, max(2, L // 3))
    with torch.no_grad():
        h = lm(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state
        m = torch.from_numpy(mask).unsqueeze(-1).float()
        want = torch.nn.functional.normalize((h * m).sum(1) / m.sum(1), dim=1).double()
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    outs = {}
    for dtype in ("float32", "float16", "bfloat16"):
        model = DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", normalize=True,
                                    model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()
        outs[dtype] = model.encode_passage(items)[1].double().cpu()
    err = (outs["float32"] - want).abs().max().item()
    ref = outs["float32"]
    cos16, cosb = _cos(outs["float16"], ref), _cos(outs["bfloat16"], ref)
    rel16 = ((outs["float16"] - ref).abs().max() / ref.abs().max()).item()
    print(f"\n[head_dim 32, L={L}] f32 vs HF max|err| {err:.2e}; f16 vs f32: 1 - cos {1 - cos16:.2e}, max rel {rel16:.2e} (bf16 1 - cos {1 - cosb:.2e})")
    assert err < 1e-4, err
    assert 1 - cos16 < 5e-6 and rel16 < 5e-3, (cos16, rel16)
    assert (1 - cos16) < 0.25 * (1 - cosb) + 1e-7, (cos16, cosb)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [128, 384])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_packed_rows_are_bit_identical_to_padded(dtype, L):
    """hidden 256 with 8 heads of 32 takes the packed-rows entry: same bits as the padded entry (ragged lengths, a full row, a mask
    with holes, an empty row)."""
    from openmatch.modeling import DRModelForInference
    from openmatch_amd import encoder as enc_mod
    from openmatch_amd.encoder import compute_dtype_code, hip_encode, packed_rows_bound
    torch.manual_seed(5)
    lm = _bert(SMALL, 2, 640)
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()
    code = compute_dtype_code(model.model_args)
    rng = np.random.default_rng(L)
    B = 24 if L == 128 else 12
    ids, mask = _ragged(rng, B, L, 5)
    mask[1, :] = 0; mask[1, ::3] = 1
    mask[2, :] = 0
    m = torch.from_numpy(mask)
    rows = packed_rows_bound(m)
    assert rows is not None and rows < B * L
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": m.to(DEV)}
    padded = hip_encode(model.lm_p, items, "mean", None, False, code, want_hidden=False)[1]
    assert enc_mod.LAST_CALL == {"rows": B * L, "packed": False}
    packed = hip_encode(model.lm_p, items, "mean", None, False, code, want_hidden=False, packed_rows=rows)[1]
    assert enc_mod.LAST_CALL["packed"] is True and enc_mod.LAST_CALL["rows"] == rows
    keep = torch.ones(B, dtype=torch.bool); keep[2] = False           # (the empty row: a softmax over no keys)
    assert torch.isfinite(padded[keep]).all()
    assert torch.equal(packed[keep], padded[keep]), (L, (packed[keep] - padded[keep]).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_few_rows_track_f32_and_are_batch_invariant(dtype):
    """A served 32-token query and a batch of 8 at the MiniLM shape (the weight-streaming few-rows path): both track the f32 path,
    and the query's row is the same bits alone and inside the batch."""
    from openmatch.modeling import DRModelForInference
    torch.manual_seed(11)
    lm = _bert(MINILM, 3, 512)
    mk = lambda dt: DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=False, dtype=dt)).to(DEV).eval()
    m16, m32 = mk(dtype), mk("float32")
    rng = np.random.default_rng(2)
    tol = 5e-6 if dtype == "float16" else 2e-4
    ids, mask = _ragged(rng, 8, 32, 8)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    alone_items = {k: v[:1] for k, v in items.items()}
    batch = m16.encode_passage(items)[1]
    alone = m16.encode_passage(alone_items)[1]
    c_batch = 1 - _cos(batch.double().cpu(), m32.encode_passage(items)[1].double().cpu())
    c_alone = 1 - _cos(alone.double().cpu(), m32.encode_passage(alone_items)[1].double().cpu())
    print(f"\n[head_dim 32 few rows, {dtype}] 1 - cos vs f32: query {c_alone:.2e}, batch of 8 {c_batch:.2e}")
    assert c_batch < tol and c_alone < tol, (c_batch, c_alone)
    assert torch.equal(alone[0], batch[0])


@pytest.mark.gpu
def test_minilm_cross_encoder_matches_hf():
    """RRModel over the MiniLM shape with LinearHead(384, 1): 162-token pairs with token types 0 / 1.  f32 scores within 1e-4 of HF
    fp32; float16 scores track them."""
    from openmatch.modeling import LinearHead, RRModel
    torch.manual_seed(21)
    lm = _bert(MINILM, 3, 512)
    head = LinearHead(384, 1)
    rng = np.random.default_rng(9)
    n = 16
    ids, mask = _ragged(rng, n, 162, 20)
    tt = np.zeros_like(ids)
    for i in range(n):
        ln = int(mask[i].sum()); tt[i, ln // 3:ln] = 1
    items = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask), "token_type_ids": torch.from_numpy(tt)}
    with torch.no_grad():
        cls = lm(**items).last_hidden_state[:, 0]
        want = (cls @ head.linear.weight.detach().t()).double()
    got = {}
    for dtype in ("float32", "float16"):
        model = RRModel(lm=lm, head=head, pooling="first", model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()
        with torch.no_grad():
            got[dtype] = model.encode({k: v.to(DEV) for k, v in items.items()}).double().cpu()
        assert got[dtype].shape == (n, 1)
    scale = max(1.0, want.abs().max().item())
    err32 = (got["float32"] - want).abs().max().item()
    err16 = (got["float16"] - got["float32"]).abs().max().item()
    print(f"\n[head_dim 32 cross-encoder] f32 vs HF max|err| {err32:.2e}; f16 vs f32 {err16:.2e} (scores up to {want.abs().max().item():.2f})")
    assert err32 < 1e-4 * scale, err32
    assert err16 < 1e-2 * scale, err16


@pytest.mark.gpu
@pytest.mark.parametrize("L", [64, 200, 256])
@pytest.mark.parametrize("shape", ["minilm", "small"])
def test_training_step_matches_torch_autograd(shape, L, monkeypatch):
    """Loss and every parameter gradient of a contrastive step (no dropout) against torch autograd through the HF module in fp32 on
    the CPU, ragged right-padded batches.  f32 as tight as test_training_step_f32_matches_reference_gradients (float32 trains to
    256 tokens with 32-wide heads); float16 (loss-scaled) and bfloat16 at the bars of the other 16-bit training tests."""
    monkeypatch.delenv("OM_TRAIN_F16", raising=False)
    from openmatch.modeling import DRModel
    from oracle import retrieval_ref
    torch.manual_seed(29 + L)
    sh = MINILM if shape == "minilm" else SMALL
    lm = _bert(sh, 2, 256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    ref_lm = _bert(sh, 2, 256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    ref_lm.load_state_dict(lm.state_dict())
    rng = np.random.default_rng(L + 1)
    p_ids, p_mask = _ragged(rng, 6, L, L // 2)
    q_ids, q_mask = synth_tokens(rng, 2, L, vocab=600, lo_len=5, lo_id=300)
    common = dict(data_args=NS(train_n_passages=3), train_args=NS(negatives_x_device=False, per_device_train_batch_size=2))

    def ref_mean(ids, mask):
        ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
        h_ = ref_lm(input_ids=ids, attention_mask=mask).last_hidden_state
        m_ = mask.unsqueeze(-1).float()
        return (h_ * m_).sum(1) / m_.sum(1).clamp(min=1e-9)
    ref_lm.train()
    loss_ref, _ = retrieval_ref.contrastive_loss(ref_mean(q_ids, q_mask), ref_mean(p_ids, p_mask), 3)
    loss_ref.backward()
    gref = {n: t.grad.detach().clone() for n, t in ref_lm.named_parameters() if t.grad is not None}
    tens = lambda a: torch.from_numpy(a).to(DEV)
    for dtype in ("float32", "float16", "bfloat16"):
        model = DRModel(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=False, dtype=dtype), **common).to(DEV).train()
        model.zero_grad(set_to_none=True)
        out = model(query={"input_ids": tens(q_ids), "attention_mask": tens(q_mask)}, passage={"input_ids": tens(p_ids), "attention_mask": tens(p_mask)})
        lscale = 4096.0 if dtype == "float16" else 1.0
        (out.loss * lscale).backward()
        worst = ("", 0.0, 0.0)
        for n, t in lm.named_parameters():
            if n not in gref:
                continue
            got, ref = t.grad.detach().float().cpu() / lscale, gref[n]
            rel = ((got - ref).norm() / (ref.norm() + 1e-12)).item()
            amax = (got - ref).abs().max().item()
            if dtype == "float32":
                # (the golden test's absolute bar, 2e-5, scaled to the tensor: here the embedding gradients sum over ~1 500 tokens)
                assert (rel < 1e-3 or amax < 1e-7) and amax < 5e-5 * max(1.0, ref.norm().item()), (shape, L, n, rel, amax)
            elif ref.norm() < 1e-9 or n.endswith("attention.self.key.bias"):
                continue
            if amax >= 1e-7 and rel > worst[1]:
                worst = (n, rel, amax)
        dl = abs(out.loss.item() - loss_ref.item())
        print(f"\n[head_dim 32 training, {shape}, L={L}, {dtype}] loss {out.loss.item():.6f} vs torch fp32 {loss_ref.item():.6f}; worst gradient rel-L2 {worst[1]:.2e} ({worst[0]})")
        if dtype == "float32":
            # (the scores are dot products of unnormalised 384-wide means behind perturbed LayerNorms: f32 rounding of those alone moves
            # a loss of ~2 by ~1e-5, so the golden test's 1e-5 is taken relative to the loss; measured <= 8.1e-6)
            assert dl < 2e-5 * max(1.0, abs(loss_ref.item())), dl
        else:
            assert dl < (2e-3 if dtype == "float16" else 2e-2) * max(1.0, abs(loss_ref.item())), dl
            assert worst[1] < (3e-2 if dtype == "float16" else 8e-2), worst
        for t in lm.parameters():
            t.grad = None


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_packed_training_equals_padded_under_dropout(dtype):
    """Dropout 0.1 at both sites, hidden 256 with 8 heads of 32, L = 128: the packed-rows training step draws the same attention
    masks as the padded one (keyed on the token's padded coordinates) -- the same representations bit for bit, the same gradients up
    to the summation order of the weight gradients."""
    from openmatch_amd import train as T
    from openmatch_amd.encoder import compute_dtype_code, rows_bound_of, token_rows_of
    torch.manual_seed(41)
    lm = _bert(SMALL, 2, 256, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1).to(DEV).train()
    rng = np.random.default_rng(6)
    B, L = 24, 128
    ids, mask = _ragged(rng, B, L, 3)
    mask[1, :] = 0; mask[1, ::3] = 1
    ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
    rows = rows_bound_of(token_rows_of(mask))
    assert rows is not None and rows < B * L
    items = {"input_ids": ids.to(DEV), "attention_mask": mask.to(DEV)}
    code = compute_dtype_code(NS(dtype=dtype))
    wgt = torch.randn(B, 256, generator=torch.Generator().manual_seed(2)).to(DEV)

    def step(packed_rows):
        lm.zero_grad(set_to_none=True)
        torch.manual_seed(1234)
        reps = T.encode_train(lm, None, items, "mean", False, code, True, packed_rows=packed_rows)[1]
        (reps * wgt).sum().backward()
        return reps.detach().clone(), {n: p.grad.detach().clone() for n, p in lm.named_parameters() if p.grad is not None}

    reps0, g0 = step(None)
    assert T.LAST_CALL == {"rows": B * L, "packed": False}
    reps1, g1 = step(rows)
    assert T.LAST_CALL == {"rows": rows, "packed": True}
    assert torch.isfinite(reps1).all() and all(torch.isfinite(v).all() for v in g1.values())
    err = (reps1 - reps0).abs().max().item() / reps0.abs().max().item()
    worst = ("", 0.0)
    for n in g0:
        if "key.bias" in n:          # (the true gradient is zero: rounding noise only)
            continue
        a, b = g0[n].float(), g1[n].float()
        rel = ((a - b).norm() / a.norm().clamp_min(1e-12)).item()
        if a.norm().item() > 1e-6 and rel > worst[1]:
            worst = (n, rel)
    print(f"\n[head_dim 32 packed training, {dtype}, dropout 0.1] {rows} of {B * L} rows; reps max rel err vs padded {err:.2e}; "
          f"worst gradient rel-L2 {worst[1]:.2e} ({worst[0]})")
    assert torch.equal(reps1, reps0), err
    assert worst[1] < 1e-6, worst          # (the order of the weight gradients' f32 atomic sums: measured 3.6e-7)


@pytest.mark.gpu
def test_refusals_name_the_limit():
    """16-bit training beyond 256 tokens with 32-wide heads, a BERT with 48-wide heads and a T5 encoder with d_kv 32 are refused
    with a message that says why."""
    from transformers import BertConfig, BertModel, T5Config, T5EncoderModel
    from openmatch.modeling import DRModel, DRModelForInference
    torch.manual_seed(1)
    rng = np.random.default_rng(1)
    L = 320
    lm = _bert(SMALL, 1, 512, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    p_ids, p_mask = _ragged(rng, 6, L, 100)
    q_ids, q_mask = synth_tokens(rng, 2, L, vocab=600, lo_len=5, lo_id=300)
    tens = lambda a: torch.from_numpy(a).to(DEV)
    model = DRModel(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=False, dtype="float16"),
                    data_args=NS(train_n_passages=3), train_args=NS(negatives_x_device=False, per_device_train_batch_size=2)).to(DEV).train()
    with pytest.raises(N.NativeError, match="head_dim 32 supports sequence lengths up to 256"):
        model(query={"input_ids": tens(q_ids), "attention_mask": tens(q_mask)}, passage={"input_ids": tens(p_ids), "attention_mask": tens(p_mask)})
    ids, mask = _ragged(rng, 2, 64, 10)
    items = {"input_ids": tens(ids), "attention_mask": tens(mask)}
    wide = BertModel(BertConfig(hidden_size=768, num_hidden_layers=1, num_attention_heads=16, intermediate_size=1024, vocab_size=600,
                                max_position_embeddings=128)).eval()
    inf = DRModelForInference(lm_q=wide, lm_p=wide, pooling="mean", model_args=NS(encoder_only=False, dtype="float32")).to(DEV).eval()
    with pytest.raises(N.NativeError, match="head_dim must be 32 or 64"):
        inf.encode_passage(items)
    t5 = T5EncoderModel(T5Config(d_model=256, d_ff=512, num_layers=1, num_heads=8, d_kv=32, vocab_size=600, feed_forward_proj="relu")).eval()
    inf = DRModelForInference(lm_q=t5, lm_p=t5, pooling="mean", model_args=NS(encoder_only=True, dtype="float32")).to(DEV).eval()
    with pytest.raises(N.NativeError, match="d_kv 64"):
        inf.encode_passage(items)
