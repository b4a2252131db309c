"""DistilBERT (DistilBertModel) and MPNet (MPNetModel) through the HIP path: the BERT post-LayerNorm stack without a token-type
table, and for MPNet with RoBERTa position numbering and one relative-position bias table shared by all layers
(openmatch_amd/flavours.py, csrc/encoder.hip, csrc/train.hip, csrc/attention_d32.hip).  The HF module is built at test time (seeded
random init; norms, biases, embeddings and the relative-bias table perturbed -- the table at N(0, 1): at HF's N(0, 0.02) it moves
nothing) and evaluated in fp32 on the CPU.

HF's MPNetEncoder.forward calls compute_position_bias with its default num_buckets = 32 whatever the config says; the HIP encoder
follows config.relative_attention_num_buckets (equal for every published checkpoint).  `_mpnet` makes the HF module follow the
config too, so that a 16-bucket configuration can be compared at all (HF as it stands indexes a 16-row table with 32 buckets)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

from openmatch_amd import native as N
from tests.helpers import NS

DEV = "cuda:0"
SMALL = dict(hidden=256, heads=4, ffn=1024)
BASE = dict(hidden=768, heads=12, ffn=3072)
D32 = dict(hidden=128, heads=4, ffn=512)               # 32-wide heads
PAD = 1                                                 # MPNet / RoBERTa pad id
COS_BAR = {"float16": 5e-6, "bfloat16": 2e-4}          # tests/test_head_dim32.py, tests/test_modernbert.py: the same formats' bars
F32_BAR = 1e-4


def _perturb(lm, table_std=1.0):
    with torch.no_grad():
        for name, p in lm.named_parameters():
            if "relative_attention_bias" in name:
                p.copy_(table_std * torch.randn_like(p))
            elif ("LayerNorm" in name or "layer_norm" in name) and name.endswith("weight"):
                p.copy_(1.0 + 0.3 * torch.randn_like(p))
            elif name.endswith("bias"):
                p.copy_(0.1 * torch.randn_like(p))
            elif "embeddings" in name:
                p.add_(0.02 * torch.randn_like(p))
    return lm


def _distil(shape=SMALL, layers=3, seed=0, max_pos=512, **kw):
    from transformers import DistilBertConfig, DistilBertModel
    torch.manual_seed(seed)
    kw.setdefault("dropout", 0.0); kw.setdefault("attention_dropout", 0.0)
    cfg = DistilBertConfig(dim=shape["hidden"], n_heads=shape["heads"], hidden_dim=shape["ffn"], n_layers=layers, vocab_size=600,
                           max_position_embeddings=max_pos, pad_token_id=0, attn_implementation="eager", **kw)
    return _perturb(DistilBertModel(cfg).eval())


def _mpnet(shape=SMALL, layers=3, seed=0, max_pos=516, sharp=1.0, buckets=32, **kw):
    """sharp > 1 scales the q / k weights: peaked attention, so that the position bias moves the output far"""
    from transformers import MPNetConfig, MPNetModel
    torch.manual_seed(seed)
    kw.setdefault("hidden_dropout_prob", 0.0); kw.setdefault("attention_probs_dropout_prob", 0.0)
    cfg = MPNetConfig(hidden_size=shape["hidden"], num_attention_heads=shape["heads"], intermediate_size=shape["ffn"],
                      num_hidden_layers=layers, vocab_size=600, max_position_embeddings=max_pos, pad_token_id=PAD,
                      relative_attention_num_buckets=buckets, layer_norm_eps=1e-5, **kw)
    lm = _perturb(MPNetModel(cfg).eval())
    lm.encoder.compute_position_bias = functools.partial(lm.encoder.compute_position_bias, num_buckets=buckets)    # (module docstring)
    if sharp != 1.0:
        with torch.no_grad():
            for layer in lm.encoder.layer:
                layer.attention.attn.q.weight.mul_(sharp)
                layer.attention.attn.k.weight.mul_(sharp)
    return lm


def _make(kind, *a, **kw):
    return _distil(*a, **kw) if kind == "distilbert" else _mpnet(*a, **kw)


def _ragged(rng, n, L, lo_len, pad=0):
    ids = np.full((n, L), pad, np.int64)
    mask = np.zeros((n, L), np.int64)
    for i in range(n):
        ln = L if i == 0 else int(rng.integers(min(lo_len, L), L + 1))        # one full-length row
        ids[i, :ln] = rng.integers(3, 600, ln)
        mask[i, :ln] = 1
    return ids, mask


def _pad_of(kind):
    return PAD if kind == "mpnet" else 0


def _hf_reps(lm, ids, mask, pooling, head=None, normalize=False):
    with torch.no_grad():
        h = lm(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).last_hidden_state
        if pooling == "first":
            r = h[:, 0]
        else:
            m = torch.from_numpy(mask).unsqueeze(-1).float()
            r = (h * m).sum(1) / m.sum(1)
        if head is not None:
            r = r @ head.linear.weight.detach().cpu().t()        # (LinearHead.forward itself is a device op)
        if normalize:
            r = torch.nn.functional.normalize(r, dim=1)
    return r.double()


def _hip_reps(lm, ids, mask, pooling, dtype, head=None, normalize=False, packed=False):
    """Through DRModelForInference.encode_passage (the padded entry); packed: hip_encode over the packed-rows bound of the mask."""
    from openmatch.modeling import DRModelForInference
    from openmatch_amd import encoder as E
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling=pooling, normalize=normalize, head_q=head, head_p=head,
                                model_args=NS(encoder_only=False, dtype=dtype)).to(DEV).eval()
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    with torch.no_grad():
        if packed:
            rows = E.packed_rows_bound(torch.from_numpy(mask))
            assert rows is not None
            out = E.hip_encode(model.lm_p, items, pooling, head, normalize, E.compute_dtype_code(model.model_args), want_hidden=False,
                               packed_rows=rows)[1]
            assert E.LAST_CALL == {"rows": rows, "packed": True}, E.LAST_CALL
        else:
            out = model.encode_passage(items)[1]
            assert not E.LAST_CALL["packed"]
    out = out.double().cpu()
    lm.to("cpu")
    if head is not None:
        head.to("cpu")
    return out


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def _cos_gap(a, b):
    return 1.0 - torch.nn.functional.cosine_similarity(a, b, dim=1).min().item()


# ------------------------------------------------------------------------------------------------------------- CPU
def test_arch_of_and_position_offset():
    from openmatch_amd.encoder import _arch_of, position_offset
    d, m = _distil(layers=1), _mpnet(layers=1)
    assert _arch_of(d) == "bert" and _arch_of(m) == "bert"
    assert position_offset(d) == 0 and position_offset(m) == 2


def test_other_bert_named_classes_are_refused_by_name():
    from transformers import AlbertConfig, AlbertModel, GPT2Config, GPT2Model
    from openmatch_amd.encoder import _arch_of
    alb = AlbertModel(AlbertConfig(hidden_size=32, embedding_size=16, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64,
                                   vocab_size=50))
    with pytest.raises(NotImplementedError, match="AlbertModel"):
        _arch_of(alb)
    with pytest.raises(NotImplementedError, match="GPT2Model"):
        _arch_of(GPT2Model(GPT2Config(n_embd=32, n_layer=1, n_head=1, vocab_size=50)))


def test_subclasses_of_served_backbones_keep_their_flavour():
    from transformers import MPNetModel
    from openmatch_amd.flavours import dropout_probs, flavour_of

    class MyRetrieverBackbone(MPNetModel):
        pass
    m = _mpnet(layers=1, hidden_dropout_prob=0.2, attention_probs_dropout_prob=0.3)
    assert flavour_of(MyRetrieverBackbone(m.config)) == "mpnet"
    assert dropout_probs(m) == (0.2, 0.3) and dropout_probs(_distil(layers=1, dropout=0.1, attention_dropout=0.4)) == (0.1, 0.4)


def test_mpnet_left_padding_is_refused():
    from openmatch_amd.encoder import check_position_layout
    m, d = _mpnet(layers=1), _distil(layers=1)
    right = torch.tensor([[5, 6, 7, PAD, PAD]])
    check_position_layout(m, right, (right != PAD).long())
    left = torch.tensor([[PAD, PAD, 5, 6, 7]])
    with pytest.raises(ValueError, match="pad token precedes"):
        check_position_layout(m, left, (left != PAD).long())
    check_position_layout(d, left, (left != PAD).long())         # DistilBERT numbers positions 0 .. L-1 regardless


def test_bucket_rule_is_mpnets():
    """om_t5_relative_bucket (the rule behind rel_buckets / rel_max_dist) against MPNetEncoder.relative_position_bucket for every
    offset of a 512-token sequence, at 32 and at 16 buckets."""
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    lib = N.lib()
    lib.om_t5_relative_bucket.restype = C.c_int
    lib.om_t5_relative_bucket.argtypes = [C.c_int, C.c_int, C.c_int]
    rel = torch.arange(-511, 512)
    for nb in (32, 16):
        want = MPNetEncoder.relative_position_bucket(rel, num_buckets=nb, max_distance=128).tolist()
        got = [lib.om_t5_relative_bucket(int(r), nb, 128) for r in rel.tolist()]
        assert got == want, nb


def test_accessor_layer_names_the_modules_own_tensors():
    """flavours.bert_parts for each flavour (BERT and RoBERTa as a regression guard): the packed Q|K|V matrix is the concatenation of
    the module's three weights, and the LayerNorm / FFN / embedding tensors are the module's own parameters."""
    from transformers import BertConfig, BertModel, RobertaConfig, RobertaModel
    from openmatch_amd.flavours import bert_parts
    from openmatch_amd.train import _bert_params
    tiny = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=1, intermediate_size=128, vocab_size=50)
    bert, rob = BertModel(BertConfig(**tiny)), RobertaModel(RobertaConfig(max_position_embeddings=40, **tiny))
    d, m = _distil(dict(hidden=64, heads=1, ffn=128), 2), _mpnet(dict(hidden=64, heads=1, ffn=128), 2)
    named = {
        bert: lambda l: (l.attention.self.query, l.attention.self.key, l.attention.self.value, l.attention.output.dense,
                         l.attention.output.LayerNorm, l.intermediate.dense, l.output.dense, l.output.LayerNorm),
        d: lambda l: (l.attention.q_lin, l.attention.k_lin, l.attention.v_lin, l.attention.out_lin, l.sa_layer_norm, l.ffn.lin1,
                      l.ffn.lin2, l.output_layer_norm),
        m: lambda l: (l.attention.attn.q, l.attention.attn.k, l.attention.attn.v, l.attention.attn.o, l.attention.LayerNorm,
                      l.intermediate.dense, l.output.dense, l.output.LayerNorm),
    }
    named[rob] = named[bert]
    for lm, pick in named.items():
        bp = bert_parts(lm)
        hf_layers = lm.transformer.layer if lm is d else lm.encoder.layer
        assert len(bp.layers) == len(hf_layers) == 2
        for lp, hl in zip(bp.layers, hf_layers):
            assert all(a is b for a, b in zip(lp, pick(hl)))
            qkv = torch.cat([lp.q.weight, lp.k.weight, lp.v.weight], 0)
            q, k, v = pick(hl)[:3]
            assert torch.equal(qkv, torch.cat([q.weight, k.weight, v.weight], 0)) and qkv.shape == (192, 64)
        assert bp.word.weight is lm.embeddings.word_embeddings.weight and bp.pos.weight is lm.embeddings.position_embeddings.weight
        assert bp.emb_ln is lm.embeddings.LayerNorm
        assert (bp.type is None) == (lm is d or lm is m)
        assert (bp.rel_bias is not None) == (lm is m)
        # every encoder parameter the backward writes a gradient for is one of the module's own, each once
        ps = _bert_params(lm, None)
        own = {id(p) for p in lm.parameters()}
        assert all(id(p) in own for p in ps) and len({id(p) for p in ps}) == len(ps)
        missing = [n for n, p in lm.named_parameters() if id(p) not in {id(q) for q in ps} and "pooler" not in n]
        assert missing == [], missing
    assert bert_parts(m).rel_bias.weight is m.encoder.relative_attention_bias.weight
    assert bert_parts(d).eps == 1e-12 and bert_parts(m).eps == 1e-5


def test_config_fields_for_the_two_backbones():
    from openmatch_amd.encoder import bert_config_fields
    m = bert_config_fields(_mpnet(layers=1, buckets=32))
    assert m["rel_buckets"] == 32 and m["rel_max_dist"] == 128 and m["type_vocab"] == 0 and m["max_pos"] == 514 and m["arch"] == N.ARCH_BERT
    assert bert_config_fields(_mpnet(layers=1, buckets=16))["rel_buckets"] == 16
    d = bert_config_fields(_distil(layers=1))
    assert d["rel_buckets"] == 0 and d["rel_max_dist"] == 0 and d["type_vocab"] == 0 and d["max_pos"] == 512 and d["ln_eps"] == 1e-12
    N.OmEncoderConfig(dtype=N.OM_F32, pooling=N.POOL_FIRST, **m)        # every field exists in the (unchanged) ABI struct


def test_workspace_accounts_for_the_bias_only_when_configured():
    lib = N.lib()
    base = dict(arch=N.ARCH_BERT, dtype=N.OM_F16, hidden=768, n_layers=2, n_heads=12, head_dim=64, ffn=3072, vocab=600, max_pos=512,
                act=N.ACT_GELU_ERF, ln_eps=1e-12, pooling=N.POOL_MEAN)
    plain = N.OmEncoderConfig(type_vocab=2, **base)
    notype = N.OmEncoderConfig(type_vocab=0, **base)
    rel = N.OmEncoderConfig(type_vocab=0, rel_buckets=32, rel_max_dist=128, **base)
    B, L = 16, 128
    for fn in (lib.om_encoder_workspace_bytes, lib.om_encoder_train_workspace_bytes):
        a, b, c = (fn(C.byref(x), B, L) for x in (plain, notype, rel))
        assert a == b and c >= a + 12 * L * L * 4, (a, b, c)
    assert lib.om_encoder_tape_bytes(C.byref(plain), B, L) == lib.om_encoder_tape_bytes(C.byref(rel), B, L)
    assert lib.om_encoder_packed_supported(C.byref(rel), 0, 64, 128, 4096) == lib.om_encoder_packed_supported(C.byref(plain), 0, 64, 128, 4096) == 1


def test_token_type_ids_are_dropped_with_one_warning():
    """INTEGRATION.md, observable differences: a batch that carries token_type_ids for a backbone without a token-type table has
    them dropped, with one warning per backbone class."""
    from openmatch_amd import encoder as E
    E._TTI_WARNED.clear()
    d = _distil(layers=1)
    items = {"input_ids": torch.ones(1, 4, dtype=torch.long), "token_type_ids": torch.zeros(1, 4, dtype=torch.long)}
    with pytest.warns(UserWarning, match="DistilBertModel has no token-type embeddings"):
        assert E.token_types_of(d, items) is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert E.token_types_of(d, items) is None            # once only
    from transformers import BertConfig, BertModel
    bert = BertModel(BertConfig(hidden_size=32, num_hidden_layers=1, num_attention_heads=1, intermediate_size=64, vocab_size=50))
    assert E.token_types_of(bert, items) is items["token_type_ids"]


# ------------------------------------------------------------------------------------------------------------- GPU
ENCODE_CASES = [  # (shape, layers, B, L): few rows (<= 64 token rows), the plain / few-rows paths, the fused path (>= 512 rows in 16 bits),
    (SMALL, 3, 2, 24),        # 48 rows: few rows with the LayerNorms folded into the contractions
    (SMALL, 3, 5, 128),       # 640 rows: few-rows kernels (<= 1 024 rows) in f16, fused two-plane path in bf16
    (BASE, 2, 12, 200),       # 2 400 rows: the fused path; 200 tokens: distances beyond max_distance
    (SMALL, 2, 6, 320),       # beyond 256 tokens: the key-chunked attention
    (BASE, 2, 4, 512),        # the longest sequence of the position table
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(ENCODE_CASES)))
@pytest.mark.parametrize("kind", ["distilbert", "mpnet"])
def test_encode_matches_hf(kind, case):
    from openmatch.modeling import LinearHead
    shape, layers, B, L = ENCODE_CASES[case]
    lm = _make(kind, shape, layers, seed=case)
    rng = np.random.default_rng(case)
    ids, mask = _ragged(rng, B, L, 3, _pad_of(kind))
    torch.manual_seed(case)
    head = LinearHead(shape["hidden"], 128)
    for pooling, hd, nrm in (("first", None, False), ("mean", head, True)):
        want = _hf_reps(lm, ids, mask, pooling, hd, nrm)
        got = _hip_reps(lm, ids, mask, pooling, "float32", hd, nrm)
        rel = _rel(got, want)
        gaps = {dt: _cos_gap(_hip_reps(lm, ids, mask, pooling, dt, hd, nrm), want) for dt in ("float16", "bfloat16")}
        print(f"\n[{kind} encode, H={shape['hidden']}, {layers} layers, {B}x{L}, {pooling}{'+head+normalize' if hd else ''}] f32 max rel err "
              f"{rel:.2e}; 1 - min cos: f16 {gaps['float16']:.2e}, bf16 {gaps['bfloat16']:.2e}")
        assert rel < F32_BAR, rel
        for dt, gap in gaps.items():
            assert gap < COS_BAR[dt], (dt, gap)


def _sharp_mpnet(shape=SMALL, layers=2, seed=3, **kw):
    """An MPNet whose output depends strongly on the position bias: table entries of O(1) (N(0, 2)) and the attention branch's v / o
    weights x 8, so that what the softmax weighs dominates the residual stream.  (Sharpening q / k instead -- scores x 64 -- makes
    the content term drown an O(1) bias: zeroing the table then moves the output by 1-4 % only, measured on the CPU.)"""
    lm = _mpnet(shape, layers, seed=seed, **kw)
    with torch.no_grad():
        lm.encoder.relative_attention_bias.weight.mul_(2.0)
        for layer in lm.encoder.layer:
            layer.attention.attn.v.weight.mul_(8.0)
            layer.attention.attn.o.weight.mul_(8.0)
    return lm


def _zero_table_reps(lm, ids, mask, pooling):
    table = lm.encoder.relative_attention_bias.weight
    keep = table.detach().clone()
    with torch.no_grad():
        table.zero_()
    out = _hf_reps(lm, ids, mask, pooling)
    with torch.no_grad():
        table.copy_(keep)
    return out


D32W = dict(hidden=256, heads=8, ffn=1024)             # 32-wide heads at a width the fused / packed paths take

# path -> (shape, B, L, dtype, packed entry, what om_encoder_forward must report under OM_OPT_ENCODER_DEBUG)
BIAS_PATHS = {
    "plain_f32": (SMALL, 6, 128, "float32", False, dict(fused_ln=0, packed=0, few_rows=0, pending_ln=0, head_dim=64)),
    "plain_f16": (D32, 12, 128, "float16", False, dict(fused_ln=0, packed=0, few_rows=0, pending_ln=0, head_dim=32)),
    "few_rows_ln_folded": (SMALL, 2, 30, "float16", False, dict(fused_ln=0, packed=0, few_rows=1, pending_ln=1, head_dim=64)),
    "few_rows": (SMALL, 6, 128, "float16", False, dict(fused_ln=0, packed=0, few_rows=1, pending_ln=0, head_dim=64)),
    "fused": (SMALL, 12, 128, "float16", False, dict(fused_ln=1, packed=0, few_rows=0, pending_ln=0, head_dim=64)),
    "fused_bf16": (SMALL, 12, 128, "bfloat16", False, dict(fused_ln=1, packed=0, few_rows=0, pending_ln=0, head_dim=64)),
    "packed": (SMALL, 24, 128, "bfloat16", True, dict(fused_ln=1, packed=1, few_rows=0, pending_ln=0, head_dim=64)),
    "long": (SMALL, 4, 384, "float16", False, dict(fused_ln=1, packed=0, few_rows=0, pending_ln=0, head_dim=64)),
    "long_packed": (SMALL, 8, 384, "float16", True, dict(fused_ln=1, packed=1, few_rows=0, pending_ln=0, head_dim=64)),
    "long_f32": (SMALL, 2, 300, "float32", False, dict(fused_ln=0, packed=0, few_rows=0, pending_ln=0, head_dim=64)),
    "d32": (D32, 6, 128, "float32", False, dict(fused_ln=0, packed=0, few_rows=0, pending_ln=0, head_dim=32)),
    "d32_long": (D32, 3, 300, "float16", False, dict(fused_ln=0, packed=0, few_rows=1, pending_ln=0, head_dim=32)),
    "d32_packed": (D32W, 24, 128, "float16", True, dict(fused_ln=1, packed=1, few_rows=0, pending_ln=0, head_dim=32)),
}


def _debug_lines(text):
    """The fields of every 'om_encoder_forward: ...' line the library wrote to stderr (csrc/encoder.hip, OM_OPT_ENCODER_DEBUG)."""
    out = []
    for line in text.splitlines():
        if line.startswith("om_encoder_forward:"):
            out.append({k: int(v) for k, v in (f.split("=") for f in line.split(":", 1)[1].split())})
    return out


def _planned(cfg, rows, B, L, packed, gated=False):
    """What om_debug_encoder_plan (csrc/encoder_plan.h, no GPU) says of the call that wrote a debug line, in the line's own fields."""
    word = N.lib().om_debug_encoder_plan(C.byref(cfg), int(gated), int(cfg.arch == N.ARCH_T5 or cfg.rel_buckets > 0), B, L, rows if packed else 0, 0)
    assert word > 0, (word, N.lib().om_last_error())
    path = word & 0xff
    return dict(path=path, fused_ln=int(path == N.ENC_PATH["bert_fused"]), pending_ln=int(path == N.ENC_PATH["bert_pending_ln"]),
                fused_norm=int(path == N.ENC_PATH["t5_fused"]), few_rows=(word >> 8) & 1, packed=int(packed), M=rows)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(BIAS_PATHS))
def test_bias_is_used_on_every_path(path, capfd):
    """An MPNet that leans on its position bias (_sharp_mpnet) with a table of O(1) entries: HF with the table zeroed is > 0.1 away
    from HF with it (asserted first, on the CPU), so a path that dropped the bias could not pass.  The shapes are chosen by the
    dispatch rules of csrc/encoder.hip AND the path taken is asserted: OM_OPT_ENCODER_DEBUG is switched on for the call and the
    line om_encoder_forward writes to stderr must name the expected path (fused LayerNorm / few rows / pending LayerNorms / packed
    rows), the sequence length and head width that select the attention kernel (beyond 256 tokens: key-chunked / online-softmax;
    head_dim 32: attention_d32.hip) and rel_bias=1.  A moved default (few-rows limit, two-plane switch, fused-LayerNorm switch)
    fails the case instead of silently testing another path twice."""
    shape, B, L, dtype, packed, expect = BIAS_PATHS[path]
    lm = _sharp_mpnet(shape)
    rng = np.random.default_rng(11)
    ids, mask = _ragged(rng, B, L, 3 if packed else L // 2, PAD)
    want = _hf_reps(lm, ids, mask, "mean")
    without = _zero_table_reps(lm, ids, mask, "mean")
    moved = _rel(without, want)
    assert moved > 0.1, moved
    lib = N.lib()
    OPT_ENCODER_DEBUG = 1                       # include/openmatch_hip.h: OM_OPT_ENCODER_DEBUG
    before = lib.om_debug_option_value(OPT_ENCODER_DEBUG)
    capfd.readouterr()
    N.check(lib.om_debug_option(OPT_ENCODER_DEBUG, 1))
    try:
        got = _hip_reps(lm, ids, mask, "mean", dtype, packed=packed)
        torch.cuda.synchronize()
    finally:
        N.check(lib.om_debug_option(OPT_ENCODER_DEBUG, before))
    lines = _debug_lines(capfd.readouterr().err)
    assert len(lines) == 1, lines
    took = lines[0]
    assert took["rel_bias"] == 1 and took["L"] == L, took
    assert {k: took[k] for k in expect} == expect, (path, took)
    # the line is printed from the call's plan: the plan asked on its own, for this configuration and these rows, says the same
    from openmatch_amd import encoder as E
    cfg = N.OmEncoderConfig(arch=N.ARCH_BERT, dtype={"float32": N.OM_F32, "bfloat16": N.OM_BF16, "float16": N.OM_F16}[dtype],
                            hidden=shape["hidden"], n_heads=shape["heads"], head_dim=shape["hidden"] // shape["heads"], ffn=shape["ffn"],
                            n_layers=2, vocab=600, max_pos=516, act=N.ACT_GELU_ERF, ln_eps=1e-5, rel_buckets=32, rel_max_dist=128,
                            pooling=N.POOL_MEAN)
    planned = _planned(cfg, E.LAST_CALL["rows"], B, L, packed)
    assert {k: took[k] for k in ("M", "fused_ln", "packed", "few_rows", "pending_ln")} == {k: planned[k] for k in ("M", "fused_ln", "packed", "few_rows", "pending_ln")}, (took, planned)
    if dtype == "float32":
        err = _rel(got, want)
        print(f"\n[MPNet bias, {path}] {took}; table zeroed moves HF by {moved:.2f}; HIP f32 max rel err {err:.2e}")
        assert err < F32_BAR, err
    else:
        gap, gap0 = _cos_gap(got, want), _cos_gap(got, without)
        print(f"\n[MPNet bias, {path}, {dtype}] {took}; table zeroed moves HF by {moved:.2f}; HIP 1 - min cos {gap:.2e} (vs the zeroed run {gap0:.2e})")
        assert gap < COS_BAR[dtype], gap


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fused", "per_site"])
def test_t5_debug_line_names_the_planned_path(case, capfd):
    """The T5 stack's OM_OPT_ENCODER_DEBUG line against om_debug_encoder_plan, on both of its loops: RMSNorm fused across the
    contractions (bfloat16, 1 536 rows, widths of 256) and one normalisation kernel per site (float32)."""
    from transformers import T5Config, T5EncoderModel
    from openmatch.modeling import DRModelForInference
    from openmatch_amd import encoder as E
    dtype, code, fused = ("bfloat16", N.OM_BF16, 1) if case == "fused" else ("float32", N.OM_F32, 0)
    B, L = (12, 128) if fused else (6, 128)
    torch.manual_seed(8)
    lm = T5EncoderModel(T5Config(d_model=256, d_ff=1024, num_layers=2, num_heads=4, d_kv=64, vocab_size=600, feed_forward_proj="relu")).eval()
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=True, dtype=dtype)).to(DEV).eval()
    ids, mask = _ragged(np.random.default_rng(13), B, L, L // 2)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    lib = N.lib()
    before = lib.om_debug_option_value(1)                   # OM_OPT_ENCODER_DEBUG
    capfd.readouterr()
    N.check(lib.om_debug_option(1, 1))
    try:
        with torch.no_grad():
            reps = E.hip_encode(model.lm_p, items, "mean", None, False, E.compute_dtype_code(model.model_args), want_hidden=False)[1]
        torch.cuda.synchronize()
    finally:
        N.check(lib.om_debug_option(1, before))
    lines = [dict((f.split("=")[0], int(f.split("=")[1])) for f in ln.split(":", 1)[1].split())
             for ln in capfd.readouterr().err.splitlines() if ln.startswith("om_encoder_forward (t5):")]
    assert len(lines) == 1 and torch.isfinite(reps).all(), lines
    cfg = N.OmEncoderConfig(arch=N.ARCH_T5, dtype=code, hidden=256, n_heads=4, head_dim=64, ffn=1024, n_layers=2, vocab=600, act=N.ACT_RELU,
                            ln_eps=1e-6, rel_buckets=32, rel_max_dist=128, pooling=N.POOL_MEAN)
    planned = _planned(cfg, B * L, B, L, False)
    assert planned["path"] == N.ENC_PATH["t5_fused" if fused else "t5_plain"] and planned["few_rows"] == 0, planned
    assert lines[0] == {"M": B * L, "fused_norm": fused, "packed": 0} == {k: planned[k] for k in ("M", "fused_norm", "packed")}, (lines, planned)


@pytest.mark.gpu
def test_bucket_edges_and_bucket_count():
    """240 tokens: offsets beyond max_distance = 128 and the log-spaced buckets.  The same weights read with 16 buckets (the first 16
    rows of the table) are far away in HF, and the HIP encoder configured with 16 buckets matches THAT run."""
    lm32 = _sharp_mpnet(buckets=32)
    lm16 = _sharp_mpnet(buckets=16)
    sd = lm32.state_dict()
    sd["encoder.relative_attention_bias.weight"] = sd["encoder.relative_attention_bias.weight"][:16].clone()
    lm16.load_state_dict(sd)
    rng = np.random.default_rng(12)
    ids, mask = _ragged(rng, 4, 240, 200, PAD)
    want32, want16 = _hf_reps(lm32, ids, mask, "mean"), _hf_reps(lm16, ids, mask, "mean")
    apart = _rel(want16, want32)
    assert apart > 0.1, apart
    e32, e16 = _rel(_hip_reps(lm32, ids, mask, "mean", "float32"), want32), _rel(_hip_reps(lm16, ids, mask, "mean", "float32"), want16)
    print(f"\n[MPNet buckets, L=240] 16 vs 32 buckets in HF: {apart:.2f} apart; HIP f32 max rel err {e32:.2e} (32), {e16:.2e} (16)")
    assert e32 < F32_BAR and e16 < F32_BAR, (e32, e16)


@pytest.mark.gpu
@pytest.mark.parametrize("pooling", ["first", "mean"])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("kind", ["distilbert", "mpnet"])
def test_packed_rows_are_bit_identical_to_padded(kind, dtype, pooling):
    lm = _make(kind, SMALL, 3, seed=5)
    rng = np.random.default_rng(9)
    ids, mask = _ragged(rng, 40, 128, 3, _pad_of(kind))
    padded = _hip_reps(lm, ids, mask, pooling, dtype)
    packed = _hip_reps(lm, ids, mask, pooling, dtype, packed=True)
    assert torch.isfinite(padded).all() and torch.equal(packed, padded)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
@pytest.mark.parametrize("kind", ["distilbert", "mpnet"])
def test_padding_invariance(kind, dtype):
    """128 more pad columns change no bit of the representations (padded keys are masked; MPNet: the bias table's pitch grows with
    the padded length, the entries a real token reads do not move)."""
    lm = _make(kind, SMALL, 2, seed=6)
    rng = np.random.default_rng(10)
    ids, mask = _ragged(rng, 12, 96, 10, _pad_of(kind))
    wide_ids = np.concatenate([ids, np.full((12, 128), _pad_of(kind), np.int64)], 1)
    wide_mask = np.concatenate([mask, np.zeros((12, 128), np.int64)], 1)
    for pooling in ("first", "mean"):
        a = _hip_reps(lm, ids, mask, pooling, dtype)
        b = _hip_reps(lm, wide_ids, wide_mask, pooling, dtype)
        assert torch.equal(a, b), (pooling, (a - b).abs().max().item())


COMMON = dict(data_args=NS(train_n_passages=3), train_args=NS(negatives_x_device=False, per_device_train_batch_size=2))


# 64 / 192: every format (192: the longest sequence float32 trains with 64-wide heads).  224, 320, 384, 512: the 16-bit formats on the
# tile-at-a-time attention backward (from 193 tokens on; beyond 256 the forward is the key-chunked kernel) -- with MPNet's bias AND the
# BERT scale 1 / sqrt(d), a pair T5 (scale 1) never exercised.  mpnet_d32 at 256: the eight-tile instantiation of the 32-wide-head
# backward with the bias, float32 included (32-wide heads train to 256 tokens in every format).
TRAIN_CASES = [(k, L) for k in ("distilbert", "mpnet", "mpnet_d32") for L in (64, 192)] + [
    ("mpnet", 224), ("mpnet", 320), ("mpnet", 384), ("mpnet", 512), ("distilbert", 384), ("mpnet_d32", 256)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,L", TRAIN_CASES)
def test_training_step_matches_torch_autograd(kind, L, monkeypatch):
    """DRModel.forward + loss.backward() on 2 queries x 3 passages, dropout 0: the loss and EVERY parameter gradient against torch
    autograd through the HF module in fp32 on the CPU -- relative_attention_bias.weight (summed over the layers) and the position
    table behind MPNet's offset included; the position rows below the offset get exactly zero.  Bars: tests/test_head_dim32.py's
    training test (f32: rel-L2 1e-3; float16 loss-scaled / bfloat16: its 16-bit bars).  mpnet_d32: 32-wide heads."""
    monkeypatch.delenv("OM_TRAIN_F16", raising=False)
    from openmatch.modeling import DRModel
    from oracle import retrieval_ref
    base_kind = "mpnet" if kind.startswith("mpnet") else kind
    shape = D32 if kind == "mpnet_d32" else SMALL
    lm, ref_lm = _make(base_kind, shape, 2, seed=29 + L), _make(base_kind, shape, 2, seed=1)
    ref_lm.load_state_dict(lm.state_dict())
    rng = np.random.default_rng(L + 1)
    pad = _pad_of(base_kind)
    p_ids, p_mask = _ragged(rng, 6, L, L // 2, pad)
    q_ids, q_mask = _ragged(rng, 2, L, 5, pad)

    def ref_mean(ids, mask):
        ids, mask = torch.from_numpy(ids), torch.from_numpy(mask)
        h_ = ref_lm(input_ids=ids, attention_mask=mask).last_hidden_state
        m_ = mask.unsqueeze(-1).float()
        return (h_ * m_).sum(1) / m_.sum(1).clamp(min=1e-9)
    ref_lm.train()
    loss_ref, _ = retrieval_ref.contrastive_loss(ref_mean(q_ids, q_mask), ref_mean(p_ids, p_mask), 3)
    loss_ref.backward()
    gref = {n: t.grad.detach().clone() for n, t in ref_lm.named_parameters() if t.grad is not None}
    expected = {n for n, _ in ref_lm.named_parameters() if "pooler" not in n}
    assert set(gref) == expected
    if base_kind == "mpnet":
        assert gref["encoder.relative_attention_bias.weight"].norm() > 0
    tens = lambda a: torch.from_numpy(a).to(DEV)
    f32_limit = 256 if kind == "mpnet_d32" else 192
    for dtype in (("float32",) if L <= f32_limit else ()) + ("float16", "bfloat16"):
        model = DRModel(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=False, dtype=dtype), **COMMON).to(DEV).train()
        model.zero_grad(set_to_none=True)
        out = model(query={"input_ids": tens(q_ids), "attention_mask": tens(q_mask)},
                    passage={"input_ids": tens(p_ids), "attention_mask": tens(p_mask)})
        lscale = 4096.0 if dtype == "float16" else 1.0
        (out.loss * lscale).backward()
        grads = {n: t.grad for n, t in lm.named_parameters() if t.grad is not None}
        assert set(grads) == expected, set(grads) ^ expected
        worst = ("", 0.0, 0.0)
        for n, ref in gref.items():
            got = grads[n].detach().float().cpu() / lscale
            rel = ((got - ref).norm() / (ref.norm() + 1e-12)).item()
            amax = (got - ref).abs().max().item()
            if n == "embeddings.position_embeddings.weight" and base_kind == "mpnet":
                assert torch.count_nonzero(got[:2]) == 0 and torch.count_nonzero(ref[:PAD]) == 0
            if dtype == "float32":
                assert (rel < 1e-3 or amax < 1e-7) and amax < 5e-5 * max(1.0, ref.norm().item()), (kind, L, n, rel, amax)
            elif ref.norm() < 1e-9 or n.endswith(("attn.k.bias", "k_lin.bias")):      # (true gradient zero: rounding noise only)
                continue
            if amax >= 1e-7 and rel > worst[1]:
                worst = (n, rel, amax)
        dl = abs(out.loss.item() - loss_ref.item())
        if base_kind == "mpnet":
            nb = "encoder.relative_attention_bias.weight"
            gb, rb = grads[nb].detach().float().cpu() / lscale, gref[nb]
            rel_b = ((gb - rb).norm() / rb.norm()).item()
            print(f"\n[{kind} training, L={L}, {dtype}] relative_attention_bias.weight gradient rel-L2 {rel_b:.2e}")
            assert rel_b < (1e-3 if dtype == "float32" else 3e-2 if dtype == "float16" else 8e-2), rel_b
        print(f"\n[{kind} training, L={L}, {dtype}] loss {out.loss.item():.6f} vs torch fp32 {loss_ref.item():.6f}; worst gradient rel-L2 "
              f"{worst[1]:.2e} ({worst[0]})")
        if dtype == "float32":
            assert dl < 2e-5 * max(1.0, abs(loss_ref.item())), dl
        else:
            assert dl < (2e-3 if dtype == "float16" else 2e-2) * max(1.0, abs(loss_ref.item())), dl
            assert worst[1] < (3e-2 if dtype == "float16" else 8e-2), worst
        for t in lm.parameters():
            t.grad = None


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("kind", ["distilbert", "mpnet", "mpnet_d32"])
def test_packed_training_equals_padded_under_dropout(kind, dtype):
    """Dropout 0.1 at both sites: the packed-rows step draws the padded step's masks (keyed on padded coordinates) and reads the
    bias at each sequence's own positions -- the same representations bit for bit, the same gradients up to the summation order
    (tests/test_head_dim32.py's tolerance for BERT)."""
    from openmatch_amd import train as T
    from openmatch_amd.encoder import compute_dtype_code, rows_bound_of, token_rows_of
    drop = dict(dropout=0.1, attention_dropout=0.1) if kind == "distilbert" else dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    shape = D32W if kind == "mpnet_d32" else SMALL       # (mpnet_d32: hidden 256 as 8 heads of 32 -- the 32-wide-head kernels on packed rows with the bias)
    kind = "mpnet" if kind == "mpnet_d32" else kind
    lm = _make(kind, shape, 2, seed=41, **drop).to(DEV).train()
    rng = np.random.default_rng(6)
    B, L = 24, 128
    ids, mask = _ragged(rng, B, L, 3, _pad_of(kind))
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
    worst = ("", 0.0)
    for n in g0:
        if n.endswith(("attn.k.bias", "k_lin.bias")):
            continue
        a, b = g0[n].float(), g1[n].float()
        rel = ((a - b).norm() / a.norm().clamp_min(1e-12)).item()
        if a.norm().item() > 1e-6 and rel > worst[1]:
            worst = (n, rel)
    print(f"\n[{kind} packed training, {dtype}, dropout 0.1] {rows} of {B * L} rows; worst gradient rel-L2 vs padded {worst[1]:.2e} ({worst[0]})")
    assert torch.equal(reps1, reps0)
    assert worst[1] < 1e-6, worst


@pytest.mark.gpu
@pytest.mark.parametrize("fp16", [False, True])
def test_gradient_cache_step_equals_full_batch_step_mpnet(tmp_path, fp16):
    """GCDenseTrainer (chunked, re-encoded) gives the full-batch step's gradients for MPNet, the relative-bias table included
    (tolerances of tests/test_gpu_parity.py::test_gradient_cache_step_equals_full_batch_step)."""
    from openmatch.modeling import DRModel
    from openmatch.trainer import DRTrainer, GCDenseTrainer
    from tests.test_gpu_parity import _trainer_args
    rng = np.random.default_rng(3)
    q_ids, q_mask = _ragged(rng, 4, 16, 4, PAD)
    p_ids, p_mask = _ragged(rng, 12, 48, 10, PAD)
    batch = ({"input_ids": torch.from_numpy(q_ids), "attention_mask": torch.from_numpy(q_mask)},
             {"input_ids": torch.from_numpy(p_ids), "attention_mask": torch.from_numpy(p_mask)})
    grads = []
    for cls in (DRTrainer, GCDenseTrainer):
        lm = _mpnet(SMALL, 2, seed=8)
        model = DRModel(lm_q=lm, lm_p=lm, pooling="first", model_args=NS(encoder_only=False, dtype="float32"),
                        data_args=NS(train_n_passages=3), train_args=NS(negatives_x_device=False, per_device_train_batch_size=4)).to(DEV)
        extra = dict(gc_q_chunk_size=2, gc_p_chunk_size=6) if cls is GCDenseTrainer else {}
        t = cls(model=model, args=_trainer_args(tmp_path, fp16=fp16, fp16_init_scale=1024.0, **extra), train_dataset=None)
        t.training_step(model, batch)
        inv = 1.0 / float(t._loss_scaler().state[0]) if fp16 else 1.0
        grads.append({n: p.grad.clone() * inv for n, p in model.named_parameters() if p.grad is not None})
    assert any("relative_attention_bias" in n for n in grads[0])
    for n in grads[0]:
        a, b = grads[0][n], grads[1][n]
        if fp16 and n.endswith("attn.k.bias"):       # the true gradient is exactly zero (softmax is shift-invariant): 16-bit noise only,
            assert a.abs().max() < 1e-4 and b.abs().max() < 1e-4, n       # nothing to compare relatively (test_head_dim32.py skips it too)
            continue
        if fp16:
            assert (a - b).norm() <= 2e-2 * a.norm() + 1e-7, (n, ((a - b).norm() / a.norm()).item())
        else:
            assert (a - b).abs().max() <= 1e-6 + 1e-4 * a.abs().max(), n


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["distilbert", "mpnet"])
def test_retrieval_end_to_end(kind, tmp_path):
    """96 passages + 12 queries -> Retriever.from_embeddings(...).search(10): the ids of HF fp32 embeddings searched by the oracle's
    IndexFlatIP."""
    import pickle
    from openmatch.modeling import DRModelForInference
    from openmatch.retriever import Retriever
    from oracle import flatip
    lm = _make(kind, SMALL, 2, seed=13)
    rng = np.random.default_rng(13)
    p_ids, p_mask = _ragged(rng, 96, 64, 8, _pad_of(kind))
    q_ids, q_mask = _ragged(rng, 12, 16, 4, _pad_of(kind))
    want_p = _hf_reps(lm, p_ids, p_mask, "mean", None, True).float().numpy()
    want_q = _hf_reps(lm, q_ids, q_mask, "mean", None, True).float().numpy()
    got_p = _hip_reps(lm, p_ids, p_mask, "mean", "float32", None, True).float().numpy()
    got_q = _hip_reps(lm, q_ids, q_mask, "mean", "float32", None, True).float().numpy()
    doc_ids, qry_ids = [f"d{i}" for i in range(96)], [f"q{i}" for i in range(12)]
    with open(tmp_path / "embeddings.corpus.rank.0", "wb") as f:
        pickle.dump((got_p, doc_ids), f, protocol=4)
    with open(tmp_path / "embeddings.query.rank.0", "wb") as f:
        pickle.dump((got_q, qry_ids), f, protocol=4)
    model = DRModelForInference(lm_q=lm, lm_p=lm, pooling="mean", normalize=True, model_args=NS(encoder_only=False, dtype="float32")).to(DEV).eval()
    args = NS(device=DEV, output_dir=str(tmp_path), world_size=1, process_index=0, local_process_index=0, fp16=False)
    run = Retriever.from_embeddings(model, args).search(10)
    o = flatip.IndexFlatIP(want_p.shape[1]); o.add(want_p)
    _, want_ids = o.search(want_q, 10)
    for qi, q in enumerate(qry_ids):
        assert list(run[q].keys()) == [doc_ids[j] for j in want_ids[qi]], q


@pytest.mark.gpu
def test_cross_encoder_over_distilbert():
    """RRModel over DistilBERT with LinearHead(H, 1): scores within 1e-4 of HF; the reranker collator's token_type_ids are dropped."""
    from openmatch.modeling import LinearHead, RRModel
    lm = _distil(SMALL, 2, seed=21)
    torch.manual_seed(21)
    head = LinearHead(256, 1)
    rng = np.random.default_rng(9)
    ids, mask = _ragged(rng, 16, 162, 20)
    items = {"input_ids": torch.from_numpy(ids), "attention_mask": torch.from_numpy(mask), "token_type_ids": torch.zeros_like(torch.from_numpy(ids))}
    with torch.no_grad():
        cls = lm(input_ids=items["input_ids"], attention_mask=items["attention_mask"]).last_hidden_state[:, 0]
        want = (cls @ head.linear.weight.detach().t()).double()
    model = RRModel(lm=lm, head=head, pooling="first", model_args=NS(encoder_only=False, dtype="float32")).to(DEV).eval()
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = model.encode({k: v.to(DEV) for k, v in items.items()}).double().cpu()
    err = (got - want).abs().max().item()
    print(f"\n[DistilBERT cross-encoder] max|err| {err:.2e} (scores up to {want.abs().max().item():.2f})")
    assert got.shape == (16, 1) and err < 1e-4 * max(1.0, want.abs().max().item()), err


@pytest.mark.gpu
@pytest.mark.parametrize("tied", [True, False])
def test_save_build_round_trip_mpnet(tmp_path, tied):
    from openmatch.modeling import DRModel
    lm_q = _mpnet(SMALL, 2, seed=31)
    lm_p = lm_q if tied else _mpnet(SMALL, 2, seed=32)
    margs = NS(encoder_only=False, dtype="float32", untie_encoder=not tied, add_linear_head=False, feature="last_hidden_state",
               pooling="mean", normalize=False, projection_in_dim=256, projection_out_dim=1, model_name_or_path=str(tmp_path),
               cache_dir=None)
    model = DRModel(lm_q=lm_q, lm_p=lm_p, tied=tied, pooling="mean", model_args=margs, **COMMON).to(DEV).eval()
    rng = np.random.default_rng(5)
    ids, mask = _ragged(rng, 4, 40, 10, PAD)
    items = {"input_ids": torch.from_numpy(ids).to(DEV), "attention_mask": torch.from_numpy(mask).to(DEV)}
    with torch.no_grad():
        before = [model.encode_query(items)[1].clone(), model.encode_passage(items)[1].clone()]
    model.save(str(tmp_path))
    again = DRModel.build(margs).to(DEV).eval()
    assert type(again.lm_p).__name__ == "MPNetModel" and (again.lm_q is again.lm_p) == tied
    with torch.no_grad():
        after = [again.encode_query(items)[1], again.encode_passage(items)[1]]
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


@pytest.mark.gpu
def test_training_refusals_keep_the_device_usable():
    """MPNet 16-bit training at 513 tokens and float32 training at 224 raise the limits' existing messages; the next call works."""
    from openmatch.modeling import DRModel
    lm = _mpnet(SMALL, 1, seed=1, max_pos=600)
    rng = np.random.default_rng(1)
    tens = lambda a: torch.from_numpy(a).to(DEV)

    def step(dtype, L):
        p_ids, p_mask = _ragged(rng, 6, L, L // 2, PAD)
        q_ids, q_mask = _ragged(rng, 2, L, 5, PAD)
        model = DRModel(lm_q=lm, lm_p=lm, pooling="mean", model_args=NS(encoder_only=False, dtype=dtype), **COMMON).to(DEV).train()
        return model(query={"input_ids": tens(q_ids), "attention_mask": tens(q_mask)}, passage={"input_ids": tens(p_ids), "attention_mask": tens(p_mask)})
    with pytest.raises(N.NativeError, match="sequence lengths up to 512"):
        step("float16", 513)
    with pytest.raises(N.NativeError, match="float32 training supports sequence lengths up to 192"):
        step("float32", 224)
    out = step("float16", 320)
    out.loss.backward()
    assert torch.isfinite(out.loss) and torch.isfinite(lm.encoder.relative_attention_bias.weight.grad).all()
