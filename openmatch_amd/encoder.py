"""Host side of the HIP encoder: turns a HF `BertModel` / `RobertaModel` / `DistilBertModel` / `MPNetModel` / `T5EncoderModel` /
`ModernBertModel` / `NomicBertModel` / `LlamaModel` / `Qwen2Model` / `Qwen3Model` / `Gemma3TextModel` (the parameter
container the reference keeps in `DRModel.lm_q / lm_p`) into the packed device weights that
`om_encoder_forward` (`om_causal_encoder_forward` for the decoder-only backbones, `om_gemma3_encoder_forward` for EmbeddingGemma)
consumes, and launches it.

The HF module's own `forward` is never called on this path; it stays the owner of the
parameters so `state_dict()` / `save_pretrained()` keep the reference's checkpoint layout
(modeling/dense_retrieval_model.py:230-245).
"""
import ctypes as C
import os

import torch

from . import native as N
from .flavours import bert_parts, flavour_of

_ACT = {"gelu": N.ACT_GELU_ERF, "relu": N.ACT_RELU, "gelu_new": N.ACT_GELU_TANH,
        "gelu_pytorch_tanh": N.ACT_GELU_TANH}


def compute_dtype_code(model_args=None):
    """The compute format the caller asked for, the way the reference asks: `--fp16` -> torch autocast in
    retriever/dense_retriever.py:76 (float16 on a GPU), or ModelArguments.dtype.  float16 and bfloat16 both run on the
    16-bit MFMA path at the same rate; float32 on the exact f32 MFMA path."""
    if torch.is_autocast_enabled():
        return N.OM_F16 if torch.get_autocast_dtype("cuda") == torch.float16 else N.OM_BF16
    dt = getattr(model_args, "dtype", None) if model_args is not None else None
    if dt in ("float16", "fp16"):
        return N.OM_F16
    if dt in ("bfloat16", "bf16"):
        return N.OM_BF16
    return N.OM_F32


def torch_dtype_of(code):
    return {N.OM_BF16: torch.bfloat16, N.OM_F16: torch.float16}.get(code, torch.float32)


def inference_code(model, code, seq_len):
    """float16 is served where it is built: BERT-family encoders with erf-GELU (three more mantissa bits than bfloat16 in every
    stored activation, same speed) and (round 5) T5 ENCODER stacks with ReLU / tanh-GELU feed-forwards -- the reference's `--fp16`
    is float16 autocast for every backbone (retriever/dense_retriever.py:76).  As there, nothing clamps: a T5 checkpoint whose
    feed-forward activations leave the float16 range overflows in the reference and here alike; OM_T5_F16=0 (or `--bf16` /
    dtype="bfloat16") serves such a checkpoint with the bfloat16 kernels.  Other activations: a 16-bit request means bfloat16."""
    if code != N.OM_F16:
        return code
    cfg = getattr(model, "config", None)
    if _arch_of(model) == "causal":              # Llama / Qwen2: float16 and bfloat16 as asked (nothing clamps, as under the reference's autocast)
        return code
    if _arch_of(model) == "nomicbert":           # float16 under BERT's no-clamp statement: as asked
        return code
    if _arch_of(model) == "gemma3":              # as for the decoder-only stacks: the format asked for, nothing clamps
        return code
    if _arch_of(model) == "modernbert":          # the GeGLU feed-forward with erf-GELU: float16 as for erf-GELU BERT
        return code if getattr(cfg, "hidden_activation", None) == "gelu" else N.OM_BF16
    if _arch_of(model) == "t5":
        ok = _ACT.get(getattr(cfg, "dense_act_fn", None)) in (N.ACT_RELU, N.ACT_GELU_TANH) and os.environ.get("OM_T5_F16", "1") != "0"
        return code if ok else N.OM_BF16
    act = getattr(cfg, "activation", None) if flavour_of(model) == "distilbert" else getattr(cfg, "hidden_act", None)
    if _ACT.get(act) != N.ACT_GELU_ERF:
        return N.OM_BF16
    return code


def training_code(code, model=None):
    """The compute format of a TRAINING step.  float16 (the reference's `--fp16` training: HF Trainer's torch.cuda.amp autocast +
    GradScaler, trainer/dense_trainer.py:141-149) is served for BERT-family erf-GELU encoders (round 5; the trainer scales the
    loss, openmatch_amd/trainer/dense_trainer.py) and (round 6) for T5 stacks with ReLU / tanh-GELU feed-forwards, encoder and
    decoder position alike -- under the same conditions as float16 inference (inference_code: as under the reference's autocast nothing
    clamps, OM_T5_F16=0 keeps T5 in bfloat16).  Other activations train in bfloat16; OM_TRAIN_F16=0 sends every float16 request
    there.  Without a model (callers that only name a format): the conservative bfloat16."""
    if code != N.OM_F16:
        return code
    if model is None or os.environ.get("OM_TRAIN_F16", "1") == "0":
        return N.OM_BF16
    return inference_code(model, code, 0)


class _Packed:
    """Device copies of one encoder's weights in one compute dtype + the ctypes views of them."""

    def __init__(self):
        self.keep = []       # tensors that must outlive the ctypes pointers
        self.cfg = {}
        self.weights = N.OmEncoderWeights()
        self.layers = None

    def dev(self, t, dtype, device, sources=None):
        """Device copy of `t` in `dtype` (an alias of `t` itself when it already is that).  `sources`: the parameters the
        buffer is made of, in row order (default: `t` itself when it is a parameter) -- recorded so that an optimizer which
        updates the parameters in place can refresh the copy in the same pass (openmatch_amd/optim.py)."""
        src = t
        t = t.detach().to(device=device, dtype=dtype).contiguous()
        self.keep.append(t)
        if sources is None and isinstance(src, torch.nn.Parameter):
            sources = [src]
        if sources:
            off = 0
            for s_ in sources:
                if t.data_ptr() + off * t.element_size() != s_.data_ptr():       # not an alias of the parameter's own storage
                    _register_shadow(s_, self, t, off)
                off += s_.numel()
        return t.data_ptr()


# parameter -> the packed copies of it that live in some _Packed: [(weakref to the _Packed, buffer, element offset)]
_SHADOWS = {}


def _register_shadow(param, pk, buf, offset):
    import weakref
    key = id(param)
    lst = _SHADOWS.setdefault(key, [])
    lst[:] = [e for e in lst if e[0]() is not None and e[3]() is param]
    lst.append((weakref.ref(pk), buf, int(offset), weakref.ref(param)))


def shadows_of(param):
    """Live packed copies of `param`: [(packed object, buffer tensor, element offset)]; a _Packed that was replaced in its
    cache (or whose model is gone) no longer counts."""
    out = []
    for ref, buf, off, pref in _SHADOWS.get(id(param), ()):
        pk = ref()
        if pk is not None and pref() is param and not getattr(pk, "retired", False):
            out.append((pk, buf, off))
    return out


# what AutoModel returns for RepLLaMA-style / Qwen2-based / SmolLM / TinyLlama embedders; MistralModel (head_dim 128 checkpoints, a
# sliding window) and every *ForCausalLM wrapper stay refused by name.  Qwen3Model (the Qwen3-Embedding models): heads of 64 or 128
# columns, an attention width of its own and q / k norms, through the om_causal2_* entries
_CAUSAL_CLASSES = ("LlamaModel", "Qwen2Model", "Qwen3Model")


# what AutoModel returns for google/embeddinggemma-300m and its fine-tunes; the multimodal wrapper, the LM-head wrappers and the
# classification heads carry a Gemma3TextModel inside and are refused by name
_GEMMA3_REFUSED = ("Gemma3Model", "Gemma3ForCausalLM", "Gemma3ForConditionalGeneration", "Gemma3ForSequenceClassification",
                   "Gemma3TextForSequenceClassification", "Gemma3PreTrainedModel")


def _arch_of(model):
    name = type(model).__name__
    if name == "Gemma3TextModel":        # EmbeddingGemma: bidirectional Gemma3, heads of 256 columns, sliding and full layers
        return "gemma3"
    if name in _GEMMA3_REFUSED or name.startswith("Gemma3"):
        raise NotImplementedError(
            f"openmatch_amd serves Gemma3 through Gemma3TextModel with use_bidirectional_attention (EmbeddingGemma, inference) only; "
            f"got {name}: hand over its text model (AutoModel of an EmbeddingGemma checkpoint returns Gemma3TextModel)")
    if "T5" in name:
        return "t5"
    if name.startswith("ModernBert"):    # ModernBertModel: pre-LayerNorm stack with rotary positions and sliding-window layers
        return "modernbert"
    if name == "NomicBertModel":         # nomic-embed-text-v1 / v1.5: the post-LayerNorm BERT stack without biases, rotary Q / K, SwiGLU
        return "nomicbert"
    if name in _CAUSAL_CLASSES:          # decoder-only backbones as encoders: pre-RMSNorm, rotary grouped-query CAUSAL attention, SwiGLU
        return "causal"
    # BertModel; RobertaModel / XLMRobertaModel (the BERT stack behind offset position ids); DistilBertModel (no token types);
    # MPNetModel (no token types, RoBERTa position numbering, one relative-position bias table for all layers) -- by an explicit
    # rule (flavours.FLAVOURS): AlbertModel, MobileBertModel, SqueezeBertModel, ... carry "Bert" in their names and another layout
    if flavour_of(model) is not None:
        return "bert"
    raise NotImplementedError(
        f"openmatch_amd has HIP encoders for BERT / RoBERTa / DistilBERT / MPNet, T5-encoder, ModernBERT, NomicBERT (NomicBertModel, "
        f"inference), Llama / Qwen2 (head_dim 64, inference) / Qwen3 (head_dim 64 or 128, inference) and bidirectional Gemma3 "
        f"(Gemma3TextModel / EmbeddingGemma, head_dim 256, inference) backbones; got {name}")


def position_offset(model):
    """RoBERTa-family models number positions from padding_idx + 1 (HF:models/roberta/modeling_roberta.py
    create_position_ids_from_input_ids: cumsum over non-pad tokens + padding_idx): token t of a right-padded sequence
    reads row t + padding_idx + 1 of the position table.  The kernels index positions from 0, so the table (and its
    gradient) is handed over starting at that row.  Padded positions read other rows than HF's (row padding_idx) -- they
    are masked out of attention and pooling, so no output depends on them.  MPNet numbers positions the same way
    (HF:models/mpnet/modeling_mpnet.py create_position_ids_from_input_ids).  0 for BERT and DistilBERT."""
    if flavour_of(model) in ("roberta", "mpnet"):
        return _position_pad_id(model) + 1
    return 0


def _position_pad_id(model):
    pad = getattr(model.config, "pad_token_id", None)
    return 1 if pad is None else int(pad)


def check_position_layout(model, ids, mask):
    """RoBERTa-family and MPNet models only: the kernels read position row t (+ position_offset) for token t, HF reads
    cumsum(input_ids != pad)[t] + padding_idx (modeling_roberta.py create_position_ids_from_input_ids).  The two agree on
    every attended token exactly when no pad id precedes an attended token (right-padded text without pad ids inside
    it).  Anything else -- left padding, pad ids inside the text -- would silently read other rows than the reference:
    rejected here (one small device reduction + host read per call, RoBERTa only)."""
    if position_offset(model) == 0:
        return
    pad = _position_pad_id(model)
    L = ids.shape[1]
    pos = torch.arange(L, device=ids.device)
    first_pad = torch.where(ids == pad, pos, L).amin(dim=1)
    last_attended = torch.where(mask != 0, pos, -1).amax(dim=1)
    if bool((last_attended > first_pad).any()):
        raise ValueError("RoBERTa position ids: a pad token precedes an attended token (left-padded input, or pad ids "
                         "inside the text); the HIP encoder numbers positions for right-padded inputs only")


def bert_config_fields(model):
    """The OmEncoderConfig fields of a BERT-family module that do not depend on the compute format (flavours.bert_parts)."""
    bp = bert_parts(model)
    if bp.act not in _ACT:
        raise NotImplementedError(f"activation {bp.act!r} has no HIP epilogue")
    off = position_offset(model)
    return dict(arch=N.ARCH_BERT, hidden=bp.hidden, n_layers=bp.hidden_layers, n_heads=bp.heads, head_dim=bp.hidden // bp.heads,
                ffn=bp.ffn, vocab=bp.vocab, max_pos=bp.max_pos - off, type_vocab=bp.type_vocab if bp.type is not None else 0,
                act=_ACT[bp.act], ln_eps=bp.eps, rel_buckets=bp.rel_buckets if bp.rel_bias is not None else 0,
                rel_max_dist=bp.rel_max_dist if bp.rel_bias is not None else 0)


def _pack_bert(model, code, device):
    bp = bert_parts(model)
    fields = bert_config_fields(model)
    wd = torch_dtype_of(code)
    f32 = torch.float32
    pk = _Packed()
    w = pk.weights
    w.word_emb = pk.dev(bp.word.weight, f32, device)
    off = position_offset(model)
    w.pos_emb = pk.dev(bp.pos.weight, f32, device) + off * bp.hidden * 4
    if bp.type is not None:                  # (DistilBERT, MPNet: no token types -- type_emb stays NULL, type_vocab 0)
        w.type_emb = pk.dev(bp.type.weight, f32, device)
    w.emb_ln_g = pk.dev(bp.emb_ln.weight, f32, device)
    w.emb_ln_b = pk.dev(bp.emb_ln.bias, f32, device)
    if bp.rel_bias is not None:              # (MPNet: one [buckets, heads] table for all layers)
        w.rel_bias = pk.dev(bp.rel_bias.weight, f32, device)
    layers = (N.OmLayerWeights * len(bp.layers))()
    for i, lp in enumerate(bp.layers):
        lw = layers[i]
        qkv_w = torch.cat([lp.q.weight, lp.k.weight, lp.v.weight], 0)
        qkv_b = torch.cat([lp.q.bias, lp.k.bias, lp.v.bias], 0)
        lw.qkv_w = pk.dev(qkv_w, wd, device, [lp.q.weight, lp.k.weight, lp.v.weight])
        lw.qkv_b = pk.dev(qkv_b, f32, device, [lp.q.bias, lp.k.bias, lp.v.bias])
        lw.o_w = pk.dev(lp.o.weight, wd, device)
        lw.o_b = pk.dev(lp.o.bias, f32, device)
        lw.ln1_g = pk.dev(lp.ln1.weight, f32, device)
        lw.ln1_b = pk.dev(lp.ln1.bias, f32, device)
        lw.ffn1_w = pk.dev(lp.ffn1.weight, wd, device)
        lw.ffn1_b = pk.dev(lp.ffn1.bias, f32, device)
        lw.ffn2_w = pk.dev(lp.ffn2.weight, wd, device)
        lw.ffn2_b = pk.dev(lp.ffn2.bias, f32, device)
        lw.ln2_g = pk.dev(lp.ln2.weight, f32, device)
        lw.ln2_b = pk.dev(lp.ln2.bias, f32, device)
    pk.layers = layers
    w.layers_host = C.cast(layers, C.POINTER(N.OmLayerWeights))
    pk.cfg = dict(dtype=code, **fields)
    return pk


def _pack_t5(model, code, device):
    cfg = model.config
    if cfg.num_heads * cfg.d_kv != cfg.d_model:
        raise NotImplementedError("T5 with inner_dim != d_model is not supported")
    wd = torch_dtype_of(code)
    f32 = torch.float32
    pk = _Packed()
    enc = model.encoder
    w = pk.weights
    w.word_emb = pk.dev(enc.embed_tokens.weight, f32, device)
    w.final_ln_g = pk.dev(enc.final_layer_norm.weight, f32, device)
    w.rel_bias = pk.dev(enc.block[0].layer[0].SelfAttention.relative_attention_bias.weight, f32, device)
    layers = (N.OmLayerWeights * cfg.num_layers)()
    gated = bool(getattr(cfg, "is_gated_act", False))
    for i, block in enumerate(enc.block):
        sa, ff, lw = block.layer[0].SelfAttention, block.layer[1].DenseReluDense, layers[i]
        lw.qkv_w = pk.dev(torch.cat([sa.q.weight, sa.k.weight, sa.v.weight], 0), wd, device, [sa.q.weight, sa.k.weight, sa.v.weight])
        lw.o_w = pk.dev(sa.o.weight, wd, device)
        lw.ln1_g = pk.dev(block.layer[0].layer_norm.weight, f32, device)
        lw.ln2_g = pk.dev(block.layer[1].layer_norm.weight, f32, device)
        if gated:
            lw.ffn1_w = pk.dev(ff.wi_0.weight, wd, device)
            lw.ffn1g_w = pk.dev(ff.wi_1.weight, wd, device)
        else:
            lw.ffn1_w = pk.dev(ff.wi.weight, wd, device)
        lw.ffn2_w = pk.dev(ff.wo.weight, wd, device)
    pk.layers = layers
    w.layers_host = C.cast(layers, C.POINTER(N.OmLayerWeights))
    act = cfg.dense_act_fn
    if act not in _ACT:
        raise NotImplementedError(f"activation {act!r} has no HIP epilogue")
    pk.cfg = dict(arch=N.ARCH_T5, dtype=code, hidden=cfg.d_model, n_layers=cfg.num_layers,
                  n_heads=cfg.num_heads, head_dim=cfg.d_kv, ffn=cfg.d_ff, vocab=cfg.vocab_size,
                  max_pos=0, type_vocab=0, act=_ACT[act], ln_eps=float(cfg.layer_norm_epsilon),
                  rel_buckets=cfg.relative_attention_num_buckets,
                  rel_max_dist=cfg.relative_attention_max_distance)
    return pk


def modernbert_config_fields(cfg):
    """The ModernBERT-only OmEncoderConfig fields of a `ModernBertConfig`: the two rope thetas, the half window and the per-layer
    sliding flags (bit l: config.layer_types[l] == "sliding_attention"), after refusing what the HIP encoder does not serve."""
    if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False):
        raise NotImplementedError("ModernBERT with attention_bias / mlp_bias = True is not supported by the HIP encoder")
    if cfg.hidden_size % cfg.num_attention_heads or cfg.hidden_size // cfg.num_attention_heads != 64:
        raise NotImplementedError(f"ModernBERT: only head_dim 64 is supported (got {cfg.hidden_size} / {cfg.num_attention_heads} heads)")
    if cfg.hidden_activation != "gelu":
        raise NotImplementedError(f"ModernBERT: hidden_activation must be 'gelu' (erf); got {cfg.hidden_activation!r}")
    types = list(cfg.layer_types)
    if len(types) != cfg.num_hidden_layers or any(t not in ("full_attention", "sliding_attention") for t in types):
        raise NotImplementedError(f"ModernBERT layer_types must name full_attention / sliding_attention per layer; got {types}")
    if len(types) > 64:
        raise NotImplementedError("ModernBERT: at most 64 layers")
    rp = cfg.rope_parameters
    for kind in ("full_attention", "sliding_attention"):
        if rp[kind].get("rope_type", "default") != "default":
            raise NotImplementedError(f"ModernBERT: only default rope is supported (got {rp[kind]['rope_type']!r} for {kind})")
    mask = 0
    for i, t in enumerate(types):
        if t == "sliding_attention":
            mask |= 1 << i
    return dict(rope_theta_global=float(rp["full_attention"]["rope_theta"]),
                rope_theta_local=float(rp["sliding_attention"]["rope_theta"]),
                half_window=int(cfg.local_attention) // 2, sliding_layers=mask)


def _pack_modernbert(model, code, device):
    cfg = model.config
    extra = modernbert_config_fields(cfg)
    wd = torch_dtype_of(code)
    f32 = torch.float32
    pk = _Packed()
    w = pk.weights
    opt = lambda t: pk.dev(t, f32, device) if t is not None else None       # noqa: E731  (norm_bias = False: no bias)
    w.word_emb = pk.dev(model.embeddings.tok_embeddings.weight, f32, device)
    w.emb_ln_g = pk.dev(model.embeddings.norm.weight, f32, device)
    w.emb_ln_b = opt(model.embeddings.norm.bias)
    w.final_ln_g = pk.dev(model.final_norm.weight, f32, device)
    w.final_ln_b = opt(model.final_norm.bias)
    F = cfg.intermediate_size
    layers = (N.OmLayerWeights * cfg.num_hidden_layers)()
    for i, layer in enumerate(model.layers):
        lw = layers[i]
        lw.qkv_w = pk.dev(layer.attn.Wqkv.weight, wd, device)               # rows q | k | v already
        lw.o_w = pk.dev(layer.attn.Wo.weight, wd, device)
        if isinstance(layer.attn_norm, torch.nn.LayerNorm):                   # (nn.Identity in layer 0)
            lw.ln1_g = pk.dev(layer.attn_norm.weight, f32, device)
            lw.ln1_b = opt(layer.attn_norm.bias)
        lw.ln2_g = pk.dev(layer.mlp_norm.weight, f32, device)
        lw.ln2_b = opt(layer.mlp_norm.bias)
        wi = pk.dev(layer.mlp.Wi.weight, wd, device)                          # [2F, H]: input rows 0..F-1, gate rows F..2F-1
        lw.ffn1_w = wi
        lw.ffn1g_w = wi + F * cfg.hidden_size * torch.finfo(wd).bits // 8
        lw.ffn2_w = pk.dev(layer.mlp.Wo.weight, wd, device)
    pk.layers = layers
    w.layers_host = C.cast(layers, C.POINTER(N.OmLayerWeights))
    pk.cfg = dict(arch=N.ARCH_MODERNBERT, dtype=code, hidden=cfg.hidden_size, n_layers=cfg.num_hidden_layers,
                  n_heads=cfg.num_attention_heads, head_dim=64, ffn=F, vocab=cfg.vocab_size, max_pos=0, type_vocab=0,
                  act=N.ACT_GELU_ERF, ln_eps=float(cfg.norm_eps), rel_buckets=0, rel_max_dist=0, **extra)
    return pk


def nomicbert_config_fields(cfg, model=None):
    """The OmEncoderConfig fields of a `NomicBertModel` that do not depend on the compute format, after refusing (by name and limit,
    before anything touches the device) what the HIP stack does not serve.  The theta is `rope_parameters["rope_theta"]`: the device
    derives the default rope's frequencies 1 / theta ** (2i / 64) from it as NomicBertRotaryEmbedding does in f32, with cos / sin
    unscaled -- so any other rope type, or a scaling other than 1, is refused.  max_pos bounds the sequence length only (there is no
    position table)."""
    name = "NomicBertModel"
    heads, hidden, ffn = int(cfg.num_attention_heads), int(cfg.hidden_size), int(cfg.intermediate_size)
    rp = getattr(cfg, "rope_parameters", None) or {}
    rope_type = rp.get("rope_type", "default")
    if rope_type != "default":
        raise NotImplementedError(f"{name}: rope type {rope_type!r} is not supported by the HIP encoder; only default rope is")
    scaling = float(getattr(getattr(model, "rotary_emb", None), "attention_scaling", 1.0))
    if scaling != 1.0:
        raise NotImplementedError(f"{name}: rotary attention_scaling must be 1; got {scaling}")
    head_dim = getattr(cfg, "head_dim", None) or hidden // heads
    if head_dim != 64 or heads * 64 != hidden:
        raise NotImplementedError(f"{name}: only head_dim 64 with num_attention_heads * 64 == hidden_size is supported "
                                  f"(got head_dim {head_dim}, {heads} heads, hidden_size {hidden})")
    if cfg.hidden_act != "silu":
        raise NotImplementedError(f"{name}: hidden_act must be 'silu'; got {cfg.hidden_act!r}")
    if hidden % 64 or ffn % 64 or hidden > 2048:
        raise NotImplementedError(f"{name}: hidden_size and intermediate_size must be multiples of 64, hidden_size at most 2048 "
                                  f"(got {hidden}, {ffn}): the row kernels hold a row of at most 2048 columns")
    theta = float(rp.get("rope_theta", getattr(cfg, "default_theta", 1000.0)))
    if not theta > 0:
        raise NotImplementedError(f"{name}: rope_theta must be positive; got {theta}")
    return dict(arch=N.ARCH_NOMICBERT, hidden=hidden, n_layers=int(cfg.num_hidden_layers), n_heads=heads, head_dim=64, ffn=ffn,
                vocab=int(cfg.vocab_size), max_pos=int(cfg.max_position_embeddings), type_vocab=int(cfg.type_vocab_size),
                act=N.ACT_SILU, ln_eps=float(cfg.layer_norm_eps), rel_buckets=0, rel_max_dist=0, rope_theta_global=theta)


def _pack_nomicbert(model, code, device):
    """NomicBertModel: word and token-type tables and every LayerNorm in f32, the matrices in the compute dtype, no biases anywhere;
    qkv_w = [q; k; v] and ffn1_w = [gate_proj; up_proj] ([2F, H]: ONE FFN1 contraction, split again by the SwiGLU pass), ffn2_w =
    down_proj; ln1 = post_attention_layernorm, ln2 = post_mlp_layernorm."""
    cfg = model.config
    fields = nomicbert_config_fields(cfg, model)
    wd = torch_dtype_of(code)
    f32 = torch.float32
    pk = _Packed()
    w = pk.weights
    emb = model.embeddings
    w.word_emb = pk.dev(emb.word_embeddings.weight, f32, device)
    w.type_emb = pk.dev(emb.token_type_embeddings.weight, f32, device)
    w.emb_ln_g = pk.dev(emb.LayerNorm.weight, f32, device)
    w.emb_ln_b = pk.dev(emb.LayerNorm.bias, f32, device)
    layers = (N.OmLayerWeights * cfg.num_hidden_layers)()
    for i, layer in enumerate(model.layers):
        sa, mlp, lw = layer.self_attn, layer.mlp, layers[i]
        projs = [sa.q_proj.weight, sa.k_proj.weight, sa.v_proj.weight]
        lw.qkv_w = pk.dev(torch.cat(projs, 0), wd, device, projs)
        lw.o_w = pk.dev(sa.o_proj.weight, wd, device)
        lw.ln1_g = pk.dev(layer.post_attention_layernorm.weight, f32, device)
        lw.ln1_b = pk.dev(layer.post_attention_layernorm.bias, f32, device)
        gate_up = [mlp.gate_proj.weight, mlp.up_proj.weight]
        lw.ffn1_w = pk.dev(torch.cat(gate_up, 0), wd, device, gate_up)
        lw.ffn2_w = pk.dev(mlp.down_proj.weight, wd, device)
        lw.ln2_g = pk.dev(layer.post_mlp_layernorm.weight, f32, device)
        lw.ln2_b = pk.dev(layer.post_mlp_layernorm.bias, f32, device)
    pk.layers = layers
    w.layers_host = C.cast(layers, C.POINTER(N.OmLayerWeights))
    pk.cfg = dict(dtype=code, **fields)
    return pk


def causal_config_fields(cfg, model):
    """The OmCausalConfig fields of a `LlamaModel` / `Qwen2Model` that do not depend on the compute format, after refusing (by name and
    limit, before anything touches the device) what the HIP stack does not serve.  The rotary frequencies and the cos / sin scaling
    are the module's OWN (`rotary_emb.inv_freq`, `rotary_emb.attention_scaling`): `default`, `linear` and `llama3` rope without
    restating HF's rules; the types whose frequencies depend on the sequence length are refused."""
    name = type(model).__name__ if model is not None else "Llama / Qwen2"
    heads, hidden = int(cfg.num_attention_heads), int(cfg.hidden_size)
    head_dim = getattr(cfg, "head_dim", None) or hidden // heads
    if head_dim != 64 or heads * 64 != hidden:
        raise NotImplementedError(f"{name}: only head_dim 64 with num_attention_heads * 64 == hidden_size is supported "
                                  f"(got head_dim {head_dim}, {heads} heads, hidden_size {hidden}); head_dim 128 has no attention kernel")
    n_kv = int(getattr(cfg, "num_key_value_heads", None) or heads)
    if n_kv < 1 or heads % n_kv:
        raise NotImplementedError(f"{name}: num_key_value_heads ({n_kv}) must divide num_attention_heads ({heads})")
    if hidden % 64 or cfg.intermediate_size % 64 or hidden > 2048:
        raise NotImplementedError(f"{name}: hidden_size and intermediate_size must be multiples of 64, hidden_size at most 2048 "
                                  f"(got {hidden}, {cfg.intermediate_size})")
    if getattr(cfg, "mlp_bias", False):
        raise NotImplementedError(f"{name} with mlp_bias = True is not supported by the HIP encoder")
    if getattr(cfg, "use_sliding_window", False):
        raise NotImplementedError(f"{name} with use_sliding_window = True is not supported by the HIP encoder (causal attention over the whole prefix only)")
    if any(t != "full_attention" for t in (getattr(cfg, "layer_types", None) or ())):
        raise NotImplementedError(f"{name}: every layer must be full_attention; got layer_types {list(cfg.layer_types)}")
    if cfg.hidden_act != "silu":
        raise NotImplementedError(f"{name}: hidden_act must be 'silu'; got {cfg.hidden_act!r}")
    rp = getattr(cfg, "rope_parameters", None) or {}
    rope_type = rp.get("rope_type", "default")
    if rope_type not in ("default", "linear", "llama3"):
        raise NotImplementedError(f"{name}: rope type {rope_type!r} is not supported by the HIP encoder (its frequencies depend on the "
                                  "sequence length); default, linear and llama3 are")
    rot = model.rotary_emb
    inv = rot.inv_freq.detach().to("cpu", torch.float32).reshape(-1)
    if inv.numel() != 32:
        raise NotImplementedError(f"{name}: expected 32 rotary frequencies (head_dim 64, full rotation); got {inv.numel()}")
    return dict(arch=N.ARCH_CAUSAL, hidden=hidden, n_layers=int(cfg.num_hidden_layers), n_heads=heads, head_dim=64,
                ffn=int(cfg.intermediate_size), vocab=int(cfg.vocab_size), max_pos=0, type_vocab=0, act=N.ACT_SILU,
                ln_eps=float(cfg.rms_norm_eps), rel_buckets=0, rel_max_dist=0,
                n_kv_heads=n_kv, rope_attention_scaling=float(rot.attention_scaling), inv_freq=[float(v) for v in inv])


def is_qwen3(model):
    return type(model).__name__ == "Qwen3Model"


def qwen3_config_fields(cfg, model):
    """The OmCausalConfig2 fields of a `Qwen3Model` that do not depend on the compute format, after refusing (naming Qwen3Model and the
    limit, before anything touches the device) what the HIP stack does not serve.  head_dim is the config's own (64 or 128) and the
    attention width num_attention_heads * head_dim need not equal hidden_size; the D / 2 rotary frequencies and the cos / sin scaling
    are the module's own, under Llama's rope-type rule; eps is rms_norm_eps, for the block norms and the q / k norms alike."""
    name = "Qwen3Model"
    heads, hidden = int(cfg.num_attention_heads), int(cfg.hidden_size)
    head_dim = int(getattr(cfg, "head_dim", None) or hidden // heads)
    if head_dim not in (64, 128):
        raise NotImplementedError(f"{name}: head_dim {head_dim} is not supported by the HIP encoder (attention kernels exist for head_dim 64 and 128)")
    n_kv = int(getattr(cfg, "num_key_value_heads", None) or heads)
    if n_kv < 1 or heads % n_kv:
        raise NotImplementedError(f"{name}: num_key_value_heads ({n_kv}) must divide num_attention_heads ({heads})")
    if hidden % 64 or cfg.intermediate_size % 64 or hidden > 2048:
        raise NotImplementedError(f"{name}: hidden_size and intermediate_size must be multiples of 64, hidden_size at most 2048 "
                                  f"(got {hidden}, {cfg.intermediate_size}): the row kernels hold a row of at most 2048 columns")
    if getattr(cfg, "use_sliding_window", False):
        raise NotImplementedError(f"{name} with use_sliding_window = True is not supported by the HIP encoder (causal attention over the whole prefix only)")
    if any(t != "full_attention" for t in (getattr(cfg, "layer_types", None) or ())):
        raise NotImplementedError(f"{name}: every layer must be full_attention; got layer_types {list(cfg.layer_types)}")
    if cfg.hidden_act != "silu":
        raise NotImplementedError(f"{name}: hidden_act must be 'silu'; got {cfg.hidden_act!r}")
    rp = getattr(cfg, "rope_parameters", None) or {}
    rope_type = rp.get("rope_type", "default")
    if rope_type not in ("default", "linear", "llama3"):
        raise NotImplementedError(f"{name}: rope type {rope_type!r} is not supported by the HIP encoder (its frequencies depend on the "
                                  "sequence length); default, linear and llama3 are")
    rot = model.rotary_emb
    inv = rot.inv_freq.detach().to("cpu", torch.float32).reshape(-1)
    if inv.numel() != head_dim // 2:
        raise NotImplementedError(f"{name}: expected {head_dim // 2} rotary frequencies (head_dim {head_dim}, full rotation); got {inv.numel()}")
    return dict(arch=N.ARCH_CAUSAL, hidden=hidden, n_layers=int(cfg.num_hidden_layers), n_heads=heads, head_dim=head_dim,
                ffn=int(cfg.intermediate_size), vocab=int(cfg.vocab_size), max_pos=0, type_vocab=0, act=N.ACT_SILU,
                ln_eps=float(cfg.rms_norm_eps), rel_buckets=0, rel_max_dist=0,
                n_kv_heads=n_kv, rope_attention_scaling=float(rot.attention_scaling), inv_freq=[float(v) for v in inv], qk_norm=1)


def gemma3_config_fields(cfg, model):
    """The OmGemma3Config fields of a bidirectional `Gemma3TextModel` (EmbeddingGemma) that do not depend on the compute format, after
    refusing (naming Gemma3TextModel and the limit, before anything touches the device) what the HIP stack does not serve.  The half
    window is `config.sliding_window - 1` read AFTER construction: with use_bidirectional_attention the config has already replaced
    sliding_window by sliding_window // 2 + 1, and a sliding layer sees key k from query q iff |q - k| < config.sliding_window.  The two
    sets of 128 rotary frequencies and their cos / sin scalings are the module's own buffers (`rotary_emb.<layer type>_inv_freq`,
    `rotary_emb.<layer type>_attention_scaling`); the score scale is query_pre_attn_scalar ** -0.5, a config field of its own."""
    name = "Gemma3TextModel"
    heads, hidden, ffn = int(cfg.num_attention_heads), int(cfg.hidden_size), int(cfg.intermediate_size)
    head_dim = int(getattr(cfg, "head_dim", None) or hidden // heads)
    if head_dim != 256:
        raise NotImplementedError(f"{name}: head_dim {head_dim} is not supported by the HIP encoder (the Gemma3 stack has attention kernels for head_dim 256 only)")
    if not getattr(cfg, "use_bidirectional_attention", False):
        raise NotImplementedError(f"{name} with use_bidirectional_attention = False (a causal Gemma3) is not supported by the HIP encoder; "
                                  "EmbeddingGemma's bidirectional encoder is")
    n_kv = int(getattr(cfg, "num_key_value_heads", None) or heads)
    if n_kv < 1 or heads % n_kv:
        raise NotImplementedError(f"{name}: num_key_value_heads ({n_kv}) must divide num_attention_heads ({heads})")
    if hidden % 64 or ffn % 64 or hidden > 2048:
        raise NotImplementedError(f"{name}: hidden_size and intermediate_size must be multiples of 64, hidden_size at most 2048 "
                                  f"(got {hidden}, {ffn}): the row kernels hold a row of at most 2048 columns")
    if cfg.hidden_activation != "gelu_pytorch_tanh":
        raise NotImplementedError(f"{name}: hidden_activation must be 'gelu_pytorch_tanh'; got {cfg.hidden_activation!r}")
    if getattr(cfg, "attention_bias", False):
        raise NotImplementedError(f"{name} with attention_bias = True is not supported by the HIP encoder")
    if getattr(cfg, "attn_logit_softcapping", None) is not None:
        raise NotImplementedError(f"{name}: attn_logit_softcapping must be None; got {cfg.attn_logit_softcapping}")
    types = list(cfg.layer_types)
    if len(types) != cfg.num_hidden_layers or any(t not in ("full_attention", "sliding_attention") for t in types):
        raise NotImplementedError(f"{name}: layer_types must name full_attention / sliding_attention per layer; got {types}")
    if len(types) > 64:
        raise NotImplementedError(f"{name}: at most 64 layers")
    rp = getattr(cfg, "rope_parameters", None) or {}
    rot = model.rotary_emb
    freqs, scalings = {}, {}
    for kind in ("full_attention", "sliding_attention"):
        if kind not in types:                      # (no layer reads this table)
            freqs[kind], scalings[kind] = [0.0] * 128, 1.0
            continue
        rope_type = (rp.get(kind) or {}).get("rope_type", "default")
        if rope_type not in ("default", "linear"):
            raise NotImplementedError(f"{name}: rope type {rope_type!r} ({kind}) is not supported by the HIP encoder; default and linear are")
        inv = getattr(rot, f"{kind}_inv_freq").detach().to("cpu", torch.float32).reshape(-1)
        if inv.numel() != 128:
            raise NotImplementedError(f"{name}: expected 128 rotary frequencies for {kind} (head_dim 256, full rotation); got {inv.numel()}")
        freqs[kind] = [float(v) for v in inv]
        scalings[kind] = float(getattr(rot, f"{kind}_attention_scaling"))
    mask = 0
    for i, t in enumerate(types):
        if t == "sliding_attention":
            mask |= 1 << i
    half_window = int(cfg.sliding_window) - 1 if mask else 0
    if mask and half_window < 1:
        raise NotImplementedError(f"{name}: sliding layers need config.sliding_window of at least 2; got {cfg.sliding_window}")
    return dict(arch=N.ARCH_GEMMA3, hidden=hidden, n_layers=int(cfg.num_hidden_layers), n_heads=heads, head_dim=256, ffn=ffn,
                vocab=int(cfg.vocab_size), max_pos=0, type_vocab=0, act=N.ACT_GELU_TANH, ln_eps=float(cfg.rms_norm_eps), rel_buckets=0,
                rel_max_dist=0, n_kv_heads=n_kv, attn_scale=float(cfg.query_pre_attn_scalar) ** -0.5, half_window=half_window,
                sliding_layers=mask, full_scaling=scalings["full_attention"], sliding_scaling=scalings["sliding_attention"],
                full_inv_freq=freqs["full_attention"], sliding_inv_freq=freqs["sliding_attention"])


_GEMMA3_OWN = ("n_kv_heads", "attn_scale", "half_window", "sliding_layers", "full_scaling", "sliding_scaling", "full_inv_freq", "sliding_inv_freq")


def gemma3_config(pk_cfg, pooling, normalize):
    """The OmGemma3Config of a packed Gemma3TextModel (`_pack_gemma3`'s cfg dict + the head fields) for one call."""
    base = N.OmEncoderConfig(pooling=pooling, normalize=int(bool(normalize)), **{k: v for k, v in pk_cfg.items() if k not in _GEMMA3_OWN})
    inner = N.OmCausalConfig(base=base, n_kv_heads=pk_cfg["n_kv_heads"], rope_attention_scaling=1.0, inv_freq=(C.c_float * 32)(*([0.0] * 32)))
    return N.OmGemma3Config(base=inner, attn_scale=pk_cfg["attn_scale"], half_window=pk_cfg["half_window"], sliding_layers=pk_cfg["sliding_layers"],
                            full_scaling=pk_cfg["full_scaling"], sliding_scaling=pk_cfg["sliding_scaling"], attn_logit_softcapping=0.0,
                            bidirectional=1, full_inv_freq=(C.c_float * 128)(*pk_cfg["full_inv_freq"]),
                            sliding_inv_freq=(C.c_float * 128)(*pk_cfg["sliding_inv_freq"]))


def _pack_gemma3(model, code, device):
    """Gemma3TextModel: the matrices in the compute dtype, q / k / v fused to rows q | k | v of [(heads + 2 kv) * 256, H]; every
    RMSNorm weight as g = 1 + weight in f32 (Gemma3RMSNorm multiplies by 1.0 + weight.float(): the same f32 sum), the four that
    OmLayerWeights has no field for in pk.norms (an OmGemma3Norms array); the embedding table multiplied in f32 by float32(sqrt(hidden)),
    the factor HF applies to the looked-up row."""
    cfg = model.config
    fields = gemma3_config_fields(cfg, model)
    wd = torch_dtype_of(code)
    f32 = torch.float32
    pk = _Packed()
    w = pk.weights
    one_plus = lambda p: pk.dev(1.0 + p.detach().to(f32), f32, device)       # noqa: E731
    scale = torch.tensor(cfg.hidden_size ** 0.5, dtype=f32)
    w.word_emb = pk.dev(model.embed_tokens.weight.detach().to(f32) * scale.to(model.embed_tokens.weight.device), f32, device)
    w.final_ln_g = one_plus(model.norm.weight)
    layers = (N.OmLayerWeights * cfg.num_hidden_layers)()
    norms = (N.OmGemma3Norms * cfg.num_hidden_layers)()
    for i, layer in enumerate(model.layers):
        sa, mlp, lw = layer.self_attn, layer.mlp, layers[i]
        projs = [sa.q_proj, sa.k_proj, sa.v_proj]
        if any(p.bias is not None for p in projs) or sa.o_proj.bias is not None:
            raise NotImplementedError("Gemma3TextModel with attention_bias = True is not supported by the HIP encoder")
        lw.qkv_w = pk.dev(torch.cat([p.weight for p in projs], 0), wd, device, [p.weight for p in projs])
        lw.o_w = pk.dev(sa.o_proj.weight, wd, device)
        lw.ln1_g = one_plus(layer.input_layernorm.weight)
        lw.ln2_g = one_plus(layer.pre_feedforward_layernorm.weight)
        lw.ffn1_w = pk.dev(mlp.gate_proj.weight, wd, device)
        lw.ffn1g_w = pk.dev(mlp.up_proj.weight, wd, device)
        lw.ffn2_w = pk.dev(mlp.down_proj.weight, wd, device)
        norms[i].q_norm_g = one_plus(sa.q_norm.weight)
        norms[i].k_norm_g = one_plus(sa.k_norm.weight)
        norms[i].post_attention_norm_g = one_plus(layer.post_attention_layernorm.weight)
        norms[i].post_feedforward_norm_g = one_plus(layer.post_feedforward_layernorm.weight)
    pk.layers = layers
    pk.norms = norms
    w.layers_host = C.cast(layers, C.POINTER(N.OmLayerWeights))
    pk.cfg = dict(dtype=code, **fields)
    return pk


def _pack_causal(model, code, device):
    """LlamaModel / Qwen2Model / Qwen3Model: the embedding table and the RMSNorm weights in f32, the matrices in the compute dtype;
    q / k / v fused to rows q | k | v of [(heads + 2 kv) * head_dim, H] (a missing bias of a projection that has siblings with one
    counts as zero).  Qwen3Model: the per-layer q_norm / k_norm weights [head_dim] in f32 as well (pk.qk_norm, an OmCausalQkNorm
    array), and a cfg dict that carries qk_norm -- the key that routes its calls to the om_causal2_* entries."""
    cfg = model.config
    fields = qwen3_config_fields(cfg, model) if is_qwen3(model) else causal_config_fields(cfg, model)
    qk_norm = (N.OmCausalQkNorm * cfg.num_hidden_layers)() if is_qwen3(model) else None
    wd = torch_dtype_of(code)
    f32 = torch.float32
    pk = _Packed()
    w = pk.weights
    w.word_emb = pk.dev(model.embed_tokens.weight, f32, device)
    w.final_ln_g = pk.dev(model.norm.weight, f32, device)
    layers = (N.OmLayerWeights * cfg.num_hidden_layers)()
    for i, layer in enumerate(model.layers):
        sa, mlp, lw = layer.self_attn, layer.mlp, layers[i]
        projs = [sa.q_proj, sa.k_proj, sa.v_proj]
        lw.qkv_w = pk.dev(torch.cat([p.weight for p in projs], 0), wd, device, [p.weight for p in projs])
        if any(p.bias is not None for p in projs):
            if all(p.bias is not None for p in projs):
                lw.qkv_b = pk.dev(torch.cat([p.bias for p in projs], 0), f32, device, [p.bias for p in projs])
            else:
                lw.qkv_b = pk.dev(torch.cat([p.bias if p.bias is not None else p.weight.new_zeros(p.out_features) for p in projs], 0), f32, device)
        lw.o_w = pk.dev(sa.o_proj.weight, wd, device)
        if sa.o_proj.bias is not None:
            lw.o_b = pk.dev(sa.o_proj.bias, f32, device)
        lw.ln1_g = pk.dev(layer.input_layernorm.weight, f32, device)
        lw.ln2_g = pk.dev(layer.post_attention_layernorm.weight, f32, device)
        lw.ffn1_w = pk.dev(mlp.gate_proj.weight, wd, device)
        lw.ffn1g_w = pk.dev(mlp.up_proj.weight, wd, device)
        lw.ffn2_w = pk.dev(mlp.down_proj.weight, wd, device)
        if qk_norm is not None:
            qk_norm[i].q_norm_g = pk.dev(sa.q_norm.weight, f32, device)
            qk_norm[i].k_norm_g = pk.dev(sa.k_norm.weight, f32, device)
    pk.layers = layers
    pk.qk_norm = qk_norm
    w.layers_host = C.cast(layers, C.POINTER(N.OmLayerWeights))
    pk.cfg = dict(dtype=code, **fields)
    return pk


def causal2_config(pk_cfg, pooling, normalize):
    """The OmCausalConfig2 of a packed Qwen3 (`_pack_causal`'s cfg dict + the head fields) for one call: the frequencies go into the
    embedded 32 when head_dim is 64, into the struct's own 64 when it is 128."""
    own = ("n_kv_heads", "rope_attention_scaling", "inv_freq", "qk_norm")
    base = N.OmEncoderConfig(pooling=pooling, normalize=int(bool(normalize)), **{k: v for k, v in pk_cfg.items() if k not in own})
    freq = list(pk_cfg["inv_freq"])
    wide = pk_cfg["head_dim"] == 128
    inner = N.OmCausalConfig(base=base, n_kv_heads=pk_cfg["n_kv_heads"], rope_attention_scaling=pk_cfg["rope_attention_scaling"],
                             inv_freq=(C.c_float * 32)(*([0.0] * 32 if wide else freq)))
    return N.OmCausalConfig2(base=inner, qk_norm=int(pk_cfg["qk_norm"]), reserved=0, inv_freq=(C.c_float * 64)(*(freq if wide else [0.0] * 64)))


def causal_config(pk_cfg, pooling, normalize):
    """The OmCausalConfig of a packed Llama / Qwen2 (`_pack_causal`'s cfg dict + the head fields) for one call."""
    own = ("n_kv_heads", "rope_attention_scaling", "inv_freq")
    base = N.OmEncoderConfig(pooling=pooling, normalize=int(bool(normalize)), **{k: v for k, v in pk_cfg.items() if k not in own})
    return N.OmCausalConfig(base=base, n_kv_heads=pk_cfg["n_kv_heads"], rope_attention_scaling=pk_cfg["rope_attention_scaling"],
                            inv_freq=(C.c_float * 32)(*pk_cfg["inv_freq"]))


_PACKERS = {"bert": _pack_bert, "t5": _pack_t5, "modernbert": _pack_modernbert, "causal": _pack_causal, "nomicbert": _pack_nomicbert,
            "gemma3": _pack_gemma3}


def _pack_t5_decoder(model, code, device):
    """Decoder-side weights of a T5Model / T5ForConditionalGeneration for om_t5_decoder_step (one decoder position:
    self-attention needs only v, o; cross-attention k | v fused to [2H, H])."""
    cfg = model.config
    wd = torch_dtype_of(code)
    f32 = torch.float32
    pk = _Packed()
    dec = model.decoder
    # the reference feeds decoder_input_ids = zeros([B, 1]) (dense_retrieval_model.py:138): token 0, whatever the
    # config's decoder_start_token_id says
    w = N.OmT5DecoderWeights()
    w.start_emb = pk.dev(dec.embed_tokens.weight[0], f32, device)
    w.final_ln_g = pk.dev(dec.final_layer_norm.weight, f32, device)
    layers = (N.OmT5DecoderLayer * len(dec.block))()
    gated = bool(getattr(cfg, "is_gated_act", False))
    for i, block in enumerate(dec.block):
        sa, ca, ff, lw = block.layer[0].SelfAttention, block.layer[1].EncDecAttention, block.layer[2].DenseReluDense, layers[i]
        lw.sa_v_w = pk.dev(sa.v.weight, wd, device)
        lw.sa_o_w = pk.dev(sa.o.weight, wd, device)
        lw.sa_ln_g = pk.dev(block.layer[0].layer_norm.weight, f32, device)
        lw.ca_q_w = pk.dev(ca.q.weight, wd, device)
        lw.ca_kv_w = pk.dev(torch.cat([ca.k.weight, ca.v.weight], 0), wd, device, [ca.k.weight, ca.v.weight])
        lw.ca_o_w = pk.dev(ca.o.weight, wd, device)
        lw.ca_ln_g = pk.dev(block.layer[1].layer_norm.weight, f32, device)
        if gated:
            lw.ffn1_w = pk.dev(ff.wi_0.weight, wd, device)
            lw.ffn1g_w = pk.dev(ff.wi_1.weight, wd, device)
        else:
            lw.ffn1_w = pk.dev(ff.wi.weight, wd, device)
        lw.ffn2_w = pk.dev(ff.wo.weight, wd, device)
        lw.ffn_ln_g = pk.dev(block.layer[2].layer_norm.weight, f32, device)
    pk.layers = layers
    w.layers_host = C.cast(layers, C.POINTER(N.OmT5DecoderLayer))
    w.n_layers = len(dec.block)
    pk.weights = w
    return pk


_PACK_CACHE_ATTR = "_openmatch_amd_packed"


class _PackCache(dict):
    """Per-module cache of packed device weights (ctypes structs + device buffers).  It hangs off the module's __dict__,
    so `copy.deepcopy(model)` and `torch.save(model)` meet it: a copy / a pickle gets an EMPTY cache (the weights are
    re-packed on first use) instead of failing on the ctypes pointers."""
    def __deepcopy__(self, memo):
        return _PackCache()

    def __reduce__(self):
        return (_PackCache, ())


def _version_key(model, head):
    mods = [model] + ([head] if head is not None else [])
    return tuple((p.data_ptr(), p._version) for m in mods for p in m.parameters())


def packed_weights(model, head, code, device):
    """Packed weights for (model, head, dtype, device), rebuilt only when a parameter changed."""
    cache = model.__dict__.setdefault(_PACK_CACHE_ATTR, _PackCache())
    key = (code, str(device), id(head))
    ver = _version_key(model, head)
    hit = cache.get(key)
    if hit is not None and hit[0] == ver:
        return hit[1]
    if hit is not None:
        hit[1].retired = True                   # its buffers are no longer anyone's weights: optimizers stop refreshing them
    pk = _PACKERS[_arch_of(model)](model, code, device)
    pk.owner_cache, pk.owner_key = cache, key
    if head is not None:
        lin = head.linear
        pk.weights.head_w = pk.dev(lin.weight, torch.float32, device)
        pk.cfg.update(head_in=lin.in_features, head_out=lin.out_features)
    else:
        pk.cfg.update(head_in=0, head_out=0)
    cache[key] = (ver, pk)
    return pk


def _ensure_folded(pk, device):
    """LayerNorm-folded weights of the fused 16-bit INFERENCE path, once per weight version, in a buffer the packed
    object owns (include/openmatch_hip.h: om_encoder_fold_weights; 0 bytes when the configuration has no fused path).
    Done on first inference use, not at packing time: training repacks every step and never reads them."""
    if getattr(pk, "fold_done", False):
        return
    pk.fold_done = True
    if pk.cfg.get("arch") in (N.ARCH_CAUSAL, N.ARCH_GEMMA3):      # (no fused-norm path: nothing to fold)
        return
    lib = N.lib()
    cfg = N.OmEncoderConfig(pooling=N.POOL_NONE, normalize=0, **pk.cfg)
    nfold = lib.om_encoder_fold_bytes(C.byref(cfg))
    if nfold:
        with torch.cuda.device(device):
            # ONE blob per packed object for its whole life: an optimizer that refreshes the packed copies in place
            # (after_inplace_update) invalidates the fold, and the next inference use folds again INTO THE SAME BUFFER
            # (a fresh blob per step/eval cycle appended to pk.keep grew by ~170 MB per cycle at bert-base)
            blob = getattr(pk, "fold_blob", None)
            if blob is None or blob.numel() < nfold + 256 or blob.device != torch.device(device):
                blob = torch.empty(nfold + 256, dtype=torch.uint8, device=device)
                pk.fold_blob = blob
            ptr = blob.data_ptr() + (-blob.data_ptr()) % 256
            N.check(lib.om_encoder_fold_weights(C.byref(cfg), C.byref(pk.weights), C.c_void_p(ptr), nfold, N.stream_ptr(device)))
        pk.weights.folded = ptr


def after_inplace_update(refreshed, stale):
    """An optimizer rewrote parameters through raw pointers (no version bump).  `refreshed`: packed objects whose copies it
    rewrote in the same pass -- they stay valid, only what was DERIVED from them (LayerNorm-folded inference weights) is
    dropped; `stale`: packed objects it could not refresh -- evicted from their cache, re-packed on next use."""
    for pk in refreshed:
        if getattr(pk, "fold_done", False):
            pk.fold_done = False
            pk.weights.folded = None
    for pk in stale:
        pk.retired = True
        cache, key = getattr(pk, "owner_cache", None), getattr(pk, "owner_key", None)
        if cache is not None and cache.get(key, (None, None))[1] is pk:
            del cache[key]


def invalidate_packed(root):
    """Drop every packed-weight cache under `root` (an nn.Module tree): the next HIP forward re-packs from the parameters.
    For optimizers that update parameters without bumping their version counters (torch's fused AdamW does not) -- the
    cache's freshness test cannot see those updates."""
    for mod in root.modules():
        for attr in (_PACK_CACHE_ATTR, _PACK_CACHE_ATTR + "_dec"):
            cache = mod.__dict__.get(attr)
            if cache:
                for _ver, pk in cache.values():
                    pk.retired = True
                cache.clear()


_TTI_WARNED = set()


def token_types_of(model, items):
    """The batch's token_type_ids, or None.  DistilBERT and MPNet have no token-type table: a batch that carries the ids all the
    same (a BERT tokenizer's habit, and what the reranker's collator emits) has them DROPPED, with one warning per backbone class
    (observable differences)."""
    tti = items.get("token_type_ids") if hasattr(items, "get") else None
    if tti is not None and flavour_of(model) in ("distilbert", "mpnet"):
        name = type(model).__name__
        if name not in _TTI_WARNED:
            _TTI_WARNED.add(name)
            import warnings
            warnings.warn(f"{name} has no token-type embeddings: token_type_ids in the batch are ignored")
        return None
    return tti


_POOL = {None: N.POOL_NONE, "first": N.POOL_FIRST, "mean": N.POOL_MEAN, "last": N.POOL_LAST}


def check_pooling(model, pooling):
    """Unknown values: the reference's ValueError.  "last" (the hidden state of each row's last unmasked token, the usual
    last_token_pool of decoder-only embedders) exists for the causal backbones only."""
    if pooling not in _POOL:
        raise ValueError("Unknown pooling type: {}".format(pooling))
    if pooling == "last" and _arch_of(model) != "causal":
        raise NotImplementedError(f"pooling='last' is served for Llama / Qwen2 / Qwen3 backbones only; {type(model).__name__} pools with 'first' or 'mean'")


def packed_rows_bound(mask):
    """om_encoder_forward_packed's row bound for an attention mask held on the HOST (the collator's output, before it is
    moved to the device): sum over sequences of (1 + index of the last unmasked token; L for an all-masked row),
    rounded up to whole 256-row tiles.  None when packing cannot apply (fewer than 512 rows)."""
    m = mask.cpu() != 0
    L = m.shape[1]
    last = torch.where(m.any(1), L - m.flip(1).to(torch.int8).argmax(1), torch.full((m.shape[0],), L))
    rows = (int(last.sum()) + 255) // 256 * 256
    return rows if rows >= 512 else None


TOKEN_ROWS_KEY = "om_token_rows"      # batch-dict entry (a Python int): the batch's token count as the HOST knows it -- see token_rows_of


def token_rows_of(mask):
    """Per sequence: 1 + index of the last unmasked token (L for an all-masked row), as a HOST int64 tensor [B], for an attention mask
    that still lives on the host -- what the packed-rows entries need to size their row bound without a device synchronisation (the
    sum is the batch's token count; per sequence so that a batch that is split into chunks or merged keeps its counts).  None for a
    device tensor."""
    if not torch.is_tensor(mask) or mask.is_cuda or mask.dim() != 2:
        return None
    m = mask != 0
    L = m.shape[1]
    return torch.where(m.any(1), L - m.flip(1).to(torch.int8).argmax(1), torch.full((m.shape[0],), L)).to(torch.int64)


def rows_bound_of(tokens):
    """Row bound of the packed entries for a token count (an int, or token_rows_of's per-sequence tensor): whole 256-row tiles, None
    below 512 rows."""
    if tokens is None:
        return None
    total = int(tokens.sum()) if torch.is_tensor(tokens) else int(tokens)
    rows = (total + 255) // 256 * 256
    return rows if rows >= 512 else None


LAST_CALL = {}       # what the most recent hip_encode ran on: {"rows": token rows of the contractions, "packed": bool} (tests, bench)


def packed_rows_apply(cfg, B, L, rows, want_hidden, pooling, gated=False):
    """Whether om_encoder_forward_packed takes this call (include/openmatch_hip.h states the same conditions) and pays:
    a 16-bit encoder on its fused path (BERT-family erf-GELU; NomicBERT; T5 without a gated feed-forward), representations only, and
    at least one 256-row tile saved.
    OM_ENCODER_PACKED=0 keeps every batch on the padded entry."""
    if os.environ.get("OM_ENCODER_PACKED", "1") == "0" or want_hidden or pooling is None:
        return False
    if cfg.dtype not in (N.OM_BF16, N.OM_F16) or cfg.hidden % 256 or cfg.ffn % 256 or cfg.n_layers < 1 or L > 1024:
        return False
    if cfg.arch == N.ARCH_BERT and cfg.act != N.ACT_GELU_ERF:
        return False
    if cfg.arch == N.ARCH_T5 and gated:
        return False
    if not (rows % 256 == 0 and 512 <= rows <= (B * L) // 256 * 256 - 256):
        return False
    # the library's own view under the current run-time switches (an A/B switch that takes the fused path away degrades the batch to
    # the padded entry instead of failing the call)
    if not isinstance(cfg, N.OmEncoderConfig):
        cfg = N.OmEncoderConfig(**{f: getattr(cfg, f) for f, _ in N.OmEncoderConfig._fields_ if hasattr(cfg, f)})
    return bool(N.lib().om_encoder_packed_supported(C.byref(cfg), int(bool(gated)), B, L, rows))


def hip_encode(model, items, pooling, head, normalize, code, want_hidden=True, packed_rows=None):
    """(hidden [B,L,H], reps [B,D] f32) through om_encoder_forward.  `items` holds
    input_ids / attention_mask / optional token_type_ids as int64 device tensors.
    packed_rows (with want_hidden=False): run om_encoder_forward_packed (Llama / Qwen2 / Qwen3: om_causal[2]_encoder_forward_packed;
    Gemma3TextModel: om_gemma3_encoder_forward_packed) over
    that many rows (packed_rows_bound of the mask, computed where the mask still lives on the host) instead of B * L padded ones."""
    check_pooling(model, pooling)
    ids = items["input_ids"]
    mask = items["attention_mask"]
    tti = token_types_of(model, items)
    if ids.dim() != 2:
        raise ValueError("input_ids must be [batch, length]")
    ids = ids.to(torch.int64).contiguous()
    mask = mask.to(device=ids.device, dtype=torch.int64).contiguous()
    if tti is not None:
        tti = tti.to(device=ids.device, dtype=torch.int64).contiguous()
    N.require_device(ids, mask, tti)
    check_position_layout(model, ids, mask)
    device = ids.device
    code = inference_code(model, code, ids.shape[1])
    pk = packed_weights(model, head, code, device)
    if _arch_of(model) in ("causal", "gemma3"):
        return _hip_encode_prenorm(pk, ids, mask, pooling, normalize, code, want_hidden, packed_rows)
    _ensure_folded(pk, device)
    cfg = N.OmEncoderConfig(pooling=_POOL[pooling], normalize=int(bool(normalize)), **pk.cfg)
    B, L = ids.shape
    H = cfg.hidden
    D = cfg.head_out if cfg.head_in > 0 else H
    lib = N.lib()
    gated = bool(getattr(getattr(model, "config", None), "is_gated_act", False))
    if packed_rows and not packed_rows_apply(cfg, B, L, int(packed_rows), want_hidden, pooling, gated):
        packed_rows = None
    LAST_CALL.update(rows=int(packed_rows) if packed_rows else B * L, packed=bool(packed_rows))
    with torch.cuda.device(device):
        if packed_rows:
            nbytes = lib.om_encoder_workspace_bytes_packed(C.byref(cfg), B, L, int(packed_rows))
        else:
            nbytes = lib.om_encoder_workspace_bytes(C.byref(cfg), B, L)
        ws_buf, ws_ptr = N.Workspace.get(device, nbytes, "encoder")
        hidden = None
        if want_hidden:
            hidden = torch.empty(B, L, H, device=device,
                                 dtype=torch_dtype_of(code))
        reps = torch.empty(B, D, device=device, dtype=torch.float32) if pooling is not None else None
        if packed_rows:
            N.check(lib.om_encoder_forward_packed(C.byref(cfg), C.byref(pk.weights), N.ptr(ids), N.ptr(mask),
                                                  N.ptr(tti), B, L, int(packed_rows), N.ptr(reps),
                                                  C.c_void_p(ws_ptr), nbytes, N.stream_ptr(device)))
            return None, reps
        N.check(lib.om_encoder_forward(C.byref(cfg), C.byref(pk.weights), N.ptr(ids), N.ptr(mask),
                                       N.ptr(tti), B, L, N.ptr(hidden), N.ptr(reps),
                                       C.c_void_p(ws_ptr), nbytes, N.stream_ptr(device)))
    return hidden, reps


def _prenorm_packed_rows_apply(supported, least, cfg, B, L, rows, want_hidden, pooling):
    """The one rule of the pre-norm stacks' packed entries: representations only, whole 256-row tiles from `least` rows with at least one
    tile saved -- a left-padded batch's bound is B * L, so it stays on the padded entry -- and the library's own view (`supported`: the
    family's om_*_encoder_packed_supported of include/openmatch_hip.h).  OM_ENCODER_PACKED=0 keeps every batch on the padded entry."""
    if os.environ.get("OM_ENCODER_PACKED", "1") == "0" or want_hidden or pooling is None:
        return False
    if not (rows % 256 == 0 and least <= rows <= (B * L) // 256 * 256 - 256):
        return False
    return bool(getattr(N.lib(), supported)(C.byref(cfg), B, L, rows))


def causal_packed_rows_apply(cfg, B, L, rows, want_hidden, pooling):
    """Whether om_causal_encoder_forward_packed (cfg: an OmCausalConfig; an OmCausalConfig2: the om_causal2_* entry) takes this call and
    pays: from 512 rows."""
    v2 = "2" if isinstance(cfg, N.OmCausalConfig2) else ""
    return _prenorm_packed_rows_apply(f"om_causal{v2}_encoder_packed_supported", 512, cfg, B, L, rows, want_hidden, pooling)


def gemma3_packed_rows_apply(cfg, B, L, rows, want_hidden, pooling):
    """Whether om_gemma3_encoder_forward_packed (cfg: an OmGemma3Config) takes this call and pays: above the few-rows threshold."""
    least = N.lib().om_debug_option_value(N.OPT_GEMM_SKINNY_M) + 1
    return _prenorm_packed_rows_apply("om_gemma3_encoder_packed_supported", least, cfg, B, L, rows, want_hidden, pooling)


# The f32-residual pre-norm families (csrc/prenorm_stack.h): the config builder, the prefix of the four entries (om_<prefix>_encoder_
# workspace_bytes[_packed] / _forward[_packed]), the packed-rows rule, and the per-layer array its forward takes after the weights (the
# packer's attribute and the array's element type)
_PRENORM = {
    "causal": (causal_config, "om_causal", causal_packed_rows_apply, None),
    "causal2": (causal2_config, "om_causal2", causal_packed_rows_apply, ("qk_norm", N.OmCausalQkNorm)),
    "gemma3": (gemma3_config, "om_gemma3", gemma3_packed_rows_apply, ("norms", N.OmGemma3Norms)),
}


def _hip_encode_prenorm(pk, ids, mask, pooling, normalize, code, want_hidden, packed_rows=None):
    """hip_encode for a packed Llama / Qwen2, Qwen3 (its cfg carries qk_norm) or Gemma3TextModel (sliding_layers): the family's
    _forward_packed entry over `packed_rows` rows where its rule admits the call, its _forward entry over the B * L padded rows otherwise."""
    family = "gemma3" if "sliding_layers" in pk.cfg else "causal2" if "qk_norm" in pk.cfg else "causal"
    make_config, prefix, rows_apply, per_layer = _PRENORM[family]
    device = ids.device
    cfg = make_config(pk.cfg, _POOL[pooling], normalize)
    B, L = ids.shape
    base = cfg.base
    while not isinstance(base, N.OmEncoderConfig):
        base = base.base
    H = base.hidden
    D = base.head_out if base.head_in > 0 else H
    lib = N.lib()
    extra = ()
    if per_layer is not None:
        array, struct = getattr(pk, per_layer[0]), per_layer[1]
        extra = (C.cast(array, C.POINTER(struct)) if array is not None and len(array) else None,)
    if packed_rows and not rows_apply(cfg, B, L, int(packed_rows), want_hidden, pooling):
        packed_rows = None
    LAST_CALL.update(rows=int(packed_rows) if packed_rows else B * L, packed=bool(packed_rows))
    rows = (int(packed_rows),) if packed_rows else ()
    suffix = "_packed" if packed_rows else ""
    with torch.cuda.device(device):
        reps = torch.empty(B, D, device=device, dtype=torch.float32) if pooling is not None else None
        hidden = torch.empty(B, L, H, device=device, dtype=torch_dtype_of(code)) if want_hidden else None      # (never with packed rows: the rule)
        nbytes = getattr(lib, f"{prefix}_encoder_workspace_bytes{suffix}")(C.byref(cfg), B, L, *rows)
        if not nbytes:
            raise N.NativeError(lib.om_last_error().decode("utf-8", "replace"))
        ws_buf, ws_ptr = N.Workspace.get(device, nbytes, "encoder")
        out = (N.ptr(reps),) if packed_rows else (N.ptr(hidden), N.ptr(reps))
        N.check(getattr(lib, f"{prefix}_encoder_forward{suffix}")(C.byref(cfg), C.byref(pk.weights), *extra, N.ptr(ids), N.ptr(mask), B, L, *rows, *out,
                                                                  C.c_void_p(ws_ptr), nbytes, N.stream_ptr(device)))
    return hidden, reps


def packed_decoder_weights(model, code, device):
    """Packed decoder-side weights for (model, dtype, device), rebuilt only when a parameter changed."""
    cache = model.__dict__.setdefault(_PACK_CACHE_ATTR + "_dec", _PackCache())
    key = (code, str(device))
    ver = _version_key(model, None)
    hit = cache.get(key)
    if hit is None or hit[0] != ver:
        if hit is not None:
            hit[1].retired = True
        hit = (ver, _pack_t5_decoder(model, code, device))
        hit[1].owner_cache, hit[1].owner_key = cache, key
        cache[key] = hit
    return hit[1]


def hip_t5_decoder_step(model, items, code):
    """Decoder hidden state [B, H] (f32) of a T5 encoder-decoder after ONE decoder position fed token 0 -- the
    reference's `model(**items, decoder_input_ids=zeros([B, 1])).last_hidden_state[:, 0]`
    (modeling/dense_retrieval_model.py:137-141).  Encoder through om_encoder_forward, decoder through om_t5_decoder_step."""
    if not hasattr(model, "decoder") or not hasattr(model, "encoder"):
        raise ValueError("an encoder-decoder T5 model is required")
    code = inference_code(model, code, 0)  # float16 where the T5 stack takes it (round 6: the decoder position too), else bfloat16
    enc_hidden, _ = hip_encode(model, items, None, None, False, code, want_hidden=True)
    device = enc_hidden.device
    mask = items["attention_mask"].to(device=device, dtype=torch.int64).contiguous()
    dpk = packed_decoder_weights(model, code, device)
    epk = packed_weights(model, None, code, device)
    cfg = N.OmEncoderConfig(pooling=N.POOL_NONE, normalize=0, **epk.cfg)
    B, L = mask.shape
    lib = N.lib()
    with torch.cuda.device(device):
        nbytes = lib.om_t5_decoder_workspace_bytes(C.byref(cfg), B, L)
        _buf, ws_ptr = N.Workspace.get(device, nbytes, "decoder")
        out = torch.empty(B, cfg.hidden, device=device, dtype=torch.float32)
        N.check(lib.om_t5_decoder_step(C.byref(cfg), C.byref(dpk.weights), N.ptr(enc_hidden), N.ptr(mask), B, L,
                                       N.ptr(out), C.c_void_p(ws_ptr), nbytes, N.stream_ptr(device)))
    return out


class _LinearF32(torch.autograd.Function):
    """y = x W^T in f32 with its backward on the device (om_gemm_nt / om_linear_f32_backward): the LinearHead and the two
    LM-head rows of monoT5 behind the T5 decoder position when it is trained."""
    @staticmethod
    def forward(ctx, x, weight):
        x32 = x.to(torch.float32).contiguous()
        w32 = weight.to(device=x.device, dtype=torch.float32).contiguous()
        ctx.save_for_backward(x32, w32)
        return hip_linear_f32(x32, w32)

    @staticmethod
    def backward(ctx, dy):
        x32, w32 = ctx.saved_tensors
        dy = dy.to(torch.float32).contiguous()
        dx = torch.empty_like(x32)
        dw = torch.zeros_like(w32)
        with torch.cuda.device(x32.device):
            N.check(N.lib().om_linear_f32_backward(N.ptr(dy), N.ptr(x32), N.ptr(w32), N.ptr(dw), N.ptr(dx), x32.shape[0],
                                                  w32.shape[0], x32.shape[1], N.stream_ptr(x32.device)))
        return dx, dw


def hip_linear_f32_autograd(x, weight):
    return _LinearF32.apply(x, weight)


def hip_linear_f32(x, weight):
    """x [B, K] f32 @ weight[N, K]^T on the device through om_gemm_nt (LinearHead / LM-head columns)."""
    x = x.to(torch.float32).contiguous()
    w = weight.detach().to(device=x.device, dtype=torch.float32).contiguous()
    out = torch.empty(x.shape[0], w.shape[0], device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        N.check(N.lib().om_gemm_nt(N.OM_F32, N.ptr(x), x.shape[1], N.ptr(w), w.shape[1], N.OM_F32, N.ptr(out), w.shape[0],
                                   x.shape[0], w.shape[0], x.shape[1], None, None, 0, 0, N.stream_ptr(x.device)))
    return out
