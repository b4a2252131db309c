"""The BERT-family backbones the post-LayerNorm HIP stack (OM_ARCH_BERT) serves, behind one accessor.

BERT / RoBERTa, DistilBERT and MPNet compute the same stack -- embeddings + LayerNorm, then per layer
`x1 = LN(x + o(attn(x)))`, `x' = LN(x1 + ffn2(gelu(ffn1(x1))))` -- under different module names, and differ in two options the
device side takes: a token-type table (BERT, RoBERTa) or none, and a relative-position bias shared by all layers (MPNet) or
none.  `bert_parts(model)` names the modules once; the packer (encoder.py), the training parameter order and the gradient
write-back (train.py) read them from here and never spell `encoder.layer[i].attention.self.query` themselves.  The HF modules
stay the owners of every parameter, so `state_dict()` / `save_pretrained()` keep each backbone's own checkpoint layout.
"""
from collections import namedtuple

# q, k, v, o, ffn1, ffn2: nn.Linear with bias; ln1 (after attention), ln2 (after the feed-forward): nn.LayerNorm
LayerParts = namedtuple("LayerParts", "q k v o ln1 ffn1 ffn2 ln2")
# word / pos / type: nn.Embedding (type: None where the backbone has no token types); emb_ln: nn.LayerNorm; rel_bias: nn.Embedding
# [buckets, heads] or None; rel_buckets / rel_max_dist: T5's bidirectional bucket rule (0, 0 without a table)
BertParts = namedtuple("BertParts", "word pos type emb_ln layers eps rel_bias rel_buckets rel_max_dist act "
                                    "hidden hidden_layers heads ffn vocab max_pos type_vocab")

# class name -> flavour.  Explicit: a class that merely has "Bert" in its name (ALBERT's shared layers and factorised embedding,
# MobileBERT's bottlenecks, SqueezeBERT's convolutions, ...) has another layout and is refused by name (encoder._arch_of).
FLAVOURS = {
    "BertModel": "bert",
    "RobertaModel": "roberta", "XLMRobertaModel": "roberta",
    "DistilBertModel": "distilbert",
    "MPNetModel": "mpnet",
}

MPNET_MAX_DISTANCE = 128      # HF:models/mpnet/modeling_mpnet.py relative_position_bucket(max_distance=128): not a config field


def flavour_of(model):
    """"bert" | "roberta" | "distilbert" | "mpnet", or None for a class this layer does not know."""
    # the class or any of its bases by name: a subclass of a served backbone keeps its layout, whichever family it is
    for cls in type(model).__mro__:
        if cls.__name__ in FLAVOURS:
            return FLAVOURS[cls.__name__]
    # renamed copies of the two original families keep the layout they always had here
    name = type(model).__name__
    if name.startswith("Bert"):
        return "bert"
    if "Roberta" in name:
        return "roberta"
    return None


def _act_name(a):
    return a if isinstance(a, str) else "gelu"


def bert_parts(model):
    """BertParts of a BERT-family HF module (see the module docstring)."""
    fl = flavour_of(model)
    cfg = model.config
    emb = model.embeddings
    if fl in ("bert", "roberta"):
        if getattr(cfg, "position_embedding_type", "absolute") != "absolute":
            raise NotImplementedError("only absolute position embeddings are supported")
        layers = [LayerParts(l.attention.self.query, l.attention.self.key, l.attention.self.value, l.attention.output.dense,
                             l.attention.output.LayerNorm, l.intermediate.dense, l.output.dense, l.output.LayerNorm)
                  for l in model.encoder.layer]
        return BertParts(emb.word_embeddings, emb.position_embeddings, emb.token_type_embeddings, emb.LayerNorm, layers,
                         float(cfg.layer_norm_eps), None, 0, 0, _act_name(cfg.hidden_act), cfg.hidden_size, cfg.num_hidden_layers,
                         cfg.num_attention_heads, cfg.intermediate_size, cfg.vocab_size, cfg.max_position_embeddings,
                         cfg.type_vocab_size)
    if fl == "distilbert":
        # sinusoidal_pos_embds only changes how the table is initialised: it is a parameter either way
        layers = [LayerParts(l.attention.q_lin, l.attention.k_lin, l.attention.v_lin, l.attention.out_lin, l.sa_layer_norm,
                             l.ffn.lin1, l.ffn.lin2, l.output_layer_norm) for l in model.transformer.layer]
        return BertParts(emb.word_embeddings, emb.position_embeddings, None, emb.LayerNorm, layers, float(emb.LayerNorm.eps),
                         None, 0, 0, _act_name(cfg.activation), cfg.dim, cfg.n_layers, cfg.n_heads, cfg.hidden_dim, cfg.vocab_size,
                         cfg.max_position_embeddings, 0)
    if fl == "mpnet":
        layers = [LayerParts(l.attention.attn.q, l.attention.attn.k, l.attention.attn.v, l.attention.attn.o, l.attention.LayerNorm,
                             l.intermediate.dense, l.output.dense, l.output.LayerNorm) for l in model.encoder.layer]
        return BertParts(emb.word_embeddings, emb.position_embeddings, None, emb.LayerNorm, layers, float(cfg.layer_norm_eps),
                         model.encoder.relative_attention_bias, int(cfg.relative_attention_num_buckets), MPNET_MAX_DISTANCE,
                         _act_name(cfg.hidden_act), cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                         cfg.intermediate_size, cfg.vocab_size, cfg.max_position_embeddings, 0)
    raise NotImplementedError(f"no BERT-family accessor for {type(model).__name__}")


def dropout_probs(model):
    """(hidden dropout, attention dropout) of a BERT-family module's config, whatever the backbone calls them -- the one place
    that knows (train.encode_train and DRModel.encode both ask here)."""
    cfg = model.config
    if flavour_of(model) == "distilbert":
        return float(cfg.dropout), float(cfg.attention_dropout)
    return float(cfg.hidden_dropout_prob), float(cfg.attention_probs_dropout_prob)
