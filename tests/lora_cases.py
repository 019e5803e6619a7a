"""Seeded LoRA adapters and the plain-torch LoRA rule shared by tests/golden/make_golden_lora.py and the tests that read its fixture
(tests/golden/lora*.npz).  The adapters regenerate bit-exactly from the seed (torch CPU generator), so the fixture stores results only.

The rule is peft's `base(x) + s * B(A(drop(x)))`, wrapped around the seven Linears of every HuggingFace LlamaDecoderLayer in plain torch
(peft itself is not needed).  B is seeded NON-ZERO: a zero B makes every dA vanish and would hide any error in it."""
import torch
import torch.nn as nn
import torch.nn.functional as F

TARGETS = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")

FP32_CASES = ("tiny_left", "gqa_tiny_left", "dh128", "mqa_dh128_left")      # of llama_bwd_cases.LLAMA_CASES, r = 16
LOW_CASES = ("dh128", "mqa_dh128_left")                                      # 16-bit drift, r = 64
R32, R16 = 16, 64
SCALING = 2.0                                                                # lora_alpha = 2 r, the reference's ratio (256 / 128)


def shapes(lc):
    D, Fd, kv = lc.hidden_size, lc.intermediate_size, lc.num_key_value_heads * lc.head_dim
    return {"q_proj": (D, D), "k_proj": (kv, D), "v_proj": (kv, D), "o_proj": (D, D), "gate_proj": (Fd, D), "up_proj": (Fd, D),
            "down_proj": (D, Fd)}                                            # (out, in)


def adapters(lc, r, seed, targets=TARGETS):
    """{"{layer}.{target}.lora_A": (r, in), "....lora_B": (out, r)}: A uniform in +-1 / sqrt(in) (peft's init), B normal with sigma 0.05."""
    g = torch.Generator().manual_seed(7000 + seed)
    out = {}
    for i in range(lc.num_hidden_layers):
        for t in TARGETS:
            o, ii = shapes(lc)[t]
            A = (torch.rand(r, ii, generator=g) * 2 - 1) / ii ** 0.5
            B = torch.randn(o, r, generator=g) * 0.05
            if t in targets:
                out[f"{i}.{t}.lora_A"], out[f"{i}.{t}.lora_B"] = A, B
    return out


def peft_keys(ad):
    """The adapters under the adapter-file keys `load_lora_state_dict` takes."""
    sd = {}
    for k, v in ad.items():
        i, t, which = k.split(".")
        sd[f"base_model.model.model.layers.{i}.{'self_attn' if t in ATTN else 'mlp'}.{t}.{which}.weight"] = v
    return sd


class LoraLinear(nn.Module):
    """base(x) + s * B(A(drop(x))).  `mask`: None, or the dropout mask of this projection's input, (rows, in) of 0 / 1, applied as
    x * mask / (1 - p)."""

    def __init__(self, base, A, B, s, mask=None, p=0.0):
        super().__init__()
        self.base, self.s, self.mask, self.p = base, s, mask, p
        self.lora_A, self.lora_B = nn.Parameter(A.clone()), nn.Parameter(B.clone())

    def forward(self, x):
        xd = x
        if self.mask is not None:
            xd = x * (self.mask.reshape(x.shape).to(x.dtype) / (1.0 - self.p))
        return self.base(x) + F.linear(F.linear(xd, self.lora_A), self.lora_B) * self.s


def wrap_hf(m, ad, s, dtype, masks=None, p=0.0):
    """Put a LoraLinear around the targeted Linears of HF LlamaForCausalLM `m` (frozen).  Returns {"{layer}.{target}": LoraLinear}."""
    wrapped = {}
    for k in ad:
        i, t, which = k.split(".")
        if which != "lora_A":
            continue
        parent = getattr(m.model.layers[int(i)], "self_attn" if t in ATTN else "mlp")
        mod = LoraLinear(getattr(parent, t), ad[k].to(dtype), ad[f"{i}.{t}.lora_B"].to(dtype), s, None if masks is None else masks[f"{i}.{t}"], p)
        setattr(parent, t, mod)
        wrapped[f"{i}.{t}"] = mod
    return wrapped


def cat_grads(grads, which):
    """Every gradient whose name ends with `which` ("lora_A" / "lora_B"), flattened and concatenated in sorted-name order."""
    return torch.cat([v.reshape(-1) for k, v in sorted(grads.items()) if k.endswith(which)])


def hf_llama(kw, lc, sd, dtype=torch.float32):
    """HuggingFace LlamaForCausalLM with eager attention on the state dict `sd`, every parameter frozen (make_golden_llama_bwd.py builds it the
    same way)."""
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(**kw, rms_norm_eps=lc.rms_norm_eps, rope_theta=lc.rope_theta, attention_bias=False, mlp_bias=False, tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    with torch.device("meta"):
        m = LlamaForCausalLM(cfg)
    m = m.to_empty(device="cpu").eval()
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True, assign=True)
    inv = 1.0 / (lc.rope_theta ** (torch.arange(0, lc.head_dim, 2, dtype=torch.int64).float() / lc.head_dim))      # (non-persistent buffer: rebuilt as HF does)
    m.model.rotary_emb.inv_freq = inv
    if hasattr(m.model.rotary_emb, "original_inv_freq"):
        m.model.rotary_emb.original_inv_freq = inv
    return m.requires_grad_(False)


def additive_mask(am, dtype):
    """The (B, 1, T, T) causal + key-padding mask HF's Llama takes as it is, filled with float32's lowest value whatever `dtype`: the eager
    attention takes its softmax in float32, where float64's lowest value is -inf and a padded query's row of scores would become NaN."""
    B, T = am.shape
    allow = torch.tril(torch.ones(T, T, dtype=torch.bool))[None, None] & am.bool()[:, None, None, :]
    return torch.zeros(B, 1, T, T, dtype=dtype).masked_fill(~allow, torch.finfo(torch.float32).min)


def lm_loss(logits, labels, am):
    """The shifted cross entropy of the reference's forward over the counted positions (setokim_llama.py:145-160), in the logits' precision
    promoted to fp32 at least."""
    lg = logits if logits.dtype == torch.float64 else logits.float()
    keep = am[:, 1:] != 0
    return F.cross_entropy(lg[:, :-1][keep], labels[:, 1:][keep], ignore_index=-100)
