"""LLM prefill of BASELINE config 5 on the HIP library: what `SetokimLlamaForCausalLM.forward`
(src/model/language_model/setokim_llama.py:94-143) runs after `prepare_inputs_labels_for_multimodal` —

    outputs = self.model(attention_mask=..., position_ids=..., inputs_embeds=...)      # HF LlamaModel      :130-139
    logits  = self.lm_head(outputs[0])                                                 #                    :143

`self.model` is HuggingFace `transformers` LlamaModel (third-party code; Vicuna-7B = 32 layers, hidden 4096, 32 heads of 128, SwiGLU
11008, RMSNorm, rotary embeddings).  This module holds the same parameters under the same state-dict names
(`model.embed_tokens.weight`, `model.layers.{i}.self_attn.{q,k,v,o}_proj.weight`, `model.layers.{i}.mlp.{gate,up,down}_proj.weight`,
`model.layers.{i}.{input,post_attention}_layernorm.weight`, `model.norm.weight`, `lm_head.weight`) so a Vicuna / Llama-2 checkpoint loads
unchanged, and runs the prefill (no KV cache, eager-attention arithmetic) as: RMSNorm -> one fused q|k|v GEMM -> rotary embedding in place
-> causal + padding-masked MFMA attention -> o_proj GEMM with the residual fused -> RMSNorm -> one fused gate|up GEMM -> SwiGLU ->
down_proj GEMM with the residual fused.  The LLM's own weights get no gradient here (training them is the reference's HF-Trainer side); with the
decoder stack FROZEN the forward is differentiable with respect to `inputs_embeds` (llama_train.py, autograd.LlamaFn / LlamaLMFn): the
reference's stage 2, which trains mm_in_projector through the language-model loss.  Grouped-query attention (num_key_value_heads < num_attention_heads: Llama-2-70B,
Llama-3, Mistral — Vicuna-7B / 13B do not use it) runs on the same kernels: the fused q|k|v rows are [H | Hkv | Hkv] heads wide and query head h
reads key / value head h // (H // Hkv), HF's `repeat_kv` without the copies.

Generation (`SetokimLlamaForCausalLM.generate`, setokim_llama.py:329-396) is greedy decoding with a KV cache: `LlamaModel.prefill` is the same
prefill that also fills a `generation.KVCache`, `LlamaModel.decode_step` runs one token per sequence against it (csrc/attn_decode.hip), and
`SetokimLlamaPrefill.generate` calls the parts of the loop, which live in generation.py.  The three entry points run the stack through
one layer loop, `LlamaModel._run_layers`, and differ in its attention step.  `LlamaModel.extend` adds Tn >= 1 tokens per sequence to a cache that already holds
some (csrc/attn_extend.hip): `generate(prefill_chunk=)` feeds a prompt in windows through it and `generate(past=)` continues a conversation from the
state an earlier call returned.

Fine-tuning (the reference's scripts/finetune.sh: LoRA on every decoder Linear): `add_lora_` attaches adapters (lora.py) and freezes the stack; with
them `forward` is differentiable with respect to `inputs_embeds` AND the adapters (autograd.LlamaLoraFn / LlamaLoraLMFn), `merge_lora_` folds them
into the weights, and the KV-cached entry points refuse unmerged adapters.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn as nn

from . import autograd, lora, ops
from ._packcache import PackCacheMixin
from .arch import SetokimVisionMixin, config_get
from .lora import ALL_SEVEN


class _WeightFormat(NamedTuple):
    """A quantised storage format of the decoder stack: what `LlamaModel` needs to know of it (the kernels: csrc/wstream.h and the format's file)."""
    weight_format: str                                   # LlamaModel.weight_format
    tag: str                                             # the short name in messages and in quantize_<tag>_
    quantize: Callable                                   # w (N, K) -> the stored pair
    dequantize: Callable                                 # (*pair, out=) -> w' (N, K)
    linear: Callable                                     # the weight-streaming GEMM on a pair ...
    max_m: int                                           # ... and the rows it takes; more dequantise and go through ops.linear
    shape: Callable                                      # pair -> (N, K)
    k_granule: Optional[Callable] = None                 # dtype -> the in_features granule quantize_ insists on (None: any K)


_FP8 = _WeightFormat("fp8_e4m3", "fp8", ops.quantize_fp8_rows, ops.dequantize_fp8_rows, ops.linear_fp8w, ops.FP8W_MAX_M,
                     shape=lambda pair: tuple(pair[0].shape))                  # (no granule: the prefill works at any K through the dequantise path)
_MXFP4 = _WeightFormat("mxfp4_e2m1", "mxfp4", ops.quantize_mxfp4_rows, ops.dequantize_mxfp4_rows, ops.linear_mxfp4w, ops.MXFP4W_MAX_M,
                       shape=lambda pair: (pair[0].shape[0], 2 * pair[0].shape[1]),
                       k_granule=lambda dtype: 32 if dtype == torch.float32 else 128)


class _RMSNorm(nn.Module):
    def __init__(self, dim, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.variance_epsilon = eps


class _Attention(nn.Module):
    def __init__(self, D, H, Hkv):
        super().__init__()
        dh = D // H
        self.q_proj = nn.Linear(D, H * dh, bias=False)
        self.k_proj = nn.Linear(D, Hkv * dh, bias=False)
        self.v_proj = nn.Linear(D, Hkv * dh, bias=False)
        self.o_proj = nn.Linear(H * dh, D, bias=False)


class _MLP(nn.Module):
    def __init__(self, D, F):
        super().__init__()
        self.gate_proj = nn.Linear(D, F, bias=False)
        self.up_proj = nn.Linear(D, F, bias=False)
        self.down_proj = nn.Linear(F, D, bias=False)


class _DecoderLayer(nn.Module):
    def __init__(self, D, H, Hkv, F, eps):
        super().__init__()
        self.self_attn = _Attention(D, H, Hkv)
        self.mlp = _MLP(D, F)
        self.input_layernorm = _RMSNorm(D, eps)
        self.post_attention_layernorm = _RMSNorm(D, eps)


class LlamaModel(PackCacheMixin, nn.Module):
    """Parameter container with HF LlamaModel's tree + the prefill on the HIP library."""

    def __init__(self, vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads, num_key_value_heads, rms_norm_eps,
                 rope_theta):
        super().__init__()
        if num_key_value_heads < 1 or num_attention_heads % num_key_value_heads != 0:
            raise ValueError(f"num_attention_heads ({num_attention_heads}) must be a multiple of num_key_value_heads ({num_key_value_heads})")
        self.num_heads, self.head_dim, self.rope_theta, self.eps = num_attention_heads, hidden_size // num_attention_heads, rope_theta, rms_norm_eps
        self.num_kv_heads = num_key_value_heads
        self.embed_tokens = nn.Embedding(vocab_size, hidden_size)
        self.layers = nn.ModuleList([_DecoderLayer(hidden_size, num_attention_heads, num_key_value_heads, intermediate_size, rms_norm_eps)
                                     for _ in range(num_hidden_layers)])
        self.norm = _RMSNorm(hidden_size, rms_norm_eps)
        self._init_pack_cache()
        self._quant = None                                                      # quantize_fp8_() / quantize_mxfp4_(): the packed stack in that storage, with its _WeightFormat
        self.lora = None                                                        # add_lora_(): a lora.LoraAdapters, outside self.layers

    # ---- LoRA adapters (lora.py; the arithmetic is llama_train.llama_lora_forward_train / llama_lora_backward) ---------------------------------
    def add_lora_(self, r: int, lora_alpha: float, target_modules=ALL_SEVEN, lora_dropout: float = 0.0):
        """Attach LoRA adapters to the targeted projections of every decoder layer (the reference's finetune stage: peft's LoraConfig over all
        seven Linears, r = 128, lora_alpha = 256, dropout 0.05): per projection `lora_A` (r, in), Kaiming-uniform with a = sqrt(5), and `lora_B`
        (out, r), zero, in the model's element type and on its device, kept in `self.lora`; the scaling is lora_alpha / r.  `layers.*` and `norm`
        are frozen.  A fresh adapter changes no bit of the forward.  Refused by name: r off the GEMM's K granule (64 in the 16-bit types, 16 in
        fp32) or above 128, an unknown target, a second call, a stack in fp8 storage.  Call it on the device and in the dtype the model trains in."""
        targets = lora.check_request(self, r, lora_alpha, target_modules, lora_dropout)
        self.lora = lora.LoraAdapters(self, r, lora_alpha, targets, lora_dropout)
        self.layers.requires_grad_(False)
        self.norm.requires_grad_(False)
        return self

    def _need_lora(self, what: str):
        if self.lora is None:
            raise ValueError(f"LlamaModel.{what}: no adapters are attached (add_lora_ first)")
        return self.lora

    def _refuse_unmerged(self, what: str) -> None:
        if self.lora is not None:
            raise NotImplementedError(f"{what}: LoRA adapters are attached and the inference kernels read the base weights only; call merge_lora_() "
                                      "first (forward() applies unmerged adapters)")

    def lora_state_dict(self):
        """The adapters under peft's adapter-file keys (lora.state_dict_of: `base_model.model.model.layers.{i}.self_attn.q_proj.lora_A.weight`, ...).
        The format follows the reference's save and load code and is not checked against a peft-written file."""
        return lora.state_dict_of(self._need_lora("lora_state_dict"))

    def load_lora_state_dict(self, sd) -> None:
        """Load what lora_state_dict wrote; the `.lora_A.default.weight` spelling of an in-memory PeftModel is accepted too."""
        lora.load_state_dict_into(self._need_lora("load_lora_state_dict"), sd)

    @torch.no_grad()
    def merge_lora_(self):
        """W <- W + (lora_alpha / r) B A for every adapted projection, formed in fp32 and rounded once; the adapters are then removed (peft's
        merge_and_unload).  The packed copies rebuild through their version key."""
        self._need_lora("merge_lora_")
        lora.merge_into(self)
        self.lora = None
        return self

    def _stack_and_embed_parameters(self):
        """Every parameter but the adapters': what the packed copies are built from."""
        return [p for n, p in self.named_parameters() if not n.startswith("lora.")]

    @property
    def weight_format(self) -> str:
        """"native" (the Linear weights in the model's element type), "fp8_e4m3" after quantize_fp8_() or "mxfp4_e2m1" after quantize_mxfp4_()."""
        return "native" if self._quant is None else self._quant["fmt"].weight_format

    @torch.no_grad()
    def quantize_fp8_(self, free_master: bool = True):
        """Store the stack's projection weights as e4m3fn bytes with one power-of-two exponent per output row (include/setok_hip.h, "FP8
        weight-only decode"): the four fused operands `_pack` builds per layer — q|k|v, o, pair-interleaved gate|up, down — quantised on the device,
        one layer at a time.  Rows are independent, so quantising a fused matrix equals quantising its parts.  embed_tokens, the norms and
        lm_head stay as they are.  The model then IS the Llama whose weights are W' = value(q) * 2^e (exactly representable in the element
        type): `_forward` / `prefill` dequantise each matrix into one reusable scratch buffer and run the existing kernels on it,
        `decode_step` streams the bytes through `ops.linear_fp8w`.  With `free_master` the Linear parameters release their storage (N * K + N
        bytes per matrix remain) and `state_dict()` is refused; without it the masters stay for `state_dict()` only — the fp8 copy computes, and an
        in-place update of any stack parameter afterwards is refused at the next forward instead of being silently ignored.  Call it on the device and in the dtype the model will run in.  Inference only."""
        return self._quantize_(_FP8, free_master)

    @torch.no_grad()
    def quantize_mxfp4_(self, free_master: bool = True):
        """Store the stack's projection weights in OCP MXFP4 (include/setok_hip.h, "MXFP4 weight-only decode"): e2m1 nibbles with one e8m0
        power-of-two scale per 32 elements of a row, for the same four fused operands per layer as `quantize_fp8_`, quantised on the device one layer
        at a time.  Blocks lie along K inside a row, so fused rows stay independent.  embed_tokens, the norms and lm_head stay.  The model then
        IS the Llama whose weights are W' = value(nibble) * 2^(s - 127), exactly representable in the element type: `_forward` / `prefill`
        dequantise each matrix into one reusable scratch buffer and run the existing kernels, `decode_step` and `extend` stream the nibbles through
        `ops.linear_mxfp4w` up to 64 rows.  With `free_master` the Linear parameters release their storage (N * K / 2 + N * K / 32 bytes per matrix
        remain) and `state_dict()` is refused.  Refused before anything is freed: a hidden or intermediate size off the streaming GEMM's K granule
        (128 in the 16-bit types, 32 in fp32; ValueError naming the matrix), a stack already quantised, unmerged adapters.  Inference only."""
        return self._quantize_(_MXFP4, free_master)

    def _quantize_(self, fmt: _WeightFormat, free_master: bool):
        what = f"LlamaModel.quantize_{fmt.tag}_"
        self._refuse_unmerged(what)
        if self._quant is not None:
            raise NotImplementedError(f"{what}: the stack is already in {self._quant['fmt'].tag} storage and its masters may be gone (a second "
                                      "quantisation would re-round it)")
        f32 = lambda t: t.detach().float().contiguous()
        w0 = self.norm.weight
        lins = lambda l: (("self_attn.q_proj", l.self_attn.q_proj), ("self_attn.k_proj", l.self_attn.k_proj), ("self_attn.v_proj", l.self_attn.v_proj),
                          ("self_attn.o_proj", l.self_attn.o_proj), ("mlp.gate_proj", l.mlp.gate_proj), ("mlp.up_proj", l.mlp.up_proj),
                          ("mlp.down_proj", l.mlp.down_proj))
        if fmt.k_granule is not None:
            gran = fmt.k_granule(w0.dtype)
            for li, l in enumerate(self.layers):
                for name, lin in lins(l):
                    K = lin.weight.shape[1]
                    if K % gran != 0:
                        raise ValueError(f"{what}: layers.{li}.{name} has in_features={K}, not a multiple of {gran} (the K granule of the {fmt.tag} "
                                         f"streaming GEMM in {w0.dtype}); nothing was quantised")
        if not w0.is_cuda:
            raise NotImplementedError(f"{what}: the {fmt.tag} quantiser runs on the device; move the model there first")
        layers, largest = [], 0
        for l in self.layers:
            a, m = l.self_attn, l.mlp
            fused = dict(wqkv=torch.cat([a.q_proj.weight, a.k_proj.weight, a.v_proj.weight], 0), wo=a.o_proj.weight.contiguous(),
                         wgu=ops.interleave_gate_up(m.gate_proj.weight, m.up_proj.weight), wd=m.down_proj.weight.contiguous())
            L = dict(n1=f32(l.input_layernorm.weight), n2=f32(l.post_attention_layernorm.weight))
            for k, w in fused.items():
                L[k] = fmt.quantize(w)
                largest = max(largest, w.numel())
            layers.append(L)
            del fused
            if free_master:
                for _, lin in lins(l):
                    lin.weight.requires_grad_(False)
                    lin.weight.data = torch.empty(0, dtype=w0.dtype, device=w0.device)
        self._quant = dict(fmt=fmt, key=(w0.dtype, str(w0.device)), layers=layers, norm=f32(self.norm.weight), largest=largest, scratch=None,
                           freed=bool(free_master), versions=self._versions(self._stack_and_embed_parameters()))
        self._packed = {}
        return self

    def state_dict(self, *args, **kwargs):
        if self._quant is not None and self._quant["freed"]:
            tag = self._quant["fmt"].tag
            raise NotImplementedError(f"LlamaModel.state_dict: the Linear weights were released by quantize_{tag}_(free_master=True); saving "
                                      f"a stack in {tag} storage is not implemented (quantise with free_master=False to keep the masters)")
        return super().state_dict(*args, **kwargs)

    def _w(self, w):
        """A quantised operand - a (q, e) or (q, s) pair - as `linear` takes it: dequantised into the one scratch buffer (stream order makes the
        reuse safe: the GEMM that reads it is enqueued before the next dequantisation)."""
        f = self._quant
        if f["scratch"] is None:
            f["scratch"] = torch.empty(f["largest"], dtype=f["key"][0], device=self.norm.weight.device)
        N, K = f["fmt"].shape(w)
        return f["fmt"].dequantize(*w, out=f["scratch"][:N * K].view(N, K))

    def _pack(self):
        w = self.norm.weight
        if self._quant is not None:
            tag = self._quant["fmt"].tag
            if self._quant["key"] != (w.dtype, str(w.device)):
                raise NotImplementedError(f"LlamaModel: the stack was quantised to {tag} as {self._quant['key']} and cannot follow a move to "
                                          f"{(w.dtype, str(w.device))}")
            if self._versions(self._stack_and_embed_parameters()) != self._quant["versions"]:
                # (free_master=False keeps the masters for state_dict(); the quantised copy is what computes, and it cannot follow them)
                raise NotImplementedError(f"LlamaModel: a parameter of the stack was modified in place after quantize_{tag}_ (a LoRA merge, an "
                                          f"optimiser step): the {tag} copy is stale and re-quantising is not implemented; quantise after the last "
                                          "update")
            return self._quant
        key = (w.dtype, str(w.device), self._versions(self._stack_and_embed_parameters()))      # every tensor: a LoRA merge into q_proj / v_proj alone must rebuild the fused copies
        if self._packed.get("key") == key:
            return self._packed
        f32 = lambda t: t.detach().float().contiguous()
        layers = []
        for l in self.layers:
            a, m = l.self_attn, l.mlp
            layers.append(dict(n1=f32(l.input_layernorm.weight), n2=f32(l.post_attention_layernorm.weight),
                               wqkv=torch.cat([a.q_proj.weight.detach(), a.k_proj.weight.detach(), a.v_proj.weight.detach()], 0).contiguous(),
                               wo=a.o_proj.weight.detach().contiguous(),
                               wgu=ops.interleave_gate_up(m.gate_proj.weight.detach(), m.up_proj.weight.detach()),      # (gate_j, up_j) row pairs: linear_swiglu
                               wd=m.down_proj.weight.detach().contiguous()))
        self._packed = dict(key=key, layers=layers, norm=f32(self.norm.weight))
        return self._packed

    def forward(self, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, position_ids: Optional[torch.Tensor] = None):
        """inputs_embeds (B, T, D); attention_mask (B, T), 1 = token (None = all); position_ids (B, T) (None = 0..T-1).
        Returns the hidden states after the final norm, (B, T, D).  Three situations:
          gradients disabled, or nothing requires one            the prefill, no graph
          a decoder-stack parameter (layers.*, norm) requires one   the prefill runs and the result's backward raises — training the LLM's own
                                                                 weights is the reference's HF-Trainer side (SURVEY.md §2 "OUT")
          the stack is frozen and inputs_embeds requires one     the same values with a grad_fn (autograd.LlamaFn): backward() delivers
                                                                 d loss / d inputs_embeds
          adapters attached (add_lora_), the stack frozen, an    the adapted forward with a grad_fn (autograd.LlamaLoraFn): backward() delivers
          adapter or inputs_embeds requires one                  d loss / d inputs_embeds and every dA, dB
        With adapters attached the no-graph rows apply them too (the same calls, nothing kept)."""
        if self._quant is not None and torch.is_grad_enabled() and inputs_embeds.requires_grad:
            tag = self._quant["fmt"].tag
            raise NotImplementedError(f"LlamaModel.forward: a stack in {tag} storage is inference-only (no backward pass reads the {tag} weights)")
        if self.lora is not None and torch.is_grad_enabled() and not self.stack_requires_grad():
            # adapters attached, the stack frozen, an adapter or inputs_embeds requires a gradient: d / d inputs_embeds and every dA, dB
            names, params = self.lora.flat()
            if inputs_embeds.requires_grad or any(p.requires_grad for p in params):
                return autograd.LlamaLoraFn.apply(self, inputs_embeds, attention_mask, position_ids, *params)
        elif torch.is_grad_enabled() and inputs_embeds.requires_grad and not self.stack_requires_grad():
            return autograd.LlamaFn.apply(self, inputs_embeds, attention_mask, position_ids)
        with torch.no_grad():
            out = self._forward(inputs_embeds, attention_mask, position_ids)
        return autograd.no_backward("LlamaModel.forward (the prefill has no backward pass for the LLM's own weights on the HIP path; "
                                    "freeze the LLM to train through it)", out, [inputs_embeds, *self.parameters()])

    def stack_requires_grad(self) -> bool:
        """Does any parameter of the decoder stack (layers.*, norm — not embed_tokens, whose gradient comes from the splice) require a gradient?"""
        return any(p.requires_grad for p in self.layers.parameters()) or self.norm.weight.requires_grad

    def _projections(self, M: int, stream: bool = True):
        """(linear(a, w, residual=, out=), gate_up(a, w): the gate|up Linear with SwiGLU) for a pass of M rows over packed operands `w`.  The one choice
        between the native operand, the weight-streaming GEMM on the stored pair (up to `max_m` rows where the entry point streams: decode_step,
        extend) and dequantise-into-scratch + `linear` (more rows, and every prefill)."""
        fmt = None if self._quant is None else self._quant["fmt"]
        if fmt is None:
            return ops.linear, ops.linear_swiglu
        if stream and M <= fmt.max_m:
            return (lambda a, w, **kw: fmt.linear(a, *w, **kw)), (lambda a, w: ops.swiglu_pairs(fmt.linear(a, *w)))
        return (lambda a, w, **kw: ops.linear(a, self._w(w), **kw)), (lambda a, w: ops.linear_swiglu(a, self._w(w)))

    def _run_layers(self, x, layers, pos, attend, stream: bool = True):
        """The decoder stack over x (M, D), in place; `attend(li, qkv) -> o` is the entry point's attention step with its own `cache.append`, the
        only thing that differs between prefill, decode_step and extend.  Returns the norm's scratch rows for the caller's final norm."""
        H, Hkv, dh, eps, theta = self.num_heads, self.num_kv_heads, self.head_dim, self.eps, self.rope_theta
        linear, gate_up = self._projections(x.shape[0], stream)
        rmsnorm, rope_ = ops.rmsnorm, ops.rope_                               # (looked up once: a decode step is launch-bound, and the host pays per layer)
        y = None
        for li, L in enumerate(layers):
            y = rmsnorm(x, L["n1"], eps, out=y)
            qkv = linear(y, L["wqkv"])
            rope_(qkv, pos, H, dh, theta, Hkv)
            o = attend(li, qkv)
            linear(o, L["wo"], residual=x, out=x)
            y = rmsnorm(x, L["n2"], eps, out=y)
            linear(gate_up(y, L["wgu"]), L["wd"], residual=x, out=x)          # (gate_up: SwiGLU in the GEMM's epilogue in the 16-bit modes; the unfused pair otherwise: same bits)
        return y

    def _forward(self, inputs_embeds, attention_mask=None, position_ids=None, cache=None):
        """The prefill.  With `cache` (a generation.KVCache, empty) every layer's post-rotary keys / values are also copied to its slots [0, T):
        one more launch per layer, nothing else changes."""
        if self.lora is not None:                                               # unmerged adapters: the training forward's calls (its bits), nothing kept
            if cache is not None:
                self._refuse_unmerged("LlamaModel.prefill")
            from .llama_train import llama_lora_forward_train
            return llama_lora_forward_train(self, inputs_embeds, attention_mask, position_ids, keep=False)[0]
        B, T, D = inputs_embeds.shape
        pk = self._pack()
        H, Hkv, dh = self.num_heads, self.num_kv_heads, self.head_dim
        dev = inputs_embeds.device
        x = inputs_embeds.to(self.norm.weight.dtype).reshape(B * T, D).contiguous().clone()
        if position_ids is None:
            position_ids = torch.arange(T, device=dev)[None].expand(B, T)
        pos = position_ids.to(device=dev, dtype=torch.int64).reshape(B * T).contiguous()
        km = None if attention_mask is None else attention_mask.to(device=dev).bool().to(torch.uint8).reshape(B * T).contiguous()

        def attend(li, qkv):
            if cache is not None:
                cache.append(li, qkv, T, H, 0)                                  # (the cache's own format; the prefill attends over qkv itself)
            return ops.attention_causal(qkv, km, B, T, H, dh, dh ** -0.5, Hkv)
        y = self._run_layers(x, pk["layers"], pos, attend, stream=False)        # (quantised storage: dequantised at every M, `linear`'s summation order)
        if cache is not None:
            # every sequence's next rotary position: the position of its last attended token + 1 (HF extends `cumsum(attention_mask) - 1` the same way)
            p2 = pos.reshape(B, T)
            if km is None:
                cache.key_mask[:, :T] = 1
                cache.next_pos.copy_(p2[:, -1] + 1)
            else:
                m2 = km.reshape(B, T)
                cache.key_mask[:, :T] = m2
                last = (m2.long() * torch.arange(T, device=dev)[None]).max(dim=1).values
                cache.next_pos.copy_(torch.where(m2.bool().any(dim=1), p2.gather(1, last[:, None])[:, 0] + 1, torch.zeros_like(last)))
            cache.len = T
        return ops.rmsnorm(x, pk["norm"], self.eps, out=y).reshape(B, T, D)

    @torch.no_grad()
    def prefill(self, inputs_embeds, attention_mask=None, position_ids=None, cache=None):
        """`_forward` (the same calls in the same order: the same bits) that also fills `cache` — the first call of HF's generate, which returns
        `past_key_values` next to the hidden states (setokim_llama.py:133,189).  Returns the final-norm hidden states (B, T, D)."""
        self._refuse_unmerged("LlamaModel.prefill")
        if cache is None:
            raise ValueError("LlamaModel.prefill needs a generation.KVCache to fill (forward() is the prefill without one)")
        B, T, _ = inputs_embeds.shape
        if cache.len != 0 or cache.B != B or cache.cap < T or cache.num_layers != len(self.layers) or cache.dtype != self.norm.weight.dtype:
            raise ValueError(f"LlamaModel.prefill: the cache (B={cache.B}, cap={cache.cap}, len={cache.len}, {cache.num_layers} layers, "
                             f"{cache.dtype}, {cache.kv_format}) does not fit an empty prefill of B={B}, T={T}")
        return self._forward(inputs_embeds, attention_mask, position_ids, cache)

    @torch.no_grad()
    def decode_step(self, inputs_embeds, cache):
        """One token per sequence against the cache: inputs_embeds (B, D) -> the final-norm hidden states (B, D).  The token is appended at slot
        `cache.len` of every sequence and rotated to the sequence's own next position (`cache.next_pos`: the position of its last attended token
        + 1), so left- and right-padded prompts both work — with right padding the masked slots simply stay masked.  HF LlamaDecoderLayer.forward with
        `past_key_values` on a one-token input; the GEMMs are the prefill's, at M = B."""
        self._refuse_unmerged("LlamaModel.decode_step")
        B, D = inputs_embeds.shape
        slot = cache.len
        if slot < 1 or slot >= cache.cap or B != cache.B:
            raise ValueError(f"LlamaModel.decode_step: cache of B={cache.B} with {slot} of {cache.cap} slots filled cannot take a step of B={B} "
                             "(prefill first; cap = prompt length + max_new_tokens)")
        pk = self._pack()
        H, dh = self.num_heads, self.head_dim
        x = inputs_embeds.to(self.norm.weight.dtype).contiguous().clone()
        pos = cache.next_pos
        cache.key_mask[:, slot] = 1
        ws, scale, o = cache.workspace(H), dh ** -0.5, None

        def attend(li, qkv):
            nonlocal o
            cache.append(li, qkv, 1, H, slot)                                       # (native, fp8 or mxfp4: the cache's format decides these two calls)
            o = cache.attend(li, qkv, H, slot + 1, scale, ws, o)
            return o
        y = self._run_layers(x, pk["layers"], pos, attend)
        cache.len = slot + 1
        cache.next_pos = pos + 1
        return ops.rmsnorm(x, pk["norm"], self.eps, out=y)

    @torch.no_grad()
    def extend(self, inputs_embeds, cache, attention_mask=None):
        """Tn >= 1 tokens per sequence against the cache: inputs_embeds (B, Tn, D) -> the final-norm hidden states (B, Tn, D).  `decode_step`
        generalised (chunked prefill, the next turn of a conversation, scoring several candidate tokens in one pass): the rows go to slots
        [cache.len, cache.len + Tn) and attend causally over the older slots plus themselves (csrc/attn_extend.hip).  attention_mask (B, Tn),
        1 = attended (None = all): row i of sequence b is rotated to cache.next_pos[b] + (the attended rows before i in the chunk); a masked row's slot
        stays masked and its hidden state means nothing.  HF LlamaDecoderLayer.forward with `past_key_values` on a Tn-token input; the GEMMs are the
        prefill's at M = B * Tn (fp8 weights: `decode_step`'s streaming GEMM up to FP8W_MAX_M rows, the dequantise scratch above).
        Over an mxfp4 KV cache the rows are quantised on append and the attention reads the stored slots, the new rows' own included
        (ops.attention_extend_mxfp4kv: at head dim 128 in bf16 / fp16 the native MFMA kernel on tiles converted from nibbles, so the bits are the
        native extend's over the stored values; every other head dim and fp32 the wave-per-chunk kernel).
        Refused with the cache untouched: an fp8 KV cache (NotImplementedError), a wrong B, Tn == 0 on an empty cache, len + Tn > cap (ValueError)."""
        self._refuse_unmerged("LlamaModel.extend")
        B, Tn, D = inputs_embeds.shape
        len0 = cache.len
        if not cache.extendable:
            raise NotImplementedError("LlamaModel.extend: extending an fp8 KV cache by several tokens is not implemented (the extend attention over "
                                      "e4m3fn rows is a follow-up kernel); use kv_cache='native'")
        if (B != cache.B or (Tn == 0 and len0 == 0) or len0 + Tn > cache.cap or cache.num_layers != len(self.layers)
                or cache.dtype != self.norm.weight.dtype):
            raise ValueError(f"LlamaModel.extend: the cache (B={cache.B}, cap={cache.cap}, len={len0}, {cache.num_layers} layers, {cache.dtype}) "
                             f"cannot take B={B} x Tn={Tn} more tokens (len + Tn > cap, a different B, or nothing to attend to)")
        dev = inputs_embeds.device
        if attention_mask is not None and tuple(attention_mask.shape) != (B, Tn):
            raise ValueError(f"LlamaModel.extend: attention_mask {tuple(attention_mask.shape)} is not (B, Tn) = ({B}, {Tn})")
        if Tn == 0:
            return inputs_embeds.to(self.norm.weight.dtype).reshape(B, 0, D)
        pk = self._pack()
        H, dh = self.num_heads, self.head_dim
        M = B * Tn
        x = inputs_embeds.to(self.norm.weight.dtype).reshape(M, D).contiguous().clone()
        if attention_mask is None:
            am = torch.ones((B, Tn), dtype=torch.int64, device=dev)
        else:
            am = attention_mask.to(device=dev).bool().long()
        pos = (cache.next_pos[:, None] + am.cumsum(1) - am).reshape(M).contiguous()     # attended rows before i; a masked row gets the next row's (valid) position
        cache.key_mask[:, len0:len0 + Tn] = am.to(torch.uint8)
        ws, scale, o = cache.workspace(H, Tn, len0), dh ** -0.5, None

        def attend(li, qkv):
            nonlocal o
            cache.append(li, qkv, Tn, H, len0)
            o = cache.extend_attend(li, qkv, H, Tn, len0, scale, ws, o)
            return o
        y = self._run_layers(x, pk["layers"], pos, attend)
        cache.len = len0 + Tn
        cache.next_pos = cache.next_pos + am.sum(1)
        return ops.rmsnorm(x, pk["norm"], self.eps, out=y).reshape(B, Tn, D)

    def _check_paged(self, who: str, cache) -> None:
        from .generation import PagedKVCache
        self._refuse_unmerged(who)
        if not isinstance(cache, PagedKVCache):
            raise TypeError(f"{who}: cache must be a generation.PagedKVCache, got {type(cache).__name__}")
        if (cache.num_layers != len(self.layers) or cache.dtype != self.norm.weight.dtype or cache.Hkv != self.num_kv_heads
                or cache.Dh != self.head_dim):
            raise ValueError(f"{who}: the cache ({cache.num_layers} layers, Hkv={cache.Hkv}, Dh={cache.Dh}, {cache.dtype}) was not built for this "
                             f"model ({len(self.layers)} layers, Hkv={self.num_kv_heads}, Dh={self.head_dim}, {self.norm.weight.dtype})")

    @torch.no_grad()
    def prefill_paged(self, inputs_embeds, cache, row: int):
        """The prefill of ONE compact sequence into row `row` of a generation.PagedKVCache: inputs_embeds (1, T, D) -> the final-norm hidden states
        (1, T, D).  The dense `prefill` at B = 1 without a mask - the same calls in the same order, so the same bits -: positions are arange(T), the
        attention runs over the pass's own q | k | v, and every layer's keys / values go to slots [0, T) of the row through the table (T may cross
        pages).  Afterwards lens[row] = T.  The row must already own pages for T slots (`cache.assign`) and be empty (ValueError otherwise)."""
        who = "LlamaModel.prefill_paged"
        self._check_paged(who, cache)
        B, T, D = inputs_embeds.shape
        if isinstance(row, bool) or not isinstance(row, int) or not 0 <= row < cache.rows:
            raise ValueError(f"{who}: row={row!r} is outside [0, {cache.rows})")
        room = len(cache.pages_of(row)) * ops.KV_PAGE
        if B != 1 or T < 1 or cache.lens_host[row] != 0 or T > room:
            raise ValueError(f"{who}: row {row} (length {cache.lens_host[row]}, pages for {room} slots) cannot take a prefill of B={B}, T={T} "
                             "(one sequence, into an empty row that owns pages for its T slots)")
        pk = self._pack()
        H, Hkv, dh = self.num_heads, self.num_kv_heads, self.head_dim
        x = inputs_embeds.to(self.norm.weight.dtype).reshape(T, D).contiguous().clone()
        pos = torch.arange(T, device=x.device, dtype=torch.int64)
        slot0 = cache._zero

        def attend(li, qkv):
            cache.append(li, qkv, T, H, slot0, row=row)
            return ops.attention_causal(qkv, None, 1, T, H, dh, dh ** -0.5, Hkv)
        y = self._run_layers(x, pk["layers"], pos, attend, stream=False)
        cache.set_len(row, T)
        return ops.rmsnorm(x, pk["norm"], self.eps, out=y).reshape(1, T, D)

    @torch.no_grad()
    def decode_step_paged(self, inputs_embeds, cache, active, active_host=None):
        """One token for every row of a generation.PagedKVCache, at M = rows: inputs_embeds (rows, D) -> the final-norm hidden states (rows, D).
        `active` (rows,) bool on the device says which rows hold a running sequence.  An active row's token is rotated to position lens[row] (compact:
        position == slot), appended at that slot and attends over lens[row] + 1 slots; afterwards lens += active.  An idle row's state is computed and
        means nothing; its pages and length are not touched (slot0 = -1 skips its append, and it attends over its unchanged length).
        `active_host`: the same flags as a host sequence of bools - what a scheduler has anyway; without it they are read back from `active`
        (a device read).  The host mirror of the lengths and the attention's `max_len` come from it.  ValueError if an active row lacks a page
        for its next slot."""
        who = "LlamaModel.decode_step_paged"
        self._check_paged(who, cache)
        R, D = inputs_embeds.shape
        if R != cache.rows or tuple(active.shape) != (R,) or active.dtype != torch.bool:
            raise ValueError(f"{who}: a step is (rows, D) states and (rows,) bool flags for the cache's rows = {cache.rows}, got {R} and {tuple(active.shape)} {active.dtype}")
        flags = [bool(a) for a in (active.tolist() if active_host is None else active_host)]
        if len(flags) != R:
            raise ValueError(f"{who}: active_host has {len(flags)} entries for {R} rows")
        new_host = [n + a for n, a in zip(cache.lens_host, flags)]
        for r in range(R):
            if flags[r] and new_host[r] > len(cache.pages_of(r)) * ops.KV_PAGE:
                raise ValueError(f"{who}: row {r} holds {cache.lens_host[r]} slots and owns pages for {len(cache.pages_of(r)) * ops.KV_PAGE}: no room for one more")
        pk = self._pack()
        H, dh = self.num_heads, self.head_dim
        x = inputs_embeds.to(self.norm.weight.dtype).contiguous().clone()
        lens = cache.lens
        pos = lens.to(torch.int64)
        slot0 = torch.where(active, lens, torch.full_like(lens, -1))
        new_lens = lens + active.to(torch.int32)
        max_len = max(new_host)
        ws, scale, o = cache.workspace(H), dh ** -0.5, None

        def attend(li, qkv):
            nonlocal o
            cache.append(li, qkv, 1, H, slot0)
            o = cache.attend(li, qkv, H, max_len, scale, ws, o, lens=new_lens)
            return o
        y = self._run_layers(x, pk["layers"], pos, attend)
        cache.lens = new_lens
        cache.lens_host = new_host
        return ops.rmsnorm(x, pk["norm"], self.eps, out=y)

    @torch.no_grad()
    def extend_paged(self, inputs_embeds, cache, rows):
        """Tn >= 1 tokens for each of the n distinct rows `rows` of a generation.PagedKVCache: inputs_embeds (n, Tn, D) -> the final-norm hidden
        states (n, Tn, D).  The dense `extend` over pages: row r's token i is rotated to position lens[r] + i (compact: position == slot), appended
        at that slot through the table and attends over the row's older slots plus the new ones (csrc/attn_extend_paged.hip, at len0 = lens[rows]
        over the gathered table rows); afterwards lens[r] += Tn on the device and the host.  With native weights a row's states are the dense
        `extend`'s for that row alone, bit for bit.  The rows not listed are not touched.  Each listed row must own pages for lens_host[row] + Tn
        slots (ValueError otherwise, with nothing launched); what it attends over may lie in pages it shares - only its own new slots are written."""
        who = "LlamaModel.extend_paged"
        self._check_paged(who, cache)
        n, Tn, D = inputs_embeds.shape
        rows = [int(r) for r in rows]
        if n < 1 or Tn < 1 or len(rows) != n or len(set(rows)) != n or any(not 0 <= r < cache.rows for r in rows):
            raise ValueError(f"{who}: inputs_embeds {tuple(inputs_embeds.shape)} needs n >= 1 distinct rows of the cache's {cache.rows} and Tn >= 1, got rows={rows}")
        for r in rows:
            room = len(cache.pages_of(r)) * ops.KV_PAGE
            if cache.lens_host[r] + Tn > room:
                raise ValueError(f"{who}: row {r} holds {cache.lens_host[r]} slots and owns pages for {room}: no room for {Tn} more")
        pk = self._pack()
        H, dh = self.num_heads, self.head_dim
        dev = cache.lens.device
        x = inputs_embeds.to(self.norm.weight.dtype).reshape(n * Tn, D).contiguous().clone()
        idx = torch.tensor(rows, dtype=torch.int64, device=dev)
        len0 = cache.lens.index_select(0, idx).contiguous()
        table = cache.block_table.index_select(0, idx).contiguous()
        pos = (len0.to(torch.int64)[:, None] + torch.arange(Tn, device=dev)[None]).reshape(n * Tn).contiguous()
        max_len0 = max(cache.lens_host[r] for r in rows)
        ws, scale, o = cache.extend_workspace(n, Tn, H, max_len0), dh ** -0.5, None

        def attend(li, qkv):
            nonlocal o
            cache.append(li, qkv, Tn, H, len0, table=table)
            o = cache.extend_attend(li, qkv, H, Tn, max_len0, scale, ws, o, table, len0)
            return o
        y = self._run_layers(x, pk["layers"], pos, attend)
        cache.lens[idx] = len0 + Tn
        for r in rows:
            cache.lens_host[r] += Tn
        return ops.rmsnorm(x, pk["norm"], self.eps, out=y).reshape(n, Tn, D)


def _refuse_unsupported_llama_fields(g) -> None:
    """The prefill reads hidden / intermediate sizes, layer and head counts, `num_key_value_heads`, `rms_norm_eps` and `rope_theta` — plain
    multi-head or grouped-query Llama (Vicuna-7B, the reference's LLM: scripts/finetune.sh).  A checkpoint whose config carries anything
    that changes the arithmetic beyond that would load cleanly and give wrong logits, so it is refused here:
    `rope_scaling` (llama3 / linear / dynamic / yarn: other inverse frequencies at every position), an explicit `head_dim` that is not
    hidden_size / num_attention_heads, `attention_bias` / `mlp_bias` (the fused q|k|v, gate|up and down projections have no bias input),
    and a `sliding_window` (checked against the sequence length in forward: a window that covers the prompt is plain causal attention)."""
    for key in ("rope_scaling", "rope_parameters"):                         # (`rope_parameters`: the name newer HF configs carry the same dict under)
        rs = g(key)
        if rs is None:
            continue
        kind = (rs.get("rope_type", rs.get("type")) if isinstance(rs, dict) else getattr(rs, "rope_type", getattr(rs, "type", rs)))
        if kind not in (None, "default"):
            raise NotImplementedError(f"SetokimLlamaPrefill: {key}={rs!r} is not implemented on the HIP path (only the plain rotary "
                                      "embedding with `rope_theta`): a Llama-3.1-style checkpoint would give wrong logits")
    _rope_theta(g)                                                          # (raises on two different values)
    hd, H, D = g("head_dim"), g("num_attention_heads"), g("hidden_size")
    if hd is not None and int(hd) != int(D) // int(H):
        raise NotImplementedError(f"SetokimLlamaPrefill: head_dim={hd} != hidden_size / num_attention_heads = {int(D) // int(H)} is not implemented")
    for k in ("attention_bias", "mlp_bias"):
        if g(k, False):
            raise NotImplementedError(f"SetokimLlamaPrefill: {k}=True is not implemented (the projections are loaded without a bias)")


def _rope_theta(g) -> float:
    """The rotary base.  Older HF configs carry it as the top-level `rope_theta`; newer ones keep it INSIDE `rope_parameters` (and some inside
    `rope_scaling`) next to `rope_type: "default"`, which the guard above accepts — reading only the top-level field then silently used 10000
    for a 500000-base checkpoint.  The dict's value wins when the top level has none; two different values are refused."""
    top = g("rope_theta")
    inner = None
    for key in ("rope_parameters", "rope_scaling"):
        rs = g(key)
        if rs is None:
            continue
        v = rs.get("rope_theta") if isinstance(rs, dict) else getattr(rs, "rope_theta", None)
        if v is None:
            continue
        if inner is not None and float(v) != float(inner):
            raise NotImplementedError(f"SetokimLlamaPrefill: rope_parameters / rope_scaling carry two different rope_theta values ({inner} and {v})")
        inner = v
    if top is not None and inner is not None and float(top) != float(inner):
        raise NotImplementedError(f"SetokimLlamaPrefill: rope_theta={top} at the top level of the config but {inner} inside rope_parameters: "
                                  "refusing to pick one")
    if inner is not None:
        return float(inner)
    return float(top) if top is not None else 10000.0


class SetokimLlamaPrefill(nn.Module, SetokimVisionMixin):
    """`SetokimLlamaForCausalLM.forward` without the loss (setokim_llama.py:94-143): splice the image tokens into the text embeddings,
    run the LLM over them, project to the vocabulary.  `vision_tower` / `mm_in_projector` are the SetokTokenizer and projector of the
    encode path (may be None when `inputs_embeds` are passed directly)."""

    def __init__(self, config: Any, vision_tower=None, mm_in_projector=None):
        super().__init__()
        g = lambda k, d=None: config_get(config, k, d)
        self.config = config
        _refuse_unsupported_llama_fields(g)
        self.model = LlamaModel(g("vocab_size"), g("hidden_size"), g("intermediate_size"), g("num_hidden_layers"), g("num_attention_heads"),
                                g("num_key_value_heads", g("num_attention_heads")), g("rms_norm_eps", 1e-5), _rope_theta(g))
        self.lm_head = nn.Linear(g("hidden_size"), g("vocab_size"), bias=False)
        self.vision_tower = vision_tower
        self.mm_in_projector = mm_in_projector

    def get_model(self):
        return self.model

    @property
    def weight_format(self) -> str:
        return self.model.weight_format

    def add_lora_(self, r: int, lora_alpha: float, target_modules=ALL_SEVEN, lora_dropout: float = 0.0):
        """`LlamaModel.add_lora_` on the decoder stack; lm_head is frozen with it (the reference excludes it from the adapted Linears)."""
        self.model.add_lora_(r, lora_alpha, target_modules, lora_dropout)
        self.lm_head.requires_grad_(False)
        return self

    def lora_state_dict(self):
        return self.model.lora_state_dict()

    def load_lora_state_dict(self, sd) -> None:
        self.model.load_lora_state_dict(sd)

    def merge_lora_(self):
        self.model.merge_lora_()
        return self

    def quantize_fp8_(self, free_master: bool = True):
        """`LlamaModel.quantize_fp8_`: the decoder stack's projection weights into fp8 storage (embed_tokens, the norms and lm_head stay)."""
        self.model.quantize_fp8_(free_master)
        return self

    def quantize_mxfp4_(self, free_master: bool = True):
        """`LlamaModel.quantize_mxfp4_`: the decoder stack's projection weights into MXFP4 storage (embed_tokens, the norms and lm_head stay)."""
        self.model.quantize_mxfp4_(free_master)
        return self

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, inputs_embeds=None, labels=None, comp_images=None,
                last_token_only: bool = False, return_loss: bool = False):
        """Returns (logits, new_labels, attention_mask): logits (B, T', vocab) — or (B, vocab) for every sequence's last token with
        `last_token_only` (what a generation step after the prefill needs) — on the spliced sequence of length T'.  With `return_loss`
        (and labels) a fourth element is the language-model loss of setokim_llama.py:145-160 (shifted cross entropy over the positions whose
        next token is neither padding nor IGNORE_INDEX), as a 0-d fp32 tensor; the diffusion term of :163-180 is not part of this path.

        Inference unless something upstream of the LLM is being trained THROUGH it: with the decoder stack (model.layers.*, model.norm, lm_head)
        frozen and `inputs_embeds` requiring a gradient — passed in, or produced by the splice from a trainable projector / tokenizer head /
        embed_tokens.weight — logits and loss carry a grad_fn (autograd.LlamaLMFn) and `loss.backward()` fills those gradients: the
        reference's stage 2.  A stack parameter that requires a gradient keeps the inference behaviour: the forward runs, backward raises.
        `last_token_only` and a `sliding_window` shorter than the sequence are inference-only."""
        stack_live = self.model.stack_requires_grad() or self.lm_head.weight.requires_grad
        may_train = torch.is_grad_enabled() and not stack_live
        what = "SetokimLlamaPrefill.forward (inference: encode -> splice -> prefill -> logits; freeze the LLM to train through it)"
        given = inputs_embeds
        with torch.set_grad_enabled(may_train):
            inputs_embeds, attention_mask, position_ids, new_labels = self._embed(input_ids, attention_mask, position_ids, inputs_embeds, labels, comp_images)
        if self.model.weight_format != "native" and torch.is_grad_enabled() and inputs_embeds.requires_grad:
            tag = self.model._quant["fmt"].tag
            raise NotImplementedError(f"SetokimLlamaPrefill.forward: a stack in {tag} storage is inference-only (no backward pass reads the {tag} "
                                      "weights); run it under torch.no_grad() or detach inputs_embeds")
        adapters = self.model.lora.flat()[1] if self.model.lora is not None else []
        if may_train and (inputs_embeds.requires_grad or any(p.requires_grad for p in adapters)):
            if last_token_only:
                what = "SetokimLlamaPrefill.forward with last_token_only=True (a generation step: inference-only)"
            else:
                if return_loss and new_labels is None:
                    raise ValueError("return_loss needs labels")
                if adapters:
                    logits, loss = autograd.LlamaLoraLMFn.apply(self, inputs_embeds, attention_mask, position_ids, new_labels if return_loss else None,
                                                                *adapters)
                else:
                    logits, loss = autograd.LlamaLMFn.apply(self, inputs_embeds, attention_mask, position_ids, new_labels if return_loss else None)
                return (logits, new_labels, attention_mask, loss) if return_loss else (logits, new_labels, attention_mask)
        with torch.no_grad():
            out = self._head(inputs_embeds.detach(), attention_mask, position_ids, new_labels, last_token_only, return_loss)
        return autograd.no_backward(what, out, [given, inputs_embeds, *self.parameters()])

    def _forward(self, input_ids=None, attention_mask=None, position_ids=None, inputs_embeds=None, labels=None, comp_images=None,
                 last_token_only: bool = False, return_loss: bool = False):
        """The inference arithmetic in one call (no graph handling): splice, then the LLM and the vocabulary projection."""
        inputs_embeds, attention_mask, position_ids, new_labels = self._embed(input_ids, attention_mask, position_ids, inputs_embeds, labels, comp_images)
        return self._head(inputs_embeds, attention_mask, position_ids, new_labels, last_token_only, return_loss)

    def _embed(self, input_ids, attention_mask, position_ids, inputs_embeds, labels, comp_images):
        """(inputs_embeds, attention_mask, position_ids, labels) on the spliced sequence (setokim_llama.py:118-128)."""
        new_labels = labels
        self._last_features = None
        if inputs_embeds is None:
            _, position_ids, attention_mask, _, inputs_embeds, new_labels = self.prepare_inputs_labels_for_multimodal(
                input_ids, position_ids, attention_mask, None, labels, comp_images)
            if inputs_embeds is None:                                              # no images: plain text
                # text only: embed_tokens(input_ids).  An id the table cannot serve — an IMAGE_TOKEN_INDEX although no images came, a leaked
                # TARGET_TOKEN_INDEX, an id >= vocab — raises the reference's IndexError (torch's embedding) instead of becoming an address
                w_e = self.model.embed_tokens.weight.detach().contiguous()
                status = torch.empty(2, dtype=torch.int32, device=w_e.device)
                src = input_ids.to(device=w_e.device, dtype=torch.int32).contiguous()
                inputs_embeds = ops.splice_rows(src, w_e, None, status)
                st = status.cpu()
                if int(st[0]) != 0:
                    b, t = divmod(int(st[1]), input_ids.shape[1])
                    raise IndexError(f"index out of range in self: input_ids[{b}, {t}] = {int(input_ids[b, t])} is not a row of the "
                                     f"{w_e.shape[0]}-row embedding table (and no images were passed for image placeholders)")
                if autograd.grad_needed(self.model.embed_tokens.weight):           # a trainable embedding table: the same rows with a grad_fn
                    inputs_embeds = autograd.SpliceRowsFn.apply(None, self.model.embed_tokens.weight, src)
        sw = config_get(self.config, "sliding_window")
        if sw is not None and int(sw) < inputs_embeds.shape[1]:
            raise NotImplementedError(f"SetokimLlamaPrefill: sliding_window={sw} is shorter than the sequence ({inputs_embeds.shape[1]} positions): "
                                      "windowed attention is not implemented on the HIP path")
        return inputs_embeds, attention_mask, position_ids, new_labels

    @torch.no_grad()
    def generate(self, inputs=None, comp_images=None, attention_mask=None, position_ids=None, inputs_embeds=None, max_new_tokens: int = 200,
                 eos_token_id=None, pad_token_id=None, do_sample: bool = False, return_dict_in_generate: bool = False,
                 output_hidden_states: bool = False, output_logits: bool = False, images=None, kv_cache: str = "native", sampler=None, prefill_chunk: Optional[int] = None,
                 return_past: bool = False, past=None, cache_capacity: Optional[int] = None, draft=None, beams=None, processors=None,
                 output_scores: bool = False, **unsupported):
        """Greedy decoding with a KV cache: `SetokimLlamaForCausalLM.generate` (setokim_llama.py:329-396) — encode the images, splice them into
        the prompt (the existing `_embed`), prefill, then one token per step: lm_head on the B last states, argmax on the device, the new ids'
        embedding rows, `LlamaModel.decode_step`.  `images=` is the reference's keyword for `comp_images`.

        Returns the NEW tokens only, (B, n_new) int64: the splice makes the prompt ragged (an image placeholder becomes L_i rows), and with
        `inputs_embeds` HF's generate returns the new tokens only as well.  With `eos_token_id` (an int or a list) a finished sequence emits
        `pad_token_id` (default: the first eos id, HF's rule) from then on and the loop ends when every sequence has finished (one small host read
        per step).  `return_dict_in_generate` returns a generation.GenerateOutput: sequences, hidden_states (B, n_new, D) with
        `output_hidden_states` — row j is the final-norm state that produced token j, what the reference hands its image head (:363-379) — and
        logits (B, n_new, V) with `output_logits`.  Passing `inputs_embeds` (the spliced embeddings) is a superset of the reference, which raises.

        `kv_cache="fp8"` keeps the cache as e4m3fn rows with one power-of-two exponent per row (generation.KVCache, half the bytes of a 16-bit
        cache): the prefill is unchanged, a decode step quantises the new token's k / v on append and attends over the stored values.  It is
        independent of `quantize_fp8_()`.  "native" (the default) is the cache in the model's element type.

        `kv_cache="mxfp4"` keeps the cache as OCP MXFP4 rows — e2m1 nibbles with one e8m0 scale byte per 32 elements, 68 bytes per row at head
        dim 128 against fp8's 129 and 256 in 16 bits; the head dim must be a multiple of 32 (ValueError before any device call).  Only the cache
        is quantised: an unchunked prefill attends over its own unquantised q | k | v (`prefill` with an mxfp4 cache stays `torch.equal` to
        `_forward`) and stores the quantised rows; every later step attends over the stored values.  Unlike the fp8 cache it works with `draft=`,
        `prefill_chunk=`, `past=` / `return_past` and `LlamaModel.extend`.  A window of a chunked prefill attends over the stored, quantised
        slots — its own rows included — so `prefill_chunk=N` over a quantised cache is NOT the unchunked function (over the native cache it is).
        The extend attention over nibbles is the native MFMA kernel at head dim 128 in bf16 / fp16 (its tiles are converted on their way to LDS);
        in fp32 and at other head dims it is a functional kernel without MFMA, where long windows and turns are slow.

        `sampler=` (a generation.Sampler: temperature, top_k, top_p and the uniforms, given or drawn from a generator) replaces the step's argmax
        by one `setok_sample_rows` launch; everything else in the loop is the same, and `sampler=None` is the greedy path bit for bit.  A row
        whose logits hold a NaN or +inf (HF: "probability tensor contains either inf, nan") raises RuntimeError naming the sequence and the step:
        at the per-step host read when `eos_token_id` is given, otherwise once after the loop.

        `prefill_chunk=N` (an int >= 1) feeds the spliced prompt as `prefill` over columns [0, N) and `LlamaModel.extend` over each following window
        of N columns, each with its columns of the mask: the activations scale with N rows instead of the whole prompt.  None, or N >= the prompt
        length, is the unchunked path bit for bit.  Positions continue from the cache, so explicit `position_ids` cannot be combined with windows.

        `return_past=True` (with `return_dict_in_generate`) adds `GenerateOutput.past`, a generation.GenerationState: the cache and every sequence's
        pending token.  `generate(past=state, inputs= / inputs_embeds=, comp_images=, attention_mask=(B, Tn'))` continues the conversation: the new turn
        is spliced as usual, one column with the pending tokens' embedding rows (masked where there is none) is put in front of it, and the cache is
        extended by that chunk — through `prefill_chunk` windows if given — before decoding as before.  A cache without room for the turn plus
        `max_new_tokens` is replaced by a larger one holding the same slots; `cache_capacity=` lets a call reserve the room up front.  With `past`,
        `position_ids` must be None (ValueError); a state of another batch size or element type (ValueError) or with an fp8 cache
        (NotImplementedError: the extend attention over e4m3fn rows is a follow-up) is refused without being touched.  `kv_cache="fp8"` with a
        `prefill_chunk` that cuts the prompt is refused the same way.

        `draft=` (a generation.Drafter, e.g. generation.LookupDrafter(K)) decodes by draft and verify: a round feeds every sequence's pending token and
        K proposed ones through ONE `LlamaModel.extend`, selects a token from each of the K + 1 states (the same argmax or sampler launch) and
        `setok_spec_accept` keeps the longest prefix of the proposals that the model itself selected plus one more token.  Selection is a pure function
        of (logits, u), so the tokens are the plain loop's, greedy and with `Sampler(u=...)` (row j of `u` draws emitted token j; `u` needs
        max_new_tokens rows); a `Sampler(generator=...)` draws `torch.rand(max_new_tokens, B)` once at the start, which is NOT the plain loop's
        stream.  One host read per round (the kernel's 3-int summary).  The cache gets K more slots than the plain loop's and all sequences share
        `len`, so at B > 1 a sequence that accepts fewer tokens than the round's best keeps masked holes; a round that lacks K + 1 free slots
        first replaces the cache by one of twice the capacity.  Outputs, pad rule and `return_past` are the plain loop's (the state's pending token is
        each sequence's last emitted one, an eos included).  Refused before any device call: a `draft` that is no Drafter (TypeError), a `draft.K`
        outside [1, 63] (ValueError), `kv_cache="fp8"` with a draft (NotImplementedError: `extend` refuses that cache).  `draft=None` is the plain loop.

        `beams=` (a generation.BeamSearch(num_beams, length_penalty, early_stopping, num_return_sequences)) runs HF's beam search
        (include/setok_hip.h, "Beam search", states the rule): after the prefill on B rows the cache is replicated to B * num_beams rows
        (`KVCache.expanded`) and a step is lm_head on those rows, `setok_beam_topk` (the C = max(2, 1 + n_eos) * num_beams best accumulated
        log-probabilities per sequence), `setok_beam_advance` (running beams, finished set, stop test; its 2-int summary is the step's one host
        read), `KVCache.reorder` (every beam's generated slots become its parent's, two launches for the whole cache), the new ids' embedding rows
        and `decode_step`.  Returns (B * R, n_new) int64, R = num_return_sequences: rows b * R + r in descending score, cropped to the longest returned
        hypothesis, shorter ones padded with `pad_token_id` (default: the first eos id).  `GenerateOutput` then carries `sequences_scores`,
        `beam_indices`, and hidden_states / logits gathered along each hypothesis' ancestry.  `prefill_chunk=` and `kv_cache="fp8"` work as in the
        plain loop (a step appends one slot).  Refused before any device call: a `beams` that is no BeamSearch (TypeError); C > 64 or V < C
        (ValueError); `beams=` with `sampler=`, `draft=`, `past=` or `return_past=True` (NotImplementedError: beam sampling and continuing a beam
        state are not built).  `beams=None` is the plain loop bit for bit.

        `processors=` (a generation.LogitsProcessors(repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppress_tokens)) changes every step's
        logits before the token is selected, by HF's rule and in HF's order (include/setok_hip.h, "Logits processors").  Each sequence keeps a
        history on the device that starts as its attended prompt ids in order (`LookupDrafter.begin`'s convention: negative ids stay and match
        nothing, and with `inputs_embeds` alone it starts empty); `prompt_len` is its length.  A step is then lm_head, `setok_logits_process` (the
        fp32 scores), the same argmax or sampler launch on those scores, and `setok_history_append`: two launches more than without.  With `draft=`
        the K + 1 rows of a round are processed in one launch, row i seeing the history plus drafts 0 .. i - 1, and the emitted tokens are appended
        after the accept rule: the tokens are the plain loop's.  `min_new_tokens` bans the `eos_token_id` ids and does nothing without one (HF's
        rule).  `output_scores=True` (with `return_dict_in_generate`) adds `GenerateOutput.scores` (B, n_new, V) float32: the processed logits each
        token was selected from, before the sampler's warpers.  Refused before any device call: a `processors` that is no LogitsProcessors
        (TypeError); `processors=` with `beams=` (NotImplementedError: HF applies processors to the beams' log-probabilities, a different rule) or
        with `past=` (NotImplementedError: a GenerationState keeps no history); `output_scores=True` without `processors=` or without
        `return_dict_in_generate` (ValueError).  `processors=None` is the loop without them bit for bit.

        HF's own spelling stays refused: `do_sample=True`, temperature= / top_p= / top_k= or beams raise NotImplementedError (the reference's
        defaults, temperature=0.1 and top_p=10.0, are not valid HF arguments, and torch's Philox multinomial cannot be reproduced here: pass a
        `sampler=`, whose uniforms are an input).  A
        `sliding_window` shorter than prompt + max_new_tokens is refused like every field `_refuse_unsupported_llama_fields` names."""
        from . import generation as G
        req = G.check_request(self, comp_images=comp_images, images=images, position_ids=position_ids, max_new_tokens=max_new_tokens, eos_token_id=eos_token_id,
                              pad_token_id=pad_token_id, do_sample=do_sample, return_dict_in_generate=return_dict_in_generate, output_hidden_states=output_hidden_states,
                              output_logits=output_logits, kv_cache=kv_cache, sampler=sampler, prefill_chunk=prefill_chunk, return_past=return_past, past=past,
                              cache_capacity=cache_capacity, draft=draft, beams=beams, processors=processors, output_scores=output_scores, unsupported=unsupported)
        embeds, am, pos, _ = self._embed(inputs, attention_mask, position_ids, inputs_embeds, None, req.comp_images)
        w_lm, w_e = self.lm_head.weight.detach().contiguous(), self.model.embed_tokens.weight.detach().contiguous()      # the call's one fetch
        h, cache, eos, pad = G.feed_prompt(self, req, w_e, embeds, am, pos, config_get(self.config, "sliding_window"), w_lm.device)
        if beams is not None:
            return G.loop_beams(self, req, w_lm, w_e, h, cache, eos, pad if eos is not None else int(pad_token_id or 0))
        if draft is not None:
            return G.loop_speculative(self, req, w_lm, w_e, h, cache, eos, pad if eos is not None else 0, inputs, attention_mask)
        return G.loop_plain(self, req, w_lm, w_e, h, cache, eos, pad, inputs, attention_mask)

    def _head(self, inputs_embeds, attention_mask, position_ids, new_labels, last_token_only, return_loss):
        hidden = self.model._forward(inputs_embeds, attention_mask, position_ids)  # setokim_llama.py:130-140
        B, T, D = hidden.shape
        w = self.lm_head.weight.detach().contiguous()
        if last_token_only:
            if attention_mask is None:
                last = torch.full((B,), T - 1, device=hidden.device)
            else:
                am = attention_mask.to(hidden.device).bool()
                last = (am * torch.arange(T, device=hidden.device)[None]).max(dim=1).values
            rows = hidden[torch.arange(B, device=hidden.device), last].contiguous()
            return ops.linear(rows, w), new_labels, attention_mask
        logits = ops.linear(hidden.reshape(B * T, D), w).reshape(B, T, -1)         # :143
        if return_loss:
            if new_labels is None:
                raise ValueError("return_loss needs labels")
            return logits, new_labels, attention_mask, ops.lm_loss(logits, new_labels, attention_mask)[0]      # :145-160
        return logits, new_labels, attention_mask
