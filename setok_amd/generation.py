"""KV-cached greedy decoding on the HIP library: the state `SetokimLlamaForCausalLM.generate` (src/model/language_model/setokim_llama.py:329-396)
keeps between steps as HF's `past_key_values` (:99,133,189), and what it returns.

`KVCache` is allocated once per `generate` call; `LlamaModel.prefill` fills slots [0, T') of every layer, every `LlamaModel.decode_step` appends
one slot for all sequences, `LlamaModel.extend` appends Tn >= 1 slots (chunked prefill, the next turn of a conversation).  The loop itself is
`SetokimLlamaPrefill.generate` (llama.py); `GenerationState` is what it hands back so that a later call can continue from the same cache."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import torch

from . import ops


class KVCache:
    """Per-layer keys / values (B, Hkv, cap, Dh) in the model's element type — the keys of one (sequence, key / value head) are contiguous rows, 256 B
    each at head dim 128 in 16 bits —, `key_mask` (B, cap) uint8 (1 = the slot holds an attended token), `next_pos` (B,) int64 (every sequence's
    next rotary position = the position of its last attended token + 1) and `len`, the number of filled slots (the same for all sequences: padding
    slots are filled and masked).  Memory: 2 * layers * B * Hkv * cap * Dh elements.

    `kv_format="fp8"` stores a row as Dh e4m3fn bytes + one int8 power-of-two exponent instead (`k_q`, `v_q` (B, Hkv, cap, Dh) uint8 and `k_e`, `v_e`
    (B, Hkv, cap) int8 per layer; `k` and `v` are then empty): 2 * layers * B * Hkv * cap * (Dh + 1) bytes.  `append` and `attend` are the
    two calls that differ between the formats."""

    FORMATS = ("native", "fp8")

    def __init__(self, num_layers: int, B: int, Hkv: int, cap: int, Dh: int, dtype: torch.dtype, device, kv_format: str = "native"):
        if kv_format not in self.FORMATS:
            raise ValueError(f"KVCache: kv_format={kv_format!r} is not one of 'native', 'fp8'")
        self.B, self.Hkv, self.cap, self.Dh = B, Hkv, cap, Dh
        self.num_layers, self.dtype, self.kv_format = num_layers, dtype, kv_format
        # zero-filled: the decode kernel reads masked slots below `len` before it discards them, so they must hold initialised memory
        zeros = lambda shape, dt: [torch.zeros(shape, dtype=dt, device=device) for _ in range(num_layers)]
        self.k: List[torch.Tensor] = []
        self.v: List[torch.Tensor] = []
        if kv_format == "fp8":
            # a row is Dh e4m3fn bytes + one int8 exponent and means value(code) * 2^exponent (include/setok_hip.h, "FP8 KV cache")
            self.k_q, self.v_q = zeros((B, Hkv, cap, Dh), torch.uint8), zeros((B, Hkv, cap, Dh), torch.uint8)
            self.k_e, self.v_e = zeros((B, Hkv, cap), torch.int8), zeros((B, Hkv, cap), torch.int8)
        else:
            self.k, self.v = zeros((B, Hkv, cap, Dh), dtype), zeros((B, Hkv, cap, Dh), dtype)
        self.key_mask = torch.zeros((B, cap), dtype=torch.uint8, device=device)
        self.next_pos = torch.zeros(B, dtype=torch.int64, device=device)
        self.len = 0
        self._ws: Optional[torch.Tensor] = None

    @classmethod
    def for_model(cls, model, B: int, cap: int, device=None, kv_format: str = "native") -> "KVCache":
        """A cache for `model` (a LlamaModel) with room for `cap` slots per sequence."""
        w = model.norm.weight
        return cls(len(model.layers), B, model.num_kv_heads, cap, model.head_dim, w.dtype, device if device is not None else w.device, kv_format)

    def append(self, li: int, qkv: torch.Tensor, T: int, H: int, pos0: int) -> None:
        """Layer `li`: the post-rotary k / v columns of the fused qkv buffer -> slots [pos0, pos0 + T), in the cache's own format."""
        if self.kv_format == "fp8":
            ops.kv_append_fp8(qkv, self.k_q[li], self.k_e[li], self.v_q[li], self.v_e[li], T, H, pos0)
        else:
            ops.kv_append(qkv, self.k[li], self.v[li], T, H, pos0)

    def attend(self, li: int, q: torch.Tensor, H: int, length: int, scale: float, ws: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
        """Layer `li`: one query row per (sequence, query head) against slots [0, length), in the cache's own format."""
        if self.kv_format == "fp8":
            return ops.attention_decode_fp8kv(q, self.k_q[li], self.k_e[li], self.v_q[li], self.v_e[li], self.key_mask, H, length, scale, ws=ws, out=out)
        return ops.attention_decode(q, self.k[li], self.v[li], self.key_mask, H, length, scale, ws=ws, out=out)

    def extend_attend(self, li: int, q: torch.Tensor, H: int, Tn: int, len0: int, scale: float, ws: torch.Tensor,
                      out: Optional[torch.Tensor]) -> torch.Tensor:
        """Layer `li`: Tn query rows per (sequence, query head) against slots [0, len0 + Tn), causal inside the new rows (ops.attention_extend).  The
        native format only: reading several query rows over e4m3 rows is a second kernel."""
        if self.kv_format == "fp8":
            raise NotImplementedError("KVCache.extend_attend: extending an fp8 KV cache by several tokens is not implemented (the extend attention "
                                      "over e4m3fn rows is a follow-up kernel); use kv_cache='native'")
        return ops.attention_extend(q, self.k[li], self.v[li], self.key_mask, H, Tn, len0, scale, ws=ws, out=out)

    def grown(self, cap: int) -> "KVCache":
        """A cache of capacity `cap` >= self.len holding the same filled slots, mask and positions (`cap` is part of the layout, so growing copies)."""
        if self.kv_format == "fp8":
            raise NotImplementedError("KVCache.grown: an fp8 KV cache cannot be extended by several tokens, so it is never grown")
        if cap < self.len:
            raise ValueError(f"KVCache.grown: cap={cap} is below the {self.len} filled slots")
        new = KVCache(self.num_layers, self.B, self.Hkv, cap, self.Dh, self.dtype, self.key_mask.device)
        n = self.len
        for dst, src in ((new.k, self.k), (new.v, self.v)):
            for d, t in zip(dst, src):
                d[:, :, :n].copy_(t[:, :, :n])
        new.key_mask[:, :n].copy_(self.key_mask[:, :n])
        new.next_pos.copy_(self.next_pos)
        new.len = n
        return new

    def nbytes(self) -> int:
        if self.kv_format == "fp8":                                    # codes + exponents
            return sum(t.numel() * t.element_size() for t in self.k_q + self.k_e + self.v_q + self.v_e)
        return sum(t.numel() * t.element_size() for t in self.k + self.v)

    def workspace(self, H: int, Tn: int = 0, len0: int = 0) -> torch.Tensor:
        """The attention's fp32 partials: the decode step's, sized once for the full capacity, or — with Tn > 0 — the larger of that and what an
        extend of Tn rows behind len0 slots needs."""
        chunk = ops.DECODE_CHUNK_FP8KV if self.kv_format == "fp8" else ops.DECODE_CHUNK
        need = ops.attention_decode_workspace(self.B, H, self.Dh, self.cap, chunk)
        if Tn > 0:
            need = max(need, ops.attention_extend_workspace(self.B, Tn, H, self.Dh, len0, self.Hkv, self.dtype))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1), dtype=torch.float32, device=self.key_mask.device)
        return self._ws


class Sampler:
    """Sampled token selection for `SetokimLlamaPrefill.generate(sampler=...)`: temperature, then top-k, then top-p (HF's order), one launch of
    `setok_sample_rows` per step (include/setok_hip.h, "Sampling", states the rule).  The draw is one uniform number per row per step and that
    number is an input of the kernel, so a run is reproducible from its uniforms alone:

      u=          (max_new_tokens, B) float32 in [0, 1): step j uses row j.  The reproducible path.
      generator=  otherwise step j draws `torch.rand(B, generator=generator, device=...)` (the device's default generator when None).

    One uniform is consumed per row per step whether or not the row has finished, so a row's stream does not depend on its neighbours.
    `top_k=0` and `top_p=1.0` mean no filter.  The arguments are validated like the C call's and raise ValueError."""

    def __init__(self, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, generator: Optional[torch.Generator] = None,
                 u: Optional[torch.Tensor] = None):
        temperature, top_p = float(temperature), float(top_p)
        if not math.isfinite(temperature) or temperature <= 0.0:
            raise ValueError(f"Sampler: temperature={temperature} must be finite and > 0 (greedy decoding is generate(sampler=None) or top_k=1)")
        if isinstance(top_k, bool) or int(top_k) != top_k or int(top_k) < 0:
            raise ValueError(f"Sampler: top_k={top_k!r} must be an integer >= 0 (0 = no filter)")
        if not (0.0 < top_p <= 1.0):
            raise ValueError(f"Sampler: top_p={top_p} is not a probability: it must lie in (0, 1] (1.0 = no filter; the reference's default "
                             "top_p=10.0 is not a valid nucleus either)")
        if u is not None:
            if generator is not None:
                raise ValueError("Sampler: pass the uniforms as `u` or a `generator` to draw them, not both")
            if u.dim() != 2 or u.dtype != torch.float32:
                raise ValueError(f"Sampler: u must be a (max_new_tokens, B) float32 tensor, got {tuple(u.shape)} {u.dtype}")
        self.temperature, self.top_k, self.top_p, self.generator, self.u = temperature, int(top_k), top_p, generator, u

    def uniforms(self, step: int, B: int, device) -> torch.Tensor:
        """The (B,) float32 uniforms of decode step `step`, on `device`."""
        if self.u is not None:
            if step >= self.u.shape[0] or self.u.shape[1] != B:
                raise ValueError(f"Sampler: u has shape {tuple(self.u.shape)}, step {step} of a batch of {B} needs (at least {step + 1}, {B})")
            if self.u.device != torch.device(device):
                self.u = self.u.to(device)                                         # once: a step's row is then a view, no copy per step
            return self.u[step]
        return torch.rand(B, generator=self.generator, device=device, dtype=torch.float32)

    def select(self, logits: torch.Tensor, step: int) -> torch.Tensor:
        """int64 (B,): the step's tokens, -1 for a row whose logits hold a NaN or +inf or no finite entry."""
        return ops.sample_rows(logits, self.uniforms(step, logits.shape[0], logits.device), self.temperature, self.top_k, self.top_p)


@dataclass
class GenerationState:
    """What `generate(return_past=True)` hands back and `generate(past=...)` continues from: the `KVCache` and `pending` (B,) int64 — the last real
    token of each sequence that the stack has not consumed yet, -1 where there is none.  The state is equivalent to each sequence having consumed
    exactly its prompt plus its emitted tokens up to and including its first eos (all of them without an eos), the last real token possibly
    still pending: the slots a finished sequence's pads went to are masked out and its next position is set back.  The call that continues a
    state extends its cache in place when the capacity allows (`cache_capacity=` reserves it), so a state is continued once."""
    cache: KVCache
    pending: torch.Tensor


@dataclass
class GenerateOutput:
    """`generate(return_dict_in_generate=True)`: sequences (B, n_new) int64 — the NEW tokens only; hidden_states (B, n_new, D): row j is the final-norm
    state that produced token j (what the reference collects as `x[-1]` per step, setokim_llama.py:363, for its image head); logits (B, n_new, V)
    when requested; past (a GenerationState) with `return_past`."""
    sequences: torch.Tensor
    hidden_states: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past: Optional[GenerationState] = None
