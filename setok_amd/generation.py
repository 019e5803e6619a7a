"""KV-cached greedy decoding on the HIP library: the state `SetokimLlamaForCausalLM.generate` (src/model/language_model/setokim_llama.py:329-396)
keeps between steps as HF's `past_key_values` (:99,133,189), and what it returns.

`KVCache` is allocated once per `generate` call; `LlamaModel.prefill` fills slots [0, T') of every layer, every `LlamaModel.decode_step` appends
one slot for all sequences.  The loop itself is `SetokimLlamaPrefill.generate` (llama.py)."""
from __future__ import annotations

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

    def nbytes(self) -> int:
        if self.kv_format == "fp8":                                    # codes + exponents
            return sum(t.numel() * t.element_size() for t in self.k_q + self.k_e + self.v_q + self.v_e)
        return sum(t.numel() * t.element_size() for t in self.k + self.v)

    def workspace(self, H: int) -> torch.Tensor:
        """The decode attention's fp32 partials, sized once for the full capacity."""
        chunk = ops.DECODE_CHUNK_FP8KV if self.kv_format == "fp8" else ops.DECODE_CHUNK
        need = ops.attention_decode_workspace(self.B, H, self.Dh, self.cap, chunk)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1), dtype=torch.float32, device=self.key_mask.device)
        return self._ws


@dataclass
class GenerateOutput:
    """`generate(return_dict_in_generate=True)`: sequences (B, n_new) int64 — the NEW tokens only; hidden_states (B, n_new, D): row j is the final-norm
    state that produced token j (what the reference collects as `x[-1]` per step, setokim_llama.py:363, for its image head); logits (B, n_new, V)
    when requested."""
    sequences: torch.Tensor
    hidden_states: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
