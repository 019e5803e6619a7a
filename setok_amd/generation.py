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
    slots are filled and masked).  Memory: 2 * layers * B * Hkv * cap * Dh elements."""

    def __init__(self, num_layers: int, B: int, Hkv: int, cap: int, Dh: int, dtype: torch.dtype, device):
        self.B, self.Hkv, self.cap, self.Dh = B, Hkv, cap, Dh
        # zero-filled: the decode kernel reads masked slots below `len` before it discards them, so they must hold initialised memory
        self.k: List[torch.Tensor] = [torch.zeros((B, Hkv, cap, Dh), dtype=dtype, device=device) for _ in range(num_layers)]
        self.v: List[torch.Tensor] = [torch.zeros((B, Hkv, cap, Dh), dtype=dtype, device=device) for _ in range(num_layers)]
        self.key_mask = torch.zeros((B, cap), dtype=torch.uint8, device=device)
        self.next_pos = torch.zeros(B, dtype=torch.int64, device=device)
        self.len = 0
        self._ws: Optional[torch.Tensor] = None

    @classmethod
    def for_model(cls, model, B: int, cap: int, device=None) -> "KVCache":
        """A cache for `model` (a LlamaModel) with room for `cap` slots per sequence."""
        w = model.norm.weight
        return cls(len(model.layers), B, model.num_kv_heads, cap, model.head_dim, w.dtype, device if device is not None else w.device)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.k + self.v)

    def workspace(self, H: int) -> torch.Tensor:
        """The decode attention's fp32 partials, sized once for the full capacity."""
        need = ops.attention_decode_workspace(self.B, H, self.Dh, self.cap)
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
