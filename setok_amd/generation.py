"""KV-cached greedy decoding on the HIP library: the state `SetokimLlamaForCausalLM.generate` (src/model/language_model/setokim_llama.py:329-396)
keeps between steps as HF's `past_key_values` (:99,133,189), and what it returns.

`KVCache` is allocated once per `generate` call; `LlamaModel.prefill` fills slots [0, T') of every layer, every `LlamaModel.decode_step` appends
one slot for all sequences, `LlamaModel.extend` appends Tn >= 1 slots (chunked prefill, the next turn of a conversation).  The loop itself is
`SetokimLlamaPrefill.generate` (llama.py); `GenerationState` is what it hands back so that a later call can continue from the same cache.
`Drafter` / `LookupDrafter` are the sources of proposals for `generate(draft=...)`, which verifies K drafted tokens per `extend`.  `BeamSearch` is the
setting of `generate(beams=...)`, which decodes on `KVCache.expanded(num_beams)` and re-points the beams' slots with `KVCache.reorder` every step.
`LogitsProcessors` is the setting of `generate(processors=...)`, which changes a step's logits before a token is selected."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import torch

from . import ops


@dataclass
class _KVFormat:
    """What differs between the cache formats, chosen once in `KVCache.__init__`: the per-layer tensor lists in the order both ops take them,
    `append(qkv, *tensors, T, H, pos0)`, `attend(q, *tensors, key_mask, H, length, scale, ws=, out=)`, the decode attention's slots per partial,
    whether the format can be extended by several tokens (`extend_attend`, `grown`) and, if so, the extend attention
    `extend(q, *tensors, key_mask, H, Tn, len0, scale, ws=, out=)` with its workspace rule `extend_ws(B, Tn, H, Dh, len0, Hkv, dtype)`."""
    tensors: Tuple[List[torch.Tensor], ...]
    append: Callable
    attend: Callable
    chunk: int
    extendable: bool
    extend: Optional[Callable] = None
    extend_ws: Optional[Callable] = None


class KVCache:
    """Per-layer keys / values (B, Hkv, cap, Dh) in the model's element type — the keys of one (sequence, key / value head) are contiguous rows, 256 B
    each at head dim 128 in 16 bits —, `key_mask` (B, cap) uint8 (1 = the slot holds an attended token), `next_pos` (B,) int64 (every sequence's
    next rotary position = the position of its last attended token + 1) and `len`, the number of filled slots (the same for all sequences: padding
    slots are filled and masked).  Memory: 2 * layers * B * Hkv * cap * Dh elements.

    `kv_format="fp8"` stores a row as Dh e4m3fn bytes + one int8 power-of-two exponent instead (`k_q`, `v_q` (B, Hkv, cap, Dh) uint8 and `k_e`, `v_e`
    (B, Hkv, cap) int8 per layer; `k` and `v` are then empty): 2 * layers * B * Hkv * cap * (Dh + 1) bytes.

    `kv_format="mxfp4"` stores a row as OCP MXFP4 (include/setok_hip.h, "MXFP4 KV cache"): `k_q`, `v_q` (B, Hkv, cap, Dh/2) uint8 — two e2m1 nibbles
    per byte — and `k_s`, `v_s` (B, Hkv, cap, Dh/32) uint8 — one e8m0 scale byte per 32 elements; 2 * layers * B * Hkv * cap * (Dh/2 + Dh/32)
    bytes, 68 per row at head dim 128 against fp8's 129 and 256 in 16 bits.  The kernels need Dh % 32 == 0 (`for_model` and `generate` refuse
    anything else; the constructor allocates ceil(Dh/2) and ceil(Dh/32) columns and leaves the check to them).  Unlike the fp8 format it can be
    extended by several tokens (`extend_attend`, `grown`), so it works with `LlamaModel.extend`, drafting, chunked prefill and turns.  Only the
    cache is quantised: an unchunked prefill attends over its own unquantised q | k | v and only then stores them, while an `extend` — a window of
    a chunked prefill — attends over the stored, quantised slots; so `prefill_chunk=N` over a quantised cache is not the unchunked function.

    What differs between the formats is one `_KVFormat` record."""

    FORMATS = ("native", "fp8", "mxfp4")

    def __init__(self, num_layers: int, B: int, Hkv: int, cap: int, Dh: int, dtype: torch.dtype, device, kv_format: str = "native"):
        if kv_format not in self.FORMATS:
            raise ValueError(f"KVCache: kv_format={kv_format!r} is not one of 'native', 'fp8', 'mxfp4'")
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
            self._fmt = _KVFormat((self.k_q, self.k_e, self.v_q, self.v_e), ops.kv_append_fp8, ops.attention_decode_fp8kv, ops.DECODE_CHUNK_FP8KV, False)
        elif kv_format == "mxfp4":
            # a row is Dh / 2 nibble bytes + Dh / 32 e8m0 scale bytes (include/setok_hip.h, "MXFP4 KV cache"); zero bytes mean 0.0 * 2^-127
            nq, ns = (Dh + 1) // 2, (Dh + 31) // 32
            self.k_q, self.v_q = zeros((B, Hkv, cap, nq), torch.uint8), zeros((B, Hkv, cap, nq), torch.uint8)
            self.k_s, self.v_s = zeros((B, Hkv, cap, ns), torch.uint8), zeros((B, Hkv, cap, ns), torch.uint8)
            self._fmt = _KVFormat((self.k_q, self.k_s, self.v_q, self.v_s), ops.kv_append_mxfp4, ops.attention_decode_mxfp4kv,
                                  ops.DECODE_CHUNK_MXFP4KV, True, ops.attention_extend_mxfp4kv,
                                  lambda B, Tn, H, Dh, len0, Hkv, dtype: ops.attention_extend_mxfp4kv_workspace(B, Tn, H, Dh, len0))
        else:
            self.k, self.v = zeros((B, Hkv, cap, Dh), dtype), zeros((B, Hkv, cap, Dh), dtype)
            self._fmt = _KVFormat((self.k, self.v), ops.kv_append, ops.attention_decode, ops.DECODE_CHUNK, True, ops.attention_extend,
                                  ops.attention_extend_workspace)
        self.key_mask = torch.zeros((B, cap), dtype=torch.uint8, device=device)
        self.next_pos = torch.zeros(B, dtype=torch.int64, device=device)
        self.len = 0
        self._ws: Optional[torch.Tensor] = None
        self._plan = None                                                          # ops.KVReorderPlan of the first `reorder`

    @classmethod
    def for_model(cls, model, B: int, cap: int, device=None, kv_format: str = "native") -> "KVCache":
        """A cache for `model` (a LlamaModel) with room for `cap` slots per sequence.  ValueError, before anything is allocated, for
        `kv_format="mxfp4"` on a head dim that is no multiple of 32 (the MX block)."""
        w = model.norm.weight
        if kv_format == "mxfp4" and model.head_dim % 32 != 0:
            raise ValueError(f"KVCache.for_model: kv_format='mxfp4' needs a head dim that is a multiple of 32 (the MX block), the model's is "
                             f"{model.head_dim}; use kv_format='native' or 'fp8'")
        return cls(len(model.layers), B, model.num_kv_heads, cap, model.head_dim, w.dtype, device if device is not None else w.device, kv_format)

    def append(self, li: int, qkv: torch.Tensor, T: int, H: int, pos0: int) -> None:
        """Layer `li`: the post-rotary k / v columns of the fused qkv buffer -> slots [pos0, pos0 + T), in the cache's own format."""
        self._fmt.append(qkv, *(t[li] for t in self._fmt.tensors), T, H, pos0)

    def attend(self, li: int, q: torch.Tensor, H: int, length: int, scale: float, ws: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
        """Layer `li`: one query row per (sequence, query head) against slots [0, length), in the cache's own format."""
        return self._fmt.attend(q, *(t[li] for t in self._fmt.tensors), self.key_mask, H, length, scale, ws=ws, out=out)

    def extend_attend(self, li: int, q: torch.Tensor, H: int, Tn: int, len0: int, scale: float, ws: torch.Tensor,
                      out: Optional[torch.Tensor]) -> torch.Tensor:
        """Layer `li`: Tn query rows per (sequence, query head) against slots [0, len0 + Tn), causal inside the new rows, in the cache's own format
        (ops.attention_extend, ops.attention_extend_mxfp4kv).  Not the fp8 format: reading several query rows over e4m3 rows is a second kernel."""
        if not self._fmt.extendable:
            raise NotImplementedError("KVCache.extend_attend: extending an fp8 KV cache by several tokens is not implemented (the extend attention "
                                      "over e4m3fn rows is a follow-up kernel); use kv_cache='native'")
        return self._fmt.extend(q, *(t[li] for t in self._fmt.tensors), self.key_mask, H, Tn, len0, scale, ws=ws, out=out)

    def grown(self, cap: int) -> "KVCache":
        """A cache of capacity `cap` >= self.len holding the same filled slots, mask and positions (`cap` is part of the layout, so growing copies)."""
        if not self._fmt.extendable:
            raise NotImplementedError("KVCache.grown: an fp8 KV cache cannot be extended by several tokens, so it is never grown")
        if cap < self.len:
            raise ValueError(f"KVCache.grown: cap={cap} is below the {self.len} filled slots")
        new = KVCache(self.num_layers, self.B, self.Hkv, cap, self.Dh, self.dtype, self.key_mask.device, self.kv_format)
        n = self.len
        for dst, src in zip(new._fmt.tensors, self._fmt.tensors):
            for d, t in zip(dst, src):
                d[:, :, :n].copy_(t[:, :, :n])
        new.key_mask[:, :n].copy_(self.key_mask[:, :n])
        new.next_pos.copy_(self.next_pos)
        new.len = n
        return new

    def truncate(self, n: int) -> None:
        """Give slots [n, len) back: `len = n` and their mask bytes are cleared (the rows themselves stay, unread).  What a draft-and-verify round does
        with the slots of its rejected drafts.  ValueError for n outside [0, len]; positions are the caller's business."""
        if isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= self.len:
            raise ValueError(f"KVCache.truncate: n={n!r} is outside [0, len] = [0, {self.len}]")
        if n < self.len:
            self.key_mask[:, n:self.len] = 0
        self.len = n

    def expanded(self, n: int) -> "KVCache":
        """A cache of B * n rows whose row b * n + j copies row b (filled slots, mask, positions): what beam search decodes on.  A torch copy, once
        per `generate` call; the format and the capacity stay."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"KVCache.expanded: n={n!r} must be an int >= 1")
        new = KVCache(self.num_layers, self.B * n, self.Hkv, self.cap, self.Dh, self.dtype, self.key_mask.device, self.kv_format)
        L = self.len
        for dst, src in zip(new._fmt.tensors, self._fmt.tensors):
            for d, t in zip(dst, src):
                d[:, :, :L].copy_(t[:, :, :L].repeat_interleave(n, dim=0))
        new.key_mask.copy_(self.key_mask.repeat_interleave(n, dim=0))
        new.next_pos.copy_(self.next_pos.repeat_interleave(n, dim=0))
        new.len = L
        return new

    def reorder(self, src_row: torch.Tensor, slot0: int, n: int) -> torch.Tensor:
        """Slots [slot0, len) of row r of every tensor of every layer become what row src_row[r] held (src_row (self.B,) int32, inside r's own group of n
        rows): two launches for the whole cache (ops.kv_reorder).  The slots below slot0 - the prompt, identical across a sequence's beams - never
        move; mask and positions are shared by a group.  Returns the sticky (B,) int32 status: 1 where a src_row was outside its group."""
        if self._plan is None or self._plan.n != n:
            self._plan = ops.KVReorderPlan([t for layers in self._fmt.tensors for t in layers], n)
        return ops.kv_reorder(self._plan, src_row, slot0, self.len, reserve=self.cap - slot0)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for layers in self._fmt.tensors for t in layers)

    def workspace(self, H: int, Tn: int = 0, len0: int = 0) -> torch.Tensor:
        """The attention's fp32 partials: the decode step's, sized once for the full capacity, or — with Tn > 0 — the larger of that and what an
        extend of Tn rows behind len0 slots needs."""
        need = ops.attention_decode_workspace(self.B, H, self.Dh, self.cap, self._fmt.chunk)
        if Tn > 0:
            need = max(need, self._fmt.extend_ws(self.B, Tn, H, self.Dh, len0, self.Hkv, self.dtype))
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

    def uniform_matrix(self, steps: int, B: int, device) -> torch.Tensor:
        """All (steps, B) float32 uniforms of a call at once — what `generate(draft=...)` needs, since a round selects tokens for several steps.  With
        `u` these are the plain loop's (row j is step j's); with a generator it is ONE `torch.rand(steps, B)` draw, which is not the stream the
        plain loop's per-step draws consume."""
        if self.u is not None:
            if self.u.shape[0] < steps or self.u.shape[1] != B:
                raise ValueError(f"Sampler: u has shape {tuple(self.u.shape)}, {steps} steps of a batch of {B} with a draft need (at least {steps}, {B})")
            if self.u.device != torch.device(device):
                self.u = self.u.to(device)
            return self.u[:steps]
        return torch.rand((steps, B), generator=self.generator, device=device, dtype=torch.float32)

    def select(self, logits: torch.Tensor, step: int) -> torch.Tensor:
        """int64 (B,): the step's tokens, -1 for a row whose logits hold a NaN or +inf or no finite entry."""
        return ops.sample_rows(logits, self.uniforms(step, logits.shape[0], logits.device), self.temperature, self.top_k, self.top_p)


class BeamSearch:
    """Beam search for `SetokimLlamaPrefill.generate(beams=...)`: HF's `num_beams`, `length_penalty`, `early_stopping` (False, True or "never") and
    `num_return_sequences` with HF's meaning (include/setok_hip.h, "Beam search", states the rule).  The arguments are validated here and raise
    ValueError; what depends on the call - C = max(2, 1 + n_eos) * num_beams <= 64 and V >= C - is checked by `candidates`."""

    def __init__(self, num_beams: int, length_penalty: float = 1.0, early_stopping=False, num_return_sequences: int = 1):
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= ops.BEAM_MAX_N:
            raise ValueError(f"BeamSearch: num_beams={num_beams!r} must be an int in [1, {ops.BEAM_MAX_N}]")
        if isinstance(num_return_sequences, bool) or not isinstance(num_return_sequences, int) or not 1 <= num_return_sequences <= num_beams:
            raise ValueError(f"BeamSearch: num_return_sequences={num_return_sequences!r} must be an int in [1, num_beams] = [1, {num_beams}]")
        if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or not math.isfinite(length_penalty):
            raise ValueError(f"BeamSearch: length_penalty={length_penalty!r} must be a finite number")
        if not (isinstance(early_stopping, bool) or (isinstance(early_stopping, str) and early_stopping == "never")):
            raise ValueError(f"BeamSearch: early_stopping={early_stopping!r} is not one of False, True, 'never'")
        self.num_beams, self.length_penalty = num_beams, float(length_penalty)
        self.early_stopping, self.num_return_sequences = early_stopping, num_return_sequences

    def candidates(self, n_eos: int, V: int) -> int:
        """C, the candidates kept per sequence and step; ValueError when one wave cannot hold them or the vocabulary cannot supply them."""
        C = max(2, 1 + n_eos) * self.num_beams
        if C > ops.BEAM_MAX_C:
            raise ValueError(f"BeamSearch: C = max(2, 1 + n_eos) * num_beams = {C} candidates per sequence exceed {ops.BEAM_MAX_C} "
                             f"({n_eos} eos ids, {self.num_beams} beams)")
        if V < C:
            raise ValueError(f"BeamSearch: the vocabulary (V = {V}) is smaller than the C = {C} candidates a step keeps")
        return C


def _prompt_history(B: int, device, prompt_ids: Optional[torch.Tensor], prompt_mask: Optional[torch.Tensor], cap_h: int):
    """(hist (B, cap_h) int64 filled with -1, hist_len (B,) int32) on `device`: each sequence's attended prompt ids in order.  Negative ids (image
    placeholders) stay; with `prompt_ids` None (`inputs_embeds` alone) the histories start empty."""
    T = 0 if prompt_ids is None else prompt_ids.shape[1]
    hist = torch.full((B, cap_h), -1, dtype=torch.int64, device=device)
    hist_len = torch.zeros(B, dtype=torch.int32, device=device)
    if T:
        ids = prompt_ids.to(device=device, dtype=torch.int64)
        if prompt_mask is None:
            hist[:, :T] = ids
            hist_len.fill_(T)
        else:
            am = prompt_mask.to(device).bool()
            order = torch.argsort((~am).to(torch.int8), dim=1, stable=True)       # the attended columns first, in their order
            hist[:, :T] = ids.gather(1, order)
            hist_len.copy_(am.sum(1))
    return hist, hist_len


class LogitsProcessors:
    """What `SetokimLlamaPrefill.generate(processors=...)` applies to a step's logits before a token is selected: HF's `repetition_penalty`,
    `no_repeat_ngram_size`, `min_new_tokens` and `suppress_tokens` with HF's meaning and order (include/setok_hip.h, "Logits processors", states the
    rule), one launch of `setok_logits_process` per step and one of `setok_history_append` behind the selection.  The neutral values - 1.0, 0, 0, None -
    switch a processor off; `min_new_tokens` bans the call's `eos_token_id` and does nothing without one.  The arguments are validated here and raise
    ValueError.  The object holds settings only: a call's histories live in the `ProcessorState` that `begin` returns."""

    def __init__(self, repetition_penalty: float = 1.0, no_repeat_ngram_size: int = 0, min_new_tokens: int = 0, suppress_tokens=None):
        if isinstance(repetition_penalty, bool) or not isinstance(repetition_penalty, (int, float)) or not math.isfinite(repetition_penalty) \
                or repetition_penalty <= 0:
            raise ValueError(f"LogitsProcessors: repetition_penalty={repetition_penalty!r} must be a finite number > 0 (1.0 = no penalty)")
        if isinstance(no_repeat_ngram_size, bool) or not isinstance(no_repeat_ngram_size, int) or not 0 <= no_repeat_ngram_size <= ops.LOGITS_MAX_NGRAM:
            raise ValueError(f"LogitsProcessors: no_repeat_ngram_size={no_repeat_ngram_size!r} must be an int in [0, {ops.LOGITS_MAX_NGRAM}] (0 = no ban)")
        if isinstance(min_new_tokens, bool) or not isinstance(min_new_tokens, int) or min_new_tokens < 0:
            raise ValueError(f"LogitsProcessors: min_new_tokens={min_new_tokens!r} must be an int >= 0")
        ids = [] if suppress_tokens is None else suppress_tokens
        if isinstance(ids, (str, bytes)) or not hasattr(ids, "__iter__"):
            raise ValueError(f"LogitsProcessors: suppress_tokens={suppress_tokens!r} must be a list of token ids or None")
        ids = list(ids)
        if len(ids) > ops.LOGITS_MAX_IDS or any(isinstance(s, bool) or not isinstance(s, int) or s < 0 for s in ids):
            raise ValueError(f"LogitsProcessors: suppress_tokens={suppress_tokens!r} must hold at most {ops.LOGITS_MAX_IDS} ints >= 0")
        self.repetition_penalty, self.no_repeat_ngram_size = float(repetition_penalty), no_repeat_ngram_size
        self.min_new_tokens, self.suppress_tokens = min_new_tokens, ids

    def begin(self, B: int, device, prompt_ids: Optional[torch.Tensor], prompt_mask: Optional[torch.Tensor], max_new_tokens: int,
              eos: Optional[torch.Tensor]) -> "ProcessorState":
        """The state of one `generate` call: the histories start as each sequence's attended prompt ids (`LookupDrafter.begin`'s convention) and have
        room for `max_new_tokens` more; `eos` is the call's (n_eos,) int64 device tensor or None."""
        return ProcessorState(self, B, device, prompt_ids, prompt_mask, max_new_tokens, eos)


class ProcessorState:
    """A call's histories on the device - hist (B, cap_h) int64, hist_len and prompt_len (B,) int32 - and the two launches that use them."""

    def __init__(self, settings: LogitsProcessors, B, device, prompt_ids, prompt_mask, max_new_tokens, eos):
        T = 0 if prompt_ids is None else prompt_ids.shape[1]
        self.settings = settings
        self.hist, self.hist_len = _prompt_history(B, device, prompt_ids, prompt_mask, T + int(max_new_tokens))
        self.prompt_len = self.hist_len.clone()
        self._hi = T                                                               # host bound on every hist_len
        if eos is not None and eos.numel() > ops.LOGITS_MAX_IDS:
            raise ValueError(f"LogitsProcessors: {eos.numel()} eos ids exceed the {ops.LOGITS_MAX_IDS} a call takes")
        self.eos = eos if settings.min_new_tokens > 0 else None                    # only the minimum-length ban reads them
        self.suppress = torch.tensor(settings.suppress_tokens, dtype=torch.int64, device=device) if settings.suppress_tokens else None

    def process(self, logits: torch.Tensor, tail: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 (B * n, V): the scores a token is selected from; row b * n + i sees the history followed by tail[b, :i] (the drafts of a round)."""
        s = self.settings
        return ops.logits_process(logits, self.hist, self.hist_len, self.prompt_len, tail, s.repetition_penalty, s.no_repeat_ngram_size,
                                  s.min_new_tokens, self.eos, self.suppress)

    def append(self, emitted: torch.Tensor, m: Optional[torch.Tensor] = None) -> None:
        """emitted (B, n) int64: row b's first m[b] entries (all n with m None) join its history."""
        self._hi = min(self._hi + emitted.shape[1], self.hist.shape[1])            # a call emits max_new_tokens per sequence at the most
        ops.history_append(self.hist, self.hist_len, emitted.contiguous(), self._hi, m)


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
    when requested; past (a GenerationState) with `return_past`.  With `beams=` the rows are the B * num_return_sequences hypotheses, row b * R + r in
    descending score: sequences_scores (B * R,) float32 and beam_indices (B * R, n_new) int32 - entry [r, j] is the flat row b * num_beams + beam
    whose state produced token j, -1 past the hypothesis' end (HF's meaning) -; hidden_states and logits follow that ancestry, zeros past the end.
    With `processors=` and `output_scores`: scores (B, n_new, V) float32, the processed logits token j was selected from, before the sampler's warpers."""
    sequences: torch.Tensor
    hidden_states: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past: Optional[GenerationState] = None
    sequences_scores: Optional[torch.Tensor] = None
    beam_indices: Optional[torch.Tensor] = None
    scores: Optional[torch.Tensor] = None


class Drafter:
    """What `SetokimLlamaPrefill.generate(draft=...)` drives: a source of K proposed tokens per sequence per round.  `generate` calls

      begin(B, device, prompt_ids, prompt_mask, max_new_tokens)   once: prompt_ids (B, T) int64 as the caller passed them (image placeholders and
                                                                   other specials are negative) or None with `inputs_embeds`; prompt_mask (B, T) or None
      update(emitted, m)     after the first token and after every round: emitted (B, n) int64, the first m[b] (int32) entries of row b are the tokens
                             sequence b just emitted, the rest is -1
      propose(pending)       before every round: pending (B,) int64 is each sequence's last emitted token; returns (B, K) int64, -1 = no proposal
                             (everything behind a row's first -1 is ignored)

    all on the device.  A proposal costs nothing but its slots when it is wrong: the verify pass keeps the tokens the model itself selects.  `K`
    (an int in [1, 63]) is fixed for a call.  A model-backed drafter would subclass this; `LookupDrafter` is the one that is built."""
    K: int = 0

    def begin(self, B: int, device, prompt_ids: Optional[torch.Tensor], prompt_mask: Optional[torch.Tensor], max_new_tokens: Optional[int] = None) -> None:
        pass

    def propose(self, pending: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def update(self, emitted: torch.Tensor, m: torch.Tensor) -> None:
        pass


class LookupDrafter(Drafter):
    """Prompt-lookup drafting, no second model: propose the continuation of the most recent earlier occurrence of the sequence's trailing n-gram,
    n = max_ngram down to min_ngram (include/setok_hip.h, "Speculative decoding", states the rule).  The history `hist` (B, cap_h) int64 with
    `hist_len` (B,) int32 lives on the device: `begin` stores each sequence's attended prompt ids in order (negative ids stay and match nothing;
    with `inputs_embeds` alone the history starts empty, and every call starts a new history), `update` followed by `propose` is ONE launch of
    `setok_ngram_propose`.  What it accepts depends on how repetitive the text is."""

    def __init__(self, K: int, max_ngram: int = 3, min_ngram: int = 1):
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= ops.SPEC_MAX_K:
            raise ValueError(f"LookupDrafter: K={K!r} must be an int in [1, {ops.SPEC_MAX_K}]")
        for v in (max_ngram, min_ngram):
            if isinstance(v, bool) or not isinstance(v, int):
                raise ValueError(f"LookupDrafter: the n-gram lengths must be ints, got {v!r}")
        if not 1 <= min_ngram <= max_ngram <= ops.NGRAM_MAX_N:
            raise ValueError(f"LookupDrafter: the n-gram range [{min_ngram}, {max_ngram}] must satisfy 1 <= min_ngram <= max_ngram <= {ops.NGRAM_MAX_N}")
        self.K, self.max_ngram, self.min_ngram = K, max_ngram, min_ngram
        self.hist: Optional[torch.Tensor] = None
        self.hist_len: Optional[torch.Tensor] = None
        self._queued = None                                                        # (emitted, m) of an update that no launch has appended yet
        self._hi = 0                                                               # host bound on every hist_len, queued update included
        self._limit: Optional[int] = None                                          # prompt + max_new_tokens when the call said so

    def begin(self, B, device, prompt_ids, prompt_mask, max_new_tokens=None):
        T = 0 if prompt_ids is None else prompt_ids.shape[1]
        self._limit = None if max_new_tokens is None else T + int(max_new_tokens)
        cap_h = T + (int(max_new_tokens) if max_new_tokens is not None else 64) + self.K + 1
        self.hist, self.hist_len = _prompt_history(B, device, prompt_ids, prompt_mask, cap_h)
        self._queued, self._hi = None, T

    def _room(self, n: int) -> int:
        """The bound on hist_len after `n` more entries per row; the history is regrown when a row could not take them."""
        self._hi += n
        if self._limit is not None:
            self._hi = min(self._hi, self._limit)                                   # a call emits max_new_tokens per sequence at the most
        if self._hi > self.hist.shape[1]:
            grown = torch.full((self.hist.shape[0], max(2 * self.hist.shape[1], self._hi)), -1, dtype=torch.int64, device=self.hist.device)
            grown[:, :self.hist.shape[1]] = self.hist
            self.hist = grown
        return self._hi

    def _launch(self) -> torch.Tensor:
        if self.hist is None:
            raise RuntimeError("LookupDrafter: begin() has not been called")
        e, m = self._queued if self._queued is not None else (None, None)
        self._queued = None
        return ops.ngram_propose(self.hist, self.hist_len, self.K, self._hi, e, m, self.max_ngram, self.min_ngram)

    def update(self, emitted, m):
        if self._queued is not None:
            self._launch()                                                         # two updates in a row: append the first now
        self._room(emitted.shape[1])
        self._queued = (emitted.contiguous(), m.to(torch.int32).contiguous())

    def propose(self, pending):
        return self._launch()
