"""KV-cached greedy decoding on the HIP library: the state `SetokimLlamaForCausalLM.generate` (src/model/language_model/setokim_llama.py:329-396)
keeps between steps as HF's `past_key_values` (:99,133,189), and what it returns.

`KVCache` is allocated once per `generate` call; `LlamaModel.prefill` fills slots [0, T') of every layer, every `LlamaModel.decode_step` appends
one slot for all sequences, `LlamaModel.extend` appends Tn >= 1 slots (chunked prefill, the next turn of a conversation).  The loop is here too, as
the plain functions `SetokimLlamaPrefill.generate` (llama.py) calls in turn: `check_request` (every refusal that needs no device call), `feed_prompt`,
then `loop_plain`, `loop_beams` or `loop_speculative`; `GenerationState` is what it hands back so that a later call can continue from the same cache.
`Drafter` / `LookupDrafter` are the sources of proposals for `generate(draft=...)`, which verifies K drafted tokens per `extend`.  `BeamSearch` is the
setting of `generate(beams=...)`, which decodes on `KVCache.expanded(num_beams)` and re-points the beams' slots with `KVCache.reorder` every step.
`LogitsProcessors` is the setting of `generate(processors=...)`, which changes a step's logits before a token is selected."""
from __future__ import annotations

import math
from collections import namedtuple
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import torch

from . import ops


@dataclass
class _KVFormat:
    """What differs between the cache formats, chosen once in `KVCache.__init__`: the per-layer tensor lists in the order both ops take them,
    `append(qkv, *tensors, T, H, pos0)`, `attend(q, *tensors, key_mask, H, length, scale, ws=, out=)`, the decode attention's slots per partial
    and, where the format can be extended by several tokens (`KVCache.extendable`), the extend attention
    `extend(q, *tensors, key_mask, H, Tn, len0, scale, ws=, out=)` with its workspace rule `extend_ws(B, Tn, H, Dh, len0, Hkv, dtype)`."""
    tensors: Tuple[List[torch.Tensor], ...]
    append: Callable
    attend: Callable
    chunk: int
    extend: Optional[Callable] = None
    extend_ws: Optional[Callable] = None


def check_kv_head_dim(kv_format: str, head_dim: int, who: str, arg: str) -> None:
    """The one head-dim rule of the cache formats: the mxfp4 kernels need whole MX blocks.  ValueError naming the caller `who` and its argument `arg`."""
    if kv_format == "mxfp4" and head_dim % 32 != 0:
        raise ValueError(f"{who}: {arg}='mxfp4' needs a head dim that is a multiple of 32 (the MX block), the model's is {head_dim}; "
                         f"use {arg}='native' or 'fp8'")


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
    EXTENDABLE = ("native", "mxfp4")                       # the formats with an extend attention; reading several query rows over e4m3 rows is a follow-up kernel

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
            self._fmt = _KVFormat((self.k_q, self.k_e, self.v_q, self.v_e), ops.kv_append_fp8, ops.attention_decode_fp8kv, ops.DECODE_CHUNK_FP8KV)
        elif kv_format == "mxfp4":
            # a row is Dh / 2 nibble bytes + Dh / 32 e8m0 scale bytes (include/setok_hip.h, "MXFP4 KV cache"); zero bytes mean 0.0 * 2^-127
            nq, ns = (Dh + 1) // 2, (Dh + 31) // 32
            self.k_q, self.v_q = zeros((B, Hkv, cap, nq), torch.uint8), zeros((B, Hkv, cap, nq), torch.uint8)
            self.k_s, self.v_s = zeros((B, Hkv, cap, ns), torch.uint8), zeros((B, Hkv, cap, ns), torch.uint8)
            self._fmt = _KVFormat((self.k_q, self.k_s, self.v_q, self.v_s), ops.kv_append_mxfp4, ops.attention_decode_mxfp4kv,
                                  ops.DECODE_CHUNK_MXFP4KV, ops.attention_extend_mxfp4kv,
                                  lambda B, Tn, H, Dh, len0, Hkv, dtype: ops.attention_extend_mxfp4kv_workspace(B, Tn, H, Dh, len0))
        else:
            self.k, self.v = zeros((B, Hkv, cap, Dh), dtype), zeros((B, Hkv, cap, Dh), dtype)
            self._fmt = _KVFormat((self.k, self.v), ops.kv_append, ops.attention_decode, ops.DECODE_CHUNK, ops.attention_extend,
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
        check_kv_head_dim(kv_format, model.head_dim, "KVCache.for_model", "kv_format")
        return cls(len(model.layers), B, model.num_kv_heads, cap, model.head_dim, w.dtype, device if device is not None else w.device, kv_format)

    @property
    def extendable(self) -> bool:
        """Can the cache take several tokens per sequence at once (`extend_attend`, `grown`: extend, chunked prefill, turns, drafting)?  Not fp8."""
        return self.kv_format in self.EXTENDABLE

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
        if not self.extendable:
            raise NotImplementedError("KVCache.extend_attend: extending an fp8 KV cache by several tokens is not implemented (the extend attention "
                                      "over e4m3fn rows is a follow-up kernel); use kv_cache='native'")
        return self._fmt.extend(q, *(t[li] for t in self._fmt.tensors), self.key_mask, H, Tn, len0, scale, ws=ws, out=out)

    def grown(self, cap: int) -> "KVCache":
        """A cache of capacity `cap` >= self.len holding the same filled slots, mask and positions (`cap` is part of the layout, so growing copies)."""
        if not self.extendable:
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


def _count(v, name: str, who: str) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{who}: {name}={v!r} must be an int >= 1")
    return v


@dataclass
class _PagedKVFormat:
    """`_KVFormat` for the pools of `PagedKVCache`, chosen once in its `__init__`: the per-layer pool lists in the order the ops take them,
    `append(qkv, *pools, table, slot0, T, H)`, `attend(q, *pools, table, lens, H, max_len, scale, ws=, out=)`,
    `extend(q, *pools, table, len0, H, Tn, max_len0, scale, ws=, out=)`, the two workspace rules `decode_ws(B, H, Dh, max_len)` and
    `extend_ws(n, Tn, H, Dh, max_len0, Hkv, dtype)`, and the bytes one slot of one key / value head takes."""
    pools: Tuple[List[torch.Tensor], ...]
    append: Callable
    attend: Callable
    extend: Callable
    decode_ws: Callable
    extend_ws: Callable
    row_nbytes: int


class PagedKVCache:
    """The cache without a capacity per sequence (include/setok_hip.h, "Paged KV cache"): per layer two pools `k[li]`, `v[li]` of
    shape (num_pages, Hkv, ops.KV_PAGE, Dh) in the model's element type, shared by `rows` sequences.  A sequence is row r of `block_table`
    ((rows, max_pages_per_seq) int32 on the device, -1 = no page; entry p holds slots [128 p, 128 p + 128)) and `lens[r]` ((rows,) int32 on the device):
    every row has a length of its own, a compact sequence has no dead slots (there is no key mask; position == slot), and a finished sequence's
    pages go back to the pool.  Memory: 2 * layers * num_pages * Hkv * 128 * Dh elements, whatever `rows` is.

    Pages are counted by reference (`page_refs`, on the host; 0 = free): a row holds one reference to each page of its table entries, `assign(shared=)`
    points a row's first entries at pages somebody already holds, `detach` turns a row's references into the caller's and `drop` gives those back.  Shared
    pages are never written: sharing is in whole pages and a row's first own slot is at a page boundary, so there is no copy-on-write.

    `table_host` / `lens_host` mirror both on the host and `_free` is the host's free list.  The scheduler (this class's methods, called by
    `LlamaModel.prefill_paged` / `decode_step_paged` and `ContinuousBatcher`) is the only writer, so the mirrors are exact without any device read.
    The pools are `torch.empty`: nothing depends on their initial contents - a slot is written before the sequence's length covers it.

    `kv_format="mxfp4"` stores a slot as OCP MXFP4, as `KVCache` does (include/setok_hip.h, "Paged MXFP4 KV cache"): per layer `k_q`, `v_q`
    (num_pages, Hkv, 128, Dh/2) uint8 and `k_s`, `v_s` (num_pages, Hkv, 128, Dh/32) uint8, and `k` and `v` are empty lists;
    2 * layers * num_pages * Hkv * 128 * (Dh/2 + Dh/32) bytes, 68 per slot at head dim 128 against 256 in 16 bits.  Head dims 32, 64 and 128 (the
    ones the decode attention over nibble rows has a lane layout for); `"fp8"` is not built - that format has no extend attention, so it could not
    serve prefixes.  Scheduling - pages, references, lengths - does not depend on the format; what does is one `_PagedKVFormat` record."""

    FORMATS = ("native", "mxfp4")

    def __init__(self, num_layers: int, rows: int, Hkv: int, Dh: int, dtype: torch.dtype, device, num_pages: int, max_pages_per_seq: int,
                 kv_format: str = "native"):
        who = "PagedKVCache"
        if kv_format == "fp8":
            raise NotImplementedError(f"{who}: kv_format='fp8' is not implemented over pages (the fp8 cache has no extend attention, so it could not "
                                      "serve shared prefixes); use kv_format='native' or 'mxfp4'")
        if kv_format not in self.FORMATS:
            raise ValueError(f"{who}: kv_format={kv_format!r} is not one of 'native', 'mxfp4'")
        for name, v in (("num_layers", num_layers), ("rows", rows), ("Hkv", Hkv), ("Dh", Dh), ("num_pages", num_pages),
                        ("max_pages_per_seq", max_pages_per_seq)):
            _count(v, name, who)
        self.num_layers, self.rows, self.Hkv, self.Dh, self.dtype = num_layers, rows, Hkv, Dh, dtype
        self.num_pages, self.max_pages_per_seq, self.kv_format = num_pages, max_pages_per_seq, kv_format
        pool = lambda cols, dt: [torch.empty((num_pages, Hkv, ops.KV_PAGE, cols), dtype=dt, device=device) for _ in range(num_layers)]
        self.k: List[torch.Tensor] = []
        self.v: List[torch.Tensor] = []
        if kv_format == "mxfp4":
            check_kv_head_dim(kv_format, Dh, who, "kv_format")
            if Dh not in ops.PAGED_MXFP4_HEAD_DIMS:
                raise ValueError(f"{who}: kv_format='mxfp4' needs a head dim of 32, 64 or 128 (the lane layouts of the decode attention over nibble "
                                 f"rows), the model's is {Dh}; use kv_format='native'")
            self.k_q, self.v_q = pool(Dh // 2, torch.uint8), pool(Dh // 2, torch.uint8)
            self.k_s, self.v_s = pool(Dh // 32, torch.uint8), pool(Dh // 32, torch.uint8)
            self._fmt = _PagedKVFormat((self.k_q, self.k_s, self.v_q, self.v_s), ops.kv_append_paged_mxfp4, ops.attention_decode_paged_mxfp4kv,
                                       ops.attention_extend_paged_mxfp4kv, ops.attention_decode_paged_mxfp4kv_workspace,
                                       lambda n, Tn, H, Dh, max_len0, Hkv, dtype: ops.attention_extend_paged_mxfp4kv_workspace(n, Tn, H, Dh, max_len0),
                                       Dh // 2 + Dh // 32)
        else:
            self.k, self.v = pool(Dh, dtype), pool(Dh, dtype)
            self._fmt = _PagedKVFormat((self.k, self.v), ops.kv_append_paged, ops.attention_decode_paged, ops.attention_extend_paged,
                                       ops.attention_decode_paged_workspace, ops.attention_extend_paged_workspace, Dh * self.k[0].element_size())
        self.block_table = torch.full((rows, max_pages_per_seq), -1, dtype=torch.int32, device=device)
        self.lens = torch.zeros(rows, dtype=torch.int32, device=device)
        self.table_host: List[List[int]] = [[-1] * max_pages_per_seq for _ in range(rows)]
        self.lens_host: List[int] = [0] * rows
        self._free: List[int] = list(range(num_pages))                             # handed out from the front, returned to the back
        self.page_refs: List[int] = [0] * num_pages                                # references per page: table entries + what `detach` handed out; 0 = free
        self._zero = torch.zeros(1, dtype=torch.int32, device=device)              # a prefill's slot0
        self._ws: Optional[torch.Tensor] = None
        self._ws_extend: Optional[torch.Tensor] = None

    @classmethod
    def for_model(cls, model, rows: int, num_pages: int, max_pages_per_seq: int, device=None, kv_format: str = "native") -> "PagedKVCache":
        """Pools for `model` (a LlamaModel): `rows` sequences at a time, `num_pages` pages of 128 slots per layer, at most `max_pages_per_seq` per
        sequence, in `kv_format` ("native" or "mxfp4"; the constructor's refusals, before anything is allocated)."""
        w = model.norm.weight
        return cls(len(model.layers), rows, model.num_kv_heads, model.head_dim, w.dtype, device if device is not None else w.device, num_pages,
                   max_pages_per_seq, kv_format)

    @property
    def fresh(self) -> bool:
        """Nothing has used the cache yet, or everything gave it back: every row idle, every page free."""
        return len(self._free) == self.num_pages and not any(self.lens_host) and all(p < 0 for row in self.table_host for p in row)

    @property
    def pages_free(self) -> int:
        return len(self._free)

    @property
    def page_nbytes(self) -> int:
        """Bytes one page takes over all layers, keys and values."""
        return 2 * self.num_layers * self.Hkv * ops.KV_PAGE * self._fmt.row_nbytes

    def pages_of(self, row: int) -> List[int]:
        return [p for p in self.table_host[row] if p >= 0]

    def _row(self, row, who: str) -> int:
        if isinstance(row, bool) or not isinstance(row, int) or not 0 <= row < self.rows:
            raise ValueError(f"PagedKVCache.{who}: row={row!r} is outside [0, {self.rows})")
        return row

    def assign(self, row: int, n_slots: int, shared=()) -> bool:
        """Give the idle row `row` the ceil(n_slots / 128) pages that hold its slots [0, n_slots).  The first len(shared) table entries are the
        pages in `shared` - pages somebody already holds (count >= 1, else ValueError), each of which gains one reference -; the others come off
        the free list with count 1.  False, with nothing changed, if the pool cannot supply them.  ValueError for a row that already owns pages,
        n_slots < 1, more pages than a table row has entries, or len(shared) * 128 >= n_slots: a row must own the page it writes to."""
        self._row(row, "assign")
        n = (_count(n_slots, "n_slots", "PagedKVCache.assign") + ops.KV_PAGE - 1) // ops.KV_PAGE
        shared = list(shared)
        if self.pages_of(row):
            raise ValueError(f"PagedKVCache.assign: row {row} already owns pages (release it first)")
        if n > self.max_pages_per_seq:
            raise ValueError(f"PagedKVCache.assign: {n_slots} slots need {n} pages, a sequence has at most max_pages_per_seq = {self.max_pages_per_seq}")
        for p in shared:
            if isinstance(p, bool) or not isinstance(p, int) or not 0 <= p < self.num_pages or self.page_refs[p] < 1:
                raise ValueError(f"PagedKVCache.assign: shared page {p!r} is not a page somebody holds (a free page cannot be shared)")
        if len(shared) * ops.KV_PAGE >= n_slots:
            raise ValueError(f"PagedKVCache.assign: {len(shared)} shared pages cover all of the row's {n_slots} slots (a row must own the page it "
                             "writes to: shared pages are never written)")
        own = n - len(shared)
        if own > len(self._free):
            return False
        pages, self._free = self._free[:own], self._free[own:]
        for p in shared + pages:
            self.page_refs[p] += 1
        self.table_host[row] = shared + pages + [-1] * (self.max_pages_per_seq - n)
        self.block_table[row] = torch.tensor(self.table_host[row], dtype=torch.int32)
        return True

    def _idle(self, row: int) -> None:
        self.table_host[row] = [-1] * self.max_pages_per_seq
        self.lens_host[row] = 0
        self.block_table[row] = -1
        self.lens[row] = 0

    def release(self, row: int) -> None:
        """Every page of the row loses one reference; those that reach 0 go to the back of the free list in table order.  The row's table entries
        become -1 and its length 0.  ValueError for an idle row."""
        self._row(row, "release")
        pages = self.pages_of(row)
        if not pages:
            raise ValueError(f"PagedKVCache.release: row {row} is idle (it owns no pages)")
        self._unref(pages)
        self._idle(row)

    def _unref(self, pages: List[int]) -> None:
        for p in pages:
            self.page_refs[p] -= 1
            if self.page_refs[p] == 0:
                self._free.append(p)

    def detach(self, row: int) -> List[int]:
        """The row becomes idle - entries -1, length 0, on the device and in the host mirrors - but its pages are not freed: the caller now holds
        the row's reference to each of the returned pages (table order) and gives it back with `drop`, after handing the pages to other rows as
        `assign(shared=)` if it likes.  ValueError for an idle row."""
        self._row(row, "detach")
        pages = self.pages_of(row)
        if not pages:
            raise ValueError(f"PagedKVCache.detach: row {row} is idle (it owns no pages)")
        self._idle(row)
        return pages

    def drop(self, pages) -> None:
        """Give back one reference to each page of `pages` (what `detach` handed out); a page whose count reaches 0 goes to the back of the free
        list.  ValueError, with nothing changed, for a page id out of range or a count that would go below 0."""
        pages = list(pages)
        for p in set(pages):
            if isinstance(p, bool) or not isinstance(p, int) or not 0 <= p < self.num_pages:
                raise ValueError(f"PagedKVCache.drop: page {p!r} is outside [0, {self.num_pages})")
            if self.page_refs[p] < pages.count(p):
                raise ValueError(f"PagedKVCache.drop: page {p} has {self.page_refs[p]} references, {pages.count(p)} to give back")
        self._unref(pages)

    def set_len(self, row: int, n: int) -> None:
        """The row's slots [0, n) are filled (a prefill's last act)."""
        self.lens_host[row] = n
        self.lens[row] = n

    def append(self, li: int, qkv: torch.Tensor, T: int, H: int, slot0: torch.Tensor, row: Optional[int] = None,
               table: Optional[torch.Tensor] = None) -> None:
        """Layer `li`: the post-rotary k / v columns of the fused qkv buffer -> slots [slot0[b], slot0[b] + T) of every row (qkv: rows * T rows; a row
        with slot0 < 0 is skipped), or - with `row` - of that one row (qkv: T rows, slot0 (1,)), or - with `table` (n, max_pages_per_seq), gathered
        rows of the block table - of those n sequences (qkv: n * T rows, slot0 (n,)); in the cache's own format."""
        if table is None:
            table = self.block_table if row is None else self.block_table[row:row + 1]
        self._fmt.append(qkv, *(t[li] for t in self._fmt.pools), table, slot0, T, H)

    def attend(self, li: int, q: torch.Tensor, H: int, max_len: int, scale: float, ws: torch.Tensor, out: Optional[torch.Tensor],
               lens: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Layer `li`: one query row per (row, query head) against the row's own slots [0, lens[row]) (`lens`: the cache's, or the caller's (rows,)
        int32 - a decode step attends over the lengths it is about to commit); `max_len` is the host's upper bound on them."""
        return self._fmt.attend(q, *(t[li] for t in self._fmt.pools), self.block_table, self.lens if lens is None else lens, H, max_len, scale, ws=ws,
                                out=out)

    def extend_attend(self, li: int, q: torch.Tensor, H: int, Tn: int, max_len0: int, scale: float, ws: torch.Tensor, out: Optional[torch.Tensor],
                      table: torch.Tensor, len0: torch.Tensor) -> torch.Tensor:
        """Layer `li`: Tn query rows per (sequence, query head) of the sequences `table` (n, max_pages_per_seq) describes, each behind its own
        len0 (n,) int32 filled slots and over its new rows, which `append` has already written (ops.attention_extend_paged, ops.attention_extend_paged_mxfp4kv)."""
        return self._fmt.extend(q, *(t[li] for t in self._fmt.pools), table, len0, H, Tn, max_len0, scale, ws=ws, out=out)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for layers in self._fmt.pools for t in layers)

    def extend_workspace(self, n: int, Tn: int, H: int, max_len0: int) -> torch.Tensor:
        """The paged extend attention's fp32 partials for n sequences of Tn new rows behind at most max_len0 slots, sized by the library's rule."""
        need = self._fmt.extend_ws(n, Tn, H, self.Dh, max_len0, self.Hkv, self.dtype)
        if self._ws_extend is None or self._ws_extend.numel() < need:
            self._ws_extend = torch.empty(max(need, 1), dtype=torch.float32, device=self.lens.device)
        return self._ws_extend

    def workspace(self, H: int) -> torch.Tensor:
        """The decode attention's fp32 partials, sized once for the longest sequence a table row can describe."""
        need = self._fmt.decode_ws(self.rows, H, self.Dh, self.max_pages_per_seq * ops.KV_PAGE)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1), dtype=torch.float32, device=self.lens.device)
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
        return _select(logits, self, self.uniforms(step, logits.shape[0], logits.device))


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

    @classmethod
    def after_plain_loop(cls, cache: KVCache, seq: torch.Tensor, eos: Optional[torch.Tensor], fed0: int) -> "GenerationState":
        """The state behind the plain loop: of the n emitted tokens seq (B, n) the stack has consumed the first n - 1 (slots fed0 .. fed0 + n - 2).  A
        sequence's real tokens end with its first eos: the pads behind it that were fed are masked out and its next position is set back by their
        number; its last real token is pending iff it was never fed (the sequence did not finish before the last step)."""
        B, n = seq.shape
        real = torch.full((B,), n, dtype=torch.int64, device=seq.device)
        if eos is not None:
            hit = torch.isin(seq, eos)
            real = torch.where(hit.any(dim=1), hit.long().argmax(dim=1) + 1, real)
        j = torch.arange(n - 1, device=seq.device)[None]
        cache.key_mask[:, fed0:fed0 + n - 1] = (j < real[:, None]).to(torch.uint8)
        cache.next_pos = cache.next_pos - (n - 1 - real).clamp_min(0)
        return cls(cache=cache, pending=torch.where(real == n, seq[:, -1], torch.full_like(real, -1)))


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


# ---- the parts of `SetokimLlamaPrefill.generate` (llama.py): the refusals, feeding the prompt, and the three loops -----------------------------------
_SAMPLING_ARGS = ("temperature", "top_p", "top_k", "num_beams", "penalty_alpha", "repetition_penalty")      # generate(): named so that they are refused by name


# A `generate` call once `check_request` has let it through: `eos_ids` a list or None, K drafts per round and C beam candidates per step (0 without).
Request = namedtuple("Request", "comp_images max_new eos_ids pad_token_id kv_cache sampler prefill_chunk cache_capacity past draft K beams C processors "
                                "as_dict want_hidden want_logits want_scores want_past")


def check_request(lm, *, comp_images, images, position_ids, max_new_tokens, eos_token_id, pad_token_id, do_sample, return_dict_in_generate,
                  output_hidden_states, output_logits, kv_cache, sampler, prefill_chunk, return_past, past, cache_capacity, draft, beams, processors,
                  output_scores, unsupported) -> Request:
    """Every refusal of `lm.generate` (lm: a SetokimLlamaPrefill) that needs no device call, in the order they have always fired, and the request
    the rest of the call works from."""
    who = "SetokimLlamaPrefill.generate"
    lm.model._refuse_unmerged(who)
    sampling = [k for k in _SAMPLING_ARGS if unsupported.get(k) is not None]
    if do_sample or sampling:
        raise NotImplementedError(f"{who}: greedy decoding (do_sample=False, no {', '.join(sampling) or 'sampling arguments'}) "
                                  "is the implemented mode; sampling and beam search are not implemented on the HIP path")
    unknown = [k for k in unsupported if k not in _SAMPLING_ARGS]
    if unknown:
        raise TypeError(f"{who}: unexpected arguments {unknown}")
    if images is not None:
        if comp_images is not None:
            raise ValueError(f"{who}: pass the images as `comp_images` or as `images`, not both")
        comp_images = images
    if max_new_tokens < 1:
        raise ValueError(f"{who}: max_new_tokens must be at least 1")
    if kv_cache not in KVCache.FORMATS:
        raise ValueError(f"{who}: kv_cache={kv_cache!r} is not one of 'native', 'fp8', 'mxfp4'")
    check_kv_head_dim(kv_cache, lm.model.head_dim, who, "kv_cache")
    if sampler is not None and not isinstance(sampler, Sampler):
        raise TypeError(f"{who}: sampler must be a generation.Sampler or None, got {type(sampler).__name__}")
    K = 0
    if draft is not None:
        if not isinstance(draft, Drafter):
            raise TypeError(f"{who}: draft must be a generation.Drafter or None, got {type(draft).__name__}")
        K = draft.K
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= ops.SPEC_MAX_K:
            raise ValueError(f"{who}: draft.K={K!r} must be an int in [1, {ops.SPEC_MAX_K}]")
        if kv_cache not in KVCache.EXTENDABLE:
            raise NotImplementedError(f"{who}: draft= with kv_cache='fp8' is not implemented (a round extends the cache by "
                                      "K + 1 tokens, and the extend attention over e4m3fn rows is a follow-up kernel); use kv_cache='native'")
    if beams is not None:
        if not isinstance(beams, BeamSearch):
            raise TypeError(f"{who}: beams must be a generation.BeamSearch or None, got {type(beams).__name__}")
        for name, given in (("sampler=", sampler is not None), ("draft=", draft is not None), ("past=", past is not None),
                            ("return_past=True", bool(return_past))):
            if given:
                raise NotImplementedError(f"{who}: beams= with {name} is not implemented (beam sampling, drafting into beams and continuing a beam state are not built)")
    eos_ids = None if eos_token_id is None else [eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id)
    n_eos = 0 if eos_ids is None else len(eos_ids)
    C = 0 if beams is None else beams.candidates(n_eos, lm.lm_head.weight.shape[0])
    if processors is not None:
        if not isinstance(processors, LogitsProcessors):
            raise TypeError(f"{who}: processors must be a generation.LogitsProcessors or None, got {type(processors).__name__}")
        if beams is not None:
            raise NotImplementedError(f"{who}: processors= with beams= is not implemented (HF applies its processors to the beams' log-probabilities, which is a different rule)")
        if past is not None:
            raise NotImplementedError(f"{who}: processors= with past= is not implemented (a GenerationState keeps no history of the earlier turns)")
        if processors.min_new_tokens > 0 and n_eos > ops.LOGITS_MAX_IDS:
            raise ValueError(f"{who}: min_new_tokens with {n_eos} eos ids exceeds the {ops.LOGITS_MAX_IDS} a step bans")
    if output_scores and (processors is None or not return_dict_in_generate):
        raise ValueError(f"{who}: output_scores=True needs processors= (the scores are the processed logits) and return_dict_in_generate=True (they are GenerateOutput.scores)")
    for name, v in (("prefill_chunk", prefill_chunk), ("cache_capacity", cache_capacity)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 1):
            raise ValueError(f"{who}: {name}={v!r} must be an integer >= 1 (or None)")
    if return_past and not return_dict_in_generate:
        raise ValueError(f"{who}: return_past=True needs return_dict_in_generate=True (the state is GenerateOutput.past)")
    if past is not None:
        if not isinstance(past, GenerationState):
            raise TypeError(f"{who}: past must be a generation.GenerationState (GenerateOutput.past), got {type(past).__name__}")
        if position_ids is not None:
            raise ValueError(f"{who}: with past= the new turn's positions continue from the cache; position_ids must be None")
        if not past.cache.extendable:
            raise NotImplementedError(f"{who}: continuing from an fp8 KV cache is not implemented (the extend attention "
                                      "over e4m3fn rows is a follow-up kernel); generate the first turn with kv_cache='native'")
        if past.cache.dtype != lm.model.norm.weight.dtype or past.cache.num_layers != len(lm.model.layers):
            raise ValueError(f"{who}: past holds a {past.cache.dtype} cache of {past.cache.num_layers} layers, the model "
                             f"runs {len(lm.model.layers)} layers in {lm.model.norm.weight.dtype}")
    return Request(comp_images, max_new_tokens, eos_ids, pad_token_id, kv_cache, sampler, prefill_chunk, cache_capacity, past, draft, K, beams, C,
                   processors, bool(return_dict_in_generate), bool(output_hidden_states), bool(output_logits), bool(output_scores), bool(return_past))


def feed_prompt(lm, req: Request, w_e, embeds, am, pos, sliding_window, dev):
    """The spliced prompt `embeds` (B, T, D), mask and positions (`lm._embed`'s result) - with `req.past` the new turn behind the pending tokens' column -
    into a filled cache.  Returns (h (B, D): every sequence's last attended state, the cache, the eos ids on the device or None, the pad id or None)."""
    who = "SetokimLlamaPrefill.generate"
    B, T, D = embeds.shape
    past, len0 = req.past, 0
    if past is not None:
        if past.cache.B != B or past.pending.shape != (B,):
            raise ValueError(f"{who}: past holds {past.cache.B} sequences, the new turn {B}")
        len0 = past.cache.len
        pend = past.pending.to(dev)
        front = ops.splice_rows(pend.clamp_min(0).to(torch.int32).reshape(B, 1), w_e, None)       # the pending tokens' embedding rows, one column
        embeds = torch.cat([front, embeds.to(device=dev, dtype=front.dtype)], dim=1)
        turn = torch.ones((B, T), dtype=torch.int64, device=dev) if am is None else am.to(dev).long()
        am = torch.cat([(pend >= 0).long()[:, None], turn], dim=1)
        T += 1
    if sliding_window is not None and int(sliding_window) < len0 + T + req.max_new:
        raise NotImplementedError(f"{who}: sliding_window={sliding_window} is shorter than prompt + max_new_tokens "
                                  f"({len0 + T} + {req.max_new} positions): windowed attention is not implemented on the HIP path")
    windows = req.prefill_chunk is not None and req.prefill_chunk < T             # the prompt is really cut (N >= T is the unchunked path)
    if windows and pos is not None:
        raise ValueError(f"{who}: prefill_chunk windows take their positions from the cache; position_ids must be None")
    if windows and req.kv_cache not in KVCache.EXTENDABLE:
        raise NotImplementedError(f"{who}: prefill_chunk with kv_cache='fp8' is not implemented (the extend attention over e4m3fn rows is a follow-up kernel)")
    if am is not None:
        am = am.to(dev)
        if pos is None and past is None:                                       # HF generate's rule for a padded prompt without position_ids
            pos = (am.long().cumsum(-1) - 1).masked_fill(am == 0, 1)
    eos = pad = None
    if req.eos_ids is not None:
        eos = torch.as_tensor(req.eos_ids, dtype=torch.int64, device=dev)
        pad = int(eos[0]) if req.pad_token_id is None else int(req.pad_token_id)
    need = len0 + T + req.max_new + req.K                                      # (K = 0 without a draft: a round may fill K slots it gives back)
    if past is None:
        cache = KVCache.for_model(lm.model, B, max(need, req.cache_capacity or 0), dev, kv_format=req.kv_cache)
    else:
        cache = past.cache if past.cache.cap >= need else past.cache.grown(max(need, req.cache_capacity or 0))
    # windows of the prompt (the whole prompt or new turn is the one-window case): the first window of a fresh prompt is a prefill, everything else
    # extends the cache; each sequence's last attended row is looked up in the window that holds it
    N = req.prefill_chunk if windows else max(T, 1)
    embeds = embeds.to(dev)
    h = None
    for c0 in range(0, T, N):
        c1 = min(c0 + N, T)
        amw = None if am is None else am[:, c0:c1]
        if past is None and c0 == 0:
            hidden = lm.model.prefill(embeds[:, c0:c1], amw, None if pos is None else pos[:, c0:c1], cache)
        else:
            hidden = lm.model.extend(embeds[:, c0:c1], cache, amw)
        if amw is None:
            h = hidden[:, -1].contiguous()
            continue
        last = (amw.bool() * torch.arange(c1 - c0, device=dev)[None]).max(dim=1).values
        hw = hidden[torch.arange(B, device=dev), last]
        h = hw.contiguous() if h is None else torch.where(amw.bool().any(dim=1)[:, None], hw, h)
    return h, cache, eos, pad


def _raise_undrawable(raws) -> None:
    """generate(sampler=...): `raws` holds every step's tokens as drawn, (B,) each, -1 where a row's logits could not be drawn from."""
    if not raws:
        return
    bad = (torch.stack(raws, dim=1) < 0).nonzero().cpu().tolist()                  # (sequence, step) pairs, sequence-major
    if bad:
        b, s = min(bad, key=lambda bs: (bs[1], bs[0]))                             # the first step, its first sequence
        raise RuntimeError(f"SetokimLlamaPrefill.generate: the logits of sequence {b} at step {s} contain a NaN or +inf, or no finite entry: "
                           f"no token can be drawn ((sequence, step) pairs affected: {bad[:8]}{' ...' if len(bad) > 8 else ''})")


def _select(scores: torch.Tensor, sampler: Optional[Sampler], u: Optional[torch.Tensor]) -> torch.Tensor:
    """scores (rows, V) -> the rows' tokens, int64: the argmax, or ONE `setok_sample_rows` launch on the uniforms u (rows,): -1 = the row cannot be drawn from."""
    if sampler is None:
        return ops.argmax_rows(scores)
    return ops.sample_rows(scores, u, sampler.temperature, sampler.top_k, sampler.top_p)


def _decode_ids(lm, w_e, ids: torch.Tensor, cache: KVCache) -> torch.Tensor:
    # ids (rows,) int64 -> embed_tokens' rows -> one `decode_step`: the states (rows, D) the next tokens are selected from
    e = ops.splice_rows(ids.to(torch.int32).reshape(-1, 1), w_e, None)
    return lm.model.decode_step(e.reshape(ids.shape[0], -1), cache)


def loop_plain(lm, req: Request, w_lm, w_e, h, cache, eos, pad, prompt_ids, prompt_mask):
    """One token per step from the last attended state `h` (B, D) on: lm_head, the processors, `_select`, `_decode_ids`; with an eos one host read per step."""
    B, dev, sampler = h.shape[0], h.device, req.sampler
    proc = None if req.processors is None else req.processors.begin(B, dev, prompt_ids, prompt_mask, req.max_new, eos)
    fed0 = cache.len                                                           # the first slot a decode step of this call fills
    finished = torch.zeros(B, dtype=torch.bool, device=dev)
    toks, hids, lgs, scs = [], [], [], []
    raws = []                                                                  # sampler only: the tokens as drawn, -1 where a row could not be drawn from
    for step in range(req.max_new):
        logits = ops.linear(h, w_lm)                                           # (B, V): never copied to the host
        scores = logits if proc is None else proc.process(logits)              # (B, V) fp32 with processors: what the token is selected from
        tok = raw = _select(scores, sampler, None if sampler is None else sampler.uniforms(step, B, dev))
        if sampler is not None:
            raws.append(raw)
            tok = raw.clamp_min(0)                                             # a valid row for the embedding lookup; the error is raised below
        if eos is not None:
            tok = torch.where(finished, torch.full_like(tok, pad), tok)
            finished = finished | torch.isin(tok, eos)
        toks.append(tok)
        if proc is not None:
            proc.append(tok.reshape(B, 1))
        if req.want_hidden:
            hids.append(h)
        if req.want_logits:
            lgs.append(logits)
        if req.want_scores:
            scs.append(scores)
        if step + 1 == req.max_new:
            break
        if eos is not None:
            stop = finished.all() if sampler is None else finished.all() | (raw < 0).any()
            if bool(stop):                                                     # the one host read per step
                _raise_undrawable(raws)                                        # raises iff a row could not be drawn; else every sequence has finished
                break
        h = _decode_ids(lm, w_e, tok, cache)
    _raise_undrawable(raws)
    seq = torch.stack(toks, dim=1)
    if not req.as_dict:
        return seq
    return GenerateOutput(sequences=seq, hidden_states=torch.stack(hids, dim=1) if req.want_hidden else None,
                          logits=torch.stack(lgs, dim=1) if req.want_logits else None,
                          past=GenerationState.after_plain_loop(cache, seq, eos, fed0) if req.want_past else None,
                          scores=torch.stack(scs, dim=1) if req.want_scores else None)


def loop_beams(lm, req: Request, w_lm, w_e, h, cache, eos, pad):
    """The loop with beam search, from the last attended state `h` (B, D) on.  The running scores, the finished set and the back-pointers live on
    the device (ops.BeamState); the host reads `setok_beam_advance`'s 2-int summary once per step, and the hypotheses are materialised from the
    back-pointers once at the end."""
    beams, max_new = req.beams, req.max_new
    B, n, R, dev = h.shape[0], beams.num_beams, beams.num_return_sequences, h.device
    state = ops.BeamState(B, n, max_new, dev)
    cache = cache.expanded(n)
    fed0 = cache.len                                                           # the first slot a decode step of this call fills: what `reorder` moves starts here
    running0 = torch.zeros((B, 1), dtype=torch.float32, device=dev)            # step 0: one row per sequence, score 0
    ws = torch.empty(B * n * (2 * ops.BEAM_MAX_C + 1), dtype=torch.int32, device=dev)
    hids, lgs = [], []
    for step in range(max_new):
        logits = ops.linear(h, w_lm)                                           # (B, V) at step 0, then (B * n, V)
        cand = ops.beam_topk(logits, running0 if step == 0 else state.run_score, req.C, ws)
        tok, src_row, summary = ops.beam_advance(*cand, state, eos, step, beams.length_penalty, beams.early_stopping)
        if req.want_hidden:
            hids.append(h.repeat_interleave(n, dim=0) if step == 0 else h)
        if req.want_logits:
            lgs.append(logits.repeat_interleave(n, dim=0) if step == 0 else logits)
        go_on, bad = summary.tolist()                                          # the step's one host read
        if bad:
            rows = torch.nonzero(cand[3]).flatten().tolist()
            raise RuntimeError(f"SetokimLlamaPrefill.generate: the logits of sequence(s) {rows} hold a NaN or +inf at beam-search step {step}")
        if not go_on:
            break
        cache.reorder(src_row, fed0, n)
        h = _decode_ids(lm, w_e, tok, cache)
    # the returned hypotheses: the first R entries of every finished set, walked back through the parents
    length = state.fin_len[:, :R].reshape(B * R).long().clamp_min(1)
    beam = state.fin_parent[:, :R].reshape(B * R).long()
    n_new = int(length.max())
    base = (torch.arange(B, device=dev) * n).repeat_interleave(R)
    rows = torch.arange(B * R, device=dev)
    seq = torch.full((B * R, n_new), pad, dtype=torch.int64, device=dev)
    anc = torch.full((B * R, n_new), -1, dtype=torch.int64, device=dev)
    seq[rows, length - 1] = state.fin_token[:, :R].reshape(B * R)
    anc[rows, length - 1] = base + beam
    for j in range(n_new - 2, -1, -1):
        live = j <= length - 2                                                 # token j of these hypotheses belongs to running beam `beam` after step j
        at = base + beam
        parent = state.bp_parent[j][at].long()
        seq[:, j] = torch.where(live, state.bp_token[j][at], seq[:, j])
        anc[:, j] = torch.where(live, base + parent, anc[:, j])
        beam = torch.where(live, parent, beam)
    if not req.as_dict:
        return seq

    def along(kept):                                                           # (steps, B * n, X) -> (B * R, n_new, X): row j from the state that produced token j
        got = torch.stack(kept[:n_new], dim=0)[torch.arange(n_new, device=dev)[None], anc.clamp_min(0)]
        return got * (anc >= 0)[..., None].to(got.dtype)

    return GenerateOutput(sequences=seq, hidden_states=along(hids) if req.want_hidden else None, logits=along(lgs) if req.want_logits else None,
                          sequences_scores=state.fin_score[:, :R].reshape(B * R).clone(), beam_indices=anc.to(torch.int32))


def loop_speculative(lm, req: Request, w_lm, w_e, h, cache, eos, pad, prompt_ids, prompt_mask):
    """The loop with a drafter, from the last attended state `h` (B, D) on.  Between rounds the state lives on the device: pending (B,) int64,
    count (B,) int32, finished (B,) uint8 and seq (B, max_new) int64; `setok_spec_accept` advances it, and the host reads the kernel's 3-int
    summary once per round.  With processors the K + 1 rows of a round are processed in one launch (row i sees the history plus drafts
    0 .. i - 1) before the selection, and the emitted tokens join the history behind the accept rule."""
    draft, K, sampler, max_new = req.draft, req.K, req.sampler, req.max_new
    (B, D), dev = h.shape, h.device
    seq = torch.full((B, max_new), pad, dtype=torch.int64, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    finished = torch.zeros(B, dtype=torch.uint8, device=dev)
    pending = torch.zeros(B, dtype=torch.int64, device=dev)
    summary = torch.zeros(3, dtype=torch.int32, device=dev)
    u = None if sampler is None else sampler.uniform_matrix(max_new, B, dev)
    steps = torch.arange(K + 1, device=dev, dtype=torch.int64)[None]
    rows_b = torch.arange(B, device=dev)[:, None]
    outs = {}                                                                  # "hidden" / "logits" / "scores": (B, max_new + 1, X); column max_new takes the rows no sequence emitted
    proc = None if req.processors is None else req.processors.begin(B, dev, prompt_ids, prompt_mask, max_new, eos)

    def verify(hidden, d, tail, slot):
        # hidden (B * n, D), the states behind the pending token and the n - 1 drafts d: select, accept, keep rows -> (longest acceptance, live sequences)
        n = d.shape[1] + 1
        logits = ops.linear(hidden, w_lm)
        scores = logits if proc is None else proc.process(logits, tail)
        ur = None if sampler is None else u[(count.long()[:, None] + steps[:, :n]).clamp_max(max_new - 1), rows_b].reshape(B * n).contiguous()
        sel = _select(scores, sampler, ur).reshape(B, n)
        before = count.clone()
        emitted, m, _ = ops.spec_accept(d, sel, eos, seq, count, finished, pending, cache.key_mask, cache.next_pos, slot, summary=summary)
        cols = torch.where(steps[:, :n] < m.long()[:, None], before.long()[:, None] + steps[:, :n], torch.full_like(steps[:, :n], max_new))
        for name, want, rows in (("hidden", req.want_hidden, hidden), ("logits", req.want_logits, logits), ("scores", req.want_scores, scores)):
            if want:                                                           # row i < m[b] of sequence b -> column before[b] + i
                if name not in outs:
                    outs[name] = torch.zeros((B, max_new + 1, rows.shape[-1]), dtype=rows.dtype, device=dev)
                outs[name][rows_b, cols] = rows.reshape(B, n, -1)
        if proc is not None:
            proc.append(emitted, m)
        draft.update(emitted, m)
        mx, live, bad = summary.tolist()                                       # the round's one host read
        if bad:
            c = int(count.max())
            drawn = torch.where((seq[:, :c] < 0) & (torch.arange(c, device=dev)[None] < count[:, None]), -1, 0)
            _raise_undrawable(list(drawn.unbind(dim=1)))
        return mx, live

    cache.next_pos = cache.next_pos.contiguous()
    draft.begin(B, dev, prompt_ids, prompt_mask, max_new)
    # step 0: the token selected from the last attended state, put into the loop state by the accept rule with no drafts
    _, live = verify(h, torch.empty((B, 0), dtype=torch.int64, device=dev), None, cache.len)
    cache.key_mask[:, cache.len] = 0                                           # (nothing was fed: the slot the rule marked is not filled yet)
    while live > 0:
        if cache.len + K + 1 > cache.cap:
            cache = cache.grown(2 * cache.cap)
        d = draft.propose(pending)
        if not (isinstance(d, torch.Tensor) and d.dtype == torch.int64 and tuple(d.shape) == (B, K)):
            raise TypeError(f"SetokimLlamaPrefill.generate: draft.propose must return a (B, K) = ({B}, {K}) int64 tensor")
        d = d.to(dev).contiguous()
        live_b = finished == 0
        am = torch.cat([live_b[:, None], ((d >= 0).long().cummin(dim=1).values > 0) & live_b[:, None]], dim=1)
        ids = torch.cat([pending[:, None], d], dim=1).clamp_min(0).to(torch.int32)
        len0 = cache.len
        hidden = lm.model.extend(ops.splice_rows(ids, w_e, None), cache, am)   # (B, K + 1, D): one pass over the weights
        mx, live = verify(hidden.reshape(B * (K + 1), D), d, d, len0)
        cache.truncate(len0 + mx)
    n = int(count.max())
    out = seq[:, :n].contiguous()
    if not req.as_dict:
        return out
    kept = lambda name, want: outs[name][:, :n].contiguous() if want else None
    return GenerateOutput(sequences=out, hidden_states=kept("hidden", req.want_hidden), logits=kept("logits", req.want_logits),
                          past=GenerationState(cache=cache, pending=pending) if req.want_past else None, scores=kept("scores", req.want_scores))


# ---- continuous batching over the paged cache ---------------------------------------------------------------------------------------------------
@dataclass
class _Running:
    ticket: int
    max_new: int
    tokens: List[int]
    sampled: bool = False


@dataclass(eq=False)
class PrefixHandle:
    """What `ContinuousBatcher.register_prefix` returns: a prompt prefix of P rows whose Ps = 128 * (P // 128) leading slots live once in `pages`
    (the batcher holds one reference to each until `drop_prefix`), and the embeddings of its tail rows [Ps, P), which every request recomputes
    with its remainder."""
    owner: object
    P: int
    Ps: int
    pages: List[int]
    tail: torch.Tensor
    dropped: bool = False


class ContinuousBatcher:
    """Greedy - or, per request, sampled - decoding of many requests of different lengths on `rows` rows of one PagedKVCache: a request joins the running batch as soon as a row is
    idle and the pool can reserve the pages for ALL of its prompt + max_new_tokens slots, and leaves - its pages back in the pool - the step it emits
    an eos id or its last token.  Because a request's pages are reserved up front, a running request never runs out of pages: nothing is preempted.

    `submit(prompt, max_new_tokens)` queues a request (spliced embeddings (T, D) or token ids (T,)) and returns its ticket; `step()` is one round of
    the loop and returns the (ticket, tokens) pairs that finished in it; `run(requests)` submits (prompt, max_new_tokens) pairs, steps until drained
    and returns the token tensors in submit order.  A request's tokens are `lm.generate(inputs_embeds=x[None], max_new_tokens=n, eos_token_id=...)`'s
    for that request alone - the new tokens, an eos included and nothing behind it: the paged attention gives the dense kernel's bits
    (include/setok_hip.h, "Paged KV cache") and every other kernel of a step computes a row from that row's operands alone.

    One step: admissions in FIFO order (nothing overtakes the queue's head) - `assign`, `LlamaModel.prefill_paged`, lm_head on the last state,
    argmax: the first token -, then ONE `LlamaModel.decode_step_paged` over all rows, lm_head at M = rows, argmax, and one host read of the step's
    tokens.  `stats`: steps, row_steps_active / row_steps_total (the occupancy of the decode steps), pages_high_water, admitted, admitted_midflight
    (requests that joined while others were running), page_waits (steps in which a row was idle but the head of the queue had to wait for pages),
    pages_reused (pages handed to a request after another one released them).

    Prompt prefixes are shared in whole pages: `register_prefix(prefix)` prefills the Ps = 128 * (P // 128) leading rows of a P-row prefix once, into
    pages of their own, and returns a handle; `submit(remainder, n, prefix=handle)` queues the request prefix ++ remainder, whose first table entries
    point at those pages (counted by reference: `PagedKVCache.assign(shared=)`) and whose admission runs only the P - Ps tail rows and the remainder
    through the stack - one `LlamaModel.extend_paged` behind Ps filled slots.  Its tokens are those of
    `lm.generate(inputs_embeds=full[None], max_new_tokens=n, prefill_chunk=Ps)` for that request alone (the same prefill and, while P - Ps + S <= Ps,
    one dense extend).  `drop_prefix(handle)` gives the batcher's references back; running requests keep their own, so the pages return to the pool
    when the last of them leaves.  `prefix_stats`: registered, hits (admissions behind a prefix), slots_shared (prompt rows that were not recomputed,
    summed over hits).

    `cache=`: a fresh `PagedKVCache` the caller built for this model - `PagedKVCache.for_model(lm.model, rows, num_pages, max_pages_per_seq,
    kv_format="mxfp4")` for MXFP4 pages - in the place of the native pools the batcher would build.  `num_pages` / `max_pages_per_seq` must then equal
    the cache's or be omitted; admission, prefixes and release run unchanged over whichever format the cache has.  Over MXFP4 pages a request's
    tokens are those of `lm.generate(..., kv_cache="mxfp4")` for that request alone, a prefixed request's those of the same call with
    `prefill_chunk=Ps`: the paged kernels run the dense MXFP4 kernels' arithmetic on the same partition of the keys.

    Sampling is per request: `submit(..., sampler=Sampler(temperature, top_k, top_p, u= | generator=))` - or a fourth element of a `run` tuple -
    makes that request a sampled one; the others stay greedy and sit next to it in the batch.  The request's j-th emitted token is drawn with
    u[j, 0] of ITS OWN stream, `u` (>= max_new_tokens, 1) float32; with `generator=` (or neither) the whole stream is ONE
    `torch.rand((max_new_tokens, 1), generator=...)` draw at admission - not the per-step draws `generate`'s plain loop makes from a generator, so
    only `u=` reproduces a `generate` call.  The first token is drawn from the admission's last state with u[0, 0], behind a prefix too.  The
    batcher keeps (rows,) device arrays of the three parameters - an idle or greedy row holds temperature 0 - and the rows' uniforms on the device
    by decode step; a step with at least one sampled running row selects for ALL rows with one `setok_sample_rows_each` launch, a step with none
    calls `argmax_rows` exactly as before (the same launches in the same order), and neither adds a host read.  A sampled request's tokens are
    those of `lm.generate(inputs_embeds=x[None], max_new_tokens=n, sampler=Sampler(temperature, top_k, top_p, u=u))` for that request alone.
    A row that cannot be drawn from (-1: a NaN or +inf in its logits, or no finite entry) does not raise as `generate` does: the request ends in
    that step - its row released, its pages back in the pool -, is reported in the step's result with the tokens drawn before it, and
    `errors[ticket]` holds the message; the other requests are unaffected, and `run` drains everything and then raises RuntimeError naming the
    failed tickets.  Not built (follow-ups): per-request `processors=`, n parallel samples over shared prompt pages, log-probabilities in the result.

    Refused by name (NotImplementedError): sampler= at the constructor (a sampler belongs to a request: `submit(sampler=)`), beams=, draft=,
    processors=, prefill_chunk= and a quantised kv_cache= string (quantised pages come in through `cache=`)."""

    def __init__(self, lm, rows: int, num_pages: Optional[int] = None, max_pages_per_seq: Optional[int] = None, eos_token_id=None, pad_token_id=None, *,
                 sampler=None, beams=None, draft=None, processors=None, prefill_chunk=None, kv_cache: str = "native", cache: Optional[PagedKVCache] = None):
        who = "ContinuousBatcher"
        if sampler is not None:
            raise NotImplementedError(f"{who}: sampler= is not an argument of the batcher: requests that share a batch each bring their own "
                                      "temperature, nucleus and random stream; pass it per request, submit(..., sampler=Sampler(...))")
        for name, given, why in (("beams=", beams is not None, "a beam's pages would have to be shared between rows"),
                                 ("draft=", draft is not None, "a verify pass over pages is not wired to LlamaModel.extend_paged yet"),
                                 ("processors=", processors is not None, "the rows' histories are not kept"),
                                 ("prefill_chunk=", prefill_chunk is not None, "a window over pages is not wired to LlamaModel.extend_paged yet")):
            if given:
                raise NotImplementedError(f"{who}: {name} is not implemented over the paged cache ({why}); use SetokimLlamaPrefill.generate")
        if kv_cache != "native":
            if kv_cache in KVCache.FORMATS:
                raise NotImplementedError(f"{who}: kv_cache={kv_cache!r} is not implemented over the paged cache: the pools the batcher builds hold the "
                                          "model's element type; for MXFP4 pages pass cache=PagedKVCache.for_model(lm.model, rows, num_pages, "
                                          "max_pages_per_seq, kv_format=\"mxfp4\")")
            raise ValueError(f"{who}: kv_cache={kv_cache!r} is not one of 'native', 'fp8', 'mxfp4'")
        lm.model._refuse_unmerged(who)
        _count(rows, "rows", who)
        if cache is not None:
            if not isinstance(cache, PagedKVCache):
                raise TypeError(f"{who}: cache= must be a PagedKVCache, got {type(cache).__name__}")
            for name, given, has in (("rows", rows, cache.rows), ("num_pages", num_pages, cache.num_pages),
                                     ("max_pages_per_seq", max_pages_per_seq, cache.max_pages_per_seq)):
                if given is not None and (isinstance(given, bool) or given != has):
                    raise ValueError(f"{who}: {name}={given!r} conflicts with cache= ({name} = {has}); omit it or pass the cache's value")
            if not cache.fresh:
                raise ValueError(f"{who}: cache= must be fresh - every row idle and every page free - but {cache.num_pages - cache.pages_free} of its "
                                 f"{cache.num_pages} pages are in use and its lengths are {cache.lens_host}")
            lm.model._check_paged(who, cache)
            num_pages, max_pages_per_seq = cache.num_pages, cache.max_pages_per_seq
        _count(num_pages, "num_pages", who)
        if max_pages_per_seq is None:
            max_pages_per_seq = num_pages
        _count(max_pages_per_seq, "max_pages_per_seq", who)
        self.lm, self.rows = lm, rows
        self.w_lm, self.w_e = lm.lm_head.weight.detach().contiguous(), lm.model.embed_tokens.weight.detach().contiguous()
        self.device = self.w_lm.device
        self.cache = cache if cache is not None else PagedKVCache.for_model(lm.model, rows, num_pages, max_pages_per_seq, self.device)
        self.eos_ids = None if eos_token_id is None else [eos_token_id] if isinstance(eos_token_id, int) else list(eos_token_id)
        self.pad_token_id = pad_token_id                                           # (kept for HF's signature: a finished request leaves, nothing is padded)
        self.queue: List[Tuple[int, torch.Tensor, int, Optional[PrefixHandle], Optional[Sampler]]] = []      # (ticket, prompt, max_new, prefix, sampler) in submit order
        self.running: List[Optional[_Running]] = [None] * rows
        self.cur = torch.zeros(rows, dtype=torch.int64, device=self.device)        # every row's latest token: the next decode step's input
        # per-request sampling: the rows' parameters (temperature 0 = an idle or greedy row: setok_sample_rows_each takes its argmax) and their
        # uniforms by decode step - row t - _u_t0 of `_u` is what decode step t draws with; an admission writes its request's column ahead
        self.temperature = torch.zeros(rows, dtype=torch.float32, device=self.device)
        self.top_k = torch.zeros(rows, dtype=torch.int32, device=self.device)
        self.top_p = torch.ones(rows, dtype=torch.float32, device=self.device)
        self._u = torch.zeros((0, rows), dtype=torch.float32, device=self.device)
        self._u_t0 = 0
        self._t = 0                                                                # decode steps taken
        self.errors: dict = {}                                                     # ticket -> why a sampled request ended early (an undrawable row)
        self._tickets = 0
        self._released: set = set()                                                # pages that went back to the pool at least once
        self.stats = dict(steps=0, row_steps_active=0, row_steps_total=0, pages_high_water=0, admitted=0, admitted_midflight=0, page_waits=0,
                          pages_reused=0)
        self.prefix_stats = dict(registered=0, hits=0, slots_shared=0)
        self._prefixes: List[PrefixHandle] = []                                    # the registered prefixes that have not been dropped

    @property
    def occupancy(self) -> float:
        return self.stats["row_steps_active"] / max(self.stats["row_steps_total"], 1)

    def _prompt_of(self, who: str, inputs_embeds, input_ids) -> torch.Tensor:
        """The one prompt tensor of a call that takes embeddings (T, D) or token ids (T,), checked."""
        if (inputs_embeds is None) == (input_ids is None):
            raise ValueError(f"{who}: pass the prompt as inputs_embeds (T, D) or as input_ids (T,), one of them")
        prompt = inputs_embeds if input_ids is None else input_ids
        if not isinstance(prompt, torch.Tensor):
            raise TypeError(f"{who}: the prompt must be a tensor, got {type(prompt).__name__}")
        D = self.w_e.shape[1]
        if prompt.is_floating_point():
            if prompt.dim() != 2 or prompt.shape[1] != D or input_ids is not None:
                raise ValueError(f"{who}: inputs_embeds {tuple(prompt.shape)} is not (T, D = {D})")
        elif prompt.dim() != 1 or prompt.dtype == torch.bool:
            raise ValueError(f"{who}: input_ids {tuple(prompt.shape)} {prompt.dtype} is not an integer (T,)")
        return prompt

    def _embeds(self, prompt: torch.Tensor) -> torch.Tensor:
        """A checked prompt as embeddings (T, D) on the device."""
        return prompt.to(self.device) if prompt.is_floating_point() else self._embed_ids(prompt)

    def _own(self, who: str, prefix) -> "PrefixHandle":
        if not isinstance(prefix, PrefixHandle) or prefix.owner is not self or prefix.dropped:
            raise ValueError(f"{who}: prefix= is not a live handle of this batcher's register_prefix (a dropped or a foreign one)")
        return prefix

    def register_prefix(self, inputs_embeds=None, input_ids=None) -> PrefixHandle:
        """Prefill the Ps = 128 * (P // 128) leading rows of a prompt prefix - (P, D) embeddings or (P,) ids - once, into Ps / 128 pages that requests
        then share (`submit(prefix=)`): `assign` on an idle row, `LlamaModel.prefill_paged` of prefix[:Ps] - so the pages hold the dense prefill's
        bits -, `detach`.  The handle keeps the pages and the embeddings of the tail rows [Ps, P).  ValueError for P < 128 (nothing to share) or a
        prefix that leaves a table row no entry of its own; RuntimeError, with nothing changed, without an idle row or Ps / 128 free pages now, and
        if holding these pages too would leave a queued request fewer pages than it needs of its own even in an empty batcher (a held prefix's pages
        leave the pool until `drop_prefix`, and a request that can never be admitted would block the queue for good).  If the prefill itself raises,
        the row is released first: it is idle again and its pages are free."""
        who = "ContinuousBatcher.register_prefix"
        prompt = self._prompt_of(who, inputs_embeds, input_ids)
        P = prompt.shape[0]
        Ps = ops.KV_PAGE * (P // ops.KV_PAGE)
        if Ps == 0:
            raise ValueError(f"{who}: a prefix of {P} rows fills no whole page of {ops.KV_PAGE} slots: there is nothing to share")
        n = Ps // ops.KV_PAGE
        if n >= self.cache.max_pages_per_seq:
            raise ValueError(f"{who}: the prefix's {n} shared pages leave a request none of its max_pages_per_seq = {self.cache.max_pages_per_seq}")
        idle = [r for r in range(self.rows) if self.running[r] is None]
        if not idle:
            raise RuntimeError(f"{who}: no idle row to prefill the prefix on (all {self.rows} rows run a request)")
        if n > self.cache.pages_free:
            raise RuntimeError(f"{who}: the prefix needs {n} free pages, the pool has {self.cache.pages_free} of {self.cache.num_pages}")
        room = self.cache.num_pages - self._pinned() - n                           # what an empty batcher could still hand out with this prefix held too
        for ticket, queued, max_new, pre, _ in self.queue:
            own = self._own_pages(queued.shape[0], max_new, pre)
            if own > room:
                raise RuntimeError(f"{who}: holding {n} more pages would leave the pool {room} pages for requests, and the queued request {ticket} "
                                   f"needs {own} of its own: it could never be admitted (register the prefix once it has been admitted, or drop another)")
        row, x = idle[0], self._embeds(prompt)
        self.cache.assign(row, Ps)
        try:
            self.lm.model.prefill_paged(x[None, :Ps], self.cache, row)
        except BaseException:
            self.cache.release(row)                                                # the row is idle again and the pages are back: nothing changed
            raise
        self.stats["pages_high_water"] = max(self.stats["pages_high_water"], self.cache.num_pages - self.cache.pages_free)
        handle = PrefixHandle(self, P, Ps, self.cache.detach(row), x[Ps:].to(self.w_e.dtype).clone())
        self._prefixes.append(handle)
        self.prefix_stats["registered"] += 1
        return handle

    def _pinned(self) -> int:
        """Pages the registered prefixes hold: the part of the pool no request can have as its own until a `drop_prefix`."""
        return sum(len(h.pages) for h in self._prefixes)

    @staticmethod
    def _own_pages(T: int, max_new: int, prefix: Optional[PrefixHandle]) -> int:
        """Pages a request must take off the free list: all of its prompt's + max_new slots' pages but the shared ones."""
        P, shared = (0, 0) if prefix is None else (prefix.P, len(prefix.pages))
        return (P + T + max_new + ops.KV_PAGE - 1) // ops.KV_PAGE - shared

    def drop_prefix(self, handle: PrefixHandle) -> None:
        """Give the batcher's references to the prefix's pages back.  Running requests keep their own: the pages return to the pool when the last of
        them leaves.  ValueError for a dropped or foreign handle, and while a queued request names it."""
        who = "ContinuousBatcher.drop_prefix"
        self._own(who, handle)
        if any(entry[3] is handle for entry in self.queue):
            raise ValueError(f"{who}: a queued request names this prefix (drop it once the request has been admitted)")
        self._released.update(p for p in handle.pages if self.cache.page_refs[p] == 1)
        self.cache.drop(handle.pages)
        handle.dropped = True
        self._prefixes.remove(handle)

    def submit(self, inputs_embeds=None, max_new_tokens: int = 1, input_ids=None, prefix: Optional[PrefixHandle] = None,
               sampler: Optional[Sampler] = None) -> int:
        """Queue one request: its spliced prompt embeddings (T, D), or its token ids (T,) (as `input_ids=`, or an integer tensor in the first place).
        With `prefix=` (a handle of `register_prefix`) the prompt argument is the remainder behind the prefix, S >= 1 rows, and the request's prompt
        is prefix ++ remainder.  With `sampler=` (a `Sampler`) the request's tokens are drawn instead of taken by argmax: token j with u[j, 0] of
        the sampler's `u` (>= max_new_tokens, 1), or - with a generator, or neither - of one `torch.rand((max_new_tokens, 1), generator=...)` draw
        made at admission.  Returns the ticket.  ValueError - the queue and the cache untouched - if the prompt's + max_new_tokens slots cannot
        fit in max_pages_per_seq pages, or could never fit in the pool - the pool less the pages the registered prefixes hold, which no request can
        have as its own until a `drop_prefix` -, for a dropped or foreign handle, and for a sampler whose `u` is not (>= max_new_tokens, 1);
        TypeError for a `sampler=` that is not a `Sampler`."""
        who = "ContinuousBatcher.submit"
        prompt = self._prompt_of(who, inputs_embeds, input_ids)
        _count(max_new_tokens, "max_new_tokens", who)
        if sampler is not None:
            if not isinstance(sampler, Sampler):
                raise TypeError(f"{who}: sampler= must be a Sampler, got {type(sampler).__name__}")
            if sampler.u is not None and (sampler.u.shape[0] < max_new_tokens or sampler.u.shape[1] != 1):
                raise ValueError(f"{who}: the sampler's u has shape {tuple(sampler.u.shape)}; a request's stream is (at least max_new_tokens = "
                                 f"{max_new_tokens}, 1): row j draws its j-th token")
        T = prompt.shape[0]
        if T < 1:
            raise ValueError(f"{who}: an empty prompt")
        if prefix is not None:
            self._own(who, prefix)
        pinned = self._pinned()
        own = self._own_pages(T, max_new_tokens, prefix)
        held = f", of which registered prefixes hold {pinned}" if pinned else ""
        if prefix is None:
            if own > self.cache.max_pages_per_seq or own > self.cache.num_pages - pinned:
                raise ValueError(f"{who}: {T} + {max_new_tokens} slots need {own} pages; a sequence has at most max_pages_per_seq = "
                                 f"{self.cache.max_pages_per_seq} and the pool num_pages = {self.cache.num_pages}{held}")
        else:
            pages = own + len(prefix.pages)
            if pages > self.cache.max_pages_per_seq or own > self.cache.num_pages - pinned:
                raise ValueError(f"{who}: {prefix.P} + {T} + {max_new_tokens} slots need {pages} pages, {own} of them the "
                                 f"request's own behind the prefix's {len(prefix.pages)} shared ones; a sequence has at most max_pages_per_seq = "
                                 f"{self.cache.max_pages_per_seq} and the pool num_pages = {self.cache.num_pages}{held}")
        ticket, self._tickets = self._tickets, self._tickets + 1
        self.queue.append((ticket, prompt, max_new_tokens, prefix, sampler))
        return ticket

    def _tokens_of(self, h: torch.Tensor) -> torch.Tensor:
        """States (M, D) -> lm_head -> the rows' argmax, (M,) int64 on the device."""
        return ops.argmax_rows(ops.linear(h, self.w_lm))

    def _stream_of(self, row: int, sampler: Sampler, max_new: int) -> torch.Tensor:
        """A sampled admission: the request's parameters into the row's entries of the device arrays, its uniforms u[1:] into the row's column of
        `_u` at the decode steps that will draw with them (a running row decodes in every step from its admission's on).  Returns u[0], (1,)."""
        dev = self.device
        if sampler.u is None:                                                      # the whole stream at once: one draw per request
            u = torch.rand((max_new, 1), generator=sampler.generator, dtype=torch.float32,
                           device=dev if sampler.generator is None else sampler.generator.device).to(dev)
        else:
            u = sampler.u[:max_new].to(dev)
        self.temperature[row], self.top_k[row], self.top_p[row] = sampler.temperature, sampler.top_k, sampler.top_p
        ahead, lo = max_new - 1, self._t - self._u_t0
        if lo + ahead > self._u.shape[0]:                                          # regrow from the current step on: earlier rows are spent
            keep = max(self._u.shape[0] - lo, 0)
            grown = torch.zeros((max(2 * keep, ahead, 16), self.rows), dtype=torch.float32, device=dev)
            grown[:keep] = self._u[self._u.shape[0] - keep:]
            self._u, self._u_t0, lo = grown, self._t, 0
        if ahead:
            self._u[lo:lo + ahead, row] = u[1:, 0]
        return u[0]

    def _embed_ids(self, ids: torch.Tensor) -> torch.Tensor:
        """Token ids (M,) -> embed_tokens' rows (M, D)."""
        return ops.splice_rows(ids.to(device=self.device, dtype=torch.int32).reshape(-1, 1), self.w_e, None).reshape(ids.shape[0], -1)

    def _admit(self) -> List[int]:
        """Admissions of this step, FIFO: the rows that got a request, each with its first token in `cur`."""
        cache, st, fresh = self.cache, self.stats, []
        while self.queue:
            idle = [r for r in range(self.rows) if self.running[r] is None]
            if not idle:
                break
            ticket, prompt, max_new, prefix, sampler = self.queue[0]
            row, T = idle[0], prompt.shape[0]
            shared = [] if prefix is None else prefix.pages
            if not cache.assign(row, (0 if prefix is None else prefix.P) + T + max_new, shared=shared):
                if all(r is None for r in self.running):                           # nobody will ever release a page: refuse by name, never spin
                    raise RuntimeError(f"ContinuousBatcher.step: request {ticket} at the head of the queue needs "
                                       f"{self._own_pages(T, max_new, prefix)} pages of its own and no request is running, but only {cache.pages_free} "
                                       f"of {cache.num_pages} pages are free ({self._pinned()} are held by registered prefixes): drop a prefix")
                st["page_waits"] += 1                                             # a row is idle, the pages are not there yet: nothing overtakes
                break
            self.queue.pop(0)
            st["admitted"] += 1
            st["admitted_midflight"] += int(any(self.running[r] is not None and r not in fresh for r in range(self.rows)))
            st["pages_reused"] += sum(p in self._released for p in cache.pages_of(row)[len(shared):])
            x = self._embeds(prompt)
            if prefix is None:
                h = self.lm.model.prefill_paged(x[None], cache, row)
            else:                                                                  # the shared slots are filled: only the prefix's tail and the remainder run
                cache.set_len(row, prefix.Ps)
                h = self.lm.model.extend_paged(torch.cat([prefix.tail, x.to(prefix.tail.dtype)])[None], cache, [row])
                self.prefix_stats["hits"] += 1
                self.prefix_stats["slots_shared"] += prefix.Ps
            if sampler is None:
                self.cur[row:row + 1] = self._tokens_of(h[:, -1].contiguous())
            else:                                                                  # the first token: drawn from the admission's last state with u[0]
                u0 = self._stream_of(row, sampler, max_new)
                self.cur[row:row + 1] = ops.sample_rows(ops.linear(h[:, -1].contiguous(), self.w_lm), u0, sampler.temperature, sampler.top_k,
                                                        sampler.top_p)
            self.running[row] = _Running(ticket, max_new, [], sampler is not None)
            fresh.append(row)
        st["pages_high_water"] = max(st["pages_high_water"], cache.num_pages - cache.pages_free)
        return fresh

    def step(self) -> List[Tuple[int, torch.Tensor]]:
        """One round: admissions with their prefills, one decode step over all rows, one host read, releases.  Returns [(ticket, tokens (n,) int64)]
        of the requests that finished in it - a sampled request that could not be drawn from among them, with the tokens drawn before and its
        message in `errors`."""
        fresh = self._admit()
        if all(r is None for r in self.running):
            return []
        first = self.cur.clone() if fresh else None                               # the admitted rows' first tokens (the decode step overwrites `cur`)
        # a running row decodes unless it was admitted with max_new_tokens = 1: its first token is its last
        flags = [r is not None and not (i in fresh and r.max_new == 1) for i, r in enumerate(self.running)]
        if any(flags):
            active = torch.tensor(flags, dtype=torch.bool, device=self.device)
            sampled = any(f and r.sampled for f, r in zip(flags, self.running))
            if not sampled:
                h = self.lm.model.decode_step_paged(self._embed_ids(self.cur), self.cache, active, active_host=flags)
                self.cur = self._tokens_of(h)
            else:                                                                  # one launch selects for all rows; a -1 (read below) embeds as token 0
                h = self.lm.model.decode_step_paged(self._embed_ids(self.cur.clamp_min(0)), self.cache, active, active_host=flags)
                self.cur = ops.sample_rows_each(ops.linear(h, self.w_lm), self._u[self._t - self._u_t0], self.temperature, self.top_k, self.top_p)
            self._t += 1
            self.stats["steps"] += 1
            self.stats["row_steps_active"] += sum(flags)
            self.stats["row_steps_total"] += self.rows
        read = (self.cur if first is None else torch.stack([self.cur, first])).tolist()      # the step's one host read
        toks, firsts = (read, None) if first is None else read
        done = []
        for row, run in enumerate(self.running):
            if run is None:
                continue
            new = ([firsts[row]] if row in fresh else []) + ([toks[row]] if flags[row] else [])
            for t in new:
                if t < 0:                                                          # a sampled row that could not be drawn from: the request ends here
                    self.errors[run.ticket] = (f"ContinuousBatcher.step: the logits of request {run.ticket} at step {len(run.tokens)} contain a NaN "
                                               "or +inf, or no finite entry: no token can be drawn")
                else:
                    run.tokens.append(int(t))
                if t < 0 or len(run.tokens) == run.max_new or (self.eos_ids is not None and int(t) in self.eos_ids):
                    self._released.update(p for p in self.cache.pages_of(row) if self.cache.page_refs[p] == 1)      # those that go back to the pool
                    self.cache.release(row)
                    self.running[row] = None
                    if run.sampled:
                        self.temperature[row] = 0.0                                # an idle row is a greedy row
                    done.append((run.ticket, torch.tensor(run.tokens, dtype=torch.int64, device=self.device)))
                    break
        return done

    def run(self, requests) -> List[torch.Tensor]:
        """Submit every (prompt, max_new_tokens) pair - or (remainder, max_new_tokens, prefix handle or None[, sampler or None]) tuple -, step until
        the queue and the rows are empty; the token tensors in submit order.  RuntimeError, after everything has drained, if a sampled request of
        this call could not be drawn from: it names the tickets, `errors` holds each message, and the other requests' tokens were computed."""
        tickets = [self.submit(r[0], r[1], prefix=r[2] if len(r) > 2 else None, sampler=r[3] if len(r) > 3 else None) for r in requests]
        out = {}
        while self.queue or any(r is not None for r in self.running):
            out.update(self.step())
        failed = [t for t in tickets if t in self.errors]
        if failed:
            raise RuntimeError(f"ContinuousBatcher.run: the requests with tickets {failed} could not be drawn from and ended early (every other "
                               f"request drained): {self.errors[failed[0]]}")
        return [out[t] for t in tickets]
