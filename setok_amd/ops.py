"""Torch-tensor front end of the C ABI: pointer extraction, shape/dtype checks, output allocation.

PyTorch is plumbing here (device memory + streams); every operator below is one call into
libsetok_hip.so on torch's current HIP stream."""
from __future__ import annotations

import os

import math
from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import ACT_GELU_ERF, ACT_NONE, ACT_QUICK_GELU, ACT_SILU, BF16, F16, F32  # noqa: F401

Tensor = torch.Tensor


def _code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16                               # (a marked int: _lib.call sends the call to libsetok_hip_f16.so)
    raise TypeError(f"setok_amd supports float32, bfloat16 and float16, got {dt}")


LOW = (torch.bfloat16, torch.float16)            # the 16-bit element types: MFMA throughput mode, fp32 accumulation


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """The HIP stream torch is currently recording on, as an integer handle.  (`torch.cuda.current_stream()` builds a Python Stream object
    per call — 8 us, 1.5 ms of host time per encode at ~200 launches; the raw getter is 0.3 us.)"""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]) -> Optional[int]:
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-contiguous tensor required"
    return t.data_ptr()


def _f32(t: Optional[Tensor]) -> Optional[Tensor]:
    if t is not None:
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous()
    return t


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def k_align(dt: torch.dtype) -> int:
    return 64 if dt in LOW else 16


# ---- optional launch profiler (bench.py): HIP events recorded INSIDE the library around every GEMM / clustering call ---------------------
_ACT_NAMES = ("plain", "quick_gelu", "gelu_erf")


def _profiled_libs():
    """(half, lib) of the library builds this process has loaded: the profiler's state is per library."""
    _lib.load()
    return sorted(_lib._libs.items())


def profile_start() -> None:
    for half, _ in _profiled_libs():
        _lib.call("setok_profile_start", half=half)


def profile_pause(pause: bool = True) -> None:
    """Between profile_start() and profile_stop(): stop (True) / resume (False) attaching events to launches; what was recorded stays."""
    for half, _ in _profiled_libs():
        _lib.call("setok_profile_pause", 1 if pause else 0, half=half)


def profile_stop():
    """Synchronise and return [{kernel, flops, ms, bytes}] for every launch the library recorded since profile_start()."""
    import numpy as np
    cap = 1 << 16
    out = []
    for half, lib in _profiled_libs():
        kind, cls = np.empty(cap, np.int32), np.empty(cap, np.int32)
        work, nbytes, ms = np.empty(cap, np.float64), np.empty(cap, np.float64), np.empty(cap, np.float32)
        n = lib.setok_profile_stop(kind.ctypes.data, cls.ctypes.data, work.ctypes.data, nbytes.ctypes.data, ms.ctypes.data, cap)
        if n < 0:
            raise _lib.SetokHipError("setok_profile_stop failed")
        low = "gemm_f16:" if half else "gemm_bf16:"
        for i in range(n):
            if kind[i] == 2:
                name, w = "cluster_dpc_knn", float(nbytes[i])            # the clustering record's headline quantity is algorithmic BYTES
            else:
                c = int(cls[i])
                name = (low if kind[i] == 0 else "gemm_f32:") + _ACT_NAMES[c & 3] + ("+residual" if c & 4 else "") + ("+layernorm" if c & 8 else "")
                w = float(work[i])
            out.append(dict(kernel=name, flops=w, ms=float(ms[i]), bytes=float(nbytes[i])))
    return out


def linear(a: Tensor, w: Tensor, bias: Optional[Tensor] = None, residual: Optional[Tensor] = None,
           act: int = ACT_NONE, out: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """out = act(a @ w.T + bias) + residual;  a: (M, K), w: (N, K), bias fp32 (N,)."""
    M, K = a.shape
    N, K2 = w.shape
    assert K == K2 and a.dtype == w.dtype
    od = out_dtype or a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=od, device=a.device)
    assert out.shape == (M, N) and out.dtype == od
    if residual is not None:
        assert residual.shape == (M, N) and residual.dtype == od
    if not (a.is_contiguous() and out.is_contiguous() and (residual is None or residual.is_contiguous())):
        return _linear_windows(a, w, bias, residual, act, out)
    _lib.call("setok_linear", _stream(), _code(a.dtype), _code(od), _p(a), K, _p(w), _p(_f32(bias)), _p(residual),
              _p(out), N, M, N, K, act, 1, 0, 0, 0)
    return out


def _linear_windows(a: Tensor, w: Tensor, bias, residual, act: int, out: Tensor) -> Tensor:
    """`linear` on column windows of wider buffers: `a` and `out` with dense rows and their buffers' row strides (a stride changes addresses
    only); a residual shares out's stride, as setok_linear reads it (the LoRA update of a window of the fused q|k|v output, in place)."""
    M, K = a.shape
    N = w.shape[0]
    ldc = _rows_ld(out)
    assert w.is_contiguous() and (residual is None or M <= 1 or _rows_ld(residual) == ldc), "residual shares out's row stride"
    _lib.call("setok_linear", _stream(), _code(a.dtype), _code(out.dtype), a.data_ptr(), _rows_ld(a), _p(w), _p(_f32(bias)),
              None if residual is None else residual.data_ptr(), out.data_ptr(), ldc, M, N, K, act, 1, 0, 0, 0)
    return out


# ---- the skinny GEMM of a LoRA adapter (csrc/gemm_skinny.hip) -------------------------------------------------------------------------------
SKINNY_MAX_N = 256                                # SETOK_SKINNY_MAX_N of include/setok_hip.h


def linear_skinny_workspace(M: int, N: int, K: int, half: bool = False) -> int:
    """Floats of workspace `setok_linear_skinny` needs for an (M, K) x (N, K) problem: ceil(K / SETOK_SKINNY_KSLICE) * M * N."""
    return int(_lib.load(half).setok_linear_skinny_workspace(M, N, K))


def skinny_kslice(half: bool = False) -> int:
    """SETOK_SKINNY_KSLICE of the loaded library, read off its workspace rule: the largest K that is still one slice."""
    K = 64
    while linear_skinny_workspace(1, 16, K + 64, half) == 16:
        K += 64
    return K


def linear_skinny(a: Tensor, w: Tensor, alpha: float = 1.0, out: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None,
                  ws: Optional[Tensor] = None) -> Tensor:
    """out = alpha * a @ w.T for a narrow output: a (M, K), w (N, K) with N <= SKINNY_MAX_N, N % 16 == 0; out in a.dtype or fp32.  Split-K by a
    rule in K alone with a fixed-order sum (include/setok_hip.h: setok_linear_skinny): a row's bits do not depend on M or the strides.  a, w and
    out may be column windows of wider buffers.  `ws`: fp32 scratch of at least linear_skinny_workspace(M, N, K) floats (default: the
    stream-ordered scratch `linear_tn` uses)."""
    M, K = a.shape
    N, K2 = w.shape
    assert K == K2 and a.dtype == w.dtype
    od = out_dtype or a.dtype
    if out is None:
        out = torch.empty((M, N), dtype=od, device=a.device)
    assert out.shape == (M, N) and out.dtype == od
    if M == 0:                                        # nothing to compute (an empty tensor has no address to pass)
        return out
    need = linear_skinny_workspace(M, N, K, a.dtype == torch.float16)
    if ws is None:
        ws = _ws(a.device, need)
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.is_cuda
    _lib.call("setok_linear_skinny", _stream(), _code(a.dtype), _code(od), a.data_ptr(), _rows_ld(a), w.data_ptr(), _rows_ld(w), out.data_ptr(),
              _rows_ld(out), M, N, K, float(alpha), ws.data_ptr(), ws.numel())
    return out


def layernorm(x: Tensor, gamma: Tensor, beta: Tensor, eps: float = 1e-5, out: Optional[Tensor] = None) -> Tensor:
    rows, Cc = x.shape
    if out is None:
        out = torch.empty_like(x)
    _lib.call("setok_layernorm", _stream(), _code(x.dtype), _p(x), _p(_f32(gamma)), _p(_f32(beta)), _p(out), rows, Cc, eps)
    return out


# ---- LayerNorm folded into the consuming Linear (bf16 throughput mode; include/setok_hip.h explains the algebra) -------------------------
def row_stats(x: Tensor, eps: float = 1e-5, out: Optional[Tensor] = None) -> Tensor:
    """(rows, 8) fp32 words per row: [0:2] the compact MFMA fragment of (-mean, 1 / rstd) (bf16 pairs), [4] rstd = 1 / sqrt(var + eps), [5] mean — the
    statistics setok_layernorm computes, without writing a normalised copy."""
    rows, Cc = x.shape
    if out is None:
        out = torch.empty((rows, 8), dtype=torch.float32, device=x.device)
    assert out.shape == (rows, 8) and out.dtype == torch.float32
    _lib.call("setok_row_stats", _stream(), _code(x.dtype), _p(x), _p(out), rows, Cc, eps)
    return out


def ln_fold(w: Tensor, gamma: Tensor, beta: Tensor, bias: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Once per weight load: (W' = bf16(gamma * W), c = W' 1, b' = b + W beta, the (N, 4)-word MFMA fragments of (c, b')) for linear_ln."""
    assert w.dtype in LOW and w.dim() == 2
    N, K = w.shape
    wg = torch.empty_like(w)
    cs = torch.empty((N,), dtype=torch.float32, device=w.device)
    bf = torch.empty((N,), dtype=torch.float32, device=w.device)
    fr = torch.empty((N, 4), dtype=torch.float32, device=w.device)
    _lib.call("setok_ln_fold", _stream(), _p(w.contiguous()), _p(_f32(gamma)), _p(_f32(beta)), _p(_f32(bias)), _p(wg), _p(cs), _p(bf), _p(fr), N, K,
              half=w.dtype == torch.float16)
    return wg, cs, bf, fr


def linear_ln(a: Tensor, folded: Tuple[Tensor, Tensor, Tensor, Tensor], stats: Tensor, act: int = ACT_NONE, out: Optional[Tensor] = None) -> Tensor:
    """out = act(LayerNorm(a) @ W.T + b) from the raw rows `a`, their statistics and the folded weights of ln_fold."""
    wg, _, _, fr = folded
    M, K = a.shape
    N = wg.shape[0]
    assert a.dtype in LOW and wg.dtype == a.dtype and wg.shape[1] == K and stats.shape == (M, 8)
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    _lib.call("setok_linear_ln", _stream(), _p(a), K, _p(wg), _p(fr), _p(stats), _p(out), N, M, N, K, act, half=a.dtype == torch.float16)
    return out


def attention(qkv: Tensor, H: int, Dh: int, scale: float, seg_len: int, seg_offsets: Optional[Tensor] = None,
              n_segs: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """Block-diagonal attention.  Uniform segments of `seg_len` rows, or ragged ones given by the int32
    device tensor `seg_offsets` (n_segs + 1 entries; `seg_len` is then an upper bound on the length)."""
    rows = qkv.shape[0]
    assert qkv.shape[1] == 3 * H * Dh
    if out is None:
        out = torch.empty((rows, H * Dh), dtype=qkv.dtype, device=qkv.device)
    if seg_offsets is not None:
        assert seg_offsets.dtype == torch.int32 and seg_offsets.numel() >= n_segs + 1
    _lib.call("setok_attention", _stream(), _code(qkv.dtype), _p(qkv), _p(seg_offsets), n_segs, seg_len, _p(out),
              rows, H, Dh, scale)
    return out


def cross_attention(q: Tensor, k: Tensor, v: Tensor, H: int, Dh: int, scale: float, q_len: int, kv_offsets: Optional[Tensor],
                    n_segs: int, max_kv: int, out: Optional[Tensor] = None) -> Tensor:
    """Cross-attention of `n_segs` groups of `q_len` query rows to ragged key / value segments (`kv_offsets`: int32
    device tensor of n_segs + 1 row offsets into k / v; None = uniform segments of `max_kv` rows).  q, k, v are 2-D row views
    (column windows of wider buffers are fine: only the row stride is passed down)."""
    assert q.dim() == 2 and k.dim() == 2 and v.dim() == 2 and q.shape[1] == H * Dh and k.shape[1] == H * Dh and v.shape[1] == H * Dh
    assert q.stride(1) == 1 and k.stride(1) == 1 and v.stride(1) == 1 and k.stride(0) == v.stride(0) and k.dtype == q.dtype == v.dtype
    assert q.shape[0] == n_segs * q_len
    if out is None:
        out = torch.empty((q.shape[0], H * Dh), dtype=q.dtype, device=q.device)
    if kv_offsets is not None:
        assert kv_offsets.dtype == torch.int32 and kv_offsets.numel() >= n_segs + 1
    assert q.is_cuda and k.is_cuda and v.is_cuda
    _lib.call("setok_cross_attention", _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0), _p(kv_offsets), n_segs,
              q_len, max_kv, _p(out), out.stride(0), H, Dh, scale)
    return out


def patchify(images: Tensor, p: int, kpad: int) -> Tensor:
    B, Cin, H, W = images.shape
    assert Cin == 3
    out = torch.empty((B * (H // p) * (W // p), kpad), dtype=images.dtype, device=images.device)
    _lib.call("setok_patchify", _stream(), _code(images.dtype), _p(images), _p(out), B, H, W, p, kpad)
    return out


def vit_assemble(patch_embed: Tensor, cls: Tensor, pos: Tensor, B: int, N: int) -> Tensor:
    Cc = patch_embed.shape[1]
    out = torch.empty((B * (N + 1), Cc), dtype=patch_embed.dtype, device=patch_embed.device)
    _lib.call("setok_vit_assemble", _stream(), _code(patch_embed.dtype), _p(patch_embed), _p(cls), _p(pos), _p(out), B, N, Cc)
    return out


def select_add_pos(hidden: Tensor, pos2d: Tensor, B: int, N: int, skip: int) -> Tensor:
    Cc = hidden.shape[-1]
    assert hidden.numel() == B * (N + skip) * Cc and pos2d.shape == (N, Cc) and pos2d.dtype == hidden.dtype
    out = torch.empty((B * N, Cc), dtype=hidden.dtype, device=hidden.device)
    _lib.call("setok_select_add_pos", _stream(), _code(hidden.dtype), _p(hidden), _p(pos2d), _p(out), B, N, Cc, skip)
    return out


def cluster_dpc_knn(x: Tensor, B: int, N: int, k: int, threshold: float, min_cluster_num: int,
                    noise: Optional[Tensor] = None, token_mask: Optional[Tensor] = None
                    ) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """x: (B*N, C).  Returns (idx_cluster int64 (B,N), score fp32 (B,N), index_down int64 (B,N) [-1 padded],
    counts int32 (B,)).  No host synchronisation."""
    Cc = x.shape[-1]
    assert x.numel() == B * N * Cc
    dev = x.device
    idx = torch.empty((B, N), dtype=torch.int64, device=dev)
    score = torch.empty((B, N), dtype=torch.float32, device=dev)
    index_down = torch.empty((B, N), dtype=torch.int64, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    nd, nv = _lib.C.c_int64(0), _lib.C.c_int64(0)
    _lib.call("setok_cluster_workspace", _code(x.dtype), B, N, Cc, _lib.C.byref(nd), _lib.C.byref(nv))
    dist_ws = torch.empty((nd.value,), dtype=torch.float32, device=dev) if nd.value else None       # 0: the fused single-launch form
    vec_ws = torch.empty((nv.value,), dtype=torch.float32, device=dev) if nv.value else None
    if noise is not None:
        noise = noise.to(device=dev, dtype=torch.float32).contiguous()
        assert noise.numel() == B * N
    if token_mask is not None:
        token_mask = token_mask.to(device=dev, dtype=torch.float32).contiguous()
        assert token_mask.numel() == B * N
    _lib.call("setok_cluster_dpc_knn", _stream(), _code(x.dtype), _p(x), B, N, Cc, int(k), float(threshold),
              int(min_cluster_num), _p(noise), _p(token_mask), _p(idx), _p(score), _p(index_down), _p(counts),
              _p(dist_ws), _p(vec_ws))
    return idx, score, index_down, counts


def cluster_sort(idx_cluster: Tensor, counts: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    B, N = idx_cluster.shape
    dev = idx_cluster.device
    perm = torch.empty((B * N,), dtype=torch.int32, device=dev)
    seg_offsets = torch.empty((B * N + 1,), dtype=torch.int32, device=dev)
    img_offsets = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    _lib.call("setok_cluster_sort", _stream(), _p(idx_cluster), _p(counts), B, N, _p(perm), _p(seg_offsets), _p(img_offsets))
    return perm, seg_offsets, img_offsets


def gather_rows(x: Tensor, perm: Tensor) -> Tensor:
    rows, Cc = perm.numel(), x.shape[-1]
    out = torch.empty((rows, Cc), dtype=x.dtype, device=x.device)
    _lib.call("setok_gather_rows", _stream(), _code(x.dtype), _p(x), _p(perm), _p(out), rows, Cc)
    return out


def segment_mean(h: Tensor, seg_offsets: Tensor, n_segs_dev: Tensor, n_segs: int, out: Optional[Tensor] = None) -> Tensor:
    """n_segs_dev: 1-element int32 device tensor (e.g. img_offsets[B:]); n_segs: rows to allocate/launch.  Rows of `out` at or beyond
    n_segs_dev are not written."""
    Cc = h.shape[-1]
    if out is None:
        out = torch.empty((n_segs, Cc), dtype=h.dtype, device=h.device)
    assert out.shape == (n_segs, Cc) and out.dtype == h.dtype
    _lib.call("setok_segment_mean", _stream(), _code(h.dtype), _p(h), _p(seg_offsets), _p(n_segs_dev), n_segs, _p(out), Cc)
    return out


def activation(x: Tensor, act: int, out: Optional[Tensor] = None) -> Tensor:
    if out is None:
        out = torch.empty_like(x)
    _lib.call("setok_activation", _stream(), _code(x.dtype), _p(x), _p(out), x.numel(), act)
    return out


def activation_dropout(x: Tensor, act: int, p: float, seed: int, offset: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """dropout(activation(x)) in one pass (bit-identical to the two calls)."""
    if out is None:
        out = torch.empty_like(x)
    _lib.call("setok_activation_dropout", _stream(), _code(x.dtype), _p(x), _p(out), x.numel(), act, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
              int(offset) & 0xFFFFFFFFFFFFFFFF)
    return out


def dropout(x: Tensor, p: float, seed: int, offset: int = 0, residual: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """out = residual + x * mask / (1 - p), mask_i a pure function of (seed, offset + i) (include/setok_hip.h: setok_dropout).  Applying the same
    call (no residual) to an incoming gradient is the backward pass."""
    if out is None:
        out = torch.empty_like(x)
    assert x.is_contiguous() and out.is_contiguous() and out.shape == x.shape and (residual is None or (residual.shape == x.shape and residual.is_contiguous()))
    _lib.call("setok_dropout", _stream(), _code(x.dtype), _p(x), _p(residual), _p(out), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
              int(offset) & 0xFFFFFFFFFFFFFFFF)
    return out


# ---- prepare_inputs_labels_for_multimodal (setokim_arch.py:213-355) --------------------------------------------------------
def splice_lengths(input_ids: Tensor, attention_mask: Optional[Tensor], img_offsets: Tensor, n_images: int, image_token_index: int,
                   max_length: int, vocab: int = 0) -> Tuple[Tensor, Tensor, Tensor]:
    """Returns (seq_len int32 (B,), img_start int32 (B,), status int32 (4,)) on the device; no host synchronisation."""
    B, T = input_ids.shape
    dev = input_ids.device
    assert input_ids.dtype == torch.int64 and img_offsets.dtype == torch.int32 and img_offsets.numel() >= n_images + 1
    if attention_mask is not None:
        assert attention_mask.dtype == torch.uint8 and attention_mask.shape == (B, T)
    seq_len = torch.empty((B,), dtype=torch.int32, device=dev)
    img_start = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((4,), dtype=torch.int32, device=dev)
    ws = torch.empty((3 * B,), dtype=torch.int32, device=dev)
    _lib.call("setok_splice_lengths", _stream(), _p(input_ids), _p(attention_mask), B, T, image_token_index, int(vocab), _p(img_offsets), n_images,
              int(max_length), _p(seq_len), _p(img_start), _p(status), _p(ws))
    return seq_len, img_start, status


def splice_plan(input_ids: Tensor, attention_mask: Optional[Tensor], labels: Optional[Tensor], img_offsets: Tensor, seq_len: Tensor,
                img_start: Tensor, max_len: int, left_pad: bool, image_token_index: int, ignore_index: int, target_token_index: int,
                want_mask: bool, want_pos: bool):
    B, T = input_ids.shape
    dev = input_ids.device
    src = torch.empty((B, max_len), dtype=torch.int32, device=dev)
    new_labels = torch.empty((B, max_len), dtype=torch.int64, device=dev) if labels is not None else None
    new_mask = torch.empty((B, max_len), dtype=torch.uint8, device=dev) if want_mask else None
    new_pos = torch.empty((B, max_len), dtype=torch.int64, device=dev) if want_pos else None
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.shape == (B, T)
    _lib.call("setok_splice_plan", _stream(), _p(input_ids), _p(attention_mask), _p(labels), B, T, image_token_index, ignore_index,
              target_token_index, _p(img_offsets), _p(seq_len), _p(img_start), max_len, 1 if left_pad else 0, _p(src), _p(new_labels),
              _p(new_mask), _p(new_pos))
    return src, new_labels, new_mask, new_pos


def splice_rows(src: Tensor, embed_table: Tensor, image_tokens: Optional[Tensor], status: Optional[Tensor] = None) -> Tensor:
    """status: optional int32[2] device tensor — [0] = 1 / [1] = first row whose src neither table can serve (such rows are zero-filled)."""
    B, max_len = src.shape
    V, D = embed_table.shape
    out = torch.empty((B, max_len, D), dtype=embed_table.dtype, device=embed_table.device)
    n_img_rows = 0
    if image_tokens is not None:
        assert image_tokens.dtype == embed_table.dtype and image_tokens.shape[-1] == D
        n_img_rows = image_tokens.shape[0]
    if status is not None:
        assert status.dtype == torch.int32 and status.numel() >= 2
    _lib.call("setok_splice_rows", _stream(), _code(embed_table.dtype), _p(src), _p(embed_table), V, _p(image_tokens), n_img_rows, _p(out),
              B * max_len, D, _p(status))
    return out


def splice_rows_bwd(src: Tensor, d_out: Tensor, n_image_rows: int, want_embed: int = 0) -> Tuple[Optional[Tensor], Optional[Tensor]]:
    """(d image_tokens (n_image_rows, D) in d_out's dtype, d embed_table (want_embed, D) fp32 or None)."""
    rows, D = src.numel(), d_out.shape[-1]
    d_out = d_out.reshape(rows, D)
    assert d_out.is_contiguous()
    dfe = torch.empty((n_image_rows, D), dtype=d_out.dtype, device=d_out.device) if n_image_rows > 0 else None
    dem = torch.zeros((want_embed, D), dtype=torch.float32, device=d_out.device) if want_embed > 0 else None
    _lib.call("setok_splice_rows_bwd", _stream(), _code(d_out.dtype), _p(src), _p(d_out), rows, D, _p(dfe), n_image_rows, _p(dem), want_embed)
    return dfe, dem


# ---- pixel head of the reconstruction decoder (include/setok_hip.h: the output the reference never defines) ---------------------------------
def unpatchify(patches: Tensor, B: int, gh: int, gw: int, p: int) -> Tensor:
    """patches (B*gh*gw, >= 3 p^2) -> image (B, 3, gh*p, gw*p); only the first 3 p^2 columns are read (a padded GEMM output is fine)."""
    assert patches.dim() == 2 and patches.shape[0] == B * gh * gw and patches.shape[1] >= 3 * p * p and patches.stride(1) == 1
    img = torch.empty((B, 3, gh * p, gw * p), dtype=patches.dtype, device=patches.device)
    assert patches.is_cuda
    _lib.call("setok_unpatchify", _stream(), _code(patches.dtype), patches.data_ptr(), patches.stride(0), _p(img), B, gh, gw, p)
    return img


def pixel_loss(pred: Tensor, target: Tensor, kind: str = "mse") -> Tensor:
    """0-d fp32 tensor: mean squared ("mse") or mean absolute ("l1") difference over all elements."""
    assert pred.shape == target.shape and pred.dtype == target.dtype and kind in ("mse", "l1")
    out = torch.empty((1,), dtype=torch.float32, device=pred.device)
    _lib.call("setok_pixel_loss", _stream(), _code(pred.dtype), _p(pred.contiguous()), _p(target.contiguous()), pred.numel(), 0 if kind == "mse" else 1,
              _p(_ws(pred.device, 1024)), _p(out))
    return out[0]


# ---- backward pass of the trainable head (csrc/backward.hip) ----------------------------------------------------------------
def transpose(x: Tensor, pad_to: int = 1, splits: int = 1, with_colsum: bool = False, colsum_out: Optional[Tensor] = None):
    """(rows, cols) -> (cols, P) with P = rows zero-padded to a multiple of pad_to: the A / W operand of a dW = dY^T X GEMM.
    splits > 1: P is padded to splits * chunk (chunk a multiple of pad_to) and the result is (splits, cols, chunk) — the split-K layout.
    with_colsum: also returns the fp32 column sums of x (the bias gradient when x is dY), computed inside the same pass."""
    rows, cols = x.shape
    assert x.is_contiguous()
    if splits <= 1:
        ldo, chunk = round_up(max(rows, 1), pad_to), 0
        out = torch.empty((cols, ldo), dtype=x.dtype, device=x.device)
    else:
        chunk = round_up((max(rows, 1) + splits - 1) // splits, pad_to)
        ldo = splits * chunk
        out = torch.empty((splits, cols, chunk), dtype=x.dtype, device=x.device)
    part = torch.empty(((ldo + 63) // 64, cols), dtype=torch.float32, device=x.device) if with_colsum else None
    _lib.call("setok_transpose", _stream(), _code(x.dtype), _p(x), cols, rows, cols, _p(out), ldo, chunk, _p(part))
    if not with_colsum:
        return out
    return out, colsum(part, out=colsum_out)


def linear_tn(aT: Tensor, bT: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """dW = sum_s aT[s] @ bT[s]^T in fp32 for split-K operands aT (S, N, chunk), bT (S, K, chunk) from `transpose(..., splits=S)`
    (or 2-D (N, P), (K, P) for S = 1): one batched GEMM for the partial products, then a fixed-order sum over the splits."""
    if aT.dim() == 2:
        return linear(aT, bT, out=out, out_dtype=torch.float32)
    S, N, chunk = aT.shape
    S2, K, chunk2 = bT.shape
    assert S == S2 and chunk == chunk2 and aT.dtype == bT.dtype
    part = torch.empty((S, N, K), dtype=torch.float32, device=aT.device)
    _lib.call("setok_linear", _stream(), _code(aT.dtype), F32, _p(aT), chunk, _p(bT), None, None, _p(part), K, N, K, chunk, ACT_NONE, S,
              N * chunk, K * chunk, N * K)
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=aT.device)
    assert out.shape == (N, K) and out.dtype == torch.float32 and out.is_contiguous()
    ws = _ws(aT.device, N * K)
    _lib.call("setok_colsum", _stream(), F32, _p(part), S, N * K, _p(out), 0, _p(ws), 1)
    return out


_WS: dict = {}


def _ws(device, n: int) -> Tensor:
    """fp32 scratch reused across calls on the same stream (kernels of one stream run in order)."""
    key = str(device)
    if key not in _WS or _WS[key].numel() < n:
        _WS[key] = torch.empty((max(n, 1 << 20),), dtype=torch.float32, device=device)
    return _WS[key]


def colsum(x: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    rows, cols = x.shape
    if out is None:
        out = torch.empty((cols,), dtype=torch.float32, device=x.device)
        assert not accumulate
    ws_rows = 128
    ws = _ws(x.device, ws_rows * cols)
    _lib.call("setok_colsum", _stream(), _code(x.dtype), _p(x), rows, cols, _p(out), 1 if accumulate else 0, _p(ws), ws_rows)
    return out


def layernorm_bwd(x: Tensor, dy: Tensor, gamma: Tensor, eps: float, dgamma: Tensor, dbeta: Tensor, accumulate: bool,
                  need_dx: bool = True, res: Optional[Tensor] = None) -> Optional[Tensor]:
    rows, Cc = x.shape
    assert dy.shape == x.shape and dgamma.dtype == torch.float32 and dbeta.dtype == torch.float32
    dx = torch.empty_like(x) if need_dx else None
    ws_rows = 2048
    ws = _ws(x.device, ws_rows * Cc)
    _lib.call("setok_layernorm_bwd", _stream(), _code(x.dtype), _p(x), _p(dy), _p(_f32(gamma)), eps, rows, Cc, _p(dx), _p(res),
              _p(dgamma), _p(dbeta), 1 if accumulate else 0, _p(ws), ws_rows)
    return dx


def gelu_bwd(pre: Tensor, dy: Tensor) -> Tensor:
    dx = torch.empty_like(pre)
    _lib.call("setok_gelu_bwd", _stream(), _code(pre.dtype), _p(pre), _p(dy), _p(dx), pre.numel())
    return dx


def gelu_bwd_dropout(pre: Tensor, dy: Tensor, p: float, seed: int, offset: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """gelu'(pre) * dropout(dy) in one pass (bit-identical to dropout(dy) then gelu_bwd); `out` may be `dy`."""
    dx = torch.empty_like(pre) if out is None else out
    _lib.call("setok_gelu_bwd_dropout", _stream(), _code(pre.dtype), _p(pre), _p(dy), _p(dx), pre.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
              int(offset) & 0xFFFFFFFFFFFFFFFF)
    return dx


def attention_bwd(qkv: Tensor, out: Tensor, dout: Tensor, H: int, Dh: int, scale: float, seg_len: int,
                  seg_offsets: Optional[Tensor] = None, n_segs: int = 0) -> Tensor:
    rows = qkv.shape[0]
    dqkv = torch.empty_like(qkv)
    ws = _ws(qkv.device, 2 * rows * H)
    _lib.call("setok_attention_bwd", _stream(), _code(qkv.dtype), _p(qkv), _p(seg_offsets), n_segs, seg_len, _p(out), _p(dout), _p(dqkv),
              rows, H, Dh, scale, _p(ws))
    return dqkv


def mha_bwd(q: Tensor, k: Tensor, v: Tensor, out: Tensor, dout: Tensor, H: int, Dh: int, scale: float, q_len: int,
            kv_offsets: Optional[Tensor], n_segs: int, max_kv: int, dq: Optional[Tensor] = None, dk: Optional[Tensor] = None,
            dv: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Backward of cross_attention (self-attention: kv_offsets None, max_kv = q_len, q / k / v the column windows of one qkv buffer).
    All operands are 2-D row views with unit column stride; dq, dk, dv may be given as views (the windows of one dqkv buffer, or the
    [dk | dv] halves of one buffer), else fresh (rows, H*Dh) tensors are returned.  k / v and dk / dv share their row strides."""
    C = H * Dh
    for t in (q, k, v, out, dout):
        assert t.dim() == 2 and t.shape[1] == C and t.stride(1) == 1 and t.is_cuda and t.dtype == q.dtype
    assert k.stride(0) == v.stride(0) and q.shape[0] == n_segs * q_len and out.shape[0] == dout.shape[0] == q.shape[0] and k.shape[0] == v.shape[0]
    if kv_offsets is not None:
        assert kv_offsets.dtype == torch.int32 and kv_offsets.numel() >= n_segs + 1
        if n_segs:                                                # every key row must get its dk / dv (one host read of the longest segment)
            longest = int((kv_offsets[1:n_segs + 1] - kv_offsets[:n_segs]).max())
            assert longest <= max_kv, f"a key / value segment has {longest} rows, more than max_kv = {max_kv}"
    else:
        assert k.shape[0] == n_segs * max_kv
    if dq is None:
        dq = torch.empty((q.shape[0], C), dtype=q.dtype, device=q.device)
    if dk is None or dv is None:
        dkv = torch.empty((k.shape[0], 2 * C), dtype=q.dtype, device=q.device)
        dk, dv = dkv[:, :C], dkv[:, C:]
    for t, like in ((dq, q), (dk, k), (dv, v)):
        assert t.shape == like.shape and t.stride(1) == 1 and t.dtype == q.dtype
    assert dk.stride(0) == dv.stride(0)
    ws = _ws(q.device, 2 * q.shape[0] * H)
    _lib.call("setok_mha_bwd", _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), k.data_ptr(), v.data_ptr(), k.stride(0), _p(kv_offsets), n_segs,
              q_len, max_kv, out.data_ptr(), out.stride(0), dout.data_ptr(), dout.stride(0), dq.data_ptr(), dq.stride(0), dk.data_ptr(), dv.data_ptr(),
              dk.stride(0), H, Dh, scale, _p(ws))
    return dq, dk, dv


def pixel_loss_bwd(pred: Tensor, gold: Optional[Tensor], kind: str, upstream: Tensor, n_pad: int, gh: int, gw: int, p: int) -> Tensor:
    """d loss / d patch rows (B*gh*gw, n_pad) for loss = pixel_loss(unpatchify(patches), gold, kind), times the 0-d fp32 device tensor
    `upstream`; pad columns are zero.  kind "unpatchify": the backward of unpatchify alone (`pred` is d loss / d image, `gold` unused)."""
    code = {"mse": 0, "l1": 1, "unpatchify": 2}[kind]
    B = pred.shape[0]
    assert pred.dim() == 4 and tuple(pred.shape[1:]) == (3, gh * p, gw * p) and pred.is_contiguous()
    if code != 2:
        assert gold is not None and gold.shape == pred.shape and gold.dtype == pred.dtype and gold.is_contiguous()
    up = upstream.detach().reshape(1).to(device=pred.device, dtype=torch.float32).contiguous()
    out = torch.empty((B * gh * gw, n_pad), dtype=pred.dtype, device=pred.device)
    _lib.call("setok_pixel_loss_bwd", _stream(), _code(pred.dtype), _p(pred), _p(gold) if code != 2 else None, code, _p(up), _p(out), n_pad,
              B, gh, gw, p)
    return out


def segment_mean_bwd(dseg: Tensor, seg_offsets: Tensor, n_segs_dev: Tensor, n_segs: int, rows: int) -> Tensor:
    Cc = dseg.shape[-1]
    out = torch.empty((rows, Cc), dtype=dseg.dtype, device=dseg.device)
    _lib.call("setok_segment_mean_bwd", _stream(), _code(dseg.dtype), _p(dseg), _p(seg_offsets), _p(n_segs_dev), n_segs, _p(out), Cc)
    return out


def adamw(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, param_lp: Optional[Tensor], lr: float, beta1: float,
          beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0) -> None:
    assert param.dtype == grad.dtype == exp_avg.dtype == exp_avg_sq.dtype == torch.float32
    n = param.numel()
    assert grad.numel() == n and (param_lp is None or param_lp.numel() == n)
    lp = _code(param_lp.dtype) if param_lp is not None else 0
    _lib.call("setok_adamw", _stream(), lp, _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), _p(param_lp), n, lr, beta1, beta2, eps,
              weight_decay, step, grad_scale)


# ---- LLM prefill (csrc/llama.hip) ------------------------------------------------------------------------------------------------
def rmsnorm(x: Tensor, weight: Tensor, eps: float, out: Optional[Tensor] = None) -> Tensor:
    rows, Cc = x.shape
    if out is None:
        out = torch.empty_like(x)
    w = weight if weight.dtype == torch.float32 else weight.float()       # a bf16 weight is exact in fp32; the kernel re-rounds it to the activation dtype
    _lib.call("setok_rmsnorm", _stream(), _code(x.dtype), _p(x), _p(w.contiguous()), _p(out), rows, Cc, eps)
    return out


def rope_(qkv: Tensor, position_ids: Tensor, H: int, Dh: int, theta: float, Hkv: Optional[int] = None) -> Tensor:
    """In place on the q and k parts of qkv (rows, (H + 2*Hkv)*Dh) laid out [q | k | v]; Hkv (grouped-query attention) defaults to H."""
    rows = qkv.shape[0]
    Hkv = H if Hkv is None else Hkv
    assert qkv.shape[1] == (H + 2 * Hkv) * Dh and position_ids.dtype == torch.int64 and position_ids.numel() == rows
    _lib.call("setok_rope_gqa", _stream(), _code(qkv.dtype), _p(qkv), _p(position_ids.contiguous()), rows, H, Hkv, Dh, theta)
    return qkv


def swiglu(gate_up: Tensor) -> Tensor:
    rows, F2 = gate_up.shape
    out = torch.empty((rows, F2 // 2), dtype=gate_up.dtype, device=gate_up.device)
    _lib.call("setok_swiglu", _stream(), _code(gate_up.dtype), _p(gate_up), _p(out), rows, F2 // 2)
    return out


def swiglu_pairs(gate_up_pairs: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """act_fn(gate) * up on INTERLEAVED (gate_j, up_j) columns — the output of `linear` with pair-interleaved weight rows (interleave_gate_up)."""
    rows, F2 = gate_up_pairs.shape
    if out is None:
        out = torch.empty((rows, F2 // 2), dtype=gate_up_pairs.dtype, device=gate_up_pairs.device)
    _lib.call("setok_swiglu_pairs", _stream(), _code(gate_up_pairs.dtype), _p(gate_up_pairs), _p(out), rows, F2 // 2)
    return out


def interleave_gate_up(gate_w: Tensor, up_w: Tensor) -> Tensor:
    """(F, K), (F, K) -> (2 F, K) with row 2 j = gate_w[j], row 2 j + 1 = up_w[j]: the weight layout of linear_swiglu."""
    assert gate_w.shape == up_w.shape
    return torch.stack([gate_w, up_w], dim=1).reshape(2 * gate_w.shape[0], gate_w.shape[1]).contiguous()


def linear_swiglu(a: Tensor, w_pairs: Tensor) -> Tensor:
    """act_fn(a @ Wg.T) * (a @ Wu.T) for pair-interleaved weights (interleave_gate_up): LlamaMLP's gate|up Linear + SwiGLU.  In the 16-bit modes the whole 256-row
    tiles go through ONE launch (SwiGLU in the GEMM's epilogue: the (M, 2 F) intermediate is never written); the rows behind them — and everything when the
    problem is too small for the persistent kernel, or in fp32 — through `linear` + `swiglu_pairs`.  The two forms give the same bits (the epilogue keeps torch's
    rounding points), so a row's result does not depend on which of them it took."""
    M, K = a.shape
    F2 = w_pairs.shape[0]
    out = torch.empty((M, F2 // 2), dtype=a.dtype, device=a.device)
    main = 0
    if os.environ.get("SETOK_SWIGLU_FUSED", "1") != "0" and a.dtype in LOW and F2 % 256 == 0 and K % 64 == 0 and K >= 128 and (M // 256) * (F2 // 256) >= 90:
        main = M // 256 * 256
        _lib.call("setok_linear_swiglu", _stream(), _code(a.dtype), _p(a), K, _p(w_pairs), _p(out), F2 // 2, main, F2 // 2, K)
    if main < M:
        swiglu_pairs(linear(a[main:], w_pairs), out=out[main:])
    return out


def lm_loss(logits: Tensor, labels: Tensor, attention_mask: Optional[Tensor], ignore_index: int = -100) -> Tensor:
    """The shifted, padding-masked cross entropy of setokim_llama.py:145-160.  logits (B, T, V) fp32 / bf16 (read as fp32), labels (B, T)
    int64, attention_mask (B, T) or None.  Returns a 2-element fp32 tensor: [mean loss, number of positions that counted]."""
    B, T, V = logits.shape
    lg = logits.reshape(B * T, V)
    assert lg.stride(1) == 1
    lab = labels.to(device=logits.device, dtype=torch.int64).reshape(B * T).contiguous()
    am = None if attention_mask is None else (attention_mask.to(logits.device) != 0).to(torch.uint8).reshape(B * T).contiguous()
    ws = torch.empty(2 * B * T, dtype=torch.float32, device=logits.device)
    out = torch.empty(2, dtype=torch.float32, device=logits.device)
    _lib.call("setok_lm_loss", _stream(), _code(logits.dtype), lg.data_ptr(), lg.stride(0), _p(lab), _p(am), B, T, V, ignore_index, _p(ws), _p(out))
    return out


def attention_causal(qkv: Tensor, key_mask: Optional[Tensor], B: int, T: int, H: int, Dh: int, scale: float, Hkv: Optional[int] = None) -> Tensor:
    """Causal, key-padding-masked attention over B sequences of T rows [q: H heads | k: Hkv | v: Hkv]; Hkv < H: grouped-query attention."""
    Hkv = H if Hkv is None else Hkv
    assert qkv.shape == (B * T, (H + 2 * Hkv) * Dh) and H % Hkv == 0
    if key_mask is not None:
        assert key_mask.dtype == torch.uint8 and key_mask.numel() == B * T
    out = torch.empty((B * T, H * Dh), dtype=qkv.dtype, device=qkv.device)
    _lib.call("setok_attention_causal_gqa", _stream(), _code(qkv.dtype), _p(qkv), _p(key_mask), _p(out), B, T, H, Hkv, Dh, scale)
    return out


# ---- backward through the frozen LLM (csrc/llama_bwd.hip, csrc/attn_causal_bwd.hip): the dX chain only ----------------------------------------
def lm_loss_bwd(logits: Tensor, labels: Tensor, attention_mask: Optional[Tensor], loss_out: Tensor, upstream: Optional[Tensor] = None,
                ignore_index: int = -100, out: Optional[Tensor] = None) -> Tensor:
    """d loss / d logits for `loss_out = lm_loss(logits, labels, attention_mask)` (its 2-element result: the count is read on the device), times
    the 0-d / 1-element fp32 device tensor `upstream` (None = 1).  Rows the forward did not count are exact zeros.  `out`: (B, T, V) in the
    dtype of logits with unit column stride (a view with its own row stride is fine)."""
    B, T, V = logits.shape
    lg = logits.reshape(B * T, V)
    assert lg.stride(1) == 1 and lg.is_cuda and loss_out.dtype == torch.float32 and loss_out.numel() >= 2
    if out is None:
        out = torch.empty((B, T, V), dtype=logits.dtype, device=logits.device)
    do = out.reshape(B * T, V)
    assert do.dtype == logits.dtype and do.stride(1) == 1 and do.data_ptr() == out.data_ptr()
    lab = labels.to(device=logits.device, dtype=torch.int64).reshape(B * T).contiguous()
    am = None if attention_mask is None else (attention_mask.to(logits.device) != 0).to(torch.uint8).reshape(B * T).contiguous()
    up = None if upstream is None else upstream.detach().reshape(1).to(device=logits.device, dtype=torch.float32).contiguous()
    _lib.call("setok_lm_loss_bwd", _stream(), _code(logits.dtype), lg.data_ptr(), lg.stride(0), _p(lab), _p(am), B, T, V, ignore_index,
              _p(loss_out.contiguous()), _p(up), do.data_ptr(), do.stride(0))
    return out


def rmsnorm_bwd(x: Tensor, weight: Tensor, dy: Tensor, eps: float, dres: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """dx of rmsnorm(x, weight, eps) for the upstream dy, plus `dres` (the residual branch's gradient) in the same pass.  `out` may be dy or dres."""
    rows, Cc = x.shape
    assert dy.shape == x.shape and dy.dtype == x.dtype and (dres is None or (dres.shape == x.shape and dres.dtype == x.dtype))
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype
    w = weight if weight.dtype == torch.float32 else weight.float()
    _lib.call("setok_rmsnorm_bwd", _stream(), _code(x.dtype), _p(x), _p(w.contiguous()), _p(dy), _p(dres), _p(out), rows, Cc, eps)
    return out


def rope_bwd_(dqkv: Tensor, position_ids: Tensor, H: int, Dh: int, theta: float, Hkv: Optional[int] = None) -> Tensor:
    """The transpose of rope_, in place on the dq and dk parts of dqkv (rows, (H + 2*Hkv)*Dh); dv untouched."""
    rows = dqkv.shape[0]
    Hkv = H if Hkv is None else Hkv
    assert dqkv.shape[1] == (H + 2 * Hkv) * Dh and position_ids.dtype == torch.int64 and position_ids.numel() == rows
    _lib.call("setok_rope_bwd_gqa", _stream(), _code(dqkv.dtype), _p(dqkv), _p(position_ids.contiguous()), rows, H, Hkv, Dh, theta)
    return dqkv


def swiglu_pairs_bwd(gate_up_pairs: Tensor, dout: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """d (gate_j, up_j) pairs (rows, 2 F) from the pre-activation pairs and d loss / d swiglu_pairs(...) (rows, F).  `out` may be gate_up_pairs."""
    rows, F2 = gate_up_pairs.shape
    assert dout.shape == (rows, F2 // 2) and dout.dtype == gate_up_pairs.dtype
    if out is None:
        out = torch.empty_like(gate_up_pairs)
    assert out.shape == gate_up_pairs.shape and out.dtype == gate_up_pairs.dtype
    _lib.call("setok_swiglu_pairs_bwd", _stream(), _code(gate_up_pairs.dtype), _p(gate_up_pairs), _p(dout), _p(out), rows, F2 // 2)
    return out


def attention_causal_bwd(qkv: Tensor, key_mask: Optional[Tensor], out: Tensor, dout: Tensor, B: int, T: int, H: int, Dh: int, scale: float,
                         Hkv: Optional[int] = None) -> Tensor:
    """Backward of attention_causal: dqkv in the layout of qkv ([dq: H heads | dk: Hkv | dv: Hkv]) from the forward's (post-rotary) input, its output
    and d loss / d out."""
    Hkv = H if Hkv is None else Hkv
    assert qkv.shape == (B * T, (H + 2 * Hkv) * Dh) and H % Hkv == 0
    assert out.shape == (B * T, H * Dh) and dout.shape == out.shape and out.dtype == qkv.dtype and dout.dtype == qkv.dtype
    if key_mask is not None:
        assert key_mask.dtype == torch.uint8 and key_mask.numel() == B * T
    dqkv = torch.empty_like(qkv)
    ws = _ws(qkv.device, 2 * B * T * H)
    _lib.call("setok_attention_causal_bwd_gqa", _stream(), _code(qkv.dtype), _p(qkv), _p(key_mask), _p(out), _p(dout), _p(dqkv), B, T, H, Hkv, Dh, scale,
              _p(ws))
    return dqkv


# ---- KV-cached decoding (csrc/attn_decode.hip) ------------------------------------------------------------------------------------------------
DECODE_CHUNK = 128                                # SETOK_DECODE_CHUNK of include/setok_hip.h


def kv_append(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, T: int, H: int, pos0: int) -> None:
    """The post-rotary k / v columns of qkv (B*T rows [q: H | k: Hkv | v: Hkv]) -> slots [pos0, pos0 + T) of the (B, Hkv, cap, Dh) caches."""
    B, Hkv, cap, Dh = k_cache.shape
    assert v_cache.shape == k_cache.shape and k_cache.dtype == v_cache.dtype == qkv.dtype
    assert qkv.shape == (B * T, (H + 2 * Hkv) * Dh)
    _lib.call("setok_kv_append", _stream(), _code(qkv.dtype), _p(qkv), _p(k_cache), _p(v_cache), B, T, H, Hkv, Dh, cap, pos0)


def attention_decode_workspace(B: int, H: int, Dh: int, length: int, chunk: int = DECODE_CHUNK) -> int:
    """Floats of workspace setok_attention_decode_gqa needs for `length` candidate slots (chunk=DECODE_CHUNK_FP8KV: the fp8-cache call)."""
    return B * H * ((length + chunk - 1) // chunk) * (Dh + 2)


def attention_decode(q: Tensor, k_cache: Tensor, v_cache: Tensor, key_mask: Tensor, H: int, length: int, scale: float,
                     ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """One query row per (sequence, query head) against slots [0, length) of the caches (B, Hkv, cap, Dh); q: (B, >= H*Dh) rows, row stride
    q.stride(0) (the step's fused qkv buffer is read in place); key_mask (B, cap) uint8.  Returns (B, H*Dh)."""
    B, Hkv, cap, Dh = k_cache.shape
    assert v_cache.shape == k_cache.shape and k_cache.dtype == v_cache.dtype == q.dtype
    return _attention_decode("setok_attention_decode_gqa", q, (_p(k_cache), _p(v_cache)), key_mask, B, H, Hkv, Dh, cap, length, scale, DECODE_CHUNK, ws, out)


def _attention_decode(symbol: str, q: Tensor, cache_ptrs: tuple, key_mask: Tensor, B: int, H: int, Hkv: int, Dh: int, cap: int, length: int,
                      scale: float, chunk: int, ws: Optional[Tensor], out: Optional[Tensor]) -> Tensor:
    """What the decode attention over either cache format does once the cache's own operands are checked: `cache_ptrs` are the cache's
    pointers in the order of `symbol`'s signature, `chunk` the format's slots per partial."""
    assert q.shape[0] == B and q.shape[1] >= H * Dh and q.stride(1) == 1 and q.is_cuda
    assert key_mask.dtype == torch.uint8 and key_mask.shape == (B, cap)
    need = attention_decode_workspace(B, H, Dh, length, chunk)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need
    if out is None:
        out = torch.empty((B, H * Dh), dtype=q.dtype, device=q.device)
    assert out.shape == (B, H * Dh) and out.dtype == q.dtype
    _lib.call(symbol, _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), *cache_ptrs, _p(key_mask), _p(out), B, H, Hkv, Dh, cap, length, scale,
              _p(ws), ws.numel())
    return out


DECODE_CHUNK_FP8KV = 256                          # SETOK_DECODE_CHUNK_FP8KV of include/setok_hip.h


def _fp8kv_shapes(k_q: Tensor, k_e: Tensor, v_q: Tensor, v_e: Tensor) -> Tuple[int, int, int, int]:
    B, Hkv, cap, Dh = k_q.shape
    assert v_q.shape == k_q.shape and k_q.dtype == v_q.dtype == torch.uint8 and k_q.is_contiguous() and v_q.is_contiguous()
    assert k_e.shape == v_e.shape == (B, Hkv, cap) and k_e.dtype == v_e.dtype == torch.int8 and k_e.is_contiguous() and v_e.is_contiguous()
    return B, Hkv, cap, Dh


def kv_append_fp8(qkv: Tensor, k_q: Tensor, k_e: Tensor, v_q: Tensor, v_e: Tensor, T: int, H: int, pos0: int) -> None:
    """kv_append into an fp8 cache: the post-rotary k / v rows of qkv are quantised (e4m3fn codes + one power-of-two exponent per row, the
    rule of quantize_fp8_rows) into slots [pos0, pos0 + T) of k_q / v_q (B, Hkv, cap, Dh) uint8 and k_e / v_e (B, Hkv, cap) int8."""
    B, Hkv, cap, Dh = _fp8kv_shapes(k_q, k_e, v_q, v_e)
    assert qkv.shape == (B * T, (H + 2 * Hkv) * Dh) and qkv.is_contiguous()
    _lib.call("setok_kv_append_fp8", _stream(), _code(qkv.dtype), _p(qkv), _p(k_q), _p(k_e), _p(v_q), _p(v_e), B, T, H, Hkv, Dh, cap, pos0)


def attention_decode_fp8kv(q: Tensor, k_q: Tensor, k_e: Tensor, v_q: Tensor, v_e: Tensor, key_mask: Tensor, H: int, length: int, scale: float,
                           ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """attention_decode over an fp8 cache (the keys / values are value(code) * 2^exponent, exactly); q and the result in q.dtype."""
    B, Hkv, cap, Dh = _fp8kv_shapes(k_q, k_e, v_q, v_e)
    return _attention_decode("setok_attention_decode_gqa_fp8kv", q, (_p(k_q), _p(k_e), _p(v_q), _p(v_e)), key_mask, B, H, Hkv, Dh, cap, length, scale,
                             DECODE_CHUNK_FP8KV, ws, out)


# ---- the paged KV cache (csrc/attn_paged.hip) ----------------------------------------------------------------------------------------------------
KV_PAGE = 128                                     # SETOK_KV_PAGE of include/setok_hip.h (== DECODE_CHUNK: a chunk's workgroup reads one page)


def _paged_shapes(k_pool: Tensor, v_pool: Tensor, block_table: Tensor, per_seq: Tensor) -> Tuple[int, int, int, int, int]:
    num_pages, Hkv, page, Dh = k_pool.shape
    assert page == KV_PAGE and v_pool.shape == k_pool.shape and k_pool.dtype == v_pool.dtype
    B, max_pages = block_table.shape
    assert block_table.dtype == torch.int32 and per_seq.dtype == torch.int32 and per_seq.shape == (B,)
    return num_pages, Hkv, Dh, B, max_pages


def kv_append_paged(qkv: Tensor, k_pool: Tensor, v_pool: Tensor, block_table: Tensor, slot0: Tensor, T: int, H: int) -> None:
    """The post-rotary k / v columns of rows b*T + t of qkv ([q: H | k: Hkv | v: Hkv]) -> slot slot0[b] + t of sequence b: page
    block_table[b][slot // KV_PAGE] of the (num_pages, Hkv, KV_PAGE, Dh) pools, row slot % KV_PAGE.  block_table (B, max_pages) and slot0 (B,)
    are int32 on the device; a sequence with slot0[b] < 0 is skipped, a table entry outside [0, num_pages) is no page (nothing is written)."""
    num_pages, Hkv, Dh, B, max_pages = _paged_shapes(k_pool, v_pool, block_table, slot0)
    assert qkv.dtype == k_pool.dtype and qkv.shape == (B * T, (H + 2 * Hkv) * Dh)
    _lib.call("setok_kv_append_paged", _stream(), _code(qkv.dtype), _p(qkv), _p(k_pool), _p(v_pool), _p(block_table), max_pages, num_pages, _p(slot0),
              B, T, H, Hkv, Dh)


def attention_decode_paged_workspace(B: int, H: int, Dh: int, max_len: int) -> int:
    """Floats of workspace setok_attention_decode_gqa_paged needs for lengths up to `max_len`."""
    return B * H * ((max_len + KV_PAGE - 1) // KV_PAGE) * (Dh + 2)


def attention_decode_paged(q: Tensor, k_pool: Tensor, v_pool: Tensor, block_table: Tensor, lens: Tensor, H: int, max_len: int, scale: float,
                           ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """One query row per (sequence, query head) against slots [0, lens[b]) of sequence b, found through row b of block_table in the pools; q: (B, >=
    H*Dh) rows of stride q.stride(0); lens (B,) int32 on the device, `max_len` the host's upper bound on it.  Returns (B, H*Dh); a sequence's bits
    are attention_decode's at B = 1 on its gathered slots."""
    num_pages, Hkv, Dh, B, max_pages = _paged_shapes(k_pool, v_pool, block_table, lens)
    assert q.dtype == k_pool.dtype and q.shape[0] == B and q.shape[1] >= H * Dh and q.stride(1) == 1 and q.is_cuda
    need = attention_decode_paged_workspace(B, H, Dh, max_len)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need
    if out is None:
        out = torch.empty((B, H * Dh), dtype=q.dtype, device=q.device)
    assert out.shape == (B, H * Dh) and out.dtype == q.dtype
    _lib.call("setok_attention_decode_gqa_paged", _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), _p(k_pool), _p(v_pool), _p(block_table),
              max_pages, num_pages, _p(lens), _p(out), B, H, Hkv, Dh, max_len, scale, _p(ws), ws.numel())
    return out


# ---- extending a cache by Tn tokens (csrc/attn_extend.hip) ---------------------------------------------------------------------------------------
EXTEND_CHUNK = 256                                # SETOK_EXTEND_CHUNK of include/setok_hip.h


def attention_extend_workspace(B: int, Tn: int, H: int, Dh: int, len0: int, Hkv: Optional[int] = None, dtype: torch.dtype = torch.float32) -> int:
    """Floats of workspace setok_attention_extend_gqa needs for Tn new rows per sequence behind len0 cached slots, as the library states it
    (setok_attention_extend_workspace: the rule lives there).  Without Hkv and dtype: B * Tn * H * ceil((len0 + Tn) / EXTEND_CHUNK) * (Dh + 2),
    which suffices for every call; with them, what the kernel that call runs needs (the MFMA kernel with many rows leaves fewer partials)."""
    code = _code(dtype)
    return int(_lib.load(_lib.is_half(code)).setok_attention_extend_workspace(code, B, Tn, H, H if Hkv is None else Hkv, Dh, len0))


def attention_extend(q: Tensor, k_cache: Tensor, v_cache: Tensor, key_mask: Tensor, H: int, Tn: int, len0: int, scale: float,
                     ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """Tn query rows per (sequence, query head) against the caches (B, Hkv, cap, Dh), which already hold the new rows' keys / values in slots
    [len0, len0 + Tn): query i of sequence b counts slot j iff j <= len0 + i and key_mask[b, j] != 0.  q: (B * Tn, >= H*Dh) rows, row stride
    q.stride(0) (the step's fused qkv buffer is read in place); key_mask (B, cap) uint8.  Returns (B * Tn, H*Dh)."""
    B, Hkv, cap, Dh = k_cache.shape
    assert v_cache.shape == k_cache.shape and k_cache.dtype == v_cache.dtype == q.dtype
    assert Tn >= 1 and len0 >= 0 and len0 + Tn <= cap, f"attention_extend: slots [{len0}, {len0} + {Tn}) exceed the cache (cap = {cap})"
    assert q.shape[0] == B * Tn and q.shape[1] >= H * Dh and q.stride(1) == 1 and q.is_cuda
    assert key_mask.dtype == torch.uint8 and key_mask.shape == (B, cap)
    need = attention_extend_workspace(B, Tn, H, Dh, len0, Hkv, q.dtype)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need
    if out is None:
        out = torch.empty((B * Tn, H * Dh), dtype=q.dtype, device=q.device)
    assert out.shape == (B * Tn, H * Dh) and out.dtype == q.dtype
    _lib.call("setok_attention_extend_gqa", _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), _p(k_cache), _p(v_cache), _p(key_mask), _p(out),
              B, Tn, H, Hkv, Dh, cap, len0, scale, _p(ws), ws.numel())
    return out


# ---- extending sequences of the paged cache (csrc/attn_extend_paged.hip) ------------------------------------------------------------------------
def attention_extend_paged_workspace(B: int, Tn: int, H: int, Dh: int, max_len0: int, Hkv: Optional[int] = None,
                                     dtype: torch.dtype = torch.float32) -> int:
    """Floats of workspace setok_attention_extend_gqa_paged needs for Tn new rows per sequence behind at most max_len0 filled slots, as the library
    states it (setok_attention_extend_paged_workspace: attention_extend_workspace's rule at len0 = max_len0)."""
    code = _code(dtype)
    return int(_lib.load(_lib.is_half(code)).setok_attention_extend_paged_workspace(code, B, Tn, H, H if Hkv is None else Hkv, Dh, max_len0))


def attention_extend_paged(q: Tensor, k_pool: Tensor, v_pool: Tensor, block_table: Tensor, len0: Tensor, H: int, Tn: int, max_len0: int, scale: float,
                           ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """Tn query rows per (sequence, query head) against the sequence's slots in the pools, which already hold the new rows' keys / values in slots
    [len0[b], len0[b] + Tn) (kv_append_paged with slot0 = len0): query i of sequence b counts slot j iff j <= len0[b] + i and
    block_table[b][j // KV_PAGE] is a page.  q: (B * Tn, >= H*Dh) rows of stride q.stride(0); len0 (B,) int32 on the device, < 0 for an idle
    sequence (zeros), `max_len0` the host's upper bound on it.  Returns (B * Tn, H*Dh); a sequence's bits are attention_extend's at B = 1 on its
    gathered slots."""
    num_pages, Hkv, Dh, B, max_pages = _paged_shapes(k_pool, v_pool, block_table, len0)
    assert Tn >= 1 and 0 <= max_len0 and max_len0 + Tn <= max_pages * KV_PAGE, \
        f"attention_extend_paged: slots [{max_len0}, {max_len0} + {Tn}) lie beyond the table ({max_pages} pages)"
    assert q.dtype == k_pool.dtype and q.shape[0] == B * Tn and q.shape[1] >= H * Dh and q.stride(1) == 1 and q.is_cuda
    need = attention_extend_paged_workspace(B, Tn, H, Dh, max_len0, Hkv, q.dtype)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need
    if out is None:
        out = torch.empty((B * Tn, H * Dh), dtype=q.dtype, device=q.device)
    assert out.shape == (B * Tn, H * Dh) and out.dtype == q.dtype
    _lib.call("setok_attention_extend_gqa_paged", _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), _p(k_pool), _p(v_pool), _p(block_table),
              max_pages, num_pages, _p(len0), _p(out), B, Tn, H, Hkv, Dh, max_len0, scale, _p(ws), ws.numel())
    return out


# ---- the MXFP4 KV cache (csrc/attn_decode.hip, csrc/attn_extend.hip; include/setok_hip.h, "MXFP4 KV cache") --------------------------------------
DECODE_CHUNK_MXFP4KV = 256                        # SETOK_DECODE_CHUNK_MXFP4KV of include/setok_hip.h


def _mxfp4kv_shapes(k_q: Tensor, k_s: Tensor, v_q: Tensor, v_s: Tensor) -> Tuple[int, int, int, int]:
    B, Hkv, cap, half = k_q.shape
    Dh = 2 * half
    if Dh % MXFP4_BLOCK != 0:
        raise ValueError(f"the MXFP4 KV cache needs a head dim that is a multiple of {MXFP4_BLOCK}, the MX block; the nibble rows hold {Dh} elements")
    assert v_q.shape == k_q.shape and k_q.dtype == v_q.dtype == torch.uint8 and k_q.is_contiguous() and v_q.is_contiguous()
    assert k_s.shape == v_s.shape == (B, Hkv, cap, Dh // MXFP4_BLOCK) and k_s.dtype == v_s.dtype == torch.uint8
    assert k_s.is_contiguous() and v_s.is_contiguous()
    return B, Hkv, cap, Dh


def kv_append_mxfp4(qkv: Tensor, k_q: Tensor, k_s: Tensor, v_q: Tensor, v_s: Tensor, T: int, H: int, pos0: int) -> None:
    """kv_append into an MXFP4 cache: the post-rotary k / v rows of qkv are quantised (e2m1 nibbles + one e8m0 scale byte per 32 elements, the
    rule of quantize_mxfp4_rows) into slots [pos0, pos0 + T) of k_q / v_q (B, Hkv, cap, Dh/2) uint8 and k_s / v_s (B, Hkv, cap, Dh/32) uint8."""
    B, Hkv, cap, Dh = _mxfp4kv_shapes(k_q, k_s, v_q, v_s)
    assert qkv.shape == (B * T, (H + 2 * Hkv) * Dh) and qkv.is_contiguous()
    _lib.call("setok_kv_append_mxfp4", _stream(), _code(qkv.dtype), _p(qkv), _p(k_q), _p(k_s), _p(v_q), _p(v_s), B, T, H, Hkv, Dh, cap, pos0)


def attention_decode_mxfp4kv(q: Tensor, k_q: Tensor, k_s: Tensor, v_q: Tensor, v_s: Tensor, key_mask: Tensor, H: int, length: int, scale: float,
                             ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """attention_decode over an MXFP4 cache (the keys / values are value(nibble) * 2^(scale byte - 127), exactly); q and the result in q.dtype."""
    B, Hkv, cap, Dh = _mxfp4kv_shapes(k_q, k_s, v_q, v_s)
    return _attention_decode("setok_attention_decode_gqa_mxfp4kv", q, (_p(k_q), _p(k_s), _p(v_q), _p(v_s)), key_mask, B, H, Hkv, Dh, cap, length, scale,
                             DECODE_CHUNK_MXFP4KV, ws, out)


def attention_extend_mxfp4kv_workspace(B: int, Tn: int, H: int, Dh: int, len0: int) -> int:
    """Floats of workspace setok_attention_extend_gqa_mxfp4kv needs: B * Tn * H * ceil((len0 + Tn) / EXTEND_CHUNK) * (Dh + 2), whatever the
    element type and head dim (one partial per chunk; the MFMA path, 16 bits at head dim 128, leaves a partial per span as attention_extend
    does and uses a prefix of it: the rule does not follow it)."""
    return B * Tn * H * ((len0 + Tn + EXTEND_CHUNK - 1) // EXTEND_CHUNK) * (Dh + 2)


def attention_extend_mxfp4kv(q: Tensor, k_q: Tensor, k_s: Tensor, v_q: Tensor, v_s: Tensor, key_mask: Tensor, H: int, Tn: int, len0: int,
                             scale: float, ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """attention_extend over an MXFP4 cache, which already holds the new rows' quantised keys / values in slots [len0, len0 + Tn), with
    attention_extend's dispatch.  bf16 / fp16 at head dim 128: the native MFMA kernel on tiles converted from nibbles — the result's bits are
    attention_extend's over caches holding K', V' = value(nibble) * 2^(scale byte - 127), which must be representable in q.dtype (every row
    kv_append_mxfp4 writes is).  fp32 and the other head dims: one wave per (query row, query head, chunk), no MFMA."""
    B, Hkv, cap, Dh = _mxfp4kv_shapes(k_q, k_s, v_q, v_s)
    assert Tn >= 1 and len0 >= 0 and len0 + Tn <= cap, f"attention_extend_mxfp4kv: slots [{len0}, {len0} + {Tn}) exceed the cache (cap = {cap})"
    assert q.shape[0] == B * Tn and q.shape[1] >= H * Dh and q.stride(1) == 1 and q.is_cuda
    assert key_mask.dtype == torch.uint8 and key_mask.shape == (B, cap)
    need = attention_extend_mxfp4kv_workspace(B, Tn, H, Dh, len0)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need
    if out is None:
        out = torch.empty((B * Tn, H * Dh), dtype=q.dtype, device=q.device)
    assert out.shape == (B * Tn, H * Dh) and out.dtype == q.dtype
    _lib.call("setok_attention_extend_gqa_mxfp4kv", _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), _p(k_q), _p(k_s), _p(v_q), _p(v_s),
              _p(key_mask), _p(out), B, Tn, H, Hkv, Dh, cap, len0, scale, _p(ws), ws.numel())
    return out


# ---- MXFP4 pools of the paged cache (csrc/attn_paged.hip, csrc/attn_extend_paged.hip; include/setok_hip.h, "Paged MXFP4 KV cache") ---------------
PAGED_MXFP4_HEAD_DIMS = (32, 64, 128)             # the head dims with a lane layout over nibble rows: what the paged append and decode entries take


def _paged_mxfp4_shapes(k_q: Tensor, k_s: Tensor, v_q: Tensor, v_s: Tensor, block_table: Tensor, per_seq: Tensor) -> Tuple[int, int, int, int, int]:
    num_pages, Hkv, page, Dh = _mxfp4kv_shapes(k_q, k_s, v_q, v_s)         # the dense cache's rules with a page where a sequence was
    assert page == KV_PAGE
    B, max_pages = block_table.shape
    assert block_table.dtype == torch.int32 and per_seq.dtype == torch.int32 and per_seq.shape == (B,)
    return num_pages, Hkv, Dh, B, max_pages


def kv_append_paged_mxfp4(qkv: Tensor, k_q: Tensor, k_s: Tensor, v_q: Tensor, v_s: Tensor, block_table: Tensor, slot0: Tensor, T: int, H: int) -> None:
    """kv_append_paged into MXFP4 pools: rows b*T + t of qkv are quantised by kv_append_mxfp4's rule into slot slot0[b] + t of sequence b - page
    block_table[b][slot // KV_PAGE], row slot % KV_PAGE of k_q / v_q (num_pages, Hkv, KV_PAGE, Dh/2) and k_s / v_s (num_pages, Hkv, KV_PAGE, Dh/32),
    all uint8.  A sequence with slot0[b] < 0 is skipped; a table entry outside [0, num_pages) is no page (nothing is written)."""
    num_pages, Hkv, Dh, B, max_pages = _paged_mxfp4_shapes(k_q, k_s, v_q, v_s, block_table, slot0)
    assert qkv.shape == (B * T, (H + 2 * Hkv) * Dh) and qkv.is_contiguous()
    _lib.call("setok_kv_append_paged_mxfp4", _stream(), _code(qkv.dtype), _p(qkv), _p(k_q), _p(k_s), _p(v_q), _p(v_s), _p(block_table), max_pages,
              num_pages, _p(slot0), B, T, H, Hkv, Dh)


def attention_decode_paged_mxfp4kv_workspace(B: int, H: int, Dh: int, max_len: int) -> int:
    """Floats of workspace setok_attention_decode_gqa_paged_mxfp4kv needs for lengths up to `max_len`: a partial per DECODE_CHUNK_MXFP4KV slots."""
    return B * H * ((max_len + DECODE_CHUNK_MXFP4KV - 1) // DECODE_CHUNK_MXFP4KV) * (Dh + 2)


def attention_decode_paged_mxfp4kv(q: Tensor, k_q: Tensor, k_s: Tensor, v_q: Tensor, v_s: Tensor, block_table: Tensor, lens: Tensor, H: int,
                                   max_len: int, scale: float, ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """attention_decode_paged over MXFP4 pools; q and the result in q.dtype.  A sequence's bits are attention_decode_mxfp4kv's at B = 1 on its
    gathered slots."""
    num_pages, Hkv, Dh, B, max_pages = _paged_mxfp4_shapes(k_q, k_s, v_q, v_s, block_table, lens)
    assert q.shape[0] == B and q.shape[1] >= H * Dh and q.stride(1) == 1 and q.is_cuda
    need = attention_decode_paged_mxfp4kv_workspace(B, H, Dh, max_len)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need
    if out is None:
        out = torch.empty((B, H * Dh), dtype=q.dtype, device=q.device)
    assert out.shape == (B, H * Dh) and out.dtype == q.dtype
    _lib.call("setok_attention_decode_gqa_paged_mxfp4kv", _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), _p(k_q), _p(k_s), _p(v_q), _p(v_s),
              _p(block_table), max_pages, num_pages, _p(lens), _p(out), B, H, Hkv, Dh, max_len, scale, _p(ws), ws.numel())
    return out


def attention_extend_paged_mxfp4kv_workspace(B: int, Tn: int, H: int, Dh: int, max_len0: int) -> int:
    """Floats of workspace setok_attention_extend_gqa_paged_mxfp4kv needs: attention_extend_mxfp4kv_workspace's rule at len0 = max_len0 (on the
    MFMA path an upper bound of which a prefix is used, as there)."""
    return attention_extend_mxfp4kv_workspace(B, Tn, H, Dh, max_len0)


def attention_extend_paged_mxfp4kv(q: Tensor, k_q: Tensor, k_s: Tensor, v_q: Tensor, v_s: Tensor, block_table: Tensor, len0: Tensor, H: int, Tn: int,
                                   max_len0: int, scale: float, ws: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """attention_extend_paged over MXFP4 pools, which already hold the new rows' quantised keys / values in slots [len0[b], len0[b] + Tn)
    (kv_append_paged_mxfp4 with slot0 = len0), for every head dim that is a multiple of 32.  bf16 / fp16 at head dim 128: attention_extend_paged's
    MFMA kernel on tiles converted from nibbles — the result's bits are attention_extend_paged's over pools holding K', V' (representable in
    q.dtype: every row kv_append_paged_mxfp4 writes is); everything else the wave-per-chunk kernel.  Either way a sequence's bits are
    attention_extend_mxfp4kv's at B = 1 on its gathered slots."""
    num_pages, Hkv, Dh, B, max_pages = _paged_mxfp4_shapes(k_q, k_s, v_q, v_s, block_table, len0)
    assert Tn >= 1 and 0 <= max_len0 and max_len0 + Tn <= max_pages * KV_PAGE, \
        f"attention_extend_paged_mxfp4kv: slots [{max_len0}, {max_len0} + {Tn}) lie beyond the table ({max_pages} pages)"
    assert q.shape[0] == B * Tn and q.shape[1] >= H * Dh and q.stride(1) == 1 and q.is_cuda
    need = attention_extend_paged_mxfp4kv_workspace(B, Tn, H, Dh, max_len0)
    if ws is None:
        ws = torch.empty(max(need, 1), dtype=torch.float32, device=q.device)
    assert ws.dtype == torch.float32 and ws.numel() >= need
    if out is None:
        out = torch.empty((B * Tn, H * Dh), dtype=q.dtype, device=q.device)
    assert out.shape == (B * Tn, H * Dh) and out.dtype == q.dtype
    _lib.call("setok_attention_extend_gqa_paged_mxfp4kv", _stream(), _code(q.dtype), q.data_ptr(), q.stride(0), _p(k_q), _p(k_s), _p(v_q), _p(v_s),
              _p(block_table), max_pages, num_pages, _p(len0), _p(out), B, Tn, H, Hkv, Dh, max_len0, scale, _p(ws), ws.numel())
    return out


def argmax_rows(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """int64 (rows,): the lowest index of each row's maximum; x (rows, V) with any row stride."""
    rows, V = x.shape
    assert x.stride(1) == 1 and x.is_cuda
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=x.device)
    assert out.dtype == torch.int64 and out.numel() == rows
    _lib.call("setok_argmax_rows", _stream(), _code(x.dtype), x.data_ptr(), x.stride(0), rows, V, _p(out))
    return out


def sample_rows(logits: Tensor, u: Tensor, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, out: Optional[Tensor] = None,
                probs: Optional[Tensor] = None) -> Tensor:
    """int64 (rows,): the token each row of `logits` (rows, V; any row stride) draws with its uniform u[r] (fp32, (rows,)) after temperature, top-k
    and top-p in HF's order (include/setok_hip.h, "Sampling"); -1 for a row with a NaN, +inf or no finite entry.  `probs` (rows, V) fp32, if
    given, receives the distribution drawn from."""
    rows, V = logits.shape
    assert logits.stride(1) == 1 and logits.is_cuda
    assert u.dtype == torch.float32 and u.numel() == rows
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=logits.device)
    assert out.dtype == torch.int64 and out.numel() == rows
    ldp = 0
    if probs is not None:
        assert probs.dtype == torch.float32 and probs.shape == (rows, V) and probs.stride(1) == 1 and probs.is_cuda
        ldp = probs.stride(0) if rows > 1 else max(probs.stride(0), V)
    _lib.call("setok_sample_rows", _stream(), _code(logits.dtype), logits.data_ptr(), logits.stride(0) if rows > 1 else max(logits.stride(0), V), rows, V,
              _p(u), float(temperature), int(top_k), float(top_p), _p(out), None if probs is None else probs.data_ptr(), ldp)
    return out


def sample_rows_each(logits: Tensor, u: Tensor, temperature: Tensor, top_k: Tensor, top_p: Tensor, out: Optional[Tensor] = None,
                     probs: Optional[Tensor] = None) -> Tensor:
    """`sample_rows` with the three parameters per row, still one launch: `temperature` and `top_p` fp32 (rows,), `top_k` int32 (rows,), on the
    logits' device.  Row r is drawn under its own three values, bit for bit as `sample_rows` would draw it; temperature[r] == 0 makes it a greedy
    row - `argmax_rows`' token, one-hot `probs`, u[r] ignored -; any other value outside `sample_rows`' domain gives -1 and zero `probs` for that
    row alone (include/setok_hip.h, "Sampling")."""
    rows, V = logits.shape
    assert logits.stride(1) == 1 and logits.is_cuda
    assert u.dtype == torch.float32 and u.numel() == rows
    for name, t, dt in (("temperature", temperature, torch.float32), ("top_k", top_k, torch.int32), ("top_p", top_p, torch.float32)):
        assert isinstance(t, Tensor) and t.dtype == dt and t.shape == (rows,) and t.is_contiguous() and t.device == logits.device, \
            f"sample_rows_each: {name} must be a contiguous {dt} ({rows},) tensor on {logits.device}"
    assert u.device == logits.device and (rows <= 1 or u.dim() == 0 or u.is_contiguous())
    if out is None:
        out = torch.empty(rows, dtype=torch.int64, device=logits.device)
    assert out.dtype == torch.int64 and out.numel() == rows
    ldp = 0
    if probs is not None:
        assert probs.dtype == torch.float32 and probs.shape == (rows, V) and probs.stride(1) == 1 and probs.is_cuda
        ldp = probs.stride(0) if rows > 1 else max(probs.stride(0), V)
    _lib.call("setok_sample_rows_each", _stream(), _code(logits.dtype), logits.data_ptr(), logits.stride(0) if rows > 1 else max(logits.stride(0), V),
              rows, V, _p(u), _p(temperature), _p(top_k), _p(top_p), _p(out), None if probs is None else probs.data_ptr(), ldp)
    return out


# ---- speculative decoding (csrc/speculate.hip) ---------------------------------------------------------------------------------------------------
SPEC_MAX_K = 63                                   # drafted tokens per round: K + 1 <= 64 rows per sequence
NGRAM_MAX_N = 8


def _i(t: Tensor, dtype: torch.dtype, shape, what: str) -> Tensor:
    if not (isinstance(t, Tensor) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_cuda and t.is_contiguous()):
        got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, Tensor) else type(t).__name__
        raise ValueError(f"{what} must be a contiguous device {dtype} tensor of shape {tuple(shape)}, got {got}")
    return t


def spec_accept(draft: Tensor, sel: Tensor, eos: Optional[Tensor], seq: Tensor, count: Tensor, finished: Tensor, pending: Tensor, key_mask: Tensor,
                next_pos: Tensor, len0: int, emitted: Optional[Tensor] = None, m_out: Optional[Tensor] = None,
                summary: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """The accept rule of a draft-and-verify round (include/setok_hip.h, "Speculative decoding"), one launch: draft (B, K) int64 and the selected
    tokens sel (B, K + 1) int64 -> what every sequence emits.  Updated in place: seq (B, max_new) int64, count (B,) int32, finished (B,) uint8,
    pending (B,) int64, key_mask (B, cap) uint8 (slots [len0, len0 + K]) and next_pos (B,) int64.  eos: (n_eos,) int64 or None.  Returns
    (emitted (B, K + 1) int64, m (B,) int32, summary (3,) int32 = {max m, unfinished sequences, 1 iff a negative token was emitted})."""
    if sel.dim() != 2 or draft.dim() != 2:
        raise ValueError(f"spec_accept: draft and sel must be (B, K) and (B, K + 1), got {tuple(draft.shape)} and {tuple(sel.shape)}")
    B, K = sel.shape[0], sel.shape[1] - 1
    if not 0 <= K <= SPEC_MAX_K:
        raise ValueError(f"spec_accept: K={K} is outside [0, {SPEC_MAX_K}]")
    if seq.dim() != 2 or seq.shape[1] < 1 or key_mask.dim() != 2:
        raise ValueError(f"spec_accept: seq must be (B, max_new >= 1) and key_mask (B, cap), got {tuple(seq.shape)} and {tuple(key_mask.shape)}")
    max_new, cap = seq.shape[1], key_mask.shape[1]
    if len0 < 0 or len0 + K + 1 > cap:
        raise ValueError(f"spec_accept: slots [{len0}, {len0} + {K}] exceed the cache (cap = {cap})")
    i64, i32, u8 = torch.int64, torch.int32, torch.uint8
    _i(draft, i64, (B, K), "spec_accept: draft"); _i(sel, i64, (B, K + 1), "spec_accept: sel"); _i(seq, i64, (B, max_new), "spec_accept: seq")
    _i(count, i32, (B,), "spec_accept: count"); _i(finished, u8, (B,), "spec_accept: finished"); _i(pending, i64, (B,), "spec_accept: pending")
    _i(key_mask, u8, (B, cap), "spec_accept: key_mask"); _i(next_pos, i64, (B,), "spec_accept: next_pos")
    n_eos = 0
    if eos is not None:
        n_eos = eos.numel()
        _i(eos, i64, (n_eos,), "spec_accept: eos")
    dev = sel.device
    emitted = torch.empty((B, K + 1), dtype=i64, device=dev) if emitted is None else _i(emitted, i64, (B, K + 1), "spec_accept: emitted")
    m_out = torch.empty(B, dtype=i32, device=dev) if m_out is None else _i(m_out, i32, (B,), "spec_accept: m_out")
    summary = torch.zeros(3, dtype=i32, device=dev) if summary is None else _i(summary, i32, (3,), "spec_accept: summary")
    _lib.call("setok_spec_accept", _stream(), draft.data_ptr() if K else None, sel.data_ptr(), B, K, eos.data_ptr() if n_eos else None, n_eos, max_new,
              seq.data_ptr(), count.data_ptr(), finished.data_ptr(), pending.data_ptr(), key_mask.data_ptr(), next_pos.data_ptr(), cap, len0,
              emitted.data_ptr(), m_out.data_ptr(), summary.data_ptr())
    return emitted, m_out, summary


def ngram_propose(hist: Tensor, hist_len: Tensor, K: int, len_max: int, emitted: Optional[Tensor] = None, m: Optional[Tensor] = None,
                  max_ngram: int = 3, min_ngram: int = 1, out: Optional[Tensor] = None) -> Tensor:
    """The lookup drafter's launch (include/setok_hip.h, "Speculative decoding"): append emitted[b, :m[b]] to the history hist (B, cap_h) int64 /
    hist_len (B,) int32 (in place; both None: propose only), then out (B, K) int64 = the continuation of the most recent earlier occurrence of the
    longest trailing n-gram, max_ngram down to min_ngram, -1 where there is none.  len_max: the caller's bound on max_b (hist_len[b] + m[b])."""
    if hist.dim() != 2:
        raise ValueError(f"ngram_propose: hist must be (B, cap_h), got {tuple(hist.shape)}")
    B, cap_h = hist.shape
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= SPEC_MAX_K:
        raise ValueError(f"ngram_propose: K={K!r} must be an int in [1, {SPEC_MAX_K}]")
    if not 1 <= min_ngram <= max_ngram <= NGRAM_MAX_N:
        raise ValueError(f"ngram_propose: the n-gram range [{min_ngram}, {max_ngram}] must satisfy 1 <= min_ngram <= max_ngram <= {NGRAM_MAX_N}")
    if cap_h < 1 or not 0 <= len_max <= cap_h:
        raise ValueError(f"ngram_propose: hist_len + m > cap_h (the history may reach {len_max} entries, a row holds {cap_h})")
    _i(hist, torch.int64, (B, cap_h), "ngram_propose: hist"); _i(hist_len, torch.int32, (B,), "ngram_propose: hist_len")
    n_emit = 0
    if (emitted is None) != (m is None):
        raise ValueError("ngram_propose: pass emitted and m together, or neither")
    if emitted is not None:
        if emitted.dim() != 2 or not 1 <= emitted.shape[1] <= SPEC_MAX_K + 1:
            raise ValueError(f"ngram_propose: emitted must be (B, 1 .. {SPEC_MAX_K + 1}), got {tuple(emitted.shape)}")
        n_emit = emitted.shape[1]
        _i(emitted, torch.int64, (B, n_emit), "ngram_propose: emitted"); _i(m, torch.int32, (B,), "ngram_propose: m")
    out = torch.empty((B, K), dtype=torch.int64, device=hist.device) if out is None else _i(out, torch.int64, (B, K), "ngram_propose: out")
    _lib.call("setok_ngram_propose", _stream(), hist.data_ptr(), hist_len.data_ptr(), B, cap_h, int(len_max), emitted.data_ptr() if n_emit else None,
              m.data_ptr() if n_emit else None, n_emit, K, int(max_ngram), int(min_ngram), out.data_ptr())
    return out


# ---- logits processors (csrc/logits.hip) ---------------------------------------------------------------------------------------------------------
LOGITS_MAX_NGRAM = 8
LOGITS_MAX_IDS = 64                               # eos ids / suppressed ids per call


def logits_process(logits: Tensor, hist: Tensor, hist_len: Tensor, prompt_len: Tensor, tail: Optional[Tensor] = None, penalty: float = 1.0,
                   ngram: int = 0, min_new: int = 0, eos: Optional[Tensor] = None, suppress: Optional[Tensor] = None,
                   out: Optional[Tensor] = None) -> Tensor:
    """fp32 (B * n, V): the step's logits (B * n, V; any row stride) after the repetition penalty, the n-gram bans, the minimum-length eos ban and
    the suppression (include/setok_hip.h, "Logits processors"), one launch.  hist (B, cap_h) int64 with hist_len (B,) int32 valid entries and
    prompt_len (B,) int32; row b * n + i sees sequence b's history followed by tail[b, :i] (tail (B, n - 1) int64, None with n = 1).  eos and
    suppress: (count <= 64,) int64 or None.  `out` may be a (B * n, V) fp32 view with any row stride; it must not overlap `logits`."""
    if logits.dim() != 2 or hist.dim() != 2:
        raise ValueError(f"logits_process: logits must be (B * n, V) and hist (B, cap_h), got {tuple(logits.shape)} and {tuple(hist.shape)}")
    rows, V = logits.shape
    B, cap_h = hist.shape
    n = 1 if tail is None else tail.shape[1] + 1
    if rows != B * n:
        raise ValueError(f"logits_process: {rows} rows of logits are not B * n = {B} * {n}")
    assert logits.stride(1) == 1 and logits.is_cuda
    i64, i32 = torch.int64, torch.int32
    _i(hist, i64, (B, cap_h), "logits_process: hist"); _i(hist_len, i32, (B,), "logits_process: hist_len")
    _i(prompt_len, i32, (B,), "logits_process: prompt_len")
    if tail is not None:
        _i(tail, i64, (B, n - 1), "logits_process: tail")
    counts = []
    for ids, what in ((eos, "eos"), (suppress, "suppress")):
        counts.append(0 if ids is None else ids.numel())
        if ids is not None:
            _i(ids, i64, (counts[-1],), f"logits_process: {what}")
    if out is None:
        out = torch.empty((rows, V), dtype=torch.float32, device=logits.device)
    assert out.dtype == torch.float32 and out.shape == (rows, V) and out.stride(1) == 1 and out.is_cuda
    ld = logits.stride(0) if rows > 1 else max(logits.stride(0), V)
    ld_out = out.stride(0) if rows > 1 else max(out.stride(0), V)
    _lib.call("setok_logits_process", _stream(), _code(logits.dtype), logits.data_ptr(), ld, B, n, V, hist.data_ptr(), hist_len.data_ptr(),
              prompt_len.data_ptr(), cap_h, tail.data_ptr() if n > 1 else None, float(penalty), int(ngram), int(min_new),
              eos.data_ptr() if counts[0] else None, counts[0], suppress.data_ptr() if counts[1] else None, counts[1], out.data_ptr(), ld_out)
    return out


def history_append(hist: Tensor, hist_len: Tensor, emitted: Tensor, len_max: int, m: Optional[Tensor] = None) -> None:
    """hist[b, hist_len[b]:] = emitted[b, :m[b]] and hist_len[b] += m[b], in place, one launch (hist (B, cap_h) int64, hist_len (B,) int32, emitted
    (B, n_emit <= 64) int64, m (B,) int32 or None = every row appends n_emit entries).  len_max: the caller's bound on max_b (hist_len[b] + m[b]);
    a bound above cap_h is refused, and the kernel never writes behind a row."""
    if hist.dim() != 2 or emitted.dim() != 2:
        raise ValueError(f"history_append: hist must be (B, cap_h) and emitted (B, n_emit), got {tuple(hist.shape)} and {tuple(emitted.shape)}")
    B, cap_h = hist.shape
    n_emit = emitted.shape[1]
    if n_emit > SPEC_MAX_K + 1:
        raise ValueError(f"history_append: emitted must be (B, 0 .. {SPEC_MAX_K + 1}), got {tuple(emitted.shape)}")
    if cap_h < 1 or not 0 <= len_max <= cap_h:
        raise ValueError(f"history_append: hist_len + m > cap_h (the history may reach {len_max} entries, a row holds {cap_h})")
    _i(hist, torch.int64, (B, cap_h), "history_append: hist"); _i(hist_len, torch.int32, (B,), "history_append: hist_len")
    _i(emitted, torch.int64, (B, n_emit), "history_append: emitted")
    if m is not None:
        _i(m, torch.int32, (B,), "history_append: m")
    _lib.call("setok_history_append", _stream(), hist.data_ptr(), hist_len.data_ptr(), B, cap_h, int(len_max), emitted.data_ptr() if n_emit else None,
              None if m is None else m.data_ptr(), n_emit)


# ---- beam search (csrc/beam.hip) -----------------------------------------------------------------------------------------------------------------
BEAM_MAX_C = 64                                   # candidates per sequence: C = max(2, 1 + n_eos) * num_beams
BEAM_MAX_N = 16                                   # beams per sequence
EARLY_STOPPING = {False: 0, True: 1, "never": 2}  # setok_beam_advance's code of HF's early_stopping


def beam_topk(logits: Tensor, running: Tensor, C: int, ws: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """Per sequence, the C largest of running[b][j] + log_softmax(row j)[v] over its n_in rows (include/setok_hip.h, "Beam search"): logits
    (B * n_in, V) with any row stride, running (B, n_in) fp32 -> (cand_score (B, C) fp32, cand_token (B, C) int64, cand_beam (B, C) int32,
    status (B,) int32 = 1 where a row of the sequence holds a NaN or +inf), descending, ties to the lower flat index j * V + v."""
    if logits.dim() != 2 or running.dim() != 2 or running.shape[0] * running.shape[1] != logits.shape[0]:
        raise ValueError(f"beam_topk: logits must be (B * n_in, V) and running (B, n_in), got {tuple(logits.shape)} and {tuple(running.shape)}")
    (B, n_in), V = running.shape, logits.shape[1]
    if isinstance(C, bool) or not isinstance(C, int) or not 1 <= C <= BEAM_MAX_C or C > n_in * V:
        raise ValueError(f"beam_topk: C={C!r} must be an int in [1, {BEAM_MAX_C}] and at most n_in * V = {n_in * V}")
    if not 1 <= n_in <= BEAM_MAX_N:
        raise ValueError(f"beam_topk: n_in={n_in} is outside [1, {BEAM_MAX_N}]")
    assert logits.stride(1) == 1 and logits.is_cuda
    _i(running, torch.float32, (B, n_in), "beam_topk: running")
    dev = logits.device
    need = B * n_in * (BEAM_MAX_C * 2 + 1)
    if ws is None or ws.numel() < need:
        ws = torch.empty(max(need, 1), dtype=torch.int32, device=dev)
    assert ws.dtype == torch.int32 and ws.is_cuda and ws.is_contiguous()
    score = torch.empty((B, C), dtype=torch.float32, device=dev)
    token = torch.empty((B, C), dtype=torch.int64, device=dev)
    beam = torch.empty((B, C), dtype=torch.int32, device=dev)
    status = torch.empty(B, dtype=torch.int32, device=dev)
    rows = B * n_in
    _lib.call("setok_beam_topk", _stream(), _code(logits.dtype), logits.data_ptr(), logits.stride(0) if rows > 1 else max(logits.stride(0), V), B, n_in, V,
              running.data_ptr(), C, score.data_ptr(), token.data_ptr(), beam.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    return score, token, beam, status


class BeamState:
    """The device-resident state of `setok_beam_advance` for B sequences of n beams over at most max_new steps (include/setok_hip.h, "Beam search")."""

    def __init__(self, B: int, n: int, max_new: int, device):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)
        self.B, self.n, self.max_new = B, n, max_new
        self.run_score = z((B, n), torch.float32)
        self.fin_score = torch.full((B, n), -1.0e9, dtype=torch.float32, device=device)
        self.fin_flag, self.fin_len, self.fin_parent, self.fin_token = z((B, n), torch.uint8), z((B, n), torch.int32), z((B, n), torch.int32), z((B, n), torch.int64)
        self.heur = torch.ones(B, dtype=torch.uint8, device=device)
        self.bp_token, self.bp_parent = z((max_new, B * n), torch.int64), z((max_new, B * n), torch.int32)
        self.next_token, self.src_row, self.summary = z(B * n, torch.int64), z(B * n, torch.int32), z(2, torch.int32)


def beam_advance(score: Tensor, token: Tensor, beam: Tensor, status: Tensor, state: BeamState, eos: Optional[Tensor], step: int,
                 length_penalty: float = 1.0, early_stopping=False) -> Tuple[Tensor, Tensor, Tensor]:
    """One step of HF's beam bookkeeping on the candidates of `beam_topk` (include/setok_hip.h, "Beam search"), one launch: `state` is updated in
    place; returns (next_token (B * n,) int64, src_row (B * n,) int32, summary (2,) int32 = {continue, bad row}) - views of the state."""
    B, n = state.B, state.n
    if score.dim() != 2:
        raise ValueError(f"beam_advance: the candidates must be (B, C), got {tuple(score.shape)}")
    C = score.shape[1]
    if not n <= C <= BEAM_MAX_C:
        raise ValueError(f"beam_advance: C={C} is outside [n, {BEAM_MAX_C}] = [{n}, {BEAM_MAX_C}]")
    if not (isinstance(early_stopping, bool) or (isinstance(early_stopping, str) and early_stopping == "never")):
        raise ValueError(f"beam_advance: early_stopping={early_stopping!r} is not one of False, True, 'never'")
    if not 0 <= step < state.max_new:
        raise ValueError(f"beam_advance: step {step} is outside [0, max_new = {state.max_new})")
    _i(score, torch.float32, (B, C), "beam_advance: cand_score"); _i(token, torch.int64, (B, C), "beam_advance: cand_token")
    _i(beam, torch.int32, (B, C), "beam_advance: cand_beam"); _i(status, torch.int32, (B,), "beam_advance: status")
    n_eos = 0
    if eos is not None:
        n_eos = eos.numel()
        _i(eos, torch.int64, (n_eos,), "beam_advance: eos")
    s = state
    _lib.call("setok_beam_advance", _stream(), score.data_ptr(), token.data_ptr(), beam.data_ptr(), status.data_ptr(), B, n, C,
              eos.data_ptr() if n_eos else None, n_eos, int(step), s.max_new, float(length_penalty), EARLY_STOPPING[early_stopping],
              s.run_score.data_ptr(), s.fin_score.data_ptr(), s.fin_flag.data_ptr(), s.fin_len.data_ptr(), s.fin_parent.data_ptr(), s.fin_token.data_ptr(),
              s.heur.data_ptr(), s.bp_token.data_ptr(), s.bp_parent.data_ptr(), s.next_token.data_ptr(), s.src_row.data_ptr(), s.summary.data_ptr())
    return s.next_token, s.src_row, s.summary


class KVReorderPlan:
    """The device tables `setok_kv_reorder` takes, built once for a list of cache tensors - each (rows, Hkv, cap) or (rows, Hkv, cap, Dh), contiguous,
    any element size - and the scratch region, grown to the largest slot range asked for."""

    def __init__(self, tensors, n: int):
        t0 = tensors[0]
        self.rows, self.Hkv, self.cap = t0.shape[:3]
        self.n, self.tensors = n, list(tensors)
        if self.rows % n:
            raise ValueError(f"kv_reorder: {self.rows} rows are not groups of n = {n}")
        rb = []
        for t in self.tensors:
            if tuple(t.shape[:3]) != (self.rows, self.Hkv, self.cap) or t.dim() not in (3, 4) or not (t.is_cuda and t.is_contiguous()):
                raise ValueError(f"kv_reorder: every tensor must be a contiguous device (rows, Hkv, cap[, Dh]) = ({self.rows}, {self.Hkv}, {self.cap}), "
                                 f"got {tuple(t.shape)}")
            rb.append(t.element_size() * (t.shape[3] if t.dim() == 4 else 1))
        unit, acc = [], 0
        for b in rb:
            unit.append(acc)
            acc += (b + 15) // 16 * 16
        dev = t0.device
        self.unit_total = acc
        self.ptrs = torch.tensor([t.data_ptr() for t in self.tensors], dtype=torch.int64).to(dev)
        self.row_bytes = torch.tensor(rb, dtype=torch.int32).to(dev)
        self.scratch_unit = torch.tensor(unit, dtype=torch.int64).to(dev)
        self.scratch: Optional[Tensor] = None
        self.status = torch.zeros(self.rows, dtype=torch.int32, device=dev)

    def room(self, ns: int) -> Tensor:
        need = self.unit_total * self.rows * self.Hkv * ns
        if self.scratch is None or self.scratch.numel() < need:
            self.scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=self.status.device)
        return self.scratch


def kv_reorder(plan: KVReorderPlan, src_row: Tensor, slot0: int, slot1: int, reserve: Optional[int] = None) -> Tensor:
    """Slots [slot0, slot1) of row r of every tensor of `plan` become what row src_row[r] (int32, inside r's own group of plan.n rows) held before the
    call: two launches for all tensors (include/setok_hip.h, "Beam search").  `reserve`: size the scratch for that many slots at once.  Returns
    plan.status (rows,) int32: 1 where a src_row was outside its group (that row then keeps its data), sticky across calls."""
    if not 0 <= slot0 <= slot1 <= plan.cap:
        raise ValueError(f"kv_reorder: slots [{slot0}, {slot1}) are not inside the cache (cap = {plan.cap})")
    _i(src_row, torch.int32, (plan.rows,), "kv_reorder: src_row")
    scratch = plan.room(max(slot1 - slot0, reserve or 0))
    _lib.call("setok_kv_reorder", _stream(), plan.ptrs.data_ptr(), plan.row_bytes.data_ptr(), plan.scratch_unit.data_ptr(), len(plan.tensors),
              plan.unit_total, plan.rows, plan.n, plan.Hkv, plan.cap, int(slot0), int(slot1), src_row.data_ptr(), scratch.data_ptr(), scratch.numel(),
              plan.status.data_ptr())
    return plan.status


# ---- fp8 weight-only storage (csrc/gemm_fp8w.hip; the M <= 64 GEMM it shares with MXFP4: csrc/wstream.h, here _linear_wstream) -----------------
FP8W_MAX_M = 64                                   # rows setok_linear_fp8w takes; more rows dequantise and go through `linear`


def _rows_ld(t: Tensor) -> int:
    """Row stride of a 2-d tensor whose rows are dense (a column window of a wider buffer is fine)."""
    assert t.dim() == 2 and t.is_cuda and (t.stride(1) == 1 or t.shape[1] == 1), "2-d device tensor with dense rows required"
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _linear_wstream(sym: str, max_m: int, dequantize, a: Tensor, q: Tensor, scale_args: tuple, pair: tuple, N: int, K: int,
                    residual: Optional[Tensor], out: Optional[Tensor], scratch: Optional[Tensor], min_wgs: Optional[int]) -> Tensor:
    """What linear_fp8w and linear_mxfp4w share once their operands are checked (csrc/wstream.h): up to `max_m` rows ONE launch of the entry point `sym`
    (`sym`_wgs with a floor), more rows `dequantize(*pair)` into `scratch` and the existing `linear`.  `scale_args` is what the entry
    point takes between q's row stride and the residual."""
    M, Ka = a.shape
    assert K == Ka
    if M > max_m:
        if scratch is None or scratch.dtype != a.dtype or scratch.numel() < N * K:
            raise ValueError(f"{sym[6:]}: M={M} > {max_m} dequantises the weight: pass `scratch`, {N * K} elements of {a.dtype}")
        w = dequantize(*pair, out=scratch.reshape(-1)[:N * K].view(N, K))
        return linear(a, w, residual=residual, out=out)
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    assert out.shape == (M, N) and out.dtype == a.dtype
    ldc = _rows_ld(out)
    if residual is not None:
        assert residual.shape == (M, N) and residual.dtype == a.dtype and (M == 1 or _rows_ld(residual) == ldc), "residual shares out's row stride"
    args = (_stream(), _code(a.dtype), a.data_ptr(), _rows_ld(a), q.data_ptr(), _rows_ld(q), *scale_args,
            None if residual is None else residual.data_ptr(), out.data_ptr(), ldc, M, N, K)
    if min_wgs is None:
        _lib.call(sym, *args)
    else:
        _lib.call(sym + "_wgs", *args, int(min_wgs))
    return out


def quantize_fp8_rows(w: Tensor, q: Optional[Tensor] = None, e: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """w (N, K) fp32 / bf16 / fp16 -> (q (N, K) uint8 of e4m3fn codes, e (N,) int8) with w' = value(q) * 2^e[:, None] (include/setok_hip.h)."""
    N, K = w.shape
    if q is None:
        q = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    if e is None:
        e = torch.empty(N, dtype=torch.int8, device=w.device)
    assert q.shape == (N, K) and q.dtype == torch.uint8 and e.shape == (N,) and e.dtype == torch.int8 and e.is_contiguous()
    _lib.call("setok_quantize_fp8_rows", _stream(), _code(w.dtype), w.data_ptr(), _rows_ld(w), q.data_ptr(), _rows_ld(q), _p(e), N, K)
    return q, e


def dequantize_fp8_rows(q: Tensor, e: Tensor, dtype: Optional[torch.dtype] = None, out: Optional[Tensor] = None) -> Tensor:
    """The exact inverse of quantize_fp8_rows into `dtype` (or into `out`, whose rows may be wider than K)."""
    N, K = q.shape
    if out is None:
        out = torch.empty((N, K), dtype=dtype, device=q.device)
    assert out.shape == (N, K) and (dtype is None or out.dtype == dtype)
    assert q.dtype == torch.uint8 and e.shape == (N,) and e.dtype == torch.int8 and e.is_contiguous()
    _lib.call("setok_dequantize_fp8_rows", _stream(), _code(out.dtype), q.data_ptr(), _rows_ld(q), _p(e), out.data_ptr(), _rows_ld(out), N, K)
    return out


def linear_fp8w(a: Tensor, q: Tensor, e: Tensor, residual: Optional[Tensor] = None, out: Optional[Tensor] = None,
                scratch: Optional[Tensor] = None, min_wgs: Optional[int] = None) -> Tensor:
    """out = a @ w'.T + residual with w' = value(q) * 2^e[:, None];  a: (M, K), q: (N, K) uint8, e: (N,) int8.  M <= 64 is ONE launch of the
    weight-streaming kernel (a, residual and out may be column windows of wider buffers).  More rows dequantise w' into `scratch` — the
    caller's, at least N * K elements of a.dtype — and run the existing `linear` on it: the same function, `linear`'s summation order.
    `min_wgs` replaces the floor of the kernel's band rule (setok_linear_fp8w_wgs; None: the library's own, one workgroup per CU): it moves
    columns between workgroups and changes no bit."""
    N, K = q.shape
    assert q.dtype == torch.uint8 and e.shape == (N,) and e.dtype == torch.int8 and e.is_contiguous()
    return _linear_wstream("setok_linear_fp8w", FP8W_MAX_M, dequantize_fp8_rows, a, q, (_p(e),), (q, e), N, K, residual, out, scratch, min_wgs)


# ---- MXFP4 weight-only storage (csrc/gemm_mxfp4w.hip; the M <= 64 GEMM it shares with fp8: csrc/wstream.h, here _linear_wstream above) ----------
MXFP4W_MAX_M = 64                                 # rows setok_linear_mxfp4w takes; more rows dequantise and go through `linear`
MXFP4_BLOCK = 32                                  # elements per e8m0 scale byte


def _mxfp4_check(q: Tensor, s: Tensor) -> Tuple[int, int]:
    N, K2 = q.shape
    K = 2 * K2
    assert K % MXFP4_BLOCK == 0 and q.dtype == torch.uint8 and s.dtype == torch.uint8 and s.shape == (N, K // MXFP4_BLOCK), \
        "q (N, K/2) uint8 and s (N, K/32) uint8 with K % 32 == 0 required"
    return N, K


def quantize_mxfp4_rows(w: Tensor, q: Optional[Tensor] = None, s: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """w (N, K) fp32 / bf16 / fp16, K % 32 == 0 -> (q (N, K/2) uint8 of e2m1 nibble pairs, s (N, K/32) uint8 of e8m0 scale bytes) with
    w' = value(nibble) * 2^(s - 127) per block of 32 elements of a row (include/setok_hip.h, "MXFP4 weight-only decode")."""
    N, K = w.shape
    if K % MXFP4_BLOCK != 0:
        raise ValueError(f"quantize_mxfp4_rows: K={K} is not a multiple of {MXFP4_BLOCK}, the MX block")
    if q is None:
        q = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    if s is None:
        s = torch.empty((N, K // MXFP4_BLOCK), dtype=torch.uint8, device=w.device)
    assert _mxfp4_check(q, s) == (N, K)
    _lib.call("setok_quantize_mxfp4_rows", _stream(), _code(w.dtype), w.data_ptr(), _rows_ld(w), q.data_ptr(), _rows_ld(q), s.data_ptr(), _rows_ld(s), N, K)
    return q, s


def dequantize_mxfp4_rows(q: Tensor, s: Tensor, dtype: Optional[torch.dtype] = None, out: Optional[Tensor] = None) -> Tensor:
    """The exact inverse of quantize_mxfp4_rows into `dtype` (or into `out`, whose rows may be wider than K)."""
    N, K = _mxfp4_check(q, s)
    if out is None:
        out = torch.empty((N, K), dtype=dtype, device=q.device)
    assert out.shape == (N, K) and (dtype is None or out.dtype == dtype)
    _lib.call("setok_dequantize_mxfp4_rows", _stream(), _code(out.dtype), q.data_ptr(), _rows_ld(q), s.data_ptr(), _rows_ld(s), out.data_ptr(),
              _rows_ld(out), N, K)
    return out


def linear_mxfp4w(a: Tensor, q: Tensor, s: Tensor, residual: Optional[Tensor] = None, out: Optional[Tensor] = None,
                  scratch: Optional[Tensor] = None, min_wgs: Optional[int] = None) -> Tensor:
    """out = a @ w'.T + residual with w' = value(nibble) * 2^(s - 127);  a: (M, K), q: (N, K/2) uint8, s: (N, K/32) uint8.  M <= 64 is ONE launch of
    the weight-streaming kernel (every operand may be a column window of a wider buffer).  More rows dequantise w' into `scratch` — the caller's,
    at least N * K elements of a.dtype — and run the existing `linear` on it: the same function, `linear`'s summation order.
    `min_wgs` replaces the floor of the kernel's band rule (setok_linear_mxfp4w_wgs; None: the library's own, one workgroup per CU): it moves
    columns between workgroups and changes no bit."""
    N, K = _mxfp4_check(q, s)
    return _linear_wstream("setok_linear_mxfp4w", MXFP4W_MAX_M, dequantize_mxfp4_rows, a, q, (s.data_ptr(), _rows_ld(s)), (q, s), N, K, residual, out,
                           scratch, min_wgs)


# ---- the DiffLoss image head (csrc/diffusion.hip) ---------------------------------------------------------------------------------------------
def timestep_embedding(t: Tensor, dim: int, dtype: torch.dtype, max_period: float = 10000.0, out: Optional[Tensor] = None) -> Tensor:
    """[cos(t f_j) | sin(t f_j)], f_j = exp(-ln(max_period) j / (dim / 2)): t fp32 (rows,) on the device -> (rows, dim) in `dtype`."""
    rows = t.numel()
    _f32(t)
    if out is None:
        out = torch.empty((rows, dim), dtype=dtype, device=t.device)
    assert out.shape == (rows, dim) and out.dtype == dtype
    if rows == 0:                                    # (an empty tensor has no storage: nothing to hand to the library)
        return out
    _lib.call("setok_timestep_embedding", _stream(), _code(dtype), _p(t), _p(out), rows, dim, float(max_period))
    return out


def add_silu(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """SiLU(a + b); b: a's shape, or ONE row (C,) / (1, C) added to every row of a."""
    rows, Cc = a.shape
    assert b.dtype == a.dtype and b.shape[-1] == Cc and b.stride(-1) == 1 and b.is_cuda
    one = b.dim() == 1 or b.shape[0] == 1
    assert one or (b.dim() == 2 and b.shape[0] == rows)
    if out is None:
        out = torch.empty_like(a)
    if rows == 0:
        return out
    _lib.call("setok_add_silu", _stream(), _code(a.dtype), _p(a), b.data_ptr(), 0 if one else b.stride(0), _p(out), rows, Cc)
    return out


def adaln_modulate(x: Tensor, shift: Tensor, scale: Tensor, gamma: Optional[Tensor] = None, beta: Optional[Tensor] = None, eps: float = 1e-6,
                   h: Optional[Tensor] = None, gate: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """[x += gate * h, in place;]  LayerNorm(x; gamma, beta) * (1 + scale) + shift.  shift / scale / gate: (rows, C) column windows of ONE wider
    row-major buffer (they share its row stride); gamma / beta None: no affine."""
    rows, Cc = x.shape
    wins = [shift, scale] + ([gate] if gate is not None else [])
    for w in wins:
        assert w.shape == (rows, Cc) and w.dtype == x.dtype and w.stride(1) == 1 and w.is_cuda and (rows <= 1 or w.stride(0) == shift.stride(0))
    ldm = shift.stride(0) if rows > 1 else max(shift.stride(0), Cc)
    assert (h is None) == (gate is None) and (h is None or (h.shape == x.shape and h.dtype == x.dtype))
    if out is None:
        out = torch.empty_like(x)
    assert out.shape == x.shape and out.dtype == x.dtype
    if rows == 0:
        return out
    _lib.call("setok_adaln_modulate", _stream(), _code(x.dtype), _p(x), _p(h), None if gate is None else gate.data_ptr(), _p(_f32(gamma)), _p(_f32(beta)),
              shift.data_ptr(), scale.data_ptr(), ldm, _p(out), rows, Cc, float(eps))
    return out


def ddpm_step(out: Tensor, x: Tensor, noise: Tensor, x_in: Tensor, coef, nonzero: float, temperature: float = 1.0, cfg: float = 1.0, half: int = 0) -> None:
    """One reverse DDPM step in place on the fp32 state x (rows, C) from the net's output `out` (rows, 2 C; x_in's dtype or fp32); x_in (rows, C): the
    next evaluation's operand.  coef: (sqrt_recip_alphas_cumprod, sqrt_recipm1_alphas_cumprod, posterior_mean_coef1, posterior_mean_coef2,
    posterior_log_variance_clipped, log beta) of the step.  half > 0: classifier-free guidance over rows [0, half) | [half, 2 half)."""
    rows, Cc = x.shape
    _f32(x), _f32(noise)
    assert out.shape == (rows, 2 * Cc) and out.stride(1) == 1 and out.is_cuda and out.dtype in (x_in.dtype, torch.float32)
    assert x_in.shape == (rows, Cc) and noise.dim() == 2 and noise.shape[1] == Cc
    a, b, c1, c2, lo, hi = (float(v) for v in coef)
    if rows == 0:
        return
    _lib.call("setok_ddpm_step", _stream(), _code(x_in.dtype), _code(out.dtype), out.data_ptr(), out.stride(0) if rows > 1 else max(out.stride(0), 2 * Cc),
              _p(x), _p(noise), noise.shape[0], _p(x_in), rows, Cc, int(half), float(cfg), a, b, c1, c2, lo, hi, float(nonzero), float(temperature))
