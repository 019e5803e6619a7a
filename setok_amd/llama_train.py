"""Forward with saved activations and the dX chain through the FROZEN Llama (llama.LlamaModel) — what stage 2 of the reference's recipe needs
from the LLM: d loss / d inputs_embeds, carried across the decoder layers to the splice and the projector (scripts/pretrain_mm_proj.sh,
src/train/train_setokim.py:335-339 freeze everything but mm_in_projector).  No weight gradient is formed: no dW GEMM runs.

What is kept per layer (policy): the layer input x0, the post-rotary qkv, the attention output o and the post-attention residual stream x1 —
(3 D + (H + 2 Hkv) Dh) elements per row, 6 D for multi-head attention.  Recomputed in the backward pass: the two RMSNorm outputs (one pass over
a row each) and the gate|up pre-activations, by ONE unfused `ops.linear(y, wgu)` (the fused `linear_swiglu` never writes them; the unfused pair
gives the same bits).  Keeping the (rows, 2 F) pre-activations instead would nearly double the footprint (22016 more elements per row against
24576 at Vicuna-7B dims).

The transposed copies of the frozen weights that the dX GEMMs read are formed per layer per step (`ops.transpose`) and dropped: 2 x 13.5 GB of
traffic per step at 7B in bf16 (a few per cent of the step) against 13.5 GB held next to ~30 GB of saved activations."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch

from . import ops


def _inputs(model, inputs_embeds, attention_mask, position_ids):
    """The (B*T, D) rows, key mask and positions exactly as LlamaModel._forward derives them."""
    B, T, D = inputs_embeds.shape
    dev = inputs_embeds.device
    x = inputs_embeds.to(model.norm.weight.dtype).reshape(B * T, D).contiguous()
    if position_ids is None:
        position_ids = torch.arange(T, device=dev)[None].expand(B, T)
    pos = position_ids.to(device=dev, dtype=torch.int64).reshape(B * T).contiguous()
    km = None if attention_mask is None else attention_mask.to(device=dev).bool().to(torch.uint8).reshape(B * T).contiguous()
    return x, km, pos


def llama_forward_train(model, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                        position_ids: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Dict[str, Any]]:
    """(hidden (B, T, D), saved).  The same library calls in the same order as LlamaModel._forward — the same bits — writing each residual
    stream to a fresh buffer instead of in place."""
    B, T, D = inputs_embeds.shape
    pk = model._pack()
    H, Hkv, dh = model.num_heads, model.num_kv_heads, model.head_dim
    x, km, pos = _inputs(model, inputs_embeds, attention_mask, position_ids)
    layers: List[Tuple[torch.Tensor, ...]] = []
    y = None
    for L in pk["layers"]:
        y = ops.rmsnorm(x, L["n1"], model.eps, out=y)
        qkv = ops.linear(y, L["wqkv"])
        ops.rope_(qkv, pos, H, dh, model.rope_theta, Hkv)
        o = ops.attention_causal(qkv, km, B, T, H, dh, dh ** -0.5, Hkv)
        x1 = ops.linear(o, L["wo"], residual=x)
        y = ops.rmsnorm(x1, L["n2"], model.eps, out=y)
        g = ops.linear_swiglu(y, L["wgu"])
        x2 = ops.linear(g, L["wd"], residual=x1)
        layers.append((x, qkv, o, x1))
        x = x2
    hidden = ops.rmsnorm(x, pk["norm"], model.eps).reshape(B, T, D)
    return hidden, dict(layers=layers, x_last=x, km=km, pos=pos, B=B, T=T)


def saved_bytes(saved: Dict[str, Any]) -> int:
    n = saved["x_last"].numel() * saved["x_last"].element_size()
    for tensors in saved["layers"]:
        n += sum(t.numel() * t.element_size() for t in tensors)
    return n


def _dx(dy: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX = dY W for y = x W^T with W (N, K) frozen: one GEMM against the transposed copy."""
    return ops.linear(dy, ops.transpose(w), out=out)


def llama_backward(model, saved: Dict[str, Any], dhidden: torch.Tensor) -> torch.Tensor:
    """d loss / d inputs_embeds (B, T, D) from d loss / d hidden.  Consumes `saved` layer by layer (each layer's activations are released as
    soon as its gradient has passed)."""
    B, T = saved["B"], saved["T"]
    pk = model._pack()
    H, Hkv, dh = model.num_heads, model.num_kv_heads, model.head_dim
    km, pos = saved["km"], saved["pos"]
    x_last = saved.pop("x_last")
    D = x_last.shape[1]
    dy = dhidden.to(x_last.dtype).reshape(B * T, D).contiguous()
    dx = ops.rmsnorm_bwd(x_last, pk["norm"], dy, model.eps)                       # d loss / d (residual stream after the last layer)
    del x_last, dy
    layers = saved["layers"]
    for L in reversed(pk["layers"]):
        x0, qkv, o, x1 = layers.pop()
        # MLP branch: x2 = x1 + down(swiglu(gate|up(rmsnorm(x1))))
        y = ops.rmsnorm(x1, L["n2"], model.eps)
        pre = ops.linear(y, L["wgu"])                                             # the pre-activation pairs, recomputed
        del y
        dg = _dx(dx, L["wd"])                                                     # 1. down_proj dX
        ops.swiglu_pairs_bwd(pre, dg, out=pre)                                    # 2. d (gate_j, up_j), in place of the pre-activations
        del dg
        dy2 = _dx(pre, L["wgu"])                                                  # 3. gate|up dX (against the pair-interleaved weight)
        del pre
        dx1 = ops.rmsnorm_bwd(x1, L["n2"], dy2, model.eps, dres=dx, out=dy2)      # 4. + the residual branch's gradient
        del dx, dy2, x1
        # attention branch: x1 = x0 + o_proj(attention(rope(qkv(rmsnorm(x0)))))
        do = _dx(dx1, L["wo"])                                                    # 5. o_proj dX
        dqkv = ops.attention_causal_bwd(qkv, km, o, do, B, T, H, dh, dh ** -0.5, Hkv)      # 6.
        del do, qkv, o
        ops.rope_bwd_(dqkv, pos, H, dh, model.rope_theta, Hkv)                    # 7.
        dy1 = _dx(dqkv, L["wqkv"])                                                # 8. q|k|v dX
        del dqkv
        dx = ops.rmsnorm_bwd(x0, L["n1"], dy1, model.eps, dres=dx1, out=dy1)      # 9.
        del dx1, dy1, x0
    return dx.reshape(B, T, D)
