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


# ----------------------------------------------------------------------------------------------------------------------------------------
# LoRA (lora.py): the same stack with adapters on its projections.  Per adapted projection Y = X W^T:
#     forward    T = linear_skinny(drop(X), A);  Y += T (s B)^T          — the existing GEMM with `residual=`, K = r, in place
#     backward   dT = linear_skinny(dY, B^T, alpha = s);  dB = s dY^T T;  dA = dT^T drop(X)   (transpose + linear_tn, fp32)
#                dX += drop_bwd(dT A)                                     — the existing GEMM with `residual=`
# q|k|v stay one fused base GEMM and the adapters write into its column windows; gate|up on an adapted layer run as the unfused `linear` +
# `swiglu_pairs` (the bits of the fused call) with ONE pair-interleaved update: rows 2j / 2j + 1 of its B operand are [B_gate[j] | 0] and
# [0 | B_up[j]] over the columns [T_gate | T_up] (the zero products change no bit of an fp32 accumulation).  Kept per layer on top of the
# frozen path's tensors: the T's, 7 r elements per row.  Recomputed: the RMSNorm outputs, the gate|up pre-activations, the SwiGLU output.
# ----------------------------------------------------------------------------------------------------------------------------------------
class _Drop:
    """drop(X) of one projection: the identity, or ops.dropout with the projection's own counters; the same call on a gradient is its backward."""

    def __init__(self, p: float, seed: Optional[int], layer: int):
        self.p, self.seed, self.layer = p, seed, layer
        self.on = seed is not None

    def offset(self, target: str) -> int:
        from .lora import LoraAdapters
        return LoraAdapters.dropout_offset(self.layer, target)

    def __call__(self, x: torch.Tensor, target: str) -> torch.Tensor:
        return ops.dropout(x, self.p, self.seed, self.offset(target)) if self.on else x

    def add_bwd(self, dxd: torch.Tensor, target: str, into: torch.Tensor) -> None:
        """into += drop_bwd(dxd)"""
        ops.dropout(dxd, self.p, self.seed, self.offset(target), residual=into, out=into)


def _scaled(B: torch.Tensor, s: float) -> torch.Tensor:
    """s B in B's type (exact for a power-of-two s such as the reference's 256 / 128)."""
    return (B.detach() * s).contiguous()


def _gu_operand(pairs, r: int, F: int, s: float):
    """(targets, Bgu): the adapted ones of gate / up and the (2 F, len(targets) r) operand that updates the pair-interleaved pre-activations."""
    ts = [t for t in ("gate_proj", "up_proj") if t in pairs]
    if not ts:
        return ts, None
    B0 = pairs[ts[0]].lora_B
    Bgu = torch.zeros((F, 2, len(ts) * r), dtype=B0.dtype, device=B0.device)
    for j, t in enumerate(ts):
        Bgu[:, 0 if t == "gate_proj" else 1, j * r:(j + 1) * r] = pairs[t].lora_B.detach() * s
    return ts, Bgu.reshape(2 * F, len(ts) * r)


def _qkv_windows(H: int, Hkv: int, dh: int):
    return {"q_proj": (0, H * dh), "k_proj": (H * dh, (H + Hkv) * dh), "v_proj": ((H + Hkv) * dh, (H + 2 * Hkv) * dh)}


def _dropout_seed(model) -> Optional[int]:
    ad = model.lora
    ad.seed = None
    if model.training and ad.lora_dropout > 0.0:
        ad.seed = int(torch.empty((), dtype=torch.int64).random_().item())      # torch's default CPU generator, as the head's dropout draws its seed
    return ad.seed


def llama_lora_forward_train(model, inputs_embeds: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                             position_ids: Optional[torch.Tensor] = None, keep: bool = True) -> Tuple[torch.Tensor, Optional[Dict[str, Any]]]:
    """llama_forward_train with the adapters of `model.lora` applied.  keep=False is the no-graph forward: the same calls, nothing saved."""
    B, T, D = inputs_embeds.shape
    pk = model._pack()
    ad = model.lora
    r, s = ad.r, ad.scaling
    H, Hkv, dh = model.num_heads, model.num_kv_heads, model.head_dim
    win = _qkv_windows(H, Hkv, dh)
    seed = _dropout_seed(model)
    x, km, pos = _inputs(model, inputs_embeds, attention_mask, position_ids)
    layers: List[Tuple[Any, ...]] = []
    for li, L in enumerate(pk["layers"]):
        pairs, drop, Ts = ad.layers[li], _Drop(ad.lora_dropout, seed, li), {}
        y = ops.rmsnorm(x, L["n1"], model.eps)
        qkv = ops.linear(y, L["wqkv"])
        for t in ("q_proj", "k_proj", "v_proj"):
            if t in pairs:
                w = qkv[:, win[t][0]:win[t][1]]
                Ts[t] = ops.linear_skinny(drop(y, t), pairs[t].lora_A.detach())
                ops.linear(Ts[t], _scaled(pairs[t].lora_B, s), residual=w, out=w)
        ops.rope_(qkv, pos, H, dh, model.rope_theta, Hkv)
        o = ops.attention_causal(qkv, km, B, T, H, dh, dh ** -0.5, Hkv)
        x1 = ops.linear(o, L["wo"], residual=x)
        if "o_proj" in pairs:
            Ts["o_proj"] = ops.linear_skinny(drop(o, "o_proj"), pairs["o_proj"].lora_A.detach())
            ops.linear(Ts["o_proj"], _scaled(pairs["o_proj"].lora_B, s), residual=x1, out=x1)
        y = ops.rmsnorm(x1, L["n2"], model.eps, out=y)
        gu, Bgu = _gu_operand(pairs, r, L["wd"].shape[1], s)
        if gu:
            pre = ops.linear(y, L["wgu"])
            Tgu = torch.empty((B * T, len(gu) * r), dtype=y.dtype, device=y.device)
            for j, t in enumerate(gu):
                ops.linear_skinny(drop(y, t), pairs[t].lora_A.detach(), out=Tgu[:, j * r:(j + 1) * r])
            ops.linear(Tgu, Bgu, residual=pre, out=pre)
            Ts["gu"] = Tgu
            g = ops.swiglu_pairs(pre)
            del pre
        else:
            g = ops.linear_swiglu(y, L["wgu"])
        x2 = ops.linear(g, L["wd"], residual=x1)
        if "down_proj" in pairs:
            Ts["down_proj"] = ops.linear_skinny(drop(g, "down_proj"), pairs["down_proj"].lora_A.detach())
            ops.linear(Ts["down_proj"], _scaled(pairs["down_proj"].lora_B, s), residual=x2, out=x2)
        if keep:
            layers.append((x, qkv, o, x1, Ts))
        x = x2
    hidden = ops.rmsnorm(x, pk["norm"], model.eps).reshape(B, T, D)
    if not keep:
        return hidden, None
    return hidden, dict(layers=layers, x_last=x, km=km, pos=pos, B=B, T=T, seed=seed)


def _splits(M: int, N: int, K: int) -> int:
    """Split-K count of a dW = dY^T X GEMM with an (N, K) result over M rows: training.linear_bwd's rule."""
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    return max(1, min(16, 1024 // max(tiles, 1), M // 2048))


def _tn(a: torch.Tensor, b: torch.Tensor, aT: Optional[torch.Tensor] = None, bT: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a^T b in fp32 for a (M, N), b (M, K): transpose + linear_tn.  aT / bT: a transposed copy made earlier with the same split."""
    pad = ops.k_align(a.dtype)
    S = _splits(a.shape[0], a.shape[1], b.shape[1])
    return ops.linear_tn(ops.transpose(a, pad, S) if aT is None else aT, ops.transpose(b, pad, S) if bT is None else bT)


def _lora_bwd(pair, s: float, dy: torch.Tensor, T: torch.Tensor, xd: torch.Tensor, grads: Dict[str, torch.Tensor], name: str) -> torch.Tensor:
    """One adapted projection: fills grads[name.lora_A / lora_B] (fp32) and returns dT (rows, r).  dy, T and xd have dense rows."""
    dT = ops.linear_skinny(dy, ops.transpose(pair.lora_B.detach().contiguous()), alpha=s)
    grads[name + ".lora_B"] = _tn(dy, T).mul_(s)
    grads[name + ".lora_A"] = _tn(dT, xd)
    return dT


def llama_lora_backward(model, saved: Dict[str, Any], dhidden: torch.Tensor) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """(d loss / d inputs_embeds (B, T, D), {"{layer}.{target}.lora_A" / "lora_B": fp32 gradient}).  llama_backward's chain with the adapter
    terms; dropout re-applies the forward's (seed, offset) — no mask was stored."""
    B, T = saved["B"], saved["T"]
    pk = model._pack()
    ad = model.lora
    r, s = ad.r, ad.scaling
    H, Hkv, dh = model.num_heads, model.num_kv_heads, model.head_dim
    win = _qkv_windows(H, Hkv, dh)
    km, pos, seed = saved["km"], saved["pos"], saved["seed"]
    x_last = saved.pop("x_last")
    D = x_last.shape[1]
    dy = dhidden.to(x_last.dtype).reshape(B * T, D).contiguous()
    dx = ops.rmsnorm_bwd(x_last, pk["norm"], dy, model.eps)
    del x_last, dy
    grads: Dict[str, torch.Tensor] = {}
    layers = saved["layers"]
    for li in reversed(range(len(pk["layers"]))):
        L, pairs, drop = pk["layers"][li], ad.layers[li], _Drop(ad.lora_dropout, seed, li)
        x0, qkv, o, x1, Ts = layers.pop()
        A_T = lambda t: ops.transpose(pairs[t].lora_A.detach().contiguous())      # (in, r): the operand of dX += dT A

        def add_dx(dT, t, into):                                                  # into += drop_bwd(dT A)
            if drop.on:
                drop.add_bwd(ops.linear(dT, A_T(t)), t, into)
            else:
                ops.linear(dT, A_T(t), residual=into, out=into)

        # MLP branch
        y = ops.rmsnorm(x1, L["n2"], model.eps)
        pre = ops.linear(y, L["wgu"])
        gu, Bgu = _gu_operand(pairs, r, L["wd"].shape[1], 1.0)                    # (unscaled: alpha = s below)
        if gu:
            ops.linear(Ts["gu"], _gu_operand(pairs, r, L["wd"].shape[1], s)[1], residual=pre, out=pre)
        dg = _dx(dx, L["wd"])                                                     # 1. down_proj dX
        if "down_proj" in pairs:
            gd = drop(ops.swiglu_pairs(pre), "down_proj")
            dT = _lora_bwd(pairs["down_proj"], s, dx, Ts["down_proj"], gd, grads, f"{li}.down_proj")
            del gd
            add_dx(dT, "down_proj", dg)
        ops.swiglu_pairs_bwd(pre, dg, out=pre)                                    # 2.
        del dg
        dy2 = _dx(pre, L["wgu"])                                                  # 3. gate|up dX
        if gu:
            dTgu = ops.linear_skinny(pre, ops.transpose(Bgu), alpha=s)            # (rows, len(gu) r) = [dT_gate | dT_up]
            dBgu = _tn(pre, Ts["gu"]).mul_(s).reshape(-1, 2, len(gu) * r)         # (F, 2, len(gu) r)
            for j, t in enumerate(gu):
                grads[f"{li}.{t}.lora_B"] = dBgu[:, 0 if t == "gate_proj" else 1, j * r:(j + 1) * r].contiguous()
                dT = dTgu[:, j * r:(j + 1) * r].contiguous()
                grads[f"{li}.{t}.lora_A"] = _tn(dT, drop(y, t))
                add_dx(dT, t, dy2)
            del dTgu, dBgu
        del pre, y
        dx1 = ops.rmsnorm_bwd(x1, L["n2"], dy2, model.eps, dres=dx, out=dy2)      # 4.
        del dx, dy2, x1
        # attention branch
        do = _dx(dx1, L["wo"])                                                    # 5. o_proj dX
        if "o_proj" in pairs:
            dT = _lora_bwd(pairs["o_proj"], s, dx1, Ts["o_proj"], drop(o, "o_proj"), grads, f"{li}.o_proj")
            add_dx(dT, "o_proj", do)
        dqkv = ops.attention_causal_bwd(qkv, km, o, do, B, T, H, dh, dh ** -0.5, Hkv)      # 6.
        del do, qkv, o
        ops.rope_bwd_(dqkv, pos, H, dh, model.rope_theta, Hkv)                    # 7.
        dy1 = _dx(dqkv, L["wqkv"])                                                # 8. q|k|v dX
        qkv_t = [t for t in ("q_proj", "k_proj", "v_proj") if t in pairs]
        if qkv_t:
            y = ops.rmsnorm(x0, L["n1"], model.eps)
            for t in qkv_t:
                dyw = dqkv[:, win[t][0]:win[t][1]].contiguous()
                dT = _lora_bwd(pairs[t], s, dyw, Ts[t], drop(y, t), grads, f"{li}.{t}")
                add_dx(dT, t, dy1)
                del dyw
            del y
        del dqkv
        dx = ops.rmsnorm_bwd(x0, L["n1"], dy1, model.eps, dres=dx1, out=dy1)      # 9.
        del dx1, dy1, x0
    return dx.reshape(B, T, D), grads
