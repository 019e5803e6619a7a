"""Backward pass of the reconstruction decoder (SetokDeTokenizer, detokenizer.py) on the HIP library.

The reference trains SeTok's first stage as one autograd graph: tokenize, detokenize, pixel loss, `backward()` (src/model/setok/model.py:86-92).
Here the decoder's forward runs on the library and keeps its activations (SetokDeTokenizer._compute with `saved`); this module writes out the
backward in reverse stage order, every GEMM a `setok_linear` call (training.linear_bwd: dX = dY W, split-K dW = dY^T X, the bias gradient from
dY's transpose):

    pixel loss + unpatchify        ops.pixel_loss_bwd: d(patch rows) in the pixel head GEMM's padded layout, one pass
    to_pixels, decoder_norm        linear_bwd, setok_layernorm_bwd
    pixel decoder blocks (pre-LN)  fc2, erf-GELU (pre-activation recomputed), fc1, norm2 (+ residual), proj, attention (ops.mha_bwd), qkv,
                                   norm1 (+ residual); the normalised rows the dW GEMMs read are recomputed with ops.layernorm, so the bf16
                                   LN-folded forward needs nothing extra
    decoder_fc_in                  the 2-D positional table is a constant: its add passes the gradient through
    Q-Former layers (post-LN)      output_query LayerNorm, FFN; crossattention LayerNorm, dense, cross-attention (ops.mha_bwd, ragged keys),
                                   query and fused key|value — the token side sums into d(enc) over the cross-attention layers;
                                   self-attention LayerNorm, dense, attention, fused q|k|v
    shared-query prefix            the forward ran it on Q rows once and broadcast them to B images: the gradient is summed over the images in
                                   a fixed order (setok_colsum on a (B, Q * hidden) view), then continues on Q rows into
                                   mapper.embeddings.LayerNorm and mask_tokens
    mapper_fc_in                   d(tokens)

Only what is asked for is computed: a Linear whose parameters need no gradient skips its dW GEMMs, and the pass stops at the first stage
nothing upstream of which needs a gradient (a frozen decoder with tokens requiring one computes the dX chain only).  Deterministic: no atomics.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import torch

from . import ops
from .training import linear_bwd


def _ln_bwd(x, dy, ln, grads, name, res=None, need_dx=True):
    C = x.shape[1]
    dg = torch.empty((C,), dtype=torch.float32, device=x.device)
    db = torch.empty_like(dg)
    dx = ops.layernorm_bwd(x, dy, ln[0], ln[2], dg, db, accumulate=False, need_dx=need_dx, res=res)
    grads[name + ".weight"], grads[name + ".bias"] = dg, db
    return dx


def _split(grads, src, names, sizes):
    """Rows of a fused weight's gradient (and its bias's) back under the reference's parameter names."""
    w, b = grads.pop(src + ".weight", None), grads.pop(src + ".bias", None)
    r = 0
    for n, k in zip(names, sizes):
        if w is not None:
            grads[n + ".weight"] = w[r:r + k]
            grads[n + ".bias"] = b[r:r + k]
        r += k


@torch.no_grad()
def detok_backward(det, saved: dict, g: torch.Tensor, need_tokens: bool, need: Dict[str, bool]) -> Tuple[Optional[torch.Tensor], Dict[str, torch.Tensor]]:
    """g: the incoming gradient of the forward's result — (B, Q, D) for "feats", (B, 3, H, W) for "image", 0-d for "loss".
    need: parameter name -> requires a gradient.  Returns (d packed tokens or None, fp32 gradients under the reference's names)."""
    pk, mode = saved["pk"], saved["mode"]
    B, Q, D = len(saved["counts"]), det.num_mask_token, det.decoder_embed_dim
    cfg = det.mapper.cfg
    hs, Hh = cfg["hidden_size"], cfg["num_attention_heads"]
    Dh_q = hs // Hh
    Hd = det.decoder_nheads
    Dh_d = D // Hd
    dt = saved["packed"].dtype
    grads: Dict[str, torch.Tensor] = {}

    def wants(prefix: str) -> bool:
        return any(v for n, v in need.items() if n.startswith(prefix))

    # what each stage upstream of the pixel decoder needs: stage k must hand a gradient on iff some stage before it wants one
    need_enc = need_tokens or wants("mapper_fc_in.")
    qf = saved["qformer"]
    stage_wants = []
    for e in qf:
        if e[0] == "self":
            stage_wants.append(wants(f"mapper.encoder.layer.{e[1]}.attention."))
        elif e[0] == "cross":
            stage_wants.append(need_enc or wants(f"mapper.encoder.layer.{e[1]}.crossattention."))
        elif e[0] == "ffn":
            stage_wants.append(wants(f"mapper.encoder.layer.{e[1]}.intermediate_query.") or wants(f"mapper.encoder.layer.{e[1]}.output_query."))
        else:
            stage_wants.append(False)
    emb_wants = wants("mapper.embeddings.") or need.get("mask_tokens", False)
    upstream = [emb_wants or any(stage_wants[:k]) for k in range(len(qf))]      # upstream[k]: a stage before k wants a gradient

    # ---- pixel head and loss -----------------------------------------------------------------------------------------------------
    if mode == "feats":
        dh = g.to(dt).reshape(B * Q, D).contiguous()
    else:
        wpx = pk["pix"][0]
        gh, gw, p = det.height, det.weight, det.patch_size
        if mode == "loss":
            dpatch = ops.pixel_loss_bwd(saved["img"], saved["gold"], saved["kind"], g, wpx.shape[0], gh, gw, p)
        else:
            one = torch.ones((), dtype=torch.float32, device=wpx.device)
            dpatch = ops.pixel_loss_bwd(g.to(dt).contiguous(), None, "unpatchify", one, wpx.shape[0], gh, gw, p)
        want_px = wants("to_pixels.")
        dh = linear_bwd(saved["feats"], wpx, dpatch, grads, "to_pixels", need_dw=want_px)
        if want_px:
            n_out = det.to_pixels.out_features
            grads["to_pixels.weight"] = grads["to_pixels.weight"][:n_out]
            grads["to_pixels.bias"] = grads["to_pixels.bias"][:n_out]

    # ---- decoder_norm, pixel decoder blocks in reverse ---------------------------------------------------------------------------
    blocks = saved["blocks"]
    dh = _ln_bwd(blocks[-1][1], dh, pk["dec_ln"], grads, "decoder_norm")
    for _, bi, h_in, qkv, o, h_mid, u in reversed(blocks[:-1]):
        b = pk["blocks"][bi]
        pre = f"pixel_decoder.{bi}."
        du = linear_bwd(u, b["fc2"][0], dh, grads, pre + "mlp.fc2", need_dw=wants(pre + "mlp.fc2."))
        y2 = ops.layernorm(h_mid, *b["n2"][:2], b["n2"][2])
        dpre = ops.gelu_bwd(ops.linear(y2, *b["fc1"]), du)
        dy2 = linear_bwd(y2, b["fc1"][0], dpre, grads, pre + "mlp.fc1", need_dw=wants(pre + "mlp.fc1."))
        dh_mid = _ln_bwd(h_mid, dy2, b["n2"], grads, pre + "norm2", res=dh)
        do = linear_bwd(o, b["proj"][0], dh_mid, grads, pre + "attn.proj", need_dw=wants(pre + "attn.proj."))
        dqkv = torch.empty_like(qkv)
        ops.mha_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, do, Hd, Dh_d, Dh_d ** -0.5, Q, None, B, Q,
                    dq=dqkv[:, :D], dk=dqkv[:, D:2 * D], dv=dqkv[:, 2 * D:])
        y1 = ops.layernorm(h_in, *b["n1"][:2], b["n1"][2])
        dy1 = linear_bwd(y1, b["qkv"][0], dqkv, grads, pre + "attn.qkv", need_dw=wants(pre + "attn.qkv."))
        dh = _ln_bwd(h_in, dy1, b["n1"], grads, pre + "norm1", res=dh_mid)

    # ---- decoder_fc_in (+ the constant positional table) -------------------------------------------------------------------------
    dh = linear_bwd(saved["mapped"], pk["dec_in"][0], dh, grads, "decoder_fc_in", need_dx=bool(qf) and (upstream[-1] or stage_wants[-1]),
                    need_dw=wants("decoder_fc_in."))

    # ---- Q-Former in reverse ------------------------------------------------------------------------------------------------------
    enc, kv_offsets = saved["enc"], saved["kv_offsets"]
    denc = None
    for k in reversed(range(len(qf))):
        if dh is None:
            break
        e = qf[k]
        go_on = upstream[k]                                                    # hand a gradient to the stage before?
        if e[0] == "ffn":
            _, li, h_c, u, y = e
            d, pre = pk["layers"][li], f"mapper.encoder.layer.{li}."
            dy = _ln_bwd(y, dh, d["fln"], grads, pre + "output_query.LayerNorm")
            du = linear_bwd(u, d["fo"][0], dy, grads, pre + "output_query.dense", need_dw=wants(pre + "output_query.dense."))
            dpre = ops.gelu_bwd(ops.linear(h_c, *d["fi"]), du)
            dh = linear_bwd(h_c, d["fi"][0], dpre, grads, pre + "intermediate_query.dense", need_dx=go_on, residual=dy,
                            need_dw=wants(pre + "intermediate_query.dense."))
        elif e[0] == "cross":
            _, li, h_b, q, kv, o, y = e
            d, pre = pk["layers"][li], f"mapper.encoder.layer.{li}.crossattention."
            dy = _ln_bwd(y, dh, d["cln"], grads, pre + "output.LayerNorm")
            do = linear_bwd(o, d["co"][0], dy, grads, pre + "output.dense", need_dw=wants(pre + "output.dense."))
            dkv = torch.empty_like(kv)
            dq, _, _ = ops.mha_bwd(q, kv[:, :hs], kv[:, hs:], o, do, Hh, Dh_q, 1.0 / math.sqrt(Dh_q), Q, kv_offsets, B, max(saved["counts"]),
                                   dk=dkv[:, :hs], dv=dkv[:, hs:])
            want_kv = wants(pre + "self.key.") or wants(pre + "self.value.")
            if need_enc or want_kv:
                denc = linear_bwd(enc, d["ckv"][0], dkv, grads, pre + "self.kv", need_dx=need_enc, residual=denc if need_enc else None,
                                  need_dw=want_kv)
                _split(grads, pre + "self.kv", [pre + "self.key", pre + "self.value"], [hs, hs])
            dh = linear_bwd(h_b, d["cq"][0], dq, grads, pre + "self.query", need_dx=go_on, residual=dy, need_dw=wants(pre + "self.query."))
        elif e[0] == "bcast":                                                  # the shared rows were broadcast to B images: sum over them
            if go_on:
                dh = ops.colsum(dh.reshape(B, Q * hs)).to(dt).reshape(Q, hs)
            else:
                dh = None
        else:
            _, li, nb, h_a, qkv, o, y = e
            d, pre = pk["layers"][li], f"mapper.encoder.layer.{li}.attention."
            dy = _ln_bwd(y, dh, d["sln"], grads, pre + "output.LayerNorm")
            do = linear_bwd(o, d["so"][0], dy, grads, pre + "output.dense", need_dw=wants(pre + "output.dense."))
            dqkv = torch.empty_like(qkv)
            ops.mha_bwd(qkv[:, :hs], qkv[:, hs:2 * hs], qkv[:, 2 * hs:], o, do, Hh, Dh_q, 1.0 / math.sqrt(Dh_q), Q, None, nb, Q,
                        dq=dqkv[:, :hs], dk=dqkv[:, hs:2 * hs], dv=dqkv[:, 2 * hs:])
            want_qkv = wants(pre + "self.")
            dh = linear_bwd(h_a, d["qkv"][0], dqkv, grads, pre + "self.qkv", need_dx=go_on, residual=dy, need_dw=want_qkv)
            if want_qkv:
                _split(grads, pre + "self.qkv", [pre + "self.query", pre + "self.key", pre + "self.value"], [hs, hs, hs])
    if dh is not None and emb_wants:                                           # embeddings LayerNorm over the learned queries
        dq0 = _ln_bwd(pk["queries"], dh, pk["emb_ln"], grads, "mapper.embeddings.LayerNorm", need_dx=need.get("mask_tokens", False))
        if dq0 is not None:
            grads["mask_tokens"] = dq0

    # ---- mapper_fc_in ---------------------------------------------------------------------------------------------------------------
    dtok = None
    packed = saved["packed"]
    if denc is not None:
        dtok = linear_bwd(packed, pk["fc_in"][0], denc, grads, "mapper_fc_in", need_dx=need_tokens, need_dw=wants("mapper_fc_in."))
    elif need_tokens:                                                          # no cross-attention layer: the tokens do not reach the output
        dtok = torch.zeros_like(packed)
    return dtok, grads
