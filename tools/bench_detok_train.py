"""Forward + backward step of the reconstruction decoder at cfg3 (bench.py:build_decoder dims, bf16): reconstruction_loss(tokens, gold).backward()
with the decoder's parameters and the tokens requiring gradients, and the attention backward kernels at the step's shapes on their own.

    python tools/bench_detok_train.py [--batch 256] [--steps 5] [--warmup 2]

Prints one JSON line: ms per step (forward and backward split by events), us per pixel-decoder self-attention backward and per Q-Former
cross-attention backward (setok_mha_bwd: the MFMA kernels, and the generic wave-per-row kernels via SETOK_ATTN_BWD_GENERIC=1 in the same
process), the forward attention of a pixel-decoder layer for comparison, and the attention-backward FLOP rate (10 B H T^2 D per
self-attention layer: the five T x T x D products of the backward)."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=5)
    a = ap.parse_args()
    from bench import build_decoder
    from setok_amd import ops
    from setok_amd.tokenizer import RaggedTokens

    dev = "cuda:0"
    dt = torch.bfloat16
    det = build_decoder(dev)
    B = a.batch
    g = torch.Generator().manual_seed(0)
    counts = [int(c) for c in torch.randint(24, 57, (B,), generator=g)]          # L_i in the dynamic-k range
    packed = (torch.randn(sum(counts), 4096, generator=g) * 0.5).to(device=dev, dtype=dt).requires_grad_(True)
    side = det.height * det.patch_size
    gold = torch.randn(B, 3, side, side, generator=g).to(device=dev, dtype=dt)

    fwd, bwd = [], []
    for i in range(a.warmup + a.steps):
        det.zero_grad(set_to_none=True)
        packed.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        loss = det.reconstruction_loss(RaggedTokens(packed, counts), gold)
        e[1].record()
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            fwd.append(e[0].elapsed_time(e[1]))
            bwd.append(e[1].elapsed_time(e[2]))
    assert all(p.grad is not None for p in det.parameters()) and packed.grad is not None

    # the attention backward at the step's shapes
    Q = det.num_mask_token
    D, H = det.decoder_embed_dim, det.decoder_nheads
    Dh = D // H
    qkv = torch.randn(B * Q, 3 * D, generator=g).to(device=dev, dtype=dt)
    o = ops.attention(qkv, H, Dh, Dh ** -0.5, seg_len=Q)
    do = torch.randn(B * Q, D, generator=g).to(device=dev, dtype=dt)
    dqkv = torch.empty_like(qkv)
    self_bwd = lambda: ops.mha_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], o, do, H, Dh, Dh ** -0.5, Q, None, B, Q,
                                   dq=dqkv[:, :D], dk=dqkv[:, D:2 * D], dv=dqkv[:, 2 * D:])
    self_fwd = lambda: ops.attention(qkv, H, Dh, Dh ** -0.5, seg_len=Q, out=o)
    hs, Hq = det.mapper.cfg["hidden_size"], det.mapper.cfg["num_attention_heads"]
    Dq = hs // Hq
    offs = torch.zeros(B + 1, dtype=torch.int32)
    offs[1:] = torch.tensor(counts, dtype=torch.int32).cumsum(0)
    kv_off = offs.to(dev)
    q = torch.randn(B * Q, hs, generator=g).to(device=dev, dtype=dt)
    kv = torch.randn(sum(counts), 2 * hs, generator=g).to(device=dev, dtype=dt)
    oc = ops.cross_attention(q, kv[:, :hs], kv[:, hs:], Hq, Dq, 1.0 / math.sqrt(Dq), Q, kv_off, B, max(counts))
    doc = torch.randn(B * Q, hs, generator=g).to(device=dev, dtype=dt)
    cross_bwd = lambda: ops.mha_bwd(q, kv[:, :hs], kv[:, hs:], oc, doc, Hq, Dq, 1.0 / math.sqrt(Dq), Q, kv_off, B, max(counts))
    t_self = _time(self_bwd, a.kernel_reps)
    t_fwd = _time(self_fwd, a.kernel_reps)
    t_cross = _time(cross_bwd, a.kernel_reps)
    os.environ["SETOK_ATTN_BWD_GENERIC"] = "1"
    t_self_gen = _time(self_bwd, max(1, a.kernel_reps // 2))
    t_cross_gen = _time(cross_bwd, max(1, a.kernel_reps // 2))
    del os.environ["SETOK_ATTN_BWD_GENERIC"]
    flop = 10.0 * B * H * Q * Q * Dh
    med = lambda xs: sorted(xs)[len(xs) // 2]
    print(json.dumps(dict(
        workload="cfg3 decoder: reconstruction_loss forward + backward (bf16, tokens and decoder parameters trainable)",
        batch=B, tokens=sum(counts), steps=a.steps,
        ms_per_step=round(med([f + b for f, b in zip(fwd, bwd)]), 3), ms_forward=round(med(fwd), 3), ms_backward=round(med(bwd), 3),
        us_pixel_decoder_attention_bwd=round(t_self * 1e3, 1), us_pixel_decoder_attention_fwd=round(t_fwd * 1e3, 1),
        bwd_over_fwd=round(t_self / t_fwd, 2), us_pixel_decoder_attention_bwd_generic=round(t_self_gen * 1e3, 1),
        mfma_speedup_self=round(t_self_gen / t_self, 1), us_qformer_cross_attention_bwd=round(t_cross * 1e3, 1),
        us_qformer_cross_attention_bwd_generic=round(t_cross_gen * 1e3, 1), mfma_speedup_cross=round(t_cross_gen / t_cross, 1),
        attention_bwd_tflops=round(flop / (t_self * 1e-3) / 1e12, 2))))


if __name__ == "__main__":
    main()
