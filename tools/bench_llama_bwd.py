"""Forward and forward + backward through the frozen LLM at the cfg5 shape (Vicuna-7B dims, bf16, B = 32 sequences of 512 prompt tokens + image
tokens): SetokimLlamaPrefill(inputs_embeds, labels, return_loss=True) under no_grad, and the same call with inputs_embeds requiring a gradient
followed by loss.backward() — the LLM's share of a stage-2 step (the dX chain only: no weight gradient is formed).

    python tools/bench_llama_bwd.py [--layers 32] [--batch 32] [--seq 552] [--steps 3] [--warmup 1] [--attention-only]

Prints one JSON line: ms per forward, ms per forward + backward (forward and backward split by events), the causal attention backward and its
forward per layer (the MFMA pair, and the generic wave-per-row pair via SETOK_LLAMA_ATTN_BWD_GENERIC=1 in the same process), each of the five
new kernels per call and as a share of the backward pass, the per-step cost of transposing the frozen weights, the bytes the saved activations
hold and the peak allocation.  --attention-only: just the attention kernels at the layer's shape (the program a counter run is pointed at)."""
from __future__ import annotations

import argparse
import json
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
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=552)            # 512 prompt tokens - 1 placeholder + ~41 image tokens
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--attention-only", action="store_true")
    a = ap.parse_args()
    from setok_amd import ops
    from setok_amd.llama import SetokimLlamaPrefill
    from setok_amd import llama_train

    dev, dt = "cuda:0", torch.bfloat16
    B, T, D, H, Dh, Fd, V = a.batch, a.seq, 4096, 32, 128, 11008, 32000
    rows = B * T
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float32).to(dt)
    am = torch.ones(B, T, dtype=torch.bool, device=dev)
    for b in range(1, B, 3):
        am[b, T - 40 - b:] = False                                 # ragged right padding, as the full-size tests build it
    km = am.to(torch.uint8).reshape(-1).contiguous()

    # ---- the attention kernels at a layer's shape ----
    qkv, do = rnd(rows, 3 * D), rnd(rows, D)
    o = ops.attention_causal(qkv, km, B, T, H, Dh, Dh ** -0.5)
    attn_fwd = lambda: ops.attention_causal(qkv, km, B, T, H, Dh, Dh ** -0.5)
    attn_bwd = lambda: ops.attention_causal_bwd(qkv, km, o, do, B, T, H, Dh, Dh ** -0.5)
    t_af, t_ab = _time(attn_fwd, a.kernel_reps), _time(attn_bwd, a.kernel_reps)
    if a.attention_only:
        print(json.dumps(dict(us_attention_fwd=round(t_af * 1e3, 1), us_attention_bwd=round(t_ab * 1e3, 1))))
        return
    os.environ["SETOK_LLAMA_ATTN_BWD_GENERIC"] = "1"
    t_ab_gen = _time(attn_bwd, 1)
    del os.environ["SETOK_LLAMA_ATTN_BWD_GENERIC"]
    flop_bwd = 10.0 * B * H * T * T * Dh / 2                       # five T x T x Dh products over the causal half

    # ---- the other new kernels at the step's shapes ----
    x, dy, w = rnd(rows, D), rnd(rows, D), torch.ones(D, device=dev)
    pos = torch.arange(T, device=dev)[None].expand(B, T).reshape(-1).contiguous()
    pre, dg = rnd(rows, 2 * Fd), rnd(rows, Fd)
    t_norm = _time(lambda: ops.rmsnorm_bwd(x, w, dy, 1e-5, dres=x), a.kernel_reps)
    t_rope = _time(lambda: ops.rope_bwd_(qkv, pos, H, Dh, 10000.0), a.kernel_reps)
    t_swi = _time(lambda: ops.swiglu_pairs_bwd(pre, dg, out=pre), a.kernel_reps)
    del pre, dg
    logits = rnd(rows, V).reshape(B, T, V)
    labels = torch.randint(0, V, (B, T), generator=g, device=dev)
    labels[:, :64] = -100
    lo = ops.lm_loss(logits, labels, am)
    dl = torch.empty_like(logits)
    t_loss = _time(lambda: ops.lm_loss_bwd(logits, labels, am, lo, out=dl), a.kernel_reps)
    del logits, dl, qkv, do, o

    # ---- the model ----
    cfg = dict(vocab_size=V, hidden_size=D, intermediate_size=Fd, num_hidden_layers=a.layers, num_attention_heads=H, num_key_value_heads=H,
               rms_norm_eps=1e-5, rope_theta=10000.0)
    with torch.device(dev):
        llm = SetokimLlamaPrefill(cfg).to(dt)
    for p in llm.parameters():
        if p.dim() == 2:
            p.data.normal_(0.0, 0.02, generator=g)
        else:
            p.data.fill_(1.0)
    llm.eval().requires_grad_(False)
    pk = llm.model._pack()
    L0 = pk["layers"][0]
    t_transpose = _time(lambda: [ops.transpose(L0[k]) for k in ("wqkv", "wo", "wgu", "wd")], a.kernel_reps) * a.layers
    emb = rnd(B, T, D)
    kw = dict(attention_mask=am, labels=labels, return_loss=True)
    with torch.no_grad():
        t_fwd = _time(lambda: llm(inputs_embeds=emb, **kw), a.steps)
    fwd, bwd, held = [], [], 0
    torch.cuda.reset_peak_memory_stats()
    for i in range(a.warmup + a.steps):
        xe = emb.clone().requires_grad_(True)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        _, _, _, loss = llm(inputs_embeds=xe, **kw)
        e[1].record()
        held = llama_train.saved_bytes(loss.grad_fn.saved)
        loss.backward()
        e[2].record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            fwd.append(e[0].elapsed_time(e[1])); bwd.append(e[1].elapsed_time(e[2]))
    assert xe.grad is not None and bool(torch.isfinite(xe.grad.float()).all())
    med = lambda xs: sorted(xs)[len(xs) // 2]
    t_b = med(bwd)
    share = lambda t, calls: round(t * calls / t_b, 4)
    print(json.dumps(dict(
        workload="cfg5 LLM: frozen Llama at Vicuna-7B dims, bf16; forward with the LM loss, and forward + loss.backward() to inputs_embeds",
        layers=a.layers, batch=B, seq=T, rows=rows, steps=a.steps,
        ms_forward_inference=round(t_fwd, 2), ms_forward_train=round(med(fwd), 2), ms_backward=round(t_b, 2),
        ms_forward_backward=round(med([f + b for f, b in zip(fwd, bwd)]), 2), backward_over_forward=round(t_b / t_fwd, 2),
        us_attention_fwd_per_layer=round(t_af * 1e3, 1), us_attention_bwd_per_layer=round(t_ab * 1e3, 1), attention_bwd_over_fwd=round(t_ab / t_af, 2),
        us_attention_bwd_generic_per_layer=round(t_ab_gen * 1e3, 1), mfma_speedup=round(t_ab_gen / t_ab, 1),
        attention_bwd_tflops=round(flop_bwd / (t_ab * 1e-3) / 1e12, 1),
        us_rmsnorm_bwd=round(t_norm * 1e3, 1), us_rope_bwd=round(t_rope * 1e3, 1), us_swiglu_pairs_bwd=round(t_swi * 1e3, 1), us_lm_loss_bwd=round(t_loss * 1e3, 1),
        share_of_backward=dict(attention_causal_bwd=share(t_ab, a.layers), rmsnorm_bwd=share(t_norm, 2 * a.layers + 1), rope_bwd=share(t_rope, a.layers),
                               swiglu_pairs_bwd=share(t_swi, a.layers), lm_loss_bwd=share(t_loss, 1), weight_transposes=share(t_transpose, 1)),
        ms_weight_transposes_per_step=round(t_transpose, 2),
        saved_activation_bytes=held, peak_bytes=torch.cuda.max_memory_allocated())))


if __name__ == "__main__":
    main()
