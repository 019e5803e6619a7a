"""LoRA fine-tuning of the Llama stack on an MI355X: the skinny GEMM against `setok_linear` on the same operands, and the frozen forward +
backward (stage 2, what tools/bench_llama_bwd.py times) against the LoRA forward + backward at the same shape.

    python tools/bench_lora.py [--layers 32] [--batch 32] [--seq 552] [--steps 3] [--warmup 1] [--rounds 7] [--kernel-only] [--out profiles/lora_bench.json]

Kernel part (bf16): N = 64 and 128 (the rank as the output width), K = 4096 and 11008, M = 552, 4416 and 17664.  The two kernels alternate within
a round, every round times `--reps` back-to-back calls of each after a warm-up call, and the JSON keeps the median over the rounds with the
smallest and largest round (the spread).  Both write a bf16 (M, N) result from the same operands; their largest difference is reported.
Model part: Vicuna-7B dims, bf16, r = 128 on all seven projections (the reference's scripts/finetune.sh), the largest batch of
bench_llama_bwd.py's shape that fits; the time of `transpose` + `linear_tn` (the dA / dB GEMMs) inside one backward pass by events around those
calls; peak allocations.  Prints one JSON line and, with --out, writes it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _round(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3                         # microseconds per call


def _stats(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 1), min=round(xs[0], 1), max=round(xs[-1], 1))


def kernel_part(a, ops):
    dev, dt = "cuda:0", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for K in (4096, 11008):
        for N in (64, 128):
            w = (torch.randn(N, K, generator=g, device=dev) * 0.02).to(dt)
            for M in (552, 4416, 17664):
                x = torch.randn(M, K, generator=g, device=dev).to(dt)
                c1, c2 = torch.empty(M, N, dtype=dt, device=dev), torch.empty(M, N, dtype=dt, device=dev)
                skinny = lambda: ops.linear_skinny(x, w, out=c1)
                tiled = lambda: ops.linear(x, w, out=c2)
                ts, tl = [], []
                for _ in range(a.rounds):                            # alternate: other work shares the machine
                    ts.append(_round(skinny, a.reps))
                    tl.append(_round(tiled, a.reps))
                diff = float((c1.float() - c2.float()).abs().max() / c2.float().abs().max())
                s, l = _stats(ts), _stats(tl)
                out.append(dict(M=M, N=N, K=K, us_linear_skinny=s, us_setok_linear=l, speedup=round(l["median"] / s["median"], 2),
                                skinny_wins=bool(s["max"] < l["min"]), max_rel_difference=diff,
                                workspace_mb=round(ops.linear_skinny_workspace(M, N, K) * 4 / 2 ** 20, 1)))
                print(out[-1], file=sys.stderr)
    return out


def model_part(a, ops):
    from setok_amd import llama_train
    from setok_amd.llama import SetokimLlamaPrefill
    dev, dt = "cuda:0", torch.bfloat16
    T, D, H, Fd, V = a.seq, 4096, 32, 11008, 32000
    g = torch.Generator(device=dev).manual_seed(0)
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
    med = lambda xs: sorted(xs)[len(xs) // 2]

    def steps(B, tn_events=None):
        am = torch.ones(B, T, dtype=torch.bool, device=dev)
        for b in range(1, B, 3):
            am[b, T - 40 - b:] = False
        labels = torch.randint(0, V, (B, T), generator=g, device=dev)
        labels[:, :64] = -100
        emb = torch.randn(B, T, D, generator=g, device=dev).to(dt)
        kw = dict(attention_mask=am, labels=labels, return_loss=True)
        fwd, bwd = [], []
        torch.cuda.reset_peak_memory_stats()
        for i in range(a.warmup + a.steps):
            llm.zero_grad(set_to_none=True)
            xe = emb.clone().requires_grad_(True)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            if tn_events is not None:
                tn_events.clear()
            e[0].record()
            _, _, _, loss = llm(inputs_embeds=xe, **kw)
            e[1].record()
            loss.backward()
            e[2].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                fwd.append(e[0].elapsed_time(e[1])); bwd.append(e[1].elapsed_time(e[2]))
        assert bool(torch.isfinite(xe.grad.float()).all())
        both = [f + b for f, b in zip(fwd, bwd)]
        return dict(ms_forward=round(med(fwd), 2), ms_backward=round(med(bwd), 2), ms_forward_backward=round(med(both), 2),
                    ms_forward_backward_min=round(min(both), 2), ms_forward_backward_max=round(max(both), 2),
                    peak_bytes=torch.cuda.max_memory_allocated())

    res = dict(layers=a.layers, seq=T, r=128, lora_alpha=256, targets="all seven", steps=a.steps)
    frozen = {}
    B = a.batch
    while True:                                                      # the largest batch that fits with the adapters and the dW scratch
        try:
            frozen[B] = steps(B)
            if llm.model.lora is None:
                llm.add_lora_(128, 256)
                for p in llm.model.lora.parameters():                # a non-zero B: every GEMM of the backward pass does real work
                    p.data.normal_(0.0, 0.02, generator=g)
            events = []
            real = llama_train._tn

            def timed(*args, **kwargs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r = real(*args, **kwargs)
                e1.record()
                events.append((e0, e1))
                return r
            plain = steps(B)
            llama_train._tn = timed
            try:
                marked = steps(B, events)
                tn_ms = sum(e0.elapsed_time(e1) for e0, e1 in events)
            finally:
                llama_train._tn = real
            res.update(batch=B, rows=B * T, frozen=frozen[B], lora=plain,
                       lora_over_frozen=round(plain["ms_forward_backward"] / frozen[B]["ms_forward_backward"], 3),
                       ms_transpose_linear_tn_per_backward=round(tn_ms, 2), transpose_linear_tn_calls=len(events),
                       transpose_linear_tn_share_of_lora_backward=round(tn_ms / marked["ms_backward"], 4))
            return res
        except torch.cuda.OutOfMemoryError:
            res.setdefault("out_of_memory_at_batch", []).append(B)
            if llm.model.lora is not None:
                llm.model.lora = None
            torch.cuda.empty_cache()
            B //= 2
            if B < 1:
                raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seq", type=int, default=552)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lora.py measures on the GPU"
    from setok_amd import ops
    from setok_amd import _lib
    name, cus = _lib.device_info()
    res = dict(workload="LoRA on the Llama stack, bf16: linear_skinny against setok_linear; frozen against LoRA forward + backward at Vicuna-7B dims",
               device=name, compute_units=cus, kslice=ops.skinny_kslice(), rounds=a.rounds, reps=a.reps, kernel=kernel_part(a, ops))
    if not a.kernel_only:
        res["model"] = model_part(a, ops)
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
