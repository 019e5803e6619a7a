"""Sampled token selection (setok_sample_rows) against what it replaces and what it would otherwise cost, on the GPU.

    python tools/bench_sample.py [--reps 200] [--rounds 3] [--out profiles/sample_bench.json] [--no-step] [--layers 32]

Per (B, V) in (1, 32000), (8, 32000), (32, 32000), (32, 128256), bf16 logits, in microseconds per call:
  sample_rows          filters off, and with top_k = 50 + top_p = 0.9 (T = 0.8)
  argmax_rows          the greedy selection at the same shape: what the parent's decode step pays
  torch composition    the same rule out of torch ops on the device: fp32 cast, division, sort, softmax, cumsum, the two thresholds, the inverse CDF
Each number is HIP events around `reps` back-to-back calls after a warm-up, the median of `rounds` rounds taken alternately over the variants; beside
it the host's enqueue time per call (a call the host cannot enqueue faster than the device runs it is launch-bound, and the event time is then the
enqueue rate, not the kernel's).  The tool also checks, on the timed inputs, that the torch composition and the kernel draw the same tokens.

Decode step (unless --no-step): lm_head + selection + embedding + `LlamaModel.decode_step` at the cfg5 dims (Vicuna-7B, bf16, B = 32, cache of 552
slots), greedy against a Sampler drawing its uniforms with torch.rand, alternating.  The difference is the selection kernel's time plus the two
launches the sampler adds (torch.rand, the clamp of -1)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 32000), (8, 32000), (32, 32000), (32, 128256))
T, TOP_K, TOP_P = 0.8, 50, 0.9


def torch_sample(logits, u, temperature, top_k, top_p):
    """The rule of include/setok_hip.h ("Sampling") out of torch ops: float weights in place of the fixed-point ones."""
    s = logits.float() / temperature
    V = s.shape[1]
    srt, idx = torch.sort(s, dim=1, descending=True)
    if 0 < top_k < V:
        srt = srt.masked_fill(srt < srt[:, top_k - 1:top_k], float("-inf"))
    p = torch.softmax(srt, dim=1)
    if top_p < 1.0:
        above = p.cumsum(1) - p
        p = p.masked_fill(above >= top_p, 0.0)                        # (a run of equal scores at the cut is split here, kept together by the kernel)
        p = p / p.sum(1, keepdim=True)
    back = torch.zeros_like(p).scatter_(1, idx, p)                    # index order
    cdf = back.cumsum(1)
    target = (u.clamp(0.0, 1.0 - 2.0 ** -24) * cdf[:, -1]).unsqueeze(1)
    return (cdf <= target).sum(1).clamp_max(V - 1)


def timed(fn, reps):
    """(device us per call by events, host enqueue us per call)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    t1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps, (t1 - t0) * 1e6 / reps


def bench_shape(B, V, reps, rounds, dev):
    from setok_amd import ops
    g = torch.Generator(device=dev).manual_seed(B * 1000003 + V)
    logits = (torch.randn(B, V, generator=g, device=dev) * 3.0).to(torch.bfloat16)
    u = torch.rand(B, generator=g, device=dev)
    out = torch.empty(B, dtype=torch.int64, device=dev)
    variants = {
        "sample_rows_no_filter": lambda: ops.sample_rows(logits, u, T, 0, 1.0, out=out),
        "sample_rows_top_k50_top_p0.9": lambda: ops.sample_rows(logits, u, T, TOP_K, TOP_P, out=out),
        "argmax_rows": lambda: ops.argmax_rows(logits, out=out),
        "torch_no_filter": lambda: torch_sample(logits, u, T, 0, 1.0),
        "torch_top_k50_top_p0.9": lambda: torch_sample(logits, u, T, TOP_K, TOP_P),
    }
    same = {}
    for tag, k, p in (("no_filter", 0, 1.0), ("top_k50_top_p0.9", TOP_K, TOP_P)):
        a, b = ops.sample_rows(logits, u, T, k, p), torch_sample(logits, u, T, k, p)
        # not all of B where bf16 rows tie at the top-p cut (the composition splits the run of equal scores, the kernel keeps it together), or where
        # a u lies within the float prefix sums' error of an interval end
        same[tag] = f"{int((a == b).sum())} of {B}"
    for fn in variants.values():                                      # warm-up: code objects, the allocator's blocks
        for _ in range(3):
            fn()
    dev_us = {k: [] for k in variants}
    host_us = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            n = reps if not k.startswith("torch") else max(10, reps // 10)
            d, h = timed(fn, n)
            dev_us[k].append(d); host_us[k].append(h)
    res = {k: dict(us=round(statistics.median(dev_us[k]), 2), us_min=round(min(dev_us[k]), 2), us_max=round(max(dev_us[k]), 2),
                   host_enqueue_us=round(statistics.median(host_us[k]), 2)) for k in variants}
    res["tokens_equal_to_the_torch_composition"] = same
    res["logit_bytes"] = B * V * 2
    return res


def bench_step(layers, reps, rounds, dev):
    """ms per decode step at the cfg5 dims, B = 32: greedy against a sampler, alternating."""
    import bench_generate as BG
    from setok_amd import ops
    from setok_amd.generation import Sampler
    B, Tp = 32, 552
    dt = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    llm = BG._llm(layers, g, dev, dt)
    w_lm, w_e = llm.lm_head.weight.detach(), llm.model.embed_tokens.weight.detach()
    c = BG._filled_cache(llm, B, Tp + 8, Tp, g)
    h = torch.randn(B, BG.D, generator=g, device=dev, dtype=torch.float32).to(dt)
    smp = Sampler(temperature=T, top_k=TOP_K, top_p=TOP_P, generator=torch.Generator(device=dev).manual_seed(1))

    def step(select):
        BG._set_len(c, Tp)
        tok = select(ops.linear(h, w_lm))
        e = ops.splice_rows(tok.to(torch.int32).reshape(-1, 1), w_e, None)
        return llm.model.decode_step(e.reshape(-1, BG.D), c)

    variants = {"greedy": lambda: step(ops.argmax_rows), "sampler_top_k50_top_p0.9": lambda: step(lambda lg: smp.select(lg, 0).clamp_min(0))}
    for fn in variants.values():
        for _ in range(2):
            fn()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(timed(fn, reps)[0] / 1e3)
    res = {k: dict(ms_per_step=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4)) for k, v in ms.items()}
    res["difference_us"] = round((res["sampler_top_k50_top_p0.9"]["ms_per_step"] - res["greedy"]["ms_per_step"]) * 1e3, 1)
    res["shape"] = dict(B=B, cache_len=Tp + 1, layers=layers, dtype="bf16", vocab=BG.V)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--step-reps", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample.py measures on the GPU: no device found (there is no CPU fallback)")
    dev = "cuda:0"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from setok_amd import _lib
    run = dict(workload="token selection for a decode step, bf16 logits: setok_sample_rows against setok_argmax_rows and the same rule out of torch ops",
               device=_lib.device_info()[0], reps=a.reps, rounds=a.rounds, temperature=T, shapes={})
    for B, V in SHAPES:
        run["shapes"][f"B{B}_V{V}"] = bench_shape(B, V, a.reps, a.rounds, dev)
    run["sample_rows_faster_than_torch_at_every_shape"] = all(
        r["sample_rows_no_filter"]["us"] < r["torch_no_filter"]["us"] and r["sample_rows_top_k50_top_p0.9"]["us"] < r["torch_top_k50_top_p0.9"]["us"]
        for r in run["shapes"].values())
    if not a.no_step:
        run["decode_step"] = bench_step(a.layers, a.step_reps, a.rounds, dev)
    line = json.dumps(run)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
