"""Per-request sampling in the continuous batcher at Vicuna-7B dims in bf16, two measurements in one process, arms alternated round by round
(tools/bench_paged_mxfp4.py's rule):

    python tools/bench_paged_sampling.py [--layers 32] [--rounds 7] [--reps 50] [--requests 64] [--rows 32] [--skip-workload]
                                         [--out profiles/paged_sampling_bench.json]

  (a) the selection launch at V = 32000, 32 rows: `sample_rows_each` against `sample_rows` under the same parameters (T = 0.8, top_k = 50,
      top_p = 0.9 and T = 0.8 alone) - the scalar launch is the kernel this one was made from -, and against `argmax_rows` with every row greedy
      and with every other row greedy.  Each arm's median and spread over the rounds; "the same" means inside the two arms' own spread.
  (b) the seeded ragged workload of tools/bench_paged.py - prompt lengths uniform in [32, 1024], max_new_tokens uniform in [16, 256] - through
      `ContinuousBatcher(rows=32)` in three arms: every request greedy, every request sampled (T = 0.8, top_k = 50, top_p = 0.9, its own stream),
      every other request sampled.  Time to drain and emitted tokens per second.
Random weights, prompts and logits; no eos.  Writes the JSON file and prints it as one line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import D, V, _llm, _spread, _time                      # noqa: E402  (the 7B dims and the timing helpers of the dense benchmark)

T_S, K_S, P_S = 0.8, 50, 0.9


def _selection(a, g, dev, dt):
    from setok_amd import ops
    rows = a.rows
    x = torch.randn(rows, V, generator=g, device=dev, dtype=torch.float32).mul_(3.0).to(dt)
    u = torch.rand(rows, generator=g, device=dev)
    out = torch.empty(rows, dtype=torch.int64, device=dev)
    full = lambda v, t: torch.full((rows,), v, dtype=t, device=dev)
    half = torch.arange(rows, device=dev) % 2 == 0                         # every other row greedy
    tkp = (full(T_S, torch.float32), full(K_S, torch.int32), full(P_S, torch.float32))
    t_only = (full(T_S, torch.float32), full(0, torch.int32), full(1.0, torch.float32))
    greedy = (full(0.0, torch.float32), full(0, torch.int32), full(1.0, torch.float32))
    mixed = (torch.where(half, greedy[0], tkp[0]), tkp[1], tkp[2])
    arms = dict(scalar_t_k_p=lambda: ops.sample_rows(x, u, T_S, K_S, P_S, out=out),
                each_t_k_p=lambda: ops.sample_rows_each(x, u, *tkp, out=out),
                scalar_t=lambda: ops.sample_rows(x, u, T_S, 0, 1.0, out=out),
                each_t=lambda: ops.sample_rows_each(x, u, *t_only, out=out),
                argmax=lambda: ops.argmax_rows(x, out=out),
                each_all_greedy=lambda: ops.sample_rows_each(x, u, *greedy, out=out),
                each_half_greedy=lambda: ops.sample_rows_each(x, u, *mixed, out=out))
    same = bool(torch.equal(ops.sample_rows_each(x, u, *tkp), ops.sample_rows(x, u, T_S, K_S, P_S)) and
                torch.equal(ops.sample_rows_each(x, u, *t_only), ops.sample_rows(x, u, T_S, 0, 1.0)) and
                torch.equal(ops.sample_rows_each(x, u, *greedy), ops.argmax_rows(x)))
    us = {name: [] for name in arms}
    for fn in arms.values():
        _time(fn, 5)                                                       # warm-up
    for _ in range(a.rounds):
        for name, fn in arms.items():
            us[name].append(1e3 * _time(fn, a.reps))
    r = {name: dict(us=_spread(xs)) for name, xs in us.items()}
    spread = lambda *names: round(max(r[n]["us"]["max"] - r[n]["us"]["min"] for n in names), 4)
    for each, base in (("each_t_k_p", "scalar_t_k_p"), ("each_t", "scalar_t"), ("each_all_greedy", "argmax"), ("each_half_greedy", "argmax")):
        diff = r[each]["us"]["median"] - r[base]["us"]["median"]
        r[f"{each}_minus_{base}_us"] = round(diff, 4)
        r[f"{each}_vs_{base}_largest_spread_us"] = spread(each, base)
        r[f"{each}_differs_from_{base}_beyond_spread"] = bool(abs(diff) > spread(each, base))
    r["bit_identical_outputs"] = same
    return dict(shape=dict(rows=rows, V=V, dtype="bf16"), parameters=dict(temperature=T_S, top_k=K_S, top_p=P_S), rounds=a.rounds, reps=a.reps,
                timing="device events around `reps` back-to-back launches, per launch", **r)


def _workload(a, g, dev, dt):
    from setok_amd import ops
    from setok_amd.generation import ContinuousBatcher, Sampler
    llm = _llm(a.layers, g, dev, dt)
    gen = torch.Generator().manual_seed(a.seed)
    T = torch.randint(32, 1025, (a.requests,), generator=gen).tolist()
    N = torch.randint(16, 257, (a.requests,), generator=gen).tolist()
    xs = [torch.randn(t, D, generator=g, device=dev, dtype=dt) for t in T]
    streams = [torch.rand(n, 1, generator=torch.Generator().manual_seed(a.seed + 1 + i)).to(dev) for i, n in enumerate(N)]
    per_seq = (1024 + 256 + ops.KV_PAGE - 1) // ops.KV_PAGE
    num_pages = a.rows * per_seq

    def drain(sampled):
        b = ContinuousBatcher(llm, a.rows, num_pages, max_pages_per_seq=per_seq)
        calls = dict(each=0, argmax=0)
        each, argmax = ops.sample_rows_each, ops.argmax_rows

        def count(name, fn):
            def counted(x, *args, **kw):
                calls[name] += x.shape[0] == a.rows                        # a decode step's selection; an admission's has one row
                return fn(x, *args, **kw)
            return counted
        ops.sample_rows_each, ops.argmax_rows = count("each", each), count("argmax", argmax)
        try:
            reqs = [(x, n, None, Sampler(T_S, K_S, P_S, u=streams[i]) if sampled(i) else None) for i, (x, n) in enumerate(zip(xs, N))]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = b.run(reqs)
            torch.cuda.synchronize()
            dt_s = time.perf_counter() - t0
        finally:
            ops.sample_rows_each, ops.argmax_rows = each, argmax
        assert [o.numel() for o in outs] == N and not b.errors
        return dt_s, dict(steps=b.stats["steps"], occupancy=round(b.occupancy, 4), steps_selected_by_sample_rows_each=calls["each"],
                          steps_selected_by_argmax_rows=calls["argmax"])

    arms = dict(all_greedy=lambda: drain(lambda i: False), all_sampled=lambda: drain(lambda i: True), half_sampled=lambda: drain(lambda i: i % 2 == 0))
    for fn in arms.values():
        fn()                                                               # warm-up: every arm once (allocator, first launches)
    runs, info = {name: [] for name in arms}, {}
    for _ in range(a.workload_rounds):
        for name, fn in arms.items():
            s, info[name] = fn()
            runs[name].append(s)
    r = {}
    for name, ts in runs.items():
        sp = _spread(ts)
        r[name] = dict(drain_s=sp, tokens_per_s=round(sum(N) / sp["median"], 1), **info[name])
    assert r["all_greedy"]["steps_selected_by_sample_rows_each"] == 0      # the all-greedy arm makes the launches it made before
    r["largest_drain_spread_s"] = round(max(x["drain_s"]["max"] - x["drain_s"]["min"] for x in r.values()), 4)
    for name in ("all_sampled", "half_sampled"):
        r[f"{name}_over_all_greedy_tokens_per_s"] = round(r[name]["tokens_per_s"] / r["all_greedy"]["tokens_per_s"], 4)
    return dict(requests=a.requests, rows=a.rows, layers=a.layers, dtype="bf16", seed=a.seed, prompt_tokens=sum(T), emitted_tokens=sum(N),
                num_pages=num_pages, rounds=a.workload_rounds, sampler=dict(temperature=T_S, top_k=K_S, top_p=P_S), **r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workload-rounds", type=int, default=3)
    ap.add_argument("--skip-workload", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_sampling_bench.json"))
    a = ap.parse_args()
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        run = dict(device=torch.cuda.get_device_name(0), selection_launch=_selection(a, g, dev, dt))
        if not a.skip_workload:
            run["ragged_workload"] = _workload(a, g, dev, dt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(run, f, indent=1)
    print(json.dumps(run))


if __name__ == "__main__":
    main()
