"""MXFP4 pages at Vicuna-7B dims in bf16, three measurements in one process, arms alternated round by round (tools/bench_paged.py's method):

    python tools/bench_paged_mxfp4.py [--layers 32] [--rounds 5] [--reps 5] [--requests 64] [--rows 32] [--skip-workload] [--skip-prefix]
                                      [--out profiles/paged_mxfp4_bench.json]

  (a) the decode-attention launch pair (chunks + merge) summed over every layer's cache at B = 32 and 553 / 752 uniform slots, three arms: MXFP4
      pools read through a shuffled block table, the dense MXFP4 cache with the same rows, and native pools through the same table.  Each arm's
      median and spread over the rounds.
  (b) the seeded ragged workload of tools/bench_paged.py - prompt lengths uniform in [32, 1024], max_new_tokens uniform in [16, 256] - through
      `ContinuousBatcher(rows=32)` on native pages and on MXFP4 pages (`cache=PagedKVCache.for_model(..., kv_format="mxfp4")`): time to drain,
      emitted tokens per second, pages and bytes in use at the high-water mark.
  (c) the shared-prefix workload of tools/bench_paged.py --prefix (a 600-row prefix, 512 shared slots) on both page formats: what an admission
      costs when the extend attention behind the prefix is the functional wave-per-chunk kernel (MXFP4) instead of the MFMA kernel (native).
Random weights, prompts and cache rows; no eos.  Writes the JSON file and prints it as one line."""
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

from bench_generate import D, DH, H, _llm, _spread, _time                  # noqa: E402  (the 7B dims and the timing helpers of the dense benchmark)


def _kernel_pair(a, g, dev, dt):
    from setok_amd import ops
    B, out, scale = 32, {}, DH ** -0.5
    for length in (553, 752):
        pages_per = (length + ops.KV_PAGE - 1) // ops.KV_PAGE
        cap, n_pages = pages_per * ops.KV_PAGE, B * pages_per
        perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(length)).to(torch.int32).reshape(B, pages_per)
        table, idx = perm.to(dev), perm.reshape(-1).long().to(dev)
        as_pages = lambda t: t.reshape(B, H, pages_per, ops.KV_PAGE, t.shape[-1]).transpose(1, 2).reshape(n_pages, H, ops.KV_PAGE, t.shape[-1])
        rnd8 = lambda cols, lo, hi: torch.randint(lo, hi, (B, H, cap, cols), generator=g, device=dev, dtype=torch.int32).to(torch.uint8)
        dense4, pools4, pools = [], [], []
        for _ in range(a.layers):
            d = [rnd8(DH // 2, 0, 256), rnd8(DH // 32, 122, 128), rnd8(DH // 2, 0, 256), rnd8(DH // 32, 122, 128)]       # k_q, k_s, v_q, v_s
            p = []
            for t in d:
                pool = torch.empty(n_pages, H, ops.KV_PAGE, t.shape[-1], device=dev, dtype=torch.uint8)
                pool[idx] = as_pages(t)
                p.append(pool)
            dense4.append(d)
            pools4.append(p)
            pools.append((torch.randn(n_pages, H, ops.KV_PAGE, DH, generator=g, device=dev, dtype=dt),
                          torch.randn(n_pages, H, ops.KV_PAGE, DH, generator=g, device=dev, dtype=dt)))
        q = torch.randn(B, 3 * H * DH, generator=g, device=dev, dtype=dt)
        mask = torch.ones(B, cap, dtype=torch.uint8, device=dev)
        lens = torch.full((B,), length, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.attention_decode_workspace(B, H, DH, cap), dtype=torch.float32, device=dev)
        o = torch.empty(B, H * DH, dtype=dt, device=dev)
        arms = dict(paged_mxfp4=lambda: [ops.attention_decode_paged_mxfp4kv(q, *p, table, lens, H, length, scale, ws=ws, out=o) for p in pools4],
                    dense_mxfp4=lambda: [ops.attention_decode_mxfp4kv(q, *d, mask, H, length, scale, ws=ws, out=o) for d in dense4],
                    paged_native=lambda: [ops.attention_decode_paged(q, kp, vp, table, lens, H, length, scale, ws=ws, out=o) for kp, vp in pools])
        same = torch.equal(ops.attention_decode_paged_mxfp4kv(q, *pools4[0], table, lens, H, length, scale),
                           ops.attention_decode_mxfp4kv(q, *dense4[0], mask, H, length, scale))
        ms = {name: [] for name in arms}
        for fn in arms.values():
            _time(fn, 2)                                                   # warm-up
        for _ in range(a.rounds):
            for name, fn in arms.items():
                ms[name].append(_time(fn, a.reps))
        row_bytes = dict(paged_mxfp4=DH // 2 + DH // 32, dense_mxfp4=DH // 2 + DH // 32, paged_native=DH * 2)
        r = {name: dict(ms=_spread(xs), tb_per_s=round(2.0 * a.layers * B * H * length * row_bytes[name] / (sorted(xs)[len(xs) // 2] * 1e-3) / 1e12, 3))
             for name, xs in ms.items()}
        pm, dm, pn = r["paged_mxfp4"]["ms"], r["dense_mxfp4"]["ms"], r["paged_native"]["ms"]
        r["paged_mxfp4_over_dense_mxfp4"] = round(pm["median"] / dm["median"], 4)
        r["paged_mxfp4_minus_dense_mxfp4_ms"] = round(pm["median"] - dm["median"], 4)
        r["paged_native_over_paged_mxfp4"] = round(pn["median"] / pm["median"], 4)
        r["largest_spread_ms"] = round(max(x["max"] - x["min"] for x in (pm, dm, pn)), 4)
        r["paged_mxfp4_slower_than_dense_beyond_spread"] = bool(pm["median"] - dm["median"] > r["largest_spread_ms"])
        r["bit_identical_outputs"] = bool(same)
        out[f"len{length}"] = r
        del dense4, pools4, pools
        torch.cuda.empty_cache()
    return dict(shape=dict(B=B, H=H, Hkv=H, Dh=DH, layers=a.layers, dtype="bf16"), launches_of_the_pair=2, **out)


def _batcher(llm, a, num_pages, per_seq, fmt):
    from setok_amd.generation import ContinuousBatcher, PagedKVCache
    return ContinuousBatcher(llm, a.rows, cache=PagedKVCache.for_model(llm.model, a.rows, num_pages, per_seq, kv_format=fmt))


def _alternate(arms, rounds, useful):
    for fn in arms.values():
        fn()                                                               # warm-up: every arm once (allocator, first launches)
    runs, info = {name: [] for name in arms}, {}
    for _ in range(rounds):
        for name, fn in arms.items():
            s, info[name] = fn()
            runs[name].append(s)
    r = {}
    for name, xs in runs.items():
        sp = _spread(xs)
        r[name] = dict(drain_s=sp, tokens_per_s=round(useful / sp["median"], 1), **info[name])
    return r


def _workload(a, llm, g, dev, dt):
    from setok_amd import ops
    gen = torch.Generator().manual_seed(a.seed)
    T = torch.randint(32, 1025, (a.requests,), generator=gen).tolist()
    N = torch.randint(16, 257, (a.requests,), generator=gen).tolist()
    xs = [torch.randn(t, D, generator=g, device=dev, dtype=dt) for t in T]
    per_seq = (1024 + 256 + ops.KV_PAGE - 1) // ops.KV_PAGE
    num_pages = a.rows * per_seq

    def drain(fmt):
        b = _batcher(llm, a, num_pages, per_seq, fmt)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = b.run(list(zip(xs, N)))
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        assert [o.numel() for o in outs] == N
        return dt_s, dict(steps=b.stats["steps"], occupancy=round(b.occupancy, 4), pages_high_water=b.stats["pages_high_water"],
                          page_bytes=b.cache.page_nbytes, cache_bytes=b.stats["pages_high_water"] * b.cache.page_nbytes, pool_bytes=b.cache.nbytes(),
                          page_waits=b.stats["page_waits"])

    r = _alternate(dict(native_pages=lambda: drain("native"), mxfp4_pages=lambda: drain("mxfp4")), a.workload_rounds, sum(N))
    n, m = r["native_pages"], r["mxfp4_pages"]
    r["mxfp4_over_native_tokens_per_s"] = round(m["tokens_per_s"] / n["tokens_per_s"], 3)
    r["mxfp4_over_native_cache_bytes"] = round(m["cache_bytes"] / n["cache_bytes"], 4)
    r["largest_drain_spread_s"] = round(max(x["drain_s"]["max"] - x["drain_s"]["min"] for x in (n, m)), 4)
    return dict(requests=a.requests, rows=a.rows, layers=a.layers, dtype="bf16", seed=a.seed, prompt_tokens=sum(T), emitted_tokens=sum(N),
                num_pages=num_pages, rounds=a.workload_rounds, **r)


def _prefix_workload(a, llm, g, dev, dt):
    from setok_amd import ops
    gen = torch.Generator().manual_seed(a.seed)
    P = 600
    S = torch.randint(16, 129, (a.requests,), generator=gen).tolist()
    N = torch.randint(16, 129, (a.requests,), generator=gen).tolist()
    prefix = torch.randn(P, D, generator=g, device=dev, dtype=dt)
    rest = [torch.randn(s, D, generator=g, device=dev, dtype=dt) for s in S]
    per_seq = (P + 128 + 128 + ops.KV_PAGE - 1) // ops.KV_PAGE
    num_pages = a.rows * per_seq + P // ops.KV_PAGE

    def drain(fmt):
        b = _batcher(llm, a, num_pages, per_seq, fmt)
        admit, spent, calls = b._admit, [0.0], [0]                         # (tools/bench_paged.py's admission clock: `step()` admits through `_admit`)

        def timed_admit():
            torch.cuda.synchronize()
            t = time.perf_counter()
            fresh = admit()
            torch.cuda.synchronize()
            spent[0] += time.perf_counter() - t
            calls[0] += 1
            return fresh
        b._admit = timed_admit
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = b.register_prefix(prefix)
        outs = b.run([(x, n, h) for x, n in zip(rest, N)])
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        assert [o.numel() for o in outs] == N
        assert calls[0] >= b.stats["steps"] > 0 and b.stats["admitted"] == a.requests, "step() no longer admits through _admit: the admission clock saw nothing"
        return dt_s, dict(steps=b.stats["steps"], pages_high_water=b.stats["pages_high_water"], cache_bytes=b.stats["pages_high_water"] * b.cache.page_nbytes,
                          admission_ms=round(1e3 * spent[0] / b.stats["admitted"], 3), prefix_stats=dict(b.prefix_stats))

    r = _alternate(dict(native_pages=lambda: drain("native"), mxfp4_pages=lambda: drain("mxfp4")), a.workload_rounds, sum(N))
    n, m = r["native_pages"], r["mxfp4_pages"]
    r["mxfp4_over_native_admission_ms"] = round(m["admission_ms"] / n["admission_ms"], 3)
    r["mxfp4_over_native_tokens_per_s"] = round(m["tokens_per_s"] / n["tokens_per_s"], 3)
    r["largest_drain_spread_s"] = round(max(x["drain_s"]["max"] - x["drain_s"]["min"] for x in (n, m)), 4)
    return dict(requests=a.requests, rows=a.rows, layers=a.layers, dtype="bf16", seed=a.seed, prefix_rows=P, shared_slots=ops.KV_PAGE * (P // ops.KV_PAGE),
                remainder_rows=dict(min=min(S), max=max(S), total=sum(S)), emitted_tokens=sum(N), num_pages=num_pages, rounds=a.workload_rounds, **r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--requests", type=int, default=64)
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--workload-rounds", type=int, default=2)
    ap.add_argument("--skip-workload", action="store_true")
    ap.add_argument("--skip-prefix", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_mxfp4_bench.json"))
    a = ap.parse_args()
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    with torch.no_grad():
        run = dict(device=torch.cuda.get_device_name(0), decode_attention_pair=_kernel_pair(a, g, dev, dt))
        if not (a.skip_workload and a.skip_prefix):
            llm = _llm(a.layers, g, dev, dt)
            if not a.skip_workload:
                run["ragged_workload"] = _workload(a, llm, g, dev, dt)
            if not a.skip_prefix:
                run["shared_prefix_workload"] = _prefix_workload(a, llm, g, dev, dt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(run, f, indent=1)
    print(json.dumps(run))


if __name__ == "__main__":
    main()
