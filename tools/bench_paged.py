"""The paged KV cache and continuous batching at Vicuna-7B dims in bf16, two measurements in one process, arms alternated round by round:

    python tools/bench_paged.py [--layers 32] [--rounds 5] [--reps 5] [--requests 64] [--rows 32] [--skip-workload] [--out profiles/paged_bench.json]

  (a) what paging costs the kernel: the decode-attention launch pair (chunks + merge) summed over every layer's cache at B = 32 and 553 / 752
      uniform slots (the shapes of profiles/generate_bench.json), the dense cache against pools read through a shuffled block table.  Each arm's
      median and spread over the rounds; the paged pair does one table load and one length load per workgroup more.
  (b) what the feature is for: a seeded ragged workload - prompt lengths uniform in [32, 1024], max_new_tokens uniform in [16, 256] - through
      `ContinuousBatcher(rows=32)` against the same requests through the dense `generate` in static left-padded batches of `rows`, each run to its
      longest member.  Time to drain, emitted tokens per second (the tokens the requests asked for), occupancy, and cache bytes.
Random weights and prompts; no eos, so every request runs to its max_new_tokens in both arms.  Writes the JSON file and prints it as one line.

    python tools/bench_paged.py --prefix [--requests 64] [--rows 32] [--workload-rounds 2] [--prefix-out profiles/prefix_bench.json]

  (c) prefix sharing: requests behind one 600-row prefix (512 shared slots) with remainders of 16 - 128 rows, the prefix registered once against the
      same requests with their full prompts; time to drain, tokens per second, time per admission, pages at the high-water mark.  Recorded as
      the section `shared_prefix_workload` of profiles/prefix_bench.json, next to tools/bench_extend.py --only paged_pair's."""
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


def _kernel_cost(a, g, dev, dt):
    from setok_amd import ops
    B, out = 32, {}
    for length in (553, 752):
        cap = pages_per = (length + ops.KV_PAGE - 1) // ops.KV_PAGE
        cap *= ops.KV_PAGE
        n_pages = B * pages_per
        dense = [(torch.randn(B, H, cap, DH, generator=g, device=dev, dtype=dt), torch.randn(B, H, cap, DH, generator=g, device=dev, dtype=dt))
                 for _ in range(a.layers)]
        # the same keys / values as pages: sequence b's chunk p lies at a shuffled page
        perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(length)).to(torch.int32).reshape(B, pages_per)
        table = perm.to(dev)
        pools = []
        for k, v in dense:
            kp, vp = torch.empty(n_pages, H, ops.KV_PAGE, DH, device=dev, dtype=dt), torch.empty(n_pages, H, ops.KV_PAGE, DH, device=dev, dtype=dt)
            idx = perm.reshape(-1).long().to(dev)
            kp[idx] = k.reshape(B, H, pages_per, ops.KV_PAGE, DH).transpose(1, 2).reshape(n_pages, H, ops.KV_PAGE, DH)
            vp[idx] = v.reshape(B, H, pages_per, ops.KV_PAGE, DH).transpose(1, 2).reshape(n_pages, H, ops.KV_PAGE, DH)
            pools.append((kp, vp))
        q = torch.randn(B, 3 * H * DH, generator=g, device=dev, dtype=dt)
        mask = torch.ones(B, cap, dtype=torch.uint8, device=dev)
        lens = torch.full((B,), length, dtype=torch.int32, device=dev)
        ws = torch.empty(ops.attention_decode_workspace(B, H, DH, cap), dtype=torch.float32, device=dev)
        o = torch.empty(B, H * DH, dtype=dt, device=dev)
        arms = dict(dense=lambda: [ops.attention_decode(q, k, v, mask, H, length, DH ** -0.5, ws=ws, out=o) for k, v in dense],
                    paged=lambda: [ops.attention_decode_paged(q, kp, vp, table, lens, H, length, DH ** -0.5, ws=ws, out=o) for kp, vp in pools])
        same = all(torch.equal(ops.attention_decode(q, k, v, mask, H, length, DH ** -0.5), ops.attention_decode_paged(q, kp, vp, table, lens, H, length, DH ** -0.5))
                   for (k, v), (kp, vp) in zip(dense[:1], pools[:1]))
        ms = {name: [] for name in arms}
        for fn in arms.values():
            _time(fn, 2)                                                   # warm-up
        for _ in range(a.rounds):
            for name, fn in arms.items():
                ms[name].append(_time(fn, a.reps))
        live = 2.0 * a.layers * B * H * length * DH * 2
        r = {name: dict(ms=_spread(xs), tb_per_s=round(live / (sorted(xs)[len(xs) // 2] * 1e-3) / 1e12, 3)) for name, xs in ms.items()}
        d, p = r["dense"]["ms"], r["paged"]["ms"]
        r["paged_over_dense"] = round(p["median"] / d["median"], 4)
        r["difference_ms"] = round(p["median"] - d["median"], 4)
        r["largest_spread_ms"] = round(max(d["max"] - d["min"], p["max"] - p["min"]), 4)
        r["paged_slower_beyond_spread"] = bool(p["median"] - d["median"] > r["largest_spread_ms"])
        r["bit_identical_outputs"] = bool(same)
        out[f"len{length}"] = r
        del dense, pools
        torch.cuda.empty_cache()
    return dict(shape=dict(B=B, H=H, Hkv=H, Dh=DH, layers=a.layers, dtype="bf16"), launches_of_the_pair=2, **out)


def _workload(a, g, dev, dt):
    from setok_amd import ops
    from setok_amd.generation import ContinuousBatcher
    gen = torch.Generator().manual_seed(a.seed)
    T = torch.randint(32, 1025, (a.requests,), generator=gen).tolist()
    N = torch.randint(16, 257, (a.requests,), generator=gen).tolist()
    llm = _llm(a.layers, g, dev, dt)
    xs = [torch.randn(t, D, generator=g, device=dev, dtype=dt) for t in T]
    per_seq = (1024 + 256 + ops.KV_PAGE - 1) // ops.KV_PAGE
    num_pages = a.rows * per_seq
    useful = sum(N)

    def continuous():
        b = ContinuousBatcher(llm, a.rows, num_pages, max_pages_per_seq=per_seq)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = b.run(list(zip(xs, N)))
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        assert [o.numel() for o in outs] == N
        return dt_s, dict(steps=b.stats["steps"], occupancy=round(b.occupancy, 4), pages_high_water=b.stats["pages_high_water"],
                          cache_bytes=b.stats["pages_high_water"] * b.cache.page_nbytes, pool_bytes=b.cache.nbytes(),
                          page_waits=b.stats["page_waits"])

    def static():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = active = cache_bytes = 0
        for i in range(0, a.requests, a.rows):
            ts, ns, chunk = T[i:i + a.rows], N[i:i + a.rows], xs[i:i + a.rows]
            tm, nm = max(ts), max(ns)
            x = torch.zeros(len(chunk), tm, D, device=dev, dtype=dt)
            am = torch.zeros(len(chunk), tm, dtype=torch.int64, device=dev)
            for j, c in enumerate(chunk):                                  # left-padded
                x[j, tm - ts[j]:], am[j, tm - ts[j]:] = c, 1
            out = llm.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=nm)
            assert tuple(out.shape) == (len(chunk), nm)
            steps += nm - 1
            active += sum(n - 1 for n in ns)
            cache_bytes = max(cache_bytes, 2 * a.layers * len(chunk) * H * (tm + nm) * DH * 2)      # KVCache.nbytes() of the call's cache
        torch.cuda.synchronize()
        return time.perf_counter() - t0, dict(steps=steps, occupancy=round(active / max(steps * a.rows, 1), 4), cache_bytes=cache_bytes)

    arms = dict(continuous=continuous, static=static)
    continuous()                                                           # warm-up: both arms once (allocator, first launches)
    static()
    runs = {name: [] for name in arms}
    info = {}
    for _ in range(a.workload_rounds):
        for name, fn in arms.items():
            s, info[name] = fn()
            runs[name].append(s)
    r = {}
    for name, xs_ in runs.items():
        sp = _spread(xs_)
        r[name] = dict(drain_s=sp, tokens_per_s=round(useful / sp["median"], 1), **info[name])
    r["continuous_over_static_tokens_per_s"] = round(r["continuous"]["tokens_per_s"] / r["static"]["tokens_per_s"], 3)
    r["cache_bytes_continuous_over_static"] = round(r["continuous"]["cache_bytes"] / r["static"]["cache_bytes"], 3)
    return dict(requests=a.requests, rows=a.rows, layers=a.layers, dtype="bf16", seed=a.seed, prompt_tokens=sum(T), emitted_tokens=useful,
                prompt_lengths=dict(min=min(T), max=max(T)), max_new_tokens=dict(min=min(N), max=max(N)), num_pages=num_pages,
                page_bytes=2 * a.layers * H * ops.KV_PAGE * DH * 2, **r)


def _prefix_workload(a, g, dev, dt):
    """Requests that share a 600-row prompt prefix (a system prompt and an image: Ps = 512 shared slots, a tail of 88) with remainders uniform in
    [16, 128] rows and max_new_tokens uniform in [16, 128], through `ContinuousBatcher`: the prefix registered once and every request submitted
    behind it, against the same requests submitted with their full prompts.  The same pool in both arms.  Time to drain (the registration
    included), emitted tokens per second, seconds per admission (the host clock around a step's admissions, the device drained before and after -
    in both arms) and the pages in use at the high-water mark."""
    from setok_amd import ops
    from setok_amd.generation import ContinuousBatcher
    gen = torch.Generator().manual_seed(a.seed)
    P = 600
    S = torch.randint(16, 129, (a.requests,), generator=gen).tolist()
    N = torch.randint(16, 129, (a.requests,), generator=gen).tolist()
    llm = _llm(a.layers, g, dev, dt)
    prefix = torch.randn(P, D, generator=g, device=dev, dtype=dt)
    rest = [torch.randn(s, D, generator=g, device=dev, dtype=dt) for s in S]
    full = [torch.cat([prefix, x]) for x in rest]
    per_seq = (P + 128 + 128 + ops.KV_PAGE - 1) // ops.KV_PAGE
    num_pages = a.rows * per_seq + P // ops.KV_PAGE
    useful = sum(N)

    def drain(shared):
        b = ContinuousBatcher(llm, a.rows, num_pages, max_pages_per_seq=per_seq)
        # The batcher has no timing hook: the admissions of a step are `ContinuousBatcher._admit`, which `step()` calls once, so that method is
        # wrapped on this instance.  `calls` is checked below: if `step()` stops going through `_admit`, this fails instead of reporting 0 ms.
        admit, spent, calls = b._admit, [0.0], [0]

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
        if shared:
            h = b.register_prefix(prefix)
            outs = b.run([(x, n, h) for x, n in zip(rest, N)])
        else:
            outs = b.run(list(zip(full, N)))
        torch.cuda.synchronize()
        dt_s = time.perf_counter() - t0
        assert [o.numel() for o in outs] == N
        assert calls[0] >= b.stats["steps"] > 0 and b.stats["admitted"] == a.requests, "step() no longer admits through _admit: the admission clock saw nothing"
        return dt_s, dict(steps=b.stats["steps"], occupancy=round(b.occupancy, 4), pages_high_water=b.stats["pages_high_water"],
                          cache_bytes=b.stats["pages_high_water"] * b.cache.page_nbytes, page_waits=b.stats["page_waits"],
                          admission_ms=round(1e3 * spent[0] / b.stats["admitted"], 3), prefix_stats=dict(b.prefix_stats))

    arms = dict(shared_prefix=lambda: drain(True), full_prompts=lambda: drain(False))
    for fn in arms.values():
        fn()                                                               # warm-up: both arms once (allocator, first launches)
    runs, info = {name: [] for name in arms}, {}
    for _ in range(a.workload_rounds):
        for name, fn in arms.items():
            s, info[name] = fn()
            runs[name].append(s)
    r = {}
    for name, xs_ in runs.items():
        sp = _spread(xs_)
        r[name] = dict(drain_s=sp, tokens_per_s=round(useful / sp["median"], 1), **info[name])
    s, f = r["shared_prefix"], r["full_prompts"]
    r["shared_over_full_tokens_per_s"] = round(s["tokens_per_s"] / f["tokens_per_s"], 3)
    r["shared_over_full_admission_ms"] = round(s["admission_ms"] / f["admission_ms"], 3)
    r["largest_drain_spread_s"] = round(max(s["drain_s"]["max"] - s["drain_s"]["min"], f["drain_s"]["max"] - f["drain_s"]["min"]), 4)
    r["pages_high_water_shared_over_full"] = round(s["pages_high_water"] / f["pages_high_water"], 3)
    return dict(requests=a.requests, rows=a.rows, layers=a.layers, dtype="bf16", seed=a.seed, prefix_rows=P, shared_slots=ops.KV_PAGE * (P // ops.KV_PAGE),
                remainder_rows=dict(min=min(S), max=max(S), total=sum(S)), max_new_tokens=dict(min=min(N), max=max(N)), emitted_tokens=useful,
                num_pages=num_pages, page_bytes=2 * a.layers * H * ops.KV_PAGE * DH * 2, rounds=a.workload_rounds, **r)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_bench.json"))
    ap.add_argument("--prefix", action="store_true", help="only the shared-prefix workload, recorded as a section of --prefix-out")
    ap.add_argument("--prefix-out", default=os.path.join(ROOT, "profiles", "prefix_bench.json"))
    a = ap.parse_args()
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    if a.prefix:
        from bench_extend import _merge_into                           # (the file is shared with tools/bench_extend.py --only paged_pair)
        with torch.no_grad():
            res = dict(device=torch.cuda.get_device_name(0), **_prefix_workload(a, g, dev, dt))
        _merge_into(a.prefix_out, "shared_prefix_workload", res)
        print(json.dumps(res))
        return
    with torch.no_grad():
        run = dict(device=torch.cuda.get_device_name(0), kernel_cost_of_paging=_kernel_cost(a, g, dev, dt))
        if not a.skip_workload:
            run["ragged_workload"] = _workload(a, g, dev, dt)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(run, f, indent=1)
    print(json.dumps(run))


if __name__ == "__main__":
    main()
