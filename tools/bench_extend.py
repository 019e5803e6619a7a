"""Extending a filled KV cache by several tokens (LlamaModel.extend, csrc/attn_extend.hip) at Vicuna-7B dims in bf16, each use against the way the
library had to do the same work before, both arms alternated round by round in ONE process:

  verify        B in {1, 8}, 2048 cached slots: one extend(Tn = 8)            against  eight decode_steps
  second_turn   B = 8, 600 cached slots: extend(Tn = 64)                      against  a fresh prefill of 664 rows
  chunked       generate over a 2048-row prompt with prefill_chunk = 512      against  the unchunked call; time and torch.cuda.max_memory_allocated
                (also with the call's KV cache, the same in both arms, taken off: what the windows bound is the rest)
  attention     the extend attention's launch pair (chunks + merge) alone over every layer's cache at those shapes: live K / V bytes per second
                (next to the decode pair at the same cache length) and, at Tn = 512, the MFMA rate

    python tools/bench_extend.py [--layers 32] [--rounds 5] [--reps 10] [--out profiles/extend_bench.json]
    python tools/bench_extend.py --only attention          # one section
    python tools/bench_extend.py --only paged_pair         # the paged extend attention's launch pair against the dense pair at the same rows
                                                           # (B = 1, 88 rows behind 512 slots; B = 8, 8 rows behind 2048) -> a section of profiles/prefix_bench.json
    python tools/bench_extend.py --trace-arm unchunked      # two calls of one arm of the chunked section and nothing else (what a kernel trace is pointed at)

After a warm-up of both arms every arm runs `--rounds` times, `--reps` calls per run between two device events; median, min, max and every run are
recorded, and `beats_by_more_than_the_spread` says whether the new arm's slowest run is faster than the old arm's fastest.  The caches hold random
data (zeros would flatter the softmax and the clocks).  Writes one JSON object to `--out` and prints it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import D, DH, H, _filled_cache, _llm, _set_len, _spread, _time      # noqa: E402  (the same model, cache filling and timer)


def _arms(arms, rounds, reps):
    """{name: fn} -> {name: spread of ms per call}, the arms alternated round by round after one warm-up call each."""
    for fn in arms.values():
        _time(fn, 1)
    runs = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            runs[k].append(_time(fn, reps))
    return {k: _spread(v) for k, v in runs.items()}


def _versus(r, new, old):
    r["new_over_old_median"] = round(r[new]["median"] / r[old]["median"], 3)
    r["beats_by_more_than_the_spread"] = r[new]["max"] < r[old]["min"]
    return r


def verify(llm, a, g, rnd):
    out = {}
    len0, Tn = 2048, 8
    for B in (1, 8):
        c = _filled_cache(llm, B, len0 + Tn, len0, g)
        e = rnd(B, Tn, D)

        def extend():
            _set_len(c, len0)
            return llm.model.extend(e, c)

        def steps():
            _set_len(c, len0)
            for i in range(Tn):
                llm.model.decode_step(e[:, i], c)

        out[f"B{B}"] = _versus(_arms({"extend_8": extend, "decode_step_x8": steps}, a.rounds, a.reps), "extend_8", "decode_step_x8")
        del c
    return dict(len0=len0, Tn=Tn, ms=out)


def second_turn(llm, a, g, rnd):
    B, len0, Tn = 8, 600, 64
    c = _filled_cache(llm, B, len0 + Tn, len0, g)
    fresh = _filled_cache(llm, B, len0 + Tn, 0, g)
    e, whole = rnd(B, Tn, D), rnd(B, len0 + Tn, D)

    def extend():
        _set_len(c, len0)
        return llm.model.extend(e, c)

    def prefill():
        _set_len(fresh, 0)
        return llm.model.prefill(whole, None, None, fresh)

    r = _versus(_arms({"extend_64": extend, "prefill_664": prefill}, a.rounds, a.reps), "extend_64", "prefill_664")
    return dict(B=B, len0=len0, Tn=Tn, ms=r)


def chunked(llm, a, g, rnd):
    B, T, N = a.chunked_batch, 2048, 512
    x = rnd(B, T, D)
    res, peaks = {}, {}
    cache_gb = 2 * len(llm.model.layers) * B * llm.model.num_kv_heads * (T + 1) * DH * 2 / 1e9      # the call's KV cache: the same in both arms

    def run(chunk):
        return llm.generate(inputs_embeds=x, max_new_tokens=1, prefill_chunk=chunk)

    for k, chunk in (("prefill_chunk_512", N), ("unchunked", None)):
        run(chunk)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        run(chunk)
        torch.cuda.synchronize()
        above = (torch.cuda.max_memory_allocated() - base) / 1e9
        peaks[k] = dict(max_memory_allocated_gb=round(torch.cuda.max_memory_allocated() / 1e9, 3), above_weights_and_input_gb=round(above, 3),
                        kv_cache_gb=round(cache_gb, 3), activations_and_workspace_gb=round(above - cache_gb, 3))
    res = _arms({"prefill_chunk_512": lambda: run(N), "unchunked": lambda: run(None)}, a.rounds, max(1, a.reps // 2))
    res["chunked_over_unchunked_median"] = round(res["prefill_chunk_512"]["median"] / res["unchunked"]["median"], 3)
    return dict(B=B, T=T, prefill_chunk=N, ms=res, memory=peaks)


def attention(llm, a, g, rnd):
    """The launch pair alone, over every layer's own cache (the keys are never re-read from a cache level between layers)."""
    from setok_amd import ops
    out = {}
    for B, Tn, len0 in ((1, 8, 2048), (8, 8, 2048), (8, 64, 600), (a.chunked_batch, 512, 1536)):
        c = _filled_cache(llm, B, len0 + Tn, len0 + Tn, g)
        q = rnd(B * Tn, 3 * D)
        ws = c.workspace(H, Tn, len0)
        o = torch.empty(B * Tn, H * DH, dtype=q.dtype, device=q.device)
        ext = lambda: [ops.attention_extend(q, k, v, c.key_mask, H, Tn, len0, DH ** -0.5, ws=ws, out=o) for k, v in zip(c.k, c.v)]
        q1, o1 = q[:B], o[:B]
        dec = lambda: [ops.attention_decode(q1, k, v, c.key_mask, H, len0 + Tn, DH ** -0.5, ws=ws, out=o1) for k, v in zip(c.k, c.v)]
        r = _arms({"extend_pair": ext, "decode_pair_one_row": dec}, a.rounds, a.reps)
        live = 2.0 * len(c.k) * B * c.Hkv * (len0 + Tn) * DH * 2
        flops = 4.0 * len(c.k) * B * H * DH * (Tn * len0 + Tn * (Tn + 1) / 2)
        for k in r:
            r[k]["kv_tb_per_s"] = round(live / (r[k]["median"] * 1e-3) / 1e12, 3)
        r["extend_pair"]["tflops"] = round(flops / (r["extend_pair"]["median"] * 1e-3) / 1e12, 1)
        r["live_kv_gb"] = round(live / 1e9, 3)
        r["workspace_gb"] = round(ops.attention_extend_workspace(B, Tn, H, DH, len0, c.Hkv, q.dtype) * 4 / 1e9, 3)
        out[f"B{B}_Tn{Tn}_len0_{len0}"] = r
        del c
    return out


def paged_pair(llm, a, g, rnd):
    """The paged extend attention's launch pair (csrc/attn_extend_paged.hip) against the dense pair at the same rows, over every layer's cache: the
    dense caches' slots copied into pools at a shuffled block table.  An admission behind a shared prefix (B = 1, 88 rows behind 512 slots) and a
    verify-shaped call (B = 8, 8 rows behind 2048).  The ratio of the medians against each arm's spread (max - min over the rounds)."""
    from setok_amd import ops
    out = {}
    for B, Tn, len0 in ((1, 88, 512), (8, 8, 2048)):
        c = _filled_cache(llm, B, len0 + Tn, len0 + Tn, g)
        per = (len0 + Tn + ops.KV_PAGE - 1) // ops.KV_PAGE
        n_pages = B * per
        perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(len0)).to(torch.int32).reshape(B, per)
        q_dev = c.key_mask.device
        table, idx = perm.to(q_dev), perm.reshape(-1).long().to(q_dev)
        pools = []
        for k, v in zip(c.k, c.v):
            pair = []
            for src in (k, v):
                padded = torch.zeros(B, c.Hkv, per * ops.KV_PAGE, DH, dtype=src.dtype, device=q_dev)
                padded[:, :, :len0 + Tn] = src
                pool = torch.empty(n_pages, c.Hkv, ops.KV_PAGE, DH, dtype=src.dtype, device=q_dev)
                pool[idx] = padded.reshape(B, c.Hkv, per, ops.KV_PAGE, DH).transpose(1, 2).reshape(n_pages, c.Hkv, ops.KV_PAGE, DH)
                pair.append(pool)
            pools.append(tuple(pair))
        q = rnd(B * Tn, 3 * D)
        lens = torch.full((B,), len0, dtype=torch.int32, device=q_dev)
        ws = c.workspace(H, Tn, len0)
        o = torch.empty(B * Tn, H * DH, dtype=q.dtype, device=q.device)
        dense = lambda: [ops.attention_extend(q, k, v, c.key_mask, H, Tn, len0, DH ** -0.5, ws=ws, out=o) for k, v in zip(c.k, c.v)]
        paged = lambda: [ops.attention_extend_paged(q, kp, vp, table, lens, H, Tn, len0, DH ** -0.5, ws=ws, out=o) for kp, vp in pools]
        same = torch.equal(ops.attention_extend(q, c.k[0], c.v[0], c.key_mask, H, Tn, len0, DH ** -0.5),
                           ops.attention_extend_paged(q, pools[0][0], pools[0][1], table, lens, H, Tn, len0, DH ** -0.5))
        r = _arms({"dense_pair": dense, "paged_pair": paged}, a.rounds, a.reps)
        d, p = r["dense_pair"], r["paged_pair"]
        r["paged_over_dense"] = round(p["median"] / d["median"], 4)
        r["difference_ms"] = round(p["median"] - d["median"], 4)
        r["largest_spread_ms"] = round(max(d["max"] - d["min"], p["max"] - p["min"]), 4)
        r["paged_slower_beyond_spread"] = bool(p["median"] - d["median"] > r["largest_spread_ms"])
        r["bit_identical_outputs"] = bool(same)
        out[f"B{B}_Tn{Tn}_len0_{len0}"] = r
        del c, pools
        torch.cuda.empty_cache()
    return dict(shape=dict(H=H, Hkv=H, Dh=DH, layers=a.layers, dtype="bf16"), launches_of_the_pair=2, ms=out)


def _merge_into(path, key, value):
    """One section of a JSON file that several tools write: the file's other keys are kept."""
    run = {}
    if os.path.isfile(path):
        with open(path) as f:
            run = json.load(f)
    run[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(run, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chunked-batch", type=int, default=4)
    ap.add_argument("--only", choices=("verify", "second_turn", "chunked", "attention", "paged_pair"), default=None)
    ap.add_argument("--prefix-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "prefix_bench.json"),
                    help="where --only paged_pair records its section (a file it shares with tools/bench_paged.py --prefix)")
    ap.add_argument("--trace-arm", choices=("prefill_chunk_512", "unchunked"), default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "extend_bench.json"))
    a = ap.parse_args()
    from setok_amd import ops

    dev, dt = "cuda:0", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float32).to(dt)
    llm = _llm(a.layers, g, dev, dt)
    if a.trace_arm:
        x = rnd(a.chunked_batch, 2048, D)
        for _ in range(2):
            llm.generate(inputs_embeds=x, max_new_tokens=1, prefill_chunk=512 if a.trace_arm == "prefill_chunk_512" else None)
        torch.cuda.synchronize()
        print(json.dumps(dict(arm=a.trace_arm, calls=2, B=a.chunked_batch, T=2048, layers=a.layers)))
        return
    if a.only == "paged_pair":                                            # its own file: not a section of extend_bench.json
        res = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, reps=a.reps, **paged_pair(llm, a, g, rnd))
        _merge_into(a.prefix_out, "paged_against_dense_launch_pair", res)
        print(json.dumps(res))
        return
    sections = dict(verify=verify, second_turn=second_turn, chunked=chunked, attention=attention)
    res = {k: fn(llm, a, g, rnd) for k, fn in sections.items() if a.only in (None, k)}
    run = dict(workload="extending a KV cache by Tn tokens, Llama at Vicuna-7B dims, bf16: each use against the parent's way of doing the same work, "
                        "arms alternated in one process; ms per call",
               layers=a.layers, rounds=a.rounds, reps=a.reps, extend_chunk=ops.EXTEND_CHUNK, decode_chunk=ops.DECODE_CHUNK,
               device=torch.cuda.get_device_name(0), results=res)
    if a.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(run, f, indent=1)
            f.write("\n")
    print(json.dumps(run))


if __name__ == "__main__":
    main()
