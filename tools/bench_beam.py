"""Beam search (`generate(beams=...)`, csrc/beam.hip) at Vicuna-7B dims in bf16 against the plain greedy loop at the same row count, all arms
alternated round by round in ONE process after a warm-up, every timing ended by a device synchronise:

  loop      (B, n) in {(1, 2), (1, 4), (1, 8), (4, 4)}: `beams=BeamSearch(n)` on B sequences against the greedy loop on B * n rows (the same decode
            step, GEMMs at M = B * n, the same cache size), no eos, so both run all `--new` steps.
  kernels   setok_beam_topk, setok_beam_advance and setok_kv_reorder alone at the same shapes (the reorder with every row moving, over `--new` / 2
            generated slots), HIP events over 100 back-to-back calls, and the wall time of the step's one host read.

    python tools/bench_beam.py [--layers 32] [--rounds 5] [--prompt 512] [--new 64] [--out profiles/beam_bench.json]

ms per step = (the call - the same round's one-token call of the same arm) / (new - 1): the prefill, the first selection and - for the beam arm - the
replication of the cache are common to both calls.  Writes one JSON object to `--out` and prints it."""
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

from bench_generate import D, V, _llm, _spread      # noqa: E402  (the same model and statistics)

SHAPES = ((1, 2), (1, 4), (1, 8), (4, 4))


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _events(fn, calls=100):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3                           # us per call


def loop(llm, a, rnd):
    from setok_amd.generation import BeamSearch
    out = {}
    for B, n in SHAPES:
        x = rnd(B, a.prompt, D)
        xr = x.repeat_interleave(n, dim=0).contiguous()
        beams = BeamSearch(n)
        arms = dict(greedy_first=lambda: llm.generate(inputs_embeds=xr, max_new_tokens=1),
                    greedy=lambda: llm.generate(inputs_embeds=xr, max_new_tokens=a.new),
                    beams_first=lambda: llm.generate(inputs_embeds=x, max_new_tokens=1, beams=beams),
                    beams=lambda: llm.generate(inputs_embeds=x, max_new_tokens=a.new, beams=beams))
        for fn in arms.values():
            _wall(fn)
        runs = {k: [] for k in arms}
        for _ in range(a.rounds):
            for k, fn in arms.items():
                runs[k].append(_wall(fn)[0])
        res = dict(call_ms={k: _spread(v) for k, v in runs.items()})
        per = {k: [(t - p) / (a.new - 1) for t, p in zip(runs[k], runs[k + "_first"])] for k in ("greedy", "beams")}
        res["ms_per_step"] = {k: _spread(v) for k, v in per.items()}
        res["beams_minus_greedy_ms_per_step_median"] = round(res["ms_per_step"]["beams"]["median"] - res["ms_per_step"]["greedy"]["median"], 4)
        res["new_tokens_of_the_best_hypothesis"] = int(llm.generate(inputs_embeds=x, max_new_tokens=a.new, beams=beams).shape[1])
        out[f"B{B}_n{n}"] = res
    return out


def kernels(llm, a, rnd, dev):
    from setok_amd import ops
    from setok_amd.generation import KVCache
    out = {}
    for B, n in SHAPES:
        C, rows = 2 * n, B * n
        logits = rnd(rows, V)
        state = ops.BeamState(B, n, a.new, dev)
        state.run_score.copy_(-torch.rand(B, n, device=dev))
        ws = torch.empty(rows * 129, dtype=torch.int32, device=dev)
        cand = ops.beam_topk(logits, state.run_score, C, ws)
        res = dict(beam_topk_us=round(_events(lambda: ops.beam_topk(logits, state.run_score, C, ws)), 2))
        keep = state.run_score.clone()

        def advance():
            state.run_score.copy_(keep)                                 # (one small copy: the kernel reads what it wrote, the candidates stay the same)
            ops.beam_advance(*cand, state, None, 3, 1.0, False)

        res["beam_advance_us_with_one_copy"] = round(_events(advance), 2)
        cache = KVCache.for_model(llm.model, rows, a.prompt + a.new)
        cache.len = a.prompt + a.new // 2
        src = ((torch.arange(rows, device=dev) // n) * n + (torch.arange(rows, device=dev) + 1) % n).to(torch.int32)
        res["kv_reorder_us_every_row_moving"] = round(_events(lambda: cache.reorder(src, a.prompt, n)), 2)
        res["kv_reorder_us_identity"] = round(_events(lambda: cache.reorder(torch.arange(rows, device=dev, dtype=torch.int32), a.prompt, n)), 2)
        res["kv_reorder_bytes_moved_each_way"] = cache.nbytes() // cache.cap * (a.new // 2)
        reads = []
        for _ in range(20):
            ops.beam_advance(*cand, state, None, 3, 1.0, False)
            reads.append(_wall(lambda: state.summary.tolist())[0] * 1e3)
        res["summary_read_us"] = _spread(reads)["median"]
        del cache
        out[f"B{B}_n{n}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    a = ap.parse_args()
    dev, dt = "cuda:0", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float32).to(dt)
    llm = _llm(a.layers, g, dev, dt)
    res = dict(kernels_per_call=kernels(llm, a, rnd, dev), loop=loop(llm, a, rnd))
    run = dict(workload="beam search against the greedy loop at the same row count, Llama at Vicuna-7B dims, bf16, seeded weights, no eos; arms "
                        "alternated in one process, wall clock between device synchronises; the new kernels alone by HIP events over 100 calls",
               layers=a.layers, rounds=a.rounds, prompt=a.prompt, new=a.new, device=torch.cuda.get_device_name(0), results=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(run, f, indent=1)
        f.write("\n")
    print(json.dumps(run))


if __name__ == "__main__":
    main()
