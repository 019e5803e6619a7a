"""Logits processors (`generate(processors=...)`, csrc/logits.hip) at Vicuna-7B dims in bf16 against the greedy loop without them, all arms alternated
round by round in ONE process after a warm-up, every timing ended by a device synchronise:

  loop      B in {1, 8, 32} x prompts of 64 and 2048 ids (the starting history): the greedy step with `processors=None` against the greedy step with
            repetition_penalty 1.3 + no_repeat_ngram_size 3 + min_new_tokens (an eos id the run is kept from emitting), `--new` steps each.
  parent    the greedy loop with `processors=None` at the setting of profiles/generate_bench.json (prompt 552, 200 new tokens), measured as two
            identical arms: their difference is the run's own arm-to-arm noise, their value stands next to the recorded one.
  kernels   setok_logits_process and setok_history_append alone at the same shapes, HIP events over 100 back-to-back calls.

    python tools/bench_processors.py [--layers 32] [--rounds 3] [--new 64] [--out profiles/processors_bench.json] [--parent-setting-only]

`--parent-setting-only` measures the `parent` part alone and needs nothing of this feature, so the same file also runs from a checkout of the commit
before it: processes of both checkouts, alternated, are the comparison with the parent commit (`greedy_step_across_processes` in the profile).

ms per step = (the call - the same round's one-token call of the same arm) / (new - 1): the prefill and the first selection are common to both calls.
Writes one JSON object to `--out` and prints it."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_beam import _events, _wall               # noqa: E402  (the same clocks)
from bench_generate import V, _llm, _spread         # noqa: E402  (the same model and statistics)

BATCHES = (1, 8, 32)
HISTORIES = (64, 2048)
EOS = 7


def _alternate(arms, rounds):
    for fn in arms.values():
        _wall(fn)
    runs = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            runs[k].append(_wall(fn)[0])
    return runs


def loop(llm, a, g, dev):
    from setok_amd.generation import LogitsProcessors
    proc = LogitsProcessors(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=a.new + 1)
    out = {}
    for B in BATCHES:
        for T in HISTORIES:
            ids = torch.randint(0, V, (B, T), generator=g, device=dev)
            arms = dict(none_first=lambda: llm.generate(inputs=ids, max_new_tokens=1, eos_token_id=EOS),      # (the eos id: both arms read the host once per step)
                        none=lambda: llm.generate(inputs=ids, max_new_tokens=a.new, eos_token_id=EOS),
                        processors_first=lambda: llm.generate(inputs=ids, max_new_tokens=1, processors=proc, eos_token_id=EOS),
                        processors=lambda: llm.generate(inputs=ids, max_new_tokens=a.new, processors=proc, eos_token_id=EOS))
            runs = _alternate(arms, a.rounds)
            per = {k: [(t - p) / (a.new - 1) for t, p in zip(runs[k], runs[k + "_first"])] for k in ("none", "processors")}
            res = dict(call_ms={k: _spread(v) for k, v in runs.items()}, ms_per_step={k: _spread(v) for k, v in per.items()})
            res["processors_minus_none_ms_per_step_median"] = round(res["ms_per_step"]["processors"]["median"] - res["ms_per_step"]["none"]["median"], 4)
            out[f"B{B}_hist{T}"] = res
    return out


def parent(llm, a, g, dev, recorded):
    out = {}
    for B in BATCHES:
        ids = torch.randint(0, V, (B, 552), generator=g, device=dev)
        arms = dict(a_first=lambda: llm.generate(inputs=ids, max_new_tokens=1), a=lambda: llm.generate(inputs=ids, max_new_tokens=200),
                    b_first=lambda: llm.generate(inputs=ids, max_new_tokens=1), b=lambda: llm.generate(inputs=ids, max_new_tokens=200))
        runs = _alternate(arms, a.rounds)
        per = {k: _spread([(t - p) / 199 for t, p in zip(runs[k], runs[k + "_first"])]) for k in ("a", "b")}
        out[f"B{B}"] = dict(ms_per_step_two_identical_arms=per, arm_to_arm_ms=round(abs(per["a"]["median"] - per["b"]["median"]), 4),
                            recorded_ms_per_token_after_prefill=recorded.get(f"B{B}", {}).get("generate", {}).get("ms_per_token_after_prefill"))
    return out


def kernels(a, g, dev):
    from setok_amd import ops
    out = {}
    for B in BATCHES:
        logits = torch.randn(B, V, generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
        scores = torch.empty(B, V, dtype=torch.float32, device=dev)
        eos = torch.tensor([EOS], dtype=torch.int64, device=dev)
        for T in HISTORIES:
            hist = torch.randint(0, V, (B, T + 8), generator=g, device=dev)
            hist_len = torch.full((B,), T, dtype=torch.int32, device=dev)
            res = dict(logits_process_us=round(_events(lambda: ops.logits_process(logits, hist, hist_len, hist_len, None, 1.3, 3, a.new + 1, eos, None,
                                                                                    out=scores)), 2),
                       logits_process_bytes=B * (V * 6 + T * 8))
            tok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
            zero = torch.zeros(B, dtype=torch.int32, device=dev)                            # (m = 0: the launch, no growth over 100 calls)
            res["history_append_us"] = round(_events(lambda: ops.history_append(hist, hist_len, tok, T + 8, zero)), 2)
            out[f"B{B}_hist{T}"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "processors_bench.json"))
    ap.add_argument("--parent-setting-only", action="store_true")
    a = ap.parse_args()
    dev, dt = "cuda:0", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    with open(os.path.join(ROOT, "profiles", "generate_bench.json")) as f:
        recorded = json.load(f)["results"]
    res = {} if a.parent_setting_only else dict(kernels_per_call=kernels(a, g, dev))
    llm = _llm(a.layers, g, dev, dt)
    if not a.parent_setting_only:
        res["loop"] = loop(llm, a, g, dev)
    res["parent_setting"] = parent(llm, a, g, dev, recorded)
    run = dict(workload="greedy generate with logits processors (penalty 1.3, 3-gram ban, min_new_tokens) against processors=None, Llama at Vicuna-7B "
                        "dims, bf16, seeded weights; arms alternated in one process, wall clock between device synchronises; the new kernels alone by "
                        "HIP events over 100 calls",
               layers=a.layers, rounds=a.rounds, new=a.new, device=torch.cuda.get_device_name(0), results=res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(run, f, indent=1)
        f.write("\n")
    print(json.dumps(run))


if __name__ == "__main__":
    main()
