"""Draft-and-verify decoding (`generate(draft=...)`, csrc/speculate.hip) at Vicuna-7B dims in bf16 against the plain loop, all arms alternated round
by round in ONE process after a warm-up, every timing ended by a device synchronise:

  ceiling   B in {1, 8}, K in {3, 7}: a ScriptedDrafter (tests/spec_cases.py) that proposes the run's own tokens.  The tokens come from a first
            plain run and are then iterated to a fixed point: in bf16 the extend and the decode kernels round differently, so a speculative run
            may leave the plain run's tokens at a near-tie; its own tokens are fed back until a run reproduces what it was fed (`iterations`).
  floor     the same with an always-wrong drafter: what a useless draft costs.
  kernels   setok_spec_accept (B in {1, 32}, K = 7) and setok_ngram_propose (history 4096, B in {1, 8, 32}) alone, HIP events over 200 back-to-back
            calls, each against the torch composition of the same rule.

    python tools/bench_speculate.py [--layers 32] [--rounds 5] [--prompt 512] [--new 64] [--out profiles/speculate_bench.json]

ms per emitted token = (the call - the same round's prefill-only call) / (new - 1): the prompt's prefill and the first token are common to both arms.
`mean_m` is the realised number of tokens a sequence emitted per round.  Writes one JSON object to `--out` and prints it."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_generate import D, V, _llm, _spread      # noqa: E402  (the same model and statistics)


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def loop(llm, a, rnd):
    import spec_cases as S
    out = {}
    n = a.new
    for B in (1, 8):
        x = rnd(B, a.prompt, D)
        kw = dict(inputs_embeds=x, max_new_tokens=n)
        plain_tokens = llm.generate(**kw)
        for K in (3, 7):
            truth, its = plain_tokens.cpu(), 0
            for its in range(1, 21):                                   # to a fixed point: a run that reproduces the tokens it was fed
                got = llm.generate(draft=S.ScriptedDrafter(truth, K, "right", V), **kw).cpu()
                if torch.equal(got, truth):
                    break
                truth = got
            right, wrong = S.ScriptedDrafter(truth, K, "right", V), S.ScriptedDrafter(truth, K, "wrong", V)
            arms = dict(prefill_only=lambda: llm.generate(inputs_embeds=x, max_new_tokens=1), plain=lambda: llm.generate(**kw),
                        ceiling=lambda: llm.generate(draft=right, **kw), floor=lambda: llm.generate(draft=wrong, **kw))
            for fn in arms.values():
                _wall(fn)
            runs = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, fn in arms.items():
                    runs[k].append(_wall(fn)[0])
            res = dict(call_ms={k: _spread(v) for k, v in runs.items()})
            per = {k: [(t - p) / (n - 1) for t, p in zip(runs[k], runs["prefill_only"])] for k in ("plain", "ceiling", "floor")}
            res["ms_per_emitted_token"] = {k: _spread(v) for k, v in per.items()}
            res["rounds"] = dict(ceiling=right.rounds, floor=wrong.rounds)
            res["mean_m"] = dict(ceiling=round((n - 1) / max(right.rounds, 1), 3), floor=round((n - 1) / max(wrong.rounds, 1), 3))
            res["fixed_point_iterations"] = its
            res["tokens_equal_the_plain_runs"] = bool(torch.equal(truth, plain_tokens.cpu()))
            t = res["ms_per_emitted_token"]
            res["ceiling_over_plain_median"] = round(t["ceiling"]["median"] / t["plain"]["median"], 3)
            res["floor_over_plain_median"] = round(t["floor"]["median"] / t["plain"]["median"], 3)
            res["ceiling_beats_plain_by_more_than_the_spread"] = t["ceiling"]["max"] < t["plain"]["min"]
            out[f"B{B}_K{K}"] = res
    return out


# ---- the kernels alone ----------------------------------------------------------------------------------------------------------------------------
def _events(fn, calls=200):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3                           # us per call


def _torch_accept(draft, sel, eos, seq, count, finished, pending, key_mask, next_pos, len0):
    """The accept rule as a composition of torch ops (no host read); seq has one spare column that takes the rows nobody emitted."""
    B, K = draft.shape
    max_new = seq.shape[1] - 1
    steps = torch.arange(K + 1, device=sel.device)[None]
    nd = (draft >= 0).long().cummin(1).values.sum(1)
    n = ((draft >= 0) & (draft == sel[:, :K])).long().cummin(1).values.sum(1)
    live = (finished == 0) & (count < max_new)
    m = torch.minimum(n + 1, max_new - count.long())
    hit = torch.isin(sel, eos) & (steps < m[:, None])
    m = torch.where(hit.any(1), hit.long().argmax(1) + 1, m)
    done = hit.any(1) | (count.long() + m == max_new)
    m = torch.where(live, m, torch.zeros_like(m))
    took = steps < m[:, None]
    rows = torch.arange(B, device=sel.device)[:, None]
    seq[rows, torch.where(took, count.long()[:, None] + steps, max_new)] = sel
    emitted = torch.where(took, sel, -1)
    pending.copy_(torch.where(live, sel.gather(1, (m - 1).clamp_min(0)[:, None])[:, 0], pending))
    key_mask[:, len0:len0 + K + 1] = took.to(torch.uint8)
    next_pos += torch.where(live, m - 1 - nd, torch.zeros_like(m))
    count += m.to(torch.int32)
    finished |= (live & done).to(torch.uint8)
    summary = torch.stack([m.max(), (finished == 0).sum(), (emitted.where(took, torch.zeros_like(sel)) < 0).any().long()]).to(torch.int32)
    return emitted, m.to(torch.int32), summary


def _torch_ngram(hist, hist_len, emitted, m, K, max_ngram=3, min_ngram=1):
    """The lookup rule as a composition of torch ops."""
    B, cap = hist.shape
    dev = hist.device
    i = torch.arange(emitted.shape[1], device=dev)[None]
    rows = torch.arange(B, device=dev)[:, None]
    keep = i < m[:, None]
    at = torch.where(keep, hist_len.long()[:, None] + i, cap - 1)
    hist[rows, at] = torch.where(keep, emitted, hist[rows, at])
    hist_len += m
    L = hist_len.long()
    out = torch.full((B, K), -1, dtype=torch.int64, device=dev)
    found = torch.zeros(B, dtype=torch.bool, device=dev)
    k = torch.arange(K, device=dev)[None]
    for n in range(max_ngram, min_ngram - 1, -1):
        t = torch.arange(n, device=dev)[None]
        suf = hist.gather(1, (L[:, None] - n + t).clamp_min(0))
        ok = (L > n) & (suf >= 0).all(1)
        win = hist.unfold(1, n, 1)                                     # (B, cap - n + 1, n)
        j = torch.arange(win.shape[1], device=dev)[None]
        eq = (win == suf[:, None, :]).all(2) & (j <= (L - n - 1)[:, None]) & ok[:, None]
        best = torch.where(eq, j, -1).max(1).values
        idx = best[:, None] + n + k
        cont = torch.where(idx < L[:, None], hist.gather(1, idx.clamp(0, cap - 1)), -1)
        use = (best >= 0) & ~found
        out = torch.where(use[:, None], cont, out)
        found |= use
    return out


def kernels(dev):
    from setok_amd import ops
    g = torch.Generator(device=dev).manual_seed(1)
    out, calls = {}, 200
    K = 7
    for B in (1, 32):
        max_new, cap, len0 = (K + 1) * (calls + 2) + 1, 64, 20
        sel = torch.randint(0, 32000, (B, K + 1), generator=g, device=dev)
        draft = sel[:, :K].contiguous()                                # every draft right: K + 1 tokens per call, nobody finishes inside the run
        eos = torch.tensor([32001], device=dev)

        def state(spare):
            return (torch.zeros((B, max_new + spare), dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
                    torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int64, device=dev),
                    torch.zeros((B, cap), dtype=torch.uint8, device=dev), torch.full((B,), 100, dtype=torch.int64, device=dev))

        s_hip, s_torch = state(0), state(1)
        bufs = (torch.empty((B, K + 1), dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                torch.zeros(3, dtype=torch.int32, device=dev))
        hip = _events(lambda: ops.spec_accept(draft, sel, eos, *s_hip, len0, *bufs), calls)
        ref = _events(lambda: _torch_accept(draft, sel, eos, *s_torch, len0), calls)
        same = all(torch.equal(a[..., :max_new] if a.dim() == 2 and a.shape[1] > cap else a, b) for a, b in zip(s_torch, s_hip))
        out[f"spec_accept_B{B}_K{K}"] = dict(hip_us=round(hip, 2), torch_us=round(ref, 2), torch_over_hip=round(ref / hip, 1), same_state=bool(same))
    Lh = 4096
    for B in (1, 8, 32):
        hist0 = torch.randint(0, 2000, (B, Lh + (K + 1) * (calls + 2)), generator=g, device=dev)
        emitted = torch.randint(0, 2000, (B, K + 1), generator=g, device=dev)
        m = torch.full((B,), K + 1, dtype=torch.int32, device=dev)
        h_hip, l_hip = hist0.clone(), torch.full((B,), Lh, dtype=torch.int32, device=dev)
        h_t, l_t = hist0.clone(), torch.full((B,), Lh, dtype=torch.int32, device=dev)
        o = torch.empty((B, K), dtype=torch.int64, device=dev)
        hip = _events(lambda: ops.ngram_propose(h_hip, l_hip, K, hist0.shape[1], emitted, m, out=o), calls)
        last = []
        ref = _events(lambda: last.__setitem__(slice(None), [_torch_ngram(h_t, l_t, emitted, m, K)]), calls)
        same = torch.equal(last[0], o) and torch.equal(l_hip, l_t)
        out[f"ngram_propose_B{B}_hist{Lh}"] = dict(hip_us=round(hip, 2), torch_us=round(ref, 2), torch_over_hip=round(ref / hip, 1),
                                                    same_proposal=bool(same))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--only", choices=("loop", "kernels"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "speculate_bench.json"))
    a = ap.parse_args()
    dev, dt = "cuda:0", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float32).to(dt)
    res = {}
    if a.only in (None, "kernels"):
        res["kernels_us_per_call"] = kernels(dev)
    if a.only in (None, "loop"):
        res["loop"] = loop(_llm(a.layers, g, dev, dt), a, rnd)
    run = dict(workload="draft-and-verify decoding against the plain loop, Llama at Vicuna-7B dims, bf16, seeded weights; arms alternated in one "
                        "process, wall clock between device synchronises; the new kernels alone by HIP events over 200 back-to-back calls",
               layers=a.layers, rounds=a.rounds, prompt=a.prompt, new=a.new, device=torch.cuda.get_device_name(0), results=res)
    if a.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(run, f, indent=1)
            f.write("\n")
    print(json.dumps(run))


if __name__ == "__main__":
    main()
