"""KV-cached greedy decoding at the cfg5 shape (Vicuna-7B dims, bf16, prompt T' = 552 spliced positions) against the only way the library had
to produce token n + 1 before: the whole prefill again over the sequence grown by one token.

    python tools/bench_generate.py [--layers 32] [--batches 32,8,1] [--prompt 552] [--new 200] [--reps 5]
    python tools/bench_generate.py --steps-only 3 [--batch 32]          # prefill-free: a few decode steps and nothing else (what a kernel trace is pointed at)
    python tools/bench_generate.py --attention-only [--gqa 4]           # the decode-attention launch pair alone (what a counter run is pointed at)
    python tools/bench_generate.py --weights fp8 ...                    # any of the above with the stack in fp8 storage (quantize_fp8_); mxfp4: quantize_mxfp4_
    python tools/bench_generate.py --compare-weights [--rounds 3]       # native, fp8 and mxfp4 arms alternated in one process: decode step + the four GEMMs
    python tools/bench_generate.py --compare-bands [--rounds 3]         # linear_fp8w's 16 / 32 / 64-column bands alternated in one process, four GEMMs
    python tools/bench_generate.py --compare-kv [--attention-only]      # native, fp8 and mxfp4 KV caches alternated in one process: the decode step (and two
                                                                        # `extend` calls, native against mxfp4), or the attention pair alone

Prints one JSON line.  Per batch size, in one process:
  (a) ms per token the old way: forward(inputs_embeds of T' + 1 positions, last_token_only=True);
  (b) ms per token with the cache at the first and at the `--new`-th new token (lm_head + argmax + embedding rows + decode_step), the
      decode_step alone, and a whole generate() call divided by its tokens;
  (c) the decode-attention launch pair (chunks + merge) over all layers' caches — each layer has its own, so the keys are never re-read from a
      cache level — as live K/V bytes / time: TB/s, the fraction of 8 TB/s (HBM3E peak) and of the 6.0-6.3 TB/s the LayerNorm kernels reach
      on this chip.
The caches are filled with random data (zeros would flatter the softmax and the clocks)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, H, DH, FD, V = 4096, 32, 128, 11008, 32000


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


def _llm(layers, g, dev, dt, hkv=H):
    from setok_amd.llama import SetokimLlamaPrefill
    cfg = dict(vocab_size=V, hidden_size=D, intermediate_size=FD, num_hidden_layers=layers, num_attention_heads=H, num_key_value_heads=hkv,
               rms_norm_eps=1e-5, rope_theta=10000.0)
    with torch.device(dev):
        llm = SetokimLlamaPrefill(cfg).to(dt)
    for p in llm.parameters():
        if p.dim() == 2:
            p.data.normal_(0.0, 0.02, generator=g)
        else:
            p.data.fill_(1.0)
    return llm.eval().requires_grad_(False)


def _filled_cache(llm, B, cap, length, g):
    """A cache as a prompt of `length` positions leaves it, with random keys / values (no prefill needed for timing)."""
    from setok_amd.generation import KVCache
    c = KVCache.for_model(llm.model, B, cap)
    for t in c.k + c.v:
        t.normal_(0.0, 1.0, generator=g)
    c.key_mask[:, :length] = 1
    c.next_pos.fill_(length)
    c.len = length
    return c


def _set_len(c, length):
    c.key_mask.zero_()
    c.key_mask[:, :length] = 1
    c.next_pos.fill_(length)
    c.len = length


def _attention_pair(c, q, length, reps):
    """ms of the chunks + merge pair summed over every layer's cache, and the live K / V bytes it reads."""
    from setok_amd import ops
    ws = c.workspace(H)
    out = torch.empty(c.B, H * DH, dtype=q.dtype, device=q.device)
    fn = lambda: [ops.attention_decode(q, k, v, c.key_mask, H, length, DH ** -0.5, ws=ws, out=out) for k, v in zip(c.k, c.v)]
    ms = _time(fn, reps)
    live = 2.0 * len(c.k) * c.B * c.Hkv * length * DH * c.k[0].element_size()
    return ms, live


LAYER_SHAPES = ((3 * D, D), (D, D), (2 * FD, D), (D, FD))          # (N, K) of the fused q|k|v, o, gate|up and down projections


def _spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4), runs=[round(x, 4) for x in xs])


def _compare_weights(a, g, dev, dt, rnd):
    """Three arms in ONE process, alternated round by round after a warm-up, every timing ended by a device synchronise: the decode step of a
    native, an fp8-quantised and an mxfp4-quantised stack (three models with the same weights up to the rounding) at the prompt length, and
    `linear_mxfp4w` against `linear_fp8w` against `linear` on the fp8-dequantised weight at the four layer shapes.  Every arm runs `--rounds`
    times: min / median / max are reported, and the run is appended to `--weights-out`."""
    from setok_amd import ops
    T, N = a.prompt, a.new
    native = _llm(a.layers, g, dev, dt)
    fp8 = _llm(a.layers, g, dev, dt)
    fp8.load_state_dict(native.state_dict())
    fp8.quantize_fp8_()
    mx4 = _llm(a.layers, g, dev, dt)
    mx4.load_state_dict(native.state_dict())
    mx4.quantize_mxfp4_()
    arms = (("native", native), ("fp8", fp8), ("mxfp4", mx4))
    ahead = lambda r, x, y: r[x]["max"] < r[y]["min"]                      # x faster than y by more than the spread of both arms
    step = {}
    for B in [int(b) for b in a.batches.split(",")]:
        caches = {k: _filled_cache(m, B, T + N, T, g) for k, m in arms}
        e1 = rnd(B, D)

        def one(k, m):
            _set_len(caches[k], T)
            return m.model.decode_step(e1, caches[k])

        runs = {k: [] for k, _ in arms}
        for _ in range(a.rounds):
            for k, m in arms:
                runs[k].append(_time(lambda: one(k, m), a.reps))
        r = {k: _spread(v) for k, v in runs.items()}
        r["fp8_over_native_median"] = round(r["fp8"]["median"] / r["native"]["median"], 3)
        r["faster_by_more_than_the_spread"] = ahead(r, "fp8", "native")
        r["mxfp4_over_native_median"] = round(r["mxfp4"]["median"] / r["native"]["median"], 3)
        r["mxfp4_over_fp8_median"] = round(r["mxfp4"]["median"] / r["fp8"]["median"], 3)
        r["mxfp4_faster_than_fp8_by_more_than_the_spread"] = ahead(r, "mxfp4", "fp8")
        step[f"B{B}"] = r
        del caches
    del native, fp8, mx4
    torch.cuda.empty_cache()
    kern = {}
    for Nn, K in LAYER_SHAPES:
        # as many copies of each operand as hold 1.2 GB of fp8 q (23 to 71 at the layer shapes; 0.6 GB of nibbles), visited round robin: the
        # weights come from HBM, as the 32 layers of a step do
        copies = max(2, int(1.2e9 // (Nn * K)))
        w = [(torch.randn(Nn, K, generator=g, device=dev, dtype=torch.float32) * 0.02).to(dt) for _ in range(copies)]
        qe = [ops.quantize_fp8_rows(x) for x in w]
        qs = [ops.quantize_mxfp4_rows(x) for x in w]
        w = [ops.dequantize_fp8_rows(q, e, dtype=dt) for q, e in qe]
        for M in (1, 8, 32, 64):
            x = rnd(M, K)
            out = torch.empty(M, Nn, dtype=dt, device=dev)
            fns = dict(native=lambda: [ops.linear(x, wi, out=out) for wi in w],
                       fp8=lambda: [ops.linear_fp8w(x, q, e, out=out) for q, e in qe],
                       mxfp4=lambda: [ops.linear_mxfp4w(x, q, s, out=out) for q, s in qs])
            runs = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, fn in fns.items():
                    runs[k].append(_time(fn, a.reps) / copies)
            r = {k: _spread(v) for k, v in runs.items()}
            r["fp8_q_tb_per_s"] = round(Nn * K / (r["fp8"]["median"] * 1e-3) / 1e12, 3)
            r["native_w_tb_per_s"] = round(2 * Nn * K / (r["native"]["median"] * 1e-3) / 1e12, 3)
            r["mxfp4_qs_tb_per_s"] = round((Nn * K / 2 + Nn * K / 32) / (r["mxfp4"]["median"] * 1e-3) / 1e12, 3)
            r["mxfp4_over_fp8_median"] = round(r["mxfp4"]["median"] / r["fp8"]["median"], 3)
            r["mxfp4_over_native_median"] = round(r["mxfp4"]["median"] / r["native"]["median"], 3)
            r["mxfp4_faster_than_fp8_by_more_than_the_spread"] = ahead(r, "mxfp4", "fp8")
            kern[f"N{Nn}_K{K}_M{M}"] = r
        del w, qe, qs
    run = dict(
        workload="cfg5 LLM decode step, Llama at Vicuna-7B dims, bf16: the stack's projection weights native (bf16) against fp8 e4m3 storage against "
                 "MXFP4 (e2m1 nibbles + one e8m0 scale per 32); ms per decode step at cache length = prompt, and ms per GEMM call at the four layer "
                 "shapes (operands cycled through >= 1.2 GB of fp8 bytes)",
        layers=a.layers, prompt=T, reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), decode_step_ms=step, gemm_ms=kern,
        peak_bytes=torch.cuda.max_memory_allocated())
    runs = []
    if os.path.isfile(a.weights_out):
        with open(a.weights_out) as f:
            runs = json.load(f)
    runs.append(run)
    os.makedirs(os.path.dirname(os.path.abspath(a.weights_out)), exist_ok=True)
    with open(a.weights_out, "w") as f:
        json.dump(runs, f, indent=1)
        f.write("\n")
    print(json.dumps(run))


def _fp8_twin(c):
    """The fp8 cache that holds what the native cache `c` holds, quantised row by row (the library's own quantiser: the same rule)."""
    from setok_amd import ops
    from setok_amd.generation import KVCache
    f = KVCache(len(c.k), c.B, c.Hkv, c.cap, c.Dh, c.dtype, c.key_mask.device, kv_format="fp8")
    for li in range(len(c.k)):
        for src, q, e in ((c.k[li], f.k_q[li], f.k_e[li]), (c.v[li], f.v_q[li], f.v_e[li])):
            ops.quantize_fp8_rows(src.view(-1, c.Dh), q=q.view(-1, c.Dh), e=e.view(-1))
    f.key_mask.copy_(c.key_mask)
    f.next_pos.copy_(c.next_pos)
    f.len = c.len
    return f


def _mxfp4_twin(c):
    """The mxfp4 cache that holds what the native cache `c` holds, quantised block by block (the library's own quantiser: the same rule)."""
    from setok_amd import ops
    from setok_amd.generation import KVCache
    f = KVCache(len(c.k), c.B, c.Hkv, c.cap, c.Dh, c.dtype, c.key_mask.device, kv_format="mxfp4")
    for li in range(len(c.k)):
        for src, q, sc in ((c.k[li], f.k_q[li], f.k_s[li]), (c.v[li], f.v_q[li], f.v_s[li])):
            ops.quantize_mxfp4_rows(src.view(-1, c.Dh), q=q.view(-1, c.Dh // 2), s=sc.view(-1, c.Dh // 32))
    f.key_mask.copy_(c.key_mask)
    f.next_pos.copy_(c.next_pos)
    f.len = c.len
    return f


def _versus(r, a, b):
    """Arm `a` against arm `b` of one cell: the ratio of the medians, and whether the medians differ by more than the larger of the two arms'
    spreads (max - min over the rounds)."""
    gap = abs(r[a]["median"] - r[b]["median"])
    return dict(ratio=round(r[a]["median"] / r[b]["median"], 3),
                exceeds_the_larger_spread=gap > max(r[a]["max"] - r[a]["min"], r[b]["max"] - r[b]["min"]))


def _compare_extend(a, llm, g, dev, dt, rnd):
    """One `LlamaModel.extend` of Tn rows behind len0 filled slots at B = 1, over the native cache and over its mxfp4 twin, alternated round by
    round: 8 rows behind 2048 slots (a verify-shaped call) and 512 rows behind 512 (a window of a chunked prefill, a turn)."""
    from setok_amd.generation import KVCache
    res = {}
    for len0, Tn in ((2048, 8), (512, 512)):
        native = KVCache(a.layers, 1, H, len0 + Tn, DH, dt, dev)
        for t in native.k + native.v:
            t.normal_(0.0, 1.0, generator=g)
        _set_len(native, len0)
        caches = {"native": native, "mxfp4": _mxfp4_twin(native)}
        x = rnd(1, Tn, D)

        def fn(k):
            _set_len(caches[k], len0)
            return llm.model.extend(x, caches[k])

        for k in caches:
            _time(lambda: fn(k), 1)
        runs = {k: [] for k in caches}
        for _ in range(a.rounds):
            for k in caches:
                runs[k].append(_time(lambda: fn(k), a.reps))
        r = {k: _spread(v) for k, v in runs.items()}
        r["mxfp4_vs_native"] = _versus(r, "mxfp4", "native")
        res[f"len0_{len0}_Tn{Tn}"] = r
        del caches, native
        torch.cuda.empty_cache()
    return res


def _compare_kv(a, g, dev, dt, rnd):
    """The native, the fp8 and the mxfp4 KV cache in ONE process, alternated round by round after a warm-up, every timing ended by a device
    synchronise, `--rounds` runs of `--reps` steps per arm: the decode step of one model over the three caches — or, with --attention-only, the
    decode-attention launch pair over every layer's cache — at cache lengths prompt + 1 and prompt + new, with the pair's rate in TB/s of LIVE
    cache bytes (codes + exponents in the fp8 arm, nibbles + scale bytes in the mxfp4 arm).  The quantised caches hold the native cache's random
    rows, quantised.  Without --attention-only the run also times two `extend` calls over the native and the mxfp4 cache (_compare_extend).
    Every run is appended to `--out`."""
    from setok_amd import ops
    from setok_amd.generation import KVCache
    T, N = a.prompt, a.new
    llm = None if a.attention_only else _llm(a.layers, g, dev, dt)      # (the pair needs no model: one cache per layer, as a step has)
    res = {}
    for B in [int(b) for b in a.batches.split(",")]:
        native = KVCache(a.layers, B, H, T + N, DH, dt, dev)
        for t in native.k + native.v:
            t.normal_(0.0, 1.0, generator=g)
        _set_len(native, T)
        caches = {"native": native, "fp8": _fp8_twin(native), "mxfp4": _mxfp4_twin(native)}
        e1, q = rnd(B, D), rnd(B, 3 * D)
        out = torch.empty(B, H * DH, dtype=dt, device=dev)
        rb = dict(kv_cache_gb={k: round(c.nbytes() / 1e9, 3) for k, c in caches.items()})
        for length in (T + 1, T + N):
            def pair(k):
                c = caches[k]
                ws = c.workspace(H)
                return [c.attend(li, q, H, length, DH ** -0.5, ws, out) for li in range(a.layers)]

            def step(k):
                _set_len(caches[k], length - 1)
                return llm.model.decode_step(e1, caches[k])

            fn = pair if a.attention_only else step
            for c in caches.values():
                _set_len(c, length)                                      # (the pair reads the mask of `length` slots)
            for k in caches:
                _time(lambda: fn(k), 1)                                  # warm-up of both arms before the first timed round
            runs = {k: [] for k in caches}
            for _ in range(a.rounds):
                for k in caches:
                    runs[k].append(_time(lambda: fn(k), a.reps))
            r = {k: _spread(v) for k, v in runs.items()}
            r["fp8_over_native_median"] = round(r["fp8"]["median"] / r["native"]["median"], 3)
            r["faster_by_more_than_the_spread"] = r["fp8"]["max"] < r["native"]["min"]
            r["mxfp4_vs_native"], r["mxfp4_vs_fp8"] = _versus(r, "mxfp4", "native"), _versus(r, "mxfp4", "fp8")
            if a.attention_only:
                rows = 2.0 * a.layers * B * H * length                   # K and V rows the pair reads (Hkv = H)
                for k, per_row in (("native", DH * 2), ("fp8", DH + 1), ("mxfp4", DH // 2 + DH // 32)):
                    r[k]["live_cache_gb"] = round(rows * per_row / 1e9, 3)
                    r[k]["tb_per_s"] = round(rows * per_row / (r[k]["median"] * 1e-3) / 1e12, 3)
            rb[f"len{length}"] = r
        res[f"B{B}"] = rb
        del caches, native
        torch.cuda.empty_cache()
    what = "decode-attention launch pair (chunks + merge) over all layers' caches" if a.attention_only else "decode step"
    extend = None if a.attention_only else _compare_extend(a, llm, g, dev, dt, rnd)
    run = dict(workload=f"cfg5 LLM decode, Llama at Vicuna-7B dims, bf16: the KV cache native (bf16) against fp8 e4m3 rows + a power-of-two exponent "
                        f"per row and against MXFP4 rows (e2m1 nibbles + an e8m0 scale byte per 32 elements); ms per {what}, arms alternated in "
                        f"one process",
               measured="attention_pair" if a.attention_only else "decode_step", layers=a.layers, prompt=T, new_tokens=N, reps=a.reps, rounds=a.rounds,
               decode_chunk=dict(native=ops.DECODE_CHUNK, fp8=ops.DECODE_CHUNK_FP8KV, mxfp4=ops.DECODE_CHUNK_MXFP4KV),
               device=torch.cuda.get_device_name(0), results=res, peak_bytes=torch.cuda.max_memory_allocated())
    if extend is not None:
        run["extend_B1_ms"] = extend
    runs = []
    if os.path.isfile(a.out):
        with open(a.out) as f:
            runs = json.load(f)
    runs.append(run)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(runs, f, indent=1)
        f.write("\n")
    print(json.dumps(run))


def _compare_bands(a, g, dev, dt, rnd):
    """`linear_fp8w` at the four layer shapes with the band named through the floor of its rule (`min_wgs`; setok_linear_fp8w_wgs): 16, 32 and
    64 columns per workgroup where the row tiles allow them, and the library's own choice.  One process, the arms alternated round by round,
    every timing ended by a device synchronise, `--rounds` runs per arm.  The bits do not depend on the band; the time does."""
    from setok_amd import ops
    cdiv = lambda x, y: -(-x // y)
    out_ = {}
    for Nn, K in LAYER_SHAPES:
        copies = max(2, int(1.2e9 // (Nn * K)))              # 1.2 GB of q, visited round robin: the weights come from HBM
        qe = [ops.quantize_fp8_rows((torch.randn(Nn, K, generator=g, device=dev, dtype=torch.float32) * 0.02).to(dt)) for _ in range(copies)]
        for M in (32, 64):
            x = rnd(M, K)
            out = torch.empty(M, Nn, dtype=dt, device=dev)
            widest = 2 if M <= 32 else 4
            arms = {f"cols{16 * nt}": cdiv(Nn, 16 * nt) for nt in (1, 2, 4) if nt <= widest}      # the floor that this band just meets
            arms["library"] = None
            runs = {k: [] for k in arms}
            for _ in range(a.rounds):
                for k, floor in arms.items():
                    runs[k].append(_time(lambda: [ops.linear_fp8w(x, q, e, out=out, min_wgs=floor) for q, e in qe], a.reps) / copies)
            r = {k: dict(_spread(v), workgroups=arms[k]) for k, v in runs.items()}
            out_[f"N{Nn}_K{K}_M{M}"] = r
        del qe
    print(json.dumps(dict(
        workload="linear_fp8w, bf16, ms per call at the four layer shapes of Vicuna-7B (operands cycled through >= 1.2 GB): the columns a workgroup "
                 "owns, named through min_wgs, against the library's own rule (the widest band that leaves 256 workgroups)",
        reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0), gemm_ms=out_)))


def _bw(ms, live):
    tbs = live / (ms * 1e-3) / 1e12
    return dict(ms_all_layers=round(ms, 4), live_kv_gb=round(live / 1e9, 3), tb_per_s=round(tbs, 3), of_8_tb_per_s=round(tbs / 8.0, 3),
                of_layernorm_6p0_to_6p3=[round(tbs / 6.3, 3), round(tbs / 6.0, 3)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--batches", default="32,8,1")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--prompt", type=int, default=552)
    ap.add_argument("--new", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps-only", type=int, default=0)
    ap.add_argument("--attention-only", action="store_true")
    ap.add_argument("--gqa", type=int, default=4)
    ap.add_argument("--weights", choices=("native", "fp8", "mxfp4"), default="native")
    ap.add_argument("--compare-weights", action="store_true")
    ap.add_argument("--compare-bands", action="store_true")
    ap.add_argument("--compare-kv", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "generate_fp8kv_bench.json"),
                    help="--compare-kv appends its run to this JSON list")
    ap.add_argument("--weights-out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "generate_mxfp4_bench.json"),
                    help="--compare-weights appends its run to this JSON list")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    from setok_amd import ops

    dev, dt = "cuda:0", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float32).to(dt)
    T, N = a.prompt, a.new

    if a.compare_kv:
        _compare_kv(a, g, dev, dt, rnd)
        return

    if a.attention_only:                             # one GQA shape, K / V well past the 256 MiB the last cache level holds; two launches of the pair
        B, Hkv, n = 32, H // a.gqa, 4000
        k, v = rnd(B, Hkv, n, DH), rnd(B, Hkv, n, DH)
        q, mask = rnd(B, (H + 2 * Hkv) * DH), torch.ones(B, n, dtype=torch.uint8, device=dev)
        for _ in range(2):
            ops.attention_decode(q, k, v, mask, H, n, DH ** -0.5)
        torch.cuda.synchronize()
        print(json.dumps(dict(shape=dict(B=B, H=H, Hkv=Hkv, Dh=DH, len=n), launches_of_the_pair=2, live_kv_bytes_per_launch=2 * k.numel() * 2)))
        return

    if a.compare_weights:
        _compare_weights(a, g, dev, dt, rnd)
        return
    if a.compare_bands:
        _compare_bands(a, g, dev, dt, rnd)
        return

    llm = _llm(a.layers, g, dev, dt)
    if a.weights == "fp8":
        llm.quantize_fp8_()
    elif a.weights == "mxfp4":
        llm.quantize_mxfp4_()
    w_lm, w_e = llm.lm_head.weight.detach(), llm.model.embed_tokens.weight.detach()

    def token_step(c, h):
        tok = ops.argmax_rows(ops.linear(h, w_lm))
        e = ops.splice_rows(tok.to(torch.int32).reshape(-1, 1), w_e, None)
        return llm.model.decode_step(e.reshape(-1, D), c)

    if a.steps_only:
        B = a.batch
        c = _filled_cache(llm, B, T + N, T, g)
        h = rnd(B, D)
        for _ in range(a.steps_only):
            h = token_step(c, h)
        torch.cuda.synchronize()
        print(json.dumps(dict(batch=B, prompt=T, decode_steps=a.steps_only, layers=a.layers, weights=a.weights)))
        return

    res = {}
    for B in [int(b) for b in a.batches.split(",")]:
        grown = rnd(B, T + 1, D)
        am = torch.ones(B, T + 1, dtype=torch.bool, device=dev)
        t_old = _time(lambda: llm(inputs_embeds=grown, attention_mask=am, last_token_only=True), max(2, a.reps // 2))
        c = _filled_cache(llm, B, T + N, T, g)
        h, e1 = rnd(B, D), rnd(B, D)
        r = dict(ms_per_token_by_full_prefill=round(t_old, 3), kv_cache_gb=round(c.nbytes() / 1e9, 3))
        for tag, length in (("first", T), (f"token_{N}", T + N - 1)):
            def step(fn):
                _set_len(c, length)
                return fn()
            t_tok = _time(lambda: step(lambda: token_step(c, h)), a.reps)
            t_dec = _time(lambda: step(lambda: llm.model.decode_step(e1, c)), a.reps)
            ms_att, live = _attention_pair(c, rnd(B, 3 * D), length + 1, a.reps)
            r[tag] = dict(cache_len=length + 1, ms_per_token=round(t_tok, 3), ms_decode_step=round(t_dec, 3),
                          speedup_over_full_prefill=round(t_old / t_tok, 1), attention_pair=_bw(ms_att, live),
                          attention_share_of_decode_step=round(ms_att / t_dec, 3))
        del c
        torch.cuda.synchronize()
        e0, e9 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        prompt = grown[:, :T].contiguous()
        llm.generate(inputs_embeds=prompt, max_new_tokens=2)
        e0.record()
        seq = llm.generate(inputs_embeds=prompt, max_new_tokens=N)
        e9.record()
        torch.cuda.synchronize()
        t_prefill = _time(lambda: llm(inputs_embeds=prompt, last_token_only=True), 2)
        r["generate"] = dict(new_tokens=int(seq.shape[1]), ms_total=round(e0.elapsed_time(e9), 1), ms_prefill=round(t_prefill, 2),
                             ms_per_token_after_prefill=round((e0.elapsed_time(e9) - t_prefill) / max(1, seq.shape[1] - 1), 3))
        res[f"B{B}"] = r
        del grown, am, prompt
    print(json.dumps(dict(
        workload="cfg5 LLM decode: Llama at Vicuna-7B dims, bf16, greedy, KV cache of prompt + new slots; baseline = the prefill over the grown sequence",
        weights=a.weights, layers=a.layers, prompt=T, new_tokens=N, reps=a.reps, decode_chunk=ops.DECODE_CHUNK, results=res, peak_bytes=torch.cuda.max_memory_allocated())))


if __name__ == "__main__":
    main()
