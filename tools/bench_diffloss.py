"""DiffLoss.sample() at the sizes the reference implies (target_channels = z_channels = 4096, width 1024, depth 3, '100' steps): ms per call, per
step, launches per step, and where a step's time goes.

    python tools/bench_diffloss.py [--ms 1,32,64,256] [--dtypes bf16,fp32] [--reps 3] [--out profiles/diffloss_bench.json]
                                   [--split-m 32] [--stats-out profiles/diffloss_kernel_stats.csv]
    python tools/bench_diffloss.py --trace-only --m 32 --dtype bf16       # one warm-up call, a pause, one call: what a kernel trace is pointed at

Prints one JSON line (and writes it to --out).  Per (dtype, M): ms per sample() by HIP events, ms per step, the host's enqueue time per step (a
step that the host cannot enqueue faster than the device runs it is launch-bound), library launches per step counted at the ctypes boundary.
The floor beside it: the bytes of the weights one step reads (every Linear's matrix once) over the HBM rate — no step can be faster while the
weights come from memory.  With --split-m the tool starts `rocprofv3 --kernel-trace --stats` on a child process of its own (--trace-only) and reports
the measured call's split between GEMM kernels, the kernels of csrc/diffusion.hip (+ the SiLU launches), other kernels and the gaps between
dispatches; the per-kernel table goes to --stats-out."""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import shutil
import sqlite3
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C, Z, W, DEPTH, STEPS = 4096, 4096, 1024, 3, "100"
HBM_TB_S = 8.0                       # HBM3E peak of the MI355X; the streaming kernels of this library reach 6.0-6.3
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
OURS = ("timestep_embedding_kernel", "add_silu_kernel", "adaln_modulate_kernel", "ddpm_step_kernel", "activation_kernel")


def _head(dt, dev, steps=STEPS):
    from setok_amd import DiffLoss
    g = torch.Generator().manual_seed(0)
    dl = DiffLoss(target_channels=C, z_channels=Z, depth=DEPTH, width=W, num_sampling_steps=steps)
    for p in dl.parameters():                     # no zero layer (the reference's initialisation zeroes the adaLN and output layers), small enough to stay finite
        p.data.normal_(0.0, 0.02, generator=g)
    return dl.to(dev).to(dt).eval().requires_grad_(False)


def _weight_bytes_per_step(dl):
    net = dl.net
    lins = [net.input_proj, net.final_layer.linear, net.final_layer.adaLN_modulation[1]]
    for b in net.res_blocks:
        lins += [b.mlp[0], b.mlp[2], b.adaLN_modulation[1]]
    return sum(l.weight.numel() * l.weight.element_size() for l in lins)


def _measure(dl, M, reps, dev):
    from setok_amd import _lib
    steps = dl.num_sampling_steps
    g = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(M, Z, generator=g, device=dev)
    noise = torch.randn(1 + steps, M, C, generator=g, device=dev)
    dl.sample(z, noise=noise)                                        # warm-up: packs the weights
    torch.cuda.synchronize()
    calls, orig = [0], _lib.call

    def counting(name, *a, **k):
        calls[0] += 1
        return orig(name, *a, **k)
    _lib.call = counting
    try:
        dl.sample(z, noise=noise)
    finally:
        _lib.call = orig
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host = 0.0
    e0.record()
    for _ in range(reps):
        t0 = time.perf_counter()
        out = dl.sample(z, noise=noise)
        host += time.perf_counter() - t0
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    per_step_calls = (calls[0] - 5) / steps                         # 5 calls per sample() embed z and the timesteps; the rest is the loop
    return dict(ms_per_sample=round(ms, 3), ms_per_step=round(ms / steps, 4), host_enqueue_ms_per_step=round(host / reps / steps * 1e3, 4),
                library_calls_per_sample=calls[0], launches_per_step=per_step_calls, finite=bool(torch.isfinite(out).all()))


def _trace_only(a):
    dev = "cuda:0"
    dl = _head(DT[a.dtype], dev)
    g = torch.Generator(device=dev).manual_seed(1)
    z = torch.randn(a.m, Z, generator=g, device=dev)
    noise = torch.randn(1 + dl.num_sampling_steps, a.m, C, generator=g, device=dev)
    dl.sample(z, noise=noise)
    torch.cuda.synchronize()
    time.sleep(0.3)                                                  # an idle stretch no dispatch gap comes near: the trace is cut here
    dl.sample(z, noise=noise)
    torch.cuda.synchronize()
    print(json.dumps(dict(traced="one sample() after the pause", m=a.m, dtype=a.dtype)))


def _split(a):
    """rocprofv3 on a child (--trace-only); the kernels after the last long idle stretch are the measured call."""
    if not shutil.which("rocprofv3"):
        return dict(error="rocprofv3 is not on PATH")
    tmp = tempfile.mkdtemp(prefix="diffloss_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--trace-only",
               "--m", str(a.split_m), "--dtype", a.split_dtype]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if r.returncode != 0 or not dbs:
            return dict(error=f"rocprofv3 exited {r.returncode}, {len(dbs)} result databases", stderr=r.stderr[-400:])
        con = sqlite3.connect(dbs[0])
        cols = [c[1] for c in con.execute("pragma table_info(kernels)")]
        name_col = "name" if "name" in cols else [c for c in cols if "name" in c][0]
        rows = con.execute(f"select {name_col}, start, end from kernels order by start").fetchall()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    cut = max((i for i in range(1, len(rows)) if rows[i][1] - rows[i - 1][2] > 100e6), default=0)
    rows = rows[cut:]
    span = rows[-1][2] - rows[0][1]
    kind = lambda n: "gemm" if "gemm" in n else ("diffusion" if any(k in n for k in OURS) else "other")
    tot, per = {"gemm": 0, "diffusion": 0, "other": 0}, {}
    for n, s, e in rows:
        tot[kind(n)] += e - s
        short = re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", ""))[:90]
        c = per.setdefault(short, [0, 0, 1 << 62, 0])
        c[0] += 1; c[1] += e - s; c[2] = min(c[2], e - s); c[3] = max(c[3], e - s)
    busy = sum(tot.values())
    if a.stats_out:
        lines = ["kernel,calls,total_ms,avg_us,min_us,max_us,share"]
        for n, (cnt, t, mn, mx) in sorted(per.items(), key=lambda kv: -kv[1][1]):
            lines.append(f"\"{n}\",{cnt},{t / 1e6:.3f},{t / cnt / 1e3:.2f},{mn / 1e3:.2f},{mx / 1e3:.2f},{t / busy:.4f}")
        lines.append(f"\"TOTAL\",{len(rows)},{busy / 1e6:.3f},,,,1.0")
        with open(a.stats_out, "w") as f:
            f.write("\n".join(lines) + "\n")
    ms = lambda v: round(v / 1e6, 3)
    return dict(m=a.split_m, dtype=a.split_dtype, kernels=len(rows), span_ms=ms(span), gemm_ms=ms(tot["gemm"]), diffusion_kernels_ms=ms(tot["diffusion"]),
                other_kernels_ms=ms(tot["other"]), gaps_ms=ms(span - busy), share=dict(gemm=round(tot["gemm"] / span, 3), diffusion_kernels=round(tot["diffusion"] / span, 3),
                                                                                        other=round(tot["other"] / span, 3), gaps=round((span - busy) / span, 3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ms", default="1,32,64,256")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--split-m", type=int, default=0)
    ap.add_argument("--split-dtype", default="bf16")
    ap.add_argument("--stats-out", default="")
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--dtype", default="bf16")
    a = ap.parse_args()
    if a.trace_only:
        return _trace_only(a)
    dev, res, floor = "cuda:0", {}, {}
    for name in a.dtypes.split(","):
        dl = _head(DT[name], dev)
        wb = _weight_bytes_per_step(dl)
        floor[name] = dict(weight_bytes_per_step=wb, floor_ms_per_step_at_hbm_peak=round(wb / (HBM_TB_S * 1e12) * 1e3, 5))
        for M in [int(m) for m in a.ms.split(",")]:
            res[f"{name}_M{M}"] = _measure(dl, M, a.reps, dev)
        del dl
        torch.cuda.empty_cache()
    doc = dict(workload=f"DiffLoss.sample: target_channels={C}, z_channels={Z}, width={W}, depth={DEPTH}, '{STEPS}' steps, cfg=1, recorded noise",
               device=torch.cuda.get_device_name(0), device_arch=torch.cuda.get_device_properties(0).gcnArchName, compute_units=torch.cuda.get_device_properties(0).multi_processor_count, hbm_tb_per_s_assumed=HBM_TB_S, reps=a.reps, floor=floor, results=res)
    if a.split_m:
        doc["kernel_split"] = _split(a)
    line = json.dumps(doc)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
