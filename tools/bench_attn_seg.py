#!/usr/bin/env python
"""Micro-benchmark of the head's 2 x 512 attention over long segments (attn_seg_big_kernel): the inter encoder's shape, one segment of L
cluster tokens per image.  python tools/bench_attn_seg.py [images [L]]   (default 256 images of 96 tokens; L > 32 or the small kernel runs)"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from setok_amd import ops
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
L = int(sys.argv[2]) if len(sys.argv) > 2 else 96
H, Dh = 2, 512
qkv = (torch.randn(B * L, 3 * H * Dh, device="cuda") * 0.5).bfloat16()
offs = torch.arange(0, (B + 1) * L, L, dtype=torch.int32, device="cuda")
out = torch.empty(B * L, H * Dh, device="cuda", dtype=torch.bfloat16)
run = lambda: ops.attention(qkv, H, Dh, Dh ** -0.5, seg_len=L, seg_offsets=offs, n_segs=B, out=out)
for _ in range(3):
    run()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(20):
    run()
e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / 20
print(f"attn_seg Dh={Dh} H={H} L={L} B={B}: {ms*1e3:.1f} us  {4.0 * B * H * L * L * Dh / ms / 1e9:.1f} TFLOP/s")
