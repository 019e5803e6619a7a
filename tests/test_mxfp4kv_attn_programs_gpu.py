"""The attention kernels over the MXFP4 KV cache where their running maximum, their wave combine and their chunk merge must work: the score programs
of tests/attn_programs.py through setok_attention_decode_gqa_mxfp4kv — attn_decode_kernel over KvMxfp4 at 2, 4 and 8 lanes per row and 1, 2, 4 and 8
query heads per workgroup, and the generic wave-per-chunk kernel at head dim 96 — and through setok_attention_extend_gqa_mxfp4kv (the generic kernel,
causal), against fp64 over the dequantised cache K', V'.  tests/test_mxfp4kv_gpu.py draws Gaussian rows and a random q: nothing there moves a wave's
maximum by 8 nats, and its dead slots never hold a finite key that would win.

Every offset a program writes into k[:, 0] is one an MX block carries exactly (0, +-8 .. +-32, 16 and -64: tests/test_mxfp4kv_paged_attn_programs_cpu.py),
so the stairs are stairs of K' and climb through the scale byte of block 0; the other 31 values of that block flush towards 0, which the reference,
taken over K', shares.  Dead slots keep nibble bytes 0xFF under scale bytes 0xFF / 0x00; a dead slot that a `hot@` program heats holds the finite
nibbles and scale bytes of its K row under a V row whose scale bytes are 0xFF.

Every case asserts finite outputs, the global AND the worst per-row max-rel error below the bound, equal bits on a second run, and exact zeros in
the rows that can count no key.  The bound is the project's own: in 16 bits `_tol` (1e-2 at head dim 128, 2e-2 below it), in fp32 four times the
error of torch's fp32 evaluation of the same formula against fp64, floored at 3e-6 (`_bounds32`).  The decode cases also run the native kernel on
K', V' cast to the element type (exact) against the same reference.  Every figure goes to SETOK_PARITY_LOG
(profiles/mxfp4kv_paged_attn_programs_parity.txt).  `pytest -m gpu`."""
import pytest
import torch

import attn_programs as AP
import mxfp4_cases as M
import mxfp4kv_cases as K
import test_cache_attn_programs_gpu as G
from test_attn_programs_gpu import NAME, _Cases, _bounds32, _decode_ref32
from test_extend_gpu import _extend_ref, _tol
from test_generate_gpu import _decode_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops

DEV = "cuda"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
CH = K.define("SETOK_DECODE_CHUNK_MXFP4KV")         # slots per partial of the decode kernel; a wave's slice is a quarter of it
XC = K.define("SETOK_EXTEND_CHUNK")


def label(program, tile):
    return program if program.startswith(("hot@", "shift")) else f"{program}/{tile}"


# ---- decode --------------------------------------------------------------------------------------------------------------------------------------
MX_SHAPES = [(128, 8, 1), (64, 4, 2), (32, 2, 2), (32, 4, 1), (96, 4, 2)]       # (Dh, H, Hkv): 8 / 4 / 2 lanes per row; GT = 8, 2, 1, 4; the generic kernel
MX_LENS = (CH + 1, 1000)


def mx_walk(Dh):
    """(slots per partial, keys per wave slice) of setok_attention_decode_gqa_mxfp4kv: the generic kernel runs one softmax per chunk."""
    return CH, (CH // 4 if Dh in (32, 64, 128) else CH)


def mx_programs(n):
    """Stairs at the wave slice (the combine in LDS; two chunks: five levels) and at the chunk (the merge; four chunks); a hot key on either side of a
    slice edge and of a chunk edge, in the last live slot, in a slot the left-padded sequence masks and in slot n."""
    tile = CH // 4 if n == CH + 1 else CH
    return G._programs_with_hot([("stair8", tile), ("down8", tile)], [63, 64, CH - 1, CH, n - 1, n // 3 - 1, n])


def mx_problem(dt, Dh, H, Hkv, n, program, tile, seed):
    """mxfp4kv_cases.decode_problem's four sequences (all keys, left-padded, right-padded, fully masked) with K steered: build_cache's rows through the
    oracle quantiser, V the module's `cache_rows`.  Returns (qkv, k_q, k_s, v_q, v_s, mask)."""
    B, cap, Gq = 4, n + 5, H // Hkv
    qkv, k_q, k_s, v_q, v_s, mask = K.decode_problem(dt, H, Hkv, Dh, n, cap, seed)
    qkv, kf = qkv.float(), torch.empty(B, Hkv, cap, Dh)
    for b in range(B):
        for j in range(Hkv):
            q, kf[b, j], _ = AP.build_cache(1, cap, Dh, Gq, program, seed + 100 * b + j, tile)
            qkv.reshape(B, H + 2 * Hkv, Dh)[b, j * Gq:(j + 1) * Gq] = q[0]
    nq, ns = K.quantize_cache(kf)
    dead = mask == 0
    dead[:, n:] = True
    if program.startswith("hot@"):
        p = AP.hot_key(program, cap)
        v_s[:, :, p] = torch.where(dead[:, None, p, None], torch.full_like(v_s[:, :, p], M.NAN_SCALE), v_s[:, :, p])      # a heated dead slot: V stays NaN
        dead[:, p] = False
    dead = dead[:, None, :, None].expand(B, Hkv, cap, 1)
    return qkv.to(dt), torch.where(dead, k_q, nq), torch.where(dead, k_s, ns), v_q, v_s, mask


@pytest.mark.parametrize("dt", [F32, BF, HF], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("Dh,H,Hkv", MX_SHAPES)
@pytest.mark.parametrize("n", MX_LENS)
def test_mxfp4_cache_and_native_decode_programs(dt, Dh, H, Hkv, n):
    """The reference is fp64 over the dequantised cache K', V', which every element type holds exactly: the native kernel runs on those."""
    cases = _Cases()
    for program, tile in mx_programs(n):
        qkv, k_q, k_s, v_q, v_s, mask = mx_problem(dt, Dh, H, Hkv, n, program, tile, seed=700 + n)
        kd, vd = K.dequant(k_q, k_s), K.dequant(v_q, v_s)
        ref = _decode_ref(qkv, kd, vd, mask, H, Hkv, Dh, n)
        bound = (_tol(dt, Dh),) * 2 if dt != F32 else _bounds32(_decode_ref32(qkv, kd, vd, mask, H, Hkv, Dh, n), ref, Dh)
        dq, dm = qkv.to(DEV), mask.to(DEV)
        codes = [t.to(DEV) for t in (k_q, k_s, v_q, v_s)]
        kn, vn = kd.to(dt).to(DEV), vd.to(dt).to(DEV)
        for kernel, run in (("mxfp4kv", lambda: ops.attention_decode_mxfp4kv(dq, *codes, dm, H, n, Dh ** -0.5)),
                            ("native", lambda: ops.attention_decode(dq, kn, vn, dm, H, n, Dh ** -0.5))):
            got = run()
            name = f"decode {kernel} {NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len={n} {label(program, tile)}"
            cases.check(name, got, ref, Dh, *bound)
            cases.same_bits(name + " second run", run(), got)
            if G._not_zero(got, 3):
                cases.bad.append(f"{name}: the fully masked sequence is not zero")
    cases.done()


# ---- extend --------------------------------------------------------------------------------------------------------------------------------------
# (dt, Dh, H, Hkv, Tn, len0): one wave per (query row, query head, chunk) whatever the type and head dim.  Two chunks with one slot and with nine in
# the second, five chunks; G = 8, 1 and 2.  fp32 at one shape per head dim.
_MX_EXTEND = [(128, 8, 1, 4, XC - 3), (128, 8, 1, 17, XC - 8), (128, 2, 2, 40, 1000), (32, 4, 2, 7, 1000), (32, 4, 2, 17, XC - 8)]
MX_EXTEND_CASES = [(dt,) + c for dt in (BF, HF) for c in _MX_EXTEND] + [(F32,) + _MX_EXTEND[0], (F32,) + _MX_EXTEND[4]]


def mx_extend_programs(dt, Dh, H, Hkv, Tn, len0):
    """Stairs per chunk (at most five levels), the level shift an MX block carries, and the hot slots of the dense module's extend_programs."""
    hot = [(p, t) for p, t in G.extend_programs(dt, Dh, H, Hkv, Tn, len0) if p.startswith("hot@")]
    return [("stair8", XC), ("down8", XC), ("shift-64", XC)] + hot


def mx_extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile, mask, seed):
    """extend_problem of the dense module with k and v through the oracle quantiser (a NaN row becomes 0xFF blocks): (q, k_q, k_s, v_q, v_s)."""
    q, k, v = G.extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile, mask, seed)
    return (q,) + K.quantize_cache(k) + K.quantize_cache(v)


@pytest.mark.parametrize("case", MX_EXTEND_CASES, ids=G._case_id)
def test_mxfp4_cache_extend_programs(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    mask, counts = G.extend_mask(*case)
    blind = ~counts.any(-1).reshape(-1)                                # (4 * Tn) rows that can count no key: the fully masked sequence, and more
    assert int(blind.sum()) > Tn
    cases = _Cases()
    for program, tile in mx_extend_programs(*case):
        q, k_q, k_s, v_q, v_s = mx_extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile, mask, seed=len0 + Tn)
        kd, vd = K.dequant(k_q, k_s), K.dequant(v_q, v_s)
        ref = _extend_ref(q, kd, vd, mask, H, Hkv, Dh, len0, Tn)
        bound = (_tol(dt, Dh),) * 2 if dt != F32 else _bounds32(G._extend_ref32(q, kd, vd, mask, H, Hkv, Dh, len0, Tn), ref, Dh)
        args = (q.to(DEV), k_q.to(DEV), k_s.to(DEV), v_q.to(DEV), v_s.to(DEV), mask.to(DEV), H, Tn, len0, Dh ** -0.5)
        got = ops.attention_extend_mxfp4kv(*args)
        name = f"extend mxfp4kv {NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len0={len0} Tn={Tn} {label(program, tile)}"
        cases.check(name, got, ref, Dh, *bound)
        cases.same_bits(name + " second run", ops.attention_extend_mxfp4kv(*args), got)
        if G._not_zero(got, blind):
            cases.bad.append(f"{name}: rows that can count no key are not zero")
    cases.done()
