"""The kernels that attend over a KV cache where their running maximum, their wave combine and their chunk merge must work: the score programs of
tests/attn_programs.py through setok_attention_extend_gqa — its one-wave and four-wave MFMA kernels and the generic wave-per-chunk kernel
(attn_extend.hip, attn_partials.h) — and through attn_decode_kernel over the fp8 cache and over the native one (attn_decode.hip), against fp64.
tests/test_extend_gpu.py and tests/test_fp8kv_gpu.py draw unit-variance scores, under which no rescale inside a span goes below e^-2.1 and no merge
factor below e^-4.6 (tests/test_cache_attn_programs_cpu.py); here the stairs put e^-8 at every 32-key tile, at every chunk and at every span, a hot
key sits 16 nats up on either side of each edge, on the diagonal inside a tile (where the rows of one wave disagree about it), and — as a finite K row
whose V row stays NaN — in a hole of the mask and in the slot just past the end.  On the fp8 cache the stairs move the row's exponent byte.

Every case asserts finite outputs, the global AND the worst per-row max-rel error (max_d |err| / max_d |ref| of one query's output in one head) below
the bound, equal bits on a second run, and exact zeros in the rows that can count no key.  The bound is the project's own: in 16 bits `_tol` (1e-2 at
head dim 128, 2e-2 below it), in fp32 four times the error of torch's fp32 evaluation of the same formula against fp64, floored at 3e-6
(`_bounds32`).  Every figure goes to SETOK_PARITY_LOG (profiles/cache_attn_programs_parity.txt).  `pytest -m gpu`."""
import pytest
import torch

import attn_programs as AP
import fp8_cases as F
from test_attn_programs_gpu import NAME, _Cases, _bounds32, _decode_ref32
from test_extend_gpu import CH, SP, _extend_problem, _extend_ref, _tol
from test_fp8kv_gpu import CHUNK as CHUNK8, _dequant, _fp8_problem
from test_generate_gpu import CHUNK as CHUNKN, _decode_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops

DEV = "cuda"
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
NAN = float("nan")


def _programs_with_hot(stairs, slots):
    """[(program, stair tile)]: the stairs, then one `hot@slot` per slot, each slot once, in the order given."""
    return stairs + [(f"hot@{p}", 32) for p in dict.fromkeys(slots)]


def _label(program, tile):
    return program if program.startswith("hot@") or program == "shift-60" else f"{program}/{tile}"


# ---- extend --------------------------------------------------------------------------------------------------------------------------------------
# (dt, Dh, H, Hkv, Tn, len0).  Head dim 128 in 16 bits: G * Tn = 32 (exactly one wave of stacked rows) and 14 on the one-wave kernel, two chunks
# each; 136 rows on the four-wave kernel inside one span, across the span edge (its wave of queries 12 .. 15 ends below SP: the second span lies above
# its rows, next to a wave that reaches into it), and G = 1.  Everything else is the generic kernel: one chunk edge, four chunks.
EXTEND_CASES = [(dt, 128, H, Hkv, Tn, len0) for dt in (BF, HF) for H, Hkv, Tn in ((8, 1, 4), (4, 2, 7)) for len0 in (CH - 3, 300)]
EXTEND_CASES += [(dt, 128) + rest for dt in (BF, HF) for rest in ((8, 1, 17, CH - 8), (8, 1, 17, SP - 8), (2, 2, 40, 1000))]
EXTEND_CASES += [(dt, Dh, 4, 2, Tn, len0) for dt, Dh in ((F32, 16), (BF, 64), (HF, 40)) for Tn, len0 in ((17, CH - 8), (7, 1000))]


def _case_id(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    return f"{NAME[dt]}-Dh{Dh}-H{H}-Hkv{Hkv}-Tn{Tn}-len{len0}"


def extend_walk(dt, Dh, H, Hkv, Tn):
    """(slots per partial, keys per online-softmax step) of the path a call takes: extend_span() of attn_extend.hip."""
    if dt != F32 and Dh == 128:
        return (SP if (H // Hkv) * Tn > 32 else CH), 32
    return CH, CH


def extend_programs(dt, Dh, H, Hkv, Tn, len0):
    span, tile = extend_walk(dt, Dh, H, Hkv, Tn)
    n = len0 + Tn
    tiles = ([32] if tile == 32 else []) + [CH] + ([SP] if span == SP else [])
    assert n <= SP + 64                                                # the tile-32 stairs stay at or below 272 nats
    stairs = [(p, t) for t in tiles for p in ("stair8", "down8")] + [("shift-60", 32)]
    # len0 + Tn // 2 is the hole of sequence 1 and, in the others, a key that only the rows at or after it may count; slot n lies past the end
    slots = [p for p in (len0 - 1, len0, len0 + Tn // 2, CH - 1, CH, SP - 1, SP) if 0 <= p < n] + [n]
    return _programs_with_hot(stairs, slots)


def extend_mask(dt, Dh, H, Hkv, Tn, len0):
    """(mask (4, cap) of _extend_problem's four sequences — whole; left-padded with a hole in the new chunk; every old slot masked, with holes; fully
    masked —, counts (4, Tn, n): query i of sequence b counts slot j)."""
    n = len0 + Tn
    mask = _extend_problem(dt, H, Hkv, Dh, len0, Tn, n + 5, seed=0)[3]
    assert Tn < 3 or int(mask[1, len0 + Tn // 2]) == 0
    counts = mask[:, None, :n].bool() & (torch.arange(n)[None, :] <= len0 + torch.arange(Tn)[:, None])[None]
    return mask, counts


def extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile, mask, seed):
    """(q (4 * Tn, H * Dh), k, v (4, Hkv, cap, Dh)) in `dt`: every (sequence, key / value head) its own draw of the program.  NaN sits in every slot
    that counts for nobody; the slot a `hot@` program heats keeps, where it is such a slot, its finite K row (k[0] = 16) over a NaN V row."""
    B, n, G = 4, len0 + Tn, H // Hkv
    cap = mask.shape[1]
    q, k, v = torch.empty(B, Tn, Hkv, G, Dh), torch.empty(B, Hkv, cap, Dh), torch.empty(B, Hkv, cap, Dh)
    for b in range(B):
        for j in range(Hkv):
            q[b, :, j], k[b, j], v[b, j] = AP.build_cache(Tn, cap, Dh, G, program, seed + 100 * b + j, tile)
    dead = mask == 0
    dead[:, n:] = True
    dead_k = dead.clone()
    if program.startswith("hot@"):
        dead_k[:, AP.hot_key(program, cap)] = False
    k, v = k.masked_fill(dead_k[:, None, :, None], NAN), v.masked_fill(dead[:, None, :, None], NAN)
    return q.reshape(B * Tn, H * Dh).to(dt), k.to(dt), v.to(dt)


def _extend_ref32(q, k, v, mask, H, Hkv, Dh, len0, Tn):
    """test_extend_gpu._extend_ref's formula in torch fp32 on the CPU: the yardstick of the fp32 bound."""
    B, n = k.shape[0], len0 + Tn
    qq = q[:, :H * Dh].float().reshape(B, Tn, H, Dh)
    kk = k[:, :, :n].float().nan_to_num(0.0).repeat_interleave(H // Hkv, dim=1)
    vv = v[:, :, :n].float().nan_to_num(0.0).repeat_interleave(H // Hkv, dim=1)
    s = torch.einsum("bihd,bhjd->bhij", qq, kk) * Dh ** -0.5
    counts = mask[:, None, None, :n].bool() & (torch.arange(n)[None, :] <= len0 + torch.arange(Tn)[:, None])[None, None]
    p = torch.softmax(s.masked_fill(~counts, float("-inf")), -1).nan_to_num(0.0)
    return torch.einsum("bhij,bhjd->bihd", p, vv).reshape(B * Tn, H * Dh)


def _not_zero(got, rows):
    """True unless every element of the chosen rows is an exact zero (a NaN is not)."""
    return float(got.detach().cpu()[rows].float().abs().max()) != 0.0


@pytest.mark.parametrize("case", EXTEND_CASES, ids=_case_id)
def test_extend_attention_programs(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    mask, counts = extend_mask(*case)
    blind = ~counts.any(-1).reshape(-1)                                # (4 * Tn) rows that can count no key: the fully masked sequence, and more
    assert int(blind.sum()) > Tn
    cases = _Cases()
    for program, tile in extend_programs(*case):
        q, k, v = extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile, mask, seed=len0 + Tn)
        ref = _extend_ref(q, k, v, mask, H, Hkv, Dh, len0, Tn)
        bound = (_tol(dt, Dh),) * 2 if dt != F32 else _bounds32(_extend_ref32(q, k, v, mask, H, Hkv, Dh, len0, Tn), ref, Dh)
        args = (q.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV), H, Tn, len0, Dh ** -0.5)
        got = ops.attention_extend(*args)
        label = f"extend {NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len0={len0} Tn={Tn} {_label(program, tile)}"
        cases.check(label, got, ref, Dh, *bound)
        cases.same_bits(label + " second run", ops.attention_extend(*args), got)
        if _not_zero(got, blind):
            cases.bad.append(f"{label}: rows that can count no key are not zero")
    cases.done()


# ---- decode over the fp8 cache, and the native kernel over the same K', V' ---------------------------------------------------------------------------
FP8_SHAPES = [(128, 8, 1), (64, 4, 2), (32, 2, 2), (16, 4, 1), (40, 4, 2)]       # (Dh, H, Hkv): GT = 8, 2, 1, 4 query heads per workgroup; the generic path
FP8_LENS = (CHUNK8 + 1, 1000)


def fp8_walk(Dh):
    """(slots per partial, keys per wave slice) of setok_attention_decode_gqa_fp8kv: the generic kernel runs one softmax per chunk."""
    return CHUNK8, (CHUNK8 // 4 if Dh in (16, 32, 64, 128) else CHUNK8)


def native_walk(dt, Dh):
    lpr = Dh // (4 if dt == F32 else 8)
    return CHUNKN, (CHUNKN // 4 if Dh % (4 if dt == F32 else 8) == 0 and lpr in (2, 4, 8, 16, 32) else CHUNKN)


def fp8_programs(n):
    """Stairs at the wave slice (the combine in LDS; two chunks) and at the chunk (the merge; four chunks); a hot key on either side of a slice edge and
    of a chunk edge, in the last live slot, in a slot the left-padded sequence masks and in slot n."""
    tile = CHUNK8 // 4 if n == CHUNK8 + 1 else CHUNK8
    return _programs_with_hot([("stair8", tile), ("down8", tile)], [63, 64, CHUNK8 - 1, CHUNK8, n - 1, n // 3 - 1, n])


def fp8_problem(dt, Dh, H, Hkv, n, program, tile, seed):
    """_fp8_problem's four sequences (all keys, left-padded, right-padded, fully masked) with K steered: build_cache's rows quantised by the CPU
    oracle, V its `_cache_rows`.  Dead slots hold the NaN code and exponent bytes 127 / -128; a dead slot that a `hot@` program heats holds the
    finite codes and the exponent of its K row (its V row stays the NaN code).  Also returns the fp32 K rows before quantisation."""
    B, cap, G = 4, n + 5, H // Hkv
    qkv, k_q, k_e, v_q, v_e, mask = _fp8_problem(dt, H, Hkv, Dh, n, cap, seed)
    qkv, kf = qkv.float(), torch.empty(B, Hkv, cap, Dh)
    for b in range(B):
        for j in range(Hkv):
            q, kf[b, j], _ = AP.build_cache(1, cap, Dh, G, program, seed + 100 * b + j, tile)
            qkv.reshape(B, H + 2 * Hkv, Dh)[b, j * G:(j + 1) * G] = q[0]
    nq, ne = F.quantize_rows(kf.reshape(-1, Dh))
    dead = mask == 0
    dead[:, n:] = True
    if program.startswith("hot@"):
        dead[:, AP.hot_key(program, cap)] = False
    dead = dead[:, None].expand(B, Hkv, cap)
    k_q = torch.where(dead[..., None], k_q, nq.reshape(B, Hkv, cap, Dh))
    k_e = torch.where(dead, k_e, ne.reshape(B, Hkv, cap))
    return qkv.to(dt), k_q, k_e, v_q, v_e, mask, kf


@pytest.mark.parametrize("dt", [F32, BF, HF], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("Dh,H,Hkv", FP8_SHAPES)
@pytest.mark.parametrize("n", FP8_LENS)
def test_fp8_cache_and_native_decode_programs(dt, Dh, H, Hkv, n):
    """The reference is fp64 over the dequantised cache K', V', which every element type holds exactly: the native kernel runs on those."""
    cases = _Cases()
    for program, tile in fp8_programs(n):
        qkv, k_q, k_e, v_q, v_e, mask, _ = fp8_problem(dt, Dh, H, Hkv, n, program, tile, seed=600 + n)
        kd, vd = _dequant(k_q, k_e), _dequant(v_q, v_e)
        ref = _decode_ref(qkv, kd, vd, mask, H, Hkv, Dh, n)
        bound = (_tol(dt, Dh),) * 2 if dt != F32 else _bounds32(_decode_ref32(qkv, kd, vd, mask, H, Hkv, Dh, n), ref, Dh)
        dq, dm = qkv.to(DEV), mask.to(DEV)
        codes = [t.to(DEV) for t in (k_q, k_e, v_q, v_e)]
        kn, vn = kd.to(dt).to(DEV), vd.to(dt).to(DEV)
        for kernel, run in (("fp8kv", lambda: ops.attention_decode_fp8kv(dq, *codes, dm, H, n, Dh ** -0.5)),
                            ("native", lambda: ops.attention_decode(dq, kn, vn, dm, H, n, Dh ** -0.5))):
            got = run()
            label = f"decode {kernel} {NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len={n} {_label(program, tile)}"
            cases.check(label, got, ref, Dh, *bound)
            cases.same_bits(label + " second run", run(), got)
            if _not_zero(got, 3):
                cases.bad.append(f"{label}: the fully masked sequence is not zero")
    cases.done()
