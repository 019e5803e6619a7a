"""The online-softmax attention kernels where the running maximum must move: the score programs of tests/attn_programs.py (stairs that force a
rescale at every tile, at every second tile, or never; one hot key on a tile edge, in the short tail form, behind a mask; a shifted score level;
one steered row in a wave of flat ones) through every kernel that keeps a running maximum — the ViT tower's deferred-maximum kernel and its
cross-attention form (attn_vit.hip), the causal prefill (llama.hip), the decode kernel's chunk merge (attn_decode.hip) and the head-dim-512 segment
kernel (attn_seg.hip) — against fp64.  Unit-variance inputs never raise the deferred maximum after the first key tile
(tests/test_attn_programs_cpu.py), so none of this ran before.

Every case asserts finite outputs, the global max-rel error AND the worst per-row max-rel error (max_d |err| / max_d |ref| of each output row)
below the bound, and equal bits on a second run.  The bound is the project's 16-bit attention bar, 1e-2; for fp32 kernels it is four times the error
of torch's own fp32 evaluation of the same formula against fp64 (a different summation order), floored at the existing 3e-6: one fp32 ulp of a
score of 50 nats is already 4e-6 in the probability.  Every measured figure goes to SETOK_PARITY_LOG (profiles/attn_programs_parity.txt).

The backward kernels are in tests/test_attn_bwd_programs_gpu.py: the same programs plus pairs of hot keys, against a reference that takes the
rounded `out` as given (D = dO . out) and an error-scale bound per output row (tests/attn_bwd_programs.py; shown attainable and sharp on the CPU in
tests/test_attn_bwd_programs_cpu.py).  The extend kernels and the decode kernel over the fp8 cache are in tests/test_cache_attn_programs_gpu.py.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import attn_programs as AP
from test_generate_gpu import CHUNK, _decode_problem, _decode_ref, _log
from test_llama_gpu import _causal_ref_gqa
from test_ops_gpu import _attn_ref, _cross_ref, _with_env

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops

DEV = "cuda"
BOUND16 = 1e-2
FLOOR32 = 3e-6
LOW = [torch.bfloat16, torch.float16]
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}


class _Cases:
    """Collects the figures of a test's cases, logs each, and fails at the end naming every case over its bound: one slow case does not hide the next."""

    def __init__(self):
        self.bad = []

    def check(self, label, got, ref, Dh, bound=BOUND16, bound_rows=None):
        got = got.detach().cpu()
        glob, rows = AP.errors(got.reshape(-1, Dh), ref.reshape(-1, Dh))                 # a row: one query's output in one head
        bound_rows = bound if bound_rows is None else bound_rows
        _log(label + ": global, per-row, their bounds", glob, rows, bound, bound_rows)
        if not bool(torch.isfinite(got.float()).all()):
            self.bad.append(f"{label}: not finite")
        elif not (glob < bound and rows < bound_rows):
            self.bad.append(f"{label}: global {glob:.3e} (bound {bound:.1e}) per-row {rows:.3e} (bound {bound_rows:.1e})")

    def same_bits(self, label, a, b):
        if not torch.equal(a, b):
            self.bad.append(f"{label}: bits differ")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _bounds32(ref32, ref, Dh):
    glob, rows = AP.errors(ref32.reshape(-1, Dh), ref.reshape(-1, Dh))
    return max(4 * glob, FLOOR32), max(4 * rows, FLOOR32)


def _fused_qkv(T, Dh, H, B, program, dt, seed):
    """(B * T, 3 * H * Dh) rows [q | k | v], every (image, head) its own draw of the program."""
    parts = [[AP.build(T, Dh, program, seed + 1000 * b + h) for h in range(H)] for b in range(B)]
    qkv = torch.stack([torch.stack([torch.stack([parts[b][h][i] for h in range(H)], 1) for i in range(3)], 1) for b in range(B)])   # B, T, 3, H, Dh
    return qkv.reshape(B * T, 3 * H * Dh).to(dt)


# ---- dense self-attention: attn_vit_kernel ------------------------------------------------------------------------------------------------
#   T = 65: one wave, three key tiles, a 1-key short tail; 200: an 8-key short tail; 201: 9 keys, the general tail; 257: 8 waves + the class-token
#   pass; 577: the 12-wave launch, 19 tiles; head dim 48: T = 65 (1 wave) and 289 (9-wave launch, short tail)
DENSE = [(65, 64, 3, 2), (200, 64, 2, 2), (201, 64, 2, 2), (257, 64, 3, 2), (577, 64, 2, 1), (65, 48, 3, 2), (289, 48, 2, 2)]


@pytest.mark.parametrize("dt", LOW, ids=["bf16", "fp16"])
@pytest.mark.parametrize("T,Dh,H,B", DENSE)
def test_dense_attention_programs(dt, T, Dh, H, B):
    """ops.attention at head dim 64 / 48 in both 16-bit builds; every query split gives the automatic choice's bits."""
    cases = _Cases()
    for program in AP.PROGRAMS:
        qkv = _fused_qkv(T, Dh, H, B, program, dt, seed=T + Dh)
        ref = _attn_ref(qkv, H, Dh, Dh ** -0.5, [i * T for i in range(B + 1)])
        dq = qkv.to(DEV)
        run = lambda: ops.attention(dq, H, Dh, Dh ** -0.5, seg_len=T)
        got = run()
        label = f"dense {NAME[dt]} T={T} Dh={Dh} {program}"
        cases.check(label, got, ref, Dh)
        cases.same_bits(label + " second run", run(), got)
        for qs in ("1", "3"):
            cases.same_bits(label + f" QSPLIT={qs}", _with_env("SETOK_ATTN_QSPLIT", qs, run), got)
    cases.done()


@pytest.mark.parametrize("dt", LOW, ids=["bf16", "fp16"])
@pytest.mark.parametrize("T,H,B", [(200, 2, 2), (257, 3, 2)])
def test_row_kernel_programs(dt, T, H, B):
    """SETOK_ATTN_ROW=1: the row-resident kernel has no running maximum; the same programs, the same bound."""
    Dh = 64
    cases = _Cases()
    for program in AP.PROGRAMS:
        qkv = _fused_qkv(T, Dh, H, B, program, dt, seed=T + Dh)
        ref = _attn_ref(qkv, H, Dh, Dh ** -0.5, [i * T for i in range(B + 1)])
        dq = qkv.to(DEV)
        run = lambda: _with_env("SETOK_ATTN_ROW", "1", lambda: ops.attention(dq, H, Dh, Dh ** -0.5, seg_len=T))
        got = run()
        label = f"row {NAME[dt]} T={T} {program}"
        cases.check(label, got, ref, Dh)
        cases.same_bits(label + " second run", run(), got)
    cases.done()


@pytest.mark.parametrize("dt", LOW, ids=["bf16", "fp16"])
@pytest.mark.parametrize("B", [8, 16])
def test_head_dim_48_image_remap(dt, B):
    """Head dim 48 with a multiple of 8 images: the kernel deals (image, head) pairs so that all heads of an image share an XCD.  Every pair has
    its own data: a wrong pair shows against fp64, and against the same images run one at a time (one image: no remap)."""
    T, Dh, H = 65, 48, 3
    cases = _Cases()
    for program in ("stair8", "hot@T-1"):
        qkv = _fused_qkv(T, Dh, H, B, program, dt, seed=7)
        ref = _attn_ref(qkv, H, Dh, Dh ** -0.5, [i * T for i in range(B + 1)])
        dq = qkv.to(DEV)
        got = ops.attention(dq, H, Dh, Dh ** -0.5, seg_len=T)
        label = f"remap {NAME[dt]} B={B} {program}"
        cases.check(label, got, ref, Dh)
        cases.same_bits(label + " second run", ops.attention(dq, H, Dh, Dh ** -0.5, seg_len=T), got)
        alone = torch.cat([ops.attention(dq[b * T:(b + 1) * T].contiguous(), H, Dh, Dh ** -0.5, seg_len=T) for b in range(B)])
        cases.same_bits(label + " one image at a time", alone, got)
    cases.done()


# ---- cross-attention: the same kernel over ragged key segments ------------------------------------------------------------------------------
@pytest.mark.parametrize("q_len", [40, 257])
def test_cross_attention_programs(q_len):
    dt, H, Dh, lens = torch.bfloat16, 2, 64, [65, 33, 8, 1, 200, 201]
    C = H * Dh
    offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
    cases = _Cases()
    for program in ("stair8", "stair5.5", "hot@T-1", "onerow8"):
        q, kv = torch.empty(len(lens), q_len, H, Dh), torch.empty(offs[-1], 2, H, Dh)
        for s, n in enumerate(lens):
            for h in range(H):
                q[s, :, h], kv[offs[s]:offs[s + 1], 0, h], kv[offs[s]:offs[s + 1], 1, h] = AP.build(n, Dh, program, 300 + 10 * s + h, Tq=q_len)
        q, kv = q.reshape(-1, C).to(dt), kv.reshape(-1, 2 * C).to(dt)
        ref = _cross_ref(q, kv[:, :C], kv[:, C:], H, Dh, Dh ** -0.5, q_len, offs)
        qd, kvd, so = q.to(DEV), kv.to(DEV), torch.tensor(offs, dtype=torch.int32, device=DEV)
        run = lambda: ops.cross_attention(qd, kvd[:, :C], kvd[:, C:], H, Dh, Dh ** -0.5, q_len, so, len(lens), max(lens))
        got = run()
        label = f"cross {NAME[dt]} q_len={q_len} {program}"
        cases.check(label, got, ref, Dh)
        cases.same_bits(label + " second run", run(), got)
    cases.done()


# ---- causal prefill -----------------------------------------------------------------------------------------------------------------------
def _causal_qkv(T, Dh, H, Hkv, B, program, dt, seed):
    """(B * T, (H + 2 Hkv) Dh) rows [q: H heads | k: Hkv | v: Hkv]; the steering dimension of a key / value head serves all its query heads."""
    x = torch.empty(B, T, H + 2 * Hkv, Dh)
    for b in range(B):
        for h in range(H):
            x[b, :, h] = AP.build(T, Dh, program, seed + 100 * b + h)[0]
        for j in range(Hkv):
            _, x[b, :, H + j], x[b, :, H + Hkv + j] = AP.build(T, Dh, program, seed + 100 * b + 50 + j)
    return x.reshape(B * T, -1).to(dt)


def _causal_ref32(qkv, km, B, T, H, Hkv, Dh):
    """test_llama_gpu._causal_ref_gqa's formula in torch fp32 on the CPU: the yardstick of the fp32 bound."""
    x = qkv.float().reshape(B, T, (H + 2 * Hkv) * Dh)
    q = x[..., :H * Dh].reshape(B, T, H, Dh).transpose(1, 2)
    k = x[..., H * Dh:(H + Hkv) * Dh].reshape(B, T, Hkv, Dh).transpose(1, 2).repeat_interleave(H // Hkv, dim=1)
    v = x[..., (H + Hkv) * Dh:].reshape(B, T, Hkv, Dh).transpose(1, 2).repeat_interleave(H // Hkv, dim=1)
    allow = torch.tril(torch.ones(T, T, dtype=torch.bool))[None, None] & km.bool().reshape(B, 1, 1, T)
    s = ((q @ k.transpose(-1, -2)) * Dh ** -0.5).masked_fill(~allow, float("-inf"))
    return (torch.softmax(s, -1).nan_to_num(0.0) @ v).transpose(1, 2).reshape(B * T, H * Dh)


@pytest.mark.parametrize("dt,H,Hkv,Dh,T", [(torch.bfloat16, 4, 2, 128, 129), (torch.bfloat16, 4, 2, 128, 300), (torch.float32, 3, 3, 16, 70)],
                         ids=["bf16-T129", "bf16-T300", "fp32-T70"])
def test_causal_attention_programs(dt, H, Hkv, Dh, T):
    """Three sequences: whole, left-padded (its first queries see no key: zeros), and one with a hole at key 40 and right padding.  The hot key sits,
    in turn, in the hole (hidden there, seen in the others), at key 0 (hidden under the left padding), in the middle (the diagonal: seen only
    by the queries at or after it), and on both sides of an edge of the kernel's partition: the 128-query block of the MFMA kernel, the 64-lane
    stride of the generic one."""
    B, hole, pad = 3, 40, T // 4
    km = torch.ones(B, T, dtype=torch.uint8)
    km[1, :pad] = 0
    km[2, hole] = 0
    km[2, T - T // 5:] = 0
    edge = 128 if Dh == 128 else 64
    programs = ["stair8", "down8", "shift-60"] + [f"hot@{p}" for p in (hole, 0, T // 2 + 3, edge - 1, edge)]
    cases = _Cases()
    for program in programs:
        qkv = _causal_qkv(T, Dh, H, Hkv, B, program, dt, seed=T)
        ref = _causal_ref_gqa(qkv, km, B, T, H, Hkv, Dh)
        bound = (BOUND16, BOUND16) if dt != torch.float32 else _bounds32(_causal_ref32(qkv, km, B, T, H, Hkv, Dh), ref, Dh)
        dq, dm = qkv.to(DEV), km.reshape(-1).to(DEV)
        got = ops.attention_causal(dq, dm, B, T, H, Dh, Dh ** -0.5, Hkv)
        label = f"causal {NAME[dt]} T={T} {program}"
        cases.check(label, got, ref, Dh, *bound)
        cases.same_bits(label + " second run", ops.attention_causal(dq, dm, B, T, H, Dh, Dh ** -0.5, Hkv), got)
        if float(got.reshape(B, T, -1)[1, :pad].float().abs().max()) != 0.0:
            cases.bad.append(f"{label}: rows without a visible key are not zero")
    cases.done()


# ---- decode: the chunk merge ---------------------------------------------------------------------------------------------------------------
def _decode_ref32(qkv, k, v, mask, H, Hkv, Dh, n):
    """test_generate_gpu._decode_ref's formula in torch fp32 on the CPU."""
    B = qkv.shape[0]
    q = qkv[:, :H * Dh].float().reshape(B, H, Dh)
    kk = k[:, :, :n].float().nan_to_num(0.0).repeat_interleave(H // Hkv, dim=1)
    vv = v[:, :, :n].float().nan_to_num(0.0).repeat_interleave(H // Hkv, dim=1)
    s = torch.einsum("bhd,bhjd->bhj", q, kk) * Dh ** -0.5
    s = s.masked_fill(~mask[:, None, :n].bool(), float("-inf"))
    return torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1).nan_to_num(0.0), vv).reshape(B, H * Dh)


@pytest.mark.parametrize("dt,Dh", [(torch.bfloat16, 128), (torch.float16, 128), (torch.float32, 128), (torch.float32, 16)],
                         ids=["bf16-128", "fp16-128", "fp32-128", "fp32-16"])
@pytest.mark.parametrize("n", [CHUNK + 1, 1000])
def test_decode_attention_programs(dt, Dh, n):
    """_decode_problem's four sequences (whole, left-padded, right-padded, fully masked; NaN in every dead slot) with steered keys: stairs of 8 nats per
    chunk (the merge scales the first chunk by e^-8 at CHUNK + 1 slots and by e^-56 at 1000), and a hot key in the last slot of a chunk, the first
    of the next, the last live slot, a masked slot and the slot just past the end — the last two hold a finite hot key (their values stay NaN):
    a kernel that lets one into its maximum or its sum shows."""
    H, Hkv, cap = 4, 2, n + 5
    masked_slot = n // 3 - 1                                       # dead in the left-padded sequence, live in the others
    programs = ["stair8", "down8"] + [f"hot@{p}" for p in (CHUNK - 1, CHUNK, n - 1, masked_slot, n)]
    cases = _Cases()
    for program in programs:
        qkv, k, v, mask = _decode_problem(dt, H, Hkv, Dh, n, cap, seed=400 + n)
        qkv, k = 0.5 * qkv.float(), 0.5 * k.float()
        qkv.reshape(4, H + 2 * Hkv, Dh)[:, :H, 0] = Dh ** 0.5
        if program.startswith("hot@"):
            p = AP.hot_key(program, n)
            k[:, :, :, 0] = torch.where(k[:, :, :, 0].isnan(), k[:, :, :, 0], torch.zeros(()))
            k[:, :, p] = k[:, :, p].nan_to_num(0.25)               # a dead slot that is heated becomes a finite key
            k[:, :, p, 0] = 16.0
        else:
            g = AP.offsets(cap, program, tile=CHUNK)
            k[:, :, :, 0] = torch.where(k[:, :, :, 0].isnan(), k[:, :, :, 0], g[None, None])
        qkv, k = qkv.to(dt), k.to(dt)
        ref = _decode_ref(qkv, k, v, mask, H, Hkv, Dh, n)
        bound = (BOUND16, BOUND16) if dt != torch.float32 else _bounds32(_decode_ref32(qkv, k, v, mask, H, Hkv, Dh, n), ref, Dh)
        args = (qkv.to(DEV), k.to(DEV), v.to(DEV), mask.to(DEV), H, n, Dh ** -0.5)
        got = ops.attention_decode(*args)
        label = f"decode {NAME[dt]} Dh={Dh} len={n} {program}"
        cases.check(label, got, ref, Dh, *bound)
        cases.same_bits(label + " second run", ops.attention_decode(*args), got)
        if float(got[3].float().abs().max()) != 0.0:
            cases.bad.append(f"{label}: the fully masked sequence is not zero")
    cases.done()


# ---- segment attention at head dim 512 ------------------------------------------------------------------------------------------------------
def test_segment_attention_head_dim_512_programs():
    H, Dh, lens = 2, 512, [1, 33, 65, 129, 300]
    offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
    so = torch.tensor(offs, dtype=torch.int32, device=DEV)
    cases = _Cases()
    for program in ("stair8", "down8", "hot@T-1", "hot@32"):
        qkv = torch.cat([_fused_qkv(n, Dh, H, 1, program, torch.float32, seed=500 + s) for s, n in enumerate(lens)]).bfloat16()
        ref = _attn_ref(qkv, H, Dh, Dh ** -0.5, offs)
        dq = qkv.to(DEV)
        run = lambda: ops.attention(dq, H, Dh, Dh ** -0.5, seg_len=max(lens), seg_offsets=so, n_segs=len(lens))
        got = run()
        label = f"seg512 bf16 {program}"
        cases.check(label, got, ref, Dh)
        cases.same_bits(label + " second run", run(), got)
    cases.done()
