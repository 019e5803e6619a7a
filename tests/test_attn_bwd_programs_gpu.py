"""The attention backward kernels under steered scores: the programs of tests/attn_bwd_programs.py (stairs up and down the key tiles, a shifted score
level, one steered row in a wave of flat ones, one hot key on a partition's edge or behind a mask, two equal hot keys astride an edge) through every
backward pair — the causal MFMA pair of head dim 128 (attn_causal_bwd.hip) and its generic twin (llama_bwd.hip), the decoder's MFMA pair of head
dims 48 / 64 (attn_mha_bwd.hip) and the generic wave-per-row pair (norm_attn.hip) in self- and ragged cross-attention, and the head-dim-512 segment
pair (attn_seg_bwd.hip).  Unit-variance inputs, all the other tests use, keep every scaled score within about a nat of the rest: the running maximum of
the first walks, the lane merges, the plain / diagonal / masked branches and an exp2(s c - lse) that overflows behind a mask never matter there.

Every case: inputs built on the CPU in the element type; `out` from the project's own forward on the GPU; the backward; the fp64 reference of the
SAME rounded inputs and that same `out` (the as-given contract: D = dO . out); then on every row of dq, dk and dv
    max_d |got - ref| < c(dt) max_d A + kappa max_d N + eta(dt) max_d S
with exact zeros where N = 0, everything finite, and equal bits on a second run.  The bound, its three scales and where c, kappa and eta come from
are in tests/attn_bwd_programs.py; tests/test_attn_bwd_programs_cpu.py shows it attainable (an honest emulation stays below 0.75 of it on every
case here) and sharp (every planted fault breaks it in every table).  Per case and gradient the worst err / tol, the three terms' shares of tol at
that row and kappa go to SETOK_PARITY_LOG (profiles/attn_bwd_programs_parity.txt).  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import attn_bwd_programs as BP
from test_generate_gpu import _log
from test_ops_gpu import _with_env

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops

DEV = "cuda"


class _Cases:
    """Collects a test's verdicts, logs each, and fails at the end naming every case over its bound."""

    def __init__(self):
        self.bad = []

    def judge(self, label, dt, problems, outs, grads):
        """problems[i] with its `out` (Hq, Tq, Dh) and grads[i] = (dq, dk, dv) as the kernel gave them, on the CPU."""
        worst = {}
        for i, (pb, out, got) in enumerate(zip(problems, outs, grads)):
            verdicts, kap, _ = BP.judge(pb, out.float(), got, dt)
            for name, vd in zip(BP.GRADS, verdicts):
                if not vd.zeros:
                    self.bad.append(f"{label} #{i} {name}: rows without a visible key / keys no query sees are not exact zeros")
                if name not in worst or not vd.ratio <= worst[name][0].ratio:
                    worst[name] = (vd, kap, i)
        for name, (vd, kap, i) in worst.items():
            _log(f"{label} {name}: err/tol, shares of tol (c A, kappa N, eta S), kappa", vd.ratio, *vd.share, kap)
            if not vd.ratio < 1.0:
                self.bad.append(f"{label} #{i} {name}: err / tol = {vd.ratio:.3f} (shares c A {vd.share[0]:.2f}, kappa N {vd.share[1]:.2f}, "
                                f"eta S {vd.share[2]:.2f})")

    def same_bits(self, label, a, b):
        if not all(torch.equal(x, y) for x, y in zip(a, b)):
            self.bad.append(f"{label}: bits differ on a second run")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _rows(x):
    """(heads, T, Dh) -> (T, heads * Dh)"""
    return x.transpose(0, 1).reshape(x.shape[1], -1)


def _heads(x, Dh):
    """(T, heads * Dh) -> (heads, T, Dh), on the CPU"""
    return x.detach().cpu().reshape(x.shape[0], -1, Dh).transpose(0, 1)


# ---- the causal pairs -------------------------------------------------------------------------------------------------------------------------
def _run_causal(cases, case):
    H, Hkv, Dh, T, _ = case.params
    dt, problems = case.dt, case.make()
    B = len(problems)
    qkv = torch.cat([torch.cat([_rows(pb.q), _rows(pb.k), _rows(pb.v)], 1) for pb in problems]).to(dt).to(DEV)
    dout = torch.cat([_rows(pb.dout) for pb in problems]).to(dt).to(DEV)
    km = BP.causal_masks(T).reshape(-1).to(DEV)
    out = ops.attention_causal(qkv, km, B, T, H, Dh, Dh ** -0.5, Hkv)
    got = ops.attention_causal_bwd(qkv, km, out, dout, B, T, H, Dh, Dh ** -0.5, Hkv)
    cases.same_bits(case.label, [ops.attention_causal_bwd(qkv, km, out, dout, B, T, H, Dh, Dh ** -0.5, Hkv)], [got])
    a, b = H * Dh, (H + Hkv) * Dh
    grads = [tuple(_heads(got[i * T:(i + 1) * T, sl], Dh) for sl in (slice(0, a), slice(a, b), slice(b, None))) for i in range(B)]
    cases.judge(case.label, dt, problems, [_heads(out[i * T:(i + 1) * T], Dh) for i in range(B)], grads)


@pytest.mark.parametrize("dt", BP.LOW, ids=["bf16", "fp16"])
@pytest.mark.parametrize("T", [129, 300])
def test_causal_mfma_bwd_programs(dt, T):
    """attn_causal_bwd.hip, (H, Hkv) = (4, 2): T = 129 leaves one row in the second 128-query block (its tiles staged with clamped rows), T = 300
    gives three blocks and a 12-key last tile.  Three sequences: whole, left-padded by T // 4, a hole at key 40 plus right padding of T // 5.  The
    hot key sits in the hole, under the left padding, on the diagonal and on both sides of the block edge; the pairs straddle a tile edge, the
    block edge, and the hole.  A hidden hot key must leave its own dk and dv rows exactly zero — exp2(s c - lse) overflows behind it inside the
    dK / dV kernel before the column is discarded — and the rest within the bound."""
    cases = _Cases()
    for case in BP.causal_cases(dt, 4, 2, 128, T):
        _run_causal(cases, case)
    cases.done()


def test_causal_mfma_bwd_programs_group_of_8():
    """(H, Hkv) = (8, 1): the dK / dV kernel's loop over the query heads of a group."""
    cases = _Cases()
    for case in BP.causal_cases(torch.bfloat16, 8, 1, 128, 129, ["stair8", "pair@127,128"]):
        _run_causal(cases, case)
    cases.done()


@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.float32, 3, 3, 16), (torch.bfloat16, 4, 2, 64)], ids=["fp32-Dh16", "bf16-Dh64"])
def test_causal_generic_bwd_programs(dt, H, Hkv, Dh):
    """llama_bwd.hip's generic pair at T = 70: the hot key and the pair on both sides of its 64-lane stride."""
    cases = _Cases()
    for case in BP.causal_cases(dt, H, Hkv, Dh, 70, BP.CAUSAL_GENERIC_PROGRAMS):
        _run_causal(cases, case)
    cases.done()


# ---- the decoder pairs ---------------------------------------------------------------------------------------------------------------------------
def _run_mha_self(cases, case, label=None):
    H, Dh, T, B, _ = case.params
    dt, problems, C = case.dt, case.make(), H * Dh
    label = case.label if label is None else label
    qkv = torch.cat([torch.cat([_rows(pb.q), _rows(pb.k), _rows(pb.v)], 1) for pb in problems]).to(dt).to(DEV)
    dout = torch.cat([_rows(pb.dout) for pb in problems]).to(dt).to(DEV)
    out = ops.attention(qkv, H, Dh, Dh ** -0.5, seg_len=T)

    def run():
        d = torch.empty_like(qkv)
        ops.mha_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], out, dout, H, Dh, Dh ** -0.5, T, None, B, T, dq=d[:, :C], dk=d[:, C:2 * C], dv=d[:, 2 * C:])
        return d

    got = run()
    cases.same_bits(label, [run()], [got])
    grads = [tuple(_heads(got[i * T:(i + 1) * T, j * C:(j + 1) * C], Dh) for j in range(3)) for i in range(B)]
    cases.judge(label, dt, problems, [_heads(out[i * T:(i + 1) * T], Dh) for i in range(B)], grads)


@pytest.mark.parametrize("dt,Dh,T", [(torch.bfloat16, 64, 65), (torch.bfloat16, 64, 200), (torch.bfloat16, 48, 65), (torch.bfloat16, 48, 200),
                                     (torch.float16, 64, 65)], ids=["bf16-64-65", "bf16-64-200", "bf16-48-65", "bf16-48-200", "fp16-64-65"])
def test_mha_bwd_self_programs(dt, Dh, T):
    """attn_mha_bwd.hip on the column windows of one qkv buffer (`out` from ops.attention): the hot key and the pairs on both sides of the 16-key
    score tile and of the 32-key step; the stairs move the per-lane online maximum that four lanes then merge."""
    cases = _Cases()
    for case in BP.mha_cases(dt, Dh, T):
        _run_mha_self(cases, case)
    cases.done()


def test_mha_bwd_self_programs_generic():
    """SETOK_ATTN_BWD_GENERIC=1: norm_attn.hip's wave-per-row pair on the same cases, the same tolerance."""
    cases = _Cases()
    for case in BP.mha_cases(torch.bfloat16, 64, 65):
        _with_env("SETOK_ATTN_BWD_GENERIC", "1", lambda: _run_mha_self(cases, case, "generic " + case.label))
    cases.done()


@pytest.mark.parametrize("q_len", [40, 65])
def test_mha_bwd_cross_programs(q_len):
    """Ragged cross-attention (`out` from ops.cross_attention): q_len = 40 leaves a wave 8 live rows, 65 puts one row into a second workgroup;
    key segments of 65, 33, 8, 1, 200 and 201 rows, each its own draw."""
    cases = _Cases()
    for case in BP.cross_cases(q_len):
        H, Dh, _, lens, _ = case.params
        dt, problems, C = case.dt, case.make(), H * Dh
        offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
        q = torch.cat([_rows(pb.q) for pb in problems]).to(dt).to(DEV)
        kv = torch.cat([torch.cat([_rows(pb.k), _rows(pb.v)], 1) for pb in problems]).to(dt).to(DEV)
        dout = torch.cat([_rows(pb.dout) for pb in problems]).to(dt).to(DEV)
        so = torch.tensor(offs, dtype=torch.int32, device=DEV)
        out = ops.cross_attention(q, kv[:, :C], kv[:, C:], H, Dh, Dh ** -0.5, q_len, so, len(lens), max(lens))
        run = lambda: ops.mha_bwd(q, kv[:, :C], kv[:, C:], out, dout, H, Dh, Dh ** -0.5, q_len, so, len(lens), max(lens))
        got = run()
        cases.same_bits(case.label, run(), got)
        qs = lambda x, s: _heads(x[s * q_len:(s + 1) * q_len], Dh)
        ks = lambda x, s: _heads(x[offs[s]:offs[s + 1]], Dh)
        grads = [(qs(got[0], s), ks(got[1], s), ks(got[2], s)) for s in range(len(lens))]
        cases.judge(case.label, dt, problems, [qs(out, s) for s in range(len(lens))], grads)
    cases.done()


# ---- the segment pair at head dim 512 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_segment_bwd_head_dim_512_programs(dt):
    """ops.attention_bwd over ragged segments (`out` from ops.attention).  bf16: segments of 1 and 32 rows go to the generic kernels, those of 33, 65,
    129 and 300 to attn_seg_bwd.hip (its tile-wise running maximum).  fp32: the generic kernels at 1, 33 and 65 rows."""
    cases = _Cases()
    for case in BP.seg_cases(dt):
        H, Dh, lens, _ = case.params
        problems, C = case.make(), H * Dh
        offs = np.concatenate([[0], np.cumsum(lens)]).tolist()
        qkv = torch.cat([torch.cat([_rows(pb.q), _rows(pb.k), _rows(pb.v)], 1) for pb in problems]).to(dt).to(DEV)
        dout = torch.cat([_rows(pb.dout) for pb in problems]).to(dt).to(DEV)
        so = torch.tensor(offs, dtype=torch.int32, device=DEV)
        out = ops.attention(qkv, H, Dh, Dh ** -0.5, seg_len=max(lens), seg_offsets=so, n_segs=len(lens))
        run = lambda: ops.attention_bwd(qkv, out, dout, H, Dh, Dh ** -0.5, max(lens), so, len(lens))
        got = run()
        cases.same_bits(case.label, [run()], [got])
        seg = lambda x, s: x[offs[s]:offs[s + 1]]
        grads = [tuple(_heads(seg(got, s)[:, j * C:(j + 1) * C], Dh) for j in range(3)) for s in range(len(lens))]
        cases.judge(case.label, dt, problems, [_heads(seg(out, s), Dh) for s in range(len(lens))], grads)
    cases.done()
