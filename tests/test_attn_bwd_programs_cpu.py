"""tests/attn_bwd_programs.py judged on the CPU before tests/test_attn_bwd_programs_gpu.py asserts anything with it: the reference's formula against
torch autograd, the tolerance shown attainable (an honest emulation of the kernels' arithmetic stays below 0.75 of it on every row of every case the
GPU test runs), its teeth (every planted fault of the emulation breaks it in every table), and the programs shown to steer.

Why the bar is an error scale and not max-rel: under `shift-60` (causal, bf16, head dim 128, T = 129) the honest emulation's plain global
max-rel error of dq against fp64 is 9.0e-2 — dq[:, 0] = -60 sum_j ds_j is ~0 exactly and rounding noise otherwise.
test_max_rel_record prints the figure; nothing asserts it."""
import math

import pytest
import torch

import attn_bwd_programs as BP
import attn_programs as AP

ATTAIN = 0.75


def _autograd(pb):
    """torch autograd of the fp64 forward."""
    q, k, v = (x.double().requires_grad_(True) for x in (pb.q, pb.k, pb.v))
    with torch.enable_grad():
        G = q.shape[0] // k.shape[0]
        s = (q @ k.repeat_interleave(G, 0).transpose(-1, -2)) * pb.scale
        some = pb.allow.any(-1, keepdim=True)
        p = torch.softmax(s.masked_fill(~(pb.allow | ~some), -math.inf), -1) * pb.allow
        o = p @ v.repeat_interleave(G, 0)
        return torch.autograd.grad((o * pb.dout.double()).sum(), (q, k, v))


@pytest.mark.parametrize("which", ["causal gqa", "ragged cross"])
def test_reference_is_the_gradient(which):
    """With `out` the exact fp64 output the as-given formula is the gradient: dq, dk, dv equal autograd's to 1e-10 relative."""
    if which == "causal gqa":
        problems = BP.causal_problems(torch.bfloat16, 4, 2, 16, 70, "stair8")              # all three masks
    else:
        problems = BP.cross_problems(torch.bfloat16, 2, 16, 40, [65, 33, 8, 1], "down8", seed=3)
    for pb in problems:
        out = BP.forward(pb.q, pb.k, pb.v, pb.allow, pb.scale)
        ref = BP.reference(pb.q, pb.k, pb.v, pb.dout, out, pb.allow, pb.scale)
        for name, g, a in zip(BP.GRADS, ref.grad, _autograd(pb)):
            assert float((g - a).abs().max()) <= 1e-10 * float(a.abs().max()), name


def _worst(case, fault=None):
    """Worst err / tol of the emulation over a case's problems and gradients (and what it was)."""
    worst, at = 0.0, ""
    for i, pb in enumerate(case.make()):
        out = BP.out_rounded(pb, case.dt)
        got = BP.emulate(pb.q, pb.k, pb.v, pb.dout, out, pb.allow, pb.scale, case.dt, fault)
        verdicts, _, _ = BP.judge(pb, out, got, case.dt)
        for name, vd in zip(BP.GRADS, verdicts):
            assert fault is not None or vd.zeros, f"{case.label} #{i} {name}: rows with N = 0 are not zero"
            if vd.ratio > worst:
                worst, at = vd.ratio, f"#{i} {name}"
    return worst, at


@pytest.mark.parametrize("table", list(BP.TABLES))
def test_bound_is_attainable(table):
    """Every case of the table, every row: the honest emulation stays below 0.75 of the tolerance.  (fp32 cases: the emulation IS the evaluation
    kappa is four times the error of: 0.25.)"""
    bad, top = [], 0.0
    for case in BP.TABLES[table][0]:
        w, at = _worst(case)
        top = max(top, w)
        print(f"{case.label}: {w:.3f} {at}")
        if not w < ATTAIN:
            bad.append(f"{case.label}: {w:.3f} at {at}")
    print(f"{table}: worst {top:.3f}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("fault", BP.FAULTS)
@pytest.mark.parametrize("table", list(BP.TABLES))
def test_faults_break_the_bound(table, fault):
    """Every planted fault pushes at least one case of the table over the tolerance, in each element type the table has.  The tables without masks or causality have no masked key and
    no diagonal: `hole_seen` and `past_diag` cannot be planted there."""
    cases, not_here = BP.TABLES[table]
    if fault in not_here:
        assert all(bool(pb.allow.all()) for pb in cases[0].make())                         # (the reason holds: nothing is masked)
        return
    for dt in sorted({case.dt for case in cases}, key=str):                                # in every element type of the table
        top = 0.0
        for case in cases:
            if case.dt == dt:
                top = max(top, _worst(case, fault)[0])
                if top > 1.0:
                    break
        print(f"{table} {BP.NAME[dt]} {fault}: {top:.2f}")
        assert top > 1.0, (BP.NAME[dt], top)


def _rows_p(pb):
    out = BP.forward(pb.q, pb.k, pb.v, pb.allow, pb.scale)
    return BP.reference(pb.q, pb.k, pb.v, pb.dout, out, pb.allow, pb.scale).p           # (Hq, Tq, Tk)


@pytest.mark.parametrize("table", list(BP.TABLES))
def test_programs_steer(table):
    """stair8: the largest p of every row that sees at least two key tiles lies in its last visible tile; pair@a,b: the rows that see both keys hold
    p_a and p_b within [0.4, 0.6]; hot@: the rows that see the key hold p >= 0.99."""
    seen = set()
    for case in BP.TABLES[table][0]:
        program = case.params[-1]
        kind = program.split("@")[0]
        if kind not in ("stair8", "pair", "hot"):
            continue
        seen.add(kind)
        for pb in case.make():
            p, Tk = _rows_p(pb), pb.k.shape[1]
            al = pb.allow[None].expand_as(p)
            if kind == "stair8":
                j = torch.arange(Tk)
                first = torch.where(al, j, torch.full((), Tk)).amin(-1) // 32
                last = torch.where(al, j, torch.full((), -1)).amax(-1) // 32
                rows = al.any(-1) & (last > first)
                assert bool((p.argmax(-1) // 32 == last)[rows].all()), case.label
            elif kind == "pair":
                a, b = BP.pair_keys(program, Tk)
                if max(a, b) >= Tk:
                    continue
                rows = al[..., a] & al[..., b]
                both = torch.stack([p[..., a][rows], p[..., b][rows]])
                assert both.numel() == 0 or (float(both.min()) >= 0.4 and float(both.max()) <= 0.6), (case.label, float(both.min()), float(both.max()))
            else:
                a = AP.hot_key(program, Tk)
                if a >= Tk:
                    continue
                rows = al[..., a]
                assert bool((p[..., a][rows] >= 0.99).all()), case.label
    assert "stair8" in seen


def test_max_rel_record():
    """The figure of the module docstring: plain global max-rel of the honest emulation's dq under shift-60.  Printed, not asserted."""
    dt = torch.bfloat16
    worst = 0.0
    for pb in BP.causal_problems(dt, 4, 2, 128, 129, "shift-60"):
        out = BP.out_rounded(pb, dt)
        got = BP.emulate(pb.q, pb.k, pb.v, pb.dout, out, pb.allow, pb.scale, dt)
        ref = BP.reference(pb.q, pb.k, pb.v, pb.dout, out, pb.allow, pb.scale)
        worst = max(worst, AP.errors(got[0], ref.grad[0])[0])
    print(f"shift-60 dq, bf16 emulation against fp64: global max-rel {worst:.3e}")
