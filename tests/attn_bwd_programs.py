"""Score programs for the attention BACKWARD kernels, with an error-scale bound.  Pure torch on the CPU; imports nothing of the library.

The programs are those of tests/attn_programs.py (steering through dimension 0: q[..., 0] = sqrt(Dh), k[..., 0] = g_j nats) plus `pair@a,b`: keys a
and b both sit 16 nats above the rest.  A single hot key saturates the softmax, so the exact dq and dk vanish and only dv and the overflow behind a
mask are probed; two hot keys hold p = 1/2 each, and dq and dk then depend on both.  The pair's second key is the first plus a quarter of a fresh draw
(k_b = k_a + 0.125 randn): their score difference then has a standard deviation of 1/16 nat.  With two independent draws it would be 0.35 nat, and
p_a would leave [0.4, 0.6] on a quarter of the rows.

One problem: q, dout, out (Hq, Tq, Dh); k, v (Hkv, Tk, Dh); `allow` a bool (Tq, Tk) or (Hq, Tq, Tk) matrix — causality, key padding, holes and
segment membership alike, so one implementation serves every kernel family.

`reference` is the fp64 gradient under the AS-GIVEN contract: the kernels receive the forward's (rounded) `out` and form D_i = dO_i . out_i from it,
so the reference does the same with the very tensor handed to the kernel.  It also returns three error scales per output element:
    A   the absolute sum of the real terms             A_q = scale |ds| |K|     A_k = scale |ds|^T |Q|    A_v = p^T |dO|
    N   the same without the cancellation in dp - D    w_ij = p_ij (|do_i|.|v_j| + |do_i|.|out_i|);  N_q = scale w |K|,  N_k = scale w^T |Q|,  N_v = A_v
    S   count-everything sums, for underflow           S_q = scale allow |K|    S_k = scale allow^T |Q|   S_v = allow^T |dO|
and the bound on max_d |got - ref| of an output row is
    tol = c(dt) max_d A + kappa max_d N + eta(dt) max_d S
on every row with max_d N > 0; rows with N = 0 (a query with no visible key, a key no query sees) must be exact zeros.
    c     2.56 u, u the half-ulp relative rounding of the type (2^-8 in bf16: c = 1e-2, the project's 16-bit attention bar; 2^-11 in fp16; 0 in fp32):
          1.28 x the first-order worst case of the two roundings a sum meets, P or dS to the 16-bit type and the stored result.
    kappa the project's fp32 rule: 4 x the worst max_d |err| / max_d N of torch's own fp32 evaluation of the same formula against fp64, floored at 3e-6.
    eta   2^-24 in fp16, one subnormal step (P and dS below 6e-5 lose relative precision there); 0 in bf16 and fp32.
A plain max-rel bar cannot work here: with k[:, 0] = -60, dq[:, 0] = -60 sum_j ds_j, whose exact value is ~0 and whose rounded value is not.

`emulate` is the same formula with the kernels' roundings (and, for fp32, the evaluation kappa is taken from); `FAULTS` are planted errors of the
emulation only.  `TABLES` lists the cases of tests/test_attn_bwd_programs_gpu.py: the CPU test shows the bound attainable on every one of them and
every fault caught in every table before the GPU test asserts anything."""
import math
from typing import List, NamedTuple, Optional

import torch

import attn_programs as AP

LOG2E = AP.LOG2E
FLOOR32 = 3e-6
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
ETA = {torch.bfloat16: 0.0, torch.float16: 2.0 ** -24, torch.float32: 0.0}
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
GRADS = ("dq", "dk", "dv")
FAULTS = ("lse_ln", "skip_key", "hole_seen", "past_diag", "d_half")          # planted errors of `emulate`; never in a kernel
SKIPPED_KEY = 32


def c_of(dt) -> float:
    return 2.56 * U[dt]


# ---- programs ------------------------------------------------------------------------------------------------------------------------------------
def pair_keys(program: str, T: int, tile: int = 32):
    """The two keys of `pair@a,b` (each a number, `T-1` or `lasttile`)."""
    a, b = program.split("@", 1)[1].split(",")
    return AP.hot_key("hot@" + a, T, tile), AP.hot_key("hot@" + b, T, tile)


def offsets(T: int, program: str, tile: int = 32) -> torch.Tensor:
    """g_j of the program in nats, fp32: AP.offsets plus `pair@a,b`.  A key index >= T heats nothing."""
    if program.startswith("pair@"):
        g = torch.zeros(T)
        for p in pair_keys(program, T, tile):
            if 0 <= p < T:
                g[p] = 16.0
        return g
    return AP.offsets(T, program, tile)


def build(Tq: int, Tk: int, Dh: int, program: str, seed: int, tile: int = 32):
    """(q (Tq, Dh), k (Tk, Dh), v (Tk, Dh), dout (Tq, Dh)) of one head, fp32: AP.build's draw and steering, then dout ~ randn."""
    g = torch.Generator().manual_seed(seed)
    q = 0.5 * torch.randn(Tq, Dh, generator=g)
    k = 0.5 * torch.randn(Tk, Dh, generator=g)
    v = torch.randn(Tk, Dh, generator=g)
    dout = torch.randn(Tq, Dh, generator=g)
    a = torch.full((Tq,), math.sqrt(Dh))
    if program == "onerow8":
        a = torch.where(torch.arange(Tq) % 32 == 5, a, torch.zeros(Tq))
    q[:, 0] = a
    k[:, 0] = offsets(Tk, program, tile)
    if program.startswith("pair@"):
        pa, pb = pair_keys(program, Tk, tile)
        if 0 <= pa < Tk and 0 <= pb < Tk:
            k[pb, 1:] = k[pa, 1:] + 0.125 * torch.randn(Dh - 1, generator=g)
    return q, k, v, dout


# ---- fp64 -----------------------------------------------------------------------------------------------------------------------------------------
def _allow3(allow, Hq):
    return allow[None].expand(Hq, -1, -1) if allow.dim() == 2 else allow


def _softmax(s, allow):
    """Softmax over the allowed keys; a row with none is all zero."""
    some = allow.any(-1, keepdim=True)
    p = torch.softmax(s.masked_fill(~(allow | ~some), -math.inf), -1)
    return torch.where(allow, p, torch.zeros((), dtype=p.dtype))


def forward(q, k, v, allow, scale):
    """softmax over the allowed keys, times v, in fp64: (Hq, Tq, Dh)."""
    Hq, G = q.shape[0], q.shape[0] // k.shape[0]
    q, k, v = q.double(), k.double().repeat_interleave(G, 0), v.double().repeat_interleave(G, 0)
    return _softmax(q @ k.transpose(-1, -2) * scale, _allow3(allow, Hq)) @ v


class Ref(NamedTuple):
    grad: tuple                                    # (dq (Hq, Tq, Dh), dk (Hkv, Tk, Dh), dv (Hkv, Tk, Dh)), fp64
    A: tuple                                       # the three scales, each a (q, k, v) triple of tensors shaped like the gradients
    N: tuple
    S: tuple
    p: torch.Tensor                                # (Hq, Tq, Tk) probabilities


def reference(q, k, v, dout, out, allow, scale) -> Ref:
    """The as-given gradient in fp64 and its error scales."""
    Hq, Hkv = q.shape[0], k.shape[0]
    G = Hq // Hkv
    q, do, o = q.double(), dout.double(), out.double()
    kk, vv = k.double().repeat_interleave(G, 0), v.double().repeat_interleave(G, 0)
    al = _allow3(allow, Hq)
    p = _softmax(q @ kk.transpose(-1, -2) * scale, al)
    D = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ vv.transpose(-1, -2) - D)
    w = p * (do.abs() @ vv.abs().transpose(-1, -2) + (do.abs() * o.abs()).sum(-1, keepdim=True))
    ald = al.double()
    group = lambda x: x.reshape(Hkv, G, *x.shape[1:]).sum(1)                 # sum over the query heads of a group
    t = lambda x: x.transpose(-1, -2)
    grad = (scale * ds @ kk, group(scale * t(ds) @ q), group(t(p) @ do))
    Av = group(t(p) @ do.abs())
    A = (scale * ds.abs() @ kk.abs(), group(scale * t(ds.abs()) @ q.abs()), Av)
    N = (scale * w @ kk.abs(), group(scale * t(w) @ q.abs()), Av)
    S = (scale * ald @ kk.abs(), group(scale * t(ald) @ q.abs()), group(t(ald) @ do.abs()))
    return Ref(grad, A, N, S, p)


def kappa(ref: Ref, eval32) -> float:
    """The fp32 rule: 4 x the worst max_d |err| / max_d N of the fp32 evaluation `eval32` (a (dq, dk, dv) triple) against fp64, floored."""
    worst = 0.0
    for g, r, n in zip(eval32, ref.grad, ref.N):
        n = n.amax(-1)
        live = n > 0
        if bool(live.any()):
            worst = max(worst, float(((g.double() - r).abs().amax(-1)[live] / n[live]).max()))
    return max(4 * worst, FLOOR32)


def tolerance(ref: Ref, dt, kap: float, eta: Optional[float] = None):
    """Per gradient: (tol per output row, the three terms per row)."""
    eta = ETA[dt] if eta is None else eta
    out = []
    for a, n, s in zip(ref.A, ref.N, ref.S):
        terms = (c_of(dt) * a.amax(-1), kap * n.amax(-1), eta * s.amax(-1))
        out.append((terms[0] + terms[1] + terms[2], terms))
    return out


class Verdict(NamedTuple):
    ratio: float                                   # worst err / tol over the rows with N > 0 (inf if anything is not finite)
    share: tuple                                   # the c A, kappa N and eta S terms' shares of tol at that row
    zeros: bool                                    # rows with N = 0 are exact zeros


def check(got, ref: Ref, dt, kap: float, eta: Optional[float] = None) -> List[Verdict]:
    """One Verdict per gradient for `got` = (dq, dk, dv) in the shapes of the reference."""
    out = []
    for g, r, n, (tol, terms) in zip(got, ref.grad, ref.N, tolerance(ref, dt, kap, eta)):
        g = g.detach().double().cpu()
        live = n.amax(-1) > 0
        zeros = bool((g[~live] == 0).all())
        if not bool(torch.isfinite(g).all()):
            out.append(Verdict(math.inf, (0.0, 0.0, 0.0), zeros))
            continue
        ratio = torch.where(live, (g - r).abs().amax(-1) / tol.clamp_min(1e-300), torch.zeros((), dtype=torch.float64))
        i = int(ratio.argmax())
        t = float(tol.reshape(-1)[i])
        share = tuple(float(x.reshape(-1)[i]) / t if t > 0 else 0.0 for x in terms)
        out.append(Verdict(float(ratio.reshape(-1)[i]), share, zeros))
    return out


# ---- the kernels' arithmetic ----------------------------------------------------------------------------------------------------------------------
def emulate(q, k, v, dout, out, allow, scale, dt, fault: Optional[str] = None):
    """The as-given formula with the kernels' roundings: inputs in `dt`; fp32 scores in log2 units; lse2 = m + log2(l) over the allowed keys;
    p = exp2(s c - lse2), zero where not allowed; dp and D in fp32; P and dS rounded to `dt` before the second products, which accumulate in fp32;
    results times scale, rounded to `dt`.  dt = fp32: the plain fp32 evaluation that kappa uses.  Returns (dq, dk, dv) in `dt`.
    `fault` plants one error:
      lse_ln     the natural log where log2 belongs in the lse
      skip_key   key 32 dropped from the second walk but kept in the lse
      hole_seen  a masked key (one no query sees) counted in the second walk by the rows whose last visible key lies behind it
      past_diag  row i counts key i + 1 (where some query sees that key)
      d_half     D summed over half the head dim"""
    assert fault is None or fault in FAULTS
    Hq, Hkv = q.shape[0], k.shape[0]
    G = Hq // Hkv
    rnd = (lambda x: x) if dt == torch.float32 else (lambda x: x.to(dt).float())
    q, do, o = rnd(q.float()), rnd(dout.float()), rnd(out.float())
    kk, vv = rnd(k.float()).repeat_interleave(G, 0), rnd(v.float()).repeat_interleave(G, 0)
    al = _allow3(allow, Hq)
    Tq, Tk = al.shape[-2:]
    c = scale * LOG2E
    t = (q @ kk.transpose(-1, -2)) * c                                        # fp32, log2 units
    m = t.masked_fill(~al, -math.inf).amax(-1, keepdim=True)
    some = al.any(-1, keepdim=True)
    m = torch.where(some, m, torch.zeros(()))
    l = torch.where(al, torch.exp2(t - m), torch.zeros(())).sum(-1, keepdim=True)
    log = torch.log if fault == "lse_ln" else torch.log2
    lse2 = torch.where(some, m + log(l.clamp_min(1e-38)), torch.zeros(()))
    count = al
    if fault == "skip_key" and Tk > SKIPPED_KEY:
        count = al.clone()
        count[..., SKIPPED_KEY] = False
    elif fault == "hole_seen":
        j = torch.arange(Tk)
        last = torch.where(al, j, torch.full((), -1)).amax(-1, keepdim=True)  # a row's last visible key
        count = al | (~al.any(-2, keepdim=True).expand_as(al) & (j < last))
    elif fault == "past_diag":
        i, j = torch.arange(Tq)[:, None], torch.arange(Tk)[None]
        count = al | ((j == i + 1) & al.any(-2, keepdim=True))
    p = torch.where(count, torch.exp2(t - lse2), torch.zeros(()))
    half = do.shape[-1] // 2 if fault == "d_half" else do.shape[-1]
    D = (do[..., :half] * o[..., :half]).sum(-1, keepdim=True)
    ds = p * (do @ vv.transpose(-1, -2) - D)
    p16, ds16 = rnd(p), rnd(ds)
    group = lambda x: x.reshape(Hkv, G, *x.shape[1:]).sum(1)
    dq = (ds16 @ kk) * scale
    dk = group(ds16.transpose(-1, -2) @ q) * scale
    dv = group(p16.transpose(-1, -2) @ do)
    return dq.to(dt), dk.to(dt), dv.to(dt)


# ---- the cases of the GPU test ----------------------------------------------------------------------------------------------------------------
class Problem(NamedTuple):
    """One sequence / segment, fp32 values already rounded to the case's type."""
    q: torch.Tensor                                # (Hq, Tq, Dh)
    k: torch.Tensor                                # (Hkv, Tk, Dh)
    v: torch.Tensor
    dout: torch.Tensor                             # (Hq, Tq, Dh)
    allow: torch.Tensor                            # (Tq, Tk) bool
    scale: float


def _problem(Hq, Hkv, Tq, Tk, Dh, program, seed, allow, dt):
    """Every query head and every key / value head its own draw (AP's causal layout: seeds seed + h and seed + 50 + j)."""
    qs = [build(Tq, Tk, Dh, program, seed + h) for h in range(Hq)]
    ks = [build(Tq, Tk, Dh, program, seed + 50 + j) for j in range(Hkv)]
    r = lambda x: x.to(dt).float()
    return Problem(r(torch.stack([x[0] for x in qs])), r(torch.stack([x[1] for x in ks])), r(torch.stack([x[2] for x in ks])),
                   r(torch.stack([x[3] for x in qs])), allow, Dh ** -0.5)


CAUSAL_HOLE = 40


def causal_masks(T: int) -> torch.Tensor:
    """(3, T) uint8 key masks of the forward's test: whole; left padding of T // 4; a hole at key 40 plus right padding of T // 5."""
    km = torch.ones(3, T, dtype=torch.uint8)
    km[1, :T // 4] = 0
    km[2, CAUSAL_HOLE] = 0
    km[2, T - T // 5:] = 0
    return km


def causal_problems(dt, H, Hkv, Dh, T, program) -> List[Problem]:
    km = causal_masks(T).bool()
    tril = torch.tril(torch.ones(T, T, dtype=torch.bool))
    return [_problem(H, Hkv, T, T, Dh, program, T + 100 * b, tril & km[b][None], dt) for b in range(3)]


def self_problems(dt, H, Dh, lens, program, seed) -> List[Problem]:
    """Self-attention inside each segment (the decoder's images: equal lengths; the head's segments: ragged)."""
    return [_problem(H, H, n, n, Dh, program, seed + 100 * s, torch.ones(n, n, dtype=torch.bool), dt) for s, n in enumerate(lens)]


def cross_problems(dt, H, Dh, q_len, lens, program, seed) -> List[Problem]:
    return [_problem(H, H, q_len, n, Dh, program, seed + 100 * s, torch.ones(q_len, n, dtype=torch.bool), dt) for s, n in enumerate(lens)]


def _causal_mfma_programs(T):
    return ["stair8", "down8", "shift-60", "onerow8", f"hot@{CAUSAL_HOLE}", "hot@0", f"hot@{T // 2 + 3}", "hot@127", "hot@128", "pair@31,32",
            "pair@127,128", f"pair@{CAUSAL_HOLE},{T // 2 + 3}"]


CAUSAL_GENERIC_PROGRAMS = ["stair8", "down8", "shift-60", f"hot@{CAUSAL_HOLE}", "hot@63", "hot@64", "pair@63,64"]
MHA_PROGRAMS = ["stair8", "down8", "shift-60", "onerow8", "hot@15", "hot@16", "hot@T-1", "pair@15,16", "pair@31,32"]
CROSS_PROGRAMS = ["stair8", "down8", "hot@T-1", "onerow8"]
CROSS_LENS = [65, 33, 8, 1, 200, 201]
SEG_PROGRAMS = ["stair8", "down8", "hot@T-1", "pair@31,32"]
SEG_LENS = [1, 32, 33, 65, 129, 300]
SEG_LENS32, SEG_PROGRAMS32 = [1, 33, 65], ["stair8", "pair@31,32"]


class Case(NamedTuple):
    label: str
    dt: torch.dtype
    make: object                                   # () -> List[Problem]
    params: tuple                                  # what the GPU test needs to lay the operands out


def _cases(prefix, dt, programs, make, params):
    return [Case(f"{prefix} {NAME[dt]} {pr}", dt, (lambda pr=pr: make(pr)), params + (pr,)) for pr in programs]


def causal_cases(dt, H, Hkv, Dh, T, programs=None) -> List[Case]:
    programs = _causal_mfma_programs(T) if programs is None else programs
    return _cases(f"causal H={H}/{Hkv} Dh={Dh} T={T}", dt, programs, lambda pr: causal_problems(dt, H, Hkv, Dh, T, pr), (H, Hkv, Dh, T))


def mha_cases(dt, Dh, T, H=2, B=2) -> List[Case]:
    return _cases(f"mha Dh={Dh} T={T}", dt, MHA_PROGRAMS, lambda pr: self_problems(dt, H, Dh, [T] * B, pr, 700 + T + Dh), (H, Dh, T, B))


def cross_cases(q_len, dt=torch.bfloat16, H=2, Dh=64) -> List[Case]:
    return _cases(f"cross q_len={q_len}", dt, CROSS_PROGRAMS, lambda pr: cross_problems(dt, H, Dh, q_len, CROSS_LENS, pr, 300 + q_len),
                  (H, Dh, q_len, tuple(CROSS_LENS)))


def seg_cases(dt, H=2, Dh=512) -> List[Case]:
    lens, programs = (SEG_LENS, SEG_PROGRAMS) if dt != torch.float32 else (SEG_LENS32, SEG_PROGRAMS32)
    return _cases("seg512", dt, programs, lambda pr: self_problems(dt, H, Dh, lens, pr, 500), (H, Dh, tuple(lens)))


LOW = (torch.bfloat16, torch.float16)
# table -> (its cases, the faults that cannot show in it).  A table without masks or causality has no masked key and no diagonal.
TABLES = {
    "causal mfma": ([c for dt in LOW for T in (129, 300) for c in causal_cases(dt, 4, 2, 128, T)]
                    + causal_cases(torch.bfloat16, 8, 1, 128, 129, ["stair8", "pair@127,128"]), ()),
    "causal generic": (causal_cases(torch.float32, 3, 3, 16, 70, CAUSAL_GENERIC_PROGRAMS)
                       + causal_cases(torch.bfloat16, 4, 2, 64, 70, CAUSAL_GENERIC_PROGRAMS), ()),
    "mha self": ([c for Dh in (64, 48) for T in (65, 200) for c in mha_cases(torch.bfloat16, Dh, T)] + mha_cases(torch.float16, 64, 65),
                 ("hole_seen", "past_diag")),
    "mha cross": ([c for q_len in (40, 65) for c in cross_cases(q_len)], ("hole_seen", "past_diag")),
    "seg512": (seg_cases(torch.bfloat16) + seg_cases(torch.float32), ("hole_seen", "past_diag")),
}


def out_rounded(pb: Problem, dt):
    """The fp64 forward rounded to the type: the `out` of the CPU tests."""
    return forward(pb.q, pb.k, pb.v, pb.allow, pb.scale).to(dt).float()


def judge(pb: Problem, out, got, dt, eta: Optional[float] = None):
    """(verdicts of `got` = (dq, dk, dv), kappa, the reference) of one problem under the as-given contract with this `out`."""
    ref = reference(pb.q, pb.k, pb.v, pb.dout, out, pb.allow, pb.scale)
    kap = kappa(ref, emulate(pb.q, pb.k, pb.v, pb.dout, out, pb.allow, pb.scale, torch.float32))
    return check(got, ref, dt, kap, eta), kap, ref
