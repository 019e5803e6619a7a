"""Cases for the row-wise and elementwise kernels (RMSNorm, RoPE, the LM loss, LayerNorm backward, column sums, the capped elementwise grids):
seeded inputs, float64 references, fp32 emulations of what the kernels compute, and the slips — each emulation wrong in one way such a kernel can
be wrong.  Pure torch on the CPU; imports nothing of the library.

The `*_verdict` functions hold every assertion tests/test_rowwise_gpu.py makes about an op's result.  tests/test_rowwise_cpu.py feeds them the
emulations (every bar must be attainable by the arithmetic) and the slips (every slip must be caught by a case of its family): the same code judges
the kernel on the GPU and its stand-ins on the CPU.

Inputs.  `ladder`: row r scaled by 10^(-3 + 6 r / (rows - 1)) and one all-zero row (row rows // 2) — rows whose mean square is far below eps, far
above it, and zero.  `lm_inputs(..., hot=True)`: logits randn * 30, whose exponentials overflow fp32 unless the row maximum is subtracted first.
Errors.  `row_err`: max_i |err_ri| / max_i |ref_ri| per row r, then the worst row — a row whose statistics are wrong cannot hide behind a larger
row.  Whole-tensor figures go through parity.close (logged under SETOK_PARITY_LOG like the per-row ones)."""
import functools
import math
import os

import torch
import torch.nn.functional as F

import parity
import setok_oracle as O

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTS = [F32, BF16, F16]
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
EW = {F32: 2e-6, BF16: 8e-3, F16: 8e-3}            # the project's elementwise bars (tests/test_llama_bwd_gpu.py)
EPS = 1e-5
CAP = 1 << 24                                      # work items of a capped launch: 65536 workgroups of 256


def vec(dt):
    """Elements of one 16-byte access."""
    return 4 if dt == F32 else 8


def rnd(t, dt):
    """One rounding to the element type, back in fp32."""
    return t.to(dt).float()


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def zero_row(rows):
    return rows // 2 if rows >= 3 else None


def ladder_scales(rows):
    if rows == 1:
        return torch.ones(1)
    s = 10.0 ** (-3.0 + 6.0 * torch.arange(rows, dtype=torch.float64) / (rows - 1))
    if zero_row(rows) is not None:
        s[zero_row(rows)] = 0.0
    return s.float()


@functools.lru_cache(maxsize=2)
def _ladder32(rows, C, seed, offset, spread):
    return (randn(rows, C, seed=seed) * spread + offset) * ladder_scales(rows)[:, None]


def ladder(rows, C, seed, dt, offset=0.0, spread=1.0):
    """(rows, C) in `dt`: (spread randn + offset) times the row's scale."""
    return _ladder32(rows, C, seed, offset, spread).to(dt)


# ---- errors and the verdict's bookkeeping ---------------------------------------------------------------------------------------------------
def row_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return float(((got - ref).abs().amax(-1) / ref.abs().amax(-1).clamp_min(1e-30)).max())


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def log(label, *nums):
    path = os.environ.get("SETOK_PARITY_LOG")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as f:
            f.write(f"{test}\t{label}\t" + "\t".join(f"{n:.3e}" for n in nums) + "\n")
    print(label, *[f"{n:.3e}" for n in nums])


class Findings:
    """Collects what a verdict finds wrong, so that one case over its bar does not hide the next; `worst` keeps the largest per-row figure."""

    def __init__(self):
        self.bad = []
        self.worst = 0.0

    def rows(self, label, got, ref, tol):
        e = row_err(got, ref)
        self.worst = max(self.worst, e) if e == e else float("nan")
        log(label + ": per-row, bound", e, tol)
        if not e < tol:
            self.bad.append(f"{label}: per-row {e:.3e} (bound {tol:.1e})")

    def whole(self, label, got, ref, tol):
        try:
            parity.close(got.detach().cpu(), ref, tol, label)
        except AssertionError as e:
            self.bad.append(f"{label}: {e}")

    def rel(self, label, got, ref, tol):
        e = rel(got, ref)
        log(label + ": max-rel, bound", e, tol)
        if not e < tol:
            self.bad.append(f"{label}: max-rel {e:.3e} (bound {tol:.1e})")

    def true(self, label, cond):
        if not bool(cond):
            self.bad.append(label)

    def same(self, label, a, b):
        if not (a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))):
            self.bad.append(f"{label}: bits differ")

    def zeros(self, label, t):
        if t.numel() and not float(t.float().abs().max()) == 0.0:
            self.bad.append(f"{label}: not exact zeros")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ---- RMSNorm ---------------------------------------------------------------------------------------------------------------------------------
#   forward, the generic kernel: a lane makes 0, 1 or several trips of 64 VEC columns (C = 8: 1 lane of a wave at work in bf16, 264: 33 lanes);
#   the rows kernel (16-bit, C 2048 / 4096 / 5120, rows >= 1024): 1029 = one row past a whole workgroup, 8197 = past the 8192 waves of the grid
RMS_GENERIC = [(r, c) for r in (1, 5, 37, 1023) for c in (8, 264, 520, 4096)]
RMS_ROWS = [(r, c) for c in (2048, 4096, 5120) for r in (1024, 1029, 8197)]
RMS_BWD = [(r, c) for r in (1, 5, 37, 1029) for c in (8, 264, 520, 4096, 5120)]
RMS_SLIPS = ("first_trip", "padded_width", "no_eps", "no_rnd_w")
RMS_BWD_SLIPS = ("first_trip", "padded_width", "no_eps")


def rms_inputs(rows, C, dt):
    """x on the ladder in `dt`; the weight in fp32 and NOT representable in 16 bits: the kernels round it to `dt` themselves."""
    return ladder(rows, C, rows * 7 + C, dt), 1 + 0.1 * randn(C, seed=C + 2)


def rms_checked_rows(rows):
    """The rows compared with float64: all of them, or — past 8192 rows — the first 8, the last 9, the zero row and its neighbours."""
    if rows <= 2048:
        return torch.arange(rows)
    z = zero_row(rows)
    return torch.cat([torch.arange(8), torch.arange(z - 1, z + 2), torch.arange(rows - 9, rows)])


def rms_ref(x, w, eps=EPS):
    """float64: w * x * rsqrt(mean(x^2) + eps)."""
    x, w = x.double(), w.double()
    return w * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def _rms_rstd(xf, C, dt, eps, slip):
    stat = xf[:, :64 * vec(dt)] if slip == "first_trip" else xf
    width = -(-C // (64 * vec(dt))) * 64 * vec(dt) if slip == "padded_width" else C
    return torch.rsqrt(stat.pow(2).sum(-1, keepdim=True) / width + (0.0 if slip == "no_eps" else eps))


def rms_emulate(x, w32, dt, eps=EPS, slip=None):
    """rmsnorm_kernel in fp32: rnd(w) * rnd(x rstd), rounded."""
    xf = x.float()
    rstd = _rms_rstd(xf, x.shape[1], dt, eps, slip)
    w = w32 if slip == "no_rnd_w" else rnd(w32, dt)
    return (w * rnd(xf * rstd, dt)).to(dt)


def rms_verdict(f, label, got, x, w32, dt):
    """got, x: the rows to judge (rms_checked_rows of the result and of the input)."""
    got, wd = got.detach().cpu(), w32.to(dt)
    f.true(label + ": dtype", got.dtype == dt)
    ref = rms_ref(x, wd)
    f.rows(label + " vs fp64", got, ref, EW[dt])
    f.whole(label + " vs fp64", got, ref, EW[dt])
    zero = x.float().abs().amax(-1) == 0
    f.zeros(label + " zero row", got[zero])
    if dt != F32:
        # the eager 16-bit graph rounds where the kernel does: the two differ where an fp32 ulp of rstd moves a rounding, by one ulp of that element
        eager = O.llama_rmsnorm(x, wd, EPS).float()
        ulp = 2.0 ** -7 if dt == BF16 else 2.0 ** -10
        f.true(label + ": more than one ulp of the row's largest output from the eager graph",
               ((got.float() - eager).abs().amax(-1) <= ulp * eager.abs().amax(-1)).all())
        # ... and rarely: a kernel that multiplied by the UNrounded weight stays inside that ulp but agrees with the eager graph of the unrounded
        # weight more often than with the real one
        unrounded = (w32 * O.llama_rmsnorm(x, torch.ones_like(wd), EPS).float()).to(dt).float()
        n_eager, n_unrounded = int((got.float() != eager).sum()), int((got.float() != unrounded).sum())
        f.true(label + f": {n_eager} elements differ from the eager graph, {n_unrounded} from the graph with the unrounded weight",
               n_eager < n_unrounded if got.numel() >= 1024 else n_eager <= n_unrounded)


def rms_bwd_inputs(rows, C, dt):
    x, w32 = rms_inputs(rows, C, dt)
    return x, w32, randn(rows, C, seed=C + 3).to(dt), randn(rows, C, seed=C + 4).to(dt)


def rms_bwd_ref(x, w, dy, dt, eps=EPS):
    """float64 autograd through the forward's formula, from the gradient at the forward's rounding point: g = (dy * w).to(dt), the one rounding
    that rmsnorm_bwd_kernel documents and the eager 16-bit graph makes (exact in fp32: no rounding there)."""
    g = dy.double() * w.double()
    g = g if dt == F32 else g.to(dt).double()
    xr = x.double().requires_grad_(True)
    with torch.enable_grad():
        xhat = xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + eps)
        (dx,) = torch.autograd.grad((xhat * g).sum(), xr)
    return dx


def rms_bwd_emulate(x, w32, dy, dres, dt, eps=EPS, slip=None):
    """rmsnorm_bwd_kernel in fp32: g = rnd(dy rnd(w)), dx = rnd(rstd (g - x k)) [+ dres, rounded]."""
    xf, C = x.float(), x.shape[1]
    rstd = _rms_rstd(xf, C, dt, eps, slip)
    width = -(-C // (64 * vec(dt))) * 64 * vec(dt) if slip == "padded_width" else C
    g = rnd(dy.float() * rnd(w32, dt), dt)
    dot = (g * xf)[:, :64 * vec(dt)] if slip == "first_trip" else g * xf
    k = dot.sum(-1, keepdim=True) * rstd * rstd / width
    v = rnd(rstd * (g - xf * k), dt)
    return (v if dres is None else v + dres.float()).to(dt)


def rms_bwd_verdict(f, label, got, x, w32, dy, dres, dt):
    got = got.detach().cpu()
    ref = rms_bwd_ref(x, w32.to(dt), dy, dt)
    ref = ref if dres is None else ref + dres.double()
    f.true(label + ": dtype and shape", got.dtype == dt and got.shape == x.shape)
    f.rows(label + " vs fp64", got, ref, EW[dt])
    f.whole(label + " vs fp64", got, ref, EW[dt])


# ---- RoPE ------------------------------------------------------------------------------------------------------------------------------------
#   Dh / 2 = 3: the scalar kernel in every dtype; 4 and 12: the vector kernel in fp32, the scalar one in 16 bits; 16, 64, 128: vector everywhere
ROPE_HEADS = [(3, 3, 6), (2, 1, 8), (4, 2, 24), (3, 3, 32), (4, 2, 128), (2, 2, 256)]
ROPE_ROWS = [1, 50, 257]
ROPE_TOL = {F32: 2e-5, BF16: 1e-2, F16: 1e-2}      # tests/test_llama_gpu.py::test_rope
ROPE_BWD_TOL = {F32: 4e-5, BF16: 1e-2, F16: 1e-2}  # tests/test_llama_bwd_gpu.py::test_rope_bwd_is_the_transpose_of_rope
# fp32 at head dim 32, where positions reach 3000: the reference's own tables round the angle to fp32 (half an ulp of 3000 is 1.2e-4 rad), so kernel and
# reference agree below that only where they form the SAME fp32 angle, and an inv_freq one ulp apart (exp2f against pow) shows times the position.
# The emulation below — the kernel's formula with torch's exp2 — is 3.062e-5 per row from the reference at these inputs, over the 2e-5 that
# test_rope's 50 rows meet; the bar there is four times the emulation's figure.  The transpose stays inside its existing 4e-5.
ROPE_TOL_FP32_DH32 = 4 * 3.062e-5
ROPE_SLIPS = ("sign",)
THETA = 10000.0


def rope_inputs(rows, H, Hkv, Dh, dt):
    """[q | k | v] rows and positions: up to 3000 at head dim 32, below 64 otherwise (the fp32 tables carry the rounding of inv_freq times the
    position: test_rope_bwd_is_the_transpose_of_rope); row 0 sits at position 0."""
    qkv = randn(rows, (H + 2 * Hkv) * Dh, seed=rows + Dh).to(dt)
    pos = torch.randint(0, 3000 if Dh == 32 else 64, (rows,), generator=torch.Generator().manual_seed(4 + rows))
    pos[0] = 0
    return qkv, pos


def rope_tol(dt, Dh, backward=False):
    if dt == F32 and Dh == 32 and not backward:
        return ROPE_TOL_FP32_DH32
    return (ROPE_BWD_TOL if backward else ROPE_TOL)[dt]


def _rope_apply(x, cos, sin, sign):
    return x * cos + sign * O._rotate_half(x) * sin


def rope_ref(qkv, pos, H, Hkv, Dh, dt, backward=False):
    """float64 on the rotated part (rows, H + Hkv, Dh) with the oracle's tables in `dt`; the transpose rotates back."""
    cos, sin = O.llama_rope_tables(pos[None], Dh, THETA, dt)
    x = qkv[:, :(H + Hkv) * Dh].reshape(-1, H + Hkv, Dh).double()
    return _rope_apply(x, cos[0][:, None].double(), sin[0][:, None].double(), -1.0 if backward else 1.0).reshape(qkv.shape[0], -1)


def rope_emulate(qkv, pos, H, Hkv, Dh, dt, backward=False, slip=None):
    """rope_kernel / rope_bwd_kernel in fp32: the angle from exp2f as the kernels form it, every product rounded, then the sum."""
    half = Dh // 2
    d = torch.arange(half, dtype=torch.float32)
    inv = 1.0 / torch.exp2(torch.tensor(math.log2(THETA), dtype=torch.float32) * (2 * d) / float(Dh))
    ang = pos.float()[:, None] * inv[None]
    c, s = rnd(torch.cos(ang), dt)[:, None], rnd(torch.sin(ang), dt)[:, None]
    sign = (-1.0 if backward else 1.0) * (-1.0 if slip == "sign" else 1.0)
    out = qkv.clone()
    x = qkv[:, :(H + Hkv) * Dh].reshape(-1, H + Hkv, Dh).float()
    x1, x2 = x[..., :half], x[..., half:]
    o1 = rnd(x1 * c, dt) + rnd(-sign * x2 * s, dt)
    o2 = rnd(x2 * c, dt) + rnd(sign * x1 * s, dt)
    out[:, :(H + Hkv) * Dh] = torch.cat([o1, o2], -1).to(dt).reshape(qkv.shape[0], -1)
    return out


def rope_verdict(f, label, got, qkv, pos, H, Hkv, Dh, dt, backward=False):
    got, W = got.detach().cpu(), (H + Hkv) * Dh
    tol = rope_tol(dt, Dh, backward)
    ref = rope_ref(qkv, pos, H, Hkv, Dh, dt, backward)
    f.rows(label + " vs fp64", got[:, :W], ref, tol)
    f.whole(label + " vs fp64", got[:, :W], ref, tol)
    f.same(label + ": v part", got[:, W:], qkv[:, W:])
    f.same(label + ": rows at position 0", got[pos == 0], qkv[pos == 0])


# ---- LM loss -----------------------------------------------------------------------------------------------------------------------------------
#   V = 32003 / 4099: contiguous rows start off the 16-byte grid; V > 2048 (1024 in fp32): a thread's vector loop makes several trips;
#   B T = 650 > 256: the reduce kernel's thread loop makes several trips
LM_CASES = [(2, 6, 32003), (2, 6, 32000), (1, 5, 4099), (5, 130, 40)]
LM_TOL = 2e-6
LM_UP = 0.7                                        # the upstream gradient of the backward cases
LM_SLIPS = ("no_max", "vocab_first_trip", "rows_first_trip")


def lm_inputs(B, T, V, padding, hot, dt):
    """bf16-representable logits (clamped to the fp16 range for that dtype), labels with a -100 prompt stretch and scattered -100, a padding mask."""
    g = torch.Generator().manual_seed(B * 1000 + T + V + (7 if hot else 0))
    logits = (torch.randn(B, T, V, generator=g) * (30.0 if hot else 1.0)).bfloat16().float()
    if dt == F16:
        logits = logits.clamp(-65504.0, 65504.0).to(F16).float()      # (bf16 values under 2^-14 lose bits as fp16 subnormals)
    labels = torch.randint(0, V, (B, T), generator=g)
    labels[:, : T // 3] = -100
    labels[torch.rand(B, T, generator=g) < 0.1] = -100
    am = torch.ones(B, T, dtype=torch.long)
    for b in range(B):
        if padding == "right":
            am[b, T - 1 - b:] = 0
        else:
            am[b, : b + 1] = 0
    return logits, labels, am


def lm_counted(labels, am):
    """(B, T) bool: position t counts when token t + 1 is attended and its label is not -100."""
    c = torch.zeros_like(labels, dtype=torch.bool)
    c[:, :-1] = (am[:, 1:] != 0) & (labels[:, 1:] != -100)
    return c


def lm_ref(logits, labels, am, up=LM_UP):
    """float64 cross entropy over the counted positions (the reference's shift and mask), and up * its gradient by autograd."""
    x = logits.double().requires_grad_(True)
    with torch.enable_grad():
        keep = am[:, 1:] != 0
        loss = F.cross_entropy(x[:, :-1][keep], labels[:, 1:][keep], ignore_index=-100)
        (g,) = torch.autograd.grad(loss * up, x)
    return float(loss.detach()), g


def lm_emulate(logits, labels, am, dt, up=LM_UP, slip=None):
    """lm_loss_rows_kernel + lm_loss_reduce_kernel + lm_loss_bwd_kernel in fp32: ([loss, count], d logits in `dt`)."""
    B, T, V = logits.shape
    x = logits.to(dt).float().reshape(B * T, V)
    counted = lm_counted(labels, am).reshape(-1)
    target = torch.roll(labels.reshape(-1), -1).clamp_min(0)
    seen = x[:, :256 * vec(dt)] if slip == "vocab_first_trip" else x
    m = torch.zeros(B * T, 1) if slip == "no_max" else seen.amax(-1, keepdim=True)
    tot = torch.exp(seen - m).sum(-1, keepdim=True)
    loss_row = torch.where(counted, (m + torch.log(tot))[:, 0] - x.gather(1, target[:, None])[:, 0], torch.zeros(()))
    upto = 256 if slip == "rows_first_trip" else B * T
    n = counted[:upto].float().sum()
    out = torch.stack([loss_row[:upto].sum() / n, n])
    p = torch.exp(x - m) * (1.0 / tot)
    d = (up / n) * (p - F.one_hot(target, V).float())
    d = torch.where(counted[:, None], d, torch.zeros(()))
    return out, d.to(dt).reshape(B, T, V)


def lm_verdict(f, label, out, dlogits, logits, labels, am, dt, hot):
    out, dlogits = out.detach().float().cpu(), dlogits.detach().cpu()
    ref, gref = lm_ref(logits, labels, am)
    counted = lm_counted(labels, am)
    err = abs(float(out[0]) - ref)
    log(label + " loss: |err|, bound", err, LM_TOL * abs(ref) + 1e-6)
    f.true(label + f": loss {float(out[0])!r} vs {ref!r}", err <= LM_TOL * abs(ref) + 1e-6)
    f.true(label + f": count {float(out[1])} vs {int(counted.sum())}", float(out[1]) == float(counted.sum()))
    f.true(label + ": gradient dtype and shape", dlogits.dtype == dt and dlogits.shape == logits.shape)
    f.whole(label + " gradient vs fp64", dlogits, gref, EW[dt])
    f.zeros(label + ": uncounted rows", dlogits[~counted])
    f.true(label + ": every sequence's last position is uncounted", not counted[:, -1].any())
    if hot:
        f.true(label + ": finite", math.isfinite(float(out[0])) and torch.isfinite(dlogits.float()).all())


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------------------
#   C = 8 / 72: one partly idle chunk; 1280, 1536: three register chunks in bf16; the limit 64 VEC 4 (2048 in 16 bits, 1024 in fp32): all four;
#   1032 in 16 bits: a partly idle second chunk; rows > 1024: a wave walks several rows and accumulates dgamma / dbeta across them
LN_CASES = [(3, 8, DTS), (1030, 72, DTS), (5000, 512, DTS), (1030, 1280, [BF16, F16]), (2050, 1536, [BF16, F16]), (1030, 2048, [BF16, F16]),
            (1030, 1032, [BF16, F16]), (1030, 1024, [F32])]
LN_TOL = {F32: 2e-5, BF16: 2e-2, F16: 2e-2}        # tests/test_train_gpu.py::test_layernorm_bwd
LN_SLIPS = ("first_trip", "padded_width", "no_eps")


def ln_limit(dt):
    return 64 * vec(dt) * 4


def ln_inputs(rows, C, dt):
    return (ladder(rows, C, rows + C, dt, offset=0.3, spread=2.0), randn(rows, C, seed=C + 4).to(dt), randn(rows, C, seed=C + 5).to(dt),
            1 + 0.1 * randn(C, seed=C + 6))


def ln_ref(x, dy, gamma, eps=EPS):
    """float64 autograd through F.layer_norm: (dx, dgamma, dbeta)."""
    C = x.shape[1]
    xr, gr = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    br = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        F.layer_norm(xr, (C,), gr, br, eps).backward(dy.double())
    return xr.grad, gr.grad, br.grad


def ln_emulate(x, dy, res, gamma, dt, eps=EPS, slip=None):
    """layernorm_bwd_kernel in fp32: two-pass statistics, dx = rstd (g - mean g - xhat mean(g xhat)) + res rounded once, fp32 column sums."""
    xf, df, C = x.float(), dy.float(), x.shape[1]
    stat = xf[:, :64 * vec(dt)] if slip == "first_trip" else xf
    width = -(-C // (64 * vec(dt))) * 64 * vec(dt) if slip == "padded_width" else C
    mean = stat.sum(-1, keepdim=True) / width
    var = (stat - mean).pow(2).sum(-1, keepdim=True) / width
    rstd = 1.0 / torch.sqrt(var + (0.0 if slip == "no_eps" else eps))
    xh, g = (xf - mean) * rstd, df * gamma
    dx = rstd * (g - g.sum(-1, keepdim=True) / C - xh * ((g * xh).sum(-1, keepdim=True) / C)) + res.float()
    return dx.to(dt), (df * xh).sum(0), df.sum(0)


def ln_verdict(f, label, dx, dg, db, x, dy, res, gamma, dt, times=1):
    rdx, rdg, rdb = ln_ref(x, dy, gamma)
    tol = LN_TOL[dt]
    if dx is not None:
        f.rows(label + " dx vs fp64", dx.detach().cpu(), rdx + res.double(), tol)
        f.whole(label + " dx vs fp64", dx, rdx + res.double(), tol)
    f.rel(label + " dgamma", dg, times * rdg, max(tol, 1e-4))
    f.rel(label + " dbeta", db, times * rdb, max(tol, 1e-4))


# ---- column sums -------------------------------------------------------------------------------------------------------------------------------
#   chunks of the final kernel (quarters k & 3, pairs k, k + 4, then the odd one): rows 1 -> 1 chunk, 32 -> 1, 33 -> 2, 97 -> 4, 129 -> 5,
#   257 -> 9, 4096 -> 128 (the cap exactly), 4097 -> 125 (capped), 16384 -> 128, 16385 -> 33 (512-row chunks), 20000 -> 40
COLSUM_ROWS = [1, 32, 33, 97, 129, 257, 4096, 4097, 16384, 16385, 20000]
COLSUM_COLS = [8, 200, 257]
COLSUM_TOL = 1e-5                                  # tests/test_train_gpu.py::test_colsum_and_accumulate
COLSUM_SLIPS = ("last_chunk",)


def colsum_inputs(rows, cols, dt):
    return randn(rows, cols, seed=rows + cols).to(dt)


def colsum_plan(rows, ws_rows=128):
    """(chunks, rows per chunk) of setok_colsum."""
    chunks = min(-(-max(rows, 1) // (512 if rows > 16384 else 32)), ws_rows)
    rpc = -(-max(rows, 1) // chunks)
    return -(-max(rows, 1) // rpc), rpc


def colsum_emulate(x, slip=None):
    """fp32 partial sums per chunk, then their sum."""
    chunks, rpc = colsum_plan(x.shape[0])
    part = torch.stack([x[k * rpc:(k + 1) * rpc].float().sum(0) for k in range(chunks)])
    return part[:chunks - 1 if slip == "last_chunk" else chunks].sum(0)


def colsum_verdict(f, label, got, x, times=1):
    f.rel(label, got, times * x.double().sum(0), COLSUM_TOL)


# ---- capped grids ------------------------------------------------------------------------------------------------------------------------------
#   A launch is capped at 65536 x 256 = 2^24 work items; past that a thread strides to a second item.  The big call is compared bit for bit with the
#   same data sent in slices under the cap (on the GPU), and with float64 on three windows of 4096 items: the start, across item 2^24, the end.
CAP_SLIPS = ("first_cap",)
WINDOW = 4096


def windows(n_items):
    assert n_items > CAP
    return [(0, WINDOW), (CAP - WINDOW // 2, min(CAP + WINDOW // 2, n_items)), (n_items - WINDOW, n_items)]


def cap_slip(out, first_item, per_item):
    """Only the first 2^24 items written: the rest of a window of `out` (starting at item `first_item`, `per_item` elements each) stays zero."""
    out = out.clone().reshape(-1)
    keep = max(0, min(out.numel(), (CAP - first_item) * per_item))
    out[keep:] = 0
    return out


def gelu_bwd_ref(pre, dy):
    x = pre.double()
    return dy.double() * (0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))


def gelu_ref(x):
    return F.gelu(x.double())


def swiglu_pairs_bwd_ref(pairs, dout):
    """pairs (n, 2 F) of (gate_j, up_j), dout (n, F): float64 d pairs."""
    p = pairs.double()
    gate, up, go = p[..., 0::2], p[..., 1::2], dout.double()
    s = torch.sigmoid(gate)
    return torch.stack([go * up * s * (1 + gate * (1 - s)), go * gate * s], -1).reshape(p.shape)


ADAMW = dict(lr=1e-2, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.1, step=3, grad_scale=0.5)


def adamw_ref(p, g, m, v):
    """float64: one decoupled-weight-decay Adam step -> (p, m, v)."""
    h = ADAMW
    p, g, m, v = p.double(), g.double() * h["grad_scale"], m.double(), v.double()
    m = h["beta1"] * m + (1 - h["beta1"]) * g
    v = h["beta2"] * v + (1 - h["beta2"]) * g * g
    p = p * (1 - h["lr"] * h["weight_decay"]) - h["lr"] * (m / (1 - h["beta1"] ** h["step"])) / ((v / (1 - h["beta2"] ** h["step"])).sqrt() + h["eps"])
    return p, m, v


CAP_TOL = {"gelu_bwd": {F32: 1e-5, BF16: 1e-2, F16: 1e-2},           # tests/test_train_gpu.py::test_gelu_bwd
           "activation": {F32: 1e-5, BF16: 1e-2, F16: 1e-2},         # the forward twin, the same bars
           "swiglu_pairs_bwd": EW,                                   # tests/test_llama_bwd_gpu.py::test_swiglu_pairs_bwd
           "adamw": {F32: 1e-6}}                                     # tests/test_train_gpu.py::test_adamw_matches_torch


def window_verdict(f, label, got, ref, tol):
    """One window: elementwise results have no row structure, so the whole-window figures of parity.close."""
    f.whole(label, got, ref, tol)


# ---- the slips, by family: what each name gets wrong (tests/test_rowwise_cpu.py runs every one through its family's verdict) -------------------
SLIPS = {"rmsnorm": RMS_SLIPS, "rmsnorm_bwd": RMS_BWD_SLIPS, "rope": ROPE_SLIPS, "lm_loss": LM_SLIPS, "layernorm_bwd": LN_SLIPS,
         "colsum": COLSUM_SLIPS, "capped grids": CAP_SLIPS}
SLIP_MEANS = {"first_trip": "only the first 64 VEC columns of a row enter the statistics",
              "padded_width": "the statistics are divided by the width padded to a multiple of 64 VEC",
              "no_eps": "eps dropped",
              "no_rnd_w": "the weight is not rounded to the element type before the multiply",
              "sign": "rotate-half sign flipped",
              "no_max": "row maximum not subtracted before the exponentials",
              "vocab_first_trip": "only the first 256 VEC vocabulary entries enter the maximum and the sum",
              "rows_first_trip": "only the first 256 positions are reduced",
              "last_chunk": "the last chunk of partial column sums dropped",
              "first_cap": "only the first 2^24 items written"}
assert {s for family in SLIPS.values() for s in family} == set(SLIP_MEANS)
