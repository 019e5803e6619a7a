"""The row-wise and elementwise kernels on the paths the real workloads take, on a real MI355X: RMSNorm (the generic kernel at one, several and
partial trips of a lane; the 16-bit rows kernel at C = 2048 / 4096 / 5120, past one workgroup and past the 8192 waves of its capped grid; the
backward with and without the residual gradient, in place), RoPE (scalar and vector kernels, forward and transpose), the LM loss and its gradient
(vocabularies of several vector trips, misaligned rows, more than 256 positions, logits that overflow without the row maximum), LayerNorm backward
(every register-chunk count up to the limit), column sums (every chunk-count edge of the final kernel, both chunk sizes, the workspace cap) and the
elementwise launches past their 2^24-item grid cap.

Inputs, float64 references and every assertion about a result live in tests/rowwise_cases.py (the `*_verdict` functions);
tests/test_rowwise_cpu.py shows on the CPU that an fp32 emulation of each kernel meets them and that each way of getting the kernel wrong does not.
What only the GPU can show is asserted here: equal bits on a second run, in place, in slices (one big call against the same rows or items sent in
pieces that take the other kernel or stay under the grid cap).  Every figure goes to SETOK_PARITY_LOG (profiles/rowwise_parity.txt).
`pytest -m gpu`."""
import pytest
import torch

import rowwise_cases as RC

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib, ops

DEV = "cuda"
DTS = pytest.mark.parametrize("dt", RC.DTS, ids=[RC.NAME[d] for d in RC.DTS])


def _shape_id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else None


# ---- RMSNorm --------------------------------------------------------------------------------------------------------------------------------
def _rmsnorm_case(dt, rows, C, sliced):
    x, w32 = RC.rms_inputs(rows, C, dt)
    dx, dw = x.to(DEV), w32.to(DEV)
    got = ops.rmsnorm(dx, dw, RC.EPS)
    f, label, sel = RC.Findings(), f"rmsnorm {RC.NAME[dt]} {rows}x{C}", RC.rms_checked_rows(rows)
    RC.rms_verdict(f, label, got.cpu()[sel], x[sel], w32, dt)
    f.same(label + " second run", ops.rmsnorm(dx, dw, RC.EPS), got)
    if sliced:                             # slices of <= 1000 rows take the generic kernel: a row's bits must not depend on the batch around it
        parts = torch.cat([ops.rmsnorm(dx[i:i + 1000], dw, RC.EPS) for i in range(0, rows, 1000)])
        f.same(label + " one call against slices of 1000 rows", got, parts)
    f.done()


@DTS
@pytest.mark.parametrize("shape", RC.RMS_GENERIC, ids=_shape_id)
def test_rmsnorm_generic_kernel(dt, shape):
    _rmsnorm_case(dt, *shape, sliced=False)


@DTS
@pytest.mark.parametrize("shape", RC.RMS_ROWS, ids=_shape_id)
def test_rmsnorm_rows_kernel_equals_the_generic_kernel(dt, shape):
    """The 16-bit rows kernel (fp32 has none: the same shapes route to the generic kernel and must be right all the same)."""
    _rmsnorm_case(dt, *shape, sliced=True)


@DTS
@pytest.mark.parametrize("shape", RC.RMS_BWD, ids=_shape_id)
def test_rmsnorm_bwd(dt, shape):
    rows, C = shape
    x, w32, dy, dres = RC.rms_bwd_inputs(rows, C, dt)
    dx, dw, ddy, dr = x.to(DEV), w32.to(DEV), dy.to(DEV), dres.to(DEV)
    f, label = RC.Findings(), f"rmsnorm_bwd {RC.NAME[dt]} {rows}x{C}"
    plain = ops.rmsnorm_bwd(dx, dw, ddy, RC.EPS)
    both = ops.rmsnorm_bwd(dx, dw, ddy, RC.EPS, dres=dr)
    RC.rms_bwd_verdict(f, label, plain, x, w32, dy, None, dt)
    RC.rms_bwd_verdict(f, label + " +dres", both, x, w32, dy, dres, dt)
    buf = ddy.clone()
    f.same(label + " in place of dy", ops.rmsnorm_bwd(dx, dw, buf, RC.EPS, out=buf), plain)
    buf = ddy.clone()
    f.same(label + " +dres in place of dy", ops.rmsnorm_bwd(dx, dw, buf, RC.EPS, dres=dr, out=buf), both)
    buf = dr.clone()
    f.same(label + " +dres in place of dres", ops.rmsnorm_bwd(dx, dw, ddy, RC.EPS, dres=buf, out=buf), both)
    f.done()


# ---- RoPE -----------------------------------------------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("heads", RC.ROPE_HEADS, ids=_shape_id)
def test_rope_forward_and_transpose(dt, heads):
    H, Hkv, Dh = heads
    f = RC.Findings()
    for rows in RC.ROPE_ROWS:
        qkv, pos = RC.rope_inputs(rows, H, Hkv, Dh, dt)
        d, dpos = qkv.to(DEV), pos.to(DEV)
        label = f"rope {RC.NAME[dt]} H{H} Hkv{Hkv} Dh{Dh} rows{rows}"
        y = ops.rope_(d.clone(), dpos, H, Dh, RC.THETA, Hkv)
        RC.rope_verdict(f, label, y, qkv, pos, H, Hkv, Dh, dt)
        f.same(label + " second run", ops.rope_(d.clone(), dpos, H, Dh, RC.THETA, Hkv), y)
        g = ops.rope_bwd_(d.clone(), dpos, H, Dh, RC.THETA, Hkv)
        RC.rope_verdict(f, label + " bwd", g, qkv, pos, H, Hkv, Dh, dt, backward=True)
        back = ops.rope_bwd_(y.clone(), dpos, H, Dh, RC.THETA, Hkv)
        f.rows(label + " there and back", back.cpu(), qkv.double(), 2 * RC.ROPE_TOL[dt])
    f.done()


# ---- LM loss ----------------------------------------------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("case", RC.LM_CASES, ids=_shape_id)
def test_lm_loss_and_gradient(dt, case):
    B, T, V = case
    f = RC.Findings()
    up = torch.tensor(RC.LM_UP, device=DEV)
    for padding in ("right", "left"):
        for hot in (False, True):
            logits, labels, am = RC.lm_inputs(B, T, V, padding, hot, dt)
            dlab, dam = labels.to(DEV), am.to(DEV)
            contiguous = logits.to(dt).to(DEV).contiguous()
            Vp = (V + 7) // 8 * 8 + 8
            buf = torch.zeros(B, T, Vp, dtype=dt, device=DEV)
            buf[..., :V] = contiguous
            results = []
            for layout, dev in (("contiguous", contiguous), ("strided", buf[..., :V])):
                label = f"lm_loss {RC.NAME[dt]} B{B} T{T} V{V} {padding} {'hot' if hot else 'unit'} {layout}"
                out = ops.lm_loss(dev, dlab, dam)
                d = ops.lm_loss_bwd(dev, dlab, dam, out, upstream=up)
                RC.lm_verdict(f, label, out, d, logits, labels, am, dt, hot)
                f.same(label + " loss, second run", ops.lm_loss(dev, dlab, dam), out)
                f.same(label + " gradient, second run", ops.lm_loss_bwd(dev, dlab, dam, out, upstream=up), d)
                results.append(d)
            f.same(label + " gradient against the contiguous rows'", results[1], results[0])   # (the loss may differ: the head | vectors | tail split moves)
    f.done()


# ---- LayerNorm backward -----------------------------------------------------------------------------------------------------------------------
LN = [(rows, C, dt) for rows, C, dts in RC.LN_CASES for dt in dts]


@pytest.mark.parametrize("rows,C,dt", LN, ids=[f"{r}x{c}-{RC.NAME[d]}" for r, c, d in LN])
def test_layernorm_bwd(rows, C, dt):
    x, dy, res, gamma = RC.ln_inputs(rows, C, dt)
    dx_, ddy, dres, dgam = x.to(DEV), dy.to(DEV), res.to(DEV), gamma.to(DEV)
    f, label = RC.Findings(), f"layernorm_bwd {RC.NAME[dt]} {rows}x{C}"
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    dx = ops.layernorm_bwd(dx_, ddy, dgam, RC.EPS, dg, db, accumulate=False, res=dres)
    RC.ln_verdict(f, label, dx, dg, db, x, dy, res, gamma, dt)
    once_g, once_b = dg.clone(), db.clone()
    assert ops.layernorm_bwd(dx_, ddy, dgam, RC.EPS, dg, db, accumulate=True, need_dx=False) is None
    f.same(label + " dgamma accumulated twice", dg, 2 * once_g)
    f.same(label + " dbeta accumulated twice", db, 2 * once_b)
    dg2, db2 = torch.full((C,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV)
    ops.layernorm_bwd(dx_, ddy, dgam, RC.EPS, dg2, db2, accumulate=False, need_dx=False)
    f.same(label + " dgamma without dx", dg2, once_g)
    f.same(label + " dbeta without dx", db2, once_b)
    f.done()


@DTS
def test_layernorm_bwd_refuses_a_width_over_its_limit(dt):
    C = RC.ln_limit(dt) + 8
    x = torch.zeros(4, C, dtype=dt, device=DEV)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    with pytest.raises(_lib.SetokHipError, match="unsupported"):
        ops.layernorm_bwd(x, x, torch.ones(C, device=DEV), RC.EPS, dg, db, accumulate=False)


# ---- column sums ------------------------------------------------------------------------------------------------------------------------------
@DTS
@pytest.mark.parametrize("rows", RC.COLSUM_ROWS)
def test_colsum_chunk_edges(dt, rows):
    f = RC.Findings()
    pad = 16 if dt == RC.F32 else 64
    for cols in RC.COLSUM_COLS:
        x = RC.colsum_inputs(rows, cols, dt)
        dx = x.to(DEV)
        label = f"colsum {RC.NAME[dt]} {rows}x{cols}"
        out = ops.colsum(dx)
        RC.colsum_verdict(f, label, out, x)
        f.same(label + " second run", ops.colsum(dx), out)
        ops.colsum(dx, out=out, accumulate=True)
        RC.colsum_verdict(f, label + " accumulated twice", out, x, times=2)
        xt, cs = ops.transpose(dx, pad, with_colsum=True)
        RC.colsum_verdict(f, label + " inside transpose", cs, x)
        ldo = (rows + pad - 1) // pad * pad
        f.true(label + ": the transpose itself", xt.shape == (cols, ldo) and torch.equal(xt[:, :rows].cpu(), x.t()) and not bool(xt[:, rows:].any()))
    f.done()


# ---- capped grids -----------------------------------------------------------------------------------------------------------------------------
def _dev_randn(*shape, seed, dt, scale=1.0):
    return (torch.randn(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * scale).to(dt)


def _in_slices(n, step, run):
    """cat of run(lo, hi) over [0, n) in pieces of `step`."""
    return torch.cat([run(lo, min(lo + step, n)) for lo in range(0, n, step)])


@DTS
def test_gelu_bwd_past_the_grid_cap(dt):
    n = RC.CAP + 1000
    pre, dy = _dev_randn(n, seed=1, dt=dt, scale=2.0), _dev_randn(n, seed=2, dt=dt)
    f, label = RC.Findings(), f"gelu_bwd {RC.NAME[dt]} n={n}"
    big = ops.gelu_bwd(pre, dy)
    f.same(label + " one call against slices under the cap", big, _in_slices(n, 1 << 23, lambda lo, hi: ops.gelu_bwd(pre[lo:hi], dy[lo:hi])))
    for lo, hi in RC.windows(n):
        RC.window_verdict(f, f"{label} items {lo}..{hi}", big[lo:hi], RC.gelu_bwd_ref(pre[lo:hi].cpu(), dy[lo:hi].cpu()), RC.CAP_TOL["gelu_bwd"][dt])
    f.done()


@DTS
def test_activation_past_the_grid_cap(dt):
    n = RC.CAP + 1000
    x = _dev_randn(n, seed=3, dt=dt, scale=2.0)
    f, label = RC.Findings(), f"activation gelu_erf {RC.NAME[dt]} n={n}"
    big = ops.activation(x, ops.ACT_GELU_ERF)
    f.same(label + " one call against slices under the cap", big, _in_slices(n, 1 << 23, lambda lo, hi: ops.activation(x[lo:hi], ops.ACT_GELU_ERF)))
    for lo, hi in RC.windows(n):
        RC.window_verdict(f, f"{label} items {lo}..{hi}", big[lo:hi], RC.gelu_ref(x[lo:hi].cpu()), RC.CAP_TOL["activation"][dt])
    f.done()


@DTS
def test_swiglu_pairs_bwd_past_the_grid_cap(dt):
    """An item is one thread's VEC outputs: 2 VEC consecutive elements of the pairs, VEC of dout."""
    v, Fd = RC.vec(dt), 8192
    rows = 8200 if dt == RC.F32 else 16400
    n = rows * (Fd // v)
    assert n > RC.CAP and (rows // 2) * (Fd // v) < RC.CAP
    pre, dout = _dev_randn(rows, 2 * Fd, seed=4, dt=dt, scale=2.0), _dev_randn(rows, Fd, seed=5, dt=dt)
    f, label = RC.Findings(), f"swiglu_pairs_bwd {RC.NAME[dt]} {rows}x{Fd}"
    big = ops.swiglu_pairs_bwd(pre, dout)
    f.same(label + " one call against slices under the cap", big,
           _in_slices(rows, rows // 2, lambda lo, hi: ops.swiglu_pairs_bwd(pre[lo:hi], dout[lo:hi])))
    for lo, hi in RC.windows(n):
        pw, gw = pre.view(-1)[lo * 2 * v:hi * 2 * v].view(-1, 2 * v).cpu(), dout.view(-1)[lo * v:hi * v].view(-1, v).cpu()
        RC.window_verdict(f, f"{label} items {lo}..{hi}", big.view(-1)[lo * 2 * v:hi * 2 * v].view(-1, 2 * v), RC.swiglu_pairs_bwd_ref(pw, gw),
                          RC.CAP_TOL["swiglu_pairs_bwd"][dt])
    f.done()


@pytest.mark.parametrize("lp", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_adamw_past_the_grid_cap(lp):
    n = RC.CAP + 257
    h = RC.ADAMW
    p0, g = _dev_randn(n, seed=6, dt=RC.F32), _dev_randn(n, seed=7, dt=RC.F32)
    m0, v0 = _dev_randn(n, seed=8, dt=RC.F32, scale=0.1), _dev_randn(n, seed=9, dt=RC.F32, scale=0.01).abs()
    args = (h["lr"], h["beta1"], h["beta2"], h["eps"], h["weight_decay"], h["step"])

    def step(pieces):
        p, m, v, low = p0.clone(), m0.clone(), v0.clone(), torch.zeros(n, dtype=lp, device=DEV)
        for lo in range(0, n, pieces):
            s = slice(lo, min(lo + pieces, n))
            ops.adamw(p[s], g[s], m[s], v[s], low[s], *args, grad_scale=h["grad_scale"])
        return p, m, v, low

    f, label = RC.Findings(), f"adamw {RC.NAME[lp]} copy n={n}"
    big, parts = step(n), step(1 << 23)
    for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "low-precision copy"), big, parts):
        f.same(f"{label} {name}: one call against slices under the cap", a, b)
    f.same(label + ": the low-precision copy is the rounded parameter", big[3], big[0].to(lp))
    for lo, hi in RC.windows(n):
        ref = RC.adamw_ref(p0[lo:hi].cpu(), g[lo:hi].cpu(), m0[lo:hi].cpu(), v0[lo:hi].cpu())
        for name, a, r in zip(("param", "exp_avg", "exp_avg_sq"), big, ref):
            RC.window_verdict(f, f"{label} {name} items {lo}..{hi}", a[lo:hi], r, RC.CAP_TOL["adamw"][RC.F32])
    f.done()


@DTS
def test_dropout_family_past_the_grid_cap(dt):
    """setok_dropout, setok_activation_dropout and setok_gelu_bwd_dropout cap their grids at 2^24 VECTORS of 16 bytes (the element-by-element
    dropout of a misaligned view at 2^24 elements).  The mask is a pure function of (seed, offset + i), so a slice with its own offset must give the
    big call's bits; on the windows a kept element is x / (1 - p) rounded once, about 1 - p of them are kept, and the fused forms equal their
    two-launch forms."""
    v, p, seed = RC.vec(dt), 0.2, 11
    n = v * RC.CAP + 1003
    x, gr = _dev_randn(n, seed=12, dt=dt, scale=2.0), _dev_randn(n, seed=13, dt=dt)
    f, label = RC.Findings(), f"dropout {RC.NAME[dt]} n={n}"
    step = 1 << 25
    drop = ops.dropout(x, p, seed, offset=5)
    f.same(label + " one call against slices under the cap", drop, _in_slices(n, step, lambda lo, hi: ops.dropout(x[lo:hi], p, seed, offset=5 + lo)))
    act = ops.activation_dropout(x, ops.ACT_GELU_ERF, p, seed, offset=5)
    f.same(label + " activation_dropout against slices", act,
           _in_slices(n, step, lambda lo, hi: ops.activation_dropout(x[lo:hi], ops.ACT_GELU_ERF, p, seed, offset=5 + lo)))
    bwd = ops.gelu_bwd_dropout(x, gr, p, seed, offset=5)
    f.same(label + " gelu_bwd_dropout against slices", bwd,
           _in_slices(n, step, lambda lo, hi: ops.gelu_bwd_dropout(x[lo:hi], gr[lo:hi], p, seed, offset=5 + lo)))
    scale = (torch.ones((), dtype=torch.float32) / (1.0 - torch.tensor(p, dtype=torch.float32))).item()
    for lo, hi in RC.windows(n // v):
        s = slice(lo * v, min(hi * v + v, n))                                               # (the last window takes the n mod VEC tail along)
        kept = drop[s] != 0
        f.same(f"{label} kept elements of items {lo}..{hi}", drop[s][kept], (x[s].float() * scale).to(dt)[kept])
        f.true(f"{label} items {lo}..{hi}: {float(kept.float().mean()):.4f} kept", abs(float(kept.float().mean()) - (1 - p)) < 0.02)
        f.same(f"{label} activation_dropout == activation, dropout on items {lo}..{hi}", act[s],
               ops.dropout(ops.activation(x[s], ops.ACT_GELU_ERF), p, seed, offset=5 + s.start))
        f.same(f"{label} gelu_bwd_dropout == dropout, gelu_bwd on items {lo}..{hi}", bwd[s],
               ops.gelu_bwd(x[s], ops.dropout(gr[s], p, seed, offset=5 + s.start)))
    # a view one element into the allocation is not 16-byte aligned: the element-by-element kernel, capped at 2^24 elements
    m = RC.CAP + 1000
    odd = x[1:m + 1]
    f.same(label + " misaligned view against the aligned call", ops.dropout(odd, p, seed, offset=6), drop[1:m + 1])
    f.done()
