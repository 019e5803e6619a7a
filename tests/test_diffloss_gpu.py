"""The DiffLoss image head on a real MI355X: the entries of csrc/diffusion.hip against float64 torch formulas, one evaluation of the net, teacher-forced
sampler steps and whole sampling loops against the reference's records (tests/golden/diffloss.partNN.npz, tests/golden/make_golden_diffloss.py),
row invariance, determinism and the inference-only contract.  `pytest -m gpu`.

Bounds.  float32: parity.close(1e-4), the project's float32 bar.  16-bit types: the drift yardstick — the result may be at most 1.5 x as far from the
float64 truth as the reference's own arithmetic in that type is (for an entry: the same formula evaluated by torch in that type on the CPU; for the
net and the sampler: the reference under torch.autocast, whose drifts the fixture stores), in max-rel and in rms-rel."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diffloss_cases as DC
import golden_io
import parity

pytestmark = pytest.mark.gpu
grad = pytest.mark.grad

if torch.cuda.is_available():
    from setok_amd import DiffLoss, ops

DEV = "cuda"
TOL = 1e-4
DRIFT = 1.5
DTS = [torch.float32, torch.bfloat16, torch.float16]
KIND = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
LN_EPS = 1e-6


def _log(label, *nums):
    path = os.environ.get("SETOK_PARITY_LOG")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as f:
            f.write(f"{test}\t{label}\t" + "\t".join(f"{n:.3e}" for n in nums) + "\n")
    print(label, *[f"{n:.3e}" for n in nums])


def _rand(*shape, seed=0, dt=torch.float32, scale=1.0):
    """Seeded values already rounded to dt, as float32: every evaluation of a formula starts from the same numbers."""
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dt).float()


def _within_drift(got, yard, truth, what):
    """got (device result) at most DRIFT x as far from truth as the yardstick is, in max-rel and rms-rel."""
    g, y = parity.measure(got, truth), parity.measure(yard, truth)
    _log(what, g[0], g[1], y[0], y[1])
    assert g[0] <= DRIFT * y[0], (what, "max_rel", g[0], y[0])
    assert g[1] <= DRIFT * y[1], (what, "rms_rel", g[1], y[1])


def _check(got, formula, args, dt, what):
    """args: float32 tensors holding dt-representable values.  float32: 1e-4 of the float64 formula; 16-bit: against torch in that type on the CPU."""
    truth = formula(*[a.double() for a in args])
    assert got.dtype == dt and torch.isfinite(got).all()
    if dt == torch.float32:
        parity.close(got, truth, TOL, what)
    else:
        _within_drift(got, formula(*[a.to(dt) for a in args]), truth, what)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return golden_io.load(os.path.join(golden_dir, "diffloss.npz"))


# ======================================================================================================================================
# 1. the entries
# ======================================================================================================================================
@pytest.mark.parametrize("dt", DTS)
def test_timestep_embedding(dt):
    t = torch.tensor([0.0, 1.0, 10.0, 999.0, 500.0])
    dim, half = 256, 128
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float32) / half)          # float32 arguments, as the reference builds them
    args = t[:, None] * freqs[None]
    truth = torch.cat([torch.cos(args.double()), torch.sin(args.double())], -1)
    got = ops.timestep_embedding(t.to(DEV), dim, dt)
    assert got.shape == (5, dim) and got.dtype == dt
    if dt == torch.float32:
        parity.close(got, truth, TOL, "timestep_embedding")
        assert torch.equal(got[0].cpu(), torch.cat([torch.ones(half), torch.zeros(half)]))         # t = 0
    else:
        _within_drift(got, torch.cat([torch.cos(args), torch.sin(args)], -1).to(dt), truth, f"timestep_embedding {dt}")
    assert ops.timestep_embedding(t[:0].to(DEV), dim, dt).shape == (0, dim)                        # rows == 0


@pytest.mark.parametrize("dt", DTS)
def test_silu_and_add_silu(dt):
    x = _rand(67, 192, seed=1, dt=dt, scale=3.0)
    x[0, :4] = torch.tensor([-100.0, 100.0, 0.0, -20.0])
    _check(ops.activation(x.to(DEV, dt), ops.ACT_SILU), F.silu, [x], dt, "silu")
    odd = x.reshape(-1)[:1237]                                                                      # an element count that is no multiple of anything
    _check(ops.activation(odd.to(DEV, dt), ops.ACT_SILU), F.silu, [odd], dt, "silu n=1237")
    b, row = _rand(67, 192, seed=2, dt=dt), _rand(1, 192, seed=3, dt=dt)
    f = lambda a, b: F.silu(a + b)
    _check(ops.add_silu(x.to(DEV, dt), b.to(DEV, dt)), f, [x, b], dt, "add_silu rows")
    _check(ops.add_silu(x.to(DEV, dt), row.to(DEV, dt)), f, [x, row], dt, "add_silu one row")
    wide = torch.zeros(67, 400, dtype=dt, device=DEV)
    wide[:, 8:200] = b.to(DEV, dt)
    assert torch.equal(ops.add_silu(x.to(DEV, dt), wide[:, 8:200]), ops.add_silu(x.to(DEV, dt), b.to(DEV, dt)))      # b as a strided window
    assert ops.add_silu(x[:0].to(DEV, dt), row.to(DEV, dt)).shape == (0, 192)


def _modulate(x, g, b, shift, scale):
    C = x.shape[-1]
    n = F.layer_norm(x, (C,), g, b, LN_EPS) if g is not None else F.layer_norm(x, (C,), None, None, LN_EPS)
    return n * (1 + scale) + shift


def _windows(rows, C, dt, seed, n=3, pad=8):
    """n (rows, C) column windows at non-zero offsets of ONE wider device buffer, and their values."""
    vals = [_rand(rows, C, seed=seed + i, dt=dt, scale=0.5) for i in range(n)]
    wide = torch.full((rows, pad + n * C + pad), float("nan"), dtype=dt, device=DEV)
    wins = []
    for i, v in enumerate(vals):
        wins.append(wide[:, pad + i * C: pad + (i + 1) * C])
        wins[-1].copy_(v.to(dt))
    return wins, vals


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("rows,C", [(r, c) for r in (1, 5, 67) for c in (64, 192, 4096)])
def test_adaln_modulate(rows, C, affine, dt):
    x = (_rand(rows, C, seed=10, scale=2.0) + 0.5).to(dt).float()
    (sh, sc), (shv, scv) = _windows(rows, C, dt, 20, n=2)
    g = (1 + _rand(C, seed=30, scale=0.2)).to(dt).float() if affine else None
    b = _rand(C, seed=31, dt=dt, scale=0.2) if affine else None
    xd = x.to(DEV, dt)
    got = ops.adaln_modulate(xd, sh, sc, None if g is None else g.to(DEV), None if b is None else b.to(DEV), LN_EPS)
    assert torch.equal(xd.cpu().float(), x)                                                          # without a residual x is read only
    if affine:
        _check(got, _modulate, [x, g, b, shv, scv], dt, f"modulate affine {rows}x{C}")
    else:
        _check(got, lambda x, s, c: _modulate(x, None, None, s, c), [x, shv, scv], dt, f"modulate plain {rows}x{C}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("rows,C", [(5, 64), (67, 192), (3, 4096)])
def test_gated_residual_then_modulate(rows, C, dt):
    x, h = _rand(rows, C, seed=40, dt=dt, scale=2.0), _rand(rows, C, seed=41, dt=dt)
    (sh, sc, gt), (shv, scv, gtv) = _windows(rows, C, dt, 50, n=3)
    g, b = (1 + _rand(C, seed=60, scale=0.2)).to(dt).float(), _rand(C, seed=61, dt=dt, scale=0.2)
    res = lambda x, h, gate: x + gate * h
    xd = x.to(DEV, dt)
    y = ops.adaln_modulate(xd, sh, sc, g.to(DEV), b.to(DEV), LN_EPS, h=h.to(DEV, dt), gate=gt)
    _check(xd, res, [x, h, gtv], dt, f"gated residual {rows}x{C}")                                   # x <- x + gate * h, in place
    _check(y, lambda x, h, gate, g, b, s, c: _modulate(res(x, h, gate), g, b, s, c), [x, h, gtv, g, b, shv, scv], dt, f"gated residual + modulate {rows}x{C}")
    # the fused launch against the two halves run apart: the modulate reads the STORED x
    y2 = ops.adaln_modulate(xd.clone(), sh, sc, g.to(DEV), b.to(DEV), LN_EPS)
    assert torch.equal(y, y2)
    xf = x.to(DEV, dt)
    ops.adaln_modulate(xf, sh, sc, None, None, LN_EPS, h=h.to(DEV, dt), gate=gt)                      # the final layer's form: residual, no affine
    assert torch.equal(xf, xd)
    assert ops.adaln_modulate(xd[:0], sh[:0], sc[:0], None, None, LN_EPS).shape == (0, C)


def _ddpm(out, x, noise, coef, nonzero, temp, cfg, half):
    """The step by the reference's statements: eps / v in out's dtype (the guidance combination included), everything after in x's."""
    a, b, c1, c2, lo, hi = coef
    C = x.shape[1]
    eps, v = out[:, :C], out[:, C:]
    if half:
        e = eps[half:] + cfg * (eps[:half] - eps[half:])
        eps = torch.cat([e, e], 0)
        noise = torch.cat([noise, noise], 0)
    eps, v = eps.to(x.dtype), v.to(x.dtype)
    x0 = a * x - b * eps
    mean = c1 * x0 + c2 * x
    f = (v + 1) / 2
    logvar = f * hi + (1 - f) * lo
    return mean + nonzero * torch.exp(0.5 * logvar) * noise * temp


@pytest.mark.parametrize("dt,out_f32", [(torch.float32, False), (torch.bfloat16, False), (torch.bfloat16, True), (torch.float16, False), (torch.float16, True)])
@pytest.mark.parametrize("cfg,temp,last", [(1.0, 1.0, False), (2.0, 0.9, False), (1.0, 0.9, True), (2.0, 1.0, True)])
def test_ddpm_step(cfg, temp, last, out_f32, dt):
    """The state x' is float32 arithmetic in every mode and is held to the float32 bar; what the element type touches is x_in (the rounded x', the
    conditional half duplicated under guidance), held to the drift yardstick: torch's x' by the same statements with `out` in the element type."""
    half = 5 if cfg != 1.0 else 0
    rows, C = (10 if half else 6), 192
    od = torch.float32 if out_f32 else dt
    dl = DiffLoss(num_sampling_steps="100", **DC.NET_A)
    i = 0 if last else 99                                                # t = 999: sqrt_recip_alphas_cumprod at its largest (2e4)
    coef = dl.step_coefficients(i)
    out = _rand(rows, 2 * C, seed=70, dt=od)
    x = _rand(rows, C, seed=71, scale=3.0)
    noise = _rand(half or rows, C, seed=72)
    if last:
        noise = noise * 1e30                                             # large and finite: at t = 0 the noise term is multiplied by 0 and must vanish
    nonzero = 0.0 if last else 1.0
    wide = torch.full((rows, 2 * C + 16), float("nan"), dtype=od, device=DEV)           # the net's output as rows of a wider buffer
    o_d = wide[:, :2 * C]
    o_d.copy_(out.to(od))
    x_d, x_in = x.to(DEV), torch.full((rows, C), float("nan"), dtype=dt, device=DEV)
    ops.ddpm_step(o_d, x_d, noise.to(DEV), x_in, coef, nonzero, temp, cfg, half)
    truth = _ddpm(out.double(), x.double(), noise.double(), coef, nonzero, temp, cfg, half)
    assert torch.isfinite(x_d).all() and torch.isfinite(x_in).all()
    parity.close(x_d, truth, TOL, f"ddpm x' cfg={cfg} last={last}")
    want_in = torch.cat([truth[:half], truth[:half]], 0) if half else truth
    if dt == torch.float32:
        assert torch.equal(x_in, torch.cat([x_d[:half], x_d[:half]], 0) if half else x_d)
    else:
        yard = _ddpm(out.to(od), x, noise, coef, nonzero, temp, cfg, half)
        yard = (torch.cat([yard[:half], yard[:half]], 0) if half else yard).to(dt)
        _within_drift(x_in, yard, want_in, f"ddpm x_in {dt} out_f32={out_f32} cfg={cfg} last={last}")
        assert torch.equal(x_in, (torch.cat([x_d[:half], x_d[:half]], 0) if half else x_d).to(dt))
    if last:                                                              # the mean alone
        parity.close(x_d, _ddpm(out.double(), x.double(), torch.zeros_like(noise).double(), coef, 0.0, temp, cfg, half), TOL, "ddpm t=0 is the mean")
    ops.ddpm_step(o_d[:0], x_d[:0], noise[:0].to(DEV), x_in[:0], coef, nonzero, temp, 1.0, 0)      # rows == 0


# ======================================================================================================================================
# 2. one evaluation of net B against the reference's records
# ======================================================================================================================================
def _net(cfg, sd, steps, dt):
    dl = DiffLoss(num_sampling_steps=steps, **cfg)
    dl.load_state_dict(sd, strict=True)
    return dl.to(DEV).to(dt).eval()


@pytest.fixture(scope="module")
def net_b():
    sd = DC.init_state_dict(DC.NET_B, DC.B_SEED)
    return {dt: _net(DC.NET_B, sd, "8", dt) for dt in DTS}


def _vs_reference(got, gold, prefix, truth, dt, what):
    """float32: the float32 bar against the float64 record; 16-bit: at most DRIFT x the reference's own autocast drift (max-rel, rms-rel)."""
    assert torch.isfinite(got).all()
    if dt == torch.float32:
        parity.close(got, truth, TOL, what)
        return
    g, ref = parity.measure(got, truth), gold[prefix + "drift." + KIND[dt]]
    _log(what, g[0], g[1], float(ref[0]), float(ref[1]))
    assert g[0] <= DRIFT * float(ref[0]), (what, "max_rel", g[0], float(ref[0]))
    assert g[1] <= DRIFT * float(ref[1]), (what, "rms_rel", g[1], float(ref[1]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(DC.FORWARD_CASES))
def test_one_evaluation_net_b(gold, net_b, name, dt):
    M, cfg, x, t, c = DC.forward_inputs(name)
    net = net_b[dt].net
    got = net.forward(x.to(DEV), t.to(DEV), c.to(DEV)) if cfg is None else net.forward_with_cfg(x.to(DEV), t.to(DEV), c.to(DEV), cfg)
    assert got.dtype == dt and got.shape == (M, 2 * DC.NET_B["target_channels"])
    _vs_reference(got, gold, f"fwd.{name}.", torch.from_numpy(gold[f"fwd.{name}.out.f64"]), dt, f"net B {name} {KIND[dt]}")


# ======================================================================================================================================
# 3. + 4. net A: teacher-forced steps and whole loops
# ======================================================================================================================================
@pytest.fixture(scope="module")
def sd_a(gold):
    return {str(n): torch.from_numpy(gold["A.sd." + str(n)]) for n in gold["A.names"]}


@pytest.mark.parametrize("name", list(DC.SAMPLE_CASES))
def test_teacher_forced_steps_fp32(gold, sd_a, name):
    """Every step of the loop on its own: the float64 trajectory's x_t (as float32) through ONE device step against the float64 x_{t-1}.  The reference's
    own float32 step, measured the same way by the fixture's generator, errs by at most 1.2e-5 of max |x| (`step_err.f32`; the worst step is t = 999, where
    sqrt_recip_alphas_cumprod is largest): the float32 bar leaves about 8 x headroom over the reference's own rounding."""
    steps, cfg, M, temp, z, noise = DC.sample_inputs(name)
    dl = _net(DC.NET_A, sd_a, steps, torch.float32)
    traj = torch.from_numpy(gold[f"sample.{name}.traj64"])
    worst = 0.0
    for k in range(int(steps)):
        got = dl.sample_step(traj[k].float().to(DEV), int(steps) - 1 - k, z.to(DEV), noise[1 + k].to(DEV), temperature=temp, cfg=cfg)
        worst = max(worst, parity.close(got, traj[k + 1], TOL, f"{name} step {k}"))
    _log(f"{name} worst teacher-forced max_rel | the reference's own float32 step", worst, float(gold[f"sample.{name}.step_err.f32"]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", list(DC.SAMPLE_CASES))
def test_whole_loop(gold, sd_a, name, dt):
    steps, cfg, M, temp, z, noise = DC.sample_inputs(name)
    dl = _net(DC.NET_A, sd_a, steps, dt)
    got = dl.sample(z.to(DEV), temperature=temp, cfg=cfg, noise=noise.to(DEV))
    assert got.shape == (M, DC.NET_A["target_channels"]) and got.dtype == torch.float32          # both halves under guidance, the state's own type
    _vs_reference(got, gold, f"sample.{name}.", torch.from_numpy(gold[f"sample.{name}.traj64"][-1]), dt, f"loop {name} {KIND[dt]}")


# ======================================================================================================================================
# 5. invariance and determinism
# ======================================================================================================================================
@pytest.mark.parametrize("dt", DTS)
def test_rows_do_not_depend_on_the_batch_and_calls_repeat(sd_a, dt):
    dl = _net(DC.NET_A, sd_a, "8", dt)
    g = torch.Generator().manual_seed(9)
    z, noise = torch.randn(37, 64, generator=g).to(DEV), torch.randn(9, 37, 64, generator=g).to(DEV)
    full = dl.sample(z, noise=noise)
    assert torch.isfinite(full).all()
    for r in (0, 17, 36):
        alone = dl.sample(z[r:r + 1], noise=noise[:, r:r + 1].contiguous())
        assert torch.equal(alone[0], full[r]), r
    assert torch.equal(dl.sample(z, noise=noise), full)
    a = dl.sample(z, temperature=0.9, generator=torch.Generator(device=DEV).manual_seed(5))
    b = dl.sample(z, temperature=0.9, generator=torch.Generator(device=DEV).manual_seed(5))
    c = dl.sample(z, temperature=0.9, generator=torch.Generator(device=DEV).manual_seed(6))
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.isfinite(a).all()


# ======================================================================================================================================
# 6. the contract
# ======================================================================================================================================
@grad
def test_inference_only_contract(gold, sd_a):
    dl = DiffLoss(num_sampling_steps="8", **DC.NET_A)
    assert dl.load_state_dict(sd_a, strict=True).missing_keys == []                                # a reference-format state dict loads strictly
    dl = dl.to(DEV)
    assert torch.is_grad_enabled() and all(p.requires_grad for p in dl.parameters())
    z = torch.randn(4, 64, device=DEV)
    out = dl.sample(z)
    assert out.requires_grad and out.grad_fn is not None
    with pytest.raises(NotImplementedError, match="no backward"):
        out.sum().backward()
    ev = dl.net.forward(torch.randn(4, 64, device=DEV), torch.tensor([0, 10, 500, 999], device=DEV), z)
    with pytest.raises(NotImplementedError):
        ev.sum().backward()
    with pytest.raises(NotImplementedError, match="follow-up"):
        dl(torch.randn(4, 64, device=DEV), z)
    with torch.no_grad():
        assert dl.sample(z).grad_fn is None
    assert dl.sample(z[:0]).shape == (0, 64)                                                        # no rows: no launch, an empty result
