"""The DiffLoss image head (src/model/loss/diffloss.py): `SimpleMLPAdaLN`, a small AdaLN residual MLP conditioned on the LLM's final-norm hidden
state, sampled by a cosine-schedule DDPM with learned-range variance respaced to `num_sampling_steps` (src/model/diffusion/).

`DiffLoss.sample(z)` turns hidden states (`SetokimLlamaPrefill.generate(...).hidden_states` rows) into `target_channels` latents: the other half
of what the reference model is for.  The parameter tree and its state-dict keys are the reference's, so its checkpoints load strictly.

What runs where: every Linear is `ops.linear` (setok_linear), everything else of a step is csrc/diffusion.hip; the schedule is host code (float64
tables, rounded to float32 once — the reference's `_extract_into_tensor` applies `.float()`); the sampler's state `x` is fp32 in every dtype mode
(the reference's 16-bit path, autocast, promotes it the same way) and only the net runs in the 16-bit type.  Inference only: `DiffLoss.forward`,
the training loss, raises and names the follow-up."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import autograd, ops
from ._packcache import PackCacheMixin

TRAIN_STEPS = 1000          # create_diffusion(diffusion_steps=1000)
MAX_BETA = 0.999            # betas_for_alpha_bar's clamp
LN_EPS = 1e-6

TABLES = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
          "posterior_log_variance_clipped", "log_betas")


# ---- the schedule (host) ------------------------------------------------------------------------------------------------------------------------
def parse_sampling_steps(num_sampling_steps) -> int:
    """The respacings this head implements: the decimal string (or int) of one section count in [1, 1000].  'ddimN' (DDIM striding) and comma-separated
    section lists are the reference's other spellings; they are refused by name."""
    s = str(num_sampling_steps).strip()
    if s.startswith("ddim"):
        raise NotImplementedError(f"DiffLoss: num_sampling_steps={num_sampling_steps!r}: DDIM striding ('ddimN') is not implemented (the sampler is the DDPM p_sample loop)")
    if "," in s:
        raise NotImplementedError(f"DiffLoss: num_sampling_steps={num_sampling_steps!r}: comma-separated section counts are not implemented (one count in [1, {TRAIN_STEPS}])")
    if not (s.isascii() and s.isdigit()) or not 1 <= int(s) <= TRAIN_STEPS:
        raise ValueError(f"DiffLoss: num_sampling_steps={num_sampling_steps!r} must be the decimal string of an integer in [1, {TRAIN_STEPS}]")
    return int(s)


def cosine_schedule(steps: Optional[int] = None) -> Dict[str, np.ndarray]:
    """`create_diffusion(timestep_respacing=str(steps), noise_schedule="cosine")` as tables.  steps None: the unspaced 1000-step process (the
    reference's `train_diffusion`, respacing '').

    The cosine schedule of Nichol & Dhariwal: alpha_bar(u) = cos^2((u + 0.008) / 1.008 * pi / 2), beta_i = min(1 - alpha_bar((i + 1) / T) / alpha_bar(i / T), 0.999).
    Respacing keeps `steps` timesteps at a fractional stride (T - 1) / (steps - 1), each rounded to the nearest integer, and re-derives the betas of
    the shorter chain from the alphas_cumprod it keeps: beta'_k = 1 - abar[t_k] / abar[t_{k-1}].  `timestep_map[k] = t_k` is what the net sees.
    All float64; the six per-step tables the sampler reads are returned as float32 as well (key + '_f32')."""
    T = TRAIN_STEPS
    abar_fn = lambda u: math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2
    betas = np.array([min(1 - abar_fn((i + 1) / T) / abar_fn(i / T), MAX_BETA) for i in range(T)], dtype=np.float64)
    n = T if steps is None else int(steps)
    if not 1 <= n <= T:
        raise ValueError(f"cosine_schedule: steps={steps} outside [1, {T}]")
    stride = 1.0 if n <= 1 else (T - 1) / (n - 1)
    kept, pos = set(), 0.0
    for _ in range(n):
        kept.add(round(pos))
        pos += stride
    tmap = sorted(kept)
    assert len(tmap) == n
    abar_full = np.cumprod(1.0 - betas, axis=0)
    new_betas, last = [], 1.0
    for t in tmap:
        new_betas.append(1 - abar_full[t] / last)
        last = abar_full[t]
    b = np.array(new_betas, dtype=np.float64)
    alphas = 1.0 - b
    abar = np.cumprod(alphas, axis=0)
    abar_prev = np.append(1.0, abar[:-1])
    post_var = b * (1.0 - abar_prev) / (1.0 - abar)
    # the posterior variance is 0 at the chain's first step: its log is taken from the second.  A 1-step chain has no second step (the reference's table is
    # empty there and its sampler cannot run); its only step is t = 0, whose noise term is multiplied by 0, so any finite value serves: log beta.
    post_logvar = np.log(np.append(post_var[1], post_var[1:])) if n > 1 else np.log(b)
    out = dict(timestep_map=np.array(tmap, dtype=np.int64), betas=b, alphas_cumprod=abar,
               sqrt_recip_alphas_cumprod=np.sqrt(1.0 / abar), sqrt_recipm1_alphas_cumprod=np.sqrt(1.0 / abar - 1),
               posterior_mean_coef1=b * np.sqrt(abar_prev) / (1.0 - abar), posterior_mean_coef2=(1.0 - abar_prev) * np.sqrt(alphas) / (1.0 - abar),
               posterior_log_variance_clipped=post_logvar, log_betas=np.log(b))
    for k in TABLES:
        out[k + "_f32"] = out[k].astype(np.float32)
    return out


# ---- the parameter tree (the reference's names) -----------------------------------------------------------------------------------------------------
def _check_channels(what: str, n: int, gran: int, mode: str) -> None:
    if n <= 0 or n % gran != 0:
        raise ValueError(f"DiffLoss: {what}={n} is not a positive multiple of {gran}: every Linear runs on setok_linear, whose K granularity is "
                         f"{gran} in {mode} (64 in the 16-bit types, 16 in float32)")


class TimestepEmbedder(nn.Module):
    def __init__(self, hidden_size, frequency_embedding_size=256):
        super().__init__()
        if frequency_embedding_size % 2:
            raise NotImplementedError(f"TimestepEmbedder: frequency_embedding_size={frequency_embedding_size} is odd: the zero-padded odd embedding "
                                      f"(diffloss.py:89-90) is not implemented")
        _check_channels("frequency_embedding_size", frequency_embedding_size, 16, "float32")
        self.mlp = nn.Sequential(nn.Linear(frequency_embedding_size, hidden_size, bias=True), nn.SiLU(), nn.Linear(hidden_size, hidden_size, bias=True))
        self.frequency_embedding_size = frequency_embedding_size


class ResBlock(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.channels = channels
        self.in_ln = nn.LayerNorm(channels, eps=LN_EPS)
        self.mlp = nn.Sequential(nn.Linear(channels, channels, bias=True), nn.SiLU(), nn.Linear(channels, channels, bias=True))
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(channels, 3 * channels, bias=True))


class FinalLayer(nn.Module):
    def __init__(self, model_channels, out_channels):
        super().__init__()
        self.norm_final = nn.LayerNorm(model_channels, elementwise_affine=False, eps=LN_EPS)
        self.linear = nn.Linear(model_channels, out_channels, bias=True)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(model_channels, 2 * model_channels, bias=True))


class SimpleMLPAdaLN(PackCacheMixin, nn.Module):
    """diffloss.py:151-248 on the HIP library.  `forward` and `forward_with_cfg` are one evaluation of the net (inference only)."""

    def __init__(self, in_channels, model_channels, out_channels, z_channels, num_res_blocks, grad_checkpointing=False, frequency_embedding_size=256):
        super().__init__()
        for what, n in (("in_channels (target_channels)", in_channels), ("z_channels", z_channels), ("model_channels (width)", model_channels)):
            _check_channels(what, n, 16, "float32")
        if out_channels % 8:
            raise ValueError(f"SimpleMLPAdaLN: out_channels={out_channels} must be a multiple of 8 (16-byte rows)")
        if num_res_blocks < 0:
            raise ValueError(f"SimpleMLPAdaLN: num_res_blocks={num_res_blocks}")
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        self.z_channels, self.num_res_blocks = z_channels, num_res_blocks
        self.grad_checkpointing = grad_checkpointing             # (a training-time switch: nothing to checkpoint on the inference path)
        self.time_embed = TimestepEmbedder(model_channels, frequency_embedding_size)
        self.cond_embed = nn.Linear(z_channels, model_channels)
        self.input_proj = nn.Linear(in_channels, model_channels)
        self.res_blocks = nn.ModuleList([ResBlock(model_channels) for _ in range(num_res_blocks)])
        self.final_layer = FinalLayer(model_channels, out_channels)
        self.initialize_weights()
        self._init_pack_cache()

    def initialize_weights(self):
        """The reference's initialisation: Xavier-uniform Linears with zero biases, N(0, 0.02) timestep MLP, zero adaLN and output layers."""
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                nn.init.zeros_(m.bias)
        nn.init.normal_(self.time_embed.mlp[0].weight, std=0.02)
        nn.init.normal_(self.time_embed.mlp[2].weight, std=0.02)
        for lin in [b.adaLN_modulation[-1] for b in self.res_blocks] + [self.final_layer.adaLN_modulation[-1], self.final_layer.linear]:
            nn.init.zeros_(lin.weight)
            nn.init.zeros_(lin.bias)

    # -- compute-ready operands ---------------------------------------------------------------------------------------------------------------------
    def _pack(self):
        w0 = self.input_proj.weight
        key = (w0.dtype, str(w0.device), self._versions(self.parameters()))
        if self._packed.get("key") == key:
            return self._packed
        if w0.dtype in ops.LOW:
            for what, n in (("in_channels (target_channels)", self.in_channels), ("z_channels", self.z_channels), ("model_channels (width)", self.model_channels),
                            ("frequency_embedding_size", self.time_embed.frequency_embedding_size)):
                _check_channels(what, n, 64, str(w0.dtype))
        wt = lambda lin: lin.weight.detach().contiguous()
        bs = lambda lin: lin.bias.detach().float().contiguous()
        f32 = lambda t: t.detach().float().contiguous()
        ada = [b.adaLN_modulation[1] for b in self.res_blocks] + [self.final_layer.adaLN_modulation[1]]
        te = self.time_embed.mlp
        self._packed = dict(
            key=key, te0=(wt(te[0]), bs(te[0])), te2=(wt(te[2]), bs(te[2])), cond=(wt(self.cond_embed), bs(self.cond_embed)),
            inp=(wt(self.input_proj), bs(self.input_proj)),
            # every block's [shift | scale | gate] rows, then the final layer's [shift | scale]: ONE GEMM per evaluation, (3 depth + 2) W output columns
            ada=(torch.cat([l.weight.detach() for l in ada], 0).contiguous(), torch.cat([l.bias.detach().float() for l in ada], 0).contiguous()),
            blocks=[dict(g=f32(b.in_ln.weight), b=f32(b.in_ln.bias), m0=(wt(b.mlp[0]), bs(b.mlp[0])), m2=(wt(b.mlp[2]), bs(b.mlp[2]))) for b in self.res_blocks],
            fin=(wt(self.final_layer.linear), bs(self.final_layer.linear)))
        return self._packed

    @property
    def dtype(self) -> torch.dtype:
        return self.input_proj.weight.dtype

    def _time_embed(self, pk, t: torch.Tensor) -> torch.Tensor:
        """TimestepEmbedder.forward for a 1-D batch of timesteps -> (len(t), W)."""
        tf = t.to(device=self.input_proj.weight.device, dtype=torch.float32).reshape(-1).contiguous()
        e = ops.timestep_embedding(tf, self.time_embed.frequency_embedding_size, self.dtype)
        u = ops.linear(e, *pk["te0"])
        ops.activation(u, ops.ACT_SILU, out=u)
        return ops.linear(u, *pk["te2"])

    def _eval(self, pk, x_in: torch.Tensor, t_emb: torch.Tensor, c_emb: torch.Tensor, out_dtype: torch.dtype) -> torch.Tensor:
        """One evaluation from the embedded operands: x_in (M, C), t_emb (M, W) or ONE row (1, W), c_emb (M, W) -> (M, out_channels) in out_dtype.
        5 + 4 depth launches: SiLU(t + c) | the fused adaLN GEMM | input_proj | per block: [gated residual +] modulate, mlp.0, SiLU, mlp.2 |
        gated residual + final modulate | final Linear."""
        W, d = self.model_channels, self.num_res_blocks
        mod = ops.linear(ops.add_silu(c_emb, t_emb), *pk["ada"])
        x = ops.linear(x_in, *pk["inp"])
        y = torch.empty_like(x)
        h = gate = None
        for i, B in enumerate(pk["blocks"]):
            o = 3 * i * W
            ops.adaln_modulate(x, mod[:, o:o + W], mod[:, o + W:o + 2 * W], B["g"], B["b"], LN_EPS, h=h, gate=gate, out=y)
            u = ops.linear(y, *B["m0"])
            ops.activation(u, ops.ACT_SILU, out=u)
            h, gate = ops.linear(u, *B["m2"]), mod[:, o + 2 * W:o + 3 * W]
        o = 3 * d * W
        ops.adaln_modulate(x, mod[:, o:o + W], mod[:, o + W:o + 2 * W], None, None, LN_EPS, h=h, gate=gate, out=y)
        return ops.linear(y, *pk["fin"], out_dtype=out_dtype)

    def _check_inputs(self, x, t, c):
        if x.dim() != 2 or x.shape[1] != self.in_channels or c.dim() != 2 or c.shape != (x.shape[0], self.z_channels) or t.numel() != x.shape[0]:
            raise ValueError(f"SimpleMLPAdaLN: x {tuple(x.shape)}, t {tuple(t.shape)}, c {tuple(c.shape)} do not fit (N, {self.in_channels}), (N,), (N, {self.z_channels})")

    def _forward(self, x, t, c):
        self._check_inputs(x, t, c)
        pk, dt = self._pack(), self.dtype
        dev = self.input_proj.weight.device
        return self._eval(pk, x.to(device=dev, dtype=dt).contiguous(), self._time_embed(pk, t), ops.linear(c.to(device=dev, dtype=dt).contiguous(), *pk["cond"]), dt)

    def forward(self, x, t, c):
        """x (N, in_channels), t (N,) timesteps, c (N, z_channels) -> (N, out_channels) in the module's dtype."""
        with torch.no_grad():
            out = self._forward(x.detach(), t, c.detach())
        return autograd.no_backward("SimpleMLPAdaLN.forward", out, [x, c, *self.parameters()])

    def forward_with_cfg(self, x, t, c, cfg_scale):
        """diffloss.py:240-248: the net on the first half of x duplicated, eps <- uncond + cfg_scale * (cond - uncond) in both halves.  One evaluation for
        inspection: the combination here is three elementwise torch ops in fp32; the sampler does it inside setok_ddpm_step."""
        n = x.shape[0]
        if n % 2:
            raise ValueError(f"SimpleMLPAdaLN.forward_with_cfg: {n} rows: classifier-free guidance needs an even number (conditional | unconditional halves)")
        with torch.no_grad():
            half = x.detach()[: n // 2]
            out = self._forward(torch.cat([half, half], 0), t, c.detach())
            eps, rest = out[:, :self.in_channels].float(), out[:, self.in_channels:]
            ce, ue = eps[: n // 2], eps[n // 2:]
            he = (ue + cfg_scale * (ce - ue)).to(out.dtype)
            out = torch.cat([torch.cat([he, he], 0), rest], 1)
        return autograd.no_backward("SimpleMLPAdaLN.forward_with_cfg", out, [x, c, *self.parameters()])


class DiffLoss(nn.Module):
    """diffloss.py:9-52.  `sample` is implemented; `forward` (the training loss) is not."""

    def __init__(self, target_channels, z_channels, depth, width, num_sampling_steps, grad_checkpointing=False):
        super().__init__()
        self.num_sampling_steps = parse_sampling_steps(num_sampling_steps)
        self.in_channels = target_channels
        self.net = SimpleMLPAdaLN(in_channels=target_channels, model_channels=width, out_channels=target_channels * 2, z_channels=z_channels,
                                  num_res_blocks=depth, grad_checkpointing=grad_checkpointing)
        self.schedule = cosine_schedule(self.num_sampling_steps)                          # the reference's gen_diffusion, as tables

    def forward(self, target, z, mask=None):
        raise NotImplementedError("DiffLoss.forward (the training loss: q_sample, the epsilon MSE and the variational bound on the learned variance, with a backward "
                                  "through the net) is not implemented on the HIP path: it is the named follow-up of the image head.  sample() is implemented.")

    def step_coefficients(self, i: int):
        """The six float32 coefficients of respaced step i, in setok_ddpm_step's order."""
        return tuple(float(self.schedule[k + "_f32"][i]) for k in TABLES)

    def _check_rows(self, what, z, cfg):
        net = self.net
        if z.dim() != 2 or z.shape[1] != net.z_channels:
            raise ValueError(f"DiffLoss.{what}: z {tuple(z.shape)} is not (M, {net.z_channels})")
        M = z.shape[0]
        guided = float(cfg) != 1.0
        if guided and M % 2:
            raise ValueError(f"DiffLoss.{what}: M={M} is odd with cfg={cfg}: classifier-free guidance takes conditional rows [0, M/2) and unconditional rows [M/2, M)")
        return M, (M // 2 if guided else 0)

    def _step(self, pk, i, x, x_in, t_emb_row, c_emb, noise, temperature, cfg, half):
        """Respaced step i in place on the state x (and the net's next operand x_in): one evaluation (5 + 4 depth launches) + setok_ddpm_step."""
        out = self.net._eval(pk, x_in, t_emb_row, c_emb, torch.float32)        # the final Linear accumulates in fp32 anyway: its output goes to the step unrounded
        ops.ddpm_step(out, x, noise, x_in, self.step_coefficients(i), 0.0 if i == 0 else 1.0, float(temperature), float(cfg), half)

    def sample_step(self, x, i, z, noise, temperature=1.0, cfg=1.0):
        """One reverse step on its own: the state x_i (M, C) -> x_{i-1} (float32) at respaced index i (steps - 1 first, 0 last) with the draw `noise`
        (M, C), or (M / 2, C) under guidance.  What sample() does per step, for a state given from outside (one step can be checked by itself)."""
        net, C = self.net, self.in_channels
        M, half = self._check_rows("sample_step", z, cfg)
        if not 0 <= int(i) < self.num_sampling_steps or tuple(x.shape) != (M, C) or tuple(noise.shape) != ((half or M), C):
            raise ValueError(f"DiffLoss.sample_step: i={i}, x {tuple(x.shape)}, noise {tuple(noise.shape)} do not fit {self.num_sampling_steps} steps, (M, C) = {(M, C)}")
        dev = net.input_proj.weight.device
        with torch.no_grad():
            pk, dt = net._pack(), net.dtype
            if M == 0:
                return torch.empty((0, C), dtype=torch.float32, device=dev)
            xs = x.detach().to(device=dev, dtype=torch.float32, copy=True).contiguous()
            x_in = (torch.cat([xs[:half], xs[:half]], 0) if half else xs).to(dt, copy=True)
            c_emb = ops.linear(z.detach().to(device=dev, dtype=dt).contiguous(), *pk["cond"])
            t_emb = net._time_embed(pk, torch.tensor([float(self.schedule["timestep_map"][int(i)])]))
            self._step(pk, int(i), xs, x_in, t_emb, c_emb, noise.to(device=dev, dtype=torch.float32).contiguous(), temperature, cfg, half)
        return autograd.no_backward("DiffLoss.sample_step", xs, [x, z, *self.parameters()])

    def sample(self, z, temperature=1.0, cfg=1.0, *, noise: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None):
        """z (M, z_channels) -> (M, target_channels) float32 latents.  cfg != 1: M even, rows [0, M/2) conditional, [M/2, M) unconditional; all M rows are
        returned as the reference does (its callers keep the first half).  noise: (1 + steps, R, C) with R = M (M / 2 under cfg: one draw shared by both
        halves) — the start sample, then one draw per step; None: drawn on the device with torch.randn(generator=generator) in that order.
        Nothing inside the loop touches the host: 5 launches for the embeddings, then steps * (6 + 4 depth) on the current stream."""
        net, C, steps = self.net, self.in_channels, self.num_sampling_steps
        M, half = self._check_rows("sample", z, cfg)
        guided = float(cfg) != 1.0
        R = half if guided else M
        if noise is not None and tuple(noise.shape) != (1 + steps, R, C):
            raise ValueError(f"DiffLoss.sample: noise {tuple(noise.shape)} is not (1 + steps, rows, C) = {(1 + steps, R, C)}")
        dev = net.input_proj.weight.device
        with torch.no_grad():
            pk, dt = net._pack(), net.dtype
            if M == 0:
                return torch.empty((0, C), dtype=torch.float32, device=dev)
            if noise is not None:
                noise = noise.to(device=dev, dtype=torch.float32).contiguous()
            draw = (lambda k: noise[k]) if noise is not None else (lambda k: torch.randn((R, C), generator=generator, device=dev, dtype=torch.float32))
            x = torch.empty((M, C), dtype=torch.float32, device=dev)
            start = draw(0)
            x[:R] = start
            if guided:
                x[R:] = start
            x_in = x.to(dt, copy=True)                                                   # (under guidance both halves start equal: this IS the conditional half duplicated)
            c_emb = ops.linear(z.detach().to(device=dev, dtype=dt).contiguous(), *pk["cond"])
            tmap = self.schedule["timestep_map"]
            t_emb = net._time_embed(pk, torch.from_numpy(np.ascontiguousarray(tmap[::-1], dtype=np.float32)))   # row k: the timestep the net sees at loop step k (999, 989, ... for '100')
            for k in range(steps):
                self._step(pk, steps - 1 - k, x, x_in, t_emb[k:k + 1], c_emb, draw(1 + k), temperature, cfg, half)
        return autograd.no_backward("DiffLoss.sample", x, [z, *self.parameters()])
