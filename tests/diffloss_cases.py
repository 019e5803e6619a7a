"""Shapes, seeds and seeded inputs shared by tests/golden/make_golden_diffloss.py and the tests that read its fixture (diffloss.partNN.npz):
everything here regenerates bit-exactly from its seed (torch CPU generator), so the fixture stores results — and net A's trained weights — only."""
import torch

# ---- net A: toy-trained, sampled through whole loops ---------------------------------------------------------------------------------------
# Trained because an untrained net with clip_denoised=False is not a usable yardstick: the reference's own fp32 samples reach |x| ~ 1e5 and its
# fp16-autocast run returns NaN; after a short fit to the toy target below all of its runs stay finite (the generator asserts it).
NET_A = dict(target_channels=64, z_channels=64, depth=2, width=128)
A_TRAIN = dict(steps=1500, batch=256, lr=1e-3, seed=1234)
SAMPLE_CASES = {
    # name: (num_sampling_steps, cfg, M, temperature, seed)
    "s8": ("8", 1.0, 6, 1.0, 101),
    "s100": ("100", 1.0, 6, 1.0, 102),
    "s8_cfg": ("8", 2.0, 2 * 5, 0.9, 103),
}

# ---- net B: seeded random weights, single evaluations only (nothing is amplified there) ---------------------------------------------------------
NET_B = dict(target_channels=64, z_channels=128, depth=3, width=192)
B_SEED = 77
FORWARD_CASES = {f"M{M}_t{t}": (M, t, None, 200 + 10 * i + j) for i, M in enumerate((1, 5, 67)) for j, t in enumerate((0, 10, 999))}
FORWARD_CASES["cfg_M6_t10"] = (6, 10, 2.0, 290)              # forward_with_cfg

SCHEDULES = ("", "8", "100")
TABLES = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
          "posterior_log_variance_clipped", "log_betas")
KINDS = ("f32", "bf16", "f16")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}


def toy_projection():
    return torch.randn(NET_A["z_channels"], NET_A["target_channels"], generator=torch.Generator().manual_seed(A_TRAIN["seed"])) / 8.0


def toy_batch(P, n, g):
    """(target, z) of the toy distribution net A is fitted to: target = tanh(z P) + 0.1 noise."""
    z = torch.randn(n, NET_A["z_channels"], generator=g)
    return torch.tanh(z @ P) + 0.1 * torch.randn(n, NET_A["target_channels"], generator=g), z


def sample_inputs(name):
    """(steps, cfg, M, temperature, z (M, Z), noise (1 + steps, R, C)) with R = M, or M / 2 under guidance (one draw shared by both halves)."""
    steps, cfg, M, temp, seed = SAMPLE_CASES[name]
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, NET_A["z_channels"], generator=g)
    R = M // 2 if cfg != 1.0 else M
    noise = torch.randn(1 + int(steps), R, NET_A["target_channels"], generator=g)
    return steps, cfg, M, temp, z, noise


def forward_inputs(name):
    """(M, cfg_scale or None, x (M, C), t (M,) int64, c (M, Z))."""
    M, t, cfg, seed = FORWARD_CASES[name]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, NET_B["target_channels"], generator=g)
    c = torch.randn(M, NET_B["z_channels"], generator=g)
    return M, cfg, x, torch.full((M,), t, dtype=torch.int64), c


def init_state_dict(cfg, seed):
    """A seeded DiffLoss state dict under the reference's keys with NO zero layer: the reference initialises every adaLN_modulation and the final Linear
    to zero, which would make the net's output identically zero and every modulation the identity."""
    g = torch.Generator().manual_seed(seed)
    C, Z, W, d = cfg["target_channels"], cfg["z_channels"], cfg["width"], cfg["depth"]
    sd = {}

    def lin(key, n_out, n_in, gain=1.0):
        sd[key + ".weight"] = torch.randn(n_out, n_in, generator=g) * (gain / n_in ** 0.5)
        sd[key + ".bias"] = torch.randn(n_out, generator=g) * 0.1

    lin("net.time_embed.mlp.0", W, 256)
    lin("net.time_embed.mlp.2", W, W)
    lin("net.cond_embed", W, Z)
    lin("net.input_proj", W, C)
    for i in range(d):
        p = f"net.res_blocks.{i}."
        sd[p + "in_ln.weight"] = 1.0 + 0.1 * torch.randn(W, generator=g)
        sd[p + "in_ln.bias"] = 0.1 * torch.randn(W, generator=g)
        lin(p + "mlp.0", W, W)
        lin(p + "mlp.2", W, W)
        lin(p + "adaLN_modulation.1", 3 * W, W, 0.5)
    lin("net.final_layer.linear", 2 * C, W)
    lin("net.final_layer.adaLN_modulation.1", 2 * W, W, 0.5)
    return sd
