"""Writes tests/golden/diffloss.partNN.npz: what the reference's DiffLoss image head (src/model/loss/diffloss.py + src/model/diffusion/) computes.

Run where the reference checkout is available:  python tests/golden/make_golden_diffloss.py

Nothing of the reference's text is kept here: its `diffusion` package and `loss/diffloss.py` are imported from the checkout by path at run time, under
stub packages `src`, `src.model`, `src.model.loss` (the real `__init__` files pull in packages that need not be installed).

  sched.<''|8|100>.*   timestep_map and the six per-step tables of create_diffusion(respacing, "cosine"), float32 as `_extract_into_tensor` rounds them
  A.sd.*               net A (diffloss_cases.NET_A) after A_TRAIN AdamW steps of the reference's own DiffLoss.forward on the toy target; A.names / A.shapes
  sample.<case>.*      whole sampling loops on net A: the float64 trajectory (1 + steps, M, C), the reference's float32 / bf16-autocast / fp16-autocast
                       final samples, each run's max |x| and each run's drift from the float64 final sample (max-rel, rms-rel)
  fwd.<case>.*         single evaluations of net B (seeded weights, rebuilt at test time): float64, float32 and the two autocast types, and the drifts

Two things in the reference are worked around: `p_sample_loop` calls `.cuda()`, so the loop over t = steps - 1 ... 0 is driven here through
`gen_diffusion.p_sample` with `torch.randn_like` patched to return the recorded noise; and the float64 truth run is `net.double()` with a forward
pre-hook on `time_embed.mlp[0]` casting its input to the weight dtype (the frequency embedding is built in float32).  The 16-bit yardstick is the
reference under `torch.autocast('cpu', dtype)`: the only way its 16-bit sampler runs at all (the step arithmetic promotes x to float32)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))

import diffloss_cases as DC  # noqa: E402
import golden_io  # noqa: E402
import rac_harness as R  # noqa: E402


def load_reference_diffloss():
    model = os.path.join(R.REF_ROOT, "src", "model")
    for name in ("src", "src.model", "src.model.loss"):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m

    def load(name, path, **kw):
        spec = importlib.util.spec_from_file_location(name, path, **kw)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    load("src.model.diffusion", os.path.join(model, "diffusion", "__init__.py"), submodule_search_locations=[os.path.join(model, "diffusion")])
    return load("src.model.loss.diffloss", os.path.join(model, "loss", "diffloss.py"))


def measure(got, ref):
    g, r = got.double(), ref.double()
    err = (g - r).abs()
    return np.array([float(err.max() / r.abs().max()), float(err.pow(2).mean().sqrt() / r.pow(2).mean().sqrt())])


class recorded_noise:
    """torch.randn_like -> the next recorded draw, in the dtype asked for (both halves under guidance: torch.cat([noise, noise]))."""

    def __init__(self, draws, dup):
        self.draws, self.dup, self.k = draws, dup, 0

    def __enter__(self):
        self.orig = torch.randn_like
        torch.randn_like = self
        return self

    def __exit__(self, *a):
        torch.randn_like = self.orig

    def __call__(self, like, **kw):
        n = self.draws[self.k]
        self.k += 1
        n = torch.cat([n, n], 0) if self.dup else n
        assert n.shape == like.shape
        return n.to(like.dtype)


def as_double(dl):
    dl = dl.double()
    w = dl.net.time_embed.mlp[0].weight
    dl.net.time_embed.mlp[0].register_forward_pre_hook(lambda m, a: (a[0].to(w.dtype),))
    return dl


def run_loop(dl, z, noise, cfg, temp, xdtype, autocast=None):
    """The reference's DiffLoss.sample with the recorded noise; returns the trajectory (1 + steps, M, C)."""
    gd = dl.gen_diffusion
    guided = cfg != 1.0
    start = torch.cat([noise[0], noise[0]], 0) if guided else noise[0]
    x = start.to(xdtype)
    kw = dict(c=z.to(xdtype), cfg_scale=cfg) if guided else dict(c=z.to(xdtype))
    fn = dl.net.forward_with_cfg if guided else dl.net.forward
    traj = [x]
    ctx = torch.autocast("cpu", dtype=autocast) if autocast is not None else torch.autocast("cpu", enabled=False)
    with torch.no_grad(), ctx, recorded_noise(noise[1:], guided):
        for i in reversed(range(gd.num_timesteps)):
            t = torch.full((x.shape[0],), i, dtype=torch.long)
            x = gd.p_sample(fn, x, t, clip_denoised=False, model_kwargs=kw, temperature=temp)["sample"]
            traj.append(x)
    return torch.stack([v.double() for v in traj])


def teacher_forced_step_error(dl, z, noise, cfg, temp, t64):
    """The reference's own float32 STEP fed the float64 trajectory's x_t: max over the steps of max|x' - x64_{t-1}| / max|x64_{t-1}|."""
    gd = dl.gen_diffusion
    guided = cfg != 1.0
    kw = dict(c=z, cfg_scale=cfg) if guided else dict(c=z)
    fn = dl.net.forward_with_cfg if guided else dl.net.forward
    worst = 0.0
    with torch.no_grad():
        for k, i in enumerate(reversed(range(gd.num_timesteps))):
            with recorded_noise(noise[1 + k:2 + k], guided):
                x = gd.p_sample(fn, t64[k].float(), torch.full((t64.shape[1],), i, dtype=torch.long), clip_denoised=False, model_kwargs=kw, temperature=temp)["sample"]
            worst = max(worst, float(measure(x, t64[k + 1])[0]))
    return np.array(worst)


def train_net_a(D):
    torch.manual_seed(DC.A_TRAIN["seed"])
    dl = D.DiffLoss(num_sampling_steps="100", **DC.NET_A)
    opt = torch.optim.AdamW(dl.parameters(), lr=DC.A_TRAIN["lr"])
    P, g = DC.toy_projection(), torch.Generator().manual_seed(DC.A_TRAIN["seed"] + 1)
    for it in range(DC.A_TRAIN["steps"]):
        target, z = DC.toy_batch(P, DC.A_TRAIN["batch"], g)
        loss = dl(target, z)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if it % 250 == 0 or it == DC.A_TRAIN["steps"] - 1:
            print(f"  net A step {it}: loss {float(loss.detach()):.4f}", flush=True)
    return {k: v.detach().clone() for k, v in dl.state_dict().items()}


def main():
    D = load_reference_diffloss()
    out = {}

    for resp in DC.SCHEDULES:
        gd = D.create_diffusion(timestep_respacing=resp, noise_schedule="cosine")
        out[f"sched.{resp}.timestep_map"] = np.array(gd.timestep_map, dtype=np.int64)
        for k in DC.TABLES:
            arr = np.log(gd.betas) if k == "log_betas" else getattr(gd, k)
            out[f"sched.{resp}.{k}"] = torch.from_numpy(arr).float().numpy()

    sd_a = train_net_a(D)
    out["A.names"] = np.array(list(sd_a))
    out["A.shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd_a.values()])
    for k, v in sd_a.items():
        out["A.sd." + k] = v.numpy()

    def build(cfg, sd, steps):
        dl = D.DiffLoss(num_sampling_steps=steps, **cfg)
        dl.load_state_dict(sd, strict=True)
        return dl.eval()

    for name in DC.SAMPLE_CASES:
        steps, cfg, M, temp, z, noise = DC.sample_inputs(name)
        t64 = run_loop(as_double(build(DC.NET_A, sd_a, steps)), z, noise, cfg, temp, torch.float64)
        dl = build(DC.NET_A, sd_a, steps)
        runs = {"f32": run_loop(dl, z, noise, cfg, temp, torch.float32), "bf16": run_loop(dl, z, noise, cfg, temp, torch.float32, torch.bfloat16),
                "f16": run_loop(dl, z, noise, cfg, temp, torch.float32, torch.float16)}
        assert torch.isfinite(t64).all(), name
        p = f"sample.{name}."
        out[p + "z"], out[p + "noise"], out[p + "traj64"] = z.numpy(), noise.numpy(), t64.numpy()
        out[p + "maxabs.f64"] = np.array(float(t64.abs().max()))
        out[p + "step_err.f32"] = teacher_forced_step_error(dl, z, noise, cfg, temp, t64)
        for kind, tr in runs.items():
            assert torch.isfinite(tr).all(), (name, kind)
            out[p + "final." + kind] = tr[-1].float().numpy()
            out[p + "maxabs." + kind] = np.array(float(tr.abs().max()))
            out[p + "drift." + kind] = measure(tr[-1], t64[-1])
        print(name, "teacher-forced f32 step err", float(out[p + "step_err.f32"]), "max|x|", {k: float(out[p + "maxabs." + k]) for k in ("f64",) + DC.KINDS}, "drift (max-rel, rms-rel)",
              {k: out[p + "drift." + k].round(7).tolist() for k in DC.KINDS}, flush=True)

    sd_b = DC.init_state_dict(DC.NET_B, DC.B_SEED)
    for name in DC.FORWARD_CASES:
        M, cfg, x, t, c = DC.forward_inputs(name)

        def ev(dl, dt, autocast=None):
            fn = (lambda *a: dl.net.forward_with_cfg(*a, cfg)) if cfg is not None else dl.net.forward
            ctx = torch.autocast("cpu", dtype=autocast) if autocast is not None else torch.autocast("cpu", enabled=False)
            with torch.no_grad(), ctx:
                return fn(x.to(dt), t, c.to(dt))

        r64 = ev(as_double(build(DC.NET_B, sd_b, "8")), torch.float64)
        dl = build(DC.NET_B, sd_b, "8")
        p = f"fwd.{name}."
        out[p + "out.f64"] = r64.numpy()
        for kind, ac in (("f32", None), ("bf16", torch.bfloat16), ("f16", torch.float16)):
            r = ev(dl, torch.float32, ac)
            assert torch.isfinite(r).all(), (name, kind)
            out[p + "out." + kind] = r.float().numpy()
            out[p + "drift." + kind] = measure(r, r64)
        print(name, {k: out[p + "drift." + k].round(7).tolist() for k in DC.KINDS}, flush=True)

    written = golden_io.save(os.path.join(HERE, "diffloss.npz"), **out)
    print("wrote", [(os.path.basename(w), os.path.getsize(w)) for w in written])


if __name__ == "__main__":
    main()
