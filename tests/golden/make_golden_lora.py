"""Golden vectors for LoRA fine-tuning of the Llama stack (tests/golden/lora.npz, stored in parts).

Run where the reference checkout and `transformers` are available:  python tests/golden/make_golden_lora.py

HuggingFace LlamaForCausalLM (eager attention, every base parameter frozen, as make_golden_llama_bwd.py builds it) on the seeded inputs of
tests/llama_bwd_cases.py, with the LoRA rule `base(x) + s * B(A(drop(x)))` wrapped around its seven Linears in plain torch
(tests/lora_cases.py: seeded adapters with a non-zero B, no dropout), under torch autograd with the loss by the reference's own statements
(rac_harness.rac_lm_loss):
  {case}:r16:loss / dx / g:{layer}.{target}.lora_A|B     fp32, r = 16, the four cases of lora_cases.FP32_CASES
  {case}:r64:loss / dx / g:...                           fp32, r = 64, the head-dim-128 cases of lora_cases.LOW_CASES
  {case}:r64:{bf16|fp16}:{dx|dA|dB}                      (max-rel, rms-rel) of HF's OWN 16-bit autograd run of the same adapted model against
                                                         its fp32 run — dx at the attended rows, all dA concatenated, all dB concatenated: the
                                                         drift yardstick.  Only these two numbers are kept of a 16-bit run, not its tensors.
Nothing of the reference's text is kept here: its modules are loaded from the checkout by oracle/rac_harness.py at run time."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))
import golden_io                 # noqa: E402
import llama_bwd_cases as C      # noqa: E402
import lora_cases as LC          # noqa: E402
import rac_harness as R          # noqa: E402
import setok_oracle as O         # noqa: E402

torch.set_grad_enabled(True)
cat = LC.cat_grads


def npy(t):
    return t.detach().cpu().float().numpy()


def run(name, r, dtype):
    """(loss, dx, {adapter name: gradient}) of the adapted HF model in `dtype`, as fp32 tensors."""
    kw, lc, seed, x, am, pos, labels, G = C.case_inputs(name)
    sd = O.init_llama_weights(lc, seed=seed)
    m = LC.hf_llama(kw, lc, sd, dtype)
    wrapped = LC.wrap_hf(m, LC.adapters(lc, r, seed), LC.SCALING, dtype)
    xe = x.to(dtype).clone().requires_grad_(True)
    out = m(inputs_embeds=xe, attention_mask=am, position_ids=pos)
    loss = R.rac_lm_loss(out.logits, labels, am)
    assert dtype != torch.float32 or abs(float(loss.detach()) - float(LC.lm_loss(out.logits.detach(), labels, am))) < 1e-5 * abs(float(loss.detach()))
    loss.backward()
    grads = {}
    for k, mod in wrapped.items():
        grads[k + ".lora_A"], grads[k + ".lora_B"] = mod.lora_A.grad.float(), mod.lora_B.grad.float()
    return loss.detach().float(), xe.grad.float(), grads, am


def rel(a, b):
    return np.array([float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)), float(((a - b).pow(2).mean() / b.pow(2).mean()).sqrt())])


def main():
    arrs = {}
    for name in LC.FP32_CASES:
        loss, dx, grads, am = run(name, LC.R32, torch.float32)
        pad = am == 0
        assert float(dx[pad].abs().max() if pad.any() else 0.0) == 0.0 and all(float(g.abs().max()) > 0 for g in grads.values()), name
        arrs[f"{name}:r16:loss"] = npy(loss.reshape(1)); arrs[f"{name}:r16:dx"] = npy(dx)
        for k, g in grads.items():
            arrs[f"{name}:r16:g:{k}"] = npy(g)
        print(f"{name} r16: loss {float(loss):.5f}  |dA| {float(cat(grads, 'lora_A').abs().max()):.3e}  |dB| {float(cat(grads, 'lora_B').abs().max()):.3e}")
    for name in LC.LOW_CASES:
        loss, dx, grads, am = run(name, LC.R16, torch.float32)
        v = am.bool()
        arrs[f"{name}:r64:loss"] = npy(loss.reshape(1)); arrs[f"{name}:r64:dx"] = npy(dx)
        for k, g in grads.items():
            arrs[f"{name}:r64:g:{k}"] = npy(g)
        for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
            _, ldx, lgrads, _ = run(name, LC.R16, dt)
            assert float(ldx[~v].abs().max() if (~v).any() else 0.0) == 0.0
            arrs[f"{name}:r64:{tag}:dx"] = rel(ldx[v], dx[v])
            arrs[f"{name}:r64:{tag}:dA"] = rel(cat(lgrads, "lora_A"), cat(grads, "lora_A"))
            arrs[f"{name}:r64:{tag}:dB"] = rel(cat(lgrads, "lora_B"), cat(grads, "lora_B"))
            print(f"{name} r64 HF-{tag} vs fp32 (max, rms): dx {arrs[f'{name}:r64:{tag}:dx']} dA {arrs[f'{name}:r64:{tag}:dA']} dB {arrs[f'{name}:r64:{tag}:dB']}")
    for path in golden_io.save(os.path.join(HERE, "lora.npz"), **arrs):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
