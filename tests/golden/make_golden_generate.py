"""Golden vectors for KV-cached greedy generation (tests/golden/generate.npz).

Run where `transformers` is available:  python tests/golden/make_golden_generate.py

For each of the eight cases of tests/llama_bwd_cases.py (seeded weights and inputs, regenerated, not stored) HuggingFace LlamaForCausalLM (eager
attention, fp32, CPU) runs a manual greedy loop with `past_key_values`: the prompt's last attended position gives the step-0 logits, every
following step feeds the argmax id, and the mask and the positions are extended as HF's generate extends them (one attended slot per step, at
position = the last attended position + 1).  Stored per case:
    tokens (n_new, B)   logits (n_new, B, V)   hidden (n_new, B, D: final norm)   margin (n_new, B) = (top1 - top2) / max|logit|
and, for the four head-dim-128 cases, HF's OWN bfloat16 and float16 logits under teacher forcing with the fp32 tokens (the drift yardstick of the
16-bit tests).  Asserted here: HF cached == HF uncached (the whole sequence recomputed) within 1e-5, and every margin >= 5e-4 — five times the
fp32 logit tolerance of the GPU tests, so an fp32 GPU run has no excuse for a different token at any step."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import golden_io                                   # noqa: E402
import llama_bwd_cases as C                        # noqa: E402
import setok_oracle as O                           # noqa: E402
from make_golden_llama_bwd import hf_llama         # noqa: E402

N_NEW = 16
N_NEW_7B = 4                                       # 256 KB of logits per step
MIN_MARGIN = 5e-4


def n_new(name):
    return N_NEW_7B if name == "7bdims" else N_NEW


def npy(t):
    return t.detach().cpu().float().numpy() if t.is_floating_point() else t.detach().cpu().numpy()


def greedy(m, x, am, pos, steps, forced=None):
    """The manual greedy loop with past_key_values.  forced (steps, B): feed these ids instead of the model's own argmax (teacher forcing).
    Returns tokens (steps, B), logits (steps, B, V), hidden (steps, B, D), and the embeddings / masks / positions of the grown sequence."""
    B, T, _ = x.shape
    dt = m.lm_head.weight.dtype
    last = (am * torch.arange(T)[None]).max(dim=1).values
    rows = torch.arange(B)
    out = m(inputs_embeds=x.to(dt), attention_mask=am, position_ids=pos, use_cache=True, output_hidden_states=True)
    pkv = out.past_key_values
    lg, hid = out.logits[rows, last].float(), out.hidden_states[-1][rows, last].float()
    nxt = pos[rows, last] + 1
    toks, lgs, hids = [], [], []
    xs, ams, poss = x, am, pos
    for j in range(steps):
        tok = lg.argmax(-1) if forced is None else forced[j]
        toks.append(tok); lgs.append(lg); hids.append(hid)
        if j + 1 == steps:
            break
        e = m.model.embed_tokens(tok)[:, None]
        ams = torch.cat([ams, torch.ones(B, 1, dtype=ams.dtype)], 1)
        poss = torch.cat([poss, nxt[:, None]], 1)
        xs = torch.cat([xs, e.float()], 1)
        out = m(inputs_embeds=e, attention_mask=ams, position_ids=nxt[:, None], past_key_values=pkv, use_cache=True, output_hidden_states=True)
        pkv = out.past_key_values
        lg, hid = out.logits[:, -1].float(), out.hidden_states[-1][:, -1].float()
        nxt = nxt + 1
    return torch.stack(toks), torch.stack(lgs), torch.stack(hids), xs, ams, poss


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)), float(((a - b).pow(2).mean() / b.pow(2).mean()).sqrt())


def main():
    arrs = {}
    with torch.no_grad():
        for name in C.LLAMA_CASES:
            kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
            sd = O.init_llama_weights(lc, seed=seed)
            m = hf_llama(kw, lc, sd)
            steps = n_new(name)
            toks, lgs, hids, xs, ams, poss = greedy(m, x, am, pos, steps)
            # HF uncached: the grown sequence recomputed from scratch reproduces the last step's logits
            full = m(inputs_embeds=xs, attention_mask=ams, position_ids=poss).logits[:, -1].float()
            unc = rel(full, lgs[-1])[0]
            assert unc <= 1e-5, (name, unc)
            top2 = lgs.topk(2, dim=-1).values
            margin = (top2[..., 0] - top2[..., 1]) / lgs.abs().amax(dim=-1)
            assert float(margin.min()) >= MIN_MARGIN, (name, float(margin.min()))
            arrs[name + ":spec"] = np.array([seed, x.shape[0], x.shape[1], 1 if C.LLAMA_CASES[name][4] == "left" else 0, steps])
            arrs[name + ":tokens"] = npy(toks); arrs[name + ":logits"] = npy(lgs); arrs[name + ":hidden"] = npy(hids)
            arrs[name + ":margin"] = npy(margin)
            line = f"{name}: steps {steps}  min margin {float(margin.min()):.1e}  cached-vs-uncached max-rel {unc:.1e}"
            if name in C.DH128:
                for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
                    ml = hf_llama(kw, lc, sd, dt)
                    _, l_lgs, _, _, _, _ = greedy(ml, x, am, pos, steps, forced=toks)
                    arrs[f"{name}:logits_{tag}"] = npy(l_lgs)
                    line += f"  HF-{tag} vs fp32 (max, rms) {rel(l_lgs, lgs)}"
            print(line)
            del m
    for path in golden_io.save(os.path.join(HERE, "generate.npz"), **arrs):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
