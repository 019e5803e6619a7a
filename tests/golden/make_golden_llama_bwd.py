"""Golden vectors for the backward pass through the frozen Llama (tests/golden/llama_bwd.npz, stage2_llm.npz).

Run where the reference checkout and `transformers` are available:  python tests/golden/make_golden_llama_bwd.py [llama_bwd] [stage2_llm]

llama_bwd.npz   HuggingFace LlamaForCausalLM (eager attention, every parameter frozen) on the seeded inputs of tests/llama_bwd_cases.py under
                torch autograd: the loss by the reference's own statements (rac_harness.rac_lm_loss), d loss / d inputs_embeds, and
                d sum(hidden * G) / d inputs_embeds for a seeded upstream G — in fp32 for every case, and from HF's own bf16 / fp16 autograd
                runs for the head-dim-128 cases (the drift yardstick of the 16-bit tests).
stage2_llm.npz  the reference's stage 2 with a real LLM behind the splice: the reference's build_vision_projector module -> the reference's
                prepare_inputs_labels_for_multimodal -> HF Llama -> rac_lm_loss -> backward(): loss, projector gradients, d loss / d tokens,
                d loss / d embed_tokens.weight.
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
import rac_harness as R          # noqa: E402
import setok_oracle as O         # noqa: E402

torch.set_grad_enabled(True)


def npy(t):
    return t.detach().cpu().float().numpy() if t.is_floating_point() else t.detach().cpu().numpy()


def save(name, **arrs):
    for path in golden_io.save(os.path.join(HERE, name + ".npz"), **arrs):
        print("wrote", path, os.path.getsize(path), "bytes")


def hf_llama(kw, lc, sd, dtype=torch.float32):
    from transformers import LlamaConfig, LlamaForCausalLM
    cfg = LlamaConfig(**kw, rms_norm_eps=lc.rms_norm_eps, rope_theta=lc.rope_theta, attention_bias=False, mlp_bias=False, tie_word_embeddings=False)
    cfg._attn_implementation = "eager"
    with torch.device("meta"):
        m = LlamaForCausalLM(cfg)
    m = m.to_empty(device="cpu").eval()
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=True, assign=True)
    inv = 1.0 / (lc.rope_theta ** (torch.arange(0, lc.head_dim, 2, dtype=torch.int64).float() / lc.head_dim))      # (non-persistent buffer: rebuilt as HF does)
    m.model.rotary_emb.inv_freq = inv
    if hasattr(m.model.rotary_emb, "original_inv_freq"):
        m.model.rotary_emb.original_inv_freq = inv
    return m.requires_grad_(False)


def hf_grads(m, x, am, pos, labels, G, dtype):
    """(loss, d loss / dx, d sum(hidden * G) / dx) by HF's autograd in `dtype`."""
    xe = x.to(dtype).clone().requires_grad_(True)
    out = m(inputs_embeds=xe, attention_mask=am, position_ids=pos, output_hidden_states=True)
    loss = R.rac_lm_loss(out.logits, labels, am)
    (g_loss,) = torch.autograd.grad(loss, xe, retain_graph=True)
    (g_hid,) = torch.autograd.grad((out.hidden_states[-1].float() * G).sum(), xe)
    return loss.detach().float(), g_loss.float(), g_hid.float()


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)), float(((a - b).pow(2).mean() / b.pow(2).mean()).sqrt())


def gen_llama_bwd():
    arrs = {}
    for name in C.LLAMA_CASES:
        kw, lc, seed, x, am, pos, labels, G = C.case_inputs(name)
        assert C.first_attended_label_is_ignored(labels, am), name
        sd = O.init_llama_weights(lc, seed=seed)
        m = hf_llama(kw, lc, sd)
        loss, g_loss, g_hid = hf_grads(m, x, am, pos, labels, G, torch.float32)
        pad = am == 0
        assert float(g_loss[pad].abs().max() if pad.any() else 0.0) == 0.0 and float(g_hid[pad].abs().max() if pad.any() else 0.0) == 0.0, name
        assert float(g_loss[~pad].abs().max()) > 0 and float(g_hid[~pad].abs().max()) > 0
        arrs[name + ":spec"] = np.array([seed, x.shape[0], x.shape[1], 1 if C.LLAMA_CASES[name][4] == "left" else 0])
        arrs[name + ":loss"] = npy(loss.reshape(1)); arrs[name + ":dx_loss"] = npy(g_loss); arrs[name + ":dx_hidden"] = npy(g_hid)
        line = f"{name}: loss {float(loss):.5f}"
        if name != "7bdims":                                    # the oracle's restatement under autograd gives HF's gradient
            xe = x.clone().requires_grad_(True)
            h, lg = O.llama_forward(sd, lc, xe, am, pos)
            (o_loss,) = torch.autograd.grad(R.rac_lm_loss(lg, labels, am), xe, retain_graph=True)
            (o_hid,) = torch.autograd.grad((h * G).sum(), xe)
            line += f"  oracle-vs-HF max-rel {rel(o_loss[~pad], g_loss[~pad])[0]:.2e} / {rel(o_hid[~pad], g_hid[~pad])[0]:.2e}"
        if name in C.DH128:
            for dt, tag in ((torch.bfloat16, "bf16"), (torch.float16, "fp16")):
                try:
                    ml = hf_llama(kw, lc, sd, dt)
                    _, l_loss, l_hid = hf_grads(ml, x, am, pos, labels, G, dt)
                except Exception as e:                           # (torch's CPU fp16 autograd: recorded when it does not run)
                    print(f"{name}: HF {tag} autograd did not run here: {type(e).__name__}: {e}")
                    continue
                assert float(l_loss[pad].abs().max() if pad.any() else 0.0) == 0.0 and float(l_hid[pad].abs().max() if pad.any() else 0.0) == 0.0
                arrs[f"{name}:dx_loss_{tag}"] = npy(l_loss); arrs[f"{name}:dx_hidden_{tag}"] = npy(l_hid)
                line += f"  HF-{tag} vs fp32 (max, rms): loss {rel(l_loss[~pad], g_loss[~pad])} hidden {rel(l_hid[~pad], g_hid[~pad])}"
        print(line)
        del m
    save("llama_bwd", **arrs)


def gen_stage2_llm():
    B_ = R.load_reference_projector_builder()
    arch = R.load_reference_arch()
    arrs = {}
    for name in C.STAGE2_LLM_CASES:
        c = C.stage2_llm_inputs(name)
        torch.manual_seed(c["seed"])
        proj = B_.build_vision_projector(c["ptype"], mm_hidden_size=c["Dt"], hidden_size=c["D"])
        g = torch.Generator().manual_seed(c["seed"] + 2000)
        with torch.no_grad():
            for p_ in proj.parameters():
                if p_.dim() == 1:
                    p_.add_(0.1 * torch.randn(p_.shape, generator=g))
        w0 = {n: p_.detach().clone() for n, p_ in proj.named_parameters()}
        m = hf_llama(c["lkw"], c["lc"], c["sd"])
        emb = m.model.embed_tokens
        emb.weight.requires_grad_(c["train_embed"])
        toks = [t.clone().requires_grad_(True) for t in c["toks"]]

        class _Model:
            embed_tokens = emb

        class _Cfg:
            pass
        cfg = _Cfg()
        cfg.tokenizer_model_max_length = c["kw"]["max_length"]
        cfg.tokenizer_padding_side = c["kw"].get("padding_side", "right")

        class Host(arch.SetokimMetaForCausalLM):
            config = cfg
            device = torch.device("cpu")

            def get_model(self):
                return _Model()

            def get_vision_tower(self):
                return object()

            def encode_images(self, images):
                return [proj(t) for t in toks]

        B, T = c["B"], c["T"]
        pos0 = torch.arange(T).expand(B, T).clone()
        images = torch.zeros(len(toks), 3, 2, 2)
        _, pos, am, _, embeds, new_labels = Host().prepare_inputs_labels_for_multimodal(c["ids"], pos0, c["am"], None, c["labels"], images)
        assert C.first_attended_label_is_ignored(new_labels, am), name
        full = O.splice_multimodal(c["ids"], pos0, c["am"], c["labels"], [torch.zeros(t.shape[0], 1) for t in c["toks"]], torch.zeros(c["V"], 1),
                                   None, cfg.tokenizer_padding_side)[2]                      # the same splice without max_length: was anything cut?
        truncated = full.shape[1] > embeds.shape[1]
        out = m(inputs_embeds=embeds, attention_mask=am, position_ids=pos)
        loss = R.rac_lm_loss(out.logits, new_labels, am)
        loss.backward()
        tg = torch.cat([t.grad if t.grad is not None else torch.zeros_like(t) for t in toks], 0)
        nz = int((tg.abs().sum(1) != 0).sum())
        assert truncated, f"{name}: max_length cuts no sequence"
        assert 2 * nz > tg.shape[0], f"{name}: only {nz} of {tg.shape[0]} token rows carry a gradient"
        arrs[name + ":loss"] = npy(loss.reshape(1))
        arrs[name + ":embeds"] = npy(embeds); arrs[name + ":new_labels"] = npy(new_labels); arrs[name + ":new_mask"] = npy(am)
        arrs[name + ":counts"] = np.array([t.shape[0] for t in toks])
        arrs[name + ":dtokens"] = npy(tg)
        for n, v in w0.items():
            arrs[f"{name}:w:{n}"] = npy(v)
        for n, p_ in proj.named_parameters():
            arrs[f"{name}:g:{n}"] = npy(p_.grad)
        if c["train_embed"]:
            arrs[name + ":dembed"] = npy(emb.weight.grad)
        print(f"{name}: loss {float(loss):.4f}  spliced {tuple(embeds.shape)} (untruncated length {full.shape[1]}: truncated={truncated})  "
              f"token rows with a gradient {nz} of {tg.shape[0]}")
    save("stage2_llm", **arrs)


if __name__ == "__main__":
    which = sys.argv[1:] or ["llama_bwd", "stage2_llm"]
    if "stage2_llm" in which:
        gen_stage2_llm()
    if "llama_bwd" in which:
        gen_llama_bwd()
