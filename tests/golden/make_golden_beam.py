"""Golden vectors for beam search (tests/golden/beam.npz).

Run where `transformers` is available:  python tests/golden/make_golden_beam.py

For each setting of tests/beam_cases.py (num_beams, length_penalty, early_stopping) HuggingFace LlamaForCausalLM (eager attention, fp32, CPU) runs its
own `generate(inputs_embeds=..., num_beams=...)` on a tiny seeded model (hidden 64, 2 layers, GQA 4/2, V = 100, the seeded weights times 3) with
B = 3 prompts, one of them left-padded, and 10 new tokens.  The eos list holds two ids taken from what the greedy run emits, so C = 3 * num_beams.
Seeds are searched in order and a seed is rejected when
  - the back-pointer statement of the rule (beam_cases.BeamReference) does not reproduce HF's sequences, beam_indices and scores (2e-6), or
  - the decision margin - the smallest gap between adjacent entries of the top C + 1 accumulated scores at any step, and between adjacent live entries
    of the finished-set ranking - is below 1.0e-3 (the margin the generate fixture uses for decisions), or
  - (the first three settings) no returned hypothesis ends early by an eos, or none runs to max_new_tokens.
Stored per case: the seed and the setting, the weights, the prompt, HF's sequences / sequences_scores / beam_indices with num_return_sequences = 1 and
= num_beams, the margin, and the reference's candidates and state after every step (what setok_beam_advance is checked against)."""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import beam_cases as BC                            # noqa: E402
import golden_io                                   # noqa: E402
import setok_oracle as O                           # noqa: E402
from make_golden_llama_bwd import hf_llama         # noqa: E402

SEEDS = range(3000)                                # (the length_penalty = 2 setting squeezes the finished scores together: its first seed is 2299)
TRACE = ("cand_score", "cand_token", "cand_beam", "run", "fin_score", "fin_flag", "fin_len", "fin_parent", "fin_token", "heur", "next_token", "src_row")


def greedy_tokens(sd, lc, x, am, pos, steps):
    """(B, steps): the oracle's uncached greedy run."""
    emb, toks = sd["model.embed_tokens.weight"], []
    for _ in range(steps):
        tok = O.llama_forward(sd, lc, x, am, pos)[1][:, -1].argmax(-1)
        toks.append(tok)
        x = torch.cat([x, emb[tok][:, None]], dim=1)
        am = torch.cat([am, torch.ones_like(am[:, :1])], dim=1)
        pos = torch.cat([pos, pos[:, -1:] + 1], dim=1)
    return torch.stack(toks, dim=1)


def hf_beams(m, x, am, n, lp, es, eos, R):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = m.generate(inputs_embeds=x, attention_mask=am, max_new_tokens=BC.N_NEW, num_beams=n, length_penalty=lp, early_stopping=es,
                         num_return_sequences=R, do_sample=False, eos_token_id=list(eos), pad_token_id=eos[0], return_dict_in_generate=True,
                         output_scores=True, output_logits=True, use_cache=True)
    return out.sequences, out.sequences_scores.float(), out.beam_indices.to(torch.int32)


def try_seed(name, seed):
    n, lp, es, both = BC.CASES[name]
    lc, sd = BC.weights(seed)
    x, am, pos = BC.prompts(seed)
    with torch.no_grad():
        g = greedy_tokens(sd, lc, x, am, pos, BC.N_NEW)
        eos = (int(g[0, 3]), int(g[1, 5]))
        if eos[0] == eos[1]:
            return None, "one eos id"
        ref = BC.run_reference(sd, lc, x, am, pos, n, lp, es, eos)
        if ref.margin < BC.MIN_MARGIN:
            return None, f"margin {ref.margin:.1e}"
        m = hf_llama(dict(BC.LLAMA), lc, sd)
        out = {}
        for R in (1, n):
            seq, score, anc = hf_beams(m, x, am, n, lp, es, eos, R)
            r_seq, r_score, r_anc = ref.hypotheses(R, eos[0])
            if seq.shape != r_seq.shape or not torch.equal(seq, r_seq) or not torch.equal(anc, r_anc):
                return None, f"the reference differs from HF (R = {R})"
            err = float((score - r_score).abs().max())
            if err > 2e-6:
                return None, f"scores differ by {err:.1e} (R = {R})"
            out[R] = (seq, score, anc)
        lengths = (out[1][2] >= 0).sum(dim=1)
        if both and not (bool((lengths < BC.N_NEW).any()) and bool((lengths == BC.N_NEW).any())):
            return None, f"lengths {lengths.tolist()}"
    arrs = {"spec": np.array([seed, n, BC.ES_CODE[es], eos[0], eos[1], ref.steps]), "length_penalty": np.array(lp, np.float64),
            "margin": np.array(ref.margin, np.float64), "x": x.numpy(), "am": am.numpy()}
    for k, v in sd.items():
        arrs["w:" + k] = v.numpy()
    for R, tag in ((1, "r1"), (n, "rn")):
        arrs[f"sequences_{tag}"], arrs[f"scores_{tag}"], arrs[f"beam_indices_{tag}"] = (t.numpy() for t in out[R])
    for k in TRACE:
        arrs["trace:" + k] = torch.stack([t[k] for t in ref.trace]).numpy()
    arrs["trace:go_on"] = np.array([t["go_on"] for t in ref.trace])
    return arrs, f"margin {ref.margin:.1e}  steps {ref.steps}  lengths (R = 1) {lengths.tolist()}"


def main():
    arrs = {}
    for name in BC.CASES:
        for seed in SEEDS:
            got, why = try_seed(name, seed)
            if got is not None:
                print(f"{name}: seed {seed}  {why}")
                arrs.update({f"{name}:{k}": v for k, v in got.items()})
                break
        else:
            raise SystemExit(f"{name}: no seed in {SEEDS} meets the conditions")
    for path in golden_io.save(os.path.join(HERE, "beam.npz"), **arrs):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
