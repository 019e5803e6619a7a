"""Golden vectors for the logits processors (tests/golden/processors.npz).

Run where `transformers` is available:  python tests/golden/make_golden_processors.py

For each setting of tests/processors_cases.py HuggingFace LlamaForCausalLM (eager attention, fp32, CPU) runs its own
`generate(input_ids=..., repetition_penalty=..., no_repeat_ngram_size=..., min_new_tokens=..., suppress_tokens=..., do_sample=False)` on the tiny seeded
model of the beam fixture (hidden 64, 2 layers, GQA 4/2, V = 100, the seeded weights times 3) with 10 new tokens.  Every sequence runs ALONE and
unpadded: HF counts pad ids in the history its processors see, this project skips masked columns.  The three prompts have 9, 6 and 8 ids, so the
batched test left-pads.  One case feeds `inputs_embeds` alone: its histories start empty.  The eos ids of the minimum-length case are what the
unprocessed greedy run emits at step 2 (reachable, and banned until 6 tokens are out); its suppressed ids are two other tokens of that run.
Seeds are searched in order; one seed serves all cases and is kept only if, for every case and sequence,
  - the torch statement of the rule (processors_cases.process) fed by the oracle's forward reproduces HF's tokens, and HF's processed scores to 2e-5,
  - the gap between the two best processed scores is >= 1.0e-3 at every step (the generate fixture's margin),
and, for every case, some sequence emits a token that differs from the unprocessed greedy run and - the n-gram and minimum-length cases - the raw
argmax is banned at one step or more.
Stored: the seed, the weights, the prompts, and per case the setting, HF's tokens (-1 past a sequence's end), the lengths, HF's processed scores
and the margin."""
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
import golden_io                                   # noqa: E402
import processors_cases as PC                      # noqa: E402
from make_golden_llama_bwd import hf_llama         # noqa: E402

SEEDS = range(3000)


def hf_run(m, ids, x, penalty, ngram, min_new, eos, suppress):
    """HF's greedy run of one sequence: (new tokens (n,), processed scores (n, V))."""
    prompt = dict(inputs_embeds=x[None]) if ids is None else dict(input_ids=ids[None])
    prompt["attention_mask"] = torch.ones(1, x.shape[0], dtype=torch.long)                 # (explicit: HF would mask prompt ids equal to the pad id)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = m.generate(**prompt, max_new_tokens=PC.N_NEW, do_sample=False, repetition_penalty=penalty if penalty != 1.0 else None,
                         no_repeat_ngram_size=ngram or None, min_new_tokens=min_new or None, suppress_tokens=list(suppress) or None,
                         eos_token_id=list(eos) or None, pad_token_id=eos[0] if eos else 0, return_dict_in_generate=True, output_scores=True,
                         use_cache=True)
    new = out.sequences[0] if ids is None else out.sequences[0, ids.numel():]
    return new, torch.cat(out.scores, dim=0).float()


def try_seed(seed):
    lc, sd = PC.weights(seed)
    ids, am, x = PC.prompts(seed)
    emb = sd["model.embed_tokens.weight"]
    m = hf_llama(dict(PC.LLAMA), lc, sd)
    m.generation_config.eos_token_id = None                                                # (LlamaConfig's default eos id 2 would end the runs)
    arrs = {"seed": np.array(seed), "ids": ids.numpy(), "am": am.numpy(), "x": x.numpy()}
    notes = []
    for name, (penalty, ngram, min_new, n_sup, embeds, must_ban) in PC.CASES.items():
        seqs = [(None if embeds else ids[b, PC.T - n:], x[b, PC.T - n:] if embeds else emb[ids[b, PC.T - n:]]) for b, n in enumerate(PC.PROMPT_LEN)]
        empty = torch.zeros(0, dtype=torch.int64)
        free = [PC.run_reference(sd, lc, xe, empty if i is None else i, 1.0, 0, 0, (), ()) for i, xe in seqs]
        eos, suppress = (), ()
        if min_new:
            eos = tuple(sorted({int(f["tokens"][2]) for f in free}))
            suppress = (int(free[0]["tokens"][0]), int(free[1]["tokens"][1]))
            if len(set(suppress)) != n_sup or set(suppress) & set(eos):
                return None, f"{name}: suppressed ids {suppress} / eos {eos}"
        tokens = torch.full((PC.B, PC.N_NEW), -1, dtype=torch.int64)
        scores = torch.zeros(PC.B, PC.N_NEW, PC.LLAMA["vocab_size"])
        lengths, margin, differs, banned = [], float("inf"), False, False
        for b, (i, xe) in enumerate(seqs):
            ref = PC.run_reference(sd, lc, xe, empty if i is None else i, penalty, ngram, min_new, eos, suppress)
            hf_tok, hf_sc = hf_run(m, i, xe, penalty, ngram, min_new, eos, suppress)
            n = ref["tokens"].numel()
            if hf_tok.numel() != n or not torch.equal(hf_tok, ref["tokens"]):
                return None, f"{name}[{b}]: the statement's tokens differ from HF's"
            if not torch.equal(hf_sc == PC.NEG_INF, ref["scores"] == PC.NEG_INF):
                return None, f"{name}[{b}]: the banned sets differ from HF's"
            err = float((hf_sc - ref["scores"]).masked_fill(hf_sc == PC.NEG_INF, 0.0).abs().max())
            if err > 2e-5:
                return None, f"{name}[{b}]: scores differ from HF's by {err:.1e}"
            if ref["margin"] < PC.MIN_MARGIN:
                return None, f"{name}[{b}]: margin {ref['margin']:.1e}"
            margin = min(margin, ref["margin"])
            k = min(n, free[b]["tokens"].numel())
            differs = differs or n != free[b]["tokens"].numel() or not torch.equal(ref["tokens"][:k], free[b]["tokens"][:k])
            banned = banned or bool((ref["scores"][torch.arange(n), ref["raw"]] == PC.NEG_INF).any())
            tokens[b, :n], scores[b, :n] = hf_tok, hf_sc
            lengths.append(n)
        if not differs:
            return None, f"{name}: no token differs from the unprocessed run"
        if must_ban and not banned:
            return None, f"{name}: the raw argmax is never banned"
        if min_new and min(lengths) < min_new:                                             # (the unprocessed run meets an eos id at step 2 at the latest)
            return None, f"{name}: lengths {lengths}"
        arrs.update({f"{name}:tokens": tokens.numpy(), f"{name}:scores": scores.numpy(), f"{name}:lengths": np.array(lengths),
                     f"{name}:margin": np.array(margin, np.float64), f"{name}:eos": np.array(eos, np.int64),
                     f"{name}:suppress": np.array(suppress, np.int64)})
        notes.append(f"{name}: margin {margin:.1e} lengths {lengths}")
    for k, v in sd.items():
        arrs["w:" + k] = v.numpy()
    return arrs, "; ".join(notes)


def main():
    for seed in SEEDS:
        got, why = try_seed(seed)
        if got is not None:
            print(f"seed {seed}: {why}")
            break
        print(f"seed {seed} rejected - {why}")
    else:
        raise SystemExit(f"no seed in {SEEDS} meets the conditions")
    for path in golden_io.save(os.path.join(HERE, "processors.npz"), **got):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
