"""Golden vectors for extending a filled KV cache by a ragged, masked chunk (tests/golden/extend.npz).

Run where `transformers` is available:  python tests/golden/make_golden_extend.py

For two grouped-query cases of tests/llama_bwd_cases.py (seeded weights and inputs, regenerated, not stored) HuggingFace LlamaForCausalLM (eager
attention, fp32, CPU) runs the prompt with `use_cache=True` and then ONE forward over a seeded chunk of TN embedding rows appended to
`past_key_values`, with a chunk mask that has a shorter sequence and a hole, the 2-d attention mask grown by the chunk's and the chunk's positions
continuing from every sequence's last attended position (a masked row takes the position the next attended row will take).  Stored per case:
    chunk_mask (B, TN)   hidden (B, TN, D: final norm)   logits (B, TN, V)
The chunk's embeddings regenerate from `chunk_inputs(name)`.  Asserted here: HF cached == HF uncached (prompt and chunk recomputed from scratch in
one forward) within 1e-5 on the attended rows.  The rows at masked positions are stored but mean nothing (the test leaves them out)."""
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

CASES = ("gqa_tiny_left", "gqa_dh128")
TN = 9


def chunk_inputs(name):
    """(chunk (B, TN, D), chunk_mask (B, TN) int64): seeded; the last sequence's chunk is two rows shorter, the second has a hole, and with three
    sequences the third starts with a masked row."""
    kw, seed, B, _, _ = C.LLAMA_CASES[name]
    g = torch.Generator().manual_seed(7000 + seed)
    chunk = torch.randn(B, TN, kw["hidden_size"], generator=g)
    cm = torch.ones(B, TN, dtype=torch.long)
    cm[1, TN // 2] = 0
    if B > 2:
        cm[2, 0] = 0
    cm[B - 1, TN - 2:] = 0
    return chunk, cm


def main():
    from make_golden_llama_bwd import hf_llama
    arrs = {}
    with torch.no_grad():
        for name in CASES:
            kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
            m = hf_llama(kw, lc, O.init_llama_weights(lc, seed=seed))
            B, T, _ = x.shape
            chunk, cm = chunk_inputs(name)
            out = m(inputs_embeds=x, attention_mask=am, position_ids=pos, use_cache=True)
            last = (am * torch.arange(T)[None]).max(dim=1).values
            nxt = pos[torch.arange(B), last] + 1
            cpos = nxt[:, None] + cm.cumsum(1) - cm
            am2 = torch.cat([am, cm], 1)
            ext = m(inputs_embeds=chunk, attention_mask=am2, position_ids=cpos, past_key_values=out.past_key_values, use_cache=True,
                    output_hidden_states=True)
            full = m(inputs_embeds=torch.cat([x, chunk], 1), attention_mask=am2, position_ids=torch.cat([pos, cpos], 1), output_hidden_states=True)
            live = cm.bool()
            a, b = ext.logits[live].float(), full.logits[:, T:][live].float()
            unc = float((a - b).abs().max() / b.abs().max())
            assert unc <= 1e-5, (name, unc)
            arrs[name + ":chunk_mask"] = cm.numpy()
            arrs[name + ":hidden"] = ext.hidden_states[-1].float().numpy()
            arrs[name + ":logits"] = ext.logits.float().numpy()
            print(f"{name}: chunk of {TN} rows, attended per sequence {cm.sum(1).tolist()}, cached-vs-uncached max-rel {unc:.1e}")
    for path in golden_io.save(os.path.join(HERE, "extend.npz"), **arrs):
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
