"""Seeded inputs shared by tests/golden/make_golden_llama_bwd.py and the tests that read its fixtures (llama_bwd.npz, stage2_llm.npz):
everything here regenerates bit-exactly from the seed (torch CPU generator), so the fixtures store results only."""
import torch

import setok_oracle as O

IGNORE = -100

# the seven cases of tests/golden/make_golden.py (llama.npz), re-declared with the same seeds
LLAMA_CASES = {
    # name: (LlamaConfigLite kwargs, seed, B, T, padding)
    "tiny_right": (dict(hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=100), 7, 3, 11, "right"),
    "tiny_left": (dict(hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=100), 8, 3, 11, "left"),
    "dh128": (dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, vocab_size=128), 9, 2, 150, "right"),
    "dh128_left": (dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, vocab_size=128), 10, 2, 70, "left"),
    "gqa_tiny_left": (dict(hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=100), 11, 3, 13, "left"),
    "gqa_dh128": (dict(hidden_size=512, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=128), 12, 2, 150, "right"),
    "mqa_dh128_left": (dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=128), 13, 2, 70, "left"),
    # Vicuna-7B layer dims, two layers (LLAMA_7B_DIMS / LLAMA_7B_CASE of make_golden.py)
    "7bdims": (dict(hidden_size=4096, intermediate_size=11008, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=32, vocab_size=32000), 21, 2, 40, "right"),
}
DH128 = ("dh128", "dh128_left", "gqa_dh128", "mqa_dh128_left")


def labels_and_upstream(seed, B, T, V, D, am):
    """(labels, G).  labels: seeded targets with the first quarter of the positions, the padding and every sequence's FIRST attended token
    ignored — what a real prompt looks like (BOS / the prompt is never a target), and what makes the loss's gradient at padded rows exactly
    zero in HuggingFace's arithmetic too (no counted position sits on a padded row).  G: the seeded upstream of sum(hidden * G), zero at
    padded rows for the same reason."""
    g = torch.Generator().manual_seed(5000 + seed)
    labels = torch.randint(0, V, (B, T), generator=g)
    labels[:, : T // 4] = IGNORE
    labels[am == 0] = IGNORE
    first = am.bool().float().argmax(dim=1)
    labels[torch.arange(B), first] = IGNORE
    G = torch.randn(B, T, D, generator=g) * am[:, :, None].float()
    return labels, G


def first_attended_label_is_ignored(labels, am) -> bool:
    first = am.bool().float().argmax(dim=1)
    return bool((labels[torch.arange(labels.shape[0]), first] == IGNORE).all())


def case_inputs(name):
    kw, seed, B, T, padding = LLAMA_CASES[name]
    lc = O.LlamaConfigLite(**kw)
    x, am, pos = O.llama_inputs(lc, seed, B, T, padding)
    labels, G = labels_and_upstream(seed, B, T, lc.vocab_size, lc.hidden_size, am)
    return kw, lc, seed, x, am, pos, labels, G


# ---- stage 2 through a real Llama (stage2_llm.npz) ---------------------------------------------------------------------------------
STAGE2_LLAMA = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1)   # Dh = 128, grouped-query
STAGE2_LLM_CASES = {
    # name: (projector type, seed, B, T, V, Dt, splice kwargs, train_embed, llama seed).  Seeds and lengths are chosen so that max_length cuts at least
    # one sequence AND more than half of the token rows carry a gradient (the generator asserts both and prints the counts): at hidden 256 the
    # right-padded batch of seed 12 has its longest sequence at 15 positions and 12 of 39 live rows at any shorter max_length; seed 14 (lengths
    # 4 18 13 9 1 7, cut at 16) gives 23 of 38, seed 13 left-padded (26 20 10 14, cut at 20) 35 of 53.
    "linear_right_trunc": ("linear", 14, 6, 10, 128, 96, dict(max_length=16), True, 31),
    "mlp2x_left_trunc": ("mlp2x_gelu", 13, 4, 14, 128, 96, dict(max_length=20, padding_side="left"), False, 32),
}


def stage2_llm_inputs(name):
    ptype, seed, B, T, V, Dt, kw, train_embed, lseed = STAGE2_LLM_CASES[name]
    lkw = dict(STAGE2_LLAMA, vocab_size=V)
    lc = O.LlamaConfigLite(**lkw)
    D = lc.hidden_size
    ids, am, labels, feats, _ = O.splice_inputs(seed, B, T, V, D)
    labels = labels.clone()
    labels[labels == O.TARGET_TOKEN_INDEX] = IGNORE          # the reference's cross entropy cannot take -300 targets
    labels[:, 0] = IGNORE                                    # the first token of a prompt is never a target
    g = torch.Generator().manual_seed(seed + 1000)
    toks = [torch.randn(f.shape[0], Dt, generator=g) for f in feats]
    sd = O.init_llama_weights(lc, seed=lseed)
    sd["model.embed_tokens.weight"] = sd["model.embed_tokens.weight"] * 50.0     # rows of unit scale, like the projected tokens next to them
    return dict(ptype=ptype, seed=seed, B=B, T=T, V=V, Dt=Dt, D=D, kw=kw, train_embed=train_embed, lkw=lkw, lc=lc, ids=ids, am=am,
                labels=labels, toks=toks, sd=sd)
