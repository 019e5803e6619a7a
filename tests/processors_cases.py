"""Logits processors: a torch statement of the rule (include/setok_hip.h, "Logits processors") and the cases of tests/golden/processors.npz.
tests/golden/make_golden_processors.py checks the statement, fed by the oracle's `llama_forward`, against HuggingFace's own
`generate(repetition_penalty=..., no_repeat_ngram_size=..., min_new_tokens=..., suppress_tokens=...)` and records what the GPU tests compare with;
tests/test_processors_cpu.py re-runs it and holds it against HF's four processor classes."""
import torch

import setok_oracle as O
from beam_cases import LLAMA, WEIGHT_SCALE, weights  # noqa: F401  (the tiny seeded fp32 Llama of the beam fixture)

B, T, N_NEW = 3, 9, 10
PROMPT_LEN = (9, 6, 8)                             # the batched test left-pads sequences 1 and 2
PROMPT_IDS = 12                                    # prompts draw from ids [0, 12): tokens repeat inside a prompt
MIN_MARGIN = 1.0e-3
NEG_INF = float("-inf")

# name: (repetition_penalty, no_repeat_ngram_size, min_new_tokens, suppressed ids wanted, the prompt is embeddings only, the raw argmax must be banned)
CASES = {
    "pen13": (1.3, 0, 0, 0, False, False),
    "g2": (1.0, 2, 0, 0, False, True),
    "g3_pen12": (1.2, 3, 0, 0, False, True),
    "minnew6_sup2": (1.0, 0, 6, 2, False, True),
    "embeds_pen13_g2": (1.3, 2, 0, 0, True, False),
}


def process(logits, hist, hist_len, prompt_len, tail=None, penalty=1.0, ngram=0, min_new=0, eos=(), suppress=()):
    """The rule.  logits (B * n, V) in any float type; hist (B, cap_h) int64 with hist_len (B,) valid entries, prompt_len (B,); tail (B, n - 1)
    int64 or None (n = 1): row b * n + i sees hist[b, :hist_len[b]] followed by tail[b, :i].  Returns fp32 (B * n, V) on the CPU."""
    x = logits.detach().cpu().float()
    hist, hist_len, prompt_len = hist.cpu(), hist_len.cpu(), prompt_len.cpu()
    rows, V = x.shape
    Bn = hist.shape[0]
    n = rows // Bn
    assert rows == Bn * n and (n == 1 or tuple(tail.shape) == (Bn, n - 1))
    pen = torch.tensor(float(penalty), dtype=torch.float32)                                # rounded to fp32 once
    out = x.clone()
    inside = lambda t: (t >= 0) & (t < V)
    for r in range(rows):
        b, i = divmod(r, n)
        hs = hist[b, :int(hist_len[b])]
        if i:
            hs = torch.cat([hs, tail[b, :i].cpu()])
        L = hs.numel()
        if float(penalty) != 1.0:
            ids = hs[inside(hs)]
            xs = x[r, ids]                                                                 # from the untouched input: once, however often an id occurs
            out[r, ids] = torch.where(xs < 0, xs * pen, xs / pen)
        g = int(ngram)
        if g >= 1 and L + 1 >= g:
            suffix = hs[L - g + 1:]
            if bool(inside(suffix).all()) and L >= g:
                w = hs.unfold(0, g, 1)                                                     # (L - g + 1, g): every window j in [0, L - g]
                banned = w[(w[:, :g - 1] == suffix).all(dim=1), g - 1]
                out[r, banned[inside(banned)]] = NEG_INF
        if min_new > 0 and L - int(prompt_len[b]) < min_new:
            for e in eos:
                if 0 <= int(e) < V:
                    out[r, int(e)] = NEG_INF
        for s in suppress:
            if 0 <= int(s) < V:
                out[r, int(s)] = NEG_INF
    return out


def append(hist, hist_len, emitted, m=None):
    """setok_history_append on CPU copies: (hist, hist_len) after hist[b, hist_len[b]:] = emitted[b, :m[b]] (m None: all of the row)."""
    hist, hist_len = hist.cpu().clone(), hist_len.cpu().clone()
    for b in range(hist.shape[0]):
        k = emitted.shape[1] if m is None else min(max(int(m[b]), 0), emitted.shape[1])
        L = int(hist_len[b])
        hist[b, L:L + k] = emitted[b, :k].cpu()
        hist_len[b] = L + k
    return hist, hist_len


def same(a, b):
    """torch.equal with NaN positions equal."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def prompts(seed):
    """ids (B, T) int64 left-padded with 0 and their mask: sequence b holds PROMPT_LEN[b] ids from [0, PROMPT_IDS); x (B, T, D), the embeddings-only
    prompts of the same lengths (masked columns are zeros)."""
    g = torch.Generator().manual_seed(7000 + seed)
    ids = torch.zeros(B, T, dtype=torch.int64)
    am = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(PROMPT_LEN):
        ids[b, T - n:] = torch.randint(0, PROMPT_IDS, (n,), generator=g)
        am[b, T - n:] = 1
    x = torch.randn(B, T, LLAMA["hidden_size"], generator=g) * am[:, :, None]
    return ids, am, x


def run_reference(sd, lc, x, ids, penalty, ngram, min_new, eos, suppress, max_new=N_NEW):
    """One sequence alone and unpadded, the rule driven by the oracle's uncached forward.  x (T_b, D) prompt embeddings, ids (T_b,) int64 the
    history they start from (empty with an embeddings-only prompt).  Greedy; ends behind an eos.  Returns dict(tokens (n,), scores (n, V), raw
    (n,) = argmax of the unprocessed logits at every step, margin = the smallest gap between the two best processed scores)."""
    emb = sd["model.embed_tokens.weight"]
    hist = torch.full((1, ids.numel() + max_new), -1, dtype=torch.int64)
    hist[0, :ids.numel()] = ids
    hist_len = torch.tensor([ids.numel()])
    prompt_len = hist_len.clone()
    x = x[None]
    toks, scs, raws, margin = [], [], [], float("inf")
    with torch.no_grad():
        for _ in range(max_new):
            logits = O.llama_forward(sd, lc, x, torch.ones(1, x.shape[1], dtype=torch.long), None)[1][:, -1]
            sc = process(logits, hist, hist_len, prompt_len, None, penalty, ngram, min_new, eos, suppress)
            top = torch.topk(sc[0], 2).values
            margin = min(margin, float(top[0] - top[1]))
            tok = sc.argmax(dim=-1)
            toks.append(int(tok)); scs.append(sc[0]); raws.append(int(logits.argmax(dim=-1)))
            hist, hist_len = append(hist, hist_len, tok[:, None])
            if int(tok) in eos:
                break
            x = torch.cat([x, emb[tok][:, None]], dim=1)
    return dict(tokens=torch.tensor(toks), scores=torch.stack(scs), raw=torch.tensor(raws), margin=margin)
