"""Beam search: the cases of tests/golden/beam.npz and a torch statement of the rule (include/setok_hip.h, "Beam search") in the form the library
keeps it - running beams, a finished set, and hypotheses as back-pointers - fed by the oracle's `llama_forward`.  tests/golden/make_golden_beam.py
checks it against HuggingFace's `generate(num_beams=...)` and records what the GPU tests compare with; tests/test_beam_cpu.py re-runs it."""
import torch

import setok_oracle as O

LLAMA = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=100)
WEIGHT_SCALE = 3.0                                 # the seeded weights times 3: logits that are not flat
B, T, N_NEW = 3, 9, 10
MIN_MARGIN = 1.0e-3
NEG = -1.0e9

# name: (num_beams, length_penalty, early_stopping, an early finisher and a full-length hypothesis are required)
CASES = {
    "n2_lp1_false": (2, 1.0, False, True),
    "n4_lp1_true": (4, 1.0, True, True),
    "n3_lp06_never": (3, 0.6, "never", True),
    "n4_lp2_false": (4, 2.0, False, False),
}
ES_CODE = {False: 0, True: 1, "never": 2}


def weights(seed):
    lc = O.LlamaConfigLite(**LLAMA)
    return lc, {k: v * WEIGHT_SCALE for k, v in O.init_llama_weights(lc, seed=seed).items()}


def prompts(seed):
    """x (B, T, D), attention mask with row 1 left-padded, HF generate's positions for it."""
    g = torch.Generator().manual_seed(3000 + seed)
    x = torch.randn(B, T, LLAMA["hidden_size"], generator=g)
    am = torch.ones(B, T, dtype=torch.long)
    am[1, :3] = 0
    pos = (am.cumsum(-1) - 1).masked_fill(am == 0, 1)
    return x, am, pos


def _best(values, k):
    """Indices of the k best entries of each row by (value descending, index ascending): the library's total order."""
    return torch.sort(values, dim=1, descending=True, stable=True)[1][:, :k]


def _gaps(sorted_desc):
    """The smallest gap between adjacent live (> -1e8) entries of rows sorted in descending order."""
    a, b = sorted_desc[:, :-1], sorted_desc[:, 1:]
    live = b > -1.0e8
    return float((a - b)[live].min()) if bool(live.any()) else float("inf")


class BeamReference:
    """The rule on explicit per-step logits.  `step(logits)` takes (B * n_in, V) logits (n_in = 1 at step 0) and returns whether the loop continues;
    afterwards `next_token` / `src_row` (B * n) say what to feed and from which row's state.  `trace` keeps every step's candidates and the state
    after it; `margin` is the smallest gap any ordering of the run depended on."""

    def __init__(self, Bn, n, C, eos, max_new, length_penalty, early_stopping):
        self.B, self.n, self.C, self.max_new, self.lp, self.es = Bn, n, C, max_new, float(length_penalty), early_stopping
        self.eos = torch.as_tensor(list(eos), dtype=torch.int64)
        self.run = torch.zeros(Bn, 1)
        self.fin_score = torch.full((Bn, n), NEG)
        self.fin_flag = torch.zeros(Bn, n, dtype=torch.bool)
        self.fin_len = torch.zeros(Bn, n, dtype=torch.int64)
        self.fin_parent = torch.zeros(Bn, n, dtype=torch.int64)
        self.fin_token = torch.zeros(Bn, n, dtype=torch.int64)
        self.heur = torch.ones(Bn, dtype=torch.bool)
        self.bp_token, self.bp_parent, self.trace = [], [], []
        self.margin, self.steps = float("inf"), 0

    def step(self, logits):
        Bn, n, C, s = self.B, self.n, self.C, self.steps
        V = logits.shape[-1]
        acc = (torch.log_softmax(logits.float(), dim=-1).view(Bn, -1, V) + self.run[:, :, None]).reshape(Bn, -1)
        order = torch.sort(acc, dim=1, descending=True, stable=True)
        self.margin = min(self.margin, _gaps(order[0][:, :C + 1]))
        score, flat = order[0][:, :C], order[1][:, :C]
        beam, tok = flat // V, flat % V
        hit = torch.isin(tok, self.eos) | (s + 1 >= self.max_new)
        # the next running beams
        rs = score + hit.float() * NEG
        keep = _best(rs, n)
        self.run = rs.gather(1, keep)
        self.next_token = tok.gather(1, keep).reshape(-1)
        parent = beam.gather(1, keep)
        self.src_row = (parent + torch.arange(Bn)[:, None] * n).reshape(-1)
        self.bp_token.append(self.next_token.clone())
        self.bp_parent.append(parent.reshape(-1).clone())
        # the finished set
        did = hit & (torch.arange(C)[None] < n)
        ns = score / ((s + 1) ** self.lp)
        ns = ns + (self.fin_flag.all(dim=1, keepdim=True) & (self.es is True)).float() * NEG
        ns = ns + (~self.heur)[:, None].float() * NEG
        ns = ns + (~did).float() * NEG
        merged = torch.cat([self.fin_score, ns], dim=1)
        self.margin = min(self.margin, _gaps(torch.sort(merged, dim=1, descending=True)[0]))
        sel = _best(merged, n)
        cat = lambda old, new: torch.cat([old, new], dim=1).gather(1, sel)
        self.fin_score = merged.gather(1, sel)
        self.fin_flag = cat(self.fin_flag, did)
        self.fin_len = cat(self.fin_len, torch.full((Bn, C), s + 1))
        self.fin_parent = cat(self.fin_parent, beam)
        self.fin_token = cat(self.fin_token, tok)
        # the heuristic and the stop test
        L = self.max_new if (self.es == "never" and self.lp > 0.0) else s + 1
        best = self.run[:, :1] / (L ** self.lp)
        worst = torch.where(self.fin_flag, self.fin_score.min(dim=1, keepdim=True)[0], torch.full((), NEG))
        self.heur = self.heur & (best > worst).any(dim=1)
        go_on = bool(self.heur.any()) and not (bool(self.fin_flag.all()) and self.es is True) and not bool(hit.all())
        self.trace.append(dict(cand_score=score.clone(), cand_token=tok.clone(), cand_beam=beam.clone(), run=self.run.clone(),
                               fin_score=self.fin_score.clone(), fin_flag=self.fin_flag.clone(), fin_len=self.fin_len.clone(),
                               fin_parent=self.fin_parent.clone(), fin_token=self.fin_token.clone(), heur=self.heur.clone(),
                               next_token=self.next_token.clone(), src_row=self.src_row.clone(), go_on=go_on))
        self.steps = s + 1
        return go_on

    def hypotheses(self, R, pad):
        """(sequences (B * R, n_new) int64, scores (B * R,), beam_indices (B * R, n_new) int32): the first R finished entries of every sequence
        walked back through the parents, cropped to the longest, HF's layout."""
        Bn, n = self.B, self.n
        length = self.fin_len[:, :R].reshape(-1)
        n_new = int(length.max())
        seq = torch.full((Bn * R, n_new), pad, dtype=torch.int64)
        anc = torch.full((Bn * R, n_new), -1, dtype=torch.int64)
        for r in range(Bn * R):
            b, i = divmod(r, R)
            j, beam = int(length[r]) - 1, int(self.fin_parent[b, i])
            seq[r, j], anc[r, j] = self.fin_token[b, i], b * n + beam
            for j in range(j - 1, -1, -1):
                seq[r, j] = self.bp_token[j][b * n + beam]
                beam = int(self.bp_parent[j][b * n + beam])
                anc[r, j] = b * n + beam
        return seq, self.fin_score[:, :R].reshape(-1).clone(), anc.to(torch.int32)


def run_reference(sd, lc, x, am, pos, n, length_penalty, early_stopping, eos, max_new=N_NEW):
    """The rule driven by the oracle's uncached forward: every step recomputes each running beam's whole sequence.  Returns the BeamReference."""
    Bn, Tn, D = x.shape
    C = max(2, 1 + len(eos)) * n
    ref = BeamReference(Bn, n, C, eos, max_new, length_penalty, early_stopping)
    emb = sd["model.embed_tokens.weight"]
    with torch.no_grad():
        go_on = ref.step(O.llama_forward(sd, lc, x, am, pos)[1][:, -1])
        xs, ams, poss = (t.repeat_interleave(n, dim=0) for t in (x, am, pos))
        while go_on:
            src = ref.src_row
            xs = torch.cat([xs[src], emb[ref.next_token][:, None]], dim=1)
            ams = torch.cat([ams[src], torch.ones(Bn * n, 1, dtype=ams.dtype)], dim=1)
            poss = torch.cat([poss[src], poss[src][:, -1:] + 1], dim=1)
            go_on = ref.step(O.llama_forward(sd, lc, xs, ams, poss)[1][:, -1])
    return ref
