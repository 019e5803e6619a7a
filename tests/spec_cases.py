"""Draft-and-verify decoding: the Python statement of the two rules of include/setok_hip.h, "Speculative decoding" (what `setok_spec_accept` and
`setok_ngram_propose` are held to, bit for bit), and the scripted drafter the loop tests drive `generate(draft=...)` with."""
import torch

from setok_amd.generation import Drafter

PATTERNS = ("right", "wrong", "first_right", "cycle", "cut")


def accept_rule(draft, sel, eos, seq, count, finished, pending, key_mask, next_pos, len0):
    """The accept rule on CPU tensors.  Returns the new (seq, count, finished, pending, key_mask, next_pos, emitted, m, summary); the inputs are
    left alone."""
    seq, count, finished, pending = seq.clone(), count.clone(), finished.clone(), pending.clone()
    key_mask, next_pos = key_mask.clone(), next_pos.clone()
    B, K = sel.shape[0], sel.shape[1] - 1
    max_new = seq.shape[1]
    eos = set() if eos is None else {int(t) for t in eos}
    emitted = torch.full((B, K + 1), -1, dtype=torch.int64)
    m_out = torch.zeros(B, dtype=torch.int32)
    live = bad = 0
    for b in range(B):
        c, m = int(count[b]), 0
        if int(finished[b]) == 0 and 0 <= c < max_new:
            d, e = draft[b].tolist(), sel[b].tolist()
            nd = 0
            while nd < K and d[nd] >= 0:
                nd += 1
            n = 0
            while n < nd and d[n] == e[n]:
                n += 1
            m = min(n + 1, max_new - c)
            done = False
            for i in range(m):
                if e[i] in eos:
                    m, done = i + 1, True
                    break
            done = done or c + m == max_new
            for i in range(m):
                seq[b, c + i] = e[i]
                emitted[b, i] = e[i]
                bad |= int(e[i] < 0)
            count[b] = c + m
            pending[b] = e[m - 1]
            next_pos[b] = int(next_pos[b]) - (1 + nd) + m
            if done:
                finished[b] = 1
            else:
                live += 1
        for i in range(K + 1):
            key_mask[b, len0 + i] = 1 if i < m else 0
        m_out[b] = m
    summary = torch.tensor([int(m_out.max()) if B else 0, live, bad], dtype=torch.int32)
    return seq, count, finished, pending, key_mask, next_pos, emitted, m_out, summary


def ngram_rule(hist, hist_len, emitted, m, K, max_ngram=3, min_ngram=1):
    """The lookup rule on CPU tensors: (hist, hist_len) after the append and the proposals (B, K)."""
    hist, hist_len = hist.clone(), hist_len.clone()
    B = hist.shape[0]
    out = torch.full((B, K), -1, dtype=torch.int64)
    for b in range(B):
        L = int(hist_len[b])
        if emitted is not None:
            mb = min(max(int(m[b]), 0), emitted.shape[1])
            hist[b, L:L + mb] = emitted[b, :mb]
            L += mb
            hist_len[b] = L
        h = hist[b, :L]
        for n in range(max_ngram, min_ngram - 1, -1):
            if L <= n or bool((h[L - n:] < 0).any()):
                continue
            hit = (h.unfold(0, n, 1)[:L - n] == h[L - n:]).all(dim=1).nonzero()          # window j is h[j .. j + n), j <= L - n - 1
            if hit.numel() == 0:
                continue
            j = int(hit.max())
            for i in range(K):
                if j + n + i < L:
                    out[b, i] = h[j + n + i]
            break
    return hist, hist_len, out


def pattern_lengths(pattern, r, B, K):
    """Round r of a scripted pattern: (good (B,), cut (B,)) — proposals at positions >= good[b] are corrupted, those at positions >= cut[b] are -1."""
    b = torch.arange(B)
    full = torch.full((B,), K)
    if pattern == "right":
        return full, full
    if pattern == "wrong":
        return torch.zeros(B, dtype=torch.int64), full
    if pattern == "first_right":                                       # sequence 0 accepts everything, the others nothing: the most holes
        return torch.where(b == 0, full, torch.zeros_like(full)), full
    if pattern == "cycle":                                             # a correct prefix of every length 0 .. K
        return (r + b) % (K + 1), full
    if pattern == "cut":                                               # correct proposals cut short by -1
        return full, (r + b) % (K + 1)
    raise KeyError(pattern)


def script(truth_row, c, good, cut, K, vocab):
    """The K proposals for a sequence that has emitted c tokens of `truth_row` (a list): the known continuation, corrupted from `good` on and cut
    to -1 from `cut` on (and behind the end of what is known)."""
    out = []
    for i in range(K):
        t = truth_row[c + i] if c + i < len(truth_row) else -1
        if t >= 0 and i >= good:
            t = (t + 1) % vocab
        out.append(-1 if i >= cut else t)
    return out


class ScriptedDrafter(Drafter):
    """Proposes the known continuation `truth` (B, n) of a run, spoiled by `pattern`; everything stays on the device (no read per round)."""

    def __init__(self, truth, K, pattern, vocab):
        self.truth, self.K, self.pattern, self.vocab = truth, K, pattern, vocab
        self.rounds = 0

    def begin(self, B, device, prompt_ids, prompt_mask, max_new_tokens=None):
        self.t = self.truth.to(device=device, dtype=torch.int64)
        self.count = torch.zeros(B, dtype=torch.int64, device=device)
        self.rounds = 0

    def update(self, emitted, m):
        self.count += m.long()

    def propose(self, pending):
        B, n = self.t.shape
        dev = self.t.device
        good, cut = (x.to(dev) for x in pattern_lengths(self.pattern, self.rounds, B, self.K))
        self.rounds += 1
        i = torch.arange(self.K, device=dev)[None]
        idx = self.count[:, None] + i
        tok = torch.where(idx < n, self.t.gather(1, idx.clamp_max(n - 1)), torch.full_like(idx, -1))
        tok = torch.where((tok >= 0) & (i >= good[:, None]), (tok + 1) % self.vocab, tok)
        return torch.where(i >= cut[:, None], torch.full_like(tok, -1), tok)


def toy_token(prefix, vocab):
    """A deterministic "model": the next token as a function of the whole prefix."""
    h = 1469598103
    for t in prefix:
        h = (h * 1099511 + int(t) + 7) % 2147483647
    return h % vocab


def toy_plain(prompt, max_new, vocab, eos):
    out = []
    while len(out) < max_new:
        out.append(toy_token(prompt + out, vocab))
        if out[-1] in eos:
            break
    return out
