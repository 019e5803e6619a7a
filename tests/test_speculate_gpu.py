"""Draft-and-verify decoding on a real MI355X: setok_spec_accept and setok_ngram_propose bit for bit against the Python statement of their rules
(tests/spec_cases.py), and `SetokimLlamaPrefill.generate(draft=...)` against HuggingFace's greedy tokens (tests/golden/generate.npz), the plain
loop's eos / pad / sampled output, its own `return_past` contract, and the 16-bit yardstick of the decode path.  `pytest -m gpu`."""
import math
import os

import numpy as np
import pytest
import torch

import golden_io
import llama_bwd_cases as C
import parity
import setok_oracle as O
import spec_cases as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib, ops
    from setok_amd.generation import GenerationState, KVCache, LookupDrafter, Sampler
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
FP32_CASES = ("tiny_left", "gqa_tiny_left", "dh128", "mqa_dh128_left")


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _log(label, *nums):
    path = os.environ.get("SETOK_PARITY_LOG")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0]
        with open(path, "a") as f:
            f.write(f"{test}\t{label}\t" + "\t".join(f"{n:.3e}" for n in nums) + "\n")
    print(label, *[f"{n:.3e}" for n in nums])


# ---- setok_spec_accept -------------------------------------------------------------------------------------------------------------------------
def _accept_problem(B, K, seed, max_new=20, vocab=11):
    """Rows of every kind: no draft right, all right, a mixed prefix; -1 tails; eos ids that occur among the accepted drafts and as the bonus
    token; counts close to the budget (it cuts inside an accepted run); finished rows; a -1 among the selected tokens."""
    g = torch.Generator().manual_seed(seed)
    r = lambda hi, *shape: torch.randint(0, hi, shape, generator=g)
    sel = r(vocab, B, K + 1)
    draft = sel[:, :K].clone()
    for b in range(B):
        kind = (b + seed) % 4
        n = (0, K, int(r(K + 1, 1)), int(r(K + 1, 1)))[kind]
        if n < K:
            draft[b, n] = (draft[b, n] + 1 + int(r(vocab - 1, 1))) % vocab          # the first wrong proposal; behind it some are right again
        if K and kind == 3:
            draft[b, int(r(K, 1)):] = -1                                           # a -1 tail (it may cut the right prefix short)
        if K and b % 7 == 5:
            draft[b, int(r(K, 1))] = -1                                            # ... and a -1 with non-negative proposals behind it
    sel[r(B, max(B // 5, 1)), r(K + 1, max(B // 5, 1))] = -1                         # undrawable rows
    count = r(max_new, B).to(torch.int32)
    count[r(B, max(B // 3, 1))] = max_new - 1 - int(r(2, 1))                          # one or two tokens of budget left
    finished = (r(4, B) == 0).to(torch.uint8)
    if B == 1:
        finished[:] = seed % 5 == 4
    cap, len0 = 40 + K + seed % 3, 17 + seed % 5
    return dict(draft=draft, sel=sel, eos=torch.tensor([3, 7]) if seed % 3 else None, seq=torch.full((B, max_new), -7),
                count=count, finished=finished, pending=torch.full((B,), -3), key_mask=torch.full((B, cap), 9, dtype=torch.uint8),
                next_pos=r(50, B) + 30, len0=len0)


def _accept_both(p):
    want = S.accept_rule(p["draft"], p["sel"], p["eos"], p["seq"], p["count"], p["finished"], p["pending"], p["key_mask"], p["next_pos"], p["len0"])
    d = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in p.items()}
    emitted, m, summary = ops.spec_accept(d["draft"], d["sel"], d["eos"], d["seq"], d["count"], d["finished"], d["pending"], d["key_mask"],
                                          d["next_pos"], d["len0"])
    got = (d["seq"], d["count"], d["finished"], d["pending"], d["key_mask"], d["next_pos"], emitted, m, summary)
    return want, [t.cpu() for t in got]


_ACCEPT_NAMES = ("seq", "count", "finished", "pending", "key_mask", "next_pos", "emitted", "m", "summary")


@pytest.mark.parametrize("B", [1, 3, 300])
@pytest.mark.parametrize("K", [0, 1, 7, 63])
def test_spec_accept_equals_the_rule_on_every_buffer(B, K):
    """torch.equal on the WHOLE of every buffer: the sentinel bytes around the written slots (seq -7, key_mask 9, pending -3) must survive."""
    seen = set()
    for seed in range(6 if B > 1 else 12):
        p = _accept_problem(B, K, seed)
        want, got = _accept_both(p)
        for name, w, g in zip(_ACCEPT_NAMES, want, got):
            assert w.dtype == g.dtype and torch.equal(w, g), (seed, name)
        m = want[7]
        seen |= {("m", int(v)) for v in m} | {("bad", int(want[8][2]))}
        assert (got[4][:, :p["len0"]] == 9).all() and (got[4][:, p["len0"] + K + 1:] == 9).all()
    if B == 300:
        assert {("m", v) for v in range(min(K, 5) + 2)} <= seen and ("bad", 1) in seen          # finished rows, every short run, a -1 emitted


def test_spec_accept_on_the_hand_made_rows():
    """tests/test_speculate_cpu.py's rows: all right with an eos as the bonus token, wrong at 1, cut at 1, the budget inside an accepted run, a
    finished row, wrong at 0 — and an eos among the accepted drafts."""
    K, max_new, len0, cap = 3, 10, 4, 12
    draft = torch.tensor([[5, 6, 7], [5, 9, 7], [5, -1, 7], [5, 6, 7], [5, 6, 7], [5, 6, 7], [9, 9, 9]])
    B = draft.shape[0]
    for eos, m_want, fin_want in (([8], [4, 2, 2, 4, 2, 0, 1], [1, 0, 0, 1, 1, 1, 0]),            # the bonus token ends rows 0 and 3
                                  ([6, 50], [2, 2, 2, 2, 2, 0, 1], [1, 1, 1, 1, 1, 1, 0])):       # an accepted draft (or, rows 1 and 2, the bonus) does
        p = dict(draft=draft, sel=torch.tensor([[5, 6, 7, 8]] * B), eos=torch.tensor(eos), seq=torch.full((B, max_new), -7),
                 count=torch.tensor([0, 0, 0, 0, 8, 3, 0], dtype=torch.int32), finished=torch.tensor([0, 0, 0, 0, 0, 1, 0], dtype=torch.uint8),
                 pending=torch.full((B,), -3), key_mask=torch.ones(B, cap, dtype=torch.uint8), next_pos=torch.full((B,), 20), len0=len0)
        want, got = _accept_both(p)
        assert got[7].tolist() == m_want and got[2].tolist() == fin_want
        for name, w, g in zip(_ACCEPT_NAMES, want, got):
            assert torch.equal(w, g), name


# ---- setok_ngram_propose -----------------------------------------------------------------------------------------------------------------------
def _ngram_both(hist, hist_len, emitted, m, K, max_ngram=3, min_ngram=1):
    want = S.ngram_rule(hist, hist_len, emitted, m, K, max_ngram, min_ngram)
    h, hl = hist.to(DEV), hist_len.to(DEV)
    e, mm = (None, None) if emitted is None else (emitted.to(DEV), m.to(DEV))
    len_max = int(hist_len.max()) + (0 if emitted is None else emitted.shape[1])
    out = ops.ngram_propose(h, hl, K, min(len_max, hist.shape[1]), e, mm, max_ngram, min_ngram)
    h2, hl2 = hist.to(DEV), hist_len.to(DEV)
    again = ops.ngram_propose(h2, hl2, K, min(len_max, hist.shape[1]), e, mm, max_ngram, min_ngram)
    assert torch.equal(out, again) and torch.equal(h, h2) and torch.equal(hl, hl2)          # bit-equal repeats
    for name, w, g in zip(("hist", "hist_len", "out"), want, (h.cpu(), hl.cpu(), out.cpu())):
        assert w.dtype == g.dtype and torch.equal(w, g), name
    return want[2]


@pytest.mark.parametrize("B", [1, 3, 33])
@pytest.mark.parametrize("L", [0, 1, 2, 3, 255, 256, 257, 4100])
def test_ngram_propose_equals_the_rule(B, L):
    """Random histories over a small vocabulary (matches at every n, several per row) with negative ids sprinkled in, appended to by m in
    {0, 1, K + 1}; the bytes of `hist` behind the new length must survive."""
    K = 7
    for seed, vocab in ((0, 3), (1, 9), (2, 400)):
        g = torch.Generator().manual_seed(1000 * L + 10 * B + seed)
        hist = torch.full((B, L + K + 4), -5, dtype=torch.int64)
        hist[:, :L] = torch.randint(0, vocab, (B, L), generator=g)
        if L:
            hist[:, :L][torch.rand(B, L, generator=g) < 0.02] = -200                    # image placeholders: they match nothing
        hist_len = torch.full((B,), L, dtype=torch.int32)
        if B > 1 and L > 3:
            hist_len[1] = L - 3                                                        # a shorter row: what lies behind its length is not history
        emitted = torch.randint(0, vocab, (B, K + 1), generator=g)
        if seed == 1 and B > 1:
            emitted[0, 0] = -1                                                         # a negative id in the suffix
        for m in (0, 1, K + 1):
            _ngram_both(hist, hist_len, emitted, torch.full((B,), m, dtype=torch.int32), K)
        _ngram_both(hist, hist_len, emitted, torch.randint(0, K + 2, (B,), generator=g).to(torch.int32), K, max_ngram=5, min_ngram=2)
        _ngram_both(hist, hist_len, None, None, 63)                                    # propose only, the widest proposal


def test_ngram_propose_on_constructed_histories():
    def run(row, K=4, **kw):
        hist = torch.full((1, len(row) + 2), -5, dtype=torch.int64)
        hist[0, :len(row)] = torch.tensor(row)
        return _ngram_both(hist, torch.tensor([len(row)], dtype=torch.int32), None, None, K, **kw)[0].tolist()

    assert run([1, 2, 3, 9, 1, 2, 3, 4, 1, 2, 3]) == [4, 1, 2, 3]                         # several matches: the latest wins
    assert run([1, 2, 3, 7, 5, 3, 8, 6, 1, 2, 3]) == [7, 5, 3, 8]                         # "1 2 3" at 0 beats the more recent "3" at 5
    assert run([1, 2, 3, 7, 5, 3, 8, 6, 1, 2, 3], max_ngram=1) == [8, 6, 1, 2]            # ... which wins when only 1-grams are tried
    assert run([7, 7, 7, 7]) == [7, -1, -1, -1]                                           # the match overlaps the suffix; the continuation is shorter than K
    assert run([4, 5, 6, 4, 5]) == [6, 4, 5, -1]
    assert run([1, 2, -200, 1, 2]) == [-200, 1, 2, -1]                                    # a negative id inside a continuation is copied
    assert run([1, -200, 2, 1, -200]) == [-1] * 4                                         # a negative last entry: no n-gram may be used
    assert run([3, -200, 2, 9, -200, 2]) == [9, -200, 2, -1]                              # n = 2 and 3 hold the negative id: the 1-gram "2" is used
    assert run([1, 2, 3, 4]) == [-1] * 4 and run([]) == [-1] * 4 and run([5]) == [-1] * 4
    assert run([1, 2, 1, 2], min_ngram=3) == [-1] * 4                                     # L <= n for n = 3 ... no shorter one allowed


def test_lookup_drafter_keeps_the_attended_prompt_and_launches_once_per_round(monkeypatch):
    ids = torch.tensor([[0, 0, 5, -200, 6, 5], [1, 2, 3, 1, 2, 3]])
    am = torch.tensor([[0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1]])
    d = LookupDrafter(3)
    d.begin(2, DEV, ids, am, 4)
    assert d.hist.shape == (2, 6 + 4 + 3 + 1) and d.hist_len.tolist() == [4, 6] and d.hist[0, :4].tolist() == [5, -200, 6, 5]
    names, real = [], _lib.call
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "call", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
        d.update(torch.tensor([[6, -1]], device=DEV).expand(2, 2).contiguous(), torch.tensor([1, 0], dtype=torch.int32, device=DEV))
        out = d.propose(torch.zeros(2, dtype=torch.int64, device=DEV))
    assert names == ["setok_ngram_propose"]                                               # update + propose: one launch
    assert out.tolist() == [[5, 6, -1], [1, 2, 3]] and d.hist_len.tolist() == [5, 6]      # "6" -> after the earlier 6; "1 2 3" -> what followed it
    e = LookupDrafter(2)
    e.begin(3, DEV, None, None, 5)                                                        # inputs_embeds alone: an empty history
    assert e.hist_len.tolist() == [0, 0, 0] and e.propose(None).tolist() == [[-1, -1]] * 3
    f = LookupDrafter(2)
    f.begin(3, DEV, None, None)                                                           # no budget given: the history is regrown when it fills up
    cap0 = f.hist.shape[1]
    for _ in range(cap0 // 3 + 1):
        f.update(torch.full((3, 3), 4, device=DEV), torch.full((3,), 3, dtype=torch.int32, device=DEV))
    assert f.propose(None).tolist() == [[4, -1]] * 3 and f.hist_len.tolist() == [3 * (cap0 // 3 + 1)] * 3 and f.hist.shape[1] > cap0


# ---- the loop against HuggingFace's tokens ---------------------------------------------------------------------------------------------------------
_MODELS = {}


def _model(name, dt=torch.float32):
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
    key = (name, dt)
    if key not in _MODELS:
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
        _MODELS[key] = m.to(device=DEV, dtype=dt).eval()
    return _MODELS[key], x.to(DEV), am.to(DEV), pos.to(DEV)


_GOLDEN = {}


def _golden(golden_dir, name):
    if name not in _GOLDEN:                                                               # read once, shared, never written to
        z = golden_io.load(os.path.join(golden_dir, "generate.npz"))
        _GOLDEN[name] = {k.split(":", 1)[1]: _t(z[k]) for k in z.files if k.startswith(name + ":")}
    return _GOLDEN[name]


def _vocab(m):
    return m.lm_head.weight.shape[0]


class _Calls:
    """The names `_lib.call` is given while the block runs."""

    def __init__(self, monkeypatch):
        self.mp, self.names = monkeypatch, []

    def __enter__(self):
        real = _lib.call
        self.ctx = self.mp.context()
        mp = self.ctx.__enter__()
        mp.setattr(_lib, "call", lambda name, *a, **k: (self.names.append(name), real(name, *a, **k))[1])
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)

    def rounds(self, m):
        return self.names.count("setok_attention_extend_gqa") // len(m.model.layers)


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("name", FP32_CASES)
def test_fp32_speculative_tokens_are_hfs(golden_dir, monkeypatch, name, K):
    """Whatever the drafter proposes, the tokens are HuggingFace's greedy ones (top-2 margins >= 1e-3 in the fixture), the returned logits and hidden
    states are within 1e-4 of the golden teacher-forced ones, and a round is one `extend`."""
    m, x, am, pos = _model(name)
    g = _golden(golden_dir, name)
    n, B = g["tokens"].shape
    truth = g["tokens"].t().contiguous()
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, return_dict_in_generate=True, output_hidden_states=True,
              output_logits=True)
    for pattern in S.PATTERNS + ("lookup",):
        draft = LookupDrafter(K) if pattern == "lookup" else S.ScriptedDrafter(truth, K, pattern, _vocab(m))
        with _Calls(monkeypatch) as calls:
            out = m.generate(draft=draft, **kw)
        assert out.sequences.dtype == torch.int64 and torch.equal(out.sequences.cpu(), truth), pattern
        parity.close(out.logits.transpose(0, 1), g["logits"], 1e-4, f"{name} K={K} {pattern} logits")
        parity.close(out.hidden_states.transpose(0, 1), g["hidden"], 1e-4, f"{name} K={K} {pattern} hidden")
        assert calls.names.count("setok_spec_accept") == calls.rounds(m) + 1 and "setok_attention_decode_gqa" not in calls.names
        if pattern == "right":
            assert calls.rounds(m) == math.ceil((n - 1) / (K + 1))
        if pattern == "wrong":
            assert calls.rounds(m) == n - 1
        assert torch.equal(m.generate(draft=draft, **dict(kw, return_dict_in_generate=False)), out.sequences)      # a drafter serves call after call


# ---- loop behaviour ------------------------------------------------------------------------------------------------------------------------------
def test_eos_and_pad_equal_the_plain_loops(golden_dir):
    name, K = "tiny_left", 3
    m, x, am, pos = _model(name)
    tokens = _golden(golden_dir, name)["tokens"]
    n, B = tokens.shape
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, pad_token_id=99)
    right = S.ScriptedDrafter(tokens.t().contiguous(), K, "right", _vocab(m))             # round 1 emits steps 1 .. 4: 1 .. 3 accepted drafts, 4 the bonus
    for step in (2, 4, 0):                                                                # an accepted draft, the bonus token, the very first token
        b = next(b for b in range(B) if int(tokens[step, b]) not in tokens[:step, b].tolist())
        eos = int(tokens[step, b])
        plain = m.generate(eos_token_id=eos, **kw)
        assert plain.shape[1] > step + 1 and plain[b, step + 1:].tolist() == [99] * (plain.shape[1] - step - 1)
        for pattern in ("right", "cycle", "first_right"):
            got = m.generate(eos_token_id=eos, draft=S.ScriptedDrafter(tokens.t().contiguous(), K, pattern, _vocab(m)), **kw)
            assert torch.equal(got, plain), (step, pattern)
        assert torch.equal(m.generate(eos_token_id=eos, draft=LookupDrafter(K), **kw), plain)
    every = sorted({int(t) for t in tokens[2]})                                           # every sequence has finished by step 2: the loop ends there
    plain = m.generate(eos_token_id=every, **dict(kw, pad_token_id=None))
    assert plain.shape[1] <= 3 and torch.equal(m.generate(eos_token_id=every, draft=right, **dict(kw, pad_token_id=None)), plain)
    for n1 in (1, 2, 5):                                                                  # the budget cuts the first round
        assert torch.equal(m.generate(draft=right, **dict(kw, max_new_tokens=n1)).cpu(), tokens[:n1].t())


def test_sampled_with_given_uniforms_equals_the_plain_sampled_loop():
    name, n = "tiny_left", 16
    m, x, am, pos = _model(name)
    B = x.shape[0]
    u = torch.rand(n, B, generator=torch.Generator().manual_seed(5))
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n)
    mk = lambda **k: Sampler(temperature=0.7, top_k=8, top_p=0.95, **k)
    plain = m.generate(sampler=mk(u=u), **kw)
    greedy = m.generate(**kw)
    assert not torch.equal(plain, greedy)                                                 # the uniforms matter
    for K, pattern in ((3, "cycle"), (7, "right"), (1, "wrong"), (3, "cut")):
        got = m.generate(sampler=mk(u=u), draft=S.ScriptedDrafter(plain.cpu(), K, pattern, _vocab(m)), **kw)
        assert torch.equal(got, plain), (K, pattern)
    assert torch.equal(m.generate(sampler=mk(u=u), draft=LookupDrafter(3), **kw), plain)
    eos = int(plain[1, 3])
    assert torch.equal(m.generate(sampler=mk(u=u), draft=S.ScriptedDrafter(plain.cpu(), 3, "cycle", _vocab(m)), eos_token_id=eos, **kw),
                       m.generate(sampler=mk(u=u), eos_token_id=eos, **kw))
    a = m.generate(sampler=mk(generator=torch.Generator(device=DEV).manual_seed(3)), draft=LookupDrafter(3), **kw)
    b = m.generate(sampler=mk(generator=torch.Generator(device=DEV).manual_seed(3)), draft=LookupDrafter(3), **kw)
    assert torch.equal(a, b) and a.shape == (B, n)                                        # one torch.rand(max_new_tokens, B) per call
    with pytest.raises(ValueError, match="u has shape"):
        m.generate(sampler=mk(u=u[:5]), draft=LookupDrafter(3), **kw)
    nan = SetokimLlamaPrefill(C.LLAMA_CASES[name][0]).to(DEV).eval()
    nan.load_state_dict(m.state_dict())
    with torch.no_grad():
        nan.lm_head.weight[7] = float("nan")
    with pytest.raises(RuntimeError, match="no token can be drawn"):
        nan.generate(sampler=mk(u=u), draft=LookupDrafter(3), **kw)


def test_no_draft_is_the_call_without_the_keyword(monkeypatch):
    m, x, am, pos = _model("tiny_left")
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=6, return_dict_in_generate=True, output_logits=True)
    with _Calls(monkeypatch) as a:
        without = m.generate(**kw)
    with _Calls(monkeypatch) as b:
        none = m.generate(draft=None, **kw)
    assert torch.equal(without.sequences, none.sequences) and torch.equal(without.logits, none.logits)
    assert a.names == b.names and "setok_spec_accept" not in a.names and "setok_attention_extend_gqa" not in a.names
    assert a.names.count("setok_attention_decode_gqa") == 5 * len(m.model.layers)


def test_the_cache_is_regrown_when_the_holes_use_it_up(golden_dir, monkeypatch):
    """B = 3, K = 7, sequence 0 always right and the others always wrong: every round of sequence 0 costs the others 7 masked slots."""
    name, K = "tiny_left", 7
    m, x, am, pos = _model(name)
    tokens = _golden(golden_dir, name)["tokens"]
    n, B = tokens.shape
    grown, real = [], KVCache.grown
    monkeypatch.setattr(KVCache, "grown", lambda self, cap: (grown.append((self.cap, cap)), real(self, cap))[1])
    out = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, return_dict_in_generate=True, return_past=True,
                     draft=S.ScriptedDrafter(tokens.t().contiguous(), K, "first_right", _vocab(m)))
    T = x.shape[1]
    assert grown == [(T + n + K, 2 * (T + n + K))] and out.past.cache.cap == 2 * (T + n + K)
    assert torch.equal(out.sequences.cpu(), tokens.t())
    c = out.past.cache
    assert c.len > T + n - 1 and not c.key_mask[:, c.len:].any()                          # holes below len, nothing attended behind it
    assert c.key_mask[:, T:c.len].sum(1).tolist() == [n - 1] * B                          # every sequence consumed its n - 1 fed tokens, wherever they lie
    assert torch.equal(c.next_pos.cpu(), am.sum(1).cpu() + n - 1) and torch.equal(out.past.pending.cpu(), tokens[-1])


def _pick_eos(tokens, n1):
    B = tokens.shape[1]
    for eos in sorted({int(t) for t in tokens[3]}):
        first = [next((j for j in range(n1) if int(tokens[j, b]) == eos), n1) for b in range(B)]
        if 3 in first and n1 in first:
            return eos, first
    raise AssertionError("no eos id of the goldens finishes one sequence at step 3 and leaves another running")


@pytest.mark.parametrize("name", ["tiny_left", "gqa_dh128"])
def test_a_second_turn_from_a_speculative_state_equals_one_from_a_plain_state(golden_dir, name):
    m, x, am, _ = _model(name)
    tokens = _golden(golden_dir, name)["tokens"]
    B, T, D = x.shape
    n1, n2, L2, K = 8, 6, 6, 3
    eos, first = _pick_eos(tokens, n1)
    turn1 = dict(inputs_embeds=x, attention_mask=am, max_new_tokens=n1, eos_token_id=eos, pad_token_id=99, return_dict_in_generate=True, return_past=True)
    plain1 = m.generate(**turn1)
    spec1 = m.generate(draft=S.ScriptedDrafter(tokens.t().contiguous(), K, "cycle", _vocab(m)), **turn1)
    assert torch.equal(spec1.sequences, plain1.sequences) and isinstance(spec1.past, GenerationState)
    seq1 = spec1.sequences.cpu()
    real = [min(f + 1, seq1.shape[1]) for f in first]
    # the state as GenerationState defines it: consumed = prompt + the real tokens except the last, which is pending (an eos included)
    assert spec1.past.pending.cpu().tolist() == [int(seq1[b, real[b] - 1]) for b in range(B)]
    c = spec1.past.cache
    assert c.key_mask[:, :c.len].sum(1).cpu().tolist() == [int(am[b].sum()) + real[b] - 1 for b in range(B)]
    assert c.next_pos.cpu().tolist() == [int(am[b].sum()) + real[b] - 1 for b in range(B)] and not c.key_mask[:, c.len:].any()
    am2 = torch.ones(B, L2, dtype=torch.long, device=DEV)
    am2[B - 1, L2 - 2:] = 0
    kw2 = dict(attention_mask=am2, max_new_tokens=n2, return_dict_in_generate=True, output_logits=True)
    for seed in range(40, 60):
        turn = torch.randn(B, L2, D, generator=torch.Generator().manual_seed(seed)).to(DEV)
        plain2 = m.generate(past=m.generate(**turn1).past, inputs_embeds=turn, **kw2)
        top2 = plain2.logits.float().topk(2, dim=-1).values
        if float(((top2[..., 0] - top2[..., 1]) / plain2.logits.float().abs().amax(dim=-1)).min()) >= 5e-4:
            break                                                                          # token equality is only meaningful above the logit bound
    else:
        raise AssertionError("no seeded turn with a top-1 / top-2 margin >= 5e-4 at every step")
    spec2 = m.generate(past=spec1.past, inputs_embeds=turn, **kw2)                          # a plain turn from the speculative state
    assert torch.equal(spec2.sequences, plain2.sequences)
    parity.close(spec2.logits, plain2.logits, 1e-4, f"{name} turn 2 from a speculative state, logits")
    again = m.generate(draft=S.ScriptedDrafter(tokens.t().contiguous(), K, "cycle", _vocab(m)), **turn1).past
    both = m.generate(past=again, inputs_embeds=turn, draft=S.ScriptedDrafter(plain2.sequences.cpu(), K, "cycle", _vocab(m)), **kw2)
    assert torch.equal(both.sequences, plain2.sequences)                                   # ... and a speculative turn from it
    parity.close(both.logits, plain2.logits, 1e-4, f"{name} speculative turn 2 from a speculative state, logits")


def test_fp8_weights_with_a_draft_equal_their_own_plain_loop():
    name, n = "dh128_left", 12
    kw, lc, seed, x, am, pos, _, _ = C.case_inputs(name)
    m = SetokimLlamaPrefill(kw)
    m.load_state_dict(O.init_llama_weights(lc, seed=seed), strict=True)
    m = m.to(DEV).eval().quantize_fp8_()
    g = dict(inputs_embeds=x.to(DEV), attention_mask=am.to(DEV), position_ids=pos.to(DEV), max_new_tokens=n)
    plain = m.generate(**g)
    for K, pattern in ((3, "cycle"), (7, "right"), (3, "wrong")):
        assert torch.equal(m.generate(draft=S.ScriptedDrafter(plain.cpu(), K, pattern, kw["vocab_size"]), **g), plain), (K, pattern)
    assert torch.equal(m.generate(draft=LookupDrafter(3), **g), plain)


def test_a_sequence_alone_equals_the_same_sequence_in_its_batch(golden_dir):
    name, K = "gqa_tiny_left", 3
    m, x, am, pos = _model(name)
    tokens = _golden(golden_dir, name)["tokens"]
    n, B = tokens.shape
    truth = tokens.t().contiguous()
    kw = dict(max_new_tokens=n, return_dict_in_generate=True, output_logits=True)
    full = m.generate(inputs_embeds=x, attention_mask=am, position_ids=pos, draft=S.ScriptedDrafter(truth, K, "cycle", _vocab(m)), **kw)
    for b in range(B):                                                                    # B = 1: no hole ever forms, the cache never grows
        one = m.generate(inputs_embeds=x[b:b + 1], attention_mask=am[b:b + 1], position_ids=pos[b:b + 1], return_past=True,
                         draft=S.ScriptedDrafter(truth[b:b + 1], K, "cycle", _vocab(m)), **kw)
        assert torch.equal(one.sequences[0], full.sequences[b]) and torch.equal(one.sequences[0].cpu(), truth[b])
        parity.close(one.logits[0], full.logits[b], 1e-4, f"{name} sequence {b} alone against its batch, logits")
        c = one.past.cache
        assert c.len == x.shape[1] + n - 1 and c.cap == x.shape[1] + n + K and bool(c.key_mask[0, x.shape[1]:c.len].all())


# ---- 16 bits ---------------------------------------------------------------------------------------------------------------------------------------
def _teacher_forced(m, x, am, pos, tokens):
    """Prefill + decode_step feeding `tokens` (n, B): the plain decode path's logits (n, B, V) under those tokens."""
    n, B = tokens.shape
    T = x.shape[1]
    cache = KVCache.for_model(m.model, B, T + n)
    hidden = m.model.prefill(x.to(m.model.norm.weight.dtype), am, pos, cache)
    last = (am.bool() * torch.arange(T, device=x.device)[None]).max(dim=1).values
    h = hidden[torch.arange(B, device=x.device), last].contiguous()
    w_lm, w_e = m.lm_head.weight.detach().contiguous(), m.model.embed_tokens.weight.detach()
    lgs = []
    for j in range(n):
        lgs.append(ops.linear(h, w_lm))
        if j + 1 < n:
            h = m.model.decode_step(w_e[tokens[j].to(x.device)], cache)
    return torch.stack(lgs)


@pytest.mark.parametrize("dt,tag", [(torch.bfloat16, "bf16"), (torch.float16, "fp16")])
@pytest.mark.parametrize("name", ["dh128", "gqa_dh128"])
def test_16bit_speculative_logits_drift_no_more_than_the_decode_paths(name, dt, tag):
    """The run's tokens are the lowest argmax of its own returned logits; and under those tokens the returned logits are at most 1.5 x as far from
    the fp32 model's teacher-forced logits as the plain 16-bit decode path's are, in max-rel and in rms-rel (the factor of the project's other
    16-bit tests)."""
    m, x, am, pos = _model(name, dt)
    m32 = _model(name)[0]
    n, K = 16, 3
    kw = dict(inputs_embeds=x, attention_mask=am, position_ids=pos, max_new_tokens=n, return_dict_in_generate=True, output_logits=True)
    plain = m.generate(**kw)
    for pattern in ("cycle", "right"):
        out = m.generate(draft=S.ScriptedDrafter(plain.sequences.cpu(), K, pattern, _vocab(m)), **kw)
        own = out.logits
        V = own.shape[-1]
        lowest = torch.where(own == own.max(dim=-1, keepdim=True).values, torch.arange(V, device=own.device), V).min(dim=-1).values
        assert torch.equal(out.sequences, lowest)
        toks = out.sequences.t().contiguous()
        ref = _teacher_forced(m32, x, am, pos, toks)
        spec, dec = parity.measure(own.transpose(0, 1).float(), ref), parity.measure(_teacher_forced(m, x, am, pos, toks).float(), ref)
        _log(f"{name} {tag} K={K} {pattern} logits under the run's tokens: speculative max-rel, decode max-rel, ratio, speculative rms-rel, "
             "decode rms-rel, ratio", spec[0], dec[0], spec[0] / dec[0], spec[1], dec[1], spec[1] / dec[1])
        assert spec[0] <= 1.5 * dec[0] and spec[1] <= 1.5 * dec[1], (spec, dec)
