"""Draft-and-verify decoding, without a GPU: setok_spec_accept and setok_ngram_propose are declared, exported by both builds and mirrored by the
ctypes table; they refuse bad arguments on the host before any launch; generate() refuses a bad `draft`, a bad K and the fp8 cache before any
device call; KVCache.truncate keeps its bounds; and the loop invariant itself — with a toy "model" that is a deterministic function of the prefix,
the Python statement of the rules (tests/spec_cases.py) reproduces the plain sequence for every draft pattern, under eos and under the budget."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

import spec_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"setok_spec_accept": 19, "setok_ngram_propose": 13}


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_the_entries_are_declared_exported_and_in_the_ctypes_table(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "setok_hip.h")).read(), flags=re.S)
    decls = {n: [a for a in args.split(",") if a.strip()] for n, args in re.findall(r"\bint\s+(setok_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)}
    for name, arity in ENTRIES.items():
        assert name in decls and len(decls[name]) == arity
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == arity
        for path in (lib.LIB_PATH, lib.LIB_PATH_F16):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additive: the ABI version stays
    assert "speculate.hip" in open(os.path.join(ROOT, "setok_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("half", [False, True])
def test_spec_accept_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    P = 64                                                            # a non-null "pointer": validation fails before anything is dereferenced

    def args(draft=P, sel=P, B=2, K=3, eos=P, n_eos=1, max_new=8, seq=P, count=P, finished=P, pending=P, key_mask=P, next_pos=P, cap=32, len0=10,
             emitted=P, m_out=P, summary=P):
        return (None, draft, sel, B, K, eos, n_eos, max_new, seq, count, finished, pending, key_mask, next_pos, cap, len0, emitted, m_out, summary)

    bad = [(dict([(k, None)]), b"null operand") for k in ("draft", "sel", "eos", "seq", "count", "finished", "pending", "key_mask", "next_pos",
                                                            "emitted", "m_out", "summary")]
    bad += [(dict(B=-1), b"bad B"), (dict(K=-1), b"bad K"), (dict(K=64, cap=200), b"bad K"), (dict(max_new=0), b"bad max_new"),
            (dict(n_eos=-1), b"bad n_eos"), (dict(len0=29), b"exceed the cache"),                     # 29 + 3 + 1 > 32
            (dict(len0=32, K=0), b"exceed the cache"), (dict(len0=-1), b"exceed the cache"),
            (dict(B=0, K=64, cap=200), b"bad K")]                                                     # ... also with nothing to do
    for kw, msg in bad:
        rc = l.setok_spec_accept(*args(**kw))
        assert rc == -1 and msg in l.setok_last_error(), (kw, l.setok_last_error())
    assert l.setok_spec_accept(*args(B=0)) == 0                       # nothing to do is not an error (and launches nothing)
    assert l.setok_spec_accept(*args(B=0, K=0, draft=None, eos=None, n_eos=0, len0=31)) == 0      # no drafts, no eos: those two may be null


@pytest.mark.parametrize("half", [False, True])
def test_ngram_propose_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    P = 64

    def args(hist=P, hist_len=P, B=2, cap_h=100, len_max=50, emitted=P, m=P, n_emit=4, K=3, max_ngram=3, min_ngram=1, out=P):
        return (None, hist, hist_len, B, cap_h, len_max, emitted, m, n_emit, K, max_ngram, min_ngram, out)

    bad = [(dict([(k, None)]), b"null operand") for k in ("hist", "hist_len", "emitted", "m", "out")]
    bad += [(dict(B=-1), b"bad shape"), (dict(cap_h=0, len_max=0), b"bad shape"), (dict(K=0), b"bad K"), (dict(K=64), b"bad K"),
            (dict(n_emit=-1), b"bad n_emit"), (dict(n_emit=65), b"bad n_emit"), (dict(min_ngram=0), b"bad n-gram"),
            (dict(min_ngram=3, max_ngram=2), b"bad n-gram"), (dict(max_ngram=9), b"bad n-gram"),
            (dict(len_max=101), b"hist_len + m > cap_h"), (dict(len_max=-1), b"hist_len + m > cap_h"),
            (dict(B=0, len_max=101), b"hist_len + m > cap_h")]
    for kw, msg in bad:
        rc = l.setok_ngram_propose(*args(**kw))
        assert rc == -1 and msg in l.setok_last_error(), (kw, l.setok_last_error())
    assert l.setok_ngram_propose(*args(B=0)) == 0
    assert l.setok_ngram_propose(*args(B=0, emitted=None, m=None, n_emit=0, len_max=100)) == 0      # propose only


def test_generate_refuses_a_bad_draft_before_any_device_call(lib):
    from setok_amd import llama, ops
    from setok_amd.generation import Drafter, LookupDrafter
    assert inspect.signature(llama.SetokimLlamaPrefill.generate).parameters["draft"].default is None
    assert "draft=" in llama.SetokimLlamaPrefill.generate.__doc__ and ops.SPEC_MAX_K == 63
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    m = llama.SetokimLlamaPrefill(kw).eval()                           # on the CPU: any device call would raise something else
    x = torch.zeros(2, 5, 64)
    with pytest.raises(TypeError, match="draft"):
        m.generate(inputs_embeds=x, max_new_tokens=4, draft=object())
    with pytest.raises(TypeError, match="draft"):
        m.generate(inputs_embeds=x, max_new_tokens=4, draft=3)

    class Bad(Drafter):
        def __init__(self, K):
            self.K = K

    for K in (0, 64, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="draft.K"):
            m.generate(inputs_embeds=x, max_new_tokens=4, draft=Bad(K))
    with pytest.raises(NotImplementedError, match="draft"):
        m.generate(inputs_embeds=x, max_new_tokens=4, draft=LookupDrafter(3), kv_cache="fp8")
    for kwd in (dict(K=0), dict(K=64), dict(K=True), dict(K=3, max_ngram=9), dict(K=3, min_ngram=0), dict(K=3, max_ngram=2, min_ngram=3)):
        with pytest.raises(ValueError, match="LookupDrafter"):
            LookupDrafter(**kwd)
    d = LookupDrafter(7)
    assert (d.K, d.max_ngram, d.min_ngram) == (7, 3, 1) and isinstance(d, Drafter)


def test_kv_cache_truncate_keeps_its_bounds(lib):
    from setok_amd.generation import KVCache
    c = KVCache(1, 2, 1, 8, 8, torch.float32, "cpu")
    c.key_mask[:, :6] = 1
    c.len = 6
    for n in (-1, 7, 8, 2.0, True):
        with pytest.raises(ValueError, match="truncate"):
            c.truncate(n)
    assert c.len == 6
    c.truncate(6)
    assert c.len == 6 and int(c.key_mask.sum()) == 12
    c.truncate(4)
    assert c.len == 4 and c.key_mask[:, :4].all() and not c.key_mask[:, 4:].any()
    c.truncate(0)
    assert c.len == 0 and not c.key_mask.any()


# ---- the loop invariant on a toy model ---------------------------------------------------------------------------------------------------------
def _toy_speculative(prompts, max_new, vocab, eos, pad, K, pattern):
    """generate(draft=...)'s rounds with tests/spec_cases.py's rules and a model that is a function of the consumed prefix.  Returns the output
    (B, n) and the number of rounds; asserts the cache invariants after every round."""
    B, T = len(prompts), len(prompts[0])
    truth = [S.toy_plain(p, max_new, vocab, set()) for p in prompts]
    cap = T + max_new + K
    seq = torch.full((B, max_new), pad, dtype=torch.int64)
    count, finished = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.uint8)
    pending, next_pos = torch.zeros(B, dtype=torch.int64), torch.full((B,), T, dtype=torch.int64)
    key_mask = torch.zeros(B, cap, dtype=torch.uint8)
    key_mask[:, :T] = 1
    length = T
    consumed = [list(p) for p in prompts]
    hist = torch.full((B, T + max_new + K + 1), -1, dtype=torch.int64)
    hist[:, :T] = torch.tensor(prompts)
    hist_len = torch.full((B,), T, dtype=torch.int32)
    sel = torch.tensor([[S.toy_token(consumed[b], vocab)] for b in range(B)])
    seq, count, finished, pending, key_mask, next_pos, emitted, m, summary = S.accept_rule(
        torch.zeros(B, 0, dtype=torch.int64), sel, eos, seq, count, finished, pending, key_mask, next_pos, length)
    key_mask[:, length] = 0
    rounds = 0
    while int(summary[1]) > 0:
        if length + K + 1 > cap:                                       # the holes used the room up: what cache.grown(2 * cap) does
            key_mask = torch.cat([key_mask, torch.zeros_like(key_mask)], dim=1)
            cap *= 2
        if pattern == "lookup":
            hist, hist_len, d = S.ngram_rule(hist, hist_len, emitted, m, K)
        else:
            good, cut = S.pattern_lengths(pattern, rounds, B, K)
            d = torch.tensor([S.script(truth[b], int(count[b]), int(good[b]), int(cut[b]), K, vocab) for b in range(B)])
        rows = []
        for b in range(B):
            fed = [int(pending[b])] + [max(int(t), 0) for t in d[b]]
            rows.append([S.toy_token(consumed[b] + fed[:i + 1], vocab) for i in range(K + 1)])
        old_pending, was_live = pending.clone(), finished == 0
        for b in range(B):
            if was_live[b]:                                            # what `extend` adds before the kernel runs: the rows it attended
                next_pos[b] += 1 + next((i for i, t in enumerate(d[b].tolist()) if t < 0), K)
        seq, count, finished, pending, key_mask, next_pos, emitted, m, summary = S.accept_rule(
            d, torch.tensor(rows), eos, seq, count, finished, pending, key_mask, next_pos, length)
        for b in range(B):
            if was_live[b]:
                consumed[b] += [int(old_pending[b])] + emitted[b, :int(m[b]) - 1].tolist()
            assert int(key_mask[b].sum()) == len(consumed[b]) == int(next_pos[b])      # attended slots == consumed tokens == next position
        length += int(summary[0])
        assert not key_mask[:, length:].any()
        rounds += 1
    n = int(count.max())
    return seq[:, :n], rounds


@pytest.mark.parametrize("K", [1, 3, 7])
@pytest.mark.parametrize("pattern", list(S.PATTERNS) + ["lookup"])
def test_the_rules_reproduce_the_plain_sequence_on_a_toy_model(pattern, K):
    vocab, pad, B, T = 6, 99, 3, 5
    prompts = [[(3 * b + 2 * t) % vocab for t in range(T)] for b in range(B)]
    for max_new, eos in ((1, None), (2, None), (12, None), (13, [4]), (12, [0, 5]), (9, [2])):
        plain = [S.toy_plain(p, max_new, vocab, set(eos or [])) for p in prompts]
        n = max(len(r) for r in plain)
        want = torch.tensor([r + [pad] * (n - len(r)) for r in plain])
        got, rounds = _toy_speculative(prompts, max_new, vocab, eos, pad, K, pattern)
        assert torch.equal(got, want), (max_new, eos)
        if eos is None:
            if pattern == "right":
                assert rounds == -(-(max_new - 1) // (K + 1))
            if pattern == "wrong":
                assert rounds == max_new - 1


def test_the_rules_on_hand_made_rows():
    """One sequence per situation, checked against values worked out by hand."""
    K, max_new, len0, cap = 3, 10, 4, 12
    draft = torch.tensor([[5, 6, 7], [5, 9, 7], [5, -1, 7], [5, 6, 7], [5, 6, 7], [5, 6, 7], [9, 9, 9]])
    sel = torch.tensor([[5, 6, 7, 8]] * 7)
    B = draft.shape[0]
    count = torch.tensor([0, 0, 0, 0, 8, 3, 0], dtype=torch.int32)
    finished = torch.tensor([0, 0, 0, 0, 0, 1, 0], dtype=torch.uint8)
    out = S.accept_rule(draft, sel, [8], torch.full((B, max_new), -7), count, finished, torch.full((B,), -3), torch.ones(B, cap, dtype=torch.uint8),
                        torch.full((B,), 20), len0)
    seq, count2, fin2, pending, km, npos, emitted, m, summary = out
    assert m.tolist() == [4, 2, 2, 4, 2, 0, 1]                         # all right (+ bonus); wrong at 1; cut at 1; all right; budget 2; finished; wrong at 0
    assert fin2.tolist() == [1, 0, 0, 1, 1, 1, 0]                      # the bonus token 8 is an eos; the budget ends row 4
    assert pending.tolist() == [8, 6, 6, 8, 6, -3, 5] and count2.tolist() == [4, 2, 2, 4, 10, 3, 1]
    assert npos.tolist() == [20, 18, 20, 20, 18, 20, 17]               # 20 - (1 + leading non-negative drafts) + m
    assert km[:, len0:len0 + 4].tolist() == [[1, 1, 1, 1], [1, 1, 0, 0], [1, 1, 0, 0], [1, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]]
    assert seq[4].tolist() == [-7] * 8 + [5, 6] and emitted[1].tolist() == [5, 6, -1, -1] and summary.tolist() == [4, 3, 0]
    hist = torch.tensor([[1, 2, 3, 9, 1, 2, 3, 4, 1, 2, 0, 0, 0, 0, 0, 0]])
    _, hl, prop = S.ngram_rule(hist, torch.tensor([10], dtype=torch.int32), torch.tensor([[3, -1]]), torch.tensor([1], dtype=torch.int32), 4)
    assert hl.tolist() == [11] and prop.tolist() == [[4, 1, 2, 3]]     # "1 2 3": the later occurrence (at 4) wins, its continuation runs to the end
