"""Logits processors on a real MI355X, all through the C ABI: setok_logits_process and setok_history_append against the torch statement of the rule
(tests/processors_cases.py) to the bit, and `SetokimLlamaPrefill.generate(processors=...)` against HuggingFace's own
`generate(repetition_penalty=..., no_repeat_ngram_size=..., min_new_tokens=..., suppress_tokens=...)` (tests/golden/processors.npz,
tests/golden/make_golden_processors.py), against itself in 16 bits, and with a draft against the plain loop.  `pytest -m gpu`.

Every output of setok_logits_process is one fp32 rounding of its inputs (a conversion, one multiply or one true division, or -inf), so the bound
against the statement is equality."""
import os

import numpy as np
import pytest
import torch

import golden_io
import llama_bwd_cases as LC
import parity
import processors_cases as PC
import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib, ops
    from setok_amd.generation import LogitsProcessors, LookupDrafter, Sampler
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
G = 3                                              # the n-gram size of the grid
SENTINEL = 777.0


# ---- setok_logits_process -------------------------------------------------------------------------------------------------------------------------
def _problem(dt, V, n, L, seed):
    """B = 3 sequences.  Histories of L, L and max(L - 1, 0) entries drawn from six ids (duplicates, repeated n-grams) that include 0 and V - 1, a
    twentieth of them replaced by negative ids and ids >= V; sequence 0 ends in in-range ids (its bans happen), the others end as drawn.  The slots
    behind hist_len hold 1e12 and negative values.  tail (B, n - 1) from the same ids, one entry negative.  Logits with both signs, +-0, -inf and a
    NaN in columns the histories name."""
    g = torch.Generator().manual_seed(seed)
    Bn = 3
    pool = torch.tensor([0, V - 1, 3, 5, 17, 42])
    odd = torch.tensor([-1, -200, V, V + 7, 10 ** 12])
    cap_h = L + 5
    hist = pool[torch.randint(0, 6, (Bn, cap_h), generator=g)]
    swap = torch.rand(Bn, cap_h, generator=g) < 0.05
    hist = torch.where(swap, odd[torch.randint(0, 5, (Bn, cap_h), generator=g)], hist)
    hist_len = torch.tensor([L, L, max(L - 1, 0)], dtype=torch.int32)
    if L >= 1:
        hist[0, max(L - G, 0):L] = pool[torch.randint(0, 6, (min(G, L),), generator=g)]
    if L >= 20:                                                                            # an 8-gram ban: window 2 repeats the last 7 entries and names id 17
        hist[0, L - 7:L] = pool[torch.randint(0, 6, (7,), generator=g)]
        hist[0, 2:9], hist[0, 9] = hist[0, L - 7:L].clone(), 17
    for b in range(Bn):
        hist[b, int(hist_len[b]):] = torch.tensor([10 ** 12, -7, 10 ** 12, -1, 10 ** 12, -3])[:cap_h - int(hist_len[b])]
    tail = None
    if n > 1:
        tail = pool[torch.randint(0, 6, (Bn, n - 1), generator=g)]
        tail[1, 1] = -1
    prompt_len = torch.tensor([0, L // 2, L], dtype=torch.int32)
    x = (torch.randn(Bn * n, V, generator=g) * 3).to(dt)
    x[:, 0], x[:, V - 1] = -x[:, 0].abs() - 0.5, x[:, V - 1].abs() + 0.5
    x[:, 3], x[:, 5], x[:, 17], x[:, 42] = float("-inf"), float("nan"), -0.0, 0.0
    x[0, 0], x[1, V - 1] = float("nan"), float("-inf")
    return x, hist.contiguous(), hist_len, prompt_len, tail


def _windows(x):
    """The logits as a column window, at an odd element offset, of a NaN-padded wider buffer with an odd row stride; `out` as a window of a
    sentinel-filled buffer."""
    rows, V = x.shape
    buf = torch.full((rows, V + 11), float("nan"), dtype=x.dtype, device=DEV)
    buf[:, 3:3 + V] = x.to(DEV)
    out = torch.full((rows, V + 6), SENTINEL, dtype=torch.float32, device=DEV)
    return buf[:, 3:3 + V], out, out[:, 2:2 + V]


def _settings(V):
    eos = [0, V - 1, V + 3, 5]
    sup = [1, V - 1, 2 ** 40, -5]
    return {"penalty": dict(penalty=1.3), "ngram": dict(ngram=G), "ngram1": dict(ngram=1), "ngram8": dict(ngram=8),
            "min_new": dict(min_new=3, eos=eos), "suppress": dict(suppress=sup),
            "below1": dict(penalty=0.5, ngram=2), "all": dict(penalty=1.2, ngram=G, min_new=3, eos=eos, suppress=sup)}          # ("all" stays last)


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("V", [100, 32003])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_logits_process_equals_the_statement_to_the_bit(dt, V, n):
    ids = lambda v: None if v is None else torch.tensor(v, dtype=torch.int64, device=DEV)
    for L in sorted({0, 1, G - 2, G - 1, G, 7, 1030}):                                     # 1030: past one workgroup's stride of 256 four times over
        x, hist, hist_len, prompt_len, tail = _problem(dt, V, n, L, seed=1000 * n + L)
        xw, buf, out = _windows(x)
        dev = [t.to(DEV) for t in (hist, hist_len, prompt_len)] + [None if tail is None else tail.to(DEV)]
        for name, kw in _settings(V).items():
            buf.fill_(SENTINEL)
            got = ops.logits_process(xw, *dev, penalty=kw.get("penalty", 1.0), ngram=kw.get("ngram", 0), min_new=kw.get("min_new", 0),
                                     eos=ids(kw.get("eos")), suppress=ids(kw.get("suppress")), out=out)
            want = PC.process(x, hist, hist_len, prompt_len, tail, kw.get("penalty", 1.0), kw.get("ngram", 0), kw.get("min_new", 0),
                              kw.get("eos", ()), kw.get("suppress", ()))
            assert got.data_ptr() == out.data_ptr() and PC.same(got, want), (name, L)
            assert bool((buf[:, :2] == SENTINEL).all()) and bool((buf[:, 2 + V:] == SENTINEL).all()), (name, L)     # the columns around the window
            if L == 1030:
                assert not PC.same(want, x.float()), (name, L)                             # the setting really changes the rows
        fresh = ops.logits_process(xw.contiguous(), *dev, penalty=1.2, ngram=G, min_new=3, eos=ids(_settings(V)["all"]["eos"]),
                                   suppress=ids(_settings(V)["all"]["suppress"]))
        assert PC.same(fresh, out)                                                         # another buffer, another alignment: the same bits


def test_logits_process_is_refused_through_the_wrapper():
    x = torch.zeros(2, 10, device=DEV)
    hist, hl = torch.zeros(2, 4, dtype=torch.int64, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.SetokHipError, match="overlaps"):
        ops.logits_process(x, hist, hl, hl, out=x)
    with pytest.raises(_lib.SetokHipError, match="bad penalty"):
        ops.logits_process(x, hist, hl, hl, penalty=0.0)
    with pytest.raises(ValueError, match="B \\* n"):
        ops.logits_process(x, hist, hl, hl, tail=torch.zeros(2, 2, dtype=torch.int64, device=DEV))


# ---- setok_history_append -------------------------------------------------------------------------------------------------------------------------
def test_history_append_equals_the_statement_and_never_writes_behind_a_row():
    g = torch.Generator().manual_seed(3)
    Bn, cap_h = 3, 12
    guard = torch.randint(-50, 50, (Bn + 1, cap_h), generator=g)                           # row Bn is what a write behind the last row would hit
    lens = torch.tensor([0, 5, 8], dtype=torch.int32)
    emitted = torch.randint(-3, 100, (Bn, 4), generator=g)
    for m in (torch.tensor([0, 4, 2], dtype=torch.int32), None):
        buf, hl = guard.clone().to(DEV), lens.clone().to(DEV)
        ops.history_append(buf[:Bn], hl, emitted.to(DEV), cap_h, None if m is None else m.to(DEV))
        want, want_len = PC.append(guard[:Bn], lens, emitted, m)
        assert torch.equal(buf[:Bn].cpu(), want) and torch.equal(hl.cpu(), want_len) and torch.equal(buf[Bn].cpu(), guard[Bn]), m
    buf, hl = guard.clone().to(DEV), lens.clone().to(DEV)                                  # (B, 1): the plain loop's step
    ops.history_append(buf[:Bn], hl, emitted[:, :1].contiguous().to(DEV), 9)
    assert hl.tolist() == [1, 6, 9] and torch.equal(buf[:Bn].cpu(), PC.append(guard[:Bn], lens, emitted[:, :1])[0])
    # full rows: the host bound refuses the call; with a bound that understates the device lengths the kernel still writes nothing
    full = torch.tensor([cap_h, cap_h, 99], dtype=torch.int32)
    buf, hl = guard.clone().to(DEV), full.clone().to(DEV)
    with pytest.raises(ValueError, match="hist_len \\+ m > cap_h"):
        ops.history_append(buf[:Bn], hl, emitted.to(DEV), cap_h + 4)
    with pytest.raises(_lib.SetokHipError, match="hist_len \\+ m > cap_h"):
        _lib.call("setok_history_append", ops._stream(), buf.data_ptr(), hl.data_ptr(), Bn, cap_h, cap_h + 1, emitted.to(DEV).data_ptr(), None, 4)
    ops.history_append(buf[:Bn], hl, emitted.to(DEV), cap_h)
    torch.cuda.synchronize()
    assert torch.equal(buf.cpu(), guard) and torch.equal(hl.cpu(), full)
    part = torch.tensor([cap_h - 2, cap_h - 1, cap_h - 4], dtype=torch.int32)              # rows with room for some of the 4 entries: cut at the row's end
    buf, hl = guard.clone().to(DEV), part.clone().to(DEV)
    ops.history_append(buf[:Bn], hl, emitted.to(DEV), cap_h)
    assert hl.tolist() == [cap_h] * 3 and torch.equal(buf[Bn].cpu(), guard[Bn])
    assert torch.equal(buf[0, -2:].cpu(), emitted[0, :2]) and torch.equal(buf[1, -1:].cpu(), emitted[1, :1]) and torch.equal(buf[2, -4:].cpu(), emitted[2])


# ---- generate(processors=...) ---------------------------------------------------------------------------------------------------------------------
_STATE = {}


def _fixture(golden_dir):
    if "g" not in _STATE:                                                                  # read once, shared, never written to
        z = golden_io.load(os.path.join(golden_dir, "processors.npz"))
        g = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
        g["sd"] = {k[2:]: v for k, v in g.items() if k.startswith("w:")}
        m = SetokimLlamaPrefill(dict(PC.LLAMA))
        m.load_state_dict(g["sd"], strict=True)
        _STATE["g"], _STATE["m"] = g, m.to(DEV).eval()
    return _STATE["m"], _STATE["g"]


def _prompt(g, embeds):
    am = g["am"].to(DEV)
    return dict(inputs_embeds=g["x"].to(DEV), attention_mask=am) if embeds else dict(inputs=g["ids"].to(DEV), attention_mask=am)


def _processors(g, name):
    penalty, ngram, min_new, _, _, _ = PC.CASES[name]
    return LogitsProcessors(penalty, ngram, min_new, g[f"{name}:suppress"].tolist() or None), g[f"{name}:eos"].tolist() or None


@pytest.mark.parametrize("name", list(PC.CASES))
def test_generate_with_processors_reproduces_huggingface(golden_dir, name):
    """fp32, the three sequences batched and left-padded: HF's tokens (each sequence ran alone there), and HF's processed scores under the bound
    the generate tests hold fp32 logits to against HF (parity.close at 1e-4) with the banned columns equal."""
    m, g = _fixture(golden_dir)
    proc, eos = _processors(g, name)
    out = m.generate(**_prompt(g, PC.CASES[name][4]), max_new_tokens=PC.N_NEW, eos_token_id=eos, processors=proc, return_dict_in_generate=True,
                     output_scores=True, output_logits=True)
    lengths = g[f"{name}:lengths"].tolist()
    n_new = max(lengths)
    want = g[f"{name}:tokens"][:, :n_new].clone()
    if eos:
        want[want < 0] = eos[0]                                                            # a finished sequence pads with the first eos id
    assert torch.equal(out.sequences.cpu(), want), name
    assert out.scores.dtype == torch.float32 and out.scores.shape == (PC.B, n_new, PC.LLAMA["vocab_size"]) == out.logits.shape
    for b, k in enumerate(lengths):
        got, ref = out.scores[b, :k].cpu(), g[f"{name}:scores"][b, :k]
        assert torch.equal(got == PC.NEG_INF, ref == PC.NEG_INF), (name, b)
        rel = parity.close(got.masked_fill(ref == PC.NEG_INF, 0.0), ref.masked_fill(ref == PC.NEG_INF, 0.0), 1e-4, f"{name}[{b}] processed scores")
        print(f"generate(processors) {name}[{b}]: scores max rel {rel:.3e}")
    plain = m.generate(**_prompt(g, PC.CASES[name][4]), max_new_tokens=PC.N_NEW, eos_token_id=eos, processors=proc)
    assert torch.equal(plain, out.sequences)
    free = m.generate(**_prompt(g, PC.CASES[name][4]), max_new_tokens=PC.N_NEW, eos_token_id=eos)
    assert free.shape != plain.shape or not torch.equal(free, plain)                       # the processors matter


def test_neutral_processors_change_nothing(golden_dir):
    m, g = _fixture(golden_dir)
    for embeds in (False, True):
        kw = dict(_prompt(g, embeds), max_new_tokens=PC.N_NEW, return_dict_in_generate=True, output_logits=True)
        base = m.generate(**kw)
        out = m.generate(processors=LogitsProcessors(), output_scores=True, **kw)
        assert torch.equal(out.sequences, base.sequences) and torch.equal(out.logits, base.logits) and torch.equal(out.scores, base.logits.float())
        assert base.scores is None
    eos = [int(base.sequences[0, 2])]                                                      # min_new_tokens without eos ids does nothing (HF's rule) ...
    assert torch.equal(m.generate(processors=LogitsProcessors(min_new_tokens=5), **kw).sequences, base.sequences)
    held = m.generate(processors=LogitsProcessors(min_new_tokens=5), eos_token_id=eos, **kw).sequences
    assert not bool((held[:, :5] == eos[0]).any()) and int(m.generate(eos_token_id=eos, **kw).sequences[0, 2]) == eos[0]      # ... and holds one back


def _dh128_model(dt):
    """The head-dim-128 grouped-query case of tests/llama_bwd_cases.py (every GEMM dimension a multiple of 64, as the 16-bit kernels need) with the
    fixture's weight scale; three prompts of ids, the second and third left-padded."""
    if dt not in _STATE:
        kw, lc, seed, _, _, _, _, _ = LC.case_inputs("gqa_dh128")
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict({k: v * PC.WEIGHT_SCALE for k, v in O.init_llama_weights(lc, seed=seed).items()}, strict=True)
        _STATE[dt] = m.to(device=DEV, dtype=dt).eval()
    ids, am, _ = PC.prompts(2)
    return _STATE[dt], ids, am


def _lowest_argmax(s):
    V = s.shape[-1]
    return torch.where(s == s.max(dim=-1, keepdim=True).values, torch.arange(V, device=s.device), V).min(dim=-1).values


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_16bit_scores_are_the_statement_of_the_steps_own_logits(dt):
    m, ids, am = _dh128_model(dt)
    eos = [5, 9]
    out = m.generate(inputs=ids.to(DEV), attention_mask=am.to(DEV), max_new_tokens=PC.N_NEW, processors=LogitsProcessors(1.3, 2, 4, [7, 11]),
                     eos_token_id=eos, return_dict_in_generate=True, output_logits=True, output_scores=True)
    n_new = out.sequences.shape[1]
    assert out.logits.dtype == dt and out.scores.dtype == torch.float32 and n_new >= 4
    hist = torch.full((PC.B, PC.T + n_new), -1, dtype=torch.int64)
    order = torch.argsort((am == 0).to(torch.int8), dim=1, stable=True)
    hist[:, :PC.T] = ids.gather(1, order)
    hist_len = am.sum(1)
    prompt_len = hist_len.clone()
    changed = False
    for j in range(n_new):
        want = PC.process(out.logits[:, j], hist, hist_len, prompt_len, None, 1.3, 2, 4, eos, [7, 11])
        assert PC.same(out.scores[:, j], want), j
        live = ~torch.isin(out.sequences[:, :j], torch.tensor(eos, device=DEV)).any(dim=1)   # (a finished sequence emits the pad id, whatever its scores)
        assert torch.equal(out.sequences[live, j], _lowest_argmax(out.scores[live, j])), j
        changed = changed or not PC.same(want, out.logits[:, j].float())
        hist, hist_len = PC.append(hist, hist_len, out.sequences[:, j:j + 1])
    assert changed                                                                         # the scores are not the logits


class _Launches:
    """Counts the `_lib.call`s of one entry while the block runs."""

    def __init__(self, monkeypatch, entry):
        self.mp, self.entry, self.count = monkeypatch, entry, 0

    def __enter__(self):
        real = _lib.call
        self.ctx = self.mp.context()

        def call(name, *a, **k):
            self.count += name == self.entry
            return real(name, *a, **k)

        self.ctx.__enter__().setattr(_lib, "call", call)
        return self

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_draft_and_verify_with_processors_emits_the_plain_loops_tokens(golden_dir, monkeypatch, sampled):
    """B = 3, fp32, LookupDrafter(3).  A repetition penalty below 1 rewards what the history holds, so the run repeats itself and the lookup drafts
    are accepted (13 and 12 rounds for 16 tokens in the torch statement of both rules): the rows behind row 0 of a round - the tail path - decide
    tokens.  The 8-gram ban and the suppressed id act on the same rows."""
    m, g = _fixture(golden_dir)
    n = 16
    u = torch.rand(n, PC.B, generator=torch.Generator().manual_seed(5))
    mk = (lambda: Sampler(temperature=0.3, top_k=3, u=u)) if sampled else (lambda: None)
    kw = dict(_prompt(g, False), max_new_tokens=n, processors=LogitsProcessors(0.4, 8, 0, [1]), return_dict_in_generate=True, output_scores=True)
    with _Launches(monkeypatch, "setok_logits_process") as steps:
        plain = m.generate(sampler=mk(), **kw)
    with _Launches(monkeypatch, "setok_logits_process") as rounds:
        out = m.generate(sampler=mk(), draft=LookupDrafter(3), **kw)
    assert steps.count == n and plain.sequences.shape == (PC.B, n)
    assert torch.equal(out.sequences, plain.sequences)
    assert rounds.count < n, rounds.count                                                  # fewer rounds (the first token included) than tokens: drafts were accepted
    assert torch.equal(out.scores == PC.NEG_INF, plain.scores == PC.NEG_INF)
    parity.close(out.scores.masked_fill(plain.scores == PC.NEG_INF, 0.0), plain.scores.masked_fill(plain.scores == PC.NEG_INF, 0.0), 1e-4,
                 "scores of a round against the plain loop's")                              # (the extend kernel sums in another order than the decode step)
    free = m.generate(sampler=mk(), **dict(kw, processors=None, output_scores=False))
    assert not torch.equal(free.sequences, plain.sequences)
