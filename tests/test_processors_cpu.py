"""Logits processors, without a GPU: the two entries of csrc/logits.hip are declared, exported by both builds and mirrored by the ctypes table; they
refuse bad arguments on the host before any launch; generate() refuses a bad `processors` and the combinations that are not built before any device
call; the torch statement of the rule (tests/processors_cases.py), fed by the oracle's forward, reproduces every case of
tests/golden/processors.npz - HuggingFace's own `generate(repetition_penalty=..., ...)` -; and the statement equals HF's four processor classes on
random scores and histories."""
import ctypes
import dataclasses
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import golden_io
import processors_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"setok_logits_process": 21, "setok_history_append": 9}
P, Q = 4096, 1 << 30                               # stand in for device pointers (far apart: logits and out may not overlap); nothing is dereferenced


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
    assert "logits.hip" in open(os.path.join(ROOT, "setok_amd", "csrc", "Makefile")).read()
    assert "---- Logits processors (csrc/logits.hip)" in open(os.path.join(ROOT, "include", "setok_hip.h")).read()


def _refused(l, fn, args_of, bad):
    for kw, msg in bad:
        rc = getattr(l, fn)(*args_of(**kw))
        assert rc == -1 and msg in l.setok_last_error(), (fn, kw, l.setok_last_error())


@pytest.mark.parametrize("half", [False, True])
def test_logits_process_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1

    def args(dtype=dt, logits=P, ld=128, B=2, n=4, V=100, hist=P, hist_len=P, prompt_len=P, cap_h=32, tail=P, penalty=1.3, ngram=3, min_new=2,
             eos=P, n_eos=2, suppress=P, n_suppress=2, out=Q, ld_out=100):
        return (None, dtype, logits, ld, B, n, V, hist, hist_len, prompt_len, cap_h, tail, penalty, ngram, min_new, eos, n_eos, suppress, n_suppress,
                out, ld_out)

    bad = [(dict([(k, None)]), b"null operand") for k in ("logits", "hist", "hist_len", "prompt_len", "tail", "eos", "suppress", "out")]
    bad += [(dict(B=-1), b"bad shape"), (dict(n=0), b"bad shape"), (dict(n=65), b"bad shape"), (dict(V=0), b"bad shape"),
            (dict(V=(1 << 20) + 1, ld=1 << 21, ld_out=1 << 21), b"bad shape"), (dict(ld=99), b"bad shape"), (dict(ld_out=99), b"bad shape"),
            (dict(cap_h=0), b"bad shape"), (dict(ngram=-1), b"bad ngram"), (dict(ngram=9), b"bad ngram"), (dict(min_new=-1), b"bad min_new"),
            (dict(n_eos=-1), b"bad id count"), (dict(n_eos=65), b"bad id count"), (dict(n_suppress=-1), b"bad id count"),
            (dict(n_suppress=65), b"bad id count"), (dict(penalty=0.0), b"bad penalty"), (dict(penalty=-1.0), b"bad penalty"),
            (dict(penalty=float("nan")), b"bad penalty"), (dict(penalty=float("inf")), b"bad penalty"),
            (dict(dtype=1 if half else 2), b"bad dtype"), (dict(dtype=7), b"bad dtype"),
            (dict(out=P), b"overlaps"), (dict(out=P + 2 * (7 * 128 + 100) - 4), b"overlaps"), (dict(logits=Q + 4 * (7 * 100 + 100) - 2), b"overlaps"),
            (dict(B=0, ngram=9), b"bad ngram")]                                                           # ... also with nothing to do
    _refused(l, "setok_logits_process", args, bad)
    assert l.setok_logits_process(*args(B=0)) == 0                   # nothing to do is not an error (and launches nothing)
    assert l.setok_logits_process(*args(B=0, n=1, tail=None, eos=None, n_eos=0, suppress=None, n_suppress=0, dtype=0, penalty=1.0, ngram=0)) == 0


@pytest.mark.parametrize("half", [False, True])
def test_history_append_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)

    def args(hist=P, hist_len=P, B=2, cap_h=32, len_max=32, emitted=P, m=P, n_emit=4):
        return (None, hist, hist_len, B, cap_h, len_max, emitted, m, n_emit)

    bad = [(dict([(k, None)]), b"null operand") for k in ("hist", "hist_len", "emitted")]
    bad += [(dict(B=-1), b"bad shape"), (dict(cap_h=0, len_max=0), b"bad shape"), (dict(n_emit=-1), b"bad n_emit"), (dict(n_emit=65), b"bad n_emit"),
            (dict(len_max=33), b"hist_len + m > cap_h"), (dict(len_max=-1), b"hist_len + m > cap_h"),
            (dict(B=0, len_max=33), b"hist_len + m > cap_h")]                                             # a full history: refused by the host bound
    _refused(l, "setok_history_append", args, bad)
    assert l.setok_history_append(*args(B=0)) == 0 and l.setok_history_append(*args(B=0, m=None)) == 0
    assert l.setok_history_append(*args(n_emit=0, emitted=None, m=None)) == 0                            # nothing to append launches nothing


def test_generate_refuses_bad_processors_before_any_device_call(lib):
    from setok_amd import llama, ops
    from setok_amd.generation import BeamSearch, GenerateOutput, GenerationState, KVCache, LogitsProcessors
    params = inspect.signature(llama.SetokimLlamaPrefill.generate).parameters
    assert params["processors"].default is None and params["output_scores"].default is False
    assert "processors=" in llama.SetokimLlamaPrefill.generate.__doc__ and (ops.LOGITS_MAX_NGRAM, ops.LOGITS_MAX_IDS) == (8, 64)
    assert callable(ops.logits_process) and callable(ops.history_append)
    fields = [f.name for f in dataclasses.fields(GenerateOutput)]
    assert fields[-1] == "scores" and dataclasses.fields(GenerateOutput)[-1].default is None
    sig = inspect.signature(LogitsProcessors.__init__).parameters
    assert [(k, v.default) for k, v in sig.items() if k != "self"] == [("repetition_penalty", 1.0), ("no_repeat_ngram_size", 0),
                                                                        ("min_new_tokens", 0), ("suppress_tokens", None)]
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.5), dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
               dict(repetition_penalty="1.3"), dict(repetition_penalty=True), dict(repetition_penalty=None),
               dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=9), dict(no_repeat_ngram_size=2.0), dict(no_repeat_ngram_size=True),
               dict(min_new_tokens=-1), dict(min_new_tokens=1.5), dict(min_new_tokens=True),
               dict(suppress_tokens=5), dict(suppress_tokens="5"), dict(suppress_tokens=[1, -2]), dict(suppress_tokens=[1.0]), dict(suppress_tokens=[True]),
               dict(suppress_tokens=list(range(65)))):
        with pytest.raises(ValueError, match="LogitsProcessors"):
            LogitsProcessors(**kw)
    p = LogitsProcessors()
    assert (p.repetition_penalty, p.no_repeat_ngram_size, p.min_new_tokens, p.suppress_tokens) == (1.0, 0, 0, [])
    p = LogitsProcessors(1.3, 3, 6, (4, 7))
    assert (p.repetition_penalty, p.no_repeat_ngram_size, p.min_new_tokens, p.suppress_tokens) == (1.3, 3, 6, [4, 7])

    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    m = llama.SetokimLlamaPrefill(kw).eval()                           # on the CPU: any device call would raise something else
    x = torch.zeros(2, 5, 64)
    for bad in (object(), 1.3, "1.3", dict(repetition_penalty=1.3)):
        with pytest.raises(TypeError, match="processors"):
            m.generate(inputs_embeds=x, max_new_tokens=4, processors=bad)
    with pytest.raises(NotImplementedError, match="processors= with beams="):
        m.generate(inputs_embeds=x, max_new_tokens=4, processors=LogitsProcessors(1.3), beams=BeamSearch(2))
    state = GenerationState(cache=KVCache(1, 2, 4, 16, 16, torch.float32, "cpu"), pending=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="processors= with past="):
        m.generate(inputs_embeds=x, max_new_tokens=4, processors=LogitsProcessors(1.3), past=state)
    with pytest.raises(ValueError, match="output_scores=True"):
        m.generate(inputs_embeds=x, max_new_tokens=4, output_scores=True, return_dict_in_generate=True)          # no processors
    with pytest.raises(ValueError, match="output_scores=True"):
        m.generate(inputs_embeds=x, max_new_tokens=4, output_scores=True, processors=LogitsProcessors(1.3))      # no return_dict_in_generate
    with pytest.raises(NotImplementedError, match="greedy"):
        m.generate(inputs_embeds=x, max_new_tokens=4, repetition_penalty=1.3)                                     # HF's own spelling stays refused


# ---- the rule against HuggingFace -----------------------------------------------------------------------------------------------------------------
def load_fixture(golden_dir):
    z = golden_io.load(os.path.join(golden_dir, "processors.npz"))
    g = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files}
    g["sd"] = {k[2:]: v for k, v in g.items() if k.startswith("w:")}
    return g


def test_the_fixture_holds_every_case():
    z = golden_io.load(os.path.join(ROOT, "tests", "golden", "processors.npz"))
    assert {k.split(":")[0] for k in z.files if ":" in k and not k.startswith("w:")} == set(PC.CASES)      # no case is left out, none is unknown


@pytest.mark.parametrize("name", list(PC.CASES))
def test_the_statement_reproduces_huggingface_on_every_fixture_case(golden_dir, name):
    g = load_fixture(golden_dir)
    penalty, ngram, min_new, n_sup, embeds, must_ban = PC.CASES[name]
    lc, sd = PC.weights(int(g["seed"]))
    ids, am, x = PC.prompts(int(g["seed"]))
    assert all(torch.equal(sd[k], g["sd"][k]) for k in sd) and torch.equal(ids, g["ids"]) and torch.equal(am, g["am"]) and torch.equal(x, g["x"])
    eos, suppress = tuple(g[f"{name}:eos"].tolist()), tuple(g[f"{name}:suppress"].tolist())
    assert len(suppress) == n_sup and (len(eos) > 0) == (min_new > 0) and float(g[f"{name}:margin"]) >= PC.MIN_MARGIN
    emb = sd["model.embed_tokens.weight"]
    differs, banned = False, False
    for b, n in enumerate(PC.PROMPT_LEN):
        i = torch.zeros(0, dtype=torch.int64) if embeds else ids[b, PC.T - n:]
        xe = x[b, PC.T - n:] if embeds else emb[i]
        ref = PC.run_reference(sd, lc, xe, i, penalty, ngram, min_new, eos, suppress)
        k = int(g[f"{name}:lengths"][b])
        assert ref["tokens"].numel() == k and torch.equal(ref["tokens"], g[f"{name}:tokens"][b, :k]) and ref["margin"] >= PC.MIN_MARGIN
        want = g[f"{name}:scores"][b, :k]
        assert torch.equal(ref["scores"] == PC.NEG_INF, want == PC.NEG_INF)
        assert float((ref["scores"] - want).masked_fill(want == PC.NEG_INF, 0.0).abs().max()) <= 5e-5
        free = PC.run_reference(sd, lc, xe, i, 1.0, 0, 0, (), ())
        differs = differs or not torch.equal(free["tokens"][:k], ref["tokens"])
        banned = banned or bool((ref["scores"][torch.arange(k), ref["raw"]] == PC.NEG_INF).any())
    assert differs and (banned or not must_ban)                        # no case passes with the processors switched off


def test_the_statement_equals_huggingfaces_processor_classes():
    lp = pytest.importorskip("transformers.generation.logits_process")
    g = torch.Generator().manual_seed(11)
    Bn, V = 4, 50
    for trial in range(40):
        L = int(torch.randint(0, 30, (1,), generator=g))
        ids = torch.randint(0, 8 if trial % 2 else V, (Bn, L), generator=g)                 # few distinct ids: repeated n-grams
        prompt = int(torch.randint(0, L + 1, (1,), generator=g))
        scores = torch.randn(Bn, V, generator=g) * 3
        scores[0, 3], scores[1, 5] = float("-inf"), 0.0
        penalty = (1.0, 1.3, 0.7)[trial % 3]
        ngram = trial % 5
        min_new = (0, 4, 40)[trial % 3]
        eos, suppress = [7, 2], [0, V - 1, 9][:trial % 4]
        want = scores.clone()
        if penalty != 1.0:
            want = lp.RepetitionPenaltyLogitsProcessor(penalty)(ids, want)
        if ngram:
            want = lp.NoRepeatNGramLogitsProcessor(ngram)(ids, want)
        if min_new:
            want = lp.MinNewTokensLengthLogitsProcessor(prompt, min_new, eos, device="cpu")(ids, want)
        if suppress:
            want = lp.SuppressTokensLogitsProcessor(suppress, device="cpu")(ids, want)
        hist = torch.cat([ids, torch.full((Bn, 3), 10 ** 12)], dim=1)
        got = PC.process(scores, hist, torch.full((Bn,), L), torch.full((Bn,), prompt), None, penalty, ngram, min_new, eos, suppress)
        assert torch.equal(got, want), (trial, penalty, ngram, min_new, suppress)
        if L >= 2:                                                     # the same rows as a verify round: the last two history entries as the tail
            wide = scores.repeat_interleave(3, dim=0)
            rows = PC.process(wide, hist[:, :L - 2].contiguous(), torch.full((Bn,), L - 2), torch.full((Bn,), prompt), ids[:, L - 2:], penalty, ngram,
                              min_new, eos, suppress)
            assert torch.equal(rows[2::3], want), trial
