"""Beam search, without a GPU: the three entries of csrc/beam.hip are declared, exported by both builds and mirrored by the ctypes table; they refuse
bad arguments on the host before any launch; generate() refuses a bad `beams` and the combinations that are not built before any device call; and
the torch statement of the rule (tests/beam_cases.py), fed by the oracle's forward, reproduces every case of tests/golden/beam.npz - HuggingFace's
own `generate(num_beams=...)`."""
import ctypes
import dataclasses
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import beam_cases as BC
import golden_io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"setok_beam_topk": 15, "setok_beam_advance": 26, "setok_kv_reorder": 16}
P = 4096                                           # stands in for a device pointer: every call below is refused before anything is dereferenced


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
    assert "beam.hip" in open(os.path.join(ROOT, "setok_amd", "csrc", "Makefile")).read()
    assert '"Beam search"' in open(os.path.join(ROOT, "setok_amd", "csrc", "beam.hip")).read()
    assert "---- Beam search (csrc/beam.hip)" in open(os.path.join(ROOT, "include", "setok_hip.h")).read()


def _refused(l, fn, args_of, bad):
    for kw, msg in bad:
        rc = getattr(l, fn)(*args_of(**kw))
        assert rc == -1 and msg in l.setok_last_error(), (fn, kw, l.setok_last_error())


@pytest.mark.parametrize("half", [False, True])
def test_beam_topk_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1

    def args(dtype=dt, logits=P, ld=128, B=2, n_in=3, V=100, running=P, C=9, score=P, token=P, beam=P, status=P, ws=P, ws_bytes=1 << 20):
        return (None, dtype, logits, ld, B, n_in, V, running, C, score, token, beam, status, ws, ws_bytes)

    bad = [(dict([(k, None)]), b"null operand") for k in ("logits", "running", "score", "token", "beam", "status", "ws")]
    bad += [(dict(B=-1), b"bad shape"), (dict(n_in=0), b"bad shape"), (dict(n_in=17), b"bad shape"), (dict(V=0), b"bad shape"),
            (dict(V=(1 << 20) + 1, ld=1 << 21), b"bad shape"), (dict(ld=99), b"bad shape"),
            (dict(C=0), b"bad C"), (dict(C=65), b"bad C"), (dict(C=9, n_in=1, V=8, ld=8), b"bad C"),      # more candidates than the sequence has
            (dict(dtype=1 if half else 2), b"bad dtype"), (dict(dtype=7), b"bad dtype"),
            (dict(ws_bytes=2 * 3 * 516 - 1), b"workspace"), (dict(ws=P + 2), b"4-byte aligned"),
            (dict(B=0, C=65), b"bad C")]                                                                  # ... also with nothing to do
    _refused(l, "setok_beam_topk", args, bad)
    assert l.setok_beam_topk(*args(B=0)) == 0                       # nothing to do is not an error (and launches nothing)
    assert l.setok_beam_topk(*args(B=0, dtype=0, C=64, ws_bytes=0)) == 0


@pytest.mark.parametrize("half", [False, True])
def test_beam_advance_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    names = ("score", "token", "beam", "status", "run_score", "fin_score", "fin_flag", "fin_len", "fin_parent", "fin_token", "heur", "bp_token",
             "bp_parent", "next_token", "src_row", "summary")

    def args(B=2, n=3, C=9, eos=P, n_eos=2, step=0, max_new=10, lp=1.0, es=0, **ptr):
        p = {k: ptr.get(k, P) for k in names}
        return (None, p["score"], p["token"], p["beam"], p["status"], B, n, C, eos, n_eos, step, max_new, lp, es, p["run_score"], p["fin_score"],
                p["fin_flag"], p["fin_len"], p["fin_parent"], p["fin_token"], p["heur"], p["bp_token"], p["bp_parent"], p["next_token"], p["src_row"],
                p["summary"])

    bad = [(dict([(k, None)]), b"null operand") for k in names + ("eos",)]
    bad += [(dict(B=-1), b"bad shape"), (dict(n=0), b"bad shape"), (dict(n=17, C=34), b"bad shape"), (dict(C=2), b"bad C"), (dict(C=65), b"bad C"),
            (dict(n=16, C=80), b"bad C"), (dict(n_eos=-1), b"bad n_eos"), (dict(step=-1), b"bad step"), (dict(step=10), b"bad step"),
            (dict(max_new=0), b"bad step"), (dict(lp=float("nan")), b"bad length_penalty"), (dict(lp=float("inf")), b"bad length_penalty"),
            (dict(es=3), b"bad early_stopping"), (dict(es=-1), b"bad early_stopping"), (dict(B=0, C=65), b"bad C")]
    _refused(l, "setok_beam_advance", args, bad)
    assert l.setok_beam_advance(*args(B=0)) == 0
    assert l.setok_beam_advance(*args(B=0, eos=None, n_eos=0, C=6, es=2, lp=-0.5, step=9)) == 0      # no eos: the list may be null


@pytest.mark.parametrize("half", [False, True])
def test_kv_reorder_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)

    def args(ptrs=P, row_bytes=P, unit=P, n_tensors=4, unit_total=4 * 256, rows=6, n=3, Hkv=2, cap=40, slot0=10, slot1=15, src_row=P, scratch=P,
             scratch_bytes=4 * 256 * 6 * 2 * 5, status=P):
        return (None, ptrs, row_bytes, unit, n_tensors, unit_total, rows, n, Hkv, cap, slot0, slot1, src_row, scratch, scratch_bytes, status)

    bad = [(dict([(k, None)]), b"null operand") for k in ("ptrs", "row_bytes", "unit", "src_row", "status")]
    bad += [(dict(n_tensors=0), b"bad shape"), (dict(n_tensors=65536), b"bad shape"), (dict(rows=-3), b"bad shape"), (dict(n=0), b"bad shape"),
            (dict(rows=7), b"bad shape"), (dict(Hkv=0), b"bad shape"), (dict(cap=0, slot0=0, slot1=0), b"bad shape"), (dict(unit_total=8), b"bad shape"),
            (dict(slot0=-1), b"not inside the cache"), (dict(slot0=16), b"not inside the cache"), (dict(slot1=41), b"not inside the cache"),
            (dict(scratch=None), b"scratch"), (dict(scratch_bytes=4 * 256 * 6 * 2 * 5 - 1), b"scratch"), (dict(scratch=P + 8), b"scratch"),
            (dict(rows=0, slot1=41), b"not inside the cache")]
    _refused(l, "setok_kv_reorder", args, bad)
    assert l.setok_kv_reorder(*args(rows=0)) == 0
    assert l.setok_kv_reorder(*args(rows=0, slot1=10, scratch=None, scratch_bytes=0)) == 0          # an empty region needs no scratch


def test_generate_refuses_bad_beams_before_any_device_call(lib):
    from setok_amd import llama, ops
    from setok_amd.generation import BeamSearch, GenerateOutput, LookupDrafter, Sampler
    assert inspect.signature(llama.SetokimLlamaPrefill.generate).parameters["beams"].default is None
    assert "beams=" in llama.SetokimLlamaPrefill.generate.__doc__ and (ops.BEAM_MAX_C, ops.BEAM_MAX_N) == (64, 16)
    fields = {f.name: f.default for f in dataclasses.fields(GenerateOutput)}
    assert fields["sequences_scores"] is None and fields["beam_indices"] is None
    for kw in (dict(num_beams=0), dict(num_beams=17), dict(num_beams=2.0), dict(num_beams=True), dict(num_beams=None),
               dict(num_beams=4, num_return_sequences=0), dict(num_beams=4, num_return_sequences=5), dict(num_beams=4, num_return_sequences=True),
               dict(num_beams=4, length_penalty=float("nan")), dict(num_beams=4, length_penalty=float("inf")), dict(num_beams=4, length_penalty="1"),
               dict(num_beams=4, early_stopping="always"), dict(num_beams=4, early_stopping=1), dict(num_beams=4, early_stopping=None)):
        with pytest.raises(ValueError, match="BeamSearch"):
            BeamSearch(**kw)
    b = BeamSearch(4)
    assert (b.num_beams, b.length_penalty, b.early_stopping, b.num_return_sequences) == (4, 1.0, False, 1)
    assert BeamSearch(3, 0.6, "never", 3).candidates(2, 100) == 9 and BeamSearch(16).candidates(0, 32000) == 32 and BeamSearch(1).candidates(0, 2) == 2

    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    m = llama.SetokimLlamaPrefill(kw).eval()                           # on the CPU: any device call would raise something else
    x = torch.zeros(2, 5, 64)
    for bad in (object(), 4, "4", dict(num_beams=4)):
        with pytest.raises(TypeError, match="beams"):
            m.generate(inputs_embeds=x, max_new_tokens=4, beams=bad)
    with pytest.raises(ValueError, match="exceed 64"):
        m.generate(inputs_embeds=x, max_new_tokens=4, beams=BeamSearch(16), eos_token_id=[1, 2, 3, 4])          # C = 5 * 16
    with pytest.raises(ValueError, match="exceed 64"):
        m.generate(inputs_embeds=x, max_new_tokens=4, beams=BeamSearch(13), eos_token_id=[1, 2, 3, 4])          # C = 65
    small = llama.SetokimLlamaPrefill(dict(kw, vocab_size=40)).eval()
    with pytest.raises(ValueError, match="vocabulary"):
        small.generate(inputs_embeds=x, max_new_tokens=4, beams=BeamSearch(16), eos_token_id=[1, 2])               # C = 48 > V = 40
    for extra, name in ((dict(sampler=Sampler()), "sampler="), (dict(draft=LookupDrafter(3)), "draft="),
                        (dict(return_past=True, return_dict_in_generate=True), "return_past=True")):
        with pytest.raises(NotImplementedError, match=f"beams= with {name}"):
            m.generate(inputs_embeds=x, max_new_tokens=4, beams=BeamSearch(2), **extra)
    from setok_amd.generation import GenerationState, KVCache
    state = GenerationState(cache=KVCache(1, 2, 4, 16, 16, torch.float32, "cpu"), pending=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="beams= with past="):
        m.generate(inputs_embeds=x, max_new_tokens=4, beams=BeamSearch(2), past=state)
    with pytest.raises(NotImplementedError, match="greedy"):
        m.generate(inputs_embeds=x, max_new_tokens=4, num_beams=4)     # HF's own spelling stays refused


def test_kv_cache_expanded_copies_every_row_n_times(lib):
    from setok_amd.generation import KVCache
    for fmt in KVCache.FORMATS:
        c = KVCache(2, 2, 2, 8, 4, torch.float32, "cpu", fmt)
        for layers in c._fmt.tensors:
            for t in layers:
                t.copy_(torch.randint(-100, 100, t.shape).to(t.dtype))
        c.key_mask[:, :5] = torch.tensor([[1, 1, 1, 1, 1], [0, 0, 1, 1, 1]], dtype=torch.uint8)
        c.next_pos.copy_(torch.tensor([5, 3]))
        c.len = 5
        e = c.expanded(3)
        assert (e.B, e.cap, e.len, e.kv_format, e.num_layers) == (6, 8, 5, fmt, 2)
        for new, old in zip(e._fmt.tensors, c._fmt.tensors):
            for a, b in zip(new, old):
                assert torch.equal(a[:, :, :5], b[:, :, :5].repeat_interleave(3, dim=0)) and not bool(a[:, :, 5:].any())
        assert torch.equal(e.key_mask, c.key_mask.repeat_interleave(3, dim=0)) and e.next_pos.tolist() == [5, 5, 5, 3, 3, 3]
        for n in (0, -1, 2.0, True):
            with pytest.raises(ValueError, match="expanded"):
                c.expanded(n)


# ---- the rule against HuggingFace -----------------------------------------------------------------------------------------------------------------
def load_case(golden_dir, name):
    z = golden_io.load(os.path.join(golden_dir, "beam.npz"))
    g = {k.split(":", 1)[1]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(name + ":")}
    seed, n, es, eos0, eos1, steps = (int(v) for v in g["spec"])
    g.update(seed=seed, n=n, es={v: k for k, v in BC.ES_CODE.items()}[es], eos=(eos0, eos1), steps=steps, lp=float(g["length_penalty"]))
    g["sd"] = {k[2:]: v for k, v in g.items() if isinstance(k, str) and k.startswith("w:")}
    return g


@pytest.mark.parametrize("name", list(BC.CASES))
def test_the_reference_reproduces_huggingface_on_every_fixture_case(golden_dir, name):
    g = load_case(golden_dir, name)
    n, lp, es, both = BC.CASES[name]
    assert (g["n"], g["lp"], g["es"]) == (n, lp, es) and float(g["margin"]) >= BC.MIN_MARGIN and g["eos"][0] != g["eos"][1]
    lc, sd = BC.weights(g["seed"])
    x, am, pos = BC.prompts(g["seed"])
    assert all(torch.equal(sd[k], g["sd"][k]) for k in sd) and torch.equal(x, g["x"]) and torch.equal(am, g["am"])     # the stored inputs are the seeded ones
    ref = BC.run_reference(g["sd"], lc, g["x"], g["am"], pos, n, lp, es, g["eos"])
    assert ref.margin >= BC.MIN_MARGIN and ref.steps == g["steps"] and 3 * n == ref.C
    for R, tag in ((1, "r1"), (n, "rn")):
        seq, score, anc = ref.hypotheses(R, g["eos"][0])
        assert torch.equal(seq, g[f"sequences_{tag}"]) and torch.equal(anc, g[f"beam_indices_{tag}"])
        assert float((score - g[f"scores_{tag}"]).abs().max()) <= 1e-5
        assert bool((score.view(-1, R)[:, :-1] >= score.view(-1, R)[:, 1:]).all())
    lengths = (g["beam_indices_r1"] >= 0).sum(dim=1)
    if both:
        assert bool((lengths < BC.N_NEW).any()) and bool((lengths == BC.N_NEW).any())
    for k in ("cand_score", "run", "fin_score"):
        now, then = torch.stack([t[k] for t in ref.trace]), g["trace:" + k]                              # the recorded per-step state is this run's
        assert float((now - then).abs().masked_fill(then < -1.0e8, 0.0).max()) <= 1e-5, k
