"""Extending a filled KV cache by several tokens, without a GPU: setok_attention_extend_gqa and SETOK_EXTEND_CHUNK are declared, exported by both
builds and mirrored by the ctypes table; the host computes the workspace by the header's formula; the entry point validates its arguments on the host
before any launch; and `generate` refuses bad `prefill_chunk` / `return_past` / `past` arguments before it touches a device."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"setok_attention_extend_gqa": 18, "setok_attention_extend_workspace": 7}


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "setok_hip.h")).read(), flags=re.S)


def test_extend_entries_are_declared_exported_and_in_the_ctypes_table(lib):
    text = _header()
    decls = {n: [a for a in args.split(",") if a.strip()]
             for n, args in re.findall(r"\b(?:int64_t|int)\s+(setok_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)}
    for name, arity in NEW.items():
        assert name in decls and len(decls[name]) == arity, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == arity, name
        for path in (lib.LIB_PATH, lib.LIB_PATH_F16):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {os.path.basename(path)}"
    # the signature the issue fixes: (stream, dtype, q, ldq, k_cache, v_cache, key_mask, out, B, Tn, H, Hkv, Dh, cap, len0, scale, workspace, workspace_floats)
    names = [a.split()[-1].lstrip("*") for a in decls["setok_attention_extend_gqa"]]
    assert names == ["stream", "dtype", "q", "ldq", "k_cache", "v_cache", "key_mask", "out", "B", "Tn", "H", "Hkv", "Dh", "cap", "len0", "scale",
                     "workspace", "workspace_floats"]
    assert lib.RESTYPES["setok_attention_extend_workspace"] is ctypes.c_int64
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additive: the ABI version stays
    chunk = int(re.search(r"#define\s+SETOK_EXTEND_CHUNK\s+(\d+)", text).group(1))
    from setok_amd import ops
    assert ops.EXTEND_CHUNK == chunk and chunk % 32 == 0              # the host sizes the workspace with the header's chunk length


def test_the_header_states_the_counting_rule():
    raw = " ".join(open(os.path.join(ROOT, "include", "setok_hip.h")).read().replace(" * ", " ").split())
    for sentence in ("Query i of sequence b counts slot j iff j <= len0 + i and key_mask[b][j] != 0.",
                     "A query with no counted key gets zeros.",
                     "Slots that do not count are never allowed to reach the output, whatever bytes they hold."):
        assert sentence in raw, sentence


@pytest.mark.parametrize("half", [False, True])
def test_workspace_formula(lib, half):
    from setok_amd import ops
    C = ops.EXTEND_CHUNK
    l = lib.load(half)
    for B, Tn, H, Dh, len0 in ((1, 1, 1, 8, 0), (4, 5, 8, 128, 0), (1, 8, 32, 128, 2048), (3, 17, 4, 40, C - 8), (2, 1, 2, 16, C - 1), (2, 1, 2, 16, C),
                               (8, 512, 32, 128, 1536), (5, 9, 8, 64, 1000)):
        want = B * Tn * H * -(-(len0 + Tn) // C) * (Dh + 2)           # the header's formula
        assert ops.attention_extend_workspace(B, Tn, H, Dh, len0) == want
        assert l.setok_attention_extend_workspace(0, B, Tn, H, H, Dh, len0) == want
        for Hkv, dt in ((H, torch.float32), (1, torch.float32), (H, torch.float16 if half else torch.bfloat16)):
            assert ops.attention_extend_workspace(B, Tn, H, Dh, len0, Hkv, dt) <= want      # the formula suffices for every path
    # the MFMA path with more than 32 stacked rows needs a partial per SETOK_EXTEND_SPAN chunks only; every other path the header's formula
    span = int(re.search(r"#define\s+SETOK_EXTEND_SPAN\s+(\d+)", _header()).group(1))
    low = torch.float16 if half else torch.bfloat16
    assert ops.attention_extend_workspace(4, 512, 32, 128, 1536, 32, low) == 4 * 512 * 32 * -(-2048 // (span * C)) * 130
    assert ops.attention_extend_workspace(4, 5, 32, 128, 1536, 4, low) == 4 * 5 * 32 * -(-1541 // (span * C)) * 130            # G * Tn = 40 > 32
    assert ops.attention_extend_workspace(1, 8, 32, 128, 2048, 32, low) == ops.attention_extend_workspace(1, 8, 32, 128, 2048)
    assert ops.attention_extend_workspace(4, 512, 32, 128, 1536, 32, torch.float32) == ops.attention_extend_workspace(4, 512, 32, 128, 1536)
    assert ops.attention_extend_workspace(4, 512, 32, 64, 1536, 32, torch.float16) == ops.attention_extend_workspace(4, 512, 32, 64, 1536)
    assert l.setok_attention_extend_workspace(0, 64, 4096, 64, 64, 128, 0) == ops.attention_extend_workspace(64, 4096, 64, 128, 0) \
        == 64 * 4096 * 64 * 16 * 130 > 2 ** 31                        # 64-bit: a long chunk's count does not fit an int
    assert l.setok_attention_extend_workspace(0, 1, 2, 4, 3, 16, 0) == 0      # H % Hkv: a shape the entry point refuses


@pytest.mark.parametrize("half", [False, True])
def test_extend_arguments_are_refused_on_the_host(lib, half):
    l = lib.load(half)
    P, WS = 64, 1 << 20                                               # a non-null, 16-byte aligned "pointer": validation fails before anything is dereferenced
    f = l.setok_attention_extend_gqa
    # (stream, dtype, q, ldq, k, v, mask, out, B, Tn, H, Hkv, Dh, cap, len0, scale, ws, ws_floats)
    bad = [
        ((None, 0, None, 128, P, P, P, P, 1, 2, 4, 2, 16, 8, 3, 0.25, P, WS), b"null operand"),
        ((None, 0, P, 128, P, P, None, P, 1, 2, 4, 2, 16, 8, 3, 0.25, P, WS), b"null operand"),       # no key mask
        ((None, 0, P, 128, P, P, P, P, 1, 2, 4, 2, 16, 8, 3, 0.25, None, WS), b"null operand"),       # no workspace
        ((None, 0, P, 128, P, P, P, P, 1, 2, 4, 3, 16, 8, 3, 0.25, P, WS), b"bad shape"),             # H % Hkv
        ((None, 0, P, 128, P, P, P, P, 1, 0, 4, 2, 16, 8, 3, 0.25, P, WS), b"bad shape"),             # Tn < 1
        ((None, 0, P, 128, P, P, P, P, 1, 2, 4, 2, 12, 8, 3, 0.25, P, WS), b"head dim"),
        ((None, 0, P, 128, P, P, P, P, 1, 2, 4, 2, 16, 8, 7, 0.25, P, WS), b"len0 + Tn > cap"),       # slots [7, 9) of 8
        ((None, 0, P, 128, P, P, P, P, 1, 2, 4, 2, 16, 8, -1, 0.25, P, WS), b"len0 + Tn > cap"),
        ((None, 0, P, 32, P, P, P, P, 1, 2, 4, 2, 16, 8, 3, 0.25, P, WS), b"16-byte aligned"),        # ldq < H * Dh
        ((None, 0, P, 128, P, P, P, P, 1, 2, 4, 2, 16, 8, 3, 0.25, P + 4, WS), b"8-byte aligned"),
        ((None, 0, P, 128, P, P, P, P, 2, 3, 4, 2, 16, 600, 510, 0.25, P, 2 * 3 * 4 * 3 * 18 - 1), b"workspace"),
        ((None, 2 if half else 1, P, 512, P, P, P, P, 1, 40, 4, 2, 128, 2000, 1500, 0.25, P, 40 * 4 * 2 * 130 - 1), b"workspace"),      # the MFMA path's span: 2 partials per row
        ((None, 0, P, 512, P, P, P, P, 1, 40, 4, 2, 128, 2000, 1500, 0.25, P, 40 * 4 * 7 * 130 - 1), b"workspace"),                      # fp32: a partial per chunk, 7
        ((None, 7, P, 128, P, P, P, P, 1, 2, 4, 2, 16, 8, 3, 0.25, P, WS), b"bad dtype"),
        ((None, 1 if half else 2, P, 128, P, P, P, P, 1, 2, 4, 2, 16, 8, 3, 0.25, P, WS), b"bad dtype"),      # the other build's 16-bit type
    ]
    for args, msg in bad:
        assert f(*args) == -1 and msg in l.setok_last_error(), (args, l.setok_last_error())
    assert f(None, 0, P, 128, P, P, P, P, 0, 2, 4, 2, 16, 8, 3, 0.25, P, 0) == 0      # nothing to do is not an error (and launches nothing)


def test_generate_validates_the_new_arguments_before_any_device_call(lib):
    from setok_amd import generation
    from setok_amd.llama import LlamaModel, SetokimLlamaPrefill
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    m = SetokimLlamaPrefill(kw).eval()                                # on the CPU: anything that reached a kernel would raise something else
    x = torch.zeros(2, 5, 64)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="prefill_chunk"):
            m.generate(inputs_embeds=x, max_new_tokens=2, prefill_chunk=bad)
    with pytest.raises(ValueError, match="cache_capacity"):
        m.generate(inputs_embeds=x, max_new_tokens=2, cache_capacity=0)
    with pytest.raises(ValueError, match="return_dict_in_generate"):
        m.generate(inputs_embeds=x, max_new_tokens=2, return_past=True)
    with pytest.raises(TypeError, match="GenerationState"):
        m.generate(inputs_embeds=x, max_new_tokens=2, past=object())
    with pytest.raises(TypeError, match="GenerationState"):
        m.generate(inputs_embeds=x, max_new_tokens=2, past=generation.KVCache(1, 2, 4, 8, 16, torch.float32, "cpu"))      # the cache alone is not a state
    state = generation.GenerationState(cache=generation.KVCache(1, 2, 4, 8, 16, torch.float32, "cpu"), pending=torch.full((2,), -1, dtype=torch.int64))
    with pytest.raises(ValueError, match="position_ids"):
        m.generate(inputs_embeds=x, max_new_tokens=2, past=state, position_ids=torch.zeros(2, 5, dtype=torch.int64))
    f8 = generation.GenerationState(cache=generation.KVCache(1, 2, 4, 8, 16, torch.float32, "cpu", kv_format="fp8"), pending=state.pending)
    with pytest.raises(NotImplementedError, match="fp8"):
        m.generate(inputs_embeds=x, max_new_tokens=2, past=f8)
    assert state.cache.len == 0 and f8.cache.len == 0                 # refused without being touched
    assert hasattr(LlamaModel, "extend") and hasattr(generation.KVCache, "extend_attend")
    import inspect
    sig = inspect.signature(SetokimLlamaPrefill.generate)
    for k, d in (("prefill_chunk", None), ("return_past", False), ("past", None), ("cache_capacity", None)):
        assert sig.parameters[k].default == d, k
    assert "past" in generation.GenerateOutput.__dataclass_fields__


@pytest.mark.parametrize("name", ["gqa_tiny_left", "gqa_dh128"])
def test_extend_fixture_shapes_and_mask(golden_dir, name):
    """tests/golden/extend.npz: HuggingFace's states for a ragged masked chunk appended to past_key_values (make_golden_extend.py)."""
    import numpy as np
    import golden_io
    import llama_bwd_cases as C
    sys.path.insert(0, golden_dir)
    from make_golden_extend import TN, chunk_inputs
    path = os.path.join(golden_dir, "extend.npz")
    assert os.path.getsize(path) <= golden_io.LIMIT
    z = golden_io.load(path)
    kw, _, B, _, _ = C.LLAMA_CASES[name]
    chunk, cm = chunk_inputs(name)
    assert chunk.shape == (B, TN, kw["hidden_size"]) and np.array_equal(z[name + ":chunk_mask"], cm.numpy())
    assert z[name + ":hidden"].shape == (B, TN, kw["hidden_size"]) and z[name + ":logits"].shape == (B, TN, kw["vocab_size"])
    assert np.isfinite(z[name + ":hidden"]).all() and np.isfinite(z[name + ":logits"]).all()
    assert int(cm.sum()) < B * TN and bool((cm.sum(1) > 0).all()) and int(cm[B - 1, -2:].sum()) == 0      # ragged, with a hole; no empty sequence
