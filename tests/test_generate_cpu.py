"""KV-cached greedy generation, without a GPU: the three new C-ABI entries (setok_kv_append, setok_attention_decode_gqa, setok_argmax_rows) are
declared, exported by both builds and mirrored by the ctypes table; they validate their arguments on the host before any launch; and the
committed fixture tests/golden/generate.npz (HuggingFace LlamaForCausalLM's greedy loop with past_key_values,
tests/golden/make_golden_generate.py) has the shapes, the ids and the top-2 margins the GPU tests rely on."""
import ctypes
import glob
import os
import re
import sys

import numpy as np
import pytest

import golden_io
import llama_bwd_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"setok_kv_append": 12, "setok_attention_decode_gqa": 17, "setok_argmax_rows": 7}


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_new_entries_are_declared_exported_and_in_the_ctypes_table(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "setok_hip.h")).read(), flags=re.S)
    decls = {n: [a for a in args.split(",") if a.strip()] for n, args in re.findall(r"\bint\s+(setok_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)}
    for name, arity in NEW.items():
        assert name in decls and len(decls[name]) == arity, name
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == arity, name
        for path in (lib.LIB_PATH, lib.LIB_PATH_F16):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additive: the ABI version stays
    chunk = int(re.search(r"#define\s+SETOK_DECODE_CHUNK\s+(\d+)", text).group(1))
    from setok_amd import ops
    assert ops.DECODE_CHUNK == chunk                                  # the host sizes the workspace with the header's chunk length


@pytest.mark.parametrize("half", [False, True])
def test_null_operands_and_bad_shapes_are_refused_on_the_host(lib, half):
    l = lib.load(half)
    P = 64                                                            # a non-null, 16-byte aligned "pointer": validation fails before anything is dereferenced
    WS = 1 << 20
    # setok_attention_decode_gqa(stream, dtype, q, ldq, k, v, mask, out, B, H, Hkv, Dh, cap, len, scale, ws, ws_floats)
    # setok_kv_append(stream, dtype, qkv, k, v, B, T, H, Hkv, Dh, cap, pos0);  setok_argmax_rows(stream, dtype, x, ld, rows, V, out)
    bad = [
        ("setok_kv_append", (None, 0, None, P, P, 1, 1, 4, 2, 16, 8, 0), b"null operand"),
        ("setok_kv_append", (None, 0, P, P, None, 1, 1, 4, 2, 16, 8, 0), b"null operand"),
        ("setok_kv_append", (None, 0, P, P, P, 1, 1, 4, 3, 16, 8, 0), b"bad shape"),                          # H % Hkv
        ("setok_kv_append", (None, 0, P, P, P, 1, 1, 4, 2, 12, 8, 0), b"head dim"),
        ("setok_kv_append", (None, 0, P, P, P, 1, 4, 4, 2, 16, 8, 5), b"len > cap"),                          # slots [5, 9) of 8
        ("setok_kv_append", (None, 0, P, P, P, 1, 1, 4, 2, 16, 8, -1), b"len > cap"),
        ("setok_kv_append", (None, 0, P + 4, P, P, 1, 1, 4, 2, 16, 8, 0), b"16-byte aligned"),
        ("setok_kv_append", (None, 7, P, P, P, 1, 1, 4, 2, 16, 8, 0), b"bad dtype"),
        ("setok_attention_decode_gqa", (None, 0, None, 128, P, P, P, P, 1, 4, 2, 16, 8, 8, 0.25, P, WS), b"null operand"),
        ("setok_attention_decode_gqa", (None, 0, P, 128, P, P, None, P, 1, 4, 2, 16, 8, 8, 0.25, P, WS), b"null operand"),     # no key mask
        ("setok_attention_decode_gqa", (None, 0, P, 128, P, P, P, P, 1, 4, 2, 16, 8, 8, 0.25, None, WS), b"null operand"),     # no workspace
        ("setok_attention_decode_gqa", (None, 0, P, 128, P, P, P, P, 1, 4, 3, 16, 8, 8, 0.25, P, WS), b"bad shape"),           # H % Hkv
        ("setok_attention_decode_gqa", (None, 0, P, 128, P, P, P, P, 1, 4, 2, 12, 8, 8, 0.25, P, WS), b"head dim"),
        ("setok_attention_decode_gqa", (None, 0, P, 128, P, P, P, P, 1, 4, 2, 16, 8, 9, 0.25, P, WS), b"len > cap"),
        ("setok_attention_decode_gqa", (None, 0, P, 128, P, P, P, P, 1, 4, 2, 16, 8, 0, 0.25, P, WS), b"len"),
        ("setok_attention_decode_gqa", (None, 0, P, 32, P, P, P, P, 1, 4, 2, 16, 8, 8, 0.25, P, WS), b"16-byte aligned"),      # ldq < H * Dh
        ("setok_attention_decode_gqa", (None, 0, P, 128, P, P, P, P, 2, 4, 2, 16, 300, 300, 0.25, P, 2 * 4 * 3 * 18 - 1), b"workspace"),
        ("setok_attention_decode_gqa", (None, 7, P, 128, P, P, P, P, 1, 4, 2, 16, 8, 8, 0.25, P, WS), b"bad dtype"),
        ("setok_argmax_rows", (None, 0, None, 8, 1, 8, P), b"null operand"),
        ("setok_argmax_rows", (None, 0, P, 8, 1, 8, None), b"null operand"),
        ("setok_argmax_rows", (None, 0, P, 7, 1, 8, P), b"bad shape"),                                        # ld < V
        ("setok_argmax_rows", (None, 0, P, 8, 1, 0, P), b"bad shape"),
        ("setok_argmax_rows", (None, 7, P, 8, 0, 8, P), b"bad dtype"),
    ]
    for name, args, msg in bad:
        rc = getattr(l, name)(*args)
        assert rc == -1 and msg in l.setok_last_error(), (name, args, l.setok_last_error())
    other = 1 if half else 2                                          # the other build's 16-bit type is refused, never read as something else
    assert l.setok_kv_append(None, other, P, P, P, 1, 1, 4, 2, 16, 8, 0) == -1 and b"bad dtype" in l.setok_last_error()
    assert l.setok_attention_decode_gqa(None, other, P, 128, P, P, P, P, 1, 4, 2, 16, 8, 8, 0.25, P, WS) == -1 and b"bad dtype" in l.setok_last_error()
    assert l.setok_argmax_rows(None, other, P, 8, 0, 8, P) == -1 and b"bad dtype" in l.setok_last_error()
    # nothing to do is not an error (and launches nothing)
    assert l.setok_kv_append(None, 0, P, P, P, 0, 1, 4, 2, 16, 8, 0) == 0
    assert l.setok_attention_decode_gqa(None, 0, P, 128, P, P, P, P, 0, 4, 2, 16, 8, 8, 0.25, P, 0) == 0
    assert l.setok_argmax_rows(None, 0, P, 8, 0, 8, P) == 0


def test_generate_host_surface_without_a_gpu(lib):
    """The Python layer is importable without a GPU and carries the documented surface."""
    import inspect
    from setok_amd import generation, llama
    sig = inspect.signature(llama.SetokimLlamaPrefill.generate)
    for k, d in (("inputs", None), ("comp_images", None), ("attention_mask", None), ("position_ids", None), ("inputs_embeds", None),
                 ("max_new_tokens", 200), ("eos_token_id", None), ("pad_token_id", None), ("do_sample", False), ("return_dict_in_generate", False),
                 ("output_hidden_states", False), ("output_logits", False), ("images", None)):
        assert sig.parameters[k].default == d, k
    assert hasattr(llama.LlamaModel, "prefill") and hasattr(llama.LlamaModel, "decode_step") and hasattr(generation, "KVCache")


def test_fixture_parts_fit_the_file_limit(golden_dir):
    parts = sorted(glob.glob(os.path.join(golden_dir, "generate.part[0-9][0-9].npz"))) or [os.path.join(golden_dir, "generate.npz")]
    for p in parts:
        assert os.path.getsize(p) <= golden_io.LIMIT, (p, os.path.getsize(p))


@pytest.mark.parametrize("name", list(C.LLAMA_CASES))
def test_fixture_shapes_ids_and_margins(golden_dir, name):
    z = golden_io.load(os.path.join(golden_dir, "generate.npz"))
    kw, seed, B, T, padding = C.LLAMA_CASES[name]
    V, D = kw["vocab_size"], kw["hidden_size"]
    n = 4 if name == "7bdims" else 16
    assert [int(v) for v in z[name + ":spec"]] == [seed, B, T, 1 if padding == "left" else 0, n]
    tokens, logits, hidden, margin = z[name + ":tokens"], z[name + ":logits"], z[name + ":hidden"], z[name + ":margin"]
    assert tokens.shape == (n, B) and logits.shape == (n, B, V) and hidden.shape == (n, B, D) and margin.shape == (n, B)
    assert tokens.dtype.kind == "i" and int(tokens.min()) >= 0 and int(tokens.max()) < V
    assert np.array_equal(tokens, logits.argmax(-1))                  # greedy: every stored id is its step's argmax
    assert np.isfinite(logits).all() and np.isfinite(hidden).all()
    top2 = np.sort(logits, axis=-1)[..., -2:]
    assert np.allclose(margin, (top2[..., 1] - top2[..., 0]) / np.abs(logits).max(-1), rtol=1e-5, atol=1e-8)
    assert float(margin.min()) >= 5e-4                                # five times the fp32 logit tolerance: no step needs to be left out
    low = [k for k in z.files if k.startswith(name + ":logits_")]
    assert sorted(low) == ([name + ":logits_bf16", name + ":logits_fp16"] if name in C.DH128 else [])
    for k in low:                                                     # HF's own 16-bit runs under teacher forcing: the drift yardstick
        assert z[k].shape == logits.shape and np.isfinite(z[k]).all()
        drift = float(np.abs(z[k] - logits).max() / np.abs(logits).max())
        assert 1e-4 < drift < 5e-2, (k, drift)
