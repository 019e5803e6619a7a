"""The MXFP4 KV cache without a GPU: setok_kv_append_mxfp4, setok_attention_decode_gqa_mxfp4kv and setok_attention_extend_gqa_mxfp4kv are declared,
exported and refuse bad arguments on the host, before any launch (include/setok_hip.h, "MXFP4 KV cache"), and the Python surface —
KVCache(kv_format="mxfp4"), generate(kv_cache="mxfp4") — allocates and checks what the header states."""
import os
import re
import sys

import pytest
import torch

import mxfp4kv_cases as K

ROOT = K.ROOT
P = 4096        # stands in for a device pointer: the calls below are refused before anything is launched or dereferenced
CHUNK = K.define("SETOK_DECODE_CHUNK_MXFP4KV")
XC = K.define("SETOK_EXTEND_CHUNK")
SYMBOLS = {"setok_kv_append_mxfp4": 14, "setok_attention_decode_gqa_mxfp4kv": 19, "setok_attention_extend_gqa_mxfp4kv": 20}


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _append(dtype, qkv=P, k_q=P, k_s=P, v_q=P, v_s=P, B=2, T=3, H=4, Hkv=2, Dh=64, cap=9, pos0=2):
    return (None, dtype, qkv, k_q, k_s, v_q, v_s, B, T, H, Hkv, Dh, cap, pos0)


def _attend(dtype, q=P, ldq=None, k_q=P, k_s=P, v_q=P, v_s=P, mask=P, out=P, B=2, H=4, Hkv=2, Dh=64, cap=600, n=600, ws=P, ws_floats=None):
    ldq = (H + 2 * Hkv) * Dh if ldq is None else ldq
    need = B * H * ((n + CHUNK - 1) // CHUNK) * (Dh + 2)
    return (None, dtype, q, ldq, k_q, k_s, v_q, v_s, mask, out, B, H, Hkv, Dh, cap, n, 0.125, ws, need if ws_floats is None else ws_floats)


def _extend(dtype, q=P, ldq=None, k_q=P, k_s=P, v_q=P, v_s=P, mask=P, out=P, B=2, Tn=3, H=4, Hkv=2, Dh=64, cap=600, len0=597, ws=P, ws_floats=None):
    ldq = (H + 2 * Hkv) * Dh if ldq is None else ldq
    need = B * Tn * H * ((len0 + Tn + XC - 1) // XC) * (Dh + 2)
    return (None, dtype, q, ldq, k_q, k_s, v_q, v_s, mask, out, B, Tn, H, Hkv, Dh, cap, len0, 0.125, ws, need if ws_floats is None else ws_floats)


def test_the_symbols_are_declared_and_exported_with_the_headers_argument_counts(lib):
    text = open(os.path.join(ROOT, "include", "setok_hip.h")).read()
    for name, nargs in SYMBOLS.items():
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", text)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == nargs == len(lib.SIGNATURES[name]), name
        for half in (False, True):
            assert hasattr(lib.load(half), name), (name, half)
    assert re.search(r"\bint64_t setok_attention_extend_mxfp4kv_workspace\(int B, int Tn, int H, int Dh, int len0\);", text)
    for half in (False, True):
        assert lib.load(half).setok_attention_extend_mxfp4kv_workspace(2, 3, 4, 64, 597) == 2 * 3 * 4 * 3 * 66
        assert lib.load(half).setok_attention_extend_mxfp4kv_workspace(2, 0, 4, 64, 597) == 0
    assert "#define SETOK_ABI_VERSION 9" in text                       # pure additions


def test_the_chunk_constant_is_exported_and_mirrored():
    sys.path.insert(0, ROOT)
    from setok_amd import ops
    assert ops.DECODE_CHUNK_MXFP4KV == CHUNK and ops.EXTEND_CHUNK == XC
    assert ops.attention_decode_workspace(2, 4, 64, 600, ops.DECODE_CHUNK_MXFP4KV) == 2 * 4 * ((600 + CHUNK - 1) // CHUNK) * 66
    assert ops.attention_extend_mxfp4kv_workspace(2, 3, 4, 64, 597) == 2 * 3 * 4 * ((600 + XC - 1) // XC) * 66
    assert ops.attention_decode_workspace(2, 4, 64, 600) == 2 * 4 * 5 * 66                 # the native call's is unchanged


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kw,msg", [
    (dict(qkv=None), b"null operand"), (dict(k_q=None), b"null operand"), (dict(k_s=None), b"null operand"),
    (dict(v_q=None), b"null operand"), (dict(v_s=None), b"null operand"),
    (dict(H=5), b"bad shape"),                           # H % Hkv != 0
    (dict(Dh=60), b"unsupported head dim 60"),           # Dh % 8 != 0
    (dict(Dh=48), b"unsupported head dim 48"),           # Dh % 32 != 0: no whole number of MX blocks
    (dict(Dh=16), b"unsupported head dim 16"),
    (dict(Dh=544), b"unsupported head dim 544"),         # more than 512
    (dict(pos0=7), b"exceed the cache"),                 # pos0 + T > cap
    (dict(pos0=-1), b"exceed the cache"),
    (dict(qkv=P + 8), b"16-byte aligned"), (dict(k_q=P + 4), b"16-byte aligned"), (dict(v_q=P + 2), b"16-byte aligned"),
])
def test_kv_append_mxfp4_refuses_on_the_host(lib, half, kw, msg):
    l = lib.load(half)
    dt = 2 if half else 1
    for dtype in (0, dt):
        assert l.setok_kv_append_mxfp4(*_append(dtype, **kw)) == -1, kw
        err = l.setok_last_error()
        assert b"setok_kv_append_mxfp4" in err and msg in err, err


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), b"null operand"), (dict(k_q=None), b"null operand"), (dict(k_s=None), b"null operand"), (dict(v_q=None), b"null operand"),
    (dict(v_s=None), b"null operand"), (dict(mask=None), b"null operand"), (dict(out=None), b"null operand"), (dict(ws=None), b"null operand"),
    (dict(H=5), b"bad shape"),
    (dict(Dh=60), b"unsupported head dim 60"),
    (dict(Dh=48), b"unsupported head dim 48"),
    (dict(Dh=16), b"unsupported head dim 16"),
    (dict(n=0), b"outside [1, cap"), (dict(n=601), b"outside [1, cap"),
    (dict(ws_floats=2 * 4 * ((600 + CHUNK - 1) // CHUNK) * 66 - 1), b"workspace of"),
    (dict(ws_floats=2 * 4 * ((600 + CHUNK - 1) // CHUNK - 1) * 66), b"workspace of"),   # one chunk short
    (dict(q=P + 8), b"16-byte aligned"), (dict(k_q=P + 8), b"16-byte aligned"), (dict(v_q=P + 4), b"16-byte aligned"),
    (dict(ldq=4 * 64 - 8), b"16-byte aligned"),          # a q row shorter than H * Dh
    (dict(ldq=8 * 64 + 4), b"16-byte aligned"),          # rows that do not start on 16 bytes
])
def test_attention_decode_mxfp4kv_refuses_on_the_host(lib, half, kw, msg):
    l = lib.load(half)
    dt = 2 if half else 1
    for dtype in (0, dt):
        assert l.setok_attention_decode_gqa_mxfp4kv(*_attend(dtype, **kw)) == -1, kw
        err = l.setok_last_error()
        assert b"setok_attention_decode_mxfp4kv" in err and msg in err, err


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), b"null operand"), (dict(k_q=None), b"null operand"), (dict(k_s=None), b"null operand"), (dict(v_q=None), b"null operand"),
    (dict(v_s=None), b"null operand"), (dict(mask=None), b"null operand"), (dict(out=None), b"null operand"), (dict(ws=None), b"null operand"),
    (dict(H=5), b"bad shape"), (dict(Tn=0), b"bad shape"),
    (dict(Dh=60), b"unsupported head dim 60"),
    (dict(Dh=48), b"unsupported head dim 48"),
    (dict(len0=598), b"exceed the cache"), (dict(len0=-1), b"exceed the cache"),
    (dict(ws_floats=2 * 3 * 4 * ((600 + XC - 1) // XC) * 66 - 1), b"workspace of"),
    (dict(q=P + 8), b"16-byte aligned"), (dict(k_q=P + 8), b"16-byte aligned"), (dict(v_q=P + 4), b"16-byte aligned"),
    (dict(ldq=4 * 64 - 8), b"16-byte aligned"),
    (dict(ldq=8 * 64 + 4), b"16-byte aligned"),
])
def test_attention_extend_mxfp4kv_refuses_on_the_host(lib, half, kw, msg):
    l = lib.load(half)
    dt = 2 if half else 1
    for dtype in (0, dt):
        assert l.setok_attention_extend_gqa_mxfp4kv(*_extend(dtype, **kw)) == -1, kw
        err = l.setok_last_error()
        assert b"setok_attention_extend_mxfp4kv" in err and msg in err, err


def test_each_build_refuses_a_bad_dtype(lib):
    for half, bad in ((False, 2), (True, 1), (False, 7), (True, -1)):        # the other build's 16-bit type, and codes that name nothing
        l = lib.load(half)
        assert l.setok_kv_append_mxfp4(*_append(bad)) == -1 and b"bad dtype" in l.setok_last_error()
        assert l.setok_attention_decode_gqa_mxfp4kv(*_attend(bad)) == -1 and b"bad dtype" in l.setok_last_error()
        assert l.setok_attention_extend_gqa_mxfp4kv(*_extend(bad)) == -1 and b"bad dtype" in l.setok_last_error()


def test_kvcache_mxfp4_shapes_dtypes_bytes_and_workspaces_on_the_cpu():
    sys.path.insert(0, ROOT)
    from setok_amd import ops
    from setok_amd.generation import KVCache
    assert KVCache.FORMATS == ("native", "fp8", "mxfp4")
    layers, B, Hkv, cap, Dh = 3, 2, 4, 300, 64
    c = KVCache(layers, B, Hkv, cap, Dh, torch.bfloat16, "cpu", kv_format="mxfp4")
    assert c.kv_format == "mxfp4" and c.dtype == torch.bfloat16 and c.num_layers == layers and c.len == 0
    for q, s in ((c.k_q, c.k_s), (c.v_q, c.v_s)):
        assert len(q) == len(s) == layers
        for t in q:
            assert t.shape == (B, Hkv, cap, Dh // 2) and t.dtype == torch.uint8 and not t.any()
        for t in s:
            assert t.shape == (B, Hkv, cap, Dh // 32) and t.dtype == torch.uint8 and not t.any()
    assert c.k == [] and c.v == []
    assert c.nbytes() == 2 * layers * B * Hkv * cap * (Dh // 2 + Dh // 32)
    assert c.key_mask.shape == (B, cap) and c.key_mask.dtype == torch.uint8 and c.next_pos.shape == (B,)
    H = 8
    assert c.workspace(H).numel() == ops.attention_decode_workspace(B, H, Dh, cap, CHUNK) == B * H * ((cap + CHUNK - 1) // CHUNK) * (Dh + 2)
    Tn, len0 = 40, 250                                                 # an extend's partials outgrow the decode step's: one per chunk of XC slots, in every type
    assert c.workspace(H, Tn, len0).numel() == B * Tn * H * ((len0 + Tn + XC - 1) // XC) * (Dh + 2)
    odd = KVCache(1, 2, 1, 5, 4, torch.float32, "cpu", kv_format="mxfp4")          # the constructor rounds up and leaves Dh % 32 to for_model / generate / C
    assert odd.k_q[0].shape == (2, 1, 5, 2) and odd.k_s[0].shape == (2, 1, 5, 1)
    assert KVCache(1, 2, 1, 5, 33, torch.float32, "cpu", kv_format="mxfp4").v_s[0].shape == (2, 1, 5, 2)
    g = c.grown(cap + 7)                                               # the format can be extended: it can be grown, and keeps its format
    assert g.kv_format == "mxfp4" and g.cap == cap + 7 and g.k_q[0].shape == (B, Hkv, cap + 7, Dh // 2)
    with pytest.raises(ValueError, match="'native', 'fp8', 'mxfp4'"):
        KVCache(layers, B, Hkv, cap, Dh, torch.bfloat16, "cpu", kv_format="int4")


def test_generate_and_for_model_refuse_a_head_dim_without_whole_blocks_before_any_device_call(monkeypatch):
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    from setok_amd.generation import KVCache
    from setok_amd.llama import SetokimLlamaPrefill
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    m = SetokimLlamaPrefill(kw).eval()
    assert m.model.head_dim == 16
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: calls.append(name))
    x = torch.zeros(2, 5, 64)
    with pytest.raises(ValueError, match="mxfp4.*multiple of 32"):
        m.generate(inputs_embeds=x, max_new_tokens=2, kv_cache="mxfp4")
    with pytest.raises(ValueError, match="mxfp4.*multiple of 32"):
        KVCache.for_model(m.model, 2, 9, "cpu", kv_format="mxfp4")
    assert calls == []
    with pytest.raises(ValueError, match="'native', 'fp8', 'mxfp4'"):
        m.generate(inputs_embeds=x, max_new_tokens=2, kv_cache="int4")
