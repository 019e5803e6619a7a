"""The fp8 KV cache without a GPU: setok_kv_append_fp8 and setok_attention_decode_gqa_fp8kv refuse bad arguments on the host, before any launch
(include/setok_hip.h, "FP8 KV cache"), and the Python surface — KVCache(kv_format=...), generate(kv_cache=...) — checks its arguments."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4096        # stands in for a device pointer: the calls below are refused before anything is launched or dereferenced
CHUNK = 256     # SETOK_DECODE_CHUNK_FP8KV


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _append(dtype, qkv=P, k_q=P, k_e=P, v_q=P, v_e=P, B=2, T=3, H=4, Hkv=2, Dh=64, cap=9, pos0=2):
    return (None, dtype, qkv, k_q, k_e, v_q, v_e, B, T, H, Hkv, Dh, cap, pos0)


def _attend(dtype, q=P, ldq=None, k_q=P, k_e=P, v_q=P, v_e=P, mask=P, out=P, B=2, H=4, Hkv=2, Dh=64, cap=600, n=600, ws=P, ws_floats=None):
    ldq = (H + 2 * Hkv) * Dh if ldq is None else ldq
    need = B * H * ((n + CHUNK - 1) // CHUNK) * (Dh + 2)
    return (None, dtype, q, ldq, k_q, k_e, v_q, v_e, mask, out, B, H, Hkv, Dh, cap, n, 0.125, ws, need if ws_floats is None else ws_floats)


def test_the_chunk_constant_is_exported_and_mirrored():
    sys.path.insert(0, ROOT)
    from setok_amd import ops
    text = open(os.path.join(ROOT, "include", "setok_hip.h")).read()
    assert f"#define SETOK_DECODE_CHUNK_FP8KV {CHUNK}" in text and ops.DECODE_CHUNK_FP8KV == CHUNK
    assert ops.attention_decode_workspace(2, 4, 64, 600, ops.DECODE_CHUNK_FP8KV) == 2 * 4 * 3 * 66
    assert ops.attention_decode_workspace(2, 4, 64, 600) == 2 * 4 * 5 * 66                 # the native call's is unchanged


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kw,msg", [
    (dict(qkv=None), b"null operand"), (dict(k_q=None), b"null operand"), (dict(k_e=None), b"null operand"),
    (dict(v_q=None), b"null operand"), (dict(v_e=None), b"null operand"),
    (dict(H=5), b"bad shape"),                           # H % Hkv != 0
    (dict(Dh=60), b"unsupported head dim 60"),           # Dh % 8 != 0
    (dict(pos0=7), b"exceed the cache"),                 # pos0 + T > cap
    (dict(pos0=-1), b"exceed the cache"),
    (dict(qkv=P + 8), b"16-byte aligned"), (dict(k_q=P + 4), b"16-byte aligned"), (dict(v_q=P + 2), b"16-byte aligned"),
])
def test_kv_append_fp8_refuses_on_the_host(lib, half, kw, msg):
    l = lib.load(half)
    dt = 2 if half else 1
    for dtype in (0, dt):
        assert l.setok_kv_append_fp8(*_append(dtype, **kw)) == -1, kw
        err = l.setok_last_error()
        assert b"setok_kv_append_fp8" in err and msg in err, err


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kw,msg", [
    (dict(q=None), b"null operand"), (dict(k_q=None), b"null operand"), (dict(k_e=None), b"null operand"), (dict(v_q=None), b"null operand"),
    (dict(v_e=None), b"null operand"), (dict(mask=None), b"null operand"), (dict(out=None), b"null operand"), (dict(ws=None), b"null operand"),
    (dict(H=5), b"bad shape"),
    (dict(Dh=60), b"unsupported head dim 60"),
    (dict(n=0), b"outside [1, cap"), (dict(n=601), b"outside [1, cap"),
    (dict(ws_floats=2 * 4 * 3 * 66 - 1), b"workspace of"),
    (dict(ws_floats=2 * 4 * 2 * 66), b"workspace of"),   # what len = 512 needs: one chunk short
    (dict(q=P + 8), b"16-byte aligned"), (dict(k_q=P + 8), b"16-byte aligned"), (dict(v_q=P + 4), b"16-byte aligned"),
    (dict(ldq=4 * 64 - 8), b"16-byte aligned"),          # a q row shorter than H * Dh
    (dict(ldq=8 * 64 + 4), b"16-byte aligned"),          # rows that do not start on 16 bytes
])
def test_attention_decode_fp8kv_refuses_on_the_host(lib, half, kw, msg):
    l = lib.load(half)
    dt = 2 if half else 1
    for dtype in (0, dt):
        assert l.setok_attention_decode_gqa_fp8kv(*_attend(dtype, **kw)) == -1, kw
        err = l.setok_last_error()
        assert b"setok_attention_decode_fp8kv" in err and msg in err, err


def test_each_build_refuses_a_bad_dtype(lib):
    for half, bad in ((False, 2), (True, 1), (False, 7), (True, -1)):        # the other build's 16-bit type, and codes that name nothing
        l = lib.load(half)
        assert l.setok_kv_append_fp8(*_append(bad)) == -1 and b"bad dtype" in l.setok_last_error()
        assert l.setok_attention_decode_gqa_fp8kv(*_attend(bad)) == -1 and b"bad dtype" in l.setok_last_error()


def test_kvcache_fp8_shapes_dtypes_and_bytes_on_the_cpu():
    sys.path.insert(0, ROOT)
    from setok_amd import ops
    from setok_amd.generation import KVCache
    layers, B, Hkv, cap, Dh = 3, 2, 4, 300, 64
    c = KVCache(layers, B, Hkv, cap, Dh, torch.bfloat16, "cpu", kv_format="fp8")
    assert c.kv_format == "fp8" and c.dtype == torch.bfloat16 and c.num_layers == layers and c.len == 0
    for q, e in ((c.k_q, c.k_e), (c.v_q, c.v_e)):
        assert len(q) == len(e) == layers
        for t in q:
            assert t.shape == (B, Hkv, cap, Dh) and t.dtype == torch.uint8 and not t.any()
        for t in e:
            assert t.shape == (B, Hkv, cap) and t.dtype == torch.int8 and not t.any()
    assert c.k == [] and c.v == []
    assert c.nbytes() == 2 * layers * B * Hkv * cap * (Dh + 1)
    assert c.key_mask.shape == (B, cap) and c.key_mask.dtype == torch.uint8 and c.next_pos.shape == (B,)
    assert c.workspace(8).numel() == ops.attention_decode_workspace(B, 8, Dh, cap, ops.DECODE_CHUNK_FP8KV) == B * 8 * 2 * (Dh + 2)
    n = KVCache(layers, B, Hkv, cap, Dh, torch.bfloat16, "cpu")                          # the default is today's cache
    assert n.kv_format == "native" and n.k[0].shape == (B, Hkv, cap, Dh) and n.k[0].dtype == torch.bfloat16 and len(n.v) == layers
    assert n.nbytes() == 2 * layers * B * Hkv * cap * Dh * 2 and not hasattr(n, "k_q")
    assert n.workspace(8).numel() == B * 8 * 3 * (Dh + 2)
    with pytest.raises(ValueError, match="'native', 'fp8'"):
        KVCache(layers, B, Hkv, cap, Dh, torch.bfloat16, "cpu", kv_format="int4")


def test_generate_names_the_accepted_cache_formats():
    sys.path.insert(0, ROOT)
    from setok_amd.llama import SetokimLlamaPrefill
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4, vocab_size=100)
    m = SetokimLlamaPrefill(kw).eval()
    x = torch.zeros(2, 5, 64)
    with pytest.raises(ValueError, match="'native', 'fp8'"):
        m.generate(inputs_embeds=x, max_new_tokens=2, kv_cache="int4")
    with pytest.raises(ValueError, match="'native', 'fp8'"):
        m.generate(inputs_embeds=x, max_new_tokens=2, kv_cache=None)
