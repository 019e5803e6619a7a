"""MXFP4 pages without a GPU: the entries of "Paged MXFP4 KV cache" are declared, exported by both builds and mirrored by the ctypes table, and
refuse bad arguments on the host before any launch; `PagedKVCache` builds the nibble and scale pools it states and refuses the formats and head
dims it cannot serve; `ContinuousBatcher(cache=)` takes a fresh cache of the caller's and nothing else - over the scripted-batcher stub of
test_paged_cpu.py."""
import ctypes
import os
import re
import sys

import pytest
import torch

from test_paged_cpu import _prompt, _refused, _scripted_batcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"setok_kv_append_paged_mxfp4": 16, "setok_attention_decode_gqa_paged_mxfp4kv": 21, "setok_attention_extend_gqa_paged_mxfp4kv": 22}
P = 4096                                           # stands in for device pointers: nothing is dereferenced


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def test_the_entries_are_declared_exported_and_in_the_ctypes_table(lib):
    raw = open(os.path.join(ROOT, "include", "setok_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    decls = {n: [a for a in args.split(",") if a.strip()] for n, args in re.findall(r"\bint\s+(setok_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)}
    for name, arity in ENTRIES.items():
        assert name in decls and len(decls[name]) == arity
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == arity
        for path in (lib.LIB_PATH, lib.LIB_PATH_F16):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {os.path.basename(path)}"
    assert "---- Paged MXFP4 KV cache (csrc/attn_paged.hip, csrc/attn_extend_paged.hip)" in raw
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additive: the ABI version stays
    page = int(re.search(r"#define\s+SETOK_KV_PAGE\s+(\d+)", raw).group(1))
    chunk = int(re.search(r"#define\s+SETOK_DECODE_CHUNK_MXFP4KV\s+(\d+)", raw).group(1))
    from setok_amd import ops
    assert chunk == 2 * page == ops.DECODE_CHUNK_MXFP4KV == 2 * ops.KV_PAGE                          # a chunk's workgroup covers two pages
    assert ops.attention_decode_paged_mxfp4kv_workspace(3, 4, 32, 257) == 3 * 4 * 2 * 34
    for half in (False, True):
        l = lib.load(half)
        assert l.setok_attention_extend_paged_mxfp4kv_workspace(2, 5, 4, 96, 300) == 2 * 5 * 4 * 2 * 98 == ops.attention_extend_paged_mxfp4kv_workspace(2, 5, 4, 96, 300)


@pytest.mark.parametrize("half", [False, True])
def test_kv_append_paged_mxfp4_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1

    def args(dtype=dt, qkv=P, k_q=P, k_s=P, v_q=P, v_s=P, table=P, max_pages=2, num_pages=6, slot0=P, B=3, T=5, H=4, Hkv=2, Dh=64):
        return (None, dtype, qkv, k_q, k_s, v_q, v_s, table, max_pages, num_pages, slot0, B, T, H, Hkv, Dh)

    bad = [(dict([(k, None)]), b"null operand") for k in ("qkv", "k_q", "k_s", "v_q", "v_s", "table", "slot0")]
    bad += [(dict(dtype=1 if half else 2), b"bad dtype"), (dict(dtype=7), b"bad dtype"),
            (dict(B=-1), b"bad shape"), (dict(T=-1), b"bad shape"), (dict(H=3), b"bad shape"), (dict(max_pages=0), b"bad shape"),
            (dict(num_pages=0), b"bad shape"),
            (dict(Dh=16), b"unsupported head dim 16"), (dict(Dh=48), b"unsupported head dim 48"), (dict(Dh=96), b"unsupported head dim 96"),
            (dict(dtype=0, Dh=256), b"unsupported head dim 256"),
            (dict(k_q=P + 8), b"16-byte aligned"), (dict(v_q=P + 2), b"16-byte aligned"), (dict(qkv=P + 4), b"16-byte aligned"),
            (dict(B=0, Dh=48), b"unsupported head dim 48")]                                                # ... also with nothing to do
    _refused(l, "setok_kv_append_paged_mxfp4", args, bad)
    assert l.setok_kv_append_paged_mxfp4(*args(B=0)) == 0 and l.setok_kv_append_paged_mxfp4(*args(T=0)) == 0      # nothing to do launches nothing
    assert l.setok_kv_append_paged_mxfp4(*args(B=0, k_s=P + 1, v_s=P + 3)) == 0                                    # scale bytes need no alignment


@pytest.mark.parametrize("half", [False, True])
def test_attention_decode_paged_mxfp4kv_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1

    def args(dtype=dt, q=P, ldq=512, k_q=P, k_s=P, v_q=P, v_s=P, table=P, max_pages=3, num_pages=12, lens=P, out=P, B=6, H=8, Hkv=2, Dh=64, max_len=300,
             scale=0.125, ws=P, ws_floats=6 * 8 * 2 * 66):
        return (None, dtype, q, ldq, k_q, k_s, v_q, v_s, table, max_pages, num_pages, lens, out, B, H, Hkv, Dh, max_len, scale, ws, ws_floats)

    bad = [(dict([(k, None)]), b"null operand") for k in ("q", "k_q", "k_s", "v_q", "v_s", "table", "lens", "out", "ws")]
    bad += [(dict(dtype=1 if half else 2), b"bad dtype"), (dict(dtype=7), b"bad dtype"),
            (dict(B=-1), b"bad shape"), (dict(B=65536), b"bad shape"), (dict(H=7), b"bad shape"), (dict(Hkv=0), b"bad shape"),
            (dict(max_pages=0), b"bad shape"), (dict(num_pages=0), b"bad shape"),
            (dict(Dh=16), b"unsupported head dim 16"), (dict(Dh=48), b"unsupported head dim 48"), (dict(Dh=96, ldq=768), b"unsupported head dim 96"),
            (dict(dtype=0, Dh=256, ldq=2048), b"unsupported head dim 256"),
            (dict(max_len=385), b"beyond the table"), (dict(max_len=-1), b"beyond the table"), (dict(max_pages=2), b"beyond the table"),
            (dict(ws_floats=6 * 8 * 2 * 66 - 1), b"workspace of"),                                         # ceil(300 / 256) = 2 partials per head
            (dict(max_len=256, ws_floats=6 * 8 * 66 - 1), b"workspace of"),
            (dict(k_q=P + 8), b"16-byte aligned"), (dict(v_q=P + 2), b"16-byte aligned"), (dict(q=P + 4), b"16-byte aligned"),
            (dict(ldq=511), b"16-byte aligned"), (dict(ldq=504), b"16-byte aligned"),
            (dict(B=0, max_len=385), b"beyond the table")]                                                 # ... also with nothing to do
    _refused(l, "setok_attention_decode_gqa_paged_mxfp4kv", args, bad)
    assert l.setok_attention_decode_gqa_paged_mxfp4kv(*args(B=0)) == 0                                     # nothing to do launches nothing
    assert l.setok_attention_decode_gqa_paged_mxfp4kv(*args(B=0, max_len=384)) == 0                        # the whole table, to its last slot: still 2 chunks
    assert l.setok_attention_decode_gqa_paged_mxfp4kv(*args(B=0, max_len=256, ws_floats=6 * 8 * 66)) == 0  # one chunk covers two pages


@pytest.mark.parametrize("half", [False, True])
def test_attention_extend_paged_mxfp4kv_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1
    need = 6 * 5 * 8 * 2 * 98                                          # B * Tn * H * ceil((300 + 5) / 256) * (Dh + 2)

    def args(dtype=dt, q=P, ldq=1536, k_q=P, k_s=P, v_q=P, v_s=P, table=P, max_pages=3, num_pages=12, len0=P, out=P, B=6, Tn=5, H=8, Hkv=2, Dh=96,
             max_len0=300, scale=0.125, ws=P, ws_floats=need):
        return (None, dtype, q, ldq, k_q, k_s, v_q, v_s, table, max_pages, num_pages, len0, out, B, Tn, H, Hkv, Dh, max_len0, scale, ws, ws_floats)

    bad = [(dict([(k, None)]), b"null operand") for k in ("q", "k_q", "k_s", "v_q", "v_s", "table", "len0", "out", "ws")]
    bad += [(dict(dtype=1 if half else 2), b"bad dtype"), (dict(dtype=7), b"bad dtype"),
            (dict(B=-1), b"bad shape"), (dict(Tn=0), b"bad shape"), (dict(H=7), b"bad shape"), (dict(max_pages=0), b"bad shape"), (dict(num_pages=0), b"bad shape"),
            (dict(Dh=16), b"unsupported head dim 16"), (dict(Dh=48), b"unsupported head dim 48"), (dict(Dh=0), b"unsupported head dim 0"),
            (dict(max_len0=380), b"beyond the table"), (dict(max_len0=-1), b"beyond the table"), (dict(max_pages=2), b"beyond the table"),
            (dict(ws_floats=need - 1), b"workspace of"),
            (dict(k_q=P + 8), b"16-byte aligned"), (dict(v_q=P + 2), b"16-byte aligned"), (dict(q=P + 4), b"16-byte aligned"), (dict(ldq=1532), b"16-byte aligned"),
            (dict(B=0, max_len0=380), b"beyond the table")]
    _refused(l, "setok_attention_extend_gqa_paged_mxfp4kv", args, bad)
    assert l.setok_attention_extend_gqa_paged_mxfp4kv(*args(B=0)) == 0                                     # every multiple of 32 is a head dim; nothing to do launches nothing
    assert l.setok_attention_extend_gqa_paged_mxfp4kv(*args(B=0, max_len0=379)) == 0                       # the new rows end on the table's last slot


# ---- the cache -----------------------------------------------------------------------------------------------------------------------------------
def _cache(Dh=64, kv_format="mxfp4", rows=3, num_pages=5, max_pages=3, layers=2, Hkv=2):
    from setok_amd.generation import PagedKVCache
    return PagedKVCache(layers, rows, Hkv, Dh, torch.float32, "cpu", num_pages, max_pages, kv_format)


@pytest.mark.parametrize("Dh", [32, 64, 128])
def test_an_mxfp4_paged_cache_holds_nibble_and_scale_pools_and_is_sized_as_stated(Dh):
    c = _cache(Dh)
    assert c.kv_format == "mxfp4" and c.k == [] and c.v == []
    for pools, cols in ((c.k_q, Dh // 2), (c.v_q, Dh // 2), (c.k_s, Dh // 32), (c.v_s, Dh // 32)):
        assert len(pools) == 2 and all(t.shape == (5, 2, 128, cols) and t.dtype == torch.uint8 for t in pools)
    assert c.nbytes() == 2 * 2 * 5 * 2 * 128 * (Dh // 2 + Dh // 32) == 5 * c.page_nbytes
    assert c.block_table.tolist() == [[-1] * 3] * 3 and c.lens.tolist() == [0] * 3 and c.pages_free == 5 and c.fresh
    assert c.assign(1, 200) and not c.fresh                            # the allocator does not depend on the format
    c.release(1)
    assert c.fresh and c.page_refs == [0] * 5
    n = _cache(Dh, "native")                                           # the default format is what it was
    assert n.kv_format == "native" and n.k[0].shape == (5, 2, 128, Dh) and n.nbytes() == 2 * 2 * 5 * 2 * 128 * Dh * 4 == 5 * n.page_nbytes
    assert not hasattr(n, "k_q")


def test_the_paged_cache_refuses_the_formats_and_head_dims_it_cannot_serve():
    from setok_amd.generation import PagedKVCache
    with pytest.raises(ValueError, match="multiple of 32"):
        _cache(48)
    for Dh in (96, 256):                                               # whole MX blocks, but no lane layout in the decode attention over nibble rows
        with pytest.raises(ValueError, match="32, 64 or 128"):
            _cache(Dh)
    with pytest.raises(NotImplementedError, match="kv_format='fp8'"):
        _cache(64, "fp8")
    with pytest.raises(ValueError, match="kv_format='int4'"):
        _cache(64, "int4")
    assert _cache(48, "native").k[0].shape == (5, 2, 128, 48)          # the native pools take what they took
    import inspect
    assert inspect.signature(PagedKVCache.for_model).parameters["kv_format"].default == "native"
    assert inspect.signature(PagedKVCache.__init__).parameters["kv_format"].default == "native"


# ---- the batcher's cache= --------------------------------------------------------------------------------------------------------------------------
def _lm_cache(lm, rows=2, num_pages=3, max_pages=2, kv_format="native"):
    from setok_amd.generation import PagedKVCache
    return PagedKVCache.for_model(lm.model, rows, num_pages, max_pages, device="cpu", kv_format=kv_format)


def test_the_batcher_schedules_over_a_cache_of_the_callers(monkeypatch):
    scripts = [[10, 11, 12, 13, 14], [20, 21], [30, 31, 32]]
    b0, _ = _scripted_batcher(monkeypatch, scripts, rows=2, num_pages=4)
    cache = _lm_cache(b0.lm, 2, 4, 4)
    b, log = _scripted_batcher(monkeypatch, scripts, rows=2, cache=cache)
    assert b.cache is cache
    out = b.run([(_prompt(i, T), n) for i, (T, n) in enumerate(((3, 4), (200, 1), (2, 2)))])
    assert [o.tolist() for o in out] == [[10, 11, 12, 13], [20], [30, 31]]
    assert cache.fresh and b.stats["admitted"] == 3
    # the stated sizes may be repeated, as long as they are the cache's
    b2, _ = _scripted_batcher(monkeypatch, scripts, rows=2, num_pages=4, max_pages_per_seq=4, cache=cache)
    assert b2.cache is cache


def test_the_batcher_refuses_a_used_or_conflicting_cache_and_the_format_strings(monkeypatch):
    from setok_amd.generation import ContinuousBatcher
    b, _ = _scripted_batcher(monkeypatch, {}, rows=2, num_pages=3, max_pages_per_seq=2)
    lm = b.lm
    used = _lm_cache(lm)
    assert used.assign(0, 10)
    with pytest.raises(ValueError, match="must be fresh"):
        ContinuousBatcher(lm, 2, cache=used)
    used.set_len(0, 10)
    pages = used.detach(0)                                             # every row idle, but a page is still held
    with pytest.raises(ValueError, match="must be fresh"):
        ContinuousBatcher(lm, 2, cache=used)
    used.drop(pages)
    assert ContinuousBatcher(lm, 2, cache=used).cache is used          # everything given back: fresh again
    for kw, name in ((dict(num_pages=4), "num_pages=4"), (dict(max_pages_per_seq=3), "max_pages_per_seq=3"), (dict(num_pages=True), "num_pages=True")):
        with pytest.raises(ValueError, match=f"{name} conflicts with cache="):
            ContinuousBatcher(lm, 2, cache=_lm_cache(lm), **kw)
    with pytest.raises(ValueError, match="rows=3 conflicts with cache="):
        ContinuousBatcher(lm, 3, cache=_lm_cache(lm))
    with pytest.raises(TypeError, match="PagedKVCache"):
        ContinuousBatcher(lm, 2, cache=object())
    from setok_amd.generation import PagedKVCache
    other = PagedKVCache(3, 2, 4, 16, torch.float32, "cpu", 3, 2)      # three layers: not this model's
    with pytest.raises(ValueError, match="was not built for this model"):
        ContinuousBatcher(lm, 2, cache=other)
    with pytest.raises(ValueError, match="num_pages"):
        ContinuousBatcher(lm, 2)                                       # neither a pool size nor a cache
    # the strings stay refused, and the message says where MXFP4 pages come from
    with pytest.raises(NotImplementedError, match=r"kv_cache='mxfp4'.*cache=PagedKVCache\.for_model\(.*kv_format=\"mxfp4\"\)"):
        ContinuousBatcher(lm, 2, 3, kv_cache="mxfp4")
    with pytest.raises(NotImplementedError, match="kv_cache='fp8'"):
        ContinuousBatcher(lm, 2, 3, kv_cache="fp8")
    with pytest.raises(ValueError, match="kv_cache"):
        ContinuousBatcher(lm, 2, 3, kv_cache="int4")
    with pytest.raises(ValueError, match="multiple of 32"):
        _lm_cache(lm, kv_format="mxfp4")                               # the stub model's head dim is 16
