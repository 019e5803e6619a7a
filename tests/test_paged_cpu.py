"""The paged KV cache and continuous batching, without a GPU: the two entries of csrc/attn_paged.hip are declared, exported by both builds and
mirrored by the ctypes table; they refuse bad arguments on the host before any launch; `PagedKVCache`'s allocator hands pages out and takes them
back; `ContinuousBatcher` schedules by its stated rule (FIFO admission, all pages reserved up front, eos included) - driven by stubs in the place of
the two model entry points and torch stand-ins for the three ops a step calls."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"setok_kv_append_paged": 14, "setok_attention_decode_gqa_paged": 19}
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
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additive: the ABI version stays
    assert "attn_paged.hip" in open(os.path.join(ROOT, "setok_amd", "csrc", "Makefile")).read()
    assert "---- Paged KV cache (csrc/attn_paged.hip)" in raw
    page = int(re.search(r"#define\s+SETOK_KV_PAGE\s+(\d+)", raw).group(1))
    chunk = int(re.search(r"#define\s+SETOK_DECODE_CHUNK\s+(\d+)", raw).group(1))
    from setok_amd import ops
    assert page == chunk == ops.KV_PAGE == ops.DECODE_CHUNK == 128
    assert "static_assert(SETOK_KV_PAGE == SETOK_DECODE_CHUNK" in open(os.path.join(ROOT, "setok_amd", "csrc", "attn_paged.hip")).read()
    assert callable(ops.kv_append_paged) and callable(ops.attention_decode_paged) and ops.attention_decode_paged_workspace(3, 4, 16, 129) == 3 * 4 * 2 * 18


def _refused(l, fn, args_of, bad):
    for kw, msg in bad:
        rc = getattr(l, fn)(*args_of(**kw))
        assert rc == -1 and msg in l.setok_last_error(), (fn, kw, l.setok_last_error())


@pytest.mark.parametrize("half", [False, True])
def test_kv_append_paged_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1

    def args(dtype=dt, qkv=P, k_pool=P, v_pool=P, table=P, max_pages=2, num_pages=6, slot0=P, B=3, T=5, H=4, Hkv=2, Dh=64):
        return (None, dtype, qkv, k_pool, v_pool, table, max_pages, num_pages, slot0, B, T, H, Hkv, Dh)

    bad = [(dict([(k, None)]), b"null operand") for k in ("qkv", "k_pool", "v_pool", "table", "slot0")]
    bad += [(dict(dtype=1 if half else 2), b"bad dtype"), (dict(dtype=7), b"bad dtype"),
            (dict(B=-1), b"bad shape"), (dict(T=-1), b"bad shape"), (dict(H=3), b"bad shape"), (dict(max_pages=0), b"bad shape"),
            (dict(num_pages=0), b"bad shape"),
            (dict(Dh=8), b"unsupported head dim 8"), (dict(Dh=24), b"unsupported head dim 24"), (dict(Dh=512), b"unsupported head dim 512"),
            (dict(dtype=0, Dh=4), b"unsupported head dim 4"), (dict(dtype=0, Dh=256), b"unsupported head dim 256"),
            (dict(k_pool=P + 8), b"16-byte aligned"), (dict(v_pool=P + 2), b"16-byte aligned"), (dict(qkv=P + 4), b"16-byte aligned"),
            (dict(B=0, Dh=24), b"unsupported head dim 24")]                                                # ... also with nothing to do
    _refused(l, "setok_kv_append_paged", args, bad)
    assert l.setok_kv_append_paged(*args(B=0)) == 0 and l.setok_kv_append_paged(*args(T=0)) == 0          # nothing to do launches nothing


@pytest.mark.parametrize("half", [False, True])
def test_attention_decode_paged_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1

    def args(dtype=dt, q=P, ldq=512, k_pool=P, v_pool=P, table=P, max_pages=3, num_pages=12, lens=P, out=P, B=6, H=8, Hkv=2, Dh=64, max_len=300,
             scale=0.125, ws=P, ws_floats=6 * 8 * 3 * 66):
        return (None, dtype, q, ldq, k_pool, v_pool, table, max_pages, num_pages, lens, out, B, H, Hkv, Dh, max_len, scale, ws, ws_floats)

    bad = [(dict([(k, None)]), b"null operand") for k in ("q", "k_pool", "v_pool", "table", "lens", "out", "ws")]
    bad += [(dict(dtype=1 if half else 2), b"bad dtype"), (dict(dtype=7), b"bad dtype"),
            (dict(B=-1), b"bad shape"), (dict(B=65536), b"bad shape"), (dict(H=7), b"bad shape"), (dict(Hkv=0), b"bad shape"),
            (dict(max_pages=0), b"bad shape"), (dict(num_pages=0), b"bad shape"),
            (dict(Dh=8), b"unsupported head dim 8"), (dict(Dh=24), b"unsupported head dim 24"), (dict(Dh=96), b"unsupported head dim 96"),
            (dict(dtype=0, Dh=4), b"unsupported head dim 4"), (dict(dtype=0, Dh=256, ldq=2048), b"unsupported head dim 256"),
            (dict(max_len=385), b"beyond the table"), (dict(max_len=-1), b"beyond the table"), (dict(max_pages=2), b"beyond the table"),
            (dict(ws_floats=6 * 8 * 3 * 66 - 1), b"workspace of"), (dict(max_len=384, ws_floats=6 * 8 * 2 * 66), b"workspace of"),
            (dict(k_pool=P + 8), b"16-byte aligned"), (dict(v_pool=P + 2), b"16-byte aligned"), (dict(q=P + 4), b"16-byte aligned"),
            (dict(ldq=511), b"16-byte aligned"), (dict(ldq=504), b"16-byte aligned"),
            (dict(B=0, max_len=385), b"beyond the table")]                                                 # ... also with nothing to do
    _refused(l, "setok_attention_decode_gqa_paged", args, bad)
    assert l.setok_attention_decode_gqa_paged(*args(B=0)) == 0                                             # nothing to do launches nothing
    assert l.setok_attention_decode_gqa_paged(*args(B=0, max_len=384)) == 0                                # the whole table, to its last slot


# ---- the allocator -------------------------------------------------------------------------------------------------------------------------------
def _cache(rows=3, num_pages=5, max_pages=3):
    from setok_amd.generation import PagedKVCache
    return PagedKVCache(1, rows, 1, 8, torch.float32, "cpu", num_pages, max_pages)


def _consistent(c):
    """The device table and lengths equal their host mirrors; no page is owned twice or both owned and free."""
    assert c.block_table.tolist() == c.table_host and c.lens.tolist() == c.lens_host
    owned = [p for row in c.table_host for p in row if p >= 0]
    assert len(set(owned)) == len(owned) and not set(owned) & set(c._free) and sorted(owned + c._free) == list(range(c.num_pages))
    assert c.pages_free == len(c._free)


def test_paged_cache_starts_idle_and_sized_as_stated():
    c = _cache()
    assert c.k[0].shape == c.v[0].shape == (5, 1, 128, 8) and c.block_table.dtype == c.lens.dtype == torch.int32
    assert c.block_table.tolist() == [[-1] * 3] * 3 and c.lens.tolist() == [0] * 3 and c.pages_free == 5
    assert c.nbytes() == 2 * 5 * 128 * 8 * 4 and c.page_nbytes == 2 * 128 * 8 * 4
    _consistent(c)
    from setok_amd.generation import PagedKVCache
    for kw in (dict(rows=0), dict(num_pages=0), dict(max_pages=0), dict(rows=True), dict(num_pages=2.0)):
        with pytest.raises(ValueError, match="PagedKVCache"):
            _cache(**kw)
    assert PagedKVCache.for_model                                      # the model-shaped constructor exists


def test_assign_and_release_round_trip_the_free_list():
    c = _cache()
    assert c.assign(0, 129) is True and c.pages_of(0) == [0, 1] and c.pages_free == 3          # ceil(129 / 128) pages
    assert c.assign(2, 128) is True and c.pages_of(2) == [2] and c.pages_free == 2
    assert c.table_host == [[0, 1, -1], [-1, -1, -1], [2, -1, -1]]                             # an idle row's entries are all -1
    _consistent(c)
    c.set_len(0, 129)
    assert c.lens.tolist() == [129, 0, 0]
    c.release(0)
    assert c.pages_free == 4 and c.table_host[0] == [-1] * 3 and c.lens.tolist() == [0, 0, 0] and sorted(c._free) == [0, 1, 3, 4]
    _consistent(c)
    c.release(2)
    assert sorted(c._free) == list(range(5)) and c.block_table.tolist() == [[-1] * 3] * 3
    _consistent(c)


def test_a_request_the_pool_cannot_serve_returns_false_and_changes_nothing():
    c = _cache()
    assert c.assign(0, 384)                                            # 3 of 5 pages
    table, free = [list(r) for r in c.table_host], list(c._free)
    assert c.assign(1, 257) is False                                   # 3 more: only 2 are free
    assert c.table_host == table and c._free == free and c.block_table.tolist() == table and c.lens_host == [0] * 3
    _consistent(c)
    assert c.assign(1, 256) is True and c.pages_free == 0              # what is there can still be had
    assert c.assign(2, 1) is False
    _consistent(c)


def test_released_pages_are_handed_out_again_and_bad_calls_raise():
    c = _cache()
    assert c.assign(0, 300) and c.assign(1, 200)                       # pages [0, 1, 2] and [3, 4]
    assert c.assign(2, 1) is False
    c.release(0)
    assert c.assign(2, 384) and sorted(c.pages_of(2)) == [0, 1, 2]     # the released pages, again
    _consistent(c)
    with pytest.raises(ValueError, match="is idle"):
        c.release(0)                                                   # double release
    with pytest.raises(ValueError, match="already owns pages"):
        c.assign(1, 10)
    with pytest.raises(ValueError, match="max_pages_per_seq"):
        c.assign(0, 385)                                               # 4 pages: more than a table row holds
    for bad in (-1, 3, True, 1.0):
        with pytest.raises(ValueError, match="row="):
            c.assign(bad, 10)
        with pytest.raises(ValueError, match="row="):
            c.release(bad)
    with pytest.raises(ValueError, match="n_slots"):
        c.assign(0, 0)
    _consistent(c)


# ---- the scheduler -------------------------------------------------------------------------------------------------------------------------------
D, V, EOS = 64, 100, 63


def _scripted_batcher(monkeypatch, scripts, **kw):
    """A ContinuousBatcher on the CPU whose model entry points are stubs: request i is recognised by its prompt (x[0, 0] == i) and emits scripts[i] -
    a state whose lm_head row argmax is the scripted token.  ops.linear / argmax_rows / splice_rows are torch stand-ins, so lm_head, the selection
    and the embedding lookup of a step are the batcher's own calls."""
    from setok_amd import llama, ops
    from setok_amd.generation import ContinuousBatcher
    lm = llama.SetokimLlamaPrefill(dict(hidden_size=D, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4,
                                        vocab_size=V)).eval()
    with torch.no_grad():
        lm.lm_head.weight.zero_()
        lm.lm_head.weight[:D] = torch.eye(D)                           # state = one-hot(token) -> logits = one-hot(token)
    monkeypatch.setattr(ops, "linear", lambda a, w, **_: a @ w.T)
    monkeypatch.setattr(ops, "argmax_rows", lambda x, out=None: x.argmax(-1))
    monkeypatch.setattr(ops, "splice_rows", lambda src, table, img, status=None: table[src.long()])
    log = dict(prefills=[], decodes=[], fed=[])
    where = {}                                                         # row -> [request, tokens emitted]

    def onehot(tok):
        return torch.nn.functional.one_hot(torch.tensor(tok), D).float()

    def prefill_paged(x, cache, row):
        i = int(x[0, 0, 0])
        assert x.shape[0] == 1 and cache.lens_host[row] == 0 and len(cache.pages_of(row)) * 128 >= x.shape[1]
        cache.set_len(row, x.shape[1])
        where[row] = [i, 1]
        log["prefills"].append((i, row))
        h = torch.zeros(1, x.shape[1], D)
        h[0, -1] = onehot(scripts[i][0])
        return h

    def decode_step_paged(x, cache, active, active_host=None):
        assert active.tolist() == list(active_host) and x.shape == (cache.rows, D)
        log["decodes"].append(list(active_host))
        h = torch.zeros(cache.rows, D)
        for row, on in enumerate(active_host):
            if on:
                i, n = where[row]
                log["fed"].append((i, x[row].tolist() == lm.model.embed_tokens.weight[scripts[i][n - 1]].tolist()))
                h[row] = onehot(scripts[i][n])
                where[row][1] += 1
                cache.lens_host[row] += 1
        cache.lens = torch.tensor(cache.lens_host, dtype=torch.int32)
        return h

    monkeypatch.setattr(lm.model, "prefill_paged", prefill_paged)
    monkeypatch.setattr(lm.model, "decode_step_paged", decode_step_paged)
    return ContinuousBatcher(lm, **kw), log


def _prompt(i, T):
    x = torch.zeros(T, D)
    x[0, 0] = i
    return x


def test_the_batcher_admits_in_fifo_order_waits_for_pages_and_counts_what_happened(monkeypatch):
    # (prompt length, max_new_tokens) -> pages: A 130 -> 2, B 13 -> 1, E 7 -> 1, C 170 -> 2, D 7 -> 1; the pool has 3
    shapes = [(100, 30), (10, 3), (5, 2), (150, 20), (5, 2)]
    scripts = [[(7 * i + j) % 60 for j in range(n + 1)] for i, (_, n) in enumerate(shapes)]
    scripts[3][4] = EOS                                                # C's fifth token is an eos: it ends there, the eos included
    b, log = _scripted_batcher(monkeypatch, scripts, rows=2, num_pages=3, max_pages_per_seq=2, eos_token_id=EOS)
    tickets = [b.submit(_prompt(i, T), n) for i, (T, n) in enumerate(shapes)]
    assert tickets == [0, 1, 2, 3, 4] and len(b.queue) == 5 and b.cache.pages_free == 3            # submit touches nothing but the queue
    finished, order = {}, []
    while b.queue or any(r is not None for r in b.running):
        for ticket, toks in b.step():
            finished[ticket] = toks
            order.append((ticket, b.stats["steps"]))
    # step 1: A and B start together.  B ends in step 2 (3 tokens: one from its prefill, one per step).  Step 3: E joins A mid-flight on B's page and
    # ends at once (2 tokens).  Steps 4 .. 29: row 1 is idle but C, the queue's head, needs 2 pages and 1 is free - and D, which would fit, does
    # not overtake.  A ends in step 29 (30 tokens); step 30 admits C and D; D ends in it; C ends on its eos in step 33.
    assert [i for i, _ in log["prefills"]] == [0, 1, 2, 3, 4]                                       # FIFO
    assert order == [(1, 2), (2, 3), (0, 29), (4, 30), (3, 33)]
    assert log["prefills"] == [(0, 0), (1, 1), (2, 1), (3, 0), (4, 1)]
    for i, (T, n) in enumerate(shapes):
        want = scripts[i][:5] if i == 3 else scripts[i][:n]
        assert finished[i].dtype == torch.int64 and finished[i].tolist() == want
    assert finished[3].tolist()[-1] == EOS and len(finished[3]) == 5 < shapes[3][1]                 # the eos is included, nothing follows it
    assert all(ok for _, ok in log["fed"])                                                          # every step was fed the row's own previous token
    assert log["decodes"] == [[True, True]] * 3 + [[True, False]] * 26 + [[True, True]] + [[True, False]] * 3
    assert b.stats == dict(steps=33, row_steps_active=37, row_steps_total=66, pages_high_water=3, admitted=5, admitted_midflight=1, page_waits=26,
                           pages_reused=4)
    assert b.occupancy == 37 / 66
    assert b.cache.pages_free == 3 and b.cache.table_host == [[-1, -1]] * 2 and b.cache.lens.tolist() == [0, 0]
    assert b.step() == []                                                                           # drained: a step does nothing


def test_run_returns_the_tokens_in_submit_order_and_a_single_token_request_never_decodes(monkeypatch):
    shapes = [(3, 4), (200, 1), (2, 2)]
    scripts = [[10, 11, 12, 13, 14], [20, 21], [30, 31, 32]]
    b, log = _scripted_batcher(monkeypatch, scripts, rows=2, num_pages=4)
    assert b.cache.max_pages_per_seq == 4                              # the default: a sequence may take the whole pool
    out = b.run([(_prompt(i, T), n) for i, (T, n) in enumerate(shapes)])
    assert [o.tolist() for o in out] == [[10, 11, 12, 13], [20], [30, 31]]
    assert log["decodes"][0] == [True, False]                          # request 1 (max_new_tokens = 1) ended on its prefill's token
    ids = torch.arange(5)
    b2, log2 = _scripted_batcher(monkeypatch, {0: [1, 2, 3]}, rows=1, num_pages=1)
    with torch.no_grad():
        b2.lm.model.embed_tokens.weight[0, 0] = 0.0                    # the ids' first embedding row names request 0 to the stub
        b2.w_e = b2.lm.model.embed_tokens.weight.detach().contiguous()
    assert [o.tolist() for o in b2.run([(ids, 2)])] == [[1, 2]] and b2.submit(input_ids=ids, max_new_tokens=1) == 1


def test_submit_and_the_constructor_refuse_by_name(monkeypatch):
    from setok_amd.generation import BeamSearch, ContinuousBatcher, LogitsProcessors, LookupDrafter, Sampler
    b, _ = _scripted_batcher(monkeypatch, {}, rows=2, num_pages=3, max_pages_per_seq=2)
    for prompt, n, msg in ((_prompt(0, 250), 7, "need 3 pages"), (_prompt(0, 1), 256, "need 3 pages"), (torch.zeros(4, D + 1), 2, "is not"),
                           (torch.zeros(4), 2, "is not"), (torch.zeros(0, D), 2, "empty prompt"), (torch.zeros(2, 3, dtype=torch.int64), 2, "is not"),
                           (_prompt(0, 3), 0, "max_new_tokens"), (_prompt(0, 3), True, "max_new_tokens"), (None, 2, "one of them")):
        with pytest.raises(ValueError, match=msg):
            b.submit(prompt, n)
    b1, _ = _scripted_batcher(monkeypatch, {}, rows=2, num_pages=1, max_pages_per_seq=2)
    with pytest.raises(ValueError, match="num_pages = 1"):
        b1.submit(_prompt(0, 100), 29)                                 # fits a table row, never the pool
    assert b.queue == [] and b1.queue == [] and b.cache.pages_free == 3 and b.cache.table_host == [[-1, -1]] * 2
    for kw, name in ((dict(sampler=Sampler()), "sampler="), (dict(beams=BeamSearch(2)), "beams="), (dict(draft=LookupDrafter(2)), "draft="),
                     (dict(processors=LogitsProcessors(1.3)), "processors="), (dict(prefill_chunk=64), "prefill_chunk="),
                     (dict(kv_cache="fp8"), "kv_cache='fp8'"), (dict(kv_cache="mxfp4"), "kv_cache='mxfp4'")):
        with pytest.raises(NotImplementedError, match=name):
            ContinuousBatcher(b.lm, 2, 3, **kw)
    with pytest.raises(ValueError, match="kv_cache"):
        ContinuousBatcher(b.lm, 2, 3, kv_cache="int4")
    for args in ((0, 3), (2, 0), (2, 3, 0)):
        with pytest.raises(ValueError, match="ContinuousBatcher"):
            ContinuousBatcher(b.lm, *args)
