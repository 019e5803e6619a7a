"""The paged extend attention and prefix sharing, without a GPU: the two entries of csrc/attn_extend_paged.hip are declared, exported by both builds
and mirrored by the ctypes table; the attention refuses bad arguments on the host before any launch and its workspace rule is the dense one;
`PagedKVCache` counts its pages by reference (`assign(shared=)`, `release`, `detach`, `drop`); `ContinuousBatcher` prefills a registered prefix
once and runs only the remainder of a request that names it - driven by stubs in the place of the three model entry points."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"setok_attention_extend_paged_workspace": 7, "setok_attention_extend_gqa_paged": 20}
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
    decls = {n: [a for a in args.split(",") if a.strip()] for n, args in re.findall(r"\bint(?:64_t)?\s+(setok_\w+)\s*\(([^;]*)\)\s*;", text, flags=re.S)}
    for name, arity in ENTRIES.items():
        assert name in decls and len(decls[name]) == arity
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name]) == arity
        for path in (lib.LIB_PATH, lib.LIB_PATH_F16):
            assert hasattr(ctypes.CDLL(path), name), f"{name} not exported by {os.path.basename(path)}"
    assert lib.RESTYPES["setok_attention_extend_paged_workspace"] is ctypes.c_int64
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additive: the ABI version stays
    assert "attn_extend_paged.hip" in open(os.path.join(ROOT, "setok_amd", "csrc", "Makefile")).read()
    assert "---- Paged extend attention (csrc/attn_extend_paged.hip)" in raw
    from setok_amd import ops
    assert callable(ops.attention_extend_paged) and callable(ops.attention_extend_paged_workspace)


@pytest.mark.parametrize("half", [False, True])
def test_the_workspace_rule_is_the_dense_one_at_max_len0(lib, half):
    l = lib.load(half)
    low = 2 if half else 1
    for dtype in (0, low):
        for B, Tn, H, Hkv, Dh, n in ((3, 8, 8, 2, 128, 1020), (3, 9, 8, 2, 128, 1020),       # G * Tn = 32 and 36: on both sides of the span rule
                                     (1, 88, 32, 32, 128, 512), (8, 8, 32, 32, 128, 2048), (2, 40, 8, 2, 64, 300), (2, 1, 4, 4, 16, 0), (0, 5, 4, 4, 16, 7)):
            got = l.setok_attention_extend_paged_workspace(dtype, B, Tn, H, Hkv, Dh, n)
            assert got == l.setok_attention_extend_workspace(dtype, B, Tn, H, Hkv, Dh, n)
            span = 1024 if dtype == low and Dh == 128 and (H // Hkv) * Tn > 32 else 256
            assert got == B * Tn * H * ((n + Tn + span - 1) // span) * (Dh + 2)
    assert l.setok_attention_extend_paged_workspace(low, 3, 8, 8, 2, 128, 1020) == 3 * 8 * 8 * 5 * 130
    assert l.setok_attention_extend_paged_workspace(low, 3, 9, 8, 2, 128, 1020) == 3 * 9 * 8 * 2 * 130
    from setok_amd import ops
    dt = torch.float16 if half else torch.bfloat16
    assert ops.attention_extend_paged_workspace(3, 9, 8, 128, 1020, 2, dt) == 3 * 9 * 8 * 2 * 130
    assert ops.attention_extend_paged_workspace(3, 9, 8, 128, 1020) == 3 * 9 * 8 * 5 * 130            # without Hkv and dtype: what suffices for every call


@pytest.mark.parametrize("half", [False, True])
def test_attention_extend_paged_refuses_bad_arguments_on_the_host(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1
    need = 6 * 5 * 8 * 2 * 66                                          # B * Tn * H * ceil((300 + 5) / 256) * (Dh + 2)

    def args(dtype=dt, q=P, ldq=512, k_pool=P, v_pool=P, table=P, max_pages=3, num_pages=12, len0=P, out=P, B=6, Tn=5, H=8, Hkv=2, Dh=64, max_len0=300,
             scale=0.125, ws=P, ws_floats=need):
        return (None, dtype, q, ldq, k_pool, v_pool, table, max_pages, num_pages, len0, out, B, Tn, H, Hkv, Dh, max_len0, scale, ws, ws_floats)

    bad = [(dict([(k, None)]), b"null operand") for k in ("q", "k_pool", "v_pool", "table", "len0", "out", "ws")]
    bad += [(dict(dtype=1 if half else 2), b"bad dtype"), (dict(dtype=7), b"bad dtype"),
            (dict(B=-1), b"bad shape"), (dict(B=65536), b"bad shape"), (dict(Tn=0), b"bad shape"), (dict(H=7), b"bad shape"), (dict(Hkv=0), b"bad shape"),
            (dict(max_pages=0), b"bad shape"), (dict(num_pages=0), b"bad shape"),
            (dict(Dh=8), b"unsupported head dim 8"), (dict(Dh=24), b"unsupported head dim 24"), (dict(Dh=96), b"unsupported head dim 96"),
            (dict(dtype=0, Dh=4), b"unsupported head dim 4"), (dict(dtype=0, Dh=256, ldq=2048), b"unsupported head dim 256"),
            (dict(max_len0=380), b"beyond the table"), (dict(max_len0=-1), b"beyond the table"), (dict(max_pages=2), b"beyond the table"),
            (dict(Tn=85), b"beyond the table"),
            (dict(B=65535, Tn=128, H=512, Hkv=512, max_pages=4), b"exceed the launch grid"),                # B * Tn * H rows
            (dict(Tn=129, H=65535, Hkv=65535, ldq=65535 * 64, max_pages=4), b"exceed the launch grid"),      # Hkv * row blocks (two per head at 129 rows)
            (dict(max_len0=65536 * 256, max_pages=1 << 18, B=0), b"exceed the launch grid"),                # chunks
            (dict(ws_floats=need - 1), b"workspace of"), (dict(max_len0=512, max_pages=5, ws_floats=need), b"workspace of"),
            (dict(ws=P + 4), b"8-byte aligned"),
            (dict(k_pool=P + 8), b"16-byte aligned"), (dict(v_pool=P + 2), b"16-byte aligned"), (dict(q=P + 4), b"16-byte aligned"),
            (dict(ldq=511), b"16-byte aligned"), (dict(ldq=504), b"16-byte aligned"),
            (dict(B=0, max_len0=380), b"beyond the table")]                                                # ... also with nothing to do
    for kw, msg in bad:
        rc = l.setok_attention_extend_gqa_paged(*args(**kw))
        assert rc == -1 and msg in l.setok_last_error() and b"setok_attention_extend_paged" in l.setok_last_error(), (kw, l.setok_last_error())
    assert l.setok_attention_extend_gqa_paged(*args(B=0)) == 0                                             # nothing to do launches nothing
    assert l.setok_attention_extend_gqa_paged(*args(B=0, max_len0=379, ws_floats=0)) == 0                  # the whole table, to its last slot


# ---- the allocator -------------------------------------------------------------------------------------------------------------------------------
def _cache(rows=3, num_pages=6, max_pages=3):
    from setok_amd.generation import PagedKVCache
    return PagedKVCache(1, rows, 1, 8, torch.float32, "cpu", num_pages, max_pages)


def _consistent(c, held=()):
    """The device table and lengths equal their host mirrors; a page is free with count 0 and on the free list once, or its count equals the table
    entries that hold it plus the references `detach` handed out (`held`: those the test still holds)."""
    assert c.block_table.tolist() == c.table_host and c.lens.tolist() == c.lens_host
    entries = [p for row in c.table_host for p in row if p >= 0]
    assert len(c.page_refs) == c.num_pages and c.pages_free == len(c._free) == len(set(c._free))
    for p in range(c.num_pages):
        refs = entries.count(p) + list(held).count(p)
        assert c.page_refs[p] == refs and (p in c._free) == (refs == 0), (p, refs, c.page_refs, c._free)


def test_assign_shared_points_rows_at_held_pages_and_counts_them():
    c = _cache()
    assert c.page_refs == [0] * 6
    assert c.assign(0, 256) and c.page_refs == [1, 1, 0, 0, 0, 0]
    c.set_len(0, 256)
    held = c.detach(0)                                                 # the row is idle again, its pages are the caller's
    assert held == [0, 1] and c.table_host[0] == [-1] * 3 and c.lens_host[0] == 0 and c.pages_free == 4 and c.page_refs[:2] == [1, 1]
    _consistent(c, held)
    assert c.assign(1, 300, shared=held) and c.table_host[1] == [0, 1, 2] and c.page_refs == [2, 2, 1, 0, 0, 0] and c.pages_free == 3
    assert c.assign(2, 257, shared=held[:1]) and c.table_host[2] == [0, 3, 4] and c.page_refs == [3, 2, 1, 1, 1, 0]      # one shared page, two of its own
    _consistent(c, held)
    c.release(1)                                                       # only its own page goes back: the shared ones are still held
    assert c._free == [5, 2] and c.page_refs == [2, 1, 0, 1, 1, 0]
    _consistent(c, held)
    c.drop(held)                                                       # page 1 had no other holder; page 0 is still row 2's
    assert c._free == [5, 2, 1] and c.page_refs == [1, 0, 0, 1, 1, 0]
    _consistent(c)
    c.release(2)                                                       # table order: 0, 3, 4
    assert c._free == [5, 2, 1, 0, 3, 4] and c.page_refs == [0] * 6
    _consistent(c)


def test_a_failed_or_refused_assign_changes_nothing():
    c = _cache(num_pages=4)
    assert c.assign(0, 128)
    held = c.detach(0)
    assert c.assign(1, 384, shared=held)                               # pages [0, 1, 2]: one free page left
    state = lambda: ([list(r) for r in c.table_host], list(c._free), list(c.page_refs), c.block_table.tolist(), list(c.lens_host))
    before = state()
    assert c.assign(2, 384, shared=held) is False and state() == before                 # two of its own: only one is free
    with pytest.raises(ValueError, match="not a page somebody holds"):
        c.assign(2, 200, shared=[3])                                                    # a free page cannot be shared
    with pytest.raises(ValueError, match="not a page somebody holds"):
        c.assign(2, 200, shared=[4])                                                    # nor can a page id out of range
    with pytest.raises(ValueError, match="not a page somebody holds"):
        c.assign(2, 200, shared=[-1])
    for n_slots in (128, 100, 1):
        with pytest.raises(ValueError, match="must own the page it writes to"):
            c.assign(2, n_slots, shared=held)                                           # len(shared) * 128 >= n_slots
    with pytest.raises(ValueError, match="max_pages_per_seq"):
        c.assign(2, 385, shared=held)
    with pytest.raises(ValueError, match="already owns pages"):
        c.assign(1, 200, shared=held)
    assert state() == before
    _consistent(c, held)
    assert c.assign(2, 129, shared=held) and c.pages_free == 0
    _consistent(c, held)


def test_detach_and_drop_refuse_what_would_break_the_counts():
    c = _cache()
    with pytest.raises(ValueError, match="is idle"):
        c.detach(0)
    for bad in (-1, 3, True, 1.0):
        with pytest.raises(ValueError, match="row="):
            c.detach(bad)
    assert c.assign(0, 200) and c.assign(1, 10)
    held = c.detach(0)
    _consistent(c, held)
    before = (list(c._free), list(c.page_refs))
    for pages, msg in (([6], "outside"), ([-1], "outside"), ([True], "outside"), ([3], "references"), ([0, 0], "references"), ([0, 1, 5], "references")):
        with pytest.raises(ValueError, match=msg):
            c.drop(pages)
        assert (list(c._free), list(c.page_refs)) == before            # nothing changed, not even for the good ids of a bad list
    c.drop(held)
    assert c._free == [3, 4, 5, 0, 1]
    with pytest.raises(ValueError, match="references"):
        c.drop(held)                                                   # double drop
    _consistent(c)
    c.drop([])
    c.release(1)
    assert sorted(c._free) == list(range(6))
    _consistent(c)


# ---- the scheduler -------------------------------------------------------------------------------------------------------------------------------
D, V = 64, 100
OLD_KEYS = {"steps", "row_steps_active", "row_steps_total", "pages_high_water", "admitted", "admitted_midflight", "page_waits", "pages_reused"}


def _scripted_batcher(monkeypatch, scripts, **kw):
    """tests/test_paged_cpu.py's scripted batcher plus a stub `extend_paged`: request i is recognised by the first element of its own first row and
    emits scripts[i]; a prefix's rows carry ids >= 100 and emit nothing."""
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
    log = dict(prefills=[], extends=[], decodes=[])
    where = {}                                                         # row -> [request, tokens emitted]

    def onehot(tok):
        return torch.nn.functional.one_hot(torch.tensor(tok), D).float()

    def first_state(i, rows):
        h = torch.zeros(1, rows, D)
        if i < 100:
            h[0, -1] = onehot(scripts[i][0])
        return h

    def prefill_paged(x, cache, row):
        i = int(x[0, 0, 0])
        assert x.shape[0] == 1 and cache.lens_host[row] == 0 and len(cache.pages_of(row)) * 128 >= x.shape[1]
        cache.set_len(row, x.shape[1])
        where[row] = [i, 1]
        log["prefills"].append((i, row, x.shape[1]))
        return first_state(i, x.shape[1])

    def extend_paged(x, cache, rows):
        (row,) = rows
        tail = int(x[0, 0, 0]) - 100                                   # the prefix's tail rows come first: its id says how many
        i = int(x[0, tail, 0])
        assert x.shape[0] == 1 and (cache.lens_host[row] + x.shape[1]) <= len(cache.pages_of(row)) * 128
        log["extends"].append((i, row, x.shape[1], cache.lens_host[row], cache.lens[row].item()))
        cache.set_len(row, cache.lens_host[row] + x.shape[1])
        where[row] = [i, 1]
        return first_state(i, x.shape[1])

    def decode_step_paged(x, cache, active, active_host=None):
        log["decodes"].append(list(active_host))
        h = torch.zeros(cache.rows, D)
        for row, on in enumerate(active_host):
            if on:
                i, n = where[row]
                h[row] = onehot(scripts[i][n])
                where[row][1] += 1
                cache.lens_host[row] += 1
        cache.lens = torch.tensor(cache.lens_host, dtype=torch.int32)
        return h

    monkeypatch.setattr(lm.model, "prefill_paged", prefill_paged)
    monkeypatch.setattr(lm.model, "extend_paged", extend_paged)
    monkeypatch.setattr(lm.model, "decode_step_paged", decode_step_paged)
    return ContinuousBatcher(lm, **kw), log


def _rows(first, T, then=None):
    """(T, D) embeddings whose first row starts with `first`; row `then[0]` starts with `then[1]`."""
    x = torch.zeros(T, D)
    x[0, 0] = first
    if then is not None:
        x[then[0], 0] = then[1]
    return x


def test_a_prefix_is_prefilled_once_and_its_requests_run_only_their_remainder(monkeypatch):
    scripts = [[10, 11, 12], [20, 21], [30, 31]]
    b, log = _scripted_batcher(monkeypatch, scripts, rows=2, num_pages=4, max_pages_per_seq=3)
    prefix = _rows(100 + 12, 140, then=(128, 100 + 12))                                    # P = 140: Ps = 128 shared slots, a tail of 12 rows
    h = b.register_prefix(prefix)
    assert log["prefills"] == [(112, 0, 128)] and (h.P, h.Ps, h.pages, tuple(h.tail.shape)) == (140, 128, [0], (12, D))
    assert b.cache.pages_free == 3 and b.cache.page_refs == [1, 0, 0, 0] and b.cache.table_host == [[-1] * 3] * 2 and b.cache.lens_host == [0, 0]
    assert b.prefix_stats == dict(registered=1, hits=0, slots_shared=0)
    t = [b.submit(_rows(0, 10), 3, prefix=h), b.submit(_rows(1, 20), 2), b.submit(_rows(2, 5), 2, prefix=h)]
    assert t == [0, 1, 2] and len(b.queue) == 3 and b.cache.pages_free == 3                        # submit touches nothing but the queue
    with pytest.raises(ValueError, match="queued request names this prefix"):
        b.drop_prefix(h)
    done = dict(b.step())                                              # request 0 behind the prefix on row 0, request 1 as ever on row 1
    assert log["extends"] == [(0, 0, 22, 128, 128)] and log["prefills"][1:] == [(1, 1, 20)]
    assert b.cache.table_host[0][:2] == [0, 1] and b.cache.page_refs[0] == 2 and list(done) == [1] and done[1].tolist() == [20, 21]
    with pytest.raises(ValueError, match="queued request names this prefix"):
        b.drop_prefix(h)                                               # request 2 still waits for a row
    done.update(b.step())
    assert log["extends"][1] == (2, 1, 17, 128, 128) and len(log["prefills"]) == 2                 # never prefill_paged for a prefixed request
    assert done[0].tolist() == [10, 11, 12] and done[2].tolist() == [30, 31] and b.queue == []
    assert b.prefix_stats == dict(registered=1, hits=2, slots_shared=256)
    assert set(b.stats) == OLD_KEYS and b.stats["admitted"] == 3 and b.stats["pages_high_water"] == 3
    assert b.cache.pages_free == 3 and b.cache.page_refs[0] == 1       # the prefix page survives its requests ...
    assert b.cache.table_host == [[-1] * 3] * 2 and b.cache.lens.tolist() == [0, 0]
    b.drop_prefix(h)                                                   # ... and returns to the pool now
    assert b.cache.pages_free == 4 and b.cache.page_refs == [0] * 4 and h.dropped
    with pytest.raises(ValueError, match="dropped or a foreign"):
        b.drop_prefix(h)
    with pytest.raises(ValueError, match="dropped or a foreign"):
        b.submit(_rows(0, 10), 3, prefix=h)
    assert b.queue == [] and b._tickets == 3


def test_running_requests_keep_a_dropped_prefixs_pages_until_the_last_of_them_leaves(monkeypatch):
    scripts = [[10, 11, 12, 13], [20, 21, 22]]                         # a step gives an admitted row two tokens: request 1 ends in step 2, request 0 in step 3
    b, log = _scripted_batcher(monkeypatch, scripts, rows=2, num_pages=5, max_pages_per_seq=4)
    h = b.register_prefix(_rows(100 + 4, 260, then=(256, 100 + 4)))                   # two shared pages, a tail of 4
    assert h.pages == [0, 1] and log["prefills"] == [(104, 0, 256)]
    b.submit(_rows(0, 3), 4, prefix=h)
    b.submit(_rows(1, 30), 3, prefix=h)
    assert b.step() == [] and log["extends"] == [(0, 0, 7, 256, 256), (1, 1, 34, 256, 256)]
    b.drop_prefix(h)                                                   # nothing queued names it: the running rows keep their own references
    assert b.cache.page_refs == [2, 2, 1, 1, 0] and b.cache.pages_free == 1
    assert [t for t, _ in b.step()] == [1]
    assert b.cache.page_refs == [1, 1, 1, 0, 0] and b.cache.pages_free == 2
    assert [t for t, _ in b.step()] == [0]
    assert b.cache.page_refs == [0] * 5 and b.cache.pages_free == 5 and sorted(b.cache._free) == list(range(5))
    assert b.prefix_stats == dict(registered=1, hits=2, slots_shared=512)


def test_register_prefix_and_submit_refuse_by_name_and_change_nothing(monkeypatch):
    b, log = _scripted_batcher(monkeypatch, [[1, 2, 3]], rows=1, num_pages=3, max_pages_per_seq=4)
    other, _ = _scripted_batcher(monkeypatch, [], rows=1, num_pages=3, max_pages_per_seq=3)
    for bad, msg in ((_rows(100, 127), "nothing to share"), (torch.zeros(127, dtype=torch.int64), "nothing to share"), (torch.zeros(140, D + 1), "is not"),
                     (_rows(100, 512), "leave a request none"), (None, "one of them")):
        with pytest.raises(ValueError, match=msg):
            b.register_prefix(bad)
    ids = torch.full((130,), 7, dtype=torch.int64)
    with torch.no_grad():
        b.lm.model.embed_tokens.weight[7, 0] = 102.0                   # the ids' embedding rows name a prefix with a tail of 2 to the stub
        b.w_e = b.lm.model.embed_tokens.weight.detach().contiguous()
    h = b.register_prefix(input_ids=ids)                               # ids work as embeddings do
    assert (h.P, h.Ps, tuple(h.tail.shape)) == (130, 128, (2, D)) and torch.equal(h.tail, b.w_e[7].expand(2, D))
    foreign = other.register_prefix(_rows(100, 128))
    for prompt, n, pre, msg in ((_rows(0, 200), 60, h, "need 4 pages, 3 of them"), (_rows(0, 1), 0, h, "max_new_tokens"), (torch.zeros(0, D), 2, h, "empty prompt"),
                                (_rows(0, 5), 2, foreign, "dropped or a foreign"), (_rows(0, 5), 2, "A", "dropped or a foreign")):
        with pytest.raises(ValueError, match=msg):
            b.submit(prompt, n, prefix=pre)
    assert b.queue == [] and b._tickets == 0
    with pytest.raises(RuntimeError, match="needs 3 free pages, the pool has 2"):
        b.register_prefix(_rows(100, 384))                             # one page is h's: three are not there
    b.submit(_rows(0, 4), 3, prefix=h)
    assert b.step() == [] and b.running[0] is not None
    state = (list(b.cache._free), list(b.cache.page_refs), [list(r) for r in b.cache.table_host], len(log["prefills"]), dict(b.prefix_stats))
    with pytest.raises(RuntimeError, match="no idle row"):
        b.register_prefix(_rows(100, 128))
    assert state == (list(b.cache._free), list(b.cache.page_refs), [list(r) for r in b.cache.table_host], len(log["prefills"]), dict(b.prefix_stats))


def test_held_prefix_pages_count_against_the_pool_so_no_queued_request_waits_for_ever(monkeypatch):
    """A held prefix's pages leave the pool until drop_prefix: a request that could then never be admitted is refused at submit, a prefix that would
    strand a queued request at register_prefix, and a head of the queue nobody can ever free pages for is a RuntimeError of step(), never a spin."""
    b, log = _scripted_batcher(monkeypatch, [[1, 2, 3], [4, 5, 6]], rows=2, num_pages=4, max_pages_per_seq=4)
    h = b.register_prefix(_rows(100, 256, then=(255, 100)))           # P = 256: two pages held, no tail
    assert h.pages == [0, 1] and tuple(h.tail.shape) == (0, D)
    with pytest.raises(ValueError, match="need 3 pages.*num_pages = 4, of which registered prefixes hold 2"):
        b.submit(_rows(0, 300), 3)                                     # 3 pages fit the pool, never the 2 the prefix leaves
    with pytest.raises(ValueError, match="need 5 pages, 3 of them.*registered prefixes hold 2"):
        b.submit(_rows(0, 300), 3, prefix=h)
    assert b.queue == [] and b._tickets == 0
    b.submit(_rows(0, 200), 3)                                         # 2 pages of its own: exactly what is left
    b.submit(_rows(1, 100), 3, prefix=h)                               # 3 pages, 1 of its own
    state = (list(b.cache._free), list(b.cache.page_refs), len(log["prefills"]), dict(b.prefix_stats), len(b.queue))
    with pytest.raises(RuntimeError, match="queued request 0 needs 2 of its own"):
        b.register_prefix(_rows(100, 128, then=(127, 100)))            # one page more held would strand request 0
    assert state == (list(b.cache._free), list(b.cache.page_refs), len(log["prefills"]), dict(b.prefix_stats), len(b.queue))
    done = {}
    for _ in range(10):                                                # request 0 takes both free pages, request 1 waits for one and follows
        done.update(b.step())
        if not b.queue and all(r is None for r in b.running):
            break
    assert sorted(done) == [0, 1] and b.stats["page_waits"] >= 1 and b.cache.pages_free == 2
    b.drop_prefix(h)
    assert b.submit(_rows(0, 300), 3) == 2 and b.cache.pages_free == 4          # with the prefix dropped the same request is taken
    # pages that leave the pool behind the batcher's back: the head of the queue cannot be served and nothing runs
    b.queue.clear()
    b.submit(_rows(0, 300), 3)
    assert b.cache.assign(1, 256)
    waits = b.stats["page_waits"]
    for _ in range(2):
        with pytest.raises(RuntimeError, match="needs 3 pages of its own and no request is running, but only 2 of 4 pages are free"):
            b.step()
    assert len(b.queue) == 1 and b.stats["page_waits"] == waits and all(r is None for r in b.running)      # refused by name: not a wait, nothing admitted


def test_a_prefill_that_raises_leaves_register_prefix_without_a_trace(monkeypatch):
    b, log = _scripted_batcher(monkeypatch, [[1, 2]], rows=1, num_pages=2, max_pages_per_seq=2)

    def failing(x, cache, row):
        assert cache.pages_of(row) == [0]
        raise RuntimeError("prefill failed")
    good = b.lm.model.prefill_paged
    monkeypatch.setattr(b.lm.model, "prefill_paged", failing)
    with pytest.raises(RuntimeError, match="prefill failed"):
        b.register_prefix(_rows(100, 130, then=(128, 102)))
    assert b.cache.table_host == [[-1, -1]] and b.cache.lens_host == [0] and b.cache.page_refs == [0, 0] and sorted(b.cache._free) == [0, 1]
    assert b.prefix_stats == dict(registered=0, hits=0, slots_shared=0) and b._prefixes == [] and b.stats["pages_high_water"] == 0
    monkeypatch.setattr(b.lm.model, "prefill_paged", good)
    assert [o.tolist() for o in b.run([(_rows(0, 200), 2)])] == [[1, 2]]      # the row and both pages can be had again
