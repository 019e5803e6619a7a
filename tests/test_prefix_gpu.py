"""The paged extend attention and prefix sharing on the GPU: `attention_extend_paged` is `torch.equal` to the dense extend kernel on every sequence's
gathered slots, wherever its pages lie, whatever the rest of the pool holds and with a page missing; `LlamaModel.extend_paged` returns the dense
`extend`'s states row by row; a `ContinuousBatcher` whose requests share registered prefixes emits, for every request, the tokens `generate` gives
that request alone, and the shared pages hold the dense prefill's bits.  No tolerance anywhere: the dense kernels' key tiles, chunks and spans
never straddle a page, so the paged path runs the dense path's arithmetic."""
import pytest
import torch

import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import ContinuousBatcher, KVCache, PagedKVCache
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
PAGE = 128
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ---- kernel --------------------------------------------------------------------------------------------------------------------------------------
LEN0 = [-1, 0, 1, 127, 128, 129, 300, 1020]                            # -1: an idle sequence; 1020 + 9 crosses the 1024-slot span of the MFMA kernel
MAX_PAGES, POOL_K = 9, 24                                              # at Tn = 40 the sequences own 20 pages: the pool has spare ones
_CASES = {}


def _extend_case(dt, H, Hkv, Dh, Tn, seed=0):
    """(q, k_pool, v_pool, table, want): every sequence's len0 old slots at a random permutation's pages, its Tn new rows written by kv_append_paged
    from the fused buffer q is read from; unused pages and every slot at or above len0 + Tn are NaN, unused entries -1.  `want`: every sequence
    alone through the dense kernel - its slots gathered into a (1, Hkv, len0 + Tn, Dh) cache under an all-ones mask -, zeros for the idle one.
    Computed once per case and shared."""
    key = (dt, H, Hkv, Dh, Tn, seed)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(200 + seed)
    B = len(LEN0)
    qkv = (_rand(B * Tn, (H + 2 * Hkv) * Dh, seed=seed + 1) * 1.5).to(dt).to(DEV)      # q is read in place: a row stride above H * Dh
    q = qkv[:, :H * Dh]
    perm = torch.randperm(POOL_K, generator=g).tolist()
    table = [[-1] * MAX_PAGES for _ in range(B)]
    kp = torch.full((POOL_K, Hkv, PAGE, Dh), float("nan"), dtype=dt)
    vp = kp.clone()
    old = []
    for b, n in enumerate(LEN0):
        if n < 0:
            old.append(None)
            continue
        kd, vd = _rand(Hkv, n, Dh, seed=seed + 10 + b).to(dt), _rand(Hkv, n, Dh, seed=seed + 30 + b).to(dt)
        old.append((kd.to(DEV), vd.to(DEV)))
        for p in range((n + Tn + PAGE - 1) // PAGE):
            page = perm.pop()
            table[b][p] = page
            m = max(0, min(PAGE, n - p * PAGE))
            kp[page, :, :m], vp[page, :, :m] = kd[:, p * PAGE:p * PAGE + m], vd[:, p * PAGE:p * PAGE + m]
    assert perm, "the pool has spare pages"
    kp, vp = kp.to(DEV), vp.to(DEV)
    bt = torch.tensor(table, dtype=torch.int32, device=DEV)
    len0 = torch.tensor(LEN0, dtype=torch.int32, device=DEV)
    ops.kv_append_paged(qkv, kp, vp, bt, len0, Tn, H)
    new = qkv.reshape(B, Tn, H + 2 * Hkv, Dh)
    want, dense = [], []
    for b, n in enumerate(LEN0):
        if n < 0:
            want.append(torch.zeros(Tn, H * Dh, dtype=dt, device=DEV))
            dense.append(None)
            continue
        kd = torch.cat([old[b][0], new[b, :, H:H + Hkv].transpose(0, 1)], dim=1)[None].contiguous()
        vd = torch.cat([old[b][1], new[b, :, H + Hkv:].transpose(0, 1)], dim=1)[None].contiguous()
        dense.append((kd, vd))
        want.append(ops.attention_extend(q[b * Tn:(b + 1) * Tn], kd, vd, torch.ones(1, n + Tn, dtype=torch.uint8, device=DEV), H, Tn, n, Dh ** -0.5))
    want = torch.cat(want)
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    _CASES[key] = (q, kp, vp, bt, len0, want, dense)
    return _CASES[key]


@pytest.mark.parametrize("Tn", [1, 3, 9, 40])                          # at G = 4: 4 and 12 stacked rows (NW = 1), 36 (NW = 4, 1024-slot spans), 160 (two row blocks)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv,Dh", [(4, 4, 16), (8, 2, 64), (8, 2, 128)])
def test_attention_extend_paged_equals_the_dense_kernel_sequence_by_sequence(dt, H, Hkv, Dh, Tn):
    q, kp, vp, table, len0, want, _ = _extend_case(dt, H, Hkv, Dh, Tn)
    B, scale = len(LEN0), Dh ** -0.5
    for max_len0 in (max(LEN0), MAX_PAGES * PAGE - Tn):                # the table's end: every sequence has trailing empty spans
        got = ops.attention_extend_paged(q, kp, vp, table, len0, H, Tn, max_len0, scale)
        diff = (got.float() - want.float()).abs().reshape(B, -1).max(dim=1).values.tolist()
        print(f"{dt} H={H} Hkv={Hkv} Dh={Dh} Tn={Tn} max_len0={max_len0}: largest difference per sequence {diff}")
        assert torch.equal(got, want), (max_len0, diff)
        assert torch.equal(got[:Tn], torch.zeros_like(got[:Tn]))       # the idle sequence: exact zeros
    ws = torch.full((ops.attention_extend_paged_workspace(B, Tn, H, Dh, MAX_PAGES * PAGE - Tn, Hkv, dt),), float("nan"), device=DEV)
    out = torch.empty_like(want)
    assert ops.attention_extend_paged(q, kp, vp, table, len0, H, Tn, MAX_PAGES * PAGE - Tn, scale, ws=ws, out=out) is out
    assert torch.equal(out, want)                                      # a poisoned workspace, a caller's out
    for b in (2, 4, 7):                                                # the bits do not depend on the batch: a sequence alone, through its own table row
        one = ops.attention_extend_paged(q[b * Tn:(b + 1) * Tn], kp, vp, table[b:b + 1].contiguous(), len0[b:b + 1].contiguous(), H, Tn, LEN0[b], scale)
        assert torch.equal(one, want[b * Tn:(b + 1) * Tn]), b


@pytest.mark.parametrize("Tn", [3, 40])
@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.float32, 4, 4, 16), (torch.bfloat16, 8, 2, 128), (torch.float16, 8, 2, 128), (torch.float16, 8, 2, 64)])
def test_attention_extend_paged_counts_no_key_of_a_page_that_is_no_page(dt, H, Hkv, Dh, Tn):
    """An out-of-range table entry is "no page".  The 300-slot sequence with its middle page taken away is the dense kernel under a mask that is zero
    on [128, 256) - page-aligned, so the same tiles -; the 129-slot sequence with every page taken away gives zeros.  No error is returned."""
    q, kp, vp, table, len0, want, dense = _extend_case(dt, H, Hkv, Dh, Tn, seed=3)
    scale = Dh ** -0.5
    want = want.clone()
    kd, vd = dense[6]
    mask = torch.ones(1, 300 + Tn, dtype=torch.uint8, device=DEV)
    mask[:, 128:256] = 0
    want[6 * Tn:7 * Tn] = ops.attention_extend(q[6 * Tn:7 * Tn], kd, vd, mask, H, Tn, 300, scale)
    want[5 * Tn:6 * Tn] = 0
    for bad in (-1, POOL_K, 1 << 30):
        t = table.clone()
        t[6, 1] = bad
        t[5, 0], t[5, 1] = bad, bad
        got = ops.attention_extend_paged(q, kp, vp, t, len0, H, Tn, max(LEN0), scale)
        assert torch.equal(got, want), bad


# ---- model ---------------------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"dh16": dict(hidden_size=64, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=100),
           "dh128": dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=100)}
MIN_MARGIN = 1e-3                                                      # the fixtures' rule: top-2 margin of every selection, relative to the largest logit
_MODELS, _ALONE = {}, {}


def _model(name, dt, seed):
    key = (name, dt, seed)
    if key not in _MODELS:
        kw = CONFIGS[name]
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict(O.init_llama_weights(O.LlamaConfigLite(**kw), seed=seed), strict=True)
        _MODELS[key] = m.to(device=DEV, dtype=dt).eval()
    return _MODELS[key]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_extend_paged_keeps_the_dense_extends_bits_and_leaves_the_other_rows_alone(name):
    m = _model(name, torch.bfloat16, 5)
    D, Tn = CONFIGS[name]["hidden_size"], 5
    cache = PagedKVCache.for_model(m.model, 3, 6, 2)
    for t in cache.k + cache.v:
        t.fill_(float("nan"))
    dense, new = {}, _rand(2, Tn, D, seed=91).to(torch.bfloat16).to(DEV)
    for row, T in ((0, 127), (2, 130)):                                # row 0 extends across a page boundary; row 1 stays idle
        x = _rand(T, D, seed=50 + row).to(torch.bfloat16).to(DEV)
        assert cache.assign(row, T + Tn)
        dense[row] = KVCache.for_model(m.model, 1, T + Tn)
        assert torch.equal(m.model.prefill_paged(x[None], cache, row), m.model.prefill(x[None], None, None, dense[row]))
    before = [t.clone() for t in cache.k + cache.v]
    h = m.model.extend_paged(new, cache, (0, 2))
    assert h.shape == (2, Tn, D)
    for i, row in enumerate((0, 2)):
        assert torch.equal(h[i:i + 1], m.model.extend(new[i:i + 1], dense[row])), row
    assert cache.lens.tolist() == cache.lens_host == [132, 0, 135] and cache.pages_of(1) == [] and cache.block_table[1].tolist() == [-1, -1]
    for t, t0 in zip(cache.k + cache.v, before):                       # exactly Tn slots per listed row were written
        assert int((_bits(t) != _bits(t0)).any(dim=3).any(dim=1).sum()) == 2 * Tn
    before = [t.clone() for t in cache.k + cache.v]
    cache.set_len(0, 2 * PAGE - Tn + 1)                                # a row with room for Tn - 1 more ...
    with pytest.raises(ValueError, match="no room for 5 more"):
        m.model.extend_paged(new, cache, (0, 2))                       # ... is refused on the host, nothing launched
    with pytest.raises(ValueError, match="distinct rows"):
        m.model.extend_paged(new, cache, (2, 2))
    with pytest.raises(ValueError, match="no room"):
        m.model.extend_paged(new[:1], cache, (1,))                     # the idle row owns no pages
    assert cache.lens.tolist() == cache.lens_host == [2 * PAGE - Tn + 1, 0, 135]
    assert all(torch.equal(_bits(t), _bits(t0)) for t, t0 in zip(cache.k + cache.v, before))


# ---- batcher -------------------------------------------------------------------------------------------------------------------------------------
P_A, P_B = 140, 260                                                    # prefix A: one shared page and a tail of 12; prefix B: two shared pages, a tail of 4
# (prefix, remainder rows, max_new_tokens): at G = 2, A's 3 / 40 / 100 give 30 / 104 / 224 stacked rows - NW = 1, then NW = 4
REQUESTS = (("A", 3, 6), ("A", 40, 5), (None, 50, 7), ("A", 100, 4), ("B", 30, 5))
ROWS, POOL = 3, 5                                                      # 3 pages are held by the prefixes: two requests' own pages fit at a time, the third waits


def _inputs(name, dt, seed):
    D = CONFIGS[name]["hidden_size"]
    prefixes = {"A": _rand(P_A, D, seed=1000 * seed + 90).to(dt).to(DEV), "B": _rand(P_B, D, seed=1000 * seed + 91).to(dt).to(DEV)}
    rest = [_rand(S, D, seed=1000 * seed + i).to(dt).to(DEV) for i, (_, S, _) in enumerate(REQUESTS)]
    return prefixes, rest


def _alone(name, dt, seed):
    """Every request alone through the dense `generate` over its full prompt, the prefix's shared rows as the first window (computed once per case
    and shared): (tokens, smallest top-2 margin of any selection)."""
    key = (name, dt, seed)
    if key not in _ALONE:
        m, toks, margin = _model(name, dt, seed), [], float("inf")
        prefixes, rest = _inputs(name, dt, seed)
        for (pre, S, n), x in zip(REQUESTS, rest):
            if pre is None:
                out = m.generate(inputs_embeds=x[None], max_new_tokens=n, return_dict_in_generate=True, output_logits=True)
            else:
                full = torch.cat([prefixes[pre], x])
                Ps = PAGE * (prefixes[pre].shape[0] // PAGE)          # T - Ps <= Ps: exactly two windows, the prefill and one dense extend
                out = m.generate(inputs_embeds=full[None], max_new_tokens=n, prefill_chunk=Ps, return_dict_in_generate=True, output_logits=True)
            toks.append(out.sequences[0])
            top = out.logits[0].float().topk(2, dim=-1).values
            margin = min(margin, float(((top[:, 0] - top[:, 1]) / out.logits[0].float().abs().amax(dim=-1)).min()))
        _ALONE[key] = (toks, margin)
    return _ALONE[key]


def _batched(name, dt, seed):
    m = _model(name, dt, seed)
    prefixes, rest = _inputs(name, dt, seed)
    b = ContinuousBatcher(m, ROWS, POOL, max_pages_per_seq=3)
    for t in b.cache.k + b.cache.v:
        t.fill_(float("nan"))                                          # nothing may depend on what a pool holds
    handles = {k: b.register_prefix(v) for k, v in prefixes.items()}
    assert [len(h.pages) for h in handles.values()] == [1, 2] and b.cache.pages_free == POOL - 3
    got = b.run([(x, n) if pre is None else (x, n, handles[pre]) for (pre, _, n), x in zip(REQUESTS, rest)])
    return b, handles, got


def _check_drained(b, handles):
    st = b.stats
    assert st["admitted"] == len(REQUESTS) and st["page_waits"] >= 1 and st["pages_high_water"] == POOL
    assert b.prefix_stats == dict(registered=2, hits=4, slots_shared=3 * 128 + 256)
    assert b.cache.pages_free == POOL - 3                              # the pool minus the held prefix pages
    for h in handles.values():
        b.drop_prefix(h)
    assert b.cache.pages_free == POOL and sorted(b.cache._free) == list(range(POOL)) and b.cache.page_refs == [0] * POOL
    assert b.cache.block_table.tolist() == [[-1] * 3] * ROWS and b.cache.lens.tolist() == [0] * ROWS


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_requests_behind_shared_prefixes_equal_each_request_alone(name, dt):
    want, margin = _alone(name, dt, 5)
    print(f"{name} {dt}: smallest top-2 margin of the alone runs {margin:.3e}")
    b, handles, got = _batched(name, dt, 5)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    assert [g.numel() for g in got] == [n for _, _, n in REQUESTS]
    _check_drained(b, handles)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_requests_behind_shared_prefixes_equal_each_request_alone_in_fp32(name):
    """Tokens are compared, so no selection may sit on a coin flip: the first seed whose alone runs keep the fixtures' top-2 margin is the case."""
    for seed in (5, 6, 7, 8, 9, 10):
        want, margin = _alone(name, torch.float32, seed)
        print(f"{name} fp32 seed {seed}: smallest top-2 margin of the alone runs {margin:.3e}")
        if margin >= MIN_MARGIN:
            break
    assert margin >= MIN_MARGIN
    b, handles, got = _batched(name, torch.float32, seed)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    _check_drained(b, handles)


@pytest.mark.parametrize("name,dt", [("dh16", torch.float32), ("dh128", torch.bfloat16), ("dh128", torch.float16)])
def test_the_shared_pages_hold_the_dense_prefills_bits(name, dt):
    m = _model(name, dt, 5)
    prefixes, _ = _inputs(name, dt, 5)
    b = ContinuousBatcher(m, ROWS, POOL, max_pages_per_seq=3)
    for t in b.cache.k + b.cache.v:
        t.fill_(float("nan"))
    h = b.register_prefix(prefixes["B"])
    assert (h.P, h.Ps, len(h.pages), tuple(h.tail.shape)) == (260, 256, 2, (4, CONFIGS[name]["hidden_size"]))
    assert torch.equal(h.tail, prefixes["B"][256:])
    dense = KVCache.for_model(m.model, 1, 256)
    m.model.prefill(prefixes["B"][None, :256], None, None, dense)
    for li in range(len(b.cache.k)):
        for pool, ref in ((b.cache.k[li], dense.k[li]), (b.cache.v[li], dense.v[li])):
            for p, page in enumerate(h.pages):
                assert torch.equal(_bits(pool[page]), _bits(ref[0, :, p * PAGE:(p + 1) * PAGE])), (li, p)
    assert b.cache.lens.tolist() == [0] * ROWS and b.cache.block_table.tolist() == [[-1] * 3] * ROWS      # the row it was prefilled on is idle again
