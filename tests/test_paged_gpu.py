"""The paged KV cache on the GPU: `kv_append_paged` writes its slots through the table and nothing else; `attention_decode_paged` is `torch.equal` to
the dense decode kernel on every sequence's gathered slots, wherever its pages lie and whatever the rest of the pool holds; continuous batching over
a tiny Llama emits, for every request, the tokens `generate` gives that request alone.  No tolerance anywhere: a page is one chunk of the decode
attention, so the paged path runs the dense path's arithmetic."""
import pytest
import torch

import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import BeamSearch, ContinuousBatcher, LogitsProcessors, LookupDrafter, PagedKVCache, Sampler
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
PAGE = 128
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


# ---- append --------------------------------------------------------------------------------------------------------------------------------------
B_A, T_A, H_A, HKV_A, PAGES_A = 3, 5, 4, 2, 6
SLOT0_A = [126, -1, 0]                                                 # sequence 0 crosses a page boundary, sequence 1 is idle


def _append_case(dt, Dh, table):
    qkv = _rand(B_A * T_A, (H_A + 2 * HKV_A) * Dh, seed=1).to(dt).to(DEV)
    sentinel = lambda s: (torch.arange(PAGES_A * HKV_A * PAGE * Dh).reshape(PAGES_A, HKV_A, PAGE, Dh) % 251 + s).to(dt).to(DEV)
    k0, v0 = sentinel(1), sentinel(300)
    k, v = k0.clone(), v0.clone()
    bt = torch.tensor(table, dtype=torch.int32, device=DEV)
    ops.kv_append_paged(qkv, k, v, bt, torch.tensor(SLOT0_A, dtype=torch.int32, device=DEV), T_A, H_A)
    torch.cuda.synchronize()
    src = qkv.reshape(B_A, T_A, H_A + 2 * HKV_A, Dh)
    want_k, want_v, written = k0.clone(), v0.clone(), 0
    for b, s0 in enumerate(SLOT0_A):
        for t in range(T_A):
            slot = s0 + t
            page = table[b][slot // PAGE] if s0 >= 0 else -1
            if 0 <= page < PAGES_A:
                want_k[page, :, slot % PAGE] = src[b, t, H_A:H_A + HKV_A]
                want_v[page, :, slot % PAGE] = src[b, t, H_A + HKV_A:]
                written += 1
    # the targeted rows equal the source columns bit for bit, and every other byte of both pools is unchanged
    assert torch.equal(_bits(k), _bits(want_k)) and torch.equal(_bits(v), _bits(want_v))
    return k, v, k0, v0, written


@pytest.mark.parametrize("dt,Dh", [(torch.float32, 16), (torch.bfloat16, 128), (torch.float16, 64)])
def test_kv_append_paged_writes_its_slots_through_the_table_and_nothing_else(dt, Dh):
    table = [[4, 1], [5, 0], [2, 3]]                                   # shuffled, not monotonic
    k, v, k0, v0, written = _append_case(dt, Dh, table)
    assert written == 10
    assert not torch.equal(k[4, :, 126:], k0[4, :, 126:]) and not torch.equal(k[1, :, :3], k0[1, :, :3])      # slots 126 .. 130: pages 4 and 1
    for page in (5, 0, 3):                                             # sequence 1 wrote nothing; nor did anyone to sequence 2's second page
        assert torch.equal(_bits(k[page]), _bits(k0[page])) and torch.equal(_bits(v[page]), _bits(v0[page]))


@pytest.mark.parametrize("dt,Dh", [(torch.float32, 16), (torch.bfloat16, 128), (torch.float16, 64)])
@pytest.mark.parametrize("bad", [-1, PAGES_A, -7, 1 << 20])
def test_kv_append_paged_treats_an_out_of_range_page_id_as_no_page(dt, Dh, bad):
    # the page slots 128 .. 130 of sequence 0 would land in, and sequence 2's first page, are no pages: nothing is written for them, no error
    k, v, k0, v0, written = _append_case(dt, Dh, [[4, bad], [5, 0], [bad, 3]])
    assert written == 2                                                # slots 126 and 127 of sequence 0
    for page in (0, 1, 2, 3, 5):
        assert torch.equal(_bits(k[page]), _bits(k0[page])) and torch.equal(_bits(v[page]), _bits(v0[page]))


# ---- attention -----------------------------------------------------------------------------------------------------------------------------------
LENS = [0, 1, 127, 128, 129, 300]                                      # 0 + 1 + 1 + 1 + 2 + 3 = 8 live pages of the pool's 12
PAGES, MAX_PAGES = 12, 3


def _paged_case(dt, H, Hkv, Dh, seed=0):
    """Pools with every sequence's slots at a random permutation's pages; unused pages and the tail of each last page are NaN, unused entries -1."""
    g = torch.Generator().manual_seed(100 + seed)
    B = len(LENS)
    buf = (_rand(B, (H + 2 * Hkv) * Dh, seed=seed + 1) * 2).to(dt).to(DEV)           # q is read in place from a fused buffer: a row stride above H * Dh
    q = buf[:, :H * Dh]
    perm = torch.randperm(PAGES, generator=g).tolist()
    table = [[-1] * MAX_PAGES for _ in range(B)]
    kp = torch.full((PAGES, Hkv, PAGE, Dh), float("nan"), dtype=dt)
    vp = kp.clone()
    dense = []
    for b, n in enumerate(LENS):
        kd, vd = _rand(Hkv, n, Dh, seed=seed + 10 + b).to(dt), _rand(Hkv, n, Dh, seed=seed + 30 + b).to(dt)
        dense.append((kd.to(DEV), vd.to(DEV)))
        for p in range((n + PAGE - 1) // PAGE):
            page = perm.pop()
            table[b][p] = page
            m = min(PAGE, n - p * PAGE)
            kp[page, :, :m], vp[page, :, :m] = kd[:, p * PAGE:p * PAGE + m], vd[:, p * PAGE:p * PAGE + m]
    assert len(perm) == PAGES - 8
    return q, kp.to(DEV), vp.to(DEV), torch.tensor(table, dtype=torch.int32, device=DEV), dense


def _dense_rows(q, dense, H, scale):
    """Every sequence alone through the dense kernel: its slots as a (1, Hkv, len, Dh) cache under an all-ones mask; zeros for the empty one."""
    rows = []
    for b, (kd, vd) in enumerate(dense):
        n = kd.shape[1]
        if n == 0:
            rows.append(torch.zeros(1, q.shape[1], dtype=q.dtype, device=DEV))
            continue
        rows.append(ops.attention_decode(q[b:b + 1], kd[None].contiguous(), vd[None].contiguous(), torch.ones(1, n, dtype=torch.uint8, device=DEV), H, n,
                                         scale))
    return torch.cat(rows)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv,Dh", [(4, 4, 16), (8, 2, 64), (8, 2, 128)])
def test_attention_decode_paged_equals_the_dense_kernel_sequence_by_sequence(dt, H, Hkv, Dh):
    q, kp, vp, table, dense = _paged_case(dt, H, Hkv, Dh)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    scale = Dh ** -0.5
    want = _dense_rows(q, dense, H, scale)
    assert torch.isfinite(want).all()
    for max_len in (300, 384):                                         # 384: every row has trailing empty chunks
        got = ops.attention_decode_paged(q, kp, vp, table, lens, H, max_len, scale)
        assert torch.equal(got, want), (max_len, (got.float() - want.float()).abs().max(dim=1).values.tolist())
        assert torch.equal(got[0], torch.zeros_like(got[0]))           # lens = 0: exact zeros
    ws = torch.full((ops.attention_decode_paged_workspace(len(LENS), H, Dh, 384),), float("nan"), device=DEV)
    out = torch.empty_like(want)
    assert ops.attention_decode_paged(q, kp, vp, table, lens, H, 384, scale, ws=ws, out=out) is out and torch.equal(out, want)      # a poisoned workspace
    # the bits do not depend on the batch: a sequence alone, through its own row of the table
    for b in (2, 5):
        one = ops.attention_decode_paged(q[b:b + 1], kp, vp, table[b:b + 1].contiguous(), lens[b:b + 1].contiguous(), H, LENS[b], scale)
        assert torch.equal(one, want[b:b + 1])


@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.float32, 4, 4, 16), (torch.bfloat16, 8, 2, 128), (torch.float16, 8, 2, 64)])
def test_attention_decode_paged_counts_no_key_of_a_chunk_without_a_page(dt, H, Hkv, Dh):
    """An out-of-range table entry is "no page": the chunk's keys do not count, nothing is read through the id.  The 300-slot sequence with its middle
    page taken away is the dense kernel on its slots [0, 128) and [256, 300) - as a mask says it (chunk-aligned, so the same partition of the keys)."""
    q, kp, vp, table, dense = _paged_case(dt, H, Hkv, Dh, seed=3)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    scale = Dh ** -0.5
    want = _dense_rows(q, dense, H, scale)
    kd, vd = dense[5]
    mask = torch.ones(1, 300, dtype=torch.uint8, device=DEV)
    mask[:, 128:256] = 0
    want[5:6] = ops.attention_decode(q[5:6], kd[None].contiguous(), vd[None].contiguous(), mask, H, 300, scale)
    want[4] = 0                                                        # the 129-slot sequence loses both pages
    for bad in (-1, PAGES, 1 << 30):
        t = table.clone()
        t[5, 1] = bad
        t[4, 0], t[4, 1] = bad, bad
        got = ops.attention_decode_paged(q, kp, vp, t, lens, H, 300, scale)
        assert torch.equal(got, want), bad


# ---- model ---------------------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"dh16": dict(hidden_size=64, intermediate_size=192, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=100),
           "dh128": dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=100)}
PROMPTS, NEW = (3, 120, 127, 130, 40), (12, 10, 5, 3, 8)               # 130: a prompt that crosses a page; 120 + 10: decoding crosses one; 127 + 5
ROWS, POOL = 2, 3                                                      # pages for one 2-page and one 1-page request at a time: the 4th request must wait
MIN_MARGIN = 1e-3                                                      # the fixtures' rule: top-2 margin of every selection, relative to the largest logit
_MODELS, _ALONE = {}, {}


def _model(name, dt, seed, quantized=False):
    key = (name, dt, seed, quantized)
    if key not in _MODELS:
        kw = CONFIGS[name]
        m = SetokimLlamaPrefill(kw)
        m.load_state_dict(O.init_llama_weights(O.LlamaConfigLite(**kw), seed=seed), strict=True)
        m = m.to(device=DEV, dtype=dt).eval()
        if quantized:
            m.quantize_mxfp4_()
        _MODELS[key] = m
    return _MODELS[key]


def _prompts(name, dt, seed):
    D = CONFIGS[name]["hidden_size"]
    return [_rand(T, D, seed=1000 * seed + i).to(dt).to(DEV) for i, T in enumerate(PROMPTS)]


def _alone(name, dt, seed, quantized=False, eos=None):
    """Every request alone through the dense `generate` (computed once per case and shared): (tokens, smallest top-2 margin of any selection)."""
    key = (name, dt, seed, quantized, eos)
    if key not in _ALONE:
        m, toks, margin = _model(name, dt, seed, quantized), [], float("inf")
        for x, n in zip(_prompts(name, dt, seed), NEW):
            out = m.generate(inputs_embeds=x[None], max_new_tokens=n, eos_token_id=eos, return_dict_in_generate=True, output_logits=True)
            toks.append(out.sequences[0])
            top = out.logits[0].float().topk(2, dim=-1).values
            margin = min(margin, float(((top[:, 0] - top[:, 1]) / out.logits[0].float().abs().amax(dim=-1)).min()))
        _ALONE[key] = (toks, margin)
    return _ALONE[key]


def _batched(name, dt, seed, quantized=False, eos=None):
    m = _model(name, dt, seed, quantized)
    b = ContinuousBatcher(m, ROWS, POOL, max_pages_per_seq=2, eos_token_id=eos)
    for t in b.cache.k + b.cache.v:
        t.fill_(float("nan"))                                          # nothing may depend on what a pool holds
    return b, b.run(list(zip(_prompts(name, dt, seed), NEW)))


def _mid_sequence_eos(toks):
    """A token some request alone emits before its last position: as an eos id it cuts that request short."""
    for t in toks:
        if t.numel() > 2:
            return int(t[t.numel() // 2])
    raise AssertionError("no request is longer than two tokens")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_continuous_batching_equals_each_request_alone(name, dt):
    want, margin = _alone(name, dt, 5)
    print(f"{name} {dt}: smallest top-2 margin of the alone runs {margin:.3e}")
    b, got = _batched(name, dt, 5)
    assert [g.tolist() for g in got] == [w.tolist() for w in want] and all(torch.equal(g, w) for g, w in zip(got, want))
    assert [g.numel() for g in got] == list(NEW)
    st = b.stats
    assert st["admitted"] == 5 and st["admitted_midflight"] >= 1       # requests joined a running batch
    assert st["page_waits"] >= 1                                       # an idle row waited for pages
    assert st["pages_reused"] >= 1                                     # pages that carried a finished sequence's data were handed out again
    assert st["pages_high_water"] == POOL and 0 < st["row_steps_active"] <= st["row_steps_total"] == ROWS * st["steps"]
    assert b.cache.pages_free == POOL and b.cache.lens.tolist() == [0] * ROWS and b.cache.block_table.tolist() == [[-1, -1]] * ROWS
    eos = _mid_sequence_eos(want)
    want_e, _ = _alone(name, dt, 5, eos=eos)
    assert any(w.numel() < n for w, n in zip(want_e, NEW)) and all(int(w[-1]) == eos or w.numel() == n for w, n in zip(want_e, NEW))
    _, got_e = _batched(name, dt, 5, eos=eos)
    assert [g.tolist() for g in got_e] == [w.tolist() for w in want_e]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_continuous_batching_equals_each_request_alone_in_fp32(name):
    """Tokens are compared, so no selection may sit on a coin flip: the first seed whose alone runs keep the fixtures' top-2 margin is the case."""
    for seed in (5, 6, 7, 8, 9, 10):
        want, margin = _alone(name, torch.float32, seed)
        print(f"{name} fp32 seed {seed}: smallest top-2 margin of the alone runs {margin:.3e}")
        if margin >= MIN_MARGIN:
            break
    assert margin >= MIN_MARGIN
    _, got = _batched(name, torch.float32, seed)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    eos = _mid_sequence_eos(want)
    want_e, margin_e = _alone(name, torch.float32, seed, eos=eos)
    assert margin_e >= MIN_MARGIN and any(w.numel() < n for w, n in zip(want_e, NEW))
    _, got_e = _batched(name, torch.float32, seed, eos=eos)
    assert [g.tolist() for g in got_e] == [w.tolist() for w in want_e]


def test_continuous_batching_over_mxfp4_weights_equals_the_quantised_models_own_generate():
    want, margin = _alone("dh128", torch.bfloat16, 5, quantized=True)
    print(f"dh128 bf16 mxfp4 weights: smallest top-2 margin of the alone runs {margin:.3e}")
    m = _model("dh128", torch.bfloat16, 5, quantized=True)
    assert m.weight_format.startswith("mxfp4")
    _, got = _batched("dh128", torch.bfloat16, 5, quantized=True)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]


def test_the_model_entry_points_keep_the_dense_bits_and_leave_idle_rows_alone():
    """`prefill_paged` returns the dense prefill's states; a decode step over (active, idle, active) rows returns the dense `decode_step`'s state for
    each active row and touches neither the idle row's length nor a byte of the pages it does not write."""
    m = _model("dh16", torch.bfloat16, 5)
    from setok_amd.generation import KVCache
    xs = _prompts("dh16", torch.bfloat16, 5)
    cache = PagedKVCache.for_model(m.model, 3, 6, 2)
    for t in cache.k + cache.v:
        t.fill_(float("nan"))
    dense = {}
    for row, i in ((0, 2), (2, 3)):                                    # prompts of 127 and 130 tokens on rows 0 and 2; row 1 stays idle
        T = PROMPTS[i]
        assert cache.assign(row, T + 2)
        dense[row] = KVCache.for_model(m.model, 1, T + 2)
        assert torch.equal(m.model.prefill_paged(xs[i][None], cache, row), m.model.prefill(xs[i][None], None, None, dense[row]))
    assert cache.lens.tolist() == [127, 0, 130] == cache.lens_host
    step = _rand(3, 64, seed=77).to(torch.bfloat16).to(DEV)
    active = torch.tensor([True, False, True], device=DEV)
    for _ in range(2):                                                 # row 0 steps from slot 127 into its second page
        before = [t.clone() for t in cache.k + cache.v]
        lens0 = list(cache.lens_host)
        h = m.model.decode_step_paged(step, cache, active)
        for row in (0, 2):
            assert torch.equal(h[row:row + 1], m.model.decode_step(step[row:row + 1], dense[row]))
        assert cache.lens.tolist() == cache.lens_host == [lens0[0] + 1, 0, lens0[2] + 1]
        for t, t0 in zip(cache.k + cache.v, before):                   # exactly one slot per active row was written
            assert int((_bits(t) != _bits(t0)).any(dim=3).any(dim=1).sum()) == 2
    cache.set_len(0, 2 * PAGE)                                         # a row whose two pages are full ...
    with pytest.raises(ValueError, match="no room for one more"):
        m.model.decode_step_paged(step, cache, active)                 # ... cannot take a step: refused on the host, nothing launched
    cache.set_len(0, 129)
    with pytest.raises(ValueError, match="cannot take a prefill"):
        m.model.prefill_paged(xs[0][None], cache, 0)                   # the row is not empty
    with pytest.raises(ValueError, match="cannot take a prefill"):
        m.model.prefill_paged(xs[0][None], cache, 1)                   # the row owns no pages
    assert cache.lens.tolist() == [129, 0, 132]


def test_the_batcher_refuses_what_is_not_built_and_submit_leaves_no_trace():
    m = _model("dh16", torch.bfloat16, 5)
    for kw, name in ((dict(sampler=Sampler()), "sampler="), (dict(beams=BeamSearch(2)), "beams="), (dict(draft=LookupDrafter(2)), "draft="),
                     (dict(processors=LogitsProcessors(1.3)), "processors="), (dict(prefill_chunk=64), "prefill_chunk="),
                     (dict(kv_cache="fp8"), "kv_cache='fp8'"), (dict(kv_cache="mxfp4"), "kv_cache='mxfp4'")):
        with pytest.raises(NotImplementedError, match=name):
            ContinuousBatcher(m, ROWS, POOL, **kw)
    b = ContinuousBatcher(m, ROWS, POOL, max_pages_per_seq=2)
    x = _prompts("dh16", torch.bfloat16, 5)
    table, lens = b.cache.block_table.clone(), b.cache.lens.clone()
    for prompt, n in ((x[3], 127), (x[0], 254), (x[0][:, :32], 4), (x[0], 0)):     # 3 pages per sequence; 3 pages again; not (T, D); no token asked for
        with pytest.raises(ValueError, match="ContinuousBatcher.submit"):
            b.submit(prompt, n)
    small = ContinuousBatcher(m, ROWS, 1, max_pages_per_seq=2)
    with pytest.raises(ValueError, match="num_pages = 1"):
        small.submit(x[1], 10)                                         # fits a table row, never the pool
    assert b.queue == [] and small.queue == [] and b.cache.pages_free == POOL and b._tickets == 0
    assert torch.equal(b.cache.block_table, table) and torch.equal(b.cache.lens, lens) and b.cache.table_host == [[-1, -1]] * ROWS
    with pytest.raises(RuntimeError, match="unsupported head dim 24"):
        ops.attention_decode_paged(torch.zeros(1, 24, dtype=torch.bfloat16, device=DEV), torch.zeros(1, 1, PAGE, 24, dtype=torch.bfloat16, device=DEV),
                                   torch.zeros(1, 1, PAGE, 24, dtype=torch.bfloat16, device=DEV), torch.zeros(1, 1, dtype=torch.int32, device=DEV),
                                   torch.zeros(1, dtype=torch.int32, device=DEV), 1, 0, 1.0)
