"""MXFP4 pages on the GPU: `kv_append_paged_mxfp4` writes, through the table, exactly the bytes the dense MXFP4 append writes and nothing else;
`attention_decode_paged_mxfp4kv` and `attention_extend_paged_mxfp4kv` are `torch.equal` to the dense MXFP4 kernels on every sequence's gathered
slots, wherever its pages lie and whatever the rest of the pools holds; continuous batching over MXFP4 pages emits, for every request, the tokens
`generate(kv_cache="mxfp4")` gives that request alone.  No tolerance anywhere: the paged kernels run the dense MXFP4 kernels' arithmetic on the
same partition of the keys - a decode chunk is 256 slots, two pages, and a wave's 64 slots never straddle a page."""
import pytest
import torch

import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops
    from setok_amd.generation import ContinuousBatcher, PagedKVCache
    from setok_amd.llama import SetokimLlamaPrefill

DEV = "cuda"
PAGE = 128
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
POISON = 0xFF                                                          # a scale byte that makes every element of its block a NaN


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _bytes(*shape, lo=0, hi=256, seed=0):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int32).to(torch.uint8)


def _rows(Hkv, n, Dh, seed):
    """n MXFP4 rows per key / value head: any nibbles, scale bytes 2^-3 ... 2^0 - every byte pattern with such a scale is a valid finite row."""
    return _bytes(Hkv, n, Dh // 2, seed=seed), _bytes(Hkv, n, Dh // 32, lo=124, hi=128, seed=seed + 1)


# ---- append --------------------------------------------------------------------------------------------------------------------------------------
B_A, T_A, H_A, HKV_A, PAGES_A = 3, 5, 4, 2, 6
SLOT0_A = [126, -1, 0]                                                 # sequence 0 crosses a page boundary, sequence 1 is idle


def _append_case(dt, Dh, table, poke=None):
    qkv = _rand(B_A * T_A, (H_A + 2 * HKV_A) * Dh, seed=1).to(dt)
    if poke is not None:
        qkv[poke[0], poke[1]] = float("inf")
    qkv = qkv.to(DEV)
    sentinel = lambda cols, s: ((torch.arange(PAGES_A * HKV_A * PAGE * cols).reshape(PAGES_A, HKV_A, PAGE, cols) * 7 + s) % 251).to(torch.uint8).to(DEV)
    before = [sentinel(Dh // 2, 1), sentinel(Dh // 32, 50), sentinel(Dh // 2, 100), sentinel(Dh // 32, 150)]       # k_q, k_s, v_q, v_s
    pools = [t.clone() for t in before]
    bt = torch.tensor(table, dtype=torch.int32, device=DEV)
    ops.kv_append_paged_mxfp4(qkv, *pools, bt, torch.tensor(SLOT0_A, dtype=torch.int32, device=DEV), T_A, H_A)
    # what the dense append writes for the same source rows: a (B, Hkv, T, ·) cache filled from slot 0
    dense = [torch.zeros(B_A, HKV_A, T_A, c, dtype=torch.uint8, device=DEV) for c in (Dh // 2, Dh // 32, Dh // 2, Dh // 32)]
    ops.kv_append_mxfp4(qkv, *dense, T_A, H_A, 0)
    torch.cuda.synchronize()
    want, written = [t.clone() for t in before], 0
    for b, s0 in enumerate(SLOT0_A):
        for t in range(T_A):
            slot = s0 + t
            page = table[b][slot // PAGE] if s0 >= 0 else -1
            if 0 <= page < PAGES_A:
                for w, d in zip(want, dense):
                    w[page, :, slot % PAGE] = d[b, :, t]
                written += 1
    # the targeted rows hold the dense append's bytes, and every other byte of all four pools is unchanged
    for name, got, w in zip(("k_q", "k_s", "v_q", "v_s"), pools, want):
        assert torch.equal(got, w), name
    return pools, before, dense, written


APPEND_CASES = [(torch.float32, 32), (torch.bfloat16, 128), (torch.float16, 64)]


@pytest.mark.parametrize("dt,Dh", APPEND_CASES)
def test_kv_append_paged_mxfp4_writes_the_dense_appends_bytes_through_the_table_and_nothing_else(dt, Dh):
    table = [[4, 1], [5, 0], [2, 3]]                                   # shuffled, not monotonic
    pools, before, _, written = _append_case(dt, Dh, table)
    assert written == 10
    assert not torch.equal(pools[0][4, :, 126:], before[0][4, :, 126:]) and not torch.equal(pools[0][1, :, :3], before[0][1, :, :3])   # slots 126 .. 130
    for page in (5, 0, 3):                                             # sequence 1 wrote nothing; nor did anyone to sequence 2's second page
        assert all(torch.equal(t[page], t0[page]) for t, t0 in zip(pools, before))


@pytest.mark.parametrize("dt,Dh", APPEND_CASES)
@pytest.mark.parametrize("bad", [-1, PAGES_A, -7, 1 << 20])
def test_kv_append_paged_mxfp4_treats_an_out_of_range_page_id_as_no_page(dt, Dh, bad):
    # the page slots 128 .. 130 of sequence 0 would land in, and sequence 2's first page, are no pages: nothing is written for them, no error
    pools, before, _, written = _append_case(dt, Dh, [[4, bad], [5, 0], [bad, 3]])
    assert written == 2                                                # slots 126 and 127 of sequence 0
    for page in (0, 1, 2, 3, 5):
        assert all(torch.equal(t[page], t0[page]) for t, t0 in zip(pools, before))


@pytest.mark.parametrize("dt,Dh", APPEND_CASES)
def test_kv_append_paged_mxfp4_turns_a_block_with_a_non_finite_entry_into_the_nan_block(dt, Dh):
    # row b = 2, t = 1 of the fused buffer, the first element of key head 0: slot 1 of page 2
    pools, _, dense, _ = _append_case(dt, Dh, [[4, 1], [5, 0], [2, 3]], poke=(2 * T_A + 1, H_A * Dh))
    assert int(dense[1][2, 0, 1, 0]) == POISON and int(dense[0][2, 0, 1, :16].max()) == 0           # the dense quantiser's answer ...
    assert int(pools[1][2, 0, 1, 0]) == POISON and int(pools[0][2, 0, 1, :16].max()) == 0           # ... and the page's: scale 0xFF, zero nibbles
    assert int((pools[1] == POISON).sum()) == 1                        # that block alone


# ---- decode attention ------------------------------------------------------------------------------------------------------------------------------
LENS = [0, 1, 127, 128, 129, 255, 256, 257, 300, 513, 640]             # 0 + 1 + 1 + 1 + 2 + 2 + 2 + 3 + 3 + 5 + 5 = 25 live pages of the pool's 30
PAGES, MAX_PAGES = 30, 5                                               # an odd table row: chunk 2 of the 513- and 640-slot sequences reads entry 4, and there is no entry 5
SHAPES = [(4, 4, 32), (8, 2, 64), (8, 2, 128)]
_DECODE = {}


def _paged_case(dt, H, Hkv, Dh, seed=0):
    """Pools with every sequence's slots at a random permutation's pages; unused pages and the tail of each last page carry 0xFF scale bytes (NaN
    blocks), unused entries are -1.  `want`: every sequence alone through the dense MXFP4 kernel under an all-ones mask.  Computed once and shared."""
    key = (dt, H, Hkv, Dh, seed)
    if key in _DECODE:
        return _DECODE[key]
    g = torch.Generator().manual_seed(100 + seed)
    B = len(LENS)
    buf = (_rand(B, (H + 2 * Hkv) * Dh, seed=seed + 1) * 0.5).to(dt).to(DEV)         # q is read in place from a fused buffer: a row stride above H * Dh
    q = buf[:, :H * Dh]
    perm = torch.randperm(PAGES, generator=g).tolist()
    table = [[-1] * MAX_PAGES for _ in range(B)]
    pools = [_bytes(PAGES, Hkv, PAGE, Dh // 2, seed=seed + 5), torch.full((PAGES, Hkv, PAGE, Dh // 32), POISON, dtype=torch.uint8),
             _bytes(PAGES, Hkv, PAGE, Dh // 2, seed=seed + 6), torch.full((PAGES, Hkv, PAGE, Dh // 32), POISON, dtype=torch.uint8)]
    dense = []
    for b, n in enumerate(LENS):
        rows = _rows(Hkv, n, Dh, seed + 10 + 4 * b) + _rows(Hkv, n, Dh, seed + 12 + 4 * b)          # k_q, k_s, v_q, v_s
        dense.append([t[None].contiguous().to(DEV) for t in rows])
        for p in range((n + PAGE - 1) // PAGE):
            page = perm.pop()
            table[b][p] = page
            m = min(PAGE, n - p * PAGE)
            for pool, t in zip(pools, rows):
                pool[page, :, :m] = t[:, p * PAGE:p * PAGE + m]
    assert len(perm) == PAGES - 25
    scale = Dh ** -0.5
    want = torch.cat([_dense_decode(q[b:b + 1], d, H, LENS[b], scale) for b, d in enumerate(dense)])
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    _DECODE[key] = (q, [t.to(DEV) for t in pools], torch.tensor(table, dtype=torch.int32, device=DEV), dense, want)
    return _DECODE[key]


def _dense_decode(q1, d, H, n, scale, mask=None):
    """One sequence alone through the dense MXFP4 decode kernel: its slots as a (1, Hkv, n, ·) cache; zeros for an empty one."""
    if n == 0:
        return torch.zeros(1, q1.shape[1], dtype=q1.dtype, device=DEV)
    return ops.attention_decode_mxfp4kv(q1, *d, torch.ones(1, n, dtype=torch.uint8, device=DEV) if mask is None else mask, H, n, scale)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES)
def test_attention_decode_paged_mxfp4kv_equals_the_dense_kernel_sequence_by_sequence(dt, H, Hkv, Dh):
    q, pools, table, _, want = _paged_case(dt, H, Hkv, Dh)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    B, scale = len(LENS), Dh ** -0.5
    got = ops.attention_decode_paged_mxfp4kv(q, *pools, table, lens, H, 640, scale)    # the maximum length, which is the whole table row
    diff = (got.float() - want.float()).abs().max(dim=1).values.tolist()
    print(f"{dt} H={H} Hkv={Hkv} Dh={Dh}: largest difference per sequence {diff}")
    assert torch.equal(got, want), diff
    assert torch.equal(got[0], torch.zeros_like(got[0]))               # lens = 0: exact zeros
    # the table ends at the longest sequence (5 pages), so a max_len past every length needs a batch without it: the sequences up to 300 slots at
    # their maximum (2 chunks) and at the table's end (3 chunks: every row has trailing empty chunks)
    for max_len in (300, 640):
        part = ops.attention_decode_paged_mxfp4kv(q[:9], *pools, table[:9].contiguous(), lens[:9].contiguous(), H, max_len, scale)
        assert torch.equal(part, want[:9]), max_len
    ws = torch.full((ops.attention_decode_paged_mxfp4kv_workspace(B, H, Dh, 640),), float("nan"), device=DEV)
    out = torch.empty_like(want)
    assert ops.attention_decode_paged_mxfp4kv(q, *pools, table, lens, H, 640, scale, ws=ws, out=out) is out and torch.equal(out, want)   # a poisoned workspace
    for b in (4, 7, 9):                                                # the bits do not depend on the batch: a sequence alone, through its own table row
        one = ops.attention_decode_paged_mxfp4kv(q[b:b + 1], *pools, table[b:b + 1].contiguous(), lens[b:b + 1].contiguous(), H, LENS[b], scale)
        assert torch.equal(one, want[b:b + 1]), b


@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.float32, 4, 4, 32), (torch.bfloat16, 8, 2, 128), (torch.float16, 8, 2, 64)])
def test_attention_decode_paged_mxfp4kv_counts_no_key_of_a_page_that_is_no_page(dt, H, Hkv, Dh):
    """An out-of-range table entry is "no page": its 128 slots do not count, nothing is read through the id.  Entry 2 of the 640-slot sequence is the
    FIRST half of chunk 1 (waves 0-1), entry 1 of the 300-slot sequence the SECOND half of chunk 0 (waves 2-3), entry 4 of the 513-slot sequence its
    last slot: each is the dense kernel under a mask that is zero on that page - page-aligned, so the same partition of the keys."""
    q, pools, table, dense, want = _paged_case(dt, H, Hkv, Dh, seed=3)
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    scale = Dh ** -0.5
    want = want.clone()
    for b, entry in ((10, 2), (8, 1), (9, 4)):
        mask = torch.ones(1, LENS[b], dtype=torch.uint8, device=DEV)
        mask[:, entry * PAGE:(entry + 1) * PAGE] = 0
        want[b:b + 1] = _dense_decode(q[b:b + 1], dense[b], H, LENS[b], scale, mask)
    want[4] = 0                                                        # the 129-slot sequence loses both pages
    for bad in (-1, PAGES, 1 << 30):
        t = table.clone()
        t[10, 2], t[8, 1], t[9, 4] = bad, bad, bad
        t[4, 0], t[4, 1] = bad, bad
        got = ops.attention_decode_paged_mxfp4kv(q, *pools, t, lens, H, 640, scale)
        assert torch.equal(got, want), (bad, (got.float() - want.float()).abs().max(dim=1).values.tolist())


# ---- extend attention ------------------------------------------------------------------------------------------------------------------------------
LEN0 = [0, 100, 128, 250, 300]
POOL_X, MAX_PAGES_X = 16, 5                                            # at Tn = 40 the sequences own 1 + 2 + 2 + 3 + 3 = 11 pages
SHAPES_X = SHAPES + [(4, 2, 96)]                                       # 96: a head dim without a lane layout - the extend serves every multiple of 32
_EXTEND = {}


def _extend_case(dt, H, Hkv, Dh, Tn, seed=0):
    """(q, pools, table, len0, want, dense): every sequence's len0 old slots and Tn new ones - the dense quantiser's bytes for the k / v columns of the
    fused buffer q is read from - at a random permutation's pages; every slot at or above len0 + Tn and every unused page carries 0xFF scale bytes.
    `want`: every sequence alone through the dense MXFP4 extend under an all-ones mask.  Computed once per case and shared."""
    key = (dt, H, Hkv, Dh, Tn, seed)
    if key in _EXTEND:
        return _EXTEND[key]
    g = torch.Generator().manual_seed(200 + seed)
    B = len(LEN0)
    qkv = (_rand(B * Tn, (H + 2 * Hkv) * Dh, seed=seed + 1) * 0.5).to(dt).to(DEV)      # q is read in place: a row stride above H * Dh
    q = qkv[:, :H * Dh]
    new = [torch.zeros(B, Hkv, Tn, c, dtype=torch.uint8, device=DEV) for c in (Dh // 2, Dh // 32, Dh // 2, Dh // 32)]
    ops.kv_append_mxfp4(qkv, *new, Tn, H, 0)                          # the new rows as the quantiser stores them
    new = [t.cpu() for t in new]
    perm = torch.randperm(POOL_X, generator=g).tolist()
    table = [[-1] * MAX_PAGES_X for _ in range(B)]
    pools = [_bytes(POOL_X, Hkv, PAGE, Dh // 2, seed=seed + 5), torch.full((POOL_X, Hkv, PAGE, Dh // 32), POISON, dtype=torch.uint8),
             _bytes(POOL_X, Hkv, PAGE, Dh // 2, seed=seed + 6), torch.full((POOL_X, Hkv, PAGE, Dh // 32), POISON, dtype=torch.uint8)]
    dense = []
    for b, n in enumerate(LEN0):
        old = _rows(Hkv, n, Dh, seed + 10 + 4 * b) + _rows(Hkv, n, Dh, seed + 12 + 4 * b)
        rows = [torch.cat([o, t[b]], dim=1) for o, t in zip(old, new)]               # (Hkv, n + Tn, ·)
        dense.append([t[None].contiguous().to(DEV) for t in rows])
        for p in range((n + Tn + PAGE - 1) // PAGE):
            page = perm.pop()
            table[b][p] = page
            m = min(PAGE, n + Tn - p * PAGE)
            for pool, t in zip(pools, rows):
                pool[page, :, :m] = t[:, p * PAGE:p * PAGE + m]
    assert perm, "the pool has spare pages"
    scale = Dh ** -0.5
    want = torch.cat([ops.attention_extend_mxfp4kv(q[b * Tn:(b + 1) * Tn], *dense[b], torch.ones(1, n + Tn, dtype=torch.uint8, device=DEV), H, Tn, n, scale)
                      for b, n in enumerate(LEN0)])
    torch.cuda.synchronize()
    assert torch.isfinite(want).all()
    _EXTEND[key] = (q, [t.to(DEV) for t in pools], torch.tensor(table, dtype=torch.int32, device=DEV), torch.tensor(LEN0, dtype=torch.int32, device=DEV),
                    want, dense)
    return _EXTEND[key]


@pytest.mark.parametrize("Tn", [1, 5, 40])                             # 250 + 40 and 100 + 40 cross a page, 250 + 40 the 256-slot chunk too
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("H,Hkv,Dh", SHAPES_X)
def test_attention_extend_paged_mxfp4kv_equals_the_dense_kernel_sequence_by_sequence(dt, H, Hkv, Dh, Tn):
    q, pools, table, len0, want, _ = _extend_case(dt, H, Hkv, Dh, Tn)
    B, scale = len(LEN0), Dh ** -0.5
    for max_len0 in (max(LEN0), MAX_PAGES_X * PAGE - Tn):              # the table's end: every sequence has trailing empty chunks
        got = ops.attention_extend_paged_mxfp4kv(q, *pools, table, len0, H, Tn, max_len0, scale)
        diff = (got.float() - want.float()).abs().reshape(B, -1).max(dim=1).values.tolist()
        print(f"{dt} H={H} Hkv={Hkv} Dh={Dh} Tn={Tn} max_len0={max_len0}: largest difference per sequence {diff}")
        assert torch.equal(got, want), (max_len0, diff)
    ws = torch.full((ops.attention_extend_paged_mxfp4kv_workspace(B, Tn, H, Dh, MAX_PAGES_X * PAGE - Tn),), float("nan"), device=DEV)
    out = torch.empty_like(want)
    assert ops.attention_extend_paged_mxfp4kv(q, *pools, table, len0, H, Tn, MAX_PAGES_X * PAGE - Tn, scale, ws=ws, out=out) is out
    assert torch.equal(out, want)                                      # a poisoned workspace, a caller's out
    for b in (0, 3):                                                   # the bits do not depend on the batch: a sequence alone, through its own table row
        one = ops.attention_extend_paged_mxfp4kv(q[b * Tn:(b + 1) * Tn], *pools, table[b:b + 1].contiguous(), len0[b:b + 1].contiguous(), H, Tn, LEN0[b],
                                                 scale)
        assert torch.equal(one, want[b * Tn:(b + 1) * Tn]), b
    idle = len0.clone()
    idle[1] = -1                                                       # an idle sequence: exact zeros, the others unchanged
    got = ops.attention_extend_paged_mxfp4kv(q, *pools, table, idle, H, Tn, max(LEN0), scale)
    assert torch.equal(got[Tn:2 * Tn], torch.zeros_like(got[Tn:2 * Tn])) and torch.equal(got[2 * Tn:], want[2 * Tn:]) and torch.equal(got[:Tn], want[:Tn])


@pytest.mark.parametrize("Tn", [5, 40])
@pytest.mark.parametrize("dt,H,Hkv,Dh", [(torch.float32, 4, 4, 32), (torch.bfloat16, 8, 2, 128), (torch.float16, 4, 2, 96)])
def test_attention_extend_paged_mxfp4kv_counts_no_key_of_a_page_that_is_no_page(dt, H, Hkv, Dh, Tn):
    """The 300-slot sequence without its middle page is the dense kernel under a mask that is zero on [128, 256), the 250-slot sequence without its
    first page under one that is zero on [0, 128) - page-aligned, so the same chunks; the 100-slot sequence without any page gives zeros."""
    q, pools, table, len0, want, dense = _extend_case(dt, H, Hkv, Dh, Tn, seed=3)
    scale = Dh ** -0.5
    want = want.clone()
    for b, entry in ((4, 1), (3, 0)):
        mask = torch.ones(1, LEN0[b] + Tn, dtype=torch.uint8, device=DEV)
        mask[:, entry * PAGE:(entry + 1) * PAGE] = 0
        want[b * Tn:(b + 1) * Tn] = ops.attention_extend_mxfp4kv(q[b * Tn:(b + 1) * Tn], *dense[b], mask, H, Tn, LEN0[b], scale)
    want[Tn:2 * Tn] = 0
    for bad in (-1, POOL_X, 1 << 30):
        t = table.clone()
        t[4, 1], t[3, 0] = bad, bad
        t[1, 0], t[1, 1] = bad, bad
        got = ops.attention_extend_paged_mxfp4kv(q, *pools, t, len0, H, Tn, max(LEN0), scale)
        assert torch.equal(got, want), bad


# ---- batcher ---------------------------------------------------------------------------------------------------------------------------------------
# test_paged_gpu.py's tiny Llamas at head dims that are multiples of 32
CONFIGS = {"dh32": dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4, vocab_size=100),
           "dh128": dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1, vocab_size=100)}
PROMPTS, NEW = (3, 120, 127, 130, 250, 260, 40), (12, 10, 5, 3, 8, 4, 8)  # 120 + 10 and 127 + 5 decode across a page, 250 + 8 across the 256-slot chunk; 130 and 260 start past them
ROWS, POOL, MAX_PAGES_B = 2, 4, 3                                      # seven requests on two rows; a 3-page request leaves one page: the next 2-page request waits
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


def _prompts(name, dt, seed):
    D = CONFIGS[name]["hidden_size"]
    return [_rand(T, D, seed=1000 * seed + i).to(dt).to(DEV) for i, T in enumerate(PROMPTS)]


def _generate(m, x, n, **kw):
    out = m.generate(inputs_embeds=x[None], max_new_tokens=n, kv_cache="mxfp4", return_dict_in_generate=True, output_logits=True, **kw)
    top = out.logits[0].float().topk(2, dim=-1).values
    return out.sequences[0], float(((top[:, 0] - top[:, 1]) / out.logits[0].float().abs().amax(dim=-1)).min())


def _alone(name, dt, seed, eos=None):
    """Every request alone through the dense `generate(kv_cache="mxfp4")` (computed once per case and shared): (tokens, smallest top-2 margin)."""
    key = (name, dt, seed, eos)
    if key not in _ALONE:
        m, toks, margin = _model(name, dt, seed), [], float("inf")
        for x, n in zip(_prompts(name, dt, seed), NEW):
            t, mg = _generate(m, x, n, eos_token_id=eos)
            toks.append(t)
            margin = min(margin, mg)
        _ALONE[key] = (toks, margin)
    return _ALONE[key]


def _mxfp4_batcher(m, rows, pool, max_pages, eos=None):
    cache = PagedKVCache.for_model(m.model, rows, pool, max_pages, kv_format="mxfp4")
    for layers in (cache.k_q, cache.k_s, cache.v_q, cache.v_s):
        for t in layers:
            t.fill_(POISON)                                            # nothing may depend on what a pool holds: every unwritten block is a NaN block
    return ContinuousBatcher(m, rows, cache=cache, eos_token_id=eos)


def _batched(name, dt, seed, eos=None):
    b = _mxfp4_batcher(_model(name, dt, seed), ROWS, POOL, MAX_PAGES_B, eos)
    return b, b.run(list(zip(_prompts(name, dt, seed), NEW)))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_continuous_batching_over_mxfp4_pages_equals_each_request_alone(name, dt):
    want, margin = _alone(name, dt, 5)
    print(f"{name} {dt}: smallest top-2 margin of the alone runs {margin:.3e}")
    b, got = _batched(name, dt, 5)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    assert [g.numel() for g in got] == list(NEW)
    st, c = b.stats, b.cache
    assert st["admitted"] == len(PROMPTS) and st["admitted_midflight"] >= 1 and st["page_waits"] >= 1 and st["pages_reused"] >= 1
    assert c.pages_free == POOL and c.lens.tolist() == [0] * ROWS and c.block_table.tolist() == [[-1] * MAX_PAGES_B] * ROWS
    kw = CONFIGS[name]
    Dh = kw["hidden_size"] // kw["num_attention_heads"]
    assert c.kv_format == "mxfp4" and c.k == [] and c.v == []
    assert c.nbytes() == 2 * kw["num_hidden_layers"] * POOL * kw["num_key_value_heads"] * 128 * (Dh // 2 + Dh // 32) == POOL * c.page_nbytes
    eos = int(want[0][want[0].numel() // 2])                           # a token the first request emits mid-sequence: as an eos it cuts it short
    want_e, _ = _alone(name, dt, 5, eos=eos)
    assert any(w.numel() < n for w, n in zip(want_e, NEW))
    _, got_e = _batched(name, dt, 5, eos=eos)
    assert [g.tolist() for g in got_e] == [w.tolist() for w in want_e]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_continuous_batching_over_mxfp4_pages_equals_each_request_alone_in_fp32(name):
    """Tokens are compared, so no selection may sit on a coin flip: the first seed whose alone runs keep the fixtures' top-2 margin is the case."""
    for seed in (5, 6, 7, 8, 9, 10):
        want, margin = _alone(name, torch.float32, seed)
        print(f"{name} fp32 seed {seed}: smallest top-2 margin of the alone runs {margin:.3e}")
        if margin >= MIN_MARGIN:
            break
    assert margin >= MIN_MARGIN
    _, got = _batched(name, torch.float32, seed)
    assert [g.tolist() for g in got] == [w.tolist() for w in want]


P_A = 140                                                              # a prefix of one shared page and a tail of 12 rows
REQUESTS_P = ((True, 3, 6), (True, 100, 5), (False, 50, 7), (True, 40, 4))    # (behind the prefix?, remainder rows, max_new_tokens); 12 + 100 <= 128: one extend window


@pytest.mark.parametrize("name,dt", [("dh128", torch.bfloat16), ("dh32", torch.float16)])
def test_requests_behind_a_shared_prefix_in_mxfp4_pages_equal_each_request_alone(name, dt):
    """A prefixed request attends over the prefix's stored, quantised slots: the tokens of `generate(kv_cache="mxfp4", prefill_chunk=Ps)`."""
    m, D = _model(name, dt, 5), CONFIGS[name]["hidden_size"]
    prefix = _rand(P_A, D, seed=5090).to(dt).to(DEV)
    rest = [_rand(S, D, seed=5100 + i).to(dt).to(DEV) for i, (_, S, _) in enumerate(REQUESTS_P)]
    want = [_generate(m, torch.cat([prefix, x]), n, prefill_chunk=PAGE)[0] if pre else _generate(m, x, n)[0] for (pre, _, n), x in zip(REQUESTS_P, rest)]
    pool = 4
    b = _mxfp4_batcher(m, 2, pool, 3)
    h = b.register_prefix(prefix)
    assert len(h.pages) == 1 and b.cache.pages_free == pool - 1
    got = b.run([(x, n, h) if pre else (x, n) for (pre, _, n), x in zip(REQUESTS_P, rest)])
    assert [g.tolist() for g in got] == [w.tolist() for w in want]
    assert b.prefix_stats == dict(registered=1, hits=3, slots_shared=3 * 128) and b.cache.pages_free == pool - 1
    b.drop_prefix(h)
    assert b.cache.pages_free == pool and sorted(b.cache._free) == list(range(pool)) and b.cache.page_refs == [0] * pool
    assert b.cache.block_table.tolist() == [[-1] * 3] * 2 and b.cache.lens.tolist() == [0, 0]


def test_the_ops_refuse_a_head_dim_without_a_lane_layout_over_nibble_rows():
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=DEV)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=DEV)
    pools = (z(1, 1, PAGE, 48), z(1, 1, PAGE, 3), z(1, 1, PAGE, 48), z(1, 1, PAGE, 3))                 # head dim 96
    with pytest.raises(RuntimeError, match="unsupported head dim 96"):
        ops.attention_decode_paged_mxfp4kv(torch.zeros(1, 96, dtype=torch.bfloat16, device=DEV), *pools, i32(1, 1), i32(1), 1, 0, 1.0)
    with pytest.raises(RuntimeError, match="unsupported head dim 96"):
        ops.kv_append_paged_mxfp4(torch.zeros(1, 3 * 96, dtype=torch.bfloat16, device=DEV), *pools, i32(1, 1), i32(1), 1, 1)
