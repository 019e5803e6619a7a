"""The MFMA extend attention over MXFP4 KV caches, dense and paged, on a real MI355X (include/setok_hip.h, "MXFP4 KV cache" and "Paged MXFP4 KV
cache"; csrc/attn_extend.hip, csrc/attn_extend_paged.hip).  In the 16-bit type at head dim 128 setok_attention_extend_gqa_mxfp4kv and
setok_attention_extend_gqa_paged_mxfp4kv run the native MFMA kernel's tile arithmetic on tiles converted from nibbles, so their output BITS are the
native entries' over caches that hold K', V' = value(nibble) * 2^(scale byte - 127): every comparison here is torch.equal against the native
kernel, none carries a tolerance.  Live rows come from the oracle quantiser (tests/mxfp4_cases.py), so K', V' are exact in bf16 and fp16; dead
slots — masked, or at / above len0 + Tn — hold 0xFF nibbles under 0xFF scale bytes (the converter's NaN) in the MXFP4 tensors and NaN in the
native ones.  Everything else (fp32, other head dims) stays on the wave-per-chunk kernel: the guard at the end.  `pytest -m gpu`."""
import functools

import pytest
import torch

import mxfp4kv_cases as K
import test_cache_attn_programs_gpu as G
from test_attn_programs_gpu import _Cases, _bounds32
from test_extend_gpu import _extend_problem, _extend_ref, _rel, _tol
from test_mxfp4kv_gpu import _arm_path, _case, _extend_mx

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib, ops

DEV = "cuda"
LOW = [torch.bfloat16, torch.float16]
IDS = ["bf16", "fp16"]
DH = 128
PAGE = K.define("SETOK_KV_PAGE")


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ---- dense ---------------------------------------------------------------------------------------------------------------------------------------
# (H, Hkv, Tn, len0), the smallest that reach each branch of the MFMA kernel
DENSE = [(8, 1, 4, 253),       # NW = 1 (G * Tn = 32 rows), two chunks, the tile [256, 288) straddles top = 257
         (8, 1, 1, 0),         # one row, one slot
         (8, 1, 17, 248),      # NW = 4 (136 rows): two m-blocks, the second ragged; one 1024-slot span that holds two chunks
         (8, 1, 5, 1030),      # 40 rows, 1035 slots: two spans, so two partials and a merge
         (2, 2, 40, 1000),     # G = 1: the waves of rows 0..31 skip the tiles of later rows
         (4, 2, 3, 31)]        # a single tile that the new rows complete


@functools.lru_cache(maxsize=None)
def _dense_problem(H, Hkv, Tn, len0):
    """(q fp32, k_q, k_s, v_q, v_s, mask, K' fp64, V' fp64) on the CPU: four sequences — all keys, left-padded, right-padded, fully masked — over
    mxfp4kv_cases.cache_rows (the oracle quantiser's rows), cap = len0 + Tn + 5; every dead slot 0xFF / 0xFF, mask bytes past len0 + Tn are 1."""
    B, n = 4, len0 + Tn
    cap = n + 5
    q = _rand(B * Tn, (H + 2 * Hkv) * DH, seed=7 * len0 + Tn)                   # read in place: a row stride above H * Dh
    k_q, k_s, v_q, v_s = [t.clone() for t in K.cache_rows(B, Hkv, cap, DH, 31 * len0 + Tn)]
    mask = torch.zeros(B, cap, dtype=torch.uint8)
    mask[0, :n] = 1
    mask[1, n // 3:n] = 1
    mask[2, :n - n // 4] = 1
    dead = (mask == 0)[:, None, :].expand(B, Hkv, cap).clone()
    dead[:, :, n:] = True
    mask[:, n:] = 1                                                             # (not a licence to read)
    for t in (k_q, k_s, v_q, v_s):
        t[dead] = 0xFF
    return q, k_q, k_s, v_q, v_s, mask, K.dequant(k_q, k_s), K.dequant(v_q, v_s)


@pytest.mark.parametrize("dt", LOW, ids=IDS)
@pytest.mark.parametrize("H,Hkv,Tn,len0", DENSE)
def test_dense_mxfp4_extend_has_the_native_kernels_bits(dt, H, Hkv, Tn, len0):
    """Fails on the parent commit, whose MXFP4 extend is the wave-per-chunk kernel (another summation order, the probabilities rounded per slot).
    Elements that differed there, bf16 / fp16: (8,1,4,253) 2200 / 2229 of 16384; (8,1,1,0) 0 / 0 of 4096 (one slot: the output is V' itself);
    (8,1,17,248) 9302 / 9466 of 69632; (8,1,5,1030) 3767 / 3781 of 20480; (2,2,40,1000) 7674 / 7417 of 40960; (4,2,3,31) 2 / 0 of 6144.  The paged
    comparison below differed in 391 ... 27102 elements (10 - 13 %) of every case, the model's step-0 logits in 184 and 179 of 256."""
    q, k_q, k_s, v_q, v_s, mask, kd, vd = _dense_problem(H, Hkv, Tn, len0)
    assert bool(torch.isnan(kd[:, :, len0 + Tn:]).all()) and bool(torch.isnan(vd[3]).all())
    dq, dm, scale = q.to(dt).to(DEV), mask.to(DEV), DH ** -0.5
    got = ops.attention_extend_mxfp4kv(dq, k_q.to(DEV), k_s.to(DEV), v_q.to(DEV), v_s.to(DEV), dm, H, Tn, len0, scale)
    want = ops.attention_extend(dq, kd.to(dt).to(DEV), vd.to(dt).to(DEV), dm, H, Tn, len0, scale)
    differ = int((got != want).sum())
    print(f"mxfp4 extend against the native kernel {dt} H={H} Hkv={Hkv} Tn={Tn} len0={len0}: {differ} of {got.numel()} elements differ")
    assert bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(want.float()).all())
    assert torch.equal(got, want), differ
    rows = got.reshape(4, Tn, H * DH)
    assert torch.equal(rows[3], torch.zeros_like(rows[3]))                      # the fully masked sequence: exact zeros


# ---- paged ---------------------------------------------------------------------------------------------------------------------------------------
P_LEN0 = [37, 128, -1, 250, 300]            # four live sequences (one ends on a page edge before the new rows) and an idle one
POOL, MAX_PAGES = 12, 3                     # at Tn = 40 the live sequences own 1 + 2 + 3 + 3 = 9 pages


@functools.lru_cache(maxsize=None)
def _paged_problem(H, Hkv, Tn):
    """(q fp32, MXFP4 pools, their fp64 meaning, table, len0) on the CPU: every live sequence's len0 + Tn rows of mxfp4kv_cases.cache_rows at the
    pages of a shuffled table; every other slot of the pools — the tails of last pages, the unused pages — 0xFF / 0xFF."""
    g = torch.Generator().manual_seed(1000 + Tn)
    B = len(P_LEN0)
    q = _rand(B * Tn, (H + 2 * Hkv) * DH, seed=90 + Tn)
    rows = K.cache_rows(B, Hkv, max(P_LEN0) + Tn, DH, 300 + Tn)
    pools = [torch.full((POOL, Hkv, PAGE, c), 0xFF, dtype=torch.uint8) for c in (DH // 2, DH // 32, DH // 2, DH // 32)]
    perm = torch.randperm(POOL, generator=g).tolist()
    table = [[-1] * MAX_PAGES for _ in range(B)]
    for b, n0 in enumerate(P_LEN0):
        if n0 < 0:
            continue
        n = n0 + Tn
        for p in range((n + PAGE - 1) // PAGE):
            table[b][p] = perm.pop()
            m = min(PAGE, n - p * PAGE)
            for pool, t in zip(pools, rows):
                pool[table[b][p], :, :m] = t[b, :, p * PAGE:p * PAGE + m]
    assert perm, "the pool has spare pages"
    return (q, pools, (K.dequant(pools[0], pools[1]), K.dequant(pools[2], pools[3])), torch.tensor(table, dtype=torch.int32),
            torch.tensor(P_LEN0, dtype=torch.int32))


@pytest.mark.parametrize("dt", LOW, ids=IDS)
@pytest.mark.parametrize("Tn", [3, 40])
@pytest.mark.parametrize("H,Hkv", [(8, 1), (2, 2)])
def test_paged_mxfp4_extend_has_the_native_paged_kernels_bits(dt, H, Hkv, Tn):
    """Over the shuffled table, then with the 300-slot sequence's middle page replaced by -1 and by num_pages (no page: none of its keys count and
    no address is formed from the id), each time against the native paged kernel over pools that hold the dequantised pages, given the same table.
    Both workspaces start as NaN.  Fails on the parent commit (the wave-per-chunk kernel)."""
    q, pools, (kd, vd), table, len0 = _paged_problem(H, Hkv, Tn)
    B, scale, max_len0 = len(P_LEN0), DH ** -0.5, max(P_LEN0)
    dq, dl = q.to(dt).to(DEV), len0.to(DEV)
    mx = [t.to(DEV) for t in pools]
    kn, vn = kd.to(dt).to(DEV), vd.to(dt).to(DEV)
    ws_mx = torch.empty(ops.attention_extend_paged_mxfp4kv_workspace(B, Tn, H, DH, max_len0), device=DEV)
    ws_n = torch.empty(ops.attention_extend_paged_workspace(B, Tn, H, DH, max_len0, Hkv, dt), device=DEV)
    for bad in (None, -1, POOL):
        t = table.clone()
        if bad is not None:
            t[4, 1] = bad
        t = t.to(DEV)
        ws_mx.fill_(float("nan"))
        ws_n.fill_(float("nan"))
        got = ops.attention_extend_paged_mxfp4kv(dq, *mx, t, dl, H, Tn, max_len0, scale, ws=ws_mx)
        want = ops.attention_extend_paged(dq, kn, vn, t, dl, H, Tn, max_len0, scale, ws=ws_n)
        differ = int((got != want).sum())
        print(f"paged mxfp4 extend against the native paged kernel {dt} H={H} Hkv={Hkv} Tn={Tn} page {bad}: {differ} of {got.numel()} elements differ")
        assert bool(torch.isfinite(got.float()).all()) and bool(torch.isfinite(want.float()).all())
        assert torch.equal(got, want), (bad, differ)
        assert torch.equal(got[2 * Tn:3 * Tn], torch.zeros_like(got[2 * Tn:3 * Tn]))        # the idle sequence: exact zeros
        if bad is None:
            whole = got
        else:
            assert torch.equal(got[:4 * Tn], whole[:4 * Tn]) and not torch.equal(got[4 * Tn:], whole[4 * Tn:])    # only that sequence lost keys


# ---- model level ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", [("gqa_dh128", torch.bfloat16), ("mqa_dh128_left", torch.float16)])
def test_chunked_prefill_over_an_mxfp4_cache_has_the_fake_quantised_native_arms_logits(name, dt):
    """generate(prefill_chunk=4): every window after the first attends through the extend kernel — over nibbles here, over the round-tripped native
    cache in the arm; the first window and the arm's append are the same function on both sides.  So the step-0 logits are equal bit for bit (on
    the parent commit only the fp32 comparison at 1e-4 held)."""
    m, x, am, _ = _case(name, dt)
    assert x.shape[1] > 8                                              # at least two windows behind the first
    kw = dict(inputs_embeds=x, attention_mask=am, max_new_tokens=1, prefill_chunk=4, return_dict_in_generate=True, output_logits=True)
    with _arm_path():
        arm = m.generate(**kw)
    out = m.generate(kv_cache="mxfp4", **kw)
    a, b = out.logits[:, 0], arm.logits[:, 0]
    print(f"{name} {dt} step-0 logits, prefill_chunk=4, mxfp4 cache against the arm: {int((a != b).sum())} of {a.numel()} differ")
    assert bool(torch.isfinite(a.float()).all())
    assert torch.equal(a, b)


# ---- the functional path is still the functional path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,Dh", [(torch.float32, 128), (torch.bfloat16, 32), (torch.bfloat16, 96)], ids=["fp32-128", "bf16-32", "bf16-96"])
def test_fp32_and_other_head_dims_stay_on_the_wave_per_chunk_kernel(dt, Dh):
    """Passes before and after the MFMA path: equal bits on a second run, zeros for rows that count no key, and the error against fp64 over K', V'
    inside test_mxfp4kv_gpu.py's bound (_tol; in fp32 also four times torch's own fp32 error, _bounds32)."""
    H, Hkv = 8, 2
    for len0, Tn in ((253, 4), (248, 17)):
        q, k, v, mask = _extend_problem(dt, H, Hkv, Dh, len0, Tn, len0 + Tn + 5, seed=500 + len0 + Tn)
        got, kd, vd = _extend_mx(q, k, v, mask, H, Tn, len0, Dh)
        assert torch.equal(_extend_mx(q, k, v, mask, H, Tn, len0, Dh)[0], got), (len0, Tn)
        ref = _extend_ref(q, kd, vd, mask, H, Hkv, Dh, len0, Tn)
        err, tol = _rel(got, ref), _tol(dt, Dh)
        print(f"functional mxfp4 extend {dt} Dh={Dh} len0={len0} Tn={Tn}: max-rel {err:.3e} (tol {tol:.0e})")
        assert bool(torch.isfinite(got.float()).all()) and err < tol, (len0, Tn, err)
        if dt == torch.float32:
            cases = _Cases()
            cases.check(f"functional mxfp4 extend fp32 Dh={Dh} len0={len0} Tn={Tn}", got, ref, Dh,
                        *_bounds32(G._extend_ref32(q, kd, vd, mask, H, Hkv, Dh, len0, Tn), ref, Dh))
            cases.done()
        rows = got.reshape(4, Tn, H * Dh)
        assert torch.equal(rows[3], torch.zeros_like(rows[3])) and torch.equal(rows[2, 0], torch.zeros_like(rows[2, 0]))


# ---- refusal -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", LOW, ids=IDS)
def test_a_grid_the_mfma_kernel_cannot_launch_is_refused_before_anything_runs(dt):
    """Hkv * ceil(G * Tn / 128) = 512 * 129 > 65535 blocks in y: SETOK_EINVAL naming the grid from both entries, the output untouched.  Nothing is
    launched, so the operands need not have the call's sizes: the checks read shapes and pointers only.  (The workspace is stated as 16 floats: a
    library without the grid check refuses the call for that, with another message, and launches nothing either.)"""
    H = Hkv = 512
    Tn = 128 * 128 + 1
    l = _lib.load(dt == torch.float16)
    code = 2 if dt == torch.float16 else 1
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.full((4096,), 7, dtype=torch.uint8, device=DEV)
    idx = torch.zeros(16, dtype=torch.int32, device=DEV)
    ws = torch.zeros(16, device=DEV)
    p = buf.data_ptr()
    rc = l.setok_attention_extend_gqa_mxfp4kv(None, code, p, H * DH, p, p, p, p, p, out.data_ptr(), 1, Tn, H, Hkv, DH, Tn, 0, 0.1, ws.data_ptr(), 16)
    assert rc == -1 and b"setok_attention_extend_mxfp4kv" in l.setok_last_error() and b"launch grid" in l.setok_last_error(), l.setok_last_error()
    rc = l.setok_attention_extend_gqa_paged_mxfp4kv(None, code, p, H * DH, p, p, p, p, idx.data_ptr(), 1 + Tn // PAGE, 4, idx.data_ptr(), out.data_ptr(), 1,
                                                    Tn, H, Hkv, DH, 0, 0.1, ws.data_ptr(), 16)
    assert rc == -1 and b"setok_attention_extend_paged_mxfp4kv" in l.setok_last_error() and b"launch grid" in l.setok_last_error(), l.setok_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    # one block fewer in y is a grid the kernel takes: the same arguments are then refused for their workspace, after the grid check
    rc = l.setok_attention_extend_gqa_mxfp4kv(None, code, p, H * DH, p, p, p, p, p, out.data_ptr(), 1, 127 * 128, H, Hkv, DH, 127 * 128, 0, 0.1,
                                              ws.data_ptr(), 16)
    assert rc == -1 and b"workspace of" in l.setok_last_error(), l.setok_last_error()
