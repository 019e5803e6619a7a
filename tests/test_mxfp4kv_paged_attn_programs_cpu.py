"""The score programs do to the MXFP4-cache and paged attention kernels what tests/test_mxfp4kv_attn_programs_gpu.py and
tests/test_paged_attn_programs_gpu.py need of them — checked on the CPU, on the problems those modules build.

MXFP4 cache: an MX block holds {0, .5, 1, 1.5, 2, 3, 4, 6} * 2^e, so only some offsets survive the quantiser (test_values_an_mx_block_carries);
the programs of the GPU module use only those, K'[:, 0] is the program's offset bit for bit, and the stair climbs through the scale byte of block 0.
`attn_programs.emulate_chunked` over K', V' — the (256, 64) walk of the decode kernel at head dims 32 / 64 / 128, the (256, 256) walk of the generic
kernel and of extend — reaches a rescale <= e^-8 inside a chunk and a merge factor <= e^-8 exactly where the geometry says so, stays below
HEADROOM < `_tol` in both 16-bit types, and under the two planted errors of the emulator (never of a kernel) exceeds 1e-2 per row wherever the walk
has the step; where it has not, the flag changes no bit.  The emulator uses torch's exp2 in place of the device's: its figures show the bound
attainable, they are not bounds.

Paged: the kernels are held to their dense twins bit for bit, so no arithmetic model is needed.  What is checked here is the test's own
construction: the page-aligned masks the dense twin gets and the tables the paged kernel gets describe the same counted set, every table case
leaves the sequences meant to keep keys with at least one, and every poisoned slot — NaN V, a hot K row past the end, the spare pages — lies outside
every counted set."""
import math

import pytest
import torch

import attn_programs as AP
import mxfp4_cases as M
import mxfp4kv_cases as K
import test_cache_attn_programs_cpu as C
import test_cache_attn_programs_gpu as G
import test_extend_gpu as X
import test_mxfp4kv_attn_programs_gpu as MG
import test_paged_attn_programs_gpu as PG

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
LOW = [BF, HF]
E8, HEADROOM = C.E8, C.HEADROOM
MX_DECODE16 = [(dt, Dh, H, Hkv, n) for dt in LOW for Dh, H, Hkv in MG.MX_SHAPES for n in MG.MX_LENS]
MX_EXTEND16 = [c for c in MG.MX_EXTEND_CASES if c[0] != F32]
CARRIED = (0.0, 8.0, 16.0, 24.0, 32.0, 48.0, 64.0, 96.0, 128.0, 192.0, 256.0, -64.0)
NOT_CARRIED = ((40.0, 32.0), (56.0, 48.0), (72.0, 64.0), (272.0, 256.0), (-60.0, -48.0))


# ---- what an MX block carries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Dh", [32, 64, 96, 128])
def test_values_an_mx_block_carries(Dh):
    """A steered k[:, 0] over 0.5 randn comes back bit for bit at the offsets the MXFP4 programs use, and does not at 40, 56, 72, 272 and -60."""
    vals = torch.tensor(CARRIED + tuple(-v for v in CARRIED[1:5]) + tuple(v for v, _ in NOT_CARRIED))
    k = 0.5 * torch.randn(len(vals), Dh, generator=torch.Generator().manual_seed(Dh))
    k[:, 0] = vals
    back = K.dequant(*K.quantize_cache(k))[:, 0]
    want = torch.tensor(CARRIED + tuple(-v for v in CARRIED[1:5]) + tuple(w for _, w in NOT_CARRIED), dtype=torch.float64)
    assert torch.equal(back, want), (back.tolist(), want.tolist())


# ---- the problems of the GPU module ------------------------------------------------------------------------------------------------------------------
def _decode_runs(dt, Dh, H, Hkv, n):
    for program, tile in MG.mx_programs(n):
        qkv, k_q, k_s, v_q, v_s, mask = MG.mx_problem(dt, Dh, H, Hkv, n, program, tile, seed=700 + n)
        kd, vd = K.dequant(k_q, k_s), K.dequant(v_q, v_s)
        yield program, tile, qkv, kd, vd, mask, G._decode_ref(qkv, kd, vd, mask, H, Hkv, Dh, n)


def _extend_runs(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    mask, counts = G.extend_mask(*case)
    for program, tile in MG.mx_extend_programs(*case):
        q, k_q, k_s, v_q, v_s = MG.mx_extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile, mask, seed=len0 + Tn)
        kd, vd = K.dequant(k_q, k_s), K.dequant(v_q, v_s)
        yield program, tile, q, kd, vd, mask, counts, X._extend_ref(q, kd, vd, mask, H, Hkv, Dh, len0, Tn)


def _emulate_extend(case, q, kd, vd, counts, fault=None):
    """emulate_chunked over an MXFP4 extend problem: one softmax per 256-slot chunk, whatever the type and head dim."""
    dt, Dh, H, Hkv, Tn, len0 = case
    B, n, Gq = 4, len0 + Tn, H // Hkv
    qq = q[:, :H * Dh].reshape(B, Tn, Hkv, Gq, Dh).permute(0, 2, 1, 3, 4).reshape(B, Hkv, Tn * Gq, Dh)
    cc = counts[:, None, :, None, :].expand(B, Hkv, Tn, Gq, n).reshape(B, Hkv, Tn * Gq, n)
    out, resc, merge = AP.emulate_chunked(qq, kd[:, :, :n], vd[:, :, :n], cc, Dh ** -0.5, dt, MG.XC, MG.XC, fault)
    return out.reshape(B, Hkv, Tn, Gq, Dh).permute(0, 2, 1, 3, 4).reshape(B * Tn, H * Dh), resc, merge


def _expected(program, stair_tile, n, span, tile):
    """test_cache_attn_programs_cpu._expected; a level shift raises nothing.  Where the last partial of a stair holds fewer keys than a 32-key tile
    (one key at 257 slots, nine at 265) no claim is made about the merge, for the reason given there: the maximum of a few keys' noise against that of
    256 decides the side of e^-8 (the factor is printed: e^-8.0 to e^-7.5)."""
    if program == "shift-64":
        return False, False
    resc, merge = C._expected(program, stair_tile, n, span, tile)
    return resc, (None if program in AP.STAIRS and (n - 1) % span + 1 < 32 else merge)


# ---- the offsets survive the quantiser ------------------------------------------------------------------------------------------------------------------
def _check_offsets(kd, k_s, mask, g, n, program, tile):
    """Every slot that counts for somebody (and a heated dead one) holds the program's offset in K'[:, 0]; every other slot holds no finite key
    of the program's scale (a 0xFF block is NaN, a 0x00 scale byte 2^-127)."""
    cap = kd.shape[2]
    live = (mask != 0) & (torch.arange(cap) < n)[None]
    if program.startswith("hot@") and AP.hot_key(program, cap) < cap:
        live[:, AP.hot_key(program, cap)] = True                       # heated: finite in every sequence, the dead ones included
    live = live[:, None].expand(kd.shape[:3])
    assert not bool((kd[..., 0][~live].abs() > 1e-30).any()), (program, tile)
    assert torch.equal(kd[..., 0][live], g[None, None].expand_as(kd[..., 0])[live]), (program, tile)
    assert bool(live[0, :, :n].all()), (program, tile)                 # the whole sequence: every slot below n is checked
    if program == "stair8":
        lv = [k_s[0, 0, j * tile:min(n, (j + 1) * tile), 0].float().mean() for j in range((n + tile - 1) // tile)]
        assert all(b >= a for a, b in zip(lv, lv[1:])) and lv[1] > lv[0] + 1 and (len(lv) < 4 or lv[-1] > lv[1]), lv      # the scale byte of block 0 climbs with the stair (16 and 24 share one)


@pytest.mark.parametrize("Dh,H,Hkv", MG.MX_SHAPES)
@pytest.mark.parametrize("n", MG.MX_LENS)
def test_offsets_survive_the_mx_quantiser_in_the_decode_problem(Dh, H, Hkv, n):
    used = set()
    for program, tile in MG.mx_programs(n):
        _, k_q, k_s, v_q, v_s, mask = MG.mx_problem(F32, Dh, H, Hkv, n, program, tile, seed=700 + n)
        g = AP.offsets(n + 5, program, tile).double()
        _check_offsets(K.dequant(k_q, k_s), k_s, mask, g, n, program, tile)
        used |= set(g.tolist())
        if program.startswith("hot@"):                                 # a heated dead slot: finite K under a V row whose scale bytes are 0xFF
            p = AP.hot_key(program, n + 5)
            dead = (mask[:, p] == 0) | (p >= n)
            assert bool((v_s[dead][:, :, p] == M.NAN_SCALE).all()) and bool(dead[3])
    assert used <= set(CARRIED) | {-8.0, -16.0, -24.0, -32.0}, used


@pytest.mark.parametrize("case", MG.MX_EXTEND_CASES, ids=G._case_id)
def test_offsets_survive_the_mx_quantiser_in_the_extend_problem(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    n, used = len0 + Tn, set()
    mask, _ = G.extend_mask(*case)
    for program, tile in MG.mx_extend_programs(*case):
        _, k_q, k_s, v_q, v_s = MG.mx_extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile, mask, seed=len0 + Tn)
        g = AP.offsets(n + 5, program, tile).double()
        _check_offsets(K.dequant(k_q, k_s), k_s, mask, g, n, program, tile)
        used |= set(g.tolist())
    assert used <= set(CARRIED) | {-8.0, -16.0, -24.0, -32.0}, used


# ---- the programs reach what they are named for -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,Dh,H,Hkv,n", MX_DECODE16 + [(F32, Dh, H, Hkv, n) for Dh, H, Hkv in MG.MX_SHAPES[:1] for n in MG.MX_LENS])
def test_programs_reach_their_factors_in_the_mxfp4_decode_walk(dt, Dh, H, Hkv, n):
    """The wave slices of a chunk are replayed as steps of one online softmax: a factor `inside a span` is one of the combine in LDS."""
    span, tile = MG.mx_walk(Dh)
    for program, stair_tile, qkv, kd, vd, mask, _ in _decode_runs(dt, Dh, H, Hkv, n):
        _, resc, merge = C._emulate_decode(dt, Dh, H, Hkv, n, (span, tile), qkv, kd, vd, mask)
        want = _expected(program, stair_tile, n, span, tile)
        print(f"{G.NAME[dt]} Dh={Dh} len={n} {MG.label(program, stair_tile)}: smallest rescale e^{math.log(max(resc, 1e-300)):.1f}, merge e^{math.log(max(merge, 1e-300)):.1f}")
        assert all(w is None or w == f for w, f in zip(want, (resc <= E8, merge <= E8))), (program, stair_tile, resc, merge, want)


@pytest.mark.parametrize("case", MG.MX_EXTEND_CASES, ids=G._case_id)
def test_programs_reach_their_factors_in_the_mxfp4_extend_walk(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    for program, stair_tile, q, kd, vd, mask, counts, _ in _extend_runs(case):
        _, resc, merge = _emulate_extend(case, q, kd, vd, counts)
        want = _expected(program, stair_tile, len0 + Tn, MG.XC, MG.XC)
        print(f"{G._case_id(case)} {MG.label(program, stair_tile)}: smallest rescale e^{math.log(max(resc, 1e-300)):.1f}, merge e^{math.log(max(merge, 1e-300)):.1f}")
        assert all(w is None or w == f for w, f in zip(want, (resc <= E8, merge <= E8))), (program, stair_tile, resc, merge, want)


# ---- the bound is attainable ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,Dh,H,Hkv,n", MX_DECODE16)
def test_the_mxfp4_decode_bound_is_attainable_by_the_walk(dt, Dh, H, Hkv, n):
    worst = (0.0, 0.0)
    for program, tile, qkv, kd, vd, mask, ref in _decode_runs(dt, Dh, H, Hkv, n):
        out, _, _ = C._emulate_decode(dt, Dh, H, Hkv, n, MG.mx_walk(Dh), qkv, kd, vd, mask)
        assert torch.isfinite(out.float()).all(), (program, tile)
        glob, rows = AP.errors(out.reshape(-1, Dh), ref.reshape(-1, Dh))
        worst = (max(worst[0], glob), max(worst[1], rows))
    print(f"worst mxfp4 decode {G.NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len={n}: global {worst[0]:.2e} per-row {worst[1]:.2e}")
    assert max(worst) < HEADROOM[dt] < X._tol(dt, Dh), worst


@pytest.mark.parametrize("case", MX_EXTEND16, ids=G._case_id)
def test_the_mxfp4_extend_bound_is_attainable_by_the_walk(case):
    dt, Dh = case[0], case[1]
    worst = (0.0, 0.0)
    for program, tile, q, kd, vd, mask, counts, ref in _extend_runs(case):
        out, _, _ = _emulate_extend(case, q, kd, vd, counts)
        assert torch.isfinite(out.float()).all(), (program, tile)
        glob, rows = AP.errors(out.reshape(-1, Dh), ref.reshape(-1, Dh))
        worst = (max(worst[0], glob), max(worst[1], rows))
    print(f"worst mxfp4 extend {G._case_id(case)}: global {worst[0]:.2e} per-row {worst[1]:.2e}")
    assert max(worst) < HEADROOM[dt] < X._tol(dt, Dh), worst


# ---- two planted errors ------------------------------------------------------------------------------------------------------------------------------------
def _fault_case(runs, emulate, reachable, Dh, what):
    """`runs`: (program, stair tile, emulator arguments, reference); emulate(*arguments, fault) -> (out, ..)."""
    worst, which = 0.0, None
    for program, stair_tile, args, ref in runs:
        out = emulate(*args, fault=what[0])[0]
        if not reachable:
            assert torch.equal(out, emulate(*args)[0]), (program, stair_tile)
            continue
        rows = AP.errors(out.float().nan_to_num(1e30).reshape(-1, Dh), ref.reshape(-1, Dh))[1]
        if rows > worst:
            worst, which = rows, MG.label(program, stair_tile)
    if reachable:
        print(f"{what[0]} {what[1]}: worst per-row {worst:.2e} under {which}")
        assert worst > 1e-2, (worst, which)


@pytest.mark.parametrize("fault", AP.FAULTS)
@pytest.mark.parametrize("dt,Dh,H,Hkv,n", MX_DECODE16)
def test_a_planted_error_in_the_mxfp4_decode_walk_is_over_the_bar(dt, Dh, H, Hkv, n, fault):
    span, tile = MG.mx_walk(Dh)
    reachable = tile < span if fault == "no_rescale" else n > span
    runs = ((p, t, (qkv, kd, vd, mask), ref) for p, t, qkv, kd, vd, mask, ref in _decode_runs(dt, Dh, H, Hkv, n))
    emulate = lambda qkv, kd, vd, mask, fault=None: C._emulate_decode(dt, Dh, H, Hkv, n, (span, tile), qkv, kd, vd, mask, fault)
    _fault_case(runs, emulate, reachable, Dh, (fault, f"mxfp4 decode {G.NAME[dt]} Dh={Dh} len={n}"))


@pytest.mark.parametrize("fault", AP.FAULTS)
@pytest.mark.parametrize("case", MX_EXTEND16, ids=G._case_id)
def test_a_planted_error_in_the_mxfp4_extend_walk_is_over_the_bar(case, fault):
    dt, Dh, H, Hkv, Tn, len0 = case
    reachable = fault == "log2_max" and len0 + Tn > MG.XC              # one softmax per chunk: no rescale inside a partial to lose
    runs = ((p, t, (q, kd, vd, counts), ref) for p, t, q, kd, vd, mask, counts, ref in _extend_runs(case))
    emulate = lambda q, kd, vd, counts, fault=None: _emulate_extend(case, q, kd, vd, counts, fault)
    _fault_case(runs, emulate, reachable, Dh, (fault, f"mxfp4 extend {G._case_id(case)}"))


# ---- paged: the construction of the GPU module ----------------------------------------------------------------------------------------------------------
def _check_paged(pb, program):
    B = len(pb.ends)
    named_ever = set()
    hot = int(program[4:]) if program.startswith("hot@") else -1
    cases = PG.table_cases(pb.P, pb.new0)
    assert cases[0] == "whole" and {"lead", "last", "none"} <= set(cases)
    for case in cases:
        t, masks = pb.table(case)
        assert t.shape == (B, max(pb.P) + 1) and t.dtype == torch.int32
        for b, (e, m) in enumerate(zip(pb.ends, masks)):
            slots = torch.arange(pb.P[b] * PG.PAGE)
            ids = t[b].long()[slots // PG.PAGE]
            named = (ids >= 0) & (ids < pb.num_pages)
            assert torch.equal((slots < e) & named, m.bool()), (case, b)              # the table and the mask describe the same counted set
            assert bool((t[b, pb.P[b]:] == -1).all())
            if case != "none" and e > 0:
                assert bool(m.any()), (case, b)                        # a sequence meant to keep keys keeps one
            if case == "none" or e == 0:
                assert not bool(m.any())
            counted = slots[m.bool()]
            pages = torch.tensor(pb.pages[b], dtype=torch.long)[counted // PG.PAGE]
            assert torch.equal(ids[counted], pages)
            assert bool(torch.isfinite(pb.kp[pages, :, counted % PG.PAGE].float()).all()) and bool(torch.isfinite(pb.vp[pages, :, counted % PG.PAGE].float()).all())
            named_ever |= set(ids[named].tolist())
            k, v = pb.dense[b]
            assert bool(v[:, e:].isnan().all())                        # every slot at or above the end: NaN V ...
            past = torch.arange(k.shape[1]) >= e
            if e <= hot < k.shape[1]:
                assert float(k[0, hot, 0]) == 16.0 and bool(torch.isfinite(k[:, hot].float()).all())      # ... under the one finite hot K row
                past[hot] = False
            assert bool(k[:, past].isnan().all())
    assert named_ever.isdisjoint(pb.spare) and len(pb.spare) == PG.SPARE
    for page in pb.spare:                                              # a finished sequence's data: hot keys over NaN values
        assert bool((pb.kp[page][..., 0] == 16.0).all()) and bool(torch.isfinite(pb.kp[page].float()).all()) and bool(pb.vp[page].isnan().all())


@pytest.mark.parametrize("case", [c for c in PG.DECODE_CASES if c[0] != HF], ids=PG._decode_id)
def test_paged_decode_tables_masks_and_poison_agree(case):
    dt, Dh, H, Hkv, n = case
    programs = PG.decode_programs(n)
    assert f"hot@{n}" in [p for p, _ in programs] and n % PG.PAGE != 0
    lens = PG.decode_lens(n)
    assert 0 in lens and len(set(lens)) >= 4 and 4 <= len(lens) <= 6   # ragged, one empty
    for program, tile in programs:
        pb = PG.decode_problem(dt, Dh, H, Hkv, n, program, tile)
        assert pb.ends == lens
        _check_paged(pb, program)
    if n == 1000:
        assert PG.table_cases(pb.P, pb.new0) == list(PG.TABLES)
        assert PG.missing_pages("lead", 8, 7) == {0, 1} and PG.missing_pages("middle", 8, 7) == {4} and PG.missing_pages("last", 8, 7) == {7}


@pytest.mark.parametrize("case", [c for c in PG.EXTEND_CASES if c[0] != HF], ids=G._case_id)
def test_paged_extend_tables_masks_and_poison_agree(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    l0 = PG.extend_len0s(len0)
    assert -1 in l0 and len(set(l0)) == 4
    for program, tile in G.extend_programs(*case):
        pb = PG.extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile)
        assert pb.ends == [l + Tn if l >= 0 else 0 for l in l0]
        _check_paged(pb, program)
        _, masks = pb.table("last")                                    # the pages under the new rows: no new slot counts, every sequence keeps an old page
        for b, l in enumerate(l0):
            if l >= 0:
                assert not bool(masks[b][l:].any()) and bool(masks[b][:l].any())
    assert list(PG.TABLES) == PG.table_cases(pb.P, pb.new0) or max(pb.P) < 3
