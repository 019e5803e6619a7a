"""The score programs do to the chunked attention kernels what tests/test_cache_attn_programs_gpu.py needs of them — checked on the CPU with
`attn_programs.emulate_chunked`, a per-row replay of the extend / decode walk with the kernels' roundings — and the bounds asserted on the GPU
are attainable by that walk's arithmetic in both 16-bit element types.

What the earlier tests reach: over the unit-variance inputs of test_extend_gpu._extend_problem (its PAIRS and SPAN_PAIRS; bf16 and fp16; head dim 128
at H, Hkv = 8, 1 and head dim 64 at 4, 2) the smallest factor by which a rescale inside a span multiplies a row that had counted a key is e^-3.6, and
the smallest factor the merge applies to a partial that had is e^-6.5.  Under the programs both reach e^-8 and e^-16 wherever the program says so, and the merge factor
underflows to 0 under the descending stairs (test_programs_reach_...).  A lost factor of e^-3.6 is a gross error, which those tests see; what they never
reach is a factor small enough that the wrong one is the whole answer, a merge factor of 0 next to (-inf, 0, zeros) partials, or a hot key that the
rows of one wave, the two sides of a chunk edge or a dead slot disagree about.

The planted errors (flags of the emulator, never of a kernel): a shape shows "accumulators not rescaled" only if its walk takes more than one
online-softmax step per partial, and "the partial's maximum left in log2 units" only if a row has more than one partial.  Where a shape's walk has
the step, the error must exceed 1e-2 per row under some program; where it has not — the generic kernel runs one softmax per chunk, and the four-wave
kernel at 265 slots writes one partial — the flag must change no bit, which is asserted instead.  Each figure is printed beside the one the same
error reaches on the unit-variance inputs of the earlier tests: 2.2 and 4.6e-2 per row at the least in the extend walk, but in the decode walk at
257 slots the log2 maximum moves a row by only 1.5e-3 to 7.5e-3 at head dims 32 to 128 — under the bar — where the programs put it at 2.8e-2 to 5.0e-2."""
import math

import pytest
import torch

import attn_programs as AP
import test_cache_attn_programs_gpu as G
import test_extend_gpu as X
from test_fp8kv_gpu import _dequant

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
LOW = [BF, HF]
E8 = math.exp(-8.0)
HEADROOM = {BF: 7e-3, HF: 1e-3}                    # tests/test_attn_programs_cpu.py's: the rounding of P and of the output, 2^-9 each in bf16, 2^-12 in fp16
EXTEND16 = [c for c in G.EXTEND_CASES if c[0] != F32]
DECODE16 = [(dt, Dh, H, Hkv, n) for dt in LOW for Dh, H, Hkv in G.FP8_SHAPES for n in G.FP8_LENS]


# ---- the emulator over the problems of the GPU module ------------------------------------------------------------------------------------------------
def _emulate_extend(case, q, k, v, counts, fault=None):
    """emulate_chunked over an extend problem in the kernel's stacking (row m = i * G + g of a key / value head) -> ((4 * Tn, H * Dh), factors)."""
    dt, Dh, H, Hkv, Tn, len0 = case
    B, n, Gq = 4, len0 + Tn, H // Hkv
    span, tile = G.extend_walk(dt, Dh, H, Hkv, Tn)
    qq = q[:, :H * Dh].reshape(B, Tn, Hkv, Gq, Dh).permute(0, 2, 1, 3, 4).reshape(B, Hkv, Tn * Gq, Dh)
    cc = counts[:, None, :, None, :].expand(B, Hkv, Tn, Gq, n).reshape(B, Hkv, Tn * Gq, n)
    out, resc, merge = AP.emulate_chunked(qq, k[:, :, :n], v[:, :, :n], cc, Dh ** -0.5, dt, span, tile, fault)
    return out.reshape(B, Hkv, Tn, Gq, Dh).permute(0, 2, 1, 3, 4).reshape(B * Tn, H * Dh), resc, merge


def _emulate_decode(dt, Dh, H, Hkv, n, walk, qkv, kd, vd, mask, fault=None):
    B, Gq = 4, H // Hkv
    span, tile = walk
    qq = qkv[:, :H * Dh].reshape(B, Hkv, Gq, Dh)
    cc = mask[:, None, None, :n].bool().expand(B, Hkv, Gq, n)
    out, resc, merge = AP.emulate_chunked(qq, kd[:, :, :n], vd[:, :, :n], cc, Dh ** -0.5, dt, span, tile, fault)
    return out.reshape(B, H * Dh), resc, merge


def _extend_runs(case):
    """Every program of an extend case: (program, stair tile, q, k, v, mask, counts, fp64 reference)."""
    dt, Dh, H, Hkv, Tn, len0 = case
    mask, counts = G.extend_mask(*case)
    for program, tile in G.extend_programs(*case):
        q, k, v = G.extend_problem(dt, Dh, H, Hkv, Tn, len0, program, tile, mask, seed=len0 + Tn)
        yield program, tile, q, k, v, mask, counts, X._extend_ref(q, k, v, mask, H, Hkv, Dh, len0, Tn)


def _decode_runs(dt, Dh, H, Hkv, n):
    for program, tile in G.fp8_programs(n):
        qkv, k_q, k_e, v_q, v_e, mask, _ = G.fp8_problem(dt, Dh, H, Hkv, n, program, tile, seed=600 + n)
        kd, vd = _dequant(k_q, k_e), _dequant(v_q, v_e)
        yield program, tile, qkv, kd, vd, mask, G._decode_ref(qkv, kd, vd, mask, H, Hkv, Dh, n)


def _expected(program, stair_tile, n, span, tile):
    """(a rescale factor <= e^-8 inside a span, a merge factor <= e^-8) as the geometry of the walk says: in the sequence whose keys all count, the row
    that counts every slot.  A stair of 8 nats climbs inside a span iff a step of it lies inside one; a stair of whole spans separates the partials
    (a finer stair makes no claim about the merge: the last partial may hold a single key, whose quarter nat of noise decides the side of e^-8);
    a descending stair and a level shift never raise a maximum; a hot key raises the maximum of its span iff an earlier tile of the span holds a
    key, and outweighs the other partials iff there are any; a hot key in slot n heats nothing."""
    spans = (n + span - 1) // span
    if program in ("stair8", "down8"):
        return program == "stair8" and tile <= stair_tile < span and n > stair_tile, (n > stair_tile) if stair_tile >= span else None
    if program == "shift-60":
        return False, False
    p = AP.hot_key(program, n)
    return p < n and p % span >= tile, p < n and spans > 1


# ---- the programs reach what they are named for -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.EXTEND_CASES, ids=G._case_id)
def test_programs_reach_the_factors_they_are_named_for_in_the_extend_walk(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    span, tile = G.extend_walk(dt, Dh, H, Hkv, Tn)
    for program, stair_tile, q, k, v, mask, counts, _ in _extend_runs(case):
        _, resc, merge = _emulate_extend(case, q, k, v, counts)
        want = _expected(program, stair_tile, len0 + Tn, span, tile)
        print(f"{G._case_id(case)} {G._label(program, stair_tile)}: smallest rescale e^{math.log(max(resc, 1e-300)):.1f}, smallest merge factor e^{math.log(max(merge, 1e-300)):.1f}")
        assert all(w is None or w == f for w, f in zip(want, (resc <= E8, merge <= E8))), (program, stair_tile, resc, merge, want)


@pytest.mark.parametrize("dt,Dh,H,Hkv,n", DECODE16 + [(F32, Dh, H, Hkv, n) for Dh, H, Hkv in G.FP8_SHAPES[:1] for n in G.FP8_LENS])
def test_programs_reach_the_factors_they_are_named_for_in_the_fp8_decode_walk(dt, Dh, H, Hkv, n):
    """The wave slices of a chunk are replayed as steps of one online softmax: a factor `inside a span` is one of the combine in LDS."""
    span, tile = G.fp8_walk(Dh)
    for program, stair_tile, qkv, kd, vd, mask, _ in _decode_runs(dt, Dh, H, Hkv, n):
        _, resc, merge = _emulate_decode(dt, Dh, H, Hkv, n, (span, tile), qkv, kd, vd, mask)
        want = _expected(program, stair_tile, n, span, tile)
        assert all(w is None or w == f for w, f in zip(want, (resc <= E8, merge <= E8))), (program, stair_tile, resc, merge, want)


# ---- what the unit-variance tests reach --------------------------------------------------------------------------------------------------------------
def test_unit_variance_inputs_stay_far_above_the_factors_of_the_programs():
    """test_extend_gpu's inputs on its PAIRS and SPAN_PAIRS: no rescale inside a span and no merge factor reaches e^-8.  The gap this module closes;
    the figures of the module docstring."""
    worst = [1.0, 1.0]
    for dt in LOW:
        for Dh, H, Hkv in ((128, 8, 1), (64, 4, 2)):
            for len0, Tn in X.PAIRS + X.SPAN_PAIRS:
                case = (dt, Dh, H, Hkv, Tn, len0)
                q, k, v, mask = X._extend_problem(dt, H, Hkv, Dh, len0, Tn, len0 + Tn + 5, seed=100 + len0 + Tn)
                n = len0 + Tn
                counts = mask[:, None, :n].bool() & (torch.arange(n)[None, :] <= len0 + torch.arange(Tn)[:, None])[None]
                _, resc, merge = _emulate_extend(case, q, k, v, counts)
                worst = [min(worst[0], resc), min(worst[1], merge)]
    print(f"unit variance: smallest rescale inside a span e^{math.log(worst[0]):.2f}, smallest merge factor e^{math.log(worst[1]):.2f}")
    assert worst[0] > E8 and worst[1] > E8, worst


# ---- the offsets survive rounding and quantisation ------------------------------------------------------------------------------------------------------
def test_offsets_survive_rounding_to_16_bits():
    for case in G.EXTEND_CASES:
        n = case[5] + case[4]
        for program, tile in G.extend_programs(*case):
            g = AP.offsets(n + 5, program, tile)
            assert float(g.abs().max()) <= 272.0
            for dt in LOW:
                assert torch.equal(g.to(dt).float(), g), (program, tile, dt)


@pytest.mark.parametrize("Dh,H,Hkv", G.FP8_SHAPES)
@pytest.mark.parametrize("n", G.FP8_LENS)
def test_offsets_survive_the_fp8_quantiser(Dh, H, Hkv, n):
    """K'[:, 0] of every live slot (and of a heated dead one) is the program's offset bit for bit, so the stairs are carried by the codes AND by the
    rows' exponent bytes, which differ between the stair's levels."""
    used = set()
    for program, tile in G.fp8_programs(n):
        _, k_q, k_e, _, _, mask, kf = G.fp8_problem(F32, Dh, H, Hkv, n, program, tile, seed=600 + n)
        kd = _dequant(k_q, k_e)
        g = AP.offsets(n + 5, program, tile).double()
        live = ~kd[..., 0].isnan()
        assert torch.equal(kd[..., 0][live], g[None, None].expand_as(kd[..., 0])[live]), (program, tile)
        assert bool(live[0, :, :n].all()), (program, tile)             # the whole sequence: every slot below n is checked
        used |= set(g.tolist())
        if program == "stair8":
            lv = [k_e[0, 0, j * tile:min(n, (j + 1) * tile)].float().mean() for j in range((n + tile - 1) // tile)]
            assert lv[-1] > lv[0] + 1, lv                              # the exponent byte climbs with the stair
    assert used <= {0.0, 16.0} | {8.0 * i for i in range(-4, 5)}, used


# ---- the bound is attainable ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXTEND16, ids=G._case_id)
def test_the_extend_bound_is_attainable_by_the_walk(case):
    dt, Dh = case[0], case[1]
    worst = (0.0, 0.0)
    for program, tile, q, k, v, mask, counts, ref in _extend_runs(case):
        out, _, _ = _emulate_extend(case, q, k, v, counts)
        assert torch.isfinite(out.float()).all(), (program, tile)
        glob, rows = AP.errors(out.reshape(-1, Dh), ref.reshape(-1, Dh))
        print(f"emulate {G._case_id(case)} {G._label(program, tile)}: global {glob:.2e} per-row {rows:.2e}")
        worst = (max(worst[0], glob), max(worst[1], rows))
    print(f"worst {G._case_id(case)}: global {worst[0]:.2e} per-row {worst[1]:.2e}")
    assert max(worst) < HEADROOM[dt] < X._tol(dt, Dh), worst


@pytest.mark.parametrize("dt,Dh,H,Hkv,n", DECODE16)
def test_the_decode_bound_is_attainable_by_the_walk(dt, Dh, H, Hkv, n):
    """Both decode kernels over K', V': the fp8 walk (256-slot chunks, 64-key slices) and the native one (128, 32)."""
    worst = (0.0, 0.0)
    for program, tile, qkv, kd, vd, mask, ref in _decode_runs(dt, Dh, H, Hkv, n):
        for walk in (G.fp8_walk(Dh), G.native_walk(dt, Dh)):
            out, _, _ = _emulate_decode(dt, Dh, H, Hkv, n, walk, qkv, kd, vd, mask)
            assert torch.isfinite(out.float()).all(), (program, tile, walk)
            glob, rows = AP.errors(out.reshape(-1, Dh), ref.reshape(-1, Dh))
            print(f"emulate decode {G.NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len={n} walk={walk} {G._label(program, tile)}: global {glob:.2e} per-row {rows:.2e}")
            worst = (max(worst[0], glob), max(worst[1], rows))
    print(f"worst decode {G.NAME[dt]} Dh={Dh} H={H} Hkv={Hkv} len={n}: global {worst[0]:.2e} per-row {worst[1]:.2e}")
    assert max(worst) < HEADROOM[dt] < X._tol(dt, Dh), worst


# ---- two planted errors ------------------------------------------------------------------------------------------------------------------------------------
def _unit_variance(case):
    dt, Dh, H, Hkv, Tn, len0 = case
    mask, counts = G.extend_mask(*case)
    q, k, v, mask = X._extend_problem(dt, H, Hkv, Dh, len0, Tn, len0 + Tn + 5, seed=100 + len0 + Tn)
    return q, k, v, counts, X._extend_ref(q, k, v, mask, H, Hkv, Dh, len0, Tn)


@pytest.mark.parametrize("fault", AP.FAULTS)
@pytest.mark.parametrize("case", EXTEND16, ids=G._case_id)
def test_a_planted_error_in_the_extend_walk_is_over_the_bar(case, fault):
    dt, Dh, H, Hkv, Tn, len0 = case
    span, tile = G.extend_walk(dt, Dh, H, Hkv, Tn)
    reachable = tile < span if fault == "no_rescale" else len0 + Tn > span
    worst, which = 0.0, None
    for program, stair_tile, q, k, v, mask, counts, ref in _extend_runs(case):
        out = _emulate_extend(case, q, k, v, counts, fault)[0]
        if not reachable:
            assert torch.equal(out, _emulate_extend(case, q, k, v, counts)[0]), (program, stair_tile)
            continue
        rows = AP.errors(out.float().nan_to_num(1e30).reshape(-1, Dh), ref.reshape(-1, Dh))[1]
        if rows > worst:
            worst, which = rows, G._label(program, stair_tile)
    if not reachable:
        return
    q, k, v, counts, ref = _unit_variance(case)
    unit = AP.errors(_emulate_extend(case, q, k, v, counts, fault)[0].float().nan_to_num(1e30).reshape(-1, Dh), ref.reshape(-1, Dh))[1]
    print(f"{fault} {G._case_id(case)}: worst per-row {worst:.2e} under {which}; on the unit-variance inputs {unit:.2e}")
    assert worst > 1e-2, (worst, which)


@pytest.mark.parametrize("fault", AP.FAULTS)
@pytest.mark.parametrize("dt,Dh,H,Hkv,n", DECODE16)
def test_a_planted_error_in_the_fp8_decode_walk_is_over_the_bar(dt, Dh, H, Hkv, n, fault):
    span, tile = G.fp8_walk(Dh)
    reachable = tile < span if fault == "no_rescale" else n > span
    worst, which = 0.0, None
    for program, stair_tile, qkv, kd, vd, mask, ref in _decode_runs(dt, Dh, H, Hkv, n):
        out = _emulate_decode(dt, Dh, H, Hkv, n, (span, tile), qkv, kd, vd, mask, fault)[0]
        if not reachable:
            assert torch.equal(out, _emulate_decode(dt, Dh, H, Hkv, n, (span, tile), qkv, kd, vd, mask)[0]), (program, stair_tile)
            continue
        rows = AP.errors(out.float().nan_to_num(1e30).reshape(-1, Dh), ref.reshape(-1, Dh))[1]
        if rows > worst:
            worst, which = rows, G._label(program, stair_tile)
    if reachable:
        qkv, k_q, k_e, v_q, v_e, mask = G._fp8_problem(dt, H, Hkv, Dh, n, n + 5, 600 + n)      # test_fp8kv_gpu's own unit-variance inputs
        kd, vd = _dequant(k_q, k_e), _dequant(v_q, v_e)
        out = _emulate_decode(dt, Dh, H, Hkv, n, (span, tile), qkv, kd, vd, mask, fault)[0]
        unit = AP.errors(out.float().nan_to_num(1e30).reshape(-1, Dh), G._decode_ref(qkv, kd, vd, mask, H, Hkv, Dh, n).reshape(-1, Dh))[1]
        print(f"{fault} decode {G.NAME[dt]} Dh={Dh} len={n}: worst per-row {worst:.2e} under {which}; on the unit-variance inputs {unit:.2e}")
        assert worst > 1e-2, (worst, which)
