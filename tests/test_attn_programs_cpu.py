"""The score programs of tests/attn_programs.py do what tests/test_attn_programs_gpu.py needs of them — checked on the CPU by an fp32 replay of
attn_vit_kernel's tile walk — and the bound asserted on the GPU is attainable by that walk's arithmetic in both 16-bit element types."""
import pytest
import torch

import attn_programs as AP

SHAPES = [(65, 64), (200, 64), (201, 64), (257, 64), (577, 64), (65, 48), (289, 48)]          # the dense cases of the GPU suite
DTYPES = [torch.bfloat16, torch.float16]
BOUND = 1e-2                                                                                   # the project's 16-bit attention bar


def _rounded(T, Dh, program, dt, seed=1):
    return tuple(t.to(dt) for t in AP.build(T, Dh, program, seed))


def _short_tail(T):
    return 1 <= T % 32 <= AP.SHORT_TAIL


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("T,Dh", SHAPES)
def test_programs_reach_the_branches_they_are_named_for(T, Dh, dt):
    nq = (T + 31) // 32
    for program in AP.PROGRAMS:
        q, k, _ = _rounded(T, Dh, program, dt)
        tiles = AP.walk_qtiles(q, k, Dh ** -0.5)
        total = AP.walk(q, k, Dh ** -0.5)
        assert len(tiles) == nq and total.late == sum(w.late for w in tiles)
        what = (program, T, Dh, total)
        # onerow8 steers the rows i % 32 == 5 only: a last query tile that ends before its row 5 (the class-token tile: one row) has no steered row
        steered = [w for t, w in enumerate(tiles) if program != "onerow8" or t * 32 + 5 < T]
        assert len(steered) >= nq - 1
        if program in ("stair4", "stair5.5", "stair8", "onerow8", "hot@32", "hot@T-1"):
            assert all(w.late >= 1 for w in steered), what                   # every wave rescales after its first key tile
        if program in ("hot@T-1", "stair8", "onerow8") and _short_tail(T):
            assert all(w.short_tail >= 1 for w in steered), what             # ... and in the short form of the last tile
        if not _short_tail(T):
            assert total.short_tail == 0, what                               # T = 201: 9 tail keys take the general form
        if program in ("down8", "shift-60", "hot@0", "hot@31"):
            assert total.late == 0, what
        if program == "stair5.5" and T == 257:
            assert total.log2_pmax >= 7.5, what                              # the deferred ceiling of 2^8 is approached
        if program == "stair8":
            assert total.late == nq * ((T + 31) // 32 - 1), what             # at every tile
        assert total.log2_pmax <= 8.0 + 1e-3, what                           # what the comment at DEFER_MAX promises


def test_unit_variance_inputs_never_rescale_late():
    """The inputs of tests/test_ops_gpu.py::test_attention_uniform (unit randn, seed 8), every bf16 case that routes to attn_vit_kernel (head dim 64 /
    48): no (query tile, key tile) unit of the walk raises the maximum after the first key tile, and the closest any comes is well under the
    threshold.  The gap this module closes."""
    import test_ops_gpu
    shapes = next(m.args[1] for m in test_ops_gpu.test_attention_uniform.pytestmark if m.name == "parametrize" and m.args[0] == "T,H,Dh,nimg")
    units = late = 0
    for T, H, Dh, nimg in shapes:
        if Dh not in (64, 48):
            continue
        qkv = test_ops_gpu._rand(nimg * T, 3 * H * Dh, seed=8).bfloat16().reshape(nimg, T, 3, H, Dh)
        for b in range(nimg):
            for h in range(H):
                w = AP.walk_qtiles(qkv[b, :, 0, h], qkv[b, :, 1, h], Dh ** -0.5)
                units += len(w) * ((T + 31) // 32)
                late += sum(x.late for x in w)
    assert units == 19068, units                   # every (query tile, key tile) unit those cases run
    assert late == 0, late


def test_offsets_survive_rounding():
    for dt in DTYPES:
        for program in AP.PROGRAMS:
            g = AP.offsets(577, program)
            assert torch.equal(g.to(dt).float(), g), (program, dt)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("T,Dh", SHAPES)
def test_the_bound_is_attainable_by_the_walk(T, Dh, dt):
    worst = (0.0, 0.0)
    for program in AP.PROGRAMS:
        q, k, v = _rounded(T, Dh, program, dt)
        ref = AP.reference(q, k, v, Dh ** -0.5)
        out = AP.emulate(q, k, v, Dh ** -0.5, dt)
        assert torch.isfinite(out.float()).all(), program
        glob, rows = AP.errors(out, ref)
        print(f"emulate {dt} T={T} Dh={Dh} {program}: global {glob:.2e} per-row {rows:.2e}")
        assert glob < BOUND and rows < BOUND, (program, glob, rows)
        worst = (max(worst[0], glob), max(worst[1], rows))
    print(f"worst T={T} Dh={Dh} {dt}: global {worst[0]:.2e} per-row {worst[1]:.2e}")
    # the headroom docs/PERF_NOTES.md (section H) quotes: the rounding of P and of the output to the element type, 2^-9 each in bf16, 2^-12 in fp16
    assert max(worst) < (7e-3 if dt == torch.bfloat16 else 1e-3), worst
