"""tests/gemm_programs.py without a GPU: the programs meet their preconditions at every shape test_gemm_programs_gpu.py uses, an fp32 GEMM gives the
fp64 reference's bits in any summation order, and each slip a GEMM kernel can make is caught by at least one program at the smallest shape the GPU
test uses for the class the slip belongs to.  The `act` verdict's floor is measured here (torch's fp32 evaluation on the CPU against fp64) and logged."""
import os

import pytest
import torch

import gemm_programs as P
from gemm_dispatch import _kernel_class, source_constant

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LOW16 = [BF16, F16]
NCU = 256                                           # the CU count the case tables are written for
TK, BK, FK = source_constant("gemm_persist.hip", "TK"), source_constant("gemm.hip", "BK"), source_constant("gemm.hip", "FK")
KSLICE = 512                                        # SETOK_SKINNY_KSLICE's default (the GPU test reads the library's)
_LOG = os.environ.get("SETOK_PARITY_LOG")


def _log(text):
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0] + "\t" + text + "\n")


def test_k_tiles_are_what_the_sources_say():
    assert (TK, BK, FK) == (64, 64, 16)


# ---------------------------------------------------------------------------------------------
# preconditions
# ---------------------------------------------------------------------------------------------
def _linear_shapes():
    """(M, N, K, K-tile) of every setok_linear / swiglu / f32b case of the GPU file, on 256 CUs."""
    out = []
    for M, N in P.F32_SHAPES:
        out += [(M, N, kt * FK, FK) for kt in P.F32_K_TILES]
    for M, N in P.TILE128_SHAPES:
        out += [(M, N, kt * BK, BK) for kt in P.TILE128_K_TILES]
    for M, cls in P.SMALL_ROWS:
        out += [(M, P.SMALL_N, kt * TK, TK) for kt in P.STAGE_K_TILES[int(cls.rsplit("/", 1)[1])]]
    for (M, N), _ in P.PERSIST_SHAPES:
        out += [(M, N, kt * TK, TK) for kt in P.PERSIST_K_TILES]
    out += [((NCU // 8 + 1) * 256, P.PEELED_N, kt * TK, TK) for kt in P.PERSIST_K_TILES]
    out += [(P.loop_rows(NCU, N), N, 3 * TK, TK) for N, _ in P.LOOP_SHAPES]
    for M, N in P.F32B_SHAPES:
        out += [(M, N, kt * TK, TK) for kt in P.PERSIST_K_TILES]
    return out


def test_case_tables_reach_their_classes_on_256_cus():
    for M, cls in P.SMALL_ROWS:
        for kt in P.STAGE_K_TILES[int(cls.rsplit("/", 1)[1])]:
            assert _kernel_class(M, P.SMALL_N, kt * TK, P.SMALL_N, NCU) == cls, (M, kt)
    for (M, N), cls in P.PERSIST_SHAPES:
        for kt in P.PERSIST_K_TILES:
            assert _kernel_class(M, N, kt * TK, N, NCU) == cls
    assert _kernel_class((NCU // 8 + 1) * 256, P.PEELED_N, 192, P.PEELED_N, NCU) == "persist+tail"
    for N, cls in P.LOOP_SHAPES:
        M = P.loop_rows(NCU, N)
        assert _kernel_class(M, N, 192, N, NCU) == cls and (M // 256) * ((N + 255) // 256) >= 3 * NCU
    for M, N in P.F32B_SHAPES:
        assert _kernel_class(M, N, 192, N, NCU, out16=False, batch=24, plain=True) == "f32b"
    for M, N in P.TILE128_SHAPES:
        assert _kernel_class(M, N, 128, N + 4, NCU) == "tile128" and _kernel_class(M, N, 128, N, NCU, out16=False) == "tile128"
        assert _kernel_class(M, N, 320, N, NCU, batch=3) == "tile128" and _kernel_class(M, N, 320, N, NCU, out16=False, batch=3, plain=True) == "tile128"


def test_preconditions_hold_at_every_linear_shape():
    """The bound every program asserts when it is built depends on K and the value ranges, not on M and N: each distinct (K, tile) once at a few rows and
    columns with the programs' own assertions, and the worst case of the values at every shape's K in closed form."""
    for K, tile in sorted({(K, tile) for _, _, K, tile in _linear_shapes()}):
        M, N = 96, 64
        for p in (P.sig(M, N, K), P.onehot(M, N, K), P.cancel(M, N, K, tile=tile)):
            assert p.info["bound"] < P.TWO24
            assert bool((p.a @ p.w.t() == p.acc).all()), (p.name, K)
            assert float((p.a.abs() @ p.w.abs().t()).max()) <= p.info["bound"]            # the cheap bound dominates the sum the issue names
            for dt in LOW16 + [F32]:
                P.assert_representable(p.a, dt, p.name)
                P.assert_representable(p.w, dt, p.name)
        for dt in LOW16 + [F32]:
            for use_bias in (False, True):
                for use_res in (False, True):
                    p = P.round_program(M, N, K, dt, use_bias=use_bias, use_res=use_res)
                    for t in (p.a, p.w):
                        P.assert_representable(t, BF16 if dt == F32 else dt, "round")
                    if use_res:
                        P.assert_representable(p.res, dt, "round residual")
        for use_bias in (False, True):
            p = P.act_program(M, N, K, use_bias=use_bias, use_res=True)
            for dt in LOW16:
                P.assert_representable(p.w, dt, "act")
                P.assert_representable(p.res, dt, "act residual")
    for M, N, K, tile in _linear_shapes():
        assert 49 * K + 2 ** 14 * 2 * len(P.cancel_positions(K, tile)) < 2 ** 23, (M, N, K)           # sig's 49 K and cancel's big terms, as absolute sums
    assert float(P.sig(64, 64, 4096).acc.abs().max()) < 2 ** 17                                          # (seeded integers at K = 4096: far below the bound)


def test_cancel_partials_stay_below_2_22_in_any_order():
    p = P.cancel(64, 64, 1088)
    big = torch.zeros(1088, dtype=torch.bool)
    big[[k for pr in p.info["pairs"] for k in pr]] = True
    assert int(big.sum()) <= 256
    assert float(((p.a[:, big].abs()) @ (p.w[:, big].abs()).t()).max()) / 2 <= 2.0 ** 22     # all the +2^14 before any -2^14: the worst partial
    assert bool(((p.a[:, big] @ p.w[:, big].t()) == 0).all())                                  # and they cancel exactly
    for k0, k1 in p.info["pairs"]:
        assert k1 - k0 == 544 or (k1 % 64 == 0 and k0 == k1 - 1)


def test_preconditions_hold_for_swiglu_skinny_and_the_weight_formats():
    M, Fd = P.SWIGLU_SHAPE
    for kt in P.SWIGLU_K_TILES:
        s = P.swiglu_program(M, Fd, kt * TK)
        for dt in LOW16:
            for t in (s.a, s.w_gate, s.w_up):
                P.assert_representable(t, dt, "swiglu")
        gates = set(s.gate.unique().tolist())
        assert set(P.GATE_EXTRA) <= gates and set(P.ACT_GRID.tolist()) <= gates, kt
        assert set(P.UP_SET) <= set(s.up.unique().tolist())
    for K in P.skinny_ks(KSLICE):
        for alpha in P.SKINNY_ALPHA:
            for p in (P.sig(63, 64, K, alpha=alpha), P.cancel(63, 64, K, alpha=alpha), P.round_program(63, 64, K, BF16, alpha=alpha)):
                assert p.info["bound"] < P.TWO24
    for K in P.WSTREAM_K + P.MXFP4_K16:
        wp, e = P.fp8_weights(192, K)
        q = P.fp8_encode(wp, e)
        assert bool((P.fp8_codes_value(q) * (2.0 ** e.double())[:, None] == wp).all())
        assert set(e.tolist()) == set(range(-3, 4))
        codes = P.fp8_codes_value(q)
        assert P.grain(codes) == 1.0 and float(codes.abs().max()) == 15.0
        c = P.cancel(17, 192, K, w=wp, big_w=16.0)
        P.assert_exact(c.a, P.fp8_codes_value(P.fp8_encode(c.w, e)), what="fp8 cancel on the codes")     # what the kernel accumulates: a times the unscaled codes
        P.assert_exact(P.sig(17, 192, K).a, codes, what="fp8 sig")
        for dt in LOW16:
            P.assert_representable(c.a, dt)
            P.assert_representable(c.w, dt)
        wp, s = P.mx_weights(192, K)
        assert bool((s[:, 1:] != s[:, :-1]).all()) and bool((s[1:] != s[:-1]).all()) and set(s.unique().tolist()) == {127, 128, 129, 130}
        assert bool((P.mx_decode(P.mx_encode(wp, s), s) == wp).all())
        assert len(P.mx_encode(wp, s).unique()) > 200                                           # the full e2m1 set, negative zero included, in both nibbles
        c = P.cancel(17, 192, K, w=wp, big_w=4.0)
        P.mx_encode(c.w, s)
        assert P.grain(c.w) == 0.5 and c.info["bound"] < P.TWO24                               # halves: the bound is 2^23 in units of one
        for dt in LOW16:
            P.assert_representable(c.a, dt)
            P.assert_representable(c.w, dt)


# ---------------------------------------------------------------------------------------------
# any order is exact
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", P.ORDERS)
def test_any_order_gives_the_reference_bits(order):
    K = 1088
    for p in (P.sig(33, 48, K), P.cancel(33, 48, K), P.onehot(33, 48, K), P.round_program(33, 48, K, BF16)):
        for tile, kslice in ((64, 512), (1, 64)):                                   # slab by slab, and element by element
            got = P.emulate(p.a, p.w, tile=tile, order=order, kslice=kslice)
            assert torch.equal(got.double(), p.acc), (p.name, order, tile)
    wp, s = P.mx_weights(48, K)
    p = P.cancel(33, 48, K, w=wp, big_w=4.0)                                        # halves
    assert torch.equal(P.emulate(p.a, p.w, order=order).double(), p.acc)


def test_epilogue_emulation_gives_the_expected_bits():
    for dt in LOW16 + [F32]:
        for use_bias in (False, True):
            for use_res in (False, True):
                p = P.round_program(63, 128, 192, dt, use_bias=use_bias, use_res=use_res)
                got = P.epilogue(P.emulate(p.a, p.w), p.bias, p.res, dt)
                assert torch.equal(got, P.expected(p, dt)), (dt, use_bias, use_res)


def test_act_floor_is_the_reference_arithmetic_s_own_error():
    for act, name, measured in ((1, "quick_gelu", 6.3e-7), (2, "gelu_erf", 5.6e-7)):
        floor = P.act_floor(act)
        _log(f"act floor {name}: fp32 torch vs fp64 on the grid j/8, j=-96..96: max abs err {floor / P.DRIFT:.3e}, floor {floor:.3e}")
        assert 0 < floor / P.DRIFT <= 2 * measured and floor < 2e-6, (name, floor)         # the same order as the figures of the day it was written; 10 000 x below 2e-2
        for dt in LOW16 + [F32]:
            for use_res in (False, True):
                p = P.act_program(63, 128, 192, use_bias=True, use_res=use_res)
                ref, bound = P.act_bound(p, act, dt)
                got = P.epilogue(P.emulate(p.a, p.w), p.bias, p.res, dt, act=act).double()
                assert bool(((got - ref).abs() <= bound).all()), (name, dt, use_res)


# ---------------------------------------------------------------------------------------------
# each named slip is caught
# ---------------------------------------------------------------------------------------------
def _caught(p, out_dt=F32, **kw):
    ep = {k: kw.pop(k) for k in ("act",) if k in kw}
    ep_slip = kw.get("slip") if kw.get("slip") in ("res_before_round", "bias_after_act") else None
    if ep_slip:
        kw.pop("slip")
    got = P.epilogue(P.emulate(p.a, p.w, **kw), p.bias, p.res, out_dt, slip=ep_slip, **ep)
    return not torch.equal(got, P.expected(p, out_dt))


# (class the slip belongs to, the smallest shape the GPU file runs there on 256 CUs)
SMALLEST = {
    "fp32": (77, 96, FK, FK),
    "tile128": (300, 96, BK, BK),
    "small": (1, P.SMALL_N, TK, TK),
    "pp": (2560, 2304, 3 * TK, TK),
}


@pytest.mark.parametrize("cls", ["fp32", "tile128", "small", "pp"])
def test_a_dropped_k_tile_and_two_swapped_k_are_caught(cls):
    M, N, K, tile = SMALLEST[cls]
    p = P.sig(M, N, K)
    assert not _caught(p, tile=tile)
    assert _caught(p, tile=tile, slip="drop_last_tile")
    assert _caught(p, tile=tile, slip="swap_k")
    q = P.onehot(max(M, K), N, K)                        # ... and onehot names the k: exactly the rows whose k lies in the dropped tile are wrong
    got = P.emulate(q.a, q.w, tile=tile, slip="drop_last_tile").double()
    wrong = (got != q.acc).any(dim=1)
    assert torch.equal(wrong, (q.info["k_of_row"] >= K - tile) & (q.acc != 0).any(dim=1))


def test_a_carried_accumulator_is_caught():
    for N, _ in P.LOOP_SHAPES:                            # the persistent loop's cases: a tile row is 256 rows
        M = P.loop_rows(NCU, N)
        p = P.onehot(M, N, 3 * TK)
        acc = p.acc.to(torch.float32)
        got = torch.cat([acc[:256], acc[256:] + acc[:-256]])          # (emulate's carry_acc on the exact accumulators: no GEMM of this size on the CPU)
        assert not torch.equal(got.double(), p.acc)
    p = P.sig(2560, 2304, 3 * TK)
    assert _caught(p, slip="carry_acc")


@pytest.mark.parametrize("order", ["forward", "pairwise", "splitk"])
def test_a_16_bit_partial_is_caught(order):
    for M, N, K, tile in (SMALLEST["small"], (1, 16, 2 * KSLICE, TK), (300, 96, 2 * BK, BK)):
        if order == "splitk" and K <= KSLICE:
            K = 2 * KSLICE
        p = P.cancel(M, N, K, tile=tile)
        if K > tile:
            assert _caught(p, tile=tile, order=order, slip="bf16_partial", kslice=KSLICE), (M, N, K, order)
        assert not _caught(p, tile=tile, order=order, kslice=KSLICE)


@pytest.mark.parametrize("dt", LOW16)
def test_a_residual_added_before_rounding_is_caught(dt):
    for M, N, K, tile in SMALLEST.values():
        for use_bias in (False, True):
            p = P.round_program(max(M, 8), N, K, dt, use_bias=use_bias, use_res=True)
            assert p.info["rules_differ"] > 0
            assert _caught(p, out_dt=dt, tile=tile, slip="res_before_round")
            assert not _caught(p, out_dt=dt, tile=tile)


@pytest.mark.parametrize("act", [1, 2])
def test_a_bias_added_after_the_activation_is_caught(act):
    for dt in LOW16 + [F32]:
        p = P.act_program(63, P.SMALL_N, TK, use_bias=True)
        ref, bound = P.act_bound(p, act, dt)
        good = P.epilogue(P.emulate(p.a, p.w), p.bias, None, dt, act=act).double()
        bad = P.epilogue(P.emulate(p.a, p.w), p.bias, None, dt, act=act, slip="bias_after_act").double()
        assert bool(((good - ref).abs() <= bound).all())
        assert not bool(((bad - ref).abs() <= bound).all())


def test_a_row_read_past_the_end_is_caught():
    for M, N, K, tile in ((77, 96, FK, FK), (300, 96, BK, BK), (63, P.SMALL_N, TK, TK), (2600, 2304, 3 * TK, TK)):     # ragged last tile rows
        p = P.sig(M, N, K)
        for past in (torch.zeros(K), torch.full((K,), 3.0)):                       # whatever lies behind A
            assert _caught(p, tile=tile, slip="row_past_end", past_row=past)


def test_the_next_mx_block_s_scale_is_caught():
    for K in (64, 128):                                                            # the smallest K of the fp32 and of the 16-bit MXFP4 GEMM
        wp, s = P.mx_weights(64, K)
        q = P.mx_encode(wp, s)
        shifted = P.mx_decode(q, torch.roll(s, -1, dims=1))                        # block b read with block b + 1's scale
        assert bool((shifted[:, :K - 32] != wp[:, :K - 32])[wp[:, :K - 32] != 0].all())      # no two neighbours share one: every non-zero weight moves
        p = P.sig(1, 64, K, w=wp)
        assert not torch.equal((p.a @ shifted.t()), p.acc)
        below = P.mx_decode(q, torch.roll(s, 1, dims=0))                           # ... and the row below's scales
        assert not torch.equal((p.a @ below.t()), p.acc)


def test_a_skipped_slice_and_a_missing_alpha_are_caught():
    K = KSLICE + 64                                                                # the smallest K with two slices
    for alpha in P.SKINNY_ALPHA:
        p = P.sig(1, 16, K, alpha=alpha)
        want = P.expected(p, F32, alpha=alpha)
        run = lambda slip: P.emulate(p.a, p.w, order="splitk", kslice=KSLICE, alpha=alpha, slip=slip)
        assert torch.equal(run(None), want)
        assert not torch.equal(run("skip_slice"), want)
        if alpha != 1.0:
            assert not torch.equal(run("alpha_missing"), want)
