"""The GEMM entry points of the C ABI (include/setok_hip.h: setok_linear, setok_linear_ln, setok_linear_swiglu) at what `ops.linear` never passes them:
row strides wider than the matrix, operands that are column windows of a wider buffer, batches with strides, a separate output type.  Needs a real
MI355X: `pytest -m gpu`.

1. A stride changes nothing but addresses: the same problem contiguous (lda = K, ldc = N) and embedded in wider buffers gives the same BITS, writes
   nothing outside its window, and reads nothing outside A's window (A's padding is NaN).  One case per kernel class of gemm.hip / gemm_persist.hip;
   each case's comment names the class, `_kernel_class` restates the dispatch rules (bf16_kernel, tail_shape_for, pp_takes, the peel of
   setok_gemm_persist_bf16) and every case asserts that its shape reaches the class on the device it runs on.
2. Value parity against fp64 for the two classes that had none: the fp32-out batched persistent kernel (split-K weight gradients at full dimensions) and
   the batched 128 x 128 kernel with bias, activation and residual; and the batch invariance of the fp32 kernel.

Classes that cannot be reached:
  * the persistent kernel WITHOUT the ping-pong schedule at K < 128 (pp_takes refuses K < 128): the persistent path itself needs K >= 192 (bf16_kernel), so
    a problem with K = 64 or 128 never gets there; at K >= 192 the non-ping-pong kernel is reached through N % 256 != 0 (below);
  * the 64 x 32 shape of tail_shape_for: its rule needs t64 * 2 <= ncu with N % 32 == 0, and then cdiv(M, 32) * (N / 32) <= 4 * t64 <= 2 * ncu — the
    32 x 32 rule above it has already fired."""
import pytest
import torch
import torch.nn.functional as F

import setok_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib, ops

DEV = "cuda"
LOW16 = [torch.bfloat16, torch.float16]
BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
OFF = 8                         # the window starts 8 elements into its buffer: 16 bytes (16-bit) / 32 bytes (fp32), so accesses stay 16-byte aligned
EXTRA_ROWS = 3
SENTINEL = -7.0                 # what C's buffer holds before a run (exact in every element type)


# ---------------------------------------------------------------------------------------------
# raw calls: tensors are only pointers here (a view's data_ptr() is its first element), every number of the ABI is explicit
# ---------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _raw_linear(a, lda, w, c, ldc, M, N, K, bias=None, res=None, act=0, batch=1, sA=0, sW=0, sC=0):
    _lib.call("setok_linear", ops._stream(), ops._code(a.dtype), ops._code(c.dtype), _ptr(a), lda, _ptr(w), _ptr(bias), _ptr(res), _ptr(c), ldc,
              M, N, K, act, batch, sA, sW, sC)


def _raw_linear_ln(a, lda, folded, stats, c, ldc, M, N, K, act):
    _lib.call("setok_linear_ln", ops._stream(), _ptr(a), lda, _ptr(folded[0]), _ptr(folded[3]), _ptr(stats), _ptr(c), ldc, M, N, K, act,
              half=a.dtype == torch.float16)


def _raw_linear_swiglu(a, lda, w_pairs, out, ldo, M, Fd, K):
    _lib.call("setok_linear_swiglu", ops._stream(), ops._code(a.dtype), _ptr(a), lda, _ptr(w_pairs), _ptr(out), ldo, M, Fd, K)


def _randn(*shape, seed, scale=1.0, dt=torch.float32):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(dt)


def _embed(vals, pad, fill):
    """(M, W) values -> an (M + 3, W + pad) buffer of `fill` that holds them as the column window [OFF, OFF + W) of its first M rows."""
    M, W = vals.shape
    buf = torch.full((M + EXTRA_ROWS, W + pad), fill, dtype=vals.dtype, device=vals.device)
    buf[:M, OFF:OFF + W] = vals
    return buf


def _window(buf, M, W):
    return buf[:M, OFF:OFF + W]


def _assert_only_the_window_changed(buf, before, M, W):
    """Everything of `buf` outside rows [0, M) x columns [OFF, OFF + W) has the bits it had in `before`."""
    chk = buf.clone()
    chk[:M, OFF:OFF + W] = before[:M, OFF:OFF + W]
    it = BITS[buf.dtype]
    assert torch.equal(chk.view(it), before.view(it)), "a store outside the C window"


# ---------------------------------------------------------------------------------------------
# the dispatch rules, restated (gemm.hip: bf16_kernel; gemm_persist.hip: tail_shape_for, pp_takes, setok_gemm_persist_bf16): tests/gemm_dispatch.py,
# shared with test_gemm_programs_gpu.py
# ---------------------------------------------------------------------------------------------
from gemm_dispatch import _cdiv, _kernel_class, _ncu, _persist_class, _rows_reaching, _tail_shape  # noqa: E402,F401


# ---------------------------------------------------------------------------------------------
# references and the project's bounds per output type (test_ops_gpu.py: test_linear_f32 / _bf16 / _bf16_large_tiles; test_fp16_gpu.py: test_linear_fp16)
# ---------------------------------------------------------------------------------------------
def _act_ref(ref, act):
    return [ref, O.quick_gelu(ref), F.gelu(ref)][act]


def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def _assert_close(got, ref, in_dt, out_dt, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    rel = _rel(got, ref)
    err = (got - ref).abs()
    if out_dt == torch.float32:
        bound = 2e-6 if in_dt == torch.float32 else 2e-5     # fp32 rounding class / exact 16-bit products, fp32 accumulation
        print(f"{what} rel {rel:.3g} (bound {bound})")
        assert rel < bound, (what, rel)
        return
    bound, ulp, floor = (6e-3, 2.0 ** -7, 2e-2) if out_dt == torch.bfloat16 else (1e-3, 2.0 ** -10, 4e-3)
    print(f"{what} rel {rel:.3g} (bound {bound}), worst element excess {float((err - ulp * ref.abs()).max()):.3g} (bound {floor})")
    assert rel < bound, (what, rel)
    assert bool((err <= ulp * ref.abs() + floor).all()), what


def _ref_rows(M):
    """All rows of a small problem; of one with >= 2560 rows the first, the last and every 256-row tile boundary +- 1."""
    if M < 2560:
        return torch.arange(M)
    rows = {0, M - 1}
    for b in range(256, M, 256):
        rows.update((b - 1, b, b + 1))
    return torch.tensor(sorted(r for r in rows if 0 <= r < M))


def _linear_ref(a, w, b, r, act, out_dt, rows):
    """fp64 F.linear on the CPU over the same rounded inputs; a 16-bit output is rounded BEFORE the residual is added (torch's 16-bit semantics)."""
    idx = rows.to(a.device)
    ref = F.linear(a[idx].double().cpu(), w.double().cpu(), None if b is None else b.double().cpu())
    ref = _act_ref(ref, act)
    if r is not None:
        ref = (ref.to(out_dt).double() if out_dt != torch.float32 else ref) + r[idx].double().cpu()
    return ref


# ---------------------------------------------------------------------------------------------
# 1. a stride changes nothing but addresses
# ---------------------------------------------------------------------------------------------
def _strided_equals_contiguous(dt, M, N, K, act, use_res, *, out_dt=None, use_bias=True, inplace=False, a_pad=24, c_pad=40, want=None, plain=False):
    """setok_linear contiguous and embedded (A in (M + 3, K + a_pad), residual / C in (M + 3, N + c_pad), each operand the column window at OFF): equal bits,
    no store outside C's window, the residual buffer untouched, no NaN from A's padding; and the result within the project's bound of fp64."""
    out_dt = out_dt or dt
    lda, ldc = K + a_pad, N + c_pad
    if want is not None:                                     # both runs in the class the case is about
        for ld in (N, ldc):
            got_cls = _kernel_class(M, N, K, ld, _ncu(), out16=out_dt != torch.float32, plain=plain)
            assert got_cls == want, f"({M}, {N}, {K}) ldc={ld} goes to {got_cls}, not {want}"
    a, w = _randn(M, K, seed=1, dt=dt), _randn(N, K, seed=2, scale=K ** -0.5, dt=dt)
    b = _randn(N, seed=3) if use_bias else None
    r = _randn(M, N, seed=4, dt=out_dt) if use_res else None

    c0 = torch.empty((M, N), dtype=out_dt, device=DEV)
    _raw_linear(a, K, w, c0, N, M, N, K, b, r, act)

    abuf = _embed(a, a_pad, float("nan"))
    if inplace:                                              # C aliases the residual: one strided buffer
        cbuf = _embed(r, c_pad, SENTINEL)
        rbuf = cbuf
    else:
        cbuf = torch.full((M + EXTRA_ROWS, ldc), SENTINEL, dtype=out_dt, device=DEV)
        rbuf = _embed(r, c_pad, float("nan")) if use_res else None
    c_before = cbuf.clone()
    r_before = rbuf.clone() if (use_res and not inplace) else None
    _raw_linear(abuf[:, OFF:], lda, w, cbuf[:, OFF:], ldc, M, N, K, b, None if rbuf is None else rbuf[:, OFF:], act)
    got = _window(cbuf, M, N)
    assert not bool(torch.isnan(got).any()), "A's NaN padding reached C: a K loop or a row ran over"
    assert torch.equal(got, c0), "the strided run differs from the contiguous one"
    _assert_only_the_window_changed(cbuf, c_before, M, N)
    if r_before is not None:
        assert torch.equal(rbuf.view(BITS[out_dt]), r_before.view(BITS[out_dt])), "the residual buffer was written"
    rows = _ref_rows(M)
    _assert_close(got[rows.to(DEV)], _linear_ref(a, w, b, r, act, out_dt, rows), dt, out_dt, f"({M}, {N}, {K}) act {act}")


# fp32 kernel (gemm_f32_kernel): 64 x 64 tiles; lda = K + 24 is a multiple of 4
@pytest.mark.parametrize("M,N,K", [(77, 96, 64), (257, 192, 128)])
@pytest.mark.parametrize("act,use_res", [(0, False), (1, True), (2, True)])
def test_stride_fp32_kernel(M, N, K, act, use_res):
    _strided_equals_contiguous(torch.float32, M, N, K, act, use_res)
    _strided_equals_contiguous(torch.float32, M, N, K, act, True, inplace=True, a_pad=8, c_pad=12)     # ldc needs no alignment in this kernel


# 128 x 128 kernel (gemm_bf16_kernel<16-bit, true>), 16-bit out: N % 64 != 0 keeps the problem off the LDS-DMA kernels at any ldc
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("M,N,K", [(300, 96, 128), (260, 2056, 64)])
@pytest.mark.parametrize("act,use_res", [(0, False), (1, True), (2, True), (2, False)])
def test_stride_tile128_kernel_16_bit_out(dt, M, N, K, act, use_res):
    _strided_equals_contiguous(dt, M, N, K, act, use_res, want="tile128")
    if use_res:
        _strided_equals_contiguous(dt, M, N, K, act, True, inplace=True, c_pad=12, want="tile128")     # (scalar stores: ldc % 8 == 4 is fine here)


# 128 x 128 kernel, 16-bit out, N % 64 == 0: reached only through ldc % 8 != 0 (bf16_kernel), so there is no contiguous run of the same class and output type.
# The contiguous run is forced into the class by out_dtype = float32: without activation its fp32 result, rounded once (and the residual added to the rounded
# value), is what the 16-bit instantiation stores — the same accumulators.  With an activation the two instantiations differ on purpose (fast / exact forms), so
# those cases are held to the fp64 reference with the bounds of the 16-bit output type.
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("act,use_res", [(0, False), (0, True), (1, True), (2, False)])
def test_stride_tile128_kernel_through_an_odd_ldc(dt, act, use_res):
    M, N, K = 257, 192, 128
    lda, ldc = K + 24, N + 40 + 4
    ncu = _ncu()
    assert ldc % 8 == 4 and _kernel_class(M, N, K, ldc, ncu) == "tile128" and _kernel_class(M, N, K, N, ncu, out16=False) == "tile128"
    a, w, b = _randn(M, K, seed=1, dt=dt), _randn(N, K, seed=2, scale=K ** -0.5, dt=dt), _randn(N, seed=3)
    r = _randn(M, N, seed=4, dt=dt) if use_res else None
    abuf = _embed(a, 24, float("nan"))
    cbuf = torch.full((M + EXTRA_ROWS, ldc), SENTINEL, dtype=dt, device=DEV)
    rbuf = _embed(r, 44, float("nan")) if use_res else None
    c_before, r_before = cbuf.clone(), None if rbuf is None else rbuf.clone()
    _raw_linear(abuf[:, OFF:], lda, w, cbuf[:, OFF:], ldc, M, N, K, b, None if rbuf is None else rbuf[:, OFF:], act)
    got = _window(cbuf, M, N)
    assert not bool(torch.isnan(got).any())
    _assert_only_the_window_changed(cbuf, c_before, M, N)
    if use_res:
        assert torch.equal(rbuf.view(torch.int16), r_before.view(torch.int16))
    if act == 0:
        c32 = torch.empty((M, N), dtype=torch.float32, device=DEV)
        _raw_linear(a, K, w, c32, N, M, N, K, b, None, act)
        want = c32.to(dt)
        if use_res:
            want = (want.float() + r.float()).to(dt)
        assert torch.equal(got, want)
    rows = _ref_rows(M)
    _assert_close(got, _linear_ref(a, w, b, r, act, dt, rows), dt, dt, f"tile128 at ldc % 8 == 4, act {act}")


# 128 x 128 kernel, fp32 out (gemm_bf16_kernel<float, false>) with bias + activation + residual
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("act", [0, 1, 2])
def test_stride_tile128_kernel_fp32_out(dt, act):
    _strided_equals_contiguous(dt, 257, 192, 128, act, True, out_dt=torch.float32, want="tile128")
    _strided_equals_contiguous(dt, 257, 192, 128, act, True, out_dt=torch.float32, inplace=True, c_pad=12, want="tile128")


# Small-tile kernel (gemm_tail_kernel), N = 1024: the shapes tail_shape_for picks on 256 CUs.  K = 64, 192, 256 are 1, 3 and 4 K-tiles: the pipeline's
# prologue alone, an odd count (the pair-wise loop's lone last K-tile) and an even one.
SMALL_CASES = [
    # rows on 256 CUs, class, activation, residual
    (1, "small 32x32/8", 0, False),               # 32 x 32, a single row
    (63, "small 32x32/8", 1, True),               # 32 x 32, a ragged second tile row
    (640, "small 64x64/8", 2, True),              # 64 x 64, eight stages
    (640, "small 64x64/8", 1, False),
    (1028, "small 64x64/4", 0, True),             # 64 x 64, four stages: two workgroups per CU
    (1028, "small 64x64/4", 2, False),
    (2056, "small 128x64/6", 1, True),            # 128 x 64 + the 8 rows behind them as 32 x 32 tiles inside the launch (t.A / t.C / t.res = base + M * stride)
    (2056, "small 128x64/6", 0, False),
]


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("K", [64, 192, 256])
@pytest.mark.parametrize("M256,want,act,use_res", SMALL_CASES)
def test_stride_small_tile_kernel(dt, K, M256, want, act, use_res):
    N = 1024
    M = _rows_reaching(want, M256, N, K, _ncu())
    _strided_equals_contiguous(dt, M, N, K, act, use_res, want=want)


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("M256,want", [(63, "small 32x32/8"), (640, "small 64x64/8"), (1028, "small 64x64/4"), (2056, "small 128x64/6")])
def test_stride_small_tile_kernel_in_place(dt, M256, want):
    """C aliases the residual (the in-place residual stream) at a stride."""
    N, K = 1024, 192
    _strided_equals_contiguous(dt, _rows_reaching(want, M256, N, K, _ncu()), N, K, 0, True, inplace=True, want=want)


# Small-tile kernel, more than two rounds of 64 x 64 tiles (1040 tiles on 256 CUs x 2 workgroups)
@pytest.mark.parametrize("dt", LOW16)
def test_stride_small_tile_kernel_many_rounds(dt):
    ncu = _ncu()
    M, N, K = 4112, 1024, 128
    if _cdiv(M, 64) * (N // 64) <= 4 * ncu:                                # another CU count: enough rows for more than two rounds
        M = 64 * (4 * ncu // (N // 64) + 1) + 16
    _strided_equals_contiguous(dt, M, N, K, 1, True, want="small 64x64/8")


# Persistent kernels (K = 192: the three K-tiles the tile-boundary waits need at the least).  90 tiles of 256 x 256 whatever the CU count (PERSIST_MIN_TILES).
PERSIST_CASES = [
    # (M, N), class, activation, residual
    ((2560, 2304), "pp", 0, False),               # ping-pong, 10 x 9 whole tiles: gemm_pp_kernel<act, false, false>
    ((2560, 2304), "pp", 1, True),                #   ... <act, false, true>: the residual rows at wave_elem / lane_off / row8
    ((2560, 2304), "pp", 2, True),
    ((2560, 2304), "pp", 2, False),
    ((2600, 2304), "pp+rem", 0, True),            # ping-pong with the 40 ragged rows merged into the launch (t.A = g.A + M * lda, t.C / t.res = ... + M * ldc)
    ((2600, 2304), "pp+rem", 1, False),
    ((2560, 2240), "persist", 0, False),          # N % 256 != 0: gemm_persist_kernel, ragged last tile column (a_off / b_off clamps, the non-interior epilogue)
    ((2560, 2240), "persist", 1, True),           #   ... with its residual instantiation
    ((2560, 2240), "persist", 2, True),
]


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("MN,want,act,use_res", PERSIST_CASES)
def test_stride_persistent_kernels(dt, MN, want, act, use_res):
    # (persistent non-ping-pong at K < 128: not reachable — bf16_kernel sends K < 192 to the small-tile kernel; see the module's docstring)
    M, N = MN
    _strided_equals_contiguous(dt, M, N, 192, act, use_res, want=want)


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("MN,want", [((2560, 2304), "pp"), ((2600, 2304), "pp+rem"), ((2560, 2240), "persist")])
def test_stride_persistent_kernels_in_place(dt, MN, want):
    M, N = MN
    _strided_equals_contiguous(dt, M, N, 192, 0, True, inplace=True, want=want)


# Persistent kernel with a peeled tail launch of its own: T = ncu + 8 tiles with 8 tile columns leave r = 8 = one tile row, which goes to the small-tile
# kernel as a launch of 256 rows (N = 1984 is not a multiple of 256: no ping-pong, nothing merged).  On 256 CUs: M = 8448 = 33 x 256.
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("act,use_res", [(0, True), (1, False)])
def test_stride_persistent_kernel_with_peeled_tail(dt, act, use_res):
    ncu = _ncu()
    if ncu % 8 != 0:
        pytest.skip(f"{ncu} CUs: no tile count of 8 columns leaves one whole tile row")
    M, N, K = (ncu // 8 + 1) * 256, 1984, 192
    _strided_equals_contiguous(dt, M, N, K, act, use_res, want="persist+tail")


# LayerNorm folded into the GEMM (setok_linear_ln): small-tile (64 x 64, four stages), ping-pong with the remainder merged, and the non-ping-pong persistent kernel
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("M,N,K,want,act", [(1028, 1024, 256, "small 64x64/4", 1), (2600, 2304, 256, "pp+rem", 0), (2600, 2304, 256, "pp+rem", 2),
                                            (2560, 2240, 256, "persist", 1)])
def test_stride_linear_ln(dt, M, N, K, want, act):
    """Strided A and C; the row statistics come from ops.row_stats on a contiguous copy (they are a dense (M, 8) array in the ABI)."""
    a_pad, c_pad = 24, 40
    lda, ldc = K + a_pad, N + c_pad
    assert _kernel_class(M, N, K, ldc, _ncu(), ln=True) == want and _kernel_class(M, N, K, N, _ncu(), ln=True) == want
    x = (_randn(M, K, seed=1) * 1.7 + 0.3).to(dt)
    w, b = _randn(N, K, seed=2, scale=K ** -0.5, dt=dt), _randn(N, seed=3)
    gamma, beta = 1.0 + 0.1 * _randn(K, seed=4), 0.1 * _randn(K, seed=5)
    folded = ops.ln_fold(w, gamma, beta, b)
    stats = ops.row_stats(x, 1e-5)
    c0 = torch.empty((M, N), dtype=dt, device=DEV)
    _raw_linear_ln(x, K, folded, stats, c0, N, M, N, K, act)
    abuf = _embed(x, a_pad, float("nan"))
    cbuf = torch.full((M + EXTRA_ROWS, ldc), SENTINEL, dtype=dt, device=DEV)
    before = cbuf.clone()
    _raw_linear_ln(abuf[:, OFF:], lda, folded, stats, cbuf[:, OFF:], ldc, M, N, K, act)
    got = _window(cbuf, M, N)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, c0)
    _assert_only_the_window_changed(cbuf, before, M, N)
    rows = _ref_rows(M)
    ref = F.linear(F.layer_norm(x[rows.to(DEV)].double().cpu(), (K,), gamma.double().cpu(), beta.double().cpu(), 1e-5), w.double().cpu(), b.double().cpu())
    rel = _rel(got[rows.to(DEV)], _act_ref(ref, act))
    bound = 8e-3 if dt == torch.bfloat16 else 2.5e-3        # test_linear_ln_equals_layernorm_then_linear / test_layernorm_folded_linear_fp16
    print(f"linear_ln ({M}, {N}, {K}) act {act}: rel {rel:.3g} (bound {bound})")
    assert rel < bound


# SwiGLU epilogue of the ping-pong kernel (setok_linear_swiglu): lda, ldo wider than K, F
@pytest.mark.parametrize("dt", LOW16)
def test_stride_linear_swiglu(dt):
    M, Fd, K = 512, 1280, 128
    a_pad, o_pad = 24, 40
    x = _randn(M, K, seed=1, dt=dt)
    wg, wu = _randn(Fd, K, seed=2, scale=K ** -0.5, dt=dt), _randn(Fd, K, seed=3, scale=K ** -0.5, dt=dt)
    wp = ops.interleave_gate_up(wg, wu)
    o0 = torch.empty((M, Fd), dtype=dt, device=DEV)
    _raw_linear_swiglu(x, K, wp, o0, Fd, M, Fd, K)
    abuf = _embed(x, a_pad, float("nan"))
    obuf = torch.full((M + EXTRA_ROWS, Fd + o_pad), SENTINEL, dtype=dt, device=DEV)
    before = obuf.clone()
    _raw_linear_swiglu(abuf[:, OFF:], K + a_pad, wp, obuf[:, OFF:], Fd + o_pad, M, Fd, K)
    got = _window(obuf, M, Fd)
    assert not bool(torch.isnan(got).any())
    assert torch.equal(got, o0)
    _assert_only_the_window_changed(obuf, before, M, Fd)
    assert torch.equal(got, ops.swiglu_pairs(ops.linear(x, wp)))               # the unfused pair (small-tile GEMM): the header promises the same bits
    g, u = (x.double() @ wg.double().t()).to(dt).double().cpu(), (x.double() @ wu.double().t()).to(dt).double().cpu()
    rel = _rel(got, F.silu(g).to(dt).double() * u)
    bound = 1.5e-2 if dt == torch.bfloat16 else 2e-3        # test_gate_up_linear_with_swiglu_in_its_epilogue
    print(f"linear_swiglu: rel {rel:.3g} (bound {bound})")
    assert rel < bound


# ---------------------------------------------------------------------------------------------
# 2. value parity for the classes that had none
# ---------------------------------------------------------------------------------------------
def _batched(vals, rows_pad, cols_pad, gap, fill):
    """(B, M, W) values -> a flat buffer of `fill` in which matrix b is the (M, W) window at row stride W + cols_pad starting at element OFF + b * stride,
    stride = (M + rows_pad) * (W + cols_pad) + gap.  Returns (buffer, ld, stride, the (B, M, W) strided view of the windows)."""
    B, M, W = vals.shape
    ld = W + cols_pad
    stride = (M + rows_pad) * ld + gap
    buf = torch.full((OFF + B * stride,), fill, dtype=vals.dtype, device=vals.device)
    view = buf.as_strided((B, M, W), (stride, ld, 1), OFF)
    view.copy_(vals)
    return buf, ld, stride, view


# Bf16Kernel::PersistF32Batched (gemm_persist_kernel<0, true>): 16-bit in, fp32 out, batch * tiles256 >= 96, no bias / activation / residual
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("M,N,K", [(512, 512, 192), (300, 320, 256)])
def test_persistent_fp32_batched_values_and_strides(dt, M, N, K):
    B = 24
    assert _kernel_class(M, N, K, N, _ncu(), out16=False, batch=B, plain=True) == "f32b"
    a, w = _randn(B, M, K, seed=1, dt=dt), _randn(B, N, K, seed=2, scale=K ** -0.5, dt=dt)
    c0 = torch.empty((B, M, N), dtype=torch.float32, device=DEV)
    _raw_linear(a, K, w, c0, N, M, N, K, batch=B, sA=M * K, sW=N * K, sC=M * N)
    ref = torch.bmm(a.double().cpu(), w.double().cpu().transpose(1, 2))
    for bi in range(B):                                                      # each batch member against fp64 (a wrong batch stride shows as one wrong slice)
        rel = _rel(c0[bi], ref[bi])
        assert rel < 2e-5, (bi, rel)
    # strided batches: padded lda / ldc, batch strides larger than the matrices (multiples of 8 / 4: the class's conditions), sentinels between the matrices
    abuf, lda, sA, _ = _batched(a, EXTRA_ROWS, 24, 8, float("nan"))
    wbuf, _, sW, _ = _batched(w, EXTRA_ROWS, 0, 16, float("nan"))            # (W has no leading dimension in the ABI: dense rows, a gap between the matrices)
    cbuf, ldc, sC, cview = _batched(torch.full((B, M, N), SENTINEL, device=DEV), EXTRA_ROWS, 20, 4, SENTINEL)
    assert lda % 8 == 0 and sA % 8 == 0 and sW % 8 == 0 and ldc % 4 == 0 and sC % 4 == 0
    assert _kernel_class(M, N, K, ldc, _ncu(), out16=False, batch=B, plain=True) == "f32b"
    before = cbuf.clone()
    _raw_linear(abuf[OFF:], lda, wbuf[OFF:], cbuf[OFF:], ldc, M, N, K, batch=B, sA=sA, sW=sW, sC=sC)
    assert not bool(torch.isnan(cview).any())
    assert torch.equal(cview, c0)
    chk = cbuf.clone()
    chk.as_strided((B, M, N), (sC, ldc, 1), OFF).copy_(before.as_strided((B, M, N), (sC, ldc, 1), OFF))
    assert torch.equal(chk.view(torch.int32), before.view(torch.int32)), "a store outside the C windows"


@pytest.mark.parametrize("dt", LOW16)
def test_split_k_weight_gradient_on_the_persistent_kernel(dt):
    """dW = dY^T X through ops.transpose(..., splits=S) + ops.linear_tn with S * tiles256 = 6 * 16 = 96: the batched partial products take the fp32-out persistent
    kernel (test_split_k_weight_gradient's shapes all stay on the 128 x 128 one), at that test's bound."""
    rows, N, K, S = 1500, 1024, 1024, 6
    dy, x = _randn(rows, N, seed=20, dt=dt), _randn(rows, K, seed=21, dt=dt)
    aT, bT = ops.transpose(dy, 64, S), ops.transpose(x, 64, S)
    chunk = aT.shape[2]
    assert aT.shape == (S, N, chunk) and chunk == 256
    assert _kernel_class(N, K, chunk, K, _ncu(), out16=False, batch=S, plain=True) == "f32b"
    got = ops.linear_tn(aT, bT)
    rel = _rel(got, dy.double().cpu().t() @ x.double().cpu())
    assert got.dtype == torch.float32 and rel < 2e-5, rel
    assert torch.equal(got, ops.linear_tn(aT, bT))


# The 128 x 128 kernel, batched, with bias (shared by the batch), activation and residual (at strideC)
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("out32,N", [(False, 96), (True, 192)])          # 16-bit out: N % 64 != 0 keeps the single calls in the class as well
@pytest.mark.parametrize("act", [1, 2])
def test_tile128_batched_with_bias_activation_residual(dt, out32, N, act):
    B, M, K = 3, 257, 128
    out_dt = torch.float32 if out32 else dt
    assert _kernel_class(M, N, K, N, _ncu(), out16=not out32, batch=B) == "tile128" and _kernel_class(M, N, K, N, _ncu(), out16=not out32) == "tile128"
    a, b, r = _randn(B, M, K, seed=1, dt=dt), _randn(N, seed=3), _randn(B, M, N, seed=4, dt=out_dt)
    w = _randn(B, N, K, seed=2, scale=K ** -0.5, dt=dt)
    # strideW = 0: one weight for all members = three single calls of the same class, bit for bit
    shared = torch.empty((B, M, N), dtype=out_dt, device=DEV)
    _raw_linear(a, K, w[0], shared, N, M, N, K, b, r, act, batch=B, sA=M * K, sW=0, sC=M * N)
    for bi in range(B):
        single = torch.empty((M, N), dtype=out_dt, device=DEV)
        _raw_linear(a[bi], K, w[0], single, N, M, N, K, b, r[bi], act)
        assert torch.equal(shared[bi], single), bi
    # a weight per member: each slice against fp64
    got = torch.empty((B, M, N), dtype=out_dt, device=DEV)
    _raw_linear(a, K, w, got, N, M, N, K, b, r, act, batch=B, sA=M * K, sW=N * K, sC=M * N)
    rows = _ref_rows(M)
    for bi in range(B):
        _assert_close(got[bi], _linear_ref(a[bi], w[bi], b, r[bi], act, out_dt, rows), dt, out_dt, f"batch member {bi}")
    # ... and strided: padded lda / ldc, gaps between the members, the residual in a buffer of C's geometry
    abuf, lda, sA, _ = _batched(a, EXTRA_ROWS, 24, 8, float("nan"))
    rbuf, ldc, sC, _ = _batched(r, EXTRA_ROWS, 12, 4, float("nan"))
    cbuf, _, _, cview = _batched(torch.full((B, M, N), SENTINEL, dtype=out_dt, device=DEV), EXTRA_ROWS, 12, 4, SENTINEL)
    before, r_before = cbuf.clone(), rbuf.clone()
    _raw_linear(abuf[OFF:], lda, w, cbuf[OFF:], ldc, M, N, K, b, rbuf[OFF:], act, batch=B, sA=sA, sW=N * K, sC=sC)
    assert torch.equal(cview, got)
    chk = cbuf.clone()
    chk.as_strided((B, M, N), (sC, ldc, 1), OFF).copy_(before.as_strided((B, M, N), (sC, ldc, 1), OFF))
    it = BITS[out_dt]
    assert torch.equal(chk.view(it), before.view(it)) and torch.equal(rbuf.view(it), r_before.view(it))


# fp32 kernel, batched: a k-ordered chain that does not depend on the launch's geometry — slice b of a batch equals the single call on slice b
@pytest.mark.parametrize("M,N,K", [(77, 96, 64), (257, 192, 128)])
def test_fp32_kernel_batch_slices_equal_single_calls(M, N, K):
    B = 3
    a, w = _randn(B, M, K, seed=1), _randn(B, N, K, seed=2, scale=K ** -0.5)
    b, r = _randn(N, seed=3), _randn(B, M, N, seed=4)
    got = torch.empty((B, M, N), device=DEV)
    _raw_linear(a, K, w, got, N, M, N, K, b, r, 2, batch=B, sA=M * K, sW=N * K, sC=M * N)
    rows = _ref_rows(M)
    for bi in range(B):
        single = torch.empty((M, N), device=DEV)
        _raw_linear(a[bi], K, w[bi], single, N, M, N, K, b, r[bi], 2)
        assert torch.equal(got[bi], single), bi
        _assert_close(got[bi], _linear_ref(a[bi], w[bi], b, r[bi], 2, torch.float32, rows), torch.float32, torch.float32, f"fp32 batch member {bi}")
