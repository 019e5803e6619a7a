"""Every GEMM entry point under the exact-integer operand programs of tests/gemm_programs.py, bit for bit.  Needs a real MI355X: `pytest -m gpu`.

With small-integer operands every product and every partial sum is exact in fp32, so the result does not depend on the summation order and the
tolerance is ZERO at every element, in every kernel class: `sig`, `onehot`, `cancel` and `round` are held to `torch.equal` with the fp64 reference
rounded as the entry point documents (setok_linear: round_T(round_T(acc + bias) + residual); the weight-streaming GEMMs and the skinny GEMM: one
rounding), `act` to one ulp_T plus the floor of the reference arithmetic's own error (gemm_programs.act_floor), `swiglu` to two ulp_T and to equal
bits where SiLU is exact and with the unfused pair.  Every launch runs twice and must give the same bits.  The reference GEMM is fp64 on the CPU; the
elementwise rounding of the reference runs through torch on the device (the programs are built once per shape and shared by the element types).

Each case names its kernel class and asserts through tests/gemm_dispatch.py that its shape reaches the class on the device it runs on.  K is chosen by
K-tile count: NS - 1, NS, NS + 1, 2 NS + 1 (and 1) K-tiles for a class with NS pipeline stages, 3, 4, 5 and 17 for the persistent classes.

The 16-bit MXFP4 GEMM takes K % 128 == 0 only (include/setok_hip.h): at K = 64, 192 and 1088 the test asserts that it refuses the call before any
launch, runs those K in fp32, and runs the 16-bit types at 128, 256 and 1152 (1, 2 and 9 steps)."""
import functools
import os
import re

import pytest
import torch

import gemm_programs as P
from gemm_dispatch import CSRC, _cdiv, _kernel_class, _ncu, _rows_reaching, source_constant

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import _lib, ops

DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LOW16 = [BF16, F16]
ALL3 = [BF16, F16, F32]
TK, BK, FK = source_constant("gemm_persist.hip", "TK"), source_constant("gemm.hip", "BK"), source_constant("gemm.hip", "FK")
_LOG = os.environ.get("SETOK_PARITY_LOG")


def _log(text):
    if _LOG:
        with open(_LOG, "a") as f:
            f.write(os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0] + "\t" + text + "\n")


class _Worst:
    """What a test logs at its end: launches, elements compared, mismatches (integer programs), the largest excess over the bound (act, swiglu)."""

    def __init__(self):
        self.launches = self.elements = self.mismatches = 0
        self.excess = self.ratio = None

    def log(self):
        tail = "" if self.excess is None else f"\tworst (err - bound) {self.excess:.3e}\tworst err / bound {self.ratio:.3f}"
        _log(f"launches {self.launches}\telements {self.elements}\tmismatches {self.mismatches}{tail}")


# ---------------------------------------------------------------------------------------------
# operands, launches, verdicts
# ---------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(t, dt):
    """An fp64 operand of a program in the element type, on the device; nothing is lost."""
    if t is None:
        return None
    P.assert_representable(t, dt)
    return t.to(torch.float32).to(dt).to(DEV)


def _on_dev(p):
    return p._replace(a=None, w=None, acc=p.acc.to(DEV), bias=None if p.bias is None else p.bias.to(DEV), res=None if p.res is None else p.res.to(DEV))


def _raw_linear(a, lda, w, c, ldc, M, N, K, bias=None, res=None, act=0, batch=1, sA=0, sW=0, sC=0):
    _lib.call("setok_linear", ops._stream(), ops._code(a.dtype), ops._code(c.dtype), _ptr(a), lda, _ptr(w), _ptr(bias), _ptr(res), _ptr(c), ldc,
              M, N, K, act, batch, sA, sW, sC)


def _twice(run, worst):
    """Two runs of a launch: the same bits."""
    first, second = run().clone(), run()
    assert torch.equal(first, second) and not bool(torch.isnan(first).any()), "a second run gives other bits"
    worst.launches += 1
    worst.elements += first.numel()
    return first


def _assert_bits(got, want, what, worst, p=None):
    want = want.to(got.device)
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    worst.mismatches += int(bad.sum())
    worst.log()
    idx = bad.nonzero()[0].tolist()
    where = tuple(idx)
    extra = ""
    if p is not None and "k_of_row" in p.info:
        extra = f", k = {int(p.info['k_of_row'][idx[-2]])}"
    pytest.fail(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {where}{extra}: got {float(got[where])}, want {float(want[where])}; "
                f"rows {sorted(set(bad.nonzero()[:, -2].tolist()))[:8]} columns {sorted(set(bad.nonzero()[:, -1].tolist()))[:8]}")


def _assert_within(got, ref, bound, what, worst):
    err = (got.double() - ref).abs()
    excess, ratio = float((err - bound).max()), float((err / bound.clamp_min(1e-300)).max())
    worst.excess = excess if worst.excess is None else max(worst.excess, excess)
    worst.ratio = ratio if worst.ratio is None else max(worst.ratio, ratio)
    if not excess <= 0.0:
        worst.log()
        bad = ((got.double() - ref).abs() > bound).nonzero()[0].tolist()
        pytest.fail(f"{what}: |got - ref| exceeds the bound by {excess:.3e} (first at {tuple(bad)}: got {float(got[tuple(bad)])}, ref {float(ref[tuple(bad)])})")


@functools.lru_cache(maxsize=12)
def _program(name, M, N, K, tile=64, out_dt=None, use_bias=False, use_res=False, seed=0):
    if name == "sig":
        return P.sig(M, N, K, seed=seed)
    if name == "onehot":
        return P.onehot(M, N, K, w=P.distinct_codes(N, K).roll(seed, 0))
    if name == "cancel":
        return P.cancel(M, N, K, tile=tile, seed=1 + seed)
    if name == "round":
        return P.round_program(M, N, K, out_dt, seed=2 + seed, use_bias=use_bias, use_res=use_res)
    assert name == "act"
    return P.act_program(M, N, K, use_bias=use_bias, use_res=use_res)


INTEGER_PROGRAMS = [("sig", False, False), ("onehot", False, False), ("cancel", False, False),
                    ("round", False, False), ("round", True, False), ("round", False, True), ("round", True, True)]
ACT_PROGRAMS = [(1, True, False), (1, True, True), (2, True, True), (2, False, False)]       # activation, bias, residual


def _linear_case(in_dt, out_dt, M, N, K, tile, want=None, ldc=None, plain=False, acts=True):
    """All programs through setok_linear at one shape: C is the (M, N) window of an (M, ldc) buffer."""
    ldc = ldc or N
    if want is not None:
        got_cls = _kernel_class(M, N, K, ldc, _ncu(), out16=out_dt != F32, plain=plain)
        assert got_cls == want, f"({M}, {N}, {K}) ldc={ldc} goes to {got_cls}, not {want}"
    worst = _Worst()
    cbuf = torch.empty((M, ldc), dtype=out_dt, device=DEV)
    c = cbuf[:, :N]

    def launch(p, act=0):
        a, w = _dev(p.a, in_dt), _dev(p.w, in_dt)
        bias = None if p.bias is None else p.bias.to(torch.float32).to(DEV)
        rbuf = None
        if p.res is not None:
            rbuf = torch.zeros((M, ldc), dtype=out_dt, device=DEV)
            rbuf[:, :N] = _dev(p.res, out_dt)

        def run():
            cbuf.fill_(float("nan"))
            _raw_linear(a, K, w, cbuf, ldc, M, N, K, bias, rbuf, act)
            return c
        return _twice(run, worst)

    for name, use_bias, use_res in INTEGER_PROGRAMS:
        if plain and (name == "round" or use_bias or use_res):
            continue
        p = _program(name, M, N, K, tile, out_dt if name == "round" else None, use_bias, use_res)
        _assert_bits(launch(p), P.expected(_on_dev(p), out_dt), f"{name} bias={use_bias} res={use_res} ({M}, {N}, {K}) {in_dt}->{out_dt}", worst, p)
    if acts and not plain:
        for act, use_bias, use_res in ACT_PROGRAMS:
            p = _program("act", M, N, K, tile, None, use_bias, use_res)
            ref, bound = P.act_bound(_on_dev(p), act, out_dt)
            _assert_within(launch(p, act), ref, bound, f"act {act} bias={use_bias} res={use_res} ({M}, {N}, {K}) {in_dt}->{out_dt}", worst)
    worst.log()


# ---------------------------------------------------------------------------------------------
# setok_linear, class by class
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", P.F32_K_TILES)
@pytest.mark.parametrize("M,N", P.F32_SHAPES)
def test_fp32_kernel(M, N, kt):
    _linear_case(F32, F32, M, N, kt * FK, FK)


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("kt", P.TILE128_K_TILES)
@pytest.mark.parametrize("M,N", P.TILE128_SHAPES)
@pytest.mark.parametrize("out32", [False, True])
def test_tile128_kernel(dt, M, N, kt, out32):
    """16-bit out: N % 64 != 0 keeps (300, 96) in the class; (257, 192) gets there through ldc % 8 == 4.  fp32 out: every shape."""
    ldc = N if (out32 or N % 64 != 0) else N + 4
    _linear_case(dt, F32 if out32 else dt, M, N, kt * BK, BK, want="tile128", ldc=ldc)


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("kt", P.TILE128_K_TILES)
@pytest.mark.parametrize("M,N", P.TILE128_SHAPES)
@pytest.mark.parametrize("out32", [False, True])
def test_tile128_kernel_batch_of_three_with_a_weight_per_member(dt, M, N, kt, out32):
    B, K, out_dt = 3, kt * BK, F32 if out32 else dt
    assert _kernel_class(M, N, K, N, _ncu(), out16=not out32, batch=B) == "tile128"
    worst = _Worst()
    for name, use_bias, use_res in INTEGER_PROGRAMS:
        ps = [_program(name, M, N, K, BK, out_dt if name == "round" else None, use_bias, use_res, seed=b) for b in range(B)]
        a, w = torch.stack([_dev(p.a, dt) for p in ps]), torch.stack([_dev(p.w, dt) for p in ps])
        bias = None if ps[0].bias is None else ps[0].bias.to(torch.float32).to(DEV)          # shared by the members
        res = None if ps[0].res is None else torch.stack([_dev(p.res, out_dt) for p in ps])
        c = torch.empty((B, M, N), dtype=out_dt, device=DEV)

        def run():
            c.fill_(float("nan"))
            _raw_linear(a, K, w, c, N, M, N, K, bias, res, 0, batch=B, sA=M * K, sW=N * K, sC=M * N)
            return c
        got = _twice(run, worst)
        for b, p in enumerate(ps):
            _assert_bits(got[b], P.expected(_on_dev(p), out_dt), f"{name} bias={use_bias} res={use_res} member {b} ({M}, {N}, {K}) {dt}->{out_dt}", worst, p)
    worst.log()


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("M256,want,kt", [(M, cls, kt) for M, cls in P.SMALL_ROWS for kt in P.STAGE_K_TILES[int(cls.rsplit("/", 1)[1])]])
def test_small_tile_kernels(dt, M256, want, kt):
    N, K = P.SMALL_N, kt * TK
    _linear_case(dt, dt, _rows_reaching(want, M256, N, K, _ncu()), N, K, TK, want=want)


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("kt", P.PERSIST_K_TILES)
@pytest.mark.parametrize("MN,want", P.PERSIST_SHAPES)
def test_persistent_kernels(dt, MN, want, kt):
    _linear_case(dt, dt, MN[0], MN[1], kt * TK, TK, want=want)


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("kt", P.PERSIST_K_TILES)
def test_persistent_kernel_with_peeled_tail(dt, kt):
    ncu = _ncu()
    if ncu % 8 != 0:
        pytest.skip(f"{ncu} CUs: no tile count of 8 columns leaves one whole tile row")
    _linear_case(dt, dt, (ncu // 8 + 1) * 256, P.PEELED_N, kt * TK, TK, want="persist+tail")


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("N,want", P.LOOP_SHAPES)
def test_persistent_loop_over_three_tiles_per_workgroup(dt, N, want):
    """3 * ncu tiles of 256 x 256: every workgroup runs three tiles, so an accumulator, a bias row or a residual row carried from a workgroup's previous tile
    into the next one shows at every element of the later tiles."""
    ncu = _ncu()
    M, K = P.loop_rows(ncu, N), 3 * TK
    assert _cdiv(M, 256) * _cdiv(N, 256) >= 3 * ncu and _kernel_class(M, N, K, N, ncu) == want
    worst = _Worst()
    c = torch.empty((M, N), dtype=dt, device=DEV)
    for name, use_bias, use_res in [("sig", False, False), ("onehot", False, False), ("round", True, True)]:
        p = _program(name, M, N, K, TK, dt if name == "round" else None, use_bias, use_res)
        a, w = _dev(p.a, dt), _dev(p.w, dt)
        bias, res = (None if p.bias is None else p.bias.to(torch.float32).to(DEV)), _dev(p.res, dt)

        def run():
            c.fill_(float("nan"))
            _raw_linear(a, K, w, c, N, M, N, K, bias, res, 0)
            return c
        _assert_bits(_twice(run, worst), P.expected(_on_dev(p), dt), f"{name} ({M}, {N}, {K}) {dt}", worst, p)
    worst.log()


# ---------------------------------------------------------------------------------------------
# the batched fp32-out persistent kernel (behind linear_tn)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("kt", P.PERSIST_K_TILES)
@pytest.mark.parametrize("M,N", P.F32B_SHAPES)
def test_persistent_fp32_batched_kernel(dt, M, N, kt):
    B, K = 24, kt * TK
    assert _kernel_class(M, N, K, N, _ncu(), out16=False, batch=B, plain=True) == "f32b"
    worst = _Worst()
    for name in ("sig", "onehot", "cancel"):
        ps = [_program(name, M, N, K, TK, seed=b) for b in range(B)]
        a, w = torch.stack([_dev(p.a, dt) for p in ps]), torch.stack([_dev(p.w, dt) for p in ps])
        c = torch.empty((B, M, N), dtype=F32, device=DEV)

        def run():
            c.fill_(float("nan"))
            _raw_linear(a, K, w, c, N, M, N, K, batch=B, sA=M * K, sW=N * K, sC=M * N)
            return c
        got = _twice(run, worst)
        want = torch.stack([P.expected(p, F32) for p in ps])
        _assert_bits(got, want, f"{name} batch of {B} ({M}, {N}, {K}) {dt}", worst)
    worst.log()


@pytest.mark.parametrize("dt", LOW16)
def test_split_k_weight_gradient(dt):
    """dW = dY^T X through ops.transpose(..., splits=6) + ops.linear_tn on integer dY and X: every split's partial and their sum are exact."""
    rows, N, K, S = 1500, 1024, 1024, 6
    g = torch.Generator().manual_seed(5)
    dy, x = torch.randint(-7, 8, (rows, N), generator=g).double(), torch.randint(-7, 8, (rows, K), generator=g).double()
    P.assert_exact(dy.t().contiguous(), x.t().contiguous(), what="dW")
    aT, bT = ops.transpose(_dev(dy, dt), 64, S), ops.transpose(_dev(x, dt), 64, S)
    assert _kernel_class(N, K, aT.shape[2], K, _ncu(), out16=False, batch=S, plain=True) == "f32b"
    worst = _Worst()
    got = _twice(lambda: ops.linear_tn(aT, bT), worst)
    _assert_bits(got, (dy.t() @ x).to(F32), f"dW {dt}", worst)
    worst.log()


# ---------------------------------------------------------------------------------------------
# setok_linear_swiglu
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("kt", P.SWIGLU_K_TILES)
def test_linear_swiglu(dt, kt):
    (M, Fd), K = P.SWIGLU_SHAPE, kt * TK
    s = P.swiglu_program(M, Fd, K)
    a, wp = _dev(s.a, dt), ops.interleave_gate_up(_dev(s.w_gate, dt), _dev(s.w_up, dt))
    out = torch.empty((M, Fd), dtype=dt, device=DEV)
    worst = _Worst()

    def run():
        out.fill_(float("nan"))
        _lib.call("setok_linear_swiglu", ops._stream(), ops._code(dt), _ptr(a), K, _ptr(wp), _ptr(out), Fd, M, Fd, K)
        return out
    got = _twice(run, worst)
    pairs = ops.linear(a, wp)                                               # the unfused pair: the accumulators themselves, then the same bits
    want_pairs = torch.stack([P.round_to(s.gate, dt), P.round_to(s.up, dt)], dim=2).reshape(M, 2 * Fd).to(dt)
    _assert_bits(pairs, want_pairs, f"gate|up accumulators ({M}, {2 * Fd}, {K}) {dt}", worst)
    _assert_bits(got, ops.swiglu_pairs(pairs), f"fused against linear + swiglu_pairs, K={K} {dt}", worst)
    want, exact = P.swiglu_expected(s.gate, s.up, dt)
    want, exact = want.to(DEV), exact.to(DEV)
    assert int(exact.sum()) > 0 and int((~exact).sum()) > 0
    _assert_bits(torch.where(exact, got, want), want, f"swiglu where SiLU is exact, K={K} {dt}", worst)
    _assert_within(got, want.double(), 2 * P.ULP[dt] * want.double().abs(), f"swiglu, K={K} {dt}", worst)
    worst.log()


# ---------------------------------------------------------------------------------------------
# setok_linear_skinny
# ---------------------------------------------------------------------------------------------
def _skinny_max_n():
    """SETOK_SKINNY_MAX_N: the header's value, which ops.SKINNY_MAX_N restates and the library enforces (the next multiple of 16 is refused before any launch)."""
    with open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "setok_hip.h")) as f:
        n = int(re.search(r"#define SETOK_SKINNY_MAX_N (\d+)", f.read()).group(1))
    assert n == ops.SKINNY_MAX_N
    return n


def test_skinny_widest_output_is_the_library_s():
    n = _skinny_max_n()
    a, w = torch.ones((1, 64), dtype=BF16, device=DEV), torch.ones((n + 16, 64), dtype=BF16, device=DEV)
    assert torch.equal(ops.linear_skinny(a, w[:n]), torch.full((1, n), 64.0, dtype=BF16, device=DEV))
    with pytest.raises(_lib.SetokHipError, match="must be a multiple of 16 in"):
        ops.linear_skinny(a, w)


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("ki", range(4))
@pytest.mark.parametrize("M", P.SKINNY_M)
@pytest.mark.parametrize("N", P.SKINNY_N)
def test_linear_skinny(dt, N, M, ki):
    N = N or _skinny_max_n()
    kslice = ops.skinny_kslice(dt == F16)
    K = P.skinny_ks(kslice)[ki]
    assert ops.linear_skinny_workspace(M, N, K, dt == F16) == _cdiv(K, kslice) * M * N
    worst = _Worst()
    for name in ("sig", "onehot", "cancel", "round"):
        for out_dt in ([dt, F32] if dt != F32 else [F32]):
            for alpha in P.SKINNY_ALPHA:
                if name == "sig":
                    p = P.sig(M, N, K, alpha=alpha)
                elif name == "onehot":
                    p = P.onehot(M, N, K)
                elif name == "cancel":
                    p = P.cancel(M, N, K, tile=64, alpha=alpha)
                else:
                    p = P.round_program(M, N, K, out_dt, alpha=alpha)
                a, w = _dev(p.a, dt), _dev(p.w, dt)
                got = _twice(lambda: ops.linear_skinny(a, w, alpha=alpha, out_dtype=out_dt), worst)
                _assert_bits(got, P.expected(p, out_dt, alpha=alpha), f"{name} alpha={alpha} ({M}, {N}, {K}) {dt}->{out_dt}", worst, p)
    worst.log()


# ---------------------------------------------------------------------------------------------
# setok_linear_fp8w, setok_linear_mxfp4w: q built directly, the reference fp64 over the dequantised values, ONE rounding (include/setok_hip.h)
# ---------------------------------------------------------------------------------------------
def _wstream_case(dt, M, N, K, fmt):
    worst = _Worst()
    if fmt == "fp8":
        wp, scale = P.fp8_weights(N, K)
        big_w, encode = 16.0, P.fp8_encode
        linear = lambda a, q, sc, r, mw: ops.linear_fp8w(a, q, sc, residual=r, min_wgs=mw)
    else:
        wp, scale = P.mx_weights(N, K)
        big_w, encode = 4.0, P.mx_encode
        linear = lambda a, q, sc, r, mw: ops.linear_mxfp4w(a, q, sc, residual=r, min_wgs=mw)
    out_dt = dt
    g = torch.Generator().manual_seed(6)
    for name in ("sig", "onehot", "cancel", "round"):
        if name == "sig":
            p = P.sig(M, N, K, w=wp)
        elif name == "onehot":
            p = P.onehot(M, N, K, w=wp)
        elif name == "cancel":
            p = P.cancel(M, N, K, tile=64, w=wp, big_w=big_w)
        else:
            p = P.round_program(M, N, K, out_dt, w=wp)
        q, sc = encode(p.w, scale).to(DEV), scale.to(DEV)
        if fmt == "fp8":
            P.assert_exact(p.a, P.fp8_codes_value(q.cpu()), what=f"fp8 {name}: a times the unscaled codes, what the kernel accumulates")
        a = _dev(p.a, dt)
        for use_res in (False, True):
            res = None
            if use_res:                                              # multiples of 8: acc * 2^e + r stays exact in fp32 for every e >= -3
                res = 8.0 * torch.randint(-3, 4, (M, N), generator=g).double()
            pr = p._replace(res=res)
            want = P.expected(pr, out_dt, rule="fused")
            for min_wgs in (None, 1):
                got = _twice(lambda: linear(a, q, sc, _dev(res, dt), min_wgs), worst)
                _assert_bits(got, want, f"{fmt} {name} res={use_res} min_wgs={min_wgs} ({M}, {N}, {K}) {dt}", worst, p)
    worst.log()


@pytest.mark.parametrize("dt", ALL3)
@pytest.mark.parametrize("K", P.WSTREAM_K)
@pytest.mark.parametrize("N", P.WSTREAM_N)
@pytest.mark.parametrize("M", P.WSTREAM_M)
def test_linear_fp8w(dt, M, N, K):
    _wstream_case(dt, M, N, K, "fp8")


@pytest.mark.parametrize("K", P.WSTREAM_K)
@pytest.mark.parametrize("N", P.WSTREAM_N)
@pytest.mark.parametrize("M", P.WSTREAM_M)
def test_linear_mxfp4w_fp32(M, N, K):
    _wstream_case(F32, M, N, K, "mxfp4")


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("K", P.MXFP4_K16)
@pytest.mark.parametrize("N", P.WSTREAM_N)
@pytest.mark.parametrize("M", P.WSTREAM_M)
def test_linear_mxfp4w_16_bit(dt, M, N, K):
    _wstream_case(dt, M, N, K, "mxfp4")


@pytest.mark.parametrize("dt", LOW16)
@pytest.mark.parametrize("K", P.WSTREAM_K)
def test_linear_mxfp4w_16_bit_refuses_k_off_its_step(dt, K):
    """K = 64, 192, 1088 are no multiples of the 16-bit kernel's 128-wide step: SETOK_EINVAL naming K, before any launch (test_linear_mxfp4w_fp32 runs them)."""
    wp, s = P.mx_weights(64, K)
    a, out = torch.ones((2, K), dtype=dt, device=DEV), torch.full((2, 64), -7.0, dtype=dt, device=DEV)
    with pytest.raises(_lib.SetokHipError, match="must be a positive multiple of 128"):
        ops.linear_mxfp4w(a, P.mx_encode(wp, s).to(DEV), s.to(DEV), out=out)
    assert bool((out == -7.0).all())
