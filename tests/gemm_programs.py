"""Operand programs for the GEMM entry points: seeded operands of small integers (or of multiples of a power of two) for which every product and
every partial sum is exactly representable in fp32, so that fp32 accumulation gives the same bits in ANY order, fused or not, and the verdict on a
kernel is `torch.equal` at every element.  Pure torch on the CPU; imports nothing of the library.

A program returns a `Program`: the operands as fp64 tensors (the caller converts them to the element type — `representable` says that this loses
nothing), an optional bias and residual, and `acc` = a @ w.T, exact.  `expected` applies the epilogue's rounding points.  Every program asserts its
own precondition (`assert_exact`): with ga, gw the largest powers of two that divide every entry of a and of w,
    max_m  sum_k |a[m, k]| * max_n |w[n, k]|   <   2^24 * ga * gw
which bounds sum_k |a[m, k]| |w[n, k]| of every output from above: sums of integers below 2^24, and below 2^23 where halves occur.

  sig      a and w are seeded random integers in [-7, 7]: any dropped, duplicated or misplaced k, row or column changes the integer result
  onehot   row m of a is 1 at k = (m s) mod K (s coprime to K): C[m, n] = w[n, k(m)], so a wrong element names its k and its tile
  cancel   sig, plus at most 256 positions per row whose products are +-2^14 and cancel in pairs: k with k + K/2, and the two sides of every
           K-tile edge (a split-K slice edge is one).  The worst partial in any order is 2^22; a partial narrowed to 16 bits loses the sig part
  round    two-hot rows (a[m, k1] = 2^h, a[m, k2] = 1) put the accumulators on and beside the ties of the output type — 257, 259, ... for bf16,
           2049, 2051, ... for fp16 — with an integer bias and a residual of +-1 / +-3, for which round-then-add and add-then-round differ
  act      onehot rows over w = j / 8: pre-activations exactly on the grid j / 8, j = -96..96, bias included
  swiglu   two-hot rows: gates on the same grid plus {0, 32, 64, 100, 257} (and the same + 1), ups in {+-1, +-2, 3, 0.5}

Weight-only formats: `fp8_weights` / `mx_weights` build W' on the format's grid (integers of at most four significant bits times 2^e[n], e cycling
through -3..3; e2m1 values times 2^(s - 127) with the scale byte s cycling through 127..130 so that adjacent blocks and adjacent rows never share
one); a program may then overwrite entries of W', and `fp8_encode` / `mx_encode` turn W' into codes, asserting that nothing is lost.

`emulate` sums the K-tiles' exact fp32 partial products in a chosen order and with a chosen slip planted; `epilogue` is the epilogue of gemm.hip
with its slips.  tests/test_gemm_programs_cpu.py shows with them that every order gives the reference's bits and that every slip is caught."""
import math
from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

TWO24 = float(1 << 24)
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10, torch.float32: 0.0}      # the tests' convention: ulp_T(x) = ULP[T] * |x|
ACT_GRID = torch.arange(-96, 97, dtype=torch.float64) / 8
DRIFT = 1.5                                                                          # the project's drift margin on a measured floor


class Program(NamedTuple):
    name: str
    a: torch.Tensor                     # (M, K) fp64
    w: torch.Tensor                     # (N, K) fp64
    bias: Optional[torch.Tensor]        # (N,) fp64, exact in fp32
    res: Optional[torch.Tensor]         # (M, N) fp64, exact in the output type
    acc: torch.Tensor                   # (M, N) fp64 = a @ w.T, exact
    info: dict


# ---------------------------------------------------------------------------------------------
# preconditions
# ---------------------------------------------------------------------------------------------
def grain(t):
    """The largest power of two 2^-j, j = 0..12, that divides every entry of t."""
    for j in range(13):
        g = 2.0 ** -j
        if bool(((t / g) == (t / g).round()).all()):
            return g
    raise AssertionError("entries finer than 2^-12")


def exact_bound(a, w, alpha=1.0):
    """An upper bound of max_{m,n} sum_k |a[m,k]| |w[n,k]| * |alpha| in units of grain(a) * grain(w): what has to stay below 2^24."""
    worst = float((a.abs() @ w.abs().amax(dim=0)).max()) if a.numel() and w.numel() else 0.0
    return worst * abs(alpha) / (grain(a) * grain(w) * min(1.0, grain(torch.tensor([float(alpha)], dtype=torch.float64))))


def assert_exact(a, w, alpha=1.0, what=""):
    b = exact_bound(a, w, alpha)
    assert b < TWO24, f"{what}: sum_k |a||w| can reach {b:.0f} units, not below 2^24"
    return b


def representable(t, dt):
    """Every entry of t survives the round trip through dt."""
    return bool((t.to(torch.float32).double() == t).all()) and bool((t.to(torch.float32).to(dt).double() == t).all())


def assert_representable(t, dt, what=""):
    assert representable(t, dt), f"{what}: an entry does not survive the round trip through {dt}"


def round_to(x, dt):
    """x (fp64, exact in fp32) rounded once to dt, as fp64."""
    x32 = x.to(torch.float32)
    assert bool((x32.double() == x).all()), "a value to be rounded is not exact in fp32: the program's precondition is broken"
    return x32.to(dt).double()


def expected(p, out_dt, rule="round_then_add", alpha=1.0):
    """The output in out_dt.  `round_then_add` is what gemm.hip documents: round_T(round_T(alpha acc + bias) + residual) (one rounding for fp32 out);
    `fused` is the weight-streaming GEMMs' documented single rounding: round_T(acc + residual)."""
    pre = alpha * p.acc if p.bias is None else alpha * p.acc + p.bias
    if p.res is None:
        return round_to(pre, out_dt).to(out_dt)
    if out_dt == torch.float32 or rule == "fused":
        return round_to(pre + p.res, out_dt).to(out_dt)
    assert rule == "round_then_add"
    return round_to(round_to(pre, out_dt) + p.res, out_dt).to(out_dt)


# ---------------------------------------------------------------------------------------------
# the programs
# ---------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, lo, hi, g):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _program(name, a, w, bias=None, res=None, acc=None, alpha=1.0, **info):
    info["bound"] = assert_exact(a, w, alpha, name)
    if acc is None:
        acc = a @ w.t()
    return Program(name, a, w, bias, res, acc, info)


def sig(M, N, K, seed=0, w=None, alpha=1.0):
    g = _gen(seed)
    a = _ints((M, K), -7, 7, g)
    if w is None:
        w = _ints((N, K), -7, 7, g)
    return _program("sig", a, w, alpha=alpha)


def onehot_k(M, K, s=37):
    assert math.gcd(s, K) == 1, (s, K)
    return (torch.arange(M) * s) % K


def distinct_codes(N, K):
    """Integers in [-125, 125] (8 significant bits: exact in bf16), different for neighbouring n and k."""
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    return (((n * 37 + k * 11) % 251) - 125).double()


def onehot(M, N, K, w=None, s=37):
    kk = onehot_k(M, K, s)
    a = torch.zeros(M, K, dtype=torch.float64)
    a[torch.arange(M), kk] = 1.0
    if w is None:
        w = distinct_codes(N, K)
    return _program("onehot", a, w, acc=w[:, kk].t().contiguous(), k_of_row=kk)


def cancel_positions(K, tile):
    """[(k, k')]: the two sides of every K-tile edge, and pairs half of K apart."""
    pairs = [(e - 1, e) for e in range(tile, K, tile)]
    half = K // 2
    n_far = max(1, min(8, half // tile))
    step = tile if half >= tile else 0
    pairs += [(5 + step * i, 5 + step * i + half) for i in range(n_far)]
    flat = [k for p in pairs for k in p]
    assert len(set(flat)) == len(flat) and max(flat) < K and len(flat) <= 256, (K, tile, pairs)
    return pairs


def cancel(M, N, K, tile=64, seed=1, w=None, big_w=128.0, alpha=1.0):
    """`big_w`: the magnitude w takes at the big positions (a takes 2^14 / big_w); a caller with a weight format picks one its grid holds in every row."""
    g = _gen(seed)
    a = _ints((M, K), -7, 7, g)
    w = _ints((N, K), -7, 7, g) if w is None else w.clone()
    big_a = 2.0 ** 14 / big_w
    pairs = cancel_positions(K, tile)
    sa = _ints((M, len(pairs)), 0, 1, g) * 2 - 1
    tw = _ints((N, len(pairs)), 0, 1, g) * 2 - 1
    for i, (k0, k1) in enumerate(pairs):
        a[:, k0], a[:, k1] = sa[:, i] * big_a, -sa[:, i] * big_a
        w[:, k0] = w[:, k1] = tw[:, i] * big_w
    big = torch.zeros(K, dtype=torch.bool)
    big[[k for p in pairs for k in p]] = True
    acc = a[:, ~big] @ w[:, ~big].t()                    # the big terms cancel exactly
    return _program("cancel", a, w, acc=acc, alpha=alpha, pairs=pairs)


def two_hot_k(M, K):
    assert K % 2 == 0
    m, h = torch.arange(M), K // 2
    s = next(c for c in (37, 41, 43, 47) if math.gcd(c, h) == 1)
    return 2 * ((m * s) % h), 2 * ((m * s + 3) % h) + 1


def round_program(M, N, K, out_dt, seed=2, use_bias=False, use_res=False, w=None, alpha=1.0):
    g = _gen(seed)
    hi_a = 1024.0 if out_dt == torch.float16 and w is None else 128.0      # (a caller's weights may be large: 2^7 keeps fp16 finite)
    k1, k2 = two_hot_k(M, K)
    a = torch.zeros(M, K, dtype=torch.float64)
    a[torch.arange(M), k1] = hi_a
    a[torch.arange(M), k2] = 1.0
    own = w is None
    if own:
        w = torch.empty(N, K, dtype=torch.float64)
        w[:, 0::2] = _ints((N, K // 2), 2, 7, g)          # 2^h * (2..7): bf16 256..896, fp16 2048..7168 — spacing 2, then 4
        w[:, 1::2] = _ints((N, K // 2), 0, 15, g)
    bias = ((torch.arange(N) % 5) - 2).double() if use_bias else None
    res = None
    if use_res:
        res = torch.tensor([1.0, -1.0, 3.0, -3.0], dtype=torch.float64)[torch.randint(0, 4, (M, N), generator=g)]
    acc = hi_a * w[:, k1].t() + w[:, k2].t()
    p = _program("round", a, w, bias, res, acc=acc.contiguous(), alpha=alpha)
    if out_dt != torch.float32:                           # what the program exercises, counted on its first 64 rows
        top = slice(0, 64)
        pre = alpha * p.acc[top] if bias is None else alpha * p.acc[top] + bias
        y = round_to(pre, out_dt)
        eps = 2.0 ** -6                                   # (below every program's grain: a tie is where a nudge either way rounds apart)
        p.info["inexact"] = int((y != pre).sum())
        p.info["ties"] = int((round_to(pre - eps, out_dt) != round_to(pre + eps, out_dt)).sum())
        if use_res:
            p.info["rules_differ"] = int((round_to(y + res[top], out_dt) != round_to(pre + res[top], out_dt)).sum())
        if own and pre.numel() >= 1024:
            assert p.info["ties"] > 0 and p.info["inexact"] > p.info["ties"], p.info
            assert not use_res or p.info["rules_differ"] > 0, p.info
    return p


def act_program(M, N, K, use_bias=False, use_res=False):
    kk = onehot_k(M, K)
    a = torch.zeros(M, K, dtype=torch.float64)
    a[torch.arange(M), kk] = 1.0
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    bias = res = None
    if use_bias:
        w = (((n * 29 + k * 53) % 129) - 64).double() / 8
        bias = (((torch.arange(N) * 7) % 65) - 32).double() / 8
    else:
        w = (((n * 29 + k * 53) % 193) - 96).double() / 8
    if use_res:
        r = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=torch.float64)
        res = r[(torch.arange(M)[:, None] + torch.arange(N)[None, :] * 5) % 6]
    p = _program("act", a, w, bias, res, acc=w[:, kk].t().contiguous())
    pre = p.acc if bias is None else p.acc + bias
    assert bool(((pre * 8) == (pre * 8).round()).all()) and float(pre.abs().max()) <= 12.0
    return p


def act64(pre, act):
    """The activation in fp64: 0 none, 1 quick-GELU x sigmoid(1.702 x), 2 erf-GELU."""
    pre = pre.double()
    return [pre, pre * torch.sigmoid(1.702 * pre), F.gelu(pre)][act]


def act_floor(act):
    """DRIFT x the largest absolute error, on the grid j / 8, of torch's own fp32 evaluation of the activation on the CPU against fp64: the error of the
    reference arithmetic, never of a kernel."""
    x = ACT_GRID.float()
    got = [x, x * torch.sigmoid(1.702 * x), F.gelu(x)][act]
    return DRIFT * float((got.double() - act64(ACT_GRID, act)).abs().max())


def act_bound(p, act, out_dt):
    """(reference, bound) of the `act` verdict: |got - ref| <= 1 ulp_T(|act64(pre)|) + floor, and with a residual the half ulp_T(|ref|) of the second
    rounding on top (the output is round_T(round_T(act) + r); its spacing at x is at most ulp_T(x), fp32's 2^-23 |x|)."""
    pre = p.acc if p.bias is None else p.acc + p.bias
    y = act64(pre, act)
    bound = ULP[out_dt] * y.abs() + act_floor(act)
    if p.res is None:
        return y, bound
    ref = y + p.res
    return ref, bound + 0.5 * (ULP[out_dt] if out_dt != torch.float32 else 2.0 ** -23) * ref.abs()


GATE_EXTRA = (0.0, 32.0, 64.0, 100.0, 257.0)
UP_SET = (1.0, -1.0, 2.0, -2.0, 3.0, 0.5)


class SwigluProgram(NamedTuple):
    a: torch.Tensor
    w_gate: torch.Tensor
    w_up: torch.Tensor
    gate: torch.Tensor                  # (M, F) exact accumulators
    up: torch.Tensor


def swiglu_program(M, Fd, K):
    k1, k2 = two_hot_k(M, K)
    a = torch.zeros(M, K, dtype=torch.float64)
    a[torch.arange(M), k1] = 1.0
    a[torch.arange(M), k2] = 1.0
    G = torch.cat([ACT_GRID, torch.tensor([0.0, 32.0, 64.0, 100.0, 256.0], dtype=torch.float64)])     # 257 = 256 + the 1 of an odd position
    U = torch.tensor(UP_SET, dtype=torch.float64)
    f, k = torch.arange(Fd)[:, None], torch.arange(K // 2)[None, :]
    wg, wu = torch.zeros(Fd, K, dtype=torch.float64), torch.zeros(Fd, K, dtype=torch.float64)
    wg[:, 0::2] = G[(f * 31 + k * 17) % len(G)]
    wg[:, 1::2] = ((f + k) % 3 == 0).double()
    wu[:, 0::2] = U[(f * 5 + k * 3) % len(U)]
    assert_exact(a, wg, what="swiglu gate")
    assert_exact(a, wu, what="swiglu up")
    gate = (wg[:, k1] + wg[:, k2]).t().contiguous()
    up = (wu[:, k1] + wu[:, k2]).t().contiguous()
    return SwigluProgram(a, wg, wu, gate, up)


def swiglu_expected(gate, up, dt):
    """HF's rounding points in fp64: gate and up rounded, SiLU rounded, the product rounded.  Returns (expected, exact): `exact` marks the outputs whose
    SiLU is exact in the type (gate 0 or gate >= 32: sigmoid is 1 to fp32's last bit), where equal bits are required."""
    g, u = round_to(gate, dt), round_to(up, dt)
    s = (g * torch.sigmoid(g)).to(torch.float32).to(dt).double()
    out = (s * u).to(torch.float32).to(dt)
    return out, (g == 0) | (g >= 32)


# ---------------------------------------------------------------------------------------------
# weight-only formats
# ---------------------------------------------------------------------------------------------
def _e4m3_magnitudes():
    c = torch.arange(127)
    e, m = (c >> 3).double(), (c & 7).double()
    return torch.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * 2.0 ** (e - 7))          # codes 0..126 ascending; 127 is NaN


def fp8_exponents(N):
    return ((torch.arange(N) % 7) - 3).to(torch.int8)


def fp8_weights(N, K, seed=3):
    """(W', e): W'[n, k] = i * 2^e[n] with i a seeded integer in [-15, 15] (four significant bits) and e cycling through -3..3."""
    e = fp8_exponents(N)
    return _ints((N, K), -15, 15, _gen(seed)) * (2.0 ** e.double())[:, None], e


def fp8_encode(wp, e):
    """(N, K) uint8 e4m3fn codes with value(code) * 2^e[n] == W'[n, k] exactly."""
    v = wp * (2.0 ** -e.double())[:, None]
    mags = _e4m3_magnitudes()
    idx = torch.searchsorted(mags, v.abs().contiguous()).clamp_max(126)
    assert bool((mags[idx] == v.abs()).all()), "a weight is not on the e4m3 grid of its row"
    return (idx | (torch.signbit(v).long() << 7)).to(torch.uint8)


def fp8_codes_value(q):
    mags = torch.cat([_e4m3_magnitudes(), torch.tensor([float("nan")], dtype=torch.float64)])
    return mags[(q & 0x7f).long()] * torch.where((q & 0x80) != 0, -1.0, 1.0).double()


def mx_scales(N, K, shift=0):
    """(N, K / 32) uint8 scale bytes cycling through 127..130: block b of row n has 127 + (n + b + shift) % 4 — adjacent blocks and rows differ."""
    return (127 + (torch.arange(N)[:, None] + torch.arange(K // 32)[None, :] + shift) % 4).to(torch.uint8)


def mx_factor(s):
    return (2.0 ** (s.double() - 127)).repeat_interleave(32, dim=1)


def mx_weights(N, K, seed=4):
    """(W', s): nibbles drawn from the full e2m1 set (the negative zero included) times the block scales of `mx_scales`."""
    s = mx_scales(N, K)
    code = torch.randint(0, 16, (N, K), generator=_gen(seed))
    val = torch.tensor(E2M1, dtype=torch.float64)[code & 7] * torch.where((code & 8) != 0, -1.0, 1.0).double()
    return val * mx_factor(s), s


def mx_encode(wp, s):
    """(N, K / 2) uint8: element 2 j in the low nibble of byte j.  Asserts value_e2m1(nibble) * 2^(s - 127) == W' exactly."""
    v = wp / mx_factor(s)
    grid = torch.tensor(E2M1, dtype=torch.float64)
    idx = torch.searchsorted(grid, v.abs().contiguous()).clamp_max(7)
    assert bool((grid[idx] == v.abs()).all()), "a weight is not on the e2m1 grid of its block"
    code = idx | (torch.signbit(v).long() << 3)
    return (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)


def mx_decode(q, s):
    code = torch.stack([q & 0xf, q >> 4], dim=2).reshape(q.shape[0], -1).long()
    val = torch.tensor(E2M1, dtype=torch.float64)[code & 7] * torch.where((code & 8) != 0, -1.0, 1.0).double()
    return val * mx_factor(s)


# ---------------------------------------------------------------------------------------------
# an fp32 GEMM in a chosen order, with a chosen slip
# ---------------------------------------------------------------------------------------------
ORDERS = ("forward", "backward", "pairwise", "splitk")
SLIPS = ("drop_last_tile", "swap_k", "carry_acc", "bf16_partial", "row_past_end", "skip_slice", "alpha_missing")


def emulate(a, w, tile=64, order="forward", slip=None, kslice=512, alpha=1.0, carry_rows=256, past_row=None):
    """alpha * a @ w.T accumulated in fp32 over K-tiles of `tile` columns in `order`: forward, backward, pairwise (the tiles' partials merged as a
    binary tree) or splitk (slices of `kslice` columns summed forward each, the slices then added in slice order, alpha applied per slice).
    `slip` plants one of SLIPS."""
    a32, w32 = a.to(torch.float32), w.to(torch.float32)
    M, K = a32.shape
    if slip == "swap_k":                                  # two k of the last tile change places on A alone
        k0 = (K - 1) // tile * tile
        a32 = a32.clone()
        a32[:, [k0 + 1, K - 2]] = a32[:, [K - 2, k0 + 1]]
    if slip == "row_past_end":                            # the last row is computed from the row behind A's end
        a32 = a32.clone()
        a32[M - 1] = past_row.to(torch.float32)
    tiles = [(k, min(k + tile, K)) for k in range(0, K, tile)]
    if slip == "drop_last_tile":
        tiles = tiles[:-1]
    part = lambda t: a32[:, t[0]:t[1]] @ w32[:, t[0]:t[1]].t()
    narrow = (lambda x: x.to(torch.bfloat16).float()) if slip == "bf16_partial" else (lambda x: x)
    zero = torch.zeros(M, w32.shape[0], dtype=torch.float32)

    def chain(ts):
        acc = zero.clone()
        for t in ts:
            acc = narrow(acc + part(t))
        return acc

    if order == "forward":
        acc = chain(tiles) * alpha
    elif order == "backward":
        acc = chain(tiles[::-1]) * alpha
    elif order == "pairwise":
        parts = [part(t) for t in tiles] or [zero]
        while len(parts) > 1:
            parts = [narrow(parts[i] + parts[i + 1]) if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        acc = parts[0] * alpha
    else:
        assert order == "splitk" and kslice % tile == 0
        slices = [[t for t in tiles if t[0] // kslice == s] for s in range((K + kslice - 1) // kslice)]
        if slip == "skip_slice":
            slices = slices[:1] + slices[2:]
        acc = zero.clone()
        for i, ts in enumerate(slices):
            acc = narrow(acc + chain(ts) * (1.0 if slip == "alpha_missing" and i == len(slices) - 1 else alpha))
    if slip == "carry_acc":                               # a tile starts from the accumulator of the tile `carry_rows` rows above
        acc = torch.cat([acc[:carry_rows], acc[carry_rows:] + acc[:-carry_rows]])
    return acc


def epilogue(acc32, bias, res, out_dt, act=0, slip=None):
    """gemm.hip's epilogue on an fp32 accumulator: bias, activation (torch's fp32 form), rounding to out_dt, residual, rounding.
    Slips: res_before_round, bias_after_act."""
    v = acc32.clone()
    b32 = None if bias is None else bias.to(torch.float32)
    if b32 is not None and slip != "bias_after_act":
        v = v + b32
    v = [v, v * torch.sigmoid(1.702 * v), F.gelu(v)][act]
    if b32 is not None and slip == "bias_after_act":
        v = v + b32
    if res is None:
        return v.to(out_dt)
    if slip == "res_before_round" or out_dt == torch.float32:
        return (v + res.to(torch.float32)).to(out_dt)
    return (v.to(out_dt).float() + res.to(torch.float32)).to(out_dt)


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_gemm_programs_gpu.py (row counts as the dispatch rules pick the class on 256 CUs; the GPU test re-derives them for its device)
# ---------------------------------------------------------------------------------------------
STAGE_K_TILES = {8: (1, 7, 8, 9, 17), 4: (1, 3, 4, 5, 9), 6: (1, 5, 6, 7, 13)}      # NS - 1, NS, NS + 1, 2 NS + 1, and 1 (reachable: K = 64 stays off the persistent path)
PERSIST_K_TILES = (3, 4, 5, 17)
F32_K_TILES = (1, 3, 4, 5, 9)                                                       # the fp32 kernel folds its chain every 4 K-tiles of FK columns
TILE128_K_TILES = (1, 2, 3, 5)                                                      # two LDS buffers
SMALL_ROWS = [(1, "small 32x32/8"), (63, "small 32x32/8"), (640, "small 64x64/8"), (1028, "small 64x64/4"), (2056, "small 128x64/6")]
SMALL_N = 1024
PERSIST_SHAPES = [((2560, 2304), "pp"), ((2600, 2304), "pp+rem"), ((2560, 2240), "persist")]
PEELED_N = 1984                                                                     # (ncu / 8 + 1) * 256 rows: persist+tail
LOOP_SHAPES = [(2048, "pp"), (1984, "persist")]                                     # N; rows: three 256 x 256 tiles per workgroup
F32_SHAPES = [(77, 96), (257, 192)]
TILE128_SHAPES = [(300, 96), (257, 192)]
F32B_SHAPES = [(512, 512), (300, 320)]
SWIGLU_SHAPE, SWIGLU_K_TILES = (512, 1280), (2, 4, 9)
SKINNY_N, SKINNY_M, SKINNY_ALPHA = (16, 64, None), (1, 63, 1028), (1.0, 2.0, 0.25, -3.0)      # None: SKINNY_MAX_N
WSTREAM_M, WSTREAM_N, WSTREAM_K = (1, 2, 17, 64), (64, 192, 1024), (64, 192, 1088)
MXFP4_K16 = (128, 256, 1152)        # the 16-bit MXFP4 GEMM takes K % 128 == 0 only: 1, 2 and 9 steps stand in for 64, 192 and 1088 there


def skinny_ks(kslice):
    """One, two and three whole slices, and one slice + 64: two slices, the second 64 long."""
    return (kslice, 2 * kslice, 3 * kslice, kslice + 64)


def loop_rows(ncu, N):
    """Rows of 3 * ncu tiles of 256 x 256 (rounded up to whole tile rows): every workgroup of a persistent launch runs at least three."""
    tiles_n = (N + 255) // 256
    return 256 * ((3 * ncu + tiles_n - 1) // tiles_n)
