"""The column bands of setok_linear_fp8w's 16-bit path on a real MI355X.  A workgroup owns NT = 1, 2 or 4 column tiles of 16 columns: the
widest band (4 from three row tiles, 2 at two, 1 at one) that still leaves ceil(N / (16 NT)) >= min_wgs workgroups (include/setok_hip.h,
setok_linear_fp8w_wgs).  With the library's own floor of 256 the wide bands begin at N = 8161 (NT = 2) and N = 16321 (NT = 4): the fused qkv
and gate|up operands of a 7B stack, and nothing in tests/test_fp8w_gpu.py.  Here every (row tiles, NT) variant runs
  - at N = 8200 and N = 16400 through the public rule, against fp64 with `ops.linear` on W' as the yardstick, inside a NaN frame, and bit for
    bit against calls on row slices of q short enough to take NT = 1;
  - at small N with the floor named, bit for bit against NT = 1, where N ends inside every column tile of a band.
The band moves columns between workgroups and must never change a bit.  `pytest -m gpu`."""
import pytest
import torch

import fp8_cases as F
import parity
from test_fp8w_gpu import DEV, NAN, TAG, _frame_untouched, _log, _window

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from setok_amd import ops

HALVES = [torch.bfloat16, torch.float16]
FLOOR = 256                      # setok_linear_fp8w's min_wgs


def _cdiv(a, b):
    return -(-a // b)


def band(M, N, min_wgs=FLOOR):
    """NT by the rule of the header."""
    mt = _cdiv(M, 16)
    nt = 1 if mt == 1 else (2 if mt == 2 else 4)
    while nt > 1 and _cdiv(N, 16 * nt) < min_wgs:
        nt //= 2
    return nt


_PROBLEMS = {}


def _problem(N, K, dt):
    key = (N, K, dt)
    if key not in _PROBLEMS:
        a, q, e, Wp, r = F.gemm_problem(64, N, K, dt, seed=N + K)
        ref = a.double() @ Wp.t()
        _PROBLEMS[key] = dict(a=_window(a, 1, 16, 1, 48, NAN)[1], q=_window(q, 1, 32, 1, 16, F.NAN_CODE)[1], e=e.to(DEV), r=r.to(DEV),
                              w=Wp.to(dt).to(DEV), ref=ref, ref_r=ref + r.double(), a_dense=a.to(DEV))
    return _PROBLEMS[key]


# K = 64 is one k-step (three of the four waves merge zeros); K = 576 is 9 steps: the waves' shares differ, and a loop that takes 8 steps per
# round of the workgroup (NT = 4) runs a second, partly filled round.  The longer loops do that at K = 1088 in the test below.
@pytest.mark.parametrize("dt", HALVES)
@pytest.mark.parametrize("N,K", [(N, K) for N in (8200, 16400) for K in (64, 576)])
def test_the_wide_bands_of_the_public_rule_against_fp64_and_against_the_narrow_band(dt, N, K):
    """N = 8200 = 256 * 32 + 8 takes NT = 2 from two row tiles on, N = 16400 = 256 * 64 + 16 takes NT = 2 at two row tiles and NT = 4 above:
    (row tiles, NT) = (2, 2), (3, 2), (4, 2), (3, 4), (4, 4), each with a last band that N leaves inside.  Per M: max-rel and rms-rel against fp64
    at most 1.5 x `ops.linear`'s on W'; the NaN frame of C untouched; and the columns of the full call `torch.equal` to the same columns
    computed from row slices of q of fewer than 8161 rows, which take NT = 1 — the slice that ends at N included."""
    p = _problem(N, K, dt)
    seen = set()
    for M in (17, 33, 37, 64):
        nt = band(M, N)
        assert nt > 1 and band(M, 8160) == 1
        seen.add((_cdiv(M, 16), nt))
        a, q, e = p["a"][:M], p["q"], p["e"]
        for res in (False, True):
            r = p["r"][:M] if res else None
            ref = (p["ref_r"] if res else p["ref"])[:M]
            obuf, out = _window(p["r"][:M].cpu() if res else torch.zeros(M, N, dtype=dt), 1, 5, 2, 11, NAN)
            ops.linear_fp8w(a, q, e, residual=out if res else None, out=out)                       # (with a residual: aliased, on C's stride)
            yard = ops.linear(p["a_dense"][:M].contiguous(), p["w"], residual=None if r is None else r.contiguous())
            ours, theirs = parity.measure(out, ref), parity.measure(yard, ref)
            _log(f"linear_fp8w {TAG[dt]} M={M} N={N} K={K} NT={nt} {'aliased' if res else 'plain'}: max-rel ours, linear, rms-rel ours, linear",
                 ours[0], theirs[0], ours[1], theirs[1])
            assert bool(torch.isfinite(out).all()) and _frame_untouched(obuf, 1, 5, M, N)
            assert ours[0] <= 1.5 * theirs[0] and ours[1] <= 1.5 * theirs[1], (M, res, ours, theirs)
            for lo in range(0, N, 8112):                                                          # 8112 = 507 * 16 < 8161: band edges stay where they are
                hi = min(N, lo + 8112)
                assert band(M, hi - lo) == 1
                part = ops.linear_fp8w(a, q[lo:hi], e[lo:hi].contiguous(), residual=None if r is None else r[:, lo:hi].contiguous())
                assert torch.equal(part, out[:, lo:hi]), (M, res, lo)
            odd = ops.linear_fp8w(a, q[8:4008], e[8:4008].contiguous(), residual=None if r is None else r[:, 8:4008].contiguous())
            assert torch.equal(odd, out[:, 8:4008]), (M, res)                                     # ... and where they are not: a column's bits are its own
    assert seen == ({(2, 2), (3, 2), (4, 2)} if N == 8200 else {(2, 2), (3, 4), (4, 4)})


# N = 40 and 100 end inside column tile 2 of a 64-column band and inside tile 0 of a 32-column one, N = 88 inside tile 1 of both, and N = 272
# at the end of tile 0 of both: the rest of the last band lies outside q, e and C.  K = 1088 is 17 steps: every variant's loop (8, 16 or 32 steps
# per round of the workgroup) runs a partly filled round, and the 8- and 16-step ones more than one round.
@pytest.mark.parametrize("dt", HALVES)
@pytest.mark.parametrize("N", [40, 88, 100, 272])
def test_every_band_named_by_its_floor_has_the_bits_of_the_narrow_band(dt, N):
    """setok_linear_fp8w_wgs with min_wgs = ceil(N / (16 NT)) takes NT (where the row tiles allow it), and min_wgs = ceil(N / 16) takes NT = 1:
    all nine (row tiles, NT) variants, without and with an aliased residual, inside a NaN frame, `torch.equal` to NT = 1 and to the public call."""
    K = 1088
    p = _problem(N, K, dt)
    seen = set()
    for M in (1, 16, 17, 32, 33, 48, 49, 64):
        a, q, e = p["a"][:M], p["q"], p["e"]
        for res in (False, True):
            r = p["r"][:M] if res else None
            narrow = ops.linear_fp8w(a, q, e, residual=r, min_wgs=_cdiv(N, 16))
            assert band(M, N, _cdiv(N, 16)) == 1 and torch.equal(narrow, ops.linear_fp8w(a, q, e, residual=r))
            assert parity.measure(narrow, (p["ref_r"] if res else p["ref"])[:M])[0] < 1e-2
            for want in (1, 2, 4):
                floor = _cdiv(N, 16 * want)
                nt = band(M, N, floor)
                assert nt == min(want, (1, 1, 2, 4, 4)[_cdiv(M, 16)])
                seen.add((_cdiv(M, 16), nt))
                obuf, out = _window(r.cpu() if res else torch.zeros(M, N, dtype=dt), 2, 3, 1, 10, NAN)
                ops.linear_fp8w(a, q, e, residual=out if res else None, out=out, min_wgs=floor)
                assert _frame_untouched(obuf, 2, 3, M, N) and torch.equal(out, narrow), (M, res, want)
    assert seen == {(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (3, 4), (4, 1), (4, 2), (4, 4)}
