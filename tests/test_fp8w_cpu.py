"""fp8 weight-only storage without a device: setok_linear_fp8w refuses what it cannot compute on the host, before any launch, with the
argument named (the style of test_abi_cpu.py), and the oracle's W' = value(q) * 2^e is exactly representable in every element type."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fp8_cases as F  # noqa: E402

P = 4096        # stands in for a device pointer: the calls below are refused before anything is launched or dereferenced


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def _args(dtype, M=4, N=64, K=64, lda=64, ldq=64, ldc=64):
    # setok_linear_fp8w(stream, dtype, A, lda, q, ldq, e, residual, C, ldc, M, N, K)
    return (None, dtype, P, lda, P, ldq, P, None, P, ldc, M, N, K)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kw,fp32,names", [
    (dict(M=65), False, b"M=65"),
    (dict(M=65), True, b"M=65"),
    (dict(M=0), False, b"M=0"),
    (dict(K=24, lda=24, ldq=32), True, b"K=24"),                      # fp32: K % 16
    (dict(K=80, lda=80, ldq=80), False, b"K=80"),                     # 16-bit: K % 64
    (dict(lda=56), False, b"lda=56 < K=64"),
    (dict(lda=48), True, b"lda=48 < K=64"),
    (dict(ldq=48), False, b"ldq=48 < K=64"),
    (dict(ldq=48), True, b"ldq=48 < K=64"),
    (dict(ldc=56), False, b"ldc=56 < N=64"),
    (dict(lda=68), False, b"lda=68 must be a multiple of 8"),         # A's rows are read in 16-byte pieces
    (dict(lda=66), True, b"lda=66 must be a multiple of 4"),
    (dict(ldq=72), False, b"ldq=72 must be a multiple of 16"),        # ... and so are q's
    (dict(N=0), False, b"N=0"),
])
def test_linear_fp8w_refuses_on_the_host_with_the_argument_named(lib, half, kw, fp32, names):
    l = lib.load(half)
    dt = 0 if fp32 else (2 if half else 1)
    assert l.setok_linear_fp8w(*_args(dt, **kw)) == -1
    assert names in l.setok_last_error(), l.setok_last_error()


@pytest.mark.parametrize("half", [False, True])
def test_linear_fp8w_wgs_refuses_what_linear_fp8w_refuses_and_a_floor_below_one(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1
    for min_wgs in (0, -256):
        assert l.setok_linear_fp8w_wgs(*_args(dt), min_wgs) == -1
        assert b"min_wgs=%d" % min_wgs in l.setok_last_error(), l.setok_last_error()
    assert l.setok_linear_fp8w_wgs(*_args(dt, M=65), 1) == -1 and b"M=65" in l.setok_last_error()
    assert l.setok_linear_fp8w_wgs(*_args(dt, ldq=48), 256) == -1 and b"ldq=48 < K=64" in l.setok_last_error()


def test_fp8_entry_points_refuse_nulls_and_the_other_builds_16_bit_type(lib):
    for half, bad in ((False, 2), (True, 1)):
        l = lib.load(half)
        assert l.setok_linear_fp8w(*_args(bad)) == -1 and b"dtype" in l.setok_last_error()
        assert l.setok_quantize_fp8_rows(None, bad, P, 64, P, 64, P, 4, 64) == -1 and b"dtype" in l.setok_last_error()
        assert l.setok_dequantize_fp8_rows(None, bad, P, 64, P, P, 64, 4, 64) == -1 and b"dtype" in l.setok_last_error()
        assert l.setok_linear_fp8w(None, 0, None, 64, P, 64, P, None, P, 64, 4, 64, 64) == -1 and b"null operand" in l.setok_last_error()
        assert l.setok_quantize_fp8_rows(None, 0, P, 48, P, 64, P, 4, 64) == -1 and b"ldw=48 < K=64" in l.setok_last_error()
        assert l.setok_quantize_fp8_rows(None, 0, P, 64, P, 48, P, 4, 64) == -1 and b"ldq=48 < K=64" in l.setok_last_error()
        assert l.setok_dequantize_fp8_rows(None, 0, P, 48, P, P, 64, 4, 64) == -1 and b"ldq=48 < K=64" in l.setok_last_error()
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additions: the ABI version stays


def test_the_oracles_dequantised_weights_are_exact_in_every_element_type():
    """One row per exponent of the clamp range [-15, 7] (amax = 0.9 * 448 * 2^e) plus rows beyond both ends: every W' = value(q) * 2^e — the
    smallest, 2^-9 * 2^-15, and the largest, 448 * 2^7, included — survives bf16, fp16 and fp32 unchanged."""
    g = torch.Generator().manual_seed(0)
    K = 512
    rows = []
    for ex in range(F.E_MIN - 3, F.E_MAX + 3):
        r = torch.randn(K, generator=g).double()
        r = r / r.abs().max() * 0.9 * 448.0 * 2.0 ** ex
        r[:16] = torch.ldexp(torch.arange(16).double(), torch.tensor(ex - 9))          # the fp8 subnormals and first normals of this exponent
        rows.append(r)
    W = torch.stack(rows).float()
    q, e = F.quantize_rows(W)
    assert e.tolist() == [max(F.E_MIN, min(F.E_MAX, ex)) for ex in range(F.E_MIN - 3, F.E_MAX + 3)]
    Wp = F.dequantize_rows(q, e)
    assert float(Wp.abs().max()) == 448.0 * 2.0 ** 7 and float(Wp[Wp != 0].abs().min()) == 2.0 ** -24
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        assert torch.equal(Wp.to(dt).double(), Wp), dt
    rel = ((Wp - W.double()).abs() / W.double().abs().clamp_min(1e-300))[3:-3, 16:]     # inside the clamp range: half an e4m3 ulp of a normal value, 2^-4
    big = (W.double().abs() >= torch.ldexp(torch.tensor(1.0).double(), e[:, None].to(torch.int32) - 6))[3:-3, 16:]
    assert float(rel[big].max()) <= 2.0 ** -4


def test_the_oracle_quantiser_on_its_named_cases():
    """The cases the GPU test holds the kernel to, checked against arithmetic done by hand."""
    W = torch.zeros(6, 16)
    W[1, 0] = 448.0 * 2.0 ** -6                      # amax exactly on a boundary: e = -6, code of 448
    W[2, 0] = 448.0 * 2.0 ** -6 * (1 + 2.0 ** -23)   # one fp32 ulp above: e = -5
    W[3, :5] = torch.tensor([448.0, 17.0, 19.0, 21.0, 23.0])
    W[4, :3] = torch.tensor([1e5, -1e5, 57344.0])
    W[5, :4] = torch.tensor([1.0, float("nan"), float("inf"), -float("inf")])
    q, e = F.quantize_rows(W)
    assert e.tolist() == [0, -6, -5, 0, 7, -8]
    assert q[0].tolist() == [0] * 16 and int(q[1, 0]) == 0x7E and int(q[2, 0]) == 0x76
    assert F.dequantize_rows(q, e)[3, :5].tolist() == [448.0, 16.0, 20.0, 20.0, 24.0]
    assert q[4, :3].tolist() == [0x7E, 0xFE, 0x7E]
    assert q[5, :4].tolist() == [0x78, 0x7F, 0x7F, 0x7F]
