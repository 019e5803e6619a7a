"""MXFP4 weight-only storage without a device: the CPU oracle of tests/mxfp4_cases.py against arithmetic done by hand, and the three entry points
refusing on the host what they cannot compute, before any launch, with the argument named (the style of test_abi_cpu.py)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mxfp4_cases as X  # noqa: E402

P = 4096        # stands in for a device pointer: the calls below are refused before anything is launched or dereferenced


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    from setok_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH) or not os.path.isfile(_lib.LIB_PATH_F16):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------------------
# (input at block exponent e = 0, i.e. next to an amax of 6, nibble) — taken from the contract of include/setok_hip.h, not from the oracle
HAND_TABLE = [
    (0.0, 0x0), (-0.0, 0x8), (0.25, 0x0), (0.26, 0x1), (0.5, 0x1), (0.75, 0x2), (1.0, 0x2), (1.25, 0x2), (1.26, 0x3), (1.5, 0x3), (1.75, 0x4),
    (2.0, 0x4), (2.5, 0x4), (2.51, 0x5), (3.0, 0x5), (3.5, 0x6), (4.0, 0x6), (5.0, 0x6), (5.01, 0x7), (6.0, 0x7),
    (-0.1, 0x8), (-0.25, 0x8), (-0.75, 0xA), (-1.25, 0xA), (-1.75, 0xC), (-2.5, 0xC), (-3.5, 0xE), (-5.0, 0xE), (-6.0, 0xF),
]


def test_the_oracle_on_a_hand_written_table():
    W = torch.zeros(1, 32)
    W[0, :len(HAND_TABLE)] = torch.tensor([v for v, _ in HAND_TABLE])
    q, s = X.quantize_rows(W)
    assert s.tolist() == [[127]]                                   # amax 6: floor(log2 6) - 2 = 0
    assert X.nibbles(q)[0, :len(HAND_TABLE)].tolist() == [c for _, c in HAND_TABLE]
    assert int(q[0, 0]) == 0x80                                    # element 0 (code 0) in the low nibble, element 1 (code 8) in the high one
    for shift in (-13, -3, 5, 13):                                 # the same block at another scale: the same nibbles, the scale byte moves
        q2, s2 = X.quantize_rows(W * 2.0 ** shift)
        assert torch.equal(q2, q) and s2.tolist() == [[127 + shift]]


def test_the_oracle_scale_rule_on_its_named_cases():
    W = torch.zeros(8, 32)
    W[1, 3] = 0.75                                                 # amax exactly 6 * 2^-3: e = -3, the code of 6
    W[2, 3] = float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))      # one ulp below 8 * 2^-3: e = -3, saturates to 6
    W[3, 3] = 1.0                                                  # 8 * 2^-3 itself: e = -2, the code of 4
    W[4, :2] = torch.tensor([1e5, -3e4])                           # floor(log2 1e5) - 2 = 14: clamped to 13; 1e5 / 8192 saturates, 3e4 / 8192 = 3.66 -> 4
    W[5, :3] = torch.tensor([2.0 ** -13, 2.0 ** -14, 2.0 ** -16])  # e = -15: clamped to -13; 1, 0.5, 0.125 -> 1, 0.5, 0
    W[6, :3] = torch.tensor([1.0, float("nan"), -2.0])
    W[7, 5] = -float("inf")
    q, s = X.quantize_rows(W)
    assert s[:, 0].tolist() == [127, 124, 124, 125, 140, 114, 255, 255]
    n = X.nibbles(q)
    assert n[0].tolist() == [0] * 32 and int(n[1, 3]) == 7 and int(n[2, 3]) == 7 and int(n[3, 3]) == 6
    assert n[4, :2].tolist() == [7, 0xE] and n[5, :3].tolist() == [2, 1, 0]
    assert n[6].tolist() == [0] * 32 and n[7].tolist() == [0] * 32
    Wp = X.dequantize_rows(q, s)
    assert Wp[4, :2].tolist() == [6.0 * 8192, -4.0 * 8192] and Wp[5, :3].tolist() == [2.0 ** -13, 2.0 ** -14, 0.0]
    assert bool(torch.isnan(Wp[6:]).all()) and bool(torch.isfinite(Wp[:6]).all())


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16, torch.float16])
def test_the_oracle_is_idempotent_and_its_weights_are_exact_in_every_element_type(dt):
    """quantise ∘ dequantise ∘ quantise = quantise, and W' — 0.5 * 2^-13 and 6 * 2^13 included — survives bf16, fp16 and fp32 unchanged."""
    W = X.quantizer_matrix(100, 160, dt, seed=5)
    q, s = X.quantize_rows(W)
    assert {114, 140, 127, 124} <= set(s.flatten().tolist())       # both clamps, zeros / ties, the boundary blocks
    Wp = X.dequantize_rows(q, s)
    assert float(Wp.abs().max()) == 6.0 * 2.0 ** 13 and float(Wp[Wp != 0].abs().min()) == 0.5 * 2.0 ** -13
    for t in (torch.bfloat16, torch.float16, torch.float32):
        assert torch.equal(Wp.to(t).double(), Wp), t
    q2, s2 = X.quantize_rows(Wp.to(dt))
    assert torch.equal(q2, q) and torch.equal(s2, s)
    # inside the clamp range nothing is further from its code than half a step of the grid at the block's scale: 1 * 2^e above 4 * 2^e
    e = (s.to(torch.int32) - 127).repeat_interleave(32, dim=1)
    inside = ((e > -13) & (e < 13)).flatten()
    err = ((Wp - W.double()).abs() / torch.ldexp(torch.ones(1).double(), e)).flatten()[inside]
    sat = (W.double().abs() / torch.ldexp(torch.ones(1).double(), e)).flatten()[inside] > 6.0
    assert float(err[~sat].max()) <= 1.0 and float(err[sat].max()) < 2.0


def test_the_oracles_bytes_are_torchs_float4_e2m1fn_x2():
    q, _ = X.quantize_rows(X.quantizer_matrix(4, 64, torch.float32, seed=1))
    if not hasattr(torch, "float4_e2m1fn_x2"):
        return                                                     # (this torch has no such dtype: nothing to compare with)
    v = q.view(torch.float4_e2m1fn_x2)                             # one byte = two elements, the low nibble first: torch's packing
    assert v.shape == q.shape and v.element_size() == 1 and torch.equal(v.view(torch.uint8), q)


# ---- the host-side refusals ----------------------------------------------------------------------------------------------------------------------
def _args(dtype, M=4, N=64, K=128, lda=128, ldq=64, lds=4, ldc=64):
    # setok_linear_mxfp4w(stream, dtype, A, lda, q, ldq, s, lds, residual, C, ldc, M, N, K)
    return (None, dtype, P, lda, P, ldq, P, lds, None, P, ldc, M, N, K)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kw,fp32,names", [
    (dict(M=65), False, b"M=65"),
    (dict(M=65), True, b"M=65"),
    (dict(M=0), False, b"M=0"),
    (dict(K=48, lda=48, ldq=32), True, b"K=48"),                       # fp32: K % 32
    (dict(K=192, lda=192, ldq=96, lds=6), False, b"K=192"),           # 16-bit: K % 128
    (dict(K=0), False, b"K=0"),
    (dict(lda=120), False, b"lda=120 < K=128"),
    (dict(lda=96), True, b"lda=96 < K=128"),
    (dict(ldq=48), False, b"ldq=48 < K/2=64"),
    (dict(ldq=48), True, b"ldq=48 < K/2=64"),
    (dict(lds=3), False, b"lds=3 < K/32=4"),
    (dict(lds=3), True, b"lds=3 < K/32=4"),
    (dict(ldc=56), False, b"ldc=56 < N=64"),
    (dict(lda=132), False, b"lda=132 must be a multiple of 8"),       # A's rows are read in 16-byte pieces
    (dict(lda=130), True, b"lda=130 must be a multiple of 4"),
    (dict(ldq=72), False, b"ldq=72 must be a multiple of 16"),        # ... and so are q's: a lane's 16 bytes are one block
    (dict(N=0), False, b"N=0"),
])
def test_linear_mxfp4w_refuses_on_the_host_with_the_argument_named(lib, half, kw, fp32, names):
    l = lib.load(half)
    dt = 0 if fp32 else (2 if half else 1)
    assert l.setok_linear_mxfp4w(*_args(dt, **kw)) == -1
    assert names in l.setok_last_error(), l.setok_last_error()
    assert l.setok_linear_mxfp4w_wgs(*_args(dt, **kw), 256) == -1 and names in l.setok_last_error()


@pytest.mark.parametrize("half", [False, True])
def test_linear_mxfp4w_refuses_unaligned_pointers_and_a_floor_below_one(lib, half):
    l = lib.load(half)
    dt = 2 if half else 1
    a = list(_args(dt))
    for slot in (2, 4):                                            # A, q
        bad = list(a)
        bad[slot] = P + 8
        assert l.setok_linear_mxfp4w(*bad) == -1 and b"16-byte aligned" in l.setok_last_error()
    for min_wgs in (0, -256):
        assert l.setok_linear_mxfp4w_wgs(*a, min_wgs) == -1
        assert b"min_wgs=%d" % min_wgs in l.setok_last_error(), l.setok_last_error()


def test_mxfp4_entry_points_refuse_nulls_and_the_other_builds_16_bit_type(lib):
    for half, bad in ((False, 2), (True, 1)):
        l = lib.load(half)
        assert l.setok_linear_mxfp4w(*_args(bad)) == -1 and b"dtype" in l.setok_last_error()
        # setok_quantize_mxfp4_rows(stream, dtype, W, ldw, q, ldq, s, lds, N, K) / setok_dequantize_mxfp4_rows(stream, dtype, q, ldq, s, lds, W, ldw, N, K)
        assert l.setok_quantize_mxfp4_rows(None, bad, P, 64, P, 32, P, 2, 4, 64) == -1 and b"dtype" in l.setok_last_error()
        assert l.setok_dequantize_mxfp4_rows(None, bad, P, 32, P, 2, P, 64, 4, 64) == -1 and b"dtype" in l.setok_last_error()
        for slot in (2, 4, 6, 9):                                  # A, q, s, C
            a = list(_args(0))
            a[slot] = None
            assert l.setok_linear_mxfp4w(*a) == -1 and b"null operand" in l.setok_last_error()
        assert l.setok_quantize_mxfp4_rows(None, 0, None, 64, P, 32, P, 2, 4, 64) == -1 and b"null operand" in l.setok_last_error()
        assert l.setok_dequantize_mxfp4_rows(None, 0, P, 32, None, 2, P, 64, 4, 64) == -1 and b"null operand" in l.setok_last_error()
        assert l.setok_quantize_mxfp4_rows(None, 0, P, 64, P, 32, P, 2, 4, 48) == -1 and b"K=48" in l.setok_last_error()
        assert l.setok_quantize_mxfp4_rows(None, 0, P, 48, P, 32, P, 2, 4, 64) == -1 and b"ldw=48 < K=64" in l.setok_last_error()
        assert l.setok_quantize_mxfp4_rows(None, 0, P, 64, P, 24, P, 2, 4, 64) == -1 and b"ldq=24 < K/2=32" in l.setok_last_error()
        assert l.setok_quantize_mxfp4_rows(None, 0, P, 64, P, 32, P, 1, 4, 64) == -1 and b"lds=1 < K/32=2" in l.setok_last_error()
        assert l.setok_dequantize_mxfp4_rows(None, 0, P, 24, P, 2, P, 64, 4, 64) == -1 and b"ldq=24 < K/2=32" in l.setok_last_error()
        assert l.setok_dequantize_mxfp4_rows(None, 0, P, 32, P, 2, P, 48, 4, 64) == -1 and b"ldw=48 < K=64" in l.setok_last_error()
    assert lib.load().setok_abi_version() == 9 and lib.load(half=True).setok_abi_version() == 9      # additions: the ABI version stays


def test_quantize_mxfp4_refuses_a_size_off_the_k_granule_by_the_matrix_name():
    """A 16-bit model whose hidden or intermediate size is not a multiple of 128, an fp32 one off 32: ValueError naming the matrix, before
    anything is quantised or freed (checked on the host: no device needed)."""
    sys.path.insert(0, ROOT)
    from setok_amd.llama import SetokimLlamaPrefill
    kw = dict(hidden_size=64, intermediate_size=176, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=2, vocab_size=50)
    m = SetokimLlamaPrefill(kw)
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.down_proj.*176.*32"):
        m.quantize_mxfp4_()
    m = SetokimLlamaPrefill(dict(kw, intermediate_size=256)).to(torch.bfloat16)
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.q_proj.*64.*128"):
        m.quantize_mxfp4_()
    m = SetokimLlamaPrefill(dict(kw, hidden_size=128, intermediate_size=160)).to(torch.bfloat16)
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.down_proj.*160.*128"):
        m.quantize_mxfp4_()
    assert m.weight_format == "native" and all(p.numel() for p in m.parameters())
