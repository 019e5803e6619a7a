"""CPU oracle of the fp8 weight-only storage contract (include/setok_hip.h, "FP8 weight-only decode") and the seeded inputs of its tests.
Pure torch on the CPU; never the code under test.

A matrix W (N, K) is stored as q (N, K) e4m3fn bytes + one int8 exponent per row and means exactly W'[n, k] = value(q[n, k]) * 2^e[n]."""
import torch

E_MIN, E_MAX, FP8_MAX, NAN_CODE = -15, 7, 448.0, 0x7F


def quantize_rows(W):
    """(q uint8 (N, K), e int8 (N,)) of a CPU matrix in fp32 / bf16 / fp16, by the rule of the header:
    amax over the finite entries; e = the smallest integer with amax <= 448 * 2^e, clamped to [-15, 7], 0 for a row of zeros — by frexp
    (amax = m * 2^x, m in [0.5, 1), 448 = 0.875 * 2^9), no log2; q = RNE_e4m3fn(W * 2^-e) saturating at +-448 — torch's CPU cast is
    round-to-nearest-even including the subnormals and gives NaN above 448, hence the clamp in front of it; non-finite -> the NaN code."""
    w = W.detach().cpu().double()                              # exact for all three types, and so is every power-of-two scaling below
    finite = torch.isfinite(w)
    amax = torch.where(finite, w.abs(), torch.zeros_like(w)).amax(dim=1)
    m, x = torch.frexp(amax)
    e = (x - 9 + (m > 0.875).to(x.dtype)).clamp(E_MIN, E_MAX)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).to(torch.int8)
    v = torch.ldexp(torch.where(finite, w, torch.zeros_like(w)), -e.to(torch.int32)[:, None]).clamp(-FP8_MAX, FP8_MAX)
    q = v.float().to(torch.float8_e4m3fn).view(torch.uint8)
    return torch.where(finite, q, torch.full_like(q, NAN_CODE)), e


def dequantize_rows(q, e):
    """W' in fp64: value(q) * 2^e."""
    return torch.ldexp(q.cpu().view(torch.float8_e4m3fn).double(), e.cpu().to(torch.int32)[:, None])


def special_rows(K, dtype, seed):
    """(rows, K) in `dtype`: the rows the quantiser can get wrong.  0 all zeros; 1 amax 1e-8 (the clamp at -15; fp8-subnormal and zero results);
    2 amax 1e5 (the clamp at 7, saturating; fp16 holds 6e4 at most, so there the row peaks at 60000: still above 448 * 2^7 = 57344); 3 amax exactly 448 * 2^-6
    (e = -6, not -5); 4 one ulp of the type above that (e = -5); 5 rounding ties of the e4m3 grid at e = 0 (17, 19, 21, 23, 1.5 * 2^-10, ...)
    under an amax of 448; 6 fp8-subnormal results next to an amax of 300; 7 negative zero, negative ties and a lone large negative entry;
    8 amax 1e-6, the clamp at -15 once more: fp16 cannot hold 1e-8 (row 1 is a second row of zeros there) but holds this one in its subnormals."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda s: torch.randn(K, generator=g) * s
    rows = [torch.zeros(K), rnd(1.0), rnd(1.0), rnd(1.0), rnd(1.0), rnd(100.0), rnd(1e-3), rnd(1.0), rnd(1.0)]
    rows[1] = rows[1] / rows[1].abs().max() * 1e-8
    rows[8] = rows[8] / rows[8].abs().max() * 1e-6
    big = 6e4 if dtype == torch.float16 else 1e5
    rows[2] = rows[2] / rows[2].abs().max() * big
    rows[3] = rows[3] / rows[3].abs().max() * 7.0
    rows[3][K // 2] = 448.0 * 2.0 ** -6                                          # = 7.0 exactly
    rows[4] = rows[3].clone()
    rows[4][K // 2] = float(torch.nextafter(torch.tensor(7.0, dtype=dtype), torch.tensor(8.0, dtype=dtype)))
    ties = torch.tensor([17.0, 19.0, 21.0, 23.0, -17.0, -19.0, 1.5 * 2.0 ** -10, 2.0 ** -10, 3.0 * 2.0 ** -10, 5.0 * 2.0 ** -10, 448.0, 2.0 ** -6 - 2.0 ** -10, 416.0 + 16.0])
    rows[5] = rows[5].clamp(-440.0, 440.0)
    rows[5][:len(ties)] = ties
    rows[6][0] = 300.0
    rows[6][1:9] = torch.tensor([2.0 ** -9, 2.0 ** -8, 3.0 * 2.0 ** -9, 1.1 * 2.0 ** -9, 2.0 ** -10, 0.9 * 2.0 ** -10, 7.5 * 2.0 ** -9, 2.0 ** -6])
    rows[7][:4] = torch.tensor([-0.0, -17.0, -2.0 ** -10 / 448.0, -1000.0])
    return torch.stack(rows).to(dtype)


def quantizer_matrix(N, K, dtype, seed=0):
    """(N, K) in `dtype`: the special rows (as many as fit, cycling) with seeded Gaussian rows of scales 1e-4 .. 1e2 between them."""
    g = torch.Generator().manual_seed(1000 + seed)
    sp = special_rows(K, dtype, seed)
    rows = []
    for n in range(N):
        if n % 2 == 0 or N == 1:
            rows.append(sp[(n // 2 + (2 if N == 1 else 0)) % sp.shape[0]])       # (N = 1: the saturating row)
        else:
            rows.append((torch.randn(K, generator=g) * 10.0 ** float(torch.randint(-4, 3, (1,), generator=g))).to(dtype))
    return torch.stack(rows)


def gemm_problem(M, N, K, dtype, seed):
    """(a (M, K) in `dtype`, q, e, W' in fp64, residual (M, N) in `dtype`): seeded Llama-like weights (std 0.02 with per-row scales over four
    octaves, so the exponents differ between rows) quantised by the oracle, unit-scale activations."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(N, K, generator=g) * 0.02 * (2.0 ** torch.randint(-2, 3, (N, 1), generator=g).float())
    q, e = quantize_rows(W)
    a = torch.randn(M, K, generator=g).to(dtype)
    r = torch.randn(M, N, generator=g).to(dtype)
    return a, q, e, dequantize_rows(q, e), r


def quantized_state_dict(sd, dtype=torch.float32):
    """The state dict (fp32) of the Llama whose stack projections lie on the fp8 grid: every `model.layers.*_proj.weight` replaced by the oracle's W'
    of that weight AS A MODEL IN `dtype` HOLDS IT (a bf16 model quantises its bf16 weights).  W' is exact in fp32 and in `dtype`.  Rows are
    independent, so quantising the parts equals quantising the fused matrices the model packs."""
    out = {}
    for k, v in sd.items():
        if k.startswith("model.layers.") and k.endswith("_proj.weight"):
            q, e = quantize_rows(v.float().to(dtype))
            out[k] = dequantize_rows(q, e).float()
        else:
            out[k] = v.clone()
    return out
